// host_common.h -- what the host layer of every context shares: the error path, the device check of the create
// functions, the one kernel launcher, the staging of a host-pointer call, the state blob of a module and the preamble of destroy.
// Host side only.  Everything is a template on the context type; a context has `std::string err` and `cfg.device`.
#pragma once
#include "../../include/mcarray_hip.h"
#include "stage.h"
#include "state_blob.h"

#include <string>
#include <vector>

namespace mca {

// ---- the error path.  A failing call leaves its text in the context; a failing create (a null context of the module's type) in the
// module's own creation-error string, which mca_hip_*_last_error(NULL) of that module returns
template <class Ctx> std::string &create_error()
{
    static std::string text;
    return text;
}
template <class Ctx> int fail(Ctx *c, int code, const std::string &msg)
{
    (c ? c->err : create_error<Ctx>()) = msg;
    return code;
}
template <class Ctx> const char *last_error(const Ctx *c) { return c ? c->err.c_str() : create_error<Ctx>().c_str(); }
// what a HIP call failed with: out of memory by its own code; `what` names the call or the buffers
template <class Ctx> int hip_fail(Ctx *c, hipError_t e, const char *what)
{
    return fail(c, e == hipErrorOutOfMemory ? MCA_HIP_ERR_OUT_OF_MEMORY : MCA_HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(ctx, expr)                                            \
    do {                                                              \
        const hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) return mca::hip_fail(ctx, _e, #expr);   \
    } while (0)

// a create function's device: one is visible, the ordinal names one, it is the calling thread's from here on.  none: the null context
template <class Ctx> int check_device(Ctx *none, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(none, MCA_HIP_ERR_NO_DEVICE, "no HIP device visible; libmcarray_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(none, MCA_HIP_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(none, MCA_HIP_ERR_HIP, "hipSetDevice failed");
    return MCA_HIP_OK;
}
// a context that failed on its way out of create: its text becomes the module's creation error, the context goes
template <class Ctx, class Free> int create_failed(Ctx *c, int rc, Free &&free_ctx)
{
    create_error<Ctx>() = c->err;
    free_ctx(c);
    return rc;
}
// *_destroy: everything in flight on the context's device has finished before its buffers go
template <class Ctx, class Free> void destroy_ctx(Ctx *c, Free &&free_ctx)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    free_ctx(c);
}

// ---- the one kernel launcher.  The limit of dynamic LDS is a property of the FUNCTION, shared by every context of the process, and 64 KiB is
// what a function may have without asking: the attribute is set at the launch, exactly when the launch asks for more (lds_limit: the one place)
template <class Ctx> int lds_limit(Ctx *c, const void *kernel, size_t lds)
{
    if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MCA_HIP_OK;
}
// the arguments in hipLaunchKernel's order.  A launch that fails is found at the call's hipGetLastError, as after hipLaunchKernelGGL
template <class Ctx> int launch_kernel(Ctx *c, const void *kernel, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t st)
{
    if (const int rc = lds_limit(c, kernel, lds)) return rc;
    (void)hipLaunchKernel(kernel, grid, block, args, lds, st);
    return MCA_HIP_OK;
}
// ... of a kernel by its name, the arguments converted to the kernel's parameter types
template <class T> struct launch_arg { typedef T type; };
template <class Ctx, class... A>
int launch_kernel(Ctx *c, void (*kernel)(A...), dim3 grid, dim3 block, size_t lds, hipStream_t st, typename launch_arg<A>::type... a)
{
    void *args[] = {static_cast<void *>(&a)...};
    return launch_kernel(c, reinterpret_cast<const void *>(kernel), grid, block, args, lds, st);
}

// ---- a host-pointer call on its listed buffers (slot: the layer's own enum over StagePool; the pool's buffers are reused across calls by number)
// STAGE_IN / STAGE_OUT: host NULL is an optional buffer the caller leaves out: nothing staged, the _dev call gets NULL.  STAGE_ALWAYS: an
// output the _dev call gets a device buffer for whatever the caller passed, copied back only to a host pointer.  bytes 0: nothing staged, no error
enum StageDir { STAGE_IN = 1, STAGE_OUT = 2, STAGE_ALWAYS = 4 };
struct StageBuf { int slot; const void *host; size_t bytes; int dir; void *dev; };
// the device copies, the inputs copied in the list's order, the _dev call on the null stream (it reads StageBuf::dev), the wait, the
// outputs copied in the list's order
template <class Ctx, size_t NB, class DevCall>
int staged(Ctx *c, StageBuf (&bufs)[NB], DevCall &&dev_call)
{
    for (StageBuf &b : bufs)
        if ((b.host || (b.dir & STAGE_ALWAYS)) && b.bytes && !(b.dev = c->stage.get(b.slot, b.bytes)))
            return fail(c, MCA_HIP_ERR_OUT_OF_MEMORY, NB == 1 ? "device staging buffer for the host-pointer call" : "device staging buffers for the host-pointer call");
    for (StageBuf &b : bufs)
        if (b.dev && (b.dir & STAGE_IN)) HIP_TRY(c, hipMemcpy(b.dev, b.host, b.bytes, hipMemcpyHostToDevice));
    if (const int rc = dev_call()) return rc;
    HIP_TRY(c, hipDeviceSynchronize());
    for (StageBuf &b : bufs)
        if (b.dev && b.host && (b.dir & STAGE_OUT)) HIP_TRY(c, hipMemcpy(const_cast<void *>(b.host), b.dev, b.bytes, hipMemcpyDeviceToHost));
    return MCA_HIP_OK;
}

// ---- a module's state as one blob (state_blob.h): the parts, the magic, the version and the hash of the configuration
template <class Ctx> int blob_status(Ctx *c, int rc) { return rc ? fail(c, rc == 2 ? MCA_HIP_ERR_HIP : MCA_HIP_ERR_INVALID_ARGUMENT, blob_error(rc)) : MCA_HIP_OK; }
inline long long state_size(const void *c, const std::vector<BlobPart> &parts) { return c ? blob_size(parts) : (long long)MCA_HIP_ERR_INVALID_ARGUMENT; }
template <class Ctx> int state_save(Ctx *c, const std::vector<BlobPart> &parts, const BlobHeader &h, void *blob, long long bytes)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return blob_status(c, blob_save(parts, h, blob, bytes));
}
template <class Ctx> int state_load(Ctx *c, const std::vector<BlobPart> &parts, unsigned magic, int version, unsigned cfg_hash, const void *blob, long long bytes, BlobHeader *h)
{
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return blob_status(c, blob_load(parts, magic, cfg_hash, blob, bytes, h, version));
}

}  // namespace mca

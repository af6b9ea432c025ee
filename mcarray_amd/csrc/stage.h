// stage.h -- grow-only device staging buffers for the host-pointer entry points (*_frames_host): a streaming
// caller hands over one small chunk after another, and a hipMalloc/hipFree pair per buffer and call costs
// more than the kernels of a small chunk.
#pragma once
#include "devbuf.h"

namespace mca {

struct StagePool {
    static constexpr int N = 10;          // (slots 8, 9: the update mask and the target masks of the MVDR host calls)
    DevBuf<unsigned char> buf[N];
    // returns a device buffer of at least `bytes` bytes for slot i (nullptr on allocation failure or bytes == 0)
    void *get(int i, size_t bytes)
    {
        if (bytes == 0) return nullptr;
        // head room: chunk sizes of a stream vary a little
        if (bytes > buf[i].n && buf[i].grow(bytes + bytes / 4) != hipSuccess) return nullptr;
        return buf[i].p;
    }
    void release()
    {
        for (auto &b : buf) b.reset();
    }
};

}  // namespace mca

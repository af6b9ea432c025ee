"""Python mirror of the reference's module API on top of the C ABI (libmcarray_hip.so).

Class and method names follow the reference (mca::SteeringBeamforming, mca::Beamformer,
mca::BeamformingSeparationAndLocalisation, mca::SourceSeparationAndLocalisation), so the parity
tests read like the reference's tests.  Everything numerical happens in the HIP library; numpy is
used only to marshal buffers.  torch is optional here and only used by the *_dev helpers
(device tensors in, device tensors out).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MCArrayHipError

SRP_FP32, SRP_FP16X3, SRP_FP16, SRP_ADAPTIVE = 0, 1, 2, 3
GCC_PHAT, GCC_NONE = 0, 1            # mca_hip_gcc_weighting
K_STFT_PHAT, K_SRP_GEMM, K_SCAN_PICK, K_BEAMFORM, K_GCC2_SCAN, K_MASK, K_FOLD, K_REPAIR = 0, 1, 2, 3, 4, 5, 6, 7
KERNEL_NAMES = {K_STFT_PHAT: "k_stft_phat", K_SRP_GEMM: "k_srp_gemm", K_SCAN_PICK: "k_scan_pick", K_BEAMFORM: "k_beamform_ola",
                K_FOLD: "k_sum_planes", K_REPAIR: "repair"}


class PinnedBuffer:
    """numpy view of page-locked host memory (mca_hip_host_alloc): buffers of this kind make the host-pointer entry points
    overlap upload, kernels and download at the rate of the PCIe link.  Keep the object alive while `.array` is in use."""

    def __init__(self, shape, dtype):
        self._lib = _lib.load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = self._lib.mca_hip_host_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise MCArrayHipError("mca_hip_host_alloc(%d) failed" % self.nbytes)
        raw = (C.c_char * max(self.nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(raw, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.mca_hip_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()


def pcm_layout(pcm):
    """(ptr, array_stride, ch_stride) of a torch float32 tensor [A][C][L] for the *_frames_dev entry points: sample n of channel c
    of array a at ptr[a*array_stride + c*ch_stride + n].  Rows and arrays may be padded and the view may start anywhere in its
    allocation; L may exceed what the call reads.  Reads data_ptr(), stride() and dtype only (CPU tensors work as well); the C
    layer checks ranges, parity and alignment."""
    if len(pcm.shape) != 3:
        raise MCArrayHipError("pcm must be a tensor [A][C][L]")
    if "float32" not in str(pcm.dtype):
        raise MCArrayHipError("pcm must be float32, not %s" % pcm.dtype)
    sa, sc, sn = pcm.stride()
    if sn != 1:
        raise MCArrayHipError("the samples of a pcm row must be adjacent (inner stride 1, not %d)" % sn)
    return C.c_void_p(pcm.data_ptr()), int(sa), int(sc)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _xyz(x):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 1:   # ArrayDescription::make_linear_array_description (ArrayDescription.cpp:41-49)
        a = np.stack([a, np.zeros_like(a), np.zeros_like(a)], axis=1)
    return np.ascontiguousarray(a)


class Context:
    """Owns one mca_hip_ctx (the state of max_arrays independent module objects)."""

    def __init__(self, sample_rate, mic_positions, fft_size=1024, doa_step_deg=5.0, n_sources=1, use_power_floor=False,
                 srp_precision=SRP_FP32, max_arrays=1, device=0, gcc_weighting=GCC_PHAT, adaptive_fallback=True,
                 adaptive_min_rows=0, adaptive_max_sources=0, scan_carry=False):
        self._lib = _lib.load()
        self.xyz = _xyz(mic_positions)
        self.M = len(self.xyz)
        self.N = fft_size
        self.hop = fft_size // 2
        self.S = n_sources
        self.fs = sample_rate
        self.use_power_floor = bool(use_power_floor)
        cfg = _lib.Config()
        cfg.struct_size = C.sizeof(_lib.Config)
        cfg.device = device
        cfg.sample_rate = sample_rate
        cfg.fft_size = fft_size
        cfg.n_mics = self.M
        cfg.mic_xyz = self.xyz.ctypes.data_as(_lib.c_dp)
        cfg.doa_step_deg = doa_step_deg
        cfg.n_sources = n_sources
        cfg.use_power_floor = int(use_power_floor)
        cfg.srp_precision = srp_precision
        cfg.max_arrays = max_arrays
        cfg.gcc_weighting = gcc_weighting
        cfg.adaptive_fallback = 0 if adaptive_fallback else 1      # mca_hip_adaptive_fallback: AUTO / OFF (OFF: bit-reproducible runs)
        cfg.adaptive_min_rows = adaptive_min_rows
        cfg.adaptive_max_sources = adaptive_max_sources
        cfg.scan_carry = int(scan_carry)
        h = C.c_void_p()
        rc = self._lib.mca_hip_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_create failed (%d): %s" % (rc, self._lib.mca_hip_last_error(None).decode()))
        self.h = h
        self.D = self._lib.mca_hip_num_steps(h)
        self.P = self._lib.mca_hip_num_pairs(h)
        self.G = self._lib.mca_hip_num_groups(h)

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_last_error(self.h).decode()))

    # ---- introspection ----
    def pair_delays(self):
        out = np.empty((self.P, self.D), dtype=np.float32)
        self._check(self._lib.mca_hip_get_pair_delays(self.h, out.ctypes.data_as(_lib.c_fp)))
        return out

    def doa_grid(self):
        out = np.empty(self.D, dtype=np.float32)
        self._check(self._lib.mca_hip_get_doa_grid(self.h, out.ctypes.data_as(_lib.c_fp)))
        return out

    def reset(self, stream=None):
        self._check(self._lib.mca_hip_reset(self.h, stream))

    def reserve(self, n_arrays, n_frames):
        self._check(self._lib.mca_hip_reserve(self.h, n_arrays, n_frames))

    def state_save(self):
        """checkpoint of the per-array stream state (E_prev, overlap-add tails, gate, last DOA ...) as bytes"""
        n = self._lib.mca_hip_state_size(self.h)
        buf = C.create_string_buffer(n)
        self._check(self._lib.mca_hip_state_save(self.h, buf, n))
        return buf.raw

    def state_load(self, blob):
        self._check(self._lib.mca_hip_state_load(self.h, blob, len(blob)))

    # ---- stream API, host buffers ----
    def process_frames_host(self, pcm, want_energy=False, want_audio=True, into=None):
        """pcm float32 [A][M][(F+1)*hop] -> dict(bin [A][F][S], doa, prob, energy [A][F][D], out [A][S][F*hop]).
        into: optional dict of preallocated result arrays (e.g. PinnedBuffer(...).array) for bin / doa / prob / energy / out."""
        i16 = isinstance(pcm, np.ndarray) and pcm.dtype == np.int16       # 16-bit PCM goes up as it is (half the PCIe bytes)
        pcm = np.ascontiguousarray(pcm, dtype=np.int16 if i16 else np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, M, L = pcm.shape
        if M != self.M:
            raise MCArrayHipError("pcm has %d channels, context has %d microphones" % (M, self.M))
        F = L // self.hop - 1
        if F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm length must be (F+1)*hop samples")
        S, D = self.S, self.D
        into = into or {}

        def buf(key, shape, dtype):
            b = into.get(key)
            if b is None:
                return np.empty(shape, dtype=dtype)
            if b.shape != shape or b.dtype != dtype or not b.flags["C_CONTIGUOUS"]:
                raise MCArrayHipError("into[%r] must be a contiguous %s array of shape %s" % (key, np.dtype(dtype).name, shape))
            return b
        bins = buf("bin", (A, F, S), np.int32)
        doa = buf("doa", (A, F, S), np.float32)
        prob = buf("prob", (A, F, S), np.float32)
        energy = buf("energy", (A, F, D), np.float32) if want_energy else None
        out = buf("out", (A, S, F * self.hop), np.float32) if want_audio else None
        fp = _lib.c_fp
        entry = self._lib.mca_hip_process_frames_host_i16 if i16 else self._lib.mca_hip_process_frames_host
        self._check(entry(
            self.h, pcm.ctypes.data_as(C.POINTER(C.c_short) if i16 else fp), A, F, bins.ctypes.data_as(_lib.c_ip), doa.ctypes.data_as(fp),
            prob.ctypes.data_as(fp), energy.ctypes.data_as(fp) if want_energy else None,
            out.ctypes.data_as(fp) if want_audio else None))
        res = dict(bin=bins, doa=doa, prob=prob, energy=energy, out=out)
        if self.use_power_floor:
            voiced = np.empty((A, F), dtype=np.uint8)
            power = np.empty((A, F), dtype=np.float32)
            self._check(self._lib.mca_hip_copy_gate(self.h, voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(fp)))
            res["voiced"] = voiced
            res["power"] = power
        return res

    # ---- stream API, device tensors (torch used for memory only) ----
    def process_frames_dev(self, pcm, n_frames, doa_bin, doa_rad, prob, energy=None, out_pcm=None, stream=None,
                           localise=True, separate=True, bins_are_grid=False):
        """pcm: torch float32 cuda tensor [A][M][>= (F+1)*hop], rows and arrays at any even strides (pcm_layout); outputs
        preallocated cuda tensors.
        bins_are_grid (separation only): doa_rad holds the grid angles of doa_bin (the localiser's own picks)."""
        A, M, L = pcm.shape
        if M != self.M:
            raise MCArrayHipError("pcm has %d channels, context has %d microphones" % (M, self.M))
        p, sa, sc = pcm_layout(pcm)
        ptr = _ptr
        if localise and separate and out_pcm is not None and doa_rad is not None:
            self._check(self._lib.mca_hip_process_frames_dev(self.h, p, sa, sc, A, n_frames, ptr(doa_bin), ptr(doa_rad), ptr(prob),
                                                             ptr(energy), ptr(out_pcm), stream))
            return
        if localise:
            self._check(self._lib.mca_hip_localise_frames_dev(self.h, p, sa, sc, A, n_frames, ptr(doa_bin),
                                                              ptr(doa_rad), ptr(prob), ptr(energy), stream))
        if separate and out_pcm is not None:
            if bins_are_grid and doa_bin is not None:
                self._check(self._lib.mca_hip_separate_frames_bins_dev(self.h, p, sa, sc, A, n_frames, ptr(doa_bin), ptr(doa_rad),
                                                                       ptr(out_pcm), stream))
            else:
                self._check(self._lib.mca_hip_separate_frames_dev(self.h, p, sa, sc, A, n_frames, ptr(doa_rad),
                                                                  ptr(out_pcm), stream))

    # ---- real-time mode: the stream call as a HIP graph ----
    def graph_create(self, pcm, n_frames, doa_bin, doa_rad, prob, energy=None, out_pcm=None):
        """Fixes the shape and buffers (torch cuda tensors, as process_frames_dev) of a stream call; returns a StreamGraph
        whose launch() replays the call's kernels as one HIP graph on the current contents of `pcm`."""
        A, M, L = pcm.shape
        if M != self.M:
            raise MCArrayHipError("pcm must be a [A][M][L] tensor with M = the context's microphones")
        p, sa, sc = pcm_layout(pcm)
        ptr = _ptr
        h = C.c_void_p()
        self._check(self._lib.mca_hip_graph_create(self.h, p, sa, sc, A, n_frames, ptr(doa_bin), ptr(doa_rad), ptr(prob),
                                                   ptr(energy), ptr(out_pcm), C.byref(h)))
        return StreamGraph(self, h, (pcm, doa_bin, doa_rad, prob, energy, out_pcm))

    # ---- 2-microphone GCC-PHAT path ----
    def gcc2_frames_host(self, pcm, want_corr=False):
        """pcm float32 [A][2][(F+1)*hop] -> dict(argmax [A][F], doa [A][F] (smoothed, rad), prob [A][F], corr [A][F][D])"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, M, L = pcm.shape
        F = L // self.hop - 1
        if M != 2 or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [A][2][(F+1)*hop]")
        idx = np.empty((A, F), dtype=np.int32)
        doa = np.empty((A, F), dtype=np.float32)
        prob = np.empty((A, F), dtype=np.float32)
        corr = np.empty((A, F, self.D), dtype=np.float32) if want_corr else None
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_gcc2_frames_host(self.h, pcm.ctypes.data_as(fp), A, F, idx.ctypes.data_as(_lib.c_ip),
                                                       doa.ctypes.data_as(fp), prob.ctypes.data_as(fp),
                                                       corr.ctypes.data_as(fp) if want_corr else None))
        res = dict(argmax=idx, doa=doa, prob=prob, corr=corr)
        if self.use_power_floor:     # the gate of BinauralLocalisation.cpp:425-434: which frames fired, and the power handed to setDOA
            voiced = np.empty((A, F), dtype=np.uint8)
            power = np.empty((A, F), dtype=np.float32)
            self._check(self._lib.mca_hip_copy_gate(self.h, voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(fp)))
            res["voiced"] = voiced
            res["power"] = power
        return res

    def gcc2_frames_dev(self, pcm, n_frames, argmax, doa_rad=None, prob=None, corr=None, stream=None):
        """mca_hip_gcc2_frames_dev: pcm torch float32 cuda tensor [A][2][>= (F+1)*hop]; outputs preallocated cuda tensors
        argmax int32 [A][F], doa_rad / prob float32 [A][F], corr float32 [A][F][D] (all but argmax optional)."""
        A, M, L = pcm.shape
        if M != 2:
            raise MCArrayHipError("pcm must be a [A][2][L] tensor")
        p, sa, sc = pcm_layout(pcm)
        ptr = _ptr
        self._check(self._lib.mca_hip_gcc2_frames_dev(self.h, p, sa, sc, A, n_frames, ptr(argmax), ptr(doa_rad), ptr(prob),
                                                      ptr(corr), stream))

    # ---- the particle-filter DOA tracker of the 2-microphone path ----
    def gcc2_tracker_attach(self, seed=0, n_particles=0, n_inject=0, sigma_init=0.0, sigma_step=0.0):
        """mca_hip_gcc2_tracker_attach: from now on the tracked calls below replace gcc2_frames_*, and gcc2_process_frame runs the
        tracker on the frame hook's state.  0 = the defaults (500 particles, n_particles / 20 injected, sigmas = the grid step);
        n_inject = -1: none."""
        cfg = _lib.Gcc2TrackerConfig()
        cfg.struct_size = C.sizeof(_lib.Gcc2TrackerConfig)
        cfg.n_particles, cfg.n_inject, cfg.seed = int(n_particles), int(n_inject), int(seed)
        cfg.sigma_init, cfg.sigma_step = float(sigma_init), float(sigma_step)
        self._check(self._lib.mca_hip_gcc2_tracker_attach(self.h, C.byref(cfg)))
        self.tracked = True
        self.n_particles = int(n_particles) or 500

    def gcc2_tracked_frames_host(self, pcm, want_corr=False):
        """pcm float32 [A][2][(F+1)*hop] -> dict(argmax, doa (tracked, rad), prob, fired (1 voiced, 2 coasting, 0 nothing), track
        [A][F], corr [A][F][D][, voiced, power])"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, M, L = pcm.shape
        F = L // self.hop - 1
        if M != 2 or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [A][2][(F+1)*hop]")
        idx = np.empty((A, F), dtype=np.int32)
        doa = np.empty((A, F), dtype=np.float32)
        prob = np.empty((A, F), dtype=np.float32)
        fired = np.empty((A, F), dtype=np.uint8)
        track = np.empty((A, F), dtype=np.int32)
        corr = np.empty((A, F, self.D), dtype=np.float32) if want_corr else None
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_gcc2_tracked_frames_host(
            self.h, pcm.ctypes.data_as(fp), A, F, idx.ctypes.data_as(_lib.c_ip), doa.ctypes.data_as(fp), prob.ctypes.data_as(fp),
            fired.ctypes.data_as(C.c_void_p), track.ctypes.data_as(_lib.c_ip), corr.ctypes.data_as(fp) if want_corr else None))
        res = dict(argmax=idx, doa=doa, prob=prob, fired=fired, track=track, corr=corr)
        if self.use_power_floor:
            voiced = np.empty((A, F), dtype=np.uint8)
            power = np.empty((A, F), dtype=np.float32)
            self._check(self._lib.mca_hip_copy_gate(self.h, voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(fp)))
            res["voiced"] = voiced
            res["power"] = power
        return res

    def gcc2_tracked_frames_dev(self, pcm, n_frames, doa_rad, argmax=None, prob=None, fired=None, track=None, corr=None, stream=None):
        """mca_hip_gcc2_tracked_frames_dev: pcm torch float32 cuda tensor [A][2][>= (F+1)*hop]; outputs preallocated cuda tensors
        doa_rad / prob float32, argmax / track int32, fired uint8 [A][F], corr float32 [A][F][D] (all but doa_rad optional)."""
        A, M, L = pcm.shape
        if M != 2:
            raise MCArrayHipError("pcm must be a [A][2][L] tensor")
        p, sa, sc = pcm_layout(pcm)
        ptr = _ptr
        self._check(self._lib.mca_hip_gcc2_tracked_frames_dev(self.h, p, sa, sc, A, n_frames, ptr(argmax), ptr(doa_rad), ptr(prob),
                                                              ptr(fired), ptr(track), ptr(corr), stream))

    def gcc2_tracker_particles(self, array_index=0):
        """-> dict(particles float64 [n_particles] (rad), alive, track) of array `array_index`; -1: of the frame hook"""
        x = np.empty(getattr(self, "n_particles", 500))
        alive, track = C.c_int(0), C.c_int(0)
        self._check(self._lib.mca_hip_gcc2_tracker_get_particles(self.h, int(array_index), x.ctypes.data_as(_lib.c_dp), C.byref(alive),
                                                                 C.byref(track)))
        return dict(particles=x, alive=bool(alive.value), track=track.value)

    def gcc2_set_probability(self, doas, array_index=0):
        """setProbability (BinauralLocalisation.cpp:569-631) at the angles `doas` (radians) on the smoothed correlation the last
        gcc2_frames_* call left for array `array_index` -> float64 [n]"""
        doas = np.ascontiguousarray(doas, dtype=np.float64).reshape(-1)
        probs = np.empty(len(doas))
        self._check(self._lib.mca_hip_gcc2_set_probability(self.h, int(array_index), doas.ctypes.data_as(_lib.c_dp),
                                                           probs.ctypes.data_as(_lib.c_dp), len(doas)))
        return probs

    def gcc2_set_probability_dev(self, doas, probs, stream=None):
        """The same for arrays 0..A-1 in one launch: doas / probs torch float32 cuda tensors [A][n], enqueued on `stream`."""
        if doas.dim() != 2 or tuple(probs.shape) != tuple(doas.shape) or not doas.is_contiguous() or not probs.is_contiguous():
            raise MCArrayHipError("doas and probs must be contiguous [A][n] tensors of one shape")
        A, n = doas.shape
        self._check(self._lib.mca_hip_gcc2_set_probability_dev(self.h, A, C.c_void_p(doas.data_ptr()), C.c_void_p(probs.data_ptr()), n,
                                                               stream))

    def gcc2_process_frame(self, frames):
        """FreqGCCBinauralLocalisation::processParametrisation for one frame: frames [2][N+2] CCS (double) ->
        dict(voiced, doa, prob, power, argmax, corr [D]) after the frame (BinauralLocalisation.cpp:406-567)."""
        frames, arr = self._rows(frames)
        v, i = C.c_int(0), C.c_int(0)
        doa, prob, power = C.c_double(0), C.c_double(0), C.c_double(0)
        corr = np.empty(self.D)
        self._check(self._lib.mca_hip_gcc2_process_frame(self.h, arr, frames.shape[1], C.byref(v), C.byref(doa), C.byref(prob),
                                                         C.byref(power), C.byref(i), corr.ctypes.data_as(_lib.c_dp)))
        r = dict(voiced=bool(v.value), doa=doa.value, prob=prob.value, power=power.value, argmax=i.value, corr=corr)
        if getattr(self, "tracked", False):      # with a tracker `voiced` carries fired: 1 voiced, 2 a coasting track, 0 nothing
            r["voiced"] = v.value == 1
            r["fired"] = v.value
            r["track"] = self.gcc2_tracker_particles(-1)["track"]
        return r

    def gcc2_frame_set_probability(self, doas):
        """setProbability on the frame hook's correlation (gcc2_process_frame) -> float64 [n]"""
        doas = np.ascontiguousarray(doas, dtype=np.float64).reshape(-1)
        probs = np.empty(len(doas))
        self._check(self._lib.mca_hip_gcc2_frame_set_probability(self.h, doas.ctypes.data_as(_lib.c_dp), probs.ctypes.data_as(_lib.c_dp),
                                                                 len(doas)))
        return probs

    # ---- frame API ----
    def _rows(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        if frames.shape[0] != self.M:
            raise MCArrayHipError("expected %d channel spectra" % self.M)
        arr = (_lib.c_dp * self.M)()
        for c in range(self.M):
            arr[c] = frames[c].ctypes.data_as(_lib.c_dp)
        return frames, arr

    def steering_process_frame(self, frames, n_sources=1):
        frames, arr = self._rows(frames)
        doa = np.empty(n_sources)
        prob = np.empty(n_sources)
        bins = np.empty(n_sources, dtype=np.int32)
        self._check(self._lib.mca_hip_steering_process_frame(self.h, arr, frames.shape[1], doa.ctypes.data_as(_lib.c_dp),
                                                             prob.ctypes.data_as(_lib.c_dp), bins.ctypes.data_as(_lib.c_ip),
                                                             n_sources))
        return doa, prob, bins

    def beamformer_process_frame(self, frames, doa):
        frames, arr = self._rows(frames)
        out = np.empty(frames.shape[1])
        self._check(self._lib.mca_hip_beamformer_process_frame(self.h, arr, frames.shape[1], out.ctypes.data_as(_lib.c_dp), float(doa)))
        return out

    def fft_log_power(self, frames):
        frames, arr = self._rows(frames)
        p = C.c_double(0)
        self._check(self._lib.mca_hip_fft_log_power(self.h, arr, frames.shape[1], C.byref(p)))
        return p.value

    def energy(self):
        out = np.empty(self.D)
        self._check(self._lib.mca_hip_get_energy(self.h, out.ctypes.data_as(_lib.c_dp)))
        return out

    # ---- measurement ----
    def set_timing(self, enable):
        self._check(self._lib.mca_hip_set_timing(self.h, int(enable)))

    def set_timing_kernels(self, kernel_ids):
        """event pairs around the launches of these kernel ids only (each pair costs the stream ~1.5 us)"""
        mask = 0
        for k in kernel_ids:
            mask |= 1 << int(k)
        self._check(self._lib.mca_hip_set_timing_mask(self.h, mask))

    def reset_timing(self):
        self._check(self._lib.mca_hip_reset_timing(self.h))

    def repair_stats(self):
        """SRP_ADAPTIVE: dict(frames, flagged, recomputed) since the last reset_timing()"""
        a, b, c_ = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.mca_hip_get_repair_stats(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        return {"frames": a.value, "flagged": b.value, "recomputed": c_.value}

    def steer_stats(self):
        """dict(frames, missed, fused_calls) of the device-pointer calls that steer on the half spectrum (mca_hip_get_steer_stats)"""
        a, b, c_ = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.mca_hip_get_steer_stats(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        return {"frames": a.value, "missed": b.value, "fused_calls": c_.value}

    def repair_columns(self):
        """SRP_ADAPTIVE: dict(candidate_columns, whole_row_frames) since the last reset_timing() (mca_hip_get_repair_columns)"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.mca_hip_get_repair_columns(self.h, C.byref(a), C.byref(b)))
        return {"candidate_columns": a.value, "whole_row_frames": b.value}

    def get_timing(self, kernel_id):
        n = C.c_int(0)
        ms = C.c_double(0)
        self._check(self._lib.mca_hip_get_timing(self.h, kernel_id, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class StreamGraph:
    """Handle of mca_hip_graph (include/mcarray_hip.h, real-time mode); keeps the buffers alive."""

    def __init__(self, ctx, h, keep):
        self.ctx, self.h, self._keep = ctx, h, keep
        self._lib = ctx._lib

    def launch(self, stream=None):
        rc = self.ctx._lib.mca_hip_graph_launch(self.h, stream)
        if rc != 0:     # (the context may be gone: its error string then lives in the library, not in the context)
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self.ctx._lib.mca_hip_last_error(self.ctx.h).decode()))

    def close(self):
        # safe in either order: a context that is destroyed first orphans its graphs (their recordings go with it)
        if getattr(self, "h", None):
            self._lib.mca_hip_graph_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()


class SteeringBeamforming:
    """mca::SteeringBeamforming(int sampleRate, ArrayDescription, int fftCCSLength, unsigned nchannels)
    (SteeringBeamforming.h:43); processFrame (:54) returns (DOA[S] rad, prob[S], bin[S])."""

    def __init__(self, sample_rate, mic_positions, fft_ccs_length, nchannels=None, doa_step_deg=5.0, device=0):
        self.ctx = Context(sample_rate, mic_positions, fft_ccs_length - 2, doa_step_deg, n_sources=4, device=device)
        if nchannels is not None and nchannels != self.ctx.M:
            raise MCArrayHipError("nchannels does not match the array description")

    def process_frame(self, analysis_frames, n_sources=1):
        return self.ctx.steering_process_frame(analysis_frames, n_sources)


class Beamformer:
    """mca::Beamformer(int sampleRate, ArrayDescription, int fftCCSLength, unsigned nchannels) (Beamformer.h:39)."""

    def __init__(self, sample_rate, mic_positions, fft_ccs_length, nchannels=None, device=0):
        self.ctx = Context(sample_rate, mic_positions, fft_ccs_length - 2, device=device)

    def process_frame(self, analysis_frames, doa):
        return self.ctx.beamformer_process_frame(analysis_frames, doa)


def calculate_order_from_sample_rate(sample_rate, frame_seconds):
    """[BUILD-DEFINES] stand-in for dsp::STFT::calculateOrderFromSampleRate: the frame length the
    reference's stream modules derive from the sample rate, N = 2^order."""
    order = int(np.floor(np.log2(sample_rate * frame_seconds) + 0.5))
    return min(max(order, 8), 14)


class SourceSeparationAndLocalisation:
    """mca::SourceSeparationAndLocalisation(int sampleRate, ArrayDescription, unsigned numOfSources,
    bool usePowerFloor) (SourceSeparationAndLocalisation.h:47) driven over whole buffers: process()
    takes channel-major PCM, returns the beamformed audio and calls the callback once per frame
    like LocalisationCallback::setDOA(doaDegrees, prob, power, numOfSources) (SoundLocalisationCallback.h:53)."""

    FRAME_SECONDS = 0.025        # _frameRate (SourceSeparationAndLocalisation.h:60)

    def __init__(self, sample_rate, mic_positions, n_sources=1, use_power_floor=False, doa_step_deg=5.0, fft_size=None,
                 srp_precision=SRP_FP32, device=0):
        if fft_size is None:
            fft_size = 1 << calculate_order_from_sample_rate(sample_rate, self.FRAME_SECONDS)   # .cpp:52
        self.ctx = Context(sample_rate, mic_positions, fft_size, doa_step_deg, n_sources, use_power_floor, srp_precision, 1, device)
        self.callback = None

    def set_callback(self, cb):
        self.callback = cb

    def process(self, pcm):
        r = self.ctx.process_frames_host(np.asarray(pcm, dtype=np.float32)[None], want_energy=False, want_audio=True)
        if self.callback is not None:
            deg = r["doa"][0].astype(np.float64) * (180.0 / np.pi)   # toDegrees (microhponeArrayHelpers.cpp:91-98)
            for t in range(deg.shape[0]):
                if "voiced" in r and not r["voiced"][0, t]:
                    continue                                   # gated out: the reference does not call setDOA (:87-94)
                self.callback(deg[t], r["prob"][0, t], r["power"][0, t] if "power" in r else None, self.ctx.S)
        return r["out"][0], r


class SourceLocalisation(SourceSeparationAndLocalisation):
    """mca::SourceLocalisation(int sampleRate, ArrayDescription, unsigned numOfSources, bool usePowerFloor)
    (SourceLocalisation.h:43): the analysis-only sibling -- localisation and callbacks, no audio out
    (SourceLocalisation.cpp:63-79 calls processFrameLocalisation only)."""

    def process(self, pcm):
        r = self.ctx.process_frames_host(np.asarray(pcm, dtype=np.float32)[None], want_energy=False, want_audio=False)
        if self.callback is not None:
            deg = r["doa"][0].astype(np.float64) * (180.0 / np.pi)
            for t in range(deg.shape[0]):
                if "voiced" in r and not r["voiced"][0, t]:
                    continue
                self.callback(deg[t], r["prob"][0, t], r["power"][0, t] if "power" in r else None, self.ctx.S)
        return r


class FreqGCCBinauralLocalisation:
    """mca::FreqGCCBinauralLocalisation(int sampleRate, ArrayDescription, bool usePowerFloor)
    (BinauralLocalisation.h:191), deterministic part: smoothed GCC-PHAT correlation, first-max argmax,
    DOA smoothing and setProbability.  The reference's grid is 3 degrees (BinauralLocalisation.cpp:328).
    process() (PCM, batched stream path) and process_frame() (one frame of CCS spectra, the per-frame hook) keep separate
    states; set_probability() reads the one of the path used last.
    particle_filter: None, or a dict of Context.gcc2_tracker_attach's arguments ({} = the defaults): the DOA then comes from the
    particle filter the reference is compiled with (BinauralLocalisation.cpp:38), process() / process_frame() also return `fired`
    and `track`, and the callback fires on every frame whose fired is 1 or 2 (a track coasting through a pause, :536-548)."""

    FRAME_SECONDS = 0.075        # _frameRate (BinauralLocalisation.h:196)

    def __init__(self, sample_rate, mic_positions, use_power_floor=False, doa_step_deg=3.0, fft_size=None,
                 srp_precision=SRP_FP32, max_arrays=1, device=0, particle_filter=None):
        if fft_size is None:
            fft_size = 1 << calculate_order_from_sample_rate(sample_rate, self.FRAME_SECONDS)
        self.ctx = Context(sample_rate, mic_positions, fft_size, doa_step_deg, 1, use_power_floor, srp_precision, max_arrays, device)
        if self.ctx.M != 2:
            raise MCArrayHipError("FreqGCCBinauralLocalisation needs exactly 2 microphones")
        self.tracked = particle_filter is not None
        if self.tracked:
            self.ctx.gcc2_tracker_attach(**particle_filter)
        self.callback = None
        self._frame_path_last = False

    def set_callback(self, cb):
        self.callback = cb

    def process(self, pcm, want_corr=False):
        """-> dict(argmax, doa, prob[, corr][, voiced, power]); the callback fires per frame of array 0 that passed the gate
        as setDOA(degrees, prob, power, 1) (BinauralLocalisation.cpp:521)."""
        r = self.ctx.gcc2_tracked_frames_host(pcm, want_corr) if self.tracked else self.ctx.gcc2_frames_host(pcm, want_corr)
        self._frame_path_last = False
        if self.callback is not None:
            for t in range(r["doa"].shape[1]):
                if (not r["fired"][0, t]) if self.tracked else ("voiced" in r and not r["voiced"][0, t]):
                    continue
                self.callback(np.array([np.rad2deg(float(r["doa"][0, t]))]), np.array([r["prob"][0, t]]),
                              float(r["power"][0, t]) if "power" in r else 0.0, 1)
        return r

    def process_frame(self, left, right):
        """processParametrisation (BinauralLocalisation.cpp:406-567) for one frame of CCS spectra double[N+2] -> dict(voiced, doa,
        prob, power, argmax, corr); the callback fires on a voiced frame as setDOA(degrees, prob, power, 1) (:521)."""
        r = self.ctx.gcc2_process_frame(np.stack([np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)]))
        self._frame_path_last = True
        if self.callback is not None and (r["fired"] if self.tracked else r["voiced"]):
            self.callback(np.array([np.rad2deg(r["doa"])]), np.array([r["prob"]]), r["power"], 1)
        return r

    def set_probability(self, doas, array_index=0):
        """setProbability (BinauralLocalisation.cpp:569-631) at the angles `doas` (radians) -> float64: on process_frame()'s state
        if that path ran last, else on process()'s state of array `array_index`."""
        if self._frame_path_last:
            return self.ctx.gcc2_frame_set_probability(doas)
        return self.ctx.gcc2_set_probability(doas, array_index)


class _StateBlob:
    """state_save() / state_load() over mca_hip_<module>_state_* (checkpoint / resume of everything the module carries between calls)."""
    _STATE = None    # module infix of the C entry points

    def state_save(self):
        size = getattr(self._lib, "mca_hip_%s_state_size" % self._STATE)(self.h)
        if size < 0:
            self._check(int(size))
        blob = C.create_string_buffer(int(size))
        self._check(getattr(self._lib, "mca_hip_%s_state_save" % self._STATE)(self.h, blob, size))
        return blob.raw

    def state_load(self, blob):
        self._check(getattr(self._lib, "mca_hip_%s_state_load" % self._STATE)(self.h, blob, len(blob)))


class MultibandBinarualLocalisation(_StateBlob):
    _STATE = "mb"
    """mca::MultibandBinarualLocalisation(int sampleRate, ArrayDescription, int nbins = 15, bool usePowerFloor = 1)
    (MultibandBinarualLocalisation.h:38): per sub-band GCC-PHAT + energy-weighted DOA histogram over whole buffers."""

    FRAME_SECONDS = 0.025        # _frameRate (MultibandBinarualLocalisation.h:43)

    def __init__(self, sample_rate, mic_positions, nbins=15, use_power_floor=True, fft_size=None, max_arrays=1, device=0):
        self._lib = _lib.load()
        xyz = _xyz(mic_positions)
        if len(xyz) != 2:
            raise MCArrayHipError("MultibandBinarualLocalisation needs exactly 2 microphones")
        if fft_size is None:
            fft_size = 1 << calculate_order_from_sample_rate(sample_rate, self.FRAME_SECONDS)
        cfg = _lib.MbConfig()
        cfg.struct_size = C.sizeof(_lib.MbConfig)
        cfg.device = device
        cfg.sample_rate = sample_rate
        cfg.fft_size = fft_size
        cfg.mic_xyz = xyz.ctypes.data_as(_lib.c_dp)
        cfg.nbins = nbins
        cfg.use_power_floor = int(use_power_floor)
        cfg.max_arrays = max_arrays
        h = C.c_void_p()
        rc = self._lib.mca_hip_mb_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_mb_create failed (%d): %s" % (rc, self._lib.mca_hip_mb_last_error(None).decode()))
        self.h = h
        self.N, self.hop, self.nbins = fft_size, fft_size // 2, nbins
        self.D = self._lib.mca_hip_mb_num_steps(h)
        self.callback = None

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_mb_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_mb_last_error(self.h).decode()))

    def set_callback(self, cb):
        self.callback = cb

    def reset(self):
        self._check(self._lib.mca_hip_mb_reset(self.h, None))

    def filters(self):
        out = np.empty((self.nbins, self.N // 2 + 1))
        self._check(self._lib.mca_hip_mb_get_filters(self.h, out.ctypes.data_as(_lib.c_dp)))
        return out

    def process(self, pcm, want_bands=False):
        """pcm float32 [A][2][(F+1)*hop] -> dict(doa [A][F] rad, prob, voiced, power[, band_idx [A][F][nbins],
        energy_in_doa [A][F][D], band_corr [A][F][nbins][D]]); the callback fires per voiced frame of array 0
        as setDOA(degrees, prob, power, 1) (MultibandBinarualLocalisation.cpp:248)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, ch, L = pcm.shape
        F = L // self.hop - 1
        if ch != 2 or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [A][2][(F+1)*hop]")
        doa = np.empty((A, F), dtype=np.float32)
        prob = np.empty((A, F), dtype=np.float32)
        voiced = np.empty((A, F), dtype=np.uint8)
        power = np.empty((A, F), dtype=np.float32)
        bi = np.empty((A, F, self.nbins), dtype=np.int32) if want_bands else None
        eid = np.empty((A, F, self.D), dtype=np.float32) if want_bands else None
        bc = np.empty((A, F, self.nbins, self.D), dtype=np.float32) if want_bands else None
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_mb_frames_host(
            self.h, pcm.ctypes.data_as(fp), A, F, doa.ctypes.data_as(fp), prob.ctypes.data_as(fp),
            voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(fp), bi.ctypes.data_as(_lib.c_ip) if want_bands else None,
            eid.ctypes.data_as(fp) if want_bands else None, bc.ctypes.data_as(fp) if want_bands else None))
        if self.callback is not None:
            for t in range(F):
                if voiced[0, t]:
                    self.callback(np.array([np.rad2deg(float(doa[0, t]))]), np.array([prob[0, t]]), float(power[0, t]), 1)
        return dict(doa=doa, prob=prob, voiced=voiced, power=power, band_idx=bi, energy_in_doa=eid, band_corr=bc)

    def process_dev(self, pcm, n_frames, doa_rad, prob, voiced=None, power=None, band_idx=None, energy_in_doa=None, band_corr=None,
                    stream=None):
        """device tensors (torch): pcm [A][2][>= (F+1)*hop] float32 at any even strides (pcm_layout); outputs preallocated and
        contiguous, shapes and types as process() returns them (doa_rad, prob required); asynchronous on `stream` (a raw
        hipStream_t or None)."""
        A, ch, L = pcm.shape
        if ch != 2:
            raise MCArrayHipError("pcm must be [A][2][L]")
        p, sa, sc = pcm_layout(pcm)
        self._check(self._lib.mca_hip_mb_frames_dev(self.h, p, sa, sc, A, int(n_frames), _ptr(doa_rad), _ptr(prob), _ptr(voiced),
                                                    _ptr(power), _ptr(band_idx), _ptr(energy_in_doa), _ptr(band_corr), stream))


class TemporalGCCBinauralLocalisation(_StateBlob):
    _STATE = "tgcc"
    """mca::TemporalGCCBinauralLocalisation(int sampleRate, ArrayDescription) (BinauralLocalisation.h:43): nd delay pairs of
    time-domain cross-correlations over raw frames of W = (int)(2 * 0.075 fs) samples at hop W / 2, DOA in degrees.
    use_power_floor=False (an extension, as FreqGCC's flag) voices every frame.  process() (PCM, batched stream path, float in)
    and process_frame() (one frame of doubles, the per-frame hook) keep separate states."""

    def __init__(self, sample_rate, mic_positions, use_power_floor=True, max_arrays=1, device=0):
        self._lib = _lib.load()
        xyz = _xyz(mic_positions)
        if len(xyz) != 2:
            raise MCArrayHipError("TemporalGCCBinauralLocalisation needs exactly 2 microphones")
        cfg = _lib.TgccConfig()
        cfg.struct_size = C.sizeof(_lib.TgccConfig)
        cfg.device = device
        cfg.sample_rate = sample_rate
        for j, v in enumerate(xyz.reshape(-1)):
            cfg.mic_xyz[j] = float(v)
        cfg.use_power_floor = int(use_power_floor)
        cfg.max_arrays = max_arrays
        h = C.c_void_p()
        rc = self._lib.mca_hip_tgcc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_tgcc_create failed (%d): %s" % (rc, self._lib.mca_hip_tgcc_last_error(None).decode()))
        self.h = h
        w, hop, nd = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.mca_hip_tgcc_get_geometry(h, C.byref(w), C.byref(hop), C.byref(nd)))
        self.W, self.hop, self.nd = w.value, hop.value, nd.value
        self.max_arrays = max_arrays
        self.callback = None

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_tgcc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_tgcc_last_error(self.h).decode()))

    def set_callback(self, cb):
        self.callback = cb

    def reset(self):
        self._check(self._lib.mca_hip_tgcc_reset(self.h, None))

    def get_window_size(self):
        return self.W

    get_analysis_length = get_window_size

    def num_frames(self, n_samples):
        return (n_samples - self.W) // self.hop + 1 if n_samples >= self.W else 0

    def process(self, pcm, want_index=False):
        """pcm float32 [A][2][(F-1)*hop + W] -> dict(doa [A][F] degrees, prob, voiced, power, delay_idx[, index [A][F][nd]]);
        the callback fires per voiced frame of array 0 as setDOA(degrees, prob, power, 1) (BinauralLocalisation.cpp:189-190)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, ch, L = pcm.shape
        F = self.num_frames(L)
        if ch != 2 or F < 1 or (F - 1) * self.hop + self.W != L:
            raise MCArrayHipError("pcm must be [A][2][(F-1)*hop + W]")
        doa = np.empty((A, F), dtype=np.float32)
        prob = np.empty((A, F), dtype=np.float32)
        voiced = np.empty((A, F), dtype=np.uint8)
        power = np.empty((A, F), dtype=np.float32)
        k = np.empty((A, F), dtype=np.int32)
        index = np.empty((A, F, self.nd), dtype=np.float64) if want_index else None
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_tgcc_frames_host(
            self.h, pcm.ctypes.data_as(fp), A, F, doa.ctypes.data_as(fp), prob.ctypes.data_as(fp),
            voiced.ctypes.data_as(C.c_void_p), power.ctypes.data_as(fp), k.ctypes.data_as(_lib.c_ip),
            index.ctypes.data_as(_lib.c_dp) if want_index else None))
        if self.callback is not None:
            for t in range(F):
                if voiced[0, t]:
                    self.callback(np.array([float(doa[0, t])]), np.array([float(prob[0, t])]), float(power[0, t]), 1)
        return dict(doa=doa, prob=prob, voiced=voiced, power=power, delay_idx=k, index=index)

    def process_dev(self, pcm, stream=None, want_index=False, n_frames=None, out=None):
        """device-pointer form: pcm a torch float32 CUDA tensor [A][2][(F-1)*hop + W], rows and arrays at any strides
        (pcm_layout) -> dict of torch tensors as process().  n_frames: process that many frames of rows that may be longer.
        out: a dict of preallocated tensors (doa, prob, power float32, voiced uint8, delay_idx int32 [A][F]; index float64
        [A][F][nd] with want_index) to write instead of fresh ones.  Asynchronous on `stream` (a raw hipStream_t or None)."""
        import torch
        A, ch, L = pcm.shape
        F = self.num_frames(L) if n_frames is None else int(n_frames)
        if ch != 2 or F < 1 or (n_frames is None and (F - 1) * self.hop + self.W != L):
            raise MCArrayHipError("pcm must be a float32 tensor [A][2][(F-1)*hop + W]")
        p, sa, sc = pcm_layout(pcm)
        dev = pcm.device
        if out is None:
            out = dict(doa=torch.empty((A, F), dtype=torch.float32, device=dev), prob=torch.empty((A, F), dtype=torch.float32, device=dev),
                       voiced=torch.empty((A, F), dtype=torch.uint8, device=dev), power=torch.empty((A, F), dtype=torch.float32, device=dev),
                       delay_idx=torch.empty((A, F), dtype=torch.int32, device=dev))
            out["index"] = torch.empty((A, F, self.nd), dtype=torch.float64, device=dev) if want_index else None
        self._check(self._lib.mca_hip_tgcc_frames_dev(
            self.h, p, sa, sc, A, F, _ptr(out["doa"]), _ptr(out["prob"]), _ptr(out["voiced"]), _ptr(out["power"]), _ptr(out["delay_idx"]),
            _ptr(out.get("index")) if want_index else None, stream))
        return out

    def process_frame(self, left, right):
        """processParametrisation (BinauralLocalisation.cpp:134-192) for one frame of double[W] per channel -> dict(voiced, doa
        (degrees), prob, power, delay_idx, index); the callback fires on a voiced frame as setDOA(degrees, prob, power, 1)."""
        fr = [np.ascontiguousarray(left, dtype=np.float64), np.ascontiguousarray(right, dtype=np.float64)]
        if fr[0].shape != (self.W,) or fr[1].shape != (self.W,):
            raise MCArrayHipError("process_frame needs two frames of W = %d samples" % self.W)
        ptrs = (_lib.c_dp * 2)(fr[0].ctypes.data_as(_lib.c_dp), fr[1].ctypes.data_as(_lib.c_dp))
        v, k = C.c_int(), C.c_int()
        doa, prob, power = C.c_double(), C.c_double(), C.c_double()
        index = np.empty(self.nd)
        self._check(self._lib.mca_hip_tgcc_process_frame(self.h, ptrs, self.W, C.byref(v), C.byref(doa), C.byref(prob), C.byref(power),
                                                         C.byref(k), index.ctypes.data_as(_lib.c_dp)))
        r = dict(voiced=bool(v.value), doa=doa.value, prob=prob.value, power=power.value, delay_idx=k.value, index=index)
        if self.callback is not None and r["voiced"]:
            self.callback(np.array([r["doa"]]), np.array([r["prob"]]), r["power"], 1)
        return r


def update_mask_from_decisions(decisions, center_freqs, fft_size):
    """The per-band decisions of the masking modules (FastBinauralMasking.process / BinauralMaskingImpl.process: int32 [...][45],
    0 = enhance, the band is kept as the target's; 1 = temporal mask, 2 = spatial mask, the band is attenuated) as the update_mask of
    MvdrBeamformer [...][K], K = fft_size/2 + 1: 0 where the band is enhanced (the covariance must not learn the target), 1 where it
    is masked.  center_freqs [45]: the band centres in cycles per sample, thresholds()[1] of the masking object; bin k, at
    k / fft_size cycles per sample, takes the band with the nearest centre -- the mel triangle that weighs most there."""
    dec = np.asarray(decisions)
    cen = np.asarray(center_freqs, dtype=np.float64)
    if dec.shape[-1:] != cen.shape or cen.ndim != 1 or np.any(np.diff(cen) <= 0):
        raise MCArrayHipError("decisions must be [...][B] and center_freqs [B], ascending")
    K = int(fft_size) // 2 + 1
    band_of = np.searchsorted(0.5 * (cen[:-1] + cen[1:]), np.arange(K) / float(fft_size), side="left")
    return np.ascontiguousarray((dec != 0)[..., band_of], dtype=np.float32)


class MvdrBeamformer(_StateBlob):
    _STATE = "mvdr"
    """Frequency-domain beamformer with a per-bin spatial covariance (BASELINE.json configs[3]; SURVEY A.9).
    No reference counterpart: the interface follows mca::Beamformer (Beamformer.h:39,49: frames in, one channel out,
    a look direction in radians) with the delay-and-sum weights replaced by MVDR weights.
    max_sources > 1 (up to 4) lets process_sources() separate that many look directions per frame from the one covariance;
    null_gain > 0 (up to 1000) makes every output of process_sources() steer a soft null at the other look directions of its
    frame (include/mcarray_hip.h, mca_hip_mvdr_set_null_gain; 0 is the plain MVDR output).
    configure_spectrum() / spectrum() read the Capon spatial spectrum of the held covariance and its peaks: the look directions
    of the next chunk (mca_hip_mvdr_spectrum_*).
    update= of the process calls: per-frame covariance update weights [streams][F] in [0, 1] (1: learn as usual, 0: leave the
    covariance as it is and beamform with it), e.g. 1 - voiced of a localiser for a noise-only covariance
    (mca_hip_mvdr_sources_frames_weighted_*; None: all 1).
    update_mask= instead: one weight per frame and bin, [streams][F][K] -- the mask of a mask estimator or an SNR rule: a bin
    that holds the target in a frame is left alone while the other bins of that frame learn
    (mca_hip_mvdr_sources_frames_masked_*).  update= and update_mask= are not combined: multiply them.
    set_postfilter() puts the decision-directed Wiener post-filter behind the solve of every process call: the noise-only MVDR
    becomes the multichannel Wiener filter (mca_hip_mvdr_set_postfilter).
    set_rtf() and target_mask= of the process calls: the steering vector of every look direction is estimated from a second
    covariance kept over the cells of its target mask [streams][S][F][K] -- the relative transfer function towards a reference
    microphone, which knows the microphones' gains and positions and the true direction where the geometric vector does not
    (mca_hip_mvdr_set_rtf, mca_hip_mvdr_sources_frames_rtf_*).  A call with target_mask= takes update_mask= beside it, not update=.
    set_mask_estimator() and estimate_masks=True of the process calls: both masks are formed on the device from the call's own
    spectra, by the steered coherence of every cell towards the call's look directions, and come back in the result
    (mca_hip_mvdr_set_mask_estimator, mca_hip_mvdr_sources_frames_auto_*).  Not together with a caller's update=, update_mask= or
    target_mask=.
    set_rtf_nulls() / rtf_nulls=True: the calls that steer by estimated vectors honour null_gain, with the nulls at the vectors the
    frame itself uses for the other look directions (mca_hip_mvdr_set_rtf_nulls); without it they refuse a non-zero null gain.
    set_geometry() / geometry="xyz": the steering vectors use all three coordinates of mic_positions, every look direction is an
    azimuth round the whole circle (0: +y, +pi/2: +x) at the context's one elevation, the spectrum's grid is periodic and the tracks
    live on the circle (mca_hip_mvdr_set_geometry).  The default "linear_x" reads the x coordinates alone, as it always did.
    map_configure() / map(): the Capon spectrum on a grid of azimuths x elevations and its peaks, for an array that can tell the
    elevation (geometry "xyz"; mca_hip_mvdr_map_*)."""

    GEOMETRY_LINEAR_X, GEOMETRY_XYZ = 0, 1

    K_ANALYSE, K_SOLVE, K_SYNTH, K_SPECTRUM, K_POSTFILTER, K_RTF, K_ESTMASK, K_TRACKS, K_MAP = 0, 1, 2, 3, 4, 5, 6, 7, 8
    K_TRACKS_MAP = 9

    def __init__(self, sample_rate, mic_positions, fft_size=1024, alpha=0.95, loading=1e-3, max_streams=1, device=0, max_sources=1,
                 geometry="linear_x", elevation_rad=0.0, null_gain=0.0, rtf_nulls=False):
        self._lib = _lib.load()
        xyz = _xyz(mic_positions)
        cfg = _lib.MvdrConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrConfig)
        cfg.device = device
        cfg.sample_rate = sample_rate
        cfg.fft_size = fft_size
        cfg.n_mics = len(xyz)
        cfg.mic_xyz = xyz.ctypes.data_as(_lib.c_dp)
        cfg.alpha = alpha
        cfg.loading = loading
        cfg.max_streams = max_streams
        h = C.c_void_p()
        rc = self._lib.mca_hip_mvdr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_mvdr_create failed (%d): %s" % (rc, self._lib.mca_hip_mvdr_last_error(None).decode()))
        self.h = h
        self.M, self.N, self.hop, self.K = len(xyz), fft_size, fft_size // 2, fft_size // 2 + 1
        self.max_sources = 1
        self.null_gain = 0.0
        self.max_streams = max_streams
        self.spectrum_config = None
        self.map_config = None
        self._follow, self._follow_doa = False, None
        try:
            if max_sources != 1:
                self.set_max_sources(max_sources)
            if null_gain != 0.0:
                self.set_null_gain(null_gain)
            if rtf_nulls:
                self.set_rtf_nulls(True)
            if geometry not in ("linear_x", self.GEOMETRY_LINEAR_X) or elevation_rad != 0.0:
                self.set_geometry(geometry, elevation_rad)
        except MCArrayHipError:
            self.close()
            raise

    def set_max_sources(self, max_sources):
        """look directions per frame process_sources() may carry (1 ... 4): one overlap-add tail per stream and source"""
        self._check(self._lib.mca_hip_mvdr_set_max_sources(self.h, int(max_sources)))
        self.max_sources = int(max_sources)

    def set_null_gain(self, null_gain):
        """gain of the soft nulls process_sources() steers at the other look directions (finite, 0 ... 1000; 0: plain MVDR).  A
        processing parameter: it may change between calls and is no part of the state blobs."""
        self._check(self._lib.mca_hip_mvdr_set_null_gain(self.h, float(null_gain)))
        self.null_gain = float(null_gain)

    def get_null_gain(self):
        g = C.c_double(0.0)
        self._check(self._lib.mca_hip_mvdr_get_null_gain(self.h, C.byref(g)))
        return g.value

    def set_rtf_nulls(self, enable=True):
        """let the calls with target_mask= or estimate_masks=True on an RTF context honour the null gain, at the estimated vectors
        (mca_hip_mvdr_set_rtf_nulls).  A processing parameter like the null gain; off by default, and then such a call refuses a
        non-zero null gain."""
        self._check(self._lib.mca_hip_mvdr_set_rtf_nulls(self.h, 1 if enable else 0))

    def get_rtf_nulls(self):
        e = C.c_int(0)
        self._check(self._lib.mca_hip_mvdr_get_rtf_nulls(self.h, C.byref(e)))
        return bool(e.value)

    def set_geometry(self, mode, elevation_rad=0.0):
        """the geometry of the steering vectors (include/mcarray_hip.h, mca_hip_mvdr_set_geometry): mode "linear_x" (x coordinates
        alone, the default) or "xyz" (all three, azimuths round the circle), elevation_rad in [-pi/2, pi/2] (ignored by "linear_x").
        A processing parameter; a call that changes it un-configures the spectrum and the map and disables the tracks: configure them anew."""
        kinds = {"linear_x": self.GEOMETRY_LINEAR_X, "xyz": self.GEOMETRY_XYZ}
        before = self.get_geometry()
        cfg = _lib.MvdrGeometryConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrGeometryConfig)
        cfg.mode = kinds[mode] if mode in kinds else int(mode)
        cfg.elevation_rad = float(elevation_rad)
        self._check(self._lib.mca_hip_mvdr_set_geometry(self.h, C.byref(cfg)))
        if self.get_geometry() != before:
            self.spectrum_config = None
            self.map_config = None
            self._follow, self._follow_doa = False, None

    def get_geometry(self):
        """dict(mode "linear_x" / "xyz", elevation_rad) as the context holds them"""
        cfg = _lib.MvdrGeometryConfig()
        self._check(self._lib.mca_hip_mvdr_get_geometry(self.h, C.byref(cfg)))
        return dict(mode="xyz" if cfg.mode == self.GEOMETRY_XYZ else "linear_x", elevation_rad=cfg.elevation_rad)

    def set_postfilter(self, enable=True, smoothing=0.98, gain_floor=0.1, noise_scale=1.0):
        """the decision-directed Wiener post-filter on the outputs of every process call (include/mcarray_hip.h,
        mca_hip_mvdr_set_postfilter): smoothing in [0, 1), gain_floor in [0, 1], noise_scale in (0, 100].  The three values are
        processing parameters; enabling starts the filter's state from zero, disabling frees it."""
        cfg = _lib.MvdrPostfilterConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrPostfilterConfig)
        cfg.enable = 1 if enable else 0
        cfg.smoothing = float(smoothing)
        cfg.gain_floor = float(gain_floor)
        cfg.noise_scale = float(noise_scale)
        self._check(self._lib.mca_hip_mvdr_set_postfilter(self.h, C.byref(cfg)))

    def get_postfilter(self):
        """dict(enable, smoothing, gain_floor, noise_scale) as the context holds them"""
        cfg = _lib.MvdrPostfilterConfig()
        self._check(self._lib.mca_hip_mvdr_get_postfilter(self.h, C.byref(cfg)))
        return dict(enable=bool(cfg.enable), smoothing=cfg.smoothing, gain_floor=cfg.gain_floor, noise_scale=cfg.noise_scale)

    def set_rtf(self, enable=True, target_alpha=None, iterations=2, ref_mic=0, min_share=0.05):
        """steering vectors estimated from a target covariance (include/mcarray_hip.h, mca_hip_mvdr_set_rtf): target_alpha in [0, 1)
        (None: the value the context holds, its alpha at first), iterations 1 ... 4, ref_mic 0 ... M - 1, min_share in [0, 1).  The
        four values are processing parameters; enabling allocates the target covariances (zero), disabling frees them."""
        cfg = _lib.MvdrRtfConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrRtfConfig)
        cfg.enable = 1 if enable else 0
        cfg.target_alpha = self.get_rtf()["target_alpha"] if target_alpha is None else float(target_alpha)
        cfg.iterations = int(iterations)
        cfg.ref_mic = int(ref_mic)
        cfg.min_share = float(min_share)
        self._check(self._lib.mca_hip_mvdr_set_rtf(self.h, C.byref(cfg)))

    def get_rtf(self):
        """dict(enable, target_alpha, iterations, ref_mic, min_share) as the context holds them"""
        cfg = _lib.MvdrRtfConfig()
        self._check(self._lib.mca_hip_mvdr_get_rtf(self.h, C.byref(cfg)))
        return dict(enable=bool(cfg.enable), target_alpha=cfg.target_alpha, iterations=cfg.iterations, ref_mic=cfg.ref_mic, min_share=cfg.min_share)

    def set_rtf_workspace(self, max_bytes):
        """cap of the steering plane a target_mask= call holds at a time (default 1 GiB): a call above it is cut along the frames
        internally, which changes no byte (mca_hip_mvdr_set_rtf_workspace)"""
        self._check(self._lib.mca_hip_mvdr_set_rtf_workspace(self.h, int(max_bytes)))

    def set_mask_estimator(self, enable=True, bin_lo=0, bin_hi=None, coherence_lo=0.0, coherence_hi=0.05, n_protected=0):
        """the mask estimator behind estimate_masks=True (include/mcarray_hip.h, mca_hip_mvdr_set_mask_estimator): the band of bins
        [bin_lo, bin_hi] (None: N/2) outside which the masks are the plain recursion's, the thresholds 0 <= coherence_lo <
        coherence_hi <= 1 between which the winner's steered coherence becomes its mask (a call with one look direction needs
        absolute ones such as 0.2 / 0.4), n_protected 0 ... 4 look directions that close the noise covariance where they win (0: all).
        Processing parameters; the estimator holds no state."""
        cfg = _lib.MvdrEstmaskConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrEstmaskConfig)
        cfg.enable = 1 if enable else 0
        cfg.bin_lo = int(bin_lo)
        cfg.bin_hi = self.N // 2 if bin_hi is None else int(bin_hi)
        cfg.coherence_lo = float(coherence_lo)
        cfg.coherence_hi = float(coherence_hi)
        cfg.n_protected = int(n_protected)
        self._check(self._lib.mca_hip_mvdr_set_mask_estimator(self.h, C.byref(cfg)))

    def get_mask_estimator(self):
        """dict(enable, bin_lo, bin_hi, coherence_lo, coherence_hi, n_protected) as the context holds them"""
        cfg = _lib.MvdrEstmaskConfig()
        self._check(self._lib.mca_hip_mvdr_get_mask_estimator(self.h, C.byref(cfg)))
        return dict(enable=bool(cfg.enable), bin_lo=cfg.bin_lo, bin_hi=cfg.bin_hi, coherence_lo=cfg.coherence_lo, coherence_hi=cfg.coherence_hi,
                    n_protected=cfg.n_protected)

    def target_covariance(self, stream_index=0, source=0):
        """(Psi complex [K][M][M], cpsi [K]) of one stream and slot"""
        out, norm = np.empty((self.K, self.M, self.M, 2)), np.empty(self.K)
        self._check(self._lib.mca_hip_mvdr_get_target_covariance(self.h, int(stream_index), int(source), out.ctypes.data_as(_lib.c_dp),
                                                                 norm.ctypes.data_as(_lib.c_dp)))
        return out[..., 0] + 1j * out[..., 1], norm

    def steering(self, doa_rad, stream_index=0, source=0):
        """the steering vectors a frame with look direction doa_rad would take from the held state -> (d complex [K][M], estimated
        bool [K]: the RTF, or the geometric vector where the estimate is refused)"""
        out, est = np.empty((self.K, self.M, 2)), np.empty(self.K, dtype=np.uint8)
        self._check(self._lib.mca_hip_mvdr_get_steering(self.h, int(stream_index), int(source), float(doa_rad), out.ctypes.data_as(_lib.c_dp),
                                                        est.ctypes.data_as(C.c_void_p)))
        return out[..., 0] + 1j * out[..., 1], est.astype(bool)

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_mvdr_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_mvdr_last_error(self.h).decode()))

    def reset(self):
        self._check(self._lib.mca_hip_mvdr_reset(self.h, None))

    def _update_host(self, update, A, F):
        """float32 [streams][F] from a scalar, [F] or [streams][F]"""
        try:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(update, dtype=np.float32), (A, F)))
        except ValueError:
            raise MCArrayHipError("update must broadcast to [streams][F]")

    def _update_dev(self, update, A, n_frames):
        if update.dim() != 2 or not update.is_contiguous() or update.shape[0] != A or update.shape[1] != n_frames or update.element_size() != 4:
            raise MCArrayHipError("update must be a contiguous float32 tensor [streams][F]")
        return _ptr(update)

    def _mask_host(self, update, update_mask, A, F):
        """float32 [streams][F][K] from anything that broadcasts to it"""
        if update is not None:
            raise MCArrayHipError("update and update_mask are not combined: pass their product as update_mask")
        try:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(update_mask, dtype=np.float32), (A, F, self.K)))
        except (ValueError, TypeError):
            raise MCArrayHipError("update_mask must broadcast to [streams][F][K]")

    def _mask_dev(self, update, update_mask, A, n_frames):
        if update is not None:
            raise MCArrayHipError("update and update_mask are not combined: pass their product as update_mask")
        m = update_mask
        if not getattr(m, "is_cuda", False):
            raise MCArrayHipError("update_mask must be a contiguous float32 tensor [streams][F][K] on the device")
        if m.dim() != 3 or not m.is_contiguous() or tuple(m.shape) != (A, n_frames, self.K) or m.element_size() != 4 or not m.is_floating_point():
            raise MCArrayHipError("update_mask must be a contiguous float32 tensor [streams][F][K]")
        return _ptr(m)

    def _tmask_host(self, update, target_mask, A, S, F):
        """float32 [streams][S][F][K] from anything that broadcasts to it"""
        if update is not None:
            raise MCArrayHipError("target_mask goes with update_mask, not with update")
        try:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(target_mask, dtype=np.float32), (A, S, F, self.K)))
        except (ValueError, TypeError):
            raise MCArrayHipError("target_mask must broadcast to [streams][S][F][K]")

    def _tmask_dev(self, update, target_mask, A, S, n_frames):
        if update is not None:
            raise MCArrayHipError("target_mask goes with update_mask, not with update")
        m = target_mask
        if not getattr(m, "is_cuda", False):
            raise MCArrayHipError("target_mask must be a contiguous float32 tensor [streams][S][F][K] on the device")
        if m.dim() != 4 or not m.is_contiguous() or tuple(m.shape) != (A, S, n_frames, self.K) or m.element_size() != 4 or not m.is_floating_point():
            raise MCArrayHipError("target_mask must be a contiguous float32 tensor [streams][S][F][K]")
        return _ptr(m)

    def _rtf_host(self, pcm, A, F, S, doa, update, update_mask, target_mask, po, ps):
        fp = _lib.c_fp
        tm = self._tmask_host(update, target_mask, A, S, F)
        upd = None if update_mask is None else self._mask_host(None, update_mask, A, F)
        self._check(self._lib.mca_hip_mvdr_sources_frames_rtf_host(self.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp),
                                                                   None if upd is None else upd.ctypes.data_as(fp), tm.ctypes.data_as(fp), po, ps))

    def _rtf_dev(self, p, sa, sc, A, n_frames, S, doa_rad, update, update_mask, target_mask, out_pcm, out_spec, stream):
        tm = self._tmask_dev(update, target_mask, A, S, n_frames)
        upd = None if update_mask is None else self._mask_dev(None, update_mask, A, n_frames)
        self._check(self._lib.mca_hip_mvdr_sources_frames_rtf_dev(self.h, p, sa, sc, A, n_frames, S, _ptr(doa_rad), upd, tm, _ptr(out_pcm),
                                                                  _ptr(out_spec), stream))

    @staticmethod
    def _auto_check(update, update_mask, target_mask):
        if update is not None or update_mask is not None or target_mask is not None:
            raise MCArrayHipError("estimate_masks forms the masks itself: not together with update, update_mask or target_mask")

    def _auto_host(self, pcm, A, F, S, doa, po, ps):
        """-> (update_mask [streams][F][K], target_mask [streams][S][F][K]) float32"""
        fp = _lib.c_fp
        um, tm = np.empty((A, F, self.K), dtype=np.float32), np.empty((A, S, F, self.K), dtype=np.float32)
        self._check(self._lib.mca_hip_mvdr_sources_frames_auto_host(self.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp),
                                                                    um.ctypes.data_as(fp), tm.ctypes.data_as(fp), po, ps))
        return um, tm

    def _auto_dev(self, p, sa, sc, A, n_frames, S, doa_rad, out_pcm, out_spec, stream, like, masks_out):
        """-> dict(update_mask [streams][F][K], target_mask [streams][S][F][K]) float32 tensors on the device of `like`: the pair
        masks_out = (update_mask, target_mask) of the caller, or new tensors.  New tensors come from torch's allocator on torch's
        CURRENT stream: a caller whose `stream` is another one passes masks_out (or orders the two streams), as for every other
        tensor of the call."""
        import torch
        if masks_out is not None:
            um, tm = masks_out
            for t, shape, name in ((um, (A, n_frames, self.K), "update_mask"), (tm, (A, S, n_frames, self.K), "target_mask")):
                if not getattr(t, "is_cuda", False) or tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32:
                    raise MCArrayHipError("masks_out: %s must be a contiguous float32 device tensor %s" % (name, list(shape)))
        else:
            um = torch.empty((A, n_frames, self.K), dtype=torch.float32, device=like.device)
            tm = torch.empty((A, S, n_frames, self.K), dtype=torch.float32, device=like.device)
        self._check(self._lib.mca_hip_mvdr_sources_frames_auto_dev(self.h, p, sa, sc, A, n_frames, S, _ptr(doa_rad), _ptr(um), _ptr(tm), _ptr(out_pcm),
                                                                   _ptr(out_spec), stream))
        return dict(update_mask=um, target_mask=tm)

    def process(self, pcm, doa_rad, want_audio=True, want_spec=False, update=None, update_mask=None, target_mask=None, estimate_masks=False):
        """pcm float32 [streams][M][(F+1)*hop], doa_rad [streams][F] (or a scalar), update None or [streams][F] covariance update
        weights, or update_mask None or [streams][F][K] weights per frame and bin -> dict(out [streams][F*hop], spec complex64
        [streams][F][K]).  target_mask [streams][1][F][K] (or what broadcasts to it): the call steers with the estimated vector
        (set_rtf(); mca_hip_mvdr_sources_frames_rtf_*).  estimate_masks: the masks are estimated from the spectra
        (set_mask_estimator(); mca_hip_mvdr_sources_frames_auto_*) and the result also carries update_mask [streams][F][K] and
        target_mask [streams][1][F][K]"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, M, L = pcm.shape
        F = L // self.hop - 1
        if M != self.M or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [streams][M][(F+1)*hop]")
        doa = np.ascontiguousarray(np.broadcast_to(np.asarray(doa_rad, dtype=np.float32), (A, F)))
        out = np.empty((A, F * self.hop), dtype=np.float32) if want_audio else None
        spec = np.empty((A, F, self.K), dtype=np.complex64) if want_spec else None
        fp = _lib.c_fp
        po, ps = out.ctypes.data_as(fp) if want_audio else None, spec.ctypes.data_as(fp) if want_spec else None
        if estimate_masks:
            self._auto_check(update, update_mask, target_mask)
            um, tm = self._auto_host(pcm, A, F, 1, doa, po, ps)
            return dict(out=out, spec=spec, update_mask=um, target_mask=tm)
        if target_mask is not None:
            self._rtf_host(pcm, A, F, 1, doa, update, update_mask, target_mask, po, ps)
        elif update_mask is not None:
            upd = self._mask_host(update, update_mask, A, F)
            self._check(self._lib.mca_hip_mvdr_sources_frames_masked_host(self.h, pcm.ctypes.data_as(fp), A, F, 1, doa.ctypes.data_as(fp),
                                                                          upd.ctypes.data_as(fp), po, ps))
        elif update is None:
            self._check(self._lib.mca_hip_mvdr_frames_host(self.h, pcm.ctypes.data_as(fp), A, F, doa.ctypes.data_as(fp), po, ps))
        else:
            upd = self._update_host(update, A, F)
            self._check(self._lib.mca_hip_mvdr_sources_frames_weighted_host(self.h, pcm.ctypes.data_as(fp), A, F, 1, doa.ctypes.data_as(fp),
                                                                            upd.ctypes.data_as(fp), po, ps))
        return dict(out=out, spec=spec)

    def process_dev(self, pcm, n_frames, doa_rad, out_pcm=None, out_spec=None, stream=None, update=None, update_mask=None, target_mask=None,
                    estimate_masks=False, masks_out=None):
        """device tensors (torch): pcm [streams][M][>= (F+1)*hop] float32 at any even strides (pcm_layout), doa_rad [streams][F]
        float32, out_pcm [streams][F*hop], out_spec [streams][F][K][2] (contiguous), update None or [streams][F] float32 covariance
        update weights (contiguous), or update_mask None or [streams][F][K] float32 (contiguous), target_mask None or
        [streams][1][F][K] float32 (contiguous; set_rtf()); asynchronous on `stream` (a raw hipStream_t or None).  estimate_masks
        (set_mask_estimator()): returns dict(update_mask [streams][F][K], target_mask [streams][1][F][K]), the tensors of masks_out =
        (update_mask, target_mask) or, without it, new device tensors allocated on torch's current stream."""
        A = pcm.shape[0]
        p, sa, sc = pcm_layout(pcm)
        if estimate_masks:
            self._auto_check(update, update_mask, target_mask)
            return self._auto_dev(p, sa, sc, A, n_frames, 1, doa_rad, out_pcm, out_spec, stream, pcm, masks_out)
        if target_mask is not None:
            self._rtf_dev(p, sa, sc, A, n_frames, 1, doa_rad, update, update_mask, target_mask, out_pcm, out_spec, stream)
        elif update_mask is not None:
            self._check(self._lib.mca_hip_mvdr_sources_frames_masked_dev(self.h, p, sa, sc, A, n_frames, 1, _ptr(doa_rad),
                                                                         self._mask_dev(update, update_mask, A, n_frames), _ptr(out_pcm), _ptr(out_spec), stream))
        elif update is None:
            self._check(self._lib.mca_hip_mvdr_frames_dev(self.h, p, sa, sc, A, n_frames, _ptr(doa_rad), _ptr(out_pcm), _ptr(out_spec), stream))
        else:
            self._check(self._lib.mca_hip_mvdr_sources_frames_weighted_dev(self.h, p, sa, sc, A, n_frames, 1, _ptr(doa_rad),
                                                                           self._update_dev(update, A, n_frames), _ptr(out_pcm), _ptr(out_spec), stream))

    def process_sources(self, pcm, doa_rad, want_audio=True, want_spec=True, update=None, update_mask=None, target_mask=None, estimate_masks=False):
        """S look directions per frame from one analysis, covariance recursion and factorisation: pcm float32
        [streams][M][(F+1)*hop], doa_rad [streams][F][S] (S <= max_sources; the layout of the localiser's "doa"), update None or
        [streams][F] covariance update weights (one per frame for all its directions), or update_mask None or [streams][F][K] ->
        dict(out [streams][S][F*hop], spec complex64 [streams][S][F][K]).  Output s is what process() gives with doa_rad[:, :, s].
        target_mask None or [streams][S][F][K]: the cells that hold the target of look direction s, from which its steering vector
        is estimated (set_rtf(); mca_hip_mvdr_sources_frames_rtf_*).  estimate_masks: both masks are estimated from the spectra
        (set_mask_estimator(); mca_hip_mvdr_sources_frames_auto_*) and the result also carries update_mask [streams][F][K] and
        target_mask [streams][S][F][K]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        A, M, L = pcm.shape
        F = L // self.hop - 1
        if M != self.M or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [streams][M][(F+1)*hop]")
        doa = np.asarray(doa_rad, dtype=np.float32)
        if doa.ndim != 3 or doa.shape[:2] != (A, F):
            raise MCArrayHipError("doa_rad must be [streams][F][S]")
        doa = np.ascontiguousarray(doa)
        S = doa.shape[2]
        out = np.empty((A, S, F * self.hop), dtype=np.float32) if want_audio else None
        spec = np.empty((A, S, F, self.K), dtype=np.complex64) if want_spec else None
        fp = _lib.c_fp
        po, ps = out.ctypes.data_as(fp) if want_audio else None, spec.ctypes.data_as(fp) if want_spec else None
        if estimate_masks:
            self._auto_check(update, update_mask, target_mask)
            um, tm = self._auto_host(pcm, A, F, S, doa, po, ps)
            return dict(out=out, spec=spec, update_mask=um, target_mask=tm)
        if target_mask is not None:
            self._rtf_host(pcm, A, F, S, doa, update, update_mask, target_mask, po, ps)
        elif update_mask is not None:
            upd = self._mask_host(update, update_mask, A, F)
            self._check(self._lib.mca_hip_mvdr_sources_frames_masked_host(self.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp),
                                                                          upd.ctypes.data_as(fp), po, ps))
        elif update is None:
            self._check(self._lib.mca_hip_mvdr_sources_frames_host(self.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp), po, ps))
        else:
            upd = self._update_host(update, A, F)
            self._check(self._lib.mca_hip_mvdr_sources_frames_weighted_host(self.h, pcm.ctypes.data_as(fp), A, F, S, doa.ctypes.data_as(fp),
                                                                            upd.ctypes.data_as(fp), po, ps))
        return dict(out=out, spec=spec)

    def process_sources_dev(self, pcm, n_frames, doa_rad, out_pcm=None, out_spec=None, stream=None, update=None, update_mask=None,
                            target_mask=None, estimate_masks=False, masks_out=None):
        """device tensors (torch): pcm [streams][M][>= (F+1)*hop] float32 at any even strides (pcm_layout), doa_rad [streams][F][S]
        float32 (e.g. the doa_rad tensor Context.process_frames_dev wrote, as it is), out_pcm [streams][S][F*hop], out_spec
        [streams][S][F][K][2] (contiguous), update None or [streams][F] float32 covariance update weights (contiguous), or
        update_mask None or [streams][F][K] float32 (contiguous), target_mask None or [streams][S][F][K] float32 (contiguous;
        set_rtf()); asynchronous on `stream` (a raw hipStream_t or None).  estimate_masks (set_mask_estimator()): returns
        dict(update_mask [streams][F][K], target_mask [streams][S][F][K]), the tensors of masks_out = (update_mask, target_mask) or,
        without it, new device tensors allocated on torch's current stream."""
        A = pcm.shape[0]
        p, sa, sc = pcm_layout(pcm)
        if doa_rad is None:
            doa_rad = self._tracks_doa(A, n_frames, pcm, stream)
        if doa_rad.dim() != 3 or not doa_rad.is_contiguous() or doa_rad.shape[0] != A or doa_rad.shape[1] != n_frames:
            raise MCArrayHipError("doa_rad must be a contiguous tensor [streams][F][S]")
        if estimate_masks:
            self._auto_check(update, update_mask, target_mask)
            return self._auto_dev(p, sa, sc, A, n_frames, doa_rad.shape[2], doa_rad, out_pcm, out_spec, stream, pcm, masks_out)
        if target_mask is not None:
            self._rtf_dev(p, sa, sc, A, n_frames, doa_rad.shape[2], doa_rad, update, update_mask, target_mask, out_pcm, out_spec, stream)
        elif update_mask is not None:
            self._check(self._lib.mca_hip_mvdr_sources_frames_masked_dev(self.h, p, sa, sc, A, n_frames, doa_rad.shape[2], _ptr(doa_rad),
                                                                         self._mask_dev(update, update_mask, A, n_frames), _ptr(out_pcm), _ptr(out_spec), stream))
        elif update is None:
            self._check(self._lib.mca_hip_mvdr_sources_frames_dev(self.h, p, sa, sc, A, n_frames, doa_rad.shape[2], _ptr(doa_rad), _ptr(out_pcm),
                                                                  _ptr(out_spec), stream))
        else:
            self._check(self._lib.mca_hip_mvdr_sources_frames_weighted_dev(self.h, p, sa, sc, A, n_frames, doa_rad.shape[2], _ptr(doa_rad),
                                                                           self._update_dev(update, A, n_frames), _ptr(out_pcm), _ptr(out_spec), stream))

    SPECTRUM_POWER, SPECTRUM_NORMALISED = 0, 1

    def configure_spectrum(self, n_angles, bin_lo=None, bin_hi=None, weighting="normalised", n_peaks=1):
        """the Capon spatial spectrum spectrum() evaluates on the covariance the context holds (include/mcarray_hip.h,
        mca_hip_mvdr_spectrum_configure): n_angles 2 ... 361 from -pi/2 to pi/2 (geometry "xyz": 3 ... 361 round the circle,
        theta_i = -pi + i 2 pi / n_angles), the band of bins [bin_lo, bin_hi] (default
        1 ... N/2 - 1), weighting "power" or "normalised", n_peaks 1 ... 4.  A processing parameter: it may change between calls
        and is no part of the state blobs."""
        kinds = {"power": self.SPECTRUM_POWER, "normalised": self.SPECTRUM_NORMALISED}
        cfg = _lib.MvdrSpectrumConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrSpectrumConfig)
        cfg.n_angles = int(n_angles)
        cfg.bin_lo = 1 if bin_lo is None else int(bin_lo)
        cfg.bin_hi = self.N // 2 - 1 if bin_hi is None else int(bin_hi)
        cfg.weighting = kinds[weighting] if weighting in kinds else int(weighting)
        cfg.n_peaks = int(n_peaks)
        self._check(self._lib.mca_hip_mvdr_spectrum_configure(self.h, C.byref(cfg)))
        self.spectrum_config = dict(n_angles=cfg.n_angles, bin_lo=cfg.bin_lo, bin_hi=cfg.bin_hi, weighting=cfg.weighting, n_peaks=cfg.n_peaks)

    def spectrum_grid(self):
        """float32 [D]: the angles of the spectrum's grid (radians), as peak_doa reports them"""
        if getattr(self, "spectrum_config", None) is None:
            raise MCArrayHipError("configure_spectrum() first")
        g = np.empty(self.spectrum_config["n_angles"], dtype=np.float32)
        self._check(self._lib.mca_hip_mvdr_spectrum_get_grid(self.h, g.ctypes.data_as(_lib.c_fp)))
        return g

    def spectrum(self, n_streams=None):
        """the spectrum of streams 0 ... n_streams - 1 (default: all) and its peaks -> dict(spectrum [A][D], peak_doa [A][P] radians,
        peak_val [A][P]), float32.  peak_doa is a valid doa_rad[:, t, :] of the next process_sources() call.  Reads the stream state,
        writes none of it."""
        cfgd = getattr(self, "spectrum_config", None)
        A = self.max_streams if n_streams is None else int(n_streams)
        D, P = (cfgd["n_angles"], cfgd["n_peaks"]) if cfgd else (1, 1)
        spec = np.empty((max(A, 0), D), dtype=np.float32)
        doa = np.empty((max(A, 0), P), dtype=np.float32)
        val = np.empty((max(A, 0), P), dtype=np.float32)
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_mvdr_spectrum_host(self.h, A, spec.ctypes.data_as(fp), doa.ctypes.data_as(fp), val.ctypes.data_as(fp)))
        return dict(spectrum=spec, peak_doa=doa, peak_val=val)

    def spectrum_dev(self, n_streams, spectrum=None, peak_doa=None, peak_val=None, stream=None):
        """device tensors (torch, contiguous float32): spectrum [A][D], peak_doa / peak_val [A][n_peaks]; any may be None, not all;
        asynchronous on `stream` (a raw hipStream_t or None)"""
        self._check(self._lib.mca_hip_mvdr_spectrum_dev(
            self.h, int(n_streams), spectrum.data_ptr() if spectrum is not None else None, peak_doa.data_ptr() if peak_doa is not None else None,
            peak_val.data_ptr() if peak_val is not None else None, stream))

    def map_configure(self, n_az, n_el=1, el_lo_rad=None, el_hi_rad=None, bin_lo=None, bin_hi=None, weighting="normalised", n_peaks=1):
        """the azimuth x elevation Capon map map() evaluates on the covariance the context holds (include/mcarray_hip.h,
        mca_hip_mvdr_map_configure; geometry "xyz" only): n_az 3 ... 360 azimuths round the circle, n_el 1 ... 91 elevations from
        el_lo_rad to el_hi_rad (default: both the context's elevation; n_el == 1 needs them equal), n_az n_el <= 2048, the band,
        weighting and n_peaks as configure_spectrum().  A processing parameter, no part of the state blobs."""
        kinds = {"power": self.SPECTRUM_POWER, "normalised": self.SPECTRUM_NORMALISED}
        eps = self.get_geometry()["elevation_rad"]
        cfg = _lib.MvdrMapConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrMapConfig)
        cfg.n_az, cfg.n_el = int(n_az), int(n_el)
        cfg.el_lo_rad = eps if el_lo_rad is None else float(el_lo_rad)
        cfg.el_hi_rad = cfg.el_lo_rad if el_hi_rad is None else float(el_hi_rad)
        cfg.bin_lo = 1 if bin_lo is None else int(bin_lo)
        cfg.bin_hi = self.N // 2 - 1 if bin_hi is None else int(bin_hi)
        cfg.weighting = kinds[weighting] if weighting in kinds else int(weighting)
        cfg.n_peaks = int(n_peaks)
        self._check(self._lib.mca_hip_mvdr_map_configure(self.h, C.byref(cfg)))
        self.map_config = dict(n_az=cfg.n_az, n_el=cfg.n_el, el_lo_rad=cfg.el_lo_rad, el_hi_rad=cfg.el_hi_rad, bin_lo=cfg.bin_lo,
                               bin_hi=cfg.bin_hi, weighting=cfg.weighting, n_peaks=cfg.n_peaks)

    def map_grid(self):
        """(az float32 [n_az], el float32 [n_el]): the angles of the map's grid (radians), as peak_az and peak_el report them"""
        if getattr(self, "map_config", None) is None:
            raise MCArrayHipError("map_configure() first")
        az = np.empty(self.map_config["n_az"], dtype=np.float32)
        el = np.empty(self.map_config["n_el"], dtype=np.float32)
        self._check(self._lib.mca_hip_mvdr_map_get_grid(self.h, az.ctypes.data_as(_lib.c_fp), el.ctypes.data_as(_lib.c_fp)))
        return az, el

    def map(self, n_streams=None):
        """the map of streams 0 ... n_streams - 1 (default: all) and its peaks -> dict(map [A][n_el][n_az], peak_az / peak_el [A][P]
        radians, peak_val [A][P]), float32.  peak_az is a valid doa_rad[:, t, :] of the next process_sources() call.  Reads the
        stream state, writes none of it."""
        cfgd = getattr(self, "map_config", None)
        A = self.max_streams if n_streams is None else int(n_streams)
        n_el, n_az, P = (cfgd["n_el"], cfgd["n_az"], cfgd["n_peaks"]) if cfgd else (1, 1, 1)
        m = np.empty((max(A, 0), n_el, n_az), dtype=np.float32)
        az, el, val = (np.empty((max(A, 0), P), dtype=np.float32) for _ in range(3))
        fp = _lib.c_fp
        self._check(self._lib.mca_hip_mvdr_map_host(self.h, A, m.ctypes.data_as(fp), az.ctypes.data_as(fp), el.ctypes.data_as(fp), val.ctypes.data_as(fp)))
        return dict(map=m, peak_az=az, peak_el=el, peak_val=val)

    def map_dev(self, n_streams, map=None, peak_az=None, peak_el=None, peak_val=None, stream=None):
        """device tensors (torch, contiguous float32): map [A][n_el][n_az], peak_az / peak_el / peak_val [A][n_peaks]; any may be
        None, not all; asynchronous on `stream` (a raw hipStream_t or None)"""
        self._check(self._lib.mca_hip_mvdr_map_dev(self.h, int(n_streams), *[t.data_ptr() if t is not None else None for t in (map, peak_az, peak_el, peak_val)],
                                                   stream))

    def set_elevations(self, elev_rad):
        """an elevation per stream and look-direction slot, [streams][max_sources] (or [max_sources] for one stream), radians within
        +-pi/2; NaN: the context's elevation, the state after construction (include/mcarray_hip.h, mca_hip_mvdr_set_elevations_host).
        Geometry "xyz": the process calls steer look direction s of stream a at its own elevation.  A processing parameter, kept
        across reset(); a geometry change and configure_tracks() reset it to unset, and setting it disables the tracks."""
        e = np.ascontiguousarray(np.atleast_2d(np.asarray(elev_rad, dtype=np.float32)))
        if e.ndim != 2 or e.shape[1] != self.max_sources:
            raise MCArrayHipError("elev_rad must be [streams][max_sources]")
        self._check(self._lib.mca_hip_mvdr_set_elevations_host(self.h, e.shape[0], e.ctypes.data_as(_lib.c_fp)))
        self._follow, self._follow_doa = False, None

    def set_elevations_dev(self, n_streams, elev_rad, stream=None):
        """device tensor (torch, contiguous float32) [n_streams][max_sources] -- the peak_el of map_dev() for instance; values outside
        +-pi/2 are clamped; asynchronous on `stream`"""
        self._check(self._lib.mca_hip_mvdr_set_elevations_dev(self.h, int(n_streams), elev_rad.data_ptr(), stream))
        self._follow, self._follow_doa = False, None

    def get_elevations(self, n_streams=None):
        """float32 [streams][max_sources]: NaN for a slot at the context's elevation"""
        A = self.max_streams if n_streams is None else int(n_streams)
        e = np.empty((max(A, 0), self.max_sources), dtype=np.float32)
        self._check(self._lib.mca_hip_mvdr_get_elevations(self.h, A, e.ctypes.data_as(_lib.c_fp)))
        return e

    def configure_tracks(self, n_tracks, n_own=0, max_step_rad=0.2, min_sep_rad=0.1, hold=3, enable=True):
        """tracks of the look directions, kept on the device between chunks (include/mcarray_hip.h, mca_hip_mvdr_tracks_configure):
        n_tracks 1 ... max_sources slots per stream, of which the first n_own follow their own target covariance (set_rtf() first)
        and the others the Capon peaks (configure_spectrum() first: its grid, band and n_peaks), max_step_rad in (0, pi] the
        association gate and search window, min_sep_rad in [0, pi] within which a peak is an own talker, hold 0 ... 1000 updates an
        unmatched track keeps its direction.  Clears the tracks."""
        cfg = _lib.MvdrTracksConfig()
        cfg.struct_size = C.sizeof(_lib.MvdrTracksConfig)
        cfg.enable = 1 if enable else 0
        cfg.n_tracks = int(n_tracks)
        cfg.n_own = int(n_own)
        cfg.max_step_rad = float(max_step_rad)
        cfg.min_sep_rad = float(min_sep_rad)
        cfg.hold = int(hold)
        self._check(self._lib.mca_hip_mvdr_tracks_configure(self.h, C.byref(cfg)))

    def get_tracks_config(self):
        """dict(enable, n_tracks, n_own, max_step_rad, min_sep_rad, hold) as the context holds them"""
        cfg = _lib.MvdrTracksConfig()
        self._check(self._lib.mca_hip_mvdr_tracks_get_config(self.h, C.byref(cfg)))
        return dict(enable=bool(cfg.enable), n_tracks=cfg.n_tracks, n_own=cfg.n_own, max_step_rad=cfg.max_step_rad, min_sep_rad=cfg.min_sep_rad,
                    hold=cfg.hold)

    def seed_tracks(self, doa_rad):
        """doa_rad [streams][n_tracks] (or [n_tracks] for one stream): a finite value starts a track in that slot, a NaN leaves it"""
        d = np.ascontiguousarray(np.atleast_2d(np.asarray(doa_rad, dtype=np.float32)))
        self._check(self._lib.mca_hip_mvdr_tracks_seed_host(self.h, d.shape[0], d.ctypes.data_as(_lib.c_fp)))

    def update_tracks(self, n_streams=None, want_spectrum=False):
        """one update of the tracks of streams 0 ... n_streams - 1 (default: all) from the state the context holds.  want_spectrum:
        -> dict(own_spectrum float32 [A][n_own][D], own_used bool [A][n_own][K])"""
        A = self.max_streams if n_streams is None else int(n_streams)
        if not want_spectrum:
            self._check(self._lib.mca_hip_mvdr_tracks_update_host(self.h, A, None, None))
            return None
        n_own, D = self.get_tracks_config()["n_own"], (self.spectrum_config or {}).get("n_angles", 1)
        spec = np.zeros((max(A, 0), n_own, D), dtype=np.float32)
        used = np.zeros((max(A, 0), n_own, self.K), dtype=np.uint8)
        self._check(self._lib.mca_hip_mvdr_tracks_update_host(self.h, A, spec.ctypes.data_as(_lib.c_fp), used.ctypes.data_as(C.c_void_p)))
        return dict(own_spectrum=spec, own_used=used.astype(bool))

    def update_tracks_dev(self, n_streams, own_spectrum=None, own_used=None, stream=None):
        """device tensors (torch, contiguous): own_spectrum float32 [A][n_own][D], own_used uint8 [A][n_own][K]; either may be None;
        asynchronous on `stream` (a raw hipStream_t or None)"""
        self._check(self._lib.mca_hip_mvdr_tracks_update_dev(self.h, int(n_streams), own_spectrum.data_ptr() if own_spectrum is not None else None,
                                                             own_used.data_ptr() if own_used is not None else None, stream))

    def associate_tracks_dev(self, n_streams, own_doa, cand_doa, cand_val, stream=None):
        """the association alone on candidates of the caller's (device tensors, contiguous float32): own_doa [A][n_own] or None,
        cand_doa / cand_val [A][n_cand], n_cand 1 ... 8"""
        self._check(self._lib.mca_hip_mvdr_tracks_associate_dev(self.h, int(n_streams), own_doa.data_ptr() if own_doa is not None else None,
                                                                int(cand_doa.shape[-1]), cand_doa.data_ptr(), cand_val.data_ptr(), stream))

    def seed_tracks_dev(self, n_streams, doa_rad, stream=None):
        self._check(self._lib.mca_hip_mvdr_tracks_seed_dev(self.h, int(n_streams), doa_rad.data_ptr(), stream))

    def fill_tracks_dev(self, n_streams, n_frames, doa_rad, stream=None):
        """writes doa_rad [A][n_frames][n_tracks] (device tensor, contiguous float32) of the next process_sources_dev() call"""
        self._check(self._lib.mca_hip_mvdr_tracks_fill_dev(self.h, int(n_streams), int(n_frames), doa_rad.data_ptr(), stream))

    def tracks(self, n_streams=None):
        """-> dict(theta float32, alive, miss, gen int32), each [A][n_tracks]; synchronises the device"""
        A = self.max_streams if n_streams is None else int(n_streams)
        T = self.get_tracks_config()["n_tracks"]
        th = np.zeros((max(A, 0), T), dtype=np.float32)
        al, mi, ge = (np.zeros((max(A, 0), T), dtype=np.int32) for _ in range(3))
        ip = _lib.c_ip
        self._check(self._lib.mca_hip_mvdr_tracks_get(self.h, A, th.ctypes.data_as(_lib.c_fp), al.ctypes.data_as(ip), mi.ctypes.data_as(ip),
                                                      ge.ctypes.data_as(ip)))
        return dict(theta=th, alive=al, miss=mi, gen=ge)

    # ---- the tracks' map mode: azimuth and elevation, fed by the Capon map (include/mcarray_hip.h, mca_hip_mvdr_tracks_set_map) ----
    def configure_tracks_map(self, max_step_el_rad, min_sep_el_rad, enable=True):
        """map mode of the tracks (geometry "xyz"; configure_tracks() and map_configure() first): every slot holds (theta, eps), the own
        tracks search a patch of the map within (max_step_rad, max_step_el_rad) and the others follow the map's peaks, associated in
        both angles; a peak inside the box (min_sep_rad, min_sep_el_rad) of an own track is that talker.  Clears the tracks."""
        cfg = _lib.MvdrTracksMapConfig(C.sizeof(_lib.MvdrTracksMapConfig), 1 if enable else 0, float(max_step_el_rad), float(min_sep_el_rad))
        self._check(self._lib.mca_hip_mvdr_tracks_set_map(self.h, C.byref(cfg)))

    def get_tracks_map_config(self):
        """dict(enable, max_step_el_rad, min_sep_el_rad) as the context holds them"""
        cfg = _lib.MvdrTracksMapConfig()
        self._check(self._lib.mca_hip_mvdr_tracks_get_map_config(self.h, C.byref(cfg)))
        return dict(enable=bool(cfg.enable), max_step_el_rad=cfg.max_step_el_rad, min_sep_el_rad=cfg.min_sep_el_rad)

    def seed_tracks_map(self, az_rad, el_rad):
        """az_rad, el_rad [streams][n_tracks] (or [n_tracks] for one stream): a finite pair starts a track in that slot, anything else
        leaves it"""
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(az_rad, dtype=np.float32)))
        e = np.ascontiguousarray(np.atleast_2d(np.asarray(el_rad, dtype=np.float32)))
        if a.shape != e.shape:
            raise MCArrayHipError("az_rad and el_rad must have the same shape")
        self._check(self._lib.mca_hip_mvdr_tracks_seed_map_host(self.h, a.shape[0], a.ctypes.data_as(_lib.c_fp), e.ctypes.data_as(_lib.c_fp)))

    def seed_tracks_map_dev(self, n_streams, az_rad, el_rad, stream=None):
        self._check(self._lib.mca_hip_mvdr_tracks_seed_map_dev(self.h, int(n_streams), az_rad.data_ptr(), el_rad.data_ptr(), stream))

    def update_tracks_map(self, n_streams=None, want_map=False):
        """one update of the tracks of streams 0 ... n_streams - 1 (default: all) in map mode.  want_map: -> dict(own_map float32
        [A][n_own][n_el][n_az], own_used bool [A][n_own][K]); without it only the cells of the search windows are evaluated"""
        A = self.max_streams if n_streams is None else int(n_streams)
        if not want_map:
            self._check(self._lib.mca_hip_mvdr_tracks_update_map_host(self.h, A, None, None))
            return None
        cfgd = getattr(self, "map_config", None) or {}
        n_own = self.get_tracks_config()["n_own"]
        m = np.zeros((max(A, 0), n_own, cfgd.get("n_el", 1), cfgd.get("n_az", 1)), dtype=np.float32)
        used = np.zeros((max(A, 0), n_own, self.K), dtype=np.uint8)
        self._check(self._lib.mca_hip_mvdr_tracks_update_map_host(self.h, A, m.ctypes.data_as(_lib.c_fp), used.ctypes.data_as(C.c_void_p)))
        return dict(own_map=m, own_used=used.astype(bool))

    def update_tracks_map_dev(self, n_streams, own_map=None, own_used=None, stream=None):
        """device tensors (torch, contiguous): own_map float32 [A][n_own][n_el][n_az], own_used uint8 [A][n_own][K]; either may be
        None; asynchronous on `stream` (a raw hipStream_t or None)"""
        self._check(self._lib.mca_hip_mvdr_tracks_update_map_dev(self.h, int(n_streams), own_map.data_ptr() if own_map is not None else None,
                                                                 own_used.data_ptr() if own_used is not None else None, stream))

    def associate_tracks_map_dev(self, n_streams, own_az, own_el, cand_az, cand_el, cand_val, stream=None):
        """the association alone on candidates of the caller's (device tensors, contiguous float32): own_az / own_el [A][n_own] or
        None, cand_az / cand_el / cand_val [A][n_cand], n_cand 1 ... 8"""
        self._check(self._lib.mca_hip_mvdr_tracks_associate_map_dev(self.h, int(n_streams), own_az.data_ptr() if own_az is not None else None,
                                                                    own_el.data_ptr() if own_el is not None else None, int(cand_az.shape[-1]),
                                                                    cand_az.data_ptr(), cand_el.data_ptr(), cand_val.data_ptr(), stream))

    def tracks_map(self, n_streams=None):
        """-> dict(theta, eps float32, alive, miss, gen int32), each [A][n_tracks]; synchronises the device"""
        A = self.max_streams if n_streams is None else int(n_streams)
        T = self.get_tracks_config()["n_tracks"]
        th, ep = (np.zeros((max(A, 0), T), dtype=np.float32) for _ in range(2))
        al, mi, ge = (np.zeros((max(A, 0), T), dtype=np.int32) for _ in range(3))
        ip, fp = _lib.c_ip, _lib.c_fp
        self._check(self._lib.mca_hip_mvdr_tracks_get_map(self.h, A, th.ctypes.data_as(fp), ep.ctypes.data_as(fp), al.ctypes.data_as(ip), mi.ctypes.data_as(ip),
                                                          ge.ctypes.data_as(ip)))
        return dict(theta=th, eps=ep, alive=al, miss=mi, gen=ge)

    def follow_tracks(self, enable=True):
        """while on, process_sources_dev(..., doa_rad=None) takes its look directions from the tracks: fill_tracks_dev() into a
        tensor of the context's, on the call's stream, with no host step.  In map mode the fill carries the slots' elevations too"""
        self._follow = bool(enable)
        if not enable:
            self._follow_doa = None

    def _tracks_doa(self, A, n_frames, like, stream):
        import torch
        if not getattr(self, "_follow", False):
            raise MCArrayHipError("doa_rad is None: follow_tracks(True) first")
        T = self.get_tracks_config()["n_tracks"]
        d = getattr(self, "_follow_doa", None)
        if d is None or tuple(d.shape) != (A, n_frames, T) or d.device != like.device:
            d = self._follow_doa = torch.empty((A, n_frames, T), dtype=torch.float32, device=like.device)
        self.fill_tracks_dev(A, n_frames, d, stream)
        return d

    def covariance(self, stream_index=0):
        out = np.empty((self.K, self.M, self.M, 2))
        self._check(self._lib.mca_hip_mvdr_get_covariance(self.h, stream_index, out.ctypes.data_as(_lib.c_dp)))
        return out[..., 0] + 1j * out[..., 1]

    def set_timing(self, enable):
        self._check(self._lib.mca_hip_mvdr_set_timing(self.h, int(enable)))

    def repair_stats(self):
        """SRP_ADAPTIVE: dict(frames, flagged, recomputed) since the last reset_timing()"""
        a, b, c_ = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.mca_hip_get_repair_stats(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        return {"frames": a.value, "flagged": b.value, "recomputed": c_.value}

    def get_timing(self, kernel_id):
        n, ms = C.c_int(0), C.c_double(0)
        self._check(self._lib.mca_hip_mvdr_get_timing(self.h, kernel_id, C.byref(n), C.byref(ms)))
        return n.value, ms.value


FACTOR, RELATIVE, FULL, NOISY, NOTHING = 0, 1, 3, 4, 5      # BinauralMasking::MaskingMethod (ArrayModules.h:81)
BOTH, SPATIAL, TEMPORAL = 0, 1, 2                           # BinauralMasking::MaskingAlg (ArrayModules.h:89)


class FastBinauralMasking(_StateBlob):
    _STATE = "mask"
    """mca::FastBinauralMasking(int samplerate, double microDistance, float lowFreq, float highFreq,
    MaskingMethod = RELATIVE, MaskingAlg = BOTH) (FastBinauralMasking.h:71-76)."""

    def __init__(self, samplerate, micro_distance, low_freq, high_freq, method=RELATIVE, algorithm=BOTH, fft_size=1024,
                 max_streams=1, device=0):
        self._lib = _lib.load()
        cfg = _lib.MaskConfig()
        cfg.struct_size = C.sizeof(_lib.MaskConfig)
        cfg.device = device
        cfg.sample_rate = samplerate
        cfg.fft_size = fft_size
        cfg.micro_distance = micro_distance
        cfg.low_freq = low_freq
        cfg.high_freq = high_freq
        cfg.method = method
        cfg.algorithm = algorithm
        cfg.max_streams = max_streams
        h = C.c_void_p()
        rc = self._lib.mca_hip_mask_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_mask_create failed (%d): %s" % (rc, self._lib.mca_hip_mask_last_error(None).decode()))
        self.h = h
        self.N = fft_size
        self.hop = fft_size // 2

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_mask_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_mask_last_error(self.h).decode()))

    def reset(self):
        self._check(self._lib.mca_hip_mask_reset(self.h))

    def thresholds(self):
        thr = np.empty(45)
        cen = np.empty(45)
        self._check(self._lib.mca_hip_mask_get_thresholds(self.h, thr.ctypes.data_as(_lib.c_dp), cen.ctypes.data_as(_lib.c_dp)))
        return thr, cen

    def process(self, pcm, want_decisions=True):
        """pcm float32 [streams][2][(F+1)*hop] -> (out [streams][2][F*hop], decisions [streams][F][45])"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        ns, ch, L = pcm.shape
        F = L // self.hop - 1
        if ch != 2 or F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [streams][2][(F+1)*hop]")
        out = np.empty((ns, 2, F * self.hop), dtype=np.float32)
        dec = np.empty((ns, F, 45), dtype=np.int32) if want_decisions else None
        self._check(self._lib.mca_hip_mask_frames_host(self.h, pcm.ctypes.data_as(_lib.c_fp), ns, F, out.ctypes.data_as(_lib.c_fp),
                                                       dec.ctypes.data_as(_lib.c_ip) if want_decisions else None))
        return out, dec

    def process_dev(self, pcm, n_frames, out_pcm, decisions=None, stream=None):
        """device tensors (torch): pcm [streams][2][>= (F+1)*hop] float32 at any even strides (pcm_layout), out_pcm
        [streams][2][F*hop] float32, decisions [streams][F][45] int32 or None (contiguous, preallocated); asynchronous on `stream`
        (a raw hipStream_t or None)."""
        ns, ch, L = pcm.shape
        if ch != 2:
            raise MCArrayHipError("pcm must be [streams][2][L]")
        p, sa, sc = pcm_layout(pcm)
        self._check(self._lib.mca_hip_mask_frames_dev(self.h, p, sa, sc, ns, int(n_frames), _ptr(out_pcm), _ptr(decisions), stream))

    def process_parametrisation(self, left, right):
        """The DSPONE hook for one frame: CCS double[N+2] spectra, returns the modified copies + decisions."""
        left = np.array(left, dtype=np.float64, order="C")
        right = np.array(right, dtype=np.float64, order="C")
        dec = np.zeros(45, dtype=np.int32)
        self._check(self._lib.mca_hip_mask_process_frame(self.h, left.ctypes.data_as(_lib.c_dp), right.ctypes.data_as(_lib.c_dp),
                                                         len(left), dec.ctypes.data_as(_lib.c_ip)))
        return left, right, dec


class BinauralMaskingImpl(_StateBlob):
    _STATE = "bmask"
    """mca::BinauralMaskingImpl(int samplerate, double microDistance, float lowFreq, float highFreq, MaskingMethod = RELATIVE)
    (BinauralMaskingImpl.h:78-82): the filter-bank (time-domain) formulation of the binaural masking.  The frame length is the
    module's own, W = 2^calculateOrderFromSampleRate(fs, 0.050), the hop W/2.  Methods: FACTOR, RELATIVE, FULL."""
    N_BANDS = 45

    def __init__(self, samplerate, micro_distance, low_freq, high_freq, method=RELATIVE, max_streams=1, device=0):
        self._lib = _lib.load()
        self.W = 1 << calculate_order_from_sample_rate(samplerate, float(np.float32(0.050)))
        self.hop = self.W // 2
        cfg = _lib.BmaskConfig()
        cfg.struct_size = C.sizeof(_lib.BmaskConfig)
        cfg.device = device
        cfg.sample_rate = samplerate
        cfg.frame_size = self.W
        cfg.micro_distance = micro_distance
        cfg.low_freq = low_freq
        cfg.high_freq = high_freq
        cfg.method = method
        cfg.max_streams = max_streams
        h = C.c_void_p()
        rc = self._lib.mca_hip_bmask_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MCArrayHipError("mca_hip_bmask_create failed (%d): %s" % (rc, self._lib.mca_hip_bmask_last_error(None).decode()))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._lib.mca_hip_bmask_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MCArrayHipError("libmcarray_hip error %d: %s" % (rc, self._lib.mca_hip_bmask_last_error(self.h).decode()))

    def reset(self):
        self._check(self._lib.mca_hip_bmask_reset(self.h))

    def thresholds(self):
        thr = np.empty(45)
        cen = np.empty(45)
        self._check(self._lib.mca_hip_bmask_get_thresholds(self.h, thr.ctypes.data_as(_lib.c_dp), cen.ctypes.data_as(_lib.c_dp)))
        return thr, cen

    def process(self, pcm, want_decisions=True):
        """pcm float32 [streams][2][(F+1)*hop] -> (out [streams][2][F*hop], decisions [streams][F][45])"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 2:
            pcm = pcm[None]
        ns, ch, L = pcm.shape
        F = L // self.hop - 1
        if ch != 2:
            raise MCArrayHipError("Sound localisation is only working for 2 channels by now.")
        if F < 1 or (F + 1) * self.hop != L:
            raise MCArrayHipError("pcm must be [streams][2][(F+1)*hop]")
        out = np.empty((ns, 2, F * self.hop), dtype=np.float32)
        dec = np.empty((ns, F, 45), dtype=np.int32) if want_decisions else None
        self._check(self._lib.mca_hip_bmask_frames_host(self.h, pcm.ctypes.data_as(_lib.c_fp), ns, F, out.ctypes.data_as(_lib.c_fp),
                                                        dec.ctypes.data_as(_lib.c_ip) if want_decisions else None))
        return out, dec

    def process_dev(self, pcm, n_frames, out_pcm, decisions=None, stream=None):
        """device tensors (torch): pcm [streams][2][>= (F+1)*hop] float32 at any even strides (pcm_layout), out_pcm
        [streams][2][F*hop] float32, decisions [streams][F][45] int32 or None (contiguous, preallocated); asynchronous on `stream`
        (a raw hipStream_t or None)."""
        ns, ch, L = pcm.shape
        if ch != 2:
            raise MCArrayHipError("pcm must be [streams][2][L]")
        p, sa, sc = pcm_layout(pcm)
        self._check(self._lib.mca_hip_bmask_frames_dev(self.h, p, sa, sc, ns, int(n_frames), _ptr(out_pcm), _ptr(decisions), stream))

    state = _StateBlob.state_save
    load_state = _StateBlob.state_load

    def frame_analysis(self, frame, analysis_length=None, channel=0):
        """frameAnalysis: one windowed frame double[W] -> the analysis buffer double[analysis_length] (default 46 W): band b at
        b*W for every band that fits, the residual in slot 45 when there is room; what is not written stays zero."""
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        n = 46 * self.W if analysis_length is None else int(analysis_length)
        ana = np.zeros(n)
        self._check(self._lib.mca_hip_bmask_frame_analysis(self.h, frame.ctypes.data_as(_lib.c_dp), ana.ctypes.data_as(_lib.c_dp),
                                                           len(frame), n, channel))
        return ana

    def process_parametrisation(self, left, right):
        """The hook for one frame: two analysis buffers (>= 45 W doubles), returns the modified copies + decisions."""
        left = np.array(left, dtype=np.float64, order="C")
        right = np.array(right, dtype=np.float64, order="C")
        if len(left) != len(right):
            raise MCArrayHipError("left and right analysis buffers differ in length")
        dec = np.zeros(45, dtype=np.int32)
        self._check(self._lib.mca_hip_bmask_process_frame(self.h, left.ctypes.data_as(_lib.c_dp), right.ctypes.data_as(_lib.c_dp),
                                                          len(left), dec.ctypes.data_as(_lib.c_ip)))
        return left, right, dec

    def frame_synthesis(self, analysis, analysis_length=None, channel=0):
        """frameSynthesis: the sum of the band slots the reference's loop reads for this analysis_length -> double[W]."""
        analysis = np.ascontiguousarray(analysis, dtype=np.float64)
        n = len(analysis) if analysis_length is None else int(analysis_length)
        if n > len(analysis):
            raise MCArrayHipError("analysis_length exceeds the buffer")
        out = np.empty(self.W)
        self._check(self._lib.mca_hip_bmask_frame_synthesis(self.h, out.ctypes.data_as(_lib.c_dp), analysis.ctypes.data_as(_lib.c_dp),
                                                            self.W, n, channel))
        return out

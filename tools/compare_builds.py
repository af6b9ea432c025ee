"""Bytes of the main context's and the four module contexts' calls of this build against an older build of the library (the
yardstick of a refactor of their host layer).
usage: python tools/compare_builds.py PARENT_LIB

The frame is tools/compare_mvdr_builds.py's: the same inputs go through PARENT_LIB and through mcarray_amd/libmcarray_hip.so, each in
a fresh child process (MCA_HIP_LIB names the library) under a time limit of its own; the second child is not started when the first
one fails; a child leaves one SHA-256 per case over everything the case returns, the state blob included; this process requires
equal digests (exit code 1 otherwise) and never opens the GPU itself.

Cases (2 arrays of max_arrays = 3, calls of 64, 160 and 64 frames unless said otherwise; MCA_HIP_ADAPT_MIN_ROWS = 64, adaptive_fallback
OFF and candidate columns on, so the small batches run coarse + repair whatever the reports say):
  device-pointer stream calls in the four precisions: 8-microphone ULA, the same with the power gate, 16-microphone ULA, 4 microphones;
  fft_size 512 and 2048 at 4 and 8 microphones; two sources on a non-uniform array;
  2 microphones at fft_size 1024, 2048 and 4096, and 3 microphones at 256 and 4096 (the any-length kernels), FP32 and FP16;
  FP16 and ADAPTIVE: 16 microphones with 2 and 3 sources, 5 microphones with 1 and 2, a 5-degree grid (Dp = 64), a 0.4-degree grid (D - 2 > 384);
  the host-pointer entry points: pageable, page-locked (the chunked path), 16-bit PCM, and under MCA_HIP_WS_MAX_MB = 1 (the sliced path);
  a graph: 4 launches, an eager call that grows the workspace, 2 more launches;
  the gated 2-microphone path with a tracker (the larger call takes no rows / argmaxes), its frame hook, setProbability;
  the double frame API; the multiband, temporal-GCC, mask and bmask modules: stream calls of 6, 40 and 6 frames and their frame hooks;
  every form of the modules' launch plans (csrc/module_plan.h), in host-pointer calls and in device-pointer calls of 6, 40 and 6 frames, the optional
  outputs taken in one and left out in the other: mask at N = 1024 and 2048, NOISY (whose first call is one chunk) at 1024 and 256; bmask at frames of
  1024, 2048 and 512 samples; multiband at N = 1024, 512 and 256; temporal GCC at 0.2 m and 48 kHz (above 64 KiB of LDS) and 16 kHz;
  the 2-microphone host calls, plain and tracked, and the four modules' host calls with every optional output left out (through the C ABI where
  the wrappers always take them): the _dev call behind them still gets a device buffer for some of them.

Sequences on ONE context (ADAPTIVE unless said otherwise), every call's outputs and the final state blob in the digest: what one call
decided or left behind must not reach the next call, whoever the caller is:
  a device-pointer call (lazy tails, steered), localisation alone, a pageable host call, a page-locked one (in chunks), a device-pointer
  call with 1 array (another array count: the history is settled), one with 2 -- adaptive_fallback OFF and AUTO (the policy reads its
  reports at a fixed lag, so a run is reproducible);
  three device-pointer calls under MCA_HIP_WS_MAX_MB = 1 (the sliced map, the steered path in passes);
  FP16 and ADAPTIVE: a call, a rejected call (max_arrays + 1 arrays: its error code is checked), a call;
  a graph launched twice, an eager device-pointer call, one more launch;
  2 microphones: mca_hip_gcc2_frames_dev, a tracked call, mca_hip_gcc2_frames_dev again (refused once a tracker is attached: the refusal's
  code enters the digest), a tracked call;
  4 microphones: localisation alone three times, then state_save."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_mvdr_builds as frame                               # noqa: E402

A_MAX, A = 3, 2
CALLS = (64, 160, 64)
XS4 = [0.05 * m for m in range(4)]


def child(out_path):
    import json
    os.environ["MCA_HIP_ADAPT_MIN_ROWS"] = "64"                   # read by mca_hip_create
    os.environ["MCA_HIP_ADAPT_CAND"] = "1"
    os.environ.pop("MCA_HIP_ADAPT_FALLBACK", None)
    api, np, has = frame.load_lib()
    import torch
    from mcarray_amd import synth
    dev = torch.device("cuda:0")
    res = {}
    precisions = (("FP32", api.SRP_FP32), ("FP16", api.SRP_FP16), ("FP16X3", api.SRP_FP16X3), ("ADAPTIVE", api.SRP_ADAPTIVE))

    def pcm_of(xs, fs, hop, frames, seed, quiet_frames=0):
        pcm = np.stack([synth.noise_source_stream(xs, np.deg2rad(-35.0 + 50 * a), fs, (frames + 1) * hop, seed + a, snr_db=12.0) for a in range(A)])
        pcm[:, :, :quiet_frames * hop] *= 1e-3
        return pcm.astype(np.float32)

    def ctx_of(xs, fs, N, prec, S=1, floor=False, step=0.5):
        return api.Context(fs, xs, N, step, S, use_power_floor=floor, srp_precision=prec, max_arrays=A_MAX, adaptive_fallback=False)

    def dev_call(ctx, chunk, F, parts):
        hop = ctx.hop
        r = [torch.zeros((A, F, ctx.S), dtype=torch.int32, device=dev), torch.zeros((A, F, ctx.S), device=dev), torch.zeros((A, F, ctx.S), device=dev),
             torch.zeros((A, F, ctx.D), device=dev), torch.zeros((A, ctx.S, F * hop), device=dev)]
        ctx.process_frames_dev(torch.from_numpy(chunk.copy()).to(dev), F, *r)
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in r]

    def dev_stream(name, ctx, pcm, calls=CALLS):
        parts, t0 = [], 0
        for F in calls:
            dev_call(ctx, pcm[:, :, t0 * ctx.hop:(t0 + F + 1) * ctx.hop], F, parts)
            t0 += F
        parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
        ctx.close()
        res[name] = frame.digest(*parts)

    total = sum(CALLS)
    for pname, prec in precisions:
        for name, xs, floor in (("ULA8", synth.ULA8, False), ("ULA8 gated", synth.ULA8, True), ("ULA16", synth.ULA16, False), ("4 microphones", XS4, False)):
            dev_stream("dev stream, %s, %s" % (name, pname), ctx_of(xs, 48000, 1024, prec, floor=floor), pcm_of(xs, 48000, 512, total, 500, 100 if floor else 0))
        for N in (512, 2048):
            for M in (4, 8):
                xs = [0.04 * m for m in range(M)]
                dev_stream("dev stream, N = %d, %d microphones, %s" % (N, M, pname), ctx_of(xs, 48000, N, prec), pcm_of(xs, 48000, N // 2, total, 510))
    for pname, prec in precisions[:3]:
        dev_stream("dev stream, S = 2 on a non-uniform array, %s" % pname, ctx_of(synth.REEM_C, 48000, 1024, prec, S=2, step=5.0),
                   pcm_of(synth.REEM_C, 48000, 512, total, 520))

    # the kernel families the cases above do not reach (each launch of the stream path is planned by csrc/stream_plan.h)
    for pname, prec in (precisions[0], precisions[1]):
        for N in (1024, 2048, 4096):
            dev_stream("dev stream, 2 microphones, N = %d, %s" % (N, pname), ctx_of(synth.BINAURAL, 48000, N, prec), pcm_of(synth.BINAURAL, 48000, N // 2, total, 570))
        xs3 = [0.05 * m for m in range(3)]
        for N in (256, 4096):
            dev_stream("dev stream, 3 microphones, N = %d (any length), %s" % (N, pname), ctx_of(xs3, 48000, N, prec), pcm_of(xs3, 48000, N // 2, total, 571))
    xs5 = [0.04 * m for m in range(5)]
    for pname, prec in (precisions[1], precisions[3]):
        for S in (2, 3):
            dev_stream("dev stream, ULA16, S = %d, %s" % (S, pname), ctx_of(synth.ULA16, 48000, 1024, prec, S=S), pcm_of(synth.ULA16, 48000, 512, total, 572))
        for S in (1, 2):
            dev_stream("dev stream, 5 microphones, S = %d, %s" % (S, pname), ctx_of(xs5, 48000, 1024, prec, S=S), pcm_of(xs5, 48000, 512, total, 573))
        dev_stream("dev stream, ULA8, 5 degree grid (Dp = 64), %s" % pname, ctx_of(synth.ULA8, 48000, 1024, prec, step=5.0), pcm_of(synth.ULA8, 48000, 512, total, 574))
        dev_stream("dev stream, ULA8, 0.4 degree grid (D - 2 > 384), %s" % pname, ctx_of(synth.ULA8, 48000, 1024, prec, step=0.4), pcm_of(synth.ULA8, 48000, 512, total, 575))

    # the host-pointer entry points
    def host_stream(name, ctx, pcm, convert=lambda x: x, into=None):
        parts, t0 = [], 0
        for F in CALLS:
            r = ctx.process_frames_host(convert(pcm[:, :, t0 * ctx.hop:(t0 + F + 1) * ctx.hop]), want_energy=True, into=into(F) if into else None)
            parts += [np.array(r[k]) for k in ("bin", "doa", "prob", "energy", "out", "voiced", "power") if r.get(k) is not None]
            t0 += F
        parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
        ctx.close()
        res[name] = frame.digest(*parts)

    pcm8 = pcm_of(synth.ULA8, 48000, 512, total, 530, 100)
    for pname, prec in (precisions[0], precisions[3]):
        for floor in (False, True):
            tag = "%s%s" % (pname, ", gated" if floor else "")
            host_stream("host stream, pageable, %s" % tag, ctx_of(synth.ULA8, 48000, 1024, prec, floor=floor), pcm8)
            host_stream("host stream, 16-bit PCM, %s" % tag, ctx_of(synth.ULA8, 48000, 1024, prec, floor=floor), pcm8,
                        convert=lambda x: np.ascontiguousarray(np.clip(np.rint(x * 20000.0), -32768, 32767).astype(np.int16)))
            pins = []

            def pinned(x):
                b = api.PinnedBuffer(x.shape, np.float32)
                b.array[...] = x
                pins.append(b)
                return b.array
            host_stream("host stream, page-locked input (chunks of arrays), %s" % tag, ctx_of(synth.ULA8, 48000, 1024, prec, floor=floor), pcm8, convert=pinned)
            for b in pins:
                b.close()
            os.environ["MCA_HIP_WS_MAX_MB"] = "1"
            sliced = ctx_of(synth.ULA8, 48000, 1024, prec, floor=floor)
            del os.environ["MCA_HIP_WS_MAX_MB"]
            host_stream("host stream, pageable, MCA_HIP_WS_MAX_MB = 1 (sliced), %s" % tag, sliced, pcm8)

    # a graph: 4 launches, an eager call that grows the workspace (its state saved and restored), 2 more launches
    for pname, prec in (precisions[0], precisions[3]):
        ctx = ctx_of(synth.ULA8, 48000, 1024, prec)
        F, hop = 64, 512
        pcm = pcm_of(synth.ULA8, 48000, hop, 6 * F, 540)
        buf = dict(pcm=torch.zeros((A, 8, (F + 1) * hop), device=dev), bin=torch.zeros((A, F, 1), dtype=torch.int32, device=dev), rad=torch.zeros((A, F, 1), device=dev),
                   prob=torch.zeros((A, F, 1), device=dev), energy=torch.zeros((A, F, ctx.D), device=dev), out=torch.zeros((A, 1, F * hop), device=dev))
        g = ctx.graph_create(buf["pcm"], F, buf["bin"], buf["rad"], buf["prob"], buf["energy"], buf["out"])
        parts = []
        for i in range(6):
            if i == 4:
                blob = ctx.state_save()
                dev_call(ctx, pcm[:, :, :(160 + 1) * hop], 160, [])
                ctx.state_load(blob)
            buf["pcm"].copy_(torch.from_numpy(pcm[:, :, i * F * hop:(i * F + F + 1) * hop].copy()))
            g.launch()
            torch.cuda.synchronize()
            parts += [buf[k].cpu().numpy() for k in ("bin", "rad", "prob", "energy", "out")]
        parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
        g.close()
        ctx.close()
        res["graph: 4 launches, an eager growth, 2 launches, %s" % pname] = frame.digest(*parts)

    # the gated 2-microphone path with a tracker, its frame hook and setProbability
    fs, N = 16000, 1024
    hop = N // 2
    pcm2 = pcm_of(synth.BINAURAL, fs, hop, total, 550, 100)
    ctx = api.Context(fs, synth.BINAURAL, N, 3.0, 1, True, max_arrays=A_MAX)
    ctx.gcc2_tracker_attach(seed=0x5EED0001)
    parts, t0 = [], 0
    for F in CALLS:
        full = F != max(CALLS)
        r = [torch.zeros((A, F), device=dev), torch.zeros((A, F), dtype=torch.int32, device=dev) if full else None, torch.zeros((A, F), device=dev),
             torch.zeros((A, F), dtype=torch.uint8, device=dev), torch.zeros((A, F), dtype=torch.int32, device=dev),
             torch.zeros((A, F, ctx.D), device=dev) if full else None]
        ctx.gcc2_tracked_frames_dev(torch.from_numpy(pcm2[:, :, t0 * hop:(t0 + F + 1) * hop].copy()).to(dev), F, *r)
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in r if t is not None]
        t0 += F
    parts.append(ctx.gcc2_set_probability(np.linspace(-1.2, 1.2, 7), 1))
    rng = np.random.default_rng(560)
    for _ in range(3):
        fr = rng.standard_normal((2, N + 2))
        fr[:, 1] = 0.0
        fr[:, N + 1] = 0.0
        h = ctx.gcc2_process_frame(fr)
        parts += [np.asarray([h["doa"], h["prob"], h["power"], float(h["argmax"]), float(h["fired"]), float(h["track"])]), h["corr"]]
    parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
    ctx.close()
    res["gated 2-microphone path with a tracker, frame hook, setProbability"] = frame.digest(*parts)
    plain = api.Context(fs, synth.BINAURAL, N, 3.0, 1, True, max_arrays=A_MAX)
    parts, t0 = [], 0
    for F in CALLS:
        r = plain.gcc2_frames_host(pcm2[:, :, t0 * hop:(t0 + F + 1) * hop], want_corr=True)
        parts += [r[k] for k in ("argmax", "doa", "prob", "corr", "voiced", "power")]
        t0 += F
    parts.append(np.frombuffer(plain.state_save(), dtype=np.uint8))
    plain.close()
    res["gated 2-microphone path, host calls"] = frame.digest(*parts)

    # the double frame API
    ctx = api.Context(16000, XS4, 256, 5.0, 2)
    parts = []
    for _ in range(4):
        fr = rng.standard_normal((4, 258))
        fr[:, 1] = 0.0
        fr[:, 257] = 0.0
        doa, prob, bins = ctx.steering_process_frame(fr, 2)
        parts += [doa, prob, bins, ctx.beamformer_process_frame(fr, float(doa[0])), np.asarray([ctx.fft_log_power(fr)]), ctx.energy()]
    parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
    ctx.close()
    res["double frame API: steering, beamformer, power"] = frame.digest(*parts)

    # sequences on ONE context that change the caller, the array count or the path between calls (the docstring's last paragraph)
    def outs(ctx, n_arr, F, audio=True):
        r = [torch.zeros((n_arr, F, ctx.S), dtype=torch.int32, device=dev), torch.zeros((n_arr, F, ctx.S), device=dev), torch.zeros((n_arr, F, ctx.S), device=dev),
             torch.zeros((n_arr, F, ctx.D), device=dev)]
        return r + ([torch.zeros((n_arr, ctx.S, F * ctx.hop), device=dev)] if audio else [])

    def seq_dev(ctx, chunk, F, parts, audio=True):          # process_frames_dev, or localise_frames_dev alone
        r = outs(ctx, chunk.shape[0], F, audio)
        ctx.process_frames_dev(torch.from_numpy(chunk.copy()).to(dev), F, *r, separate=audio)
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in r]

    def seq_host(ctx, chunk, parts, pin=False):
        b = api.PinnedBuffer(chunk.shape, np.float32) if pin else None
        if pin:
            b.array[...] = chunk
        r = ctx.process_frames_host(b.array if pin else chunk, want_energy=True)
        parts += [np.array(r[k]) for k in ("bin", "doa", "prob", "energy", "out")]
        if pin:
            b.close()

    def finish(name, ctx, parts):
        parts.append(np.frombuffer(ctx.state_save(), dtype=np.uint8))
        ctx.close()
        res[name] = frame.digest(*parts)

    def cut(pcm, hop, t0, F):
        return pcm[:, :, t0 * hop:(t0 + F + 1) * hop]

    adaptive = api.SRP_ADAPTIVE
    seq_frames = (64, 160, 64, 160, 64, 64)
    pcm_seq = pcm_of(synth.ULA8, 48000, 512, sum(seq_frames), 570)
    for tag, auto in (("adaptive_fallback OFF", False), ("adaptive_fallback AUTO", True)):
        ctx = api.Context(48000, synth.ULA8, 1024, 0.5, 1, srp_precision=adaptive, max_arrays=A_MAX, adaptive_fallback=auto)
        parts, t0 = [], 0
        for i, F in enumerate(seq_frames):
            chunk = cut(pcm_seq, 512, t0, F)
            if i == 0 or i == 5:
                seq_dev(ctx, chunk, F, parts)
            elif i == 1:
                seq_dev(ctx, chunk, F, parts, audio=False)
            elif i == 4:
                seq_dev(ctx, chunk[:1], F, parts)           # another array count: the history is settled
            else:
                seq_host(ctx, chunk, parts, pin=i == 3)
            t0 += F
        finish("sequence: dev, localise alone, pageable host, page-locked host, dev with 1 array, dev; ADAPTIVE, %s" % tag, ctx, parts)

    os.environ["MCA_HIP_WS_MAX_MB"] = "1"
    sliced = ctx_of(synth.ULA8, 48000, 1024, adaptive)
    del os.environ["MCA_HIP_WS_MAX_MB"]
    dev_stream("sequence: three dev calls under MCA_HIP_WS_MAX_MB = 1 (sliced map, steered path in passes), ADAPTIVE", sliced, pcm_seq)

    for pname, prec in (precisions[1], precisions[3]):
        ctx, parts, t0 = ctx_of(synth.ULA8, 48000, 1024, prec), [], 0
        for i, F in enumerate(CALLS):
            if i == 1:                                       # rejected: more arrays than the context has
                many = np.zeros((A_MAX + 1, 8, (F + 1) * 512), dtype=np.float32)
                try:
                    seq_dev(ctx, many, F, [])
                    code = 0
                except api.MCArrayHipError as e:
                    code = int(str(e).split("error")[1].split(":")[0])
                if code != -1:                               # MCA_HIP_ERR_INVALID_ARGUMENT
                    sys.exit("the call with max_arrays + 1 arrays returned %d" % code)
                parts.append(np.asarray([code]))
            else:
                seq_dev(ctx, cut(pcm_seq, 512, t0, F), F, parts)
                t0 += F
        finish("sequence: dev, a rejected call, dev; %s" % pname, ctx, parts)

    ctx = ctx_of(synth.ULA8, 48000, 1024, adaptive)
    F = 64
    buf = [torch.zeros((A, 8, (F + 1) * 512), device=dev)] + outs(ctx, A, F)
    g = ctx.graph_create(buf[0], F, *buf[1:])
    parts = []
    for i in range(4):
        chunk = cut(pcm_seq, 512, i * F, F)
        if i == 2:                                           # an eager call in between: it leaves lazy tails, the next launch settles them
            seq_dev(ctx, chunk, F, parts)
            continue
        buf[0].copy_(torch.from_numpy(chunk.copy()))
        g.launch()
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in buf[1:]]
    g.close()
    finish("sequence: a graph launched twice, an eager dev call, one more launch; ADAPTIVE", ctx, parts)

    # (gcc2_frames_dev is refused once a tracker is attached, so the third call of the sequence is that refusal and a tracked call follows it)
    ctx = api.Context(fs, synth.BINAURAL, N, 3.0, 1, True, srp_precision=adaptive, max_arrays=A_MAX)
    parts, t0 = [], 0
    for i, F in enumerate(CALLS + (64,)):
        x = torch.from_numpy(cut(pcm2, hop, t0, F).copy()).to(dev)
        r = [torch.zeros((A, F), dtype=torch.int32, device=dev), torch.zeros((A, F), device=dev), torch.zeros((A, F), device=dev), torch.zeros((A, F, ctx.D), device=dev)]
        if i == 0:
            ctx.gcc2_frames_dev(x, F, *r)
            ctx.gcc2_tracker_attach(seed=0x5EED0002)
        elif i == 2:
            try:
                ctx.gcc2_frames_dev(x, F, *r)
                sys.exit("gcc2_frames_dev ran on a context with a tracker")
            except api.MCArrayHipError as e:
                parts.append(np.asarray([int(str(e).split("error")[1].split(":")[0])]))
            continue
        else:
            ctx.gcc2_tracked_frames_dev(x, F, r[1], argmax=r[0], prob=r[2], corr=r[3])
        torch.cuda.synchronize()
        parts += [t.cpu().numpy() for t in r]
        t0 += F
    finish("sequence: gcc2_frames_dev, a tracked call, gcc2_frames_dev refused, a tracked call; 2 microphones, ADAPTIVE", ctx, parts)

    ctx, parts, t0 = ctx_of(XS4, 48000, 1024, adaptive), [], 0
    pcm4 = pcm_of(XS4, 48000, 512, total, 580)
    for F in CALLS:
        seq_dev(ctx, cut(pcm4, 512, t0, F), F, parts, audio=False)
        t0 += F
    finish("sequence: localise alone three times (lazy tails), then state_save; 4 microphones, ADAPTIVE", ctx, parts)

    # the four modules: stream calls of 6, 40 and 6 frames, then the frame hooks
    def noise(n, seed):
        return np.stack([synth.noise_source_stream(synth.BINAURAL, np.deg2rad(20.0 - 45 * a), 16000, n, seed + a) for a in range(A)]).astype(np.float32)

    def blob(m):
        return np.frombuffer(m.state_save(), dtype=np.uint8)

    frames = (6, 40, 6)
    m, parts = api.MultibandBinarualLocalisation(16000, synth.BINAURAL, nbins=5, use_power_floor=False, max_arrays=A_MAX), []
    x = noise((max(frames) + 1) * m.hop, 600)
    for F in frames:
        r = m.process(x[:, :, :(F + 1) * m.hop], want_bands=True)
        parts += [r[k] for k in ("doa", "prob", "voiced", "power", "band_idx", "energy_in_doa", "band_corr")]
    parts.append(blob(m))
    m.close()
    res["multiband module"] = frame.digest(*parts)

    m, parts = api.TemporalGCCBinauralLocalisation(16000, synth.BINAURAL, use_power_floor=False, max_arrays=A_MAX), []
    x = noise((max(frames) - 1) * m.hop + m.W, 610)
    for F in frames:
        r = m.process(x[:, :, :(F - 1) * m.hop + m.W], want_index=True)
        parts += [r[k] for k in ("doa", "prob", "voiced", "power", "delay_idx", "index")]
    h = m.process_frame(x[0, 0, :m.W].astype(np.float64), x[0, 1, :m.W].astype(np.float64))
    parts += [np.asarray([h["doa"], h["prob"], h["power"], float(h["delay_idx"]), float(h["voiced"])]), h["index"], blob(m)]
    m.close()
    res["temporal-GCC module and its frame hook"] = frame.digest(*parts)

    m, parts = api.FastBinauralMasking(16000, 0.086, 100.0, 7000.0, fft_size=512, max_streams=A_MAX), []
    x = noise((max(frames) + 1) * 256, 620)
    for F in frames:
        parts += list(m.process(x[:, :, :(F + 1) * 256]))
    spec = rng.standard_normal((2, 514))
    spec[:, 1] = 0.0
    spec[:, 513] = 0.0
    parts += list(m.process_parametrisation(spec[0], spec[1])) + [blob(m)]
    m.close()
    res["mask module and its frame hook"] = frame.digest(*parts)

    m, parts = api.BinauralMaskingImpl(16000, 0.086, 100.0, 7000.0, max_streams=A_MAX), []
    x = noise((max(frames) + 1) * m.hop, 630)
    for F in frames:
        parts += list(m.process(x[:, :, :(F + 1) * m.hop]))
    ana = [m.frame_analysis(x[0, c, :m.W].astype(np.float64), channel=c) for c in (0, 1)]
    left, right, dec = m.process_parametrisation(ana[0], ana[1])
    parts += ana + [left, right, dec, m.frame_synthesis(left, channel=0), m.frame_synthesis(right, channel=1), blob(m)]
    m.close()
    res["bmask module and its frame hooks"] = frame.digest(*parts)

    # every form of the modules' launch plans (csrc/module_plan.h), each in host-pointer calls and in device-pointer calls on a context of its own;
    # the optional outputs are taken in one of the two and left out in the other
    def cpu(ts):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in ts if t is not None]

    def z(shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def masking(name, make, hop, seed):
        x = noise((max(frames) + 1) * hop, seed)
        for tag, host in (("host calls, decisions taken", True), ("device calls, no decisions", False)):
            m, parts = make(), []
            for F in frames:
                if host:
                    parts += list(m.process(x[:, :, :(F + 1) * hop]))
                else:
                    out = z((A, 2, F * hop))
                    m.process_dev(up(x[:, :, :(F + 1) * hop]), F, out, None)
                    parts += cpu([out])
            parts.append(blob(m))
            m.close()
            res["%s, %s" % (name, tag)] = frame.digest(*parts)

    for n_fft in (1024, 2048):
        masking("mask module, N = %d" % n_fft, lambda: api.FastBinauralMasking(16000, 0.086, 100.0, 7000.0, fft_size=n_fft, max_streams=A_MAX), n_fft // 2, 640)
    masking("mask module, NOISY and its first call, N = 1024", lambda: api.FastBinauralMasking(16000, 0.086, 100.0, 7000.0, method=api.NOISY, max_streams=A_MAX), 512, 641)
    masking("mask module, NOISY and its first call, N = 256 (any length)",
            lambda: api.FastBinauralMasking(16000, 0.086, 100.0, 7000.0, method=api.NOISY, fft_size=256, max_streams=A_MAX), 128, 642)
    for fs_b, W in ((16000, 1024), (48000, 2048), (8000, 512)):
        def make_bmask():
            m = api.BinauralMaskingImpl(fs_b, 0.086, 100.0, 3500.0, max_streams=A_MAX)
            if m.W != W:
                sys.exit("bmask at %d Hz has frames of %d samples" % (fs_b, m.W))
            return m
        masking("bmask module, frames of %d samples" % W, make_bmask, W // 2, 650)

    for n_fft, host_bands in ((1024, False), (512, False), (256, True)):
        for host in (True, False):
            m, parts = api.MultibandBinarualLocalisation(16000, synth.BINAURAL, nbins=5, use_power_floor=False, fft_size=n_fft, max_arrays=A_MAX), []
            x = noise((max(frames) + 1) * m.hop, 660)
            for F in frames:
                if host:
                    r = m.process(x[:, :, :(F + 1) * m.hop], want_bands=host_bands)
                    parts += [r[k] for k in ("doa", "prob", "voiced", "power", "band_idx", "energy_in_doa", "band_corr") if r[k] is not None]
                else:                                        # what the host calls of this size left out is taken, and the other way round
                    o = [z((A, F)), z((A, F))] + ([None] * 5 if host_bands else
                                                  [z((A, F), torch.uint8), z((A, F)), z((A, F, 5), torch.int32), z((A, F, m.D)), z((A, F, 5, m.D))])
                    m.process_dev(up(x[:, :, :(F + 1) * m.hop]), F, *o)
                    parts += cpu(o)
            parts.append(blob(m))
            m.close()
            res["multiband module, N = %d, %s" % (n_fft, "host calls" if host else "device calls")] = frame.digest(*parts)

    pair = [[-0.1, 0.0, 0.0], [0.1, 0.0, 0.0]]               # 0.2 m: 27 delay pairs at 48 kHz (72 304 bytes of LDS), 9 at 16 kHz (23 392)
    for fs_t in (48000, 16000):
        for host in (True, False):
            m, parts = api.TemporalGCCBinauralLocalisation(fs_t, pair, use_power_floor=False, max_arrays=A_MAX), []
            x = noise((max(frames) - 1) * m.hop + m.W, 670)
            for F in frames:
                cutx = x[:, :, :(F - 1) * m.hop + m.W]
                r = m.process(cutx) if host else m.process_dev(up(cutx), want_index=True)
                parts += [r[k] for k in ("doa", "prob", "voiced", "power", "delay_idx")] if host else cpu([r[k] for k in ("doa", "prob", "voiced", "power", "delay_idx", "index")])
            parts.append(blob(m))
            m.close()
            res["temporal-GCC module, %d Hz, %s" % (fs_t, "host calls, no index" if host else "device calls, the index taken")] = frame.digest(*parts)

    # the 2-microphone host calls with every optional output left out (the wrappers always take them: the C ABI directly)
    import ctypes as C
    for tracked in (False, True):
        ctx = api.Context(fs, synth.BINAURAL, N, 3.0, 1, True, max_arrays=A_MAX)
        if tracked:
            ctx.gcc2_tracker_attach(seed=0x5EED0003)
        parts, t0 = [], 0
        for F in frames:
            x = np.ascontiguousarray(pcm2[:, :, t0 * hop:(t0 + F + 1) * hop])
            one = np.empty((A, F), dtype=np.float32 if tracked else np.int32)
            xp, op = x.ctypes.data_as(C.POINTER(C.c_float)), one.ctypes.data_as(C.POINTER(C.c_float if tracked else C.c_int))
            if tracked:
                rc = ctx._lib.mca_hip_gcc2_tracked_frames_host(ctx.h, xp, A, F, None, op, None, None, None, None)
            else:
                rc = ctx._lib.mca_hip_gcc2_frames_host(ctx.h, xp, A, F, op, None, None, None)
            if rc != 0:
                sys.exit("the 2-microphone host call without optional outputs returned %d" % rc)
            parts.append(one)
            t0 += F
        finish("2-microphone host calls, %s, optional outputs left out" % ("tracked" if tracked else "plain"), ctx, parts)

    # the modules' host calls with every optional output left out: the _dev call behind them still gets a device buffer for some of them
    # (StageBuf, STAGE_ALWAYS).  The multiband and temporal-GCC wrappers always take theirs: the C ABI directly
    fpt = C.POINTER(C.c_float)
    for name, m in (("mask", api.FastBinauralMasking(16000, 0.086, 100.0, 7000.0, fft_size=512, max_streams=A_MAX)),
                    ("bmask", api.BinauralMaskingImpl(16000, 0.086, 100.0, 7000.0, max_streams=A_MAX))):
        x, parts = noise((max(frames) + 1) * m.hop, 680), []
        for F in frames:
            out, dec = m.process(x[:, :, :(F + 1) * m.hop], want_decisions=False)
            if dec is not None:
                sys.exit("the %s wrapper took decisions" % name)
            parts.append(out)
        parts.append(blob(m))
        m.close()
        res["%s module, host calls without decisions" % name] = frame.digest(*parts)
    m, parts = api.MultibandBinarualLocalisation(16000, synth.BINAURAL, nbins=5, use_power_floor=False, max_arrays=A_MAX), []
    x = noise((max(frames) + 1) * m.hop, 681)
    for F in frames:
        xc = np.ascontiguousarray(x[:, :, :(F + 1) * m.hop])
        doa, prob = np.empty((A, F), dtype=np.float32), np.empty((A, F), dtype=np.float32)
        rc = m._lib.mca_hip_mb_frames_host(m.h, xc.ctypes.data_as(fpt), A, F, doa.ctypes.data_as(fpt), prob.ctypes.data_as(fpt), None, None, None, None, None)
        if rc != 0:
            sys.exit("the multiband host call without optional outputs returned %d" % rc)
        parts += [doa, prob]
    parts.append(blob(m))
    m.close()
    res["multiband module, host calls, optional outputs left out"] = frame.digest(*parts)
    for fs_t in (48000, 16000):
        m, parts = api.TemporalGCCBinauralLocalisation(fs_t, pair, use_power_floor=False, max_arrays=A_MAX), []
        x = noise((max(frames) - 1) * m.hop + m.W, 682)
        for F in frames:
            xc = np.ascontiguousarray(x[:, :, :(F - 1) * m.hop + m.W])
            doa = np.empty((A, F), dtype=np.float32)
            rc = m._lib.mca_hip_tgcc_frames_host(m.h, xc.ctypes.data_as(fpt), A, F, doa.ctypes.data_as(fpt), None, None, None, None, None)
            if rc != 0:
                sys.exit("the temporal-GCC host call without optional outputs returned %d" % rc)
            parts.append(doa)
        parts.append(blob(m))
        m.close()
        res["temporal-GCC module, %d Hz, host calls, optional outputs left out" % fs_t] = frame.digest(*parts)

    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    par, new = frame.run_both(__file__, sys.argv[1], seconds=420)
    sys.exit(frame.report(par, new, "outputs and state blobs", sys.argv[1]))


if __name__ == "__main__":
    main()

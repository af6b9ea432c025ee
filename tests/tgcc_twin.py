"""numpy float64 restatement of mca::TemporalGCCBinauralLocalisation (the time-domain 2-microphone localiser of the
reference's BinauralLocalisation.cpp:66-314) with the [BUILD-DEFINES] decisions of DESIGN.md:

* frames of W = (int)(2 * (0.075 * fs)) raw samples (the analysis is the unwindowed frame) at hop W // 2;
* nd = (int)(d * fs / 346.1) delay pairs; pair i delays channel 0 by i and channel 1 by nd - i samples;
* cross-correlation in the IPP convention dst[n] = sum_m a[m] b[m + n - nd], n = 0..2nd, b zero outside;
* deviations with denominator W - 1 over the whole delayed frame (its zeros included); a zero product skips the division;
* index[i] = sum_n |c_i[n]|, + tri, max-min normalisation (it ADDS the minimum), first maximum, samples2Degrees - 90;
* the power gate of setPowerFloor / logPower, and cur = 0.5 cur + 0.5 DOA.

Two forms of the per-frame index: `frame_index` (closed form: 4nd - 1 lagged dot products over a common body, each (i, n)
minus its tail at the frame's end) and `frame_index_literal` (delay -> cross-correlation -> deviations -> divide -> abs-sum,
line by line), which exists only to check the closed form.
"""
import numpy as np

SPEED_OF_SOUND = 346.1
FRAME_SECONDS = 0.075
FLOOR_SECONDS = 3


def geometry(fs, d):
    """-> (W, hop, nd) as the reference's constructor computes them (BinauralLocalisation.cpp:68-71)."""
    W = int(2 * (FRAME_SECONDS * fs))
    return W, W // 2, int(d * fs / SPEED_OF_SOUND)


def triangle(nd):
    """0.1 * Triangle_Direct(asym 0, phase 3 pi / 2, frequency 1 / (2 nd)) (BinauralLocalisation.cpp:96-99)."""
    n = np.arange(nd, dtype=np.float64)
    return 0.1 * (1.0 - np.abs(2.0 * n - nd) / nd)


def samples2degrees(k, nd):
    """samples2Degrees (BinauralLocalisation.cpp:277-284), without the caller's - 90."""
    k = min(k, nd - 1)
    k = max(k, -(nd - 1))
    shift = (nd - 1) / 2.0
    return np.arccos(2 * (float(k) - shift) / (nd - 1)) * 180 / np.pi


def _delayed(x, k):
    out = np.zeros_like(x)
    out[k:] = x[:len(x) - k]
    return out


def _scale(L, R, nd):
    """the divisor stddev(L_i) * stddev(R_i) of each pair (ddof = 1 over the delayed frame, zeros included)."""
    return np.array([np.std(_delayed(L, i), ddof=1) * np.std(_delayed(R, nd - i), ddof=1) for i in range(nd)])


def frame_index_literal(L, R, nd):
    """index[i] line by line: delay, IPP cross-correlation with lowLag = -nd, divide by the deviations, |.|, sum."""
    W = len(L)
    index = np.empty(nd)
    for i in range(nd):
        a, b = _delayed(L, i), _delayed(R, nd - i)
        c = np.empty(2 * nd + 1)
        for n in range(2 * nd + 1):
            lag = n - nd
            lo, hi = max(0, -lag), min(W, W - lag)
            c[n] = np.dot(a[lo:hi], b[lo + lag:hi + lag])
        s = np.std(a, ddof=1) * np.std(b, ddof=1)
        if s != 0:
            c = c / s
        index[i] = np.sum(np.abs(c))
    return index


def frame_index(L, R, nd):
    """the same index[] in closed form: c_i[n] = B(tau) - tail with tau = n + 2i - 2nd."""
    W = len(L)
    B = {}
    for tau in range(-2 * nd, 2 * nd - 1):
        if tau >= 0:
            B[tau] = np.dot(L[:W - tau], R[tau:])
        else:
            B[tau] = np.dot(L[-tau:], R[:W + tau])
    scale = _scale(L, R, nd)
    index = np.empty(nd)
    for i in range(nd):
        c = np.empty(2 * nd + 1)
        for n in range(2 * nd + 1):
            tau = n + 2 * i - 2 * nd
            full_hi = W - 1 - max(tau, 0)
            hi = min(W - 1 - i, W - 1 - nd + i - tau)
            c[n] = B[tau] - np.dot(L[hi + 1:full_hi + 1], R[hi + 1 + tau:full_hi + 1 + tau])
        if scale[i] != 0:
            c = c / scale[i]
        index[i] = np.sum(np.abs(c))
    return index


def normalise(index, nd):
    """index + tri, then maxminNormalisation (BinauralLocalisation.cpp:169-170, :238-245)."""
    x = index + triangle(nd)
    x = x + x.min()
    return x / x.max()


def top_gap(nidx):
    """relative gap between the two largest normalised index values (the maximum is 1)."""
    s = np.sort(nidx)
    return (s[-1] - s[-2]) / s[-1]


def frame_result(L, R, nd, k=None):
    """-> (k, doa_deg, prob, normalised index, gap) of one voiced frame; k forces the pick."""
    nidx = normalise(frame_index(L, R, nd), nd)
    if k is None:
        k = int(np.argmax(nidx))
    doa = samples2degrees(k, nd) - 90
    prob = np.log(nidx[k] / (np.sum(np.abs(nidx)) + 0.000001)) if nidx[k] != 0 else np.log(0.0000000001)
    return k, doa, prob, nidx, top_gap(nidx)


class Twin:
    """one module object: state cur / prob / power-floor estimation, fed frame by frame."""

    def __init__(self, fs, d, use_power_floor=True):
        self.fs = fs
        self.W, self.hop, self.nd = geometry(fs, d)
        self.use_floor = use_power_floor
        self.needed = int(FLOOR_SECONDS * fs)
        self.cur, self.prob = 0.0, -1.0
        self.floor, self.consumed, self.estimated = 0.0, 0, False

    def frame(self, L, R, k=None):
        """processParametrisation (BinauralLocalisation.cpp:134-192) -> dict(voiced, doa, prob, power, k, index, gap)."""
        L = np.asarray(L, dtype=np.float64)
        R = np.asarray(R, dtype=np.float64)
        if self.use_floor and not self.estimated:
            n = min(self.needed - self.consumed, self.W)
            p = (np.sum(L[:n] ** 2) + np.sum(R[:n] ** 2)) / (2 * n)
            self.floor += p * n
            self.consumed += n
            if self.consumed >= self.needed:
                self.estimated = True
                self.floor /= self.consumed
                self.floor = 0.15 * (100 - self.floor) + self.floor
            power = self.floor
        else:
            with np.errstate(divide="ignore"):
                power = 10 * np.log10((np.sum(L ** 2) + np.sum(R ** 2)) / (2 * len(L)))
        voiced = (not self.use_floor) or power > self.floor
        kk, doa, prob, nidx, gap = frame_result(L, R, self.nd, k)
        if voiced:
            self.prob = prob
            self.cur = self.cur * 0.5 + 0.5 * doa
        else:
            self.cur = self.cur * 0.5
            self.prob = -100000.0
        return dict(voiced=voiced, doa=self.cur, prob=self.prob, power=power, k=kk if voiced else -1, index=nidx, gap=gap)


def frames_of(pcm, W, hop):
    """pcm [2][T] -> list of (L, R) frames at hop."""
    F = (pcm.shape[1] - W) // hop + 1
    return [(pcm[0, f * hop:f * hop + W], pcm[1, f * hop:f * hop + W]) for f in range(max(F, 0))]


def run_stream(pcm, fs, d, use_power_floor=True, forced=None):
    """pcm [2][T] -> dict of per-frame arrays (voiced, doa, prob, power, k, index [F][nd], gap); forced[f] >= 0 forces the
    pick of voiced frame f."""
    tw = Twin(fs, d, use_power_floor)
    out = dict(voiced=[], doa=[], prob=[], power=[], k=[], index=[], gap=[])
    for f, (L, R) in enumerate(frames_of(np.asarray(pcm, dtype=np.float64), tw.W, tw.hop)):
        k = None if forced is None or forced[f] < 0 else int(forced[f])
        r = tw.frame(L, R, k)
        for key in out:
            out[key].append(r[key])
    return {k: np.array(v) for k, v in out.items()}


# ---- synthetic two-channel recordings ----

def _lowpass(x, fs, fc):
    X = np.fft.rfft(x)
    X[np.fft.rfftfreq(len(x), 1.0 / fs) > fc] = 0
    return np.fft.irfft(X, len(x))


def _delay_fd(x, lead):
    """x delayed by `lead` samples (fractional, circular, in the frequency domain)."""
    X = np.fft.rfft(x)
    k = np.arange(len(X))
    return np.fft.irfft(X * np.exp(-2j * np.pi * k * lead / len(x)), len(x))


def recording(fs, d, theta_deg, seconds, seed, lead_in=0.0, lowpass=2000.0, rms=1000.0, noise=2.0, dc=0.0, quantise=True):
    """[2][T] float64: `lead_in` s of quiet (exact zeros + N(0, noise^2)), then white noise low-passed at `lowpass` Hz at RMS
    `rms` (+ dc) whose channel 0 leads by d sin(theta) fs / c samples, + N(0, noise^2) on each channel.  theta_deg may be a
    (start, end) pair: a source moving linearly in angle (applied per 256-sample block).  quantise: rounded to int16
    ("int16" clips to its range; True only rounds, so a DC offset beyond int16 stays exact in float32)."""
    rng = np.random.default_rng(seed)
    T = int(round(seconds * fs))
    T0 = int(round(lead_in * fs))
    n = T - T0
    s = rng.standard_normal(n)
    if lowpass:
        s = _lowpass(s, fs, lowpass)
    s *= rms / np.sqrt(np.mean(s ** 2))
    if np.isscalar(theta_deg):
        lead = d * np.sin(np.deg2rad(theta_deg)) * fs / SPEED_OF_SOUND
        ch1 = _delay_fd(s, lead)
    else:
        blk = 256
        ch1 = np.empty(n)
        for b0 in range(0, n, blk):
            th = theta_deg[0] + (theta_deg[1] - theta_deg[0]) * b0 / max(n - 1, 1)
            lead = d * np.sin(np.deg2rad(th)) * fs / SPEED_OF_SOUND
            ch1[b0:b0 + blk] = _delay_fd(s, lead)[b0:b0 + blk]
    out = np.zeros((2, T))
    out[0, T0:] = s + dc
    out[1, T0:] = ch1 + dc
    out += rng.normal(0.0, noise, size=out.shape)
    if quantise:
        out = np.round(out)
    if quantise == "int16":
        out = np.clip(out, -32768, 32767)
    return out


# the stream-parity configurations: (fs, d)
PARITY_CONFIGS = [(44100, 0.086), (48000, 0.089), (16000, 0.086)]
LEAD_IN = 1.6           # covers the 20 floor-estimation frames (19 hops + W = 1.575 s) at every rate


def parity_streams(fs, d, gate, seed=11):
    """[5][2][T] float64 (integer-valued, exact in float32): three fixed angles, a moving source and one stream with a DC offset
    of 100x its RMS.  Gate on: 1.6 s quiet lead-in, 3 s in all; gate off: 2 s of signal."""
    seconds, lead = (3.0, LEAD_IN) if gate else (2.0, 0.0)
    src = [(60.0, 0.0), (-30.0, 0.0), (10.0, 0.0), ((-70.0, 70.0), 0.0), (20.0, 100 * 1000.0)]
    return np.stack([recording(fs, d, th, seconds, seed + 17 * j, lead_in=lead, dc=dc) for j, (th, dc) in enumerate(src)])


def bits_streams(fs=44100, d=0.086, n_batch=64):
    """the bit-identity test's inputs: one 6 s gated stream at 40 deg, and a batch of n_batch others at random angles."""
    x = recording(fs, d, 40.0, 6.0, 3, lead_in=LEAD_IN)
    rng = np.random.default_rng(8)
    batch = np.stack([recording(fs, d, float(rng.uniform(-80, 80)), 6.0, 100 + j, lead_in=LEAD_IN) for j in range(n_batch)])
    return x, batch


def hook_stream(fs=44100, d=0.086):
    """the frame-hook test's input: 3 s, gated, not rounded to integers (the hook takes doubles)."""
    return recording(fs, d, 35.0, 3.0, 29, lead_in=LEAD_IN, quantise=False)


def muted_stream(fs=44100, d=0.086, seconds=1.5, seed=5):
    """channel 0 low-passed noise, channel 1 exact zeros (the zero-deviation rule)."""
    x = recording(fs, d, 0.0, seconds, seed)
    x[1] = 0.0
    return x


# the reference test's five files (test_mcarray.cpp:313-322): name, angle of channel 0's lead, accepted DOA range
REFERENCE_FILES = [("right90", 90.0, (-90, -30)), ("right45", 45.0, (-90, 0)), ("front", 0.0, (-20, 20)),
                   ("left45", -45.0, (0, 90)), ("left90", -90.0, (30, 90))]


def reference_recordings(seconds=6.0, lead_in=LEAD_IN, fs=44100, d=0.086, seed=1):
    """the five int16 recordings of the reference's asserted property, as [(name, pcm [2][T], (lo, hi))]."""
    return [(name, recording(fs, d, th, seconds, seed + j, lead_in=lead_in, quantise="int16"), rng_)
            for j, (name, th, rng_) in enumerate(REFERENCE_FILES)]

"""Float64 numpy restatement of BinauralMaskingImpl as DESIGN.md section 2b defines it: the literal time-domain module.

A windowed frame of each channel goes through 45 inverse transforms (band b = irfft(rfft(x) H_b), W samples), the statistics
are means over the W samples of the band signals, the decision is spatial mask, else temporal mask, else enhance, the bands
are summed again and overlap-added.  The three hooks (frameAnalysis, processParametrisation, frameSynthesis) are here with
the analysisLength rule.  Besides the results the twin returns two margins per (frame, band) cell, |P - Q_new| / Q_new and
|ncorr - thr|: a cell is near a tie when either is below NEAR_TIE, and only there may an fp32 path decide otherwise.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import np_twin  # noqa: E402

FACTOR, RELATIVE, FULL = 0, 1, 3
METHODS = (FACTOR, RELATIVE, FULL)
NB = 45
NEAR_TIE = 1e-4
C_SOUND = 346.1
f32 = np.float32
LAM = float(f32(0.04))
ONE_MINUS_LAM = float(f32(1) - f32(0.04))
RHO = float(f32(0.01))
SPATIAL_FACTOR = TEMPORAL_FACTOR = ENHANCE_FACTOR = 1.0
Q_GUARD = 1e-10


def frame_size(fs):
    order = int(np.floor(np.log2(fs * float(f32(0.050))) + 0.5))
    return 1 << min(max(order, 8), 14)


def log_power(x):
    x = np.asarray(x, dtype=np.float64)
    return 10.0 * np.log10(np.mean(x * x))


class Twin:
    def __init__(self, fs, d, lo, hi, method=RELATIVE, n_sum=NB):
        self.fs, self.W = fs, frame_size(fs)
        self.hop = self.W // 2
        self.method = method
        self.n_sum = n_sum                      # bands the stream path sums again (45; 44 is the rejected literal reading)
        self.H, self.center = np_twin.mel_filterbank(self.W, NB, fs, float(f32(lo)), float(f32(hi)))
        self.thr = np.cos(self.center * fs * 2 * np.pi * d * np.sin(10 * np.pi / 180) / C_SOUND) * 0.9
        self.Q = np.zeros(NB)
        self.win = np_twin.hann(self.W)

    # ---- the three hooks ----
    def bands(self, frame):
        """[45][W] band signals of one windowed frame"""
        return np.fft.irfft(np.fft.rfft(np.asarray(frame, dtype=np.float64))[None, :] * self.H, n=self.W, axis=1)

    def frame_analysis(self, frame, analysis_length=None):
        W = self.W
        n = 46 * W if analysis_length is None else analysis_length
        ana = np.zeros(n)
        y = self.bands(frame)
        for b in range(NB):
            if (b + 1) * W <= n:
                ana[b * W:(b + 1) * W] = y[b]
        if n >= 46 * W:
            ana[45 * W:46 * W] = np.asarray(frame, dtype=np.float64) - y.sum(axis=0)
        return ana

    def process_parametrisation(self, left, right):
        """left, right: analysis buffers (>= 45 W); returns modified copies, decisions[45], margins (temporal[45], spatial[45])"""
        W = self.W
        left, right = np.array(left, dtype=np.float64), np.array(right, dtype=np.float64)
        dec = np.zeros(NB, dtype=np.int32)
        mt, ms = np.zeros(NB), np.zeros(NB)
        for b in range(NB):
            l, r = left[b * W:(b + 1) * W], right[b * W:(b + 1) * W]      # views: scaled in place
            P = np.mean(((l + r) / 2) ** 2)
            self.Q[b] = self.Q[b] * LAM + ONE_MINUS_LAM * P
            Q = self.Q[b]
            temporal = P < Q
            den = np.sqrt(np.mean(l * l)) * np.sqrt(np.mean(r * r))
            ncorr = 1.0 if den == 0 else np.mean(l * r) / den
            spatial = ncorr < self.thr[b]
            mt[b] = abs(P - Q) / Q if Q > 0 else np.inf
            ms[b] = abs(ncorr - self.thr[b])
            if spatial or temporal:
                dec[b] = 2 if spatial else 1
                factor = SPATIAL_FACTOR if spatial else TEMPORAL_FACTOR
                for x in (l, r):
                    if self.method == FULL:
                        x /= 1000.0
                    elif self.method == FACTOR:
                        x /= factor
                    else:
                        f = RHO if Q < Q_GUARD else RHO * np.mean(x * x) / Q
                        x *= np.sqrt(f)
            else:
                l *= ENHANCE_FACTOR
                r *= ENHANCE_FACTOR
        return left, right, dec, (mt, ms)

    def frame_synthesis(self, analysis, analysis_length=None):
        """the literal loop: bin <= 45 and offset < analysisLength - W"""
        W = self.W
        n = len(analysis) if analysis_length is None else analysis_length
        out = np.zeros(W)
        b, off = 0, 0
        while b <= NB and off < n - W:
            out += analysis[off:off + W]
            b, off = b + 1, off + W
        return out

    # ---- the stream path ----
    def stream(self, pcm):
        """pcm [2][(F+1)*hop] -> dict(out [2][F*hop], dec [F][45], mt, ms [F][45])"""
        pcm = np.asarray(pcm, dtype=np.float64)
        W, hop = self.W, self.hop
        F = pcm.shape[1] // hop - 1
        acc = np.zeros((2, (F + 1) * hop))
        dec = np.zeros((F, NB), dtype=np.int32)
        mt, ms = np.zeros((F, NB)), np.zeros((F, NB))
        n_ana = (self.n_sum + 1) * W            # the literal synthesis loop then sums n_sum bands
        for t in range(F):
            ana = [self.frame_analysis(pcm[c, t * hop:t * hop + W] * self.win) for c in range(2)]
            l, r, dec[t], (mt[t], ms[t]) = self.process_parametrisation(ana[0], ana[1])
            acc[0, t * hop:t * hop + W] += self.frame_synthesis(l, n_ana)
            acc[1, t * hop:t * hop + W] += self.frame_synthesis(r, n_ana)
        return dict(out=acc[:, :F * hop], dec=dec, mt=mt, ms=ms)


def near_tie(res, eps=NEAR_TIE):
    return (res["mt"] < eps) | (res["ms"] < eps)


# ---- inputs ----
PARITY = {41: (0, 0.01), 42: (1, 0.003), 43: (3, 0.01)}      # seed -> (delay, noise level)
PARITY_FRAMES = 200


def parity_input(seed, fs=16000, F=PARITY_FRAMES):
    """float32 [2][(F+1)*hop]"""
    delay, nlev = PARITY[seed]
    hop = frame_size(fs) // 2
    n = (F + 1) * hop
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n) * 0.1
    left = s + rng.standard_normal(n) * nlev
    right = np.roll(s, delay) * 0.9 + rng.standard_normal(n) * nlev
    env = np.repeat(rng.choice([1, .2, .05, .6, .1], F + 1), hop)
    return np.stack([left * env, right * env]).astype(np.float32)


def rising_tones(fs, d, lo, hi, F):
    """float32 [2][(F+1)*hop]: one tone at every band centre, the level rising 10 % per hop, so that every band's frame power
    grows from frame to frame (P > Q of the frame before: the temporal rule never fires)"""
    tw = Twin(fs, d, lo, hi)
    n = (F + 1) * tw.hop
    t = np.arange(n)
    x = sum(np.cos(2 * np.pi * c * t + b) for b, c in enumerate(tw.center)) * 1e-3 * 1.1 ** (t / tw.hop)
    return np.stack([x, x]).astype(np.float32)


def tone16(n, magn, freq, phase=0.0):
    return np.round(magn * np.cos(2 * np.pi * freq * np.arange(n) + phase)).astype(np.int16)


def spatial_signal():
    """testSpatialMaskingCore's input (int16-valued), [2][5 * 1024]"""
    n, magn, delay = 5 * 1024, 5000, 6
    interest = tone16(n, magn, 0.1).astype(np.float64)
    interf_l = tone16(n, magn, 0.3).astype(np.float64)
    interf_r = np.zeros(n)
    interf_r[:n - delay] = interf_l[delay:]
    return np.stack([interest + interf_l, interest + interf_r])


def temporal_signal(fs=16000):
    """testTemporalMaskingCore's input: (pcm [2][50 * 1024], interest_start, tonestep)"""
    magn = 5000
    delay = int(0.1 * fs)
    tonestep = int(0.1 * fs)
    freqstep = f32(0.01)
    n = 50 * 1024
    tone = np.zeros(n)
    i, sfreq, interest_start = 0, f32(0.01), 0
    interest_freq = f32(0.2)
    while i < n - tonestep and sfreq < 0.5:
        if interest_freq - freqstep / 2 < sfreq < interest_freq + freqstep / 2:
            interest_start = i
        tone[i:i + tonestep] = tone16(tonestep, magn, float(sfreq))
        i += tonestep
        sfreq = f32(sfreq + freqstep)
    sig = np.zeros(n)
    tb = tone.copy()
    for k in range(6):
        tb = np.trunc(tb / 2)
        sig[delay * k:] += tb[:n - delay * k]
    return np.stack([sig, sig]), interest_start, tonestep


def bandpass(lo, hi):
    """dsp::BandPassFIRFilter(256, lo, hi) stand-in: firwin(257), frequencies in cycles/sample"""
    from scipy import signal
    return signal.firwin(257, [lo, hi], pass_zero=False, fs=1.0)


def band_power(x, lo, hi, sl=slice(None)):
    from scipy import signal
    return log_power(signal.lfilter(bandpass(lo, hi), 1.0, x)[sl])


def whole_frames(pcm, W):
    """cut [2][n] to (F+1)*hop samples"""
    hop = W // 2
    F = pcm.shape[1] // hop - 1
    return pcm[:, :(F + 1) * hop]


def spatial_powers(out_left):
    return band_power(out_left, 0.05, 0.15), band_power(out_left, 0.25, 0.35)


def temporal_difference(x, interest_start, tonestep, n):
    sl = slice(interest_start, interest_start + tonestep)
    return band_power(x[:n], 0.19, 0.21, sl) - band_power(x[:n], 0.15, 0.20, sl)

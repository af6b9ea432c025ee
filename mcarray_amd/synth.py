"""Deterministic synthetic multichannel input (host side, numpy only).

Plane-wave far-field model of SURVEY A.2: a source at angle theta (rad, >0
towards +x) reaches microphone m as x_m(t) = s(t + x_m*sin(theta)/c); the
fractional delays are applied in the frequency domain over the whole stream.
Geometries are the [BUILD-DEFINES] ones of SURVEY 8d plus the reference's
Reem-C array (test/test_mcarray.cpp:397).
"""
import numpy as np

C_SOUND = 346.1  # src/mcarray/microhponeArrayHelpers.cpp:42

ULA8 = [0.04 * m for m in range(8)]
ULA16 = [0.02 * m for m in range(16)]
BINAURAL = [0.0, 0.086]
REEM_C = [0.0, 0.07, 0.175, 0.21]


def delay_channels(s, xs, theta, fs):
    """s [L] -> [M][L] with x_m(t) = s(t + x_m sin(theta)/c) (circular over the stream)."""
    L = len(s)
    S = np.fft.rfft(s)
    f = np.fft.rfftfreq(L, d=1.0 / fs)
    xs = np.asarray(xs, dtype=np.float64)
    adv = xs * np.sin(theta) / C_SOUND  # seconds
    return np.fft.irfft(S[None, :] * np.exp(2j * np.pi * f[None, :] * adv[:, None]), n=L, axis=1)


def noise_source_stream(xs, theta, fs, n_samples, seed, sigma=0.1, snr_db=20.0):
    """White Gaussian source at `theta` plus independent sensor noise; float32 [M][n_samples]."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n_samples) * sigma
    x = delay_channels(s, xs, theta, fs)
    nstd = sigma * 10.0 ** (-snr_db / 20.0)
    x = x + rng.standard_normal(x.shape) * nstd
    return np.clip(x, -1.0, 1.0 - 2 ** -23).astype(np.float32)


def uca(M, radius):
    """Uniform circular array in the z = 0 plane, microphone m at angle 2 pi m / M from +x -> float64 [M][3] metres."""
    a = 2.0 * np.pi * np.arange(M) / M
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(M)], axis=1)


def unit_vector(azimuth, elevation=0.0):
    """e(theta, eps) = (sin theta cos eps, cos theta cos eps, sin eps): azimuth 0 is +y, +pi/2 is +x."""
    return np.array([np.sin(azimuth) * np.cos(elevation), np.cos(azimuth) * np.cos(elevation), np.sin(elevation)])


def delay_channels_xyz(s, xyz, azimuth, fs, elevation=0.0):
    """s [L] -> [M][L] with x_m(t) = s(t + (r_m . e)/c), e = unit_vector(azimuth, elevation) (circular over the stream).  A
    coordinate that is 0 adds no term: with y = z = 0 and elevation 0 these are the arrays of delay_channels."""
    L = len(s)
    S = np.fft.rfft(s)
    f = np.fft.rfftfreq(L, d=1.0 / fs)
    xyz = np.asarray(xyz, dtype=np.float64)
    ce = np.cos(elevation) if elevation != 0.0 else 1.0
    proj = xyz[:, 0] * np.sin(azimuth) * ce
    ny, nz = xyz[:, 1] != 0.0, xyz[:, 2] != 0.0
    proj[ny] += xyz[ny, 1] * (np.cos(azimuth) * ce)
    proj[nz] += xyz[nz, 2] * np.sin(elevation)
    adv = proj / C_SOUND  # seconds
    return np.fft.irfft(S[None, :] * np.exp(2j * np.pi * f[None, :] * adv[:, None]), n=L, axis=1)


def noise_source_stream_xyz(xyz, azimuth, fs, n_samples, seed, sigma=0.1, snr_db=20.0, elevation=0.0):
    """noise_source_stream for microphones at xyz [M][3] and a source at (azimuth, elevation); float32 [M][n_samples]."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n_samples) * sigma
    x = delay_channels_xyz(s, xyz, azimuth, fs, elevation)
    nstd = sigma * 10.0 ** (-snr_db / 20.0)
    x = x + rng.standard_normal(x.shape) * nstd
    return np.clip(x, -1.0, 1.0 - 2 ** -23).astype(np.float32)


def sine_stream(xs, theta, fs, n_samples, freq, amplitude=0.5, phase=0.0):
    """Pure tone from angle theta (the 'sine_f_1000_fs_48000' files of test/test_mcarray.cpp:403)."""
    t = np.arange(n_samples) / fs
    xs = np.asarray(xs, dtype=np.float64)
    adv = xs * np.sin(theta) / C_SOUND
    return (amplitude * np.cos(2 * np.pi * freq * (t[None, :] + adv[:, None]) + phase))


def tone16(n, magn, freq, phase=0.0):
    """wipp::tone(int16*, n, magn, freq, phase) stand-in [BUILD-DEFINES]: round(A cos(2 pi f n + phase))."""
    return np.round(magn * np.cos(2 * np.pi * freq * np.arange(n) + phase)).astype(np.int16)

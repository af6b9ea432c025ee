"""numpy twin of the kernels that turn the correlation map into DOA bins (csrc/kernels_stream.hip: k_scan_partial, k_scan_carry,
k_scan_pick, k_scan_repick<PL, false>, k_hist_settle): float32 with the kernels' operation order, restated from their source.
Pinned on the CPU by tests/test_scan_twin.py, compared bit for bit with the kernels by tests/test_gpu_scan_kernels.py.

Nothing here depends on PL (positions per lane of the peak pick): the kernels' answers may not either."""
from fractions import Fraction

import numpy as np

F = np.float32
SCAN_CHUNK, REPAIR_WARM, REPAIR_GROUP = 32, 16, 4
HIST_FRAMES, HIST_UNITS = REPAIR_WARM, REPAIR_WARM // REPAIR_GROUP
NO_FLAG = 0x7F7F7F7F
NEG0 = F(-0.0)
INF = F(np.inf)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def fma32(a, b, c):
    """RN_32(a * b + c) with one rounding.  a * b is exact in float64 (48 bits); the sum is rounded to odd in float64 (53 >= 2 * 24 + 2
    bits), so the final rounding to float32 is the rounding of the exact value."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                          # TwoSum: p + c = s + err exactly
    s = np.atleast_1d(s).copy()
    err = np.broadcast_to(err, s.shape)
    even = (s.view(np.int64) & 1) == 0
    fix = even & (err != 0) & np.isfinite(s)
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    out = s.astype(np.float32)
    return out.reshape(np.shape(p)) if np.ndim(p) else out[0]


def iir_step(mu, E, omu, c):
    return fma32(F(mu), E, f32(F(omu) * f32(c)))


def exact_reciprocal(d):
    """the float32 nearest 1 / d, from exact rational arithmetic"""
    x = Fraction(1) / Fraction(float(d))
    r0 = F(float(x))
    cands = [r0, np.nextafter(r0, F(0)), np.nextafter(r0, F(np.inf))]
    return min(cands, key=lambda r: abs(Fraction(float(r)) - x))


def normalised_energy(E, P):
    """(E - mn) / (30 P), mn = -15 P: the three-instruction quotient of the kernels"""
    mn = F(-15.0) * F(P)
    d = F(-2.0) * mn
    r = exact_reciprocal(d)
    x = f32(f32(E) - mn)
    q0 = f32(x * r)
    e = fma32(-q0, d, x)
    return fma32(e, r, q0)


def plane_sum(C, order=None):
    """C [planes][...]: plane 0 first, in order"""
    idx = list(range(C.shape[0])) if order is None else list(order)
    v = f32(C[idx[0]]).copy()
    for pl in idx[1:]:
        v = f32(v + C[pl])
    return v


def chunk_scan(Cs, voiced, mu, omu, chunk=SCAN_CHUNK):
    """Cs [n_frames][D] (planes summed), voiced [n_frames] or None -> part [n_chunks][D] (the recursion from zero inside each chunk), nv [n_chunks]"""
    n, D = Cs.shape
    nc = (n + chunk - 1) // chunk
    part, nv = np.zeros((nc, D), np.float32), np.zeros(nc, np.int32)
    for c in range(nc):
        b = np.zeros(D, np.float32)
        for t in range(c * chunk, min((c + 1) * chunk, n)):
            if voiced is None or voiced[t]:
                b = iir_step(mu, b, omu, Cs[t])
                nv[c] += 1
        part[c] = b
    return part, nv


def mu_pow(mu, n):
    g = F(1.0)
    for _ in range(n):
        g = F(g * F(mu))
    return g


def compose(g, E, b, fused):
    """g * E + b as the source writes it; contraction is the compiler's choice"""
    return fma32(g, E, b) if fused else f32(f32(F(g) * f32(E)) + f32(b))


def carry(part, nv, state_in, mu, fused):
    """k_scan_carry: e_start [n_chunks][D], state_out [D]"""
    E = f32(state_in).copy()
    e_start = np.zeros_like(part)
    for c in range(part.shape[0]):
        e_start[c] = E
        E = compose(mu_pow(mu, int(nv[c])), E, part[c], fused)
    return e_start, E


def lookback(part, state_in, mu, fused, chunk=SCAN_CHUNK, depth=4):
    """the start values k_scan_pick composes itself: cut off `depth` chunks back, or at the state at entry"""
    g = mu_pow(mu, chunk)
    e_start = np.zeros_like(part)
    for c in range(part.shape[0]):
        j0 = max(0, c - depth)
        E = f32(state_in).copy() if j0 == 0 else np.zeros(part.shape[1], np.float32)
        for j in range(j0, c):
            E = compose(g, E, part[j], fused)
        e_start[c] = E
    return e_start


def run_chunks(Cs, voiced, e_start, mu, omu, chunk=SCAN_CHUNK):
    """every chunk from its start value: energy [n_frames][D] (E after each frame); the last row is the state a look-back pick leaves"""
    n, D = Cs.shape
    energy = np.zeros((n, D), np.float32)
    for c in range(e_start.shape[0]):
        E = f32(e_start[c]).copy()
        for t in range(c * chunk, min((c + 1) * chunk, n)):
            if voiced is None or voiced[t]:
                E = iir_step(mu, E, omu, Cs[t])
            energy[t] = E
    return energy


# ---- selectDOA of one frame ----------------------------------------------------------------------------------------------------------
def _chain(En):
    """df [D - 1], the median-filtered sign chain at positions 0 .. D - 2 (edges replicated), sd [D - 2]"""
    En = f32(En)
    D = En.shape[0]
    df = f32(En[1:] - En[:-1])
    fd = (df < 0).astype(np.float32)
    pad = np.concatenate([fd[:1], fd, fd[-1:]])
    md = np.sort(np.stack([pad[:-2], pad[1:-1], pad[2:]]), axis=0)[1]            # position p: fd[p - 1], fd[p], fd[p + 1]
    sd = f32(f32(md[1:] - md[:-1]) * En[1:D - 1]) + NEG0                         # (+ the penalty's -0 of the positions that stay)
    return df, md, f32(sd)


def _picks(sd, S):
    sd = sd.copy()
    bins, vals = [], []
    for _ in range(S):
        i = int(np.flatnonzero(sd == sd.max())[0])                               # first index on ties
        bins.append(i + 1)
        vals.append(sd[i])
        sd[i] = F(0.0)
    return bins, vals, sd


def pick(En, S):
    """-> bins [S] (maxIdx + 1), vals [S] float32"""
    _, _, sd = _chain(En)
    bins, vals, _ = _picks(sd, S)
    return np.array(bins, np.int32), np.array(vals, np.float32)


def sens(En, S, tau, drop=None):
    """could the picks come out differently on a map within tau / 2 of this one (wave_pick_pl<true>)?  drop: leave one of the four
    clauses out ('order', 'runner', 'uncertain', 'zero') -- the mutants tests/test_scan_twin.py shows to be unsound"""
    En, tau = f32(En), F(tau)
    D = En.shape[0]
    df, md, sd = _chain(En)
    adf = np.abs(df)
    pos = np.arange(D - 2)
    dmin = np.minimum.reduce([adf[np.clip(pos - 1 + k, 0, D - 2)] for k in range(4)])
    aE = np.abs(En[1:D - 1])
    unc = dmin <= tau
    umax = aE[unc].max() if unc.any() else -INF
    step = md[1:] != md[:-1]
    zmin = aE[step].min() if step.any() else INF
    bins, vals, rest = _picks(sd, S)
    out = False
    for s in range(1, S):
        if drop != "order" and vals[s - 1] > 0 and F(vals[s - 1] - vals[s]) <= tau:
            out = True
    v_last = vals[-1]
    if drop != "runner" and v_last > 0 and F(v_last - rest.max()) <= tau:
        out = True
    if drop != "uncertain" and ((umax >= F(v_last - tau)) if v_last > 0 else (umax > -INF)):
        out = True
    if drop != "zero" and v_last <= tau and zmin <= tau:
        out = True
    return out


def candidates(En, tau, full=False):
    """the candidate columns of a flagged frame for one source (wave_candidates) -> (mask [D] bool, every column taken)"""
    En, tau = f32(En), F(tau)
    D = En.shape[0]
    if not full:
        df = f32(En[1:] - En[:-1])
        neg, unc = df < 0, np.abs(df) <= tau
        lo, hi = neg & ~unc, neg | unc

        def filt(x, p):                                                          # median of three at position p, edges replicated
            j = np.clip([p - 1, p, p + 1], 0, D - 2)
            return int(x[j].sum()) >= 2
        vcert = -INF
        for dd in range(D - 2):
            is_open = not filt(hi, dd)                                           # pinned to "rising"
            mn = INF
            for g in range(1, 4):
                mn = min(mn, En[min(dd + g, D - 1)])
                down, up = filt(lo, dd + g), not filt(hi, dd + g)
                if is_open and down and dd + g - 1 < D - 2:
                    vcert = max(vcert, mn)
                if down or up:
                    is_open = False
        if not vcert > F(2.0) * tau:
            full = True
        thr = F(vcert - tau)
    mask = np.zeros(D, bool)
    if full:
        mask[:] = True
        return mask, True
    for dd in range(D - 2):
        if abs(En[dd + 1]) >= thr:
            mask[max(dd - 1, 0):min(dd + 3, D - 1) + 1] = True
    return mask, False


# ---- the coarse pass: flags and the repair plan ------------------------------------------------------------------------------------
def unit_of(r, a, gpa, hist_base):
    return a * gpa + r // REPAIR_GROUP if r >= 0 else hist_base + a * HIST_UNITS + (HIST_FRAMES + r) // REPAIR_GROUP


def flags_of(En_rows, voiced, unsure, S, tau, lazy=False):
    """En_rows [n_frames][D] of ONE array -> flags [n_frames], forced frame or -1"""
    n = En_rows.shape[0]
    adv = [t for t in range(n) if voiced is None or voiced[t]]
    t_force = adv[-1] if adv and not lazy else -1
    fl = np.zeros(n, np.uint8)
    for t in adv:
        uns = unsure is not None and any(unsure[u] for u in range(max(t - 6, 0), t + 1))
        if t == t_force or uns or sens(En_rows[t], S, tau):
            fl[t] = 1
    return fl, t_force


def plan_rows(flags, voiced, a, gpa, hist_base, hist_valid, chunk=SCAN_CHUNK):
    """whole rows (and every gated call), one array: -> set of units, {chunk: chunk_from}"""
    units, cfrom = set(), {}
    u_lo = -HIST_FRAMES if hist_valid and voiced is None else 0
    for t in np.flatnonzero(flags):
        rows, u = [], int(t)
        while u >= u_lo and len(rows) < REPAIR_WARM + 1:
            if u < 0 or voiced is None or voiced[u]:
                rows.append(u)
            u -= 1
        units |= {unit_of(r, a, gpa, hist_base) for r in rows}
        cf = -1 if min(rows) < 0 else min(rows) // chunk
        c = int(t) // chunk
        cfrom[c] = min(cfrom.get(c, NO_FLAG), cf)
    return units, cfrom


def plan_cand(flags, masks, dead, a, gpa, hist_base, hist_valid, chunk=SCAN_CHUNK):
    """candidate columns (ungated), one array.  masks: {t: bool [D]} of the flagged frames -> {unit: bool [D]} of the units listed,
    {chunk: chunk_from}.  A chunk lists a unit if a row of one of its flagged frames' ranges in it is not dead; the unit then takes the
    columns of every flagged frame of that chunk whose range covers it."""
    out, cfrom = {}, {}
    u_lo = -HIST_FRAMES if hist_valid else 0
    n = flags.shape[0]
    for c in range((n + chunk - 1) // chunk):
        ts = [t for t in range(c * chunk, min((c + 1) * chunk, n)) if flags[t]]
        needed, um = set(), {}
        for t in ts:
            r_lo = max(t - REPAIR_WARM, u_lo)
            for r in range(r_lo, t + 1):
                e = unit_of(r, a, gpa, hist_base)
                um[e] = um.get(e, False) | masks[t]
                if not (dead is not None and r >= 0 and dead[r]):
                    needed.add(e)
            cf = -1 if r_lo < 0 else r_lo // chunk
            cfrom[c] = min(cfrom.get(c, NO_FLAG), cf)
        for e in needed:
            out[e] = out.get(e, False) | um[e]
    return out, cfrom


def repick(Cs, voiced, flags, e_start, chunk, c_from, mu, omu, P, S, hist=None, chunk_len=SCAN_CHUNK):
    """the second pick of one listed chunk of one array on the patched map Cs [n_frames][D]: the recursion restarts at the start value of
    chunk c_from (-1: from hist = (e_hist [D], hist_C [HIST_FRAMES][D])) -> {t: (bins, vals)} of the chunk's flagged frames,
    energy rows {t: [D]} of the chunk, the state behind the chunk's last frame"""
    n = Cs.shape[0]
    t0, t1 = chunk * chunk_len, min((chunk + 1) * chunk_len, n)
    if c_from < 0:
        E = f32(hist[0]).copy()
        for j in range(HIST_FRAMES):
            E = iir_step(mu, E, omu, hist[1][j])
        start = 0
    else:
        E = f32(e_start[c_from]).copy()
        start = c_from * chunk_len
    picks, rows = {}, {}
    for t in range(start, t1):
        if voiced is None or voiced[t]:
            E = iir_step(mu, E, omu, Cs[t])
        if t >= t0:
            rows[t] = E.copy()
            if flags[t]:
                picks[t] = pick(normalised_energy(E, P), S)
    return picks, rows, E


def select_doa_f64(En, S):
    """selectDOA (SteeringBeamforming.cpp:158-194) in plain float64 on the given normalised energies, loops and all"""
    x = [float(v) for v in En]
    D = len(x)
    fd = [1.0 if x[j + 1] - x[j] < 0.0 else 0.0 for j in range(D - 1)]
    filt = []
    for j in range(D - 1):
        w = sorted([fd[max(j - 1, 0)], fd[j], fd[min(j + 1, D - 2)]])
        filt.append(w[1])
    sd = [(filt[j + 1] - filt[j]) * x[j + 1] for j in range(D - 2)]
    bins, vals = [], []
    for _ in range(S):
        m, mi = sd[0], 0
        for j in range(1, D - 2):
            if sd[j] > m:
                m, mi = sd[j], j
        sd[mi] = 0.0
        bins.append(mi + 1)
        vals.append(m)
    return bins, vals

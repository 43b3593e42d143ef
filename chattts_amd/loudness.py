"""Loudness normalisation, the host side: ITU-R BS.1770-4 integrated loudness of packed float32 segments and ONE gain per group
(csrc/loudness.hip is the device side; nothing here touches the GPU).  The definition, once:

  K-weighting  two biquads in cascade, zero initial state, float64 coefficients by the bilinear forms libebur128 and pyloudnorm use
               (`coefficients`): a high shelf (f0 1681.97 Hz, +4 dB) and a high-pass (f0 38.14 Hz).
  blocks       H = fs / 10 samples is a 100 ms sub-block, e_j the filtered signal's sum of squares over sub-block j < n // H.  Gating
               block i is sub-blocks i .. i + 3: z_i = (e_i + .. + e_{i+3}) / (4 H), l_i = -0.691 + 10 log10 z_i.  A segment with
               fewer than 4 complete sub-blocks contributes ONE block, the mean square over all its n samples.
  gates        keep l_i > -70;  G = -0.691 + 10 log10(mean z over kept) - 10;  keep l_i > G as well;  L = -0.691 + 10 log10(mean z over
               those).  No block past the absolute gate: the group is silent, L = -inf and the gain is exactly 1.
  groups       segments grp[g] .. grp[g+1]-1 (a split_text request's sentences) get ONE loudness and ONE gain: each sentence is filtered
               alone, blocks never span sentences, the gates run over the union of the group's blocks, the peak is the group's peak.
  gain         g = min(10^((target - L) / 20), 10^(MAX_GAIN_DB / 20), CEILING / peak) in float64, rounded once to float32;
               y = float32(g) * x, one rounding per sample.  No dither.  A group that goes through the look-ahead peak limiter
               (limiter.py) drops the ceiling term: the limiter runs behind the gain and holds the ceiling sample by sample.

The recurrence is computed exactly and in parallel.  The cascade is the linear system s' = A s + B x, y = C s + D x (`step` is its one
sample, transposed direct form II, and `homogeneous` probes A^i and h_i = C A^i from it), so a tile of one sub-block runs from zero state
(outputs y0_i, end state z), the true entry states follow from s_{j+1} = A^H s_j + z_j, and a tile's energy under its true entry state
s is  sum (y0_i + h_i . s)^2 = sum y0_i^2 + 2 s . (sum y0_i h_i) + s^T M s,  M = sum h_i h_i^T.  `sub_block_energies` is that route in
NumPy float64, the twin of the kernels; against a serial filter it agrees to about 1e-12 relative."""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

MAX_GAIN_DB = 30.0
CEILING = 10.0 ** (-1.0 / 20.0)                 # -1 dBFS sample peak
ABS_GATE = -70.0
OFFSET = -0.691
FS_MIN, FS_MAX = 8000, 48000
TARGET_MIN, TARGET_MAX = -40.0, -5.0
H_MIN, H_MAX = FS_MIN // 10, FS_MAX // 10      # LN_HMIN / LN_HMAX of csrc/kernels.hpp
LANES = 64                                      # a tile's chunks: lane l of a wave runs samples [l c, (l + 1) c), c = `chunk(H)`
ROW = 1072                                      # float64 per rate of the coefficient table (LN_ROW): see `rate_row`
REC = 20                                        # float64 per tile of the scratch (LN_REC)
BOUND_NONE, BOUND_TARGET, BOUND_CAP, BOUND_CEILING = -1, 0, 1, 2

# one record per group (32 bytes, csrc/loudness.hip LnStats)
STATS = np.dtype([("L", "<f8"), ("peak", "<f4"), ("g32", "<f4"), ("n_blocks", "<i4"), ("n_abs", "<i4"), ("n_rel", "<i4"), ("bound", "<i4")])


def check_rate(fs) -> int:
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or fs % 10 != 0 or not FS_MIN <= fs <= FS_MAX:
        raise ValueError(f"loudness: the rate is an integer number of Hz, a multiple of 10 in {FS_MIN} .. {FS_MAX} (got {fs!r})")
    return int(fs)


def check_target(target):
    """None (leave the group alone) or a number of LUFS in [-40, -5] -> None or float"""
    if target is None:
        return None
    if isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)) or not TARGET_MIN <= float(target) <= TARGET_MAX:
        raise ValueError(f"loudness: the target is a number of LUFS in {TARGET_MIN:g} .. {TARGET_MAX:g}, or None (got {target!r})")
    return float(target)


def per_row(loudness, n: int, who: str = "loudness"):
    """one target or one per row -> a checked list of n (entries None or float); None when nothing is asked for"""
    if loudness is None:
        return None
    vals = [loudness] * n if np.ndim(loudness) == 0 else list(loudness)
    if len(vals) != n:
        raise ValueError(f"{who}: one loudness target per row, or one for all")
    vals = [check_target(v) for v in vals]
    return None if all(v is None for v in vals) else vals


def chunk(H: int) -> int:
    """the samples a lane runs of a tile of H: ceil(H / 64), made odd (the lanes' LDS reads at that stride then hit 32 different banks)"""
    return -(-H // LANES) | 1


def coefficients(fs):
    """(b_shelf, a_shelf, b_highpass, a_highpass) of the K-weighting at rate fs, float64"""
    fs = check_rate(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def _k10(fs) -> np.ndarray:
    b1, a1, b2, a2 = coefficients(fs)
    return np.array([b1[0], b1[1], b1[2], a1[1], a1[2], b2[0], b2[1], b2[2], a2[1], a2[2]])


def step(k, x, s):
    """one sample of the cascade, transposed direct form II (ln_step of csrc/loudness.hip): k the 10 coefficients, x the input, s the
    four states (scalars or arrays, updated in place when a list) -> the output"""
    y1 = k[0] * x + s[0]
    s[0] = k[1] * x - k[3] * y1 + s[1]
    s[1] = k[2] * x - k[4] * y1
    y2 = k[5] * y1 + s[2]
    s[2] = k[6] * y1 - k[8] * y2 + s[3]
    s[3] = k[7] * y1 - k[9] * y2
    return y2


@lru_cache(maxsize=None)
def homogeneous(fs: int, steps: int):
    """the system without input from the four unit states: (h [steps, 4], P [steps + 1, 4, 4]) with h[i] = C A^i and P[i] = A^i"""
    k = _k10(fs)
    s = [np.array([1.0, 0, 0, 0]), np.array([0, 1.0, 0, 0]), np.array([0, 0, 1.0, 0]), np.array([0, 0, 0, 1.0])]   # s[r][unit state]
    h = np.empty((steps, 4))
    P = np.empty((steps + 1, 4, 4))
    P[0] = np.array(s)
    for i in range(steps):
        h[i] = step(k, 0.0, s)
        P[i + 1] = np.array(s)
    return h, P


def _tri(M: np.ndarray) -> np.ndarray:
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[0, 3], M[1, 1], M[1, 2], M[1, 3], M[2, 2], M[2, 3], M[3, 3]])


@lru_cache(maxsize=None)
def rate_row(fs: int) -> np.ndarray:
    """the coefficient table's row for rate fs, float64 [ROW]:  [0] H  [1] c  [2, 12) the 10 filter coefficients  [16, 32) A^H row-major
    [32, 42) M = sum_{i<H} h_i h_i^T (upper triangle, row-major)  [48, 48 + 64 * 16) A^(l c), l = 0 .. 63 (the entry of lane l's chunk; A^(c 2^k)
    for the lanes' scan are among them)"""
    fs = check_rate(fs)
    H = fs // 10
    c = chunk(H)
    h, P = homogeneous(fs, max(H, (LANES - 1) * c))
    row = np.zeros(ROW)
    row[0], row[1] = H, c
    row[2:12] = _k10(fs)
    row[16:32] = P[H].reshape(-1)
    row[32:42] = _tri(h[:H].T @ h[:H])
    row[48:] = P[np.arange(LANES) * c].reshape(-1)
    return row


def coef_table(rates):
    """the distinct rates of a call -> (float64 [n_rates, ROW] table, {rate: row index})"""
    uniq = sorted({check_rate(r) for r in rates})
    return np.ascontiguousarray(np.stack([rate_row(r) for r in uniq])), {r: i for i, r in enumerate(uniq)}


def sub_block_energies(x: np.ndarray, fs: int):
    """the filtered segment's energy per tile of H samples (the last tile may be partial), by the tile route -> float64 [ceil(n / H)]"""
    fs = check_rate(fs)
    x = np.asarray(x, dtype=np.float64)
    n, H = len(x), fs // 10
    nt = -(-n // H)
    k = _k10(fs)
    h, P = homogeneous(fs, max(H, (LANES - 1) * chunk(H)))
    pad = np.zeros(nt * H)
    pad[:n] = x
    tiles = pad.reshape(nt, H)
    s = [np.zeros(nt) for _ in range(4)]
    y0 = np.empty((nt, H))
    z = np.empty((nt, 4))
    r = n - (nt - 1) * H                            # the last tile's length
    for i in range(H):
        y0[:, i] = step(k, tiles[:, i], s)
        if i == r - 1:
            z[-1] = [v[-1] for v in s]
    z[:-1] = np.array(s).T[:-1]
    y0[-1, r:] = 0.0
    e0 = (y0 * y0).sum(1)
    v = y0 @ h[:H]                                  # the padded tail of y0 is zero
    M = h[:H].T @ h[:H]
    Mr = h[:r].T @ h[:r]
    e = np.empty(nt)
    st = np.zeros(4)
    for j in range(nt):
        Mj = M if j < nt - 1 or r == H else Mr
        e[j] = e0[j] + 2.0 * (st @ v[j]) + st @ Mj @ st
        st = P[H] @ st + z[j]
    return e


def blocks(x: np.ndarray, fs: int) -> np.ndarray:
    """the gating blocks' mean squares z_i of one segment"""
    e = sub_block_energies(x, fs)
    n, H = len(x), fs // 10
    nb = n // H
    if nb < 4:
        return np.array([e.sum() / n])
    return (e[0:nb - 3] + e[1:nb - 2] + e[2:nb - 1] + e[3:nb]) / (4.0 * H)


def gate(z: np.ndarray):
    """both gates over a group's blocks -> (L, n_blocks, n_abs, n_rel)"""
    with np.errstate(divide="ignore"):
        l = OFFSET + 10.0 * np.log10(z)
    keep = l > ABS_GATE
    if not keep.any():
        return -math.inf, len(z), 0, 0
    rel = OFFSET + 10.0 * math.log10(z[keep].mean()) - 10.0
    keep2 = keep & (l > rel)
    return OFFSET + 10.0 * math.log10(z[keep2].mean()), len(z), int(keep.sum()), int(keep2.sum())


def gain(L: float, peak: float, target, limiter: bool = False):
    """(float32 gain, which term bound): target None or a silent group -> (1, BOUND_NONE).  `limiter`: the group goes through the
    peak limiter behind this stage (limiter.py), which enforces the ceiling, so the ceiling term is dropped: bound is 0 or 1"""
    if target is None or L == -math.inf:
        return np.float32(1.0), BOUND_NONE
    terms = [10.0 ** ((target - L) / 20.0), 10.0 ** (MAX_GAIN_DB / 20.0)] + ([] if limiter else [CEILING / float(peak)])
    b = int(np.argmin(terms))
    return np.float32(terms[b]), b


def tables(n_total: int, offsets=None, groups=None, rates=None, targets=None):
    """every table of a call, checked: (off int64 [n_seg + 1], grp int32 [n_grp + 1], rates list [n_seg], targets list [n_grp] of None or
    float).  ValueError: what ctts_loudness_normalize_ragged would refuse, before anything is uploaded."""
    off = np.array([0, n_total], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or np.any(np.diff(off) <= 0):
        raise ValueError("loudness: the offsets ascend from 0 and no segment is empty")
    if int(off[-1]) != n_total:
        raise ValueError("loudness: the offsets do not cover the tensor")
    if n_total >= (1 << 31) - 4096:
        raise ValueError("loudness: the pack holds 2^31 - 4096 samples or more")
    n_seg = len(off) - 1
    if n_seg > 65535:
        raise ValueError("loudness: more than 65535 segments")
    grp = np.arange(n_seg + 1, dtype=np.int32) if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    if grp.ndim != 1 or len(grp) < 2 or grp[0] != 0 or grp[-1] != n_seg or np.any(np.diff(grp) <= 0):
        raise ValueError("loudness: the group table runs from 0 to the number of segments, ascending, and no group is empty")
    n_grp = len(grp) - 1
    if rates is None:
        rates = [24000] * n_seg
    elif np.ndim(rates) == 0:
        rates = [rates] * n_seg
    rates = [check_rate(r) for r in rates]
    if len(rates) != n_seg:
        raise ValueError("loudness: one rate per segment, or one for all")
    tg = [targets] * n_grp if targets is None or np.ndim(targets) == 0 else list(targets)
    if len(tg) != n_grp:
        raise ValueError("loudness: one target per group, or one for all")
    return off, grp, rates, [check_target(t) for t in tg]


def normalize(x: np.ndarray, target, offsets=None, groups=None, rates=None, limiter=None):
    """the NumPy twin of CodecEngine.loudness_normalize on a host array -> (y float32, stats STATS [n_grp]); with `limiter` (one
    bool, or one per group) also the limiter's records (limiter.STATS [n_seg]; a segment outside a flagged group has g32 = 0 there):
    a flagged group's gain drops the ceiling term and every one of its segments goes through limiter.limit_segment alone at it"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    off, grp, rates, tg = tables(len(x), offsets, groups, rates, target)
    y = np.empty_like(x)
    stats = np.zeros(len(grp) - 1, dtype=STATS)
    lim = lstats = None
    if limiter is not None:
        from . import limiter as LM
        lim = LM.per_row(limiter, len(grp) - 1, "loudness") or [False] * (len(grp) - 1)
        lstats = np.zeros(len(off) - 1, dtype=LM.STATS)
    for g in range(len(grp) - 1):
        a, b = int(grp[g]), int(grp[g + 1])
        z = np.concatenate([blocks(x[off[s]: off[s + 1]], rates[s]) for s in range(a, b)])
        L, nb, na, nr = gate(z)
        xs = x[off[a]: off[b]]
        peak = np.abs(xs).max()
        g32, bound = gain(L, peak, tg[g], bool(lim and lim[g]))
        stats[g] = (L, peak, g32, nb, na, nr, bound)
        if lim and lim[g]:
            for s in range(a, b):
                y[off[s]: off[s + 1]], lstats[s] = LM.limit_segment(x[off[s]: off[s + 1]], rates[s], g32)
        else:
            y[off[a]: off[b]] = g32 * xs
    return (y, stats) if limiter is None else (y, stats, lstats)

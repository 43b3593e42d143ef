"""An independent float64 reference for the loudness tests: ITU-R BS.1770-4 integrated loudness by a straight serial direct-form loop per
sample, with its own coefficient, block, gate and gain code.  Plain NumPy and the standard library only; it shares no function with
chattts_amd/loudness.py."""
import math

import numpy as np


def _biquad_serial(b, a, x):
    """direct form I, one sample after the other"""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for i, v in enumerate(x):
        o = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1 = x1, v
        y2, y1 = y1, o
        y[i] = o
    return y


def k_coefficients(fs):
    def poles(f0, q):
        k = math.tan(math.pi * f0 / fs)
        a0 = 1.0 + k / q + k * k
        return k, a0, [1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]

    q = 0.7071752369554196
    k, a0, a_sh = poles(1681.974450955533, q)
    vh = math.pow(10.0, 3.999843853973347 / 20.0)
    vb = math.pow(vh, 0.4996667741545416)
    b_sh = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0]
    _, _, a_hp = poles(38.13547087602444, 0.5003270373238773)
    return b_sh, a_sh, [1.0, -2.0, 1.0], a_hp


def k_weight(x, fs):
    b_sh, a_sh, b_hp, a_hp = k_coefficients(fs)
    xs = [float(v) for v in np.asarray(x, dtype=np.float64)]
    return np.array(_biquad_serial(b_hp, a_hp, _biquad_serial(b_sh, a_sh, xs)), dtype=np.float64)


def segment_blocks(x, fs):
    """mean squares of the gating blocks of one segment (400 ms, 75 % overlap; a short segment: one block over all of it)"""
    y = k_weight(x, fs)
    hop = fs // 10
    full = len(y) // hop
    if full < 4:
        return [float(np.dot(y, y)) / len(y)]
    sub = [float(np.dot(y[j * hop:(j + 1) * hop], y[j * hop:(j + 1) * hop])) for j in range(full)]
    return [(sub[i] + sub[i + 1] + sub[i + 2] + sub[i + 3]) / (4.0 * hop) for i in range(full - 3)]


def _lu(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def integrated(block_ms):
    """-> dict(L, n_blocks, n_abs, n_rel, margin): margin is the smallest distance in LU of any block from either gate (inf without one)"""
    levels = [_lu(z) for z in block_ms]
    margin = min([abs(l + 70.0) for l in levels if l > -math.inf], default=math.inf)
    first = [z for z, l in zip(block_ms, levels) if l > -70.0]
    if not first:
        return dict(L=-math.inf, n_blocks=len(block_ms), n_abs=0, n_rel=0, margin=margin)
    gate = _lu(sum(first) / len(first)) - 10.0
    margin = min([margin] + [abs(l - gate) for l in levels if l > -math.inf])
    second = [z for z, l in zip(block_ms, levels) if l > -70.0 and l > gate]
    return dict(L=_lu(sum(second) / len(second)), n_blocks=len(block_ms), n_abs=len(first), n_rel=len(second), margin=margin)


def group(segments, rates, target):
    """one group: its segments (float32 arrays) at their rates -> integrated(..) plus peak, g (float64; 1 for a silent group or no target)
    and bound (0 target, 1 the +30 dB cap, 2 the -1 dBFS ceiling, -1 none)"""
    ms = []
    for x, fs in zip(segments, rates):
        ms += segment_blocks(x, fs)
    return finish(ms, max(float(np.abs(x).max()) for x in segments), target)


def finish(block_ms, peak, target):
    """`group` from the group's blocks (every segment's `segment_blocks`, in order) and its peak"""
    r = integrated(list(block_ms))
    r["peak"] = peak
    r["g"], r["bound"] = 1.0, -1
    if target is not None and r["n_abs"] > 0:
        terms = [math.pow(10.0, (target - r["L"]) / 20.0), math.pow(10.0, 30.0 / 20.0), math.pow(10.0, -1.0 / 20.0) / r["peak"]]
        r["g"] = min(terms)
        r["bound"] = terms.index(r["g"])
    return r

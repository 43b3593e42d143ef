"""A float64 oracle of the time scaler, written from the formulas alone; it shares no code with chattts_amd.timescale.

Waveform-similarity overlap-add with window 1024, synthesis hop 512, search radius 256 and the periodic Hann window.  For speed
num / 100 and a segment x of n samples (zero outside [0, n)):
    n_out = ceil(100 n / num),  F = ceil(n_out / 512) + 1,  a_k = floor(512 k num / 100),  s_0 = -512
    k >= 1:  t[j] = x[s_{k-1} + 512 + j],  c(d) = sum_{j<1024} t[j] x[a_k - 512 + d + j],  -256 <= d < 256
             d_k = arg max c (ties: the smallest |d|, then the negative one),  s_k = a_k - 512 + d_k
    y[512 (k-1) + j] = w[j + 512] x[s_{k-1} + 512 + j] + w[j] x[s_k + j]
Besides the path and the samples the oracle returns, per frame, how safely the search's winner leads: the margin ratio
    min over d' != d_k of (c(d_k) - c(d')) / (b(d_k) + b(d')),     b(d) = 1026 * 2^-24 * sum_j |t[j]| |x[a_k - 512 + d + j]|
b is the float32 dot-product bound of 1024 terms, so above 1 a float32 search picks the same d in any summation order.  A frame whose
products are all zero is exact under the tie rule (d = 0); its ratio is reported as infinity and `zero_frame` is set."""
import numpy as np

WIN, HOP, RAD = 1024, 512, 256


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)


def _read(x, start, count):
    """x[start .. start + count) with zeros outside the segment"""
    out = np.zeros(count, dtype=np.float64)
    lo, hi = max(start, 0), min(start + count, x.shape[0])
    if lo < hi:
        out[lo - start: hi - start] = x[lo: hi]
    return out


def time_scale_f64(x, speed):
    """-> dict(y float64 [n_out], path int64 [F], ratio float64 [F] (ratio[0] = inf: frame 0 is not searched), zero_frame bool [F],
    xa / xb float64 [n_out]: the two samples behind every output (for the per-sample bound))"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    num = int(round(100 * float(speed)))
    assert n >= 1 and 50 <= num <= 200
    n_out = (100 * n + num - 1) // num
    F = (n_out + HOP - 1) // HOP + 1
    w = hann()
    path = np.zeros(F, dtype=np.int64)
    path[0] = -HOP
    ratio = np.full(F, np.inf)
    zero_frame = np.zeros(F, dtype=bool)
    cand = np.arange(-RAD, RAD)
    for k in range(1, F):
        a = (k * HOP * num) // 100
        t = _read(x, int(path[k - 1]) + HOP, WIN)
        span = _read(x, a - HOP - RAD, 2 * RAD + WIN - 1)
        rows = np.lib.stride_tricks.sliding_window_view(span, WIN)        # [512, 1024]: row i is candidate d = i - 256
        c = rows @ t
        top = c.max()
        tied = cand[c == top]
        tied = tied[np.abs(tied) == np.abs(tied).min()]
        d = int(tied.min())                                              # the negative one of +-|d|
        path[k] = a - HOP + d
        b = (WIN + 2) * 2.0 ** -24 * (np.abs(rows) @ np.abs(t))
        if not b.any():
            zero_frame[k] = True
            assert d == 0
            continue
        i = d + RAD
        others = np.arange(2 * RAD) != i
        den = b[i] + b[others]
        gap = c[i] - c[others]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(den > 0, gap / den, np.where(gap > 0, np.inf, 0.0))
        ratio[k] = r.min()
    m = np.arange(n_out)
    k1, j = m // HOP, m % HOP
    xa = np.array([0.0 if not 0 <= g < n else x[g] for g in path[k1] + HOP + j])
    xb = np.array([0.0 if not 0 <= g < n else x[g] for g in path[k1 + 1] + j])
    return dict(y=w[j + HOP] * xa + w[j] * xb, path=path, ratio=ratio, zero_frame=zero_frame, xa=xa, xb=xb, w_a=w[j + HOP], w_b=w[j])

"""float64 NumPy oracle of the device resampler, written from the filter's formulas alone (it shares no code with chattts_amd.resample):
    base = min(orig, new) * 0.99, width = ceil(6 orig / base), K = 2 width + orig            (orig, new: the rates over their gcd)
    h[i][k] = (base / orig) cos^2(pi t / 12) sinc(t),  t = clamp(((k - width) / orig - i / new) base, -6, 6)
    y[j new + i] = sum_k h[i][k] x[j orig + k - width],  x = 0 outside the signal;  ceil(n new / orig) samples out"""
import math

import numpy as np

PAIRS = [(24000, 8000), (24000, 16000), (24000, 48000), (24000, 44100), (44100, 24000), (16000, 24000), (48000, 24000)]


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def oracle_taps(orig, new):
    """(h float64 [new, K], width) for the REDUCED pair"""
    orig, new = reduced(orig, new)
    base = min(orig, new) * 0.99
    width = int(math.ceil(6 * orig / base))
    K = 2 * width + orig
    h = np.zeros((new, K), np.float64)
    for i in range(new):
        for k in range(K):
            t = min(6.0, max(-6.0, ((k - width) / orig - i / new) * base))
            sinc = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[i, k] = (base / orig) * math.cos(math.pi * t / 12) ** 2 * sinc
    return h, width


_TAPS = {}


def resample_f64(x, orig, new, with_bound=False):
    """x [n] -> y float64 [ceil(n new / orig)]; with_bound: also a[o] = sum_k |h[i][k]| |x[.]|, the scale of output o's rounding bound"""
    key = reduced(orig, new)
    if key not in _TAPS:
        _TAPS[key] = oracle_taps(orig, new)
    h, width = _TAPS[key]
    M, L = key
    K = h.shape[1]
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    n_out = (n * L + M - 1) // M
    J = (n_out + L - 1) // L
    xp = np.zeros(max((J - 1) * M + K, width + n), np.float64)
    xp[width: width + n] = x
    frames = np.lib.stride_tricks.sliding_window_view(xp, K)[:: M][:J]          # [J, K]: frames[j][k] = x[j M + k - width]
    y = (frames @ h.T).reshape(-1)[:n_out]
    if with_bound:
        return y, (np.abs(frames) @ np.abs(h).T).reshape(-1)[:n_out]
    return y

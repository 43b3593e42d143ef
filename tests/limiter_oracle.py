"""An independent restatement of the look-ahead peak limiter (chattts_amd/limiter.py holds the definition): brute force, every window
spelled out with `sliding_window_view`, no code shared with the twin or the device.  Slow and obvious on purpose."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

CEILING32 = np.float32(10.0 ** (-1.0 / 20.0))
THRESHOLD = np.float32(CEILING32 * np.float32(1.0 - 2.0 ** -22))


def stages(x, fs=None, g32=1.0, W=None):
    """one segment -> dict of u, r, m (positions -W .. n + W - 1), s, y and the record's fields"""
    W = fs // 100 if W is None else W
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    u = np.empty(n, np.float32)
    r = np.empty(n, np.float32)
    for i in range(n):
        u[i] = np.float32(g32) * x[i]
        a = np.abs(u[i])
        r[i] = THRESHOLD / a if a > THRESHOLD else np.float32(1.0)          # a NaN compares false: r = 1
    # silence outside the segment needs no gain: r = 1 there; position j of m looks at r[j - W .. j + W]
    padded = np.concatenate([np.ones(2 * W, np.float32), r, np.ones(2 * W, np.float32)])
    m = sliding_window_view(padded, 2 * W + 1).min(axis=1)                   # n + 2 W values: j = -W .. n + W - 1
    assert len(m) == n + 2 * W
    S = sliding_window_view(m.astype(np.float64), 2 * W + 1).sum(axis=1)     # n values
    assert len(S) == n
    s = (S / np.float64(2 * W + 1)).astype(np.float32)
    y = s * u
    return {"u": u, "r": r, "m": m, "s": s, "y": y, "g32": np.float32(g32), "min_gain": s.min(), "n_over": int(np.sum(np.abs(u) > THRESHOLD)),
            "n_touched": int(np.sum(s < np.float32(1.0)))}

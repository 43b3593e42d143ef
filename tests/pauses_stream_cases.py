"""Signals, specs and cuts for the pause streams, shared by the host and the device tests: a signal is built from its frames' activity (one
loud sample somewhere in an active frame, noise 40 dB under the threshold everywhere), so every case states which rule it reaches."""
import numpy as np

RATES = (8000, 11025, 22050, 24000, 48000)        # F = 80, 110, 220, 240, 480: 110 and 220 put no frame start on 16 bytes
DEFAULT = dict(max_pause_ms=400, lead_ms=50, tail_ms=100, threshold_db=-50.0, pad_ms=30)      # P 40, lead 5, tail 10, pad 3: h 20, t 20, k0 10
SPECS = {
    "default": DEFAULT,
    "h1_t0": {**DEFAULT, "max_pause_ms": 10},                       # P 1: h 1, t 0, nothing of a pause goes out early
    "pad0": {**DEFAULT, "pad_ms": 0},
    "lead0": {**DEFAULT, "lead_ms": 0},
    "tail0": {**DEFAULT, "tail_ms": 0},                             # k0 0
    "bare": dict(max_pause_ms=30, lead_ms=0, tail_ms=0, threshold_db=-50.0, pad_ms=0),
    "long_tail": dict(max_pause_ms=50, lead_ms=20, tail_ms=120, threshold_db=-40.0, pad_ms=10),   # tail > h: the front keeps more than a long run needs
    "odd": dict(max_pause_ms=70, lead_ms=30, tail_ms=20, threshold_db=-50.0, pad_ms=20),          # P 7: h 4, t 3
}


def frames_of(spec):
    c = lambda v: -(-int(v) // 10)
    return c(spec["max_pause_ms"]), c(spec["lead_ms"]), c(spec["tail_ms"]), c(spec["pad_ms"])


def signal(fs, act, n=None, seed=0, nan_at=None):
    """float32 [n] (default: the frames in full) whose frame j is active iff act[j]"""
    F = fs // 100
    act = np.asarray(act, dtype=bool)
    n = len(act) * F if n is None else n
    assert (len(act) - 1) * F < n <= len(act) * F
    rng = np.random.default_rng(seed)
    thr = 10.0 ** (-50 / 20)
    x = (rng.uniform(-1, 1, n) * thr * 0.01).astype(np.float32)
    for j in np.nonzero(act)[0]:
        lo, hi = j * F, min((j + 1) * F, n)
        x[lo + int(rng.integers(0, hi - lo))] = np.float32(rng.choice([-0.5, 0.25, 0.9]))
        if rng.random() < 0.5:                                       # some speech-like body too, so crossfades and copies move real values
            x[lo:hi] += (0.1 * np.sin(np.arange(hi - lo) * 0.3)).astype(np.float32)
    if nan_at is not None:
        x[nan_at] = np.nan
    return x


def runs(*parts):
    """activity from (count, active) pairs"""
    return np.concatenate([np.full(c, bool(a)) for c, a in parts]) if parts else np.zeros(0, bool)


def edge_cases(fs, name="default"):
    """(label, x) for one rate and spec: the cases the issue names, sized by the spec's own frame counts"""
    F = fs // 100
    P, lead, tail, pad = frames_of(SPECS[name])
    out = [
        ("one_sample_loud", np.array([0.5], np.float32)), ("one_sample_quiet", np.zeros(1, np.float32)),
        ("F-1", signal(fs, [1], F - 1)), ("F", signal(fs, [1], F)), ("F+1", signal(fs, [1, 0], F + 1)), ("F+1_loud_last", signal(fs, [0, 1], F + 1, seed=3)),
        ("silent_short", signal(fs, runs((max(1, lead + tail - 1), 0)))), ("silent_long", signal(fs, runs((lead + tail + 7, 0)), (lead + tail + 7) * F - 5)),
        ("single_active", signal(fs, runs((lead + pad + 4, 0), (1, 1), (tail + pad + 6, 0)))),
        ("nan", signal(fs, runs((12, 0), (1, 0), (tail + pad + 3, 0)), nan_at=12 * F + 7)),
        ("inner_P", signal(fs, runs((2, 1), (P + 2 * pad, 0), (2, 1)))), ("inner_P+1", signal(fs, runs((2, 1), (P + 2 * pad + 1, 0), (2, 1)))),
        ("inner_long_twice", signal(fs, runs((3, 0), (1, 1), (3 * P + 2 * pad + 5, 0), (4, 1), (P + 2 * pad + 2, 0), (1, 1), (2, 0)), seed=5)),
        ("resumes_within_pad", signal(fs, runs((1, 1), (2 * pad + 1, 0), (1, 1), (2 * pad, 0), (1, 1), (max(0, pad - 1), 0), (1, 1)))),
        ("trailing_partial", signal(fs, runs((1, 1), (pad + tail + 2, 0)), (pad + tail + 3) * F - F // 2)),
        ("active_partial_last", signal(fs, runs((lead + pad + 2, 0), (2, 1), (P + 2 * pad + 3, 0), (1, 1)), (lead + 3 * pad + P + 8) * F - 3, seed=9)),
    ]
    return out


def cuts(n, F, kind, seed=0):
    """push sizes that add up to n; the caller marks the last as final (kinds ending in '+empty' add an empty final push)"""
    rng = np.random.default_rng(seed)
    if kind == "whole":
        return [n]
    if kind == "per_sample":
        return [1] * n
    if kind == "frames":
        s = [F] * (n // F)
        return s + ([n % F] if n % F else [])
    if kind == "inside_every_frame":                                 # every push ends strictly inside a frame, a different place each time
        s, at, j = [], 0, 0
        while True:
            nxt = j * F + 1 + (7 * j) % (F - 1)
            if nxt >= n:
                break
            s.append(nxt - at)
            at, j = nxt, j + 1
        return s + [n - at]
    if kind in ("random", "random+empty"):
        k = int(rng.integers(1, 9))
        pts = np.sort(rng.integers(0, n + 1, k))
        s = [int(v) for v in np.diff(np.concatenate([[0], pts, [n]]))]
        for _ in range(2):
            s.insert(int(rng.integers(0, len(s))), 0)                # pushes of 0
        return s + ([0] if kind == "random+empty" else [])
    raise ValueError(kind)

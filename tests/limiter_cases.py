"""The segments of the limiter tests, per rate, and the twin's results on them, computed once per process.  Every length at which
csrc/limiter.hip can go wrong: 1, around the window 2 W + 1, around its tile, two tiles and one sample; every family of the issue: no
sample over the threshold, one at either end, one on either side of a tile edge, two peaks whose dips just overlap and just do not, a
dense burst, and |u| exactly at the threshold and one float32 above it."""
from functools import lru_cache

import numpy as np

from chattts_amd import limiter as LM
from tests import loudness_cases as LC

RATES = (8000, 22050, 24000, 48000)
TILE = LM.TILE


def lengths(fs: int):
    W = fs // 100
    return (1, W, 2 * W, 2 * W + 1, 2 * W + 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def enveloped(seed: int, n: int) -> np.ndarray:
    """like loudness_cases.enveloped, in stretches of 300 samples: no sample reaches 0.3"""
    r = np.random.default_rng(seed)
    env = np.repeat(r.choice([0, 0.003, 0.05, 0.3], size=n // 300 + 1), 300)[:n]
    return (r.uniform(-1, 1, n) * env).astype(np.float32)


def _with(x, **at):
    x = x.copy()
    for i, v in at.items():
        x[int(i[1:])] = v
    return x


@lru_cache(maxsize=None)
def cases(fs: int):
    """[(name, float32 segment, float32 pre-gain)] at rate fs"""
    W = fs // 100
    out = []
    for k, n in enumerate(lengths(fs)):
        base = enveloped(100 + k, n)
        out.append((f"quiet_{n}", base, 2.0))                                         # 2 * 0.3 stays under the threshold
        out.append((f"first_{n}", _with(base, i0=0.95), 1.5))
        out.append((f"last_{n}", _with(base, **{f"i{n - 1}": -0.97}), 1.0))
        if n > TILE:                                                                  # the last sample of tile 0, the first of tile 1
            out.append((f"edge_lo_{n}", _with(base, **{f"i{TILE - 1}": 0.99}), 1.25))
            out.append((f"edge_hi_{n}", _with(base, **{f"i{TILE}": -0.99}), 1.25))
        if n >= 2 * W + 2:                                                            # dips that just overlap, dips that just do not
            a = 0 if n <= TILE else min(TILE - W - 1, n - 2 * W - 2)                   # across the tile edge where there is one
            out.append((f"pair2W_{n}", _with(base, **{f"i{a}": 0.9, f"i{a + 2 * W}": -2.0}), 2.0))
            out.append((f"pair2W1_{n}", _with(base, **{f"i{a}": 0.9, f"i{a + 2 * W + 1}": -2.0}), 2.0))
    bursts = next(x for name, x, _ in LC.signals() if name == "bursts")
    out.append(("dense", bursts, 2.5))
    at = enveloped(200, TILE + 1)
    out.append(("at_T", _with(at, i700=LM.T, **{f"i{TILE}": -LM.T}), 1.0))          # |u| = T exactly: not over
    out.append(("above_T", _with(at, i700=np.nextafter(LM.T, np.float32(1))), 1.0))   # the next float32: over, r just under 1
    return out


@lru_cache(maxsize=None)
def twin(fs: int):
    """the twin's (y, record) of every case at rate fs, each segment alone"""
    return [LM.limit_segment(x, fs, g) for _, x, g in cases(fs)]


def offsets(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

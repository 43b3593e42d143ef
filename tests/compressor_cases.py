"""The segments of the compressor tests, per rate, and the twin's results on them, computed once per process.  Every length at which
csrc/compressor.hip can go wrong: 1, around one block B, around the reach (A + H + 2) B of a window, one sample before, at and behind a
sample-tile edge (TILE B samples), and five tiles and three samples, where a hold of 500 blocks reaches across more than two tile
edges; every spec at which the window arithmetic changes: the defaults, the shortest and the longest attack, no hold and the longest,
on the deepest curve the validator admits; silence, a quiet segment under the knee, and NaNs."""
from functools import lru_cache

import numpy as np

from chattts_amd import compressor as CP

RATES = (8000, 24000, 44100, 48000)
TILE = CP.TILE_BLOCKS
SPECS = (True,
         {"attack_ms": 1, "hold_ms": 0},
         {"attack_ms": 20, "hold_ms": 0, "threshold_db": -40, "ratio": 8, "knee_db": 12},
         {"attack_ms": 1, "hold_ms": 500, "knee_db": 0},
         {"attack_ms": 20, "hold_ms": 500, "threshold_db": -60, "ratio": 20, "knee_db": 0})


def enveloped(seed: int, n: int, B: int) -> np.ndarray:
    """noise under an envelope that changes every 5 blocks, from silence to 0.9: every region of the curve, many attacks and releases"""
    r = np.random.default_rng(seed)
    env = np.repeat(r.choice([0, 0.001, 0.02, 0.2, 0.9], size=n // (5 * B) + 1), 5 * B)[:n]
    return (r.uniform(-1, 1, n) * env).astype(np.float32)


def lengths(fs: int, spec):
    B = fs // 1000
    A, H = CP.blocks(CP.check(spec))
    reach = (A + H + 2) * B
    return (1, B - 1, B, B + 1, reach - 1, reach + 1, TILE * B - 1, TILE * B, TILE * B + 1)


@lru_cache(maxsize=None)
def cases(fs: int):
    """[(name, float32 segment, spec)] at rate fs"""
    B = fs // 1000
    out = []
    for k, spec in enumerate(SPECS):
        for j, n in enumerate(lengths(fs, spec)):
            out.append((f"env_{k}_{n}", enveloped(1000 * k + j, n, B), spec))
    long = 5 * TILE * B + 3
    x = np.float32(0.01) * enveloped(7, long, B)
    x[100 * B + 3] = 0.8                                                               # one loud block: held across tiles 1 .. 4
    out.append((f"held_{long}", x, SPECS[3]))
    out.append((f"held_deep_{long}", x, SPECS[4]))
    out.append((f"env_default_{long}", enveloped(8, long, B), True))
    out.append(("silence", np.zeros(3 * B + 1, np.float32), True))
    out.append(("quiet", np.float32(0.04) * enveloped(9, 2 * TILE * B + 5, B), True))  # 0.04 * 0.9 is under the knee's foot at -27 dB
    xn = enveloped(10, TILE * B + 2 * B + 1, B)
    xn[[0, 5 * B + 1, TILE * B - 1, TILE * B]] = np.nan                               # NaNs: at the start, inside a block, either side of a tile edge
    xn[7 * B: 8 * B] = np.nan                                                         # and a whole block of them
    out.append(("nan", xn, True))
    out.append(("inf", np.array([0.5, np.inf, -0.25] * B, np.float32), SPECS[1]))
    return out


@lru_cache(maxsize=None)
def twin(fs: int):
    """the twin's (y, record) of every case at rate fs, each segment alone"""
    return [CP.compress_segment(x, fs, spec) for _, x, spec in cases(fs)]


def offsets(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

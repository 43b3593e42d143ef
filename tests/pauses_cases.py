"""Fixtures of the pause-control tests: Gaussian noise under a stepped envelope, loud steps against steps at -70 dBFS, with every sample
kept a factor of 2 away from the -50 dB threshold (`margin` measures it), and the oracle's answer per (signal, rate, spec), computed once."""
from functools import lru_cache

import numpy as np

from tests import pauses_oracle as PO

RATES = (8000, 11025, 24000, 44100)
BLOCK = 256                                     # frames a workgroup of the plan kernel scans per chunk
THR_DB = -50.0
THR = np.float32(10.0 ** (THR_DB / 20.0))
QUIET = 10.0 ** (-70.0 / 20.0)
# (name, spec): what the specs exercise -- the defaults; no dilation, no edges, a short cap (many crossfades); P = 1 with a long tail
SPECS = (("defaults", {}),
         ("bare", dict(max_pause_ms=50, lead_ms=0, tail_ms=0, pad_ms=0)),
         ("p1", dict(max_pause_ms=10, lead_ms=20, tail_ms=300, pad_ms=10)))


def spec_of(k):
    d = dict(SPECS[k][1])
    d["threshold_db"] = THR_DB
    return d


def stepped(n_frames: int, F: int, n: int, seed: int, first_loud=False, quiet_runs=(2, 7, 12, 45, 60, 130)) -> np.ndarray:
    """n samples (n <= n_frames * F): alternating quiet and loud steps of whole frames; the quiet runs' lengths are drawn from
    `quiet_runs` (some under, some over every spec's cap), the loud ones hold 1 .. 8 frames"""
    rng = np.random.default_rng(seed)
    env = np.empty(n_frames, dtype=bool)
    j, loud = 0, first_loud
    while j < n_frames:
        m = int(rng.integers(1, 9)) if loud else int(rng.choice(quiet_runs))
        env[j: j + m] = loud
        j += m
        loud = not loud
    e = np.repeat(env, F)[:n]
    g = np.clip(rng.standard_normal(n), -3.0, 3.0)
    x = np.where(e, 0.25 * g, QUIET * g).astype(np.float32)
    near = e & (np.abs(x) < 2.5 * THR)              # a loud sample that came out close to the threshold moves up and away from it
    x[near] = np.where(x[near] < 0, -1.0, 1.0).astype(np.float32) * np.float32(2.5) * THR
    return x


def margin(x: np.ndarray) -> float:
    """the smallest factor between a sample's magnitude and the threshold, either way (>= 2 wanted)"""
    a = np.abs(x.astype(np.float64))
    t = float(THR)
    with np.errstate(divide="ignore"):
        return float(np.min(np.where(a < t, t / a, a / t)))


def lengths(F: int):
    """(frames, samples) of the segments of one rate: 1, F - 1, F, F + 1 samples; one block of frames, minus and plus one frame, the last
    frame partial in two of them; about 2.1 blocks, so that every scan carries twice"""
    return [(1, 1), (1, F - 1), (1, F), (2, F + 1), (BLOCK - 1, (BLOCK - 1) * F - 3), (BLOCK, BLOCK * F), (BLOCK + 1, BLOCK * F + 2),
            (538, 538 * F - F // 2 - 1)]


@lru_cache(maxsize=None)
def segments(fs: int):
    """the segments of rate fs -> tuple of (x, spec index)"""
    F = fs // 100
    out = []
    for i, (nf, n) in enumerate(lengths(F)):
        out.append((stepped(nf, F, n, 1000 * (fs % 97) + i, first_loud=i % 3 == 1), i % len(SPECS)))
    out.append((stepped(300, F, 300 * F - 7, 77, quiet_runs=(400,)), 0))           # not one active frame
    out.append((stepped(40, F, 40 * F, 78, first_loud=True, quiet_runs=(1,)), 0))  # hardly a quiet one
    return tuple(out)


_answers = {}


def answer(x: np.ndarray, fs: int, k):
    """the oracle's (y, record) of x at fs under spec k (None: copied through), computed once per distinct input"""
    key = (x.tobytes(), fs, k)
    if key not in _answers:
        _answers[key] = PO.passthrough(x, fs) if k is None else PO.trim(x, fs, spec_of(k))
    return _answers[key]


def offsets(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

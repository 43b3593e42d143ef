"""The signals of the loudness tests and their oracle results, computed once per process (tests/loudness_oracle.py is a serial loop per
sample: every (signal, rate) pair is filtered once and shared)."""
from functools import lru_cache

import numpy as np

from tests import loudness_oracle as O

LENGTHS = (1, 2399, 2400, 9599, 9600, 9601, 11999, 12000, 14400, 24000, 50000, 123457)
RATES = (8000, 22050, 24000, 48000)
TARGET = -16.0
# the seed of each length: 0 .. 5 in turn, ordered so that no block of any case lies within 0.01 LU of a gate at any of RATES
SEEDS = (0, 1, 2, 3, 4, 5, 0, 1, 2, 4, 5, 3)


def enveloped(seed: int, n: int) -> np.ndarray:
    """uniform noise under a stepped envelope: stretches of 1200 samples at four levels that put blocks on both sides of both gates"""
    r = np.random.default_rng(seed)
    sig = r.uniform(-1, 1, n)
    env = np.repeat(r.choice([0, 0.003, 0.05, 0.3], size=n // 1200 + 1), 1200)[:n]
    return (sig * env).astype(np.float32)


@lru_cache(maxsize=None)
def signals():
    """[(name, float32 signal, target)]: every length under its seed, then the six special ones"""
    out = [(f"env{seed}_{n}", enveloped(seed, n), TARGET) for seed, n in zip(SEEDS, LENGTHS)]
    out.append(("zeros", np.zeros(12000, np.float32), TARGET))
    t = np.arange(24000) / 24000.0
    sine = np.sin(2 * np.pi * 997 * t)
    out.append(("sine", sine.astype(np.float32), TARGET))                                                          # full scale, L = -2.98: attenuated
    # full scale one tenth of the time: L is near -13, the peak 1, so towards -5 LUFS the -1 dBFS ceiling binds (the plain sine is louder
    # than every allowed target, no ceiling can bind on it)
    out.append(("bursts", (sine * (np.arange(24000) % 2400 < 240)).astype(np.float32), -5.0))
    out.append(("silent", (1e-4 * np.random.default_rng(7).uniform(-1, 1, 12000)).astype(np.float32), TARGET))     # under the absolute gate
    out.append(("faint", (0.002 * np.random.default_rng(8).uniform(-1, 1, 24000)).astype(np.float32), -10.0))      # the +30 dB cap binds
    r = np.random.default_rng(9)                  # loud, a long stretch under the absolute gate, moderate: blocks on both sides of it at every rate
    out.append(("gap", (r.uniform(-1, 1, 72000) * np.repeat([0.3, 1e-4, 0.05], [24000, 36000, 12000])).astype(np.float32), TARGET))
    return out


@lru_cache(maxsize=None)
def blocks(i: int, fs: int):
    """the oracle's gating blocks of signal i at rate fs"""
    return tuple(O.segment_blocks(signals()[i][1], fs))


def peak(i: int) -> float:
    return float(np.abs(signals()[i][1]).max())


@lru_cache(maxsize=None)
def alone(i: int, fs: int, target=...):
    """the oracle's record of signal i as a group of its own at rate fs (target: the signal's own unless given)"""
    return O.finish(blocks(i, fs), peak(i), signals()[i][2] if target is ... else target)


def grouped(idx, rates, target):
    """the oracle's record of the group of signals idx at their rates"""
    ms = [z for i, fs in zip(idx, rates) for z in blocks(i, fs)]
    return O.finish(ms, max(peak(i) for i in idx), target)


def offsets(lens) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

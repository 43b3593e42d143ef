"""The signals of the IMA ADPCM tests, shared by the host and the GPU files: every length at which the block rule takes another path, and
the signals that drive the step into its clamps.  Everything is seeded; nothing here reads the code under test beyond `adpcm.STEP` and the
block sizes."""
import numpy as np

from chattts_amd import adpcm

RATES = (8000, 24000, 48000)         # blocks of 256 / 512 / 1024 bytes: S = 505 / 1017 / 2041


def lengths(rate):
    S = adpcm.samples_per_block(rate)
    return [1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 70 * S + 3]


def noise(n, seed, amp=6000.0):
    """a seeded random walk with noise on top: differences of every size up to a few thousand"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal(n) * amp * 0.05) + rng.standard_normal(n) * amp * 0.1
    return np.clip(x, -32768, 32767).astype(np.int16)


def burst(rate, seconds=4.0, seed=7):
    """speech-like: voiced bursts (harmonics of a gliding pitch under two formant bumps) between near-silent gaps, a little noise"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / rate
    f0 = 110.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(n)
    for h in range(1, 30):
        f = h * 120.0
        if f >= 0.45 * rate:
            break
        w = np.exp(-((f - 600.0) / 400.0) ** 2) + 0.5 * np.exp(-((f - 1800.0) / 600.0) ** 2) + 0.03
        x += w * np.sin(h * ph + h)
    env = np.clip(np.sin(2 * np.pi * 1.3 * t) * 3.0, 0.0, 1.0) ** 2
    x = x / np.abs(x).max() * env * 14000.0 + rng.standard_normal(n) * 8.0
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def cases(rate):
    """[(name, int16 signal)] at `rate`"""
    S = adpcm.samples_per_block(rate)
    rng = np.random.default_rng(rate)
    out = [(f"noise{n}", noise(n, rate + n)) for n in lengths(rate)]
    out.append(("zeros", np.zeros(S + 1, np.int16)))                                     # the index stays at 0
    sq = np.where((np.arange(2 * S + 1) // 20) % 2 == 0, 32767, -32767).astype(np.int16)
    out.append(("square", sq))                                                           # the predictor and index 88 clamp
    lo_hi = noise(S + 1, rate + 1)
    lo_hi[:2] = (-32768, 32767)
    out.append(("lo_hi", lo_hi))                                                         # a first difference of 65535: index0 88
    for i in (0, 1, 7, 8, 40, 87, 88):
        for extra in (0, 1):
            x = noise(50, rate + 100 * i + extra, 300.0)
            x[0] = -16000
            x[1] = int(np.clip(-16000 + adpcm.STEP[i] + extra, -32768, 32767))
            out.append((f"step{i}+{extra}", x))
    out.append(("full", rng.integers(-32768, 32768, 2 * S + 1).astype(np.int16)))        # full-range white noise
    out.append(("burst", burst(rate, seconds=(3 * S + 11) / rate)))
    return out


def pack(items):
    """[(signal, rate)] -> (flat int16 with every signal on a multiple of 8 elements and a gap of canary samples behind it, [(start, n,
    rate)])"""
    parts, ranges, at = [], [], 0
    for x, rate in items:
        ranges.append((at, len(x), rate))
        room = (len(x) + 7) // 8 * 8 + 8
        parts.append(np.concatenate([x, np.full(room - len(x), 12345, np.int16)]))
        at += room
    return np.concatenate(parts), ranges

"""The signals and cuts of the streamed IMA ADPCM tests, shared by the host and the GPU files.  Signals: `noise` and `burst` of
tests/adpcm_cases.py, all-zero, constant -32768, and a +-32767 square wave (index 88 and both clamps of the predictor).  Cuts, per block
size S (505 / 1017 / 2041 at the rates of adpcm_cases.RATES): every push length at which the cutting rule takes another path; the last
push of each list is final.  Everything is seeded; nothing here reads the code under test beyond the block sizes."""
import numpy as np

from chattts_amd import adpcm
from tests import adpcm_cases as AC

RATES = AC.RATES
SIGNALS = ("noise", "burst", "zeros", "floor", "square")


def cuts(rate):
    """{name: the push lengths}"""
    S = adpcm.samples_per_block(rate)
    rng = np.random.default_rng(rate + 17)
    out = {
        "every_path": [0, 1, S - 1, 1, 0, S, S + 1, 2 * S + 1, 3 * S + 7, 0],
        "one_block_then_nothing": [S - 1, 1, 0],
        "one_sample": [1],
        "no_samples": [0, 0],
        "two_blocks": [2 * S],
        "block_reached_by_ones": [S - 2, 1, 1, 1],
        "serial_schedule": [12000] * 5 + [3777],
    }
    for k in range(3):
        out[f"random{k}"] = [int(v) for v in rng.integers(0, 2 * S + 2, 7)]
    return out


def total(rate):
    return max(sum(c) for c in cuts(rate).values())


_CACHE = {}


def signal(name, rate):
    """the signal `name` at `rate`, long enough for every cut (int16, read-only)"""
    key = (name, rate)
    if key not in _CACHE:
        n = total(rate)
        if name == "noise":
            x = AC.noise(n, rate + 3)
        elif name == "burst":
            x = AC.burst(rate, seconds=(n + 1) / rate)[:n]
        elif name == "zeros":
            x = np.zeros(n, np.int16)
        elif name == "floor":
            x = np.full(n, -32768, np.int16)
        elif name == "square":
            x = np.where((np.arange(n) // 20) % 2 == 0, 32767, -32767).astype(np.int16)
        else:
            raise KeyError(name)
        assert len(x) == n
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def pushes(lens):
    """push lengths -> [(lo, hi, final)]"""
    out, at = [], 0
    for i, n in enumerate(lens):
        out.append((at, at + n, i == len(lens) - 1))
        at += n
    return out


def one_shot(name, rate, n):
    """`adpcm.encode_blocks(signal[:n])`, put together from the blocks of the whole signal (a block's bytes depend on its own samples
    only) and one more call for a last block that is not full; no bytes for n = 0"""
    x = signal(name, rate)
    key = (name, rate, "whole")
    if key not in _CACHE:
        _CACHE[key] = adpcm.encode_blocks(x, rate)
    A, S = adpcm.align(rate), adpcm.samples_per_block(rate)
    full = n // S
    head = _CACHE[key][: full * A]
    return np.concatenate([head, adpcm.encode_blocks(x[full * S: n], rate)]) if n % S else head


def reference(name, rate, cut):
    """what a stream of signal `name` cut by `cut` emits, push by push (a tuple of uint8 arrays, computed once): the one-shot encoder's
    blocks, dealt out by the cutting rule -- not the twin, which tests/test_adpcm_stream_host.py holds against this"""
    key = (name, rate, cut)
    if key not in _CACHE:
        lens = cuts(rate)[cut]
        blob = one_shot(name, rate, sum(lens))
        A, out, carry, at = adpcm.align(rate), [], 0, 0
        for lo, hi, final in pushes(lens):
            blocks, carry = adpcm.stream_plan(carry, hi - lo, final, rate)
            out.append(blob[at: at + blocks * A])
            at += blocks * A
        assert at == len(blob)
        _CACHE[key] = tuple(out)
    return _CACHE[key]

"""The cuts, signals and references of the streamed-FLAC tests (host and GPU share them): one signal of 3 x 4096 + 37 samples per name,
cut into pushes by the fixed lists below and by one seeded set of random cuts; the twin's chunks of a case are computed once."""
import functools

import numpy as np

from chattts_amd import flac
from tests import flac_cases as FC
from tests import flac_stream_oracle as SO

N = 3 * 4096 + 37
GPU_SIGNALS = ["noise", "silence", "dc_min", "spikes", "half_silence"]
GPU_RATES = [24000, 11025, 65535]

# name -> (the lengths of the pushes that are not final, the length of the final one)
CUTS = {
    "carry_reaches_16": ([1, 14, 1, 0, 15, 16, 17, 0, 4095], 4096),      # 1 + 14 wait, the next 1 makes a block of 16
    "around_4096": ([4097, 4111], 4112),
    "final_empty_carry_15": ([15], 0),
    "no_samples": ([], 0),
    "empty_pushes_only": ([0, 0], 0),
    "one_push": ([], N),
    "all_then_empty_final": ([N], 0),
    "rest_of_15_is_emitted_at_the_end": ([4096], 15),
}


def _random_cuts():
    rng = np.random.default_rng(20240229)
    out = {}
    for k in range(2):
        cuts, left = [], N
        while left > 0 and len(cuts) < 10:
            n = int(rng.choice([0, int(rng.integers(1, 40)), int(rng.integers(40, 5000)), int(rng.integers(4080, 4120))]))
            n = min(n, left)
            cuts.append(n)
            left -= n
        out[f"random_{k}"] = (cuts[:-1], cuts[-1]) if cuts else ([], 0)
    return out


CUTS.update(_random_cuts())


def pushes(cut):
    """-> [(lo, hi, final)]: the slices of the signal that the pushes of cut `cut` bring"""
    lens, last = CUTS[cut]
    out, at = [], 0
    for n in list(lens) + [last]:
        out.append((at, at + n, False))
        at += n
    out[-1] = out[-1][:2] + (True,)
    assert at <= N
    return out


@functools.lru_cache(maxsize=None)
def signal(name):
    x = FC.signal(name, N)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, rate, cut, first_sample=0):
    """the twin's chunk of every push of the case, as a tuple of bytes"""
    enc = flac.StreamEncoder(rate, first_sample)
    x = signal(name)
    return tuple(enc.push(x[lo:hi], final) for lo, hi, final in pushes(cut))


@functools.lru_cache(maxsize=None)
def _decoded(data, first_sample):
    """flac_stream_oracle.decode(data, info=True), once per distinct stream (a device result that equals the twin's is decoded once)"""
    return SO.decode(data, first_sample=first_sample, info=True)


def check_stream(chunks, rate, samples, first_sample=0):
    """the chunks behind the stream header decode, through the independent decoder, to `samples`, and every chunk ends where a frame
    ends (a chunk's frames are complete when it is sent); -> the decoder's facts"""
    y, r, facts = _decoded(flac.stream_header(rate) + b"".join(bytes(c) for c in chunks), first_sample)
    assert r == rate and np.array_equal(y, samples)
    ends = set(np.cumsum([0] + facts["frame_sizes"]).tolist())
    assert all(e in ends for e in np.cumsum([len(c) for c in chunks]).tolist())
    return facts

"""The equaliser's test pack, shared by tests/test_equalizer_host.py (the route twin against the serial definition) and
tests/test_gpu_equalizer.py (the kernels against it): ten segments -- the lengths at which the route takes another path, c the chunk
and 64 c the tile -- at mixed rates and specs with one segment that is off in the middle, and four kinds of input.  The reference,
`equalizer.apply` of every segment, is computed once per kind and never written."""
from functools import lru_cache

import numpy as np

from chattts_amd import equalizer as EQ

C, T = EQ.CHUNK, EQ.TILE
MAX4 = {"highpass_hz": 120, "lowshelf": {"hz": 250, "db": 4.5}, "highshelf": {"hz": 5000, "db": -6}, "peaks": [{"hz": 1800, "db": 7.5, "q": 3}]}
HP20 = {"highpass_hz": 20}          # at 48 kHz: the poles closest to 1 that the validator lets through
OFF_AT = 5
# (samples, rate, spec): every single section type, the four-section maximum, both presets; entry OFF_AT is copied through
SEGMENTS = [(1, 8000, "telephone"), (2, 24000, "rumble"), (C - 1, 48000, {"peaks": [{"hz": 3000, "db": -9, "q": 0.7}]}),
            (C, 24000, {"lowshelf": {"hz": 200, "db": 6}}), (C + 1, 8000, {"highshelf": {"hz": 3000, "db": -4}}), (100, 24000, None),
            (T - 1, 48000, {"peaks": [{"hz": 1000, "db": 5, "q": 2}]}), (T, 24000, MAX4), (T + 1, 8000, "telephone"), (3 * T + 5, 48000, HP20)]
LENS = [n for n, _, _ in SEGMENTS]
RATES = [r for _, r, _ in SEGMENTS]
SPECS = [s for _, _, s in SEGMENTS]
OFFSETS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
KINDS = ("noise", "dc_sine", "impulse_first", "impulse_chunk_end")
CAP = 1e-3                          # the share of samples that may differ from the definition at all; each of them by one ulp


def signal(kind: str, n: int, rate: int, seed: int) -> np.ndarray:
    if kind == "noise":              # seeded, 0.3 rms
        return (0.3 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)
    if kind == "dc_sine":            # an offset of 0.2 under a 440 Hz sine
        return (0.2 + 0.3 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / rate)).astype(np.float32)
    x = np.zeros(n, dtype=np.float32)
    if kind == "impulse_first":
        x[0] = 1.0
    else:                            # a chunk's last sample: the tile's last where the segment has one, else the first chunk's, else its own
        x[T - 1 if n >= T else C - 1 if n >= C else n - 1] = 1.0
    return x


@lru_cache(maxsize=None)
def pack(kind: str) -> np.ndarray:
    x = np.concatenate([signal(kind, n, r, 100 + i) for i, (n, r, _) in enumerate(SEGMENTS)])
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def reference(kind: str) -> np.ndarray:
    """`equalizer.apply` of every segment of the pack, packed: the serial definition"""
    x = pack(kind)
    y = np.concatenate([EQ.apply(x[OFFSETS[i]: OFFSETS[i + 1]], r, s) for i, (_, r, s) in enumerate(SEGMENTS)])
    y.setflags(write=False)
    return y


def ordinal(a: np.ndarray) -> np.ndarray:
    """float32 -> int64 that ascend with the values, one step per representable number; -0 and +0 share 0"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.abs(ordinal(a) - ordinal(b))


def compare(tag: str, got: dict) -> float:
    """`got[kind]`: the packed result for every kind.  Every sample within one float32 ulp of the reference, the off segment bit for
    bit, and at most CAP of all samples different at all -> the share that differs (printed per kind and per segment that has any)"""
    differ = total = 0
    for kind in KINDS:
        y, ref = got[kind], reference(kind)
        assert y.dtype == np.float32 and y.shape == ref.shape and not np.isnan(y).any(), (tag, kind)
        d = ulps(y, ref)
        lo, hi = OFFSETS[OFF_AT], OFFSETS[OFF_AT + 1]
        assert y[lo:hi].tobytes() == pack(kind)[lo:hi].tobytes(), f"{tag}, {kind}: the segment that is off did not come back bit for bit"
        per = [int((d[OFFSETS[i]: OFFSETS[i + 1]] > 0).sum()) for i in range(len(SEGMENTS))]
        print(f"{tag}, {kind}: {int((d > 0).sum())} of {len(d)} samples differ, the most by {int(d.max())} ulp; per segment {per}")
        assert int(d.max()) <= 1, f"{tag}, {kind}: sample {int(d.argmax())} is {int(d.max())} ulp from the definition"
        differ += int((d > 0).sum())
        total += len(d)
    share = differ / total
    print(f"{tag}: {differ} of {total} samples differ from the definition, a share of {share:.2e} (the cap is {CAP:g})")
    assert share <= CAP, f"{tag}: {share:.2e} of the samples differ from the definition, the cap is {CAP:g}"
    return share

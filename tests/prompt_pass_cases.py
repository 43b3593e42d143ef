"""Case table of the prompt-pass attention tests (tests/test_prompt_pass_host.py checks on CPU that it reaches every edge it claims;
tests/test_gpu_prompt_pass.py runs it on the device) and the inputs / float64 answers of each case, computed once.

A case: G row groups of T rows at KV slots [slot0, slot0 + T), a cache of `cmax` rows per utterance, one kv_start per utterance.
T >= 128 runs attention_prefill_mfma_k (64-row query tiles of four 16-row waves, key blocks of 32 on absolute multiples of 32), T < 128
the one-wave attention_k (a row's keys in blocks of 32 from its first visible key, 8 key groups).  T = 1 is no prompt-pass shape: a launch
of one row per utterance is a decode launch by GptRowMap's convention (slot = len[b] - 1) and runs the decode kernel, so the smallest
one-wave case is T = 2."""
from collections import namedtuple

import numpy as np

from tests import prompt_pass_oracle as PO

f32 = np.float32
Case = namedtuple("Case", "name T slot0 cmax kv_start qscale seed")
TRAP_V = 1024.0      # V of the cache rows below kv_start: a leaked pad key moves the output by about 1024 / n, far beyond any bound

MFMA_CASES = (
    #    name          T   slot0 cmax  kv_start              q
    Case("t128_s0",    128, 0,   168,  (0, 1, 31, 127),      1.0,  1),    # whole tiles; kv_start at the chunk's last row
    Case("t129_s33",   129, 33,  162,  (0, 33, 97, 161),     12.0, 2),    # last tile holds ONE row; cmax == slot0 + T, not a multiple of 32
    Case("t144_s31",   144, 31,  192,  (31, 32, 95, 100),    1.0,  3),    # last tile = one whole wave
    Case("t145_s32",   145, 32,  177,  (5, 63, 96, 176),     12.0, 4),    # ... plus one row of the next; cmax == slot0 + T
    Case("t191_s100",  191, 100, 291,  (0, 100, 164, 229),   1.0,  5),    # last row of the last wave missing; cmax == slot0 + T
    Case("t193_s0",    193, 0,   200,  (0, 64, 192, 65),     12.0, 6),    # four tiles, the last of one row
)
WAVE_CASES = (
    Case("t127_s0",    127, 0,   127,  (0, 5, 126),          1.0,  11),   # just under the route threshold; every key count 1 .. 127
    Case("t127_s3",    127, 3,   140,  (0, 3, 70),           12.0, 12),
    Case("t33_s200",   33,  200, 240,  (0, 199, 201, 232),   1.0,  13),   # several blocks per row
    Case("t33_s0",     33,  0,   33,   (0, 1, 32),           12.0, 14),
    Case("t2_s7",      2,   7,   9,    (0, 7, 8),            1.0,  15),   # the smallest prompt chunk
)
CASES = MFMA_CASES + WAVE_CASES
BY_NAME = {c.name: c for c in CASES}
# slots (relative to slot0) at which the causality test cuts the future off
CUTS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
# one prompt, whole and in chunks: (kv_start per utterance, chunk lengths); every chunk of an MFMA prompt is >= 128 rows (same kernel as whole)
CHUNKED = (
    ("mfma_321", (0, 9, 130, 200), (128, 193), 1.0),       # boundary on a tile edge, second chunk ragged
    ("mfma_330", (0, 31, 165, 170), (165, 165), 12.0),     # boundary 165: no multiple of 32 or 64, the chunk's tiles sit elsewhere than whole's
    ("wave_100a", (0, 5, 40), (37, 63), 1.0),
    ("wave_100b", (0, 36, 64), (64, 2, 34), 12.0),
)


def groups(c) -> int:
    return len(c.kv_start)


def cuts(c):
    return sorted({s for s in CUTS + (c.T - 1,) if 0 < s < c.T})


def make_inputs(G, T, slot0, cmax, kv_start, qscale, seed, slots=None):
    """q [G*T, 2304] f32 (N(0, qscale^2) in the q columns), K / V [slots, 12, cmax, 64] f32 holding bf16 values: N(0, 1), V = TRAP_V below
    kv_start[b], NaN from slot0 + T on (where cmax has spare rows)"""
    slots = G if slots is None else slots
    rs = np.random.RandomState(seed)
    q = rs.standard_normal((G * T, 3 * PO.H)).astype(f32)
    q[:, :PO.H] *= f32(qscale)
    K = PO.bf16_round(rs.standard_normal((slots, PO.NH, cmax, PO.HD)).astype(f32)).copy()
    V = PO.bf16_round(rs.standard_normal((slots, PO.NH, cmax, PO.HD)).astype(f32)).copy()
    for b in range(min(slots, len(kv_start))):
        V[b, :, :kv_start[b]] = TRAP_V
    K[:, :, slot0 + T:] = np.nan
    V[:, :, slot0 + T:] = np.nan
    return q, K, V


_inputs, _answers = {}, {}


def inputs(c):
    """(q, K, V, kv_start int32) of a case, made once; treat as read-only"""
    if c.name not in _inputs:
        q, K, V = make_inputs(groups(c), c.T, c.slot0, c.cmax, c.kv_start, c.qscale, c.seed)
        _inputs[c.name] = (q, K, V, np.asarray(c.kv_start, np.int32))
        for a in _inputs[c.name]:
            a.setflags(write=False)
    return _inputs[c.name]


def answer(c):
    """the oracle's dict (ref, a, delta, n, valid) of a case, computed once"""
    if c.name not in _answers:
        q, K, V, ks = inputs(c)
        _answers[c.name] = PO.reference(q, K, V, c.T, c.slot0, ks)
    return _answers[c.name]

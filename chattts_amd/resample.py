"""Host side of the device resampler (csrc/resample.hip, `CodecEngine.resample`): the rational ratio of a rate pair, the polyphase
filter table and the packed-segment arithmetic, all in Python integers / float64.  Nothing here touches the GPU.

The filter is the Hann-windowed sinc that `torchaudio.functional.resample` documents as its default (6 zero crossings, roll-off 0.99).
With orig = M and new = L (the rates divided by their gcd):
    base  = min(orig, new) * 0.99            width = ceil(6 * orig / base)            K = 2 * width + orig
    t_i[k] = clamp(((k - width) / orig - i / new) * base, -6, 6)
    h[i][k] = (base / orig) * cos^2(pi t / 12) * sinc(t)
    y[j * new + i] = sum_k h[i][k] * x[j * orig + k - width]            (x = 0 outside the segment)

Streams (`CodecEngine.resample_stream_step`, ctts_resample_stream_step): the signal arrives in pushes and its conversion leaves in chunks
whose concatenation is the one-shot result.  Output o = j L + i reads inputs [j M - width, j M + width + M); with P' samples pushed and
more to come, J(P') = (P' - width - M) // M + 1 frames j are complete (0 while P' < width + M) and the stream has emitted E' = J L
outputs; the last push, which knows the total, emits the rest up to ceil(P' L / M).  Nothing below c' = max(0, (E' // L) M - width) is read
again: the stream keeps samples [c', P'), at most K - 1 of them since J > (P' - width - M) / M (`stream_plan`, in Python integers).
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

ZEROS = 6            # zero crossings of the sinc either side
ROLLOFF = 0.99
TILE = 2048          # csrc/kernels.hpp RS_TILE: output samples per workgroup
LDS_FLOATS = 16384   # RS_LDS_FLOATS: a tile's input span (+ the table, where both fit) in LDS
TAB_MAX = 1 << 20    # RS_TAB_MAX: the largest table, in floats
CARRY = 512          # RS_CARRY: floats of a stream's carry.  A stream keeps at most K - 1 samples (`stream_plan`); 24000 -> 11025 Hz, the
#                      longest filter among the common telephony and audio rates, has K = 348


def ratio(orig: int, new: int) -> Tuple[int, int]:
    """(L, M) = (new, orig) / gcd"""
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError(f"sample rates must be positive (got {orig} -> {new})")
    g = math.gcd(orig, new)
    return new // g, orig // g


def geometry(L: int, M: int) -> Tuple[int, int]:
    """(width, K) of the table for the reduced pair"""
    width = int(math.ceil(ZEROS * M / (min(L, M) * ROLLOFF)))      # float64, as the formula is stated
    return width, 2 * width + M


def taps(orig: int, new: int) -> np.ndarray:
    """float64 [L, K] polyphase table of the conversion orig -> new"""
    L, M = ratio(orig, new)
    width, K = geometry(L, M)
    base = min(L, M) * ROLLOFF
    idx = (np.arange(K, dtype=np.float64) - width) / M
    t = (idx[None, :] - np.arange(L, dtype=np.float64)[:, None] / L) * base
    t = np.clip(t, -ZEROS, ZEROS)
    win = np.cos(t * (math.pi / (2 * ZEROS))) ** 2
    return (base / M) * win * np.sinc(t)          # np.sinc(t) = sin(pi t) / (pi t), 1 at 0


def mode(L: int, M: int, K: int) -> int:
    """what the kernel makes of a table (ctts_resample_supported): 0 = refused, 1 = table through L2, 2 = table in LDS"""
    if L < 1 or M < 1 or L == M or K <= M or (K - M) % 2:
        return 0
    span, tab = ((TILE - 1) // L + 1) * M + K, L * K
    if span > LDS_FLOATS or tab > TAB_MAX:
        return 0
    return 2 if tab + span <= LDS_FLOATS else 1


def out_len(n: int, L: int, M: int) -> int:
    """ceil(n L / M), in Python integers"""
    return -(-int(n) * int(L) // int(M))


def plan(orig: int, new: int, off) -> Tuple[int, int, int, np.ndarray]:
    """(L, M, K, off_out) of converting the packed segments at `off` (n_seg + 1 sample offsets) from `orig` to `new`; raises
    ValueError for everything the kernel must not be launched with"""
    L, M = ratio(orig, new)
    if L == M:
        raise ValueError("resample: the rates are equal, there is nothing to convert")
    _, K = geometry(L, M)
    if mode(L, M, K) == 0:
        raise ValueError(f"resample: {orig} -> {new} Hz reduces to {L}/{M} with {K} taps per phase, beyond what the kernel supports "
                         f"(a tile's input span within {LDS_FLOATS} floats, the table within {TAB_MAX})")
    off = [int(v) for v in off]
    if len(off) < 2 or off[0] != 0:
        raise ValueError("resample: offsets must start at 0 and hold at least one segment")
    out = [0]
    for i in range(len(off) - 1):
        n = off[i + 1] - off[i]
        if n <= 0:
            raise ValueError(f"resample: segment {i} is empty or the offsets do not ascend")
        out.append(out[-1] + out_len(n, L, M))
    if out[-1] >= 1 << 31:
        raise ValueError("resample: the output would hold 2^31 samples or more")
    return L, M, K, np.asarray(out, dtype=np.int64)


def window_inputs(L: int, M: int, K: int, o_lo: int, o_hi: int, total: int) -> Tuple[int, int]:
    """[a, b): the inputs inside [0, total) that outputs [o_lo, o_hi) of the conversion of a `total`-sample signal read -- output
    o = j L + i reads inputs j M + k - width, k = 0 .. K-1, so a = (o_lo // L) M - width and b = ((o_hi - 1) // L) M + width + M,
    clipped (inputs outside the signal read as zero).  What a streamed chunk's window must hold (csrc/resample.hip, resample_win_k).
    An empty range of outputs reads nothing: (a, a).  ValueError: o_lo < 0, o_hi < o_lo, o_hi beyond ceil(total L / M)."""
    L, M, K, o_lo, o_hi, total = int(L), int(M), int(K), int(o_lo), int(o_hi), int(total)
    if L < 1 or M < 1 or K <= M or (K - M) % 2 or total < 0:
        raise ValueError(f"resample: no table has L = {L}, M = {M}, K = {K} (K = 2 width + M), and a signal holds 0 samples or more")
    if o_lo < 0 or o_hi < o_lo:
        raise ValueError(f"resample: outputs [{o_lo}, {o_hi}) are not a range")
    if o_hi > out_len(total, L, M):
        raise ValueError(f"resample: output {o_hi} lies beyond the {out_len(total, L, M)} outputs of {total} samples")
    width = (K - M) // 2
    a = min(max((o_lo // L) * M - width, 0), total)
    if o_hi == o_lo:
        return a, a
    return a, max(a, min(((o_hi - 1) // L) * M + width + M, total))


def frames_final(p: int, M: int, width: int) -> int:
    """J(p): the frames j whose inputs [j M - width, j M + width + M) lie within the first p samples; monotone in p"""
    return (int(p) - width - M) // M + 1 if int(p) >= width + M else 0


def stream_plan(L: int, M: int, K: int, pushed: int, emitted: int, n_in: int, final: bool) -> dict:
    """One push of a stream in Python integers: `pushed` samples are in and `emitted` outputs out, `n_in` samples arrive, `final` says
    they are the last.  -> o_lo (= emitted), n_out (the outputs the step emits: [emitted, E')), emitted (E'), carry_in / carry_out (the
    samples kept in front of and behind the step: [c, pushed) and [c', pushed + n_in), 0 behind the last), total (-1 while not final).
    ValueError for everything the library must not be launched with."""
    L, M, K, pushed, emitted, n_in = int(L), int(M), int(K), int(pushed), int(emitted), int(n_in)
    if L < 1 or M < 1 or K <= M or (K - M) % 2:
        raise ValueError(f"resample: no table has L = {L}, M = {M}, K = {K} (K = 2 width + M)")
    if pushed < 0 or n_in < 0 or emitted < 0:
        raise ValueError("resample: a stream's position, output count and push cannot be negative")
    width = (K - M) // 2
    if emitted != frames_final(pushed, M, width) * L:
        raise ValueError(f"resample: a stream of {pushed} samples has emitted {frames_final(pushed, M, width) * L} outputs, not {emitted}")
    end = pushed + n_in
    if end >= 1 << 31 or out_len(end, L, M) >= 1 << 31:
        raise ValueError("resample: the stream would hold 2^31 samples or more")
    if final:
        if end < 1:
            raise ValueError("resample: an empty stream")
        e1 = out_len(end, L, M)
    else:
        e1 = max(emitted, frames_final(end, M, width) * L)
    carry_in = pushed - max(0, (emitted // L) * M - width)
    carry_out = 0 if final else end - max(0, (e1 // L) * M - width)
    if carry_in > CARRY or carry_out > CARRY:
        raise ValueError(f"resample: a carry of {max(carry_in, carry_out)} samples exceeds the {CARRY} a stream keeps")
    return dict(o_lo=emitted, n_out=e1 - emitted, emitted=e1, carry_in=carry_in, carry_out=carry_out, total=end if final else -1)

"""Host side of the device time scaler (csrc/timescale.hip, `CodecEngine.time_scale`): the speed as a ratio, the lengths, the window
table, the packed-segment arithmetic and a NumPy twin of the overlap-add.  Nothing here touches the GPU.

Waveform-similarity overlap-add at 24 kHz.  A segment x of n samples reads as zero outside [0, n):
    num = round(100 speed), den = 100          n_out = ceil(n den / num)          F = ceil(n_out / HS) + 1 frames
    a_k = floor(k HS num / den)                s_0 = -HS
    k >= 1:  t[j] = x[s_{k-1} + HS + j],  c(d) = sum_{j<N} t[j] x[a_k - HS + d + j],  d in [-D, D)
             d_k = arg max c (equal c: the smallest |d|, then the negative one),  s_k = a_k - HS + d_k
    y[(k-1) HS + j] = w[j + HS] x[s_{k-1} + HS + j] + w[j] x[s_k + j],  0 <= j < HS,  w[j] = 0.5 - 0.5 cos(2 pi j / N)
The search (the path s) runs on the device only; `apply` is the overlap-add given a path.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

N = 1024             # csrc/kernels.hpp TS_N: window
HS = 512             # TS_HS: synthesis hop
D = 256              # TS_D: search radius, candidates -D .. D-1
DEN = 100
NUM_MIN, NUM_MAX = 50, 200
REACH = 4096         # what the library keeps free below 2^31: a frame reaches past the input and positions are int32


def quantize(speed) -> Tuple[int, int]:
    """(num, den) = (round(100 speed), 100); ValueError outside 0.5 .. 2.0"""
    try:
        num = int(round(100.0 * float(speed)))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"time_scale: speed must be a number from 0.5 to 2.0 (got {speed!r})") from None
    if not NUM_MIN <= num <= NUM_MAX:
        raise ValueError(f"time_scale: speed must lie in 0.5 .. 2.0 (got {speed!r})")
    return num, DEN


def out_len(n: int, num: int, den: int = DEN) -> int:
    """ceil(n den / num), in Python integers"""
    return -(-int(n) * int(den) // int(num))


def frames(n_out: int) -> int:
    """ceil(n_out / HS) + 1: the entries of a segment's path"""
    return -(-int(n_out) // HS) + 1


def window() -> np.ndarray:
    """float64 [N] periodic Hann table; w[j] + w[j + HS] = 1"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def plan(speed, off) -> Tuple[int, int, np.ndarray, np.ndarray]:
    """(num, den, off_out, path_off) of scaling the packed segments at `off` (n_seg + 1 sample offsets) by `speed`; raises ValueError
    for everything the library must not be launched with"""
    num, den = quantize(speed)
    if num == den:
        raise ValueError("time_scale: the speed is 1, there is nothing to scale")
    off = [int(v) for v in off]
    if len(off) < 2 or off[0] != 0:
        raise ValueError("time_scale: offsets must start at 0 and hold at least one segment")
    if len(off) - 1 > 65535:
        raise ValueError("time_scale: at most 65535 segments in a pack")
    out, path = [0], [0]
    for i in range(len(off) - 1):
        n = off[i + 1] - off[i]
        if n <= 0:
            raise ValueError(f"time_scale: segment {i} is empty or the offsets do not ascend")
        m = out_len(n, num, den)
        out.append(out[-1] + m)
        path.append(path[-1] + frames(m))
    if off[-1] >= (1 << 31) - REACH or out[-1] >= 1 << 31:
        raise ValueError("time_scale: the pack would hold 2^31 samples or more")
    return num, den, np.asarray(out, dtype=np.int64), np.asarray(path, dtype=np.int64)


def apply(x, speed, path) -> np.ndarray:
    """the overlap-add of ONE segment along `path` (its frames(n_out) frame starts) in float32 -- the table rounded to float32, two
    products and one sum, each rounded: what the kernel's second phase computes, bit for bit"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    num, den = quantize(speed)
    n = x.shape[0]
    if n < 1:
        raise ValueError("time_scale: an empty segment")
    n_out = out_len(n, num, den)
    s = np.asarray(path, dtype=np.int64).reshape(-1)
    if s.shape[0] != frames(n_out):
        raise ValueError(f"time_scale: {n} samples at {num}/{den} take a path of {frames(n_out)} frames, got {s.shape[0]}")
    w = window().astype(np.float32)
    m = np.arange(n_out, dtype=np.int64)
    k1, j = m // HS, m % HS

    def read(g):
        ok = (g >= 0) & (g < n)
        return np.where(ok, x[np.where(ok, g, 0)], np.float32(0.0)).astype(np.float32)

    return w[j + HS] * read(s[k1] + HS + j) + w[j] * read(s[k1 + 1] + j)

"""Host side of the device time scaler (csrc/timescale.hip, `CodecEngine.time_scale`): the speed as a ratio, the lengths, the window
table, the packed-segment arithmetic and a NumPy twin of the overlap-add.  Nothing here touches the GPU.

Waveform-similarity overlap-add at 24 kHz.  A segment x of n samples reads as zero outside [0, n):
    num = round(100 speed), den = 100          n_out = ceil(n den / num)          F = ceil(n_out / HS) + 1 frames
    a_k = floor(k HS num / den)                s_0 = -HS
    k >= 1:  t[j] = x[s_{k-1} + HS + j],  c(d) = sum_{j<N} t[j] x[a_k - HS + d + j],  d in [-D, D)
             d_k = arg max c (equal c: the smallest |d|, then the negative one),  s_k = a_k - HS + d_k
    y[(k-1) HS + j] = w[j + HS] x[s_{k-1} + HS + j] + w[j] x[s_k + j],  0 <= j < HS,  w[j] = 0.5 - 0.5 cos(2 pi j / N)
The search (the path s) runs on the device only; `apply` is the overlap-add given a path.

Streams (`CodecEngine.time_scale_stream_step`, ctts_time_scale_stream_step): the signal arrives in pushes and the output leaves in chunks
whose concatenation is the one-shot result.  With n_avail samples pushed and more to come, frame k >= 1 may run once
    need(k) = max(a_{k-1} + D + N - 1, a_k - HS + D + N - 1) <= n_avail          (the template's reach at d_{k-1} = D - 1; the span's end)
K(n_avail) = `frames_final` is the largest such k; a push emits y[HS K_prev, HS K_now) and the last one, which knows the total, the
rest.  After K frames nothing below base(K) = max(0, a_K - HS - D) is read again: the stream keeps x[base(K), n_avail), fewer than
CARRY samples (`stream_plan` does this arithmetic in Python integers; the host never reads the path).
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
CARRY = 2560         # TS_CARRY: floats of a stream's carry.  After a step n_avail < need(K + 1) and base(K) >= a_K - HS - D, so the carry
#                      is at most need(K + 1) - 1 - base(K) = max(HS, a_{K+1} - a_K) + 2 D + N - 2 <= 2558 (a_{K+1} - a_K <= 2 HS = 1024)


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


def a_of(k: int, num: int, den: int = DEN) -> int:
    """a_k = floor(k HS num / den): the analysis position of frame k"""
    return int(k) * HS * int(num) // int(den)


def need(k: int, num: int, den: int = DEN) -> int:
    """the samples a stream must hold before frame k may run: one past the furthest position the frame can read (0 for frame 0,
    which is not searched)"""
    k = int(k)
    if k < 1:
        return 0
    return max(a_of(k - 1, num, den) + D + N - 1, a_of(k, num, den) - HS + D + N - 1)


def frames_final(n_avail: int, num: int, den: int = DEN) -> int:
    """K(n_avail): the largest k with need(k) <= n_avail; monotone in n_avail"""
    n_avail = int(n_avail)
    k = n_avail * int(den) // (HS * int(num)) + 2          # need(k) > a_k + D >= k HS num / den: above every k that may run
    while k > 0 and need(k, num, den) > n_avail:
        k -= 1
    return k


def base(k: int, num: int, den: int = DEN) -> int:
    """after k frames no position below this is read again"""
    return max(0, a_of(k, num, den) - HS - D)


def stream_plan(speed, pushed: int, n_in: int, final: bool) -> dict:
    """One push of a stream in Python integers: `pushed` samples are in, `n_in` arrive, `final` says they are the last.  -> num, den,
    k_prev, k_now (the step runs frames k_prev < k <= k_now), n_out (the samples it emits: y[HS k_prev, HS k_now), or up to
    out_len(total) at the end), n_path (path entries: one per frame, and s_0 with frame 1), carry_in / carry_out (the samples kept
    in front of and behind the step), total (-1 while not final).  ValueError for everything the library must not be launched with."""
    num, den = quantize(speed)
    if num == den:
        raise ValueError("time_scale: the speed is 1, there is nothing to scale")
    pushed, n_in = int(pushed), int(n_in)
    if pushed < 0 or n_in < 0:
        raise ValueError("time_scale: a stream's position and push cannot be negative")
    n_avail = pushed + n_in
    if n_avail >= (1 << 31) - REACH:
        raise ValueError("time_scale: the stream would hold 2^31 samples or more")
    k_prev = frames_final(pushed, num, den)
    if final:
        if n_avail < 1:
            raise ValueError("time_scale: an empty stream")
        m = out_len(n_avail, num, den)
        k_now = frames(m) - 1
        n_out = m - HS * k_prev
    else:
        k_now = frames_final(n_avail, num, den)
        n_out = HS * (k_now - k_prev)
    carry_in = pushed - base(k_prev, num, den)
    carry_out = 0 if final else n_avail - base(k_now, num, den)
    if carry_in > CARRY or carry_out > CARRY:
        raise ValueError(f"time_scale: a carry of {max(carry_in, carry_out)} samples exceeds the {CARRY} a stream keeps")
    return dict(num=num, den=den, k_prev=k_prev, k_now=k_now, n_out=n_out, n_path=k_now - k_prev + (1 if k_prev == 0 and k_now > 0 else 0),
                carry_in=carry_in, carry_out=carry_out, total=n_avail if final else -1)


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

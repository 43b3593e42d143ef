"""The look-ahead peak limiter, the host side and the NumPy twin (csrc/limiter.hip is the device side; nothing here touches the GPU).
The definition, once, for one segment x[0..n) at rate fs with a float32 pre-gain g32:

  W, C32, T    W = fs // 100 samples is 10 ms (fs in 8000 .. 48000: W = 80 .. 480);  C32 = float32(loudness.CEILING), the -1 dBFS sample
               peak;  T = float32(C32 * float32(1 - 2**-22)), four float32 ulps under it: the roundings of steps 1 and 5 cannot carry a
               sample above C32.
  1 pre-gain   u[i] = g32 * x[i] in float32, one rounding.
  2 required   r[i] = 1 where |u[i]| <= T, else T / |u[i]| (a correctly rounded float32 division).  A NaN sample has r = 1 and
               passes through as NaN.
  3 minimum    m[j] = min{ r[k] : |k - j| <= W, 0 <= k < n } for j in [-W, n + W): outside the segment there is silence, which needs
               no gain.
  4 smoothing  S[i] = sum of m[j] over |j - i| <= W in float64;  s[i] = float32(S[i] / (2 W + 1)), a float64 division and one rounding.
  5 output     y[i] = s[i] * u[i] in float32, one rounding.

Every m[j] in sample i's box contains r[i], so s[i] <= r[i] and |y[i]| <= C32; a segment with no sample above T has s == 1 exactly and
y == u bit for bit.  The limiter never raises a sample (s <= 1) and never goes below the segment's smallest r.

THE CONDITION: the float64 sum of step 4 has at most 961 float32 terms in (0, 1].  While min r >= 2**-19 (g32 * peak up to about
4e5, far beyond what the +30 dB cap and a sane waveform produce) every term is a multiple of 2**-42, the sum is exact and does not
depend on the order of summation: a direct sum, a sliding sum and sums of partial sums all give the same bits.  Outside the
condition the twin and the device may differ in s's last bit; the peak bound still holds.

One record per segment (`STATS`, 16 bytes, written on the device): the pre-gain, min s, the samples with |u| > T, the samples with
s < 1.  A segment's samples and record do not depend on what it is packed with.

A STREAM (`stream_plan`, `StreamLimiter`, ctts_peak_limit_stream_step): the segment arrives in pushes.  y[i] depends on x[i - 2 W .. i + 2 W],
so with P samples pushed and more to come the samples [0, P - 2 W) are decided: a stream lags by 2 W samples (20 ms), and its last push
emits the rest.  The chunks of a stream, concatenated, are `limit_segment` of the concatenated pushes -- bit for bit under THE CONDITION,
however the signal was cut -- and after the last push its record is the segment's.  A stream keeps its last min(P, 4 W) raw samples:
sample P - 2 W, the first the next push decides, needs r from P - 4 W on."""
from __future__ import annotations

import numpy as np

from . import loudness as LN

C32 = np.float32(LN.CEILING)
T = np.float32(C32 * np.float32(1.0 - 2.0 ** -22))
R_MIN = 2.0 ** -19                              # THE CONDITION: min r of every segment stays at or above this
TILE = 2048                                     # samples per workgroup of csrc/limiter.hip (LM_TILE): the tests put segments at its edges

CARRY = 4 * 480                                 # floats of one carry buffer of a stream (4 W at 48 kHz; csrc/kernels.hpp LM_CARRY)
GAIN_DB_MAX = 30.0                              # the public make-up gain of a stream lies in -30 .. +30 dB

# one record per segment (16 bytes, csrc/limiter.hip LmStats)
STATS = np.dtype([("g32", "<f4"), ("min_gain", "<f4"), ("n_over", "<i4"), ("n_touched", "<i4")])


def check_flag(v, who: str = "limiter") -> bool:
    """None, a bool (NumPy's too) -> bool; anything else is refused: 1 or "yes" would be a guess"""
    if v is None:
        return False
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{who}: the limiter is switched by True or False (got {v!r})")
    return bool(v)


def per_row(limiter, n: int, who: str = "limiter"):
    """one flag or one per row -> a checked list of n bools; None when no row asks for the limiter"""
    if limiter is None:
        return None
    vals = [limiter] * n if np.ndim(limiter) == 0 else list(limiter)
    if len(vals) != n:
        raise ValueError(f"{who}: one limiter flag per row, or one for all")
    vals = [check_flag(v, who) for v in vals]
    return vals if any(vals) else None


def tables(n_total: int, offsets=None, rates=None, gains=None):
    """every table of a call, checked: (off int64 [n_seg + 1], rates int32 [n_seg], gains float32 [n_seg]).  ValueError: what
    ctts_peak_limit_ragged would refuse, before anything is uploaded."""
    off = np.array([0, n_total], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or np.any(np.diff(off) <= 0):
        raise ValueError("limiter: the offsets ascend from 0 and no segment is empty")
    if int(off[-1]) != n_total:
        raise ValueError("limiter: the offsets do not cover the tensor")
    if n_total >= (1 << 31) - 4096:
        raise ValueError("limiter: the pack holds 2^31 - 4096 samples or more")
    n_seg = len(off) - 1
    if n_seg > 65535:
        raise ValueError("limiter: more than 65535 segments")
    if rates is None:
        rates = [24000] * n_seg
    elif np.ndim(rates) == 0:
        rates = [rates] * n_seg
    rates = [LN.check_rate(r) for r in rates]
    if len(rates) != n_seg:
        raise ValueError("limiter: one rate per segment, or one for all")
    if gains is None:
        g = np.ones(n_seg, dtype=np.float32)
    else:
        g = np.full(n_seg, gains, dtype=np.float32) if np.ndim(gains) == 0 else np.ascontiguousarray(gains, dtype=np.float32)
        if g.ndim != 1 or len(g) != n_seg:
            raise ValueError("limiter: one pre-gain per segment, or one for all")
        if not np.all(np.isfinite(g) & (g > 0)):
            raise ValueError("limiter: a pre-gain is a positive finite number")
    return off, np.array(rates, dtype=np.int32), g


def required_gain(u: np.ndarray) -> np.ndarray:
    """step 2: r float32 of u float32"""
    a = np.abs(u)
    r = np.ones(len(u), dtype=np.float32)
    over = a > T                                                  # False for a NaN
    r[over] = T / a[over]
    return r


def window_min(r: np.ndarray, W: int) -> np.ndarray:
    """step 3: m[j], j in [-W, n + W), float32 [n + 2 W] -- by doubling: min is idempotent, two overlapping power-of-two windows
    cover the 2 W + 1"""
    L = 2 * W + 1
    a = np.concatenate([np.ones(2 * W, np.float32), r, np.ones(2 * W, np.float32)])      # a[e] = r[e - 2 W]
    w = 1
    while 2 * w <= L:
        a = np.minimum(a[:-w], a[w:])                             # a[e] = min r over [e, e + 2 w)
        w *= 2
    return np.minimum(a[: len(r) + 2 * W], a[L - w: L - w + len(r) + 2 * W])


def smooth(m: np.ndarray, W: int) -> np.ndarray:
    """step 4: s float32 [n] of m [n + 2 W] -- the box sums by the binary digits of 2 W + 1 over power-of-two window sums, all exact
    under THE CONDITION"""
    L = 2 * W + 1
    n = len(m) - 2 * W
    a = m.astype(np.float64)                                      # a[e] = sum of m over [e, e + w)
    S = np.zeros(n)
    pos, w = 0, 1
    while w <= L:
        if L & w:
            S += a[pos: pos + n]
            pos += w
        if 2 * w <= L:
            a = a[:-w] + a[w:]
        w *= 2
    return (S / float(L)).astype(np.float32)


def gain_curve(x: np.ndarray, fs: int, g32=1.0, W=None):
    """steps 1 .. 4 of one segment -> (u float32, r float32, s float32); `W` overrides fs // 100 (the hand-computed examples)"""
    W = LN.check_rate(fs) // 100 if W is None else int(W)
    u = np.float32(g32) * np.ascontiguousarray(x, dtype=np.float32)
    r = required_gain(u)
    return u, r, smooth(window_min(r, W), W)


def limit_segment(x: np.ndarray, fs: int, g32=1.0, W=None):
    """one segment -> (y float32, its record)"""
    u, r, s = gain_curve(x, fs, g32, W)
    rec = np.zeros((), dtype=STATS)
    rec["g32"], rec["min_gain"], rec["n_over"], rec["n_touched"] = np.float32(g32), s.min(), int((np.abs(u) > T).sum()), int((s < 1).sum())
    return s * u, rec


def limit(x: np.ndarray, offsets=None, rates=None, gains=None):
    """the NumPy twin of CodecEngine.peak_limit on a host array -> (y float32, stats STATS [n_seg])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    off, rates, g = tables(len(x), offsets, rates, gains)
    y = np.empty_like(x)
    stats = np.zeros(len(off) - 1, dtype=STATS)
    for s in range(len(off) - 1):
        y[off[s]: off[s + 1]], stats[s] = limit_segment(x[off[s]: off[s + 1]], int(rates[s]), g[s])
    return y, stats


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
def check_gain_db(v, who: str = "gain_db"):
    """the make-up gain of a limited stream, in dB in front of the limiter: None -> None; a finite number in -30 .. +30 -> the
    float32 pre-gain g32 = float32(10 ** (v / 20)); anything else (a bool, a string, NaN, beyond the range) is refused"""
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) \
            or not -GAIN_DB_MAX <= float(v) <= GAIN_DB_MAX:
        raise ValueError(f"{who}: the make-up gain is a finite number of dB in -30 .. +30 (got {v!r})")
    return np.float32(10.0 ** (float(v) / 20.0))


def stream_plan(W: int, pushed: int, emitted: int, n_in: int, final: bool) -> dict:
    """One push of a stream in Python integers: `pushed` samples are in and `emitted` out, `n_in` arrive, `final` says they are the
    last (a stream may end empty: it emits nothing).  -> total (= pushed + n_in), e_lo (= emitted), n_out (the step emits samples [emitted, E')), emitted (E': total on the last
    push, else max(0, total - 2 W)), carry_in / carry_out (the raw samples kept in front of and behind the step: [pushed - carry_in,
    pushed) and [total - carry_out, total); min(., 4 W), 0 behind the last).  ValueError for what the library must not be launched with."""
    W, pushed, emitted, n_in = int(W), int(pushed), int(emitted), int(n_in)
    if not 80 <= W <= 480:
        raise ValueError(f"limiter: W = fs // 100 lies in 80 .. 480 (got {W})")
    if pushed < 0 or n_in < 0 or emitted < 0:
        raise ValueError("limiter: a stream's position, output count and push cannot be negative")
    if emitted != max(0, pushed - 2 * W):
        raise ValueError(f"limiter: a stream of {pushed} samples has emitted {max(0, pushed - 2 * W)}, not {emitted}")
    total = pushed + n_in
    if total >= 1 << 31:
        raise ValueError("limiter: the stream would hold 2^31 samples or more")
    e1 = total if final else max(0, total - 2 * W)
    return dict(total=total, e_lo=emitted, n_out=e1 - emitted, emitted=e1, carry_in=min(pushed, 4 * W),
                carry_out=0 if final else min(total, 4 * W))


class StreamLimiter:
    """the NumPy twin of one limiter stream at rate fs with the float32 pre-gain g32: `push(x, final) -> y` float32, `stats` the STATS
    record counted over the samples emitted so far.  The gain curve is computed on carry ++ x: an emitted sample lies 2 W or more
    from either end of that buffer unless the end is the signal's own, so the silence assumed outside it reaches no emitted sample."""

    def __init__(self, fs: int, g32=1.0):
        self.fs, self.W, self.g32 = LN.check_rate(fs), LN.check_rate(fs) // 100, np.float32(g32)
        if not (np.isfinite(self.g32) and self.g32 > 0):
            raise ValueError("limiter: a pre-gain is a positive finite number")
        self.pushed = self.emitted = 0
        self.done = False
        self.carry = np.zeros(0, dtype=np.float32)
        self.stats = np.zeros((), dtype=STATS)
        self.stats["g32"], self.stats["min_gain"] = self.g32, 1.0

    def push(self, x, final: bool = False) -> np.ndarray:
        if self.done:
            raise ValueError("limiter: the stream has had its last push")
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        p = stream_plan(self.W, self.pushed, self.emitted, len(x), final)
        assert p["carry_in"] == len(self.carry)
        buf = np.concatenate([self.carry, x])
        base = self.pushed - len(self.carry)                          # the signal position of buf[0]
        lo, hi = self.emitted - base, p["emitted"] - base
        if hi > lo:
            u, _, s = gain_curve(buf, self.fs, self.g32)
            u, s = u[lo:hi], s[lo:hi]
            y = s * u
            self.stats["min_gain"] = min(self.stats["min_gain"], s.min())
            self.stats["n_over"] += int((np.abs(u) > T).sum())
            self.stats["n_touched"] += int((s < 1).sum())
        else:
            y = np.zeros(0, dtype=np.float32)
        self.carry = buf[len(buf) - p["carry_out"]:].copy()
        self.pushed, self.emitted, self.done = p["total"], p["emitted"], bool(final)
        return y

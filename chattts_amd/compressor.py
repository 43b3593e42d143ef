"""The dynamic range compressor, the host side and the NumPy twin (csrc/compressor.hip is the device side; nothing here touches the
GPU).  A feed-forward compressor with look-ahead, stage 3 1/2 of the output chain: behind trim_pauses, in front of loudness_normalize.
The definition, once, for one segment x[0..n) at rate fs (what loudness.check_rate accepts: a multiple of 10 Hz in 8000 .. 48000):

  spec         True (the defaults) or a dict with any of threshold_db, ratio, knee_db, attack_ms, hold_ms (RANGES, DEFAULTS); None and
               False are off.  The defaults are starting values that nobody has listened to: there is no real checkpoint.
  1 blocks     B = fs // 1000 samples is 1 ms (8 .. 48); block b is [b B, min((b + 1) B, n)), nb = ceil(n / B) of them.  A = ceil(attack_ms)
               and H = ceil(hold_ms) blocks (1 .. 20, 0 .. 500).
  2 peak       p[b] = max |x[i]| over the block in float32; a NaN sample does not count (a block of NaNs has p = 0) and passes through
               as NaN.
  3 curve      the static gain is DATA: a float32 table of TABLE = 1024 entries that the host builds (`table`), no transcendental
               function runs on the device.  q = (bits(p) >> 18) - Q0 is p's exponent and top five mantissa bits, 32 bins per octave
               over 2^-24 <= p < 2^8;  c[b] = 1 for q < 0, table[min(q, 1023)] otherwise.  Entry q is float32(10^(G / 20)) at the
               level L = 20 log10(the bin's lower edge), in float64, with the soft knee: over = L - threshold;  G = 0 where
               2 over < -knee;  G = (1 / R - 1)(over + knee / 2)^2 / (2 knee) where 2 |over| <= knee;  G = (1 / R - 1) over beyond.
  4 hold       m[j] = min{ c[k] : j - H <= k <= j + A }, for every integer j; c[k] = 1 outside 0 <= k < nb.
  5 ramp       s[b] = float32( (sum of m[j], j = b - A .. b) / (A + 1) ): a float64 sum, a float64 division, one rounding to float32.
               Every window of the sum contains b, so s[b] <= c[b].
  6 gain       anchors a[b] = min(s[b - 1], s[b]) with s[-1] := s[0], a[nb] := s[nb - 1].  Sample i = b B + t gets
               g = float32( a[b] + (a[b + 1] - a[b]) * (t / B) ) in float64: the division, the difference (exact), the product and the
               sum each rounded once, no fused multiply-add, then one rounding to float32.  The gain is continuous across block edges
               (no zipper steps), and both anchors are <= s[b] <= c[b]: no sample gets more gain than the curve gives its block's peak.
  7 output     y[i] = g * x[i] in float32, one rounding.

THE CONDITION, which the validator and the table's host check guarantee: every table entry lies in [2^-18, 1] (the deepest, -60 dB
threshold, ratio 20, no knee at +48 dB, is 10^(-102.6 / 20) > 2^-18).  The sum of step 5 then has at most 21 float32 terms that are
multiples of 2^-41 with a total below 2^5: it is exact in float64 and independent of the order of summation.  The twin and the device
agree bit for bit.

What follows: g <= 1 everywhere; a segment whose block peaks all lie below the knee (c == 1) comes back bit for bit; y[i] depends on x
only in the blocks b - A - H - 1 .. b + A + 1 (a[b], a[b + 1] <- s[b - 1 .. b + 1] <- m[b - 1 - A .. b + 1] <- c[b - 1 - A - H .. b + 1 + A]):
the bounded window that a stream carries (below).  A segment's samples and record do not depend on what it is packed with.

Adjusted against the issue's wording, for exactness: the durations become whole blocks by ceil (a fractional attack_ms would leave
A undefined); m is defined for every integer j, not only inside the segment (s[b] near the edges sums m[j] with j < 0); p of a block
of NaNs is 0.

One record per segment (`STATS`, 16 bytes, written on the device): the smallest g, the blocks with c < 1, the samples with g < 1, the
largest block peak.

A STREAM (`stream_plan`, `StreamCompressor`, ctts_compress_stream_step): the segment arrives in pushes.  After a push `total` samples
are in and nbc = total // B blocks are complete; the c of a block is computed once, when the block is complete (on the last push: the
partial last block too, nb = ceil(total / B)).
  emits        a push that is not the last emits samples [emitted, E'), E' = max(0, nbc - A - 1) B: sample i of block b needs
               c[b - A - H - 1 .. b + A + 1], and every block up to nbc - 1 is complete.  The last push emits up to `total`, and only then
               do the edge rules apply (c = 1 beyond nb, a[nb] := s[nb - 1], the partial block's peak); s[-1] := s[0] at the true start only.
  lag          (A + 1) B samples and the open block: under A + 2 ms (7 ms at the defaults, 22 ms at most), whatever the hold.
  carried      the raw samples [E', total), fewer than (A + 2) B (`STREAM_CARRY` = 1055 at most); the c of the blocks
               [max(0, E' / B - A - H - 1), nbc), at most 2 A + H + 2 (`STREAM_HIST` = 542); the 16-byte record; the table (4 KiB, or an
               index to it).  No raw sample older than E': the hold's memory, up to 500 ms, lives in c, one float per millisecond.
  empty        a stream may end empty (total = 0, final): it emits nothing and its record is (1, 0, 0, 0).
  the contract the chunks, end to end, are `compress_segment` of the whole signal, bit for bit, however it was cut, and the record
               after the last push is that segment's: n_blocks and peak count once per block, when its c is computed; min_gain and
               n_touched over the emitted samples."""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from . import loudness as LN

TABLE = 1024                                    # entries of one gain table: 32 octaves of 32 bins
Q0 = (127 - 24) << 5                            # bits(2^-24) >> 18
ENTRY_MIN = 2.0 ** -18                          # THE CONDITION: no table entry lies below this
TILE_BLOCKS = 128                               # blocks per workgroup of the apply launch (CP_TILE): a sample tile is 128 B samples
A_MAX, H_MAX = 20, 500
B_MIN, B_MAX = 8, 48
STREAM_CARRY = (A_MAX + 2) * B_MAX - 1          # raw samples a stream carries, at most: fewer than (A + 2) B
STREAM_HIST = 2 * A_MAX + H_MAX + 2             # block gains c a stream carries, at most

RANGES = {"threshold_db": (-60, -6), "ratio": (1.5, 20), "knee_db": (0, 24), "attack_ms": (1, 20), "hold_ms": (0, 500)}
DEFAULTS = {"threshold_db": -24.0, "ratio": 3.0, "knee_db": 6.0, "attack_ms": 5.0, "hold_ms": 60.0}

# one record per segment (16 bytes, csrc/compressor.hip CpStats)
STATS = np.dtype([("min_gain", "<f4"), ("n_blocks", "<i4"), ("n_touched", "<i4"), ("peak", "<f4")])


def check(spec, who: str = "compress"):
    """None, False -> None (off); True -> the defaults; a dict with any of RANGES' keys -> the full spec, a tuple of five floats in
    RANGES' order (hashable: equal specs share one table).  ValueError: an unknown key, a bool or a non-number where a number
    belongs, NaN, a value out of range, anything else."""
    if spec is None or spec is False or (isinstance(spec, np.bool_) and not spec):
        return None
    if isinstance(spec, tuple) and len(spec) == len(RANGES) and not any(isinstance(v, (bool, np.bool_)) for v in spec):
        spec = dict(zip(RANGES, spec))          # a checked spec, as it comes back from this function
    if spec is True or (isinstance(spec, np.bool_) and spec):
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError(f"{who}: the compressor takes True, False, None or a dict with any of {', '.join(RANGES)} (got {spec!r})")
    unknown = sorted(set(spec) - set(RANGES), key=str)
    if unknown:
        raise ValueError(f"{who}: unknown compressor field {unknown[0]!r} (the fields are {', '.join(RANGES)})")
    vals = {**DEFAULTS, **spec}
    for k, v in vals.items():
        lo, hi = RANGES[k]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
            raise ValueError(f"{who}: {k} is a number in {lo} .. {hi} (got {v!r})")
    return tuple(float(vals[k]) for k in RANGES)


def per_row(compress, n: int, who: str = "compress"):
    """one spec or one per row (a list) -> a checked list of n (entries None or a spec tuple); None when no row asks for it"""
    if compress is None:
        return None
    vals = list(compress) if isinstance(compress, list) else [compress] * n
    if len(vals) != n:
        raise ValueError(f"{who}: one compressor spec per row, or one for all")
    vals = [check(v, who) for v in vals]
    return None if all(v is None for v in vals) else vals


def blocks(spec) -> tuple:
    """(A, H) of a checked spec, in blocks of 1 ms"""
    return int(math.ceil(spec[3])), int(math.ceil(spec[4]))


def law_db(level_db, spec):
    """the static curve in float64: the gain in dB at a level in dB (step 3)"""
    thr, ratio, knee = spec[0], spec[1], spec[2]
    L = np.asarray(level_db, dtype=np.float64)
    over = L - thr
    slope = 1.0 / ratio - 1.0
    G = np.where(2.0 * over < -knee, 0.0, slope * over)
    if knee > 0:
        G = np.where(2.0 * np.abs(over) <= knee, slope * (over + knee / 2.0) ** 2 / (2.0 * knee), G)
    return G


@lru_cache(maxsize=64)
def table(spec) -> np.ndarray:
    """the gain table of a checked spec, float32 [TABLE]: entry q at the lower edge of bin q, 2^(q // 32 - 24) (1 + (q % 32) / 32)"""
    q = np.arange(TABLE)
    edge = np.ldexp(1.0 + (q % 32) / 32.0, q // 32 - 24)
    t = (10.0 ** (law_db(20.0 * np.log10(edge), spec) / 20.0)).astype(np.float32)
    t = np.minimum(t, np.float32(1.0))
    assert t.min() >= ENTRY_MIN
    t.setflags(write=False)
    return t


def bin_index(p: np.ndarray) -> np.ndarray:
    """q of float32 peaks (not NaN): (bits >> 18) - Q0, int64; below 0: under the table, TABLE and above: beyond it"""
    return (np.ascontiguousarray(p, dtype=np.float32).view(np.uint32).astype(np.int64) >> 18) - Q0


def block_peaks(x: np.ndarray, B: int) -> np.ndarray:
    """step 2: p float32 [ceil(n / B)]"""
    n = len(x)
    nb = -(-n // B)
    a = np.zeros(nb * B, dtype=np.float32)
    a[:n] = np.abs(x)
    a[np.isnan(a)] = 0.0
    return a.reshape(nb, B).max(1)


def lookup(p: np.ndarray, tab: np.ndarray) -> np.ndarray:
    """step 3: c float32 of the block peaks"""
    q = bin_index(p)
    return np.where(q < 0, np.float32(1.0), tab[np.clip(q, 0, TABLE - 1)]).astype(np.float32)


def hold_min(c: np.ndarray, A: int, H: int) -> np.ndarray:
    """step 4: m[j] for j in [-A - 1, nb + 1), float32 [nb + A + 2] -- what the anchors of blocks 0 .. nb reach"""
    nb = len(c)
    ext = np.concatenate([np.ones(A + 1 + H, np.float32), c, np.ones(A + 1, np.float32)])       # ext[e] = c[e - A - 1 - H]
    nm = nb + A + 2
    m = ext[:nm].copy()                                                                          # m[j + A + 1] = min ext[j + A + 1 .. + A + H]
    for d in range(1, A + H + 1):
        np.minimum(m, ext[d: d + nm], out=m)
    return m


def ramp(m: np.ndarray, A: int) -> np.ndarray:
    """step 5: s[b] for b in [-1, nb], float32 [nb + 2], of m as hold_min returns it"""
    ns = len(m) - A
    S = np.zeros(ns, dtype=np.float64)
    for d in range(A + 1):
        S += m[d: d + ns].astype(np.float64)
    return (S / float(A + 1)).astype(np.float32)


def anchors(s: np.ndarray) -> np.ndarray:
    """step 6: a[b] for b in [0, nb], float32 [nb + 1], of s as ramp returns it (s[-1] := s[0], a[nb] := s[nb - 1])"""
    nb = len(s) - 2
    idx = np.arange(nb + 1)
    return np.minimum(s[1 + np.clip(idx - 1, 0, nb - 1)], s[1 + np.clip(idx, 0, nb - 1)])


def gain_curve(x: np.ndarray, fs: int, spec=True, B=None, A=None, H=None):
    """steps 1 .. 6 of one segment -> a dict: p, c [nb], m [nb + A + 2] (from j = -A - 1), s [nb + 2] (from b = -1), a [nb + 1],
    g float32 [n].  `B`, `A`, `H` override fs // 1000 and the spec's durations (the hand-computed examples)."""
    spec = check(spec)
    if spec is None:
        raise ValueError("compress: the spec is off")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("compress: a segment is 1-D and holds at least one sample")
    B = LN.check_rate(fs) // 1000 if B is None else int(B)
    A = blocks(spec)[0] if A is None else int(A)
    H = blocks(spec)[1] if H is None else int(H)
    p = block_peaks(x, B)
    c = lookup(p, table(spec))
    m = hold_min(c, A, H)
    s = ramp(m, A)
    a = anchors(s).astype(np.float64)
    i = np.arange(len(x))
    b, t = i // B, i % B
    g = (a[b] + (a[b + 1] - a[b]) * (t.astype(np.float64) / float(B))).astype(np.float32)
    return dict(p=p, c=c, m=m, s=s, a=a.astype(np.float32), g=g)


def compress_segment(x: np.ndarray, fs: int, spec=True, B=None, A=None, H=None):
    """one segment -> (y float32, its record)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = gain_curve(x, fs, spec, B, A, H)
    rec = np.zeros((), dtype=STATS)
    rec["min_gain"], rec["n_blocks"], rec["n_touched"], rec["peak"] = k["g"].min(), int((k["c"] < 1).sum()), int((k["g"] < 1).sum()), k["p"].max()
    return k["g"] * x, rec


def tables(n_total: int, spec, offsets=None, rates=None):
    """every table of a call, checked: (off int64 [n_seg + 1], rates int32 [n_seg], par int32 [n_seg, 4] (A, H, table index or -1
    for a segment that is copied through, 0), tabs float32 [n_tab, TABLE], specs).  ValueError: what ctts_compress_ragged would
    refuse, before anything is uploaded."""
    off = np.array([0, n_total], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or np.any(np.diff(off) <= 0):
        raise ValueError("compress: the offsets ascend from 0 and no segment is empty")
    if int(off[-1]) != n_total:
        raise ValueError("compress: the offsets do not cover the tensor")
    if n_total >= (1 << 31) - 4096:
        raise ValueError("compress: the pack holds 2^31 - 4096 samples or more")
    n_seg = len(off) - 1
    if n_seg > 65535:
        raise ValueError("compress: more than 65535 segments")
    if rates is None:
        rates = [24000] * n_seg
    elif np.ndim(rates) == 0:
        rates = [rates] * n_seg
    rates = [LN.check_rate(r) for r in rates]
    if len(rates) != n_seg:
        raise ValueError("compress: one rate per segment, or one for all")
    specs = per_row(spec, n_seg)
    if specs is None:
        raise ValueError("compress: no segment asks for the compressor")
    distinct = sorted({s for s in specs if s is not None})
    par = np.zeros((n_seg, 4), dtype=np.int32)
    for i, s in enumerate(specs):
        par[i, :3] = (1, 0, -1) if s is None else (*blocks(s), distinct.index(s))
    return off, np.array(rates, dtype=np.int32), par, np.stack([table(s) for s in distinct]), specs


def scratch_floats(n_total: int, n_seg: int) -> int:
    """compress_blocks of csrc/kernels.hpp: segment s's block gains start at float off[s] // 8 + s of the scratch"""
    return n_total // 8 + n_seg + 1


def compress(x: np.ndarray, spec=True, offsets=None, rates=None):
    """the NumPy twin of CodecEngine.compress on a host array -> (y float32, stats STATS [n_seg]); a segment whose spec is off comes
    back as it is, with the record (1, 0, 0, 0)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    off, rates, _, _, specs = tables(len(x), spec, offsets, rates)
    y = x.copy()
    stats = np.zeros(len(off) - 1, dtype=STATS)
    stats["min_gain"] = 1.0
    for s in range(len(off) - 1):
        if specs[s] is not None:
            y[off[s]: off[s + 1]], stats[s] = compress_segment(x[off[s]: off[s + 1]], int(rates[s]), specs[s])
    return y, stats


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
def stream_plan(B: int, A: int, pushed: int, emitted: int, n_in: int, final: bool, H: int = H_MAX) -> dict:
    """One push of a stream in Python integers: `pushed` samples are in and `emitted` out, `n_in` arrive, `final` says they are the
    last (a stream may end empty: it emits nothing).  -> total (= pushed + n_in), e_lo (= emitted), n_out (the step emits samples
    [emitted, E')), emitted (E': total on the last push, else max(0, total // B - A - 1) B), carry_in / carry_out (the raw samples kept
    in front of and behind the step: [emitted, pushed) and [E', total); 0 behind the last), c_keep (the block gains kept behind the
    step, those of the blocks [max(0, E' / B - A - H - 1), total // B); 0 behind the last; `H` defaults to the longest hold, the
    bound).  ValueError for what the library must not be launched with."""
    B, A, H, pushed, emitted, n_in = int(B), int(A), int(H), int(pushed), int(emitted), int(n_in)
    if not B_MIN <= B <= B_MAX:
        raise ValueError(f"compress: B = fs // 1000 lies in {B_MIN} .. {B_MAX} (got {B})")
    if not 1 <= A <= A_MAX or not 0 <= H <= H_MAX:
        raise ValueError(f"compress: the attack is 1 .. {A_MAX} blocks and the hold 0 .. {H_MAX} (got {A} and {H})")
    if pushed < 0 or n_in < 0 or emitted < 0:
        raise ValueError("compress: a stream's position, output count and push cannot be negative")
    if emitted != max(0, pushed // B - A - 1) * B:
        raise ValueError(f"compress: a stream of {pushed} samples has emitted {max(0, pushed // B - A - 1) * B}, not {emitted}")
    total = pushed + n_in
    if total >= 1 << 31:
        raise ValueError("compress: the stream would hold 2^31 samples or more")
    nbc = total // B
    e1 = total if final else max(0, nbc - A - 1) * B
    return dict(total=total, e_lo=emitted, n_out=e1 - emitted, emitted=e1, carry_in=pushed - emitted, carry_out=0 if final else total - e1,
                c_keep=0 if final else nbc - max(0, e1 // B - A - H - 1))


class StreamCompressor:
    """the NumPy twin of one compressor stream at rate fs with `spec`: `push(x, final) -> y` float32, `stats` the STATS record so far.
    It holds what the definition says a stream carries and nothing else: `carry`, the raw samples [emitted, pushed), and `hist`, the c
    of the blocks [h0, pushed // B)."""

    def __init__(self, fs: int, spec=True):
        self.spec = check(spec)
        if self.spec is None:
            raise ValueError("compress: the spec is off")
        self.fs, self.B = LN.check_rate(fs), LN.check_rate(fs) // 1000
        self.A, self.H = blocks(self.spec)
        self.tab = table(self.spec)
        self.pushed = self.emitted = self.h0 = 0
        self.done = False
        self.carry = np.zeros(0, dtype=np.float32)
        self.hist = np.zeros(0, dtype=np.float32)
        self.stats = np.zeros((), dtype=STATS)
        self.stats["min_gain"] = 1.0

    def push(self, x, final: bool = False) -> np.ndarray:
        if self.done:
            raise ValueError("compress: the stream has had its last push")
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        B, A, H = self.B, self.A, self.H
        p = stream_plan(B, A, self.pushed, self.emitted, len(x), final, H)
        assert p["carry_in"] == len(self.carry) and self.pushed // B - self.h0 == len(self.hist)
        buf = np.concatenate([self.carry, x])
        base, total, e1 = self.emitted, p["total"], p["emitted"]      # buf[0] is sample `base` of the signal
        nbc0 = self.pushed // B
        nbc1 = -(-total // B) if final else total // B
        if nbc1 > nbc0:                                               # the blocks this push completes (the last push: the partial one too)
            pk = block_peaks(buf[nbc0 * B - base: min(nbc1 * B, total) - base], B)
            c_new = lookup(pk, self.tab)
            self.stats["n_blocks"] += int((c_new < 1).sum())
            self.stats["peak"] = max(self.stats["peak"], pk.max())
            call = np.concatenate([self.hist, c_new])
        else:
            call = self.hist
        if e1 > base:
            eb0, eb1 = base // B, -(-e1 // B)                         # the blocks emitted: [eb0, eb1)
            k = np.arange(eb0 - 1 - A - H, eb1 + A + 1)               # the blocks their windows reach; beyond nbc1 on the last push only
            inside = (k >= 0) & (k < nbc1)
            assert np.all(k[inside] >= self.h0)
            cext = np.ones(len(k), dtype=np.float32)
            cext[inside] = call[k[inside] - self.h0]
            nm = eb1 - eb0 + 2 + A
            m = cext[:nm].copy()                                      # m[j], j from eb0 - 1 - A
            for d in range(1, A + H + 1):
                np.minimum(m, cext[d: d + nm], out=m)
            s = ramp(m, A)                                            # s[b], b from eb0 - 1
            b = np.arange(eb0, eb1 + 1)
            a = np.minimum(s[np.maximum(b - 1, 0) - (eb0 - 1)], s[np.minimum(b, nbc1 - 1) - (eb0 - 1)]).astype(np.float64)
            i = np.arange(base, e1)
            bi, t = i // B - eb0, i % B
            g = (a[bi] + (a[bi + 1] - a[bi]) * (t.astype(np.float64) / float(B))).astype(np.float32)
            y = g * buf[: e1 - base]
            self.stats["min_gain"] = min(self.stats["min_gain"], g.min())
            self.stats["n_touched"] += int((g < 1).sum())
        else:
            y = np.zeros(0, dtype=np.float32)
        h1 = nbc1 if final else nbc1 - p["c_keep"]
        self.carry = buf[len(buf) - p["carry_out"]:].copy()
        self.hist = call[h1 - self.h0:].copy()
        self.h0 = h1
        self.pushed, self.emitted, self.done = total, e1, bool(final)
        return y

"""Pause control, the host side: trim the silence at a segment's edges and cap its inner pauses (csrc/pauses.hip is the device side;
nothing here touches the GPU).  The definition, once, for a segment of n >= 1 float32 samples at rate fs (8000 .. 48000 Hz):

  frames     F = fs // 100 samples; frame j is [j F, min((j + 1) F, n)), nF = ceil(n / F) of them, the last possibly partial.  Every
             duration of the spec becomes frames by ceil(ms / 10): P (the longest inner pause, >= 1), lead, tail, pad.
  activity   thr = float32(10^(threshold_db / 20)) (float64, rounded once).  A frame is active iff some sample has !(|x| < thr): a NaN
             makes its frame active.
  speech     pa(j) the last active frame <= j, na(j) the first >= j (either may be absent).  Frame j is speech iff j - pa <= pad or
             na - j <= pad.  Every other frame is quiet and lies in the run [r0, r1): r0 = pa + pad + 1 (0 without pa), r1 = na - pad
             (nF without na), R = r1 - r0, k = j - r0.
  rules      kept: a speech frame;  in a leading run (no pa) the lead frames next to the speech, k >= R - lead;  in a trailing run (no
             na) k < tail;  with no active frame at all k < max(1, lead + tail) (an output is never empty; what goes counts as tail);
             every frame of an inner run with R <= P;  of a longer inner run, with h = ceil(P / 2) and t = P - h, k < h or k >= R - t.
  crossfade  the kept frame k = h - 1 of a shortened inner run fades into b = r1 - t - 1, the frame in front of the kept tail (both full
             frames):  y[i] = fadd(fmul(w_out[i], x[(r0 + h - 1) F + i]), fmul(w_in[i], x[b F + i])),  w_in[i] = float32(0.5 - 0.5
             cos(pi (i + 0.5) / F)), w_out[i] = w_in[F - 1 - i]; products and sum rounded separately, no fused multiply-add.  Every
             other kept sample is copied bit for bit; the output is the kept frames in order.
  record     RECORD, eight int32: frames, active frames, speech frames, lead frames removed, tail frames removed, inner runs shortened,
             inner frames removed, output samples.  A segment that is copied through (spec None) reports (frames, 0, 0, 0, 0, 0, 0, n).

`apply` is the NumPy twin of the kernels, vectorised from these formulas; `tables` builds what ctts_trim_pauses_ragged takes.

A STREAM (`StreamPauses`, `stream_walk`, ctts_trim_pauses_stream_step) is opened with a rate fs and a checked spec; samples arrive in pushes
of any size, 0 included, and the last push is marked final.  With X the concatenation of the pushes and n its length:

  result     for n >= 1 the chunks the pushes emit, end to end, are apply(X, fs, spec)[0] bit for bit, however X was cut, and after the
             final push the stream's record is apply's RECORD.  A stream closed with n = 0 emits nothing and reports an all-zero record.
  schedule   a non-final push considers complete frames only (a partial frame waits: at most F - 1 samples) and emits frames in order up
             to the first that is not decided.  With pa the last active frame <= j among the frames seen:  (1) an active frame decides
             every frame up to itself by the rules above -- a leading run or an inner run, crossfade included;  (2) before the first
             active frame nothing is decided (a leading run, or no active frame at all);  (3) j - pa <= pad: speech, emitted as it is;
             (4) else, with k = j - (pa + pad + 1) and k0 = min(h - 1, tail): k < k0 is emitted as it is -- it is kept unmixed whether the
             run turns out short, long or trailing, or speech resumes within pad -- and k >= k0 waits for an active frame or the end.
             The final push decides what is left, the last and possibly partial frame included.
  lags       through speech less than one frame (10 ms); inside a pause the first k0 frames of the run go out (100 ms with the defaults,
             behind the 30 ms of pad) and then nothing until speech resumes or the stream ends; nothing before the first active frame.
  state      what waits is two ranges of the current run's frames, a function of the run's length m so far (frames k < m seen) alone:
             before the first active frame  [0, min(m, A1)) and [max(A1, m - A2), m),  A1 = max(1, lead + tail), A2 = lead + pad;  behind
             speech  [k0, m) while m - pad <= P (the run may still be short), afterwards  [k0, min(m, H)) and [max(H, m - L), m),
             H = max(h, tail), L = t + 1 + pad  (the frames a long or trailing run keeps at its front; the crossfade partner, the kept
             tail and the pad at its back).  `stream_need` is the most frames that ever wait, max(A1 + A2, P + pad - k0, H - k0 + L):
             it depends on the spec, not on how long a pause lasts.  A device slot holds STREAM_FRAMES frames and a partial one; a spec
             that needs more is refused when the stream is opened."""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from functools import lru_cache

import numpy as np

FS_MIN, FS_MAX = 8000, 48000
ROW = 8                                          # int32 per segment row (PA_ROW): F, pad, lead, tail, P (0: copy), thr bits, fade offset, 0
REC = 8                                          # int32 per segment record (PA_REC)
RECORD = ("frames", "active", "speech", "lead_removed", "tail_removed", "runs_shortened", "inner_removed", "n_out")
RANGES = {"max_pause_ms": (10, 10000), "lead_ms": (0, 10000), "tail_ms": (0, 10000), "threshold_db": (-100, 0), "pad_ms": (0, 1000)}


@dataclass(frozen=True)
class PauseSpec:
    max_pause_ms: float = 400
    lead_ms: float = 50
    tail_ms: float = 100
    threshold_db: float = -50.0
    pad_ms: float = 30

    def frames(self):
        """(P, lead, tail, pad) in frames of 10 ms"""
        return tuple(int(math.ceil(v / 10)) for v in (self.max_pause_ms, self.lead_ms, self.tail_ms, self.pad_ms))

    def thr(self) -> np.float32:
        return np.float32(10.0 ** (float(self.threshold_db) / 20.0))


def check(spec):
    """None (off), True (the defaults), a PauseSpec or a dict of its field names -> PauseSpec or None.  ValueError: an unknown key, a
    non-number, a value out of range."""
    if spec is None:
        return None
    if spec is True:
        return PauseSpec()
    if isinstance(spec, PauseSpec):
        vals = {f.name: getattr(spec, f.name) for f in fields(PauseSpec)}
    elif isinstance(spec, dict):
        unknown = sorted(set(spec) - set(RANGES), key=str)
        if unknown:
            raise ValueError(f"pauses: unknown field {unknown[0]!r} (the fields are {', '.join(RANGES)})")
        vals = dict(spec)
    else:
        raise ValueError(f"pauses: None, True, a PauseSpec or a dict of its fields (got {spec!r})")
    for k, v in vals.items():
        lo, hi = RANGES[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
            raise ValueError(f"pauses: {k} is a number in {lo} .. {hi} (got {v!r})")
    return PauseSpec(**{k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in vals.items()})


def check_rate(fs) -> int:
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or not FS_MIN <= fs <= FS_MAX:
        raise ValueError(f"pauses: the rate is an integer number of Hz in {FS_MIN} .. {FS_MAX} (got {fs!r})")
    return int(fs)


def per_row(pauses, n: int, who: str = "pauses"):
    """one spec or one per row (a list or tuple) -> a checked list of n (entries None or PauseSpec); None when nothing is asked for"""
    if pauses is None:
        return None
    vals = list(pauses) if isinstance(pauses, (list, tuple)) else [pauses] * n
    if len(vals) != n:
        raise ValueError(f"{who}: one pause spec per row, or one for all")
    vals = [check(v) for v in vals]
    return None if all(v is None for v in vals) else vals


@lru_cache(maxsize=None)
def fade_table(F: int) -> np.ndarray:
    """w_in of a frame of F samples, float32 [F]; w_out is its reverse"""
    w = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / F)).astype(np.float32)
    w.setflags(write=False)
    return w


def scratch_bytes(frames: int, n_seg: int) -> int:
    """pause_scratch_bytes of csrc/kernels.hpp: dst, mix (int32 per frame), act (a byte per frame), len (int32 per segment), each
    rounded up to 16 bytes"""
    r16 = lambda b: (b + 15) & ~15
    return 2 * r16(4 * frames) + r16(frames) + r16(4 * n_seg)


def plan(act: np.ndarray, n: int, F: int, spec: PauseSpec):
    """the plan of one segment from its frames' activity (bool [nF]) -> (keep bool [nF], mix int64 [nF] (-1: none), record list of 8)"""
    P, lead, tail, pad = spec.frames()
    nF = len(act)
    j = np.arange(nF, dtype=np.int64)
    NONE = np.int64(1) << 40
    pa = np.maximum.accumulate(np.where(act, j, -NONE))
    na = np.minimum.accumulate(np.where(act, j, NONE)[::-1])[::-1]
    has_pa, has_na = pa >= 0, na < nF
    speech = (has_pa & (j - pa <= pad)) | (has_na & (na - j <= pad))
    r0 = np.where(has_pa, pa + pad + 1, 0)
    r1 = np.where(has_na, na - pad, nF)
    R, k = r1 - r0, j - r0
    quiet = ~speech
    none, leading, trailing, inner = quiet & ~has_pa & ~has_na, quiet & ~has_pa & has_na, quiet & has_pa & ~has_na, quiet & has_pa & has_na
    h = -(-P // 2)
    t = P - h
    long_ = inner & (R > P)
    keep = speech | (none & (k < max(1, lead + tail))) | (leading & (k >= R - lead)) | (trailing & (k < tail)) | (inner & (R <= P)) | \
        (long_ & ((k < h) | (k >= R - t)))
    mix = np.where(long_ & (k == h - 1), r1 - t - 1, -1)
    sizes = np.full(nF, F, dtype=np.int64)
    sizes[-1] = n - (nF - 1) * F
    rec = [nF, int(act.sum()), int(speech.sum()), int((leading & ~keep).sum()), int(((trailing | none) & ~keep).sum()),
           int((long_ & (k == 0)).sum()), int((long_ & ~keep).sum()), int(sizes[keep].sum())]
    return keep, mix, rec


def activity(x: np.ndarray, F: int, thr) -> np.ndarray:
    """bool [ceil(n / F)]: frame j holds a sample with !(|x| < thr)"""
    n = len(x)
    nF = -(-n // F)
    loud = np.zeros(nF * F, dtype=bool)
    with np.errstate(invalid="ignore"):
        loud[:n] = ~(np.abs(x) < np.float32(thr))
    return loud.reshape(nF, F).any(1)


def apply(x: np.ndarray, fs: int, spec):
    """the NumPy twin of CodecEngine.trim_pauses on one host segment -> (y float32, record int32 [8]); spec None copies it through"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    fs = check_rate(fs)
    spec = check(spec)
    n, F = len(x), fs // 100
    if x.ndim != 1 or n < 1:
        raise ValueError("pauses: a segment is 1-D and holds at least one sample")
    nF = -(-n // F)
    if spec is None:
        return x.copy(), np.array([nF, 0, 0, 0, 0, 0, 0, n], dtype=np.int32)
    keep, mix, rec = plan(activity(x, F, spec.thr()), n, F, spec)
    idx = np.arange(nF * F, dtype=np.int64).reshape(nF, F)
    sel = idx[keep].reshape(-1)
    sel = sel[sel < n]
    y = x[sel].copy()
    w_in = fade_table(F)
    w_out = w_in[::-1]
    start = np.cumsum(np.where(keep, np.minimum(F, n - np.arange(nF) * F), 0)) - np.where(keep, np.minimum(F, n - np.arange(nF) * F), 0)
    for a in np.nonzero(mix >= 0)[0]:
        b = int(mix[a])
        y[start[a]: start[a] + F] = (w_out * x[a * F: (a + 1) * F]) + (w_in * x[b * F: (b + 1) * F])     # float32 products, float32 sum
    return y, np.array(rec, dtype=np.int32)


def tables(off, rates=None, specs=None):
    """everything ctts_trim_pauses_ragged takes besides the samples, checked -> a dict: off int64 [n_seg + 1], rates and specs (lists of
    n_seg; spec None: the segment is copied through), rows int32 [n_seg, ROW], fbase int64 [n_seg + 1] (the frames in front of each
    segment), fade float32 (the tables of the distinct F, one behind the other), scratch (bytes of device scratch).  ValueError, before
    any launch: offsets that do not ascend from 0, an empty segment, 2^31 - 4096 samples or more, more than 65535 segments, a rate
    outside 8000 .. 48000, a bad spec."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or np.any(np.diff(off) <= 0):
        raise ValueError("pauses: the offsets ascend from 0 and no segment is empty")
    if int(off[-1]) >= (1 << 31) - 4096:
        raise ValueError("pauses: the pack holds 2^31 - 4096 samples or more")
    n_seg = len(off) - 1
    if n_seg > 65535:
        raise ValueError("pauses: more than 65535 segments")
    if rates is None:
        rates = [24000] * n_seg
    elif np.ndim(rates) == 0:
        rates = [rates] * n_seg
    rates = [check_rate(r) for r in rates]
    if len(rates) != n_seg:
        raise ValueError("pauses: one rate per segment, or one for all")
    specs = list(specs) if isinstance(specs, (list, tuple)) else [specs] * n_seg
    if len(specs) != n_seg:
        raise ValueError("pauses: one spec per segment, or one for all")
    specs = [check(s) for s in specs]
    Fs = np.array([r // 100 for r in rates], dtype=np.int64)
    fade_off, parts, at = {}, [], 0
    for F in sorted(set(int(F) for F in Fs)):
        fade_off[F] = at
        parts.append(fade_table(F))
        at += F
    rows = np.zeros((n_seg, ROW), dtype=np.int32)
    for s, (F, sp) in enumerate(zip(Fs, specs)):
        rows[s, 0] = F
        rows[s, 6] = fade_off[int(F)]
        if sp is not None:
            P, lead, tail, pad = sp.frames()
            rows[s, 1:5] = (pad, lead, tail, P)
            rows[s, 5] = np.array([sp.thr()], dtype=np.float32).view(np.int32)[0]
    fbase = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(-(-np.diff(off) // Fs), out=fbase[1:])
    return {"off": off, "rates": rates, "specs": specs, "rows": rows, "fbase": fbase, "fade": np.ascontiguousarray(np.concatenate(parts)),
            "scratch": scratch_bytes(int(fbase[-1]), n_seg)}


def trim(x: np.ndarray, spec, offsets=None, rates=None):
    """`apply` over a packed host array -> (y float32, off_out int64 [n_seg + 1], records int32 [n_seg, 8])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    tb = tables(np.array([0, len(x)]) if offsets is None else offsets, rates, spec)
    off = tb["off"]
    if int(off[-1]) != len(x):
        raise ValueError("pauses: the offsets do not cover the array")
    out = [apply(x[off[s]: off[s + 1]], tb["rates"][s], tb["specs"][s]) for s in range(len(off) - 1)]
    off_out = np.zeros(len(off), dtype=np.int64)
    np.cumsum([len(y) for y, _ in out], out=off_out[1:])
    return np.concatenate([y for y, _ in out]), off_out, np.stack([r for _, r in out])


# ---- streams ----------------------------------------------------------------------------------------------------------------------------
STREAM_FRAMES = 112                              # frames a device slot holds (csrc/kernels.hpp PA_SCAP), besides the partial frame
STATE = 16                                       # int32 per slot of the device state (PA_STATE): mode, frames seen, pa, RECORD, 5 reserved


def stream_consts(spec: PauseSpec) -> dict:
    """the frame counts a stream works with: P, lead, tail, pad, h, t, k0, A1, A2, H, L (the module's docstring)"""
    P, lead, tail, pad = spec.frames()
    h = -(-P // 2)
    t = P - h
    return dict(P=P, lead=lead, tail=tail, pad=pad, h=h, t=t, k0=min(h - 1, tail), A1=max(1, lead + tail), A2=lead + pad, H=max(h, tail),
                L=t + 1 + pad)


def stream_need(spec) -> int:
    """the most frames a stream with this spec ever holds between two pushes (the partial frame not counted)"""
    c = stream_consts(check(spec) or PauseSpec())
    return max(c["A1"] + c["A2"], c["P"] + c["pad"] - c["k0"], c["H"] - c["k0"] + c["L"])


def check_stream(fs, spec, who: str = "pauses"):
    """(fs, spec) of a stream, checked -> (fs, PauseSpec).  ValueError: a bad rate or spec, no spec at all, a spec that needs more
    frames than a slot holds"""
    fs = check_rate(fs)
    spec = check(spec)
    if spec is None:
        raise ValueError(f"{who}: a pause stream needs a spec")
    need = stream_need(spec)
    if need > STREAM_FRAMES:
        raise ValueError(f"{who}: this spec makes a stream hold {need} frames, a slot holds {STREAM_FRAMES} "
                         "(max_pause_ms <= 1000, lead_ms and tail_ms <= 250, pad_ms <= 100 always fit)")
    return fs, spec


def stream_row(fs: int, spec: PauseSpec):
    """the spec part of a stream's table entry (ctts_pa_stream: F, pad, lead, tail, P, thr)"""
    P, lead, tail, pad = spec.frames()
    return fs // 100, pad, lead, tail, P, spec.thr()


def stream_held(c: dict, mode: int, nfr: int, pa: int):
    """the frames that wait when `nfr` frames are seen: (r0, lo, a, b, m) -- the run starts at frame r0, and its frames k in [lo, a) and
    [b, m) are held, in this order (a stream's carry); mode 0: no active frame yet, 1: the last active frame is pa"""
    if mode == 0:
        m = nfr
        a = min(m, c["A1"])
        return 0, 0, a, max(a, m - c["A2"]), m
    r0, k0 = pa + c["pad"] + 1, c["k0"]
    m = max(nfr - r0, k0)
    if m - c["pad"] <= c["P"]:
        return r0, k0, m, m, m
    a = min(m, c["H"])
    return r0, k0, a, max(a, m - c["L"]), m


def stream_walk(c: dict, state, acts, final: bool):
    """One push of one stream in integers, the walk of pause_stream_walk_k.  state = (mode, frames seen, pa, record list of 8); acts:
    the activity of the newly completed frames (on the final push the partial last frame is one of them).  -> (emit, state'): emit a
    list of (frame, partner or -1) in output order, frames by their absolute index.  n_out of the record is the caller's to add."""
    mode, nfr, pa, rec = state[0], state[1], state[2], list(state[3])
    P, lead, tail, pad, h, t, k0 = c["P"], c["lead"], c["tail"], c["pad"], c["h"], c["t"], c["k0"]
    emit = []
    for act in acts:
        j = nfr
        nfr += 1
        if act:
            rec[1] += 1
            if mode == 0:
                first = max(0, j - pad - lead)
                emit.extend((i, -1) for i in range(first, j))
                rec[3] += first
                rec[2] += min(j, pad) + 1
                mode = 1
            else:
                r0 = pa + pad + 1
                m, R = j - r0, j - pad - r0
                rec[2] += min(j - pa - 1, 2 * pad) + 1
                if R <= P:
                    emit.extend((r0 + k, -1) for k in range(k0, m))
                else:
                    emit.extend((r0 + k, -1) for k in range(k0, h - 1))
                    emit.append((r0 + h - 1, r0 + R - t - 1))
                    emit.extend((r0 + k, -1) for k in range(R - t, m))
                    rec[5] += 1
                    rec[6] += R - P
            emit.append((j, -1))
            pa = j
        elif mode == 1 and (j - pa <= pad or j - pa - pad - 1 < k0):
            emit.append((j, -1))
    if final:
        if mode == 0:
            keep = min(nfr, c["A1"])
            emit.extend((i, -1) for i in range(keep))
            rec[4] += nfr - keep
        else:
            r0 = pa + pad + 1
            R = nfr - r0
            rec[2] += min(nfr - 1 - pa, pad)
            if R > 0:
                emit.extend((r0 + k, -1) for k in range(k0, min(tail, R)))
                rec[4] += max(0, R - tail)
        rec[0] = nfr
    return emit, (mode, nfr, pa, rec)


class StreamPauses:
    """the NumPy twin of one pause stream at rate fs: `push(x, final) -> y` float32, `record` the RECORD so far (apply's after the final
    push), `held` the frames that wait (never more than stream_need(spec)), `partial` the samples of the incomplete frame.  It keeps
    the frames `stream_held` names, in the device carry's order, and nothing else of the signal."""

    def __init__(self, fs: int, spec=True):
        self.fs, self.spec = check_stream(fs, spec)
        self.F = self.fs // 100
        self.c = stream_consts(self.spec)
        self.need = stream_need(self.spec)
        self.state = (0, 0, 0, [0] * REC)
        self.carry = []                                               # the held frames, float32 [F] each
        self.partial = np.zeros(0, dtype=np.float32)
        self.pushed = 0
        self.done = False

    @property
    def held(self) -> int:
        return len(self.carry)

    @property
    def record(self) -> np.ndarray:
        return np.array(self.state[3], dtype=np.int32)

    def push(self, x, final: bool = False) -> np.ndarray:
        if self.done:
            raise ValueError("pauses: the stream has had its last push")
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if self.pushed + len(x) >= 1 << 31:
            raise ValueError("pauses: the stream would hold 2^31 samples or more")
        F, c = self.F, self.c
        new = np.concatenate([self.partial, x])
        nf = len(new) // F + (1 if final and len(new) % F else 0)     # on the final push the partial frame is a frame
        acts = activity(new[: nf * F], F, self.spec.thr()) if nf else np.zeros(0, dtype=bool)
        mode0, nfr0, pa0, _ = self.state
        r0o, loo, ao, bo, _ = stream_held(c, mode0, nfr0, pa0)

        def frame(j):                                                 # a held frame of the old carry, or a new one
            if j >= nfr0:
                return new[(j - nfr0) * F: (j - nfr0 + 1) * F]
            k = j - r0o
            assert loo <= k < ao or bo <= k, "a frame the stream no longer holds"
            return self.carry[k - loo if k < ao else (ao - loo) + (k - bo)]
        emit, state = stream_walk(c, self.state, acts, final)
        w_in = fade_table(F)
        parts = [frame(j) if b < 0 else (w_in[::-1] * frame(j)) + (w_in * frame(b)) for j, b in emit]
        y = np.concatenate(parts).astype(np.float32, copy=False) if parts else np.zeros(0, dtype=np.float32)
        state[3][7] += len(y)
        if final:
            self.carry, self.partial = [], np.zeros(0, dtype=np.float32)
        else:
            r0, lo, a, b, m = stream_held(c, state[0], state[1], state[2])
            self.carry = [frame(r0 + k).copy() for k in [*range(lo, a), *range(b, m)]]
            self.partial = new[nf * F:].copy()
            assert len(self.carry) <= self.need <= STREAM_FRAMES
        self.state, self.pushed, self.done = state, self.pushed + len(x), bool(final)
        return y

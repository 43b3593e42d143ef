"""The output equaliser, the host side and the NumPy twins (csrc/equalizer.hip is the device side; nothing here touches the GPU).
A cascade of at most four biquads, stage 3 1/4 of the output chain: behind trim_pauses (the pause detector sees the signal it was tuned
on), in front of compress (the compressor, the loudness stage and the limiter see what the listener will hear).  The definition, once,
for one segment x[0..n) at rate fs (what loudness.check_rate accepts: a multiple of 10 Hz in 8000 .. 48000):

  spec         None and False are off.  A preset name (`PRESETS`: "telephone", a 300 Hz high-pass; "rumble", an 80 Hz high-pass), or a
               dict with any of  highpass_hz: hz   lowshelf: {hz, db}   highshelf: {hz, db}   peaks: [{hz, db, q}, ...]  -- at most
               MAX_SECTIONS = 4 second-order sections in all, as written.  hz in 20 .. 0.45 fs, db in -12 .. +12, q in 0.3 .. 8.  A
               section of 0 dB is the identity and is dropped; a spec with no section left is off.
  sections     in this order: the high-pass, the low shelf, the high shelf, the peaks as listed.  Coefficients in float64 by the
               bilinear forms of the RBJ Audio EQ Cookbook (`coefficients`), normalised by a0: the high-pass a Butterworth section
               (Q = 1 / sqrt 2), the shelves with slope S = 1, a peak with its q.
  cascade      transposed direct form II in float64 from ZERO state at the segment's first sample, section by section (`step`):
               y = b0 x + s0;  s0 = (b1 x - a1 y) + s1;  s1 = b2 x - a2 y;  the next section's x is this y.
  output       the last section's y rounded once to float32.  `apply` is this serial loop, and it is the definition.

THE DEVICE ROUTE (`apply_route` is its twin, in the way loudness.sub_block_energies is one).  The cascade is a linear system
s' = A s + B x of D = 2 nsec states, so a run from state s is the run from zero state plus the homogeneous run of s.  A segment is cut
into tiles of TILE = LANES * CHUNK samples anchored at ITS first sample (never at the pack's), a tile into LANES chunks of CHUNK:
  1  every chunk of every tile but the segment's last runs from zero state and keeps its end state; a Hillis-Steele scan over the
     tile's chunks with A^(CHUNK 2^k), k = 0 .. 5, leaves the tile's end state under zero entry, z_T;
  2  per segment the tiles' true entry states follow from e_0 = 0, e_{T+1} = A^TILE e_T + z_T: the same scan with A^(TILE 2^k) over
     batches of LANES - 1 tiles behind the state that the batch before left;
  3  per tile, chunk 0 runs from e_T and the others from zero, the same scan gives every chunk's true entry state, and every chunk
     runs once more from it and stores float32.
Three passes over the samples and no per-sample table.  The host builds the twelve matrices per distinct (rate, spec) (`row`).  In exact
arithmetic the route IS the serial loop; in float64 the two agree to about 1e-12 of the signal's level (each is that far from the exact
result), so after the rounding to float32 they differ only where a value sits on a float32 rounding boundary, and then by one ulp.  The
float64 error is absolute: an output that happens to lie within about 1e-5 of the signal's level of zero -- a few samples in a million
of speech or noise -- has float32 ulps smaller than it, and can come out a few of those tiny ulps off."""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from . import loudness as LN

MAX_SECTIONS = 4
HZ_MIN, HZ_SHARE = 20.0, 0.45                   # a corner or centre lies in 20 Hz .. 0.45 fs
DB_MIN, DB_MAX = -12.0, 12.0
Q_MIN, Q_MAX = 0.3, 8.0
Q_BUTTERWORTH = math.sqrt(0.5)
PRESETS = {"telephone": {"highpass_hz": 300.0}, "rumble": {"highpass_hz": 80.0}}
FIELDS = ("highpass_hz", "lowshelf", "highshelf", "peaks")
KINDS = ("highpass", "lowshelf", "highshelf", "peak")
LANES = 64                                      # chunks of a tile: lane l of a wave runs samples [l c, (l + 1) c) of its tile
CHUNK = 33                                      # c, odd: the lanes' LDS reads at that stride hit 32 different banks (EQ_CHUNK)
TILE = LANES * CHUNK                            # samples of one segment per wave (EQ_TILE)
D_MAX = 2 * MAX_SECTIONS                        # states of the longest cascade
ROW = 800                                       # float64 per (rate, spec) of the coefficient table (EQ_ROW): see `row`


def _number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def _value(who: str, what: str, v, lo: float, hi: float) -> float:
    if not _number(v) or not lo <= float(v) <= hi:
        raise ValueError(f"{who}: {what} is a number in {lo:g} .. {hi:g} (got {v!r})")
    return float(v)


def _fields(who: str, what: str, d, keys) -> dict:
    if not isinstance(d, dict):
        raise ValueError(f"{who}: {what} is a dict with {', '.join(keys)} (got {d!r})")
    unknown = sorted(set(d) - set(keys), key=str)
    if unknown:
        raise ValueError(f"{who}: unknown equaliser field {unknown[0]!r} in {what} (the fields are {', '.join(keys)})")
    missing = [k for k in keys if k not in d]
    if missing:
        raise ValueError(f"{who}: {what} needs {missing[0]!r} (the fields are {', '.join(keys)})")
    return d


def check(spec, who: str = "equalize", rate=None):
    """None, False -> None (off); a preset name or a dict with any of FIELDS -> the checked spec, a tuple of sections
    (kind, hz, db, q) in cascade order (hashable: equal specs share one table row), identity sections dropped; None when none is
    left.  `rate`: the segment's rate, which bounds hz by 0.45 rate; without it hz is held to what the highest rate allows, and the
    call that knows the rate checks again.  ValueError: an unknown preset or key, a bool or a non-number where a number belongs,
    NaN, a value out of range, more than MAX_SECTIONS sections, anything else."""
    if spec is None or spec is False or (isinstance(spec, np.bool_) and not spec):
        return None
    hz_max = HZ_SHARE * (LN.FS_MAX if rate is None else LN.check_rate(rate))
    if isinstance(spec, tuple) and all(isinstance(s, tuple) and len(s) == 4 and s[0] in KINDS for s in spec):
        back = {}                                # a checked spec, as it comes back from this function
        for kind, hz, db, q in spec:
            if kind == "highpass":
                back["highpass_hz"] = hz
            elif kind == "peak":
                back.setdefault("peaks", []).append({"hz": hz, "db": db, "q": q})
            else:
                back[kind] = {"hz": hz, "db": db}
        spec = back
    if isinstance(spec, str):
        if spec not in PRESETS:
            raise ValueError(f"{who}: unknown equaliser preset {spec!r} (the presets are {', '.join(PRESETS)})")
        spec = PRESETS[spec]
    if not isinstance(spec, dict):
        raise ValueError(f"{who}: the equaliser takes None, False, a preset name ({', '.join(PRESETS)}) or a dict with any of "
                         f"{', '.join(FIELDS)} (got {spec!r})")
    unknown = sorted(set(spec) - set(FIELDS), key=str)
    if unknown:
        raise ValueError(f"{who}: unknown equaliser field {unknown[0]!r} (the fields are {', '.join(FIELDS)})")
    sections = []
    if spec.get("highpass_hz") is not None:
        sections.append(("highpass", _value(who, "highpass_hz", spec["highpass_hz"], HZ_MIN, hz_max), 0.0, Q_BUTTERWORTH))
    for kind in ("lowshelf", "highshelf"):
        if spec.get(kind) is not None:
            d = _fields(who, kind, spec[kind], ("hz", "db"))
            sections.append((kind, _value(who, f"{kind} hz", d["hz"], HZ_MIN, hz_max), _value(who, f"{kind} db", d["db"], DB_MIN, DB_MAX), Q_BUTTERWORTH))
    if spec.get("peaks") is not None:
        if not isinstance(spec["peaks"], (list, tuple)):
            raise ValueError(f"{who}: peaks is a list of dicts with hz, db, q (got {spec['peaks']!r})")
        for i, p in enumerate(spec["peaks"]):
            d = _fields(who, f"peaks[{i}]", p, ("hz", "db", "q"))
            sections.append(("peak", _value(who, f"peaks[{i}] hz", d["hz"], HZ_MIN, hz_max), _value(who, f"peaks[{i}] db", d["db"], DB_MIN, DB_MAX),
                             _value(who, f"peaks[{i}] q", d["q"], Q_MIN, Q_MAX)))
    if len(sections) > MAX_SECTIONS:
        raise ValueError(f"{who}: at most {MAX_SECTIONS} second-order sections in all (got {len(sections)})")
    sections = tuple(s for s in sections if s[0] == "highpass" or s[2] != 0.0)
    return sections or None


def per_row(eq, n: int, who: str = "equalize"):
    """one spec or one per row (a list) -> a checked list of n (entries None or a spec tuple); None when no row asks for it"""
    if eq is None:
        return None
    vals = list(eq) if isinstance(eq, list) else [eq] * n
    if len(vals) != n:
        raise ValueError(f"{who}: one equaliser spec per row, or one for all")
    vals = [check(v, who) for v in vals]
    return None if all(v is None for v in vals) else vals


def _section(kind: str, hz: float, db: float, q: float, fs: int) -> np.ndarray:
    """(b0, b1, b2, a1, a2) of one section, normalised by a0: the cookbook's bilinear forms"""
    w0 = 2.0 * math.pi * hz / fs
    cw, sw = math.cos(w0), math.sin(w0)
    if kind == "highpass":
        al = sw / (2.0 * q)
        b = ((1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0)
        a = (1.0 + al, -2.0 * cw, 1.0 - al)
    elif kind == "peak":
        A = 10.0 ** (db / 40.0)
        al = sw / (2.0 * q)
        b = (1.0 + al * A, -2.0 * cw, 1.0 - al * A)
        a = (1.0 + al / A, -2.0 * cw, 1.0 - al / A)
    else:
        A = 10.0 ** (db / 40.0)
        al = sw / 2.0 * math.sqrt(2.0)                              # slope S = 1: sqrt((A + 1 / A)(1 / S - 1) + 2)
        r = 2.0 * math.sqrt(A) * al
        if kind == "lowshelf":
            b = (A * ((A + 1.0) - (A - 1.0) * cw + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cw), A * ((A + 1.0) - (A - 1.0) * cw - r))
            a = ((A + 1.0) + (A - 1.0) * cw + r, -2.0 * ((A - 1.0) + (A + 1.0) * cw), (A + 1.0) + (A - 1.0) * cw - r)
        else:
            b = (A * ((A + 1.0) + (A - 1.0) * cw + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cw), A * ((A + 1.0) + (A - 1.0) * cw - r))
            a = ((A + 1.0) - (A - 1.0) * cw + r, 2.0 * ((A - 1.0) - (A + 1.0) * cw), (A + 1.0) - (A - 1.0) * cw - r)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def coefficients(rate, spec) -> np.ndarray:
    """the cascade of `spec` at `rate`: float64 [nsec, 5], a row (b0, b1, b2, a1, a2) per section in cascade order.  ValueError: a
    rate loudness.check_rate refuses, a bad spec, a frequency above 0.45 rate, a spec that is off."""
    fs = LN.check_rate(rate)
    sections = check(spec, "equalize", fs)
    if sections is None:
        raise ValueError("equalize: the spec is off")
    return _coefficients(fs, sections).copy()


@lru_cache(maxsize=256)
def _coefficients(fs: int, sections: tuple) -> np.ndarray:
    k = np.stack([_section(*s, fs) for s in sections])
    k.setflags(write=False)
    return k


def response_db(k: np.ndarray, hz, fs) -> np.ndarray:
    """20 log10 |H(e^{jw})| of the cascade with coefficients k [nsec, 5] at the frequencies hz, float64"""
    z = np.exp(-2j * np.pi * np.asarray(hz, dtype=np.float64) / fs)
    H = np.ones_like(z)
    for b0, b1, b2, a1, a2 in k:
        H = H * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return 20.0 * np.log10(np.abs(H))


def step(k, x, s):
    """one sample of the cascade, transposed direct form II (eq_step of csrc/equalizer.hip): k [nsec, 5], x the input, s the
    2 nsec states (a list of scalars or arrays, updated in place) -> the output"""
    for i in range(len(k)):
        b0, b1, b2, a1, a2 = k[i]
        y = b0 * x + s[2 * i]
        s[2 * i] = (b1 * x - a1 * y) + s[2 * i + 1]
        s[2 * i + 1] = b2 * x - a2 * y
        x = y
    return x


def apply(x, rate, spec) -> np.ndarray:
    """THE DEFINITION: one segment through the cascade, serially in float64 from zero state, every output rounded once to float32.
    A spec that is off returns the samples as they are."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("equalize: a segment is 1-D and holds at least one sample")
    fs = LN.check_rate(rate)
    sections = check(spec, "equalize", fs)
    if sections is None:
        return x.copy()
    k = [tuple(float(v) for v in r) for r in _coefficients(fs, sections)]
    s = [0.0] * (2 * len(k))
    y = np.empty(len(x), dtype=np.float64)
    for i, v in enumerate(x.astype(np.float64).tolist()):
        for j, (b0, b1, b2, a1, a2) in enumerate(k):
            o = b0 * v + s[2 * j]
            s[2 * j] = (b1 * v - a1 * o) + s[2 * j + 1]
            s[2 * j + 1] = b2 * v - a2 * o
            v = o
        y[i] = v
    return y.astype(np.float32)


# ---- the device route: its table and its twin -------------------------------------------------------------------------------------------
@lru_cache(maxsize=256)
def _row(fs: int, sections: tuple) -> np.ndarray:
    k = _coefficients(fs, sections)
    D = 2 * len(k)
    s = [np.eye(D)[r].copy() for r in range(D)]                     # s[r][unit state]: state r of the run that began at each unit state
    row = np.zeros(ROW)
    row[0], row[1], row[2] = len(k), fs, CHUNK
    row[4: 4 + 5 * len(k)] = k.reshape(-1)
    # A^(CHUNK 2^j): j = 0 .. 5 for the chunks' scan, j = 6 .. 11 (A^TILE and up) for the tiles'.  Up to A^TILE they are probed by running
    # the system without input for TILE steps, as accurate as the serial loop itself -- squaring A^CHUNK instead loses a factor 2 |A^n|
    # per squaring where the poles lie next to 1 (a 20 Hz high-pass at 48 kHz: entries near 200, and a route 60 times further from the
    # exact result than the serial loop is).  From A^TILE on the entries have decayed (under 8 there, under 0.2 one squaring on) and
    # squaring loses nothing
    def put(j, P):
        M = np.zeros((D_MAX, D_MAX))
        M[:D, :D] = P
        row[32 + 64 * j: 96 + 64 * j] = M.reshape(-1)
    j = 0
    for i in range(1, TILE + 1):
        step(k, 0.0, s)
        if i == CHUNK << j:
            put(j, np.array(s))
            j += 1
    P = np.array(s)
    for j in range(7, 12):
        P = P @ P
        put(j, P)
    row.setflags(write=False)
    return row


def row(rate, spec) -> np.ndarray:
    """the coefficient table's row of (rate, spec), float64 [ROW]:  [0] nsec  [1] the rate in Hz  [2] CHUNK  [4, 4 + 5 nsec) the sections'
    (b0, b1, b2, a1, a2)  [32 + 64 j, 96 + 64 j) A^(CHUNK 2^j) for j = 0 .. 11, row-major 8 x 8 with zeros beyond D = 2 nsec (j = 0 .. 5
    the chunks' scan; j = 6 .. 11, A^TILE and up, the tiles')"""
    fs = LN.check_rate(rate)
    sections = check(spec, "equalize", fs)
    if sections is None:
        raise ValueError("equalize: the spec is off")
    return _row(fs, sections)


def _chunk_scan(S: np.ndarray, R: np.ndarray, D: int, base: int = 0) -> np.ndarray:
    """the Hillis-Steele scan of the lanes: S [nt, LANES, D] end states of the chunks -> S_l = sum_{m <= l} A^(CHUNK (l - m)) z_m
    (`base` 6: of a batch of LANES tiles, with the powers of A^TILE)"""
    S = S.copy()
    for j in range(6):
        d = 1 << j
        P = R[32 + 64 * (base + j): 96 + 64 * (base + j)].reshape(D_MAX, D_MAX)[:D, :D]
        S[:, d:] = S[:, d:] + S[:, :-d] @ P.T
    return S


def apply_route(x, rate, spec) -> np.ndarray:
    """one segment by the device's route (the three steps of the module's text) in NumPy float64 -> float32; the twin of the kernels"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("equalize: a segment is 1-D and holds at least one sample")
    fs = LN.check_rate(rate)
    sections = check(spec, "equalize", fs)
    if sections is None:
        return x.copy()
    return _route64(x, fs, sections).astype(np.float32)


def _route64(x: np.ndarray, fs: int, sections: tuple) -> np.ndarray:
    """the route's outputs before the rounding to float32"""
    R = _row(fs, sections)
    k = _coefficients(fs, sections)
    D = 2 * len(k)
    n = len(x)
    nt = -(-n // TILE)
    pad = np.zeros(nt * TILE)
    pad[:n] = x
    ch = pad.reshape(nt, LANES, CHUNK)

    def run(entry, keep: bool):
        s = [entry[..., r].copy() for r in range(D)]
        y = np.empty(ch.shape) if keep else None
        for i in range(CHUNK):
            o = step(k, ch[:, :, i], s)
            if keep:
                y[:, :, i] = o
        return np.stack(s, axis=-1), y

    # 1: every chunk from zero state; the tile's end state under zero entry (the last tile's is never read)
    Z, _ = run(np.zeros((nt, LANES, D)), False)
    zT = _chunk_scan(Z, R, D)[:, LANES - 1]
    # 2: the tiles' entry states
    E = np.zeros((nt, D))
    carry = np.zeros(D)
    for b in range(0, nt - 1, LANES - 1):                           # batches: the carry in lane 0, LANES - 1 tiles behind it, then the scan
        m = min(LANES - 1, nt - 1 - b)
        zb = np.zeros((1, LANES, D))
        zb[0, 0] = carry
        zb[0, 1: 1 + m] = zT[b: b + m]
        sb = _chunk_scan(zb, R, D, base=6)[0]
        E[b + 1: b + 1 + m] = sb[1: 1 + m]
        carry = sb[LANES - 1]
    # 3: chunk 0 from the tile's entry, the scan, every chunk again from its entry
    first = [E[:, r].copy() for r in range(D)]
    for i in range(CHUNK):
        step(k, ch[:, 0, i], first)
    Z[:, 0] = np.stack(first, axis=-1)
    S = _chunk_scan(Z, R, D)
    entry = np.concatenate([E[:, None, :], S[:, :-1]], axis=1)
    _, y = run(entry, True)
    return y.reshape(-1)[:n]


def tables(n_total: int, spec, offsets=None, rates=None):
    """every table of a call, checked: (off int64 [n_seg + 1], sel int32 [n_seg] (the segment's row of the coefficient table, -1 for a
    segment that is copied through), coef float64 [n_rows, ROW], specs).  ValueError: what ctts_equalize_ragged would refuse, before
    anything is uploaded."""
    off = np.array([0, n_total], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or np.any(np.diff(off) <= 0):
        raise ValueError("equalize: the offsets ascend from 0 and no segment is empty")
    if int(off[-1]) != n_total:
        raise ValueError("equalize: the offsets do not cover the tensor")
    if n_total >= (1 << 31) - 4096:
        raise ValueError("equalize: the pack holds 2^31 - 4096 samples or more")
    n_seg = len(off) - 1
    if n_seg > 65535:
        raise ValueError("equalize: more than 65535 segments")
    if rates is None:
        rates = [24000] * n_seg
    elif np.ndim(rates) == 0:
        rates = [rates] * n_seg
    rates = [LN.check_rate(r) for r in rates]
    if len(rates) != n_seg:
        raise ValueError("equalize: one rate per segment, or one for all")
    specs = per_row(spec, n_seg)
    if specs is None:
        raise ValueError("equalize: no segment asks for the equaliser")
    specs = [None if s is None else check(s, "equalize", r) for s, r in zip(specs, rates)]       # hz against the segment's own rate
    distinct = sorted({(r, s) for r, s in zip(rates, specs) if s is not None})
    sel = np.array([-1 if s is None else distinct.index((r, s)) for r, s in zip(rates, specs)], dtype=np.int32)
    return off, sel, np.ascontiguousarray(np.stack([_row(r, s) for r, s in distinct])), specs


def scratch_records(n_total: int, n_seg: int) -> int:
    """equalize_records of csrc/kernels.hpp: segment s's tile states (D_MAX float64 each) start at record off[s] // TILE + s"""
    return n_total // TILE + n_seg + 1


def equalize(x: np.ndarray, spec, offsets=None, rates=None, route: bool = False) -> np.ndarray:
    """the NumPy twin of CodecEngine.equalize on a host array -> y float32: every segment through `apply` alone (`route`: through
    `apply_route`); a segment whose spec is off comes back as it is"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    off, sel, _, specs = tables(len(x), spec, offsets, rates)
    rates = [24000] * len(sel) if rates is None else [rates] * len(sel) if np.ndim(rates) == 0 else list(rates)
    y = x.copy()
    for s in range(len(sel)):
        if specs[s] is not None:
            y[off[s]: off[s + 1]] = (apply_route if route else apply)(x[off[s]: off[s + 1]], int(rates[s]), specs[s])
    return y

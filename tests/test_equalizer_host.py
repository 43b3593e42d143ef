"""The output equaliser, the parts that need no GPU: the validator, the coefficients against the cookbook's design values, the serial
definition on a settled sine, the device route's NumPy twin against the definition, every refusal of ctts_equalize_ragged, and the
plumbing of `eq` through the plan, Chat, the batcher and the endpoint on stand-ins."""
import ctypes as C
import math
import threading

import numpy as np
import pytest
import torch

from chattts_amd import _lib, build, equalizer as EQ, outchain as OC
from chattts_amd.serving import SpeechBatcher
from tests import equalizer_cases as K
from tests.test_loudness_host import _LoudChat, _app, _chat
from tests.test_split_pool_host import _FakeBatcher, _Params, _Pool, _wait_idle

Q = EQ.Q_BUTTERWORTH
TEL = (("highpass", 300.0, 0.0, Q),)
RUM = (("highpass", 80.0, 0.0, Q),)
RATES = (8000, 24000, 48000)


# ---- 1. the validator -----------------------------------------------------------------------------------------------------------------
def test_the_validator():
    assert EQ.check(None) is None and EQ.check(False) is None and EQ.check(np.bool_(False)) is None
    assert EQ.check("telephone") == TEL and EQ.check("rumble") == RUM and EQ.check({"highpass_hz": 300}) == TEL and EQ.check(TEL) == TEL
    full = EQ.check(K.MAX4)
    assert full == (("highpass", 120.0, 0.0, Q), ("lowshelf", 250.0, 4.5, Q), ("highshelf", 5000.0, -6.0, Q), ("peak", 1800.0, 7.5, 3.0))
    assert EQ.check(full) == full and hash(full) == hash(EQ.check(dict(K.MAX4)))
    two = EQ.check({"peaks": [{"hz": 500, "db": 3, "q": 1}, {"hz": 900, "db": -3, "q": 8}]})
    assert two == (("peak", 500.0, 3.0, 1.0), ("peak", 900.0, -3.0, 8.0)) and EQ.check(two) == two
    # the identity is off: no high-pass and every gain 0 dB; a 0 dB section among others is dropped
    assert EQ.check({}) is None and EQ.check({"lowshelf": {"hz": 100, "db": 0}, "highshelf": {"hz": 4000, "db": 0.0}, "peaks": [{"hz": 1000, "db": 0, "q": 2}]}) is None
    assert EQ.check({"highpass_hz": None, "peaks": []}) is None
    assert EQ.check({"lowshelf": {"hz": 100, "db": 0}, "peaks": [{"hz": 1000, "db": 2, "q": 2}]}) == (("peak", 1000.0, 2.0, 2.0),)
    assert EQ.check({"highpass_hz": 20}) is not None and EQ.check({"highpass_hz": 21600}) is not None and EQ.check({"highpass_hz": 3600}, rate=8000) is not None
    pk = lambda **kw: {"peaks": [{"hz": 1000, "db": 3, "q": 1, **kw}]}
    for bad, why in ((True, "None, False, a preset name"), (1, "None, False, a preset name"), ([K.MAX4], "None, False, a preset name"),
                     ("phone", "unknown equaliser preset 'phone'"), ({"gain": 1}, "unknown equaliser field 'gain'"),
                     ({"highpass_hz": 19.9}, "highpass_hz is a number in 20 .. 21600"), ({"highpass_hz": 21601}, "highpass_hz is a number in 20 .. 21600"),
                     ({"highpass_hz": True}, "highpass_hz is a number"), ({"highpass_hz": "300"}, "highpass_hz is a number"),
                     ({"highpass_hz": math.nan}, "highpass_hz is a number"), ({"lowshelf": 100}, "lowshelf is a dict with hz, db"),
                     ({"lowshelf": {"hz": 100}}, "lowshelf needs 'db'"), ({"lowshelf": {"hz": 100, "db": 1, "q": 1}}, "unknown equaliser field 'q' in lowshelf"),
                     ({"lowshelf": {"hz": 10, "db": 1}}, "lowshelf hz is a number in 20"), ({"highshelf": {"hz": 100, "db": 12.5}}, "highshelf db is a number in -12 .. 12"),
                     ({"highshelf": {"hz": 100, "db": -12.5}}, "highshelf db is a number in -12 .. 12"), ({"peaks": {"hz": 1}}, "peaks is a list"),
                     ({"peaks": [3]}, r"peaks\[0\] is a dict with hz, db, q"), (pk(q=0.29), r"peaks\[0\] q is a number in 0.3 .. 8"),
                     (pk(q=8.5), r"peaks\[0\] q is a number in 0.3 .. 8"), (pk(db=13), r"peaks\[0\] db is a number in -12 .. 12"),
                     (pk(hz=math.inf), r"peaks\[0\] hz is a number"), (pk(db=False), r"peaks\[0\] db is a number"),
                     ({**K.MAX4, "peaks": [K.MAX4["peaks"][0]] * 2}, "at most 4 second-order sections in all"),
                     ({"peaks": [{"hz": 1000, "db": 0, "q": 1}] * 5}, "at most 4 second-order sections")):
        with pytest.raises(ValueError, match=why):
            EQ.check(bad)
    with pytest.raises(ValueError, match="submit: highpass_hz is a number in 20 .. 3600"):      # 0.45 of the rate, under the caller's name
        EQ.check({"highpass_hz": 3601}, "submit", 8000)
    for rate in (7990, 48010, 24005, 24000.0, True):                                           # what loudness.check_rate refuses
        with pytest.raises(ValueError, match="the rate is an integer number of Hz"):
            EQ.check("telephone", rate=rate)
        with pytest.raises(ValueError, match="the rate is an integer number of Hz"):
            EQ.coefficients(rate, "telephone")
    with pytest.raises(ValueError, match="the spec is off"):
        EQ.coefficients(24000, None)
    assert EQ.per_row(None, 2) is None and EQ.per_row([None, False], 2) is None and EQ.per_row([{}, None], 2) is None
    assert EQ.per_row("telephone", 2) == [TEL, TEL] and EQ.per_row([None, "rumble"], 2) == [None, RUM]
    with pytest.raises(ValueError, match="t: one equaliser spec per row"):
        EQ.per_row(["telephone"], 2, "t")
    with pytest.raises(ValueError, match="t: unknown equaliser preset"):
        EQ.per_row([None, "x"], 2, "t")


def test_the_tables_of_a_call():
    off, sel, coef, specs = EQ.tables(10, ["telephone", None, "telephone", "rumble", {"highpass_hz": 300}], offsets=[0, 2, 4, 6, 8, 10],
                                      rates=[8000, 8000, 24000, 8000, 8000])
    assert sel.tolist() == [1, -1, 2, 0, 1] and sel.dtype == np.int32 and coef.shape == (3, EQ.ROW) and coef.dtype == np.float64 and off.dtype == np.int64
    assert coef[:, 0].tolist() == [1, 1, 1] and coef[:, 1].tolist() == [8000, 8000, 24000] and coef[:, 2].tolist() == [EQ.CHUNK] * 3
    assert specs == [TEL, None, TEL, RUM, TEL] and EQ.scratch_records(10, 5) == 10 // EQ.TILE + 6 and EQ.TILE == 64 * EQ.CHUNK and EQ.CHUNK % 2 == 1
    for kw, why in ((dict(offsets=[0, 5, 5]), "no segment is empty"), (dict(offsets=[0, 4]), "do not cover"), (dict(offsets=[1, 10]), "ascend from 0"),
                    (dict(rates=[8000, 8000]), "one rate per segment"), (dict(rates=11025), "the rate is an integer"), (dict(spec=None), "no segment asks"),
                    (dict(spec=[None]), "no segment asks"), (dict(spec={"highpass_hz": 4000}, rates=8000), "highpass_hz is a number in 20 .. 3600")):
        with pytest.raises(ValueError, match=why):
            EQ.tables(10, **{"spec": "telephone", **kw})
    with pytest.raises(ValueError, match="2\\^31 - 4096"):
        EQ.tables((1 << 31) - 4096, "telephone")
    row = EQ.row(48000, K.MAX4)
    k = EQ.coefficients(48000, K.MAX4)
    assert row[0] == 4 and row[4:24].tobytes() == k.tobytes() and not row.flags.writeable
    A = np.zeros((8, 8))                                                 # the state matrix, column by column from one step without input
    for q in range(8):
        s = list(np.eye(8)[q])
        EQ.step(k, 0.0, s)
        A[:, q] = s
    for j in range(12):                                                   # the row's matrices are its powers
        np.testing.assert_allclose(row[32 + 64 * j: 96 + 64 * j].reshape(8, 8), np.linalg.matrix_power(A, EQ.CHUNK << j), rtol=1e-9, atol=1e-12)
    assert np.all(EQ.row(8000, "telephone")[32:].reshape(12, 8, 8)[:, 2:, :] == 0) and np.all(EQ.row(8000, "telephone")[32:].reshape(12, 8, 8)[:, :, 2:] == 0)


# ---- 2. the coefficients: float64 algebra against the cookbook's design values -----------------------------------------------------------
TOL_DB = 1e-9


def _db(rate, spec, hz):
    return float(EQ.response_db(EQ.coefficients(rate, spec), [hz], rate)[0])


@pytest.mark.parametrize("rate", RATES)
def test_the_coefficients_meet_the_cookbooks_design_values(rate):
    nyq = rate / 2
    for hz in (20.0, 80.0, 300.0, 1000.0, 0.45 * rate):                    # the Butterworth high-pass: -3.01 dB at its corner, a null at DC
        assert abs(_db(rate, {"highpass_hz": hz}, hz) - 10.0 * math.log10(0.5)) <= TOL_DB, (rate, hz)
        assert abs(_db(rate, {"highpass_hz": hz}, nyq)) <= TOL_DB
        k = EQ.coefficients(rate, {"highpass_hz": hz})[0]
        assert abs(k[0] + k[1] + k[2]) <= 1e-15 and k.shape == (5,)
    for hz, db, q in ((1000.0, 6.0, 2.0), (250.0, -12.0, 0.3), (0.4 * rate, 12.0, 8.0), (20.0, -3.5, 1.0)):      # a peak: db at its centre, 0 dB far from it
        spec = {"peaks": [{"hz": hz, "db": db, "q": q}]}
        assert abs(_db(rate, spec, hz) - db) <= TOL_DB and abs(_db(rate, spec, 0.0)) <= TOL_DB and abs(_db(rate, spec, nyq)) <= TOL_DB, (rate, hz)
    for hz, db in ((200.0, 6.0), (20.0, -12.0), (0.45 * rate, 12.0), (1000.0, -0.5)):                           # a shelf: db at its far end, 0 dB at the other
        lo, hi = {"lowshelf": {"hz": hz, "db": db}}, {"highshelf": {"hz": hz, "db": db}}
        assert abs(_db(rate, lo, 0.0) - db) <= TOL_DB and abs(_db(rate, lo, nyq)) <= TOL_DB, (rate, hz)
        assert abs(_db(rate, hi, nyq) - db) <= TOL_DB and abs(_db(rate, hi, 0.0)) <= TOL_DB, (rate, hz)
        assert abs(_db(rate, lo, hz) - db / 2) <= TOL_DB and abs(_db(rate, hi, hz) - db / 2) <= TOL_DB           # S = 1: half the gain at the corner
    k = EQ.coefficients(rate, {**K.MAX4, "highshelf": {"hz": 0.4 * rate, "db": -6}})                            # the cascade is the product, in the documented order
    parts = [{"highpass_hz": 120}, {"lowshelf": K.MAX4["lowshelf"]}, {"highshelf": {"hz": 0.4 * rate, "db": -6}}, {"peaks": K.MAX4["peaks"]}]
    assert k.shape == (4, 5) and k.tobytes() == np.concatenate([EQ.coefficients(rate, p) for p in parts]).tobytes()
    for a1, a2 in k[:, 3:]:                                                                                      # every section is stable
        assert abs(a2) < 1 and abs(a1) < 1 + a2


# ---- 3. the definition on a settled sine -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,spec,hz", [(8000, "telephone", 300.0), (8000, "telephone", 1000.0), (24000, K.MAX4, 250.0), (24000, K.MAX4, 1800.0),
                                          (48000, {"peaks": [{"hz": 1000, "db": -9, "q": 4}]}, 1000.0), (48000, {"highshelf": {"hz": 4000, "db": 6}}, 12000.0),
                                          (48000, K.HP20, 40.0)])
def test_apply_on_a_settled_sine_has_the_gain_of_the_response(rate, spec, hz):
    """1 s of a sine, measured over the last 0.5 s (whole periods: every frequency here has a whole number of them in 0.5 s): the
    output's amplitude over the input's, by projection on the sine and the cosine, against |H| -- within 0.01 dB"""
    t = np.arange(rate) / rate
    x = (0.5 * np.sin(2 * np.pi * hz * t)).astype(np.float32)
    y = EQ.apply(x, rate, spec)
    assert y.dtype == np.float32 and y.shape == x.shape
    h = slice(rate // 2, rate)
    amp = lambda v: math.hypot(2 * np.mean(v[h].astype(np.float64) * np.sin(2 * np.pi * hz * t[h])), 2 * np.mean(v[h].astype(np.float64) * np.cos(2 * np.pi * hz * t[h])))
    got = 20 * math.log10(amp(y) / amp(x))
    assert abs(got - _db(rate, spec, hz)) <= 0.01, (got, _db(rate, spec, hz))


def test_apply_is_the_serial_loop_from_zero_state():
    x = K.signal("noise", 50, 24000, 7)
    k = EQ.coefficients(24000, K.MAX4)
    s, want = [0.0] * 8, []
    for v in x.astype(np.float64):
        want.append(EQ.step(k, float(v), s))
    assert EQ.apply(x, 24000, K.MAX4).tobytes() == np.array(want).astype(np.float32).tobytes()
    assert EQ.apply(x, 24000, None).tobytes() == x.tobytes() and EQ.apply(x, 24000, {}).tobytes() == x.tobytes()
    y = EQ.equalize(np.concatenate([x, x]), ["rumble", None], offsets=[0, 50, 100])              # every segment from zero state, an off one as it is
    assert y[:50].tobytes() == EQ.apply(x, 24000, "rumble").tobytes() and y[50:].tobytes() == x.tobytes()
    with pytest.raises(ValueError, match="at least one sample"):
        EQ.apply(np.zeros(0, np.float32), 24000, "rumble")


# ---- 4. the device route's twin against the serial definition ---------------------------------------------------------------------------
def test_the_route_twin_is_the_definition_to_the_last_bit_but_for_rounding_boundaries():
    """`equalize(route=True)`, the NumPy twin of the three launches, on the GPU test's pack (tests/equalizer_cases.py: the 20 Hz
    high-pass at 48 kHz is its longest segment, 3 tiles + 5) and its four kinds of input, against `apply`: every sample within one
    float32 ulp, at most 1e-3 of them different at all.  Observed on the CPU: 7 of 51516 samples differ, a share of 1.36e-4 -- 1 in the
    four-section segment under the DC + sine input, 6 in the 20 Hz segment under the two impulses, none under the noise."""
    got = {kind: EQ.equalize(K.pack(kind), K.SPECS, offsets=K.OFFSETS, rates=K.RATES, route=True) for kind in K.KINDS}
    K.compare("route twin", got)
    x = K.pack("noise")
    for i in (0, 3, 7, 9):                                        # a segment's result does not depend on the pack: alone, the same bits
        a, b = K.OFFSETS[i], K.OFFSETS[i + 1]
        assert EQ.apply_route(x[a:b], K.RATES[i], K.SPECS[i]).tobytes() == got["noise"][a:b].tobytes()


def test_the_matrices_are_probed_not_squared():
    """the route is as close to the exact result as the serial loop is, also where the poles lie next to 1: at the 20 Hz high-pass at
    48 kHz both stay within 1e-12 of a long double run (matrices squared up from A^c put the route at 2e-11)"""
    x = K.signal("noise", 3 * K.T + 5, 48000, 0)
    sec = EQ.check(K.HP20)
    k = [np.longdouble(v) for v in EQ.coefficients(48000, K.HP20)[0]]
    s0 = s1 = np.longdouble(0)
    exact = np.empty(len(x), dtype=np.longdouble)
    for i, v in enumerate(x.astype(np.longdouble)):
        y = k[0] * v + s0
        s0, s1 = (k[1] * v - k[3] * y) + s1, k[2] * v - k[4] * y
        exact[i] = y
    route = EQ._route64(x, 48000, sec)
    serial = np.empty(len(x))
    s = [0.0, 0.0]
    kk = EQ.coefficients(48000, K.HP20)
    for i, v in enumerate(x.astype(np.float64)):
        serial[i] = EQ.step(kk, float(v), s)
    assert float(np.abs(serial - exact).max()) < 1e-12 and float(np.abs(route - exact).max()) < 1e-12


# ---- 5. the library's refusals, all before any launch ------------------------------------------------------------------------------------
def test_library_symbols_and_refusals_before_any_launch():
    """the C entry point checks every host table first: these calls fail without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    with open(_lib.HERE + "/../include/chattts_amd.h") as f:
        header = f.read()
    for name in ("ctts_equalize_ragged", "ctts_equalize_ragged_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "equalizer.hip" in build.SOURCES and f"#define CTTS_EQ_ROW {EQ.ROW}" in header and f"#define CTTS_EQ_TILE {EQ.TILE}" in header
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ctts_equalize_ragged_scratch_bytes(vp(i64([0, 2400, 12000])), 2) == EQ.scratch_records(12000, 2) * 64
    assert lib.ctts_equalize_ragged_scratch_bytes(vp(i64([0, 5, 5])), 2) == 0 and b"empty" in lib.ctts_last_error()
    assert lib.ctts_equalize_ragged_scratch_bytes(vp(i64([0, (1 << 31) - 4096])), 1) == 0 and b"2^31" in lib.ctts_last_error()
    last = 0
    for n in (1, EQ.TILE - 1, EQ.TILE, EQ.TILE + 1, 24000):                       # never smaller when the pack grows
        v = lib.ctts_equalize_ragged_scratch_bytes(vp(i64([0, n])), 1)
        assert v >= last and v > 0 and v % 16 == 0
        last = v
    fake = 4096                       # never dereferenced: every call below is refused on its host arguments
    good = np.stack([EQ.row(24000, "telephone"), EQ.row(8000, K.MAX4 | {"highshelf": {"hz": 3000, "db": -6}})])

    def call(off=(0, 2400, 12000), sel=(0, 1), coef=good, n_rows=2, x=fake, y=fake, scratch=fake, sb=1 << 20, null=None, n_seg=None, coef_dev=fake):
        o, s, t = i64(off), np.asarray(sel, np.int32), np.ascontiguousarray(coef, np.float64)
        d = {k: (None if k == null else fake) for k in ("off", "sel")}
        rc = lib.ctts_equalize_ragged(None if null == "x" else x, None if null == "y" else y, d["off"], vp(o), len(o) - 1 if n_seg is None else n_seg,
                                      d["sel"], None if null == "sel_host" else vp(s), None if null == "coef" else coef_dev,
                                      None if null == "coef_host" else vp(t), n_rows, scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    def bad_row(at, v):
        t = good.copy()
        t[1, at] = v
        return t

    for kw, why in ((dict(null="x"), "null"), (dict(null="y"), "null"), (dict(null="off"), "null"), (dict(null="sel"), "null"), (dict(null="sel_host"), "null"),
                    (dict(null="coef"), "null"), (dict(null="coef_host"), "null"),
                    (dict(off=(1, 2400, 12000)), "must be 0"), (dict(off=(0, 2400, 2400)), "empty"), (dict(off=(0, 2400, 100)), "ascend"),
                    (dict(n_seg=0), "1 <= n_seg <= 65535"), (dict(n_seg=65536), "1 <= n_seg <= 65535"), (dict(off=(0, 2400, (1 << 31) - 4096)), "2^31 - 4096"),
                    (dict(coef=bad_row(0, 5)), "1 .. 4 second-order sections (got 5)"), (dict(coef=bad_row(0, 0)), "1 .. 4 second-order sections"),
                    (dict(coef=bad_row(0, 2.5)), "1 .. 4 second-order sections"), (dict(coef=bad_row(0, math.nan)), "1 .. 4 second-order sections"),
                    (dict(coef=bad_row(1, 7990)), "multiple of 10 Hz in 8000 .. 48000 (got 7990)"), (dict(coef=bad_row(1, 48010)), "multiple of 10 Hz in 8000 .. 48000"),
                    (dict(coef=bad_row(1, 24005)), "multiple of 10 Hz"), (dict(coef=bad_row(1, -8000)), "multiple of 10 Hz"),
                    (dict(coef=bad_row(2, 32)), "the chunk is 33 samples"), (dict(coef=bad_row(4, math.inf)), "section 0 has a coefficient that is not finite"),
                    (dict(coef=bad_row(8, 1.0)), "section 0 is not stable"), (dict(coef=bad_row(12, 2.5)), "section 1 is not stable"),
                    (dict(coef=bad_row(100, math.nan)), "a power of the state matrix is not finite"),
                    (dict(sel=(0, 2)), "coefficient row 2 is outside"), (dict(sel=(-2, 1)), "coefficient row -2 is outside"),
                    (dict(n_rows=0), "1 <= n_rows <= n_seg"), (dict(n_rows=3), "1 <= n_rows <= n_seg"),
                    (dict(sb=100), "scratch"), (dict(scratch=None), "scratch"), (dict(scratch=4104), "scratch"), (dict(x=4100), "16-byte aligned"),
                    (dict(y=4104), "16-byte aligned"), (dict(coef_dev=4104), "16-byte aligned"), (dict(y=4096 + 160), "overlap")):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_equalize_ragged" in msg and why in msg, (kw, msg)


# ---- 6. the plan ------------------------------------------------------------------------------------------------------------------------
class _Stages:
    """a codec that records the chain's calls"""

    def __init__(self):
        self.calls = []

    def trim_pauses(self, wav, spec, **kw):
        self.calls.append(("trim_pauses", sorted(kw)))
        return wav.reshape(-1), np.array([0, 4, 8], np.int64)

    def equalize(self, wav, spec, **kw):
        self.calls.append(("equalize", spec, {k: (v if k != "out" else v is wav) for k, v in kw.items()}))
        return wav

    def compress(self, wav, spec, **kw):
        self.calls.append(("compress", sorted(kw)))
        return wav

    def loudness_normalize(self, wav, target, **kw):
        self.calls.append(("loudness_normalize", target, sorted(kw)))
        return wav


def test_the_plan_places_the_stage_between_pauses_and_compress():
    assert "eq" in OC.STAGES and OC.STAGES[:5] == ("speed", "loudness", "pauses", "compress", "limiter")
    assert [f for f in OC.Plan.__dataclass_fields__][-1] == "eq" and OC.Plan("t").eq is None and not OC.Plan("t").on
    assert OC.Plan("t", None, None, None, None, None, 24000, None) == OC.Plan("t")                  # every positional construction stays valid
    p = OC.Plan.rows("t", 2, None, None, -16.0, True, True, True, ["telephone", None])
    assert p.eq == [TEL, None] and p.on and p.kwargs("eq") == {"eq": [TEL, None]} and p.kwargs()["eq"] == [TEL, None]
    assert OC.Plan.rows("t", 2, eq=[None, False]).eq is None and not OC.Plan.rows("t", 2, eq=False).on and not OC.Plan.rows("t", 2, eq={}).on
    assert OC.Plan.batch("t", 2, eq="rumble").eq == [RUM, RUM] and OC.Plan.batch("t", 2, eq="rumble").on
    with pytest.raises(ValueError, match="t: one equaliser spec per row"):
        OC.Plan.rows("t", 2, eq=["telephone"])
    with pytest.raises(ValueError, match="rate"):
        OC.Plan.rows("t", 1, sample_rate=11025, eq="telephone")
    assert OC.Plan.rows("t", 1, sample_rate=11025).on                                                # without the option the rate is the resampler's business
    with pytest.raises(ValueError, match="t: highpass_hz is a number in 20 .. 3600"):                # a frequency against its own row's rate
        OC.Plan.rows("t", 2, sample_rate=[24000, 8000], eq={"highpass_hz": 4000})
    assert OC.Plan.rows("t", 2, sample_rate=[24000, 8000], eq=[{"highpass_hz": 4000}, None]).on
    with pytest.raises(ValueError, match="highpass_hz is a number in 20 .. 3600"):
        OC.Plan.batch("t", 2, sample_rate=8000, eq={"highpass_hz": 4000})
    g = OC.Plan.given("t", eq=["telephone", None, K.MAX4])
    assert g.eq == [TEL, None, EQ.check(K.MAX4)] and OC.Plan.given("t", eq=False).eq is None and OC.Plan.given("t", eq={}).eq is None
    assert "eq" not in OC.Plan.given("t", loudness=-16, compress=True).kwargs() and OC.Plan.given("t", eq="rumble").kwargs() == {"eq": RUM}
    with pytest.raises(ValueError, match="t: unknown equaliser preset"):
        OC.Plan.given("t", eq="loud")
    s = g.per_sentence([[0, 1], [2], [3, 4, 5]])                                                     # one per sentence, like compress
    assert s.eq == [TEL, TEL, None, *[EQ.check(K.MAX4)] * 3]
    with pytest.raises(ValueError, match="one equaliser spec per request"):
        g.per_sentence([[0], [1]])
    assert OC.Plan.given("t", eq="telephone").per_sentence([[0, 1]]).eq == TEL                        # one for all stays one
    codec, wav = _Stages(), torch.zeros((2, 4))
    OC.run(codec, wav, OC.Plan.batch("t", 2, None, None, -16.0, True, True, True, "telephone"), in_place=True)
    assert [c[0] for c in codec.calls] == ["trim_pauses", "equalize", "compress", "loudness_normalize"]
    assert codec.calls[1][1:] == ([TEL, TEL], {"offsets": pytest.approx([0, 4, 8]), "rates": 24000, "out": True})
    codec.calls.clear()
    OC.run(codec, wav, OC.Plan.batch("t", 2, eq="telephone"))
    assert codec.calls == [("equalize", [TEL, TEL], {"rates": 24000})]
    codec.calls.clear()
    OC.run(codec, wav, OC.Plan.batch("t", 2, eq="telephone"), in_place=True)
    assert codec.calls == [("equalize", [TEL, TEL], {"rates": 24000, "out": True})]
    codec.calls.clear()
    OC.run(codec, wav, OC.Plan.batch("t", 2, None, None, -16.0, True, None, True))                    # off: never called, never passed
    assert [c[0] for c in codec.calls] == ["trim_pauses", "compress", "loudness_normalize"] and all("eq" not in str(c) for c in codec.calls)


# ---- 7. Chat, the batcher, the endpoint, on stand-ins -------------------------------------------------------------------------------------
def test_chat_passes_the_spec_on_and_nothing_when_it_is_off():
    chat = _chat()
    rows = [torch.zeros(3, 768), torch.zeros(2, 768)]
    chat.decode_to_wavs(rows, ragged=True, eq=["telephone", None])
    chat.decode_to_wavs(rows, ragged=True, eq=[False, {}])
    chat.decode_to_wavs(rows, eq="rumble", loudness=-23.0, sample_rate=8000)
    chat.decode_to_wavs(rows)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": None, "eq": [TEL, None]}), ("decode_ragged", {"sample_rate": None}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": 8000, "loudness": -23.0, "eq": RUM}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": None})]
    with pytest.raises(ValueError, match="unknown equaliser field"):
        chat.decode_to_wavs(rows, eq={"on": True})
    chat.codec.calls.clear()
    groups = [[torch.zeros(3, 768), torch.zeros(2, 768)], [torch.zeros(2, 768)]]
    chat.decode_split_to_pcm16(groups, eq=["telephone", None], loudness=-19.0)
    chat.decode_split_to_pcm16(groups, eq=False)
    assert chat.codec.calls[0] == ("decode_ragged", {"sample_rate": None, "eq": [TEL, TEL, None]})               # every sentence alone
    assert chat.codec.calls[1][0] == "loudness_normalize" and "eq" not in chat.codec.calls[1][2]
    assert ("decode_ragged", {"sample_rate": None}) in chat.codec.calls[2:]
    seen = []

    def fake_infer(text, *a, **kw):
        seen.append(kw)
        yield [np.full(5, 0.5, np.float32) for _ in text]
    chat._infer = fake_infer
    kw = dict(skip_refine_text=True, split_text=False)
    chat.infer(["a", "b"], eq=["telephone", False], **kw)
    chat.infer(["a", "b"], **kw)
    chat.infer(["a", "b"], eq=False, pcm16=True, **kw)
    assert seen[0]["eq"] == [TEL, None] and "eq" not in seen[1] and "eq" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "eq"} == seen[1]
    with pytest.raises(ValueError, match="non-streamed.*filter state carried across chunks"):
        chat.infer(["hello"], stream=True, eq="telephone")
    with pytest.raises(ValueError, match="one equaliser spec"):
        chat.infer(["a", "b"], split_text=True, eq=["telephone", None])
    with pytest.raises(ValueError, match="rate"):
        chat.infer(["hello"], sample_rate=11025, eq="telephone")
    with pytest.raises(ValueError, match="infer: highpass_hz is a number in 20 .. 3600"):
        chat.infer(["hello"], sample_rate=8000, eq={"highpass_hz": 4000})


def test_the_batcher_passes_the_spec_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all three are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), **kw) for c, kw in (("a", dict(eq="telephone")), ("b", dict(eq=K.MAX4, compress=True)), ("c", {}))]
        [f.result(timeout=10) for f in futs]
        b.submit("e#8", _Params(), eq=False).result(timeout=10)
        _wait_idle(pools)
        for bad in (1, "x", ["telephone"], {"highpass_hz": 5}):
            with pytest.raises(ValueError):
                b.submit("a#8", _Params(), eq=bad)
        with pytest.raises(ValueError, match="submit: highpass_hz is a number in 20 .. 3600"):
            b.submit("a#8", _Params(), eq={"highpass_hz": 4000}, sample_rate=8000)
        with pytest.raises(TypeError):
            b.submit_stream("a#8", _Params(), eq="telephone")
    finally:
        b.close()
    assert chat.pcm_kw[0]["eq"] == [TEL, EQ.check(K.MAX4), None] and chat.pcm_kw[1] == {} and b.decode_calls == 2
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    try:
        b.submit("a#8", _Params(), eq="rumble").result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, eq="rumble").result(timeout=30)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.wav_kw == [{"eq": RUM}, {}] and chat.split_kw == [{"eq": [RUM]}]


def test_endpoint_eq():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: an unknown key -- the warning, and today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "eq": "telephone"})
        assert r.status_code == 200 and r.content == r0.content and sorted(chat.calls[-1][2]) == sorted(chat.calls[-2][2]) and "eq" not in chat.calls[-1][2]
        assert catch.msgs == ["ignoring unsupported parameters: ['eq']"]
        assert c.post("/v1/audio/speech", json={**body, "eq": 7}).status_code == 200               # ignored, whatever it holds
        h0 = c.get("/health").json()
        assert "eq" not in h0

    app, chat, catch = _app(eq=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "eq": "telephone"})
        assert r.status_code == 200 and chat.calls[-1][2]["eq"] == TEL and chat.calls[-1][1] is False and "compress" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={**body, "eq": K.MAX4})
        assert r.status_code == 200 and chat.calls[-1][2]["eq"] == EQ.check(K.MAX4)
        for off in ({}, {"eq": False}, {"eq": None}, {"eq": {}}):
            assert c.post("/v1/audio/speech", json={**body, **off}).status_code == 200 and "eq" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        assert c.post("/v1/audio/speech", json={**body, "stream": True, "eq": False}).status_code == 200
        n = len(chat.calls)
        for bad, why in ((1, "a preset name"), (True, "a preset name"), ("phone", "unknown equaliser preset"), ([K.MAX4], "a preset name"),
                         ({"on": True}, "unknown equaliser field"), ({"highpass_hz": 5}, "highpass_hz is a number in 20 .. 10800"),
                         ({"peaks": [{"hz": 1000, "db": 3}]}, "needs 'q'"), ({"peaks": [{"hz": 1000, "db": 1, "q": 1}] * 5}, "at most 4")):
            r = c.post("/v1/audio/speech", json={**body, "eq": bad})
            assert r.status_code == 400 and why in r.text, bad
        r = c.post("/v1/audio/speech", json={**body, "eq": "telephone", "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "filter state carried across chunks" in r.text and len(chat.calls) == n
        assert not catch.msgs
        assert c.get("/health").json() == {**h0, "eq": True}

    app, chat, catch = _app(eq=True, compress=True, limiter=True, loudness=True, sample_rates=(8000, 11025, 24000), g711=True, speed=True, flac=True, pauses=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "eq": "telephone", "compress": True, "limiter": True, "loudness": -20.5, "speed": 0.8, "sample_rate": 8000,
                                             "encoding": "ulaw", "pauses": True})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["eq"], kw["limiter"], kw["loudness"], kw["speed"], kw["sample_rate"], kw["encoding"]) == \
            (TEL, True, -20.5, 0.8, 8000, "ulaw") and kw["pauses"] is not None and kw["compress"] is not None
        r = c.post("/v1/audio/speech", json={**body, "response_format": "flac", "eq": "rumble"})
        assert r.status_code == 200 and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["eq"] == RUM
        r = c.post("/v1/audio/speech", json={**body, "eq": {"highpass_hz": 4000}, "sample_rate": 8000})              # above 0.45 of the request's rate
        assert r.status_code == 400 and "highpass_hz is a number in 20 .. 3600" in r.text
        assert c.post("/v1/audio/speech", json={**body, "eq": "telephone", "sample_rate": 11025}).status_code == 400      # no multiple of 10 Hz
        assert c.post("/v1/audio/speech", json={**body, "eq": False, "sample_rate": 11025}).status_code == 200

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, eq=True, loudness=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "eq": "telephone"}).status_code == 200 and bat.calls[-1][2] == {"eq": TEL}
        assert c.post("/v1/audio/speech", json={**body, "eq": "rumble", "loudness": -16}).status_code == 200
        assert bat.calls[-1][2] == {"loudness": -16.0, "eq": RUM}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

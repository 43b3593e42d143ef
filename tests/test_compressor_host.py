"""The dynamic range compressor, the parts that need no GPU: the validator, the gain table against the law, a hand-computed example, the
definition's properties on the NumPy twin (chattts_amd/compressor.py), the steady state against the law, every refusal of the host
side and of ctts_compress_ragged, and the plumbing of `compress` through the plan, Chat, the batcher and the endpoint on stand-ins."""
import ctypes as C
import math
import threading

import numpy as np
import pytest
import torch

from chattts_amd import _lib, build, compressor as CP, outchain as OC
from chattts_amd.serving import SpeechBatcher
from tests import compressor_cases as CC
from tests.test_loudness_host import _LoudChat, _app, _chat
from tests.test_split_pool_host import _FakeBatcher, _FakeChat, _Params, _Pool, _wait_idle

DEFAULT = (-24.0, 3.0, 6.0, 5.0, 60.0)


# ---- 1. the validator -----------------------------------------------------------------------------------------------------------------
def test_the_validator():
    assert CP.check(True) == DEFAULT == CP.check({}) == CP.check(np.bool_(True)) and CP.check(None) is None and CP.check(False) is None
    assert CP.check({"ratio": 4, "hold_ms": 0}) == (-24.0, 4.0, 6.0, 5.0, 0.0) and CP.check(CP.check(True)) == DEFAULT
    assert list(CP.RANGES) == ["threshold_db", "ratio", "knee_db", "attack_ms", "hold_ms"] and CP.blocks(CP.check({"attack_ms": 2.5})) == (3, 60)
    for bad, why in (({"gain": 1}, "unknown compressor field 'gain'"), (1, "True, False, None or a dict"), ("on", "True, False, None or a dict"),
                     ([True], "True, False, None or a dict"), ({"ratio": True}, "ratio is a number in 1.5 .. 20"),
                     ({"ratio": "3"}, "ratio is a number"), ({"ratio": math.nan}, "ratio is a number"), ({"ratio": 1.0}, "ratio is a number in 1.5 .. 20"),
                     ({"ratio": 21}, "ratio is a number"), ({"threshold_db": -61}, "threshold_db is a number in -60 .. -6"),
                     ({"threshold_db": -5}, "threshold_db"), ({"knee_db": -1}, "knee_db is a number in 0 .. 24"), ({"knee_db": 25}, "knee_db"),
                     ({"attack_ms": 0.5}, "attack_ms is a number in 1 .. 20"), ({"attack_ms": 21}, "attack_ms"),
                     ({"hold_ms": -1}, "hold_ms is a number in 0 .. 500"), ({"hold_ms": 501}, "hold_ms"), ({"hold_ms": math.inf}, "hold_ms")):
        with pytest.raises(ValueError, match=why):
            CP.check(bad)
    assert CP.per_row(None, 2) is None and CP.per_row([None, False], 2) is None and CP.per_row(True, 2) == [DEFAULT, DEFAULT]
    assert CP.per_row([None, {"ratio": 2}], 2) == [None, (-24.0, 2.0, 6.0, 5.0, 60.0)]
    with pytest.raises(ValueError, match="one compressor spec per row"):
        CP.per_row([True], 2)
    assert CP.STATS.itemsize == 16 and CP.STATS.names == ("min_gain", "n_blocks", "n_touched", "peak")


# ---- 2. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [True, *CC.SPECS[1:], {"threshold_db": -6, "ratio": 1.5, "knee_db": 24}])
def test_the_table_is_the_law_at_the_bin_edges(spec):
    spec = CP.check(spec)
    thr, ratio, knee = spec[:3]
    t = CP.table(spec)
    assert t.dtype == np.float32 and t.shape == (CP.TABLE,) and t.max() <= 1.0 and t.min() >= CP.ENTRY_MIN and np.all(np.diff(t) <= 0)
    for q in range(CP.TABLE):                                    # a direct float64 evaluation, entry by entry
        edge = 2.0 ** (q // 32 - 24) * (1 + (q % 32) / 32)
        over = 20 * math.log10(edge) - thr
        if 2 * over < -knee:
            G = 0.0
        elif 2 * abs(over) <= knee:
            G = (1 / ratio - 1) * (over + knee / 2) ** 2 / (2 * knee)
        else:
            G = (1 / ratio - 1) * over
        assert t[q] == np.float32(10 ** (G / 20)) or abs(float(t[q]) / 10 ** (G / 20) - 1) < 2.0 ** -23, q
        if 2 * over < -knee:
            assert t[q] == 1.0, q
    edges = np.ldexp(1.0 + (np.arange(CP.TABLE) % 32) / 32.0, np.arange(CP.TABLE) // 32 - 24).astype(np.float32)
    assert np.array_equal(CP.bin_index(edges), np.arange(CP.TABLE)) and CP.Q0 == 3296
    assert CP.bin_index(np.float32([0, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -24), np.float32(0))])).max() < 0
    assert CP.bin_index(np.float32([256.0, np.inf])).min() >= CP.TABLE
    assert CP.lookup(np.float32([0, 1e-9, 300.0, np.inf]), t).tolist() == [1.0, 1.0, t[-1], t[-1]]


# ---- 3. a hand-computed example -------------------------------------------------------------------------------------------------------
def test_a_hand_computed_example():
    """B = 2, A = 1, H = 1, six blocks, threshold -12 dB, ratio 2, no knee: the curve gives 0.5 at a peak of 1 (12 dB over: -6 dB) and
    1 at 0.125"""
    spec = {"threshold_db": -12, "ratio": 2, "knee_db": 0}
    t = CP.table(CP.check(spec))
    h = t[CP.bin_index(np.float32([1.0]))[0]]
    assert abs(20 * math.log10(h) + 6.0 + 20 * math.log10(2) - 6.0206) < 2e-3          # (1/2 - 1)(0 + 12.04) dB
    x = np.float32([.125, -.125, .125, .125, 1, .5, .125, .125, .125, .125, -.125])      # the last block holds one sample
    k = CP.gain_curve(x, 24000, spec, B=2, A=1, H=1)
    assert k["p"].tolist() == [.125, .125, 1, .125, .125, .125] and k["c"].tolist() == [1, 1, h, 1, 1, 1]
    # m[j] = min c[j - 1 .. j + 1], j = -2 .. 6
    assert k["m"].tolist() == [1, 1, 1, h, h, h, 1, 1, 1]
    hs = np.float32((float(h) + 1) / 2)
    # s[b] = (m[b - 1] + m[b]) / 2, b = -1 .. 6
    assert k["s"].tolist() == [1, 1, hs, h, h, hs, 1, 1]
    # a[b] = min(s[b - 1], s[b]), b = 0 .. 6, s[-1] := s[0], a[6] := s[5]
    assert k["a"].tolist() == [1, hs, h, h, h, hs, 1]
    a = k["a"].astype(np.float64)
    g = [a[0], (a[0] + a[1]) / 2, a[1], (a[1] + a[2]) / 2, a[2], a[2], a[3], a[3], a[4], (a[4] + a[5]) / 2, a[5]]
    assert k["g"].tolist() == [np.float32(v) for v in g]
    y, rec = CP.compress_segment(x, 24000, spec, B=2, A=1, H=1)
    assert y.tobytes() == (k["g"] * x).tobytes() and y[4] == h
    assert (rec["min_gain"], rec["n_blocks"], rec["n_touched"], rec["peak"]) == (h, 1, 10, 1.0)
    xn = x.copy()
    xn[4] = np.nan                                                                      # the block's peak is now 0.5
    yn, recn = CP.compress_segment(xn, 24000, spec, B=2, A=1, H=1)
    assert np.isnan(yn[4]) and np.isnan(yn).sum() == 1 and recn["peak"] == 0.5 and recn["n_blocks"] == 1


# ---- 4. the properties, on the cases of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", CC.RATES)
def test_the_properties_on_every_case(fs):
    B = fs // 1000
    for (name, x, spec), (y, rec) in zip(CC.cases(fs), CC.twin(fs)):
        k = CP.gain_curve(x, fs, spec)
        g, c = k["g"], k["c"]
        assert y.dtype == np.float32 and g.max() <= 1.0 and g.min() >= CP.ENTRY_MIN, name
        assert np.all(g <= c[np.arange(len(x)) // B]), name                                 # never more gain than the curve gives the block
        assert np.all(k["s"][1:-1] <= c) and rec["min_gain"] == g.min() and rec["n_blocks"] == (c < 1).sum(), name
        if rec["n_blocks"] == 0:
            assert y.tobytes() == x.tobytes() and rec["n_touched"] == 0 and rec["min_gain"] == 1.0, name
    names = [c[0] for c in CC.cases(fs)]
    assert CC.twin(fs)[names.index("quiet")][1]["n_blocks"] == 0 and CC.twin(fs)[names.index("silence")][1]["peak"] == 0
    yn = CC.twin(fs)[names.index("nan")][0]
    assert np.array_equal(np.isnan(yn), np.isnan(CC.cases(fs)[names.index("nan")][1]))


def test_a_pack_is_its_segments_alone():
    fs = 8000
    cs = CC.cases(fs)[::5]
    xs = [c[1] for c in cs]
    off = CC.offsets([len(x) for x in xs])
    specs = [c[2] for c in cs]
    specs[1] = None
    y, st = CP.compress(np.concatenate(xs), specs, offsets=off, rates=fs)
    for i in range(len(cs)):
        if i == 1:
            assert y[off[i]: off[i + 1]].tobytes() == xs[i].tobytes() and st[i].tobytes() == np.array((1.0, 0, 0, 0.0), dtype=CP.STATS).tobytes()
        else:
            ty, trec = CC.twin(fs)[5 * i]
            assert y[off[i]: off[i + 1]].tobytes() == ty.tobytes() and st[i].tobytes() == trec.tobytes()


@pytest.mark.parametrize("spec", [True, {"attack_ms": 20, "hold_ms": 30}])
def test_the_dependence_window(spec):
    """y[i] in block b depends on x only in blocks b - A - H - 1 .. b + A + 1"""
    fs, B = 8000, 8
    A, H = CP.blocks(CP.check(spec))
    x = CC.enveloped(77, 400 * B, B)
    y = CP.compress_segment(x, fs, spec)[0]
    r = np.random.default_rng(5)
    for b in (0, 57, 200, 399):
        for pb in (b - A - H - 2, b + A + 2):                                            # one block beyond either end of the window
            if 0 <= pb < 400:
                for v in (0.0, 0.99):
                    x2 = x.copy()
                    x2[pb * B + int(r.integers(B))] = v
                    y2 = CP.compress_segment(x2, fs, spec)[0]
                    assert y2[b * B: (b + 1) * B].tobytes() == y[b * B: (b + 1) * B].tobytes(), (b, pb, v)
    x2 = x.copy()
    x2[(57 + A + 1) * B] = 0.99                                                           # inside the window: the block does change
    assert CP.compress_segment(x2, fs, spec)[0][57 * B: 58 * B].tobytes() != y[57 * B: 58 * B].tobytes()


# ---- 5. the steady state ------------------------------------------------------------------------------------------------------------
BOUND_DB = 0.13         # a bin of 1/32 octave is 20 log10(2) / 32 = 0.19 dB of level; the slope 1 - 1/3 makes that 0.125 dB of gain


def test_the_steady_state_follows_the_law():
    fs = 24000
    t = np.arange(fs // 2) / fs
    x = (10 ** (-6 / 20) * np.sin(2 * np.pi * 1000 * t)).astype(np.float32)
    g = CP.gain_curve(x, fs, True)["g"]
    got = 20 * math.log10(g[int(0.2 * fs)])
    print(f"steady gain at -6 dBFS: {got:.4f} dB (the law: -12)")
    assert abs(got + 12.0) <= BOUND_DB and 20 * 0.30103 / 32 * (2 / 3) <= BOUND_DB
    # bursts of 300 ms at -6, -20 and -34 dBFS, 300 ms of silence between them: the RMS of each burst's middle 100 ms
    levels = (-6.0, -20.0, -34.0)
    n = int(0.3 * fs)
    tone = np.sin(2 * np.pi * 1000 * np.arange(n) / fs)
    x = np.concatenate([np.concatenate([10 ** (L / 20) * tone, np.zeros(n)]) for L in levels]).astype(np.float32)
    y = CP.compress_segment(x, fs, True)[0]
    rms = lambda v: 20 * math.log10(math.sqrt(float(np.mean(v.astype(np.float64) ** 2))))
    for i, L in enumerate(levels):
        mid = slice(2 * i * n + n // 3, 2 * i * n + 2 * n // 3)
        want = float(CP.law_db(L, CP.check(True)))
        got = rms(y[mid]) - rms(x[mid])
        print(f"burst at {L} dBFS: gain {got:.4f} dB, the law {want:.4f}")
        assert abs(got - want) <= BOUND_DB, L
    assert abs(float(CP.law_db(-6.0, DEFAULT)) + 12.0) < 1e-12 and float(CP.law_db(-34.0, DEFAULT)) == 0.0 and abs(float(CP.law_db(-24.0, DEFAULT)) + 0.5) < 1e-12


# ---- 6. refusals: the host tables and the C ABI ---------------------------------------------------------------------------------------
def test_tables_are_refused_on_the_host():
    for kw, why in ((dict(offsets=[1, 10]), "ascend from 0"), (dict(offsets=[0, 5, 5, 10]), "empty"), (dict(offsets=[0, 7, 5, 10]), "ascend"),
                    (dict(offsets=[0, 9]), "cover"), (dict(offsets=[0, 5, 10], rates=[24000]), "one rate per segment"),
                    (dict(rates=24005), "rate"), (dict(rates=7990), "rate"), (dict(rates=48010), "rate")):
        with pytest.raises(ValueError, match=why):
            CP.tables(10, True, **kw)
    for spec, why in ((None, "no segment asks"), ([None, False], "one compressor spec per row"), ({"ratio": 1}, "ratio")):
        with pytest.raises(ValueError, match=why):
            CP.tables(10, spec)
    with pytest.raises(ValueError, match="2\\^31"):
        CP.tables((1 << 31) - 4096, True)
    with pytest.raises(ValueError, match="65535"):
        CP.tables(65536, True, offsets=np.arange(65537))
    off, rates, par, tabs, specs = CP.tables(10, [True, None, {"hold_ms": 0}, True], offsets=[0, 2, 4, 6, 10], rates=[8000, 48000, 8000, 8000])
    assert par.tolist() == [[5, 60, 1, 0], [1, 0, -1, 0], [5, 0, 0, 0], [5, 60, 1, 0]] and tabs.shape == (2, CP.TABLE) and rates.dtype == np.int32
    assert tabs[1].tobytes() == CP.table(DEFAULT).tobytes() and CP.scratch_floats(10, 4) == 10 // 8 + 5


def test_library_symbols_and_refusals_before_any_launch():
    """the C entry point checks every host table first: these calls fail without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    with open(_lib.HERE + "/../include/chattts_amd.h") as f:
        header = f.read()
    for name in ("ctts_compress_ragged", "ctts_compress_ragged_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "compressor.hip" in build.SOURCES and "ctts_cp_stats" in header and f"#define CTTS_CP_TABLE {CP.TABLE}" in header
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ctts_compress_ragged_scratch_bytes(vp(i64([0, 2400, 12000])), 2) == (CP.scratch_floats(12000, 2) * 4 + 15) // 16 * 16
    assert lib.ctts_compress_ragged_scratch_bytes(vp(i64([0, 5, 5])), 2) == 0 and b"empty" in lib.ctts_last_error()
    assert lib.ctts_compress_ragged_scratch_bytes(vp(i64([0, (1 << 31) - 4096])), 1) == 0 and b"2^31" in lib.ctts_last_error()
    fake = 4096                       # never dereferenced: every call below is refused on its host arguments
    good = np.stack([CP.table(DEFAULT), CP.table(CP.check({"ratio": 20}))])

    def call(off=(0, 2400, 12000), rate=(24000, 8000), par=((5, 60, 0, 0), (1, 0, 1, 0)), tab=good, n_tab=2, x=fake, y=fake, scratch=fake, sb=1 << 20,
             null=None, n_seg=None, stats=fake, tab_dev=fake):
        o, r, p, t = i64(off), np.asarray(rate, np.int32), np.ascontiguousarray(par, np.int32), np.ascontiguousarray(tab, np.float32)
        d = {k: (None if k == null else fake) for k in ("off", "rate", "par")}
        rc = lib.ctts_compress_ragged(None if null == "x" else x, None if null == "y" else y, d["off"], vp(o), len(o) - 1 if n_seg is None else n_seg,
                                      d["rate"], None if null == "rate_host" else vp(r), d["par"], None if null == "par_host" else vp(p),
                                      None if null == "tab" else tab_dev, None if null == "tab_host" else vp(t), n_tab,
                                      None if null == "stats" else stats, scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    def bad_tab(v):
        t = good.copy()
        t[1, 700] = v
        return t

    for kw, why in ((dict(null="x"), "null"), (dict(null="y"), "null"), (dict(null="stats"), "null"), (dict(null="off"), "null"),
                    (dict(null="rate"), "null"), (dict(null="rate_host"), "null"), (dict(null="par"), "null"), (dict(null="par_host"), "null"),
                    (dict(null="tab"), "null"), (dict(null="tab_host"), "null"),
                    (dict(off=(1, 2400, 12000)), "must be 0"), (dict(off=(0, 2400, 2400)), "empty"), (dict(off=(0, 2400, 100)), "ascend"),
                    (dict(n_seg=0), "1 <= n_seg <= 65535"), (dict(n_seg=65536), "1 <= n_seg <= 65535"),
                    (dict(off=(0, 2400, (1 << 31) - 4096)), "2^31 - 4096"), (dict(rate=(24000, 7990)), "multiple of 10 Hz in 8000 .. 48000"),
                    (dict(rate=(48010, 8000)), "multiple of 10 Hz"), (dict(rate=(24005, 8000)), "multiple of 10 Hz"), (dict(rate=(-24000, 8000)), "multiple of 10 Hz"),
                    (dict(par=((0, 60, 0, 0), (1, 0, 1, 0))), "attack is 1 .. 20"), (dict(par=((21, 60, 0, 0), (1, 0, 1, 0))), "attack is 1 .. 20"),
                    (dict(par=((5, -1, 0, 0), (1, 0, 1, 0))), "hold is 0 .. 500"), (dict(par=((5, 60, 0, 0), (1, 501, 1, 0))), "hold is 0 .. 500"),
                    (dict(par=((5, 60, 2, 0), (1, 0, 1, 0))), "gain table 2 is outside"), (dict(par=((5, 60, 0, 0), (1, 0, -2, 0))), "gain table -2 is outside"),
                    (dict(n_tab=0), "1 <= n_tab <= n_seg"), (dict(n_tab=3), "1 <= n_tab <= n_seg"),
                    (dict(tab=bad_tab(1.5)), "table 1: entry 700"), (dict(tab=bad_tab(math.nan)), "table 1: entry 700"),
                    (dict(tab=bad_tab(2.0 ** -19)), "table 1: entry 700"), (dict(tab=bad_tab(0.0)), "table 1: entry 700"),
                    (dict(sb=1000), "scratch"), (dict(scratch=None), "scratch"), (dict(scratch=4104), "scratch"), (dict(x=4100), "16-byte aligned"),
                    (dict(y=4104), "16-byte aligned"), (dict(tab_dev=4104), "16-byte aligned"), (dict(stats=4097), "4-byte aligned"),
                    (dict(y=4096 + 160), "overlap")):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_compress_ragged" in msg and why in msg, (kw, msg)


# ---- 7. the plan ----------------------------------------------------------------------------------------------------------------------
class _Stages:
    """a codec that records the chain's calls"""

    def __init__(self):
        self.calls = []

    def trim_pauses(self, wav, spec, **kw):
        self.calls.append(("trim_pauses", sorted(kw)))
        return wav.reshape(-1), np.array([0, 4, 8], np.int64)

    def compress(self, wav, spec, **kw):
        self.calls.append(("compress", spec, {k: (v if k != "out" else v is wav) for k, v in kw.items()}))
        return wav

    def loudness_normalize(self, wav, target, **kw):
        self.calls.append(("loudness_normalize", target, sorted(kw)))
        return wav


def test_the_plan_places_the_stage_between_pauses_and_loudness():
    assert OC.STAGES.index("compress") > OC.STAGES.index("pauses") and "compress" in OC.STAGES
    p = OC.Plan.rows("t", 2, None, None, -16.0, True, True, [True, None])
    assert p.compress == [DEFAULT, None] and p.on and p.kwargs("compress") == {"compress": [DEFAULT, None]}
    assert OC.Plan.rows("t", 2, compress=[None, False]).compress is None and not OC.Plan.rows("t", 2, compress=False).on
    assert OC.Plan.batch("t", 2, compress={"ratio": 2}).compress == [(-24.0, 2.0, 6.0, 5.0, 60.0)] * 2
    with pytest.raises(ValueError, match="t: one compressor spec per row"):
        OC.Plan.rows("t", 2, compress=[True])
    with pytest.raises(ValueError, match="rate"):
        OC.Plan.rows("t", 1, sample_rate=11025, compress=True)
    assert OC.Plan.rows("t", 1, sample_rate=11025).on                                      # without the option the rate is the resampler's business
    g = OC.Plan.given("t", compress=[True, None, {"hold_ms": 0}])
    assert g.compress == [DEFAULT, None, (-24.0, 3.0, 6.0, 5.0, 0.0)] and OC.Plan.given("t", compress=False).compress is None
    assert "compress" not in OC.Plan.given("t", loudness=-16).kwargs() and OC.Plan.given("t", compress=True).kwargs() == {"compress": DEFAULT}
    s = g.per_sentence([[0, 1], [2], [3, 4, 5]])
    assert s.compress == [DEFAULT, DEFAULT, None, *[(-24.0, 3.0, 6.0, 5.0, 0.0)] * 3]
    with pytest.raises(ValueError, match="one compressor spec per request"):
        g.per_sentence([[0], [1]])
    assert OC.Plan.given("t", compress=True).per_sentence([[0, 1]]).compress == DEFAULT      # one for all stays one
    codec, wav = _Stages(), torch.zeros((2, 4))
    OC.run(codec, wav, OC.Plan.batch("t", 2, None, None, -16.0, True, True, True), in_place=True)
    assert [c[0] for c in codec.calls] == ["trim_pauses", "compress", "loudness_normalize"]
    assert codec.calls[1][1:] == ([DEFAULT, DEFAULT], {"offsets": pytest.approx([0, 4, 8]), "rates": 24000, "out": True})
    codec.calls.clear()
    OC.run(codec, wav, OC.Plan.batch("t", 2, compress=True))
    assert codec.calls == [("compress", [DEFAULT, DEFAULT], {"rates": 24000})]
    codec.calls.clear()
    OC.run(codec, wav, OC.Plan.batch("t", 2, loudness=-16.0))
    assert [c[0] for c in codec.calls] == ["loudness_normalize"]


# ---- 8. Chat --------------------------------------------------------------------------------------------------------------------------
def test_chat_passes_the_spec_on_and_nothing_when_it_is_off():
    chat = _chat()
    rows = [torch.zeros(3, 768), torch.zeros(2, 768)]
    chat.decode_to_wavs(rows, ragged=True, compress=[True, None])
    chat.decode_to_wavs(rows, ragged=True, compress=[False, None])
    chat.decode_to_wavs(rows, compress={"ratio": 2}, loudness=-23.0, sample_rate=8000)
    chat.decode_to_wavs(rows)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": None, "compress": [DEFAULT, None]}), ("decode_ragged", {"sample_rate": None}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": 8000, "loudness": -23.0, "compress": (-24.0, 2.0, 6.0, 5.0, 60.0)}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": None})]
    with pytest.raises(ValueError, match="unknown compressor field"):
        chat.decode_to_wavs(rows, compress={"on": True})
    chat.codec.calls.clear()
    groups = [[torch.zeros(3, 768), torch.zeros(2, 768)], [torch.zeros(2, 768)]]
    chat.decode_split_to_pcm16(groups, compress=[True, None], loudness=-19.0)
    chat.decode_split_to_pcm16(groups, compress=False)
    assert chat.codec.calls[0] == ("decode_ragged", {"sample_rate": None, "compress": [DEFAULT, DEFAULT, None]})       # every sentence alone
    assert chat.codec.calls[1][0] == "loudness_normalize" and "compress" not in chat.codec.calls[1][2]
    assert ("decode_ragged", {"sample_rate": None}) in chat.codec.calls[2:]
    with pytest.raises(ValueError, match="one compressor spec per request"):
        chat.decode_split_to_pcm16(groups, compress=[True])
    seen = []

    def fake_infer(text, *a, **kw):
        seen.append(kw)
        yield [np.full(5, 0.5, np.float32) for _ in text]
    chat._infer = fake_infer
    kw = dict(skip_refine_text=True, split_text=False)
    chat.infer(["a", "b"], compress=[True, False], **kw)
    chat.infer(["a", "b"], **kw)
    chat.infer(["a", "b"], compress=False, pcm16=True, **kw)
    assert seen[0]["compress"] == [DEFAULT, None] and "compress" not in seen[1] and "compress" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "compress"} == seen[1]
    seen.clear()
    chat.infer("a. b. c.", compress=True, loudness=-20.0, skip_refine_text=True)           # split on the host: the sentences compressed in the decode,
    assert seen[0]["compress"] == DEFAULT and "loudness" not in seen[0]                     # ONE gain over them afterwards
    assert chat.codec.calls[-1][0] == "loudness_normalize" and "compress" not in chat.codec.calls[-1][2]


def test_streams_are_refused():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="non-streamed.*block state carried across chunks"):
        chat.infer(["hello"], stream=True, compress=True)
    with pytest.raises(ValueError, match="True, False, None or a dict"):
        chat.infer(["hello"], compress=1)
    with pytest.raises(ValueError, match="one compressor spec"):
        chat.infer(["a", "b"], split_text=True, compress=[True, False])
    with pytest.raises(ValueError, match="rate"):
        chat.infer(["hello"], sample_rate=11025, compress=True)
    lock = threading.Lock()
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _Pool(2, lock), streams=True)
    try:
        with pytest.raises(TypeError):
            b.submit_stream("a#8", _Params(), compress=True)
        for bad in (1, "x", [True], {"ratio": 1}):
            with pytest.raises(ValueError):
                b.submit("a#8", _Params(), compress=bad)
        with pytest.raises(ValueError, match="rate"):
            b.submit("a#8", _Params(), compress=True, sample_rate=11025)
    finally:
        b.close()


# ---- 9. the batcher -------------------------------------------------------------------------------------------------------------------
def test_requests_with_and_without_the_compressor_share_one_decode():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), **kw) for c, kw in (("a", dict(compress=True)), ("b", dict(loudness=-23.0, compress={"ratio": 8})),
                                                                      ("c", {}), ("d", dict(loudness=-16.0)))]
        res = [f.result(timeout=10) for f in futs]
        b.submit("e#8", _Params(), compress=False).result(timeout=10)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.pcm_kw == [{"loudness": [None, -23.0, None, -16.0], "compress": [DEFAULT, (-24.0, 8.0, 6.0, 5.0, 60.0), None, None]}, {}]
    assert b.decode_calls == 2 and [int(r[0]) for r in res] == [ord(c) for c in "abcd"]


def test_batcher_passes_the_spec_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    try:
        b.submit("a#8", _Params(), compress=True).result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, compress=True).result(timeout=30)
        b.submit("m#8\nn#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.wav_kw == [{"compress": DEFAULT}, {}] and chat.split_kw == [{"compress": [DEFAULT]}, {}]


# ---- 10. the endpoint -----------------------------------------------------------------------------------------------------------------
def test_endpoint_compress():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: an unknown key -- the warning, and today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "compress": True})
        assert r.status_code == 200 and r.content == r0.content and sorted(chat.calls[-1][2]) == sorted(chat.calls[-2][2]) and "compress" not in chat.calls[-1][2]
        assert catch.msgs == ["ignoring unsupported parameters: ['compress']"]
        assert c.post("/v1/audio/speech", json={**body, "compress": "hard"}).status_code == 200      # ignored, whatever it holds
        assert "compress" not in c.get("/health").json()

    app, chat, catch = _app(compress=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "compress": True})
        assert r.status_code == 200 and chat.calls[-1][2]["compress"] == DEFAULT and chat.calls[-1][1] is False and "loudness" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={**body, "compress": {"ratio": 4, "hold_ms": 100}})
        assert r.status_code == 200 and chat.calls[-1][2]["compress"] == (-24.0, 4.0, 6.0, 5.0, 100.0)
        for off in ({}, {"compress": False}, {"compress": None}):
            assert c.post("/v1/audio/speech", json={**body, **off}).status_code == 200 and "compress" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        assert c.post("/v1/audio/speech", json={**body, "stream": True, "compress": False}).status_code == 200
        n = len(chat.calls)
        for bad, why in ((1, "True, False, None or a dict"), ("true", "True, False, None or a dict"), ([True], "a dict"), ({"on": True}, "unknown compressor field"),
                         ({"ratio": 1}, "ratio is a number in 1.5 .. 20"), ({"attack_ms": True}, "attack_ms is a number")):
            r = c.post("/v1/audio/speech", json={**body, "compress": bad})
            assert r.status_code == 400 and why in r.text, bad
        r = c.post("/v1/audio/speech", json={**body, "compress": True, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "block state carried across chunks" in r.text and len(chat.calls) == n
        assert not catch.msgs
        assert c.get("/health").json()["compress"] is True and "loudness" not in c.get("/health").json()

    app, chat, catch = _app(compress=True, limiter=True, loudness=True, sample_rates=(8000, 11025, 24000), g711=True, speed=True, flac=True, pauses=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "compress": True, "limiter": True, "loudness": -20.5, "speed": 0.8, "sample_rate": 8000, "encoding": "ulaw",
                                             "pauses": True})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["compress"], kw["limiter"], kw["loudness"], kw["speed"], kw["sample_rate"], kw["encoding"]) == \
            (DEFAULT, True, -20.5, 0.8, 8000, "ulaw") and kw["pauses"] is not None
        r = c.post("/v1/audio/speech", json={**body, "response_format": "flac", "compress": True})
        assert r.status_code == 200 and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["compress"] == DEFAULT
        assert c.post("/v1/audio/speech", json={**body, "compress": True, "sample_rate": 11025}).status_code == 400      # no multiple of 10 Hz
        assert c.post("/v1/audio/speech", json={**body, "compress": False, "sample_rate": 11025}).status_code == 200

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, compress=True, loudness=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "compress": True}).status_code == 200 and bat.calls[-1][2] == {"compress": DEFAULT}
        assert c.post("/v1/audio/speech", json={**body, "compress": True, "loudness": -16}).status_code == 200
        assert bat.calls[-1][2] == {"loudness": -16.0, "compress": DEFAULT}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

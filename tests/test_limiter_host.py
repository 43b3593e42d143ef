"""The look-ahead peak limiter, the parts that need no GPU: the NumPy twin (chattts_amd/limiter.py) against the brute-force oracle
(tests/limiter_oracle.py) bit for bit, the definition's two properties, a hand-computed example, the loudness twin without its ceiling
term, every refusal of the host side and of ctts_peak_limit_ragged / ctts_loudness_limited_ragged, and the plumbing of `limiter`
through Chat, the batcher and the endpoint on fakes."""
import ctypes as C
import math
import threading

import numpy as np
import pytest
import torch

from chattts_amd import _lib, build, limiter as LM, loudness as LN
from chattts_amd.serving import SpeechBatcher
from tests import limiter_cases as LMC
from tests import limiter_oracle as O
from tests import loudness_cases as LC
from tests.test_loudness_host import _LoudChat, _app, _chat
from tests.test_split_pool_host import _FakeBatcher, _FakeChat, _Params, _Pool, _spell, _wait_idle


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------------
def test_the_constants():
    assert LM.C32 == np.float32(10.0 ** (-1.0 / 20.0)) == O.CEILING32 and LM.T == O.THRESHOLD
    assert LM.T < LM.C32 and np.nextafter(np.nextafter(np.nextafter(np.nextafter(LM.T, np.float32(1)), np.float32(1)), np.float32(1)), np.float32(1)) == LM.C32
    assert LM.STATS.itemsize == 16 and LM.STATS.names == ("g32", "min_gain", "n_over", "n_touched")
    assert LM.TILE >= 2 * 480                        # a halo of 2 W reaches the adjacent tile only: what the early exit relies on


@pytest.mark.parametrize("fs", LMC.RATES)
def test_the_twin_equals_the_oracle_on_every_case(fs):
    W = fs // 100
    assert LMC.lengths(fs) == (1, W, 2 * W, 2 * W + 1, 2 * W + 2, LM.TILE - 1, LM.TILE, LM.TILE + 1, 2 * LM.TILE + 1)
    for (name, x, g), (y, rec) in zip(LMC.cases(fs), LMC.twin(fs)):
        o = O.stages(x, fs, g)
        assert y.dtype == np.float32 and y.tobytes() == o["y"].tobytes(), (name, fs)
        assert (rec["g32"], rec["min_gain"], rec["n_over"], rec["n_touched"]) == (o["g32"], o["min_gain"], o["n_over"], o["n_touched"]), (name, fs)
        u, r, s = LM.gain_curve(x, fs, g)
        assert u.tobytes() == o["u"].tobytes() and r.tobytes() == o["r"].tobytes() and s.tobytes() == o["s"].tobytes(), (name, fs)
        assert LM.window_min(r, W).tobytes() == o["m"].tobytes(), (name, fs)


@pytest.mark.parametrize("fs", LMC.RATES)
def test_the_two_properties_and_the_families(fs):
    W = fs // 100
    recs = {}
    for (name, x, g), (y, rec) in zip(LMC.cases(fs), LMC.twin(fs)):
        u, r, s = LM.gain_curve(x, fs, g)
        assert np.all(np.abs(y) <= LM.C32), (name, fs)                       # the peak bound
        assert np.all(s <= np.float32(1.0)) and np.all(s <= r) and s.min() >= r.min(), (name, fs)
        if rec["n_over"] == 0:                                               # untouched: s == 1 exactly, y == u bit for bit
            assert np.all(s == np.float32(1.0)) and y.tobytes() == u.tobytes() and rec["n_touched"] == 0 and rec["min_gain"] == 1.0, (name, fs)
        assert r.min() >= LM.R_MIN, (name, fs)                               # THE CONDITION: every case stays inside it
        recs[name] = rec
    n2 = 2 * LM.TILE + 1
    assert all(recs[f"quiet_{n}"]["n_over"] == 0 for n in LMC.lengths(fs))
    assert all(recs[f"first_{n}"]["n_over"] == 1 and recs[f"first_{n}"]["n_touched"] == min(n, 2 * W + 1) for n in LMC.lengths(fs))
    assert all(recs[f"last_{n}"]["n_over"] == 1 and recs[f"last_{n}"]["n_touched"] == min(n, 2 * W + 1) for n in LMC.lengths(fs))
    assert recs[f"edge_lo_{n2}"]["n_touched"] == recs[f"edge_hi_{n2}"]["n_touched"] == 4 * W + 1
    # peaks 2 W apart: the dips share one sample of m; 2 W + 1 apart: they do not -- either way s dips over 6 W + 1 resp. 6 W + 2 samples
    assert recs[f"pair2W_{n2}"]["n_touched"] == 6 * W + 1 and recs[f"pair2W1_{n2}"]["n_touched"] == 6 * W + 2
    assert recs["dense"]["n_over"] > 1000 and recs["at_T"]["n_over"] == 0 and recs["above_T"]["n_over"] == 1
    assert recs["above_T"]["min_gain"] == np.nextafter(np.float32(1), np.float32(0)) and recs["above_T"]["n_touched"] == 2 * W + 1


def test_a_hand_computed_example():
    """12 samples, W = 1: windows of 3"""
    T = float(LM.T)
    x = np.zeros(12, np.float32)
    x[4], x[10] = np.float32(2) * LM.T, np.float32(-4) * LM.T                # r = 1/2 and 1/4 exactly
    u, r, s = LM.gain_curve(x, 24000, 1.0, W=1)
    assert r.tolist() == [1, 1, 1, 1, 0.5, 1, 1, 1, 1, 1, 0.25, 1]
    m = LM.window_min(r, 1)                                                   # positions -1 .. 12
    assert m.tolist() == [1, 1, 1, 1, 0.5, 0.5, 0.5, 1, 1, 1, 0.25, 0.25, 0.25, 1]
    want = np.array([3, 3, 2.5, 2, 1.5, 2, 2.5, 3, 2.25, 1.5, 0.75, 1.5], np.float64) / 3.0
    assert s.tobytes() == want.astype(np.float32).tobytes() and LM.smooth(m, 1).tobytes() == s.tobytes()
    y, rec = LM.limit_segment(x, 24000, 1.0, W=1)
    assert y[4] == np.float32(0.5) * x[4] == LM.T and y[10] == -LM.T and (rec["min_gain"], rec["n_over"], rec["n_touched"]) == (0.25, 2, 9)
    o = O.stages(x, W=1)
    assert o["m"].tobytes() == m.tobytes() and o["s"].tobytes() == s.tobytes() and o["y"].tobytes() == y.tobytes()
    xn = x.copy()
    xn[7] = np.nan                                                            # a NaN asks for no gain and passes through
    yn, recn = LM.limit_segment(xn, 24000, 1.0, W=1)
    assert np.isnan(yn[7]) and np.isnan(yn).sum() == 1 and recn["n_over"] == 2 and np.delete(yn, 7).tobytes() == np.delete(y, 7).tobytes()
    assert abs(T - 0.89125067) < 1e-7


def test_a_pack_is_its_segments_alone():
    cs = LMC.cases(8000)[:9]
    xs, gs = [c[1] for c in cs], [c[2] for c in cs]
    y, st = LM.limit(np.concatenate(xs), LMC.offsets([len(x) for x in xs]), 8000, gs)
    off = LMC.offsets([len(x) for x in xs])
    for i in range(len(cs)):
        assert y[off[i]: off[i + 1]].tobytes() == LMC.twin(8000)[i][0].tobytes() and st[i].tobytes() == LMC.twin(8000)[i][1].tobytes()


# ---- 2. together with loudness ------------------------------------------------------------------------------------------------------
def test_the_loudness_twin_drops_the_ceiling_term():
    assert LN.gain(-13.0, 1.0, -5.0)[1] == LN.BOUND_CEILING
    g, b = LN.gain(-13.0, 1.0, -5.0, limiter=True)
    assert b == LN.BOUND_TARGET and g == np.float32(10.0 ** 0.4)
    assert LN.gain(-60.0, 1.0, -10.0, limiter=True) == (np.float32(10 ** 1.5), LN.BOUND_CAP)
    assert LN.gain(-20.0, 0.1, None, limiter=True) == (np.float32(1.0), LN.BOUND_NONE)
    names = [s[0] for s in LC.signals()]
    x = LC.signals()[names.index("bursts")][1]
    y0, st0 = LN.normalize(x, -5.0)
    y1, st1, ls = LN.normalize(x, -5.0, limiter=True)
    assert st0["bound"][0] == LN.BOUND_CEILING and st1["bound"][0] == LN.BOUND_TARGET and st1["g32"][0] > st0["g32"][0]
    assert st1["L"][0] == st0["L"][0] and st1["peak"][0] == st0["peak"][0]
    ty, trec = LM.limit_segment(x, 24000, st1["g32"][0])
    assert y1.tobytes() == ty.tobytes() and ls[0].tobytes() == trec.tobytes() and ls["n_over"][0] > 0 and np.abs(y1).max() <= LM.C32
    # a group: ONE gain, the limiter over every sentence alone; a group that does not ask is as without the option
    idx = [names.index(n) for n in ("bursts", "env4_9600", "env1_2399")]
    xs = [LC.signals()[i][1] for i in idx]
    off = LC.offsets([len(v) for v in xs])
    y, st, ls = LN.normalize(np.concatenate(xs), [-5.0, -16.0], offsets=off, groups=[0, 2, 3], limiter=[True, False])
    assert st["bound"][0] in (0, 1) and ls["g32"][0] == ls["g32"][1] == st["g32"][0] and ls["g32"][2] == 0
    for k in (0, 1):
        assert y[off[k]: off[k + 1]].tobytes() == LM.limit_segment(xs[k], 24000, st["g32"][0])[0].tobytes()
    plain = LN.normalize(xs[2], -16.0)
    assert y[off[2]:].tobytes() == plain[0].tobytes() and st[1].tobytes() == plain[1][0].tobytes()
    # no target, a silent group: the limiter at unity gain
    y, st, ls = LN.normalize(np.float32(3) * xs[0], None, limiter=True)
    assert st["g32"][0] == 1.0 and ls["g32"][0] == 1.0 and y.tobytes() == LM.limit_segment(np.float32(3) * xs[0], 24000)[0].tobytes()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_flags_rates_and_tables_are_refused_on_the_host():
    for v in (1, 0, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="True or False"):
            LM.check_flag(v)
    assert LM.check_flag(None) is False and LM.check_flag(np.bool_(True)) is True
    assert LM.per_row(None, 2) is None and LM.per_row(False, 2) is None and LM.per_row([False, None], 2) is None
    assert LM.per_row(True, 2) == [True, True] and LM.per_row([None, True], 2) == [False, True]
    with pytest.raises(ValueError, match="one limiter flag per row"):
        LM.per_row([True], 2)
    for kw, why in ((dict(offsets=[1, 10]), "ascend from 0"), (dict(offsets=[0, 5, 5, 10]), "empty"), (dict(offsets=[0, 7, 5, 10]), "ascend"),
                    (dict(offsets=[0, 9]), "cover"), (dict(offsets=[0]), "ascend"), (dict(offsets=[0, 5, 10], rates=[24000]), "one rate per segment"),
                    (dict(rates=24005), "rate"), (dict(rates=7990), "rate"), (dict(rates=48010), "rate"), (dict(rates=24000.0), "rate"),
                    (dict(offsets=[0, 5, 10], gains=[1.0]), "one pre-gain"), (dict(gains=0.0), "positive finite"), (dict(gains=-1.0), "positive finite"),
                    (dict(gains=math.inf), "positive finite"), (dict(gains=math.nan), "positive finite")):
        with pytest.raises(ValueError, match=why):
            LM.tables(10, **kw)
    with pytest.raises(ValueError, match="2\\^31"):
        LM.tables((1 << 31) - 4096)
    with pytest.raises(ValueError, match="65535"):
        LM.tables(65536, offsets=np.arange(65537))
    off, rates, g = LM.tables(10, offsets=[0, 4, 10], rates=[8000, 48000], gains=2)
    assert off.dtype == np.int64 and rates.dtype == np.int32 and rates.tolist() == [8000, 48000] and g.dtype == np.float32 and g.tolist() == [2.0, 2.0]
    assert LM.tables(10)[1].tolist() == [24000] and LM.tables(10)[2].tolist() == [1.0]


def test_library_symbols_and_refusals_before_any_launch():
    """the C entry points check every host table first: these calls fail without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    with open(_lib.HERE + "/../include/chattts_amd.h") as f:
        header = f.read()
    for name in ("ctts_peak_limit_ragged", "ctts_peak_limit_ragged_scratch_bytes", "ctts_loudness_limited_ragged"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "limiter.hip" in build.SOURCES and lib.ctts_version() == 1
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    off = i64([0, 2400, 12000])
    assert lib.ctts_peak_limit_ragged_scratch_bytes(vp(off), 2) == 12000 * 4 + (12000 // LM.TILE + 2 + 1) * 4
    assert lib.ctts_peak_limit_ragged_scratch_bytes(vp(i64([0, 5, 5])), 2) == 0 and b"empty" in lib.ctts_last_error()
    assert lib.ctts_peak_limit_ragged_scratch_bytes(vp(i64([0, (1 << 31) - 4096])), 1) == 0 and b"2^31" in lib.ctts_last_error()
    fake = 4096                       # never dereferenced: every call below is refused on its host arguments

    def call(off=(0, 2400, 12000), rate=(24000, 8000), x=fake, y=fake, scratch=fake, sb=1 << 20, null=None, n_seg=None, gain=fake, stats=fake):
        o, r = i64(off), np.asarray(rate, np.int32)
        p = {k: (None if k == null else fake) for k in ("off", "rate")}
        rc = lib.ctts_peak_limit_ragged(None if null == "x" else x, None if null == "y" else y, p["off"], vp(o), len(o) - 1 if n_seg is None else n_seg,
                                        p["rate"], vp(r), None if null == "gain" else gain, None if null == "stats" else stats, scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    for kw, why in ((dict(null="x"), "null"), (dict(null="y"), "null"), (dict(null="stats"), "null"), (dict(null="gain"), "null"),
                    (dict(null="off"), "null"), (dict(null="rate"), "null"),
                    (dict(off=(1, 2400, 12000)), "must be 0"), (dict(off=(0, 2400, 2400)), "empty"), (dict(off=(0, 2400, 100)), "ascend"),
                    (dict(n_seg=0), "1 <= n_seg <= 65535"), (dict(n_seg=65536), "1 <= n_seg <= 65535"),
                    (dict(off=(0, 2400, (1 << 31) - 4096)), "2^31 - 4096"), (dict(rate=(24000, 7990)), "multiple of 10 Hz in 8000 .. 48000"),
                    (dict(rate=(48010, 8000)), "multiple of 10 Hz"), (dict(rate=(24005, 8000)), "multiple of 10 Hz"), (dict(rate=(-24000, 8000)), "multiple of 10 Hz"),
                    (dict(sb=48000), "scratch"), (dict(scratch=None), "scratch"), (dict(scratch=4104), "scratch"), (dict(x=4100), "16-byte aligned"),
                    (dict(y=4104), "16-byte aligned"), (dict(gain=4098), "4-byte aligned"), (dict(stats=4097), "4-byte aligned"),
                    (dict(y=4096 + 160), "overlap")):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_peak_limit_ragged" in msg and why in msg, (kw, msg)

    coef, _ = LN.coef_table([24000, 8000])

    def loud(lim=(1, 0), null=None, target=(-16.0, math.nan), gain=fake):
        o, r, g, t, l = i64([0, 2400, 12000]), np.asarray([1, 0], np.int32), np.asarray([0, 1, 2], np.int32), np.asarray(target, np.float64), np.asarray(lim, np.int32)
        rc = lib.ctts_loudness_limited_ragged(fake, fake, fake, vp(o), 2, fake, vp(r), fake, vp(coef), coef.shape[0], fake, vp(g), 2, fake, vp(t),
                                              None if null == "lim" else fake, None if null == "lim_host" else vp(l), None if null == "gain" else gain,
                                              None if null == "stats" else fake, fake, 100, None)
        return rc, lib.ctts_last_error().decode()

    for kw, why in ((dict(null="lim"), "null"), (dict(null="lim_host"), "null"), (dict(null="gain"), "null"), (dict(lim=(2, 0)), "0 or 1"),
                    (dict(lim=(0, -1)), "0 or 1"), (dict(gain=4098), "4-byte aligned"), (dict(null="stats"), "null"), (dict(target=(-3.0, -16.0)), "-40 .. -5"),
                    (dict(), "scratch")):                                     # the last: everything passed but the 100 bytes of scratch
        rc, msg = loud(**kw)
        assert rc != 0 and "ctts_loudness_limited_ragged" in msg and why in msg, (kw, msg)


def test_streams_are_refused():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="non-streamed.*look-ahead"):
        chat.infer(["hello"], stream=True, limiter=True)
    with pytest.raises(ValueError, match="True or False"):
        chat.infer(["hello"], limiter=1)
    with pytest.raises(ValueError, match="one limiter flag"):
        chat.infer(["a", "b"], split_text=True, limiter=[True, False])
    with pytest.raises(ValueError, match="rate"):
        chat.infer(["hello"], sample_rate=11025, limiter=True)
    lock = threading.Lock()
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _Pool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed.*look-ahead"):
            b.submit_stream("a#8", _Params(), limiter=True)
        for bad in (1, "x", [True]):
            with pytest.raises(ValueError):
                b.submit("a#8", _Params(), limiter=bad)
            with pytest.raises(ValueError):
                b.submit_stream("a#8", _Params(), limiter=bad)
        with pytest.raises(ValueError, match="rate"):
            b.submit("a#8", _Params(), limiter=True, sample_rate=11025)
    finally:
        b.close()


# ---- 4. Chat: the argument reaches the decode, and nothing does without it -------------------------------------------------------------
class _Stop(Exception):
    pass


def test_chat_decode_calls_pass_the_flag_on_and_nothing_when_it_is_off():
    chat = _chat()
    rows = [torch.zeros(3, 768), torch.zeros(2, 768)]
    chat.decode_to_wavs(rows, ragged=True, limiter=[True, False])
    chat.decode_to_wavs(rows, ragged=True)
    chat.decode_to_wavs(rows, ragged=True, limiter=[False, None])
    chat.decode_to_wavs(rows, ragged=True, limiter=False, loudness=-16)
    chat.decode_to_wavs(rows, limiter=True, loudness=-23.0, sample_rate=8000)
    chat.decode_to_wavs(rows, limiter=True)
    chat.decode_to_wavs(rows)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": None, "limiter": [True, False]}), ("decode_ragged", {"sample_rate": None}),
                                ("decode_ragged", {"sample_rate": None}), ("decode_ragged", {"sample_rate": None, "loudness": -16.0}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": 8000, "loudness": -23.0, "limiter": True}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": None, "limiter": True}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": None})]
    with pytest.raises(ValueError, match="True or False"):
        chat.decode_to_wavs(rows, limiter="on")
    chat.codec.calls.clear()
    ragged = chat.codec.decode_ragged

    def decode_then_stop(rows, **kw):                 # the FLAC and G.711 paths: what reaches the decode is the point
        ragged(rows, **kw)
        raise _Stop
    chat.codec.decode_ragged = decode_then_stop
    for kw in (dict(limiter=True, loudness=[-16.0, None], flac=True, sample_rate=8000), dict(flac=True, sample_rate=8000),
               dict(limiter=[False, True], encoding="ulaw"), dict(encoding="ulaw"), dict(limiter=True)):
        with pytest.raises(_Stop):
            chat.decode_to_pcm16(rows, ragged=True, **kw)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": 8000, "loudness": [-16.0, None], "limiter": True}), ("decode_ragged", {"sample_rate": 8000}),
                                ("decode_ragged", {"sample_rate": None, "limiter": [False, True]}), ("decode_ragged", {"sample_rate": None}),
                                ("decode_ragged", {"sample_rate": None, "limiter": True})]
    chat.codec.decode_ragged = ragged
    chat.codec.calls.clear()
    groups = [[torch.zeros(3, 768), torch.zeros(2, 768)]]
    chat.decode_split_to_pcm16(groups, limiter=True, sample_rate=8000)
    chat.decode_split_to_pcm16(groups, limiter=[True], loudness=-19.0)
    chat.decode_split_to_pcm16(groups, limiter=False)
    both = {"offsets": pytest.approx([0, 12, 20]), "groups": pytest.approx([0, 2]), "out": True}
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": 8000}), ("loudness_normalize", None, {**both, "rates": [8000, 8000], "limiter": True}),
                                ("float_to_int16_groups", [0, 2]), ("decode_ragged", {"sample_rate": None}),
                                ("loudness_normalize", -19.0, {**both, "rates": [24000, 24000], "limiter": [True]}), ("float_to_int16_groups", [0, 2]),
                                ("decode_ragged", {"sample_rate": None}), ("float_to_int16_groups", [0, 2])]
    with pytest.raises(ValueError, match="one limiter flag per request"):
        chat.decode_split_to_pcm16(groups, limiter=[True, False])


def test_chat_infer_passes_the_flag_on_and_nothing_when_it_is_off():
    chat = _chat()
    seen = []

    def fake_infer(text, *a, **kw):
        seen.append(kw)
        yield [np.full(5, 0.5, np.float32) for _ in text]
    chat._infer = fake_infer
    kw = dict(skip_refine_text=True, split_text=False)
    chat.infer(["a", "b"], limiter=[True, False], **kw)
    chat.infer(["a", "b"], **kw)
    chat.infer(["a", "b"], limiter=False, pcm16=True, **kw)
    chat.infer(["a", "b"], limiter=True, loudness=-16.0, **kw)
    assert seen[0]["limiter"] == [True, False] and "limiter" not in seen[1] and "limiter" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "limiter"} == seen[1]
    assert seen[3]["limiter"] is True and seen[3]["loudness"] == -16.0
    # a split request that is concatenated on the host: the decode stays untouched, ONE group over the sentences afterwards
    seen.clear()
    out = chat.infer("a. b. c.", limiter=True, skip_refine_text=True)
    assert "limiter" not in seen[0] and "loudness" not in seen[0] and len(out) == 1 and len(out[0]) == 15
    call = chat.codec.calls[-1]
    assert call[0] == "loudness_normalize" and call[1] is None and list(call[2]["groups"]) == [0, 3] and list(call[2]["offsets"]) == [0, 5, 10, 15]
    assert call[2]["rates"] == 24000 and call[2]["limiter"] is True
    chat.infer("a. b. c.", limiter=True, loudness=-20.0, skip_refine_text=True)
    assert chat.codec.calls[-1][1] == -20.0 and chat.codec.calls[-1][2]["limiter"] is True
    n = len(chat.codec.calls)
    chat.infer("a. b. c.", loudness=-20.0, skip_refine_text=True)
    assert len(chat.codec.calls) == n + 1 and "limiter" not in chat.codec.calls[-1][2]


# ---- 5. the batcher ---------------------------------------------------------------------------------------------------------------------
def test_requests_with_and_without_the_limiter_share_one_decode():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), **kw) for c, kw in (("a", dict(limiter=True)), ("b", dict(loudness=-23.0, limiter=True)), ("c", {}),
                                                                      ("d", dict(loudness=-16.0)))]
        res = [f.result(timeout=10) for f in futs]
        b.submit("e#8", _Params(), limiter=False).result(timeout=10)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.pcm_kw == [{"loudness": [None, -23.0, None, -16.0], "limiter": [True, True, False, False]}, {}] and b.decode_calls == 2
    assert [int(r[0]) for r in res] == [ord(c) for c in "abcd"]


def test_batcher_passes_the_flag_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    try:
        b.submit("a#8", _Params(), limiter=True).result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("d#8", _Params(), loudness=-20.0, sample_rate=8000, speed=1.25, limiter=True).result(timeout=10)
        pcm = b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, limiter=True).result(timeout=30)
        b.submit("m#8\nn#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.wav_kw == [{"limiter": True}, {}, {"sample_rate": 8000, "speed": 1.25, "loudness": -20.0, "limiter": True}]
    assert chat.split_kw == [{"limiter": [True]}, {}] and _spell(pcm) == [("k", 8), ("l", 8)]


# ---- 6. the endpoint ------------------------------------------------------------------------------------------------------------------
def test_endpoint_limiter():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: an unknown key -- the warning, and today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "limiter": True})
        assert r.status_code == 200 and r.content == r0.content and sorted(chat.calls[-1][2]) == sorted(chat.calls[-2][2]) and "limiter" not in chat.calls[-1][2]
        assert catch.msgs == ["ignoring unsupported parameters: ['limiter']"]
        assert c.post("/v1/audio/speech", json={**body, "limiter": "hard"}).status_code == 200      # ignored, whatever it holds
        assert "limiter" not in c.get("/health").json()

    app, chat, catch = _app(limiter=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "limiter": True})
        assert r.status_code == 200 and chat.calls[-1][2]["limiter"] is True and chat.calls[-1][1] is False and "loudness" not in chat.calls[-1][2]
        for off in ({}, {"limiter": False}, {"limiter": None}):
            assert c.post("/v1/audio/speech", json={**body, **off}).status_code == 200 and "limiter" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        assert c.post("/v1/audio/speech", json={**body, "stream": True, "limiter": False}).status_code == 200
        n = len(chat.calls)
        for bad in (1, 0, "true", [True], {"on": True}, 0.5):
            r = c.post("/v1/audio/speech", json={**body, "limiter": bad})
            assert r.status_code == 400 and "true or false" in r.text, bad
        r = c.post("/v1/audio/speech", json={**body, "limiter": True, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "look-ahead is not carried" in r.text and len(chat.calls) == n
        assert not catch.msgs
        assert c.get("/health").json()["limiter"] is True and "loudness" not in c.get("/health").json()

    app, chat, catch = _app(limiter=True, loudness=True, sample_rates=(8000, 11025, 24000), g711=True, speed=True, flac=True, pauses=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "limiter": True, "loudness": -20.5, "speed": 0.8, "sample_rate": 8000, "encoding": "ulaw", "pauses": True})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["limiter"], kw["loudness"], kw["speed"], kw["sample_rate"], kw["encoding"]) == (True, -20.5, 0.8, 8000, "ulaw")
        assert kw["pauses"] is not None
        r = c.post("/v1/audio/speech", json={**body, "response_format": "flac", "limiter": True})
        assert r.status_code == 200 and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["limiter"] is True
        assert c.post("/v1/audio/speech", json={**body, "limiter": True, "sample_rate": 11025}).status_code == 400      # no multiple of 10 Hz
        assert c.post("/v1/audio/speech", json={**body, "limiter": False, "sample_rate": 11025}).status_code == 200
        assert c.get("/health").json()["limiter"] is True and c.get("/health").json()["loudness"] is True

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, limiter=True, loudness=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "limiter": True}).status_code == 200 and bat.calls[-1][2] == {"limiter": True}
        assert c.post("/v1/audio/speech", json={**body, "limiter": True, "loudness": -16}).status_code == 200
        assert bat.calls[-1][2] == {"loudness": -16.0, "limiter": True}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

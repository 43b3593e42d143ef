"""Host side of the limiter of streams: the NumPy twin (`limiter.StreamLimiter`) against `limit_segment` of the whole signal, bit for bit
in samples and final record, for every segment of tests/limiter_cases.py at its four rates under every cut of
tests/limiter_stream_cases.py; `stream_plan` and `check_gain_db`; the new symbol in the library, the header and `_lib`; the library's
refusals (no device is touched: every call is refused on its host arguments); the engine's planning; and the default-off plumbing of
Chat, SpeechBatcher and the endpoint on fakes."""
import ctypes as C
import logging
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from chattts_amd import _lib, limiter as LM, statepool as SP
from tests import limiter_cases as LCs, limiter_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chattts_amd.h")
TODAY = "the look-ahead is not carried across chunks"


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", SC.RATES)
def test_the_twin_stream_equals_the_one_shot_twin_under_every_cut(fs):
    W = fs // 100
    seen = set()
    for (name, x, g), (y, rec) in zip(LCs.cases(fs), LCs.twin(fs)):
        assert float(g) <= 2.5 and float(np.abs(x).max()) <= 2 and rec["min_gain"] >= LM.R_MIN      # inside THE CONDITION: equality is exact
        for cut, sizes in SC.cuts(fs).items():
            sizes = SC.schedule(len(x), sizes, fs)
            assert sum(sizes) == len(x)
            tw, out, at = LM.StreamLimiter(fs, g), [], 0
            for k, n in enumerate(sizes):
                final = k == len(sizes) - 1
                p = LM.stream_plan(W, tw.pushed, tw.emitted, n, final)
                out.append(tw.push(x[at: at + n], final))
                assert len(out[-1]) == p["n_out"] and tw.emitted == p["emitted"] and len(tw.carry) == p["carry_out"] <= 4 * W <= LM.CARRY
                if not final:
                    assert tw.emitted == max(0, tw.pushed - 2 * W)                                    # the lag: 2 W samples
                at += n
            assert tw.emitted == tw.pushed == len(x)
            assert np.concatenate(out).tobytes() == y.tobytes(), (fs, name, cut)
            assert tw.stats.tobytes() == rec.tobytes(), (fs, name, cut, tw.stats, rec)
            with pytest.raises(ValueError, match="last push"):
                tw.push(x[:1], False)
            if sizes[-1] == 0:
                seen.add("empty_final")
            if 0 < sizes[-1] < 2 * W and len(sizes) > 1:
                seen.add("short_final")
            if 0 in sizes[:-1]:
                seen.add("empties")
            if len(x) == 1 and len(sizes) > 1:
                seen.add("total_1")
            if 1 < len(x) < 2 * W and sum(n > 0 for n in sizes) > 1:
                seen.add("under_2W")
    assert seen == {"empty_final", "short_final", "empties", "total_1", "under_2W"}
    assert any(r["n_touched"] > 0 for _, r in LCs.twin(fs))


def test_stream_plan_sums_and_refusals():
    rng = np.random.default_rng(4)
    for W in (80, 220, 240, 480):
        for _ in range(40):
            sizes = [int(rng.choice([0, 1, 2 * W - 1, 2 * W, 2 * W + 1, 4 * W, 4 * W + 1, int(rng.integers(0, 6000))])) for _ in range(int(rng.integers(1, 12)))]
            pushed = emitted = 0
            for k, n in enumerate(sizes):
                final = k == len(sizes) - 1
                p = LM.stream_plan(W, pushed, emitted, n, final)
                assert p["total"] == pushed + n and p["e_lo"] == emitted and p["n_out"] == p["emitted"] - emitted >= 0
                assert p["carry_in"] == min(pushed, 4 * W) and p["carry_out"] == (0 if final else min(p["total"], 4 * W)) <= LM.CARRY
                assert p["emitted"] == (p["total"] if final else max(0, p["total"] - 2 * W))
                # sample e_lo needs r from e_lo - 2 W on: inside the carry, or before sample 0
                assert max(0, emitted - 2 * W) >= pushed - p["carry_in"]
                pushed, emitted = p["total"], p["emitted"]
            assert emitted == pushed == sum(sizes)                       # after the final push everything is out
    assert LM.CARRY == 4 * 480
    assert LM.stream_plan(240, 0, 0, 0, True)["n_out"] == 0             # a stream may end empty
    for args, why in [((240, -1, 0, 1, False), "negative"), ((240, 0, 0, -1, False), "negative"), ((240, 1000, 5, 10, False), "has emitted"),
                      ((240, 0, 0, 1 << 31, False), "2\\^31"), ((79, 0, 0, 1, False), "80 .. 480"), ((481, 0, 0, 1, False), "80 .. 480")]:
        with pytest.raises(ValueError, match=why):
            LM.stream_plan(*args)


def test_check_gain_db_is_the_one_rule():
    assert LM.check_gain_db(None) is None
    for v in (0, -30, 30, 6.5, np.float32(-3), np.int64(12)):
        g = LM.check_gain_db(v)
        assert g.dtype == np.float32 and g == np.float32(10.0 ** (float(v) / 20.0))
    assert LM.check_gain_db(0) == np.float32(1)
    for v in (30.001, -30.5, float("nan"), float("inf"), "6", True, [3.0], 3 + 0j):
        with pytest.raises(ValueError, match="finite number of dB in -30 .. \\+30"):
            LM.check_gain_db(v)
    with pytest.raises(ValueError, match="submit_stream: the make-up gain"):
        LM.check_gain_db(40, "submit_stream")


# ---- the symbol -------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_is_exported_declared_and_bound_and_the_layouts_agree():
    lib = _lib.lib()
    with open(HEADER) as f:
        header = f.read()
    name = "ctts_peak_limit_stream_step"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == 11
    assert _lib.LM_STREAM.itemsize == 80 and "} ctts_lm_stream;" in header and re.search(r"#define CTTS_LM_CARRY 1920\b", header)
    assert _lib.LM_STREAM.names == ("in_off", "n_in", "pos", "total", "e_lo", "n_out", "out_off", "slot", "phase", "c_in", "c_out", "rate", "gain")
    struct = header[header.index("#define CTTS_LM_CARRY"): header.index("} ctts_lm_stream;")]
    fields = [n for line in struct.splitlines() if line.strip().startswith(("int64_t", "int32_t", "float"))
              for n in re.sub(r"/\*.*", "", line).replace("int64_t", "").replace("int32_t", "").replace("float", "").replace(";", "").replace(" ", "").split(",")]
    assert tuple(fields) == _lib.LM_STREAM.names
    assert [_lib.LM_STREAM.fields[n][1] for n in ("slot", "rate", "gain")] == [56, 72, 76] and _lib.LM_STREAM["gain"] == np.dtype("<f4")
    with open(os.path.join(ROOT, "chattts_amd", "csrc", "kernels.hpp")) as f:
        assert re.search(r"#define LM_CARRY \(4 \* LM_WMAX\)", f.read())
    assert LM.STATS.itemsize == 16


# ---- the library's refusals -------------------------------------------------------------------------------------------------------------
def _desc(fs, pushed, n_in, final, slot=0, phase=0, gain=1.5, **over):
    W = fs // 100
    p = LM.stream_plan(W, pushed, max(0, pushed - 2 * W), n_in, final)
    row = dict(in_off=0, n_in=n_in, pos=pushed, total=p["total"] if final else -1, e_lo=p["e_lo"], n_out=p["n_out"], out_off=0, slot=slot,
               phase=phase, c_in=p["carry_in"], c_out=p["carry_out"], rate=fs, gain=gain)
    row.update(over)
    return row


def test_library_refuses_before_it_launches():
    """ctts_peak_limit_stream_step checks the host mirror first: these calls fail on a machine without a GPU, each with its reason"""
    lib = _lib.lib()
    X, Y = 1 << 24, 1 << 28            # never dereferenced: every call below is refused on its host arguments

    def call(rows, n_x=1 << 20, n_y=1 << 20, n_slots=4, null=(), y=Y):
        tab = np.zeros(len(rows), _lib.LM_STREAM)
        for i, r in enumerate(rows):
            tab[i] = tuple(r[k] for k in _lib.LM_STREAM.names)
        p = {k: (None if k in null else C.c_void_p(v)) for k, v in (("x", X), ("dev", 4096), ("y", y), ("carry", 8192), ("stats", 12288))}
        rc = lib.ctts_peak_limit_stream_step(p["x"], n_x, p["dev"], tab.ctypes.data_as(C.c_void_p), len(rows), p["y"], n_y, p["carry"], p["stats"],
                                             n_slots, None)
        return rc, lib.ctts_last_error().decode()

    good = lambda **o: {**_desc(24000, 3000, 5000, False), **o}
    g = good()
    assert g["n_out"] == 5000 and g["e_lo"] == 2520 and g["c_in"] == g["c_out"] == 960
    cases = [
        (dict(rows=[good()], null=("carry",)), "null"), (dict(rows=[good()], null=("dev",)), "null"), (dict(rows=[good()], null=("stats",)), "null"),
        (dict(rows=[good()], null=("x",)), "null"), (dict(rows=[good()], null=("y",)), "null"),
        (dict(rows=[good()] * 1025), "n_streams"), (dict(rows=[]), "n_streams"), (dict(rows=[good()], n_slots=0), "no slot"),
        (dict(rows=[good(n_in=-1)]), "negative"), (dict(rows=[good(pos=-1)]), "negative"), (dict(rows=[good(out_off=-8)]), "negative"),
        (dict(rows=[good(n_out=-1)]), "negative"), (dict(rows=[good(n_in=1 << 31)]), "2^31"),
        (dict(rows=[good()], n_x=4999), "outside the input"), (dict(rows=[good(in_off=1)], n_x=5000), "outside the input"),
        (dict(rows=[good()], n_y=4999), "outside the output"), (dict(rows=[good(out_off=8)], n_y=5007), "outside the output"),
        (dict(rows=[good()], y=X + 4 * 100), "must not overlap"), (dict(rows=[good()], y=X), "must not overlap"),
        (dict(rows=[good(rate=7990)]), "multiple of 10 Hz"), (dict(rows=[good(rate=48010)]), "multiple of 10 Hz"), (dict(rows=[good(rate=22055)]), "multiple of 10 Hz"),
        (dict(rows=[good(gain=0.0)]), "pre-gain"), (dict(rows=[good(gain=-1.0)]), "pre-gain"), (dict(rows=[good(gain=np.inf)]), "pre-gain"),
        (dict(rows=[good(gain=np.nan)]), "pre-gain"),
        (dict(rows=[good(slot=4)]), "outside the pool"), (dict(rows=[good(slot=-1)]), "outside the pool"), (dict(rows=[good(), good(slot=1), good()]), "twice"),
        (dict(rows=[good(phase=2)]), "phase"),
        (dict(rows=[good(c_in=959)]), "carries"), (dict(rows=[good(c_out=961)]), "carries"), (dict(rows=[good(c_out=LM.CARRY + 1)]), "carries"),
        (dict(rows=[{**_desc(24000, 100, 50, False), "c_in": 960}]), "carries"), (dict(rows=[{**_desc(24000, 3000, 10, True), "c_out": 960}]), "carries"),
        (dict(rows=[good(e_lo=0)]), "have emitted"), (dict(rows=[good(e_lo=2521)]), "have emitted"),
        (dict(rows=[good(n_out=4999)]), "emits"), (dict(rows=[good(n_out=0)]), "emits"), (dict(rows=[{**_desc(24000, 3000, 10, True), "n_out": 10}]), "emits"),
        (dict(rows=[good(total=8001)]), "last push"), (dict(rows=[good(total=-2)]), "last push"),
    ]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_peak_limit_stream_step" in msg and why in msg, (kw.keys(), why, msg)


# ---- the engine's planning, without a device --------------------------------------------------------------------------------------------
def _engine():
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    eng._pools = {"limiter": SP.StatePool("limiter", 4)}
    return eng


def test_the_engine_plans_a_step_and_commits_nothing_on_its_own():
    eng = _engine()
    a, b = eng.peak_limit_stream_open(8000, 2.0), eng.peak_limit_stream_open(48000)
    assert (a, b) == (0, 1) and eng.peak_limit_streams_in_use() == 2
    tab, commit = eng._lm_descriptors([(a, 0, 1000, False), (b, 1000, 500, True)])
    assert [int(v) for v in tab["n_out"]] == [840, 500] and [int(v) for v in tab["total"]] == [-1, 500] and [int(v) for v in tab["c_out"]] == [320, 0]
    assert [int(v) for v in tab["rate"]] == [8000, 48000] and [float(v) for v in tab["gain"]] == [2.0, 1.0] and [int(v) for v in tab["slot"]] == [a, b]
    assert eng._pools["limiter"].records[a] == SP.LimiterRec(8000, np.float32(2.0), 0, 0, 0, False)                 # nothing committed yet
    assert commit[a] == SP.LimiterRec(8000, np.float32(2.0), 1000, 840, 1, False) and commit[b] == SP.LimiterRec(48000, np.float32(1.0), 500, 500, 1, True)
    assert eng.peak_limit_stream_plan(a, 1000, False)["n_out"] == 840
    st = eng.peak_limit_stream_stats(a)                                                          # before the first push: nothing counted, no device read
    assert (st["g32"], st["min_gain"], st["n_over"], st["n_touched"]) == (np.float32(2.0), 1.0, 0, 0)
    with pytest.raises(ValueError, match="twice"):
        eng._lm_descriptors([(a, 0, 10, False), (a, 10, 10, False)])
    with pytest.raises(ValueError, match="not open"):
        eng._lm_descriptors([(3, 0, 10, False)])
    for rate, gain, why in [(7000, 1.0, "rate"), (24000, 0.0, "pre-gain"), (24000, float("inf"), "pre-gain"), (24005, 1.0, "rate")]:
        with pytest.raises(ValueError, match=why):
            eng.peak_limit_stream_open(rate, gain)
    eng._pools["limiter"].commit({b: eng._pools["limiter"].get(b)._replace(done=True)})
    with pytest.raises(ValueError, match="last push"):
        eng.peak_limit_stream_plan(b, 1, False)
    eng.peak_limit_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.peak_limit_stream_close(a)
    assert eng.peak_limit_stream_open(22050, 100.0) == a and eng.peak_limit_streams_in_use() == 2     # the engine-level gain is not the public range


def test_decode_windows_checks_the_limiter_streams_before_anything_else():
    eng = _engine()
    wins = [(0, 40, 0, 12000), (1, 40, 0, 12000, True)]
    h24, h8 = eng.peak_limit_stream_open(24000), eng.peak_limit_stream_open(8000)
    for kw, why in [(dict(limiter=[True], lm_streams=[h24, None]), "one limiter flag and one lm_streams entry per window"),
                    (dict(limiter=[True, False]), "one limiter flag and one lm_streams entry per window"),
                    (dict(limiter=[True, False], lm_streams=[None, None]), "needs an open limiter stream at 24000 Hz"),
                    (dict(limiter=[True, False], lm_streams=[h8, None]), "needs an open limiter stream at 24000 Hz"),
                    (dict(limiter=[True, False], lm_streams=[h24, None], sample_rates=[8000, 24000]), "needs an open limiter stream at 8000 Hz"),
                    (dict(limiter=[False, True], lm_streams=[h24, h24]), "no limiter flag but names"),
                    (dict(limiter=[False, False], lm_streams=[h24, None]), "lm_streams without a limiter flag"),
                    (dict(lm_streams=[None, h24]), "lm_streams without a limiter flag"),
                    (dict(limiter=[1, False], lm_streams=[h24, None]), "switched by True or False")]:
        with pytest.raises(ValueError, match=why):
            eng.decode_windows(None, wins, **kw)
    with pytest.raises(ValueError, match="has had its last push"):                              # a tail, then another window of the stream
        eng.decode_windows(None, [wins[1], wins[0]], limiter=[True, True], lm_streams=[h24, h24])
    assert eng._pools["limiter"].records[h24] == SP.LimiterRec(24000, np.float32(1.0), 0, 0, 0, False)


# ---- the default-off plumbing, on fakes -------------------------------------------------------------------------------------------------
def test_chat_infer_takes_the_limited_stream_when_opted_in_and_keeps_todays_refusal_otherwise():
    from tests.test_resample_stream_host import _bare_chat
    chat = _bare_chat()
    with pytest.raises(ValueError, match="limiter applies to non-streamed inference only \\(" + TODAY + "\\)"):
        chat.infer(["hello"], stream=True, limiter=True, split_text=False)
    assert not chat.calls
    chat.infer(["hello"], stream=True, limiter=True, stream_limiter=True, split_text=False)
    (a, kw), = chat.calls
    assert a[1] is True and kw["lm_gain"] == np.float32(1.0) and "limiter" not in kw
    chat.infer(["hello"], stream=True, limiter=True, stream_limiter=True, gain_db=6.0, split_text=False, sample_rate=8000, stream_resample=True,
               pcm16=True, encoding="ulaw")
    kw = chat.calls[-1][1]
    assert kw["lm_gain"] == LM.check_gain_db(6.0) and kw["sample_rate"] == 8000 and kw["encoding"] == "ulaw"
    on = dict(stream=True, limiter=True, stream_limiter=True)
    for extra, why in [(dict(split_text=True), "split_text"), (dict(split_text=False, use_decoder=False), "use_decoder=True"),
                       (dict(split_text=False, limiter=[True]), "one limiter flag for the whole batch"),
                       (dict(split_text=False, gain_db=[3.0]), "one make-up gain for the whole batch"),
                       (dict(split_text=False, gain_db=31), "-30 .. \\+30"), (dict(split_text=False, gain_db="loud"), "-30 .. \\+30"),
                       (dict(split_text=False, sample_rate=7000, stream_resample=True), "rate")]:
        with pytest.raises(ValueError, match=why):
            chat.infer(["hello"], **{**on, **extra})
    with pytest.raises(ValueError, match="needs limiter=True"):
        chat.infer(["hello"], stream=True, stream_limiter=True, gain_db=3.0, split_text=False)
    with pytest.raises(ValueError, match="limited stream only"):                                # a non-streamed call has `loudness`
        chat.infer(["hello"], limiter=True, gain_db=3.0)
    n = len(chat.calls)
    chat.infer(["hello"], stream=True, stream_limiter=True, split_text=False)                   # the switch alone changes nothing
    assert len(chat.calls) == n + 1 and "lm_gain" not in chat.calls[-1][1]
    chat.infer(["hello"], limiter=True, stream_limiter=True, split_text=False)                  # a non-streamed call is today's
    assert chat.calls[-1][1]["limiter"] is True and "lm_gain" not in chat.calls[-1][1]


class _LmCodec:
    """the part of CodecEngine the limited streams touch, recorded"""
    SAMPLE_RATE = 24000

    def __init__(self):
        self.log, self.free = [], [23, 22, 21, 20]

    def peak_limit_stream_open(self, rate, gain=1.0):
        self.log.append(("lm_open", rate, float(gain)))
        return self.free.pop()

    def peak_limit_stream_close(self, h):
        self.log.append(("lm_close", h))
        self.free.append(h)

    def decode_window(self, hiddens, a, b, sample_rate=None):
        import torch
        self.log.append(("window", a, b, sample_rate))
        return torch.arange(len(hiddens) * (b - a), dtype=torch.float32).view(len(hiddens), b - a)

    def peak_limit_stream_step(self, x, pushes):
        self.log.append(("lm_step", [tuple(p) for p in pushes]))
        B = len(pushes)
        import torch
        return torch.zeros(B * 60), np.arange(B + 1, dtype=np.int64) * 60

    def to_host(self, t):
        return t.numpy()


def test_the_serial_stream_steps_the_rows_limiter_streams_and_closes_them():
    import torch
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.codec, chat.device, chat.incremental_stream = _LmCodec(), torch.device("cpu"), True
    hid = [torch.zeros((10, 768)), torch.zeros((10, 768))]
    piece = chat._stream_piece(hid, 0, 3000, lm_handles=[20, 21])
    assert piece.shape == (2, 60) and piece.dtype == np.float32
    assert chat.codec.log == [("window", 0, 3000, None), ("lm_step", [(20, 0, 3000, False), (21, 3000, 3000, False)])]
    chat.codec.log.clear()
    piece = chat._stream_piece(hid, 256 * 19, None, rate=8000, lm_handles=[20, 21], final=True)      # nothing left: the streams are stepped all the same
    assert piece.shape == (2, 60) and chat.codec.log == [("lm_step", [(20, 0, 0, True), (21, 0, 0, True)])]
    chat.codec.log.clear()
    chat.has_loaded = lambda use_decoder=True: True
    chat.normalizer = lambda t, *a: t
    seen = {}

    def batches(text, step, stream, use_decoder, split_text, params, pcm16, ragged, raw, sample_rate, encoding, speed, sets, lm_gain=None):
        from chattts_amd.winchain import StreamSet
        seen.update(sets=sets, gain=lm_gain)
        sets.extend(StreamSet.open(chat.codec, rate=sample_rate, speed=speed, limiter_gain=lm_gain) for _ in text)
        yield "chunk"
        raise RuntimeError("the consumer's problem")
    chat._infer_batches = batches
    gen = chat._infer(["a", "b"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None), sample_rate=8000,
                      lm_gain=np.float32(2.0))
    assert next(gen) == "chunk" and [dict(st) for st in seen["sets"]] == [{"limiter": 20}, {"limiter": 21}] and seen["gain"] == np.float32(2.0)      # no other stream
    with pytest.raises(RuntimeError):
        next(gen)
    assert chat.codec.log == [("lm_open", 8000, 2.0), ("lm_open", 8000, 2.0), ("lm_close", 20), ("lm_close", 21)]
    chat._infer_batches = lambda *a, **kw: iter([kw])
    assert next(chat._infer(["a"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None))) == {}   # today's call


def _limited_chat():
    from tests.test_resample_stream_host import _RsCodec
    from tests.test_stream_pool_host import _FakeChat, _piece

    class _Codec(_RsCodec, _LmCodec):
        def __init__(self):
            _RsCodec.__init__(self)
            self.free = [23, 22, 21, 20]

    class _Chat(_FakeChat):
        def __init__(self):
            super().__init__()
            self.codec, self.kw_calls = _Codec(), []

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            return [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]
    return _Chat()


def test_submit_stream_takes_the_limiter_when_opted_in_and_gives_the_stream_back():
    from chattts_amd.serving import SpeechBatcher
    from tests.test_resample_stream_host import _wait
    from tests.test_stream_pool_host import _FakePool, _Params
    lock, holder = threading.Lock(), {}
    chat = _limited_chat()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_limiter=True)
    try:
        for kw, why in [(dict(limiter=True, gain_db=31), "-30 .. \\+30"), (dict(gain_db=3.0), "needs limiter=True"), (dict(limiter=1), "True or False"),
                        (dict(limiter=True, sample_rate=7000), "rate")]:
            with pytest.raises(ValueError, match=why):
                b.submit_stream("x", _Params(48), **kw)
        with lock:
            streams = [b.submit_stream("A", _Params(96), limiter=True, gain_db=6.0, sample_rate=8000, encoding="ulaw"), b.submit_stream("B", _Params(96)),
                       b.submit_stream("C", _Params(96), limiter=True)]
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in enumerate(streams)]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        assert all(len(got[k]) > 0 for k in range(3))
        full = [(w, kw) for w, kw in zip(chat.window_calls, chat.kw_calls) if len(w) == 3]
        assert full
        for w, kw in full:
            by = {x[0]: k for k, x in enumerate(w)}
            assert set(kw) == {"sample_rates", "encodings", "limiter", "lm_streams"}, kw
            assert [kw["limiter"][by[k]] for k in range(3)] == [True, False, True]
            assert kw["lm_streams"][by[0]] == 20 and kw["lm_streams"][by[1]] is None and kw["lm_streams"][by[2]] == 21
        _wait(lambda: sum(e[0] == "lm_close" for e in chat.codec.log) == 2)
        opens = [e for e in chat.codec.log if e[0] == "lm_open"]
        assert opens == [("lm_open", 8000, float(LM.check_gain_db(6.0))), ("lm_open", 24000, 1.0)]
        s = b.submit_stream("D", _Params(400), limiter=True)                       # a cancelled one gives its stream back too
        assert len(next(s)) > 0
        s.close()
        _wait(lambda: sum(e[0] == "lm_close" for e in chat.codec.log) == 3)
        n = len(chat.kw_calls)
        assert len(list(b.submit_stream("E", _Params(48)))) > 0                    # without the flag: the call before this option
        assert all("limiter" not in kw and "lm_streams" not in kw for kw in chat.kw_calls[n:])
        assert b.occupancy()["stream_limited_chunks"] > 0
    finally:
        b.close()
    off = SpeechBatcher(_limited_chat(), 2, lock, make_pool=lambda: _FakePool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="limiter applies to non-streamed requests only \\(" + TODAY + "\\)"):
            off.submit_stream("x", _Params(48), limiter=True)
        assert "stream_limited_chunks" not in off.occupancy()
    finally:
        off.close()
    assert not lock.locked()


def test_the_endpoint_serves_a_limited_stream_when_switched_on_and_is_todays_otherwise(caplog):
    from starlette.testclient import TestClient
    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    from tests.test_stream_resample_host import _StreamBatcher
    body = {"input": "hello", "response_format": "pcm", "stream": True, "limiter": True}

    def app(chat, **kw):
        return TestClient(server.create_app(chat, {"default": "SPK-D"}, logger=logging.getLogger("test_limiter_stream_host"), **kw))

    chat = _EndpointChat()
    with app(chat, limiter=True) as c:                                    # today: the 400 with its text; gain_db is an unknown key
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "limiter is served for non-streamed requests only" in r.text and TODAY in r.text and not chat.calls
        with caplog.at_level(logging.WARNING, logger="test_limiter_stream_host"):
            assert c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "gain_db": 99}).status_code == 200
        assert "gain_db" in caplog.text and "unsupported parameters" in caplog.text and "gain_db" not in chat.calls[-1][2]
        assert "stream_limiter" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, stream_limiter=True) as c:                             # without `limiter` the switch does nothing
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "limiter" not in chat.calls[-1][2]
        assert "stream_limiter" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, limiter=True, stream_limiter=True, g711=True, stream_sample_rates=(8000,)) as c:       # served, serially here
        r = c.post("/v1/audio/speech", json=body)
        text, stream, kw = chat.calls[-1]
        assert r.status_code == 200 and stream and (kw["limiter"], kw["stream_limiter"], kw["split_text"]) == (True, True, False) and "gain_db" not in kw
        r = c.post("/v1/audio/speech", json={**body, "gain_db": -4.5, "response_format": "ulaw", "sample_rate": 8000})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["gain_db"], kw["encoding"], kw["sample_rate"], kw["stream_resample"], kw["stream_limiter"]) == (-4.5, "ulaw", 8000, True, True)
        n = len(chat.calls)
        for bad in ({**body, "gain_db": 30.5}, {**body, "gain_db": "6"}, {**body, "gain_db": True}, {**body, "limiter": False, "gain_db": 3},
                    {"input": "hello", "response_format": "pcm", "gain_db": 3}, {"input": "hello", "response_format": "pcm", "limiter": True, "gain_db": 3},
                    {**body, "limiter": "yes"}):
            assert c.post("/v1/audio/speech", json=bad).status_code == 400, bad
        assert len(chat.calls) == n
        assert c.post("/v1/audio/speech", json={**body, "limiter": False}).status_code == 200 and "stream_limiter" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "limiter": True}).status_code == 200
        assert chat.calls[-1][1] is False and chat.calls[-1][2]["limiter"] is True and "stream_limiter" not in chat.calls[-1][2]
        assert c.get("/health").json()["stream_limiter"] is True
    chat, bat = _EndpointChat(), _StreamBatcher()                        # through the pool when the pool can take it
    bat.stream_limiter = True
    with app(chat, batcher=bat, batch_streams=True, limiter=True, stream_limiter=True) as c:
        r = c.post("/v1/audio/speech", json={**body, "gain_db": 6})
        assert r.status_code == 200 and bat.calls[-1] == ("hello", {"limiter": True, "gain_db": 6.0}) and not chat.calls
        r = c.post("/v1/audio/speech", json={k: v for k, v in body.items() if k != "limiter"})
        assert r.status_code == 200 and bat.calls[-1] == ("hello", {})
    chat, bat = _EndpointChat(), _StreamBatcher()                        # a pool built without stream_limiter: served serially
    with app(chat, batcher=bat, batch_streams=True, limiter=True, stream_limiter=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and not bat.calls and chat.calls[-1][2]["stream_limiter"] is True

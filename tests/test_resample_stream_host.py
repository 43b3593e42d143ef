"""Host side of the streamed resampler: `resample.stream_plan` over random push schedules at seven rate pairs (what a step emits, what
it reads, what it keeps), the new symbols in the library, the header and `_lib.SIGNATURES`, the library's refusals (no device is
touched: every call is refused on its host arguments), the engine's descriptor planning, and the default-off plumbing on fakes."""
import ctypes as C
import logging
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from chattts_amd import _lib, resample as RS, statepool as SP

ORIG = 24000
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
WORST = {8000: 40, 11025: 347, 16000: 22, 22050: 173, 32000: 16, 44100: 93, 48000: 14}       # K - 1 of each pair
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chattts_amd.h")
NEW_SYMBOLS = ("ctts_resample_stream_step", "ctts_codec_windows_speed_rate_workspace_bytes", "ctts_codec_decode_windows_speed_rate")


def geometry(new, orig=ORIG):
    L, M = RS.ratio(orig, new)
    width, K = RS.geometry(L, M)
    return L, M, K, width


def walk(L, M, K, sizes):
    """the plans of a stream pushed in `sizes`, the last push final"""
    pushed = emitted = 0
    plans = []
    for i, n in enumerate(sizes):
        p = RS.stream_plan(L, M, K, pushed, emitted, n, i == len(sizes) - 1)
        plans.append((pushed, n, p))
        pushed, emitted = pushed + n, p["emitted"]
    return plans


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def test_the_constants_and_the_descriptor():
    assert RS.CARRY == 512 and _lib.RS_STREAM.itemsize == 80
    assert _lib.RS_STREAM.names == ("in_off", "n_in", "pos", "total", "o_lo", "n_out", "out_off", "slot", "phase", "c_in", "c_out", "pad", "reserved")
    assert {new: geometry(new)[2] - 1 for new in RATES} == WORST and max(WORST.values()) <= RS.CARRY
    with open(os.path.join(os.path.dirname(HEADER), "..", "chattts_amd", "csrc", "kernels.hpp")) as f:
        assert re.search(r"#define RS_CARRY 512\b", f.read())
    with open(HEADER) as f:
        assert re.search(r"#define CTTS_RS_CARRY 512\b", f.read())


@pytest.mark.parametrize("new", RATES)
def test_random_schedules_tile_the_output_read_only_what_is_kept_and_stay_under_the_carry(new):
    L, M, K, width = geometry(new)
    rng = np.random.default_rng(new)
    worst = 0
    for trial in range(40):
        sizes = [int(rng.choice([0, 1, 511, 512, 513, int(rng.integers(0, 3 * K + 1))])) for _ in range(int(rng.integers(1, 60)))]
        if sum(sizes) == 0:
            sizes.append(1)
        if trial % 2:
            sizes.append(0)                                # an empty last push
        emitted = 0
        for pushed, n, p in walk(L, M, K, sizes):
            end = pushed + n
            assert p["o_lo"] == emitted and p["n_out"] >= 0 and p["emitted"] == emitted + p["n_out"]        # `emitted` never decreases
            c = pushed - p["carry_in"]
            assert c == max(0, (emitted // L) * M - width)
            if p["n_out"]:
                # outputs [o_lo, E') read inputs [(o_lo // L) M - width, ((E' - 1) // L) M + width + M): inside [c, P'), or outside the signal
                lo, hi = (emitted // L) * M - width, ((p["emitted"] - 1) // L) * M + width + M
                assert max(lo, 0) >= c, (new, sizes)
                if p["total"] < 0:
                    assert hi <= end, (new, sizes)
            if p["total"] < 0:
                J = (end - width - M) // M + 1 if end >= width + M else 0
                assert p["emitted"] == J * L
                assert 0 <= p["carry_out"] <= K - 1 and end - p["carry_out"] == max(0, J * M - width)
                assert end - p["carry_out"] >= c                         # a carry never reaches back beyond the one before it
                worst = max(worst, p["carry_out"])
            else:
                assert p["carry_out"] == 0 and p["total"] == end and p["emitted"] == RS.out_len(end, L, M)
            emitted = p["emitted"]
        assert emitted == RS.out_len(sum(sizes), L, M)
    print(f"{ORIG} -> {new}: worst carry {worst} (K - 1 = {K - 1})")
    assert worst <= K - 1


@pytest.mark.parametrize("new", RATES)
def test_one_sample_pushes_reach_the_bound_exactly(new):
    L, M, K, width = geometry(new)
    plans = walk(L, M, K, [1] * (4 * K))
    assert max(p["carry_out"] for _, _, p in plans[:-1]) == K - 1 == WORST[new]
    assert sum(p["n_out"] for _, _, p in plans) == RS.out_len(4 * K, L, M)


def test_stream_plan_refusals():
    L, M, K, _ = geometry(8000)
    with pytest.raises(ValueError, match="negative"):
        RS.stream_plan(L, M, K, -1, 0, 10, False)
    with pytest.raises(ValueError, match="negative"):
        RS.stream_plan(L, M, K, 0, 0, -1, False)
    with pytest.raises(ValueError, match="has emitted"):
        RS.stream_plan(L, M, K, 3000, 5, 10, False)
    with pytest.raises(ValueError, match="empty stream"):
        RS.stream_plan(L, M, K, 0, 0, 0, True)
    with pytest.raises(ValueError, match="2\\^31"):
        RS.stream_plan(L, M, K, 0, 0, 1 << 31, False)
    with pytest.raises(ValueError, match="no table"):
        RS.stream_plan(L, M, K + 1, 0, 0, 10, False)
    L2, M2, K2, _ = geometry(11025, 48000)                    # K = 694: supported by the one-shot kernel, beyond a stream's carry
    assert RS.mode(L2, M2, K2) == 1 and K2 - 1 > RS.CARRY
    with pytest.raises(ValueError, match="exceeds the 512"):
        RS.stream_plan(L2, M2, K2, 0, 0, 600, False)
    assert RS.stream_plan(L, M, K, 0, 0, 0, False)["n_out"] == 0


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_declared_and_bound():
    lib = _lib.lib()
    with open(HEADER) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "ctts_rs_stream;" in header and "/* 80 bytes */" in header
    assert lib.ctts_codec_windows_speed_rate_workspace_bytes(2, 40, 4096) == lib.ctts_codec_windows_speed_workspace_bytes(2, 40, 4096) > 0


# ---- the library's refusals ---------------------------------------------------------------------------------------------------------
def _desc(new, pushed, n_in, final, slot=0, phase=0, orig=ORIG, **over):
    L, M, K, width = geometry(new, orig)
    emitted = RS.frames_final(pushed, M, width) * L
    p = RS.stream_plan(L, M, K, pushed, emitted, n_in, final)
    row = dict(in_off=0, n_in=n_in, pos=pushed, total=p["total"], o_lo=emitted, n_out=p["n_out"], out_off=0, slot=slot, phase=phase,
               c_in=p["carry_in"], c_out=p["carry_out"], pad=0, reserved=0)
    row.update(over)
    return row


def _table(rows):
    tab = np.zeros(len(rows), _lib.RS_STREAM)
    for i, r in enumerate(rows):
        tab[i] = tuple(r[k] for k in _lib.RS_STREAM.names)
    return tab


def test_library_refuses_before_it_launches():
    """ctts_resample_stream_step checks the host mirror first: these calls fail on a machine without a GPU, each with its reason"""
    lib = _lib.lib()
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused on its host arguments
    L, M, K, _ = geometry(8000)

    def call(rows, n_x=1 << 20, n_y=1 << 20, n_slots=4, null=(), pair=(L, M, K)):
        tab = _table(rows)
        p = {k: (None if k in null else fake) for k in ("x", "dev", "y", "carry", "taps")}
        rc = lib.ctts_resample_stream_step(p["x"], n_x, p["dev"], tab.ctypes.data_as(C.c_void_p), len(rows), p["y"], n_y, p["carry"], n_slots,
                                           p["taps"], *pair, None)
        return rc, lib.ctts_last_error().decode()

    good = lambda **o: {**_desc(8000, 3000, 5000, False), **o}
    g = good()
    assert g["n_out"] > 0 and 0 < g["c_in"] <= 40 and 0 < g["c_out"] <= 40
    big = geometry(11025, 48000)[:3]                                                       # K = 694
    cases = [
        (dict(rows=[good()], null=("carry",)), "null"), (dict(rows=[good()], null=("dev",)), "null"), (dict(rows=[good()], null=("x",)), "null"),
        (dict(rows=[good()], null=("y",)), "null"), (dict(rows=[good()], null=("taps",)), "filter table is null"),
        (dict(rows=[good(n_out=g["n_out"] + 1)]), "emits"), (dict(rows=[good(n_out=0)]), "emits"),
        (dict(rows=[good(c_in=g["c_in"] + 1)]), "carries"), (dict(rows=[good(c_in=0)]), "carries"), (dict(rows=[good(c_out=g["c_out"] - 1)]), "carries"),
        (dict(rows=[good(c_out=RS.CARRY + 1)]), "carries"),
        (dict(rows=[dict(good(), n_in=600, pos=0, o_lo=0, n_out=0, c_in=0, c_out=600)], pair=big), "exceeds the 512"),   # 600 < width + M: all kept
        (dict(rows=[good(slot=4)]), "outside the pool"), (dict(rows=[good(slot=-1)]), "outside the pool"),
        (dict(rows=[good(), good(slot=1), good()]), "twice"),
        (dict(rows=[good()], n_y=g["n_out"] - 1), "outside the output"), (dict(rows=[good(out_off=8)], n_y=g["n_out"] + 7), "outside the output"),
        (dict(rows=[good(pad=7)], n_y=g["n_out"] + 6), "outside the output"),
        (dict(rows=[good()], n_x=4999), "outside the input"), (dict(rows=[good(in_off=1)], n_x=5000), "outside the input"),
        (dict(rows=[good()], pair=(L, M, K + 1)), "not supported"), (dict(rows=[good()], pair=(3, 3, 9)), "L != M"),
        (dict(rows=[good(o_lo=g["o_lo"] + 1)]), "have emitted"), (dict(rows=[good(o_lo=0)]), "have emitted"),
        (dict(rows=[good(total=8001)]), "last push"), (dict(rows=[good(total=-2)]), "last push"),
        (dict(rows=[{**_desc(8000, 0, 0, False), "total": 0}]), "last push"),
        (dict(rows=[good(phase=2)]), "phase"), (dict(rows=[good(pad=256)]), "pad"), (dict(rows=[good(pad=-1)]), "pad"),
        (dict(rows=[good(n_in=-1)]), "negative"), (dict(rows=[good(pos=-1)]), "negative"), (dict(rows=[good(out_off=-8)]), "negative"),
        (dict(rows=[good(n_in=1 << 31)]), "2^31"),
        (dict(rows=[]), "n_streams"), (dict(rows=[good()], n_slots=0), "no slot"),
    ]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_resample_stream_step" in msg and why in msg, (kw, msg)


def test_the_window_entry_refuses_bad_resampler_tables_before_any_launch():
    """ctts_codec_decode_windows_speed_rate: the group table and the pair are checked in front of everything else"""
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    rate = (_lib.Rate * 1)()
    rate[0].taps, rate[0].L, rate[0].M, rate[0].K = 4096, 1, 3, 41

    def call(of_ts=i32(0), grp_off=i32(0, 1), grp_rate=i32(0), n_grp=1, rates=rate, n_rates=1, rs_carry=fake, n_rs_slots=4):
        host = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = lib.ctts_codec_decode_windows_speed_rate(
            fake, None, 0, 0, 1, 1, None, None, 0, fake, fake, fake, fake, 1, fake, fake, host(i32(0, 1)), 1, fake, fake, 4, fake,
            fake, fake, host(of_ts), host(grp_off), host(grp_rate), n_grp, None if rates is None else C.cast(rates, C.c_void_p), n_rates,
            rs_carry, n_rs_slots, 1, fake, None, 0, 0.0, fake, 1 << 20, None)
        return rc, lib.ctts_last_error().decode()

    bad = (_lib.Rate * 1)()
    bad[0].taps, bad[0].L, bad[0].M, bad[0].K = 4096, 1, 3, 42
    for kw, why in [(dict(of_ts=None), "null"), (dict(grp_off=None), "null"), (dict(grp_off=i32(1, 2)), "first group at 0"),
                    (dict(n_grp=-1), "n_grp"), (dict(rs_carry=None), "null"), (dict(grp_rate=None), "null"), (dict(n_rs_slots=0), "no slot"),
                    (dict(grp_off=i32(0, 0)), "is empty"), (dict(grp_rate=i32(1)), "names rate 1 of 1"), (dict(rates=bad), "not supported")]:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_codec_decode_windows_speed_rate" in msg and why in msg, (kw, msg)


# ---- the engine's planning, without a device ------------------------------------------------------------------------------------------
def _engine():
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    eng._pools = {"resample": SP.StatePool("resample", 4), "time_scale": SP.StatePool("time_scale", 4)}
    return eng


def test_the_engine_plans_pushes_in_rounds_grouped_by_rate_and_commits_nothing_on_its_own():
    eng = _engine()
    a, b, c = eng.resample_stream_open(ORIG, 8000), eng.resample_stream_open(ORIG, 16000), eng.resample_stream_open(ORIG, 8000)
    assert (a, b, c) == (0, 1, 2) and eng.resample_streams_in_use() == 3
    tab, groups, order, commit = eng._rs_descriptors([(a, 0, 3000, False), (b, 3000, 2000, False), (c, 5000, 10, False), (a, 6000, 0, True)])
    # round 0: the two 8000 Hz streams in one launch, the 16000 Hz one in another; round 1: a's second push
    assert order == [0, 2, 1, 3] and groups == [[0, (ORIG, 8000), 0, 2], [0, (ORIG, 16000), 2, 3], [1, (ORIG, 8000), 3, 4]]
    assert [int(v) for v in tab["slot"]] == [a, c, b, a] and [int(v) for v in tab["pos"]] == [0, 0, 0, 3000]
    assert [int(v) for v in tab["phase"]] == [0, 0, 0, 1] and int(tab["total"][3]) == 3000 and int(tab["total"][0]) == -1
    assert int(tab["o_lo"][3]) == int(tab["n_out"][0]) and int(tab["c_in"][3]) == int(tab["c_out"][0]) > 0
    assert int(tab["n_out"][0]) + int(tab["n_out"][3]) == 1000 and int(tab["n_out"][1]) == 0 and int(tab["c_out"][1]) == 10
    assert eng._pools["resample"].records[a] == SP.ResampleRec(ORIG, 8000, 0, 0, 0, False)                        # nothing committed yet
    assert commit[a] == SP.ResampleRec(ORIG, 8000, 3000, 1000, 0, True) and commit[c] == SP.ResampleRec(ORIG, 8000, 10, 0, 1, False)
    assert eng.resample_stream_plan(a, 3000, False)["n_out"] == int(tab["n_out"][0])
    with pytest.raises(ValueError, match="last push"):
        eng._rs_descriptors([(a, 0, 10, True), (a, 10, 10, False)])
    with pytest.raises(ValueError, match="not open"):
        eng._rs_descriptors([(3, 0, 10, False)])
    eng.resample_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.resample_stream_close(a)
    assert eng.resample_stream_open(ORIG, 48000) == a and eng._pools["resample"].records[a] == SP.ResampleRec(ORIG, 48000, 0, 0, 0, False)
    with pytest.raises(ValueError, match="nothing to convert"):
        eng.resample_stream_open(ORIG, ORIG)
    with pytest.raises(ValueError, match="carry up to 693"):
        eng.resample_stream_open(48000, 11025)
    assert eng.resample_streams_in_use() == 3


def test_decode_windows_keeps_the_refusal_without_rs_streams_and_checks_them_when_given():
    eng = _engine()
    wins = [(0, 40, 0, 12000), (1, 40, 0, 12000)]
    with pytest.raises(ValueError, match="24000 Hz only"):
        eng.decode_windows(None, wins, speeds=[1.25, 1.0], ts_streams=[0, None], sample_rates=[8000, 24000])
    store = SimpleNamespace(dim=lambda: 3, dtype=__import__("torch").float32, is_cuda=True, size=lambda i: (2, 64, 768)[i], stride=lambda i: 1)
    t = eng.time_scale_stream_open(1.25)
    kw = dict(speeds=[1.25, 1.0], ts_streams=[t, None], sample_rates=[8000, 24000])
    with pytest.raises(ValueError, match="one sample rate and one rs_streams entry per window"):
        eng.decode_windows(store, wins, rs_streams=[None], **kw)
    with pytest.raises(ValueError, match="needs an open resampler stream 24000 -> 8000"):
        eng.decode_windows(store, wins, rs_streams=[None, None], **kw)
    r16 = eng.resample_stream_open(ORIG, 16000)
    with pytest.raises(ValueError, match="needs an open resampler stream 24000 -> 8000"):
        eng.decode_windows(store, wins, rs_streams=[r16, None], **kw)
    r8 = eng.resample_stream_open(ORIG, 8000)
    with pytest.raises(ValueError, match="speed 1 but names a stream"):
        eng.decode_windows(store, wins, rs_streams=[r8, r16], **kw)
    with pytest.raises(ValueError, match="stays at 24000 Hz but names a resampler stream"):
        eng.decode_windows(store, wins, speeds=[1.25, 1.25], ts_streams=[t, t], sample_rates=[8000, 24000], rs_streams=[r8, r16])
    assert eng._pools["resample"].records[r8] == SP.ResampleRec(ORIG, 8000, 0, 0, 0, False) and eng._pools["time_scale"].records[t].pushed == 0


# ---- the default-off plumbing, on fakes ---------------------------------------------------------------------------------------------
def _bare_chat():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.context = SimpleNamespace(set=lambda v: None)
    chat.calls = []
    chat._infer = lambda *a, **kw: chat.calls.append((a, kw)) or iter(())
    return chat


def test_chat_infer_routes_the_combination_when_opted_in_and_refuses_it_otherwise():
    chat = _bare_chat()
    base = dict(stream=True, speed=1.25, stream_time_scale=True, sample_rate=8000, stream_resample=True, split_text=False)
    with pytest.raises(ValueError, match="24000 Hz only"):
        chat.infer(["hello"], **base)
    assert not chat.calls
    chat.infer(["hello"], **base, stream_scaled_resample=True)
    (a, kw), = chat.calls
    assert kw["sample_rate"] == 8000 and kw["speed"] == 1.25 and a[1] is True
    with pytest.raises(ValueError, match="non-streamed inference only"):          # the resampled stream's own opt-in is still needed
        chat.infer(["hello"], **{**base, "stream_resample": False}, stream_scaled_resample=True)
    with pytest.raises(ValueError, match="split_text"):
        chat.infer(["hello"], **{**base, "split_text": True}, stream_scaled_resample=True)
    with pytest.raises(ValueError, match="beyond what the kernel supports|carry up to"):
        chat.infer(["hello"], **{**base, "sample_rate": 11023}, stream_scaled_resample=True)
    chat.infer(["hello"], stream=True, speed=1.25, stream_time_scale=True, split_text=False, stream_scaled_resample=True)   # 24 kHz: nothing new
    assert chat.calls[-1][1]["sample_rate"] is None


class _RsCodec:
    """the part of CodecEngine the streamed speed-and-rate path touches, recorded"""
    SAMPLE_RATE = 24000

    def __init__(self):
        self.log, self.free_ts, self.free_rs = [], [3, 2, 1, 0], [13, 12, 11, 10]

    def time_scale_stream_open(self, speed):
        self.log.append(("ts_open", speed))
        return self.free_ts.pop()

    def time_scale_stream_close(self, h):
        self.log.append(("ts_close", h))
        self.free_ts.append(h)

    def resample_stream_open(self, orig, new):
        self.log.append(("rs_open", orig, new))
        return self.free_rs.pop()

    def resample_stream_close(self, h):
        self.log.append(("rs_close", h))
        self.free_rs.append(h)

    def decode_window(self, hiddens, a, b):
        import torch
        return torch.arange(len(hiddens) * (b - a), dtype=torch.float32).view(len(hiddens), b - a)

    def time_scale_stream_step(self, x, pushes):
        self.log.append(("ts_step", [tuple(p) for p in pushes]))
        B = len(pushes)
        return x[: B * 512].clone(), np.arange(B + 1, dtype=np.int64) * 512

    def resample_stream_step(self, y, pushes):
        self.log.append(("rs_step", [tuple(p) for p in pushes]))
        B = len(pushes)
        return y[: B * 100].clone(), np.arange(B + 1, dtype=np.int64) * 100

    def to_host(self, t):
        return t.numpy()


def test_the_serial_stream_takes_the_extra_step_and_closes_both_streams():
    import torch
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.codec, chat.device, chat.incremental_stream = _RsCodec(), torch.device("cpu"), True
    hid = [torch.zeros((10, 768)), torch.zeros((10, 768))]
    piece = chat._stream_piece_scaled(hid, 0, 3000, [0, 1], False, rs_handles=[10, 11])
    assert piece.shape == (2, 100)
    assert chat.codec.log == [("ts_step", [(0, 0, 3000, False), (1, 3000, 3000, False)]), ("rs_step", [(10, 0, 512, False), (11, 512, 512, False)])]
    chat.codec.log.clear()
    assert chat._stream_piece_scaled(hid, 0, 3000, [0, 1], True).shape == (2, 512) and [e[0] for e in chat.codec.log] == ["ts_step"]
    # `_infer`: the rows' streams of both kinds are opened at the first chunk and closed in the same `finally`
    chat.codec.log.clear()
    chat.has_loaded = lambda use_decoder=True: True
    chat.normalizer = lambda t, *a: t
    seen = {}

    def batches(text, step, stream, use_decoder, split_text, params, pcm16, ragged, raw, sample_rate, encoding, speed, sets):
        from chattts_amd.winchain import StreamSet
        seen.update(sets=sets, rate=sample_rate)
        sets.extend(StreamSet.open(chat.codec, rate=sample_rate, speed=speed) for _ in text)
        yield "chunk"
        raise RuntimeError("the consumer's problem")
    chat._infer_batches = batches
    gen = chat._infer(["a", "b"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None), sample_rate=8000, speed=1.25)
    assert next(gen) == "chunk" and [dict(st) for st in seen["sets"]] == [{"time_scale": 0, "resample": 10}, {"time_scale": 1, "resample": 11}]
    with pytest.raises(RuntimeError):
        next(gen)
    assert chat.codec.log[-4:] == [("ts_close", 0), ("rs_close", 10), ("ts_close", 1), ("rs_close", 11)]            # row by row: each row's set
    gen = chat._infer(["a"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None), speed=1.25)
    chat._infer_batches = lambda *a: (a[-1].extend(StreamSet.open(chat.codec, rate=a[9], speed=a[11]) for _ in a[0]), iter([a[-1]]))[1]
    from chattts_amd.winchain import StreamSet
    assert [sorted(st) for st in next(gen)] == [["time_scale"]]       # a streamed speed at 24 kHz: no resampler streams at all


def _speed_rate_chat():
    from tests.test_stream_pool_host import _FakeChat, _piece

    class _Chat(_FakeChat):
        def __init__(self):
            super().__init__()
            self.codec, self.kw_calls = _RsCodec(), []

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            return [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]
    return _Chat()


def _wait(cond, timeout=10.0):
    import time
    t0 = time.monotonic()
    while not cond():
        assert time.monotonic() - t0 < timeout, "the batcher did not get there"
        time.sleep(0.001)


def test_submit_stream_takes_a_speed_with_a_rate_when_opted_in_and_gives_both_streams_back():
    from chattts_amd.serving import SpeechBatcher
    from tests.test_stream_pool_host import _FakePool, _Params
    lock, holder = threading.Lock(), {}
    chat = _speed_rate_chat()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_speeds=True,
                      stream_speed_rates=True)
    try:
        with pytest.raises(ValueError, match="beyond what the kernel supports|carry up to"):
            b.submit_stream("x", _Params(48), speed=1.25, sample_rate=11023)
        with lock:
            streams = [b.submit_stream("A", _Params(96), speed=1.25, sample_rate=8000, encoding="ulaw"), b.submit_stream("B", _Params(96), sample_rate=8000),
                       b.submit_stream("C", _Params(96), speed=0.75)]
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
            assert set(kw) == {"sample_rates", "encodings", "speeds", "ts_streams", "rs_streams"}, kw
            assert kw["rs_streams"][by[0]] == 10 and kw["rs_streams"][by[1]] is None and kw["rs_streams"][by[2]] is None
            assert kw["ts_streams"][by[0]] is not None and kw["ts_streams"][by[1]] is None and kw["ts_streams"][by[2]] is not None
            assert kw["sample_rates"][by[0]] == 8000 and kw["speeds"][by[0]] == 1.25 and kw["encodings"][by[0]] == "ulaw"
        _wait(lambda: sum(e[0] == "ts_close" for e in chat.codec.log) == 2 and ("rs_close", 10) in chat.codec.log)
        assert [e for e in chat.codec.log if e[0] == "rs_open"] == [("rs_open", 24000, 8000)]
        # a cancelled one gives both back too
        s = b.submit_stream("D", _Params(400), speed=1.5, sample_rate=16000)
        assert len(next(s)) > 0 and ("rs_open", 24000, 16000) in chat.codec.log
        n_close = sum(e[0] == "rs_close" for e in chat.codec.log)
        s.close()
        _wait(lambda: sum(e[0] == "rs_close" for e in chat.codec.log) == n_close + 1)
        # a speed at 24 kHz passes no rs_streams: the call is the one before this option
        n_calls = len(chat.kw_calls)
        assert len(list(b.submit_stream("E", _Params(48), speed=1.25))) > 0
        assert all("rs_streams" not in kw for kw in chat.kw_calls[n_calls:])
    finally:
        b.close()
    off = SpeechBatcher(_speed_rate_chat(), 2, lock, make_pool=lambda: _FakePool(2, lock), streams=True, stream_speeds=True)
    try:
        with pytest.raises(ValueError, match="24000 Hz only"):
            off.submit_stream("x", _Params(48), speed=1.25, sample_rate=8000)
    finally:
        off.close()
    assert not lock.locked()


def test_endpoint_serves_a_streamed_speed_at_a_listed_rate_when_opted_in():
    from starlette.testclient import TestClient
    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    from tests.test_stream_resample_host import _StreamBatcher
    body = {"input": "hello", "response_format": "wav", "stream": True, "speed": 1.25, "sample_rate": 8000}

    def app(chat, **kw):
        return TestClient(server.create_app(chat, {"default": "SPK-D"}, logger=logging.getLogger("test_resample_stream_host"), **kw))

    on = dict(speed=True, stream_speed=True, stream_sample_rates=(8000,))
    chat = _EndpointChat()
    with app(chat, **on) as c:                                            # today: the 400, with its text
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "24000 Hz only" in r.text and "look-ahead" in r.text and not chat.calls
    chat = _EndpointChat()
    with app(chat, **on, stream_speed_rates=True, g711=True) as c:        # opted in: served, serially here
        r = c.post("/v1/audio/speech", json=body)
        text, stream, kw = chat.calls[-1]
        assert r.status_code == 200 and stream and r.content[:44] == server.wav_stream_header(8000)
        assert (kw["speed"], kw["sample_rate"], kw["stream_time_scale"], kw["stream_resample"], kw["stream_scaled_resample"], kw["split_text"]) == \
            (1.25, 8000, True, True, True, False)
        r = c.post("/v1/audio/speech", json={**body, "response_format": "ulaw"})
        assert r.status_code == 200 and chat.calls[-1][2]["encoding"] == "ulaw" and chat.calls[-1][2]["stream_scaled_resample"] is True
        assert c.post("/v1/audio/speech", json={**body, "sample_rate": 16000}).status_code == 400           # not a listed rate
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.0}).status_code == 200
        assert "stream_scaled_resample" not in chat.calls[-1][2] and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={k: v for k, v in body.items() if k != "sample_rate"}).status_code == 200
        assert "stream_scaled_resample" not in chat.calls[-1][2] and chat.calls[-1][2]["stream_time_scale"] is True
    chat = _EndpointChat()
    with app(chat, speed=True, stream_sample_rates=(8000,), stream_speed_rates=True) as c:      # without stream_speed the flag does nothing
        assert c.post("/v1/audio/speech", json=body).status_code == 400 and not chat.calls
    chat, bat = _EndpointChat(), _StreamBatcher()                        # through the pool when the pool can take it
    bat.stream_speeds = bat.stream_speed_rates = True
    with app(chat, batcher=bat, batch_streams=True, **on, stream_speed_rates=True, g711=True) as c:
        r = c.post("/v1/audio/speech", json={**body, "response_format": "ulaw"})
        assert r.status_code == 200 and bat.calls[-1] == ("hello", {"sample_rate": 8000, "speed": 1.25, "encoding": "ulaw"}) and not chat.calls
    chat, bat = _EndpointChat(), _StreamBatcher()                        # a pool built without stream_speed_rates: served serially
    bat.stream_speeds = True
    with app(chat, batcher=bat, batch_streams=True, **on, stream_speed_rates=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and not bat.calls and chat.calls[-1][2]["stream_scaled_resample"] is True
        r = c.post("/v1/audio/speech", json={k: v for k, v in body.items() if k != "sample_rate"})      # at 24 kHz the pool still takes it
        assert r.status_code == 200 and bat.calls[-1] == ("hello", {"speed": 1.25})

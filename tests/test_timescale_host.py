"""Host side of the device time scaler: the speed, lengths and frame counts at the edges, `plan`'s refusals and the library's, the
window's partition of unity, the NumPy twin of the overlap-add against the float64 oracle along the oracle's path, and the serving /
endpoint plumbing of `speed` on fakes."""
import ctypes as C
import logging
import threading

import numpy as np
import pytest
import torch

from chattts_amd import _lib, timescale as TS
from chattts_amd.engine import CodecEngine
from chattts_amd.serving import SpeechBatcher
from tests.test_split_pool_host import _Catch, _EndpointChat, _FakeBatcher, _FakeChat, _Params, _Pool, _spell, _wait_idle
from tests.timescale_oracle import HOP, RAD, WIN, hann, time_scale_f64


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def test_constants_are_the_stated_ones():
    assert (TS.N, TS.HS, TS.D, TS.DEN) == (WIN, HOP, RAD, 100) == (1024, 512, 256, 100)


def test_quantize():
    assert TS.quantize(0.5) == (50, 100) and TS.quantize(2.0) == (200, 100) and TS.quantize(1) == (100, 100)
    assert TS.quantize(1.25) == (125, 100) and TS.quantize(0.9) == (90, 100) and TS.quantize(1.1) == (110, 100)
    assert TS.quantize(1.004) == (100, 100) and TS.quantize(0.496) == (50, 100) and TS.quantize(2.004) == (200, 100)
    for bad in (0.49, 2.01, 0.0, -1.0, float("nan"), float("inf"), None, "fast"):
        with pytest.raises(ValueError):
            TS.quantize(bad)


@pytest.mark.parametrize("num", [50, 75, 90, 100, 110, 125, 150, 200])
def test_lengths_and_frames_at_the_edges(num):
    for n in (1, HOP - 1, HOP, HOP + 1, WIN, 12000):
        m = TS.out_len(n, num)
        assert (m - 1) * num < n * 100 <= m * num                     # m = ceil(100 n / num)
        assert TS.frames(m) == (m + HOP - 1) // HOP + 1
    assert [TS.frames(m) for m in (1, HOP - 1, HOP, HOP + 1, 2 * HOP, 2 * HOP + 1)] == [2, 2, 2, 3, 3, 4]
    assert TS.out_len(1, 200) == 1 and TS.out_len(1, 50) == 2 and TS.out_len(HOP, 200) == HOP // 2 and TS.out_len(HOP + 1, 200) == HOP // 2 + 1


def test_window_is_the_periodic_hann_and_a_partition_of_unity():
    w = TS.window()
    assert w.dtype == np.float64 and w.shape == (WIN,) and w[0] == 0.0 and abs(w[HOP] - 1.0) < 1e-15
    assert np.array_equal(w, hann())
    assert np.abs(w[:HOP] + w[HOP:] - 1.0).max() < 1e-15
    w32 = w.astype(np.float32)
    assert np.abs(w32[:HOP].astype(np.float64) + w32[HOP:] - 1.0).max() <= 2.0 ** -24      # after the table's rounding


def test_plan_offsets_and_refusals():
    num, den, out, path = TS.plan(1.25, [0, 1, 1 + HOP, 1 + HOP + 12000])
    assert (num, den) == (125, 100) and out.dtype == path.dtype == np.int64
    assert list(np.diff(out)) == [1, 410, 9600] and list(np.diff(path)) == [2, 2, 20]
    with pytest.raises(ValueError, match="nothing to scale"):
        TS.plan(1.0, [0, 10])
    with pytest.raises(ValueError, match="0.5 .. 2.0"):
        TS.plan(2.5, [0, 10])
    with pytest.raises(ValueError, match="empty"):
        TS.plan(1.25, [0, 5, 5, 9])
    with pytest.raises(ValueError, match="ascend"):
        TS.plan(1.25, [0, 9, 5])
    with pytest.raises(ValueError, match="start at 0"):
        TS.plan(1.25, [3, 9])
    with pytest.raises(ValueError, match="at least one segment"):
        TS.plan(1.25, [0])
    with pytest.raises(ValueError, match="2\\^31"):
        TS.plan(0.5, [0, 1 << 30])                 # 2^31 samples out
    with pytest.raises(ValueError, match="2\\^31"):
        TS.plan(2.0, [0, 1 << 31])                 # 2^31 samples in
    assert int(TS.plan(0.5, [0, (1 << 30) - 1])[2][-1]) == (1 << 31) - 2


def test_library_refuses_before_it_launches():
    """the C entry point checks the host tables first: these calls fail on a machine without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused on its host arguments

    def call(off_in, off_out, path_off, num, den=100, null=None):
        oi, oo, po = i64(off_in), i64(off_out), i64(path_off)
        p = {k: (None if k == null else fake) for k in ("x", "y", "path", "window", "oi", "oo", "po")}
        rc = lib.ctts_time_scale_ragged(p["x"], p["oi"], oi.ctypes.data_as(C.c_void_p), p["y"], p["oo"], oo.ctypes.data_as(C.c_void_p),
                                        p["path"], p["po"], po.ctypes.data_as(C.c_void_p), len(oi) - 1, p["window"], num, den, None)
        return rc, lib.ctts_last_error().decode()

    big = 1 << 31
    for args, why in [(([0, 1000], [0, 800], [0, 3], 125, 100, "x"), "null"), (([0, 1000], [0, 800], [0, 3], 125, 100, "path"), "null"),
                      (([0, 1000], [0, 800], [0, 3], 125, 100, "window"), "null"), (([0, 1000], [0, 800], [0, 3], 125, 100, "po"), "null"),
                      (([0, 1000], [0, 800], [0, 3], 49), "50 <= num <= 200"), (([0, 1000], [0, 800], [0, 3], 201), "50 <= num <= 200"),
                      (([0, 1000], [0, 800], [0, 3], 125, 50), "num / 100"), (([0, 1000], [0, 1000], [0, 3], 100), "nothing to scale"),
                      (([0, 9, 9], [0, 8, 16], [0, 2, 4], 125), "empty"), (([0, 9, 5], [0, 8, 16], [0, 2, 4], 125), "ascend"),
                      (([0, 1000], [0, 801], [0, 3], 125), "ceil"), (([0, 1000], [0, 799], [0, 3], 125), "ceil"),
                      (([0, 1000], [0, 800], [0, 4], 125), "frames of path"), (([3, 1000], [0, 800], [0, 3], 125), "first offsets"),
                      (([0, big], [0, -(-big * 100 // 125)], [0, TS.frames(-(-big * 100 // 125))], 125), "2^31"),
                      (([0, 3 << 30], [0, big], [0, TS.frames(big)], 150), "2^31")]:
        rc, msg = call(*args)
        assert rc != 0 and "ctts_time_scale_ragged" in msg and why in msg, (args, msg)


# ---- the oracle and the twin ----------------------------------------------------------------------------------------------------------
def test_oracle_at_speed_one_returns_its_input():
    """at num = 100 the natural continuation IS the nominal frame (c(0) is the template's energy), so every frame keeps d = 0 and the
    two window halves sum each sample back"""
    for n in (1, 300, HOP, 1500, 4096):
        x = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
        o = time_scale_f64(x, 1.0)
        assert np.array_equal(o["path"], HOP * np.arange(len(o["path"])) - HOP)
        assert o["y"].shape == (n,) and np.abs(o["y"] - x).max() <= 2.0 ** -50


def test_oracle_all_zero_segment_keeps_the_nominal_path():
    o = time_scale_f64(np.zeros(3000, np.float32), 1.25)
    assert o["zero_frame"][1:].all() and not o["y"].any()
    assert np.array_equal(o["path"], np.arange(len(o["path"])) * HOP * 125 // 100 - HOP)


@pytest.mark.parametrize("speed", [0.5, 0.9, 1.25, 2.0])
def test_apply_equals_the_oracle_along_the_oracles_path(speed):
    for n in (1, 300, HOP - 1, HOP, HOP + 1, 1500, 4096):
        x = np.random.default_rng(1000 + n).uniform(-1, 1, n).astype(np.float32)
        o = time_scale_f64(x, speed)
        y = TS.apply(x, speed, o["path"])
        assert y.dtype == np.float32 and y.shape == o["y"].shape == (TS.out_len(n, *TS.quantize(speed)),)
        assert len(o["path"]) == TS.frames(len(y))
        bound = 4 * 2.0 ** -24 * (o["w_a"] * np.abs(o["xa"]) + o["w_b"] * np.abs(o["xb"]))      # two table roundings, two products, one sum
        assert np.all(np.abs(y.astype(np.float64) - o["y"]) <= bound), (n, speed)
    with pytest.raises(ValueError, match="frames"):
        TS.apply(np.ones(1000, np.float32), 1.25, [-HOP, 100])


# ---- CodecEngine without a device: one decode, one call per run of a speed -------------------------------------------------------------
class _Codec:
    """a CodecEngine without a device: `decode_ragged` hands out 48 samples per token and goes through the engine's own
    `time_scale_segments`; the launches are recorded instead of made"""
    time_scale, time_scale_segments = CodecEngine.time_scale, CodecEngine.time_scale_segments

    def __init__(self):
        self.decodes, self.launches = [], []

    def decode_ragged(self, rows, return_mel=False, sample_rate=None, speed=None):
        self.decodes.append(len(rows))
        lens = [48 * int(r.shape[0]) for r in rows]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        wav = torch.cat([torch.full((n,), float(r[0, 0])) for n, r in zip(lens, rows)])
        return self.time_scale_segments(wav, off, [float(v) for v in speed])

    def _time_scale_launch(self, x, off, y, path, off_out, path_off, num, den):
        self.launches.append((num, den, [int(v) for v in np.diff(off)]))
        assert y.numel() == int(off_out[-1]) and path.numel() == int(path_off[-1]) and x.numel() == int(off[-1])
        for i in range(len(off) - 1):
            y[int(off_out[i]): int(off_out[i + 1])] = x[int(off[i])]


class _SpeedChat(_FakeChat):
    def __init__(self):
        super().__init__()
        self.codec, self.pcm_kw, self.split_kw, self.wav_kw = _Codec(), [], [], []

    def decode_to_pcm16(self, hids, ragged=False, **kw):
        assert ragged
        self.pcm_kw.append(kw)
        wav, off = self.codec.decode_ragged(list(hids), speed=kw.get("speed") or [1.0] * len(hids))
        return [wav[int(off[i]): int(off[i + 1])].numpy().astype(np.int16) for i in range(len(hids))]

    def decode_split_to_pcm16(self, groups, **kw):
        self.split_kw.append(kw)
        return super().decode_split_to_pcm16(groups)

    def decode_to_wavs(self, hids, **kw):
        self.wav_kw.append(kw)
        return super().decode_to_wavs(hids)


def test_speeds_at_one_poll_share_the_decode_and_reach_it_per_row():
    lock, pools = threading.Lock(), {}
    chat = _SpeedChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), speed=s) for c, s in (("a", 1.25), ("b", 1.25), ("c", None), ("d", 0.8))]
        res = [f.result(timeout=10) for f in futs]
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.pcm_kw == [{"speed": [1.25, 1.25, 1.0, 0.8]}]
    assert chat.codec.decodes == [4], "the four requests were not decoded together"
    assert chat.codec.launches == [(125, 100, [384, 384]), (80, 100, [384])]      # one call per run of a speed; speed 1 is copied
    assert [len(r) for r in res] == [308, 308, 384, 480] and [int(r[0]) for r in res] == [ord(c) for c in "abcd"]


def test_batcher_passes_the_speed_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _SpeedChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    try:
        b.submit("a#8", _Params(), speed=1.5).result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("c#8", _Params(), speed=1.0).result(timeout=10)
        b.submit("d#8", _Params(), speed=0.75, sample_rate=8000).result(timeout=10)
        pcm = b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, speed=2.0).result(timeout=30)
        b.submit("m#8\nn#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)
        _wait_idle(pools)
        for bad in (0.4, 2.5, "x"):
            with pytest.raises(ValueError):
                b.submit("e#8", _Params(), speed=bad)
    finally:
        b.close()
    assert chat.wav_kw == [{"speed": 1.5}, {}, {}, {"sample_rate": 8000, "speed": 0.75}]
    assert chat.split_kw == [{"speed": [2.0]}, {}] and _spell(pcm) == [("k", 8), ("l", 8)]


def test_submit_stream_refuses_a_speed():
    lock = threading.Lock()
    b = SpeechBatcher(_SpeedChat(), 2, lock, make_pool=lambda: _Pool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream("a#8", _Params(), speed=1.25)
        with pytest.raises(ValueError, match="0.5 .. 2.0"):
            b.submit_stream("a#8", _Params(), speed=3.0)
    finally:
        b.close()


# ---- Chat.infer: the refusal needs no engine ------------------------------------------------------------------------------------------
def test_chat_infer_refuses_a_streamed_speed_and_a_speed_out_of_range():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="path"):
        chat.infer(["hello"], stream=True, speed=1.25)
    with pytest.raises(ValueError, match="0.5 .. 2.0"):
        chat.infer(["hello"], speed=2.5)


# ---- the endpoint on a fake chat ----------------------------------------------------------------------------------------------------
def _app(batcher=None, **kw):
    from chattts_amd import server
    log, catch = logging.getLogger(f"test_timescale_host.{id(kw)}"), _Catch()
    log.addHandler(catch)
    chat = _EndpointChat()
    return server.create_app(chat, {"default": "SPK-D"}, batcher=batcher, logger=log, **kw), chat, catch


def test_endpoint_speed():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: validated and ignored, today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
        assert r.status_code == 200 and r.content == r0.content and sorted(chat.calls[-1][2]) == sorted(chat.calls[-2][2]) and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.25, "stream": True}).status_code == 200 and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "speed": 2.5}).status_code == 422
        assert not catch.msgs

    app, chat, catch = _app(speed=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
        assert r.status_code == 200 and chat.calls[-1][2]["speed"] == 1.25 and chat.calls[-1][1] is False
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.0}).status_code == 200 and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.0, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "path" in r.text and len(chat.calls) == n
        assert c.post("/v1/audio/speech", json={**body, "speed": 0.4}).status_code == 422 and len(chat.calls) == n
        assert not catch.msgs

    app, chat, catch = _app(speed=True, sample_rates=(8000, 24000), g711=True)      # composes with the rate and the companding
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "speed": 0.8, "sample_rate": 8000, "encoding": "ulaw"})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["speed"], kw["sample_rate"], kw["encoding"]) == (0.8, 8000, "ulaw")

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, speed=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.5}).status_code == 200 and bat.calls[-1][2] == {"speed": 1.5}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}
    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.5}).status_code == 200 and bat.calls[-1][2] == {}

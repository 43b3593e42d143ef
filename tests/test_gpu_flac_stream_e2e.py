"""Streamed FLAC end to end on the GPU.  The one invariant: wherever a stream yields PCM16 chunks, the same seeded request with FLAC yields
frames that the independent stream decoder (tests/flac_stream_oracle.py) reads back, behind the 42-byte stream header, as exactly those
int16 samples at the request's rate -- `decode_windows(flac=)` on its plain, rate and speed paths against the twin over the PCM windows,
the endpoint serially and from the pool, at 8000 Hz, at speed 1.25 and at both, concurrent pooled streams, and streams that are dropped
half way.  Synthetic weights.  `pytest -m gpu`."""
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, flac  # noqa: E402
from tests import flac_stream_oracle as SO  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _store  # noqa: E402

DEV = torch.device("cuda:0")
END1 = 256 * (2 * 30 - 1)
# three streams as the windows of three polls: a first chunk, an interior chunk (stream 1's clipped by its prefix's end), a tail (stream
# 1's with nothing left: it still ends its stream)
POLLS = [[(0, 24, 0, 6000, False), (1, 30, 0, 12000, False), (2, 40, 0, 9000, False)],
         [(0, 48, 6000, 18000, False), (1, 30, 12000, END1 + 500, False), (2, 64, 9000, 21000, False)],
         [(0, 48, 18000, None, True), (1, 30, END1, None, True), (2, 64, 21000, None, True)]]


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def chat(weights):
    return _chat(weights, "f32")


def _decoded(body, rate):
    assert body[:42] == flac.stream_header(rate)
    y, r = SO.decode(body)
    assert r == rate
    return y


# ---- 1. decode_windows(flac=, flac_streams=) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates,flags,speed", [((24000, 24000, 24000), (True, True, True), None), ((24000, 24000, 24000), (True, False, True), None),
                                               ((24000, 8000, 16000), (True, True, False), None), ((24000, 8000, 24000), (True, True, True), 1.25)])
def test_flagged_windows_are_the_twins_pushes_of_the_pcm_windows(codec, rates, flags, speed):
    """every poll once without and once with the flags (streams at another speed: fresh scaler / resampler streams for each run): a
    flagged window == the twin's push of the int16 window, a tail stripped by the conversion's keep mask on the device and marked
    final; the others come back as they do without the option"""
    store = _store()

    def run(with_flac):
        ts = [None if speed is None else codec.time_scale_stream_open(speed) for _ in rates]
        rs = [None if speed is None or r == 24000 else codec.resample_stream_open(24000, r) for r in rates]
        fs = [codec.flac_stream_open(r) if with_flac and f else None for r, f in zip(rates, flags)]
        kw = {} if all(r == 24000 for r in rates) else {"sample_rates": list(rates)}
        if speed is not None:
            kw.update(speeds=[speed] * 3, ts_streams=ts, **({"rs_streams": rs} if "sample_rates" in kw else {}))
        if with_flac:
            kw.update(flac=list(flags), flac_streams=fs)
        try:
            return [codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw) for wins in POLLS]
        finally:
            for h in ts:
                if h is not None:
                    codec.time_scale_stream_close(h)
            for h in rs:
                if h is not None:
                    codec.resample_stream_close(h)
            for h in fs:
                if h is not None:
                    codec.flac_stream_close(h)
    pcm, got = run(False), run(True)
    for s, (rate, f) in enumerate(zip(rates, flags)):
        if not f:
            assert all(g[s].dtype == np.int16 and g[s].tobytes() == p[s].tobytes() for g, p in zip(got, pcm)), s
            continue
        enc = flac.StreamEncoder(rate)
        for k, (g, p) in enumerate(zip(got, pcm)):
            assert p[s].dtype == np.int16 and g[s].dtype == np.uint8 and g[s].tobytes() == enc.push(p[s], k == 2), (s, k, p[s].size)
        y = _decoded(flac.stream_header(rate) + b"".join(g[s].tobytes() for g in got), rate)
        assert np.array_equal(y, np.concatenate([p[s] for p in pcm])) and y.size > 0
    assert codec.flac_streams_in_use() == 0
    if speed is None:
        assert pcm[2][1].size == 0                                     # stream 1's tail has no sample: its last push is an empty one
    h = codec.flac_stream_open(8000)
    try:
        for kw in (dict(flac=[True, False, False], flac_streams=[h, None, None]),                                  # a stream at another rate
                   dict(flac=[True, False, False], flac_streams=[None, None, None]),
                   dict(flac=[False, False, False], flac_streams=[h, None, None]),
                   dict(flac=[True, False, False], flac_streams=[h, None, None], sample_rates=[8000] * 3, encodings=["ulaw", None, None]),
                   dict(flac=[True, False, False], flac_streams=[h, None, None], sample_rates=[8000] * 3, pcm16=False)):
            with pytest.raises(ValueError):
                codec.decode_windows(store, POLLS[0], **{"pcm16": True, **kw})
        assert codec._pool("flac").records[h] == (8000, 0, 0, False)
    finally:
        codec.flac_stream_close(h)


# ---- 2. the endpoint ----------------------------------------------------------------------------------------------------------------------------
CASES = {"serial": ({}, {}), "pooled": (dict(batch_slots=4, batch_streams=True), {}),
         "8000 Hz": (dict(stream_sample_rates=(8000,)), {"sample_rate": 8000}),
         "speed 1.25": (dict(speed=True, stream_speed=True), {"speed": 1.25}),
         "speed and rate": (dict(speed=True, stream_speed=True, stream_sample_rates=(8000,), stream_speed_rates=True), {"speed": 1.25, "sample_rate": 8000}),
         "pooled, speed and rate": (dict(batch_slots=4, batch_streams=True, speed=True, stream_speed=True, stream_sample_rates=(8000,),
                                         stream_speed_rates=True), {"speed": 1.25, "sample_rate": 8000})}


@pytest.mark.parametrize("case", list(CASES))
def test_streamed_flac_body_decodes_to_the_streamed_pcm_body(chat, case):
    from starlette.testclient import TestClient
    from chattts_amd import server
    opts, more = CASES[case]
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 80, "min_new_token": 80})       # random weights do not stop on cue
    rate = more.get("sample_rate", 24000)
    body = {"input": "A streamed sentence.", "stream": True, **more}
    app = server.create_app(chat, voices, flac=True, stream_flac=True, **opts)
    try:
        with TestClient(app) as c:
            assert c.get("/health").json()["stream_flac"] is True
            pcm = c.post("/v1/audio/speech", json={**body, "response_format": "pcm"})
            fl = c.post("/v1/audio/speech", json={**body, "response_format": "flac"})
            if app.state.batcher is not None:
                occ = c.get("/health").json()["pool"]
                assert occ["stream_flac_chunks"] > 0 and occ["completed"] == 2, occ
        assert pcm.status_code == 200 and fl.status_code == 200 and fl.headers["content-type"] == "audio/flac"
        want = np.frombuffer(pcm.content, "<i2")
        y = _decoded(fl.content, rate)
        assert want.size > 0 and y.tobytes() == want.tobytes(), (case, y.size, want.size)
        with TestClient(server.create_app(chat, voices, flac=True, **{k: v for k, v in opts.items() if not k.startswith("batch")})) as c:
            assert c.post("/v1/audio/speech", json={**body, "response_format": "flac"}).status_code == 400     # without the option
    finally:
        chat.InferCodeParams = orig
        if app.state.batcher is not None:
            app.state.batcher.close()
    assert chat.codec.flac_streams_in_use() == 0 and chat.codec.time_scale_streams_in_use() == 0 and chat.codec.resample_streams_in_use() == 0


def test_two_pooled_flac_streams_and_a_pcm_stream_side_by_side(chat):
    """three streams from threads through one pool, two of them FLAC: each decodes to what the serial endpoint streams for the same
    request -- the same number of samples, each within 1 LSB, the bar tests/test_gpu_stream_pool.py sets for a pooled stream against
    the serial one (the rows of a shared batch are generated beside other rows) -- and the (text, voice) pairs are that test's, whose
    tails keep away from the strip threshold"""
    from starlette.testclient import TestClient
    from chattts_amd import server
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker(), "alloy": chat.sample_random_speaker(), "echo": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 120})
    reqs = [("One more short line.", "alloy", "flac"), ("See you tomorrow at noon.", "echo", "flac"), ("A streamed sentence.", "echo", "pcm")]
    app = server.create_app(chat, voices, batch_slots=4, batch_streams=True, flac=True, stream_flac=True)
    try:
        with TestClient(server.create_app(chat, voices)) as c:
            want = [np.frombuffer(c.post("/v1/audio/speech", json={"input": t, "voice": v, "response_format": "pcm", "stream": True}).content, "<i2")
                    for t, v, _ in reqs]
        res = [None] * 3
        with TestClient(app) as c:
            def go(i):
                t, v, fmt = reqs[i]
                res[i] = c.post("/v1/audio/speech", json={"input": t, "voice": v, "response_format": fmt, "stream": True})
            ths = [threading.Thread(target=go, args=(i,)) for i in range(3)]
            for th in ths:
                th.start()
            for th in ths:
                th.join(timeout=600)
            occ = c.get("/health").json()["pool"]
        assert all(r is not None and r.status_code == 200 for r in res)
        for i, (r, w) in enumerate(zip(res, want)):
            g = _decoded(r.content, 24000) if reqs[i][2] == "flac" else np.frombuffer(r.content, "<i2")
            assert w.size > 0 and g.size == w.size and np.abs(g.astype(np.int32) - w.astype(np.int32)).max() <= 1, (i, g.size, w.size)
        assert occ["completed"] == 3 and occ["max_stream_group"] >= 2 and occ["stream_flac_chunks"] > 0, occ
    finally:
        chat.InferCodeParams = orig
        app.state.batcher.close()
    assert chat.codec.flac_streams_in_use() == 0


def test_a_stream_dropped_half_way_gives_its_slot_back(chat):
    from chattts_amd.serving import SpeechBatcher
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), pcm16=True)
    pcm = [np.asarray(c) for c in chat.infer(["One more short line."], **kw)]
    got = list(chat.infer(["One more short line."], **kw, flac=True, stream_flac=True))
    assert len(got) == len(pcm) > 2 and all(len(g) == 1 and g[0].dtype == np.uint8 for g in got)
    y = _decoded(flac.stream_header(24000) + b"".join(g[0].tobytes() for g in got), 24000)
    assert y.tobytes() == np.concatenate([p[0] for p in pcm]).tobytes() and chat.codec.flac_streams_in_use() == 0
    chat.incremental_stream = False                                    # every chunk converted on the host: the host twin, the same stream
    try:
        twin = list(chat.infer(["One more short line."], **kw, flac=True, stream_flac=True))
        ref = [np.asarray(c) for c in chat.infer(["One more short line."], **kw)]
    finally:
        chat.incremental_stream = True
    y = _decoded(flac.stream_header(24000) + b"".join(g[0].tobytes() for g in twin), 24000)
    assert y.tobytes() == np.concatenate([p[0] for p in ref]).tobytes() and chat.codec.flac_streams_in_use() == 0
    gen = chat.infer(["One more short line."], **kw, flac=True, stream_flac=True)
    next(gen)
    assert chat.codec.flac_streams_in_use() == 1
    gen.close()
    assert chat.codec.flac_streams_in_use() == 0
    b = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_flac=True)
    try:
        s = b.submit_stream("One more short line.", _params(chat, spk), flac=True)
        first = next(s)
        assert first.dtype == np.uint8
        s.close()
        deadline = time.time() + 30
        while chat.codec.flac_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.flac_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1
    finally:
        b.close()

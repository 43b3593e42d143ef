"""Streamed IMA ADPCM end to end on the GPU.  The one invariant: wherever a stream yields PCM16 chunks, the same seeded request with
ADPCM yields blocks that are, concatenated, `adpcm.encode_blocks` of those int16 chunks, concatenated, at the request's rate -- byte for
byte: `decode_windows(adpcm=)` on its plain, rate and speed paths against the twin over the PCM windows (a stream named twice in one call
included), `Chat.infer` plain, resampled, at another speed, limited and paused, two concurrent pooled streams at different rates, and the
endpoint's open-ended WAV file.  Synthetic weights.  `pytest -m gpu`."""
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import adpcm, engine as E  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _store  # noqa: E402

DEV = torch.device("cuda:0")
END1 = 256 * (2 * 30 - 1)
# three streams as the windows of three polls: a first chunk, an interior chunk (stream 1's clipped by its prefix's end), a tail (stream
# 1's with nothing left: it still ends its stream)
POLLS = [[(0, 24, 0, 6000, False), (1, 30, 0, 12000, False), (2, 40, 0, 9000, False)],
         [(0, 48, 6000, 18000, False), (1, 30, 12000, END1 + 500, False), (2, 64, 9000, 21000, False)],
         [(0, 48, 18000, None, True), (1, 30, END1, None, True), (2, 64, 21000, None, True)]]
TEXT = ["One more short line."]


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def chat(weights):
    return _chat(weights, "f32")


def _blocks(pcm_chunks, rate):
    x = np.concatenate([np.asarray(c).reshape(-1) for c in pcm_chunks]).astype(np.int16)
    return adpcm.encode_blocks(x, rate).tobytes() if x.size else b""


# ---- 1. decode_windows(adpcm=, adpcm_streams=) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates,flags,speed", [((24000, 24000, 24000), (True, True, True), None), ((24000, 24000, 24000), (True, False, True), None),
                                               ((24000, 8000, 16000), (True, True, False), None), ((24000, 8000, 24000), (True, True, True), 1.25)])
def test_flagged_windows_are_the_twins_pushes_of_the_pcm_windows(codec, rates, flags, speed):
    """every poll once without and once with the flags (streams at another speed: fresh scaler / resampler streams for each run): a
    flagged window == the twin's push of the int16 window, a tail stripped by the conversion's keep mask on the device and marked
    final; the others come back as they do without the option"""
    store = _store()

    def run(with_adpcm):
        ts = [None if speed is None else codec.time_scale_stream_open(speed) for _ in rates]
        rs = [None if speed is None or r == 24000 else codec.resample_stream_open(24000, r) for r in rates]
        hs = [codec.adpcm_stream_open(r) if with_adpcm and f else None for r, f in zip(rates, flags)]
        kw = {} if all(r == 24000 for r in rates) else {"sample_rates": list(rates)}
        if speed is not None:
            kw.update(speeds=[speed] * 3, ts_streams=ts, **({"rs_streams": rs} if "sample_rates" in kw else {}))
        if with_adpcm:
            kw.update(adpcm=list(flags), adpcm_streams=hs)
        try:
            return [codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw) for wins in POLLS]
        finally:
            for h in ts:
                if h is not None:
                    codec.time_scale_stream_close(h)
            for h in rs:
                if h is not None:
                    codec.resample_stream_close(h)
            for h in hs:
                if h is not None:
                    codec.adpcm_stream_close(h)
    pcm, got = run(False), run(True)
    for s, (rate, f) in enumerate(zip(rates, flags)):
        if not f:
            assert all(g[s].dtype == np.int16 and g[s].tobytes() == p[s].tobytes() for g, p in zip(got, pcm)), s
            continue
        enc = adpcm.StreamEncoder(rate)
        for k, (g, p) in enumerate(zip(got, pcm)):
            assert p[s].dtype == np.int16 and g[s].dtype == np.uint8 and g[s].tobytes() == enc.push(p[s], k == 2).tobytes(), (s, k, p[s].size)
        body = b"".join(g[s].tobytes() for g in got)
        assert body == _blocks([p[s] for p in pcm], rate) and len(body) > 0
    assert codec.adpcm_streams_in_use() == 0
    if speed is None:
        assert pcm[2][1].size == 0                                     # stream 1's tail has no sample: its last push is an empty one


def test_a_stream_named_twice_goes_through_rounds_and_flac_sits_beside_it(codec):
    """the three windows of stream 0 in ONE call (the r-th push of a stream goes to step r), a FLAC window beside them; then the refusals,
    which leave the stream as it was"""
    from chattts_amd import flac
    store = _store()
    wins = [POLLS[0][0], POLLS[0][2], POLLS[1][0], POLLS[2][0]]
    pcm = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5)
    a, f = codec.adpcm_stream_open(24000), codec.flac_stream_open(24000)
    try:
        got = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, adpcm=[True, False, True, True], adpcm_streams=[a, None, a, a],
                                   flac=[False, True, False, False], flac_streams=[None, f, None, None])
    finally:
        codec.adpcm_stream_close(a)
        codec.flac_stream_close(f)
    enc = adpcm.StreamEncoder(24000)
    for k, last in ((0, False), (2, False), (3, True)):
        assert got[k].dtype == np.uint8 and got[k].tobytes() == enc.push(pcm[k], last).tobytes(), k
    assert b"".join(got[k].tobytes() for k in (0, 2, 3)) == _blocks([pcm[0], pcm[2], pcm[3]], 24000)
    assert got[1].tobytes() == bytes(flac.StreamEncoder(24000).push(pcm[1], False))
    h, f = codec.adpcm_stream_open(8000), codec.flac_stream_open(24000)
    try:
        for kw, why in ((dict(adpcm=[True, False, False], adpcm_streams=[h, None, None]), "at 24000 Hz"),                     # a stream at another rate
                        (dict(adpcm=[True, False, False], adpcm_streams=[None, None, None]), "needs an open ADPCM stream"),
                        (dict(adpcm=[False, False, False], adpcm_streams=[h, None, None]), "adpcm_streams without an adpcm flag"),
                        (dict(adpcm=[True, False, False], adpcm_streams=[h, h, None], sample_rates=[8000] * 3), "no adpcm flag but names"),
                        (dict(adpcm=[True, False, False]), "one adpcm flag and one adpcm_streams entry"),
                        (dict(adpcm=[True, False, False], adpcm_streams=[h, None, None], sample_rates=[8000] * 3, encodings=["ulaw", None, None]),
                         "does not go with an encoding"),
                        (dict(adpcm=[True, False, False], adpcm_streams=[h, None, None], sample_rates=[8000] * 3, pcm16=False), "pcm16=True"),
                        (dict(adpcm=[True, False, False], adpcm_streams=[h, None, None], sample_rates=[8000, 24000, 24000],
                              flac=[True, False, False], flac_streams=[f, None, None]), "8000 Hz"),
                        (dict(adpcm=[False, True, False], adpcm_streams=[None, h, None], sample_rates=[24000, 8000, 24000],
                              flac=[False, True, False], flac_streams=[None, f, None]), "at 8000 Hz")):
            with pytest.raises(ValueError, match=why):
                codec.decode_windows(store, POLLS[0], **{"pcm16": True, **kw})
        g = codec.flac_stream_open(8000)
        try:
            with pytest.raises(ValueError, match="FLAC or ADPCM, not both"):
                codec.decode_windows(store, POLLS[0], pcm16=True, sample_rates=[8000, 24000, 24000], adpcm=[True, False, False],
                                     adpcm_streams=[h, None, None], flac=[True, False, False], flac_streams=[g, None, None])
        finally:
            codec.flac_stream_close(g)
        assert codec._pool("adpcm").records[h] == (8000, 0, False)
    finally:
        codec.adpcm_stream_close(h)
        codec.flac_stream_close(f)
    assert codec.adpcm_streams_in_use() == 0 and codec.flac_streams_in_use() == 0


# ---- 2. Chat.infer ----------------------------------------------------------------------------------------------------------------------------
PATHS = {"plain": ({}, 24000), "8000 Hz": (dict(sample_rate=8000, stream_resample=True), 8000),
         "speed 1.25": (dict(speed=1.25, stream_time_scale=True), 24000),
         "limiter": (dict(limiter=True, stream_limiter=True, gain_db=6.0), 24000),
         "pauses": (dict(pauses={"max_pause_ms": 50, "lead_ms": 20, "tail_ms": 20, "threshold_db": -20.0}, stream_pauses=True), 24000)}


@pytest.mark.parametrize("path", list(PATHS))
def test_the_serial_stream_is_the_one_shot_encoder_over_its_pcm_stream(chat, path):
    on, rate = PATHS[path]
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), pcm16=True, **on)
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXT, **kw, adpcm=True)
    pcm = [c[0] if isinstance(c, list) else np.asarray(c)[0] for c in chat.infer(TEXT, **kw)]
    got = list(chat.infer(TEXT, **kw, adpcm=True, stream_adpcm=True))
    assert len(got) == len(pcm) > 2 and all(len(g) == 1 and g[0].dtype == np.uint8 for g in got)
    enc = adpcm.StreamEncoder(rate)
    for k, (g, p) in enumerate(zip(got, pcm)):
        assert g[0].tobytes() == enc.push(np.ascontiguousarray(p, dtype=np.int16), k == len(pcm) - 1).tobytes(), (path, k)
    body = b"".join(g[0].tobytes() for g in got)
    assert body == _blocks(pcm, rate) and len(body) > 0
    assert chat.codec.adpcm_streams_in_use() == 0
    if path == "plain":
        chat.incremental_stream = False                                # every chunk converted on the host: the host twin, the same blocks
        try:
            twin = list(chat.infer(TEXT, **kw, adpcm=True, stream_adpcm=True))
            ref = [np.asarray(c)[0] for c in chat.infer(TEXT, **kw)]
        finally:
            chat.incremental_stream = True
        assert b"".join(g[0].tobytes() for g in twin) == _blocks(ref, rate) and chat.codec.adpcm_streams_in_use() == 0
        gen = chat.infer(TEXT, **kw, adpcm=True, stream_adpcm=True)    # a consumer that goes away gives the stream back
        next(gen)
        assert chat.codec.adpcm_streams_in_use() == 1
        gen.close()
        assert chat.codec.adpcm_streams_in_use() == 0


# ---- 3. the pool ------------------------------------------------------------------------------------------------------------------------------
def test_two_pooled_streams_at_different_rates_share_the_encoder_step(chat):
    """two streams submitted together, once as PCM and once as ADPCM: the same co-resident rows, so the same samples; each ADPCM stream
    is the one-shot encoder over its PCM stream at its rate.  A cancelled stream gives its slot back."""
    from chattts_amd.serving import SpeechBatcher
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    reqs = [("One more short line.", None), ("See you tomorrow at noon.", 8000)]

    def run(b, **kw):
        with b.lock:         # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = [b.submit_stream(t, _params(chat, spk), **({} if r is None else {"sample_rate": r}), **kw) for t, r in reqs]
        out = [None] * len(reqs)
        ths = [threading.Thread(target=lambda i, s: out.__setitem__(i, list(s)), args=(i, s)) for i, s in enumerate(streams)]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=300)
        return out
    b = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_adpcm=True)
    try:
        pcm = run(b)
        got = run(b, adpcm_blocks=True)
        for (t, r), p, g in zip(reqs, pcm, got):
            rate = 24000 if r is None else r
            assert len(g) == len(p) > 2 and all(c.dtype == np.uint8 and c.size % adpcm.align(rate) == 0 for c in g)
            assert b"".join(c.tobytes() for c in g) == _blocks(p, rate), t
        occ = b.occupancy()
        assert occ["stream_adpcm_chunks"] == sum(len(g) for g in got) and occ["completed"] == 4 and "adpcm_encoded" not in occ, occ
        s = b.submit_stream(reqs[0][0], _params(chat, spk), adpcm_blocks=True)
        first = next(s)
        assert first.dtype == np.uint8
        s.close()
        deadline = time.time() + 30
        while chat.codec.adpcm_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.adpcm_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1
    finally:
        b.close()


# ---- 4. the endpoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,more", [({}, {}), (dict(stream_sample_rates=(8000,)), {"sample_rate": 8000})])
def test_endpoint_body_is_the_header_and_the_blocks_of_the_pcm_body(chat, opts, more):
    from starlette.testclient import TestClient
    from chattts_amd import server
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 80, "min_new_token": 80})       # random weights do not stop on cue
    rate = more.get("sample_rate", 24000)
    body = {"input": "A streamed sentence.", "stream": True, **more}
    try:
        with TestClient(server.create_app(chat, voices, adpcm=True, stream_adpcm=True, **opts)) as c:
            assert c.get("/health").json()["stream_adpcm"] is True
            pcm = c.post("/v1/audio/speech", json={**body, "response_format": "pcm"})
            ad = c.post("/v1/audio/speech", json={**body, "response_format": "adpcm"})
        assert pcm.status_code == 200 and ad.status_code == 200 and ad.headers["content-type"] == "audio/wav"
        x = np.frombuffer(pcm.content, "<i2")
        blocks, trace = adpcm.encode_blocks(x, rate, trace=True)
        assert x.size > 0 and ad.content[:60] == adpcm.stream_header(rate) and ad.content[60:] == blocks.tobytes()
        y, r = adpcm.parse_wav(ad.content)                             # every whole block: the samples, then the padding the coder follows
        assert r == rate and np.array_equal(y[: x.size], trace[: x.size]) and np.array_equal(y[x.size:], trace[x.size:])
        assert 0 <= y.size - x.size < adpcm.samples_per_block(rate)
        with TestClient(server.create_app(chat, voices, adpcm=True, **opts)) as c:
            assert c.post("/v1/audio/speech", json={**body, "response_format": "adpcm"}).status_code == 400     # without the option
    finally:
        chat.InferCodeParams = orig
    assert chat.codec.adpcm_streams_in_use() == 0

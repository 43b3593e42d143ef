"""`speed` end to end on the GPU: `Chat.infer(speed=)` against the device's own pieces composed on the host, ragged rows at their own
speeds, pooled requests against their serial calls, and the endpoint.  Synthetic weights, at most 32 tokens.  `pytest -m gpu`."""
import io
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd import timescale as TS  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = np.float32(1e-5)
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there."]
SPLIT = "Hello there. How are you. Fine."


@pytest.fixture(scope="module")
def chat(weights):
    from chattts_amd.core import Chat
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts={**weights, "dvae": W.synthetic_dvae()}, device=DEV, dtype="f32", tokenizer=os.path.join(GOLD, "tokenizer"),
                  spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voice = c.sample_random_speaker()
    return c


def _params(chat, i=0, max_new=None, **kw):
    return chat.InferCodeParams(top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=max_new or [24, 32, 16][i % 3], show_tqdm=False,
                                manual_seed=300 + 7 * i, spk_emb=chat.test_voice, **kw)


def _strip(w):
    return w[np.abs(w) > THR]


def _hiddens_of(chat, run):
    """the hidden states the serial call generates, batch by batch (recorded at `_infer_code`), and the call's result"""
    orig, calls = chat._infer_code, []

    def rec(text, stream, device, return_hidden, params):
        for out in orig(text, stream, device, return_hidden, params):
            calls.append([h.clone() for h in out.hiddens])
            yield out
    chat._infer_code = rec
    try:
        res = run()
    finally:
        del chat._infer_code
    return calls, res


@pytest.mark.parametrize("speed", [1.25, 0.8])
def test_float_output_is_the_speed_1_decode_time_scaled(chat, speed):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False)
    calls1, one = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), **kw))
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), speed=speed, **kw))
    assert len(calls) == len(calls1) == 1 and all(torch.equal(a, b) for a, b in zip(calls[0], calls1[0])), "the speed changed what was generated"
    wav1 = codec.decode_to_wavs(calls[0])                                  # what the speed-1 call strips and returns
    assert [w.tobytes() for w in one] == [_strip(w).tobytes() for w in codec.to_host(wav1)]
    want = codec.to_host(codec.time_scale(wav1, speed))
    assert want.shape == (3, TS.out_len(wav1.shape[1], *TS.quantize(speed)))
    assert len(got) == 3 and all(g.dtype == np.float32 and g.tobytes() == _strip(w).tobytes() for g, w in zip(got, want))
    assert chat.decode_to_wavs(calls[0], speed=speed).tobytes() == want.tobytes()


def test_telephony_at_a_speed_is_the_host_twins_behind_the_devices_time_scaled_waveform(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True, sample_rate=8000, encoding="ulaw")
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), speed=1.25, **kw))
    scaled = codec.time_scale(codec.decode_to_wavs(calls[0]), 1.25)          # the device's time-scaled float waveform, padded batch
    wav8 = codec.to_host(codec.resample(scaled, 24000, 8000))
    assert len(got) == 3
    for g, w in zip(got, wav8):
        assert g.dtype == np.uint8 and g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()

    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), speed=1.25, ragged_decode=True, **kw))
    for g, h in zip(got, calls[0]):       # every row decoded alone, scaled alone, resampled alone
        w = codec.to_host(codec.resample(codec.time_scale(codec.decode_to_wavs([h])[0], 1.25), 24000, 8000))
        assert g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()


def test_split_request_scales_every_sentence_alone_in_front_of_the_strip(chat):
    codec = chat.codec
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), speed=1.5, ragged_decode=ragged,
                                                          skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.to_host(codec.time_scale(codec.decode_to_wavs([h])[0], 1.5)) for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch scaled alone
            ws = [w for c in calls[1:] for w in codec.to_host(codec.time_scale(codec.decode_to_wavs(c), 1.5))]
        assert len(ws) == 3
        assert len(got) == 1 and got[0].tobytes() == float_to_int16(np.concatenate([_strip(w) for w in ws])).tobytes()


def test_ragged_rows_at_their_own_speeds_equal_each_alone(chat):
    rows = [torch.randn(t, 768, device=DEV) * 0.1 for t in (9, 14, 5)]
    speeds = [1.0, 1.25, 0.8]
    got = chat.decode_to_pcm16(rows, ragged=True, speed=speeds)
    for g, r, s in zip(got, rows, speeds):
        assert g.dtype == np.int16 and g.tobytes() == chat.decode_to_pcm16([r], ragged=True, speed=s)[0].tobytes()
    today = chat.decode_to_pcm16(rows, ragged=True)
    assert got[0].tobytes() == today[0].tobytes() and got[1].tobytes() != today[1].tobytes()
    assert [x.tobytes() for x in chat.decode_to_pcm16(rows, ragged=True, speed=[1.0, 1.0, 1.0])] == [x.tobytes() for x in today]
    floats = chat.decode_to_wavs(rows, ragged=True, speed=speeds)
    assert [len(f) for f in floats] == [TS.out_len(256 * (2 * t - 1), *TS.quantize(s)) for t, s in zip((9, 14, 5), speeds)]
    mixed = chat.decode_to_pcm16(rows, ragged=True, speed=speeds, sample_rate=[8000, 8000, 24000], encoding=["ulaw", None, None])
    for g, r, s, sr, e in zip(mixed, rows, speeds, (8000, 8000, 24000), ("ulaw", None, None)):
        alone = chat.decode_to_pcm16([r], ragged=True, speed=s, sample_rate=sr, **({} if e is None else {"encoding": e}))[0]
        assert g.dtype == alone.dtype and g.tobytes() == alone.tobytes()


def test_speed_1_is_todays_call_and_a_stream_at_another_speed_raises(chat):
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
    b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), speed=1.0, **kw)
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), speed=1.25, **kw)


class _Recording(SpeechBatcher):
    def _handle(self, got):
        for it in ([got] if isinstance(got, tuple) else got if isinstance(got, list) else []):
            self.code_ids[it[0]] = it[1].cpu().numpy()
            self.hids[it[0]] = it[2].clone()
        super()._handle(got)


def test_pooled_requests_at_their_speeds_equal_their_serial_calls(chat):
    speeds = [1.25, None, 0.8]
    serial, ids = [], []
    for i, (t, s) in enumerate(zip(TEXTS, speeds)):
        orig = chat._infer_code

        def rec(text, stream, device, return_hidden, params, orig=orig):
            for out in orig(text, stream, device, return_hidden, params):
                ids.append(out.ids[0].cpu().numpy().copy())
                yield out
        chat._infer_code = rec
        try:
            serial.append(chat.infer([t], skip_refine_text=True, split_text=False, pcm16=True, ragged_decode=True, params_infer_code=_params(chat, i, 24),
                                     **({} if s is None else {"speed": s}))[0])
        finally:
            del chat._infer_code
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.code_ids, b.hids = {}, {}
    try:
        with b.lock:
            futs = [b.submit(t, _params(chat, i, 24), speed=s) for i, (t, s) in enumerate(zip(TEXTS, speeds))]
        got = [f.result(timeout=300) for f in futs]
        decodes = b.decode_calls
    finally:
        b.close()
    if len({len(i) for i in ids}) == 1:       # the same number of tokens: they finish at one poll
        assert decodes == 1, "the three requests did not share one decode"
    for i, (g, s) in enumerate(zip(got, serial)):
        assert np.array_equal(b.code_ids[futs[i].rid], ids[i]), i
        # the serial call's decode stage on the pool's own hidden states, bit for bit
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **({} if speeds[i] is None else {"speed": speeds[i]}))[0]
        assert g.dtype == np.int16 and g.tobytes() == alone.tobytes(), i
        assert g.shape == s.shape, (i, g.shape, s.shape)
        assert int(np.abs(g.astype(np.int32) - s.astype(np.int32)).max()) <= 1, i          # the pooled tests' bar: one count


def _server_params(chat):
    """the endpoint's fixed sampling parameters for the default voice (server.create_app: code_params), capped like the test's app"""
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice,
                                stream_batch=24, stream_speed=12000, pass_first_n_batches=2)


def _frames(body):
    with wave.open(io.BytesIO(body), "rb") as wf:
        assert wf.getframerate() == 24000
        return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")


def test_endpoint_serves_the_speed_when_asked_to_and_ignores_it_by_default(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        fast = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, speed=1.25)[0]
        assert 0 < len(fast) <= -(-256 * (2 * 24 - 1) * 100 // 125) and fast.tobytes() != today.tobytes()     # ceil(n / 1.25), less what the strip took
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, speed=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
            assert r.status_code == 200 and _frames(r.content).tobytes() == fast.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert c.post("/v1/audio/speech", json={**body, "speed": 1.25, "stream": True}).status_code == 400
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
    finally:
        chat.InferCodeParams = orig_params

"""Sample rates end to end on the GPU: a voice cloned from a 16 kHz clip, `Chat.infer(sample_rate=)` against the host composition of the
device's own pieces, pooled requests at five rates against their serial calls, and the endpoint.  Synthetic weights, at most 64 tokens.
`pytest -m gpu`."""
import io
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import weights as W  # noqa: E402
from chattts_amd.audio import float_to_int16, pcm_to_wav_bytes  # noqa: E402
from chattts_amd.frontend import Speaker  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests.resample_oracle import resample_f64  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = np.float32(1e-5)
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there.", "How are you today?", "The fifth one."]
RATES = [8000, 16000, 24000, 44100, 48000]
SPLIT = "Hello there. How are you. Fine."


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def chat(request, weights):
    from chattts_amd.core import Chat
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts={**weights, "dvae": W.synthetic_dvae()}, device=DEV, dtype=request.param, tokenizer=os.path.join(GOLD, "tokenizer"),
                  spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voice = c.sample_random_speaker()
    return c


def _params(chat, i=0, **kw):
    return chat.InferCodeParams(top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=[24, 32, 16][i % 3], show_tqdm=False,
                                manual_seed=300 + 7 * i, spk_emb=chat.test_voice, **kw)


def _clip(seed, n=24000):
    """one second of a voiced-looking signal: a few harmonics under a slow envelope, plus a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    f0 = rng.uniform(90, 220)
    w = sum(rng.uniform(0.1, 0.4) * np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 6)) for k in range(1, 9))
    return (0.3 * w * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _agreement(a: str, b: str) -> float:
    ca, cb = Speaker.decode_prompt(a).numpy(), Speaker.decode_prompt(b).numpy()
    n = min(ca.shape[1], cb.shape[1])
    return float((ca[:, :n] == cb[:, :n]).mean())


def test_a_voice_cloned_from_a_resampled_clip(chat):
    w = _clip(1)
    ref = chat.sample_audio_speaker(w)
    assert chat.sample_audio_speaker(w, 24000) == ref and chat.sample_audio_speaker(w, None) == ref
    got = chat.sample_audio_speaker(resample_f64(w, 24000, 16000).astype(np.float32), 16000)
    t_ref, t_got = Speaker.decode_prompt(ref).shape[1], Speaker.decode_prompt(got).shape[1]
    assert t_ref > 0 and abs(t_got - t_ref) <= 1, (t_got, t_ref)


def _clip_from_16k(seed):
    """a 24 kHz clip with a 16 kHz origin: one second of the same signal generated at 16 kHz (full band there, noise included) and
    brought to 24 kHz by the oracle -- what a 24 kHz copy of a 16 kHz recording holds"""
    rng = np.random.default_rng(seed)
    t = np.arange(16000) / 16000.0
    f0 = rng.uniform(90, 220)
    w = sum(rng.uniform(0.1, 0.4) * np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 6)) for k in range(1, 9))
    w = (0.3 * w * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * rng.standard_normal(16000)).astype(np.float32)
    return resample_f64(w, 16000, 24000).astype(np.float32)


def test_token_agreement_of_the_resampled_clip_beats_unrelated_clips(chat):
    """The tokens of a clip that went 24k -> 16k (oracle) -> 24k (device) against the tokens of the clip itself must agree more often
    than the tokens of two unrelated clips do.  The clips are 24 kHz copies of 16 kHz material (`_clip_from_16k`): the comparison
    is about what the conversion does to content a 16 kHz clip can carry.  A clip with energy between 8 and 12 kHz loses that band
    at 16 kHz whatever the resampler, and the synthetic encoder (random weights on log-mel bins up to 12 kHz) turns the loss of 12 of
    its 100 bins into a change of every token: measured 0.000 against 0.000 for such clips, on the device and with the float64 oracle
    and the NumPy DVAE oracle alike.  For the clips used here the oracles give 0.154 (round trip) against 0.037 (unrelated)."""
    w, other = _clip_from_16k(1), _clip_from_16k(2)
    ref = chat.sample_audio_speaker(w)
    got = chat.sample_audio_speaker(resample_f64(w, 24000, 16000).astype(np.float32), 16000)
    assert abs(Speaker.decode_prompt(got).shape[1] - Speaker.decode_prompt(ref).shape[1]) <= 1
    same, unrelated = _agreement(got, ref), _agreement(chat.sample_audio_speaker(other), ref)
    print(f"token agreement: 16 kHz round trip {same:.3f}, unrelated clip {unrelated:.3f}")
    assert same > unrelated


def _strip16(w):
    return float_to_int16(w[np.abs(w) > THR])


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


def test_serial_call_at_8k_is_the_host_composition_of_the_devices_pieces(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS[:3], params_infer_code=_params(chat), sample_rate=8000, **kw))
    wav8 = codec.to_host(codec.resample(codec.decode_to_wavs(calls[0]), 24000, 8000))          # padded batch, then every row resampled
    assert len(got) == 3 and all(g.dtype == np.int16 and g.tobytes() == _strip16(w).tobytes() for g, w in zip(got, wav8))

    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS[:3], params_infer_code=_params(chat), sample_rate=8000, ragged_decode=True, **kw))
    for g, h in zip(got, calls[0]):       # every row decoded alone, resampled alone
        w = codec.to_host(codec.resample(codec.decode_to_wavs([h])[0], 24000, 8000))
        assert g.tobytes() == _strip16(w).tobytes()

    calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), sample_rate=8000, ragged_decode=True,
                                                      skip_refine_text=True, split_text=True, pcm16=True))
    ws = [codec.to_host(codec.resample(codec.decode_to_wavs([h])[0], 24000, 8000)) for c in calls[1:] for h in c]      # calls[0]: the refer sentence
    assert len(ws) == 3 and any(len(w) % 8 for w in ws[:-1]), "pick lengths that leave the sentences' offsets off multiples of 8"
    assert len(got) == 1 and got[0].tobytes() == float_to_int16(np.concatenate([w[np.abs(w) > THR] for w in ws])).tobytes()


def test_24k_is_todays_call_and_a_stream_at_another_rate_raises(chat):
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
    b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), sample_rate=24000, **kw)
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), sample_rate=8000, **kw)


class _Recording(SpeechBatcher):
    def _handle(self, got):
        for it in ([got] if isinstance(got, tuple) else got if isinstance(got, list) else []):
            self.code_ids[it[0]] = it[1].cpu().numpy()
        super()._handle(got)


def test_pooled_requests_at_five_rates_equal_their_serial_calls(chat):
    serial, ids = [], []
    for i, (t, r) in enumerate(zip(TEXTS, RATES)):
        orig = chat._infer_code

        def rec(text, stream, device, return_hidden, params, orig=orig):
            for out in orig(text, stream, device, return_hidden, params):
                ids.append(out.ids[0].cpu().numpy().copy())
                yield out
        chat._infer_code = rec
        try:
            serial.append(chat.infer([t], skip_refine_text=True, split_text=False, pcm16=True, ragged_decode=True, params_infer_code=_params(chat, i),
                                     sample_rate=r)[0])
        finally:
            del chat._infer_code
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.code_ids = {}
    try:
        with b.lock:
            futs = [b.submit(t, _params(chat, i), sample_rate=r) for i, (t, r) in enumerate(zip(TEXTS, RATES))]
        got = [f.result(timeout=300) for f in futs]
    finally:
        b.close()
    for i, (g, s) in enumerate(zip(got, serial)):
        assert np.array_equal(b.code_ids[futs[i].rid], ids[i]), i
        assert g.dtype == np.int16 and g.shape == s.shape, (i, g.shape, s.shape)
        assert int(np.abs(g.astype(np.int32) - s.astype(np.int32)).max()) <= 1, i          # the pooled tests' bar: one count


def test_endpoint_rate_and_uploaded_voice(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        app = server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 16000, 24000, 44100, 48000), voice_upload=True)
        with TestClient(app) as c:
            r24 = c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "wav"})
            r8 = c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "wav", "sample_rate": 8000})
            assert r24.status_code == 200 and r8.status_code == 200
            with wave.open(io.BytesIO(r8.content), "rb") as wf:
                assert wf.getframerate() == 8000
                pcm8 = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
            p = server_params(chat)
            want = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, sample_rate=8000)[0]
            assert pcm8.tobytes() == want.tobytes()
            clip16 = resample_f64(_clip(4), 24000, 16000).astype(np.float32)
            up = c.post("/v1/audio/voices", params={"name": "anna"}, content=pcm_to_wav_bytes(clip16 / max(1.0, np.abs(clip16).max()), 16000))
            assert up.status_code == 200 and up.json()["sample_rate"] == 16000 and up.json()["tokens"] > 0, up.text
            seen = []
            orig = chat.code_prompt
            chat.code_prompt = lambda text, params: (seen.append(params.spk_smp), orig(text, params))[1]
            try:
                r = c.post("/v1/audio/speech", json={"input": TEXTS[1], "voice": "anna", "response_format": "pcm"})
            finally:
                del chat.code_prompt
            assert r.status_code == 200 and len(r.content) > 0
            assert seen and seen[0] is not None and Speaker.decode_prompt(seen[0]).shape[1] == up.json()["tokens"]
    finally:
        chat.InferCodeParams = orig_params


def server_params(chat):
    """the endpoint's fixed sampling parameters for the default voice (server.create_app: code_params), capped like the test's app"""
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice,
                                stream_batch=24, stream_speed=12000, pass_first_n_batches=2)


def test_unstripped_length_is_a_third_at_8k(chat):
    hid = torch.randn(9, 768, device=DEV) * 0.1
    a, b = chat.decode_to_wavs([hid]), chat.decode_to_wavs([hid], sample_rate=8000)
    assert b.shape == (1, -(-a.shape[1] // 3))

"""`loudness` end to end on the GPU: `Chat.infer(loudness=)` against the device's own pieces composed on the host and against the
independent oracle, with every output format, a split request under one gain, pooled requests at their own targets, and the endpoint.
Synthetic weights, at most 32 tokens.  `pytest -m gpu`."""
import io
import math
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import flac as FLAC  # noqa: E402
from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd import loudness as LN  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests import loudness_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = np.float32(1e-5)
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there."]
SPLIT = "Hello there. How are you. Fine."
TARGET = -20.0


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


def test_no_target_is_todays_call_bit_for_bit(chat):
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, ragged_decode=True), dict(ragged_decode=True)):
        kw = dict(skip_refine_text=True, split_text=False, **kw)
        a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
        b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), loudness=None, **kw)
        c = chat.infer(TEXTS[:2], params_infer_code=_params(chat), loudness=[None, None], **kw)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b] == [x.tobytes() for x in c] and a[0].dtype == b[0].dtype
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), loudness=TARGET)


def test_float_and_pcm16_output_reach_the_target_the_record_reports(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False)
    calls1, _ = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), **kw))
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), loudness=TARGET, **kw))
    assert len(calls) == len(calls1) == 1 and all(torch.equal(a, b) for a, b in zip(calls[0], calls1[0])), "the target changed what was generated"
    wav1 = codec.decode_to_wavs(calls[0])
    want_d, st = codec.loudness_normalize(wav1, TARGET, return_stats=True)
    want = codec.to_host(want_d)
    assert len(got) == 3 and all(g.dtype == np.float32 and g.tobytes() == _strip(w).tobytes() for g, w in zip(got, want))
    assert chat.decode_to_wavs(calls[0], loudness=TARGET).tobytes() == want.tobytes()
    x = codec.to_host(wav1)
    for b in range(3):
        o = O.group([x[b]], [24000], TARGET)
        assert abs(o["L"] - st["L"][b]) <= 1e-9 and o["bound"] == st["bound"][b], (b, o, st[b])
        after = O.group([want[b]], [24000], None)["L"]                     # the oracle on what the call returned
        reach = st["L"][b] + 20.0 * math.log10(float(st["g32"][b]))         # min(target, what the ceiling or the cap allows)
        print(f"row {b}: L {st['L'][b]:.4f} -> {after:.4f} LUFS, g32 {st['g32'][b]:.6g}, bound {st['bound'][b]}")
        assert abs(after - reach) <= 0.01 and reach <= TARGET + 1e-6 and (st["bound"][b] != 0 or abs(after - TARGET) <= 0.01)
        assert np.abs(want[b]).max() <= np.float32(LN.CEILING) * (1.0 + 2.0 ** -22)
    pcm = chat.infer(TEXTS, params_infer_code=_params(chat), loudness=TARGET, pcm16=True, **kw)
    for b in range(3):
        assert pcm[b].dtype == np.int16 and pcm[b].tobytes() == float_to_int16(_strip(want[b])).tobytes()
        assert int(np.abs(pcm[b].astype(np.int32)).max()) <= math.ceil(LN.CEILING * 32767 * (1.0 + 2.0 ** -22)) < 32767
    per_row = chat.infer(TEXTS, params_infer_code=_params(chat), loudness=[TARGET, None, -30.0], pcm16=True, **kw)
    alone30 = codec.to_host(codec.loudness_normalize(wav1, [None, None, -30.0]))
    assert per_row[0].tobytes() == pcm[0].tobytes() and per_row[1].tobytes() == float_to_int16(_strip(x[1])).tobytes()
    assert per_row[2].tobytes() == float_to_int16(_strip(alone30[2])).tobytes()


def test_every_output_format_is_the_host_composition_behind_the_normalised_waveform(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True, loudness=TARGET)
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), encoding="ulaw", **kw))
    wav1 = codec.decode_to_wavs(calls[0])
    norm = codec.to_host(codec.loudness_normalize(wav1, TARGET))
    for g, w in zip(got, norm):
        assert g.dtype == np.uint8 and g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()
    got = chat.infer(TEXTS, params_infer_code=_params(chat), flac=True, **kw)
    for g, w in zip(got, norm):
        assert g.dtype == np.uint8 and g.tobytes() == FLAC.encode(float_to_int16(_strip(w)), 24000)
    got = chat.infer(TEXTS, params_infer_code=_params(chat), sample_rate=8000, **kw)          # behind the resampler, at ITS rate
    norm8 = codec.to_host(codec.loudness_normalize(codec.resample(wav1, 24000, 8000), TARGET, rates=8000))
    for g, w in zip(got, norm8):
        assert g.tobytes() == float_to_int16(_strip(w)).tobytes()
    assert any(a.tobytes() != b.tobytes() for a, b in zip(norm8, codec.to_host(codec.loudness_normalize(codec.resample(wav1, 24000, 8000), TARGET))))
    got = chat.infer(TEXTS, params_infer_code=_params(chat), speed=1.25, **kw)               # behind the time scaler
    norm_s = codec.to_host(codec.loudness_normalize(codec.time_scale(wav1, 1.25), TARGET))
    for g, w in zip(got, norm_s):
        assert g.tobytes() == float_to_int16(_strip(w)).tobytes()
    # ragged rows: each decoded, scaled, resampled and normalised alone, whatever it is packed with
    rows = [torch.randn(t, 768, device=DEV) * 0.1 for t in (9, 14, 5)]
    tg, rates, encs = [TARGET, None, -30.0], [8000, 24000, 16000], ["ulaw", None, None]
    mixed = chat.decode_to_pcm16(rows, ragged=True, loudness=tg, sample_rate=rates, encoding=encs, speed=[1.0, 1.25, 0.8])
    for g, r, t, sr, e, s in zip(mixed, rows, tg, rates, encs, (1.0, 1.25, 0.8)):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, speed=s, **({} if t is None else {"loudness": t}),
                                     **({} if e is None else {"encoding": e}))[0]
        assert g.dtype == alone.dtype and g.tobytes() == alone.tobytes()
    today = chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, speed=[1.0, 1.25, 0.8])
    assert mixed[1].tobytes() == today[1].tobytes() and mixed[2].tobytes() != today[2].tobytes()
    flacs = chat.decode_to_pcm16(rows, ragged=True, loudness=TARGET, flac=[True, False, True])
    plain = chat.decode_to_pcm16(rows, ragged=True, loudness=TARGET)
    assert flacs[1].tobytes() == plain[1].tobytes() and flacs[0].tobytes() == FLAC.encode(plain[0], 24000) and flacs[2].tobytes() == FLAC.encode(plain[2], 24000)


def test_a_split_request_gets_one_gain_over_its_sentences(chat):
    codec = chat.codec
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), loudness=TARGET, ragged_decode=ragged,
                                                          skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.decode_to_wavs([h])[0] for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch
            ws = [w for c in calls[1:] for w in codec.decode_to_wavs(c)]
        assert len(ws) == 3
        off = np.concatenate([[0], np.cumsum([w.numel() for w in ws])]).astype(np.int64)
        y, st = codec.loudness_normalize(torch.cat(ws), TARGET, offsets=off, groups=[0, 3], return_stats=True)
        y = codec.to_host(y)
        o = O.group([codec.to_host(w) for w in ws], [24000] * 3, TARGET)
        assert len(st) == 1 and st["n_blocks"][0] == o["n_blocks"] and abs(st["L"][0] - o["L"]) <= 1e-9 and st["bound"][0] == o["bound"]
        want = float_to_int16(np.concatenate([_strip(y[off[i]: off[i + 1]]) for i in range(3)]))
        assert len(got) == 1 and got[0].tobytes() == want.tobytes(), ragged
    floats = chat.infer(SPLIT, params_infer_code=_params(chat), loudness=TARGET, skip_refine_text=True, split_text=True)
    assert len(floats) == 1 and float_to_int16(floats[0]).tobytes() == got[0].tobytes()


class _Recording(SpeechBatcher):
    def _handle(self, got):
        for it in ([got] if isinstance(got, tuple) else got if isinstance(got, list) else []):
            self.hids[it[0]] = it[2].clone()
        super()._handle(got)


def test_pooled_requests_at_their_targets_share_a_decode_and_equal_their_own_calls(chat):
    targets = [TARGET, -30.0, None]
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.hids = {}
    try:
        with b.lock:
            futs = [b.submit(TEXTS[0], _params(chat, 0, 24), loudness=t) for t in targets]      # the same text: they finish at one poll
        got = [f.result(timeout=300) for f in futs]
        decodes = b.decode_calls
    finally:
        b.close()
    assert decodes == 1, "the three requests did not share one decode"
    for i, (g, t) in enumerate(zip(got, targets)):
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **({} if t is None else {"loudness": t}))[0]
        assert g.dtype == np.int16 and g.tobytes() == alone.tobytes(), i
    assert got[0].tobytes() != got[1].tobytes() and got[0].tobytes() != got[2].tobytes()
    serial = chat.infer([TEXTS[0]], skip_refine_text=True, split_text=False, pcm16=True, ragged_decode=True, params_infer_code=_params(chat, 0, 24),
                        loudness=TARGET)[0]
    assert got[0].shape == serial.shape and int(np.abs(got[0].astype(np.int32) - serial.astype(np.int32)).max()) <= 1      # the pooled tests' bar


def _server_params(chat):
    """the endpoint's fixed sampling parameters for the default voice (server.create_app: code_params), capped like the test's app"""
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice,
                                stream_batch=24, stream_speed=12000, pass_first_n_batches=2)


def _frames(body):
    with wave.open(io.BytesIO(body), "rb") as wf:
        assert wf.getframerate() == 24000
        return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")


def test_endpoint_serves_the_target_when_asked_to_and_ignores_it_by_default(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        loud = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, loudness=TARGET)[0]
        assert loud.dtype == np.int16 and loud.tobytes() != today.tobytes()
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, loudness=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "loudness": TARGET})
            assert r.status_code == 200 and _frames(r.content).tobytes() == loud.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert c.post("/v1/audio/speech", json={**body, "loudness": TARGET, "stream": True}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "loudness": -3}).status_code == 400
            assert c.get("/health").json()["loudness"] is True
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            r = c.post("/v1/audio/speech", json={**body, "loudness": TARGET})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
    finally:
        chat.InferCodeParams = orig_params

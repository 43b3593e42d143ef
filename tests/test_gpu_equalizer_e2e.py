"""`eq` end to end on the GPU: `Chat.infer(eq=)` and the decode calls against the public stage methods called by hand in the chain's
order (decode, equalize, compress, loudness_normalize with the limiter), through every output format, a split request, pooled requests
and the endpoint.  Synthetic weights, at most 32 tokens.  `pytest -m gpu`."""
import logging
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import adpcm as ADPCM  # noqa: E402
from chattts_amd import equalizer as EQ  # noqa: E402
from chattts_amd import flac as FLAC  # noqa: E402
from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from tests import equalizer_cases as K  # noqa: E402
from tests.test_gpu_loudness_e2e import SPLIT, TEXTS, _Recording, _frames, _hiddens_of, _params, _server_params, _strip, chat  # noqa: E402,F401

TARGET = -16.0
TONE = {"highpass_hz": 150, "peaks": [{"hz": 2500, "db": 6, "q": 1.5}], "highshelf": {"hz": 6000, "db": -3}}
DEEP = {"threshold_db": -60, "ratio": 4, "hold_ms": 20}       # synthetic weights speak softly: a curve that reaches them whatever their level


def _within_an_ulp_of_the_definition(codec, wav, y, rate, spec):
    """the stage's result on the device against `equalizer.apply` of every row (the share that differs is tests/test_gpu_equalizer.py's)"""
    for x, g in zip(codec.to_host(wav), codec.to_host(y)):
        assert int(K.ulps(g, EQ.apply(x, rate, spec)).max()) <= 1


def test_off_is_todays_call_bit_for_bit(chat):
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, ragged_decode=True), dict(loudness=-20.0, limiter=True, pcm16=True)):
        kw = dict(skip_refine_text=True, split_text=False, **kw)
        a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
        b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), eq=None, **kw)
        c = chat.infer(TEXTS[:2], params_infer_code=_params(chat), eq=[False, {}], **kw)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b] == [x.tobytes() for x in c] and a[0].dtype == b[0].dtype
    with pytest.raises(ValueError, match="filter state carried across chunks"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), eq="telephone")


def test_the_telephone_preset_at_8_khz_in_mu_law_is_the_stages_by_hand(chat):
    """Chat.infer(eq="telephone", sample_rate=8000, pcm16=True, encoding="ulaw") is the decode without `eq`, then CodecEngine.equalize,
    then the same tail of the chain, byte for byte"""
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, sample_rate=8000, pcm16=True, encoding="ulaw")
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), eq="telephone", **kw))
    assert len(calls) == 1
    wav = codec.decode_to_wavs(calls[0], sample_rate=8000)                       # the decode without `eq`, at the request's rate
    y = codec.equalize(wav, "telephone", rates=8000)
    _within_an_ulp_of_the_definition(codec, wav, y, 8000, "telephone")
    want = codec.to_host(y)
    plain = chat.infer(TEXTS, params_infer_code=_params(chat), **kw)
    for b in range(3):
        assert got[b].dtype == np.uint8 and got[b].tobytes() == G711.encode(float_to_int16(_strip(want[b])), "ulaw").tobytes(), b
        assert got[b].tobytes() != plain[b].tobytes(), "the high-pass changed nothing"
    # with the stages behind it: equalize, then compress, then the loudness stage with the limiter
    full = dict(compress=DEEP, loudness=TARGET, limiter=True)
    got = chat.infer(TEXTS, params_infer_code=_params(chat), eq="telephone", **kw, **full)
    z = codec.loudness_normalize(codec.compress(y, DEEP, rates=8000).contiguous(), TARGET, rates=8000, limiter=True)
    for g, w in zip(got, codec.to_host(z)):
        assert g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()
    per_row = chat.infer(TEXTS, params_infer_code=_params(chat), eq=["telephone", None, "telephone"], **kw)
    first = chat.infer(TEXTS, params_infer_code=_params(chat), eq="telephone", **kw)
    assert per_row[1].tobytes() == plain[1].tobytes() and per_row[0].tobytes() == first[0].tobytes() and per_row[2].tobytes() == first[2].tobytes()


def test_every_output_format_is_the_host_composition_behind_the_equalised_waveform(chat):
    codec = chat.codec
    rows = [torch.randn(t, 768, device=torch.device("cuda:0")) * 0.1 for t in (9, 14, 5)]
    wav1 = codec.decode_to_wavs(rows)
    y = codec.equalize(wav1, TONE)
    _within_an_ulp_of_the_definition(codec, wav1, y, 24000, TONE)
    want = codec.to_host(y)
    pcm = [float_to_int16(_strip(w)) for w in want]
    for got, enc in ((chat.decode_to_pcm16(rows, eq=TONE), lambda p: p), (chat.decode_to_pcm16(rows, encoding="ulaw", eq=TONE), lambda p: G711.encode(p, "ulaw")),
                     (chat.decode_to_pcm16(rows, encoding="alaw", eq=TONE), lambda p: G711.encode(p, "alaw")),
                     (chat.decode_to_pcm16(rows, flac=True, eq=TONE), lambda p: np.frombuffer(FLAC.encode(p, 24000), np.uint8)),
                     (chat.decode_to_pcm16(rows, adpcm=True, eq=TONE), lambda p: ADPCM.encode_result(p, 24000))):
        for g, p in zip(got, pcm):
            assert g.tobytes() == np.asarray(enc(p)).tobytes()
    assert np.asarray(chat.decode_to_wavs(rows, eq=TONE)).tobytes() == want.tobytes()
    # ragged, at another rate, with pauses in front and the rest of the chain behind: each row alone through the public stages
    got = chat.decode_to_pcm16(rows, ragged=True, sample_rate=8000, pauses=True, eq="telephone", compress=DEEP, loudness=TARGET, limiter=True)
    for g, r in zip(got, rows):
        w, off = codec.decode_ragged([r], sample_rate=8000)
        w, off = codec.trim_pauses(w, True, offsets=off, rates=8000)
        e = codec.equalize(w, "telephone", offsets=off, rates=8000)
        z = codec.loudness_normalize(codec.compress(e, DEEP, offsets=off, rates=8000), TARGET, offsets=off, rates=8000, limiter=True)
        assert g.tobytes() == float_to_int16(_strip(codec.to_host(z))).tobytes()
    # mixed per-row options: each as if alone, and a row that does not ask is the parent's
    specs, rates = ["telephone", None, TONE], [8000, 24000, 16000]
    mixed = chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, eq=specs, loudness=TARGET)
    for g, r, s, sr in zip(mixed, rows, specs, rates):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, loudness=TARGET, **({} if s is None else {"eq": s}))[0]
        assert g.tobytes() == alone.tobytes()
    assert mixed[1].tobytes() == chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, loudness=TARGET)[1].tobytes()
    with pytest.raises(ValueError, match="decode_ragged: highpass_hz is a number in 20 .. 3600"):      # a frequency against its own row's rate
        chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, eq={"highpass_hz": 4000})


def test_a_split_request_has_its_sentences_filtered_alone_from_zero_state(chat):
    codec = chat.codec
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), eq=TONE, loudness=TARGET, limiter=True,
                                                          ragged_decode=ragged, skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.decode_to_wavs([h])[0] for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch
            ws = [w for c in calls[1:] for w in codec.decode_to_wavs(c)]
        assert len(ws) == 3
        off = np.concatenate([[0], np.cumsum([w.numel() for w in ws])]).astype(np.int64)
        y = codec.equalize(torch.cat(ws), TONE, offsets=off)
        alone = torch.cat([codec.equalize(w.contiguous(), TONE) for w in ws])                          # every sentence from zero state
        assert codec.to_host(y).tobytes() == codec.to_host(alone).tobytes()
        for i, w in enumerate(ws):
            assert int(K.ulps(codec.to_host(y)[off[i]: off[i + 1]], EQ.apply(codec.to_host(w), 24000, TONE)).max()) <= 1
        z = codec.to_host(codec.loudness_normalize(y, TARGET, offsets=off, groups=[0, 3], limiter=True))
        want = float_to_int16(np.concatenate([_strip(z[off[i]: off[i + 1]]) for i in range(3)]))
        assert len(got) == 1 and got[0].tobytes() == want.tobytes(), ragged


def test_pooled_requests_with_and_without_the_equaliser_share_a_decode_and_equal_their_own_calls(chat):
    opts = [dict(loudness=TARGET, eq=TONE), dict(eq="telephone", sample_rate=8000, encoding="ulaw"), dict(loudness=TARGET), dict()]
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.hids = {}
    try:
        with b.lock:
            futs = [b.submit(TEXTS[0], _params(chat, 0, 24), **o) for o in opts]      # the same text: they finish at one poll
        got = [f.result(timeout=300) for f in futs]
        decodes = b.decode_calls
        with pytest.raises(TypeError):
            b.submit_stream(TEXTS[0], _params(chat, 0, 24), eq="telephone")
    finally:
        b.close()
    assert decodes == 1, "the four requests did not share one decode"
    for i, (g, o) in enumerate(zip(got, opts)):
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **o)[0]
        assert g.dtype == alone.dtype and g.tobytes() == alone.tobytes(), i
    w = chat.codec.decode_ragged([b.hids[futs[0].rid]])[0]
    z = chat.codec.loudness_normalize(chat.codec.equalize(w, TONE), TARGET)
    assert got[0].tobytes() == float_to_int16(_strip(chat.codec.to_host(z))).tobytes()


class _Catch(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.msgs = []

    def emit(self, record):
        self.msgs.append(record.getMessage())


def test_endpoint_serves_the_equaliser_when_asked_to_and_ignores_it_by_default(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        both = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, loudness=TARGET, eq=TONE)[0]
        tel = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, eq="telephone")[0]
        assert both.dtype == np.int16 and both.tobytes() != today.tobytes() and tel.tobytes() != today.tobytes()
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, loudness=True, eq=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "loudness": TARGET, "eq": TONE})
            assert r.status_code == 200 and _frames(r.content).tobytes() == both.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "eq": "telephone"}).content).tobytes() == tel.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "eq": False}).content).tobytes() == today.tobytes()
            r = c.post("/v1/audio/speech", json={**body, "eq": "telephone", "stream": True})
            assert r.status_code == 400 and "filter state carried across chunks" in r.text
            r = c.post("/v1/audio/speech", json={**body, "eq": {"highpass_hz": 5}})
            assert r.status_code == 400 and "highpass_hz is a number in 20 .. 10800" in r.text
            assert c.post("/v1/audio/speech", json={**body, "eq": "phone"}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "eq": {"peaks": [{"hz": 1000, "db": 1, "q": 1}] * 5}}).status_code == 400
            assert c.get("/health").json()["eq"] is True
        log, catch = logging.getLogger("test_gpu_equalizer_e2e.off"), _Catch()
        log.addHandler(catch)
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, logger=log)) as c:          # the switch off
            r = c.post("/v1/audio/speech", json={**body, "eq": "telephone"})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
            assert catch.msgs == ["ignoring unsupported parameters: ['eq']"] and "eq" not in c.get("/health").json()
    finally:
        chat.InferCodeParams = orig_params

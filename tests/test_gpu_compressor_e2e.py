"""`compress` end to end on the GPU: `Chat.infer(compress=)` and the decode calls against the public stage methods called by hand in
the chain's order (decode, compress, loudness_normalize with the limiter), through every output format, a split request, pooled
requests and the endpoint.  Synthetic weights, at most 32 tokens.  `pytest -m gpu`."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import adpcm as ADPCM  # noqa: E402
from chattts_amd import compressor as CP  # noqa: E402
from chattts_amd import flac as FLAC  # noqa: E402
from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from tests.test_gpu_loudness_e2e import SPLIT, TEXTS, _Recording, _frames, _hiddens_of, _params, _server_params, _strip, chat  # noqa: E402,F401

TARGET = -16.0
DEEP = {"threshold_db": -60, "ratio": 4, "hold_ms": 20}       # synthetic weights speak softly: a curve that reaches them whatever their level


def _by_hand(codec, wav, spec, rate=24000, **kw):
    """[B, n] or a pack through compress, then loudness + limiter: the chain's order, the public methods -> (float32 host rows, records)"""
    y, cst = codec.compress(wav, spec, rates=rate, return_stats=True, **kw)
    z = codec.loudness_normalize(y.contiguous(), TARGET, rates=rate, limiter=True, **kw)
    return codec.to_host(z), cst


def test_off_is_todays_call_bit_for_bit(chat):
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, ragged_decode=True), dict(loudness=-20.0, limiter=True, pcm16=True)):
        kw = dict(skip_refine_text=True, split_text=False, **kw)
        a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
        b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), compress=None, **kw)
        c = chat.infer(TEXTS[:2], params_infer_code=_params(chat), compress=[False, None], **kw)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b] == [x.tobytes() for x in c] and a[0].dtype == b[0].dtype
    with pytest.raises(ValueError, match="block state carried across chunks"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), compress=True)


@pytest.mark.parametrize("spec", [True, DEEP])
def test_infer_is_the_stages_by_hand_in_the_chains_order(chat, spec):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, compress=spec, loudness=TARGET, limiter=True)
    calls, pcm = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), pcm16=True, **kw))
    assert len(calls) == 1
    wav1 = codec.decode_to_wavs(calls[0])
    want, cst = _by_hand(codec, wav1, spec)
    twin = np.stack([CP.compress_segment(r, 24000, spec)[0] for r in codec.to_host(wav1)])
    assert codec.to_host(codec.compress(wav1, spec)).tobytes() == twin.tobytes()
    for b in range(3):
        print(f"row {b}: min_gain {cst['min_gain'][b]:.6g} n_blocks {cst['n_blocks'][b]} n_touched {cst['n_touched'][b]} peak {cst['peak'][b]:.6g}")
        assert pcm[b].dtype == np.int16 and pcm[b].tobytes() == float_to_int16(_strip(want[b])).tobytes(), b
    if spec is DEEP:
        assert int(cst["n_blocks"].sum()) > 0, "no row of this fixture reaches the curve: the compressor was not exercised"
    floats = chat.infer(TEXTS, params_infer_code=_params(chat), **kw)
    assert all(f.dtype == np.float32 and f.tobytes() == _strip(w).tobytes() for f, w in zip(floats, want))
    per_row = chat.infer(TEXTS, params_infer_code=_params(chat), pcm16=True, **{**kw, "compress": [spec, None, spec]})
    today = chat.infer(TEXTS, params_infer_code=_params(chat), pcm16=True, loudness=TARGET, limiter=True, skip_refine_text=True, split_text=False)
    assert per_row[1].tobytes() == today[1].tobytes() and per_row[0].tobytes() == pcm[0].tobytes() and per_row[2].tobytes() == pcm[2].tobytes()


def test_every_output_format_is_the_host_composition_behind_the_compressed_waveform(chat):
    codec = chat.codec
    rows = [torch.randn(t, 768, device=torch.device("cuda:0")) * 0.1 for t in (9, 14, 5)]
    base = dict(compress=DEEP, loudness=TARGET, limiter=True)
    wav1 = codec.decode_to_wavs(rows)
    want, _ = _by_hand(codec, wav1, DEEP)
    pcm = [float_to_int16(_strip(w)) for w in want]
    for got, enc in ((chat.decode_to_pcm16(rows, **base), lambda p: p), (chat.decode_to_pcm16(rows, encoding="ulaw", **base), lambda p: G711.encode(p, "ulaw")),
                     (chat.decode_to_pcm16(rows, encoding="alaw", **base), lambda p: G711.encode(p, "alaw")),
                     (chat.decode_to_pcm16(rows, flac=True, **base), lambda p: np.frombuffer(FLAC.encode(p, 24000), np.uint8)),
                     (chat.decode_to_pcm16(rows, adpcm=True, **base), lambda p: ADPCM.encode_result(p, 24000))):
        for g, p in zip(got, pcm):
            assert g.tobytes() == np.asarray(enc(p)).tobytes()
    # ragged, at another rate, with pauses in front: each row alone through the public stages
    got = chat.decode_to_pcm16(rows, ragged=True, sample_rate=8000, pauses=True, **base)
    for g, r in zip(got, rows):
        w, off = codec.decode_ragged([r], sample_rate=8000)
        w, off = codec.trim_pauses(w, True, offsets=off, rates=8000)
        y = codec.compress(w, DEEP, offsets=off, rates=8000)
        assert codec.to_host(y).tobytes() == CP.compress_segment(codec.to_host(w), 8000, DEEP)[0].tobytes()
        z = codec.loudness_normalize(y, TARGET, offsets=off, rates=8000, limiter=True)
        assert g.tobytes() == float_to_int16(_strip(codec.to_host(z))).tobytes()
    # mixed per-row options: each as if alone, and a row that does not ask is the parent's
    specs, rates = [DEEP, None, True], [8000, 24000, 16000]
    mixed = chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, compress=specs, loudness=TARGET)
    for g, r, s, sr in zip(mixed, rows, specs, rates):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, loudness=TARGET, **({} if s is None else {"compress": s}))[0]
        assert g.tobytes() == alone.tobytes()
    assert mixed[1].tobytes() == chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, loudness=TARGET)[1].tobytes()
    f32 = chat.decode_to_wavs(rows, compress=DEEP)
    assert np.asarray(f32).tobytes() == codec.to_host(codec.compress(wav1, DEEP)).tobytes()


def test_a_split_request_has_its_sentences_compressed_alone(chat):
    codec = chat.codec
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), compress=DEEP, loudness=TARGET, limiter=True,
                                                          ragged_decode=ragged, skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.decode_to_wavs([h])[0] for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch
            ws = [w for c in calls[1:] for w in codec.decode_to_wavs(c)]
        assert len(ws) == 3
        off = np.concatenate([[0], np.cumsum([w.numel() for w in ws])]).astype(np.int64)
        y = codec.compress(torch.cat(ws), DEEP, offsets=off)
        assert codec.to_host(y).tobytes() == np.concatenate([CP.compress_segment(codec.to_host(w), 24000, DEEP)[0] for w in ws]).tobytes()
        z = codec.to_host(codec.loudness_normalize(y, TARGET, offsets=off, groups=[0, 3], limiter=True))
        want = float_to_int16(np.concatenate([_strip(z[off[i]: off[i + 1]]) for i in range(3)]))
        assert len(got) == 1 and got[0].tobytes() == want.tobytes(), ragged


def test_pooled_requests_with_and_without_the_compressor_share_a_decode_and_equal_their_own_calls(chat):
    opts = [dict(loudness=TARGET, compress=DEEP), dict(compress=True), dict(loudness=TARGET), dict()]
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.hids = {}
    try:
        with b.lock:
            futs = [b.submit(TEXTS[0], _params(chat, 0, 24), **o) for o in opts]      # the same text: they finish at one poll
        got = [f.result(timeout=300) for f in futs]
        decodes = b.decode_calls
        with pytest.raises(TypeError):
            b.submit_stream(TEXTS[0], _params(chat, 0, 24), compress=True)
    finally:
        b.close()
    assert decodes == 1, "the four requests did not share one decode"
    for i, (g, o) in enumerate(zip(got, opts)):
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **o)[0]
        assert g.dtype == np.int16 and g.tobytes() == alone.tobytes(), i
    w = chat.codec.decode_ragged([b.hids[futs[0].rid]])[0]
    z = chat.codec.loudness_normalize(chat.codec.compress(w, DEEP), TARGET)
    assert got[0].tobytes() == float_to_int16(_strip(chat.codec.to_host(z))).tobytes()


def test_endpoint_serves_the_compressor_when_asked_to_and_ignores_it_by_default(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        both = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, loudness=TARGET, compress=DEEP)[0]
        comp = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, compress=True)[0]
        assert both.dtype == np.int16 and both.tobytes() != today.tobytes()
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, loudness=True, compress=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "loudness": TARGET, "compress": DEEP})
            assert r.status_code == 200 and _frames(r.content).tobytes() == both.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "compress": True}).content).tobytes() == comp.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "compress": False}).content).tobytes() == today.tobytes()
            assert c.post("/v1/audio/speech", json={**body, "compress": True, "stream": True}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "compress": {"ratio": 1}}).status_code == 400
            assert c.get("/health").json()["compress"] is True
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            r = c.post("/v1/audio/speech", json={**body, "compress": True})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
    finally:
        chat.InferCodeParams = orig_params

"""`limiter` end to end on the GPU: `Chat.infer(limiter=)` against the NumPy twin (chattts_amd/limiter.py) applied to the float32 path's
own waveform at the device's own gain, through every output format, a split request, pooled requests and the endpoint.  Synthetic
weights, at most 32 tokens.  `pytest -m gpu`."""
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import flac as FLAC  # noqa: E402
from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd import limiter as LM  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from tests.test_gpu_loudness_e2e import SPLIT, TEXTS, _Recording, _frames, _hiddens_of, _params, _server_params, _strip, chat  # noqa: E402,F401

TARGET = -8.0
PEAK16 = int(round(float(LM.C32) * 32767))          # no 16-bit sample of a limited row lies beyond it


def _twin_rows(x, rate, g32):
    """the twin limiter over the rows of x [B, n] at the gains g32 -> (float32 [B, n], records)"""
    res = [LM.limit_segment(x[b], rate, g32[b]) for b in range(len(x))]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=LM.STATS)


def test_off_is_todays_call_bit_for_bit(chat):
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, ragged_decode=True), dict(loudness=-20.0, pcm16=True)):
        kw = dict(skip_refine_text=True, split_text=False, **kw)
        a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
        b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), limiter=None, **kw)
        c = chat.infer(TEXTS[:2], params_infer_code=_params(chat), limiter=[False, False], **kw)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b] == [x.tobytes() for x in c] and a[0].dtype == b[0].dtype
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), limiter=True)


def test_pcm16_stays_under_the_ceiling_and_is_the_twin_on_the_float_path(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False)
    calls, pcm = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), loudness=TARGET, limiter=True, pcm16=True, **kw))
    assert len(calls) == 1
    wav1 = codec.decode_to_wavs(calls[0])
    x = codec.to_host(wav1)
    y_d, st, ls = codec.loudness_normalize(wav1, TARGET, return_stats=True, limiter=True)
    _, st0 = codec.loudness_normalize(wav1, TARGET, return_stats=True)
    want, recs = _twin_rows(x, 24000, st["g32"])
    for b in range(3):
        print(f"row {b}: g32 {st['g32'][b]:.6g} (ceiling alone {st0['g32'][b]:.6g}, bound {st0['bound'][b]}) n_over {ls['n_over'][b]} "
              f"n_touched {ls['n_touched'][b]} min_gain {ls['min_gain'][b]:.6g}")
    assert ls.tobytes() == recs.tobytes() and codec.to_host(y_d).tobytes() == want.tobytes()
    assert np.all(st["bound"] != 2) and np.all(st["g32"] >= st0["g32"]) and np.array_equal(st["L"], st0["L"])
    assert int(ls["n_over"].sum()) > 0, "no row of this fixture reaches the threshold: the limiter was not exercised"
    for b in range(3):
        assert pcm[b].dtype == np.int16 and int(np.abs(pcm[b].astype(np.int32)).max()) <= PEAK16
        assert pcm[b].tobytes() == float_to_int16(_strip(want[b])).tobytes(), b
    floats = chat.infer(TEXTS, params_infer_code=_params(chat), loudness=TARGET, limiter=True, **kw)
    assert all(f.dtype == np.float32 and f.tobytes() == _strip(w).tobytes() and np.abs(f).max() <= LM.C32 for f, w in zip(floats, want))
    # without `loudness`: unity gain; per-row flags: a row that does not ask is today's
    unity, _ = _twin_rows(np.float32(3) * x, 24000, np.ones(3, np.float32))
    assert codec.to_host(codec.peak_limit(wav1 * 3, rates=24000)).tobytes() == unity.tobytes() and np.abs(unity).max() <= LM.C32
    alone, _ = _twin_rows(x, 24000, np.ones(3, np.float32))
    per_row = chat.infer(TEXTS, params_infer_code=_params(chat), limiter=[True, False, True], pcm16=True, **kw)
    today = chat.infer(TEXTS, params_infer_code=_params(chat), pcm16=True, **kw)
    assert per_row[1].tobytes() == today[1].tobytes()
    assert per_row[0].tobytes() == float_to_int16(_strip(alone[0])).tobytes() and per_row[2].tobytes() == float_to_int16(_strip(alone[2])).tobytes()


def test_every_output_format_is_the_host_composition_behind_the_limited_waveform(chat):
    codec = chat.codec
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True, loudness=TARGET, limiter=True)
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), encoding="ulaw", **kw))
    wav1 = codec.decode_to_wavs(calls[0])
    _, st, _ = codec.loudness_normalize(wav1, TARGET, return_stats=True, limiter=True)
    want, _ = _twin_rows(codec.to_host(wav1), 24000, st["g32"])
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()
    got = chat.infer(TEXTS, params_infer_code=_params(chat), flac=True, **kw)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.tobytes() == FLAC.encode(float_to_int16(_strip(w)), 24000)
    for ragged in (False, True):                                                              # behind the resampler, at ITS rate: W = 80
        got = chat.infer(TEXTS, params_infer_code=_params(chat), sample_rate=8000, ragged_decode=ragged, **kw)
        if ragged:
            ws = [codec.resample(codec.decode_to_wavs([h]), 24000, 8000)[0] for h in calls[0]]
        else:
            ws = list(codec.resample(wav1, 24000, 8000))
        for g, w in zip(got, ws):
            _, s8, _ = codec.loudness_normalize(w.contiguous(), TARGET, rates=8000, return_stats=True, limiter=True)
            w8 = LM.limit_segment(codec.to_host(w), 8000, s8["g32"][0])[0]
            assert g.tobytes() == float_to_int16(_strip(w8)).tobytes(), ragged
            assert int(np.abs(g.astype(np.int32)).max()) <= PEAK16
    # ragged rows with mixed options: each as if alone, and a row that does not ask for the limiter is the parent's
    rows = [torch.randn(t, 768, device=torch.device("cuda:0")) * 0.1 for t in (9, 14, 5)]
    tg, rates, encs, lim = [TARGET, None, -30.0], [8000, 24000, 16000], ["ulaw", None, None], [True, True, False]
    mixed = chat.decode_to_pcm16(rows, ragged=True, loudness=tg, sample_rate=rates, encoding=encs, limiter=lim)
    for g, r, t, sr, e, m in zip(mixed, rows, tg, rates, encs, lim):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, **({} if t is None else {"loudness": t}), **({} if e is None else {"encoding": e}),
                                     **({"limiter": True} if m else {}))[0]
        assert g.dtype == alone.dtype and g.tobytes() == alone.tobytes()
    today = chat.decode_to_pcm16(rows, ragged=True, loudness=tg, sample_rate=rates, encoding=encs)
    assert mixed[2].tobytes() == today[2].tobytes()
    flacs = chat.decode_to_pcm16(rows, ragged=True, loudness=TARGET, limiter=True, flac=[True, False, True])
    plain = chat.decode_to_pcm16(rows, ragged=True, loudness=TARGET, limiter=True)
    assert flacs[1].tobytes() == plain[1].tobytes() and flacs[0].tobytes() == FLAC.encode(plain[0], 24000) and flacs[2].tobytes() == FLAC.encode(plain[2], 24000)
    assert all(int(np.abs(p.astype(np.int32)).max()) <= PEAK16 for p in plain)


def test_a_split_request_gets_one_gain_and_the_limiter_per_sentence(chat):
    codec = chat.codec
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), loudness=TARGET, limiter=True, ragged_decode=ragged,
                                                          skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.decode_to_wavs([h])[0] for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch
            ws = [w for c in calls[1:] for w in codec.decode_to_wavs(c)]
        assert len(ws) == 3
        off = np.concatenate([[0], np.cumsum([w.numel() for w in ws])]).astype(np.int64)
        _, st, ls = codec.loudness_normalize(torch.cat(ws), TARGET, offsets=off, groups=[0, 3], return_stats=True, limiter=True)
        assert len(st) == 1 and st["bound"][0] in (0, 1) and np.all(ls["g32"] == st["g32"][0])
        ys = [LM.limit_segment(codec.to_host(w), 24000, st["g32"][0]) for w in ws]                 # every sentence alone at the ONE gain
        assert ls.tobytes() == np.array([r for _, r in ys], dtype=LM.STATS).tobytes()
        want = float_to_int16(np.concatenate([_strip(y) for y, _ in ys]))
        assert len(got) == 1 and got[0].tobytes() == want.tobytes(), ragged
        assert int(np.abs(got[0].astype(np.int32)).max()) <= PEAK16
    floats = chat.infer(SPLIT, params_infer_code=_params(chat), loudness=TARGET, limiter=True, skip_refine_text=True, split_text=True)
    assert len(floats) == 1 and float_to_int16(floats[0]).tobytes() == got[0].tobytes()


def test_pooled_requests_with_and_without_the_limiter_share_a_decode_and_equal_their_own_calls(chat):
    opts = [dict(loudness=TARGET, limiter=True), dict(limiter=True), dict(loudness=TARGET), dict()]
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.hids = {}
    try:
        with b.lock:
            futs = [b.submit(TEXTS[0], _params(chat, 0, 24), **o) for o in opts]      # the same text: they finish at one poll
        got = [f.result(timeout=300) for f in futs]
        decodes = b.decode_calls
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream(TEXTS[0], _params(chat, 0, 24), limiter=True)
    finally:
        b.close()
    assert decodes == 1, "the four requests did not share one decode"
    for i, (g, o) in enumerate(zip(got, opts)):
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **o)[0]
        assert g.dtype == np.int16 and g.tobytes() == alone.tobytes(), i
    assert int(np.abs(got[0].astype(np.int32)).max()) <= PEAK16 and int(np.abs(got[1].astype(np.int32)).max()) <= PEAK16
    hid = b.hids[futs[0].rid]
    w = chat.codec.decode_ragged([hid])[0]
    _, st, _ = chat.codec.loudness_normalize(w, TARGET, return_stats=True, limiter=True)
    want = LM.limit_segment(chat.codec.to_host(w), 24000, st["g32"][0])[0]
    assert got[0].tobytes() == float_to_int16(_strip(want)).tobytes()


def test_endpoint_serves_the_limiter_when_asked_to_and_ignores_it_by_default(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        both = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, loudness=TARGET, limiter=True)[0]
        lim = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, limiter=True)[0]
        assert both.dtype == np.int16 and both.tobytes() != today.tobytes() and int(np.abs(both.astype(np.int32)).max()) <= PEAK16
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, loudness=True, limiter=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "loudness": TARGET, "limiter": True})
            assert r.status_code == 200 and _frames(r.content).tobytes() == both.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "limiter": True}).content).tobytes() == lim.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert _frames(c.post("/v1/audio/speech", json={**body, "limiter": False}).content).tobytes() == today.tobytes()
            assert c.post("/v1/audio/speech", json={**body, "limiter": True, "stream": True}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "limiter": "yes"}).status_code == 400
            assert c.get("/health").json()["limiter"] is True
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            r = c.post("/v1/audio/speech", json={**body, "limiter": True})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
    finally:
        chat.InferCodeParams = orig_params

"""FLAC output end to end on the GPU.  The one invariant: on every non-streamed path that yields PCM16, `flac=True` yields a file that the
independent decoder (tests/flac_oracle.py) reads back as exactly the int16 array the same seeded call yields without it, at the call's
rate, within `flac.bound` -- the serial call at 24 kHz, at 8 kHz and at speed 1.25, ragged decode with mixed flags per row (and a
companded row beside them), split requests on the device and on the host, pooled requests beside a plain one in one poll, and the
endpoint.  Synthetic weights, at most 32 tokens.  `pytest -m gpu`."""
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import flac, g711, weights as W  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests import flac_oracle  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there."]
SPLIT = "Hello there. How are you. Fine."


@pytest.fixture(scope="module")
def chat(weights):
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts={**weights, "dvae": W.synthetic_dvae()}, device=DEV, dtype="f32", tokenizer=os.path.join(GOLD, "tokenizer"),
                  spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voice = c.sample_random_speaker()
    return c


def _params(chat, i=0, **kw):
    return chat.InferCodeParams(top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=[24, 32, 16][i % 3], show_tqdm=False,
                                manual_seed=300 + 7 * i, spk_emb=chat.test_voice, **kw)


def _is_file_of(got, pcm, rate, what):
    got, pcm = np.asarray(got), np.asarray(pcm)
    assert pcm.dtype == np.int16 and got.dtype == np.uint8 and got.ndim == 1, (what, got.dtype, pcm.dtype)
    assert got.size <= flac.bound(pcm.size), (what, got.size, pcm.size)
    y, r = flac_oracle.decode(got.tobytes())
    assert r == rate and y.dtype == np.int16 and np.array_equal(y, pcm), (what, r, y.shape, pcm.shape)
    assert got.tobytes() == flac.encode(pcm, rate), what           # and byte for byte the twin's file


@pytest.mark.parametrize("more,rate", [({}, 24000), ({"sample_rate": 8000}, 8000), ({"speed": 1.25}, 24000),
                                        ({"ragged_decode": True, "sample_rate": 8000, "speed": 1.25}, 8000)])
def test_serial_calls_decode_to_the_pcm16_samples(chat, more, rate):
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    pcm = chat.infer(TEXTS, params_infer_code=_params(chat), **kw, **more)
    got = chat.infer(TEXTS, params_infer_code=_params(chat), flac=True, **kw, **more)
    assert len(pcm) == len(got) == 3 and all(p.size > 0 for p in pcm)
    for k, (g, p) in enumerate(zip(got, pcm)):
        _is_file_of(g, p, rate, (more, k))


def test_split_requests_on_the_device_and_on_the_host(chat):
    skw = dict(skip_refine_text=True, split_text=True, pcm16=True)
    for more, rate in (({"ragged_decode": True}, 24000), ({"ragged_decode": True, "sample_rate": 8000}, 8000), ({}, 24000)):
        pcm = chat.infer(SPLIT, params_infer_code=_params(chat), **skw, **more)        # {}: the host's concatenation, the host twin
        got = chat.infer(SPLIT, params_infer_code=_params(chat), flac=True, **skw, **more)
        assert len(pcm) == len(got) == 1 and pcm[0].size > 0
        _is_file_of(got[0], pcm[0], rate, ("split", more))


def test_mixed_flags_per_row_and_per_request(chat):
    """decode_to_pcm16(ragged) and decode_split_to_pcm16 with one flag per row / request, at one rate and at mixed rates, stripped and
    not; a companded row beside the files; rows without the flag are untouched"""
    g = torch.Generator(device=DEV).manual_seed(5)
    rows = [torch.randn((n, 768), device=DEV, generator=g) * 0.5 for n in (9, 24, 5, 17)]
    flags = [True, False, True, True]
    for rate in (None, [8000, 24000, 16000, 8000]):
        rkw = {} if rate is None else {"sample_rate": rate}
        rates = [24000] * 4 if rate is None else rate
        for strip in (True, False):
            pcm = chat.decode_to_pcm16(rows, ragged=True, strip=strip, **rkw)
            got = chat.decode_to_pcm16(rows, ragged=True, strip=strip, flac=flags, **rkw)
            for k, (a, p, f) in enumerate(zip(got, pcm, flags)):
                if f:
                    _is_file_of(a, p, rates[k], (rate, strip, k))
                else:
                    assert a.dtype == np.int16 and a.tobytes() == p.tobytes(), (rate, strip, k)
        groups = [rows[:2], rows[2:3], rows[3:]]
        grate = {} if rate is None else {"sample_rate": [8000, 16000, 24000]}
        grates = [24000] * 3 if rate is None else [8000, 16000, 24000]
        pcm = chat.decode_split_to_pcm16(groups, **grate)
        for gf in (True, [False, True, True]):
            got = chat.decode_split_to_pcm16(groups, flac=gf, **grate)
            for k, (a, p) in enumerate(zip(got, pcm)):
                if gf is True or gf[k]:
                    _is_file_of(a, p, grates[k], (rate, gf, k))
                else:
                    assert a.dtype == np.int16 and a.tobytes() == p.tobytes(), (rate, gf, k)
    pcm = chat.decode_to_pcm16(rows, ragged=True)
    got = chat.decode_to_pcm16(rows, ragged=True, flac=[True, False, False, True], encoding=[None, "ulaw", None, None])
    _is_file_of(got[0], pcm[0], 24000, "beside a companded row")
    _is_file_of(got[3], pcm[3], 24000, "beside a companded row")
    assert got[1].dtype == np.uint8 and got[1].tobytes() == g711.encode(pcm[1], "ulaw").tobytes() and got[2].tobytes() == pcm[2].tobytes()
    padded = chat.decode_to_pcm16(rows, strip=True)                  # the padded batch
    for k, (a, p) in enumerate(zip(chat.decode_to_pcm16(rows, strip=True, flac=True), padded)):
        _is_file_of(a, p, 24000, ("padded", k))
    assert all(a.tobytes() == p.tobytes() for a, p in zip(chat.decode_to_pcm16(rows, strip=True, flac=False), padded))
    with pytest.raises(ValueError, match="encoding"):
        chat.decode_to_pcm16(rows, ragged=True, flac=True, encoding="ulaw")
    with pytest.raises(ValueError, match="ragged"):
        chat.decode_to_pcm16(rows, flac=flags)


def test_pooled_requests_with_and_without_flac_in_one_poll(chat):
    """three requests that finish together (ragged_decode): plain at 24 kHz, FLAC at 8 kHz, FLAC at 24 kHz == the same batch without the
    flag; then one request decoded alone (no ragged_decode): the host twin's file"""
    plan = [(False, None), (True, 8000), (True, None)]

    def run(with_flac, ragged=True):
        b = SpeechBatcher(chat, 4, threading.Lock(), ragged_decode=ragged)
        try:
            with b.lock:
                futs = [b.submit(t, _params(chat, i), sample_rate=r, **({"flac": True} if with_flac and f else {}))
                        for i, (t, (f, r)) in enumerate(zip(TEXTS, plan))]
            return [f.result(timeout=300) for f in futs], b.occupancy()
        finally:
            b.close()
    pcm, occ0 = run(False)
    got, occ = run(True)
    assert occ0["flac_encoded"] == 0 and occ["flac_encoded"] == 2 and occ["decode_calls"] == occ0["decode_calls"]
    for k, (g, p, (f, r)) in enumerate(zip(got, pcm, plan)):
        if f:
            _is_file_of(g, p, r or 24000, ("pooled", k))
        else:
            assert g.dtype == np.int16 and g.size > 0 and g.tobytes() == p.tobytes(), k
    alone_pcm, _ = run(False, ragged=False)
    alone, _ = run(True, ragged=False)
    for k, (g, p, (f, r)) in enumerate(zip(alone, alone_pcm, plan)):
        if f:
            _is_file_of(g, p, r or 24000, ("alone", k))


def test_endpoint_flac_body_decodes_to_the_wav_bodys_samples(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 32})     # (random weights do not emit EOS on cue)
    try:
        app = server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 24000), speed=True, flac=True)
        with TestClient(app) as c:
            assert "flac" in c.get("/health").json()["formats"]
            for body, rate in (({"input": TEXTS[0]}, 24000), ({"input": TEXTS[0], "sample_rate": 8000, "speed": 1.25}, 8000)):
                wav = c.post("/v1/audio/speech", json={**body, "response_format": "wav"})
                fl = c.post("/v1/audio/speech", json={**body, "response_format": "flac"})
                assert wav.status_code == 200 and fl.status_code == 200 and fl.headers["content-type"] == "audio/flac"
                samples = np.frombuffer(wav.content[44:], "<i2")
                y, r, facts = flac_oracle.decode(fl.content, info=True)
                assert r == rate == int.from_bytes(wav.content[24:28], "little") and samples.size > 0 and np.array_equal(y, samples)
                assert facts["rate"] == rate and facts["total"] == samples.size and len(fl.content) <= flac.bound(samples.size)
            assert c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "flac", "stream": True}).status_code == 400
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            assert c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "flac"}).status_code == 400
    finally:
        chat.InferCodeParams = orig_params

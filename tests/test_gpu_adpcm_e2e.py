"""IMA ADPCM output end to end on the GPU.  The one invariant: on every non-streamed path that yields PCM16, `adpcm=True` yields the
complete WAV file `adpcm.encode` makes of exactly the int16 array the same seeded call yields without it, at the call's rate -- the
serial call at 24 kHz and at 8 kHz, ragged decode, with loudness and limiter on, split requests on the device and on the host, flags
per row and per request, pooled requests beside a plain one in one poll, the endpoint, and an ADPCM clip as a cloned voice.  Synthetic
weights, at most 32 tokens.  `pytest -m gpu`."""
import os
import struct
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import adpcm, g711, weights as W  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402

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
    assert pcm.dtype == np.int16 and got.dtype == np.uint8 and got.ndim == 1 and pcm.size > 0, (what, got.dtype, pcm.dtype, pcm.size)
    assert got.size == 60 + adpcm.n_blocks(pcm.size, rate) * adpcm.align(rate), (what, got.size, pcm.size)
    assert struct.unpack_from("<HHI", got.tobytes(), 20) == (0x11, 1, rate) and struct.unpack_from("<I", got.tobytes(), 48)[0] == pcm.size, what
    assert got.tobytes() == adpcm.encode(pcm, rate), what            # byte for byte the twin's file of the same samples


@pytest.mark.parametrize("more,rate", [({}, 24000), ({"sample_rate": 8000}, 8000), ({"ragged_decode": True}, 24000),
                                        ({"ragged_decode": True, "sample_rate": 8000, "speed": 1.25, "loudness": -20.0, "limiter": True}, 8000)])
def test_serial_calls_are_the_files_of_the_pcm16_samples(chat, more, rate):
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    pcm = chat.infer(TEXTS, params_infer_code=_params(chat), **kw, **more)
    got = chat.infer(TEXTS, params_infer_code=_params(chat), adpcm=True, **kw, **more)
    assert len(pcm) == len(got) == 3
    for k, (g, p) in enumerate(zip(got, pcm)):
        _is_file_of(g, p, rate, (more, k))


def test_split_requests_on_the_device_and_on_the_host(chat):
    skw = dict(skip_refine_text=True, split_text=True, pcm16=True)
    for more, rate in (({"ragged_decode": True}, 24000), ({"ragged_decode": True, "sample_rate": 8000}, 8000), ({}, 24000)):
        pcm = chat.infer(SPLIT, params_infer_code=_params(chat), **skw, **more)        # {}: the host's concatenation, the host twin
        got = chat.infer(SPLIT, params_infer_code=_params(chat), adpcm=True, **skw, **more)
        assert len(pcm) == len(got) == 1
        _is_file_of(got[0], pcm[0], rate, ("split", more))                             # ONE file over the concatenated sentences


def test_flags_per_row_and_per_request(chat):
    """decode_to_pcm16(ragged) and decode_split_to_pcm16 with one flag per row / request, at one rate and at mixed rates, stripped and
    not; a companded row beside the files; rows without the flag are today's int16 arrays, bit for bit"""
    g = torch.Generator(device=DEV).manual_seed(5)
    rows = [torch.randn((n, 768), device=DEV, generator=g) * 0.5 for n in (9, 24, 5, 17)]
    flags = [True, False, True, True]
    for rate in (None, [8000, 24000, 48000, 8000]):
        rkw = {} if rate is None else {"sample_rate": rate}
        rates = [24000] * 4 if rate is None else rate
        for strip in (True, False):
            pcm = chat.decode_to_pcm16(rows, ragged=True, strip=strip, **rkw)
            got = chat.decode_to_pcm16(rows, ragged=True, strip=strip, adpcm=flags, **rkw)
            for k, (a, p, f) in enumerate(zip(got, pcm, flags)):
                if f:
                    _is_file_of(a, p, rates[k], (rate, strip, k))
                else:
                    assert a.dtype == np.int16 and a.tobytes() == p.tobytes(), (rate, strip, k)
        groups = [rows[:2], rows[2:3], rows[3:]]
        grate = {} if rate is None else {"sample_rate": [8000, 48000, 24000]}
        grates = [24000] * 3 if rate is None else [8000, 48000, 24000]
        pcm = chat.decode_split_to_pcm16(groups, **grate)
        for gf in (True, [False, True, True]):
            got = chat.decode_split_to_pcm16(groups, adpcm=gf, **grate)
            for k, (a, p) in enumerate(zip(got, pcm)):
                if gf is True or gf[k]:
                    _is_file_of(a, p, grates[k], (rate, gf, k))
                else:
                    assert a.dtype == np.int16 and a.tobytes() == p.tobytes(), (rate, gf, k)
    pcm = chat.decode_to_pcm16(rows, ragged=True)
    got = chat.decode_to_pcm16(rows, ragged=True, adpcm=[True, False, False, True], encoding=[None, "ulaw", None, None])
    _is_file_of(got[0], pcm[0], 24000, "beside a companded row")
    _is_file_of(got[3], pcm[3], 24000, "beside a companded row")
    assert got[1].dtype == np.uint8 and got[1].tobytes() == g711.encode(pcm[1], "ulaw").tobytes() and got[2].tobytes() == pcm[2].tobytes()
    padded = chat.decode_to_pcm16(rows, strip=True)                  # the padded batch
    for k, (a, p) in enumerate(zip(chat.decode_to_pcm16(rows, strip=True, adpcm=True), padded)):
        _is_file_of(a, p, 24000, ("padded", k))
    assert all(a.tobytes() == p.tobytes() for a, p in zip(chat.decode_to_pcm16(rows, strip=True, adpcm=False), padded))
    with pytest.raises(ValueError, match="encoding"):
        chat.decode_to_pcm16(rows, ragged=True, adpcm=True, encoding="ulaw")
    with pytest.raises(ValueError, match="flac"):
        chat.decode_to_pcm16(rows, ragged=True, adpcm=[True, False, False, False], flac=[False, True, False, False])
    with pytest.raises(ValueError, match="ragged"):
        chat.decode_to_pcm16(rows, adpcm=flags)
    with pytest.raises(ValueError, match="one adpcm flag"):
        chat.decode_split_to_pcm16([rows[:2], rows[2:]], adpcm=[True])


def test_pooled_requests_with_and_without_adpcm_in_one_poll(chat):
    """three requests that finish together (ragged_decode): plain at 24 kHz, ADPCM at 8 kHz, ADPCM at 24 kHz == the same batch without
    the flag; then the same requests decoded alone (no ragged_decode): the host twin's files"""
    plan = [(False, None), (True, 8000), (True, None)]

    def run(with_adpcm, ragged=True):
        b = SpeechBatcher(chat, 4, threading.Lock(), ragged_decode=ragged)
        try:
            with b.lock:
                futs = [b.submit(t, _params(chat, i), sample_rate=r, **({"adpcm": True} if with_adpcm and f else {}))
                        for i, (t, (f, r)) in enumerate(zip(TEXTS, plan))]
            return [f.result(timeout=300) for f in futs], b.occupancy()
        finally:
            b.close()
    pcm, occ0 = run(False)
    got, occ = run(True)
    assert "adpcm_encoded" not in occ0 and occ["adpcm_encoded"] == 2 and occ["decode_calls"] == occ0["decode_calls"]
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


def test_endpoint_bytes_the_switch_and_an_adpcm_clip_as_a_voice(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 32})     # (random weights do not emit EOS on cue)
    smps = []
    orig_clone = chat.sample_audio_speaker
    chat.sample_audio_speaker = lambda wav, rate=None: (smps.append(orig_clone(wav, rate)), smps[-1])[1]
    try:
        p = orig_params(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=32, min_new_token=0,
                        show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice, stream_batch=24, stream_speed=12000,
                        pass_first_n_batches=2)
        serial = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, adpcm=True, params_infer_code=p, sample_rate=8000)[0]
        app = server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 24000), adpcm=True, voice_upload=True)
        with TestClient(app) as c:
            assert "adpcm" in c.get("/health").json()["formats"]
            for body, rate in (({"input": TEXTS[0]}, 24000), ({"input": TEXTS[0], "sample_rate": 8000}, 8000)):
                wav = c.post("/v1/audio/speech", json={**body, "response_format": "wav"})
                ad = c.post("/v1/audio/speech", json={**body, "response_format": "adpcm"})
                assert wav.status_code == 200 and ad.status_code == 200 and ad.headers["content-type"] == "audio/wav"
                samples = np.frombuffer(wav.content[44:], "<i2")
                assert samples.size > 0 and ad.content == adpcm.encode(samples, rate)
            assert ad.content == serial.tobytes()                                          # the endpoint's bytes are the serial call's
            assert c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "adpcm", "stream": True}).status_code == 400
            # the endpoint's own ADPCM file as a voice == the PCM16 file of its decoded samples as a voice
            up = c.post("/v1/audio/voices", params={"name": "small"}, content=ad.content)
            assert up.status_code == 200 and up.json()["sample_rate"] == 8000 and up.json()["tokens"] > 0, up.text
            lin, _ = adpcm.parse_wav(ad.content)
            up2 = c.post("/v1/audio/voices", params={"name": "lin"}, content=server.pcm16_to_wav_bytes(lin, 8000))
            assert up2.status_code == 200 and up2.json()["tokens"] == up.json()["tokens"]
            assert len(smps) == 2 and smps[0] == smps[1]
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 24000), voice_upload=True)) as c:
            r = c.post("/v1/audio/speech", json={"input": TEXTS[0], "response_format": "adpcm"})
            assert r.status_code == 400 and "Unsupported audio format: adpcm, supported formats: " in r.text
            assert "adpcm" not in c.get("/health").json()["formats"]
            assert c.post("/v1/audio/voices", params={"name": "small"}, content=ad.content).status_code == 400
    finally:
        chat.InferCodeParams = orig_params
        del chat.sample_audio_speaker

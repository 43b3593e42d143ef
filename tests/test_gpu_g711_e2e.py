"""G.711 output end to end on the GPU.  The one invariant: on every path that yields PCM16, `encoding=` yields exactly `g711.encode` of
the int16 array the same seeded call yields without it -- the serial call, ragged decode, the grouped conversion of a split request, the
serial stream at 8 kHz chunk by chunk, pooled streams against their serial compositions over the pool's hidden states, pooled requests
with mixed encodings, and the endpoint (raw and WAV bodies, and its own mu-law WAV uploaded as a voice).  Synthetic weights, at most 80
tokens.  `pytest -m gpu`."""
import os
import struct
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import audio, engine as E, g711, weights as W  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, SpeechBatcher, StreamEvents, StreamSpec  # noqa: E402
from tests.test_gpu_stream_pool import _alone_stream, _engine  # noqa: E402
from tests.test_gpu_stream_resample import _serial_chunks_rate  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there."]
SPLIT = "Hello there. How are you. Fine."


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def chat(request, weights):
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


def _same(got, pcm, law, what):
    assert len(got) == len(pcm) > 0, what
    for k, (g, p) in enumerate(zip(got, pcm)):
        g, p = np.asarray(g), np.asarray(p)
        assert p.dtype == np.int16 and g.dtype == np.uint8 and g.shape == p.shape, (what, k, g.dtype, g.shape, p.shape)
        assert g.tobytes() == g711.encode(p, law).tobytes(), (what, k)


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_serial_ragged_and_split_calls_equal_the_companded_pcm16(chat, law):
    kw = dict(skip_refine_text=True, split_text=False, pcm16=True)
    for more in ({}, {"sample_rate": 8000}, {"ragged_decode": True}, {"ragged_decode": True, "sample_rate": 8000}):
        pcm = chat.infer(TEXTS, params_infer_code=_params(chat), **kw, **more)
        got = chat.infer(TEXTS, params_infer_code=_params(chat), encoding=law, **kw, **more)
        assert len(pcm) == 3 and sum(p.size for p in pcm) > 0
        _same(got, pcm, law, more)
    skw = dict(skip_refine_text=True, split_text=True, pcm16=True)
    for more in ({"ragged_decode": True}, {"ragged_decode": True, "sample_rate": 8000}, {}):      # the grouped conversion; {}: the host's concatenation
        pcm = chat.infer(SPLIT, params_infer_code=_params(chat), **skw, **more)
        got = chat.infer(SPLIT, params_infer_code=_params(chat), encoding=law, **skw, **more)
        assert len(pcm) == 1 and pcm[0].size > 0
        _same(got, pcm, law, ("split", more))
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(TEXTS, params_infer_code=_params(chat), skip_refine_text=True, encoding=law)


def test_mixed_encodings_share_the_decode_and_match_alone(chat):
    """decode_to_pcm16(ragged) and decode_split_to_pcm16 with one encoding per row / request, None among them, at 24 kHz (rows on multiples
    of 8: one range per run of rows) and at mixed rates (rows anywhere: through the grouped conversion)"""
    g = torch.Generator(device=DEV).manual_seed(5)
    rows = [torch.randn((n, 768), device=DEV, generator=g) * 0.5 for n in (9, 24, 5, 17)]
    encs = ["ulaw", None, "alaw", "alaw"]
    for rate in (None, [8000, 24000, 16000, 8000]):
        rkw = {} if rate is None else {"sample_rate": rate}
        for strip in (True, False):
            pcm = chat.decode_to_pcm16(rows, ragged=True, strip=strip, **rkw)
            got = chat.decode_to_pcm16(rows, ragged=True, strip=strip, encoding=encs, **rkw)
            for k, (a, p, e) in enumerate(zip(got, pcm, encs)):
                want = p if e is None else g711.encode(p, e)
                assert a.dtype == want.dtype and a.tobytes() == want.tobytes(), (rate, strip, k)
        groups = [rows[:2], rows[2:3], rows[3:]]
        grate = {} if rate is None else {"sample_rate": [8000, 16000, 24000]}
        pcm = chat.decode_split_to_pcm16(groups, **grate)
        for ge in (["ulaw", "alaw", "ulaw"], [None, "alaw", "ulaw"]):
            got = chat.decode_split_to_pcm16(groups, encoding=ge, **grate)
            for k, (a, p, e) in enumerate(zip(got, pcm, ge)):
                want = p if e is None else g711.encode(p, e)
                assert a.dtype == want.dtype and a.tobytes() == want.tobytes(), (rate, ge, k)
    one = chat.decode_to_pcm16(rows, strip=True, encoding="ulaw")             # the padded batch
    _same(one, chat.decode_to_pcm16(rows, strip=True), "ulaw", "padded")


def _sparams(chat, **kw):
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=80,
                                min_new_token=80, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice, stream_batch=24,
                                stream_speed=3000, pass_first_n_batches=1, **kw)


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_serial_stream_at_8k_chunk_by_chunk(chat, law):
    def run(**kw):
        return [np.asarray(c) for c in chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False, pcm16=True,
                                                  params_infer_code=_sparams(chat), sample_rate=8000, stream_resample=True, **kw)]
    pcm, got = run(), run(encoding=law)
    assert len(pcm) == 4 and pcm[-1].shape[1] > 0 and [p.shape[1] for p in pcm[:-1]] == [1000, 1000, 1000]      # 3 chunks and the stripped tail
    _same(got, pcm, law, "stream 8k")
    pcm24 = [np.asarray(c) for c in chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False, pcm16=True,
                                               params_infer_code=_sparams(chat))]
    got24 = [np.asarray(c) for c in chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False, pcm16=True,
                                               params_infer_code=_sparams(chat), encoding=law)]
    _same(got24, pcm24, law, "stream 24k")


def _serial_codes(chat, hid, counts, spec, rate, enc):
    """the `stream` branch of `Chat._infer` (pcm16, one text, `sample_rate=rate`, `encoding=enc`) replayed over `hid`"""
    kw = {} if rate == 24000 else {"rate": rate}
    chunks, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        chunks.append(chat._stream_piece([hid[:n]], length, length + spec.stream_speed, True, True, encoding=enc, **kw)[0])
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
    w = chat._stream_piece([hid], length, None, True, **kw)[0]
    w = w[np.abs(w) > 1e-5]
    chunks.append(g711.encode(audio.float_to_int16(w) if w.size else w.astype(np.int16), enc))
    return chunks


def test_pooled_streams_with_mixed_encodings_equal_the_serial_compositions(weights):
    """PCM16 at 24 kHz, mu-law at 8 kHz, A-law at 8 kHz, mu-law at 16 kHz through a 4-slot pool, the chunks of a poll from ONE
    decode_windows call: every chunk == the serial composition replayed over the hidden states the pool returned, byte for byte -- the
    PCM16 composition companded by the twin, and the serial path's own companded pieces"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec = codec
    pool = SlotPool(eng, slots=4, cap=256, hid_cap=128, per_request=True)
    rs = np.random.RandomState(33)
    plan = [(72, -1, 3000, 0, 24000, None), (80, 48, 12000, 1, 8000, "ulaw"), (60, -1, 12000, 0, 8000, "alaw"), (50, -1, 5000, 1, 16000, "ulaw")]
    reqs = {}
    for i, (max_new, stop, speed, passed, rate, enc) in enumerate(plan):
        ids = torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(int(rs.randint(4, 30)), 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(700 + 13 * i))
        reqs[i] = (ids, p, max_new, stop, StreamSpec(24, speed, passed), rate, enc)
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=reqs[i][4])
    chunks, results, groups = {}, {}, []
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            groups.append(len(got.chunks))
            out = chat.decode_windows_pcm16(pool.hiddens, [c[1:] for c in got.chunks], sample_rates=[reqs[c[0]][5] for c in got.chunks],
                                            encodings=[reqs[c[0]][6] for c in got.chunks])
            for c, a in zip(got.chunks, out):
                chunks.setdefault(c[0], []).append(a)
        else:
            results[got[0]] = (got[1].cpu().numpy(), got[2])
    assert sorted(results) == [0, 1, 2, 3] and sorted(chunks) == [0, 1, 2, 3] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec, rate, enc) in reqs.items():
        _, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        pcm = _serial_chunks_rate(chat, results[i][1], counts, spec, rate)
        got = chunks[i]
        assert [g.shape for g in got] == [w.shape for w in pcm] and sum(g.size for g in got) > 0, (i, [g.shape for g in got], [w.shape for w in pcm])
        if enc is None:
            assert all(g.dtype == np.int16 and g.tobytes() == w.tobytes() for g, w in zip(got, pcm)), i
            continue
        codes = _serial_codes(chat, results[i][1], counts, spec, rate, enc)
        for k, (g, w, c) in enumerate(zip(got, pcm, codes)):
            assert g.dtype == np.uint8 and g.tobytes() == g711.encode(w, enc).tobytes() == c.tobytes(), (i, rate, enc, k)
    pool.close()


def test_pooled_requests_with_mixed_encodings(chat):
    """three requests that finish together (ragged_decode): None at 24 kHz, mu-law at 8 kHz, A-law at 16 kHz == the same batch without
    encodings, companded by the twin"""
    plan = [(None, None), ("ulaw", 8000), ("alaw", 16000)]

    def run(with_enc):
        b = SpeechBatcher(chat, 4, threading.Lock(), ragged_decode=True)
        try:
            with b.lock:
                futs = [b.submit(t, _params(chat, i), sample_rate=r, **({"encoding": e} if with_enc else {})) for i, (t, (e, r)) in enumerate(zip(TEXTS, plan))]
            return [f.result(timeout=300) for f in futs], b.occupancy()
        finally:
            b.close()
    pcm, occ0 = run(False)
    got, occ = run(True)
    assert occ0["companded"] == 0 and occ["companded"] == 2 and occ["decode_calls"] == occ0["decode_calls"]
    for k, (g, p, (e, _)) in enumerate(zip(got, pcm, plan)):
        want = p if e is None else g711.encode(p, e)
        assert p.dtype == np.int16 and p.size > 0 and g.dtype == want.dtype and g.tobytes() == want.tobytes(), k


def test_endpoint_bodies_and_its_own_ulaw_wav_as_a_voice(chat):
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
        pcm = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, sample_rate=8000)[0]
        app = server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 24000), voice_upload=True, g711=True)
        with TestClient(app) as c:
            body = {"input": TEXTS[0], "sample_rate": 8000}
            raw = c.post("/v1/audio/speech", json={**body, "response_format": "ulaw"})
            assert raw.status_code == 200 and raw.headers["content-type"].lower() == "audio/pcmu"
            assert raw.content == g711.encode(pcm, "ulaw").tobytes() and len(raw.content) > 0
            raw_a = c.post("/v1/audio/speech", json={**body, "response_format": "alaw"})
            assert raw_a.status_code == 200 and raw_a.content == g711.encode(pcm, "alaw").tobytes()
            wav = c.post("/v1/audio/speech", json={**body, "response_format": "wav", "encoding": "ulaw"})
            assert wav.status_code == 200 and wav.content == audio.g711_to_wav_bytes(g711.encode(pcm, "ulaw"), "ulaw", 8000)
            assert struct.unpack_from("<HHI", wav.content, 20) == (7, 1, 8000)
            assert c.post("/v1/audio/speech", json={**body, "response_format": "wav", "encoding": "g722"}).status_code == 400
            # the endpoint's own mu-law file as a voice == the PCM16 file of the expanded codes as a voice
            up = c.post("/v1/audio/voices", params={"name": "tel"}, content=wav.content)
            assert up.status_code == 200 and up.json()["sample_rate"] == 8000 and up.json()["tokens"] > 0, up.text
            lin = g711.expand(g711.encode(pcm, "ulaw"), "ulaw")
            up2 = c.post("/v1/audio/voices", params={"name": "lin"}, content=server.pcm16_to_wav_bytes(lin, 8000))
            assert up2.status_code == 200 and up2.json()["tokens"] == up.json()["tokens"]
            assert len(smps) == 2 and smps[0] == smps[1]
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, sample_rates=(8000, 24000), voice_upload=True)) as c:
            assert c.post("/v1/audio/speech", json={**body, "response_format": "ulaw"}).status_code == 400
            assert c.post("/v1/audio/voices", params={"name": "tel"}, content=wav.content).status_code == 400
    finally:
        chat.InferCodeParams = orig_params
        del chat.sample_audio_speaker

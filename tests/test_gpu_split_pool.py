"""split_text requests served from the slot pool, on the GPU: concurrent multi-sentence requests through `SpeechBatcher` against the
serial `Chat.infer(text, split_text=True, ragged_decode=True, pcm16=True)` call of each, the device-side strip / convert / compact
against the host composition, a cloned voice, and the endpoint's `split_text`.  `pytest -m gpu`."""
import dataclasses
import io
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import weights as W  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import split_sentences  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = np.float32(1e-5)

SPLIT_TEXTS = ["Hello there. How are you?",                                                   # 2 sentences (". ")
               "第一句话。第二句话。tail without a stop",                                        # 3 (CJK full stops)
               "Line one\nline two is longer\nthree\nthe fourth line\nfive"]                  # 5 (newlines)
PLAIN_TEXTS = ["Good morning!", "Numbers like 42 and 7."]
MSB = [4, 2, 2]              # the 5-sentence request runs as serial batches of 2 + 2 + 1


@pytest.fixture(scope="module", params=["f32", "f32x3"])
def chat(request, weights):
    from chattts_amd.core import Chat
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts={**weights, "dvae": W.synthetic_dvae()}, device=DEV, dtype=request.param, tokenizer=os.path.join(GOLD, "tokenizer"),
                  spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voices = {"default": c.sample_random_speaker(), "alloy": c.sample_random_speaker()}
    return c


def _params(chat, i, **kw):
    vs = list(chat.test_voices.values())
    return chat.InferCodeParams(top_P=[0.5, 0.7][i % 2], top_K=[10, 20, 5][i % 3], temperature=[0.1, 0.3][i % 2], repetition_penalty=1.1,
                                max_new_token=[24, 32, 16][i % 3], show_tqdm=False, manual_seed=300 + 7 * i, spk_emb=vs[i % 2], **kw)


def _close(got, want, what):          # the pooled endpoint's bar (test_gpu_text_pool.py)
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) if got.size else 0
    assert d <= 1, (what, d)


def _host_formula(chat, hids):
    """the host lines of Chat.infer(split_text=True, pcm16=True): alone decodes, strip, concatenate, ONE float_to_int16"""
    ws = [chat.decode_to_wavs([h], ragged=True)[0] for h in hids]
    return float_to_int16(np.concatenate([w[np.abs(w) > THR] for w in ws]))


class _Serial:
    """records what the serial call generates: every `_infer_code` result (ids, hidden states) and the speaker prompt"""

    def __init__(self, chat):
        self.chat, self.orig, self.calls = chat, chat._infer_code, []

    def __enter__(self):
        def rec(text, stream, device, return_hidden, params):
            for out in self.orig(text, stream, device, return_hidden, params):
                self.calls.append(([t.cpu().numpy().copy() for t in out.ids], [h.clone() for h in out.hiddens], params.spk_smp))
                yield out
        self.chat._infer_code = rec
        return self

    def __exit__(self, *a):
        del self.chat._infer_code


class _Recording(SpeechBatcher):
    def _handle(self, got):
        for it in ([got] if isinstance(got, tuple) else got if isinstance(got, list) else []):
            self.code_ids[it[0]] = it[1].cpu().numpy()
            self.hid[it[0]] = it[2].clone()
        super()._handle(got)

    def _code_submit(self, key, t, params, **kw):
        self.smp[key] = params.spk_smp
        super()._code_submit(key, t, params, **kw)


@pytest.fixture(scope="module")
def serial(chat):
    """the serial run of every split request: (pcm, per-sentence ids, per-sentence hidden states, stage A's spk_smp)"""
    out = []
    for i, text in enumerate(SPLIT_TEXTS):
        p = _params(chat, i)
        with _Serial(chat) as rec:
            pcm = chat.infer(text, skip_refine_text=True, split_text=True, max_split_batch=MSB[i], ragged_decode=True, pcm16=True,
                             params_infer_code=p)[0]
        n = len(split_sentences(text))
        assert len(rec.calls) == 1 + -(-n // MSB[i]) and rec.calls[0][2] is None        # stage A, then the split batches
        ids = [r for c in rec.calls[1:] for r in c[0]]
        hids = [h for c in rec.calls[1:] for h in c[1]]
        assert len(ids) == n and all(r.shape[0] > 0 for r in ids), "a sentence drew EOS first: pick other seeds"
        assert p.spk_smp is not None and all(c[2] == p.spk_smp for c in rec.calls[1:])
        out.append(dict(pcm=pcm, ids=ids, hids=hids, smp=p.spk_smp, a_ids=rec.calls[0][0][0]))
    return out


@pytest.fixture(scope="module")
def pooled(chat):
    """3 split requests of 2, 3 and 5 sentences + 2 plain ones, concurrently, through 4 slots"""
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.code_ids, b.hid, b.smp = {}, {}, {}
    ps = [_params(chat, i) for i in range(5)]
    try:
        with b.lock:      # taken together
            futs = [b.submit(t, ps[i], split_text=True, max_split_batch=MSB[i]) for i, t in enumerate(SPLIT_TEXTS)]
            futs += [b.submit(t, ps[3 + k]) for k, t in enumerate(PLAIN_TEXTS)]
        got = [f.result(timeout=300) for f in futs]
        occ = b.occupancy()
    finally:
        b.close()
    assert all(p.spk_smp is None and p.txt_smp is None for p in ps)           # the callers' objects are untouched
    return dict(b=b, got=got, occ=occ, ps=ps)


def test_sentences_draw_the_serial_tokens_and_stage_a_the_serial_prompt(serial, pooled):
    """(a)"""
    b = pooled["b"]
    for i, s in enumerate(serial):
        assert np.array_equal(b.code_ids[(i, "A")], s["a_ids"]), i
        for j, want in enumerate(s["ids"]):
            assert np.array_equal(b.code_ids[(i, j)], want), (i, j, b.code_ids[(i, j)].shape, want.shape)
            assert b.smp[(i, j)] == s["smp"], (i, j)
        assert b.smp[(i, "A")] is None


def test_bytes_equal_the_host_composition_of_the_pools_own_hidden_states(chat, serial, pooled):
    """(b)"""
    b = pooled["b"]
    for i, s in enumerate(serial):
        want = _host_formula(chat, [b.hid[(i, j)] for j in range(len(s["ids"]))])
        assert pooled["got"][i].dtype == np.int16 and pooled["got"][i].tobytes() == want.tobytes(), i
    for k in range(2):          # the plain requests of the same polls: a group of one sentence
        assert pooled["got"][3 + k].tobytes() == _host_formula(chat, [b.hid[3 + k]]).tobytes(), k


def test_pcm_within_one_count_of_the_serial_call(chat, serial, pooled):
    """(c)"""
    for i, s in enumerate(serial):
        _close(pooled["got"][i], s["pcm"], i)
    for k, t in enumerate(PLAIN_TEXTS):
        want = chat.infer([t], skip_refine_text=True, params_infer_code=_params(chat, 3 + k), pcm16=True)[0]
        _close(pooled["got"][3 + k], want, ("plain", k))


def test_occupancy_shows_sentences_of_one_request_side_by_side(pooled):
    """(e)"""
    occ = pooled["occ"]
    assert occ["split"]["requests"] == 3 and occ["split"]["sentences"] == 10 and occ["split"]["max_coresident"] >= 2, occ
    assert occ["completed"] == 5 and occ["failed"] == 0 and occ["max_coresident"] == 4, occ


def test_a_cloned_voice_runs_no_stage_a(chat, serial):
    """(d)"""
    p = _params(chat, 1, spk_smp=serial[1]["smp"], txt_smp="第一句话。")
    before = dataclasses.replace(p)
    b = _Recording(chat, 4, threading.Lock())
    b.code_ids, b.hid, b.smp = {}, {}, {}
    try:
        got = b.submit(SPLIT_TEXTS[1], p, split_text=True, max_split_batch=MSB[1]).result(timeout=300)
        occ = b.occupancy()
    finally:
        b.close()
    assert sorted(b.code_ids, key=str) == [(0, 0), (0, 1), (0, 2)] and all(v == serial[1]["smp"] for v in b.smp.values())
    assert vars(p) == vars(before)
    want = chat.infer(SPLIT_TEXTS[1], skip_refine_text=True, split_text=True, max_split_batch=MSB[1], ragged_decode=True, pcm16=True,
                      params_infer_code=dataclasses.replace(p))[0]
    _close(got, want, "cloned")
    assert occ["split"] == {"requests": 1, "sentences": 3, "max_coresident": 3} and occ["decode_calls"] == 1


def test_chat_infer_split_pcm16_ragged_returns_the_bytes_of_the_host_lines(chat, serial):
    """(f): the device path of Chat.infer (decode_split_to_pcm16) == the host composition it replaces, from the same hidden states"""
    for i, s in enumerate(serial):
        assert s["pcm"].dtype == np.int16 and s["pcm"].tobytes() == _host_formula(chat, s["hids"]).tobytes(), i
    # without ragged_decode nothing changed: the padded batches, stripped and converted on the host
    p = _params(chat, 0)
    f32w = chat.infer(SPLIT_TEXTS[0], skip_refine_text=True, split_text=True, params_infer_code=dataclasses.replace(p))[0]
    pcm = chat.infer(SPLIT_TEXTS[0], skip_refine_text=True, split_text=True, pcm16=True, params_infer_code=dataclasses.replace(p))[0]
    assert pcm.tobytes() == float_to_int16(f32w).tobytes()
    # two requests in one call, one of a single sentence
    got = chat.decode_split_to_pcm16([serial[2]["hids"], serial[0]["hids"][:1]])
    assert got[0].tobytes() == serial[2]["pcm"].tobytes() and got[1].tobytes() == _host_formula(chat, serial[0]["hids"][:1]).tobytes()


def test_endpoint_split_text_round_trip(chat, serial):
    """(g)"""
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        p = chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                 min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voices["alloy"])
        want = chat.infer(SPLIT_TEXTS[0], skip_refine_text=True, split_text=True, ragged_decode=True, pcm16=True, params_infer_code=p)[0]
        app = server.create_app(chat, chat.test_voices, batch_slots=4, ragged_decode=True, batch_split=True)
        try:
            with TestClient(app) as c:
                r = c.post("/v1/audio/speech", json={"input": SPLIT_TEXTS[0], "voice": "alloy", "response_format": "wav", "split_text": True})
                health = c.get("/health").json()
        finally:
            app.state.batcher.close()
        assert r.status_code == 200, r.text
        with wave.open(io.BytesIO(r.content), "rb") as wf:
            pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
        _close(pcm, want, "endpoint")
        assert health["pool"]["split"]["requests"] == 1 and health["pool"]["split"]["sentences"] == 2, health
    finally:
        chat.InferCodeParams = orig

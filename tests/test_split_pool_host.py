"""split_text requests behind continuous batching, host side (no GPU): the shared sentence split, the stage A / stage B schedule of
`SpeechBatcher.submit(split_text=True)` with its sampling rows on fake pools, failure isolation, cancellation, the order of the
concatenation, the refine stage in front, and the endpoint's `split_text` key and dict voices."""
import logging
import re
import threading
import time
from concurrent.futures import CancelledError

import numpy as np
import pytest
import torch

from chattts_amd.core import Chat, split_sentences
from chattts_amd.serving import SpeechBatcher, split_rows


# ---- the split --------------------------------------------------------------------------------------------------------------------
SPLIT_CASES = {
    "first line\nsecond line here\n\nfourth": ["first line", "second line here", "", "fourth"],
    "中文句子。第二句。tail without stop": ["中文句子。", "第二句。", "tail without stop"],
    "One sentence. Another one. tail": ["One sentence. ", "Another one. ", "tail"],
    "No stop at all": ["No stop at all"],
    "Mixed. 中文。\nnewline wins": ["Mixed. 中文。", "newline wins"],
    "Ends with a stop. ": ["Ends with a stop. "],
    "": [],
}


def test_split_helper_is_chat_infers_split():
    chat, seen = Chat(), []

    def fake_infer(text, *a, **kw):
        seen.append(list(text))
        yield "refined"
    chat._infer = fake_infer
    for text, want in SPLIT_CASES.items():
        assert split_sentences(text) == want, text
        if want:
            assert chat.infer(text, split_text=True, refine_text_only=True) == "refined"
            assert seen[-1] == want, text
        else:
            assert chat.infer(text, split_text=True) == []
    chat.infer("a. b. c", split_text=False, refine_text_only=True)           # a str is cut only with split_text
    assert seen[-1] == list("a. b. c")


def test_split_rows_are_the_serial_batches_rows():
    for n in (1, 4, 5, 9):
        for m in (2, 4):
            want = []
            for lo in range(0, n, m):                 # Chat._infer: batches text[lo: lo + m], row b of a batch of B holds rows 4b .. 4b+3 of 4B
                B = len(range(lo, min(lo + m, n)))
                want += [(4 * b, 4 * B) for b in range(B)]
            assert split_rows(n, m) == want, (n, m)
    assert split_rows(5, 4) == [(0, 16), (4, 16), (8, 16), (12, 16), (0, 4)]
    with pytest.raises(ValueError):
        split_rows(3, 0)


# ---- fakes ------------------------------------------------------------------------------------------------------------------------
class _Params:
    def __init__(self, max_new=16, spk_smp=None, txt_smp=None):
        self.spk_emb, self.spk_smp, self.txt_smp, self.max_new_token = "spk", spk_smp, txt_smp, max_new
        self.stream_batch, self.stream_speed, self.pass_first_n_batches = 24, 12000, 2


class _Refine:
    def __init__(self, max_new=8):
        self.prompt, self.max_new_token = "", max_new


class _Tok:
    spk_emb_ids = 7


def _ids_of(text):
    t = np.frombuffer(text.encode(), dtype=np.uint8).astype(np.int64)
    return torch.from_numpy(np.repeat(t[None, :, None], 4, axis=2))


def _n_tokens(text, default):
    """"name#24": the fake engine generates 24 tokens for it ("#0": the first token is EOS); else max_new_token"""
    m = re.search(r"#(\d+)", text)
    return int(m.group(1)) if m else default


class _FakeChat:
    """prompts = the text's bytes; a sentence's hidden states carry its first byte; the decoded "audio" of a sentence is that byte, one
    sample per token, so a request's result spells its sentences in order"""
    tokenizer = _Tok()

    def __init__(self):
        self.code_calls, self.refer_calls, self.split_decodes, self.refined = [], [], [], []

    def normalizer(self, text, norm, homophones, lang):
        return text.strip(" ")

    def refine_prompt(self, texts, params):
        ids = _ids_of(texts[0])
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def refined_text(self, rows):
        t = bytes(rows[0].numpy().astype(np.uint8)).decode()
        self.refined.append(t)
        if t.startswith("boom"):
            raise ValueError("tokenizer failed")
        return [t + "!"]

    def code_prompt(self, texts, params):
        self.code_calls.append((texts[0], params.spk_smp, params.txt_smp))
        ids = _ids_of(texts[0])
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def prompt_embedding(self, ids, tmask, params, spk_emb_ids):
        return ids[..., :1].float().expand(*ids.shape[:2], 768).clone()

    def refer_speaker(self, rows, use_decoder=True, *, on_device=False, release=None):
        assert on_device and len(rows) == 1
        self.refer_calls.append(int(rows[0].shape[0]))
        return f"SMP<{int(rows[0][0, 0])}:{int(rows[0].shape[0])}>"

    def decode_to_wavs(self, hids):
        return np.stack([np.full((int(hids[0].shape[0]),), 0.5, np.float32)])

    def decode_to_pcm16(self, hids, ragged=False):
        assert ragged
        return [np.full((int(h.shape[0]),), int(h[0, 0]), np.int16) for h in hids]

    def decode_split_to_pcm16(self, groups):
        self.split_decodes.append([len(g) for g in groups])
        return [np.concatenate([np.full((int(h.shape[0]),), int(h[0, 0]), np.int16) for h in g]) for g in groups]


class _Pool:
    """S slots, 8 tokens per launch; results come one poll late, like SlotPool.  A request runs for `_n_tokens(prompt)` tokens; a code
    request's hidden states are the prompt's first byte, a text request's row is its prompt ("empty": no tokens).  `log` records every submit
    with its sampling rows."""
    POLL = 8

    def __init__(self, S, lock, text=False, cap=64):
        self.S, self.lock, self.text, self.cap = S, lock, text, cap
        self.queue, self.active, self.free, self.ready = [], {}, list(range(S)), []
        self.log, self.cancels, self.max_active, self.on_submit = [], [], 0, None

    def submit(self, rid, ids, tmask=None, max_new_token=8, *, params=None, emb=None, stream=None, row_offset=0, total_rows=None):
        text = bytes(ids[:, 0].numpy().astype(np.uint8)).decode()
        if ids.shape[0] + max_new_token > self.cap:
            raise ValueError("request does not fit a slot")
        self.log.append((rid, text, row_offset, total_rows))
        if self.on_submit is not None:
            self.on_submit(rid)
        n = _n_tokens(text, max_new_token)
        self.queue.append([rid, ids, n, 0, False])

    def cancel(self, rid):
        self.cancels.append(rid)
        for q in self.queue:
            if q[0] == rid:
                self.queue.remove(q)
                return True
        for a in self.active.values():
            if a[0] == rid:
                a[4] = True
                return True
        return False

    def busy(self):
        return bool(self.queue or self.active or self.ready)

    def launch(self):
        assert self.lock.locked()
        while self.queue and self.free:
            self.active[self.free.pop(0)] = self.queue.pop(0)
        self.max_active = max(self.max_active, len(self.active))
        return bool(self.active)

    def results(self, grouped=False):
        out, self.ready = self.ready, []
        if grouped and out:
            yield out
        elif not grouped:
            yield from out

    def poll(self, events=False):
        for s, a in list(self.active.items()):
            rid, ids, n, count, cancelled = a
            if not cancelled:
                a[3] = count = min(count + 8, n)
                if count < n:
                    continue
                row = ids[:, 0]
                if self.text:
                    self.ready.append((rid, row[:0] if bytes(row.numpy().astype(np.uint8)) == b"empty" else row, torch.zeros((0, 768))))
                else:
                    self.ready.append((rid, ids[:n], torch.full((n, 768), float(ids[0, 0]))))
            del self.active[s]
            self.free.append(s)
            self.free.sort()
        return iter(())

    def run(self, between=None, grouped=False, events=False):
        while self.busy():
            between()
            self.launch()
            yield from self.results(grouped)
            yield from self.poll(events)


def _batcher(slots=4, refine=False, **kw):
    lock = threading.Lock()
    chat, pools = _FakeChat(), {}
    extra = dict(refine=True, make_text_pool=lambda: pools.setdefault("text", _Pool(slots, lock, True))) if refine else {}
    b = SpeechBatcher(chat, slots, lock, make_pool=lambda: pools.setdefault("code", _Pool(slots, lock)), **extra, **kw)
    return b, chat, pools, lock


def _spell(pcm):
    """the fake audio as [(sentence's first character, samples)]: one entry per run of equal samples"""
    pcm = np.asarray(pcm)
    cuts = np.flatnonzero(np.diff(pcm)) + 1
    return [(chr(int(r[0])), int(r.size)) for r in np.split(pcm, cuts)]


def _wait_idle(pools, timeout=10):
    deadline = time.time() + timeout
    while any(p.busy() for p in pools.values()) and time.time() < deadline:
        time.sleep(0.01)
    assert not any(p.busy() for p in pools.values())
    assert all(sorted(p.free) == list(range(p.S)) for p in pools.values()), "a slot was not freed"


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msb", [2, 4])
@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_stage_a_then_stage_b_with_the_serial_rows(n, msb):
    b, chat, pools, lock = _batcher(slots=4)
    names = "abcdefghi"[:n]
    text = "\n".join(f"{c}#{8 * (1 + i % 3)}" for i, c in enumerate(names))
    params = _Params()
    try:
        pcm = b.submit(text, params, split_text=True, max_split_batch=msb).result(timeout=30)
        occ = b.occupancy()
    finally:
        b.close()
    log = pools["code"].log
    if n == 1:          # one sentence: an ordinary request with the pool's default rows, no stage A, the per-request decode
        assert log == [(0, "a#8", 0, None)] and chat.refer_calls == [] and chat.split_decodes == []
        assert occ["split"] == {"requests": 0, "sentences": 0, "max_coresident": 0}
        return
    assert log[0] == ((0, "A"), "a#8", 0, 4)                                      # stage A: sentence 0 alone, a batch of one
    assert chat.refer_calls == [8]
    rows = split_rows(n, msb)
    assert log[1:] == [((0, i), f"{c}#{8 * (1 + i % 3)}", *rows[i]) for i, c in enumerate(names)]      # sentence 0 again included
    # stage A's prompt has no audio prompt; every stage-B prompt carries stage A's, with sentence 0 as its text
    assert chat.code_calls[0] == ("a#8", None, None)
    assert chat.code_calls[1:] == [(f"{c}#{8 * (1 + i % 3)}", "SMP<97:8>", "a#8") for i, c in enumerate(names)]
    assert (params.spk_smp, params.txt_smp) == (None, None)                       # the caller's object is untouched
    assert _spell(pcm) == [(c, 8 * (1 + i % 3)) for i, c in enumerate(names)]     # sentence order, whatever finished first
    assert chat.split_decodes == [[n]]
    assert occ["split"]["requests"] == 1 and occ["split"]["sentences"] == n and 2 <= occ["split"]["max_coresident"] <= 4
    assert occ["completed"] == 1 and occ["failed"] == 0


def test_stage_a_is_skipped_for_a_cloned_voice():
    b, chat, pools, lock = _batcher(slots=4)
    params = _Params(spk_smp="GIVEN", txt_smp="given text")
    try:
        pcm = b.submit("x#24。y#8。z#16", params, split_text=True).result(timeout=30)
    finally:
        b.close()
    assert [e[0] for e in pools["code"].log] == [(0, 0), (0, 1), (0, 2)] and chat.refer_calls == []
    assert chat.code_calls == [("x#24。", "GIVEN", "given text"), ("y#8。", "GIVEN", "given text"), ("z#16", "GIVEN", "given text")]
    assert _spell(pcm) == [("x", 24), ("y", 8), ("z", 16)]                        # y finished first, z second, x last


def test_other_requests_interleave_and_ragged_decode_takes_them_together():
    b, chat, pools, lock = _batcher(slots=4, ragged_decode=True)
    try:
        with lock:      # taken together
            split = b.submit("k#16\nl#16\nm#16", _Params(spk_smp="V"), split_text=True)
            plain = b.submit("p#16", _Params())
        assert _spell(split.result(timeout=30)) == [("k", 16), ("l", 16), ("m", 16)]
        assert _spell(plain.result(timeout=30)) == [("p", 16)]
        occ = b.occupancy()
    finally:
        b.close()
    assert pools["code"].max_active == 4
    assert chat.split_decodes == [[1, 3]]                 # ONE pass: the plain request as a group of one, then the split request
    assert occ["decode_calls"] == 1 and occ["decoded"] == 2 and occ["split"]["max_coresident"] == 3


def test_a_failure_fails_that_request_only_and_frees_its_slots():
    b, chat, pools, lock = _batcher(slots=4)
    try:
        with lock:
            eos = b.submit("a#8\nb#0\nc#40", _Params(spk_smp="V"), split_text=True)      # sentence 1 draws EOS first
            fine = b.submit("d#8\ne#8", _Params(spk_smp="V"), split_text=True)
            long_ = b.submit("f#8\n" + "g" * 60, _Params(spk_smp="V"), split_text=True)    # sentence 1 does not fit a slot
            eos_a = b.submit("h#0\ni#8", _Params(), split_text=True)                       # the refer sentence itself is empty
            empty = b.submit("", _Params(), split_text=True)
        with pytest.raises(RuntimeError, match="returned no audio"):
            eos.result(timeout=30)
        with pytest.raises(ValueError, match="does not fit"):
            long_.result(timeout=30)
        with pytest.raises(RuntimeError, match="returned no audio"):
            eos_a.result(timeout=30)
        with pytest.raises(ValueError, match="no sentence"):
            empty.result(timeout=30)
        assert _spell(fine.result(timeout=30)) == [("d", 8), ("e", 8)]
        _wait_idle(pools)
        occ = b.occupancy()
        assert occ["failed"] == 4 and occ["completed"] == 1
        assert (0, 2) in pools["code"].cancels            # the 40-token sentence of the failed request left its slot early
        assert not b._sub and not b._splits
        assert _spell(b.submit("q#8\nr#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)) == [("q", 8), ("r", 8)]
    finally:
        b.close()


def test_cancel_covers_every_sentence():
    b, chat, pools, lock = _batcher(slots=2)
    pool = pools.setdefault("code", _Pool(2, lock))          # the pool the batcher's make_pool hands out
    resident, queued, poll = threading.Event(), threading.Event(), pool.poll

    def gated_poll(events=False):
        # the worker stops with sentences b and c resident until the cancel is queued (it takes it at its next `_between`): the test
        # thread does not have to catch the 500 polls of a sentence, which a loaded machine runs through between two of its looks
        if len(pool.active) >= 2:
            resident.set()
            queued.wait(10)
        return poll(events)
    pool.poll = gated_poll
    try:
        fut = b.submit("a#4000\nb#4000\nc#4000", _Params(spk_smp="V", max_new=40), split_text=True)
        assert resident.wait(10), "sentences b and c never became resident"
        b.cancel(fut)
        queued.set()
        with pytest.raises(CancelledError):
            fut.result(timeout=30)
        _wait_idle(pools)
        assert sorted(pools["code"].cancels) == [(0, 0), (0, 1), (0, 2)] and not b._sub and not b._splits
        assert _spell(b.submit("d#8\ne#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)) == [("d", 8), ("e", 8)]
    finally:
        b.close()


def test_refine_rows_first_and_stage_a_starts_with_sentence_0():
    b, chat, pools, lock = _batcher(slots=4, refine=True)
    params, seen = _Params(), []
    pools["code"].on_submit = lambda rid: seen.append((rid, len(pools["text"].active)))
    try:
        # sentence 0's text row is short (8 tokens), the others take 4 polls longer: stage A is submitted while they are still resident
        fut = b.submit("a#8\nb#40\nc#40", params, refine=_Refine(max_new=8), split_text=True, max_split_batch=2)
        pcm = fut.result(timeout=30)
        occ = b.occupancy()
    finally:
        b.close()
    assert pools["text"].log == [((0, "r", i), t, i, 3) for i, t in enumerate(["a#8", "b#40", "c#40"])]      # rows i of n: one serial batch
    assert seen[0] == ((0, "A"), 2) and [r for r, _ in seen[1:]] == [(0, 0), (0, 1), (0, 2)] and all(k == 0 for _, k in seen[1:])
    assert pools["code"].log[0][1] == "a#8!" and [e[2:] for e in pools["code"].log[1:]] == [(0, 8), (4, 8), (0, 4)]
    assert chat.code_calls[1:] == [(t, "SMP<97:8>", "a#8!") for t in ("a#8!", "b#40!", "c#40!")]
    assert _spell(pcm) == [("a", 8), ("b", 40), ("c", 40)] and params.spk_smp is None
    assert occ["refine"]["admissions"] == 3 and occ["refine"]["handed"] == 1 and occ["split"]["sentences"] == 3


def test_a_refine_failure_fails_the_split_request_only():
    b, chat, pools, lock = _batcher(slots=4, refine=True)
    try:
        with lock:
            bad = b.submit("ok\nboom\nfine", _Params(spk_smp="V"), refine=_Refine(), split_text=True)
            good = b.submit("g#8\nh#8", _Params(spk_smp="V"), refine=_Refine(), split_text=True)
        with pytest.raises(ValueError, match="tokenizer failed"):
            bad.result(timeout=30)
        assert _spell(good.result(timeout=30)) == [("g", 8), ("h", 8)]
        _wait_idle(pools)
    finally:
        b.close()


def test_streamed_split_is_refused():
    b, chat, pools, lock = _batcher(slots=2, streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream("a\nb", _Params(), split_text=True)
        with pytest.raises(ValueError, match="max_split_batch"):
            b.submit("a\nb", _Params(), split_text=True, max_split_batch=0)
    finally:
        b.close()


# ---- the endpoint -----------------------------------------------------------------------------------------------------------------
class _EndpointChat:
    class InferCodeParams:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    def __init__(self):
        self.calls = []

    def has_loaded(self):
        return True

    def infer(self, text, stream=False, **kw):
        self.calls.append((list(text), stream, kw))
        full = np.arange(600, dtype=np.int16)
        return (c[None, :] for c in (full[:300], full[300:])) if stream else [full]


class _FakeBatcher:
    streams = refine = False

    def __init__(self):
        self.lock, self.calls = threading.Lock(), []

    def submit(self, text, params, **kw):
        from concurrent.futures import Future
        self.calls.append((text, params, kw))
        f = Future()
        f.set_result(np.arange(100, dtype=np.int16))
        return f

    def occupancy(self):
        return {}


class _Catch(logging.Handler):
    def __init__(self):
        super().__init__()
        self.msgs = []

    def emit(self, record):
        self.msgs.append(record.getMessage())


def test_endpoint_split_text_key_and_dict_voices():
    from starlette.testclient import TestClient
    from chattts_amd import server
    voices = {"default": "SPK-D", "clone": {"spk_smp": "SMP-C", "txt_smp": "what the clip says"}, "both": {"spk_emb": "SPK-B", "spk_smp": "SMP-B"}}
    body = {"input": "One. Two. Three.", "response_format": "pcm"}

    def app_of(**kw):
        log, catch = logging.getLogger(f"test_split_pool.{len(kw)}.{sorted(kw)}"), _Catch()
        log.addHandler(catch)
        chat, bat = _EndpointChat(), _FakeBatcher()
        return server.create_app(chat, voices, batcher=bat, logger=log, **kw), chat, bat, catch

    app, chat, bat, catch = app_of(batch_split=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "split_text": True, "voice": "clone"}).status_code == 200
        text, p, kw = bat.calls[-1]
        assert text == "One. Two. Three." and kw == {"split_text": True}
        assert (p.spk_emb, p.spk_smp, p.txt_smp) == (None, "SMP-C", "what the clip says")          # a cloned voice: no stage A
        assert c.post("/v1/audio/speech", json={**body, "voice": "both"}).status_code == 200
        text, p, kw = bat.calls[-1]
        assert kw == {} and (p.spk_emb, p.spk_smp, p.txt_smp) == ("SPK-B", "SMP-B", None)            # no key: an ordinary request
        assert c.post("/v1/audio/speech", json={**body, "split_text": False}).status_code == 200 and bat.calls[-1][2] == {}
        assert c.post("/v1/audio/speech", json={**body, "voice": "nobody"}).status_code == 200
        assert (bat.calls[-1][1].spk_emb, bat.calls[-1][1].spk_smp) == ("SPK-D", None)               # a plain string keeps meaning spk_emb
        assert not catch.msgs
        n = len(bat.calls)
        r = c.post("/v1/audio/speech", json={**body, "split_text": True, "stream": True, "voice": "clone"})       # the serial stream
        assert r.status_code == 200 and len(bat.calls) == n and chat.calls[-1][1] is True
        assert chat.calls[-1][2]["params_infer_code"].spk_smp == "SMP-C" and "split_text" not in chat.calls[-1][2]
        assert any("split_text" in m and "non-streamed" in m for m in catch.msgs), catch.msgs

    app, chat, bat, catch = app_of()                       # without batch_split the key is unknown
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "split_text": True}).status_code == 200
        assert bat.calls[-1][2] == {} and any("unsupported parameters" in m and "split_text" in m for m in catch.msgs), catch.msgs

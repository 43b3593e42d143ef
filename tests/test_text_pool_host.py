"""The refine-text stage of the batched serving path, host side (no GPU): text-mode request parameters and their table row, and the
two-pool worker of `SpeechBatcher(refine=True)` on fake pools -- hand-off, order, failure isolation, cancellation, idle pools."""
import threading
import time

import numpy as np
import pytest
import torch

from chattts_amd import _lib
from chattts_amd.serving import RequestParams, SpeechBatcher, StreamCursor, StreamEvents, request_params, sampling_row


# ---- request_params(infer_text=True) / sampling_row -----------------------------------------------------------------------------------
class _Refine:
    def __init__(self, **kw):
        self.prompt, self.top_P, self.top_K, self.temperature, self.repetition_penalty = "", 0.7, 20, 0.7, 1.0
        self.max_new_token, self.min_new_token, self.ensure_non_empty, self.manual_seed = 384, 0, True, None
        self.__dict__.update(kw)


def test_text_request_params_validate_like_refine_text_ids():
    p = request_params(None, infer_text=True)                       # RefineTextParams' defaults
    assert p.infer_text and p.temperature == (0.7,) and p.plan.top_p == 0.7 and p.plan.top_k == 20 and p.plan.penalty is None
    assert p.min_new_token == 0 and p.manual_seed is None and p.ensure_non_empty
    p = request_params(_Refine(temperature=0.3, top_P=None, top_K=500, min_new_token=3, manual_seed=9), infer_text=True)
    assert p.temperature == (0.3,) and p.plan.top_p is None and p.plan.top_k == 500 and p.min_new_token == 3 and p.manual_seed == 9
    assert request_params(dict(temperature=[1.3]), infer_text=True).temperature == (1.3,)
    with pytest.raises(NotImplementedError, match="repetition_penalty = 1.0 only"):
        request_params(dict(repetition_penalty=1.05), infer_text=True)
    with pytest.raises(NotImplementedError, match="repetition_penalty = 1.0 only"):
        request_params(_Refine(repetition_penalty=0.9), infer_text=True)
    for bad in ([0.3, 0.3, 0.3, 0.3], [], [0.1, 0.2]):
        with pytest.raises(ValueError, match="one temperature"):
            request_params(dict(temperature=bad), infer_text=True)
    # the code mode is what it was: four temperatures, the penalty allowed
    assert request_params(None).temperature == (0.3,) * 4 and request_params(None).plan.penalty == 1.05 and not request_params(None).infer_text


def test_text_sampling_row_bytes():
    p = request_params(dict(temperature=0.7, top_P=0.7, top_K=20, min_new_token=2, manual_seed=5), infer_text=True)
    r = sampling_row(p, rng_seed=2 ** 40 + 3, rng_per_step=True)
    raw = bytes(r)
    assert len(raw) == 128
    f, i = np.frombuffer(raw, np.float32), np.frombuffer(raw, np.int32)
    assert f[0] == np.float32(0.7) and not f[1:4].any()              # temperature[0] only
    assert not f[4:21].any() and i[21] == 0                          # no penalty table, use_penalty = 0
    assert f[22] == np.float32(1.0 - 0.7) and i[23] == 1 and i[24] == 20 and i[25] == 1 and i[26] == 2
    assert int(np.frombuffer(raw, np.uint64)[14]) == 2 ** 40 + 3 and i[30] == 1
    # a hand-built text request with a penalty is refused on the host: the kernel's text mode never reads use_penalty
    from chattts_amd.engine import SamplingPlan
    with pytest.raises(NotImplementedError, match="repetition_penalty = 1.0 only"):
        sampling_row(RequestParams((0.7,), SamplingPlan(0.7, 20, 1.05), 0, None, True, True))
    assert _lib.SamplingRow.use_penalty.offset == 84


# ---- the two-pool worker on fake pools ------------------------------------------------------------------------------------------------
class _Params:
    def __init__(self, n_tokens, passed=0):
        self.spk_emb, self.max_new_token = "spk", n_tokens
        self.stream_batch, self.stream_speed, self.pass_first_n_batches = 24, 12000, passed


class _Tok:
    spk_emb_ids = 7


def _ids_of(text):
    t = np.frombuffer(text.encode(), dtype=np.uint8).astype(np.int64)
    return torch.from_numpy(np.repeat(t[None, :, None], 4, axis=2))


class _FakeChat:
    """prompts = the text's bytes; the refined text = the text row's bytes decoded ("boom": the tokenizer fails)"""
    tokenizer = _Tok()

    def __init__(self):
        self.refined_calls, self.code_texts = [], []

    def normalizer(self, text, norm, homophones, lang):
        return text

    def refine_prompt(self, texts, params):
        ids = _ids_of(texts[0])
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def refined_text(self, rows):
        t = bytes(rows[0].numpy().astype(np.uint8)).decode()
        self.refined_calls.append(t)
        if t.startswith("boom"):
            raise ValueError("tokenizer failed")
        return [t + "!"]

    def code_prompt(self, texts, params):
        self.code_texts.append(texts[0])
        ids = _ids_of(texts[0])
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def prompt_embedding(self, ids, tmask, params, spk_emb_ids):
        return ids[..., :1].float().expand(*ids.shape[:2], 768).clone()

    def decode_to_wavs(self, hids):
        return np.stack([np.full((int(hids[0].shape[0]),), 0.5, np.float32)])

    def decode_windows_pcm16(self, store, windows):
        return [np.full((b - a,), store[slot], np.int16) for slot, prefix, a, b, tail in windows]


class _TickPool:
    """S slots, 8 tokens per launch, a request ends at max_new_token; results come one poll late, like SlotPool.  A text pool's result
    is the prompt's own row ("empty": no tokens); a code pool's hidden states are max_new_token rows.  `hiddens[slot]`: the prompt's
    first byte."""
    POLL = 8

    def __init__(self, S, lock, text):
        self.S, self.lock, self.text = S, lock, text
        self.queue, self.active, self.free, self.ready = [], {}, list(range(S)), []
        self.hiddens = [0] * S
        self.launches, self.steps, self.submitted, self.idle_launches = 0, 0, [], 0

    def submit(self, rid, ids, tmask=None, max_new_token=8, *, params=None, emb=None, stream=None):
        self.submitted.append(rid)
        self.queue.append([rid, ids, int(max_new_token), stream, None, 0, False])

    def cancel(self, rid):
        for q in self.queue:
            if q[0] == rid:
                self.queue.remove(q)
                return True
        for a in self.active.values():
            if a[0] == rid:
                a[6] = True
                return True
        return False

    def busy(self):
        return bool(self.queue or self.active or self.ready)

    def launch(self):
        assert self.lock.locked()
        if not self.busy():
            self.idle_launches += 1
        while self.queue and self.free:
            q, s = self.queue.pop(0), self.free.pop(0)
            q[4] = StreamCursor(q[3]) if q[3] is not None else None
            self.active[s] = q
            self.hiddens[s] = int(q[1][0, 0])
        if not self.active:
            return False
        self.launches += 1
        self.steps += self.POLL
        return True

    def results(self, grouped=False):
        out, self.ready = self.ready, []
        yield from out

    def poll(self, events=False):
        chunks = []
        for s, a in list(self.active.items()):
            rid, ids, n, spec, cur, count, cancelled = a
            if cancelled:
                del self.active[s]
                self.free.append(s)
                continue
            a[5] = count = min(count + 8, n)
            if cur is not None:
                chunks += [(rid, s, *c) for c in (cur.finish(count, True) if count >= n else cur.advance(count))]
            if count >= n:
                del self.active[s]
                self.free.append(s)
                row = ids[:, 0]
                if self.text:
                    self.ready.append((rid, row[:0] if bytes(row.numpy().astype(np.uint8)) == b"empty" else row, torch.zeros((0, 768))))
                else:
                    self.ready.append((rid, ids, torch.zeros((count, 768))))
        if chunks and events:
            yield StreamEvents(chunks)


def _batcher(slots=2, **kw):
    lock = threading.Lock()
    chat, pools = _FakeChat(), {}
    b = SpeechBatcher(chat, slots, lock, make_pool=lambda: pools.setdefault("code", _TickPool(slots, lock, False)),
                      make_text_pool=lambda: pools.setdefault("text", _TickPool(slots, lock, True)), refine=True, streams=True, **kw)
    return b, chat, pools, lock


def test_refined_rows_are_handed_to_the_code_pool_once_in_order():
    b, chat, pools, lock = _batcher(slots=2)
    try:
        with lock:          # taken together: text stage lengths 8 / 8 / 24 / 8 tokens -> hand-offs in completion order, FIFO inside a poll
            futs = [b.submit(t, _Params(16), refine=_Refine(max_new_token=n)) for t, n in (("a", 8), ("b", 8), ("c", 24), ("d", 8))]
            plain = b.submit("p", _Params(8))                        # no refine: straight to the code pool
        sizes = [np.asarray(f.result(timeout=30)).size for f in futs]
        assert sizes == [16] * 4 and np.asarray(plain.result(timeout=30)).size == 8
        assert chat.refined_calls == ["a", "b", "d", "c"]            # 2 slots: a, b first; c (24 tokens) outlasts d
        assert [t for t in chat.code_texts if t != "p"] == ["a!", "b!", "d!", "c!"]      # the helper's text, exactly once each
        assert pools["text"].submitted == [0, 1, 2, 3] and sorted(pools["code"].submitted) == [0, 1, 2, 3, 4]
        occ = b.occupancy()
        r = occ["refine"]
        assert r["admissions"] == 4 and r["handed"] == 4 and r["max_coresident"] == 2 and r["steps"] == pools["text"].steps > 0
        assert r["both_live_polls"] >= 1 and occ["completed"] == 5 and occ["failed"] == 0
    finally:
        b.close()
    assert not lock.locked()


def test_a_failure_in_either_stage_fails_that_request_only():
    b, chat, pools, lock = _batcher(slots=3)
    try:
        with lock:
            ok = b.submit("fine", _Params(8), refine=_Refine(max_new_token=8))
            boom = b.submit("boom", _Params(8), refine=_Refine(max_new_token=8))           # the tokenizer fails at the hand-off
            empty = b.submit("empty", _Params(8), refine=_Refine(max_new_token=8))         # an empty refined row
            bad = b.submit("bad", _Params(8), refine=_Refine(max_new_token=8, repetition_penalty=1.2))
        assert np.asarray(ok.result(timeout=30)).size == 8
        with pytest.raises(ValueError, match="tokenizer failed"):
            boom.result(timeout=30)
        with pytest.raises(RuntimeError, match="no tokens"):
            empty.result(timeout=30)
        assert bad.result(timeout=30) is not None                    # (the fake text pool validates nothing: served)
        assert chat.code_texts.count("fine!") == 1 and "boom!" not in chat.code_texts
        occ = b.occupancy()
        assert occ["failed"] == 2 and occ["completed"] == 2 and occ["refine"]["handed"] == 2
        with pytest.raises(RuntimeError, match="refine=True"):
            SpeechBatcher.submit(type("B", (), {"refine": False, "_check_refine": SpeechBatcher._check_refine})(), "x", None, refine=_Refine())
    finally:
        b.close()


def test_a_stream_is_cancelled_in_whichever_pool_it_is():
    b, chat, pools, lock = _batcher(slots=2)
    try:
        with lock:
            s1 = b.submit_stream("s", _Params(400), refine=_Refine(max_new_token=4000))      # still in the text pool when closed
            s2 = b.submit_stream("t", _Params(400), refine=_Refine(max_new_token=8))         # closed during the code stage
        first = next(s2)
        assert first.size > 0
        s1.close()
        s2.close()
        assert list(s1) == [] and list(s2) == []
        deadline = time.time() + 10
        while (pools["text"].busy() or pools["code"].busy()) and time.time() < deadline:
            time.sleep(0.01)
        assert not pools["text"].busy() and not pools["code"].busy(), "a cancelled stream kept its slot"
        occ = b.occupancy()
        assert occ["cancelled"] == 2 and occ["refine"]["handed"] == 1 and pools["code"].submitted == [1]
        s3 = b.submit_stream("u", _Params(30), refine=_Refine(max_new_token=8))              # the freed slots serve the next one
        assert sum(c.size for c in s3) == 256 * (2 * 30 - 1)
    finally:
        b.close()


def test_only_pools_with_work_are_launched_and_plain_requests_never_touch_the_text_pool():
    b, chat, pools, lock = _batcher(slots=2)
    try:
        assert np.asarray(b.submit("one", _Params(24)).result(timeout=30)).size == 24
        assert np.asarray(b.submit("two", _Params(8), refine=None).result(timeout=30)).size == 8
        assert pools["text"].submitted == [] and pools["text"].launches == 0 and pools["text"].idle_launches == 0
        assert chat.refined_calls == [] and pools["code"].launches >= 3 + 1
        before = pools["code"].launches
        assert np.asarray(b.submit("three", _Params(8), refine=_Refine(max_new_token=40)).result(timeout=30)).size == 8
        assert pools["text"].launches == 5                            # 40 text tokens, 8 per launch
        assert pools["code"].launches == before + 1 and pools["code"].idle_launches == 0 and pools["text"].idle_launches == 0
        assert b.occupancy()["refine"]["both_live_polls"] == 0
    finally:
        b.close()


def test_a_batcher_without_refine_is_what_it_was():
    lock = threading.Lock()

    class _RunPool(_TickPool):
        def run(self, between=None):
            while self.busy():
                between()
                self.launch()
                yield from self.results()
                yield from self.poll()
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _RunPool(2, lock, False))
    try:
        assert b.text_pool is None and "refine" not in b.occupancy()
        assert np.asarray(b.submit("one", _Params(8)).result(timeout=30)).size == 8
        with pytest.raises(RuntimeError, match="refine=True"):
            b.submit("one", _Params(8), refine=_Refine())
    finally:
        b.close()

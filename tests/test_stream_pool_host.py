"""Streamed requests in the shared batch, the parts that need no GPU: the window-decode C ABI (symbols, refusals), the window arithmetic
shared by `decode_window` and `decode_windows`, the per-request chunk schedule against the serial streamed path driven with fakes, and
`SpeechBatcher.submit_stream` on a fake pool."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest
import torch

from chattts_amd import _lib
from chattts_amd.core import Chat
from chattts_amd.engine import HALO_FRAMES, window_for_samples
from chattts_amd.serving import SpeechBatcher, StreamCursor, StreamEvents, StreamSpec, stream_schedule

NEW_SYMBOLS = ("ctts_codec_windows_workspace_bytes", "ctts_codec_decode_windows")


# ---- 1. C ABI -------------------------------------------------------------------------------------------------------------------
def test_window_symbols_are_exported_and_declared():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert "} ctts_window;" in header


def test_windows_workspace_holds_the_ragged_workspace_and_the_packed_stages():
    lib = _lib.lib()
    f = lib.ctts_codec_windows_workspace_bytes
    assert f(0, 10) == 0 and f(5, 4) == 0
    prev = 0
    for n_win, total in ((1, 1), (1, 76), (8, 8 * 76), (8, 8 * 127), (16, 3000)):
        n = f(n_win, total)
        # the ragged workspace + packed hidden rows + token offsets + mel + the windows' waveforms
        assert n >= lib.ctts_codec_ragged_workspace_bytes(n_win, total) + total * 768 * 4 + (n_win + 1) * 4 + 2 * total * 100 * 4 \
            + 256 * (2 * total - n_win) * 4
        assert n >= prev and n % 256 == 0
        prev = n


def _table(rows):
    a = np.ascontiguousarray(np.array([[*r, 0, 0] for r in rows], dtype=np.int32))
    return a, a.ctypes.data_as(C.c_void_p)


def test_decode_windows_refuses_bad_tables_without_a_device():
    """every refusal comes from the host mirror before anything is launched: the pointers below are never dereferenced"""
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    S, cap = 8, 64

    def call(rows, n_win=None, keep=fake, ws=1 << 40, out_type=1, product=0, strides=(cap * 768, 768)):
        tab, p = _table(rows)
        return lib.ctts_codec_decode_windows(fake, fake, strides[0], strides[1], S, cap, fake, p, len(rows) if n_win is None else n_win, out_type,
                                             fake, keep, product, 1e-5, fake, ws, None)
    ok = (0, 0, 40, 0, 12000, 0)        # (slot, t_lo, t_hi, c_lo, c_hi, keep): 40 tokens decode to 256 * 79 = 20224 samples
    for rows, msg in (([(0, 5, 5, 0, 10, 0)], b"empty"), ([(0, 7, 3, 0, 10, 0)], b"empty"), ([ok, (0, 0, cap + 1, 0, 10, 0)], b"capacity"),
                      ([(S, 0, 4, 0, 10, 0)], b"slot"), ([(-1, 0, 4, 0, 10, 0)], b"slot"), ([(0, 0, 40, 0, 20225, 0)], b"outside"),
                      ([(0, 0, 40, -1, 10, 0)], b"outside"), ([(0, 0, 40, 10, 10, 0)], b"outside"), ([(0, -1, 40, 0, 10, 0)], b"empty")):
        assert call(rows) != 0 and msg in lib.ctts_last_error(), (rows, lib.ctts_last_error())
    assert call([ok], n_win=0) != 0 and b"n_win" in lib.ctts_last_error()
    assert call([(0, 0, 40, 0, 100, 1)], keep=None) != 0 and b"keep" in lib.ctts_last_error()
    assert call([ok], ws=1024) != 0 and b"workspace" in lib.ctts_last_error()
    assert call([ok], out_type=2) != 0 and call([ok], product=2) != 0
    assert call([ok], strides=(cap * 768, 770)) != 0 and call([ok], strides=(cap * 768 - 4, 768)) != 0      # rows must stay 16-byte aligned
    tab, p = _table([ok])
    assert lib.ctts_codec_decode_windows(None, fake, cap * 768, 768, S, cap, fake, p, 1, 1, fake, None, 0, 1e-5, fake, 1 << 40, None) != 0


# ---- 2. window arithmetic ------------------------------------------------------------------------------------------------------
def _decode_window_arith(Tn, s_lo, s_hi):
    """the arithmetic `CodecEngine.decode_window` carried before it was shared, restated: (t_lo, t_hi, crop lo, crop hi) or None"""
    hop, nfft, halo = 256, 1024, 27 + 75
    total = hop * (2 * Tn - 1)
    s_lo, s_hi = max(0, int(s_lo)), min(total, int(s_hi))
    if s_hi <= s_lo:
        return None
    f_a = (s_lo + nfft // 2) // hop - (nfft // hop - 1)
    f_b = min((s_hi - 1 + nfft // 2) // hop, 2 * Tn - 1)
    t_lo = max(0, (f_a - halo) // 2)
    t_hi = min(Tn, (f_b + halo) // 2 + 1)
    off = 2 * hop * t_lo
    return t_lo, t_hi, s_lo - off, s_hi - off


def test_window_for_samples_is_decode_windows_arithmetic():
    assert HALO_FRAMES == 102
    n = 0
    for Tn in (1, 2, 24, 25, 48, 51, 52, 53, 96, 127, 500, 2048):
        total = 256 * (2 * Tn - 1)
        los = sorted({0, 1, 255, 256, 12000, 24000, total - 12000, total - 1, total, total + 5} & set(range(0, total + 6)))
        for s_lo in los:
            for s_hi in (s_lo, s_lo + 1, s_lo + 12000, total, total + 1000, 0):
                got, want = window_for_samples(Tn, s_lo, s_hi), _decode_window_arith(Tn, s_lo, s_hi)
                assert got == want, (Tn, s_lo, s_hi, got, want)
                n += 1
                if got is None:
                    assert min(s_hi, total) <= s_lo       # empty ranges, and ranges that start at or past the prefix end
                    continue
                t_lo, t_hi, c_lo, c_hi = got
                assert 0 <= t_lo < t_hi <= Tn and 0 <= c_lo < c_hi <= 256 * (2 * (t_hi - t_lo) - 1)     # what the C entry requires
                assert c_hi - c_lo == min(s_hi, total) - s_lo and c_lo == s_lo - 512 * t_lo
                if s_lo == 0:
                    assert t_lo == 0 and c_lo == 0
                if min(s_hi, total) == total:
                    assert t_hi == Tn                     # a range that ends at the prefix end: the window's edge is the sequence's
    assert n > 300
    assert window_for_samples(500, 100000, 112000) == (143, 271, 26784, 38784)   # (392 - 3 - 102) // 2, (439 + 102) // 2 + 1, 100000 - 512 * 143


# ---- 3. the schedule against the serial streamed path ---------------------------------------------------------------------------------
class _Out:
    def __init__(self, n):
        self.hiddens, self.ids = [torch.zeros((n, 1))], [torch.zeros((n, 4), dtype=torch.int64)]

    def destroy(self):
        pass


def _reference_yields(n, max_new, stream_batch):
    """`GPT.generate(stream=True)` for ONE row that draws EOS at step `n` (or never, when n == max_new), restated step by step: the
    row's token count at every yield, the final result included (the reference's loop: end_idx and stream_iter advance while the row is
    unfinished, a yield whenever stream_iter is a positive multiple of stream_batch -- also at the step that finished the row)"""
    end_idx = stream_iter = 0
    finish = False
    out = []
    for i in range(max_new):
        finish = finish or i == n
        if i == 0 and finish:
            return []                       # "unexpected end at index": nothing is yielded (seeded request)
        end_idx += int(not finish)
        stream_iter += int(not finish)
        if stream_iter > 0 and stream_iter % stream_batch == 0:
            out.append(end_idx)
        if finish:
            break
    return out + [end_idx]


def _serial_calls(n, max_new, spec, entry):
    """the `_stream_piece` calls of the serial streamed path for a one-row batch: [(prefix tokens, a, b clipped to the prefix, tail)]"""
    chat = Chat()
    chat.device = "cpu"
    chat.normalizer = lambda t, *a: t
    chat.has_loaded = lambda use_decoder=True: True
    gen = lambda *a, **k: (_Out(k_) for k_ in _reference_yields(n, max_new, spec.stream_batch))
    chat._infer_code = gen
    chat.infer_code = gen
    calls = []

    def piece(hiddens, a, b, use_decoder=True, pcm16=False):
        Tn = int(hiddens[0].shape[0])
        total = 256 * (2 * Tn - 1)
        hi = total if b is None else min(b, total)
        calls.append((Tn, a, max(a, hi), b is None))
        return np.zeros((1, max(0, hi - a)), np.int16 if pcm16 else np.float32)
    chat._stream_piece = piece
    params = Chat.InferCodeParams(stream_batch=spec.stream_batch, stream_speed=spec.stream_speed, pass_first_n_batches=spec.pass_first_n_batches)
    if entry == "infer":
        chunks = list(chat.infer(["x"], stream=True, skip_refine_text=True, params_infer_code=params, pcm16=True))
    else:
        chunks = list(chat.infer_ids_stream(None, None, None, params))
    assert len(chunks) == len(calls)
    return calls


@pytest.mark.parametrize("passed", [0, 2])
@pytest.mark.parametrize("n", [1, 23, 24, 25, 47, 48, 71, 72, 73, 96, 97, 500])
def test_schedule_equals_the_serial_streamed_path(n, passed):
    spec = StreamSpec(24, 12000, passed)
    polls = list(range(8, n, 8))                     # the counts a live slot shows at the pool's polls (POLL = 8)
    for eos, max_new in ((True, 2048), (False, n)):  # ended by EOS / cut at max_new_token (no duplicate yield there)
        want = _serial_calls(n, max_new, spec, "infer")
        assert want == _serial_calls(n, max_new, spec, "infer_ids_stream")
        got = stream_schedule(polls, n, eos, spec)
        assert got == want, (n, passed, eos, got, want)
        assert got[-1] == (n, got[-2][2] if len(got) > 1 else 0, 256 * (2 * n - 1), True) and not any(c[3] for c in got[:-1])
        # where the polls fall does not matter: every third poll only, or none before the end
        assert stream_schedule(polls[::3], n, eos, spec) == want and stream_schedule([], n, eos, spec) == want
    if n == 96:     # the duplicate yield: 24, 48, 72, 96, 96 again, then the final result -- six yields, one fewer without EOS
        assert len(stream_schedule(polls, n, True, spec)) == 6 - passed + 1 and len(stream_schedule(polls, n, False, spec)) == 5 - passed + 1


def test_schedule_small_speed_and_empty_results():
    spec = StreamSpec(24, 3000, 0)
    for n in (30, 48, 100):
        assert stream_schedule(range(8, n, 8), n, True, spec) == _serial_calls(n, 2048, spec, "infer")
    assert stream_schedule([], 0, True, spec) == []                    # step 0 drew EOS: nothing to stream
    huge = StreamSpec(24, 10 ** 6, 1)
    assert stream_schedule([8, 16, 24, 32], 40, True, huge) == _serial_calls(40, 2048, huge, "infer")
    cur = StreamCursor(StreamSpec(24, 12000, 0))
    assert cur.advance(23) == [] and cur.advance(24) == [(24, 0, 12000, False)] and cur.advance(40) == []
    with pytest.raises(ValueError):
        StreamCursor(StreamSpec(0, 12000, 0))


# ---- 4. SpeechBatcher.submit_stream on a fake pool -----------------------------------------------------------------------------------
class _Params:
    def __init__(self, n_tokens, passed=0):
        self.spk_emb, self.max_new_token = "spk", n_tokens
        self.stream_batch, self.stream_speed, self.pass_first_n_batches = 24, 12000, passed


class _Tok:
    spk_emb_ids = 7


class _FakeChat:
    """prompt = the text's bytes; a window's audio = a ramp that names its slot's request, prefix and sample index"""
    tokenizer = _Tok()

    def __init__(self):
        self.window_calls = []

    def normalizer(self, text, norm, homophones, lang):
        return text

    def code_prompt(self, texts, params):
        t = np.frombuffer(texts[0].encode(), dtype=np.uint8).astype(np.int64)
        ids = torch.from_numpy(np.repeat(t[None, :, None], 4, axis=2))
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def prompt_embedding(self, ids, tmask, params, spk_emb_ids):
        return ids[..., :1].float().expand(*ids.shape[:2], 768).clone()

    def decode_to_wavs(self, hids):
        return np.stack([np.full((4,), 0.5, np.float32)])

    def decode_windows_pcm16(self, store, windows):
        self.window_calls.append(list(windows))
        return [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]


def _piece(tag, prefix, a, b):
    return ((np.arange(a, b) + 1000 * prefix + tag) % 30000).astype(np.int16)


class _FakePool:
    """S slots, 8 tokens per chunk, a request ends at its max_new_token (by 'EOS'); text "empty": step 0 drew EOS.  `hiddens[slot]` is
    the tag of the request in that slot; run(events=True) yields StreamEvents at the poll, results one poll later, like SlotPool"""

    def __init__(self, S, lock):
        self.S, self.lock = S, lock
        self.queue, self.active, self.free = [], {}, list(range(S))
        self.hiddens = [0] * S
        self.admitted = []

    def submit(self, rid, ids, tmask, max_new_token, *, params, emb, stream=None):
        self.queue.append([rid, ids, max_new_token, stream, None, 0, False])

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

    def run(self, between=None, grouped=False, events=False):
        assert events
        late = []
        while self.queue or self.active or late:
            if between is not None:
                between()
            assert self.lock.locked()
            while self.queue and self.free:
                q = self.queue.pop(0)
                s = self.free.pop(0)
                q[4] = StreamCursor(q[3]) if q[3] is not None else None
                self.active[s] = q
                self.hiddens[s] = int(q[1][0, 0])
                self.admitted.append((q[0], s))
            time.sleep(0.001)
            yield from late
            late = []
            chunks = []
            for s, a in list(self.active.items()):
                rid, ids, n, spec, cur, count, cancelled = a
                if cancelled:
                    del self.active[s]
                    self.free.append(s)
                    continue
                text = bytes(ids[:, 0].numpy().astype(np.uint8)).decode()
                a[5] = count = 0 if text == "empty" else min(count + 8, n)
                ended = count >= n or text == "empty"
                if cur is not None:
                    chunks += [(rid, s, *c) for c in (cur.finish(count, True) if ended else cur.advance(count))]
                if ended:
                    del self.active[s]
                    self.free.append(s)
                    late.append((rid, ids, torch.zeros((count, 768))))
            if chunks:
                yield StreamEvents(chunks)
        yield from late


def _expected(tag, n, passed):
    return [_piece(tag, p, a, b) for p, a, b, _ in stream_schedule([], n, True, StreamSpec(24, 12000, passed))]


def test_submit_stream_routes_interleaved_chunks_groups_a_poll_and_isolates_cancel_and_empty():
    lock = threading.Lock()
    chat = _FakeChat()
    holder = {}
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True)
    try:
        with pytest.raises(RuntimeError):
            SpeechBatcher.submit_stream(type("B", (), {"streams": False})(), "x", None)
        with lock:       # submitted together: admitted in one chunk, so their chunks fall due at the same polls
            s1, s2, s3 = b.submit_stream("A", _Params(96)), b.submit_stream("B", _Params(72, passed=1)), b.submit_stream("C", _Params(50))
            s4 = b.submit_stream("empty", _Params(40))          # queued behind the three slots
            s5 = b.submit_stream("D", _Params(400))             # cancelled mid-stream
            f6 = b.submit("E", _Params(16))                     # a non-streamed request beside them
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in (("A", s1), ("B", s2), ("C", s3))]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        for k, n, passed in (("A", 96, 0), ("B", 72, 1), ("C", 50, 0)):
            want = _expected(ord(k), n, passed)
            assert len(got[k]) == len(want) and all(np.array_equal(g, w) for g, w in zip(got[k], want)), k     # its own chunks, in order
        with pytest.raises(RuntimeError, match="no audio"):
            list(s4)                                             # the empty result ends only its own iterator
        first = [next(s5), next(s5)]
        s5.close()                                               # the consumer goes away
        assert list(s5) == [] and all(np.array_equal(g, w) for g, w in zip(first, _expected(ord("D"), 400, 0)))
        assert np.asarray(f6.result(timeout=30)).size == 4
        s7 = b.submit_stream("F", _Params(30))                   # served after the cancel, from a freed slot
        assert all(np.array_equal(g, w) for g, w in zip(list(s7), _expected(ord("F"), 30, 0)))
        deadline = time.time() + 10
        while holder["p"].active and time.time() < deadline:
            time.sleep(0.01)
        occ = b.occupancy()
        assert not holder["p"].active and sorted(holder["p"].free) == [0, 1, 2], "the cancelled stream's slot was not freed"
        assert occ["cancelled"] == 1 and occ["failed"] == 1 and occ["completed"] == 5 and occ["streams"] == 0
        # chunks due at one poll went into one decode call: A and B both yield at 24 / 48 / 72 tokens
        assert occ["max_stream_group"] >= 2 and occ["stream_decode_calls"] == len(chat.window_calls) < occ["stream_chunks"]
        assert any({w[0] for w in call} >= {0, 1} for call in chat.window_calls)
        d_total = sum(len(call) for call in chat.window_calls)
        assert occ["stream_chunks"] == d_total
    finally:
        b.close()
    assert not lock.locked()


def test_batcher_without_streams_reports_no_stream_counters():
    lock = threading.Lock()

    class _Plain(_FakePool):
        def run(self, between=None, grouped=False):
            yield from _FakePool.run(self, between, grouped, events=True)
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _Plain(2, lock))
    try:
        assert np.asarray(b.submit("one", _Params(8)).result(timeout=30)).size == 4
        assert "max_stream_group" not in b.occupancy()
    finally:
        b.close()

"""Streamed requests in the shared batch on the GPU: the window decode (ctts_codec_decode_windows) against `decode_window` alone and
against the serial PCM16 conversion, streams through a real `SlotPool` against the serial schedule replayed over the same hidden states,
the endpoint with `batch_streams=True`, and a cancelled stream.  `pytest -m gpu`."""
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, StreamEvents, StreamSpec, request_params  # noqa: E402

DEV = torch.device("cuda:0")
THR = np.float32(1e-5)

# (slot, prefix tokens, s_lo, s_hi, tail): a first chunk at sample 0, mid-sequence chunks (token window inside the prefix, both halos
# cut), a chunk clipped by the prefix end (30 tokens = 15,104 samples), tails, a one-token prefix
WINDOWS = [(0, 24, 0, 12000, False), (1, 96, 24000, 36000, False), (2, 150, 60000, 72000, False), (3, 30, 12000, 24000, False),
           (4, 100, 36000, None, True), (5, 1, 0, None, True), (6, 160, 70000, 82000, False), (7, 48, 12000, 24000, False)]


def _store(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((8, 160, 768), device=DEV, generator=g)


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("gemm", ["f32", "bf16x3", "f16"])
def test_window_decode_equals_decode_window_alone(weights, gemm):
    """1 to 8 windows at different positions of 8 slots, float32 output: each window == `decode_window([store[s, :Tn]], s_lo, s_hi)[0]`
    bit for bit in f32 and bf16x3 (the ragged decoder's bar, no tolerance).  f16: bit for bit while the pack stays below 1,024 frames
    (both sides on split-bf16 tiles), else within the mode's 2e-5 RMS."""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    store = _store()
    alone = [codec.decode_window([store[s, :Tn]], a, 256 * (2 * Tn - 1) if b is None else b)[0].cpu().numpy() for s, Tn, a, b, _ in WINDOWS]
    for k in range(1, len(WINDOWS) + 1):
        wins = WINDOWS[:k]
        got = codec.decode_windows(store, [w[:4] for w in wins], pcm16=False)
        frames = sum(2 * (t[1] - t[0]) for t in (E.window_for_samples(Tn, a, 256 * (2 * Tn - 1) if b is None else b) for _, Tn, a, b, _ in wins))
        for i, (g, w) in enumerate(zip(got, alone)):
            assert g.dtype == np.float32 and g.shape == w.shape, (k, i, g.shape, w.shape)
            if gemm != "f16" or frames < 1024:
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (gemm, k, i, float(np.abs(g - w).max()))
            else:
                r = _rms(g, w)
                print(f"window decode[f16] pack of {k} ({frames} frames), window {i}: rms {r:.2e}")
                assert r < 2e-5, (k, i, r)
    # windows of one slot at several positions in one call (a stream whose yield, duplicate yield and tail fall due together)
    multi = [(2, 48, 0, 12000), (2, 48, 12000, 24000), (2, 48, 24000, None), (2, 47, 0, 12000)]
    if gemm != "f16":
        for g, (s, Tn, a, b) in zip(codec.decode_windows(store, multi, pcm16=False), multi):
            w = codec.decode_window([store[s, :Tn]], a, 256 * (2 * Tn - 1) if b is None else b)[0].cpu().numpy()
            assert np.array_equal(g, w), (s, Tn, a, b)
    # ranges with nothing in them come back empty and take no part in the decode
    got = codec.decode_windows(store, [(0, 24, 12032, 24000), (1, 96, 0, 12000), (2, 0, 0, 100)], pcm16=False)
    assert got[0].size == 0 and got[2].size == 0 and np.array_equal(got[1], codec.decode_window([store[1, :96]], 0, 12000)[0].cpu().numpy())
    with pytest.raises(ValueError):
        codec.decode_windows(store, [(8, 24, 0, 100)])


@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_window_pcm16_equals_the_serial_conversion(weights, gemm):
    """int16 output == `codec.float_to_int16(win, per_row=True)` of the float windows byte for byte; a tail compacted by its keep mask
    == the serial tail (`float_to_int16(w[|w| > 1e-5])` on the host); a tail with nothing above the threshold is an empty array"""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    store = _store(5)
    store[5, 0] *= 1e-3            # a quiet one-token tail: its samples straddle the strip threshold less one-sidedly
    flt = codec.decode_windows(store, [w[:4] for w in WINDOWS], pcm16=False)
    pcm = codec.decode_windows(store, WINDOWS, pcm16=True, keep_thr=1e-5)
    raw = codec.decode_windows(store, [w[:4] for w in WINDOWS], pcm16=True)       # no strip: every window whole
    for i, (w, f, p, r) in enumerate(zip(WINDOWS, flt, pcm, raw)):
        dev_pcm = codec.float_to_int16(torch.from_numpy(f).to(DEV)[None], per_row=True)[0][0].cpu().numpy()
        assert r.dtype == np.int16 and r.tobytes() == dev_pcm.tobytes(), i
        assert r.tobytes() == float_to_int16(f).tobytes(), i
        if w[4]:
            want = float_to_int16(f[np.abs(f) > THR])
            assert p.dtype == np.int16 and p.tobytes() == want.tobytes(), (i, p.shape, want.shape)
        else:
            assert p.tobytes() == r.tobytes(), i
    # the mask itself, where it cuts through the middle of the samples; and a tail with nothing to keep
    f = flt[4]
    thr = float(np.median(np.abs(f)))
    got = codec.decode_windows(store, [WINDOWS[4], WINDOWS[0]], pcm16=True, keep_thr=thr)
    kept = np.abs(f) > np.float32(thr)
    assert 0 < kept.sum() < f.size and got[0].tobytes() == float_to_int16(f)[kept].tobytes() and got[1].tobytes() == raw[0].tobytes()
    silent = codec.decode_windows(store, [WINDOWS[4], WINDOWS[5]], pcm16=True, keep_thr=1e6)
    assert all(s.dtype == np.int16 and s.size == 0 for s in silent)
    f_tail = codec.decode_windows(store, [WINDOWS[4]], pcm16=False, keep_thr=thr)[0]
    assert np.array_equal(f_tail, f[kept])


# ---- streams through a real pool ----------------------------------------------------------------------------------------------------
def _engine(weights, dtype):
    return E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype, exact_fallback=False, certify=False)


def _alone_stream(eng, ids, p, max_new, stop_at, stream_batch):
    """the request alone at batch 1, streamed: (final outputs, the token count at every yield, the final result included)"""
    rp = request_params(p)
    w, pr = E.gen_logits(625, p["top_P"], p["top_K"], p["repetition_penalty"])
    ids_t = ids[None]
    emb = eng.embed_prompt(ids_t, torch.ones((1, ids.shape[0]), dtype=torch.bool))
    counts, last = [], None
    for out in eng.generate(emb, ids_t, torch.tensor(rp.temperature), 625, None, max_new, rp.min_new_token, (*pr, *w), return_hidden=True,
                            stream=True, stream_batch=stream_batch, manual_seed=rp.manual_seed,
                            stop_at=None if stop_at < 0 else torch.tensor([stop_at], dtype=torch.int32)):
        counts.append(int(out.hiddens[0].shape[0]))
        last = out
    return last, counts


def _serial_chunks(chat, hid, counts, spec):
    """the `stream` branch of `Chat._infer` (pcm16, one text) replayed over `hid`: generate's yields are prefixes of it"""
    chunks, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        piece = chat._stream_piece([hid[:n]], length, length + spec.stream_speed, True, True)
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
        chunks.append(piece[0])
    w = chat._stream_piece([hid], length, None, True)[0]
    w = w[np.abs(w) > 1e-5]
    chunks.append(float_to_int16(w) if w.size else w.astype(np.int16))
    return chunks


def _drive(pool, codec):
    """pool.run(events=True) with the consumer the batcher is: one window decode per StreamEvents"""
    chunks, results, groups = {}, {}, []
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            groups.append(len(got.chunks))
            for c, pcm in zip(got.chunks, codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5)):
                chunks.setdefault(c[0], []).append(pcm)
        else:
            results[got[0]] = (got[1].cpu().numpy(), got[2])
    return chunks, results, groups


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_pooled_stream_equals_the_stream_of_its_own_hidden_states(weights, dtype):
    """12 requests through 8 slots, 9 streamed (lengths that end below, on and above yield boundaries; forced ends stand in for EOS and
    bring the duplicate yield; two window sizes, 0 and 2 passed batches) and 3 not: every stream's chunks (count, lengths, bytes) ==
    the serial schedule -- the yields of the request generated ALONE with stream=True -- replayed over the hidden states the pool
    returned for it; ids == the alone run"""
    eng = _engine(weights, dtype)
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec = codec
    pool = SlotPool(eng, slots=8, cap=256, hid_cap=128, per_request=True)
    rs = np.random.RandomState(21)
    # (max_new, stop_at, streamed, stream_speed, passed)
    plan = [(96, -1, True, 12000, 2), (40, -1, True, 12000, 0), (100, 48, True, 12000, 2), (72, -1, True, 3000, 0), (30, -1, False, 0, 0),
            (100, 24, True, 12000, 0), (97, -1, True, 12000, 2), (23, -1, True, 12000, 0), (64, -1, False, 0, 0), (120, 96, True, 12000, 2),
            (49, -1, True, 5000, 1), (56, -1, False, 0, 0)]
    reqs = {}
    for i, (max_new, stop, streamed, speed, passed) in enumerate(plan):
        T = int(rs.randint(4, 30))
        ids = torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(T, 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(500 + 13 * i))
        spec = StreamSpec(24, speed, passed) if streamed else None
        reqs[i] = (ids, p, max_new, stop, spec)
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=spec)
    chunks, results, groups = _drive(pool, codec)
    assert sorted(results) == list(range(12)) and not pool.active and len(pool.free) == 8
    assert sorted(chunks) == [i for i, r in reqs.items() if r[4] is not None] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec) in reqs.items():
        ref, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        assert np.array_equal(results[i][0], ref.ids[0].cpu().numpy()), (i, results[i][0].shape, ref.ids[0].shape)
        if spec is None:
            continue
        want = _serial_chunks(chat, results[i][1], counts, spec)
        got = chunks[i]
        assert [g.shape for g in got] == [w.shape for w in want], (i, counts, [g.shape for g in got], [w.shape for w in want])
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (i, k)
    pool.close()


def test_cancelled_stream_frees_its_slot_for_a_queued_request(weights):
    """2 slots, a long stream cancelled after its first chunk event: the queued request takes the slot, its ids == its alone run, and
    nothing more is handed out for the cancelled one"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    pool = SlotPool(eng, slots=2, cap=512, hid_cap=400, per_request=True)
    rs = np.random.RandomState(4)
    mk = lambda: torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(int(rs.randint(4, 20)), 1)), 4, axis=1).astype(np.int64))
    p = lambda i: dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=900 + i)
    reqs = {"long": (mk(), p(0), 380), "other": (mk(), p(1), 60), "queued": (mk(), p(2), 50)}
    for rid, (ids, pp, max_new) in reqs.items():
        # (forced lengths: random weights may draw EOS anywhere, and the order of events below rests on the lengths)
        pool.submit(rid, ids, max_new_token=max_new, stop_at=max_new, params=pp, stream=StreamSpec(24, 12000, 0))
    seen, results, steps_at_cancel = {}, {}, None
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            pcm = codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5)
            for c, a in zip(got.chunks, pcm):
                seen.setdefault(c[0], []).append(a)
            if steps_at_cancel is None and "long" in seen:
                assert pool.cancel("long")
                steps_at_cancel = pool.steps
        else:
            results[got[0]] = got[1].cpu().numpy()
    assert sorted(results) == ["other", "queued"] and len(seen["long"]) <= 3 and not pool.active and sorted(pool.free) == [0, 1]
    assert pool.slot_of["queued"] == pool.slot_of["long"] and pool.steps < steps_at_cancel + 200      # the long request did not run on
    assert not pool.cancel("long")
    for rid in ("other", "queued"):
        ids, pp, max_new = reqs[rid]
        ref, _ = _alone_stream(eng, ids, pp, max_new, max_new, 24)
        assert np.array_equal(results[rid], ref.ids[0].cpu().numpy()), rid
    pool.close()


# ---- the endpoint ------------------------------------------------------------------------------------------------------------------
def _chunked(body, header_len=44):
    return body[header_len:]


def test_endpoint_streams_from_the_shared_batch(weights):
    """create_app(chat, voices, batch_slots=8, batch_streams=True): 4 streamed and 4 non-streamed requests from threads.  Every
    streamed body: the serial streamed endpoint's chunk count and bytes per chunk (recorded at the batcher's queue), samples within
    1 LSB; a tail of another length fails.  Precondition asserted: no serial tail sample sits within 1e-6 of the strip threshold."""
    import io
    import wave
    from starlette.testclient import TestClient
    from chattts_amd import server
    gold_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(gold_dir, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32", tokenizer=os.path.join(gold_dir, "tokenizer"), spk_stat=spk_stat)
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker(), "alloy": chat.sample_random_speaker(), "echo": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 120})      # random weights do not stop on cue
    # (text, voice) pairs whose serial tails keep every sample at least 1.8e-6 away from the strip threshold (measured on the serial
    # path, f32: 1.9e-6, 2.6e-6, 3.4e-6, 5.2e-6), and whose lengths differ: 120 tokens (cut at max_new_token), 51, 48 (EOS exactly on a
    # yield boundary: the duplicate yield) and 23 (a tail only)
    s_texts = ["One more short line.", "See you tomorrow at noon.", "A streamed sentence.", "The weather is fine today."]
    s_voices = ["alloy", "echo", "echo", "default"]
    n_texts = ["Hello there.", "The quick brown fox jumps over the lazy dog.", "Good morning!", "How are you today?"]

    def pcm_of(r):
        with wave.open(io.BytesIO(r.content), "rb") as wf:
            return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")

    try:
        # the serial app: bodies, and every stream's chunk list as Chat.infer yields it (+ the float tail for the precondition)
        serial = server.create_app(chat, voices)
        want_chunks = []
        with TestClient(serial) as c:
            want_n = [pcm_of(c.post("/v1/audio/speech", json={"input": t, "response_format": "wav"})) for t in n_texts]
            want_s = [c.post("/v1/audio/speech", json={"input": t, "voice": v, "response_format": "wav", "stream": True}).content
                      for t, v in zip(s_texts, s_voices)]
        for t, v in zip(s_texts, s_voices):
            p = orig(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=120, min_new_token=0,
                     show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=voices[v], stream_batch=24, stream_speed=12000,
                     pass_first_n_batches=2)
            want_chunks.append([np.asarray(x).reshape(-1) for x in chat.infer([t], stream=True, skip_refine_text=True, params_infer_code=p, pcm16=True)])
            flt = [np.asarray(x).reshape(-1) for x in chat.infer([t], stream=True, skip_refine_text=True, params_infer_code=p)]
            emitted = sum(x.size for x in flt[:-1])
            assert emitted == sum(x.size for x in want_chunks[-1][:-1])
            # precondition: the tail's length does not hinge on a sample that sits at the strip threshold
            hid = next(chat._infer_code([chat.normalizer(t, True, True, None)], False, DEV, True, p)).hiddens
            full = chat._stream_piece(hid, emitted, None, True)[0]
            assert not np.any(np.abs(np.abs(full.astype(np.float64)) - 1e-5) < 1e-6), t
        assert all(b"".join(x.astype("<i2").tobytes() for x in ch) == _chunked(w) for ch, w in zip(want_chunks, want_s))

        app = server.create_app(chat, voices, batch_slots=8, batch_streams=True)
        b = app.state.batcher
        got_chunks = {}
        orig_serve = b._serve_chunks

        def serve(ev):
            orig_serve(ev)
            for c in ev.chunks:
                got_chunks.setdefault(c[0], []).append(c[2:])
        b._serve_chunks = serve
        res_s, res_n = [None] * 4, [None] * 4
        with TestClient(app) as c:
            def streamed(i):
                res_s[i] = c.post("/v1/audio/speech", json={"input": s_texts[i], "voice": s_voices[i], "response_format": "wav", "stream": True})

            def plain(i):
                res_n[i] = c.post("/v1/audio/speech", json={"input": n_texts[i], "response_format": "wav"})
            ths = [threading.Thread(target=streamed, args=(i,)) for i in range(4)] + [threading.Thread(target=plain, args=(i,)) for i in range(4)]
            for th in ths:
                th.start()
            for th in ths:
                th.join(timeout=600)
            health = c.get("/health").json()
        b.close()
        assert all(r is not None and r.status_code == 200 for r in res_s + res_n)
        for i in range(4):
            g, w = pcm_of(res_n[i]), want_n[i]
            assert g.shape == w.shape and (np.abs(g.astype(np.int32) - w.astype(np.int32)).max() if g.size else 0) <= 1, i
        # per stream: the schedule the batcher served == the serial chunk list's lengths (the tail's before the strip is not comparable:
        # its length after the strip is), and the body == the serial body within 1 LSB, sample for sample
        by_len = {}
        for rid, sched in got_chunks.items():
            by_len[tuple(bb - a for _, a, bb, tail in sched if not tail)] = sched
        for i in range(4):
            lens = tuple(x.size for x in want_chunks[i][:-1])
            assert lens in by_len, (i, lens, list(by_len))
            assert len(by_len[lens]) == len(want_chunks[i]), i
            body, want = res_s[i].content, want_s[i]
            assert body[:44] == want[:44] == server.wav_stream_header()
            g, w = np.frombuffer(body[44:], dtype="<i2"), np.frombuffer(want[44:], dtype="<i2")
            assert g.size == w.size, (i, g.size, w.size)              # same chunk bytes, same tail length
            assert (np.abs(g.astype(np.int32) - w.astype(np.int32)).max() if g.size else 0) <= 1, i
        pool = health["pool"]
        assert pool["max_stream_group"] >= 2 and pool["completed"] == 8 and pool["stream_decode_calls"] < pool["stream_chunks"], pool
    finally:
        chat.InferCodeParams = orig

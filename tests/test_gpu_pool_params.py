"""Per-request sampling parameters on the GPU: the sampling kernel's per-slot table (ctts_gen_state.row_sampling), a per-request slot
pool against the reference's own sweep and against isolated generation, and the batched speech endpoint.  `pytest -m gpu`."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, rng  # noqa: E402
from chattts_amd import engine as E  # noqa: E402
from chattts_amd.serving import SlotPool, request_params, sampling_row  # noqa: E402
from oracle import cases, sampling_np  # noqa: E402

DEV = torch.device("cuda:0")
f32 = np.float32


def _sample(logits, hist, q, *, row_base, temps=None, cfg=None, table=None):
    """one ctts_k_sample launch over B = len(row_base) utterances: logits / q [4B, 626], hist [4B, h] (every row the same length);
    either call-wide parameters (`temps`, `cfg`) or `table` (a list of ctts_sampling_row, one per utterance).  Returns ids, finish,
    end_idx, len, margin."""
    lib = _lib.lib()
    rows, V = logits.shape
    B, h, T = rows // 4, hist.shape[1], 1
    tcap = T + h + 2
    ids = np.zeros((B, tcap, 4), np.int64)
    if h:
        ids[:, T: T + h, :] = hist.reshape(B, 4, h).transpose(0, 2, 1)
    keep = []
    d = lambda a: (keep.append(torch.as_tensor(np.array(a)).to(DEV)), keep[-1])[1]
    s = _lib.GenState()
    s.B, s.T, s.max_new = B, T, h + 2
    ids_d, len_d = d(ids), d(np.full(B, T + h, np.int32))
    fin_d, end_d, mg_d = d(np.zeros(B, np.uint8)), d(np.zeros(B, np.int32)), d(np.full(B, np.inf, f32))
    s.ids_buf, s.len, s.finish, s.end_idx, s.margin = ids_d.data_ptr(), len_d.data_ptr(), fin_d.data_ptr(), end_d.data_ptr(), mg_d.data_ptr()
    s.q, s.nq = d(q.reshape(1, rows, V).astype(f32)).data_ptr(), 1
    s.eos, s.row_base = 625, d(np.asarray(row_base, np.int32)).data_ptr()
    if table is None:
        s.temperature = d(np.asarray(temps, f32)).data_ptr()
        pt = rng.penalty_table(cfg["rep"])
        s.pow_table = None if pt is None else d(pt.numpy()).data_ptr()
        s.top_p_thr = float(f32(1.0 - cfg["top_P"])) if cfg["top_P"] is not None else 0.0
        s.use_top_p, s.top_k, s.use_top_k = int(cfg["top_P"] is not None), int(cfg["top_K"] or 0), int(cfg["top_K"] is not None)
        s.min_new = cfg["min_new"]
    else:
        s.row_sampling = d(np.frombuffer(b"".join(bytes(r) for r in table), np.uint8)).data_ptr()
    _lib.check(lib.ctts_k_sample(C.byref(s), d(logits.reshape(B, 4 * V).astype(f32)).data_ptr(), None), "ctts_k_sample")
    torch.cuda.synchronize()
    return (ids_d.cpu().numpy()[:, T + h, :], fin_d.cpu().numpy(), end_d.cpu().numpy(), len_d.cpu().numpy(), mg_d.cpu().numpy())


def test_sample_table_equals_call_wide_launches_and_the_oracle():
    """8 utterances, 8 different table rows, ONE launch == 8 launches with the call-wide fields (ids, len, finish, end_idx, margin bit
    for bit) == oracle/sampling_np.py.  Global rows 600..631: the last utterances straddle row 625 (no penalty there, processors.py:24-27)."""
    rs = np.random.RandomState(31)
    B, V, h = 8, 626, 12
    cfgs = [dict(temps=[0.3, 0.3, 0.3, 0.3], top_P=0.7, top_K=20, rep=1.05, min_new=0),
            dict(temps=[0.05, 1.5, 0.7, 1.0], top_P=None, top_K=None, rep=1.0, min_new=0),
            dict(temps=[1.0, 1.0, 0.7, 0.7], top_P=0.9, top_K=None, rep=2.0, min_new=h + 1),
            dict(temps=[0.7, 0.3, 1.5, 0.05], top_P=None, top_K=1, rep=0.9, min_new=0),
            dict(temps=[1.5, 1.5, 1.5, 1.5], top_P=0.99, top_K=700, rep=1.2, min_new=h + 1),
            dict(temps=[0.3, 0.7, 1.0, 1.5], top_P=0.1, top_K=3, rep=1.05, min_new=0),
            dict(temps=[1.0, 0.3, 0.3, 1.0], top_P=0.5, top_K=100, rep=2.0, min_new=h + 1),
            dict(temps=[0.7, 0.7, 0.7, 0.7], top_P=None, top_K=5, rep=1.2, min_new=0)]
    logits = (rs.randn(4 * B, V) * 3).astype(f32)
    for b in (0, 2, 3):                                       # EOS dominates these rows: finish / end_idx, and min_new masks it for b = 2
        logits[4 * b: 4 * b + 4, 625] = 40.0
    hist = rs.randint(0, 40, size=(4 * B, h)).astype(np.int64)   # repeats: the penalty counts go above 1
    q = rng.ExpDraws(4 * B, V, 77).step(0).numpy()
    base = [600 + 4 * b for b in range(B)]
    table = [sampling_row(request_params(dict(temperature=c["temps"], top_P=c["top_P"], top_K=c["top_K"], repetition_penalty=c["rep"],
                                              min_new_token=c["min_new"]))) for c in cfgs]
    got = _sample(logits, hist, q, row_base=base, table=table)
    for b, c in enumerate(cfgs):
        sl = slice(4 * b, 4 * b + 4)
        one = _sample(logits[sl], hist[sl], q[sl], row_base=[base[b]], temps=c["temps"], cfg=c)
        for name, g, w in zip(("ids", "finish", "end_idx", "len", "margin"), got, one):
            assert np.array_equal(g[b: b + 1].view(np.uint8), w.view(np.uint8)), (b, name, g[b], w)
        pt = rng.penalty_table(c["rep"])
        want = sampling_np.sample_step(logits[sl], hist[sl], q[sl], temperature=np.asarray(c["temps"], f32),
                                       top_p=c["top_P"], top_k=c["top_K"], pow_table=None if pt is None else pt.numpy(), max_input_ids=625,
                                       mask_eos=h < c["min_new"], row_offset=base[b])
        assert np.array_equal(got[0][b], want), (b, got[0][b], want)
    assert got[1][0] == 1 and got[1][3] == 1 and got[1][2] == 0 and not got[1].all()   # EOS drawn, and masked by min_new for b = 2


def _engine(weights, dtype):
    return E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype, exact_fallback=False, certify=False)


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_pool_replays_the_reference_sweep(weights, golden, dtype):
    """Every seeded configuration of cases.sweep_cases() (the reference's own runs, tests/golden/generate_sweep.npz: per-codebook
    temperatures 0.05-1.5, top-K None..700, top-P None..0.99, penalties 0.9-2.0, min_new > max_new, batch widths 1-33): all their
    utterances as individual requests, interleaved, through ONE per-request pool of 8 slots, each with its configuration's parameters and
    (row_offset = 4 b, total_rows = 4 B).  Every request's ids == the golden row.  Excluded: none -- every seeded configuration of the
    sweep yielded (no whole-batch step-0 EOS, after which the reference yields nothing for the whole batch); the test checks that."""
    Gd = golden["generate_sweep"]
    eng = _engine(weights, dtype)
    pool = SlotPool(eng, slots=8, cap=128, hid_cap=64, per_request=True)
    per_case = {}
    for name, c in cases.sweep_cases().items():
        if c["manual_seed"] is None:
            continue           # unseeded: the host pool refuses them (one constant draw per request needs a seed)
        assert bool(Gd[name + ".yielded"][0]), name
        ids, mask, tmask = cases.gen_inputs(c)
        p = dict(temperature=c["temperature"], top_P=c["top_P"], top_K=c["top_K"], repetition_penalty=c["rep"], min_new_token=c["min_new"],
                 manual_seed=c["manual_seed"])
        per_case[name] = [(b, torch.from_numpy(ids[b][mask[b]]), torch.from_numpy(tmask[b][mask[b]]), p, c) for b in range(c["B"])]
    order = []
    while any(per_case.values()):            # interleaved: one utterance of every configuration in turn
        for name in list(per_case):
            if per_case[name]:
                order.append((name, per_case[name].pop(0)))
    for name, (b, ids, tm, p, c) in order:
        pool.submit((name, b), ids, tm, max_new_token=c["max_new"], params=p, row_offset=4 * b, total_rows=4 * c["B"])
    got = {rid: ids.cpu().numpy() for rid, ids, _ in pool.run()}
    pool.close()
    assert len(got) == len(order) == 256
    bad = []
    for name, c in cases.sweep_cases().items():
        if c["manual_seed"] is None:
            continue
        lens = Gd[name + ".lens"].astype(np.int64)
        want = np.split(Gd[name + ".ids"].astype(np.int64), np.cumsum(lens)[:-1])
        for b in range(c["B"]):
            if not np.array_equal(got[(name, b)], want[b]):
                bad.append((name, b, got[(name, b)].shape, want[b].shape))
    assert not bad, bad


def _alone(eng, ids, p, max_new, *, rng_mode, row_offset, total_rows, rng_seed=None, rng_nonce=None):
    rp = request_params(p)
    w, pr = E.gen_logits(625, p["top_P"], p["top_K"], p["repetition_penalty"])
    ids_t = ids[None]
    emb = eng.embed_prompt(ids_t, torch.ones((1, ids.shape[0]), dtype=torch.bool))
    outs = list(eng.generate(emb, ids_t, torch.tensor(rp.temperature), 625, None, max_new, rp.min_new_token, (*pr, *w), return_hidden=True,
                             manual_seed=rp.manual_seed, rng=rng_mode, rng_seed=rng_seed, rng_nonce=rng_nonce, row_offset=row_offset,
                             total_rows=total_rows))
    return outs[-1] if outs else None


@pytest.mark.parametrize("rng_mode", ["host", "device"])
def test_pooled_request_equals_generating_it_alone(weights, rng_mode):
    """12 requests with distinct parameters and seeds through 4 slots: each request's ids == `GptEngine.generate` of that request alone
    at batch 1 with the same parameters / row_offset / total_rows, hiddens within 1e-5 (the existing pool test's bar).  The
    device-generator pool mixes seeded and unseeded requests; an unseeded one is compared with generate(rng_nonce=pool.nonce_of[rid])."""
    eng = _engine(weights, "f32")
    pool = SlotPool(eng, slots=4, cap=160, hid_cap=64, rng=rng_mode, rng_seed=1234, per_request=True)
    rs = np.random.RandomState(9)
    reqs = {}
    for i in range(12):
        T = int(rs.randint(4, 30))
        ids = torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(T, 1)), 4, axis=1).astype(np.int64))
        seeded = rng_mode == "host" or i % 3 != 0
        p = dict(temperature=[float(x) for x in rs.choice([0.1, 0.3, 0.7, 1.2], 4)], top_P=[None, 0.5, 0.7, 0.95][i % 4],
                 top_K=[None, 3, 20, 100, 700][i % 5], repetition_penalty=[1.0, 1.05, 1.3, 0.9][i % 4],
                 min_new_token=int(rs.randint(1, 20)), manual_seed=int(1000 + 17 * i) if seeded else None)
        max_new = int(rs.randint(8, 48))
        ro, tr = [(0, 4), (8, 16), (624, 640), (4, 40)][i % 4]     # (624, 640): rows 624 | 625.. straddle the penalty quirk
        reqs[i] = (ids, p, max_new, ro, tr)
        pool.submit(i, ids, max_new_token=max_new, params=p, row_offset=ro, total_rows=tr)
    got = {rid: (ids.cpu().numpy(), hid.cpu().numpy()) for rid, ids, hid in pool.run()}
    assert sorted(got) == list(range(12)) and not pool.active and len(pool.free) == 4
    for i, (ids, p, max_new, ro, tr) in reqs.items():
        unseeded = p["manual_seed"] is None
        ref = _alone(eng, ids, p, max_new, rng_mode=rng_mode, row_offset=ro, total_rows=tr, rng_seed=1234 if unseeded else None,
                     rng_nonce=pool.nonce_of[i] if unseeded else None)
        assert ref is not None
        assert np.array_equal(got[i][0], ref.ids[0].cpu().numpy()), (i, got[i][0].shape, ref.ids[0].shape)
        assert np.abs(got[i][1] - ref.hiddens[0].cpu().numpy()).max() < 1e-5, i
    pool.close()


def test_batched_endpoint_matches_the_serial_endpoint(weights):
    """create_app(chat, voices, batch_slots=8) on a loaded synthetic Chat: 6 concurrent non-streamed requests over 3 voices from threads,
    plus one streamed request at the same time.  Every body == what an app without batching returns for the same requests sent one
    after another: token ids identical, PCM16 within 1 LSB (the pooled hidden states come from a differently shaped batch); the streamed
    body byte-identical; the batcher saw at least 2 co-resident requests."""
    import io
    import wave
    from starlette.testclient import TestClient
    from chattts_amd import server
    from chattts_amd.core import Chat
    from chattts_amd.serving import SpeechBatcher
    gold_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(gold_dir, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32", tokenizer=os.path.join(gold_dir, "tokenizer"), spk_stat=spk_stat)
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker(), "alloy": chat.sample_random_speaker(), "echo": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    # (random weights do not emit [Ebreak] on cue: cap the length the endpoint's fixed max_new_token = 2048 would otherwise run to)
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 96})
    texts = ["What is [uv_break]your favorite english food?", "Hello there.", "The quick brown fox jumps over the lazy dog.",
             "Good morning!", "How are you today?", "Numbers like 42 and 7."]
    vs = ["default", "alloy", "echo", "alloy", "echo", "default"]
    stream_text = "A streamed sentence."

    class Recording(SpeechBatcher):
        def _take(self, item):
            self.texts[item.rid] = (item.text, item.params.spk_emb)
            super()._take(item)

    def pcm_of(r):
        with wave.open(io.BytesIO(r.content), "rb") as wf:
            return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")

    try:
        serial = server.create_app(chat, voices)
        with TestClient(serial) as c:
            want = [pcm_of(c.post("/v1/audio/speech", json={"input": t, "voice": v, "response_format": "wav"})) for t, v in zip(texts, vs)]
            want_stream = c.post("/v1/audio/speech", json={"input": stream_text, "response_format": "wav", "stream": True}).content
        want_ids = {}
        for t, v in zip(texts, vs):
            p = chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                     min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=voices[v])
            out = next(chat._infer_code([chat.normalizer(t, True, True, None)], False, DEV, True, p))
            want_ids[(t, voices[v])] = out.ids[0].cpu().numpy()

        lock = threading.Lock()
        b = Recording(chat, 8, lock)
        b.texts, got_ids = {}, {}
        orig_run = b.pool.run

        def run(between=None):
            for rid, ids, hid in orig_run(between):
                got_ids[b.texts[rid]] = ids.cpu().numpy()
                yield rid, ids, hid
        b.pool.run = run
        app = server.create_app(chat, voices, batcher=b)
        res, res_stream = [None] * len(texts), [None]
        with TestClient(app) as c:
            def one(i):
                res[i] = c.post("/v1/audio/speech", json={"input": texts[i], "voice": vs[i], "response_format": "wav"})

            def streamed():
                res_stream[0] = c.post("/v1/audio/speech", json={"input": stream_text, "response_format": "wav", "stream": True})
            ths = [threading.Thread(target=one, args=(i,)) for i in range(len(texts))] + [threading.Thread(target=streamed)]
            for th in ths:
                th.start()
            for th in ths:
                th.join(timeout=600)
            health = c.get("/health").json()
        b.close()
        assert all(r is not None and r.status_code == 200 for r in res), [None if r is None else r.status_code for r in res]
        assert res_stream[0].status_code == 200 and res_stream[0].content == want_stream
        exact = True
        for i, (t, v) in enumerate(zip(texts, vs)):
            assert np.array_equal(got_ids[(t, voices[v])], want_ids[(t, voices[v])]), i
            g = pcm_of(res[i])
            assert g.shape == want[i].shape, (i, g.shape, want[i].shape)
            d = np.abs(g.astype(np.int32) - want[i].astype(np.int32)).max() if g.size else 0
            assert d <= 1, (i, d)
            exact = exact and d == 0
        print(f"pooled PCM16 {'bit-identical to' if exact else 'within 1 LSB of'} the serial endpoint")
        assert health["pool"]["max_coresident"] >= 2 and health["pool"]["completed"] == len(texts), health
    finally:
        chat.InferCodeParams = orig

"""The refine-text stage behind continuous batching, on the GPU: `sample_text_k` with the per-slot sampling table and the device
generator, a text-mode slot pool against the reference's own refine-text runs and against isolated generation, the two-stage
SpeechBatcher and the endpoint's `refine_text`.  `pytest -m gpu`."""
import ctypes as C
import io
import logging
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, rng  # noqa: E402
from chattts_amd import engine as E  # noqa: E402
from chattts_amd.serving import SlotPool, SpeechBatcher, request_params, sampling_row  # noqa: E402
from oracle import cases, sampling_np  # noqa: E402

DEV = torch.device("cuda:0")
f32 = np.float32
V = 21178


# ---- sample_text_k alone ----------------------------------------------------------------------------------------------------------
def _sample_text(logits, q, *, eos, gen=0, cfg=None, table=None, row_base=None, device=False, seed=None, per_step=0):
    """one ctts_k_sample_text launch over B = len(logits) utterances at generation step `gen`: call-wide parameters (`cfg`) or `table`
    (one ctts_sampling_row per utterance); `q` [B, V] host draws, or device=True (no q: the kernel's own generator, call-wide `seed` /
    `per_step` unless the table brings them).  Returns ids [B], finish, end_idx, len, margin."""
    lib = _lib.lib()
    B, T = logits.shape[0], 1
    tcap = T + gen + 2
    keep = []
    d = lambda a: (keep.append(torch.as_tensor(np.array(a)).to(DEV)), keep[-1])[1]
    s = _lib.GenState()
    s.B, s.T, s.max_new = B, T, gen + 2
    ids_d, len_d = d(np.zeros((B, tcap, 4), np.int64)), d(np.full(B, T + gen, np.int32))
    fin_d, end_d, mg_d = d(np.zeros(B, np.uint8)), d(np.full(B, gen, np.int32)), d(np.full(B, np.inf, f32))
    s.ids_buf, s.len, s.finish, s.end_idx, s.margin = ids_d.data_ptr(), len_d.data_ptr(), fin_d.data_ptr(), end_d.data_ptr(), mg_d.data_ptr()
    s.eos, s.infer_text = int(eos), 1
    if row_base is not None:
        s.row_base = d(np.asarray(row_base, np.int32)).data_ptr()
    if device:
        s.rng_device, s.rng_per_step = 1, int(per_step)
        if seed is not None:
            s.rng_seed = d(np.array([seed], np.int64)).data_ptr()
    else:
        s.q, s.nq = d(q.reshape(1, B, V).astype(f32)).data_ptr(), 1
    if table is None:
        s.temperature = d(np.asarray([cfg["temp"]], f32)).data_ptr()
        s.top_p_thr = float(f32(1.0 - cfg["top_P"])) if cfg["top_P"] is not None else 0.0
        s.use_top_p, s.top_k, s.use_top_k = int(cfg["top_P"] is not None), int(cfg["top_K"] or 0), int(cfg["top_K"] is not None)
        s.min_new = cfg["min_new"]
    else:
        s.row_sampling = d(np.frombuffer(b"".join(bytes(r) for r in table), np.uint8)).data_ptr()
    _lib.check(lib.ctts_k_sample_text(C.byref(s), d(logits.astype(f32)).data_ptr(), V, None), "ctts_k_sample_text")
    torch.cuda.synchronize()
    got = ids_d.cpu().numpy()[:, T + gen, :]
    assert (got == got[:, :1]).all()                             # gpt.py:522-525: replicated over the 4 slots
    return np.ascontiguousarray(got[:, 0]), fin_d.cpu().numpy(), end_d.cpu().numpy(), len_d.cpu().numpy(), mg_d.cpu().numpy()


CFGS = [dict(temp=0.1, top_P=0.7, top_K=20, min_new=0),          # fast path (top-K <= 64)
        dict(temp=0.7, top_P=0.5, top_K=None, min_new=0),        # serial path: no top-K
        dict(temp=1.0, top_P=None, top_K=500, min_new=0),        # serial path: top-K > 64
        dict(temp=1.3, top_P=None, top_K=1, min_new=5)]          # min_new above the step: the drawn EOS is masked


def _rows():
    """4 logits rows from a fixed RandomState; exact ties at the top-K cut of the two rows filtered by top-K alone (the tie order inside
    a top-p cut is unspecified in the reference); the EOS is row 3's likeliest token"""
    rs = np.random.RandomState(2027)
    logits = (rs.standard_normal((4, V)) * 3).astype(f32)
    o2 = np.argsort(-logits[2], kind="stable")
    logits[2, o2[498:503]] = logits[2, o2[499]]                 # ranks 499..503 hold the 500th value
    o3 = np.argsort(-logits[3], kind="stable")
    logits[3, o3[2:5]] = logits[3, o3[2]]                       # top-K 1 keeps 3 (min_tokens_to_keep): ranks 3..5 tie
    return logits, int(o3[0])


def _table(cfgs, seeds=None, per_step=None):
    return [sampling_row(request_params(dict(temperature=c["temp"], top_P=c["top_P"], top_K=c["top_K"], min_new_token=c["min_new"]),
                                        infer_text=True), 0 if seeds is None else seeds[b], False if per_step is None else per_step[b])
            for b, c in enumerate(cfgs)]


def _oracle(logits, q, c, eos, gen):
    return sampling_np.sample_step(logits[None], np.zeros((1, 0), np.int64), q[None], temperature=np.full(1, c["temp"], f32), top_p=c["top_P"],
                                   top_k=c["top_K"], pow_table=None, max_input_ids=V - 1, mask_eos=gen < c["min_new"], eos=eos)[0]


def test_text_table_equals_call_wide_launches_and_the_oracle():
    """ONE sample_text_k launch over 4 rows whose table entries differ (fast path, both serial paths, a masked EOS; temperatures 0.1 /
    0.7 / 1.0 / 1.3) == 4 call-wide launches of one row each (ids, finish, end_idx, len and the certificate margin bit for bit) ==
    oracle/sampling_np.py on the same logits and draws."""
    logits, eos = _rows()
    q = rng.ExpDraws(4, V, 77).step(0).numpy()
    got = _sample_text(logits, q, eos=eos, table=_table(CFGS))
    for b, c in enumerate(CFGS):
        one = _sample_text(logits[b: b + 1], q[b: b + 1], eos=eos, cfg=c)
        for name, g, w in zip(("ids", "finish", "end_idx", "len", "margin"), got, one):
            assert np.array_equal(g[b: b + 1].view(np.uint8), w.view(np.uint8)), (b, name, g[b], w)
        want = _oracle(logits[b], q[b], c, eos, 0)
        assert got[0][b] == want, (b, got[0][b], want)
    assert got[0][3] != eos and got[1][3] == 0                   # row 3's likeliest token is the EOS, and min_new masks it


def _device_draws(seed, step, row, Vn=V):
    out = torch.empty((1, Vn), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().ctts_k_exp_draws(seed, step, row, 1, Vn, out.data_ptr(), None), "exp_draws")
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


def test_text_device_generator_draws_what_the_hook_materialises():
    """rng_device = 1 with the table, seeded and per-step rows mixed, at steps 0 and 1: the tokens == a host-generator launch fed the
    tensor `exp_draws_k` materialises for (seed, global row, step word, V = n_text) == the oracle on that tensor.  A per-step row's
    step word advances with the step, a seeded row's stays 0; a call-wide device launch of one row gives the same token."""
    logits, eos = _rows()
    seeds, per_step, base = [11, 2 ** 40 + 5, 99, 12345], [False, True, False, True], [0, 7, 16, 300]
    tab = _table(CFGS, seeds, per_step)
    for gen in (0, 1):
        q = np.stack([_device_draws(seeds[b], gen if per_step[b] else 0, base[b]) for b in range(4)])
        got = _sample_text(logits, None, eos=eos, gen=gen, table=tab, row_base=base, device=True)
        host = _sample_text(logits, q, eos=eos, gen=gen, table=_table(CFGS), row_base=base)
        for name, g, w in zip(("ids", "finish", "end_idx", "len", "margin"), got, host):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (gen, name, g, w)
        for b, c in enumerate(CFGS):
            assert got[0][b] == _oracle(logits[b], q[b], c, eos, gen), (gen, b)
            one = _sample_text(logits[b: b + 1], None, eos=eos, gen=gen, cfg=c, row_base=base[b: b + 1], device=True, seed=seeds[b],
                               per_step=per_step[b])
            assert one[0][0] == got[0][b], (gen, b)
    for b in range(4):     # stepping a row twice: per_step advances the counter, a seeded row draws the same tensor again
        same = np.array_equal(_device_draws(seeds[b], 1 if per_step[b] else 0, base[b]), _device_draws(seeds[b], 0, base[b]))
        assert same == (not per_step[b]), b


# ---- the text-mode pool -----------------------------------------------------------------------------------------------------------
def _engine(weights, dtype):
    return E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype, exact_fallback=False, certify=False)


SEEDED_TEXT_SWEEP = ["t05", "t06", "t07", "t09", "t10"]


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_text_pool_replays_the_reference_refine_runs(weights, golden, dtype):
    """Every seeded refine-text configuration the reference itself ran (cases.text_sweep_cases() t05, t06, t07, t09, t10 of
    tests/golden/generate_sweep.npz; text3 and text1_greedyish of tests/golden/text.npz: 53 utterances, batch widths 1-17, max_new 1-24,
    min_new > max_new among them): all utterances as individual requests, interleaved, through ONE text pool of 4 slots, each with its
    configuration's parameters and (row_offset = b, total_rows = B).  Every request's ids == the golden row.  Excluded: none."""
    eng = _engine(weights, dtype)
    pool = SlotPool(eng, slots=4, cap=64, per_request=True, infer_text=True, eos_token=cases.TEXT_EOS)
    sweep = {n: c for n, c in cases.text_sweep_cases().items() if c["manual_seed"] is not None}
    assert sorted(sweep) == SEEDED_TEXT_SWEEP
    for name in sweep:
        assert bool(golden["generate_sweep"][name + ".yielded"][0]), name
    where = {**{n: "generate_sweep" for n in sweep}, **{n: "text" for n in cases.TEXT_CASES}}
    allc = {**sweep, **cases.TEXT_CASES}
    per_case = {}
    for name, c in allc.items():
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
        pool.submit((name, b), ids, tm, max_new_token=c["max_new"], params=p, row_offset=b, total_rows=c["B"])
    got = {rid: ids.cpu().numpy() for rid, ids, _ in pool.run()}
    pool.close()
    assert len(got) == len(order) == 53
    bad = []
    for name, c in allc.items():
        Gd = golden[where[name]]
        lens = Gd[name + ".lens"].astype(np.int64)
        assert (lens == lens.max()).all() and lens.max() == c["max_new"], name       # full-length rows
        want = np.split(Gd[name + ".ids"].astype(np.int64), np.cumsum(lens)[:-1])
        for b in range(c["B"]):
            if got[(name, b)].ndim != 1 or not np.array_equal(got[(name, b)], want[b]):
                bad.append((name, b, got[(name, b)].shape, want[b].shape))
    assert not bad, bad


def _alone(eng, ids, p, max_new, *, device, row_offset, total_rows, rng_seed=None, rng_nonce=None):
    w, pr = E.gen_logits(V, p["top_P"], p["top_K"], 1.0)
    ids_t = ids[None]
    emb = eng.embed_prompt(ids_t, torch.ones((1, ids.shape[0]), dtype=torch.bool))
    outs = list(eng.generate(emb, ids_t, torch.tensor([p["temperature"]]), cases.TEXT_EOS, None, max_new, p["min_new_token"], (*pr, *w),
                             infer_text=True, manual_seed=p["manual_seed"], row_offset=row_offset, total_rows=total_rows,
                             text_rng="device" if device else None, rng_seed=rng_seed, rng_nonce=rng_nonce))
    return outs[-1] if outs else None


@pytest.mark.parametrize("rng_mode", ["host", "device"])
def test_pooled_text_request_equals_generating_it_alone(weights, rng_mode):
    """12 text requests with distinct parameters and seeds through 4 slots (prompts of 4-30 tokens, max_new 8-48): each request's ids ==
    `GptEngine.generate(infer_text=True)` of that request alone with the same parameters / row_offset / total_rows.  The device pool
    mixes seeded and unseeded requests; an unseeded one is compared with generate(text_rng="device", rng_nonce=pool.nonce_of[rid])."""
    eng = _engine(weights, "f32")
    pool = SlotPool(eng, slots=4, cap=128, rng=rng_mode, rng_seed=4321, per_request=True, infer_text=True, eos_token=cases.TEXT_EOS)
    rs = np.random.RandomState(19)
    reqs = {}
    for i in range(12):
        T = int(rs.randint(4, 31))
        ids = torch.from_numpy(np.repeat(rs.randint(1, V, size=(T, 1)), 4, axis=1).astype(np.int64))
        seeded = rng_mode == "host" or i % 3 != 0
        p = dict(temperature=float(rs.choice([0.1, 0.3, 0.7, 1.2])), top_P=[None, 0.5, 0.7, 0.95][i % 4], top_K=[None, 3, 20, 100, 700][i % 5],
                 min_new_token=int(rs.randint(1, 20)), manual_seed=int(2000 + 13 * i) if seeded else None)
        max_new = int(rs.randint(8, 49))
        ro, tr = [(0, 1), (2, 4), (5, 17), (1, 10)][i % 4]
        reqs[i] = (ids, p, max_new, ro, tr)
        pool.submit(i, ids, max_new_token=max_new, params=p, row_offset=ro, total_rows=tr)
    got = {rid: ids.cpu().numpy() for rid, ids, _ in pool.run()}
    assert sorted(got) == list(range(12)) and not pool.active and len(pool.free) == 4
    for i, (ids, p, max_new, ro, tr) in reqs.items():
        unseeded = p["manual_seed"] is None
        ref = _alone(eng, ids, p, max_new, device=rng_mode == "device", row_offset=ro, total_rows=tr, rng_seed=4321 if unseeded else None,
                     rng_nonce=pool.nonce_of[i] if unseeded else None)
        assert ref is not None
        assert got[i].ndim == 1 and np.array_equal(got[i], ref.ids[0].cpu().numpy()), (i, got[i].shape, ref.ids[0].shape)
    pool.close()


# ---- two stages in one worker, and the endpoint -----------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def chat(weights):
    from chattts_amd.core import Chat
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts=weights, device=DEV, dtype="f32", tokenizer=os.path.join(GOLD, "tokenizer"), spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voices = {"default": c.sample_random_speaker(), "alloy": c.sample_random_speaker()}
    return c


def _close(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) if got.size else 0
    assert d <= 1, (what, d)


class _Recording(SpeechBatcher):
    def _refined(self, rid, row):
        self.rows[rid] = row.cpu().numpy()
        super()._refined(rid, row)

    def _handle(self, got):
        if isinstance(got, tuple):
            self.code_ids[got[0]] = got[1].cpu().numpy()
        super()._handle(got)


def test_two_stage_batcher_equals_the_serial_two_stage_call(chat):
    """6 concurrent submit(text, params, refine=...) with distinct seeds and parameters + 2 submit_stream through
    SpeechBatcher(slots=4, refine=True, streams=True): each result against `Chat.infer` of that request alone with
    skip_refine_text=False -- refined token rows identical, code ids identical, PCM16 within 1 LSB (the pooled endpoint's bar), the
    streams with the serial chunking and length.  At least 2 requests were co-resident in the text pool, and at some iteration both
    pools had live slots."""
    texts = ["What is your favorite english food?", "Hello there.", "The quick brown fox jumps over the lazy dog.", "Good morning!",
             "How are you today?", "Numbers like 42 and 7.", "A streamed sentence.", "Another streamed sentence, a little longer."]
    vs = list(chat.test_voices.values())
    ps, rf = [], []
    for i in range(8):
        ps.append(chat.InferCodeParams(top_P=[0.5, 0.7][i % 2], top_K=[10, 20, 5][i % 3], temperature=[0.1, 0.3][i % 2], repetition_penalty=1.1,
                                       max_new_token=[40, 56, 72][i % 3] if i < 6 else 96, show_tqdm=False, manual_seed=100 + i, spk_emb=vs[i % 2]))
        rf.append(chat.RefineTextParams(top_P=[0.7, 0.9][i % 2], top_K=[20, 5, 100][i % 3], temperature=[0.7, 0.3, 1.0][i % 3],
                                        max_new_token=[12, 20, 9][i % 3], min_new_token=i % 4, show_tqdm=False, manual_seed=500 + 7 * i,
                                        prompt=["", "[oral_2][laugh_0][break_6]"][i % 2]))
    want = []
    for i, t in enumerate(texts):
        norm = chat.normalizer(t, True, True, None)
        refined = chat._refine_text([norm], DEV, rf[i])
        row = refined.ids[0].cpu().numpy()
        code = next(chat._infer_code(chat.refined_text(refined.ids), False, DEV, True, ps[i])).ids[0].cpu().numpy()
        if i < 6:
            pcm = chat.infer([t], skip_refine_text=False, params_refine_text=rf[i], params_infer_code=ps[i], pcm16=True)[0]
        else:
            pcm = [np.asarray(c).reshape(-1) for c in chat.infer([t], stream=True, skip_refine_text=False, params_refine_text=rf[i],
                                                                 params_infer_code=ps[i], pcm16=True)]
        want.append((row, code, pcm))
    b = _Recording(chat, 4, threading.Lock(), refine=True, streams=True)
    b.rows, b.code_ids = {}, {}
    try:
        futs = [b.submit(texts[i], ps[i], refine=rf[i]) for i in range(6)]
        streams = [b.submit_stream(texts[i], ps[i], refine=rf[i]) for i in (6, 7)]
        got_streams = [None, None]

        def drain(k):
            got_streams[k] = [np.asarray(c) for c in streams[k]]
        ths = [threading.Thread(target=drain, args=(k,)) for k in range(2)]
        for th in ths:
            th.start()
        got = [f.result(timeout=300) for f in futs]
        for th in ths:
            th.join(timeout=300)
        occ = b.occupancy()
    finally:
        b.close()
    rid_of = {i: i for i in range(8)}        # request ids are handed out in submission order
    for i in range(8):
        assert np.array_equal(b.rows[rid_of[i]], want[i][0]), i
        assert np.array_equal(b.code_ids[rid_of[i]], want[i][1]), i
    for i in range(6):
        _close(got[i], want[i][2], i)
    for k in range(2):
        assert got_streams[k] is not None and len(got_streams[k]) == len(want[6 + k][2]), k
        for j, (g, w) in enumerate(zip(got_streams[k], want[6 + k][2])):
            _close(g, w, (k, j))
    r = occ["refine"]
    assert r["admissions"] == 8 and r["handed"] == 8 and r["max_coresident"] >= 2 and r["steps"] > 0 and r["both_live_polls"] >= 1, occ
    assert occ["completed"] == 8 and occ["failed"] == 0, occ


def test_endpoint_refine_text(chat):
    """create_app(..., batch_slots=4, batch_refine=True): a `"refine_text": true` body == the serial two-stage `Chat.infer` (PCM16 within
    1 LSB); a body without the key == the batched response of an app without the option, byte for byte; an app without `batch_refine`
    ignores the key with the "unsupported parameters" warning."""
    from starlette.testclient import TestClient
    from chattts_amd import server
    voices = chat.test_voices
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 64})     # (random weights do not emit [Ebreak] on cue)
    refine = chat.RefineTextParams(show_tqdm=False, manual_seed=42, max_new_token=16)
    text = "Hello there, how are you?"

    def pcm_of(r):
        with wave.open(io.BytesIO(r.content), "rb") as wf:
            return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")

    class Catch(logging.Handler):
        def __init__(self):
            super().__init__()
            self.msgs = []

        def emit(self, record):
            self.msgs.append(record.getMessage())
    try:
        p = chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                 min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=voices["alloy"])
        want = chat.infer([text], skip_refine_text=False, params_refine_text=refine, params_infer_code=p, pcm16=True)[0]
        plain = server.create_app(chat, voices, batch_slots=4)
        log, catch = logging.getLogger("test_text_pool.plain"), Catch()
        log.addHandler(catch)
        plain_warn = server.create_app(chat, voices, batch_slots=4, logger=log)
        app = server.create_app(chat, voices, batch_slots=4, batch_refine=True, refine_params=refine)
        body = {"input": text, "voice": "alloy", "response_format": "wav"}
        try:
            with TestClient(plain) as c:
                r_plain = c.post("/v1/audio/speech", json=body)
            with TestClient(plain_warn) as c:
                r_ignored = c.post("/v1/audio/speech", json={**body, "refine_text": True})
            with TestClient(app) as c:
                r_refined = c.post("/v1/audio/speech", json={**body, "refine_text": True})
                r_same = c.post("/v1/audio/speech", json=body)
                health = c.get("/health").json()
        finally:
            for a in (plain, plain_warn, app):
                a.state.batcher.close()
        assert all(r.status_code == 200 for r in (r_plain, r_ignored, r_refined, r_same))
        _close(pcm_of(r_refined), want, "refined")
        assert r_same.content == r_plain.content
        assert r_ignored.content == r_plain.content and any("unsupported parameters" in m and "refine_text" in m for m in catch.msgs), catch.msgs
        assert health["pool"]["refine"]["handed"] == 1 and health["pool"]["completed"] == 2, health
    finally:
        chat.InferCodeParams = orig

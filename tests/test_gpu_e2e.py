"""End-to-end parity of the HIP path against goldens produced by the reference itself
(tests/golden/*.npz) and against the numpy oracle.  Needs a real MI355X: `pytest -m gpu`.

Bars (BASELINE.json north_star): sampled token ids bit-exact vs the reference CPU path at fixed seed
(f32 parity mode); float32 waveform within 1e-4 RMS."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E  # noqa: E402
from chattts_amd import synth  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from oracle import cases, codec_np, generate_np, llama_np  # noqa: E402

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", params=["x3", "exact"])
def gpt_f32(weights, request):
    """the parity mode, both arithmetics of its decode projections: "x3" = dtype "f32x3", split-bf16 planes, three bf16 MFMAs per product
    (csrc/decode32x.hip) -- WITHOUT the exact fallback, so that what is compared is that arithmetic itself -- and "exact" = dtype "f32",
    f32 MFMA on packed f32 operands (csrc/decode32.hip).  Every reference-generated golden must hold in BOTH: the bar is the reference's
    token ids, not either kernel's bits.  (The certificate + fallback have their own tests below.)"""
    eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32x3" if request.param == "x3" else "f32", exact_fallback=False, certify=True)
    assert (eng.x3 is not None) == (request.param == "x3")
    return eng


@pytest.fixture(scope="module")
def gpt_bf16(weights):
    return E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="bf16")


@pytest.fixture(scope="module", params=["bf16x3", "f32"])
def codec(weights, request):
    """both dense-layer implementations of the acoustic decoder must hold the 1e-4 RMS bar"""
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=request.param)


def run_case(eng, c, *, use_graph, rows=None, stream=False):
    ids, mask, tmask = cases.gen_inputs(c)
    B = ids.shape[0]
    sl = slice(0, B) if rows is None else rows
    ids_t, mask_t, tm_t = torch.from_numpy(ids[sl]), torch.from_numpy(mask[sl]), torch.from_numpy(tmask[sl])
    emb = eng.embed_prompt(ids_t, tm_t)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    if c["manual_seed"] is None:
        torch.manual_seed(c["global_seed"])
    outs = list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"],
                             (*procs, *warpers), return_hidden=True, stream=stream, manual_seed=c["manual_seed"],
                             use_graph=use_graph, row_offset=sl.start * 4, total_rows=B * 4))
    return outs, emb


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(cases.GEN_CASES))
def test_generate_token_ids_bit_exact(gpt_f32, golden, name, use_graph):
    c = cases.GEN_CASES[name]
    Gd = golden["generate"]
    outs, emb = run_case(gpt_f32, c, use_graph=use_graph)
    assert len(outs) == 1
    out = outs[0]
    assert np.array_equal(emb[0].cpu().numpy(), Gd[name + ".emb_row0"])
    lens = np.array([int(t.shape[0]) for t in out.ids])
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    want_lens, want = Gd[name + ".lens"], Gd[name + ".ids"]
    assert np.array_equal(lens, want_lens), (lens, want_lens)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {len(want)} token rows differ"
    for b in c["keep_hidden_rows"]:
        err = np.abs(out.hiddens[b].cpu().numpy() - Gd[name + f".hid{b}"]).max()
        assert err < 2e-4, (b, err)


@pytest.mark.parametrize("name", list(cases.BIG_CASES))
def test_generate_baseline_sizes_bit_exact(gpt_f32, golden, name):
    """BASELINE-size goldens produced by the reference itself (tests/golden/generate_big.npz): C3 at full width (64
    mixed-length left-padded utterances, 20 of them hitting EOS at different steps -> compaction across 64 rows, the
    64-row projection tiles) and C2 (batch 1, 512 steps, context up to 544 keys).  Token ids bit-exact, graph replay."""
    c = cases.BIG_CASES[name]
    Gd = golden["generate_big"]
    outs, emb = run_case(gpt_f32, c, use_graph=True)
    out = outs[-1]
    assert np.array_equal(emb[0].cpu().numpy(), Gd[name + ".emb_row0"])
    lens = np.array([int(t.shape[0]) for t in out.ids])
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    want_lens, want = Gd[name + ".lens"], Gd[name + ".ids"]
    assert np.array_equal(lens, want_lens), (lens, want_lens)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {len(want)} token rows differ"
    for b in c["keep_hidden_rows"]:
        err = np.abs(out.hiddens[b].cpu().numpy() - Gd[name + f".hid{b}"]).max()
        assert err < 2e-4, (b, err)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(cases.PARAM_CASES))
def test_generate_parameter_space_bit_exact(gpt_f32, golden, name, use_graph):
    """tests/golden/generate_params.npz, the reference's own runs over what `InferCodeParams` lets a caller turn: no top-k / no
    top-p warper at all, top_K = 2 (below min_tokens_to_keep = 3), a wide nucleus (0.95 / 50) at temperatures up to 1.0, repetition
    penalty 1.0 (no processor) / 1.2 / 1.3 -- and `wide160`: 160 utterances in ONE batch (2.5x a GPU's share of C4; 64 + 64 + 32-row
    projection tiles, 640 sampling rows of which rows >= 625 get no repetition penalty, processors.py:24-27).  Token ids bit-exact."""
    c = cases.PARAM_CASES[name]
    Gd = golden["generate_params"]
    outs, emb = run_case(gpt_f32, c, use_graph=use_graph)
    out = outs[-1]
    assert np.array_equal(emb[0].cpu().numpy(), Gd[name + ".emb_row0"])
    lens = np.array([int(t.shape[0]) for t in out.ids])
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    want_lens, want = Gd[name + ".lens"], Gd[name + ".ids"]
    assert np.array_equal(lens, want_lens), (lens, want_lens)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {len(want)} token rows differ"
    for b in c["keep_hidden_rows"]:
        err = np.abs(out.hiddens[b].cpu().numpy() - Gd[name + f".hid{b}"]).max()
        assert err < 2e-4, (b, err)


def test_generate_default_max_new_token_bit_exact(gpt_f32):
    """tests/golden/generate_max.npz: `InferCodeParams.max_new_token`'s default (2048, core.py:197) generated in full by the reference --
    two utterances (one left-padded), EOS masked to the last step, contexts up to 2088 keys.  All 2 x 2048 token rows bit-exact (graph
    replay): no f32 summation-order difference anywhere in 20 layers x 2048 steps of attention over a growing cache flips a draw."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_max.npz")
    Gd = np.load(path)
    c = cases.MAX_CASES["max2048"]
    outs, emb = run_case(gpt_f32, c, use_graph=True)
    out = outs[-1]
    assert np.array_equal(emb[0].cpu().numpy(), Gd["max2048.emb_row0"])
    assert [int(t.shape[0]) for t in out.ids] == Gd["max2048.lens"].tolist() == [2048, 2048]
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    want = Gd["max2048.ids"]
    assert np.array_equal(got, want), f"first differing token row: {int(np.argmax((got != want).any(1)))} of {len(want)}"


def test_random_sweep_equals_the_reference(gpt_f32, golden):
    """tests/golden/generate_sweep.npz: 40 seeded random configurations (cases.sweep_cases) run by the reference itself -- batch widths
    1..33 around the 16-row tile edges, one-token prompts, max_new_token = 1, min_new_token above max_new_token, top_K from 1 to above the
    vocabulary or absent, top_P 0.1..0.99 or absent, per-codebook temperatures 0.05..1.5, repetition penalties 0.9 / 1 / 1.05 / 1.2 / 2,
    seeded and unseeded.  Token ids bit-exact in every one, and the global generator left where the reference leaves it."""
    Gd = golden["generate_sweep"]
    bad = []
    for name, c in {**cases.sweep_cases(), **cases.text_sweep_cases()}.items():
        text = name.startswith("t")      # + 12 refine-text configurations (one row per utterance over the 21178-way head, top_K up to 30000)
        ids, mask, tmask = cases.gen_inputs(c)
        ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
        emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
        warpers, procs = E.gen_logits(21178 if text else 625, c["top_P"], c["top_K"], c["rep"])
        torch.manual_seed(c["global_seed"])
        outs = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), cases.TEXT_EOS if text else 625, mask_t, c["max_new"],
                                     c["min_new"], (*procs, *warpers), infer_text=text, return_hidden=True, manual_seed=c["manual_seed"],
                                     use_graph=(int(name[1:]) % 2 == 0)))
        after = torch.rand(2).numpy()
        ok = np.array_equal(after, Gd[name + ".rand_after"]) and (len(outs) == 1) == bool(Gd[name + ".yielded"][0])
        if ok and outs:
            lens = np.array([int(t.shape[0]) for t in outs[0].ids])
            got = np.concatenate([t.cpu().numpy() for t in outs[0].ids], 0)
            ok = np.array_equal(lens, Gd[name + ".lens"].astype(np.int64)) and np.array_equal(got, Gd[name + ".ids"].astype(np.int64))
        if not ok:
            bad.append((name, {k: c[k] for k in ("B", "t_min", "t_max", "top_P", "top_K", "rep", "max_new", "min_new", "manual_seed")}))
    assert not bad, bad


def test_wide_batch_tail_shard_keeps_the_global_row_quirk(gpt_f32, golden):
    """SURVEY 8e caveats 1-2 against the reference itself: utterances [128, 160) of `wide160` generated ALONE, as the last rank of a
    five-way split would (row_offset = 512 of total_rows = 640), equal the same utterances of the reference's unsharded run --
    including utterances 156..158, whose sampling rows >= 625 the reference does not penalise (that the golden discriminates the quirk --
    penalising those rows changes utterances 156, 157 and 158 -- is shown on the oracle, tests/test_oracle_vs_golden.py)."""
    c = cases.PARAM_CASES["wide160"]
    Gd = golden["generate_params"]
    lens, rows = _golden_rows(Gd, "wide160", c["B"])
    outs, _ = run_case(gpt_f32, c, use_graph=True, rows=slice(128, 160))
    for i, b in enumerate(range(128, 160)):
        assert np.array_equal(outs[-1].ids[i].cpu().numpy(), rows[b]), b


def test_scattered_shard_with_row_ids_equals_the_unsharded_reference(gpt_f32, golden):
    """round 6 (length-balanced shards): a NON-contiguous, permuted set of utterances of `wide160` generated alone with
    `row_ids` = their global indices (ctts_gen_state.row_base; the Exp(1) rows of the full-batch draw selected on the host) equals the
    same utterances of the reference's unsharded run -- on both sides of sampling row 625 (utterances 156..158 are not penalised,
    processors.py:24-27), in the caller's order."""
    c = cases.PARAM_CASES["wide160"]
    Gd = golden["generate_params"]
    lens, rows = _golden_rows(Gd, "wide160", c["B"])
    pick = [157, 3, 159, 64, 156, 12, 158, 155, 0, 131]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t, tm_t = torch.from_numpy(ids[pick]), torch.from_numpy(mask[pick]), torch.from_numpy(tmask[pick])
    emb = gpt_f32.embed_prompt(ids_t, tm_t)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    for use_graph in (True, False):
        out = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"], (*procs, *warpers),
                                    return_hidden=True, manual_seed=c["manual_seed"], use_graph=use_graph, total_rows=c["B"] * 4,
                                    row_ids=torch.tensor(pick)))[-1]
        for i, b in enumerate(pick):
            assert np.array_equal(out.ids[i].cpu().numpy(), rows[b]), (b, use_graph)


def test_two_shards_decoded_as_part_of_the_global_batch_equal_the_unsharded_call(weights):
    """`dist.infer_sharded`'s recipe on the real engine, the two ranks of a world of 2 played one after the other: shards dealt by prompt
    length (`deal_shards`), generated with `row_ids` = global utterance indices, decoded padded to the GLOBAL longest utterance
    (`pad_to`) -- token ids identical and waveforms equal (1e-6) to the single unsharded `Chat.infer_ids` call, row for row; and
    `Chat.infer_sharded` / `dist.infer_sharded` without a process group ARE that call."""
    from chattts_amd import dist as D
    from chattts_amd.core import Chat, InferCodeParams
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32")
    ids, mask, tmask = synth.make_prompts(6, 5, 14, seed=9)
    stop = torch.from_numpy(synth.make_stop_lengths(6, 6, 30, seed=9))
    a = (torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask))
    p = InferCodeParams(max_new_token=31, manual_seed=5, show_tqdm=False)
    full = chat.infer_ids(*a, p, stop_at=stop)
    full_ids = [t.cpu().numpy() for t in list(chat.infer_code(*a, p, stop_at=stop))[-1].ids]
    assert np.array_equal(D.infer_sharded(chat, *a, p, stop_at=stop), full)            # world of one
    shards = D.deal_shards(mask.sum(1).tolist(), 2)
    assert sorted(shards[0] + shards[1]) == list(range(6)) and shards[0] != [0, 1, 2]
    t_max = int(stop.max())
    got = np.zeros_like(full)
    for sel in shards:
        st = torch.tensor(sel)
        out = list(chat.infer_code(a[0][st], a[1][st], a[2][st], p, stop_at=stop[st], row_ids=st, total_rows=6 * 4))[-1]
        for j, b in enumerate(sel):
            assert np.array_equal(out.ids[j].cpu().numpy(), full_ids[b]), b
        wav = chat.decode_to_wavs(out.hiddens, pad_to=t_max)
        for j, b in enumerate(sel):
            got[b] = wav[j]
    assert np.abs(got - full).max() < 1e-6


def test_bf16_free_running_stream_regression_guard(gpt_bf16):
    """the perf mode has no bit-exact bar, so a real regression could hide inside its teacher-forced bounds.  This pins the
    bf16 engine's OWN free-running ids of case `b8` (tests/golden/bf16_guard.npz, tools/make_bf16_guard.py): on the tree that wrote the
    file every row is identical; a deliberate change of the bf16 arithmetic moves rows apart after tens of steps (then the file is
    regenerated); a bug moves them apart at once -- at least 6 of the 8 rows must agree on their first 8 steps, graph replay == eager."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_guard.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/bf16_guard.npz not generated (python tools/make_bf16_guard.py on the GPU box)")
    g = np.load(path)
    off = np.concatenate([[0], np.cumsum(g["lens"])])
    want = [g["ids"][off[b]: off[b + 1]] for b in range(len(g["lens"]))]
    c = cases.GEN_CASES["b8"]
    got = [t.cpu().numpy() for t in run_case(gpt_bf16, c, use_graph=True)[0][-1].ids]
    eager = [t.cpu().numpy() for t in run_case(gpt_bf16, c, use_graph=False)[0][-1].ids]
    assert all(np.array_equal(a, b) for a, b in zip(got, eager))
    first = []
    for a, b in zip(got, want):
        n = min(len(a), len(b))
        neq = np.nonzero((a[:n] != b[:n]).any(1))[0]
        first.append(int(neq[0]) if len(neq) else n)
    assert sum(f >= 8 for f in first) >= 6, first


def _cert_engines(weights, embed=None):
    emb_sd = weights["embed"] if embed is None else embed
    exact = E.GptEngine(weights["gpt"], emb_sd, DEV, dtype="f32")
    x3 = E.GptEngine(weights["gpt"], emb_sd, DEV, dtype="f32x3", exact_fallback=False)
    return exact, x3


def test_parity_certificate_and_exact_fallback(weights, monkeypatch):
    """round 6: dtype "f32x3" certifies every call.  (1) the margins are there, positive, and the bound follows the head's logit scale;
    (2) with the bound raised so that every utterance is flagged, the fallback regenerates them all on the exact kernels: ids AND hidden
    states are the "f32" engine's bits; (3) with the bound at the median margin only the utterances below it are regenerated -- theirs
    are the exact engine's bits, the others keep the split-bf16 engine's."""
    c = cases.GEN_CASES["b8"]
    exact, x3 = _cert_engines(weights)
    out_e = run_case(exact, c, use_graph=True)[0][-1]
    out_x = run_case(x3, c, use_graph=True)[0][-1]
    st = dict(x3.last_stats)
    mg = x3.last_margins.copy()
    assert mg.shape == (8,) and np.isfinite(mg).all() and (mg >= 0).all() and st["min_margin"] == float(mg.min())
    want_bound = 2.0 * E.GptEngine.REL_ERR_X3 * x3.logit_scale[False] / min(c["temperature"])
    assert abs(st["margin_bound"] - want_bound) < 1e-9 * max(1.0, want_bound) and st["exact_rerun_rows"] == []
    assert "min_margin" not in exact.last_stats                      # one arithmetic: nothing to certify
    # an exact call on the engine that did not build the packed f32 copies (no fallback asked for): the row-major f32 kernels, same bits
    assert x3.packed is None and exact.packed is not None
    ids_c, mask_c, tmask_c = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids_c), torch.from_numpy(mask_c)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    out_xe = list(x3.generate(x3.embed_prompt(ids_t, torch.from_numpy(tmask_c)), ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"],
                              c["min_new"], (*procs, *warpers), return_hidden=True, manual_seed=c["manual_seed"], exact=True))[-1]
    for b in range(8):
        assert torch.equal(out_xe.ids[b], out_e.ids[b]) and torch.equal(out_xe.hiddens[b], out_e.hiddens[b]), b
    fb = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32x3", exact_fallback=True)
    monkeypatch.setattr(E.GptEngine, "REL_ERR_X3", 1e3)              # (2) everything is "unsafe"
    out_f = run_case(fb, c, use_graph=True)[0][-1]
    assert fb.last_stats["exact_rerun_rows"] == list(range(8)) and fb.last_stats["certified"]
    for b in range(8):
        assert torch.equal(out_f.ids[b], out_e.ids[b]) and torch.equal(out_f.hiddens[b], out_e.hiddens[b]), b
    med = float(np.median(mg))
    monkeypatch.setattr(E.GptEngine, "REL_ERR_X3", med * min(c["temperature"]) / (2.0 * x3.logit_scale[False]))   # (3)
    out_h = run_case(fb, c, use_graph=True)[0][-1]
    flagged = [b for b in range(8) if mg[b] < fb.last_stats["margin_bound"]]
    assert 0 < len(flagged) < 8 and fb.last_stats["exact_rerun_rows"] == flagged
    for b in range(8):
        ref = out_e if b in flagged else out_x
        assert torch.equal(out_h.ids[b], ref.ids[b]), b
        assert np.abs(out_h.hiddens[b].cpu().numpy() - ref.hiddens[b].cpu().numpy()).max() <= (1e-6 if b in flagged else 0.0), b
    # a second call reuses both sessions (main + exact re-run) and gives the same result
    out_h2 = run_case(fb, c, use_graph=True)[0][-1]
    assert all(torch.equal(a, b_) for a, b_ in zip(out_h.ids, out_h2.ids))


def test_exact_fallback_replays_the_unseeded_draws(weights, golden, monkeypatch):
    """the reference's DEFAULT is manual_seed=None: every step draws from torch's global CPU generator (gpt.py:498-500).  The exact
    fallback then has to re-run flagged utterances with the SAME per-step draws the main call consumed and leave the generator where the
    reference would: with every utterance flagged, the f32x3 engine returns the reference's golden ids of case `unseeded` (== the "f32"
    engine's) and the global generator ends in the state the "f32" engine's own call leaves."""
    c = cases.GEN_CASES["unseeded"]
    Gd = golden["generate"]
    exact = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    out_e = run_case(exact, c, use_graph=True)[0][-1]
    state_e = torch.get_rng_state()
    fb = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32x3", exact_fallback=True)
    monkeypatch.setattr(E.GptEngine, "REL_ERR_X3", 1e3)              # everything is flagged
    out_f = run_case(fb, c, use_graph=True)[0][-1]
    assert fb.last_stats["exact_rerun_rows"] == list(range(c["B"]))
    assert torch.equal(torch.get_rng_state(), state_e)
    got = np.concatenate([t.cpu().numpy() for t in out_f.ids], 0)
    assert np.array_equal(got, Gd["unseeded.ids"]) and all(torch.equal(a, b) for a, b in zip(out_f.ids, out_e.ids))


@pytest.mark.parametrize("gain", [1.0 / 16.0, 1.0, 8.0])
def test_split_bf16_ids_diverge_only_where_the_certificate_fired(weights, gain):
    """the certificate is sound on a head-gain sweep (flatter and peakier logits than the synthetic checkpoint's): wherever
    the split-bf16 engine's free-running ids differ from the exact f32 engine's, that utterance's margin was below the bound -- and the
    fallback engine returns the exact engine's ids for every utterance."""
    emb_sd = dict(weights["embed"])
    for k in range(4):
        key = f"head_code.{k}.parametrizations.weight.original0"
        emb_sd[key] = emb_sd[key] * gain
    exact, x3 = _cert_engines(weights, emb_sd)
    c = dict(cases.GEN_CASES["b8"])
    c["max_new"], c["min_new"] = 96, 96
    out_e = run_case(exact, c, use_graph=True)[0][-1]
    out_x = run_case(x3, c, use_graph=True)[0][-1]
    mg, bound = x3.last_margins, x3.last_stats["margin_bound"]
    assert abs(x3.logit_scale[False] / (E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32").logit_scale[False] * gain) - 1.0) < 1e-5
    for b in range(8):
        if not torch.equal(out_e.ids[b], out_x.ids[b]):
            assert mg[b] < bound, (gain, b, float(mg[b]), bound)
    fb = E.GptEngine(weights["gpt"], emb_sd, DEV, dtype="f32x3", exact_fallback=True)
    out_f = run_case(fb, c, use_graph=True)[0][-1]
    for b in range(8):
        assert torch.equal(out_f.ids[b], out_e.ids[b]), (gain, b)


def test_wide_batch_bf16_rows_do_not_depend_on_the_batch(gpt_bf16):
    """perf mode at 160 utterances in one batch: an utterance's tokens do not depend on which others share the batch -- the first
    and the last 32 of `wide160` generated as shards (same global row numbering) give the tokens they get inside the batch of 160.
    (32 utterances keep the prompt on the kernels the 160 use -- >= 256 prompt rows; below that the prompt runs on the small-batch
    kernels, whose bf16 sums are ordered differently: bf16 results are batch-invariant per kernel family, f32 results everywhere.)"""
    c = cases.PARAM_CASES["wide160"]
    full, _ = run_case(gpt_bf16, c, use_graph=True)
    assert len(full[-1].ids) == 160
    for sl in (slice(0, 32), slice(128, 160)):
        part, _ = run_case(gpt_bf16, c, use_graph=True, rows=sl)
        for i, b in enumerate(range(sl.start, sl.stop)):
            assert torch.equal(part[-1].ids[i], full[-1].ids[b]), b


def test_bench_workload_f32_equals_reference_golden(gpt_f32):
    """the workload bench.py times (C3: 64 utterances, prompts 16-48 tokens, forced lengths U{128..512}, 513 steps, contexts
    up to 560 keys) in parity mode: every one of the 21,438 generated token rows equals the reference's own run of this
    workload (tests/golden/bench_c3.npz, oracle/make_bench_golden.py: the reference's GPT.generate with the harness-side
    length-forcing processor) -- the sha256 bench.py's `parity_mode` reports is this comparison."""
    import os
    import bench
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_c3.npz"))
    wl = bench.shard_workload(64, 1, 0, 128, 512)
    ids_t, mask_t = torch.from_numpy(wl["ids"]), torch.from_numpy(wl["mask"])
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(wl["tmask"]))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    out = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, int(wl["stop_all"].max()) + 1, 0, (*procs, *warpers),
                                return_hidden=True, manual_seed=42, stop_at=torch.from_numpy(wl["stop"])))[-1]
    rows = [t.cpu().numpy() for t in out.ids]
    assert np.array_equal(np.array([len(r) for r in rows]), gold["lens"])
    got = np.concatenate(rows, 0)
    want = gold["ids"].astype(np.int64)
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())} of {len(want)} token rows differ"
    assert bench.ids_digest(rows) == str(gold["sha256"])
    assert np.abs(out.hiddens[0][:4].cpu().numpy() - gold["hid0_first"]).max() < 2e-4
    assert np.abs(out.hiddens[0][-4:].cpu().numpy() - gold["hid0_last"]).max() < 2e-4


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_workload_dealt_over_ranks_equals_the_reference_run_of_the_global_batch(gpt_f32, world):
    """What `bench.py --gpus N` runs, the N ranks played one after the other on this GPU: the GLOBAL batch of 64 N utterances dealt by prompt
    length (bench.shard_workload -> dist.deal_shards), every shard generated with its global row ids / total_rows -- each of its token rows
    is compared with the reference's row of the SAME utterance in its single run of the whole global batch (tests/golden/bench_c3_w{N}.npz,
    `python -m oracle.make_bench_golden --world N`: the reference has no data-parallel mode).  This is the comparison behind
    `ids_check.ids_match_reference` on an N-rank bench line; the Exp(1) draws of a row and the rows >= 625 penalty quirk (row 157 onwards:
    N = 4 has 99 such utterances) follow the global numbering.
    THE FLOAT32 FLOOR, met here for the first time (profiles/r6D_w2_divergence.log): of the 128 utterances of N = 2 (163,052 draws) ONE --
    global 32, step 364 of 445, code book 2 -- leaves the reference's stream, at the same step in BOTH parity arithmetics (f32 MFMA and
    split-fp16).  Evaluated in float64 on the reference's own tokens (tools/near_tie_f64.py, profiles/r6D_near_tie_f64.log) that draw is
    decided by 9.3e-6 tempered-logit units = THREE float32 ulps of the logit (float64 sides with the reference's token): the summation
    order of a float32 dot product moves a logit by more than that (MKL's blocked AVX-512 sums on the reference's side, MFMA accumulation
    here; rms distance of either engine to float64: 2-3e-7 relative).  No float32 engine other than the reference's own binary at the same
    thread count reproduces such a draw; the certificate exists to name them (this one: margin 5.2e-6 on the device, flagged).  The bar of this test: every other
    utterance is bit-exact, an utterance may differ only if its own decision margin (`last_margins`, computed by `sample_k` in either
    arithmetic) is below the certificate's bound, and at most 1 % of the utterances do."""
    import os
    import bench
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_c3_w%d.npz" % world)
    if not os.path.exists(path):
        pytest.skip("tests/golden/bench_c3_w%d.npz not generated (python -m oracle.make_bench_golden --world %d, build container)" % (world, world))
    gold = np.load(path)
    off = np.concatenate([[0], np.cumsum(gold["lens"].astype(np.int64))])
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    bound = 2.0 * E.GptEngine.REL_ERR_X3 * gpt_f32.logit_scale[False] / 0.3
    seen, differing = [], []
    for rank in range(world):
        wl = bench.shard_workload(64, world, rank, 128, 512)
        assert len(wl["sel"]) == 64 and wl["total_rows"] == 64 * world * 4
        ids_t, mask_t = torch.from_numpy(wl["ids"]), torch.from_numpy(wl["mask"])
        emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(wl["tmask"]))
        out = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, int(wl["stop_all"].max()) + 1, 0, (*procs, *warpers),
                                    manual_seed=42, stop_at=torch.from_numpy(wl["stop"]), row_offset=wl["row_offset"], row_ids=wl["row_ids"],
                                    total_rows=wl["total_rows"]))[-1]
        rows = [t.cpu().numpy() for t in out.ids]
        bad = [j for j, (r, b) in enumerate(zip(rows, wl["sel"])) if not np.array_equal(r, gold["ids"][off[b]: off[b + 1]].astype(np.int64))]
        assert all(float(gpt_f32.last_margins[j]) < bound for j in bad), (rank, [(wl["sel"][j], float(gpt_f32.last_margins[j])) for j in bad])
        if gpt_f32.x3 is not None:
            assert set(bad) <= set(gpt_f32.last_stats["uncertified_rows"])
        differing += [int(wl["sel"][j]) for j in bad]
        seen += list(wl["sel"])
    assert sorted(seen) == list(range(64 * world))
    assert len(differing) <= max(1, 64 * world // 100), differing

def _golden_rows(Gd, name, B):
    lens = Gd[name + ".lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    return lens, [Gd[name + ".ids"][off[b]: off[b + 1]] for b in range(B)]


@pytest.mark.parametrize("name,file", [("b8", "generate"), ("long", "generate"), ("c3w", "generate_big")])
def test_bf16_mode_teacher_forced_drift(gpt_bf16, weights, golden, name, file):
    """perf mode (bf16 weights, bf16 KV cache, bf16 inter-kernel activations) is not bit-exact by construction; this
    bounds its drift over ALL steps on the reference's own token stream: both sides are fed the golden ids (teacher
    forcing), the oracle (f32 restatement pinned on those goldens) gives the per-step hidden states and pre-processor
    logits, and the bf16 engine must stay within a relative hidden error of 1.5e-2 and an absolute logit error of 0.25
    (logit std ~4) at every step of every row -- no growth with the step index.  The free-running match rate is printed."""
    c = (cases.GEN_CASES if file == "generate" else cases.BIG_CASES)[name]
    Gd = golden[file]
    ids, mask, tmask = cases.gen_inputs(c)
    B, n = ids.shape[0], c["max_new"]
    if name == "c3w":          # 64 rows x 40 steps through the numpy oracle is slow: teacher-force the first 16 utterances
        B = 16
    lens, rows = _golden_rows(Gd, name, ids.shape[0])
    teacher = np.zeros((B, n, 4), np.int64)
    for b in range(B):
        teacher[b, : lens[b]] = rows[b]
        if lens[b] < n:
            teacher[b, lens[b]] = 625     # the EOS step itself (gpt.py:512-518): the row finishes exactly like the golden run
    sl = slice(0, B)
    ids, mask, tmask = ids[sl], mask[sl], tmask[sl]
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    heads = generate_np.fold_heads(esd)
    ref = generate_np.generate(llama, esd, heads, generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                               temperature=np.array(c["temperature"], np.float32), draw_q=lambda i: None, pow_table=None,
                               max_new_token=n, teacher_ids=teacher, keep_logits=True)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_bf16.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    out = list(gpt_bf16.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                 return_hidden=True, manual_seed=c["manual_seed"], teacher_ids=torch.from_numpy(teacher),
                                 total_rows=cases.gen_inputs(c)[0].shape[0] * 4))[-1]
    worst_h, worst_l, first_h, last_h = 0.0, 0.0, [], []
    for b in range(B):
        assert np.array_equal(out.ids[b].cpu().numpy(), rows[b]), b      # the forced stream was followed, finish included
        got = out.hiddens[b].cpu().numpy().astype(np.float64)
        want = ref.hiddens[b].astype(np.float64)
        assert got.shape == want.shape == (lens[b], 768)
        rel = np.abs(got - want).max(1) / np.abs(want).max(1)
        dlog = np.abs((got - want) @ heads.astype(np.float64).T).max(1)
        worst_h, worst_l = max(worst_h, rel.max()), max(worst_l, dlog.max())
        first_h.append(rel[: max(1, lens[b] // 4)].mean())
        last_h.append(rel[-max(1, lens[b] // 4):].mean())
    # free-running agreement with the reference stream (informational)
    free = list(gpt_bf16.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                  return_hidden=False, manual_seed=c["manual_seed"],
                                  total_rows=cases.gen_inputs(c)[0].shape[0] * 4))[-1]
    match = sum(int((free.ids[b].cpu().numpy()[: min(len(free.ids[b]), lens[b])] == rows[b][: min(len(free.ids[b]), lens[b])]).all(1).sum())
                for b in range(B))
    print(f"bf16 teacher-forced [{name}]: worst hidden rel err {worst_h:.3e}, worst |dlogit| {worst_l:.3e}, "
          f"mean rel err first quarter {np.mean(first_h):.3e} / last quarter {np.mean(last_h):.3e}; "
          f"free-running token-row match {match}/{int(lens[:B].sum())}")
    assert worst_h < 1.5e-2, worst_h     # measured 3.0e-3 .. 5.1e-3
    assert worst_l < 0.25, worst_l       # measured 0.06 .. 0.09
    assert np.mean(last_h) < 2.0 * np.mean(first_h) + 1e-3     # no systematic growth with the step index


@pytest.mark.parametrize("env", ["CTTS_QKV_ATT", "CTTS_ATT_OPROJ"])
def test_opt_in_fused_launches_follow_the_default_path(weights, golden, env, monkeypatch):
    """The two opt-in launch fusions of the perf mode's decode step (round 4, measured and left OFF by default: profiles/r4*.log) --
    CTTS_QKV_ATT=1: QKV + attention as one launch whose attention units pick q / the newest key up through per-head arrival words;
    CTTS_ATT_OPROJ=1: o_proj + residual folded into the attention launch (12 -> 1 hand-off through memory per row) -- against the
    default launch sequence, both teacher-forced on the reference's golden stream `b8` (left-padded rows, rows finishing at different
    steps): same forced tokens, hidden states of EVERY step within 5e-3 relative (they differ in summation order only), and the
    fused engine's own free run repeats itself bit for bit (graph replay == eager launches: the hand-offs are race-free)."""
    c = cases.GEN_CASES["b8"]
    ids, mask, tmask = cases.gen_inputs(c)
    B, n = ids.shape[0], c["max_new"]
    lens, rows = _golden_rows(golden["generate"], "b8", B)
    teacher = np.zeros((B, n, 4), np.int64)
    for b in range(B):
        teacher[b, : lens[b]] = rows[b]
        if lens[b] < n:
            teacher[b, lens[b]] = 625
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])

    def run(eng, **kw):
        emb = eng.embed_prompt(ids_t, torch.from_numpy(tmask))
        return list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                 return_hidden=True, manual_seed=c["manual_seed"], **kw))[-1]

    base = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="bf16")
    ref = run(base, teacher_ids=torch.from_numpy(teacher))
    ref_h = [h.cpu().numpy().astype(np.float64) for h in ref.hiddens]
    del base
    monkeypatch.setenv(env, "1")      # read once, by ctts_gpt_create
    fused = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="bf16")
    got = run(fused, teacher_ids=torch.from_numpy(teacher))
    worst = 0.0
    for b in range(B):
        assert np.array_equal(got.ids[b].cpu().numpy(), rows[b]), b
        g = got.hiddens[b].cpu().numpy().astype(np.float64)
        assert g.shape == ref_h[b].shape
        worst = max(worst, float((np.abs(g - ref_h[b]).max(1) / np.abs(ref_h[b]).max(1)).max()))
    assert worst < 5e-3, worst
    a = run(fused, use_graph=True)
    b_ = run(fused, use_graph=False)
    assert all(torch.equal(x, y) for x, y in zip(a.ids, b_.ids))
    assert all(torch.equal(x, y) for x, y in zip(a.hiddens, b_.hiddens))
    print(f"{env}=1 vs default, teacher-forced b8: worst relative hidden difference {worst:.2e}")


def test_capi_weight_broadcast_world1():
    """`ctts_broadcast_weights` (the ONE collective of the path) through the C ABI on a real MI355X: librccl.so is
    dlopen'ed lazily, a communicator of world size 1 is made from a unique id (`ctts_rccl_unique_id` / `ctts_rccl_comm_create`), and an
    in-place byte-typed broadcast of two flat weight buffers leaves them unchanged and completes on the caller's stream.  (N > 1 needs
    a multi-GPU box: `bench.py --gpus N --capi-broadcast-check` checks the same entry point against torch.distributed's broadcast there.)"""
    from chattts_amd import dist as D
    comm = D.CapiComm(1, 0)
    a = torch.arange(1 << 20, dtype=torch.float32, device=DEV)
    b = torch.full((12345,), 3, dtype=torch.bfloat16, device=DEV)
    a0, b0 = a.clone(), b.clone()
    comm.broadcast([a, b, torch.empty(0, device=DEV)], root=0)
    torch.cuda.synchronize()
    assert torch.equal(a, a0) and torch.equal(b, b0)
    comm.close()


def test_stream_chunks_match_oracle(weights):
    """stream=True (core.py:455-503): every emitted chunk is the next `stream_speed` samples of the ORACLE's decode of
    the prefix the reference would have at that yield (ids bit-exact in f32 mode, waveform within 1e-4 RMS)."""
    from chattts_amd import rng
    from chattts_amd.core import Chat, InferCodeParams
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32")
    ids, mask, tmask = synth.make_prompts(3, 8, 12, seed=3)
    stop = np.array([80, 52, 30], np.int32)
    p = InferCodeParams(max_new_token=96, manual_seed=5, show_tqdm=False, stream_speed=9000)
    chunks = list(chat.infer_ids_stream(torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask), p,
                                        stop_at=torch.from_numpy(stop)))
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    draws = rng.ExpDraws(3 * 4, 626, 5)
    ref = generate_np.generate(llama, esd, generate_np.fold_heads(esd), generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                               temperature=np.array([0.3] * 4, np.float32), draw_q=lambda i: draws.step(i).numpy(),
                               pow_table=rng.penalty_table(1.05).numpy(), max_new_token=96, stop_at=stop)
    assert [r.shape[0] for r in ref.ids] == stop.tolist()
    dsd = {k: v.numpy() for k, v in weights["decoder"].items()}
    vsd = {k: v.numpy() for k, v in weights["vocos"].items()}
    # yields at 24, 48, 72 live steps and the final result at 80 (the last row's EOS step is 80: not a multiple of 24);
    # the first two are dropped (pass_first_n_batches = 2)
    want, length = [], 0
    for n in (72, 80):
        wav = codec_np.decode_to_wavs(dsd, vsd, [h[: min(n, h.shape[0])] for h in ref.hiddens])
        if n == 72:
            want.append(wav[:, length: min(length + 9000, wav.shape[1])])
            length = min(length + 9000, wav.shape[1])
        else:   # the final yield: first its regular slice, then the tail with all-silent columns removed
            want.append(wav[:, length: min(length + 9000, wav.shape[1])])
            length = min(length + 9000, wav.shape[1])
            tail = wav[:, length:]
    assert len(chunks) == 3
    for got, w in zip(chunks[:2], want):
        assert got.shape == w.shape, (got.shape, w.shape)
        assert float(np.sqrt(np.mean((got - w) ** 2))) < 1e-4
    keep = np.sum(np.abs(tail) > 1e-5, axis=0) > 0
    if chunks[2].shape == tail[:, keep].shape:      # the 1e-5 silence filter can flip on a borderline column
        assert float(np.sqrt(np.mean((chunks[2] - tail[:, keep]) ** 2))) < 1e-4
    else:
        assert abs(chunks[2].shape[1] - int(keep.sum())) <= 8


def test_sharded_rows_equal_full_batch(gpt_f32, golden):
    """rows [4,8) of the b8 batch generated alone (row_offset / total_rows) == the same rows of the
    full-batch reference run: the data-parallel sharding contract."""
    c = cases.GEN_CASES["b8"]
    outs, _ = run_case(gpt_f32, c, use_graph=True, rows=slice(4, 8))
    Gd = golden["generate"]
    lens = Gd["b8.lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, b in enumerate(range(4, 8)):
        want = Gd["b8.ids"][off[b]: off[b + 1]]
        got = outs[0].ids[i].cpu().numpy()
        # the shard stops as soon as ITS rows finish; rows that finished earlier in the full batch are identical
        assert np.array_equal(got, want), b


def test_lanes_do_not_change_results(gpt_f32, golden):
    """the batch cut into 3 concurrently decoding lanes (own stream, graph, compaction state each) == reference run"""
    c = cases.GEN_CASES["b8"]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    out = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"], (*procs, *warpers),
                                return_hidden=True, manual_seed=c["manual_seed"], lanes=3))[-1]
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    assert np.array_equal(np.array([int(t.shape[0]) for t in out.ids]), golden["generate"]["b8.lens"])
    assert np.array_equal(got, golden["generate"]["b8.ids"])
    assert gpt_f32.last_stats["lanes"] == 3


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(cases.GEN_STREAM_CASES))
def test_stream_yields_equal_the_reference(gpt_f32, golden, name, use_graph):
    """tests/golden/generate_stream.npz: EVERY yield of the reference's GPT.generate(stream=True) (gpt.py:579-589) -- how many there
    are, where each row is cut (its own end_idx: finished rows stop growing), the ids inside, the number of hidden rows -- for
    stream_batch 24 (default), 5 (not a divisor of max_new), 7 with the unseeded global-generator draws, and 16 where the final
    yield repeats the last streamed one.  Copies are taken at yield time, as a consumer would see them."""
    base, sb = cases.GEN_STREAM_CASES[name]
    c = cases.GEN_CASES[base]
    Gd = golden["generate_stream"]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    if c["manual_seed"] is None:
        torch.manual_seed(c["global_seed"])
    lens, hid_lens, rows = [], [], []
    for out in gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"], (*procs, *warpers),
                                return_hidden=True, stream=True, stream_batch=sb, manual_seed=c["manual_seed"], use_graph=use_graph):
        lens.append([int(t.shape[0]) for t in out.ids])
        hid_lens.append([int(h.shape[0]) for h in out.hiddens])
        rows += [t.cpu().numpy().copy() for t in out.ids]
    assert np.array_equal(np.array(lens), Gd[name + ".lens"]), (lens, Gd[name + ".lens"].tolist())
    assert np.array_equal(np.array(hid_lens), Gd[name + ".hid_lens"])
    assert np.array_equal(np.concatenate(rows, 0), Gd[name + ".ids"])


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(cases.REGEN_CASES))
def test_unexpected_end_at_step0_follows_the_reference(gpt_f32, golden, name, use_graph):
    """tests/golden/generate_regen.npz: a row draws EOS at the very first step (gpt.py:527-570).  Unseeded, the reference discards the
    attempt and calls itself again with the global generator one [rows, 626] draw further on -- the engine's second attempt must see
    exactly those draws (ids bit-exact) and leave the generator where the reference leaves it; seeded, the reference warns and yields
    NOTHING, and so does the engine (and neither touches the global generator)."""
    c = cases.REGEN_CASES[name]
    Gd = golden["generate_regen"]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    torch.manual_seed(c.get("global_seed", 999))
    outs = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"], (*procs, *warpers),
                                 return_hidden=True, manual_seed=c["manual_seed"], use_graph=use_graph))
    after = torch.rand(3).numpy()
    assert np.array_equal(after, Gd[name + ".rand_after"])
    if not bool(Gd[name + ".yielded"][0]):
        assert outs == []
        return
    assert len(outs) == 1
    assert np.array_equal(np.array([int(t.shape[0]) for t in outs[0].ids]), Gd[name + ".lens"])
    assert np.array_equal(np.concatenate([t.cpu().numpy() for t in outs[0].ids], 0), Gd[name + ".ids"])
    assert [int(h.shape[0]) for h in outs[0].hiddens] == Gd[name + ".lens"].tolist()


def test_stream_yield_schedule(gpt_f32):
    c = dict(cases.GEN_CASES["c1"])
    outs, _ = run_case(gpt_f32, c, use_graph=True, stream=True)
    # 48 steps, stream_batch 24, never finishes: yields at step 24 and 48 (gpt.py:579-589) + the final yield
    assert [int(o.ids[0].shape[0]) for o in outs] == [24, 48, 48]


def test_stop_at_matches_oracle(gpt_f32, weights):
    """bench workload hook: forced output lengths, HIP path vs the numpy oracle (4 layers would be
    cheaper, but the full model is what ships)."""
    B = 3
    ids, mask, tmask = synth.make_prompts(B, 8, 12, seed=9)
    stop = np.array([5, 9, 14], np.int32)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    out = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, 32, 0, (*procs, *warpers), return_hidden=True,
                                manual_seed=3, stop_at=torch.from_numpy(stop)))[-1]
    from chattts_amd import rng
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    draws = rng.ExpDraws(B * 4, 626, 3)
    ref = generate_np.generate(llama, esd, generate_np.fold_heads(esd), generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                               temperature=np.array([0.3] * 4, np.float32), draw_q=lambda i: draws.step(i).numpy(),
                               pow_table=rng.penalty_table(1.05).numpy(), max_new_token=32, stop_at=stop)
    assert [int(t.shape[0]) for t in out.ids] == stop.tolist() == [r.shape[0] for r in ref.ids]
    for b in range(B):
        assert np.array_equal(out.ids[b].cpu().numpy(), ref.ids[b])
        assert np.abs(out.hiddens[b].cpu().numpy() - ref.hiddens[b]).max() < 2e-4


def test_bf16_mode_runs_and_tracks_f32(gpt_bf16, golden):
    """perf mode (bf16 weights + KV): not bit-exact by construction; report the token match rate and
    require the first sampled token row and the teacher-free hidden state of step 0 to stay close."""
    c = cases.GEN_CASES["b8"]
    outs, _ = run_case(gpt_bf16, c, use_graph=True)
    out = outs[0]
    Gd = golden["generate"]
    lens = Gd["b8.lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    match, total = 0, 0
    for b in range(8):
        got = out.ids[b].cpu().numpy()
        want = Gd["b8.ids"][off[b]: off[b + 1]]
        n = min(len(got), len(want))
        assert n > 0 and (got >= 0).all() and (got <= 625).all()
        match += int((got[:n] == want[:n]).all(1).sum())
        total += n
    h0 = out.hiddens[0].cpu().numpy()[0]
    ref0 = Gd["b8.hid0"][0]
    rel = np.abs(h0 - ref0).max() / np.abs(ref0).max()
    print(f"bf16 token-row match rate {match}/{total}, step-0 hidden rel err {rel:.3e}")
    assert rel < 5e-2


def test_packed_decode_equals_row_major_decode(weights, golden, monkeypatch):
    """perf mode: the decode step on fragment-packed operands (csrc/decode.hip) multiplies the same bf16 values as the row-major kernels
    it replaces.  Until round 4 both split K over 4 waves the same way and free-running token ids were identical; since round 5 the packed
    QKV / gate-up launches split K over 8 waves (another order of the f32 partial sums), so the two engines are compared the way the perf
    mode is bounded anywhere else: TEACHER-FORCED on the reference's token stream (b8), hidden states of every step within bf16 rounding
    noise of each other (measured 2e-3 relative; asserted 1e-2), and -- with CTTS_DEC_NW-independent arithmetic -- the f32 twin of this
    test stays bit-identical."""
    c = cases.GEN_CASES["b8"]
    Gd = golden["generate"]
    ids, mask, tmask = cases.gen_inputs(c)
    B, n = ids.shape[0], c["max_new"]
    lens, rows = _golden_rows(Gd, "b8", B)
    teacher = np.zeros((B, n, 4), np.int64)
    for b in range(B):
        teacher[b, : lens[b]] = rows[b]
        if lens[b] < n:
            teacher[b, lens[b]] = 625
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    hid = []
    for packed in ("1", "0"):
        monkeypatch.setenv("CTTS_DEC_PACKED", packed)
        eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="bf16")
        emb = eng.embed_prompt(ids_t, torch.from_numpy(tmask))
        out = list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                return_hidden=True, manual_seed=c["manual_seed"], teacher_ids=torch.from_numpy(teacher)))[-1]
        assert [int(t.shape[0]) for t in out.ids] == lens.tolist()
        hid.append([h.cpu().numpy() for h in out.hiddens])
        del eng
    worst = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(*hid) if len(a))
    print(f"packed vs row-major bf16 decode, teacher-forced b8: worst hidden rel diff {worst:.3e}")
    assert worst < 1e-2


def test_packed_f32_decode_is_bit_identical_to_row_major(weights, monkeypatch):
    """parity mode: the decode step on fragment-packed f32 operands (csrc/decode32.hip) keeps the operation order of the
    row-major kernels the goldens were established with -> identical token ids AND bit-identical hidden states"""
    c = cases.GEN_CASES["b8"]
    packed = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    outs_p, _ = run_case(packed, c, use_graph=True)
    monkeypatch.setenv("CTTS_DEC_PACKED", "0")
    plain = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    outs_r, _ = run_case(plain, c, use_graph=True)
    for a, b in zip(outs_p[0].ids, outs_r[0].ids):
        assert torch.equal(a, b)
    for a, b in zip(outs_p[0].hiddens, outs_r[0].hiddens):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["bf16", "f32x3"])
def test_bounded_row_graphs_replay_to_the_same_bits(weights, dtype, monkeypatch):
    """round 5, opt-in (CTTS_GRAPH_ROWS=1; measured no gain, profiles/r5o_ab_graph_rows.log): chunks of decode steps are replayed from the
    graph captured for a BOUND on the live rows (16-row buckets; ctts_gpt_graph_build_rows) once finish polls have seen utterances leave -- the grids shrink, the kernels still read the exact live
    count.  c3w (64 utterances, 20 of them hitting EOS at different steps) and a batch in which most rows finish early: token ids AND
    hidden states torch.equal to the batch-sized graph (CTTS_GRAPH_ROWS=0), bounded graphs really used, a second call reuses them."""
    outs = {}
    for rows in ("1", "0"):
        monkeypatch.setenv("CTTS_GRAPH_ROWS", rows)
        eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)
        res = []
        for name, stop in (("c3w", None), ("c3w", "early")):
            c = dict(cases.BIG_CASES[name])
            ids, mask, tmask = cases.gen_inputs(c)
            B = ids.shape[0]
            ids_t, mask_t, tm_t = torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask)
            emb = eng.embed_prompt(ids_t, tm_t)
            warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
            kw = {}
            n = c["max_new"]
            if stop == "early":      # 50 of the 64 rows are forced to stop within the first chunks: bounds 64 -> 32 -> 16
                n = 96
                st = np.full(B, 90, np.int32)
                st[:50] = 3 + (np.arange(50) % 30)
                kw["stop_at"] = torch.from_numpy(st)
            for rep in range(2):
                out = list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                        return_hidden=True, manual_seed=c["manual_seed"], **kw))[-1]
            res.append(([t.clone() for t in out.ids], [h.clone() for h in out.hiddens]))
            built = eng._session.get("rows_built", [set()])[0]
            if stop == "early":
                assert (len(built) >= 2 and max(built) < 64) if rows == "1" else (len(built) == 0), (rows, built)
        outs[rows] = res
        del eng
    for (ia, ha), (ib, hb) in zip(outs["1"], outs["0"]):
        assert all(torch.equal(x, y) for x, y in zip(ia, ib)) and all(torch.equal(x, y) for x, y in zip(ha, hb))


def test_attention_split_in_the_engine(weights, golden, monkeypatch):
    """the whole decode step with and without the attention remainder splitting, teacher-forced on the same token stream
    (the c3w batch: 64 utterances whose number drops as they finish, so the split geometry changes from step to step):
    hidden states agree to bf16-rounding noise at every step"""
    c = cases.BIG_CASES["c3w"]
    Gd = golden["generate_big"]
    ids, mask, tmask = cases.gen_inputs(c)
    B, n = ids.shape[0], c["max_new"]
    lens, rows = _golden_rows(Gd, "c3w", B)
    teacher = np.zeros((B, n, 4), np.int64)
    for b in range(B):
        teacher[b, : lens[b]] = rows[b]
        if lens[b] < n:
            teacher[b, lens[b]] = 625
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    hid = []
    for split in ("1", "0"):
        monkeypatch.setenv("CTTS_ATT_SPLIT", split)
        eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="bf16")
        emb = eng.embed_prompt(ids_t, torch.from_numpy(tmask))
        out = list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, n, c["min_new"], (*procs, *warpers),
                                return_hidden=True, manual_seed=c["manual_seed"], teacher_ids=torch.from_numpy(teacher)))[-1]
        assert [int(t.shape[0]) for t in out.ids] == lens.tolist()
        hid.append([h.cpu().numpy() for h in out.hiddens])
        del eng
    worst = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(*hid) if len(a))
    print(f"attention split vs whole units, teacher-forced c3w: worst hidden rel diff {worst:.3e}")
    assert worst < 1e-2


@pytest.mark.parametrize("name", list(cases.CODEC_CASES))
def test_codec_vs_reference_golden(codec, golden, name):
    c = cases.CODEC_CASES[name]
    hid = cases.codec_inputs(c)
    mel = codec.dvae_decode(torch.from_numpy(hid))
    ref_mel = golden["codec"][name + ".mel"].transpose(0, 2, 1)
    merr = np.abs(mel.cpu().numpy() - ref_mel).max()
    assert merr < 1e-4 * max(1.0, np.abs(ref_mel).max()), merr
    wav = codec.vocos_decode(mel).cpu().numpy()
    ref = golden["codec"][name + ".wav"]
    assert wav.shape == ref.shape
    rms = float(np.sqrt(np.mean((wav - ref) ** 2)))
    print(f"codec[{codec.gemm}] {name}: mel max err {merr:.2e}, wav rms err {rms:.2e}")
    assert rms < 1e-4, rms   # north_star: float32 waveform within 1e-4 RMS (signal rms ~ 3.5e-2)


@pytest.mark.parametrize("gemm", ["bf16x3", "f16", "f32"])
@pytest.mark.parametrize("name", list(cases.CODEC_BIG_CASES))
def test_codec_baseline_sizes_vs_reference_golden(weights, golden, name, gemm):
    """The acoustic decoder AT THE SIZES THE BENCH RUNS IT, against the reference itself: inputs are the reference
    GPT's own hidden states (runs of generate_big.npz c2.hid0), mel is the output of the reference's DVAE class
    (ChatTTS/model/dvae.py:276-297), the waveform that of oracle/torch_port.vocos_decode on it (tests/golden/codec_big.npz,
    oracle/make_goldens.py codec_big).  c2size = 1 x 512 tokens (1024 frames: gemm_x3p_k / gemm_h1p_k, the LDS-DMA point-wise pairs);
    r16x400 = 16 ragged rows zero-padded to 400 tokens (12800 frames: 256 x 256 split-bf16 tiles, dwconv_ln_run_k).  Every dense-layer
    mode is compared DIRECTLY -- no HIP-vs-HIP step: strided samples whose phase walks with the row (every 4th mel frame, every 16th
    waveform sample) and float64 block sums over every element.  Bars: mel within 1e-4 of its peak and waveform within 1e-4 RMS
    (north_star) for the f32-class modes; gemm="f16" (one fp16 MFMA per product): mel within 2e-3 of its peak, waveform within 2e-5 RMS
    -- measured 1.3e-5, a fifth of the bar."""
    c = cases.CODEC_BIG_CASES[name]
    Gd = golden["codec_big"]
    hid, lens = cases.codec_big_inputs(c, golden["generate_big"]["c2.hid0"])
    assert np.array_equal(lens, Gd[name + ".lens"])
    assert W.fingerprint({"h": torch.from_numpy(hid)}) == str(Gd[name + ".hid_sha256"])     # the input the reference saw, bit for bit
    eng = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    mel = eng.dvae_decode(torch.from_numpy(hid))                 # [B, 2T, 100]
    wav = eng.vocos_decode(mel).cpu().numpy()                    # [B, 256 (2T - 1)]
    got = cases.codec_big_subsample(mel.cpu().numpy().transpose(0, 2, 1), wav)
    peak, wrms = float(Gd[name + ".mel_peak"][0]), float(Gd[name + ".wav_rms"][0])
    merr = float(np.abs(got["mel_s"] - Gd[name + ".mel_s"]).max()) / peak
    rms = float(np.sqrt(np.mean((got["wav_s"].astype(np.float64) - Gd[name + ".wav_s"]) ** 2)))
    # block sums: every mel bin of every 32-frame block, every 2048-sample block of the waveform (a wrong tile / row / tail shows here even
    # if the strided samples miss it); |sum of n errors| <= n * max error
    mblk = float(np.abs(got["mel_blk"] - Gd[name + ".mel_blk"]).max()) / (32 * peak)
    wblk = float(np.abs(got["wav_blk"] - Gd[name + ".wav_blk"]).max()) / 2048
    wsq = float(np.abs(np.sqrt(got["wav_sq"] / 2048) - np.sqrt(Gd[name + ".wav_sq"] / 2048)).max())
    print(f"codec[{gemm}] {name}: mel max err / peak {merr:.2e} (block mean {mblk:.2e}), wav rms err {rms:.2e} (block mean {wblk:.2e}, "
          f"block rms {wsq:.2e}; signal rms {wrms:.2e})")
    mel_bar, wav_bar = (2e-3, 2e-5) if gemm == "f16" else (1e-4, 1e-4)
    assert merr < mel_bar and mblk < mel_bar, (merr, mblk)
    assert rms < wav_bar and wblk < wav_bar and wsq < wav_bar, (rms, wblk, wsq)


def test_generate_rows_are_views_of_the_padded_batch(gpt_f32, weights):
    """`GptEngine.generate` hands out its per-utterance rows as views of ONE copy per result (engine.RowList): the hidden rows sit in
    the zero-padded [B, Tmax, 768] batch `_decode_to_wavs` would rebuild from them (core.py:525-533), which the decoder takes as
    is.  Same waveform, bit for bit, as the generic path over a plain list of the same rows; ragged lengths (b8)."""
    outs, _ = run_case(gpt_f32, cases.GEN_CASES["b8"], use_graph=True)
    out = outs[-1]
    lens = [int(r.shape[0]) for r in out.hiddens]
    assert isinstance(out.hiddens, E.RowList) and out.hiddens.padded is not None and len(set(lens)) > 1
    pad = out.hiddens.padded
    assert tuple(pad.shape) == (len(lens), max(lens), 768)
    for b, n in enumerate(lens):
        assert torch.equal(pad[b, :n], out.hiddens[b]) and not bool(pad[b, n:].any())
        assert out.ids[b].shape[0] == n and out.ids[b].is_contiguous() and out.hiddens[b].is_contiguous()
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV)
    fast = codec.decode_to_wavs(out.hiddens)
    plain = codec.decode_to_wavs([r.clone() for r in out.hiddens])
    assert torch.equal(fast, plain)
    assert torch.equal(codec.decode_to_wavs(out.hiddens[:3]), codec.decode_to_wavs([r.clone() for r in out.hiddens[:3]]))   # a slice is a plain list


def test_to_host_in_pieces_equals_cpu_numpy(weights):
    """`CodecEngine.to_host` of a batch's worth of waveforms (>= 16 MB): the bus copy and the copy out of the pinned staging buffer run
    in 4 overlapped pieces; the result is a fresh array equal to `.cpu().numpy()`, for sizes that do and do not divide evenly"""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    for shape in ((64, 261888), (5, 1000016), (3, 700000)):
        t = torch.randn(shape, device=DEV, generator=g)
        a = codec.to_host(t)
        b = codec.to_host(t * 2.0)          # the staging buffer is reused: `a` must not change
        ref = t.cpu().numpy()
        assert a.dtype == np.float32 and a.shape == tuple(shape) and np.array_equal(a, ref) and np.array_equal(b, ref * 2.0)


def test_decode_to_wavs_padding(codec, weights, golden):
    """ragged rows are zero padded like core.py:525-533; compare with the oracle on a larger batch, and with what the reference's own
    `Chat._decode_to_wavs` (run unmodified over the reference DVAE, codec.npz `ragged.wav`) returns for these rows"""
    rows = cases.ragged_rows()
    wav = codec.decode_to_wavs([torch.from_numpy(r) for r in rows]).cpu().numpy()
    gold = golden["codec"]["ragged.wav"]
    assert wav.shape == gold.shape and wav.dtype == gold.dtype
    assert float(np.sqrt(np.mean((wav - gold) ** 2))) < 1e-4
    dsd = {k: v.numpy() for k, v in weights["decoder"].items()}
    vsd = {k: v.numpy() for k, v in weights["vocos"].items()}
    ref = codec_np.decode_to_wavs(dsd, vsd, rows)
    assert wav.shape == ref.shape == (4, 256 * (2 * 40 - 1))
    assert float(np.sqrt(np.mean((wav - ref) ** 2))) < 1e-4


def test_long_audio_prompt_prefill_tracks_oracle(gpt_bf16, weights):
    """a zero-shot style prompt: 40 text tokens followed by ~400 audio-code tokens per row (`spk_smp`, core.py:435-453;
    tokenizer.py:85-110 puts the codes in the 4 slots with text_mask False), B = 4 mixed lengths, left padded -- the
    flash-style MFMA prefill attention (T >= 128) -- then 6 teacher-forced decode steps: hidden states stay within the bf16
    drift bound of the oracle; the same prompt prefilled in chunks of 192 slots gives the same result to rounding"""
    rs = np.random.RandomState(21)
    lens = [440, 300, 512, 397]
    T, B, n = max(lens), 4, 6
    ids = np.zeros((B, T, 4), np.int64)
    mask = np.zeros((B, T), bool)
    tmask = np.zeros((B, T), bool)
    for b, L in enumerate(lens):
        ids[b, T - L: T - L + 40] = rs.randint(1, 21178, size=(40, 1))
        ids[b, T - L + 40:] = rs.randint(0, 625, size=(L - 40, 4))
        mask[b, T - L:] = True
        tmask[b, T - L: T - L + 40] = True
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    heads = generate_np.fold_heads(esd)
    teacher = rs.randint(0, 625, size=(B, n, 4)).astype(np.int64)
    ref = generate_np.generate(llama, esd, heads, generate_np.embed_prompt(esd, ids, tmask), ids, mask, temperature=np.array([0.3] * 4, np.float32),
                               draw_q=lambda i: None, pow_table=None, max_new_token=n, teacher_ids=teacher)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_bf16.embed_prompt(ids_t, torch.from_numpy(tmask))
    assert np.array_equal(emb.cpu().numpy(), generate_np.embed_prompt(esd, ids, tmask))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    outs = {}
    for chunk in (None, 192):
        out = list(gpt_bf16.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, n, 0, (*procs, *warpers), return_hidden=True,
                                     manual_seed=1, teacher_ids=torch.from_numpy(teacher), prefill_chunk=chunk))[-1]
        outs[chunk] = [h.cpu().numpy() for h in out.hiddens]
        worst = max(float((np.abs(g - r).max(1) / np.abs(r).max(1)).max()) for g, r in zip(outs[chunk], ref.hiddens))
        print(f"long audio prompt (T={T}), prefill_chunk={chunk}: worst hidden rel err vs oracle {worst:.3e}")
        assert worst < 1.5e-2, worst
    assert max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(outs[None], outs[192])) < 1e-2


def test_codec_lds_dma_path_equals_tile_path(weights, monkeypatch):
    """from 12288 frames the ConvNeXt point-wise layers run on pre-split fragment-order planes staged by LDS-DMA
    (csrc/codec_gemm.hip; the depthwise-conv + LayerNorm kernel and the GELU epilogue write the planes); below that, and
    with CTTS_X3P_MIN_ROWS=0, on the register-staged tiles.  Same products, same accumulation order over k: the waveforms
    of a 16 x 400-token batch (12800 frames, ragged rows) agree to 1e-6 RMS -- and with the numpy oracle on a slice"""
    rs = np.random.RandomState(33)
    rows = [torch.from_numpy(rs.standard_normal((n, 768)).astype(np.float32)) for n in [400, 390, 120, 400] + [300] * 12]
    new = E.CodecEngine(weights["decoder"], weights["vocos"], DEV)
    w_new = new.decode_to_wavs(rows).cpu().numpy()
    monkeypatch.setenv("CTTS_X3P_MIN_ROWS", "0")
    old = E.CodecEngine(weights["decoder"], weights["vocos"], DEV)
    w_old = old.decode_to_wavs(rows).cpu().numpy()
    assert w_new.shape == w_old.shape == (16, 256 * 799) and np.isfinite(w_new).all()
    rms = float(np.sqrt(np.mean((w_new - w_old) ** 2)))
    print(f"codec LDS-DMA path vs tile path: wav rms diff {rms:.2e} (signal rms {float(np.sqrt(np.mean(w_old ** 2))):.2e})")
    assert rms < 1e-6, rms
    dsd = {k: v.numpy() for k, v in weights["decoder"].items()}
    vsd = {k: v.numpy() for k, v in weights["vocos"].items()}
    ref = codec_np.decode_to_wavs(dsd, vsd, [rows[2].numpy()])      # a 120-token row alone: its first 100 tokens do not see the padding
    n = 256 * (2 * 100 - 1) - 256 * 110
    assert float(np.sqrt(np.mean((w_new[2, :n] - ref[0, :n]) ** 2))) < 1e-4


def test_codec_f16_mode_holds_the_waveform_bar(weights):
    """gemm="f16" (the perf mode's acoustic decoder): from 1024 frames (12288 until round 4) the ConvNeXt point-wise pairs take ONE fp16 MFMA per product
    (csrc/codec_gemm.hip: gemm_h1p_k; planes written by the depthwise-conv + LayerNorm kernel and the GELU epilogue).  Stated
    bounds, against the split-bf16 decoder (itself 4e-7 from the float32 oracle) on a 16 x 400-token ragged batch: mel within
    2e-3 of its peak, waveform within 2e-5 RMS -- a fifth of the north-star's 1e-4 -- and within 1e-4 RMS of the numpy oracle on
    a row slice.  Below 1024 frames the mode runs the split-bf16 tiles, i.e. equals gemm="bf16x3"."""
    rs = np.random.RandomState(33)
    rows = [torch.from_numpy(rs.standard_normal((n, 768)).astype(np.float32)) for n in [400, 390, 120, 400] + [300] * 12]
    ref_eng = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    f16_eng = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f16")
    Tmax = 400
    batch = torch.zeros((16, Tmax, 768))
    for i, r in enumerate(rows):
        batch[i, : r.shape[0]] = r
    mel_ref = ref_eng.dvae_decode(batch).cpu().numpy()
    mel_f16 = f16_eng.dvae_decode(batch).cpu().numpy()
    merr = float(np.abs(mel_f16 - mel_ref).max() / np.abs(mel_ref).max())
    w_ref = ref_eng.decode_to_wavs(rows).cpu().numpy()
    w_f16 = f16_eng.decode_to_wavs(rows).cpu().numpy()
    assert w_f16.shape == w_ref.shape == (16, 256 * 799) and np.isfinite(w_f16).all()
    rms = float(np.sqrt(np.mean((w_f16 - w_ref) ** 2)))
    print(f"codec f16 vs bf16x3: mel max err / peak {merr:.2e}, wav rms diff {rms:.2e} (signal rms {float(np.sqrt(np.mean(w_ref ** 2))):.2e})")
    assert rms > 0.0          # the fp16 kernels really ran
    assert merr < 2e-3, merr
    assert rms < 2e-5, rms
    dsd = {k: v.numpy() for k, v in weights["decoder"].items()}
    vsd = {k: v.numpy() for k, v in weights["vocos"].items()}
    ref = codec_np.decode_to_wavs(dsd, vsd, [rows[2].numpy()])
    n = 256 * (2 * 100 - 1) - 256 * 110
    assert float(np.sqrt(np.mean((w_f16[2, :n] - ref[0, :n]) ** 2))) < 1e-4
    small = [r[:40] for r in rows[:4]]               # 320 frames: below the threshold the mode IS the split-bf16 decoder
    assert torch.equal(f16_eng.decode_to_wavs(small), ref_eng.decode_to_wavs(small))
    # ... so in this mode an utterance's waveform depends on the size of the batch it was decoded in: pinned across the
    # threshold -- row 2 alone (240 frames: split-bf16 tiles) against row 2 inside the 16-row batch (12800 frames: fp16 planes)
    alone = f16_eng.decode_to_wavs([rows[2]]).cpu().numpy()[0]
    n2 = 256 * (2 * 120 - 1) - 256 * 110            # clear of the zero-padded tail's edge effects
    assert float(np.sqrt(np.mean((alone[:n2] - w_f16[2, :n2]) ** 2))) < 2e-5


@pytest.mark.parametrize("tmax", [400, 399])
@pytest.mark.parametrize("gemm", ["bf16x3", "f16"])
def test_codec_dwconv_transposed_plane_writes_are_bit_identical(weights, monkeypatch, gemm, tmax):
    """round 6: from 12288 frames the depthwise-conv + LayerNorm kernel hands the GEMMs their operand planes through a wave-private LDS
    transpose -- 64 contiguous bytes per lane quad instead of 64 isolated 16-byte stores per row (csrc/codec.hip dwconv_ln_seq_k: consecutive
    frames per wave at both dilations; PMC: 415 / 231 MB written per launch for 134 MB of planes before) -- same arithmetic per frame: the
    waveforms of a ragged 16 x 400-token batch (12800 frames; DVAE dilation 2 and Vocos dilation 1; the last run of every utterance partial)
    equal CTTS_DWCONV_SEQ=0's bit for bit, in both operand formats; 399 tokens = 798 frames: the last group of four rows of every utterance is
    half full (the partial flush)."""
    rs = np.random.RandomState(35)
    rows = [torch.from_numpy(rs.standard_normal((n, 768)).astype(np.float32)) for n in [tmax, 390, 120, 397] + [300] * 12]
    eng = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    w_def = eng.decode_to_wavs(rows).cpu().numpy()              # default: the transposed writes at dilation 1 (Vocos)
    monkeypatch.setenv("CTTS_DWCONV_SEQ", "2")                  # ... and at dilation 2 (DVAE decoder)
    w_new = eng.decode_to_wavs(rows).cpu().numpy()
    monkeypatch.setenv("CTTS_DWCONV_SEQ", "0")
    w_old = eng.decode_to_wavs(rows).cpu().numpy()
    assert w_new.shape == w_old.shape == (16, 256 * (2 * tmax - 1)) and np.isfinite(w_new).all()
    assert np.array_equal(w_new.view(np.int32), w_old.view(np.int32)), float(np.abs(w_new - w_old).max())
    assert np.array_equal(w_def.view(np.int32), w_old.view(np.int32)), float(np.abs(w_def - w_old).max())


def test_codec_fused_mlp_switch_is_bit_identical(weights, monkeypatch):
    """CTTS_MLP_FUSED=1 (round 6: every ConvNeXt MLP of the gemm="f16" decoder in ONE launch, csrc/codec_gemm.hip mlp_fused_h1p_k; off by
    default -- measured no faster) through the whole acoustic decoder: the waveforms of a ragged 16 x 400-token batch (12800 frames: whole and
    ragged 128-row tiles, both widths 1536 / 2048) equal the default path's bit for bit."""
    rs = np.random.RandomState(34)
    rows = [torch.from_numpy(rs.standard_normal((n, 768)).astype(np.float32)) for n in [400, 390, 120, 400] + [300] * 12]
    eng = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f16")
    w_two = eng.decode_to_wavs(rows).cpu().numpy()
    monkeypatch.setenv("CTTS_MLP_FUSED", "1")
    w_one = eng.decode_to_wavs(rows).cpu().numpy()
    assert w_one.shape == w_two.shape == (16, 256 * 799) and np.isfinite(w_one).all()
    assert np.array_equal(w_one.view(np.int32), w_two.view(np.int32)), float(np.abs(w_one - w_two).max())


def test_codec_f16_mode_threshold_straddle(weights, golden):
    """gemm="f16" on both sides of the frame count from which the point-wise pairs take the fp16 kernels (ctts_codec.x3p_min_rows = 1024;
    ADVICE r4): 8 utterances x 64 tokens = 1024 frames run gemm_h1p_k, 8 x 63 = 1008 frames run the split-bf16 tiles -- i.e. equal
    gemm="bf16x3" bit for bit -- and the fp16 side stays within the mode's stated 2e-5 RMS of the f32-class decoder; a STREAMED window
    (decode_window: 8 x 55 tokens = 880 frames, below the threshold) of a batch whose full decode is above it (8 x 100 = 1600 frames)
    differs from the slice of the full decode by the same bound.  Inputs: the reference GPT's own hidden states (c2.hid0)."""
    hid0 = torch.from_numpy(golden["generate_big"]["c2.hid0"])
    f16 = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f16")
    ref = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    rows64 = [hid0[40 * i: 40 * i + 64].clone() for i in range(8)]
    rows63 = [r[:63] for r in rows64]
    w63_f, w63_r = f16.decode_to_wavs(rows63), ref.decode_to_wavs(rows63)
    assert torch.equal(w63_f, w63_r)                                          # 1008 frames: the mode IS the split-bf16 decoder
    w64_f, w64_r = f16.decode_to_wavs(rows64).cpu().numpy(), ref.decode_to_wavs(rows64).cpu().numpy()
    rms = float(np.sqrt(np.mean((w64_f - w64_r) ** 2)))
    assert 0.0 < rms < 2e-5, rms                                              # 1024 frames: the fp16 kernels ran, within the stated bound
    rows100 = [hid0[30 * i: 30 * i + 100].clone() for i in range(8)]
    full = f16.decode_to_wavs(rows100).cpu().numpy()                          # 1600 frames: fp16 path
    n = 256 * 4                                                               # halo 102 frames -> a 55-token window = 880 frames < 1024
    win = f16.decode_window(rows100, 0, n).cpu().numpy()                      # its first samples from that window: split-bf16 path
    d = float(np.sqrt(np.mean((win - full[:, :n]) ** 2)))
    print(f"codec f16 threshold: 1024 frames vs bf16x3 {rms:.2e} RMS; streamed window (tiles) vs full decode (fp16) {d:.2e} RMS")
    assert d < 2e-5, d


def test_decode_window_vs_the_reference_decode(codec, golden):
    """streamed windows against the REFERENCE's decode of the whole utterance (codec_big.npz `c2size`: the reference's DVAE class + the vocos
    restatement on the reference GPT's own 512 hidden states; the golden keeps every 16th waveform sample): windows at the start, in the
    interior (token window + halos only: 12000 samples need ~126 of the 512 tokens), and at the end -- each within the 1e-4 RMS bar of the
    samples the reference produced for that range"""
    Gd = golden["codec_big"]
    hid, _ = cases.codec_big_inputs(cases.CODEC_BIG_CASES["c2size"], golden["generate_big"]["c2.hid0"])
    rows = [torch.from_numpy(hid[0]).to(DEV)]
    ref_s = Gd["c2size.wav_s"][0]                  # samples 0, 16, 32, ... of row 0
    total = 256 * (2 * 512 - 1)
    st = cases.CODEC_BIG_WAV_STRIDE
    for lo, hi in [(0, 12000), (12000, 24000), (100000, 112000), (200000, 212000), (131072, 131072 + 500), (total - 9000, total)]:
        got = codec.decode_window(rows, lo, hi).cpu().numpy()[0]
        assert got.shape == (hi - lo,)
        p = np.arange((lo + st - 1) // st * st, hi, st)
        p = p[p // st < ref_s.shape[0]]
        err = got[p - lo] - ref_s[p // st]
        assert float(np.sqrt(np.mean(err ** 2))) < 1e-4, (lo, hi, float(np.sqrt(np.mean(err ** 2))))


def test_decode_window_equals_slices_of_the_full_decode(codec):
    """`CodecEngine.decode_window` (what streaming emits): any sample range of the batch decode, computed from the token
    window it depends on (+ halos) -- interior ranges, ranges touching either end, ragged rows shorter than the window"""
    rs = np.random.RandomState(12)
    rows = [torch.from_numpy(rs.standard_normal((n, 768)).astype(np.float32)).to(DEV) for n in (300, 170, 260, 40)]
    full = codec.decode_to_wavs(rows).cpu().numpy()
    total = full.shape[1]
    assert total == 256 * (2 * 300 - 1)
    for lo, hi in [(0, 12000), (12000, 24000), (60000, 72000), (100000, 100001), (total - 9000, total), (0, total), (total, total + 5)]:
        got = codec.decode_window(rows, lo, hi).cpu().numpy()
        want = full[:, lo: min(hi, total)]
        assert got.shape == want.shape, (lo, hi, got.shape, want.shape)
        if want.size:
            assert float(np.sqrt(np.mean((got - want) ** 2))) < 2e-6, (lo, hi)
            assert np.abs(got - want).max() < 1e-4


@pytest.mark.parametrize("chunk", [5, 16])
def test_chunked_prefill_bit_exact(gpt_f32, golden, chunk):
    """the prompt prefilled in pieces (`ctts_gpt_prefill_chunk`: keys of earlier pieces come from the KV cache, only the last
    piece samples) produces the reference's golden ids like the one-shot prefill -- mixed-length left-padded batch b8"""
    c = cases.GEN_CASES["b8"]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])
    out = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, c["max_new"], c["min_new"], (*procs, *warpers),
                                return_hidden=True, manual_seed=c["manual_seed"], prefill_chunk=chunk))[-1]
    got = np.concatenate([t.cpu().numpy() for t in out.ids], 0)
    assert np.array_equal(np.array([int(t.shape[0]) for t in out.ids]), golden["generate"]["b8.lens"])
    assert np.array_equal(got, golden["generate"]["b8.ids"])
    for b in c["keep_hidden_rows"]:
        assert np.abs(out.hiddens[b].cpu().numpy() - golden["generate"][f"b8.hid{b}"]).max() < 2e-4


def test_full_size_properties(gpt_bf16, codec):
    """BASELINE-size batch (B=64, mixed lengths): size-independent properties -- forced lengths are
    honoured exactly, every id is in range, EOS never appears inside a row, the waveform is finite and
    a row's audio does not depend on which other rows share the batch (batch invariance of a shard)."""
    B = 64
    ids, mask, tmask = synth.make_prompts(B, 16, 48, seed=0)
    stop = synth.make_stop_lengths(B, 16, 48, seed=0)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    emb = gpt_bf16.embed_prompt(ids_t, torch.from_numpy(tmask))
    out = list(gpt_bf16.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, 64, 0, (*procs, *warpers), return_hidden=True,
                                 manual_seed=42, stop_at=torch.from_numpy(stop)))[-1]
    assert [int(t.shape[0]) for t in out.ids] == stop.tolist()
    allids = torch.cat(out.ids, 0)
    assert int(allids.min()) >= 0 and int(allids.max()) < 625
    wav = codec.decode_to_wavs(out.hiddens)
    assert torch.isfinite(wav).all() and wav.shape == (B, 256 * (2 * int(stop.max()) - 1))
    # batch invariance: rows 8..15 alone (same global row numbering) give the same tokens
    sl = slice(8, 16)
    emb2 = gpt_bf16.embed_prompt(ids_t[sl], torch.from_numpy(tmask[sl]))
    out2 = list(gpt_bf16.generate(emb2, ids_t[sl], torch.tensor([0.3] * 4), 625, mask_t[sl], 64, 0, (*procs, *warpers),
                                  return_hidden=True, manual_seed=42, stop_at=torch.from_numpy(stop[sl]), row_offset=32,
                                  total_rows=B * 4))[-1]
    same = sum(int(torch.equal(out.ids[8 + i], out2.ids[i])) for i in range(8))
    assert same == 8, same


def test_chat_facade_stream_and_batch(weights):
    """`Chat.infer_ids` / `infer_ids_stream` (mirrors of core.py:469-503): chunk schedule and shapes"""
    from chattts_amd.core import Chat, InferCodeParams
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="bf16") and chat.has_loaded()
    ids, mask, tmask = synth.make_prompts(4, 8, 12, seed=3)
    stop = torch.tensor([100, 60, 30, 100], dtype=torch.int32)
    p = InferCodeParams(max_new_token=128, manual_seed=5, show_tqdm=False)
    args = (torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask), p)
    wav = chat.infer_ids(*args, stop_at=stop)
    assert wav.dtype == np.float32 and wav.shape == (4, 256 * (2 * 100 - 1)) and np.isfinite(wav).all()
    chunks = list(chat.infer_ids_stream(*args, stop_at=stop))
    # generator yields at 24, 48, 72, 96 tokens + the final result: the first two are dropped
    # (pass_first_n_batches=2), each later one emits the next 12000 samples (stream_speed), then the remainder
    # with silent columns removed (core.py:488-503)
    assert [c.shape[1] for c in chunks[:3]] == [12000, 12000, 12000]
    assert len(chunks) == 4 and chunks[3].shape[1] <= wav.shape[1] - 36000
    assert all(c.shape[0] == 4 and np.isfinite(c).all() for c in chunks)
    # Chat.infer-level post-processing: silence strip per row, concatenation with split_text (core.py:258-270)
    rows = chat.infer_tokens(*args, stop_at=stop)
    assert len(rows) == 4 and all(r.ndim == 1 and (np.abs(r) > 1e-5).all() for r in rows)
    one = chat.infer_tokens(*args, split_text=True, max_split_batch=2, stop_at=stop)
    assert len(one) == 1 and one[0].ndim == 1 and one[0].size > 0
    chat.interrupt()
    out = list(chat.infer_code(*args[:3], p, stop_at=stop))  # interrupted before the first poll completes a chunk
    assert len(out) == 1 and max(int(t.shape[0]) for t in out[0].ids) <= 16
    chat.unload()
    assert not chat.has_loaded()


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", list(cases.TEXT_CASES))
def test_refine_text_mode_bit_exact(gpt_f32, golden, name, use_graph):
    """infer_text=True: text embedding, 21178-way head, block-wide sampling kernel; token ids
    bit-exact vs the reference run (tests/golden/text.npz)"""
    c = cases.TEXT_CASES[name]
    Gd = golden["text"]
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(21178, c["top_P"], c["top_K"], c["rep"])
    out = list(gpt_f32.generate(emb, ids_t, torch.tensor(c["temperature"]), cases.TEXT_EOS, mask_t, c["max_new"], c["min_new"],
                                (*procs, *warpers), infer_text=True, return_hidden=True, manual_seed=c["manual_seed"],
                                use_graph=use_graph))[-1]
    assert all(t.dim() == 1 for t in out.ids)
    assert np.array_equal(np.array([int(t.shape[0]) for t in out.ids]), Gd[name + ".lens"])
    assert np.array_equal(np.concatenate([t.cpu().numpy() for t in out.ids]), Gd[name + ".ids"])
    for b in c["keep_hidden_rows"]:
        assert np.abs(out.hiddens[b].cpu().numpy() - Gd[name + f".hid{b}"]).max() < 2e-4


def test_text_and_code_calls_keep_a_session_each(weights, golden):
    """The default `Chat.infer` (core.py:341-360) alternates a refine-text call and a code call per request: each mode has a session slot
    and decode-graph handles of its own, so the second request finds BOTH from the first (no reallocation, no graph re-capture), and the
    results are what a fresh engine gives."""
    eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32x3")
    name = list(cases.TEXT_CASES)[0]
    ct, cc = cases.TEXT_CASES[name], cases.BIG_CASES["c3w"]

    def text_call():
        ids, mask, tmask = cases.gen_inputs(ct)
        ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
        warpers, procs = E.gen_logits(21178, ct["top_P"], ct["top_K"], ct["rep"])
        out = list(eng.generate(eng.embed_prompt(ids_t, torch.from_numpy(tmask)), ids_t, torch.tensor(ct["temperature"]), cases.TEXT_EOS, mask_t,
                                ct["max_new"], ct["min_new"], (*procs, *warpers), infer_text=True, manual_seed=ct["manual_seed"]))[-1]
        return np.concatenate([t.cpu().numpy() for t in out.ids])

    def code_call():
        out, _ = run_case(eng, cc, use_graph=True)
        return np.concatenate([t.cpu().numpy().reshape(-1) for t in out[-1].ids])

    t0, c0 = text_call(), code_call()
    st, sc = eng._session_text, eng._session
    assert st is not None and sc is not None and st is not sc and st["graph"] and sc["graph"]
    assert {id(ln.handle) for ln in st["lanes"]}.isdisjoint({id(ln.handle) for ln in sc["lanes"]})
    t1, c1 = text_call(), code_call()
    assert eng._session_text is st and eng._session is sc
    assert np.array_equal(t0, t1) and np.array_equal(c0, c1)
    assert np.array_equal(t0, golden["text"][name + ".ids"])


def test_refine_text_facade_and_rejections(weights):
    from chattts_amd.core import Chat, RefineTextParams
    chat = Chat()
    chat.load(state_dicts=weights, device=DEV, dtype="bf16")
    ids, mask, tmask = synth.make_prompts(5, 6, 14, seed=8)
    a = (torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask))
    out = chat.refine_text_ids(*a, cases.TEXT_EOS, RefineTextParams(max_new_token=20, manual_seed=1, show_tqdm=False),
                               stop_at=torch.tensor([3, 20, 7, 1, 12], dtype=torch.int32))
    assert [int(t.shape[0]) for t in out.ids] == [3, 20, 7, 1, 12]
    assert all(int(t.max()) < 21178 and int(t.min()) >= 0 and (t != cases.TEXT_EOS).all() for t in out.ids)
    with pytest.raises(NotImplementedError):   # the reference's penalty processor mis-broadcasts in text mode
        chat.refine_text_ids(*a, cases.TEXT_EOS, RefineTextParams(repetition_penalty=1.2, max_new_token=4, manual_seed=1))


def test_long_context_prefix_consistency(gpt_bf16):
    """2000 decode steps (context > 2000 keys, KV cache near max_position_embeddings): the run is finite, honours the
    forced lengths, and -- generation being causal -- its first 150 tokens equal those of a 160-step run."""
    ids, mask, tmask = synth.make_prompts(3, 20, 40, seed=11)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    emb = gpt_bf16.embed_prompt(ids_t, torch.from_numpy(tmask))

    def run(max_new, stop):
        return list(gpt_bf16.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, max_new, 0, (*procs, *warpers), return_hidden=True,
                                      manual_seed=9, stop_at=torch.tensor(stop, dtype=torch.int32)))[-1]
    long = run(2001, [2000, 700, 1500])
    short = run(161, [160, 160, 160])
    assert [int(t.shape[0]) for t in long.ids] == [2000, 700, 1500]
    for b in range(3):
        assert torch.equal(long.ids[b][:150], short.ids[b][:150])
        assert torch.isfinite(long.hiddens[b]).all()
    with pytest.raises(ValueError):   # T + max_new_token beyond the RoPE table / max_position_embeddings (config.py:57)
        run(4096, [10, 10, 10])


def test_continuous_batching_equals_isolated_generation(gpt_f32):
    """SlotPool: 9 requests through 4 slots, admitted as slots free up; every request's tokens are
    bit-identical to generating it alone at its pool row (row_offset = 4*slot, total_rows = 4*slots), whatever group it
    was left-padded into and whatever ran beside it."""
    from chattts_amd.serving import SlotPool
    S = 4
    pool = SlotPool(gpt_f32, slots=S, cap=160, hid_cap=64, manual_seed=21)
    rs = np.random.RandomState(6)
    reqs = {}
    lens = [5, 40, 17, 33, 9, 21, 3, 48, 12]
    for i, n in enumerate(lens):
        T = int(rs.randint(6, 30))
        ids = np.repeat(rs.randint(1, 21178, size=(T, 1)), 4, axis=1).astype(np.int64)
        reqs[i] = (ids, n)
        pool.submit(i, ids, max_new_token=48, stop_at=n)
    got = {rid: (ids.cpu().numpy(), hid.cpu().numpy()) for rid, ids, hid in pool.run()}
    assert sorted(got) == list(range(len(lens)))
    assert len(set(pool.slot_of.values())) <= S and not pool.active and len(pool.free) == S
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    for rid, (ids, n) in reqs.items():
        assert got[rid][0].shape == (n, 4), (rid, got[rid][0].shape)
        ids_t = torch.from_numpy(ids)[None]
        emb = gpt_f32.embed_prompt(ids_t, torch.ones((1, ids.shape[0]), dtype=torch.bool))
        ref = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, None, 64, 0, (*procs, *warpers), return_hidden=True,
                                    manual_seed=21, stop_at=torch.tensor([n], dtype=torch.int32), row_offset=4 * pool.slot_of[rid],
                                    total_rows=4 * S))[-1]
        assert np.array_equal(got[rid][0], ref.ids[0].cpu().numpy()), rid
        assert np.abs(got[rid][1] - ref.hiddens[0].cpu().numpy()).max() < 1e-5, rid
    pool.close()


def test_unseeded_leaves_global_generator_where_the_reference_would(gpt_f32, golden):
    """manual_seed=None: the host draws run ahead of the GPU in a worker thread, but afterwards torch's global CPU
    generator must sit exactly after one [rows, 626] draw per executed step, like the reference's (gpt.py:498-500)"""
    c = cases.GEN_CASES["unseeded"]
    outs, _ = run_case(gpt_f32, c, use_graph=True)
    after = torch.rand(3)
    torch.manual_seed(c["global_seed"])
    steps = int(max(t.shape[0] for t in outs[0].ids))     # never finished: max_new_token steps were executed
    for _ in range(steps):
        torch.empty(2 * 4, 626).exponential_(1)
    assert torch.equal(after, torch.rand(3))


def test_unseeded_stream_batch_not_aligned_to_the_draw_ring(gpt_f32, weights):
    """manual_seed=None with stream=True and stream_batch=50 (neither a divisor nor a multiple of the 32-step blocks the
    Exp(1) ring is uploaded in): every step must still consume ITS draw of torch's global CPU stream, like the reference
    (gpt.py:498-500) -- the chunks are enqueued in pieces that never straddle a ring block."""
    from chattts_amd import rng
    ids, mask, tmask = synth.make_prompts(2, 10, 14, seed=2)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    n = 130
    torch.manual_seed(7)
    outs = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3, 0.5, 0.7, 1.0]), 625, mask_t, n, n, (*procs, *warpers), return_hidden=True,
                                 stream=True, stream_batch=50, manual_seed=None))
    assert [int(o.ids[0].shape[0]) for o in outs] == [50, 100, 130]
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    torch.manual_seed(7)
    draws = rng.ExpDraws(2 * 4, 626, None)
    ref = generate_np.generate(llama, esd, generate_np.fold_heads(esd), generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                               temperature=np.array([0.3, 0.5, 0.7, 1.0], np.float32), draw_q=lambda i: draws.step(i).numpy(),
                               pow_table=rng.penalty_table(1.05).numpy(), max_new_token=n, min_new_token=n)
    for b in range(2):
        assert np.array_equal(outs[-1].ids[b].cpu().numpy(), ref.ids[b]), b


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_chat_infer_text_level_matches_oracle(weights, dtype):
    """`Chat.infer(text, ...)` (core.py:208-270) end to end in both parity modes: normalise -> decorate -> tokenise ->
    embed -> speaker vector at [spk_emb] -> generate, and the refine-text leg; token ids and refined strings equal the
    numpy oracle driven by the same host front end (the front end itself is pinned in tests/test_frontend.py)."""
    import os
    from chattts_amd import frontend as F, rng
    from chattts_amd.core import Chat
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(gold, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype=dtype, tokenizer=os.path.join(gold, "tokenizer"), spk_stat=spk_stat)
    tok = chat.tokenizer
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    texts = ["What is [uv_break]your favorite english food?[laugh][lbreak]", "hello world"]
    p = Chat.InferCodeParams(spk_emb=spk, max_new_token=20, manual_seed=7, show_tqdm=False)
    normed = [chat.normalizer(t, True, True, None) for t in texts]
    assert normed[0] == "What is [uv_break]your favorite english food[laugh][lbreak]"   # '?' is outside the model's alphabet
    out = next(chat._infer_code(list(normed), False, DEV, True, p))
    wavs = chat.infer(list(texts), skip_refine_text=True, split_text=False, params_infer_code=p)
    full = chat.decode_to_wavs(out.hiddens)
    assert len(wavs) == 2 and all(np.array_equal(w, r[np.abs(r) > 1e-5]) for w, r in zip(wavs, full))
    sharded = chat.infer_sharded(list(texts), params_infer_code=p)        # no process group: the unsharded call
    assert len(sharded) == 2 and all(np.array_equal(a, b) for a, b in zip(sharded, wavs))

    # oracle leg: same normaliser + decoration + tokenizer, numpy embedding with the unit speaker vector substituted
    ids, mask, tmask = tok.encode(F.Speaker.decorate_code_prompts(normed, p.prompt, None, spk), 4)
    ids, mask, tmask = ids.numpy(), mask.numpy(), tmask.numpy()
    assert (ids[..., 0] == tok.spk_emb_ids).sum() == 2
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    emb = generate_np.embed_prompt(esd, ids, tmask)
    unit = torch.nn.functional.normalize(torch.from_numpy(F.Speaker.decode_vector(spk)), p=2.0, dim=0, eps=1e-12).float().numpy()
    emb[ids[..., 0] == tok.spk_emb_ids] = unit
    draws = rng.ExpDraws(2 * 4, 626, 7)
    ref = generate_np.generate(llama, esd, generate_np.fold_heads(esd), emb, ids, mask, temperature=np.array([0.3] * 4, np.float32),
                               draw_q=lambda i: draws.step(i).numpy(), pow_table=rng.penalty_table(1.05).numpy(), max_new_token=20)
    for b in range(2):
        assert np.array_equal(out.ids[b].cpu().numpy(), ref.ids[b])
        assert np.abs(out.hiddens[b].cpu().numpy() - ref.hiddens[b]).max() < 2e-4

    # refine-text leg (the shape of /root/reference/tests/#655.py:34-48): strings out
    rp = Chat.RefineTextParams(prompt="[oral_2][laugh_0][break_6]", manual_seed=12345, max_new_token=10, show_tqdm=False)
    refined = chat.infer(list(texts), refine_text_only=True, split_text=False, params_refine_text=rp)
    ids, mask, tmask = tok.encode(F.Speaker.decorate_text_prompts(normed, rp.prompt), 4)
    ids, mask, tmask = ids.numpy(), mask.numpy(), tmask.numpy()
    draws = rng.ExpDraws(2, 21178, 12345)
    rt = generate_np.generate(llama, esd, generate_np.fold_head_text(esd), generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                              temperature=np.array([0.7], np.float32), draw_q=lambda i: draws.step(i).numpy(), pow_table=None,
                              max_new_token=10, eos=tok.eos_token, infer_text=True)
    want = tok.decode([torch.from_numpy(r)[torch.from_numpy(r) < tok.break_0_ids] for r in rt.ids])
    assert isinstance(refined, list) and refined == want
    joined = chat.infer("hello world\nthe time of day", refine_text_only=True, split_text=True, params_refine_text=rp)
    assert isinstance(joined, str) and joined.count("\n") == 1
    with pytest.raises(RuntimeError):      # several sentences need the full DVAE for the speaker prompt (tests/test_gpu_dvae.py)
        chat.infer(list(texts), skip_refine_text=True, split_text=True, params_infer_code=Chat.InferCodeParams(max_new_token=4, manual_seed=1))
    with pytest.raises(AssertionError):    # has_loaded(use_decoder=False) is False without it (core.py:404)
        chat.infer(texts[0], skip_refine_text=True, split_text=False, use_decoder=False)


def test_chat_infer_stream_text_level_equals_token_level(weights):
    """`Chat.infer(..., stream=True)` (core.py:455-503 through the text front end) yields exactly the chunks of the
    token-level `infer_ids_stream` for the same prompts, and the non-stream result is their source waveform."""
    import os
    from chattts_amd import frontend as F
    from chattts_amd.core import Chat
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    chat = Chat()
    chat.load(state_dicts=weights, device=DEV, dtype="bf16", tokenizer=os.path.join(gold, "tokenizer"))
    texts = ["hello world the time of day", "chat tts test string"]
    mk = lambda: Chat.InferCodeParams(max_new_token=100, manual_seed=9, show_tqdm=False, stream_speed=6000)
    chunks = list(chat.infer(list(texts), stream=True, skip_refine_text=True, split_text=False, params_infer_code=mk()))
    ids, mask, tmask = chat.tokenizer.encode(F.Speaker.decorate_code_prompts(list(texts), "[speed_5]", None, None), 4)
    want = list(chat.infer_ids_stream(ids, mask, tmask, mk()))
    assert len(chunks) == len(want) >= 2
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(chunks, want))
    assert all(c.shape[1] == 6000 for c in chunks[:-1])
    whole = chat.infer(list(texts), skip_refine_text=True, split_text=False, params_infer_code=mk())
    full = chat.infer_ids(ids, mask, tmask, mk())
    assert all(np.array_equal(w, r[np.abs(r) > 1e-5]) for w, r in zip(whole, full))


def test_session_reuse_has_no_stale_state(gpt_f32, weights):
    """Two calls of identical geometry and sampling constants share device buffers and the captured graph (session
    reuse): the second call, with different prompts / padding / forced lengths, must equal the oracle exactly as if it
    ran on a fresh engine, and the first call's returned tensors must not change under it."""
    from chattts_amd import rng
    llama = llama_np.LlamaWeights({k: v.numpy() for k, v in weights["gpt"].items()})
    esd = {k: v.numpy() for k, v in weights["embed"].items()}
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    kept = None
    for seed, stop in ((21, [6, 11, 3]), (22, [9, 2, 12])):
        ids, mask, tmask = synth.make_prompts(3, 12, 12, seed=seed)     # same T for both calls
        if seed == 22:
            mask[1, :4] = 0                                               # different left padding the second time
            ids[1, :4] = 0
            tmask[1, :4] = False
        stop = np.array(stop, np.int32)
        ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
        emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
        out = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, 16, 0, (*procs, *warpers), return_hidden=True,
                                    manual_seed=5, stop_at=torch.from_numpy(stop)))[-1]
        draws = rng.ExpDraws(3 * 4, 626, 5)
        ref = generate_np.generate(llama, esd, generate_np.fold_heads(esd), generate_np.embed_prompt(esd, ids, tmask), ids, mask,
                                   temperature=np.array([0.3] * 4, np.float32), draw_q=lambda i: draws.step(i).numpy(),
                                   pow_table=rng.penalty_table(1.05).numpy(), max_new_token=16, stop_at=stop)
        for b in range(3):
            assert np.array_equal(out.ids[b].cpu().numpy(), ref.ids[b]), (seed, b)
            assert np.abs(out.hiddens[b].cpu().numpy() - ref.hiddens[b]).max() < 2e-4
        if kept is None:
            kept = (out, [t.clone() for t in out.ids], [t.clone() for t in out.hiddens])
    first, ids0, hid0 = kept
    assert all(torch.equal(a, b) for a, b in zip(first.ids, ids0)) and all(torch.equal(a, b) for a, b in zip(first.hiddens, hid0))
    assert gpt_f32._session is not None and gpt_f32._session["graph"]


def test_bf16_parity_on_the_bench_workload(gpt_bf16, gpt_f32, weights):
    """Parity evidence for the configuration bench.py's `value` is quoted in (bf16, C3: 64 utterances, 513 steps, contexts to 560
    keys): both engines are TEACHER-FORCED on the reference's own token stream of this workload (tests/golden/bench_c3.npz, all
    64 rows, all steps); the f32 engine is the pinned one (its free run IS that stream, `test_bench_workload_f32_equals_...`).
    Bounds at every step of every row: relative hidden error, |delta logit| through the folded heads, no growth from the first to
    the last quarter of a row, and the teacher-forced token agreement rate -- the fraction of (row, step, codebook) where the bf16
    sampler's own draw under the same Exp(1) tensor is the reference's token (SURVEY 7 hard parts (iv); gpt.py:497-508: free
    running, one flipped argmax diverges the suffix, which is why agreement is measured under the reference's history).
    The numbers bench.py prints as `bf16_parity` come from the same functions."""
    import os
    import bench
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_c3.npz"))
    wl = bench.shard_workload(64, 1, 0, 128, 512)
    max_new = int(wl["stop_all"].max()) + 1
    lens, rows, teacher = bench.teacher_from_golden(gold, max_new)
    ids_t, mask_t = torch.from_numpy(wl["ids"]), torch.from_numpy(wl["mask"])
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)

    def forced(eng):
        emb = eng.embed_prompt(ids_t, torch.from_numpy(wl["tmask"]))
        out = list(eng.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, max_new, 0, (*procs, *warpers), return_hidden=True,
                                manual_seed=42, stop_at=torch.from_numpy(wl["stop"]), teacher_ids=torch.from_numpy(teacher),
                                return_sampled=True))[-1]
        for b in range(64):
            assert np.array_equal(out.ids[b].cpu().numpy(), rows[b]), b      # the forced stream was followed, lengths included
        return [h.cpu().numpy() for h in out.hiddens], [t.cpu().numpy() for t in eng.last_sampled]

    hid32, samp32 = forced(gpt_f32)
    # the f32 engine under teacher forcing draws the reference's tokens itself, every one of them (it is bit-exact free running)
    assert all(np.array_equal(a, b) for a, b in zip(samp32, rows))
    hid16, samp16 = forced(gpt_bf16)
    pm = bench.parity_metrics(hid16, hid32, samp16, rows, bench.generate_heads(weights["embed"]))
    print("bf16 vs f32, teacher-forced on the bench workload:", pm)
    assert pm["tokens_compared"] == 4 * int(lens.sum()) == 4 * 21438
    assert pm["worst_rel_hidden_err"] < 1.5e-2, pm
    assert pm["worst_abs_dlogit"] < 0.25, pm
    assert pm["rel_hidden_err_last_quarter"] < 2.0 * pm["rel_hidden_err_first_quarter"] + 1e-3, pm   # no growth with the step index / context
    assert pm["token_agreement"] > 0.90, pm


def test_slot_pool_with_finished_rows_kept_in_the_step(weights, monkeypatch):
    """CTTS_SKIP_FINISHED=0 (the reference's own behaviour: finished rows keep stepping, gpt.py:512-518,592) with a caller that left
    the compaction to the device (row_map = NULL, a zero-initialised n_active): nobody writes the live count then, so the step must
    not read it -- every slot steps.  (Regression: the pool span forever on *n_active == 0.)"""
    from chattts_amd.serving import SlotPool
    eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    monkeypatch.setenv("CTTS_SKIP_FINISHED", "0")
    pool = SlotPool(eng, slots=3, cap=96, hid_cap=32, manual_seed=21)     # the pool's own handle reads the variable at creation
    monkeypatch.delenv("CTTS_SKIP_FINISHED")
    rs = np.random.RandomState(3)
    reqs = {}
    for i, n in enumerate([4, 11, 7, 9]):
        T = int(rs.randint(5, 12))
        ids = np.repeat(rs.randint(1, 21178, size=(T, 1)), 4, axis=1).astype(np.int64)
        reqs[i] = (ids, n)
        pool.submit(i, ids, max_new_token=24, stop_at=n)
    got = {}
    for k, (rid, ids, hid) in enumerate(pool.run()):
        got[rid] = ids.cpu().numpy()
        assert pool.steps < 400, "the pool is not making progress"
    assert sorted(got) == [0, 1, 2, 3]
    ref_eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    for rid, (ids, n) in reqs.items():
        assert got[rid].shape == (n, 4)
        ids_t = torch.from_numpy(ids)[None]
        emb = ref_eng.embed_prompt(ids_t, torch.ones((1, ids.shape[0]), dtype=torch.bool))
        ref = list(ref_eng.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, None, 32, 0, (*procs, *warpers), return_hidden=False,
                                    manual_seed=21, stop_at=torch.tensor([n], dtype=torch.int32), row_offset=4 * pool.slot_of[rid],
                                    total_rows=12))[-1]
        assert np.array_equal(got[rid], ref.ids[0].cpu().numpy()), rid
    pool.close()


def test_compaction_order_does_not_change_results(weights, golden, monkeypatch):
    """ctts_gen_state.order (utterances visited by descending context in the device-side compaction, so the attention grid starts
    its longest units first) moves utterances between compact rows, nothing else: token ids AND hidden states of the f32 engine are
    bit-identical with CTTS_ORDER=0 (ascending slot) on the left-padded golden batch with rows finishing at different steps."""
    c = cases.BIG_CASES["c3w"]
    eng = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    a, _ = run_case(eng, c, use_graph=True)
    monkeypatch.setenv("CTTS_ORDER", "0")
    eng._session = None
    b, _ = run_case(eng, c, use_graph=True)
    for x, y in zip(a[-1].ids, b[-1].ids):
        assert torch.equal(x, y)
    for x, y in zip(a[-1].hiddens, b[-1].hiddens):
        assert torch.equal(x, y)


def test_interrupt_keeps_tokens_steps_and_outputs_consistent(gpt_f32):
    """Chat.interrupt() (core.py:272-273 -> Context, gpt.py:592) while a chunk is already enqueued behind the one being looked at
    (run-ahead): the tokens handed out, `last_stats['steps']` and the lengths all describe the same number of steps."""
    B = 3
    ids, mask, tmask = synth.make_prompts(B, 8, 12, seed=2)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    ctx = E.Context()

    class Trip(E.Context):
        """reports an interrupt from the second look on: the first look let chunk 2 be enqueued behind chunk 1 (run-ahead), the second --
        right after chunk 1 was collected -- stops the loop with chunk 2 still in flight"""
        def __init__(self):
            super().__init__()
            self.n = 0

        def get(self):
            self.n += 1
            return self.n >= 2

    out = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, 200, 200, (*procs, *warpers), return_hidden=True,
                                manual_seed=5, context=Trip()))[-1]
    steps = gpt_f32.last_stats["steps"]
    assert 1 < steps < 200
    for b in range(B):
        assert out.ids[b].shape[0] == steps == out.hiddens[b].shape[0], (b, out.ids[b].shape, steps)
    full = list(gpt_f32.generate(emb, ids_t, torch.tensor([0.3] * 4), 625, mask_t, 200, 200, (*procs, *warpers), return_hidden=False,
                                 manual_seed=5, context=ctx))[-1]
    for b in range(B):
        assert torch.equal(out.ids[b], full.ids[b][:steps])     # an interrupted run is a prefix of the uninterrupted one


def test_device_guard_path_on_any_box():
    """CttsDeviceGuard (csrc/kernels.hpp) -- what every C-ABI entry point wraps its enqueues in -- exercised through its probe on
    whatever this box has: for a stream of EVERY visible device the guard resolves the owning device, makes it current inside, says
    whether it had to switch, and restores the caller's device; the null stream changes nothing.  (The two-GPU end-to-end test below is
    skipped on a 1-GPU box; this one still runs the guard's code there.)"""
    import ctypes as C
    from chattts_amd import _lib
    lib = _lib.lib()
    cur = torch.cuda.current_device()
    for d in range(torch.cuda.device_count()):
        st = torch.cuda.Stream(device=d)
        o = [C.c_int32(-7) for _ in range(4)]
        _lib.check(lib.ctts_k_device_guard_probe(st.cuda_stream, *[C.byref(x) for x in o]), "guard probe")
        before, sdev, inside, switched = [x.value for x in o]
        assert (before, sdev, inside, switched) == (cur, d, d, int(d != cur))
        assert torch.cuda.current_device() == cur
    o = [C.c_int32(-7) for _ in range(4)]
    _lib.check(lib.ctts_k_device_guard_probe(None, *[C.byref(x) for x in o]), "guard probe (null stream)")
    assert [x.value for x in o] == [cur, -1, cur, 0]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_engines_on_a_non_current_device(weights):
    """Chat.load(device=cuda:1) without torch.cuda.set_device: every C-ABI entry point makes the device that owns the stream it was
    given current while it enqueues (CttsDeviceGuard, csrc/kernels.hpp), so engines built for a non-current device work."""
    d1 = torch.device("cuda:1")
    assert torch.cuda.current_device() == 0
    gpt = E.GptEngine(weights["gpt"], weights["embed"], d1, dtype="f32")
    cod = E.CodecEngine(weights["decoder"], weights["vocos"], d1)
    ids, mask, tmask = synth.make_prompts(2, 6, 9, seed=1)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)
    out = list(gpt.generate(gpt.embed_prompt(ids_t, torch.from_numpy(tmask)), ids_t, torch.tensor([0.3] * 4), 625, mask_t, 12, 12,
                            (*procs, *warpers), return_hidden=True, manual_seed=3))[-1]
    ref = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    out0 = list(ref.generate(ref.embed_prompt(ids_t, torch.from_numpy(tmask)), ids_t, torch.tensor([0.3] * 4), 625, mask_t, 12, 12,
                             (*procs, *warpers), return_hidden=True, manual_seed=3))[-1]
    for a, b in zip(out.ids, out0.ids):
        assert torch.equal(a.cpu(), b.cpu())
    with torch.cuda.device(d1):
        wav = cod.decode_to_wavs(out.hiddens)
    assert torch.isfinite(wav).all() and wav.device == d1
    assert torch.cuda.current_device() == 0


def test_device_generator_mode(gpt_f32, weights):
    """rng="device" (the sampling kernel draws the multinomial's Exp(1) variates itself; the reference on a GPU device uses the
    device generator too, gpt.py:39).  manual_seed=None -- the reference's default -- is repeatable under torch.manual_seed (the
    key is ONE draw from torch's global CPU generator) and differs between keys; a shard reproduces its rows of the full batch
    (counter = global row); a seeded call repeats its draw at every step like the reference's re-seeded generator; SlotPool serves
    unseeded requests and each equals its isolated generation."""
    from chattts_amd.serving import SlotPool
    B = 6
    ids, mask, tmask = synth.make_prompts(B, 8, 14, seed=9)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = gpt_f32.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(625, 0.7, 20, 1.05)

    def run(sl=slice(0, B), seed=None, **kw):
        out = list(gpt_f32.generate(emb[sl], ids_t[sl], torch.tensor([0.3] * 4), 625, mask_t[sl], 40, 40, (*procs, *warpers),
                                    return_hidden=False, manual_seed=seed, rng="device", row_offset=4 * sl.start, total_rows=4 * B, **kw))[-1]
        return [t.cpu().numpy() for t in out.ids]

    torch.manual_seed(77)
    a = run()
    state = torch.get_rng_state()
    torch.manual_seed(77)
    b = run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and torch.equal(torch.get_rng_state(), state)
    c = run()      # the global generator moved on: another key
    assert any(not np.array_equal(x, y) for x, y in zip(a, c))
    assert all(len(x) == 40 and x.min() >= 0 and x.max() < 625 for x in a)
    # explicit key; shard [2, 5) == rows 2..4 of the full batch
    full = run(rng_seed=4242)
    part = run(slice(2, 5), rng_seed=4242)
    assert all(np.array_equal(full[2 + i], part[i]) for i in range(3))
    # unseeded = a fresh draw per step; seeded = the same draw at every step (so the two differ for the same key)
    seeded = run(seed=4242)
    assert any(not np.array_equal(x, y) for x, y in zip(full, seeded))
    assert all(np.array_equal(x, y) for x, y in zip(seeded, run(seed=4242)))
    # continuous batching without a seed
    S = 3
    pool = SlotPool(gpt_f32, slots=S, cap=96, hid_cap=48, manual_seed=None, rng="device", rng_seed=99)
    rs = np.random.RandomState(8)
    reqs = {}
    for i, n in enumerate([6, 13, 9, 4, 11]):
        T = int(rs.randint(5, 12))
        rid = np.repeat(rs.randint(1, 21178, size=(T, 1)), 4, axis=1).astype(np.int64)
        reqs[i] = (rid, n)
        pool.submit(i, rid, max_new_token=32, stop_at=n)
    got = {rid: t.cpu().numpy() for rid, t, _ in pool.run()}
    for rid, (pid, n) in reqs.items():
        p_t = torch.from_numpy(pid)[None]
        e1 = gpt_f32.embed_prompt(p_t, torch.ones((1, pid.shape[0]), dtype=torch.bool))
        ref = list(gpt_f32.generate(e1, p_t, torch.tensor([0.3] * 4), 625, None, 40, 0, (*procs, *warpers), manual_seed=None, rng="device",
                                    rng_seed=99, stop_at=torch.tensor([n], dtype=torch.int32), row_offset=4 * pool.slot_of[rid],
                                    total_rows=4 * S, rng_nonce=pool.nonce_of[rid]))[-1]
        assert np.array_equal(got[rid], ref.ids[0].cpu().numpy()), rid
    # every admission draws from its own stream (one pool-wide seed replayed the previous occupant's Exp(1) stream in a reused
    # slot): admission numbers never repeat, a second round through the SAME slots is reproduced in isolation only with ITS numbers,
    # and the number really is part of the generator's counter -- at a flat temperature two numbers give different tokens
    assert len(set(pool.nonce_of.values())) == len(reqs)
    for i, (pid, n) in reqs.items():
        pool.submit(("again", i), pid, max_new_token=32, stop_at=n)
    again = {rid: t.cpu().numpy() for rid, t, _ in pool.run()}
    assert len(set(pool.nonce_of.values())) == 2 * len(reqs)
    assert any(pool.slot_of[("again", i)] == pool.slot_of[i] for i in reqs), "the replay was meant to reuse slots"
    for i, (pid, n) in reqs.items():
        p_t = torch.from_numpy(pid)[None]
        e1 = gpt_f32.embed_prompt(p_t, torch.ones((1, pid.shape[0]), dtype=torch.bool))
        ref = list(gpt_f32.generate(e1, p_t, torch.tensor([0.3] * 4), 625, None, 40, 0, (*procs, *warpers), manual_seed=None, rng="device",
                                    rng_seed=99, stop_at=torch.tensor([n], dtype=torch.int32), row_offset=4 * pool.slot_of[("again", i)],
                                    total_rows=4 * S, rng_nonce=pool.nonce_of[("again", i)]))[-1]
        assert np.array_equal(again[("again", i)], ref.ids[0].cpu().numpy()), i
    pid = reqs[1][0]
    p_t = torch.from_numpy(pid)[None]
    e1 = gpt_f32.embed_prompt(p_t, torch.ones((1, pid.shape[0]), dtype=torch.bool))
    flat = lambda nonce: list(gpt_f32.generate(e1, p_t, torch.tensor([3.0] * 4), 625, None, 24, 24, (), manual_seed=None, rng="device",
                                               rng_seed=99, rng_nonce=nonce))[-1].ids[0].cpu().numpy()
    assert np.array_equal(flat(1), flat(1)) and not np.array_equal(flat(1), flat(2))
    pool.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_final_norm_heads_is_bit_identical(weights, golden, monkeypatch, dtype):
    """decode step: final RMSNorm + hidden capture + heads as ONE launch (decode32.hip gemm_dec32_fnorm16_k: row statistics from the
    MFMA fragments in final_norm_k's association) vs the separate final_norm_k + heads launches (CTTS_FNORM_FUSE=0): token ids AND
    the captured hidden states are bit-identical, in both numeric modes (rows finishing at different steps, left padding)."""
    c = cases.GEN_CASES["b8"]
    fused = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)
    a, _ = run_case(fused, c, use_graph=True)
    monkeypatch.setenv("CTTS_FNORM_FUSE", "0")
    sep = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)
    monkeypatch.delenv("CTTS_FNORM_FUSE")
    b, _ = run_case(sep, c, use_graph=True)
    assert len(a[-1].ids) == len(b[-1].ids) == 8
    for x, y in zip(a[-1].ids, b[-1].ids):
        assert torch.equal(x, y)
    for x, y in zip(a[-1].hiddens, b[-1].hiddens):
        assert x.shape == y.shape and torch.equal(x, y)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_embed_fold_is_bit_identical(weights, golden, monkeypatch, dtype):
    """multi-step graphs with the next step's first kernel folded into sample_k's tail (CTTS_EMBED_FOLD=1: steps 2 .. 8 of a group take
    their input rows and descriptors from the previous step's sampling launch, kernels.hpp EmbedNext) vs the default, where every step
    launches embed_codes_k: token ids AND the captured hidden states are bit-identical, in both numeric modes (rows finishing at
    different steps -- inside a group their compact rows go dead instead of being re-ranked -- and left padding)."""
    c = cases.GEN_CASES["b8"]
    plain = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)
    a, _ = run_case(plain, c, use_graph=True)
    monkeypatch.setenv("CTTS_EMBED_FOLD", "1")
    fold = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)
    monkeypatch.delenv("CTTS_EMBED_FOLD")
    b, _ = run_case(fold, c, use_graph=True)
    assert len(a[-1].ids) == len(b[-1].ids) == 8
    for x, y in zip(a[-1].ids, b[-1].ids):
        assert torch.equal(x, y)
    for x, y in zip(a[-1].hiddens, b[-1].hiddens):
        assert x.shape == y.shape and torch.equal(x, y)


def test_pipelined_batches_equal_sequential(weights):
    """`Chat.infer_ids_pipelined` (acoustic decode + D2H of batch i on the codec engine's side stream while batch i+1 is generated,
    `CodecEngine.decode_to_wavs_async`) yields, per batch and in order, exactly what `Chat.infer_ids` returns for that batch --
    different batch geometries back to back (the GPT session and the codec workspace are re-used / re-grown underneath)."""
    from chattts_amd.core import Chat, InferCodeParams
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32")
    p = InferCodeParams(max_new_token=40, manual_seed=3, show_tqdm=False)
    batches = []
    for i, (B, stop) in enumerate([(3, [9, 20, 14]), (5, [30, 7, 12, 25, 18]), (3, [11, 11, 5]), (1, [33])]):
        ids, mask, tmask = synth.make_prompts(B, 6, 12, seed=20 + i)
        batches.append((torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask), {"stop_at": torch.tensor(stop, dtype=torch.int32)}))
    seq = [chat.infer_ids(*b[:3], p, **b[3]) for b in batches]
    pip = list(chat.infer_ids_pipelined(batches, p))
    assert len(pip) == len(seq)
    for a, b in zip(seq, pip):
        assert a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
    # a pending result can be asked for late, and twice
    out = list(chat.infer_code(*batches[0][:3], p, **batches[0][3]))[-1]
    fut = chat.codec.decode_to_wavs_async(out.hiddens)
    list(chat.infer_code(*batches[1][:3], p, **batches[1][3]))
    assert np.array_equal(fut.result(), seq[0]) and fut.result() is fut.result() and fut.done()


def test_packed_f32_prefill_is_bit_identical_to_row_major(weights, golden, monkeypatch):
    """parity mode: the prompt pass on fragment-packed f32 operands (decode32.hip's 64-row workgroups, RoPE + KV append in the QKV
    epilogue from per-row descriptors, packed attention output) against the row-major kernels the goldens were established with
    (CTTS_PRE32_PACKED=0): token ids AND hidden states torch.equal -- left-padded batch, whole prompt and prefill in chunks."""
    c = cases.GEN_CASES["b8"]
    new = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    monkeypatch.setenv("CTTS_PRE32_PACKED", "0")
    old = E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype="f32")
    monkeypatch.delenv("CTTS_PRE32_PACKED")
    ids, mask, tmask = cases.gen_inputs(c)
    ids_t, mask_t, tm_t = torch.from_numpy(ids), torch.from_numpy(mask), torch.from_numpy(tmask)
    warpers, procs = E.gen_logits(625, c["top_P"], c["top_K"], c["rep"])

    def run(eng, chunk):
        emb = eng.embed_prompt(ids_t, tm_t)
        return list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), 625, mask_t, 24, c["min_new"], (*procs, *warpers),
                                 return_hidden=True, manual_seed=c["manual_seed"], prefill_chunk=chunk))[-1]

    for chunk in (None, 5):
        a, b = run(new, chunk), run(old, chunk)
        for x, y in zip(a.ids, b.ids):
            assert torch.equal(x, y)
        for x, y in zip(a.hiddens, b.hiddens):
            assert x.shape == y.shape and torch.equal(x, y)

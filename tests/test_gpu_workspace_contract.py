"""The library's side of the workspace contract, on the GPU: every call that runs inside a caller-supplied byte buffer -- the GPT
workspace, the codec workspaces, the DVAE's, the output stages' scratch -- is run in a buffer of EXACTLY the size its size function
declares, with guards on both sides, pre-filled with zeros, with 0x7F bytes (huge finite floats) and with 0xFF bytes (NaNs, -1)
(tests/ws_arena.py, put in the place of `engine.device_scratch`).  Every test asserts the same four things:

  * the arena handed out at least one buffer during the call (the call really went through the seam);
  * no guard byte changed (the size function covers what the kernels write);
  * the results are bit-identical under the three patterns (nothing reads what the call did not write first);
  * and bit-identical to an un-instrumented run of the same engine.

No tolerance anywhere.  In the parity modes the token ids are also the committed goldens'.  The patterns run in the order zeros, 0x7F,
0xFF.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import compressor as CP  # noqa: E402
from chattts_amd import engine as E  # noqa: E402
from chattts_amd import limiter as LM  # noqa: E402
from chattts_amd import loudness as LN  # noqa: E402
from chattts_amd import synth  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from oracle import cases  # noqa: E402
from tests.gpu_util import ragged_edge_rows  # noqa: E402
from tests.ws_arena import GUARD_MIN, Arena  # noqa: E402

DEV = torch.device("cuda:0")
ORDER = (0x00, 0x7F, 0xFF)
MIB = 1 << 20


def _bits(x):
    """a result as something `np.array_equal` compares bit for bit (NaNs included)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "f":
        return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
    if x.dtype.names:
        return x.view(np.uint8)
    return x


def _same(got, want, what):
    """two results (arrays, tensors, or nested lists / tuples of them) are equal bit for bit"""
    if isinstance(got, (list, tuple)):
        assert isinstance(want, (list, tuple)) and len(got) == len(want), (what, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{what}[{i}]")
        return
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if not np.array_equal(g, w):
        d = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        pytest.fail(f"{what}: {d.size} of {g.size} elements differ, first at flat index {int(d[0])}")


def _contract(monkeypatch, call, capacity, what, patch, guard=GUARD_MIN, reset=None, min_takes=1):
    """the four assertions.  `call()` -> the results; `patch(mp, arena)` puts the arena in the allocation's place; `reset()` makes the
    next call allocate again (a cached session would keep the previous call's workspace); `min_takes`: the buffers a call that
    allocates in several places must ask for"""
    plain = call()
    torch.cuda.synchronize()
    for fill in ORDER:
        if reset is not None:
            reset()
        arena = Arena(capacity, fill, DEV, guard=guard)
        with monkeypatch.context() as mp:
            patch(mp, arena)
            got = call()
            torch.cuda.synchronize()
        assert arena.takes >= min_takes, \
            f"{what}: the call allocated {arena.takes} of its {min_takes} workspaces through the seam (pattern 0x{fill:02X})"
        arena.assert_guards_intact()
        _same(got, plain, f"{what}, pattern 0x{fill:02X} against the un-instrumented run")
        del arena
    return plain


def _seam(mp, arena):
    mp.setattr(E, "device_scratch", arena.device_scratch)


# ---- GPT ---------------------------------------------------------------------------------------------------------------------------
GPT_DTYPES = ["f32", "f32x3", "bf16"]


def _gpt(weights, dtype):
    return E.GptEngine(weights["gpt"], weights["embed"], DEV, dtype=dtype)


def _drop_sessions(eng):
    """the next generate() allocates its lanes again: a session keeps its workspace (and its captured graph) for the next call of the
    same geometry"""
    eng._session = eng._session_alt = eng._session_text = None


def _gpt_capacity(eng, B, T, takes=1):
    n = max(eng.lib.ctts_gpt_workspace_bytes(B, T), eng.lib.ctts_gpt_workspace_bytes(B, 1))
    return Arena.room([n] * takes)


def _generate(eng, c, ids, mask, tmask, *, use_graph, text=False, **kw):
    """tests/test_gpu_e2e.run_case's recipe -> (lens, ids of all utterances, hidden rows of all utterances)"""
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    emb = eng.embed_prompt(ids_t, torch.from_numpy(tmask))
    warpers, procs = E.gen_logits(21178 if text else 625, c["top_P"], c["top_K"], c["rep"])
    out = list(eng.generate(emb, ids_t, torch.tensor(c["temperature"]), cases.TEXT_EOS if text else 625, mask_t, c["max_new"], c["min_new"],
                            (*procs, *warpers), infer_text=text, return_hidden=True, manual_seed=c["manual_seed"], use_graph=use_graph, **kw))[-1]
    lens = np.array([int(t.shape[0]) for t in out.ids])
    return lens, np.concatenate([t.cpu().numpy() for t in out.ids], 0), torch.cat(list(out.hiddens), 0)


def _gpt_contract(monkeypatch, weights, dtype, call_of, B, T, what):
    eng = _gpt(weights, dtype)
    return _contract(monkeypatch, lambda: call_of(eng), _gpt_capacity(eng, B, T), f"{what} [{dtype}]", _seam, reset=lambda: _drop_sessions(eng))


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name", ["c1", "b8"])
@pytest.mark.parametrize("dtype", GPT_DTYPES)
def test_gpt_generate_cases(monkeypatch, weights, golden, dtype, name, use_graph):
    """cases.GEN_CASES c1 (one row: 15 pad rows in the 16-row tile) and b8 (a left-padded batch of 8); parity modes: the golden ids"""
    c = cases.GEN_CASES[name]
    ids, mask, tmask = cases.gen_inputs(c)
    lens, got, _ = _gpt_contract(monkeypatch, weights, dtype, lambda eng: _generate(eng, c, ids, mask, tmask, use_graph=use_graph),
                                 ids.shape[0], ids.shape[1], f"generate {name}, graph={use_graph}")
    if dtype != "bf16":
        Gd = golden["generate"]
        assert np.array_equal(lens, Gd[name + ".lens"]) and np.array_equal(got, Gd[name + ".ids"])


_SHAPES = {
    # 3 utterances x 21 slots: 63 prompt rows, a multiple of no tile
    "rows63": dict(B=3, t_min=21, t_max=21, pseed=21, stop=[6, 11, 3], max_new=16),
    # 17 utterances: Bp = 32, 15 pad rows inside every packed plane of the decode step
    "b17": dict(B=17, t_min=6, t_max=11, pseed=17, stop=[3 + (5 * i) % 10 for i in range(17)], max_new=13),
}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("shape", list(_SHAPES))
@pytest.mark.parametrize("dtype", GPT_DTYPES)
def test_gpt_rows_inside_padded_tiles(monkeypatch, weights, dtype, shape, use_graph):
    s = _SHAPES[shape]
    c = dict(top_P=0.7, top_K=20, rep=1.05, temperature=[0.3] * 4, max_new=s["max_new"], min_new=0, manual_seed=5)
    ids, mask, tmask = synth.make_prompts(s["B"], s["t_min"], s["t_max"], seed=s["pseed"])
    stop = torch.tensor(s["stop"], dtype=torch.int32)
    lens, _, _ = _gpt_contract(monkeypatch, weights, dtype,
                               lambda eng: _generate(eng, c, ids, mask, tmask, use_graph=use_graph, stop_at=stop),
                               ids.shape[0], ids.shape[1], f"generate {shape}, graph={use_graph}")
    assert lens.tolist() == s["stop"]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", GPT_DTYPES)
def test_gpt_chunked_prefill_with_a_short_last_chunk(monkeypatch, weights, golden, dtype, use_graph):
    """b8 (27 prompt slots) prefilled in chunks of 5: five whole chunks and a last one of 2 -- one workspace carved three ways in one
    call (chunk, last chunk, decode step).  The workspace is sized for a chunk, not for the prompt"""
    c = cases.GEN_CASES["b8"]
    ids, mask, tmask = cases.gen_inputs(c)
    assert ids.shape[1] == 27
    lens, got, _ = _gpt_contract(monkeypatch, weights, dtype,
                                 lambda eng: _generate(eng, c, ids, mask, tmask, use_graph=use_graph, prefill_chunk=5),
                                 ids.shape[0], 5, f"chunked prefill of b8, graph={use_graph}")
    if dtype != "bf16":
        assert np.array_equal(lens, golden["generate"]["b8.lens"]) and np.array_equal(got, golden["generate"]["b8.ids"])


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", GPT_DTYPES)
def test_gpt_refine_text_mode(monkeypatch, weights, golden, dtype, use_graph):
    """infer_text: the `logits` field is read at its full NTEXT_MAX-sized width"""
    c = cases.TEXT_CASES["text3"]
    ids, mask, tmask = cases.gen_inputs(c)
    lens, got, _ = _gpt_contract(monkeypatch, weights, dtype,
                                 lambda eng: _generate(eng, c, ids, mask, tmask, use_graph=use_graph, text=True),
                                 ids.shape[0], ids.shape[1], f"refine-text text3, graph={use_graph}")
    if dtype != "bf16":
        assert np.array_equal(lens, golden["text"]["text3.lens"]) and np.array_equal(got, golden["text"]["text3.ids"])


@pytest.mark.parametrize("dtype", GPT_DTYPES)
def test_slot_pool_admissions_and_decode(monkeypatch, weights, dtype):
    """6 short requests through 2 slots: the pool's decode workspace (one row per slot, graph replay) and one prefill workspace per
    admission, each of its own size"""
    from chattts_amd.serving import SlotPool
    eng = _gpt(weights, dtype)
    rs = np.random.RandomState(6)
    reqs = [(np.repeat(rs.randint(1, 21178, size=(int(rs.randint(6, 22)), 1)), 4, axis=1).astype(np.int64), n) for n in (5, 11, 3, 9, 2, 7)]
    S, sizes = 2, []

    def call():
        pool = SlotPool(eng, slots=S, cap=64, hid_cap=16, manual_seed=21)
        for i, (ids, n) in enumerate(reqs):
            pool.submit(i, ids, max_new_token=16, stop_at=n)
        got = {rid: (ids.cpu().numpy(), hid.cpu().numpy()) for rid, ids, hid in pool.run()}
        pool.close()
        assert sorted(got) == list(range(len(reqs)))
        return [got[i][0] for i in range(len(reqs))], [got[i][1] for i in range(len(reqs))]

    def patch(mp, arena):
        sizes.append(arena.sizes)
        _seam(mp, arena)

    worst = max(eng.lib.ctts_gpt_workspace_bytes(S, 22), eng.lib.ctts_gpt_workspace_bytes(S, 1))
    ids_out, _ = _contract(monkeypatch, call, Arena.room([worst] * (len(reqs) + 1)), f"slot pool [{dtype}]", patch)
    assert [a.shape for a in ids_out] == [(n, 4) for _, n in reqs]
    for got in sizes:                       # the decode workspace, then at least one admission per slot-load of requests
        assert got[0] == eng.lib.ctts_gpt_workspace_bytes(S, 1) and len(reqs) // S <= len(got) - 1 <= len(reqs), got


# ---- acoustic decoder --------------------------------------------------------------------------------------------------------------
GEMMS = ["f32", "bf16x3", "f16"]
# [B, T] with B * 2 T frames one frame pair either side of a 256-row tile, of the 1,024-frame switch to the x3p / h1p planes and of the
# 12,288-frame switch to the big tile and the sliding-window dwconv; [3, 43]: three rows, 258 frames, no multiple of 256; and
# [1, 128]: exactly one 256-row tile -- the only kind of size at which the fields have no pad rows behind their last frame, so that a
# size function that is short shows in the back guard
DENSE = [(1, 1), (1, 127), (1, 128), (1, 129), (1, 511), (1, 513), (1, 6145), (3, 43)]


def _codec(weights, gemm):
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("CTTS_X3P_MIN_ROWS", raising=False)        # the default thresholds
        return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)


def _codec_ws(codec):
    """the override of `CodecEngine._ws_bytes`: exactly the n bytes asked for, and n as the size the library is told"""
    return lambda mp, arena: mp.setattr(codec, "_ws_bytes", arena.codec_ws_bytes)


def _hid(B, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (0.5 * torch.randn((B, T, 768), generator=g)).to(DEV)


@pytest.mark.parametrize("gemm", GEMMS)
def test_codec_dense_decode_at_tile_edges_and_kernel_switches(monkeypatch, weights, gemm):
    codec = _codec(weights, gemm)
    for B, T in DENSE:
        hid = _hid(B, T, 100 * B + T)

        def call():
            mel = codec.dvae_decode(hid)
            return mel, codec.vocos_decode(mel)

        n = codec.lib.ctts_codec_workspace_bytes(B, 2 * T)
        mel, wav = _contract(monkeypatch, call, Arena.room([n, n], 4 * MIB), f"dense decode [{gemm}] B={B} T={T}", _codec_ws(codec), guard=4 * MIB)
        assert mel.shape == (B, 2 * T, 100) and wav.shape == (B, 256 * (2 * T - 1)) and bool(torch.isfinite(wav).all())


def test_codec_grow_only_buffer_comes_from_the_seam(monkeypatch, weights):
    """`CodecEngine._ws_bytes` itself: a fresh engine's first call allocates through the seam, exactly what it asked for; a smaller call
    behind it allocates nothing"""
    hid = _hid(1, 129, 7)
    want = _codec(weights, "f32").dvae_decode(hid)
    for fill in ORDER:
        codec = _codec(weights, "f32")
        n = codec.lib.ctts_codec_workspace_bytes(1, 258)
        arena = Arena(Arena.room([n]), fill, DEV)
        with monkeypatch.context() as mp:
            _seam(mp, arena)
            got = codec.dvae_decode(hid)
            small = codec.dvae_decode(hid[:, :5])
            torch.cuda.synchronize()
        assert arena.sizes == [n]
        arena.assert_guards_intact()
        _same(got, want, f"first decode of a fresh engine, pattern 0x{fill:02X}")
        _same(small, codec.dvae_decode(hid[:, :5]), "a smaller decode in the grown buffer")


@pytest.mark.parametrize("total", [1026, 12290])
@pytest.mark.parametrize("gemm", GEMMS)
def test_codec_ragged_decode_with_the_segment_table_behind_the_carve(monkeypatch, weights, gemm, total):
    codec = _codec(weights, gemm)
    lens, rows = ragged_edge_rows(total)
    rows = [torch.from_numpy(r).to(DEV) for r in rows]

    def call():
        wav, off, mel = codec.decode_ragged(rows, return_mel=True)
        return wav, off, mel

    n = codec.lib.ctts_codec_ragged_workspace_bytes(len(rows), total // 2)
    wav, off, mel = _contract(monkeypatch, call, Arena.room([n], 4 * MIB), f"ragged decode [{gemm}] of {total} frames", _codec_ws(codec), guard=4 * MIB)
    assert mel.shape == (total, 100) and int(off[-1]) == wav.numel() == 256 * (total - len(rows))


# windows: (slot, prefix tokens, s_lo, s_hi); unequal token counts, a 1-token prefix, crops that cut both halos
WINDOWS = [(0, 1, 0, None), (1, 30, 2000, 9000), (2, 7, 0, None), (3, 3, 256, 1000), (4, 12, 100, 5000)]
N_WIN = [1, 3, 5]
RATES = [16000, 8000]
SPEEDS = [0.5, 2.0]


def _store(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((5, 32, 768), device=DEV, generator=g)


def _windows_capacity(codec, n_win):
    """room for one window workspace of any of the four entries: the plain one for the whole token total plus a generous chunk area"""
    T = sum(w[1] for w in WINDOWS[:n_win])
    return Arena.room([codec.lib.ctts_codec_windows_speed_workspace_bytes(n_win, T, 4 * 512 * T + 65536)] * 2, MIB)


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("n_win", N_WIN)
@pytest.mark.parametrize("gemm", GEMMS)
def test_window_decode_plain_and_at_other_rates(monkeypatch, weights, gemm, n_win, pcm16):
    """ctts_codec_decode_windows and ctts_codec_decode_windows_rate: the resampled chunks are the last field of the workspace, sized on
    the host"""
    codec, store = _codec(weights, gemm), _store()
    wins = WINDOWS[:n_win]
    rates = [RATES[i % 2] for i in range(n_win)]
    cap = _windows_capacity(codec, n_win)
    _contract(monkeypatch, lambda: codec.decode_windows(store, wins, pcm16=pcm16), cap, f"windows [{gemm}] n={n_win}", _codec_ws(codec), guard=MIB)
    got = _contract(monkeypatch, lambda: codec.decode_windows(store, wins, pcm16=pcm16, sample_rates=rates), cap,
                    f"windows at {rates} Hz [{gemm}] n={n_win}", _codec_ws(codec), guard=MIB)
    assert all(g.size > 0 for g in got)


@pytest.mark.parametrize("with_rate", [False, True])
@pytest.mark.parametrize("n_win", N_WIN)
@pytest.mark.parametrize("gemm", GEMMS)
def test_window_decode_of_time_scaled_streams(monkeypatch, weights, gemm, n_win, with_rate):
    """ctts_codec_decode_windows_speed and ctts_codec_decode_windows_speed_rate: every window is the one push of a stream of its own
    (first and last), at speed 0.5 or 2.0, and with `with_rate` on into a resampler stream"""
    codec, store = _codec(weights, gemm), _store(4)
    wins = [(*w[:2], 0, None, True) for w in WINDOWS[:n_win]]
    speeds = [SPEEDS[i % 2] for i in range(n_win)]
    rates = [RATES[i % 2] for i in range(n_win)]

    def call():
        ts = [codec.time_scale_stream_open(v) for v in speeds]
        rs = [codec.resample_stream_open(24000, r) for r in rates] if with_rate else None
        try:
            kw = dict(sample_rates=rates, rs_streams=rs) if with_rate else {}
            return codec.decode_windows(store, wins, pcm16=False, speeds=speeds, ts_streams=ts, **kw)
        finally:
            for h in ts:
                codec.time_scale_stream_close(h)
            for h in rs or []:
                codec.resample_stream_close(h)

    got = _contract(monkeypatch, call, _windows_capacity(codec, n_win), f"windows at speeds {speeds} (rates: {with_rate}) [{gemm}] n={n_win}",
                    _codec_ws(codec), guard=MIB)
    assert all(g.dtype == np.float32 and g.size > 0 for g in got)


# ---- the DVAE engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [513, 10257])            # the shortest clip the encoder takes; 40 hops + 17 samples, an odd frame count
def test_dvae_encode_in_its_declared_workspace(monkeypatch, n):
    from chattts_amd.dvae import DvaeEngine
    eng = DvaeEngine(W.synthetic_dvae(), DEV)
    wav = (0.3 * np.random.RandomState(n).standard_normal(n)).astype(np.float32)
    nb = eng.lib.ctts_dvae_encode_workspace_bytes(n)
    codes = _contract(monkeypatch, lambda: eng.sample_audio(wav), Arena.room([nb]), f"dvae encode of {n} samples", _seam)
    assert tuple(codes.shape) == (4, int(eng.lib.ctts_dvae_code_frames(n))) and int(codes.min()) >= 0 and int(codes.max()) < 625


@pytest.mark.parametrize("T", [1, 33])
def test_dvae_decode_codes_in_its_declared_workspace(monkeypatch, T):
    from chattts_amd.dvae import DvaeEngine
    eng = DvaeEngine(W.synthetic_dvae(), DEV)
    ids = torch.from_numpy(np.random.RandomState(T).randint(0, 625, size=(2, T, 4))).to(DEV)
    nb = eng.lib.ctts_dvae_decode_workspace_bytes(2, T)
    mel = _contract(monkeypatch, lambda: eng.decode_codes(ids), Arena.room([nb]), f"dvae decode of [2, {T}] codes", _seam)
    assert mel.shape == (2, 2 * T, 100) and bool(torch.isfinite(mel).all())


# ---- output stages: three segments of 1 sample, one tile - 1 and one tile + 1 ---------------------------------------------------------
GROUP_TILE = 2048          # samples per workgroup of the grouped conversion (csrc/codec.hip, GT)
PAUSE_TILE_FRAMES = 16     # frames per workgroup of the pause stage's copy pass (csrc/kernels.hpp, PA_FPB); a frame is rate // 100 samples


def _pack(tile, seed):
    """(packed float32 device tensor, int64 offsets) of segments of 1, tile - 1 and tile + 1 samples: N(0, 0.3) with a quiet stretch in
    the middle of each long one, so that limiter, compressor and pause stage all have something to do"""
    lens = [1, tile - 1, tile + 1]
    rs = np.random.RandomState(seed)
    xs = []
    for n in lens:
        x = (0.3 * rs.standard_normal(n)).astype(np.float32)
        x[n // 3: n // 2] *= np.float32(1e-4)
        xs.append(x)
    return torch.from_numpy(np.concatenate(xs)).to(DEV), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.fixture()
def stage_codec(weights):
    return _codec(weights, "f32")


def _stage_contract(monkeypatch, call, what, min_takes=1):
    return _contract(monkeypatch, call, 8 * MIB, what, _seam, min_takes=min_takes)


@pytest.mark.parametrize("limiter", [None, [True, False, True]])
def test_stage_loudness_normalize(monkeypatch, stage_codec, limiter):
    fs = 10 * LN.H_MIN                                                   # 8 kHz: a sub-block of LN.H_MIN = 800 samples
    assert LN.H_MIN == 800
    x, off = _pack(LN.H_MIN, 1)
    # with the limiter table: the loudness stage's own scratch, then one limiter call per run of flagged neighbours (two here)
    _stage_contract(monkeypatch, lambda: stage_codec.loudness_normalize(x, -20.0, offsets=off, rates=fs, return_stats=True, limiter=limiter),
                    f"loudness_normalize(limiter={limiter})", min_takes=1 if limiter is None else 3)


def test_stage_peak_limit(monkeypatch, stage_codec):
    x, off = _pack(LM.TILE, 2)
    y, st = _stage_contract(monkeypatch, lambda: stage_codec.peak_limit(x, offsets=off, gains=4.0, return_stats=True), "peak_limit")
    assert int(st["n_over"].sum()) > 0


def test_stage_compress(monkeypatch, stage_codec):
    x, off = _pack(CP.TILE_BLOCKS * 24, 3)                              # 24 kHz: a block is 24 samples
    y, st = _stage_contract(monkeypatch, lambda: stage_codec.compress(x, True, offsets=off, return_stats=True), "compress")
    assert int(st["n_blocks"].sum()) > 0


def test_stage_trim_pauses_ragged(monkeypatch, stage_codec):
    x, off = _pack(PAUSE_TILE_FRAMES * 240, 4)
    spec = dict(max_pause_ms=20, lead_ms=0, tail_ms=0)
    _stage_contract(monkeypatch, lambda: stage_codec.trim_pauses(x, spec, offsets=off, return_stats=True), "trim_pauses")


def test_stage_trim_pauses_stream_step(monkeypatch, stage_codec):
    """three streams stepped together, twice: pushes of 1, tile - 1 and tile + 1 samples, the second push their last"""
    x, off = _pack(PAUSE_TILE_FRAMES * 240, 5)
    spec = dict(max_pause_ms=20, lead_ms=0, tail_ms=0)

    def call():
        hs = [stage_codec.trim_pauses_stream_open(24000, spec) for _ in range(3)]
        try:
            out = []
            for final in (False, True):
                y, o = stage_codec.trim_pauses_stream_step(x, [(h, int(off[i]), int(off[i + 1] - off[i]), final) for i, h in enumerate(hs)])
                out += [y, o]
            return out
        finally:
            for h in hs:
                stage_codec.trim_pauses_stream_close(h)

    _stage_contract(monkeypatch, call, "trim_pauses_stream_step")


@pytest.mark.parametrize("keep_thr", [None, 1e-3])
def test_stage_float_to_int16_groups(monkeypatch, stage_codec, keep_thr):
    x, off = _pack(GROUP_TILE, 6)
    grp = np.array([0, 1, 3], dtype=np.int32)                            # the 1-sample segment alone; tile - 1 and tile + 1 together

    def call():
        blob, starts = stage_codec.float_to_int16_groups(x, off, grp, keep_thr=keep_thr)
        return stage_codec.unpack_groups(blob.cpu().numpy(), starts)

    got = _stage_contract(monkeypatch, call, f"float_to_int16_groups(keep_thr={keep_thr})")
    assert len(got) == 2 and (keep_thr is not None or [g.size for g in got] == [1, 2 * GROUP_TILE])

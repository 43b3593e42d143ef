"""The kernels that decide which compact row is which utterance (csrc/gpt.hip), one by one through the C ABI: `embed_codes_k` /
`embed_text_k` with a caller-filled StepPrep (`ctts_k_step_prep`: device-side and host compaction, `write_desc`, `write_rope_cs`,
`step_zero`, every output format of `emit_row`), `prefill_prep32_k` and `prefill_compact_k`.

The reference is a numpy restatement of the contract (tests/gpu_util.py `row_desc`, `live_rows`) and of the embedding sum -- codebooks
0..3 added in float32 in that order -- so descriptors, row maps and every copy of the rows are compared EXACTLY; only the 48 partial
sums of squares have a bound.  Every output buffer starts as NaN or a sentinel word: a slot the kernel must not write is compared
with that, a slot it skipped cannot pass.

The readers of the descriptors at the end of the step -- `final_norm_k`, the fused final norm + heads, the samplers -- and the one
remaining writer, the `EmbedNext` fold in `sample_k`'s tail (CTTS_EMBED_FOLD), are in tests/test_gpu_step_back.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E  # noqa: E402

f32 = np.float32
HID, NVQ, NAUDIO = 768, 4, 626
HO_STRIDE = 1088          # csrc/kernels.hpp: ints between two arrival words of the fused QKV + attention launch
N_TEXT = 300              # rows of the text table these tests use (the kernel takes any n_text)
EDGE_CODE, EDGE_TEXT = 600, 250   # table rows that hold EDGE_VALUES (codebooks 1..3 of EDGE_CODE are zero: the sum IS the row)
# what a 16-bit copy can get wrong: signed zeros, below fp16's normal range, fp16 / bf16 rounding ties, fp16's largest finite value,
# the saturating range of the split-fp16 format, the top of bf16's range
EDGE_VALUES = np.array([0.0, -0.0, 1e-7, -6e-5, 6.1e-5, 2.0 ** -14, 2.0 ** -24, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                        65504.0, 65519.99, 65520.0, 70000.0, -70000.0, 3.0e38, 0.1, 1.0 / 3.0, 2049.0, -2051.0, 1e-3, 5.9604645e-8, 1.0], f32)


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


# ---- inputs (shared between the tests, never written) ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _tables():
    rs = np.random.RandomState(1234)
    code = rs.standard_normal((NVQ, NAUDIO, HID)).astype(f32)
    code[:, EDGE_CODE] = 0
    code[0, EDGE_CODE] = np.resize(EDGE_VALUES, HID)
    text = rs.standard_normal((N_TEXT, HID)).astype(f32)
    text[EDGE_TEXT] = np.resize(EDGE_VALUES, HID)
    cos, sin = E.rope_tables(64)
    return code, text, cos.numpy(), sin.numpy()


@functools.lru_cache(maxsize=1)
def _tables_dev():
    from tests import gpu_util as G
    return tuple(G.dev(t) for t in _tables())


def _embed_ref(ids_row, text):
    """the row the kernels sum: codebooks 0..3 in float32 in that order, ids clamped into the table (text: slot 0's id alone)"""
    code, txt, _, _ = _tables()
    if text:
        return txt[min(max(int(ids_row[0]), 0), N_TEXT - 1)].copy()
    s = None
    for k in range(NVQ):
        v = code[k, min(max(int(ids_row[k]), 0), NAUDIO - 1)]
        s = v.copy() if s is None else (s + v).astype(f32)
    return s


def _state(rs, B, tcap=12, text=False, pad_rows=True):
    """ids_buf [B, tcap, 4] (ids away from the edge rows), len in [1, tcap], kv_start in [0, tcap + 2) -- so some kv_start > slot"""
    ids = rs.randint(0, EDGE_TEXT if text else EDGE_CODE, size=(B, tcap, NVQ)).astype(np.int64)
    lens = rs.randint(1, tcap + 1, size=B).astype(np.int32)
    ks = rs.randint(0, tcap + 2, size=B).astype(np.int32)
    if pad_rows:
        ks[rs.randint(0, B)] = tcap + 1           # at least one pad row (kv_start > slot) ...
    ks[rs.randint(0, B)] = 0                      # ... and one row whose position is its slot (a later draw may hit the same utterance)
    return ids, lens, ks


def _ceil16(n):
    return (n + 15) // 16 * 16


def _step(G, B, ids, lens, *, text=False, tcap=12, row_map=None, n_active=None, kv_start=None, finish=None, fmt=None, xp32=False, ssq=False,
          desc=False, compact=False, order=None, rope=False, zero=None, zero_n=0, zero_stride=1):
    """one ctts_k_step_prep launch; every requested output starts as NaN / the sentinel and comes back as numpy"""
    code_d, text_d, cos_d, sin_d = _tables_dev()
    Bp = _ceil16(B)
    keep = {k: (None if v is None else G.dev(v)) for k, v in dict(ids=ids, lens=lens, row_map=row_map, kv_start=kv_start, finish=finish,
                                                                  order=order).items()}
    na_d = None if n_active is None else G.dev(np.array([n_active], np.int32))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=G.DEV)
    x = nan(B, HID)
    xb = None if fmt is None else torch.full({"rows": (B * HID,), "packed": (Bp * HID,), "x3": (2 * Bp * HID,)}[fmt], G.CANARY16,
                                             dtype=torch.int16, device=G.DEV)
    ssq_d = nan(B, 48) if ssq else None
    xp32_d = nan(Bp * HID) if xp32 else None
    desc_d = torch.full((B, 4), G.CANARY32, dtype=torch.int32, device=G.DEV) if desc else None
    rope_d = nan(B, 64) if rope else None
    rmo = torch.full((B,), G.CANARY32, dtype=torch.int32, device=G.DEV) if compact else None
    nao = torch.full((1,), G.CANARY32, dtype=torch.int32, device=G.DEV) if compact else None
    _lib.check(_lib.lib().ctts_k_step_prep((text_d if text else code_d).data_ptr(), N_TEXT if text else 0, keep["ids"].data_ptr(), tcap,
                                           keep["lens"].data_ptr(), x.data_ptr(), _lib.ptr(xb), _lib.ptr(ssq_d), B, _lib.ptr(keep["row_map"]),
                                           _lib.ptr(na_d), _lib.ptr(desc_d), _lib.ptr(keep["kv_start"]), _lib.ptr(keep["finish"]),
                                           1 if fmt in ("packed", "x3") else 0, _lib.ptr(xp32_d), Bp * HID if fmt == "x3" else 0, _lib.ptr(rmo),
                                           _lib.ptr(nao), _lib.ptr(keep["order"]), _lib.ptr(rope_d), cos_d.data_ptr() if rope else None,
                                           sin_d.data_ptr() if rope else None, _lib.ptr(zero), zero_n, zero_stride, None), "ctts_k_step_prep")
    torch.cuda.synchronize()
    out = dict(x=x, ssq=ssq_d, desc=desc_d, rope=rope_d, row_map_out=rmo, n_active_out=nao)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    if xp32:
        out["xp32"] = E.unpack_frag32(xp32_d.cpu(), Bp, HID).numpy()
    if fmt == "rows":
        out["xb"] = xb.cpu().reshape(B, HID)
    elif fmt == "packed":
        out["xb"] = E.unpack_frag(xb.cpu(), Bp, HID)
    elif fmt == "x3":
        out["xb"] = torch.stack([E.unpack_frag(p, Bp, HID) for p in xb.cpu().reshape(2, Bp * HID)], 0)   # [hi | lo'][Bp][768] int16 words
        out["x3"] = E.unpack_frag_x3(xb.cpu().view(torch.float16).reshape(2, Bp * HID), Bp, HID)            # hi + lo' / 2048, float32
    return out


def _is_nan_rows(a, rows):
    return bool(np.isnan(a[rows]).all())


# ---- (a) device-side compaction ----------------------------------------------------------------------------------------------------
A_SIZES = [1, 5, 63, 64, 65, 128, 130, 200]      # one 64-lane round, its last lane, the second round's first lane, its last, the third and fourth
A_PATTERNS = ["none", "all", "last", "slot64", "half"]
A_CASES = [(B, p) for B in A_SIZES for p in A_PATTERNS if p != "slot64" or B >= 65]


def _finish(rs, B, pattern):
    fin = np.ones(B, np.uint8)
    if pattern == "none":
        fin[:] = 0
    elif pattern == "last":
        fin[B - 1] = 0
    elif pattern == "slot64":
        fin[64] = 0
    elif pattern == "half":
        fin[rs.permutation(B)[: (B + 1) // 2]] = 0
    return fin


def _device_compaction(G, B, pattern, use_order, text):
    rs = np.random.RandomState(B * 17 + A_PATTERNS.index(pattern) * 3 + use_order)
    ids, lens, ks = _state(rs, B, text=text)
    fin = _finish(rs, B, pattern)
    order = rs.permutation(B).astype(np.int32) if use_order else None
    live = G.live_rows(fin, order)
    n = len(live)
    o = _step(G, B, ids, lens, text=text, kv_start=ks, finish=fin, fmt="packed", xp32=True, ssq=True, desc=True, compact=True, order=order,
              rope=True)
    _, _, cos, sin = _tables()
    assert int(o["n_active_out"][0]) == n
    assert o["row_map_out"][:n].tolist() == live
    assert (o["row_map_out"][n:] == G.CANARY32).all()                       # behind the live count: untouched
    want_desc = [G.row_desc(b, lens[b] - 1, ks[b]) for b in live] + [G.DESC_ABSENT] * (B - n)
    assert o["desc"].tolist() == [list(d) for d in want_desc]
    if n:
        want_x = np.stack([_embed_ref(ids[b, lens[b] - 1], text) for b in live])
        assert np.array_equal(o["x"][:n], want_x)
        assert np.array_equal(o["xp32"][:n], want_x)
        assert np.array_equal(o["xb"][:n].view(torch.bfloat16).float().numpy(), G.bf16_round(want_x))
        pos = np.array([d[2] for d in want_desc[:n]])
        assert np.array_equal(o["rope"][:n], np.concatenate([cos[pos], sin[pos]], 1))
        want_sq = (want_x.astype(np.float64).reshape(n, 48, 16) ** 2).sum(-1)
        assert (np.abs(o["ssq"][:n] - want_sq) <= 2e-6 * want_sq).all()         # a term passes <= 5 f32 roundings on its way into its partial: 5 x 2^-24 < 2e-6
    absent = slice(n, B)
    for name in ("x", "ssq", "rope"):
        assert _is_nan_rows(o[name], absent), name
    assert np.isnan(o["xp32"][n:]).all()
    assert (o["xb"][n:].numpy() == G.CANARY16).all()


@pytest.mark.parametrize("use_order", [False, True], ids=["ascending", "order"])
@pytest.mark.parametrize("B,pattern", A_CASES)
def test_embed_codes_device_compaction(G, B, pattern, use_order):
    """embed_codes_k ranks the finish flags itself (nth_unfinished, 64 utterances per round): live count, row map and descriptors exact,
    the live rows exact in every copy, the absent rows' descriptors {-1, 0, 0, 0} and nothing else of them written"""
    _device_compaction(G, B, pattern, use_order, False)


@pytest.mark.parametrize("use_order", [False, True], ids=["ascending", "order"])
@pytest.mark.parametrize("B,pattern", [(B, p) for B, p in A_CASES if B in (65, 130)])
def test_embed_text_device_compaction(G, B, pattern, use_order):
    """embed_text_k carries its own copy of the compaction's call site: the same contract past the first 64-lane round"""
    _device_compaction(G, B, pattern, use_order, True)


# ---- (b) host compaction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_act", [(5, 3), (40, 33), (64, None), (130, 70)])
def test_embed_codes_host_compaction(G, B, n_act):
    """the host's row_map + n_active (no row_map_out): a finished utterance in the middle keeps its row -- written in full, its
    descriptor carries b = -1 -- and rows from n_active on are not touched at all, descriptors included"""
    rs = np.random.RandomState(B + 1000)
    ids, lens, ks = _state(rs, B)
    n = B if n_act is None else n_act
    row_map = rs.permutation(B).astype(np.int32)
    fin = np.zeros(B, np.uint8)
    fin[row_map[n // 2]] = 1
    fin[row_map[n - 1]] = 1
    o = _step(G, B, ids, lens, row_map=row_map, n_active=n_act, kv_start=ks, finish=fin, xp32=True, desc=True, rope=True)
    _, _, cos, sin = _tables()
    want_desc = [G.row_desc(b, lens[b] - 1, ks[b], bool(fin[b])) for b in row_map[:n]]
    assert want_desc[n // 2][0] == -1
    assert o["desc"][:n].tolist() == [list(d) for d in want_desc]
    assert (o["desc"][n:] == G.CANARY32).all()
    want_x = np.stack([_embed_ref(ids[b, lens[b] - 1], False) for b in row_map[:n]])
    assert np.array_equal(o["x"][:n], want_x) and _is_nan_rows(o["x"], slice(n, B))
    assert np.array_equal(o["xp32"][:n], want_x) and np.isnan(o["xp32"][n:]).all()
    pos = np.array([d[2] for d in want_desc])
    assert np.array_equal(o["rope"][:n], np.concatenate([cos[pos], sin[pos]], 1)) and _is_nan_rows(o["rope"], slice(n, B))


def test_embed_codes_identity_rows_without_a_map(G):
    """neither row_map nor n_active nor finish: row m is utterance m"""
    B = 19
    rs = np.random.RandomState(7)
    ids, lens, ks = _state(rs, B)
    o = _step(G, B, ids, lens, kv_start=ks, desc=True)
    assert o["desc"].tolist() == [list(G.row_desc(b, lens[b] - 1, ks[b])) for b in range(B)]
    assert np.array_equal(o["x"], np.stack([_embed_ref(ids[b, lens[b] - 1], False) for b in range(B)]))


# ---- (c) every output format of emit_row -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rows", "packed", "f32", "x3"])
@pytest.mark.parametrize("text", [False, True], ids=["codes", "text"])
def test_emit_row_formats(G, text, fmt):
    """B = 37 rows (two full 16-row tiles and a partial one), ids outside the table clamped, one row of edge values in the 16-bit
    formats: x, the bf16 copies, the packed f32 copy and both split-fp16 planes exact; 48 partial sums of squares within f32 rounding"""
    B = 37
    rs = np.random.RandomState(100 + 2 * ["rows", "packed", "f32", "x3"].index(fmt) + text)
    ids, lens, ks = _state(rs, B, text=text)
    top = N_TEXT if text else NAUDIO
    for b, bad in zip((1, 2, 3, 20), (-3, top, 10 ** 6, -(10 ** 6))):       # clamped to row 0 / the last row
        ids[b, lens[b] - 1] = bad
    ids[4, lens[4] - 1, 1:] = [-1, top + 5, 17]                              # text reads slot 0 only; codes clamp each codebook by itself
    sq = fmt == "rows"
    if not sq:                                                               # (70000^2 is outside the bound the partial sums are held to)
        ids[0, lens[0] - 1] = EDGE_TEXT if text else EDGE_CODE
    o = _step(G, B, ids, lens, text=text, kv_start=ks, fmt=None if fmt == "f32" else fmt, xp32=fmt == "f32", ssq=sq, desc=True, rope=True)
    _, _, cos, sin = _tables()
    want_x = np.stack([_embed_ref(ids[b, lens[b] - 1], text) for b in range(B)])
    if text:                                                                 # (the reference's own clamp, restated)
        assert np.array_equal(want_x[1], _tables()[1][0]) and np.array_equal(want_x[2], _tables()[1][N_TEXT - 1])
    assert np.array_equal(o["x"], want_x)
    want_desc = [G.row_desc(b, lens[b] - 1, ks[b]) for b in range(B)]
    assert o["desc"].tolist() == [list(d) for d in want_desc]
    pos = np.array([d[2] for d in want_desc])
    assert np.array_equal(o["rope"], np.concatenate([cos[pos], sin[pos]], 1))
    Bp = _ceil16(B)
    if fmt in ("rows", "packed"):
        assert np.array_equal(o["xb"][:B].view(torch.bfloat16).float().numpy(), G.bf16_round(want_x))
    if fmt == "f32":
        assert np.array_equal(o["xp32"][:B], want_x) and np.isnan(o["xp32"][B:]).all()
    if fmt == "x3":
        hi, lo = E.split_f16(torch.from_numpy(want_x))
        got = o["xb"][:, :B].view(torch.float16)
        for name, g, w in (("hi", got[0], hi), ("lo", got[1], lo)):
            bad = np.argwhere(g.view(torch.int16).numpy() != w.view(torch.int16).numpy())
            assert bad.size == 0, (name, bad[:4].tolist(), [(float(want_x[r, c]), float(g[r, c]), float(w[r, c])) for r, c in bad[:4]])
        assert np.array_equal(o["x3"][:B].numpy(), (hi.float() + lo.float() / E.X3_LO_SCALE).numpy())   # engine.unpack_frag_x3 inverts the layout
    if fmt in ("packed", "x3"):
        assert (o["xb"][..., B:, :].numpy() == G.CANARY16).all()              # the partial tile's pad rows
    if sq:
        want_sq = (want_x.astype(np.float64).reshape(B, 48, 16) ** 2).sum(-1)
        assert np.abs(o["ssq"].sum(1) - want_sq.sum(1)).max() < 1e-2           # the bound test_gemm_dec_packed holds the same quantity to
        assert (np.abs(o["ssq"] - want_sq) <= 2e-6 * want_sq).all()            # per partial: a term passes <= 5 f32 roundings, 5 x 2^-24 < 2e-6


# ---- (d) step_zero -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("zero_stride", [1, HO_STRIDE])
@pytest.mark.parametrize("zero_n", [1, 240, 1000])
def test_step_zero(G, zero_n, zero_stride, B):
    """the step's first kernel zeroes zero_n words, zero_stride ints apart, with a grid-stride loop over B x 192 threads: exactly those"""
    rs = np.random.RandomState(zero_n + B)
    ids, lens, _ = _state(rs, B)
    words = (zero_n - 1) * zero_stride + 1 + 64
    buf = torch.full((words,), 7, dtype=torch.int32, device=G.DEV)
    o = _step(G, B, ids, lens, zero=buf, zero_n=zero_n, zero_stride=zero_stride)
    want = np.full(words, 7, np.int32)
    want[np.arange(zero_n) * zero_stride] = 0
    assert np.array_equal(buf.cpu().numpy(), want)
    assert np.array_equal(o["x"], np.stack([_embed_ref(ids[b, lens[b] - 1], False) for b in range(B)]))


# ---- (e) prefill_prep32_k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_map", [False, True], ids=["identity", "row_map"])
@pytest.mark.parametrize("slot0", [0, 5])
@pytest.mark.parametrize("q_per_b", [1, 7, 23])
@pytest.mark.parametrize("M", [1, 16, 17, 161])
def test_prefill_prep32(G, M, q_per_b, slot0, with_map):
    """prompt rows of the parity mode: the packed f32 copy and the descriptor of every row (utterance m / q_per_b through the row map,
    KV slot slot0 + m % q_per_b) exact; pad rows of the last tile and the descriptors behind M untouched"""
    rs = np.random.RandomState(M * 31 + q_per_b + slot0)
    nb = (M + q_per_b - 1) // q_per_b
    slots = nb + 3
    row_map = rs.permutation(slots)[:nb].astype(np.int32) if with_map else None
    ks = rs.randint(0, slot0 + q_per_b + 2, size=slots).astype(np.int32)      # some in front of the chunk, some inside, some behind it
    x = rs.standard_normal((M, HID)).astype(f32)
    Mp = _ceil16(M)
    xp = torch.full((Mp * HID,), float("nan"), dtype=torch.float32, device=G.DEV)
    desc = torch.full((M + 8, 4), G.CANARY32, dtype=torch.int32, device=G.DEV)
    keep = [G.dev(x), G.dev(ks), None if row_map is None else G.dev(row_map)]
    _lib.check(_lib.lib().ctts_k_prefill_prep32(keep[0].data_ptr(), xp.data_ptr(), desc.data_ptr(), q_per_b, slot0, keep[1].data_ptr(),
                                                _lib.ptr(keep[2]), M, None), "ctts_k_prefill_prep32")
    torch.cuda.synchronize()
    got = E.unpack_frag32(xp.cpu(), Mp, HID).numpy()
    assert np.array_equal(got[:M], x) and np.isnan(got[M:]).all()
    want = []
    for m in range(M):
        bq = m // q_per_b
        b = int(row_map[bq]) if with_map else bq
        want.append(list(G.row_desc(b, slot0 + m - bq * q_per_b, ks[b])))
    d = desc.cpu().numpy()
    assert d[:M].tolist() == want
    assert (d[M:] == G.CANARY32).all()


# ---- (f) prefill_compact_k ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 19])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 193, 400])     # the prefix sum over the utterances in front: 3 waves, a 192 stride
def test_prefill_compact(G, B, T):
    """the prompt pass over the valid tokens only: utterance b's slots kv_start[b] .. T-1 gathered in order behind those of the
    utterances in front of it, descriptors {b, ks + j, j, ks}, last_row exact, rows of x behind the valid count untouched.
    kv_start[b] == T (an utterance without a valid token) is outside the kernel's contract -- engine.py refuses an empty prompt row
    before anything is launched -- and is not tested."""
    rs = np.random.RandomState(B * 5 + T)
    ks = rs.randint(0, T, size=B).astype(np.int32)
    ks[rs.randint(0, B)] = T - 1                                               # exactly one valid token
    emb = rs.standard_normal((B, T, HID)).astype(f32)
    n = int((T - ks).sum())
    x = torch.full((B * T, HID), float("nan"), dtype=torch.float32, device=G.DEV)
    desc = torch.full((B * T, 4), G.CANARY32, dtype=torch.int32, device=G.DEV)
    last = torch.full((B,), G.CANARY32, dtype=torch.int32, device=G.DEV)
    keep = [G.dev(emb), G.dev(ks)]
    _lib.check(_lib.lib().ctts_k_prefill_compact(keep[0].data_ptr(), x.data_ptr(), desc.data_ptr(), last.data_ptr(), B, T, keep[1].data_ptr(),
                                                 None), "ctts_k_prefill_compact")
    torch.cuda.synchronize()
    want_x = np.concatenate([emb[b, ks[b]:] for b in range(B)], 0)
    want_desc = [[b, int(ks[b]) + j, j, int(ks[b])] for b in range(B) for j in range(T - ks[b])]
    got_x, got_d = x.cpu().numpy(), desc.cpu().numpy()
    assert np.array_equal(got_x[:n], want_x) and np.isnan(got_x[n:]).all()
    assert got_d[:n].tolist() == want_desc and (got_d[n:] == G.CANARY32).all()
    assert np.array_equal(last.cpu().numpy(), np.cumsum(T - ks) - 1)

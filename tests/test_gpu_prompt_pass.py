"""The perf-mode prompt pass kernel by kernel, as run_step launches it (bf16 output, chunk offset, slot-pool row_map), on EVERY row:
attention (attention_prefill_mfma_k from 128 rows per group, the one-wave attention_k below) against the float64 oracle and its derived
bounds (tests/prompt_pass_oracle.py), its mask by exact invariances -- a norm-wise bound has little power against a mask that is off by
one key once the softmax is peaked --, and the fused QKV + RoPE + KV append (gemm_fast_k, both tile sizes of gemm_prefill_k) against
float64, with every cache cell it must not touch under a canary.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib  # noqa: E402
from oracle import llama_np  # noqa: E402
from tests import prompt_pass_cases as PC  # noqa: E402
from tests import prompt_pass_oracle as PO  # noqa: E402

f32 = np.float32
H = PO.H
UNUSED_KV_START = 1 << 20      # kv_start of a pool slot no row group maps to: never read


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    """bit for bit, on the device"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def attn(G, q_d, kc, vc, ks_d, T, slot0, out_bf16=0, row_map=None):
    """one prompt-pass attention launch -> [M, 768] f32 / bf16 device tensor; everything that keeps the launch inside its buffers is
    checked here, in front of it"""
    M, (slots, nh, cmax, hd) = q_d.shape[0], kc.shape
    assert q_d.dtype == torch.float32 and q_d.shape[1] == 3 * H and q_d.is_contiguous() and M % T == 0 and T >= 2
    assert kc.dtype == vc.dtype == torch.bfloat16 and vc.shape == kc.shape and (nh, hd) == (PO.NH, PO.HD)
    assert kc.is_contiguous() and vc.is_contiguous() and 0 <= slot0 and slot0 + T <= cmax
    assert ks_d.dtype == torch.int32 and ks_d.numel() == slots
    rm_d = None
    if row_map is None:
        assert M // T <= slots
    else:
        assert len(row_map) == M // T and 0 <= min(row_map) and max(row_map) < slots
        rm_d = G.dev(np.asarray(row_map, np.int32))
    out = torch.full((M, H), float("nan"), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=G.DEV)
    _lib.check(_lib.lib().ctts_k_attention_prefill_ex(q_d.data_ptr(), kc.data_ptr(), vc.data_ptr(), cmax, out.data_ptr(), out_bf16, T, slot0,
                                                      ks_d.data_ptr(), _lib.ptr(rm_d), M, None), "attention_prefill_ex")
    torch.cuda.synchronize()
    return out


_dev = {}


def on_device(G, c):
    """(q, K cache, V cache, kv_start) of a case on the device and its two base launches (f32 out, bf16 out), made once; read-only"""
    if c.name not in _dev:
        q, K, V, ks = PC.inputs(c)
        q_d, kc, vc, ks_d = G.dev(q.copy()), G.dev(K.copy(), torch.bfloat16), G.dev(V.copy(), torch.bfloat16), G.dev(ks.copy())   # (the case's arrays are read-only)
        o32 = attn(G, q_d, kc, vc, ks_d, c.T, c.slot0, 0)
        o16 = attn(G, q_d, kc, vc, ks_d, c.T, c.slot0, 1)
        _dev[c.name] = (q_d, kc, vc, ks_d, o32, o16)
    return _dev[c.name]


def fresh(G, shape, seed, scale=1.0):
    """finite replacement values: N(0, scale^2) as a device tensor of bf16 values"""
    return G.dev((np.random.RandomState(seed).standard_normal(shape) * scale).astype(f32), torch.bfloat16)


case_param = pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.name)


# ---- 1, 2: every row against float64, in both output types ------------------------------------------------------------------------
@case_param
def test_attention_every_row_within_the_derived_bound(G, c):
    """all valid rows of the f32-out launch within the kernel's bound; pad rows (which see only themselves) finite"""
    o32 = on_device(G, c)[4].cpu().numpy()
    r = PC.answer(c)
    kern = PO.kernel_of(c.T)
    assert np.isfinite(o32).all()
    ratio = PO.worst_ratio(o32, r, kern)
    print(f"{c.name}: {kern} f32 out, worst |err| / bound = {ratio:.3f} over {int(r['valid'].sum())} rows")
    assert ratio <= 1.0, (c.name, ratio)


@case_param
def test_attention_shipped_bf16_output_is_the_rounded_f32_output(G, c):
    """the instantiation the prompt pass ships (bf16 out) differs from its f32 sibling in store_out only: its output is the f32 output
    rounded to nearest even, bit for bit on every row -- and inside the bf16-out bound"""
    o32, o16 = on_device(G, c)[4:6]
    got16 = o16.float().cpu().numpy()
    assert got16.tobytes() == G.bf16_round(o32.cpu().numpy()).tobytes()
    r = PC.answer(c)
    kern = PO.kernel_of(c.T)
    ratio = PO.worst_ratio(got16, r, kern, out_bf16=True)
    print(f"{c.name}: {kern} bf16 out, worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (c.name, ratio)


# ---- 3, 4, 5: the mask by exact invariances -----------------------------------------------------------------------------------------
@case_param
@pytest.mark.parametrize("out_bf16", [0, 1])
def test_attention_causality_by_perturbation(G, c, out_bf16):
    """everything at slots >= s* replaced (K, V x 1000 in the cache, the rows of qkv): the rows in front of s* keep their bits"""
    q_d, kc, vc, ks_d = on_device(G, c)[:4]
    base = on_device(G, c)[4 + out_bf16].view(PC.groups(c), c.T, H)
    newK, newV = fresh(G, kc.shape, 100 + c.seed), fresh(G, kc.shape, 200 + c.seed, 1000.0)
    newq = G.dev((np.random.RandomState(300 + c.seed).standard_normal(q_d.shape) * c.qscale).astype(f32))
    for r in PC.cuts(c):
        k2, v2, q2 = kc.clone(), vc.clone(), q_d.clone()
        k2[:, :, c.slot0 + r:] = newK[:, :, c.slot0 + r:]
        v2[:, :, c.slot0 + r:] = newV[:, :, c.slot0 + r:]
        q2.view(PC.groups(c), c.T, 3 * H)[:, r:] = newq.view(PC.groups(c), c.T, 3 * H)[:, r:]
        got = attn(G, q2, k2, v2, ks_d, c.T, c.slot0, out_bf16).view(PC.groups(c), c.T, H)
        assert same(got[:, :r].contiguous(), base[:, :r].contiguous()), (c.name, "cut at slot0 +", r)
        assert not same(got[:, r:].contiguous(), base[:, r:].contiguous())        # the replacement did reach the kernel


@case_param
def test_attention_left_pad_by_perturbation(G, c):
    """every cache row below kv_start[b] replaced: the valid rows keep their bits"""
    q_d, kc, vc, ks_d, o32, o16 = on_device(G, c)
    k2, v2 = kc.clone(), vc.clone()
    newK, newV = fresh(G, kc.shape, 400 + c.seed), fresh(G, kc.shape, 500 + c.seed, 1000.0)
    for b, k in enumerate(c.kv_start):
        k2[b, :, :k] = newK[b, :, :k]
        v2[b, :, :k] = newV[b, :, :k]
    valid = G.dev(PC.answer(c)["valid"])
    for out_bf16, base in ((0, o32), (1, o16)):
        got = attn(G, q_d, k2, v2, ks_d, c.T, c.slot0, out_bf16)
        assert same(got[valid], base[valid]), (c.name, out_bf16)


@case_param
def test_attention_utterances_are_independent(G, c):
    """one utterance's cache and q replaced: the other utterances keep their bits, this one does not"""
    q_d, kc, vc, ks_d, o32, o16 = on_device(G, c)
    u, Gn = 1, PC.groups(c)
    k2, v2, q2 = kc.clone(), vc.clone(), q_d.clone()
    k2[u], v2[u] = fresh(G, kc.shape[1:], 600 + c.seed), fresh(G, kc.shape[1:], 700 + c.seed, 1000.0)
    q2.view(Gn, c.T, 3 * H)[u] = G.dev(np.random.RandomState(800 + c.seed).standard_normal((c.T, 3 * H)).astype(f32))
    others = [g for g in range(Gn) if g != u]
    for out_bf16, base in ((0, o32), (1, o16)):
        got = attn(G, q2, k2, v2, ks_d, c.T, c.slot0, out_bf16).view(Gn, c.T, H)
        assert same(got[others], base.view(Gn, c.T, H)[others]), (c.name, out_bf16)
        assert not same(got[u], base.view(Gn, c.T, H)[u])


# ---- 6: chunks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kvs,chunks,qscale", PC.CHUNKED, ids=[x[0] for x in PC.CHUNKED])
def test_attention_chunked_prompt_equals_whole(G, name, kvs, chunks, qscale):
    """A prompt run as one launch and as chunks (slot0 > 0, the keys below it from the cache) gives the same bits on every valid row
    wherever both take the same kernel: the MFMA kernel's key blocks sit on absolute multiples of 32 and a block without a visible key
    is a no-op; the one-wave kernel walks a row's keys from the row's own first visible key"""
    T, Gn = sum(chunks), len(kvs)
    q, K, V = PC.make_inputs(Gn, T, 0, T + 5, kvs, qscale, 900 + T + len(chunks))
    q_d, kc, vc, ks_d = G.dev(q), G.dev(K, torch.bfloat16), G.dev(V, torch.bfloat16), G.dev(np.asarray(kvs, np.int32))
    valid = G.dev(np.arange(T)[None, :] >= np.asarray(kvs)[:, None])               # [G, T]
    for out_bf16 in (0, 1):
        whole = attn(G, q_d, kc, vc, ks_d, T, 0, out_bf16).view(Gn, T, H)
        assert bool(torch.isfinite(whole.float()).all())
        c0 = 0
        for n in chunks:
            qc = q_d.view(Gn, T, 3 * H)[:, c0: c0 + n].reshape(Gn * n, 3 * H).contiguous()
            got = attn(G, qc, kc, vc, ks_d, n, c0, out_bf16).view(Gn, n, H)
            v = valid[:, c0: c0 + n]
            assert int(v.sum()) > 0
            assert same(got[v], whole[:, c0: c0 + n][v]), (name, out_bf16, "chunk at", c0)
            c0 += n


# ---- 7: pool slots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t145_s32", "t129_s33", "t33_s200", "t127_s3"])
def test_attention_pool_slots_through_row_map(G, name):
    """row groups mapped into a 7-slot cache by row_map, kv_start indexed by slot, the unused slots NaN with an absurd kv_start: the
    same bits as the identity launch on cache[row_map], kv_start[row_map]"""
    c = PC.BY_NAME[name]
    q_d, kc, vc, ks_d, o32, o16 = on_device(G, c)
    row_map = [5, 0, 3, 6][: PC.groups(c)]
    pk = torch.full((7,) + tuple(kc.shape[1:]), float("nan"), dtype=torch.bfloat16, device=G.DEV)
    pv = pk.clone()
    ks = np.full(7, UNUSED_KV_START, np.int32)
    for g, s in enumerate(row_map):
        pk[s], pv[s], ks[s] = kc[g], vc[g], c.kv_start[g]
    for out_bf16, base in ((0, o32), (1, o16)):
        got = attn(G, q_d, pk, pv, G.dev(ks), c.T, c.slot0, out_bf16, row_map=row_map)
        assert same(got, base), (name, out_bf16)


# ---- 8, 9, 10: QKV + RoPE + KV append ------------------------------------------------------------------------------------------------
QKV_SHAPES = ((3, 23), (4, 64), (3, 86), (7, 256), (11, 163))    # groups x rows: M = 69 gemm_fast_k | 256 first M on prefill.hip | 258 ragged last
QKV_M_MAX = 1793                                                  # 64-row tile | 1792 largest launch on 64-row tiles | 1793 128-row tiles
SHIFT = 37
_qkv = {}


def qkv_common(G):
    """the rows, the weights and the float64 projection of the largest shape, once: every shape takes a prefix of the rows"""
    if "common" not in _qkv:
        from chattts_amd.engine import rope_row_perm, rope_tables
        rs = np.random.RandomState(23)
        x32 = (rs.standard_normal((QKV_M_MAX, H)) * 1.5).astype(f32)
        W = G.bf16_round((rs.standard_normal((3 * H, H)) * 0.05).astype(f32))
        perm = rope_row_perm().numpy()
        Wp = np.concatenate([W[:H][perm], W[H:2 * H][perm], W[2 * H:]], 0)
        xb = torch.empty((QKV_M_MAX, H), dtype=torch.bfloat16, device=G.DEV)
        ssq = torch.empty((QKV_M_MAX, 48), dtype=torch.float32, device=G.DEV)
        _lib.check(_lib.lib().ctts_k_rows_prep(G.dev(x32).data_ptr(), xb.data_ptr(), ssq.data_ptr(), QKV_M_MAX, None), "rows_prep")
        torch.cuda.synchronize()
        rstd = 1.0 / np.sqrt((x32.astype(np.float64) ** 2).mean(1, keepdims=True) + 1e-6)
        y = (G.bf16_round(x32).astype(np.float64) @ W.astype(np.float64).T) * rstd          # test_qkv_rope_fused's reference
        cos, sin = rope_tables(512)
        _qkv["common"] = dict(xb=xb, ssq=ssq, Wp=G.dev(Wp, torch.bfloat16), cos=G.dev(cos), sin=G.dev(sin), y=y)
    return _qkv["common"]


def qkv_launch(G, Gn, Tc, slot0, ks_pool, row_map, pool, cmax):
    """one fused launch over Gn x Tc rows into canary-filled caches -> (q [M, 768] f32, K cache, V cache [pool, 12, cmax, 64] int16 bits)"""
    cm = qkv_common(G)
    M = Gn * Tc
    assert M <= QKV_M_MAX and len(row_map) == Gn and len(set(row_map)) == Gn and 0 <= min(row_map) and max(row_map) < pool
    assert 0 <= slot0 and slot0 + Tc <= cmax and len(ks_pool) == pool and slot0 + Tc < cm["cos"].shape[0]
    qkv = torch.full((M, 3 * H), G.CANARY32, dtype=torch.int32, device=G.DEV).view(torch.float32)
    kc = torch.full((pool, PO.NH, cmax, PO.HD), G.CANARY16, dtype=torch.int16, device=G.DEV).view(torch.bfloat16)
    vc = kc.clone()
    ks_d, rm_d = G.dev(np.asarray(ks_pool, np.int32)), G.dev(np.asarray(row_map, np.int32))
    _lib.check(_lib.lib().ctts_k_qkv_rope_ex(cm["xb"].data_ptr(), cm["Wp"].data_ptr(), M, cm["ssq"].data_ptr(), 1e-6, qkv.data_ptr(),
                                             kc.data_ptr(), vc.data_ptr(), cmax, cm["cos"].data_ptr(), cm["sin"].data_ptr(), Tc, None,
                                             ks_d.data_ptr(), slot0, rm_d.data_ptr(), 0, None), "qkv_rope_ex")
    torch.cuda.synchronize()
    return qkv[:, :H].contiguous(), kc, vc


def qkv_runs(G, shape):
    """the three launches of a shape and its float64 answer, once:
         A  slot0 = 0,  kv_start,      map A       B  slot0 = 37, kv_start + 37, map A       C  slot0 = 0, kv_start, another map"""
    if shape not in _qkv:
        Gn, Tc = shape
        M, pool, cmax = Gn * Tc, Gn + 2, SHIFT + Tc + 3
        rs = np.random.RandomState(Gn * 1000 + Tc)
        ks = np.array([(3 * g + 2 * (g % 2)) % 7 for g in range(Gn)])                # 0, 5, 6, 4, ...: pad rows in most groups
        mapA = rs.permutation(pool)[:Gn]
        mapC = np.roll(mapA, 1)
        assert (mapA != np.arange(Gn)).any() and (mapC != mapA).all()
        runs = {}
        for tag, slot0, shift, rmap in (("A", 0, 0, mapA), ("B", SHIFT, SHIFT, mapA), ("C", 0, 0, mapC)):
            ks_pool = np.full(pool, UNUSED_KV_START)
            ks_pool[rmap] = ks + shift
            runs[tag] = (slot0, rmap) + qkv_launch(G, Gn, Tc, slot0, ks_pool, rmap.tolist(), pool, cmax)
        # float64 answer per row (the same for all three: the rotary position is slot - kv_start, 1 on a pad row)
        pos = np.arange(Tc)[None, :] - ks[:, None]
        pos = np.where(pos < 0, 1, pos).reshape(M)
        inv_freq = (1.0 / (10000.0 ** (np.arange(0, PO.HD, 2, dtype=np.float64) / PO.HD))).astype(f32)
        c, s = llama_np.rope_tables(pos, inv_freq)                                   # [M, 64]
        y = qkv_common(G)["y"][:M]

        def rope(v):
            v = v.reshape(M, PO.NH, PO.HD)
            rot = np.concatenate([-v[..., PO.HD // 2:], v[..., : PO.HD // 2]], -1)
            return v * c[:, None].astype(np.float64) + rot * s[:, None].astype(np.float64)
        _qkv[shape] = (runs, rope(y[:, :H]), rope(y[:, H:2 * H]), y[:, 2 * H:].reshape(M, PO.NH, PO.HD), ks)
    return _qkv[shape]


def cache_rows(cache, rmap, slot0, Gn, Tc):
    """the addressed cells of a cache as [Gn, Tc, 12, 64] (row order of the launch)"""
    return cache[torch.as_tensor(np.asarray(rmap), device=cache.device)][:, :, slot0: slot0 + Tc].permute(0, 2, 1, 3).contiguous()


shape_param = pytest.mark.parametrize("shape", QKV_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


@shape_param
@pytest.mark.parametrize("tag", ["A", "B"])
def test_qkv_rope_append_against_float64(G, shape, tag):
    """q within test_qkv_rope_fused's tolerance of its float64 reference on every row; the cache within 2^-8 |ref| plus that tolerance:
    the bf16 rounding of a value that is itself within the tolerance"""
    runs, rq, rk, rv, _ = qkv_runs(G, shape)
    Gn, Tc = shape
    M = Gn * Tc
    slot0, rmap, q, kc, vc = runs[tag]
    tol = lambda ref: 2e-4 * np.maximum(1.0, np.abs(ref).reshape(M, -1).max(1))[:, None, None]      # per row, as test_qkv_rope_fused
    got_q = q.cpu().numpy().astype(np.float64).reshape(M, PO.NH, PO.HD)
    eq = np.abs(got_q - rq) / tol(rq)
    worst = [float(eq.max())]
    assert eq.max() < 1.0, (shape, tag, "q", np.unravel_index(eq.argmax(), eq.shape))
    for what, cache, ref in (("k", kc, rk), ("v", vc, rv)):
        got = cache_rows(cache, rmap, slot0, Gn, Tc).float().cpu().numpy().astype(np.float64).reshape(M, PO.NH, PO.HD)
        e = np.abs(got - ref) / (2.0 ** -8 * np.abs(ref) + tol(ref))
        worst.append(float(e.max()))
        assert e.max() <= 1.0, (shape, tag, what, np.unravel_index(e.argmax(), e.shape))
    print(f"qkv {Gn}x{Tc} {tag}: worst |err| / bound q {worst[0]:.3f}, k {worst[1]:.3f}, v {worst[2]:.3f}")


@shape_param
def test_qkv_rope_append_leaves_every_other_cell_alone(G, shape):
    """the caches start as canaries: every cell outside the addressed (row_map[g], head, slot0 + t) set still holds one, every addressed
    cell was written"""
    runs = qkv_runs(G, shape)[0]
    Gn, Tc = shape
    for tag, (slot0, rmap, q, kc, vc) in runs.items():
        addressed = torch.zeros((kc.shape[0], kc.shape[2]), dtype=torch.bool, device=kc.device)
        addressed[torch.as_tensor(rmap, device=kc.device), slot0: slot0 + Tc] = True
        assert int(addressed.sum()) == Gn * Tc
        for cache in (kc, vc):
            cells = bits(cache).permute(0, 2, 1, 3)                                  # [pool, cmax, 12, 64]
            assert bool((cells[~addressed] == G.CANARY16).all()), (shape, tag)
            assert bool((cells[addressed] != G.CANARY16).all()) and bool(torch.isfinite(cache.permute(0, 2, 1, 3)[addressed].float()).all())
        assert bool(torch.isfinite(q).all())


@shape_param
def test_qkv_rope_append_shift_and_relocation(G, shape):
    """(slot0 = s, kv_start + s) gives the same q bits, and the same K / V bits s slots later, as (0, kv_start); another row_map moves the
    same bits to the slots it names"""
    runs = qkv_runs(G, shape)[0]
    Gn, Tc = shape
    s0, mA, qA, kA, vA = runs["A"]
    for tag in ("B", "C"):
        s1, m1, q1, k1, v1 = runs[tag]
        assert same(q1, qA), (shape, tag, "q")
        assert same(cache_rows(k1, m1, s1, Gn, Tc), cache_rows(kA, mA, s0, Gn, Tc)), (shape, tag, "k")
        assert same(cache_rows(v1, m1, s1, Gn, Tc), cache_rows(vA, mA, s0, Gn, Tc)), (shape, tag, "v")

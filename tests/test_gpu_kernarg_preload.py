"""The decode step's kernels take what their first loads need as leading plain parameters, which the dispatcher preloads into user
SGPRs; the struct they used to take alone follows.  What can go wrong is an argument landing in the wrong place:
a swapped pair of pointers, a count taken for a stride, or -- the preload's own failure -- SGPRs that still hold the values of the
neighbouring dispatch.  Every converted kernel is therefore run through its C-ABI kernel entry at the smallest shapes at which its
arguments differ from one another, and each case makes two checks:

  (a) the result equals the float64 numpy value under the tolerance tests/test_gpu_kernels.py uses for that kernel;
  (b) two nodes of the SAME kernel with DIFFERENT buffers, captured back to back into one linear graph on one stream and replayed
      twice, each give exactly the bits of their own eager launch (outputs refilled between replays: rows a launch must not touch
      are part of the comparison).

The QKV + RoPE epilogue of gemm_dec32x_k has no kernel entry of its own (the C ABI is unchanged); its shape -- the RMSNorm launch with
K = 768 and N = 2304 -- runs here with the gate/up epilogue, which takes the same leading arguments, and the epilogue itself is
pinned bit for bit by the decode-step tests of tests/test_gpu_e2e.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, rng  # noqa: E402
from oracle import sampling_np  # noqa: E402

f32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


class _Set:
    """one launch with buffers of its own: launch(stream), the tensors it writes, their state before the launch"""

    def __init__(self, launch, outs, keep=()):
        self.launch, self.outs, self.keep = launch, outs, keep
        self.init = [o.clone() for o in outs]

    def reset(self):
        for o, i in zip(self.outs, self.init):
            o.copy_(i)


def _eager(sets):
    for s in sets:
        s.reset()
    for s in sets:
        s.launch(None)
    torch.cuda.synchronize()
    return [[_bits(o) for o in s.outs] for s in sets]


def _graph_matches_eager(sets, eager_bits):
    """check (b): the sets' launches as consecutive nodes of one captured graph, replayed twice"""
    for s in sets:
        s.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        for s in sets:
            s.launch(st)
    for rep in range(2):
        for s in sets:
            s.reset()
        g.replay()
        torch.cuda.synchronize()
        for i, s in enumerate(sets):
            for j, o in enumerate(s.outs):
                assert torch.equal(_bits(o), eager_bits[i][j]), ("graph node differs from its eager launch", rep, i, j)


# ------------------------------------------------------------------------------------------------
# projections of the f32x3 step (gemm_dec32x_k)
# ------------------------------------------------------------------------------------------------
def _x3_set(G, seed, M, n_act, N, K, epi):
    from chattts_amd.engine import X3_LO_SCALE, pack_frag, pack_frag_x3, split_f16, unpack_frag, unpack_frag32
    lib = _lib.lib()
    rs = np.random.RandomState(seed)
    rms = epi == 2
    Mp = (M + 15) // 16 * 16
    live = M if n_act is None else n_act
    na_d = None if n_act is None else G.dev(np.array([n_act], np.int32))
    A = (rs.standard_normal((M, K)) * (2.0 if rms else 1.0)).astype(f32)
    nrows = 2 * N if epi == 2 else N
    Wm = (rs.standard_normal((nrows, K)) * 0.03).astype(f32)
    res = rs.standard_normal((M, N)).astype(f32) if epi == 1 else None
    Apad = np.full((Mp, K), np.nan, f32)          # pad rows = NaN: they must never reach a live output
    Apad[:M] = A
    ah, al = split_f16(torch.from_numpy(Apad))
    planes_a = torch.stack([pack_frag(ah), pack_frag(al)], 0).contiguous().to(G.DEV)
    planes_w = pack_frag_x3(torch.from_numpy(Wm)).to(G.DEV)
    Cc = torch.full((M, N), NAN, dtype=torch.float32, device=G.DEV)
    Cp = torch.full((2, Mp * N), NAN, dtype=torch.float32, device=G.DEV).to(torch.bfloat16)
    Cp32 = torch.full((Mp * N,), NAN, dtype=torch.float32, device=G.DEV) if epi == 1 else None
    res_d = None if res is None else G.dev(res)
    ssq_in = G.dev((A.reshape(M, 48, 16).astype(np.float64) ** 2).sum(-1).astype(f32)) if rms else None   # the decode step's way
    ssq_out = torch.full((M, 48), NAN, dtype=torch.float32, device=G.DEV) if epi == 1 else None

    def launch(st):
        _lib.check(lib.ctts_k_gemm_dec32x(planes_a.data_ptr(), Mp * K, planes_w.data_ptr(), nrows * K, M, N, K, _lib.ptr(na_d), None, K, 1e-6, epi,
                                          Cc.data_ptr() if epi == 1 else None, N, _lib.ptr(res_d), N, Cp.data_ptr(), Mp * N, N // 32, _lib.ptr(Cp32), 0,
                                          _lib.ptr(ssq_in), _lib.ptr(ssq_out), st), "dec32x")

    def check():   # (a): tests/test_gpu_kernels.py test_gemm_dec32x_split_bf16, its float64 models and its bounds
        a_h, a_l = (x.float().numpy().astype(np.float64)[:live] for x in split_f16(torch.from_numpy(A)))
        w_h, w_l = (x.float().numpy().astype(np.float64) for x in split_f16(torch.from_numpy(Wm)))
        a_l, w_l = a_l / X3_LO_SCALE, w_l / X3_LO_SCALE
        exact = (a_h + a_l) @ (w_h + w_l).T - a_l @ w_l.T
        full = A[:live].astype(np.float64) @ Wm.astype(np.float64).T
        if rms:
            rstd = 1.0 / np.sqrt((A[:live].astype(np.float64) ** 2).mean(1, keepdims=True) + 1e-6)
            exact, full = exact * rstd, full * rstd
        if epi == 2:
            sil = lambda v: v / (1.0 + np.exp(-v))
            exact, full = sil(exact[:, :N]) * exact[:, N:], sil(full[:, :N]) * full[:, N:]
        else:
            exact, full = exact + res[:live], full + res[:live]
        got_planes = (unpack_frag(Cp[0].view(torch.float16).float().cpu(), Mp, N).numpy().astype(np.float64)
                      + unpack_frag(Cp[1].view(torch.float16).float().cpu(), Mp, N).numpy() / X3_LO_SCALE)
        scale = np.abs(full).max()
        if epi == 1:
            got = Cc.cpu().numpy()
            e_exact, e_full = np.abs(got[:live] - exact).max() / scale, np.abs(got[:live] - full).max() / scale
            print(f"dec32x M={M} live={live} N={N} K={K} epi={epi}: vs split model {e_exact:.3g}, vs float64 {e_full:.3g} (bound 5e-6)")
            assert np.isnan(got[live:]).all()                       # rows at or beyond the live count stay untouched
            assert e_exact < 5e-6 and e_full < 5e-6, (M, N, K, e_exact, e_full)
            assert np.array_equal(unpack_frag32(Cp32.cpu(), Mp, N).numpy()[:live], got[:live])
            assert np.abs(got_planes[:live] - got[:live]).max() < 2e-6 * scale
            sq = ssq_out.cpu().numpy()
            want_sq = (got[:live].astype(np.float64).reshape(live, N // 16, 16) ** 2).sum(-1)
            assert np.abs(sq[:live, : N // 16] - want_sq).max() < 1e-5 * want_sq.max()
            assert np.isnan(sq[live:]).all() and np.isnan(sq[:, N // 16:]).all()
        else:
            e_exact = np.abs(got_planes[:live] - exact).max() / scale
            print(f"dec32x M={M} live={live} N={N} K={K} epi={epi}: vs split model {e_exact:.3g} (bound 5e-6)")
            assert e_exact < 5e-6, (M, N, K, e_exact)
        assert np.isnan(got_planes[live:M]).all()

    s = _Set(launch, [t for t in (Cc, Cp, Cp32, ssq_out) if t is not None], keep=(planes_a, planes_w, res_d, ssq_in, na_d))
    s.check = check
    return s


X3_SHAPES = [(32, 768, 1), (32, 3072, 1), (32, 768, 2), (2304, 768, 2)]   # (N, K, epi): o_proj-, down-, gate/up-like; the QKV shape (docstring)


@pytest.mark.parametrize("M,n_act", [(1, None), (17, None), (64, None), (64, 17)])
@pytest.mark.parametrize("shape", X3_SHAPES)
def test_projection_arguments_land_where_they_belong(G, shape, M, n_act):
    N, K, epi = shape
    sets = [_x3_set(G, 1000 * i + M * 7 + N + K + epi + (n_act or 0), M, n_act, N, K, epi) for i in (1, 2)]
    eager = _eager(sets)
    for s in sets:
        s.check()
    _graph_matches_eager(sets, eager)


# ------------------------------------------------------------------------------------------------
# decode attention of the f32x3 step (attention_k<float, 4, x3p_t>: f32 KV cache, packed split output)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kv_cache(G):
    rs = np.random.RandomState(77)
    B, nh, cmax, d = 4, 12, 320, 64
    Kc = rs.standard_normal((B, nh, cmax, d)).astype(f32)
    Vc = rs.standard_normal((B, nh, cmax, d)).astype(f32)
    return Kc, Vc, G.dev(Kc), G.dev(Vc), cmax


def _att_set(G, kv_cache, seed, rows, covers_all, n_active):
    """rows: (b, first visible key, newest key) per compact row, b = -1: absent"""
    from chattts_amd.engine import X3_LO_SCALE, unpack_frag
    lib = _lib.lib()
    Kc, Vc, kc_d, vc_d, cmax = kv_cache
    rs = np.random.RandomState(seed)
    M, H, nh, d = len(rows), 768, 12, 64
    Mp = (M + 15) // 16 * 16
    desc = np.zeros((M, 4), np.int32)
    for m, (b, jlo, slot) in enumerate(rows):
        desc[m] = (b, slot, slot - jlo, jlo)
    qkv = rs.standard_normal((M, 3 * H)).astype(f32)
    q_d, desc_d = G.dev(qkv), G.dev(desc)
    na_d = None if n_active is None else G.dev(np.array([n_active], np.int32))
    pl = torch.full((2, Mp * H), NAN, dtype=torch.float32, device=G.DEV).to(torch.bfloat16)

    def launch(st):
        _lib.check(lib.ctts_k_attention_dec2(q_d.data_ptr(), kc_d.data_ptr(), vc_d.data_ptr(), 2, cmax, pl.data_ptr(), desc_d.data_ptr(),
                                             _lib.ptr(na_d), covers_all, M, st), "attention_dec2")

    def check():   # (a): the float64 softmax(q K^T / 8 + mask) V of test_attention_decode_persistent_grid, its f32 bound
        got = (unpack_frag(pl[0].view(torch.float16).float().cpu(), Mp, H).numpy().astype(np.float64)
               + unpack_frag(pl[1].view(torch.float16).float().cpu(), Mp, H).numpy() / X3_LO_SCALE)
        live = [m for m, r in enumerate(rows) if r[0] >= 0 and (n_active is None or m < n_active)]
        for m in live:
            b, jlo, slot = rows[m]
            q = qkv[m, :H].reshape(nh, d).astype(np.float64)
            Kb, Vb = Kc[b, :, jlo: slot + 1].astype(np.float64), Vc[b, :, jlo: slot + 1].astype(np.float64)
            sc = np.einsum("hd,hjd->hj", q, Kb) * 0.125
            pr = np.exp(sc - sc.max(-1, keepdims=True))
            pr /= pr.sum(-1, keepdims=True)
            ref = np.einsum("hj,hjd->hd", pr, Vb).reshape(H)
            err = np.abs(got[m] - ref).max()
            print(f"attention row {m} ({slot + 1 - jlo} keys): {err:.3g} (bound 2e-5)")
            assert err < 2e-5, (m, err)
        untouched = [m for m in range(Mp) if m not in live]
        assert np.isnan(got[untouched]).all()

    s = _Set(launch, [pl], keep=(q_d, desc_d, na_d))
    s.check = check
    return s


def test_attention_arguments_land_where_they_belong(G, kv_cache):
    """3 utterances with contexts of 1, 5 and 300 keys and an absent row (b = -1): once with descriptors that cover every row, once
    behind a device-side live-row count with a stale descriptor beyond it"""
    try:
        _lib.check(_lib.lib().ctts_k_attention_cfg(0, 0, 0), "attention_cfg")    # one workgroup per (utterance, head): attention_k
        sets = [_att_set(G, kv_cache, 5, [(2, 3, 302), (0, 0, 4), (-1, 0, 0), (3, 7, 7)], 1, None),
                _att_set(G, kv_cache, 6, [(1, 10, 309), (-1, 0, 0), (3, 20, 24), (0, 5, 5), (2, 0, 100)], 0, 4)]
        eager = _eager(sets)
        for s in sets:
            s.check()
        _graph_matches_eager(sets, eager)
    finally:
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        _lib.check(_lib.lib().ctts_k_attention_cfg(0, ncu, 4), "attention_cfg")


# ------------------------------------------------------------------------------------------------
# embedding, heads, sampling: 3 utterances
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emb_table(G):
    emb = np.random.RandomState(3).standard_normal((4, 626, 768)).astype(f32)
    return emb, G.dev(emb)


def _embed_set(G, emb_table, seed):
    lib = _lib.lib()
    emb, e_d = emb_table
    rs = np.random.RandomState(seed)
    B, tcap = 3, 20
    ids = rs.randint(0, 626, size=(B, tcap, 4)).astype(np.int64)
    lens = rs.randint(1, tcap + 1, size=B).astype(np.int32)
    i_d, l_d = G.dev(ids), G.dev(lens)
    x = torch.full((B, 768), NAN, dtype=torch.float32, device=G.DEV)

    def launch(st):
        _lib.check(lib.ctts_k_embed_codes(e_d.data_ptr(), i_d.data_ptr(), tcap, l_d.data_ptr(), x.data_ptr(), B, st), "embed")

    def check():   # (a): test_embed_and_final_norm -- the same k-ordered f32 adds, bit exact (so within any tolerance of the float64 sum)
        t = [ids[b, lens[b] - 1] for b in range(B)]
        ref = np.stack([((emb[0][t[b][0]] + emb[1][t[b][1]]) + emb[2][t[b][2]]) + emb[3][t[b][3]] for b in range(B)])
        ref64 = np.stack([sum(emb[k][t[b][k]].astype(np.float64) for k in range(4)) for b in range(B)])
        assert np.array_equal(x.cpu().numpy(), ref)
        assert np.abs(x.cpu().numpy() - ref64).max() < 4 * 2.0 ** -23 * np.abs(ref64).max()

    s = _Set(launch, [x], keep=(i_d, l_d))
    s.check = check
    return s


def _heads_set(G, seed):
    """the heads GEMM of the parity modes (decode32.hip, 16-row kernel): N = 2504 columns padded to 2512 weight rows, n_cols = 2504"""
    from chattts_amd.engine import pack_frag32
    lib = _lib.lib()
    rs = np.random.RandomState(seed)
    M, N, K, Np, Mp = 3, 2504, 768, 2512, 16
    A = rs.standard_normal((M, K)).astype(f32)
    W = (rs.standard_normal((N, K)) * 0.03).astype(f32)
    Apad = np.full((Mp, K), np.nan, f32)
    Apad[:M] = A
    Ap = pack_frag32(torch.from_numpy(Apad)).to(G.DEV)
    Wp = pack_frag32(torch.from_numpy(np.concatenate([W, np.zeros((Np - N, K), f32)], 0))).to(G.DEV)
    Cc = torch.full((M, N), NAN, dtype=torch.float32, device=G.DEV)

    def launch(st):
        _lib.check(lib.ctts_k_gemm_dec32(Ap.data_ptr(), Wp.data_ptr(), M, Np, K, None, None, K, None, 1e-6, 0, Cc.data_ptr(), N, None, N, None, N // 16,
                                         0, N, st), "dec32 heads")

    def check():   # (a): the f32 bound of test_gemm_skinny (the kernel test_gemm_dec32_bit_identical pins these bits to)
        err = G.relerr(Cc.cpu().numpy(), A.astype(np.float64) @ W.astype(np.float64).T)
        print(f"heads: {err:.3g} (bound 3e-6)")
        assert np.isfinite(Cc.cpu().numpy()).all() and err < 3e-6, err

    s = _Set(launch, [Cc], keep=(Ap, Wp))
    s.check = check
    return s


def _sample_set(G, seed):
    lib = _lib.lib()
    rs = np.random.RandomState(seed)
    B, V, h, T = 3, 626, 7, 1
    rows, tcap = B * 4, T + h + 2
    logits = (rs.standard_normal((rows, V)) * 2.0).astype(f32)
    hist = rs.randint(0, V, size=(rows, h)).astype(np.int64)
    hist[:, : h // 2] = np.argsort(-logits, axis=1)[:, : h // 2]
    temp4 = np.array([0.3, 0.7, 1.0, 1.5], f32)
    top_p, top_k, rep = 0.7, 20, 1.05
    q = rng.ExpDraws(rows, V, seed).step(0).numpy()
    ids = np.zeros((B, tcap, 4), np.int64)
    ids[:, T: T + h, :] = hist.reshape(B, 4, h).transpose(0, 2, 1)
    keep = []
    d = lambda a: (keep.append(G.dev(a)), keep[-1])[1]
    s = _lib.GenState()
    s.B, s.T, s.max_new = B, T, h + 2
    ids_d, len_d, fin_d, end_d = d(ids), d(np.full(B, T + h, np.int32)), d(np.zeros(B, np.uint8)), d(np.zeros(B, np.int32))
    s.ids_buf, s.len, s.finish, s.end_idx = ids_d.data_ptr(), len_d.data_ptr(), fin_d.data_ptr(), end_d.data_ptr()
    s.q, s.nq = d(q.reshape(1, rows, V)).data_ptr(), 1
    s.temperature = d(temp4).data_ptr()
    pt = rng.penalty_table(rep)
    s.pow_table = d(pt.numpy()).data_ptr()
    s.top_p_thr, s.use_top_p, s.top_k, s.use_top_k = float(np.float32(1.0 - top_p)), 1, top_k, 1
    s.min_new, s.eos, s.row_offset = 0, 625, 0
    lg = d(logits.reshape(B, 4 * V))

    def launch(st):
        _lib.check(lib.ctts_k_sample(C.byref(s), lg.data_ptr(), st), "sample")

    def check():   # (a): test_sample_randomised_vs_oracle -- the float64 oracle of the reference chain, exact token ids
        want = sampling_np.sample_step(logits, hist, q, temperature=np.tile(temp4, B), top_p=top_p, top_k=top_k, pow_table=pt.numpy(),
                                       max_input_ids=625, mask_eos=False)
        got = ids_d.cpu().numpy()[:, T + h, :].reshape(-1)
        assert np.array_equal(got, want), int((got != want).sum())
        assert (len_d.cpu().numpy() == T + h + 1).all()

    st_ = _Set(launch, [ids_d, len_d, fin_d, end_d], keep=(keep, s))
    st_.check = check
    return st_


@pytest.mark.parametrize("kernel", ["embed", "heads", "sample"])
def test_embed_heads_sample_arguments_land_where_they_belong(G, emb_table, kernel):
    make = {"embed": lambda seed: _embed_set(G, emb_table, seed), "heads": lambda seed: _heads_set(G, seed), "sample": lambda seed: _sample_set(G, seed)}[kernel]
    sets = [make(41), make(42)]
    eager = _eager(sets)
    for s in sets:
        s.check()
    _graph_matches_eager(sets, eager)

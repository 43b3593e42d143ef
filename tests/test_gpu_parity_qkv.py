"""The fused RMSNorm + QKV + RoPE + KV append epilogue of the float32 parity mode (D32_EPI_QKV_ROPE) in every kernel that runs it --
decode32.hip (`gemm_dec32_rms16_k`, `gemm_dec32_k`), prefill32.hip (`gemm_pre32_k`), decode32x.hip (RoPE factors through the
descriptor or through the per-row table of the step's first kernel) -- given row descriptors, and `gemm_pre32_k`'s two other epilogues.

The EXACT reference is the chain the parity goldens were made with: `gemm_skinny_k<float>` (G.gemm, weights in natural row order),
then `rope_append_k` into a float32 cache with one pseudo-utterance per row (len' = slot + 1, kv_start' = the row's utterance's), so
row m is roped at its descriptor's position whatever utterance and slot the fused kernel is told to write it to.  The fused kernels
get the q / k weight rows in engine.rope_row_perm() order; q, k and v of every live row must be equal bit for bit, every cache cell
no live descriptor names must still be NaN, and so must C[:, 768:].

Descriptors: the utterances a random permutation of the rows, slots non-monotone, kv_start in [0, 6) with pad rows (slot < kv_start:
position 1), rows with b = -1 including row 0 and the last live row ("edges"), or row 0 but never the last live row ("head": the
rows behind the live ones, whose descriptor index is clamped to the last live row's, then meet a descriptor that would let them
write).  The rows a launch must skip under *n_active carry FINITE activations like every other row, and the descriptors BEHIND the
live rows name a spare utterance of the cache with a valid slot and position: a kernel that wrote a row it must skip leaves finite
values where the expected outputs hold NaN -- in C[row], in the spare utterance or over the last live row's cell -- and is caught
by the comparison, not by a fault.  Only the pad rows that fill the packed activations up to a whole 16-row tile are NaN.
(A kernel that merely READ a descriptor behind the last live row -- desc[row] where desc[min(row, M - 1)] is meant -- changes no output
bit, every store being guarded by row < M: that is the one slip these tests cannot see.)"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E  # noqa: E402

f32 = np.float32
HID, NH, HD, CMAX, NPOS = 768, 12, 64, 40, 64
QKV_ROPE = 100      # csrc/kernels.hpp D32_EPI_QKV_ROPE
EPS = 1e-6
PRE_M = [1, 15, 16, 17, 31, 33, 63, 64, 65, 130]      # gemm_pre32_k: 64-row workgroups of 2 x 2 waves, 32 rows per wave, clamped tiles behind M


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


def _ceil(n, m):
    return (n + m - 1) // m * m


# ---- shared inputs (never written) -------------------------------------------------------------------------------------------------
class _Weights:
    def __init__(self):
        from tests import gpu_util as G
        rs = np.random.RandomState(4242)
        self.W = (rs.standard_normal((3 * HID, HID)) * 0.05).astype(f32)                    # natural row order: the reference's
        self.g = (1.0 + 0.1 * rs.standard_normal(HID)).astype(f32)
        perm = E.rope_row_perm().numpy()
        self.Wperm = np.concatenate([self.W[:HID][perm], self.W[HID:2 * HID][perm], self.W[2 * HID:]], 0)
        cos, sin = E.rope_tables(NPOS)
        self.cos, self.sin = cos.numpy(), sin.numpy()
        self.cos_d, self.sin_d, self.g_d = G.dev(cos), G.dev(sin), G.dev(self.g)
        self.Wp32_d = E.pack_frag32(torch.from_numpy(self.Wperm)).to(G.DEV)
        self.Wfold = (self.Wperm * self.g[None, :]).astype(f32)                             # decode32x.hip: the gain folded into W
        self.Wx3_d = E.pack_frag_x3(torch.from_numpy(self.Wfold)).to(G.DEV)


@functools.lru_cache(maxsize=1)
def _weights():
    return _Weights()


class _Case:
    """M rows of finite activations, `live` of them in front of *n_active (the rest must never reach an output), and their descriptors"""

    def __init__(self, M, live, dead="edges"):
        from tests import gpu_util as G
        rs = np.random.RandomState(M * 101 + live)
        self.M, self.live = M, live
        self.A = (rs.standard_normal((M, HID)) * 2.0).astype(f32)       # rows live..M - 1 too: what a launch must skip would be seen if written
        self.n_utt = M                                   # utterance M is the spare one the descriptors behind the live rows name
        self.b = rs.permutation(M)[:live].astype(np.int32)
        self.ks = rs.randint(0, 6, size=M + 1).astype(np.int32)
        self.slot = rs.randint(0, CMAX, size=live).astype(np.int32)     # non-monotone, anywhere in the cache
        for m in rs.permutation(live)[: max(1, live // 8)]:             # a few pad rows: slot in front of the utterance's first valid one
            self.ks[self.b[m]] = rs.randint(1, 6)
            self.slot[m] = rs.randint(0, self.ks[self.b[m]])
        self.dead = np.zeros(live, bool)
        if dead == "edges":                              # b = -1 on row 0, the last live row and a few in between
            self.dead[[0, live - 1]] = True
            self.dead[rs.permutation(live)[: live // 10]] = True
        elif dead == "head":                             # b = -1 on row 0 and a few in between; the last live row writes
            self.dead[rs.permutation(live)[: live // 10]] = True
            self.dead[0], self.dead[live - 1] = True, False
        elif dead == "all":
            self.dead[:] = True
        rows = _ceil(M, 64)
        d = [G.row_desc(self.b[m], self.slot[m], self.ks[self.b[m]], bool(self.dead[m])) for m in range(live)]
        d += [(M, 3 + (m % 7), 2, 0) for m in range(live, rows)]        # behind the live rows: the spare utterance
        self.desc = np.array(d, np.int32)
        self.pos = self.desc[:live, 2]
        assert self.pos.max() < NPOS and (self.pos[self.slot < self.ks[self.b]] == 1).all()


@functools.lru_cache(maxsize=None)
def _case(M, live, dead="edges"):
    return _Case(M, live, dead)


@functools.lru_cache(maxsize=None)
def _reference(M, live):
    """gemm_skinny_k<float>, then rope_append_k with one pseudo-utterance per row: (q [live, 768], k [live, 12, 64], v [live, 12, 64]),
    and the un-roped projection"""
    from tests import gpu_util as G
    c, w = _case(M, live), _weights()
    raw = G.gemm(c.A[:live], w.W, wt="f32", epi=0, norm_w=w.g, eps=EPS)
    qkv = G.dev(raw)
    kc = torch.full((live, NH, CMAX, HD), float("nan"), dtype=torch.float32, device=G.DEV)
    vc = torch.full_like(kc, float("nan"))
    keep = [G.dev((c.slot + 1).astype(np.int32)), G.dev(c.ks[c.b].astype(np.int32))]
    _lib.check(_lib.lib().ctts_k_rope_append(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), _lib.F32, CMAX, w.cos_d.data_ptr(), w.sin_d.data_ptr(), 1,
                                             keep[0].data_ptr(), keep[1].data_ptr(), live, None), "rope_append")
    torch.cuda.synchronize()
    idx = torch.arange(live)
    slot = torch.from_numpy(c.slot.astype(np.int64))
    k, v = kc.cpu()[idx, :, slot].numpy(), vc.cpu()[idx, :, slot].numpy()
    assert np.isfinite(k).all() and np.isfinite(v).all()
    assert int(torch.isfinite(kc).sum()) == live * NH * HD          # the reference wrote each row's own slot and nothing else
    return qkv.cpu().numpy()[:, :HID].copy(), k, v, raw


def _expected(c, q, k, v):
    """what the fused launch must leave: C [M, 2304] and both caches [M + 1, 12, CMAX, 64], NaN wherever nothing may be written"""
    C = np.full((c.M, 3 * HID), np.nan, f32)
    kc = np.full((c.n_utt + 1, NH, CMAX, HD), np.nan, f32)
    vc = kc.copy()
    for m in np.flatnonzero(~c.dead):
        C[m, :HID] = q[m]
        kc[c.b[m], :, c.slot[m]] = k[m]
        vc[c.b[m], :, c.slot[m]] = v[m]
    return C, kc, vc


def _outputs(G, c):
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=G.DEV)
    return nan(c.M, 3 * HID), nan(c.n_utt + 1, NH, CMAX, HD), nan(c.n_utt + 1, NH, CMAX, HD)


def _assert_same(got, want, what):
    for name, g, w in zip(("C", "kcache", "vcache"), got, want):
        g = g.cpu().numpy()
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [(float(g[tuple(i)]), float(w[tuple(i)])) for i in bad[:4]]))


def _packed32(G, A):
    pad = np.full((_ceil(A.shape[0], 16), A.shape[1]), np.nan, f32)      # pad rows = NaN
    pad[: A.shape[0]] = A
    return E.pack_frag32(torch.from_numpy(pad)).to(G.DEV)


def _run_dec32(G, c, n_act, force_mb):
    w = _weights()
    keep = [_packed32(G, c.A), G.dev(c.A), G.dev(c.desc), None if n_act is None else G.dev(np.array([n_act], np.int32))]
    out = _outputs(G, c)
    _lib.check(_lib.lib().ctts_k_qkv_rope32(0, keep[0].data_ptr(), 0, w.Wp32_d.data_ptr(), 0, c.M, _lib.ptr(keep[3]), keep[1].data_ptr(), HID,
                                            w.g_d.data_ptr(), None, EPS, out[0].data_ptr(), keep[2].data_ptr(), None, w.cos_d.data_ptr(),
                                            w.sin_d.data_ptr(), out[1].data_ptr(), out[2].data_ptr(), CMAX, force_mb, None), "qkv_rope32")
    torch.cuda.synchronize()
    return out


def _run_pre32_qkv(G, c):
    w = _weights()
    keep = [_packed32(G, c.A), G.dev(c.A), G.dev(c.desc), torch.full((c.M,), float("nan"), dtype=torch.float32, device=G.DEV)]
    out = _outputs(G, c)
    _lib.check(_lib.lib().ctts_k_gemm_pre32(keep[0].data_ptr(), w.Wp32_d.data_ptr(), c.M, 3 * HID, HID, keep[1].data_ptr(), HID, w.g_d.data_ptr(), EPS,
                                            keep[3].data_ptr(), QKV_ROPE, out[0].data_ptr(), 3 * HID, None, 0, None, 0, keep[2].data_ptr(),
                                            w.cos_d.data_ptr(), w.sin_d.data_ptr(), out[1].data_ptr(), out[2].data_ptr(), CMAX, None), "gemm_pre32 qkv")
    torch.cuda.synchronize()
    return out


# ---- decode32.hip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_mb", [0, 1, 2, 4])
@pytest.mark.parametrize("M,n_act", [(1, None), (16, 16), (17, None), (40, 33), (64, 45), (100, 70)])
def test_dec32_qkv_rope_bit_identical(G, M, n_act, force_mb):
    """gemm_dec32_rms16_k (16-row workgroups, the default) and gemm_dec32_k (32- / 64-row workgroups) == the row-major chain, bit for bit"""
    live = M if n_act is None else n_act
    for dead in (("edges", "head") if M > 1 else ("none", "all")):          # one row cannot be both: run it live, then with b = -1
        c = _case(M, live, dead)
        got = _run_dec32(G, c, n_act, force_mb)
        variant = _lib.lib().ctts_k_dec32_last_variant().decode()
        assert variant == ("generic" if force_mb in (2, 4) else "rms16"), (force_mb, variant)
        q, k, v, _ = _reference(M, live)
        _assert_same(got, _expected(c, q, k, v), (M, n_act, force_mb, dead))


# ---- prefill32.hip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", PRE_M)
def test_pre32_qkv_rope_bit_identical(G, M):
    """gemm_pre32_k<QKV_ROPE> == the row-major chain, bit for bit; rows behind M (clamped tile loads, desc[min(row, M - 1)]) write nothing"""
    for dead in (("edges", "head") if M > 1 else ("none", "all")):
        c = _case(M, M, dead)
        q, k, v, _ = _reference(M, M)
        _assert_same(_run_pre32_qkv(G, c), _expected(c, q, k, v), (M, dead))


@pytest.mark.parametrize("M", PRE_M)
def test_pre32_res_and_silu_bit_identical(G, M):
    """gemm_pre32_k's residual and SiLU(gate) * up epilogues == gemm_skinny_k<float> on C and on the packed copy, with and without the
    RMSNorm prologue; pad rows of the packed copy stay NaN.  gemm_skinny_k has the residual epilogue without the prologue and the SiLU
    one with it (what the model runs); the residual epilogue WITH the prologue is held to res + (its store epilogue with the prologue),
    one float32 add as in the kernel.  SiLU without the prologue is not run: no other kernel states that arithmetic.  The prologue's
    1 / rms comes from launch_rows_rstd32, which is written for 768-column rows: the K = 3072 shape runs without it, as in the model.
    Every other combination of the three shapes, the two epilogues and the prologue is run."""
    lib = _lib.lib()
    rs = np.random.RandomState(M * 7 + 5)
    Mp = _ceil(M, 16)
    for N, K, epi, rms in [(768, 768, 1, False), (768, 768, 1, True), (768, 768, 2, True), (768, 3072, 1, False), (3072, 768, 1, False),
                           (3072, 768, 1, True), (3072, 768, 2, True)]:
        A = (rs.standard_normal((M, K)) * (2.0 if rms else 1.0)).astype(f32)
        W = (rs.standard_normal((2 * N if epi == 2 else N, K)) * 0.03).astype(f32)
        nw = (1.0 + 0.1 * rs.standard_normal(K)).astype(f32) if rms else None
        res = rs.standard_normal((M, N)).astype(f32) if epi == 1 else None
        if epi == 1 and rms:
            want = (res + G.gemm(A, W, wt="f32", epi=0, norm_w=nw, eps=EPS)).astype(f32)
        else:
            want = G.gemm(A, W, wt="f32", epi=epi, norm_w=nw, res=res, n_out=N, eps=EPS)
        keep = [_packed32(G, A), E.pack_frag32(torch.from_numpy(W)).to(G.DEV), G.dev(A), None if nw is None else G.dev(nw),
                None if res is None else G.dev(res), torch.full((M,), float("nan"), dtype=torch.float32, device=G.DEV)]
        Cc = torch.full((M, N), float("nan"), dtype=torch.float32, device=G.DEV)
        Cp = torch.full((Mp * N,), float("nan"), dtype=torch.float32, device=G.DEV)
        _lib.check(lib.ctts_k_gemm_pre32(keep[0].data_ptr(), keep[1].data_ptr(), M, N, K, keep[2].data_ptr() if rms else None, K, _lib.ptr(keep[3]),
                                         EPS, keep[5].data_ptr() if rms else None, epi, Cc.data_ptr() if epi == 1 else None, N, _lib.ptr(keep[4]), N,
                                         Cp.data_ptr(), N // 16, None, None, None, None, None, 0, None), "gemm_pre32")
        torch.cuda.synchronize()
        got_p = E.unpack_frag32(Cp.cpu(), Mp, N).numpy()
        assert np.array_equal(got_p[:M], want), (N, K, epi, rms)
        assert np.isnan(got_p[M:]).all(), (N, K, epi, rms)
        if epi == 1:
            assert np.array_equal(Cc.cpu().numpy(), want), (N, K, epi, rms)


# ---- float64 cross-check: a bug shared by both sides of the exact comparison ---------------------------------------------------------
def _rope64(y, pos, cos, sin):
    """rotate-half RoPE of [rows, 12, 64] in float64 with the (float32) tables' entries"""
    c, s = cos[pos].astype(np.float64)[:, None, :], sin[pos].astype(np.float64)[:, None, :]
    x1, x2 = y[..., :32], y[..., 32:]
    return np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _float64_qkv(c, w):
    A = c.A[: c.live].astype(np.float64)
    rstd = 1.0 / np.sqrt((A ** 2).mean(1, keepdims=True) + EPS)
    y = (A * rstd * w.g.astype(np.float64)) @ w.W.astype(np.float64).T
    n = c.live
    return (_rope64(y[:, :HID].reshape(n, NH, HD), c.pos, w.cos, w.sin), _rope64(y[:, HID:2 * HID].reshape(n, NH, HD), c.pos, w.cos, w.sin),
            y[:, 2 * HID:].reshape(n, NH, HD))


def _gather(c, out):
    """(q, k, v) [rows with b >= 0, 12, 64] out of a fused launch's outputs"""
    rows = np.flatnonzero(~c.dead)
    C, kc, vc = (t.cpu().numpy() for t in out)
    return C[rows, :HID].reshape(-1, NH, HD), kc[c.b[rows], :, c.slot[rows]], vc[c.b[rows], :, c.slot[rows]]


@pytest.mark.parametrize("kernel", ["dec32", "pre32"])
def test_qkv_rope_against_float64(G, kernel):
    """the fused kernels against the float64 value of RMSNorm -> projection -> RoPE, held to twice the error the row-major chain itself
    shows against float64 on the same inputs (the two are bit-identical; the factor absorbs nothing but that reference's own rounding)"""
    M, live = (64, 45) if kernel == "dec32" else (65, 65)
    c, w = _case(M, live), _weights()
    out = _run_dec32(G, c, 45, 0) if kernel == "dec32" else _run_pre32_qkv(G, c)
    rows = np.flatnonzero(~c.dead)
    want = [t[rows] for t in _float64_qkv(c, w)]
    q, k, v, _ = _reference(M, live)
    ref_err = max(np.abs(r[rows].reshape(-1, NH, HD) - t).max() for r, t in zip((q, k, v), want))
    got_err = max(np.abs(g - t).max() for g, t in zip(_gather(c, out), want))
    scale = max(np.abs(t).max() for t in want)
    print(f"{kernel}: fused {got_err:.3e}, row-major chain {ref_err:.3e}, output scale {scale:.3f}")
    assert 0 < ref_err < 1e-4 * scale                      # the reference itself is float32-class, and it did compute something
    assert got_err <= 2 * ref_err, (kernel, got_err, ref_err)


# ---- decode32x.hip -----------------------------------------------------------------------------------------------------------------
def _step_prep_rows(G, c, with_n_active):
    """the descriptors and per-row RoPE factors of the case's live rows as the step's first kernel writes them (ctts_k_step_prep): row m
    is utterance b[m] through the host row map, len = slot + 1, finish set for the rows with b = -1"""
    n_utt = c.n_utt + 1
    row_map = np.full(c.M, c.n_utt, np.int32)
    row_map[: c.live] = c.b
    lens = np.ones(n_utt, np.int32)
    lens[c.b] = c.slot + 1
    fin = np.zeros(n_utt, np.uint8)
    fin[c.b[c.dead]] = 1
    tcap = CMAX
    keep = [torch.zeros((4 * 626 * HID,), dtype=torch.float32, device=G.DEV), torch.zeros((n_utt * tcap * 4,), dtype=torch.int64, device=G.DEV),
            G.dev(lens), G.dev(row_map), G.dev(np.array([c.live], np.int32)), G.dev(c.ks), G.dev(fin)]
    w = _weights()
    x = torch.full((c.M, HID), float("nan"), dtype=torch.float32, device=G.DEV)
    desc = torch.full((_ceil(c.M, 64), 4), G.CANARY32, dtype=torch.int32, device=G.DEV)
    desc[c.live:] = torch.from_numpy(c.desc[c.live:]).to(G.DEV)      # behind the live rows the kernel writes nothing: keep the spare utterance there
    rope = torch.full((c.M, 64), float("nan"), dtype=torch.float32, device=G.DEV)
    _lib.check(_lib.lib().ctts_k_step_prep(keep[0].data_ptr(), 0, keep[1].data_ptr(), tcap, keep[2].data_ptr(), x.data_ptr(), None, None, c.M,
                                           keep[3].data_ptr(), keep[4].data_ptr() if with_n_active else None, desc.data_ptr(), keep[5].data_ptr(),
                                           keep[6].data_ptr(), 0, None, 0, None, None, None, rope.data_ptr(), w.cos_d.data_ptr(), w.sin_d.data_ptr(),
                                           None, 0, 1, None), "ctts_k_step_prep")
    torch.cuda.synchronize()
    return desc, rope


@pytest.mark.parametrize("force_mb", [0, 1, 2, 4, 9, 12])      # rows per workgroup (x 16); + 8: eight waves split K instead of four; 0: the default (64 rows, eight waves)
@pytest.mark.parametrize("M,n_act", [(1, None), (17, None), (33, 20), (64, 45)])
def test_dec32x_qkv_rope(G, M, n_act, force_mb):
    """the split-fp16 QKV launch: against the float64 value of what it is defined to compute -- (hi+lo)(hi+lo) - lo*lo over the split
    operands, 1 / rms on the accumulator, RoPE -- within the 5e-6 of the output's scale test_gemm_dec32x_split_bf16 holds the other
    epilogues to; once with the RoPE factors through the descriptor, once through the per-row table ctts_k_step_prep writes (with
    that kernel's descriptors): the two runs must agree bit for bit"""
    live = M if n_act is None else n_act
    c, w = _case(M, live, "edges" if M > 1 else "none"), _weights()
    Mp = _ceil(M, 16)
    Apad = np.full((Mp, HID), np.nan, f32)
    Apad[:M] = c.A
    ah, al = E.split_f16(torch.from_numpy(Apad))
    planes_a = torch.stack([E.pack_frag(ah), E.pack_frag(al)], 0).contiguous().to(G.DEV)
    via_ssq = (M + force_mb) % 2 == 1                                  # 1 / rms from the rows themselves, or from their 48 partial sums of squares
    ssq = (c.A.reshape(M, 48, 16).astype(np.float64) ** 2).sum(-1).astype(f32)      # of every row, the ones behind *n_active included
    keep = [G.dev(c.A), G.dev(ssq), None if n_act is None else G.dev(np.array([n_act], np.int32)), G.dev(c.desc)]
    desc_k, rope_k = _step_prep_rows(G, c, n_act is not None)
    assert np.array_equal(desc_k.cpu().numpy(), c.desc)                # the kernel's descriptors ARE the numpy ones
    assert np.array_equal(rope_k.cpu().numpy()[:live], np.concatenate([w.cos[c.pos], w.sin[c.pos]], 1))
    outs = []
    for desc_d, rope_d in ((keep[3], None), (desc_k, rope_k)):
        out = _outputs(G, c)
        _lib.check(_lib.lib().ctts_k_qkv_rope32(1, planes_a.data_ptr(), Mp * HID, w.Wx3_d.data_ptr(), 3 * HID * HID, M, _lib.ptr(keep[2]),
                                                None if via_ssq else keep[0].data_ptr(), HID, None, keep[1].data_ptr() if via_ssq else None, EPS,
                                                out[0].data_ptr(), desc_d.data_ptr(), _lib.ptr(rope_d), w.cos_d.data_ptr(), w.sin_d.data_ptr(),
                                                out[1].data_ptr(), out[2].data_ptr(), CMAX, force_mb, None), "qkv_rope32 x3")
        torch.cuda.synchronize()
        outs.append(out)
    for a, b in zip(*outs):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    # where it wrote: exactly the cells of the live descriptors
    q0, k0, v0, _ = _reference(M, live)
    for got, want in zip(outs[0], _expected(c, q0, k0, v0)):
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want))
    # what it wrote
    rows = np.flatnonzero(~c.dead)
    if rows.size == 0:
        return
    sp = lambda a: [t.double().numpy() for t in E.split_f16(torch.from_numpy(a))]
    (a_h, a_l), (w_h, w_l) = sp(c.A[:live]), sp(w.Wfold)
    a_l, w_l = a_l / E.X3_LO_SCALE, w_l / E.X3_LO_SCALE
    y = (a_h + a_l) @ (w_h + w_l).T - a_l @ w_l.T
    y *= 1.0 / np.sqrt((c.A[:live].astype(np.float64) ** 2).mean(1, keepdims=True) + EPS)
    inv = np.argsort(E.rope_row_perm().numpy())                        # the permuted q / k rows back in natural order
    yq, yk, yv = y[:, :HID][:, inv], y[:, HID:2 * HID][:, inv], y[:, 2 * HID:]
    want = (_rope64(yq.reshape(live, NH, HD), c.pos, w.cos, w.sin)[rows], _rope64(yk.reshape(live, NH, HD), c.pos, w.cos, w.sin)[rows],
            yv.reshape(live, NH, HD)[rows])
    scale = max(np.abs(t).max() for t in want)
    err = max(np.abs(g - t).max() for g, t in zip(_gather(c, outs[0]), want))
    assert err < 5e-6 * scale, (M, n_act, force_mb, err / scale)

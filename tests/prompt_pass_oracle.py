"""Oracle of the perf-mode prompt pass's attention: float64 softmax(q K^T / 8 + mask) V over EVERY row of a launch, the derived error
bounds of the two kernels that compute it (csrc/gpt.hip: attention_prefill_mfma_k from 128 rows per group, the one-wave attention_k
below), and numpy emulations of the two kernels' arithmetic, which tests/test_prompt_pass_host.py holds against those bounds on CPU.

A launch: G row groups of T query rows; row t of group g is KV slot `slot0 + t` of utterance b = row_map[g] (identity without a map) and
sees the keys [min(kv_start[b], slot), slot] of that utterance's cache rows."""
import numpy as np

f32 = np.float32
NH, HD, H = 12, 64, 768
KB = 32                       # keys per block, both kernels
U_BF16 = 2.0 ** -8            # unit roundoffs
U_F32 = 2.0 ** -24


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 -> nearest bf16 (ties to even), as float32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(f32)


def row_slots(T, slot0, kvs):
    """slot, first visible key and validity of the T rows of a group whose utterance starts at kvs"""
    slot = slot0 + np.arange(T)
    return slot, np.minimum(kvs, slot), slot >= kvs


def reference(q, Kc, Vc, T, slot0, kv_start, row_map=None):
    """q [G*T, 768] (any float), Kc / Vc [slots, 12, cmax, 64], kv_start [slots] -> dict of
         ref [G*T, 768] float64, a = sum_j p_j |v_j| [G*T, 768], delta = max_j sum_d |q_d k_jd| / 8 [G*T, 12],
         n = visible keys [G*T], valid [G*T] (slot >= kv_start[b]: the row's output is consumed)"""
    M = q.shape[0]
    G = M // T
    S = slot0 + T                                   # keys any row of the launch can see: cache rows [0, S)
    ref, a = np.empty((M, H)), np.empty((M, H))
    delta, n, valid = np.empty((M, NH)), np.empty(M, np.int64), np.empty(M, bool)
    j = np.arange(S)
    for g in range(G):
        b = g if row_map is None else int(row_map[g])
        slot, lo, ok = row_slots(T, slot0, int(kv_start[b]))
        vis = (j[None, :] >= lo[:, None]) & (j[None, :] <= slot[:, None])            # [T, S]
        qg = q[g * T: (g + 1) * T, :H].astype(np.float64).reshape(T, NH, HD)
        K, V = Kc[b, :, :S].astype(np.float64), Vc[b, :, :S].astype(np.float64)   # [12, S, 64]
        s = np.einsum("thd,hjd->htj", qg, K) * 0.125
        sa = np.einsum("thd,hjd->htj", np.abs(qg), np.abs(K)) * 0.125
        s = np.where(vis[None], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        rows = slice(g * T, (g + 1) * T)
        ref[rows] = np.einsum("htj,hjd->thd", p, V).reshape(T, H)
        a[rows] = np.einsum("htj,hjd->thd", p, np.abs(V)).reshape(T, H)
        delta[rows] = np.where(vis[None], sa, -np.inf).max(-1).T
        n[rows] = vis.sum(-1)
        valid[rows] = ok
    return dict(ref=ref, a=a, delta=delta, n=n, valid=valid)


def bound(r, kernel: str, out_bf16: bool = False):
    """The derived bound of |out - ref| per output element, [M, 768].
    MFMA kernel, f32 out: (2^-8 + 2 * 2^-17 delta + n 2^-23) a
      2^-8: P enters the second product rounded to bf16 (unit roundoff 2^-8) while l sums the unrounded p;
      2^-17 delta: q / 8 is split into two bf16 terms (residual 2^-18 relative) plus the f32 accumulation of the 64-term dot product; a
      score error e changes p by a relative 2 e, once through the score and once through the running max;
      n 2^-23: the f32 accumulation of n terms.
    one-wave kernel, f32 out: (2 * 2^-18 delta + (n + 8) 2^-23) a -- the 64 f32 fma roundings of the dot product; the accumulation.
    bf16 out, either kernel: b + 2^-8 (|ref| + b) with b the f32-out bound -- the rounding of a value that is itself within b."""
    d = np.repeat(r["delta"], HD, axis=1)
    n = r["n"][:, None].astype(np.float64)
    if kernel == "mfma":
        b = (2.0 ** -8 + 2.0 * 2.0 ** -17 * d + n * 2.0 ** -23) * r["a"]
    elif kernel == "wave":
        b = (2.0 * 2.0 ** -18 * d + (n + 8.0) * 2.0 ** -23) * r["a"]
    else:
        raise ValueError(kernel)
    return b + 2.0 ** -8 * (np.abs(r["ref"]) + b) if out_bf16 else b


def kernel_of(T: int) -> str:
    """the kernel launch_attention picks for a prompt chunk of T rows per group (CTTS_FLASH_MIN_T at its default)"""
    return "mfma" if T >= 128 else "wave"


def worst_ratio(got, r, kernel, out_bf16=False):
    """max over the valid rows of |got - ref| / bound"""
    v = r["valid"]
    return float((np.abs(got[v].astype(np.float64) - r["ref"][v]) / bound(r, kernel, out_bf16)[v]).max())


# ---- the kernels' arithmetic in numpy ------------------------------------------------------------------------------------------------
def emulate_mfma(q, Kc, Vc, T, slot0, kv_start, row_map=None, lo_shift=0, hi_shift=0):
    """attention_prefill_mfma_k in float32 numpy: key blocks of 32 on ABSOLUTE multiples of 32, q / 8 = hi + lo in bf16, scores
    accumulated in f32 (lo product first, per 32-wide d chunk), online softmax in f32 per block, P rounded to bf16 into the second
    product while l sums the unrounded p.  A block with no visible key is a no-op in the kernel (alpha = 1, p = 0), so walking every
    block of [0, slot0 + T) for every row gives what the kernel's per-tile range gives.  lo_shift / hi_shift move the mask's two ends
    (a deliberately wrong kernel, for the tests of the tests)."""
    M = q.shape[0]
    G = M // T
    S = slot0 + T
    out = np.empty((M, H), f32)
    for g in range(G):
        b = g if row_map is None else int(row_map[g])
        slot, lo, _ = row_slots(T, slot0, int(kv_start[b]))
        lo, hi_key = lo + lo_shift, slot + hi_shift
        v = (q[g * T: (g + 1) * T, :H].astype(f32) * f32(0.125)).reshape(T, NH, HD).transpose(1, 0, 2)   # [12, T, 64]
        qh = bf16_round(v)
        ql = bf16_round(v - qh)
        m = np.full((NH, T), -np.inf, f32)
        l = np.zeros((NH, T), f32)
        o = np.zeros((NH, T, HD), f32)
        for j0 in range(0, S, KB):
            j1 = min(j0 + KB, S)
            K, V = Kc[b, :, j0:j1].astype(f32), Vc[b, :, j0:j1].astype(f32)                              # [12, kb, 64]
            s = np.zeros((NH, T, j1 - j0), f32)
            for c in range(2):
                d = slice(32 * c, 32 * c + 32)
                s = s + np.einsum("htd,hjd->htj", ql[..., d], K[..., d])
                s = s + np.einsum("htd,hjd->htj", qh[..., d], K[..., d])
            j = np.arange(j0, j1)
            vis = (j[None, :] >= lo[:, None]) & (j[None, :] <= hi_key[:, None])
            s = np.where(vis[None], s, f32(-np.inf))
            mnew = np.maximum(m, s.max(-1))
            dead = np.isneginf(mnew)
            with np.errstate(invalid="ignore"):
                alpha = np.where(dead, f32(1), np.exp(m - np.where(dead, f32(0), mnew))).astype(f32)
                p = np.where(vis[None], np.exp(s - np.where(dead, f32(0), mnew)[..., None]), f32(0)).astype(f32)
            l = l * alpha + p.sum(-1, dtype=f32)
            m = mnew
            o = o * alpha[..., None] + np.einsum("htj,hjd->htd", bf16_round(p), np.where(np.isfinite(V), V, f32(0)))
        out[g * T: (g + 1) * T] = (o * (f32(1) / l)[..., None]).transpose(1, 0, 2).reshape(T, H)
    return out


def emulate_wave(q, Kc, Vc, T, slot0, kv_start, row_map=None, lo_shift=0, hi_shift=0):
    """attention_k<bf16, 1 wave> in float32 numpy: a row walks ITS keys from its first visible one in blocks of 32, key i of a block
    belongs to key group i mod 8, every group keeps its own f32 sum and accumulator under the wave's shared running max, the groups
    are added at the end; everything in f32 (q unscaled, the 2^-3 on the finished dot product)."""
    M = q.shape[0]
    G = M // T
    out = np.empty((M, H), f32)
    for g in range(G):
        b = g if row_map is None else int(row_map[g])
        slot, lo, _ = row_slots(T, slot0, int(kv_start[b]))
        lo, hi_key = lo + lo_shift, slot + hi_shift
        qg = q[g * T: (g + 1) * T, :H].astype(f32).reshape(T, NH, HD)
        K, V = Kc[b].astype(f32), Vc[b].astype(f32)                                      # [12, cmax, 64]
        m = np.full((T, NH), -np.inf, f32)
        l = np.zeros((T, NH, 8), f32)
        acc = np.zeros((T, NH, 8, HD), f32)
        nblk = int((hi_key - lo).max()) // KB + 1
        for blk in range(nblk):
            j = lo[:, None] + blk * KB + np.arange(KB)[None, :]                          # [T, 32] absolute keys
            ok = j <= hi_key[:, None]
            jc = np.minimum(j, hi_key[:, None])                                          # clamped lanes re-read the last key, masked below
            Kb = K[:, jc].transpose(1, 0, 2, 3)                                          # [T, 12, 32, 64]
            Vb = V[:, jc].transpose(1, 0, 2, 3)
            s = (qg[:, :, None, :] * Kb).sum(-1, dtype=f32) * f32(0.125)
            s = np.where(ok[:, None, :], s, f32(-np.inf))
            live = ok[:, 0]                                                              # rows that still have a block to consume
            mnew = np.where(live[:, None], np.maximum(m, s.max(-1)), m)
            alpha = np.where(live[:, None], np.exp(m - mnew), f32(1)).astype(f32)
            p = np.where(ok[:, None, :], np.exp(s - mnew[..., None]), f32(0)).astype(f32)
            l = l * alpha[..., None] + p.reshape(T, NH, 4, 8).sum(2, dtype=f32)
            pv = (p[..., None] * Vb).reshape(T, NH, 4, 8, HD)
            acc = acc * alpha[..., None, None]
            for i in range(4):
                acc = acc + pv[:, :, i]
            m = mnew
        o = acc.sum(2, dtype=f32) * (f32(1) / l.sum(-1, dtype=f32))[..., None]
        out[g * T: (g + 1) * T] = o.reshape(T, H)
    return out

"""The kernels that turn compact rows back into per-utterance state at the end of a decode step, one by one through the C ABI:
`final_norm_k` with every index argument (`ctts_k_final_norm_rows`), the one-launch final norm + hidden capture + heads
`gemm_dec32_fnorm16_k` (`ctts_k_fnorm_heads`), `sample_k` / `sample_text_k` on compact rows and the `EmbedNext` fold in `sample_k`'s tail
(`ctts_k_sample_rows`).  tests/test_gpu_step_front.py covers the writers of the row descriptors; these are their readers.

Logits, hidden rows and descriptors are indexed by compact row m; token ids, len, finish, end_idx, the draws, the history, the sampling
table and the captured hidden states by utterance slot b.  Every test makes the two differ (a permuted map, absent rows inside the
descriptor list, per-utterance prompt lengths) and states the contract as a numpy restatement.  Comparisons between kernels are EXACT;
the only bound is the 2e-6 test_embed_and_final_norm already holds final_norm_k to against oracle/llama_np.py.  Every output buffer starts
as NaN or a sentinel word: a location the kernel must not write is compared with that."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, rng, engine as E  # noqa: E402
from chattts_amd.serving import request_params, sampling_row  # noqa: E402
from oracle import llama_np, sampling_np  # noqa: E402
from tests.gpu_util import CANARY32  # noqa: E402
from tests.test_gpu_step_front import EDGE_CODE, HID, NAUDIO, NVQ, _ceil16, _embed_ref, _step, _tables_dev  # noqa: E402

f32 = np.float32
EOS = 625
IDS_CANARY = -0x5A5A5A5A          # int64 pattern of a token slot no kernel may write (as a history token it matches no vocabulary entry)
FIN_CANARY = 0x5A                 # finish byte of an utterance that is not in the list
MARGIN_CANARY = f32(1.0e30)       # finite, above every real margin: "lowered" is `<`, "untouched" is bit equality


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _nan(G, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=G.DEV)


@functools.lru_cache(maxsize=1)
def _norm_w():
    return (1 + 0.1 * np.random.RandomState(5).standard_normal(HID)).astype(f32)


# ---- (a) final_norm_k ----------------------------------------------------------------------------------------------------------------
def _final_norm_rows(G, x, qpb, lens, T, B, *, slots, max_new, row_map=None, n_active=None, prompt_len=None, last_row=None):
    """one ctts_k_final_norm_rows launch over a grid of B rows: hfin [B, 768], hiddens [slots, max_new, 768], hfin_packed (unpacked here)"""
    Bp = _ceil16(B)
    hfin, hid, pk = _nan(G, B, HID), _nan(G, slots, max_new, HID), _nan(G, Bp * HID)
    keep = [G.dev(x), G.dev(_norm_w()), G.dev(lens)] + [None if a is None else G.dev(np.asarray(a, np.int32)) for a in (row_map, prompt_len, last_row)]
    na = None if n_active is None else G.dev(np.array([n_active], np.int32))
    _lib.check(_lib.lib().ctts_k_final_norm_rows(keep[0].data_ptr(), qpb, keep[1].data_ptr(), 1e-6, hfin.data_ptr(), hid.data_ptr(), max_new,
                                                 keep[2].data_ptr(), T, B, _lib.ptr(keep[3]), _lib.ptr(na), _lib.ptr(keep[4]), pk.data_ptr(),
                                                 _lib.ptr(keep[5]), None), "ctts_k_final_norm_rows")
    torch.cuda.synchronize()
    return hfin.cpu().numpy(), hid.cpu().numpy(), E.unpack_frag32(pk.cpu(), Bp, HID).numpy()


def _final_norm_identity(G, rows):
    """the plain ctts_k_final_norm on pre-gathered rows: identity rows, one T, no hidden capture"""
    n = rows.shape[0]
    hfin = _nan(G, n, HID)
    keep = [G.dev(rows), G.dev(_norm_w()), G.dev(np.ones(n, np.int32))]
    _lib.check(_lib.lib().ctts_k_final_norm(keep[0].data_ptr(), 1, keep[1].data_ptr(), 1e-6, hfin.data_ptr(), None, 1, keep[2].data_ptr(), 1, n, None),
               "ctts_k_final_norm")
    torch.cuda.synchronize()
    return hfin.cpu().numpy()


def _check_final_norm(G, got, rows, utt, gens, slots, max_new):
    """rows [n, 768]: the input row of every live compact row; utt / gens: its utterance and `len - prompt_len`"""
    hfin, hid, pk = got
    n = rows.shape[0]
    want_h = np.full((slots, max_new, HID), np.nan, f32)
    if n:
        ref = llama_np.rmsnorm(rows, _norm_w(), f32(1e-6))
        assert np.abs(hfin[:n] - ref).max() < 2e-6                          # the bar of test_embed_and_final_norm
        assert np.array_equal(_bits(hfin[:n]), _bits(_final_norm_identity(G, rows)))
        assert np.array_equal(_bits(pk[:n]), _bits(hfin[:n]))               # pack_frag32 of hfin, bit for bit
        for m in range(n):
            if 0 <= gens[m] < max_new:
                want_h[utt[m], gens[m]] = hfin[m]
    assert np.isnan(hfin[n:]).all() and np.isnan(pk[n:]).all()              # rows behind the live count, pad rows of the last tile
    assert np.array_equal(_bits(hid), _bits(want_h))                        # every other (b, gen) still holds its NaN


@pytest.mark.parametrize("B,n_act", [(B, a) for B in (1, 5, 64, 70) for a in ("zero", "mid", "all", "null") if (B, a) != (1, "mid")])   # 1 // 2 = 0
def test_final_norm_rows_decode(G, B, n_act):
    """decode layout (q_per_b = 1), B slots and B grid rows: a permuted row_map, n_active 0 / B // 2 / B / absent, a prompt_len per
    utterance against a call-wide T that fits none of them, gen = len - prompt_len at -1, 0, max_new - 1 and max_new (the first and
    the last leave hiddens alone, hfin is written all the same)"""
    rs = np.random.RandomState(B * 7 + ["zero", "mid", "all", "null"].index(n_act))
    max_new = 6
    n = {"zero": 0, "mid": B // 2, "all": B, "null": B}[n_act]
    row_map = rs.permutation(B).astype(np.int32)
    gens = np.array([[-1, 0, max_new - 1, max_new][m % 4] if m < 8 else rs.randint(0, max_new) for m in range(B)])   # by compact row
    if B == 1:
        gens[0] = max_new - 1
    plen = rs.randint(2, 10, size=B).astype(np.int32)                       # by utterance; T = 1 below is nobody's prompt length
    lens = np.zeros(B, np.int32)
    lens[row_map] = plen[row_map] + gens
    x = (rs.standard_normal((B, HID)) * 3).astype(f32)
    got = _final_norm_rows(G, x, 1, lens, 1, B, slots=B, max_new=max_new, row_map=row_map, n_active=None if n_act == "null" else n,
                           prompt_len=plen)
    _check_final_norm(G, got, x[:n], row_map[:n], gens[:n], B, max_new)
    if B >= 5 and n >= 4:
        assert len({int(lens[b]) - int(plen[b]) for b in row_map[:n]}) >= 4   # the four edges of gen are among the live rows


@pytest.mark.parametrize("with_map", [False, True], ids=["identity", "row_map"])
@pytest.mark.parametrize("layout", ["q_per_b", "last_row"])
def test_final_norm_rows_prefill(G, layout, with_map):
    """prompt pass: the last row of each group of T rows (q_per_b = T), or the rows prefill_compact_k names in last_row when only the
    valid tokens were computed; with a slot pool's row_map the hidden state of step 0 goes to the pool slot's row"""
    rs = np.random.RandomState(40 + 2 * (layout == "last_row") + with_map)
    B, T, max_new = 5, 6, 4
    slots = B + 4 if with_map else B
    row_map = rs.permutation(slots)[:B].astype(np.int32) if with_map else None
    utt = np.arange(B) if row_map is None else row_map
    lens = np.full(slots, T, np.int32)                                       # the prompt has just been written: gen = 0
    if layout == "q_per_b":
        x = (rs.standard_normal((B * T, HID)) * 3).astype(f32)
        last = None
        rows = x.reshape(B, T, HID)[:, -1]
    else:
        ks = rs.randint(0, T, size=B)
        ks[1] = T - 1                                                        # one valid token
        last = (np.cumsum(T - ks) - 1).astype(np.int32)                      # what prefill_compact_k writes (test_prefill_compact)
        x = (rs.standard_normal((int((T - ks).sum()), HID)) * 3).astype(f32)
        rows = x[last]
    plen = np.full(slots, T, np.int32) if with_map else None                 # a pool passes prompt_len and a T of its own
    got = _final_norm_rows(G, x, T, lens, 1 if with_map else T, B, slots=slots, max_new=max_new, row_map=row_map, prompt_len=plen, last_row=last)
    _check_final_norm(G, got, np.ascontiguousarray(rows), utt, np.zeros(B, np.int64), slots, max_new)


# ---- (b) gemm_dec32_fnorm16_k --------------------------------------------------------------------------------------------------------
HEADS = {"codes": (2512, 2504), "text": (304, 300)}     # N (padded to 16), n_cols; 300 % 16 = 12


@functools.lru_cache(maxsize=2)
def _heads(kind):
    N, n_cols = HEADS[kind]
    W = (np.random.RandomState(N).standard_normal((n_cols, HID)) * 0.03).astype(f32)
    return W, np.concatenate([W, np.zeros((N - n_cols, HID), f32)], 0)


@functools.lru_cache(maxsize=2)
def _heads_dev(kind):
    from tests import gpu_util as G
    return E.pack_frag32(torch.from_numpy(_heads(kind)[1])).to(G.DEV)


FH_CASES = [(1, None), (1, 0), (15, None), (15, 7), (16, None), (16, 16), (17, None), (17, 16), (33, 20), (33, 32), (64, None), (64, 45), (64, 0),
            (70, None), (70, 33), (70, 64)]


def _fnorm_heads(G, kind, M, n_act, capture=True):
    N, n_cols = HEADS[kind]
    rs = np.random.RandomState(M * 13 + (n_act or 0) + N)
    Mp, live = _ceil16(M), M if n_act is None else n_act
    hid_cap, slots = 5, M + 3
    X = (rs.standard_normal((M, HID)) * 3).astype(f32)
    pad = np.full((Mp, HID), np.nan, f32)                                    # pad rows = NaN: they must never reach a live output
    pad[:M] = X
    # descriptors: utterances that do not ascend with the row, two absent rows in the middle of the first tile, gen = slot + 1 -
    # prompt_len[b] at -1, 0, hid_cap - 1, hid_cap and in between
    utt = rs.permutation(slots)[:M].astype(np.int64)
    for m in (3, 9):
        if m < M - 1:
            utt[m] = -1
    plen = rs.randint(2, 10, size=slots).astype(np.int32)
    gens = np.array([[0, hid_cap - 1, -1, hid_cap][m % 4] if m < 8 else rs.randint(0, hid_cap) for m in range(M)])
    desc = np.array([G.DESC_ABSENT if utt[m] < 0 else G.row_desc(utt[m], plen[utt[m]] + gens[m] - 1, 0) for m in range(M)], np.int32)
    Cc, hid = _nan(G, M, n_cols), _nan(G, slots, hid_cap, HID)
    pack_d = E.pack_frag32(torch.from_numpy(pad)).to(G.DEV)
    keep = [pack_d, G.dev(_norm_w()), G.dev(desc), G.dev(plen)]
    na = None if n_act is None else G.dev(np.array([n_act], np.int32))
    lib = _lib.lib()
    _lib.check(lib.ctts_k_fnorm_heads(pack_d.data_ptr(), _heads_dev(kind).data_ptr(), M, N, n_cols, _lib.ptr(na), keep[1].data_ptr(), 1e-6,
                                      Cc.data_ptr(), n_cols, keep[2].data_ptr() if capture else None, hid.data_ptr() if capture else None,
                                      hid_cap if capture else 0, 1, keep[3].data_ptr() if capture else None, None), "ctts_k_fnorm_heads")
    torch.cuda.synchronize()
    assert lib.ctts_k_dec32_last_variant().decode() == "fnorm16"
    got_c, got_h = Cc.cpu().numpy(), hid.cpu().numpy()
    want_h = np.full((slots, hid_cap, HID), np.nan, f32)
    if live:
        hfin = _final_norm_identity(G, X[:live])                            # final_norm_k on the same rows
        want_c = G.gemm(hfin, _heads(kind)[0], wt="f32")                     # gemm_skinny_k<float>, the path of test_gemm_dec32_bit_identical
        assert np.array_equal(_bits(got_c[:live]), _bits(want_c)), (kind, M, n_act)
        for m in range(live):
            if capture and utt[m] >= 0 and 0 <= gens[m] < hid_cap:
                want_h[utt[m], gens[m]] = hfin[m]
    assert np.isnan(got_c[live:]).all()                                      # rows from the live count on are not written
    assert np.array_equal(_bits(got_h), _bits(want_h))                       # the captured rows ARE final_norm_k's, every other location NaN
    return int((~np.isnan(want_h[:, :, 0])).sum())


@pytest.mark.parametrize("M,n_act", FH_CASES)
def test_fnorm_heads_codes(G, M, n_act):
    """final RMSNorm + hidden capture + the four code heads (N = 2512 padded, 2504 columns) in one launch: the captured hidden state
    == final_norm_k's row, the logits == gemm_skinny_k<float> of those rows, bit for bit; partial row tiles, a live count inside a
    tile, at a tile boundary and 0; absent descriptors inside a tile, gen at both edges of [0, hid_cap)"""
    captured = _fnorm_heads(G, "codes", M, n_act)
    if (M if n_act is None else n_act) >= 16:
        assert captured >= 4


@pytest.mark.parametrize("M,n_act", [(17, None), (33, 20)])
def test_fnorm_heads_text_shape(G, M, n_act):
    """a head whose column count is no multiple of 16 (300 of 304): the last weight tile stores 12 columns"""
    _fnorm_heads(G, "text", M, n_act)


@pytest.mark.parametrize("M,n_act", [(17, None), (70, 33)])
def test_fnorm_heads_without_capture(G, M, n_act):
    """hid = NULL (desc and prompt_len are not read then): the same logits"""
    _fnorm_heads(G, "codes", M, n_act, capture=False)


# ---- (c) sample_k on compact rows: the case, its oracle, the launch ------------------------------------------------------------------
TCAP, NQ, TSTRIDE = 28, 3, 18
CALL_WIDE = dict(temps=[0.3, 0.5, 0.7, 1.0], top_P=0.7, top_K=20, rep=2.0, min_new=3)
TABLE = [dict(temps=[0.3, 0.3, 0.3, 0.3], top_P=0.7, top_K=20, rep=2.5, min_new=0),
         dict(temps=[1.0, 0.7, 0.5, 0.3], top_P=None, top_K=5, rep=2.0, min_new=3),
         dict(temps=[0.5, 0.5, 1.0, 1.0], top_P=0.9, top_K=None, rep=3.0, min_new=1)]
TEXT_CFG = dict(temps=[1.0], top_P=0.95, top_K=50, rep=1.0, min_new=3)   # one sampling row per utterance: a flat distribution, so that q decides
PEAK, RUNNER_UP = 40.0, 30.0      # tempered logits of the two tokens that make codebook 3 depend on the history (SampleCase)


class SampleCase:
    """everything one sampler launch reads, as numpy: S utterance slots, R grid rows of which n_live are live; `rows[m]` = utterance
    of compact row m or -1.  Built on the CPU alone; `expect()` is the oracle and the conditions on the inputs."""

    def __init__(self, S, n_live, mode, variant, text=0):
        rs = np.random.RandomState(S * 101 + n_live * 7 + (mode == "desc") * 3 + ["plain", "table", "teacher"].index(variant) + 50 * bool(text))
        self.S, self.n_live, self.mode, self.variant, self.text = S, n_live, mode, variant, text
        self.V = text if text else NAUDIO
        self.eos = -1 if text else EOS                                       # (text: chosen below)
        self.nrow = 1 if text else NVQ                                       # sampling rows per utterance
        self.q_rows = S + 3
        self.R = R = S if n_live == S else n_live + 2
        live = [int(b) for b in rs.permutation(S)[:n_live]]                  # compact order: not ascending
        self.plen = rs.randint(1, 7, size=S).astype(np.int32)
        h = rs.randint(1, 16, size=S)
        role = {}
        if n_live >= 5:
            role.update(zip(("h0", "h20", "full", "eos", "prefin"), live[:5]))
        if n_live >= 12:
            role.update(zip(("force", "mask", "min_new", "row625", "teach_eos"), live[5:10]))
        self.role = role
        for name, hh in (("h0", 0), ("h20", 20), ("eos", 7), ("force", 9), ("mask", 5), ("min_new", 1), ("teach_eos", 4)):
            if name in role:
                h[role[name]] = hh
        if "full" in role:
            h[role["full"]] = TCAP - self.plen[role["full"]]                 # len == tcap: the slot is full
        self.lens = (self.plen + h).astype(np.int32)
        # compact rows: row_map + n_active (the live utterances in front, others behind the count) or descriptors with absent rows inside
        if mode == "map":
            rest = [b for b in rs.permutation(S) if b not in live]
            self.rows = np.array(live + [-1] * (R - n_live))
            self.row_map = np.array(live + rest[: R - n_live], np.int32)
        else:
            self.rows = np.full(R, -1)
            self.rows[np.sort(rs.permutation(R)[:n_live])] = live
            self.row_map = None
        self.row_of = {int(b): m for m, b in enumerate(self.rows) if b >= 0}
        scale = [0.3, 1.0][(S + n_live) % 2]                                 # <= 1.0: above that a swapped q can leave an answer unchanged
        self.logits = (rs.standard_normal((R * self.nrow, self.V)) * scale).astype(f32)
        self.cfgs = [TABLE[b % 3] for b in range(S)] if variant == "table" else None
        self.q = np.stack([rng.ExpDraws(self.q_rows * self.nrow, self.V, 300 + S + i).step(i).numpy() for i in range(NQ)])
        self.row_base = (4 * rs.permutation(S) + 40).astype(np.int32)        # every penalised row below 625 ...
        if "row625" in role:
            self.row_base[role["row625"]] = 640                             # ... but this utterance's: processors.py:24-27 skips it
        self.stop_at = np.full(S, -1, np.int32)
        self.ids = np.full((S, TCAP, NVQ), IDS_CANARY, np.int64)
        for b in range(S):
            self.ids[b, : self.lens[b]] = rs.randint(0, 500 if not text else text, size=(self.lens[b], NVQ))   # (codes: 500 .. 598 are kept for codebook 3's peaks below)
        for b, m in self.row_of.items():                                     # the likeliest tokens in the OLDEST slots of the 16-token window
            nh = min(int(h[b]), 16)
            for k in range(self.nrow):
                top = np.argsort(-self.logits[m * self.nrow + k], kind="stable")
                top = top[(top != self.eos) & ((top < 500) | bool(text))][: nh // 2]
                self.ids[b, self.lens[b] - nh: self.lens[b] - nh + len(top), k] = top
        if text:
            self.ids[:, :, 1:] = self.ids[:, :, :1]
        else:
            # codebook 3 is decided by the history: token `peak[b]` towers over the row, `runner[b]` over the rest, and the OLDEST token of
            # b's window is peak[b] -- penalised once (every penalty here is >= 2) it falls e^10 below the runner-up.  With a neighbour's
            # history, or with the window one token short, the peak wins.  The utterance without a history shares its neighbour's peak.
            peak, runner = 500 + rs.permutation(90)[:S], 591 + np.arange(S) % 8
            order = [b for b in live if self.lens[b] < TCAP]
            for i, b in enumerate(order):
                if h[b] == 0 and len(order) > 1:
                    peak[b] = peak[order[(i + 1) % len(order)]]
            for b, m in self.row_of.items():
                t3 = self.cfg(b)["temps"][3]
                self.logits[m * NVQ + 3, peak[b]], self.logits[m * NVQ + 3, runner[b]] = PEAK * t3, RUNNER_UP * t3
                if h[b]:
                    self.ids[b, self.lens[b] - min(int(h[b]), 16), 3] = peak[b]
        for name, col in (("eos", 2), ("mask", 0), ("min_new", 1)):          # EOS far above everything else in ONE codebook
            if name in role and not text:
                self.logits[self.row_of[role[name]] * NVQ + col, EOS] = 40.0
        if "force" in role:
            self.stop_at[role["force"]] = 4                                  # gen = 9 >= 4: forced
        if "mask" in role:
            self.stop_at[role["mask"]] = 50                                  # gen = 5 < 50: the EOS is masked
        self.finish = np.full(S, FIN_CANARY, np.uint8)
        self.end_idx = np.full(S, CANARY32, np.int32)
        self.margin = np.full(S, MARGIN_CANARY, f32)
        for b in self.row_of:
            self.finish[b], self.end_idx[b] = 0, h[b]
        if "prefin" in role:
            self.finish[role["prefin"]] = 1
        self.kv_start = rs.randint(0, TCAP + 2, size=S).astype(np.int32)     # (the fold's descriptors and RoPE rows)
        self.kv_start[live[0]] = 0
        if variant == "teacher":
            self.teacher = rs.randint(0, 600, size=(S, TSTRIDE, NVQ)).astype(np.int64)
            if "teach_eos" in role:
                self.teacher[role["teach_eos"], 4, 3] = EOS
        else:
            self.teacher = None
        if text:         # one sampling row per utterance: a spike would take q out of the draw, so the EOS is what the `eos` utterance draws anyway
            self.eos = int(self.draw(role["eos"])[0])

    def cfg(self, b):
        return TEXT_CFG if self.text else CALL_WIDE if self.cfgs is None else self.cfgs[b]

    def len_of(self, b):
        return int(self.lens[b])

    def draw(self, b, lg=None, q=None, hist=None, base=None, drop_oldest=False):
        """oracle/sampling_np.py on logits row `lg` (default: b's own compact row), the draws of utterance `q`, the history of `hist`,
        the global row of `base`; its own length, parameters and hooks"""
        m = self.row_of[b] if lg is None else lg
        qb, hb, bb = (b if v is None else v for v in (q, hist, base))
        n, gen, c = self.nrow, self.len_of(b) - int(self.plen[b]), self.cfg(b)
        hist_rows = self.ids[hb, self.plen[hb]: self.lens[hb], :n].T          # [n, h]
        if drop_oldest and hist_rows.shape[1]:
            hist_rows = hist_rows[:, -(min(hist_rows.shape[1], 16) - 1):] if min(hist_rows.shape[1], 16) > 1 else hist_rows[:, :0]
        sa = int(self.stop_at[b])
        mask = gen < c["min_new"] or (sa >= 0 and gen < sa)
        force = np.full(n, sa >= 0 and gen >= sa)
        pt = None if self.text else rng.penalty_table(c["rep"])
        return sampling_np.sample_step(self.logits[m * n: m * n + n], np.ascontiguousarray(hist_rows), self.q[gen % NQ, qb * n: qb * n + n],
                                       temperature=np.asarray(c["temps"][:n], f32), top_p=c["top_P"], top_k=c["top_K"],
                                       pow_table=None if pt is None else pt.numpy(), max_input_ids=self.V - 1 if self.text else 625, mask_eos=mask,
                                       force_eos=force, eos=self.eos, row_offset=int(self.row_base[bb]))

    def expect(self):
        """numpy restatement of the bookkeeping at the end of sample_k / sample_text_k.  Returns the arrays after the launch, the
        utterances whose margin must have been lowered, and {b: (finished, tokens)} of the rows that sampled."""
        ids, lens, fin, end = self.ids.copy(), self.lens.copy(), self.finish.copy(), self.end_idx.copy()
        sampled = np.full((self.S, TSTRIDE, NVQ), IDS_CANARY, np.int64)
        lowered, done = [], {}
        for b in self.row_of:
            ln = self.len_of(b)
            if ln >= TCAP:                                                   # slot full: the flag and nothing else
                fin[b] = 1
                continue
            gen = ln - int(self.plen[b])
            tok = self.draw(b)
            if gen < TSTRIDE and not self.text:
                sampled[b, gen] = tok
            if self.teacher is not None and gen < TSTRIDE:
                tok = self.teacher[b, gen]
            ids[b, ln] = tok if not self.text else tok[0]
            f = bool(fin[b]) or bool((tok == self.eos).any())
            fin[b] = int(f)
            end[b] += 0 if f else 1
            lens[b] = ln + 1
            if not (self.stop_at[b] >= 0 and gen >= self.stop_at[b]):
                lowered.append(b)
            done[b] = (f, np.asarray(tok))
        return dict(ids=ids, lens=lens, finish=fin, end_idx=end, sampled=sampled), lowered, done

    def check_inputs_separate(self, done):
        """on the oracle alone: a swapped index cannot pass.  The tokens written are pairwise distinct across utterances, and every
        sampling utterance's draw changes when its logits or its q come from the neighbouring compact row, or its history does (an
        utterance at global rows >= 625 has no penalty and so no history: there the draw changes with the neighbour's row_base
        instead); and with the OLDEST token of its 16-token window missing"""
        toks = [tuple(int(t) for t in v[1]) for v in done.values()]
        assert len(set(toks)) == len(toks), toks
        # (a forced EOS draws nothing: it is left out, also as a neighbour)
        order = [int(b) for b in self.rows if b >= 0 and int(b) in done and not (self.stop_at[b] >= 0 and self.len_of(b) - self.plen[b] >= self.stop_at[b])]
        for i, b in enumerate(order):
            own = self.draw(b)
            penalised = not self.text and self.row_base[b] + 3 < 625
            if penalised and self.len_of(b) > self.plen[b]:
                assert not np.array_equal(own, self.draw(b, drop_oldest=True)), ("oldest", b)
            if len(order) < 2:
                continue
            nb = order[(i + 1) % len(order)]
            assert not np.array_equal(own, self.draw(b, lg=self.row_of[nb])), ("logits", b, nb)
            assert not np.array_equal(own, self.draw(b, q=nb)), ("q", b, nb)
            if penalised:
                assert not np.array_equal(own, self.draw(b, hist=nb)), ("history", b, nb)
            elif not self.text:
                assert not np.array_equal(own, self.draw(b, base=nb)), ("row_base", b, nb)


def _run_sample(G, c, fold=None):
    """one ctts_k_sample_rows launch of case `c`; `fold`: None or an emit_row format of the front tests ("rows" | "packed" | "x3" | "f32")"""
    keep = []
    d = lambda a: (keep.append(G.dev(a)), keep[-1])[1]
    s = _lib.GenState()
    s.B, s.T, s.max_new, s.cap, s.hid_cap, s.q_batch, s.nq, s.eos = c.S, 99, TCAP, TCAP, TSTRIDE, c.q_rows, NQ, c.eos
    lens_in = c.lens.copy()
    if c.mode == "desc":
        lens_in[list(c.row_of)] = 0
    st = dict(ids=d(c.ids), lens=d(lens_in), finish=d(c.finish), end_idx=d(c.end_idx), margin=d(c.margin),
              sampled=d(np.full((c.S, TSTRIDE, NVQ), IDS_CANARY, np.int64)))
    s.ids_buf, s.len, s.finish, s.end_idx, s.margin = (st[k].data_ptr() for k in ("ids", "lens", "finish", "end_idx", "margin"))
    s.q, s.prompt_len, s.stop_at, s.row_base = d(c.q).data_ptr(), d(c.plen).data_ptr(), d(c.stop_at).data_ptr(), d(c.row_base).data_ptr()
    if not c.text:
        s.sampled_ids = st["sampled"].data_ptr()
    if c.teacher is not None:
        s.teacher_ids = d(c.teacher).data_ptr()
    if c.cfgs is None:
        cw = c.cfg(0)
        s.temperature = d(np.asarray(cw["temps"], f32)).data_ptr()
        s.pow_table = None if c.text else d(rng.penalty_table(cw["rep"]).numpy()).data_ptr()
        s.top_p_thr, s.use_top_p, s.top_k, s.use_top_k, s.min_new = float(f32(1.0 - cw["top_P"])), 1, cw["top_K"], 1, cw["min_new"]
    else:
        table = [sampling_row(request_params(dict(temperature=t["temps"], top_P=t["top_P"], top_K=t["top_K"], repetition_penalty=t["rep"],
                                                  min_new_token=t["min_new"]))) for t in c.cfgs]
        s.row_sampling = d(np.frombuffer(b"".join(bytes(r) for r in table), np.uint8).copy()).data_ptr()
    R = c.R
    if c.mode == "desc":
        desc_in = d(np.array([G.DESC_ABSENT if b < 0 else G.row_desc(b, c.len_of(b) - 1, c.kv_start[b]) for b in c.rows], np.int32))
        rm = na = None
    else:
        desc_in, rm, na = None, d(c.row_map), d(np.array([c.n_live], np.int32))
    out = {}
    args = [None] * 12
    if fold is not None:
        code_d, _, cos_d, sin_d = _tables_dev()
        Rp = _ceil16(R)
        out["x"] = _nan(G, R, HID)
        out["desc"] = torch.full((R, 4), G.CANARY32, dtype=torch.int32, device=G.DEV)
        out["rope"] = _nan(G, R, 64)
        xb = None if fold == "f32" else torch.full({"rows": (R * HID,), "packed": (Rp * HID,), "x3": (2 * Rp * HID,)}[fold], G.CANARY16,
                                                   dtype=torch.int16, device=G.DEV)
        out["ssq"] = _nan(G, R, 48) if fold in ("rows", "packed") else None
        xp32 = _nan(G, Rp * HID) if fold == "f32" else None
        args = [code_d.data_ptr(), out["x"].data_ptr(), _lib.ptr(xb), _lib.ptr(out["ssq"]), out["desc"].data_ptr(), d(c.kv_start).data_ptr(),
                1 if fold in ("packed", "x3") else 0, _lib.ptr(xp32), Rp * HID if fold == "x3" else 0, out["rope"].data_ptr(), cos_d.data_ptr(),
                sin_d.data_ptr()]
    else:
        args[6], args[8] = 0, 0
    _lib.check(_lib.lib().ctts_k_sample_rows(C.byref(s), d(c.logits.reshape(R, -1)).data_ptr(), c.text, R, _lib.ptr(rm), _lib.ptr(na), _lib.ptr(desc_in),
                                             *args, None), "ctts_k_sample_rows")
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in st.items()}
    if fold is not None:
        Rp = _ceil16(R)
        got["fold"] = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
        if fold == "f32":
            got["fold"]["xp32"] = E.unpack_frag32(xp32.cpu(), Rp, HID).numpy()
        elif fold == "rows":
            got["fold"]["xb"] = xb.cpu().reshape(1, R, HID).numpy()
        elif fold == "packed":
            got["fold"]["xb"] = E.unpack_frag(xb.cpu(), Rp, HID)[None].numpy()
        else:
            got["fold"]["xb"] = torch.stack([E.unpack_frag(p, Rp, HID) for p in xb.cpu().reshape(2, Rp * HID)], 0).numpy()   # [hi | lo'][Rp][768]
    return got


def _check_bookkeeping(c, got, want, lowered):
    for name in ("ids", "finish", "end_idx"):
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:6].tolist())
    if c.mode == "desc":                                                     # len[b] = desc.slot + 2, whatever the array held
        want_len = want["lens"].copy()
        assert np.array_equal(got["lens"][list(c.row_of)], [want_len[b] if c.len_of(b) < TCAP else 0 for b in c.row_of])
        others = [b for b in range(c.S) if b not in c.row_of]
        assert np.array_equal(got["lens"][others], c.lens[others])
    else:
        assert np.array_equal(got["lens"], want["lens"])
    if not c.text:
        assert np.array_equal(got["sampled"], want["sampled"]), np.argwhere(got["sampled"] != want["sampled"])[:6].tolist()
    for b in range(c.S):                                                     # lowered for the utterances that sampled, bit-equal elsewhere
        if b in lowered:
            assert 0 <= got["margin"][b] < MARGIN_CANARY, b
        else:
            assert got["margin"][b].view(np.uint32) == MARGIN_CANARY.view(np.uint32), b
    unlisted = [b for b in range(c.S) if b not in c.row_of]                  # (the array comparisons above cover them; said once more by name)
    assert (got["finish"][unlisted] == FIN_CANARY).all() and (got["end_idx"][unlisted] == CANARY32).all()


C_CASES = [(S, n, mode, "plain") for S in (12, 70) for n in (1, 5, S) for mode in ("map", "desc")] + \
          [(S, n, mode, v) for S, n in ((12, 5), (70, 70)) for mode in ("map", "desc") for v in ("table", "teacher")]


@pytest.mark.parametrize("S,n_live,mode,variant", C_CASES)
def test_sample_rows_bookkeeping(G, S, n_live, mode, variant):
    """sample_k over R compact rows of S slots: logits by row, everything else by utterance -- prompt_len, a history of 0 .. 20
    tokens (so gen and gen % 3 differ), row_base, q_rows > R, in one variant a sampling table, in one teacher forcing.  Each row ==
    oracle/sampling_np.py on (logits[m], history[b], q[gen % 3, b]); ids_buf[b, len], len, finish (sticky; EOS in one codebook; a full
    slot sets it and writes nothing else), end_idx, stop_at's force and mask, teacher / sampled, margin; everything of an utterance
    that is not in the list keeps its sentinel."""
    c = SampleCase(S, n_live, mode, variant)
    want, lowered, done = c.expect()
    c.check_inputs_separate(done)
    r = c.role
    if "eos" in r:
        assert r["full"] not in done and want["finish"][r["prefin"]] == 1 and want["end_idx"][r["prefin"]] == c.end_idx[r["prefin"]]
        assert variant == "teacher" or (done[r["eos"]][0] and (done[r["eos"]][1] == EOS).sum() == 1)    # EOS in ONE codebook finishes the row
    if "force" in r and variant == "plain":
        assert (done[r["force"]][1] == EOS).all() and r["force"] not in lowered
        assert not done[r["mask"]][0] and not done[r["min_new"]][0]          # the dominant EOS is masked: by stop_at, by min_new
    if "teach_eos" in r and variant == "teacher":
        assert done[r["teach_eos"]][0] and any(c.len_of(b) - c.plen[b] >= TSTRIDE for b in done)   # forced and unforced rows in one launch
    got = _run_sample(G, c)
    _check_bookkeeping(c, got, want, lowered)


# ---- (d) sample_text_k ----------------------------------------------------------------------------------------------------------------
def test_sample_text_rows_bookkeeping(G):
    """the refine-text sampler (one sampling row per utterance, the token replicated over the 4 slots, 300 text tokens) through
    row_map + n_active with a prompt_len per utterance, against the oracle of tests/test_gpu_text_pool.py"""
    c = SampleCase(12, 5, "map", "plain", text=300)
    want, lowered, done = c.expect()
    c.check_inputs_separate(done)
    assert done[c.role["eos"]][0] and c.role["full"] not in done
    got = _run_sample(G, c)
    _check_bookkeeping(c, got, want, lowered)


# ---- (e) the EmbedNext fold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_live", [(12, 5), (70, 70)])
@pytest.mark.parametrize("fmt", ["rows", "packed", "x3", "f32"])
def test_sample_fold_equals_the_next_steps_first_kernel(G, fmt, S, n_live):
    """sample_k with the next step's first kernel folded into its tail == embed_codes_k (ctts_k_step_prep, host compaction, the same
    compact rows) launched on the state the sampler left: x, the 16-bit copies / the packed f32 copy, the partial sums of squares, the
    RoPE factors and the descriptor of every continuing row bit for bit, in every format of emit_row; one row draws the table's row
    of edge values.  A row that finishes in this launch gets b = -1 in its descriptor and nothing else.
    PINNED, not specified: a row that is absent on entry and a row whose slot is full leave every fold output of the row untouched,
    the descriptor included -- the next embed_codes_k launch re-ranks the finish flags and overwrites them (kernels.hpp EmbedNext)."""
    c = SampleCase(S, n_live, "desc", "plain")
    edge = c.role["h20"]
    c.logits[c.row_of[edge] * NVQ: c.row_of[edge] * NVQ + NVQ, EDGE_CODE] = 40.0       # all four codebooks draw the edge row
    want, lowered, done = c.expect()
    assert (done[edge][1] == EDGE_CODE).all() and done[c.role["eos"]][0]
    got = _run_sample(G, c, fold=fmt)
    _check_bookkeeping(c, got, want, lowered)
    f = got["fold"]
    R = c.R
    cont = [m for m, b in enumerate(c.rows) if b >= 0 and int(b) in done and not done[int(b)][0]]
    fins = [m for m, b in enumerate(c.rows) if b >= 0 and int(b) in done and done[int(b)][0]]
    quiet = [m for m in range(R) if m not in cont and m not in fins]                    # absent on entry, or the slot is full
    assert cont and fins and quiet and c.row_of[c.role["full"]] in quiet and len(fins) >= 2
    # the next step's first kernel on the post-sample state; a row without an utterance reads slot 0's (not compared)
    row_map = np.array([max(int(b), 0) for b in c.rows], np.int32)
    ref = _step(G, R, got["ids"], want["lens"], tcap=TCAP, row_map=row_map, n_active=R, kv_start=c.kv_start, finish=got["finish"],
                fmt=None if fmt == "f32" else fmt, xp32=fmt == "f32", ssq=fmt in ("rows", "packed"), desc=True, rope=True)
    assert np.array_equal(f["desc"][cont + fins], ref["desc"][cont + fins])
    for m in cont + fins:
        b = int(c.rows[m])
        assert f["desc"][m].tolist() == list(G.row_desc(b, c.len_of(b), c.kv_start[b], m in fins))   # slot = the token just written
    assert (f["desc"][quiet] == G.CANARY32).all()
    ref_xb = None if fmt == "f32" else ref["xb"].numpy().reshape(f["xb"].shape)
    for name, a, w in (("x", f["x"], ref["x"]), ("rope", f["rope"], ref["rope"]), ("ssq", f["ssq"], ref["ssq"]), ("xp32", f.get("xp32"), ref.get("xp32"))):
        if a is None:
            continue
        assert np.array_equal(_bits(a[cont]), _bits(w[cont])), name
        assert np.isnan(a[fins + quiet]).all() and np.isnan(a[R:]).all(), name
    assert np.array_equal(f["x"][c.row_of[edge]], _embed_ref([EDGE_CODE] * NVQ, False))
    if fmt != "f32":
        assert np.array_equal(f["xb"][:, cont], ref_xb[:, cont])
        rest = [m for m in range(f["xb"].shape[1]) if m not in cont]
        assert (f["xb"][:, rest] == G.CANARY16).all()

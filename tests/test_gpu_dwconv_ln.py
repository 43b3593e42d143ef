"""The depthwise conv + LayerNorm family of csrc/codec.hip behind `launch_dwconv_ln`, through `ctts_k_dwconv_ln_ex`: three kernels
(`dwconv_ln_k`: one wave per frame, every size below 12,288 frames and the only C = 256 kernel; `dwconv_ln_run_k`: the register ring
over 36-frame runs, dilations 1-4; `dwconv_ln_seq_k`: the ring + the wave-private LDS transpose with partial flushes, planes only),
three output formats (f32 rows, hi | lo bf16 planes in gemm_x3p_k's fragment order, one fp16 plane in gemm_h1p_k's), plain or over
packed segments.

ONE anchor against a reference -- the f32 rows of `dwconv_ln_k` against oracle/codec_np within the project's 2e-5 -- and everything
else exact, bit for bit: planes == the host packing of the rows, no write outside the rows' own slots, ring kernels == the plain
kernel, packed segments == each segment alone, degenerate statistics, refusals launch nothing.  A failure names the first differing
(row, plane, 16-channel block)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E  # noqa: E402
from oracle import codec_np  # noqa: E402
from tests.gpu_util import ragged_edge_layout  # noqa: E402

f32 = np.float32
EPS = 1e-6
BAR = 2e-5            # test_dwconv_ln's bar: max |kernel - oracle| on O(1) outputs
# untouched slots: the int16 pattern of a plane buffer (as bf16 1.5e16, as fp16 203.25) and the int32 pattern of an f32 row buffer.
# Only slots the kernel must NOT write are compared with them.
CANARY16, CANARY32 = 0x5A5A, 0x5A5A5A5A
SMALL = [(1, 1), (1, 2), (3, 5), (2, 29), (2, 35), (1, 257)]   # frames with every side tap outside, rows % 4 != 0, rows across 32- and
#                                                                  256-row plane tiles, a grid padded to 8 workgroups
BIG = [(342, 37), (200, 70), (164, 75), (251, 49), (13, 1000), (7, 1900)]   # >= 12,288 rows: run tails of 1, 34, 3 and 28 frames, every
#                          t & 3 residue of seq's partial flush, utterances shorter than two runs, the 48-frame DIL-2 run ending one frame into the next
# (CTTS_DWCONV_SEQ, dil) -> the kernel that writes the PLANES of a >= 12,288-row launch (rows always come from dwconv_ln_run_k)
RING = [("0", 1), ("0", 2), ("0", 3), ("0", 4), ("1", 1), ("2", 2)]
RING_IDS = ["run-d1", "run-d2", "run-d3", "run-d4", "seq-d1", "seq-d2"]
FMTS = ("bf16", "f16")
NP_OF = {"bf16": 2, "f16": 1}


@pytest.fixture(scope="module")
def G():
    from tests import gpu_util
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return gpu_util


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _inputs(seed, B, F, C):
    """test_dwconv_ln's distributions: x ~ N(0, 1), w = 0.4 N(0, 1) as [C, 1, 7], b and ln_b = 0.1 N(0, 1), ln_w = 1 + 0.1 N(0, 1)"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, F, C)).astype(f32)
    w = rs.standard_normal((C, 1, 7)).astype(f32) * f32(0.4)
    b = rs.standard_normal(C).astype(f32) * f32(0.1)
    lw = (1 + 0.1 * rs.standard_normal(C)).astype(f32)
    lb = rs.standard_normal(C).astype(f32) * f32(0.1)
    return x, w, b, lw, lb   # shared between tests: never written (a test that edits an input copies it)


class Params:
    """the device copies of one parameter set (w transposed to [7][C] as the kernels read it)"""

    def __init__(self, G, w, b, lw, lb):
        self.C = int(b.shape[0])
        self.dev = [G.dev(np.ascontiguousarray(w[:, 0, :].T)), G.dev(b), G.dev(lw), G.dev(lb)]


def _ref64(x, w, b, lw, lb, dil):
    """float64 throughout: the depthwise conv (zero padding 3 dil), then LayerNorm with the biased variance"""
    B, F, C = x.shape
    xp = np.zeros((B, F + 6 * dil, C), np.float64)
    xp[:, 3 * dil: 3 * dil + F] = x
    y = np.zeros((B, F, C), np.float64) + b.astype(np.float64)
    for j in range(7):
        y += xp[:, j * dil: j * dil + F] * w[:, 0, j].astype(np.float64)
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).mean(-1, keepdims=True)
    return (y - mu) / np.sqrt(var + EPS) * lw.astype(np.float64) + lb.astype(np.float64)


def _twin32(x, w, b, lw, lb, dil):
    """the same formula with every intermediate in float32 NumPy: what float32 alone costs on these inputs"""
    B, F, C = x.shape
    xp = np.zeros((B, F + 6 * dil, C), f32)
    xp[:, 3 * dil: 3 * dil + F] = x
    y = np.zeros((B, F, C), f32) + b
    for j in range(7):
        y += xp[:, j * dil: j * dil + F] * w[:, 0, j]
    mu = y.mean(-1, keepdims=True, dtype=f32)
    d = y - mu
    var = (d * d).mean(-1, keepdims=True, dtype=f32)
    return d * (f32(1) / np.sqrt(var + f32(EPS))) * lw + lb


# ---- launches ----------------------------------------------------------------------------------------------------------------
def _ceil(n, m):
    return (n + m - 1) // m * m


def _launch(x_d, P, dil, B, F, y, yp=None, plane_f16=0, seg=None, C=None):
    return _lib.lib().ctts_k_dwconv_ln_ex(x_d.data_ptr(), *[t.data_ptr() for t in P.dev], EPS, dil, _lib.ptr(y), B, F, P.C if C is None else C,
                                          _lib.ptr(yp), plane_f16, _lib.ptr(seg), None)


def _rows(x_d, P, dil, B, F, seg=None):
    """f32 rows [B F, C] (device).  The buffer starts as NaN: a row the kernel skipped cannot pass a comparison."""
    y = torch.full((B * F, P.C), float("nan"), dtype=torch.float32, device=x_d.device)
    _lib.check(_launch(x_d, P, dil, B, F, y, seg=seg), "ctts_k_dwconv_ln_ex rows")
    return y


def _unpack(p, fmt, C=512):
    """planes in fragment order (int16 words) -> [rows, plane, C] in row order: a bijection of the slots, so comparing in this
    order compares every slot -- and a difference has a (row, plane, channel) name"""
    if fmt == "bf16":    # [rows/32][C/16][hi | lo][(k % 16) / 8][r % 32][k % 8]
        return p.reshape(-1, C // 16, 2, 2, 32, 8).permute(0, 4, 2, 1, 3, 5).reshape(-1, 2, C)
    return p.reshape(-1, C // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(-1, 1, C)   # [rows/32][C/16][(k % 16) / 8][r % 32][k % 8]


def _planes(x_d, P, dil, B, F, fmt, seg=None, what=""):
    """the plane output [B F, planes, C] int16 of one launch.  b. no stray writes: the plane buffer is ceil256(B F) + 256 rows of a
    canary pattern and every slot of a row >= B F must keep it; the launch also gets a real, canary-filled y, which must come back
    untouched."""
    R, C = B * F, P.C
    cap = _ceil(R, 256) + 256
    yp = torch.full((cap * C * NP_OF[fmt],), CANARY16, dtype=torch.int16, device=x_d.device)
    y = torch.full((R * C,), CANARY32, dtype=torch.int32, device=x_d.device)
    _lib.check(_launch(x_d, P, dil, B, F, y, yp, int(fmt == "f16"), seg), f"ctts_k_dwconv_ln_ex {fmt} planes")
    rows = _unpack(yp, fmt, C)
    stray = rows[R:] != CANARY16
    if bool(stray.any()):
        r, p, c = (int(v) for v in torch.nonzero(stray)[0])
        pytest.fail(f"{what} {fmt} planes, B {B} F {F} dil {dil}: wrote row {R + r} >= B F = {R} (plane {p}, channel block {c // 16})")
    assert bool((y == CANARY32).all()), f"{what} {fmt} planes, B {B} F {F} dil {dil}: the f32 row buffer was written in plane mode"
    return rows[:R].contiguous()


def _pack(rows, fmt):
    """engine.pack_x3p / pack_h1p of f32 rows [R, C] (zero padded to a multiple of 32 rows), as [R, planes, C] int16"""
    R, C = rows.shape
    pad = torch.zeros((_ceil(R, 32), C), dtype=torch.float32, device=rows.device)
    pad[:R] = rows
    p = (E.pack_x3p if fmt == "bf16" else E.pack_h1p)(pad)
    return _unpack(p.view(torch.int16), fmt, C)[:R]


def _assert_same(got, want, what):
    """bit for bit; reports the first differing (row, plane, 16-channel block) like test_gpu_ragged_codec_edges._first_diff"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if got.dtype == torch.float32:
        got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)   # NaN == NaN, -0 != +0
    if torch.equal(got, want):
        return
    g3, w3 = (t.reshape(t.shape[0], -1, t.shape[-1]) for t in (got, want))
    ne = g3 != w3
    r, p, c = (int(v) for v in torch.nonzero(ne)[0])
    m = 0xffff if got.dtype == torch.int16 else 0xffffffff
    pytest.fail(f"{what}: {int(ne.any(-1).any(-1).sum())} of {g3.shape[0]} rows differ, first at row {r}, plane {p}, channel block {c // 16} "
                f"(channel {c}): got 0x{int(g3[r, p, c]) & m:x}, want 0x{int(w3[r, p, c]) & m:x}")


def _seg_table(G, lens):
    """seg[f] = [lo, hi) in frames of frame f's segment, for token lengths `lens` (2 frames per token)"""
    edges = np.concatenate([[0], 2 * np.cumsum(lens)]).astype(np.int64)
    n = np.diff(edges)
    tab = np.stack([np.repeat(edges[:-1], n), np.repeat(edges[1:], n)], 1).astype(np.int32)
    return edges, G.dev(tab)


# ---- the anchor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dil", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [512, 256])
def test_rows_of_the_plain_kernel_against_float64(G, C, dil, capsys):
    """`dwconv_ln_k`'s f32 rows vs codec_np.layer_norm(codec_np.dwconv1d_cl(.)) < 2e-5 at every small shape.  Printed next to it: the
    kernel's and a float32 NumPy twin's distance from an all-float64 evaluation -- the twin says what float32 costs on these inputs
    (measured on the CPU at 0.8-1.5e-6); were it above a quarter of the bar, the INPUT would be ill conditioned, not the kernel."""
    worst = [0.0, 0.0, 0.0]
    for B, F in SMALL:
        x, w, b, lw, lb = _inputs(100 * dil + B + F, B, F, C)
        P = Params(G, w, b, lw, lb)
        got = _rows(G.dev(x), P, dil, B, F).cpu().numpy().reshape(B, F, C)
        ref = codec_np.layer_norm(codec_np.dwconv1d_cl(x, w, b, pad=3 * dil, dil=dil), lw, lb, EPS)
        r64 = _ref64(x, w, b, lw, lb, dil)
        e_ref, e_k, e_t = (float(np.abs(a - r).max()) for a, r in ((got, ref), (got.astype(np.float64), r64), (_twin32(x, w, b, lw, lb, dil).astype(np.float64), r64)))
        worst = [max(a, e) for a, e in zip(worst, (e_ref, e_k, e_t))]
        assert np.isfinite(got).all(), (C, dil, B, F)
        assert e_t < BAR / 4, f"C {C} dil {dil} B {B} F {F}: the float32 twin is {e_t:.2e} from float64 -- change the input, not the bar"
        assert e_ref < BAR and e_k < BAR, f"C {C} dil {dil} B {B} F {F}: kernel vs oracle {e_ref:.2e}, vs float64 {e_k:.2e}"
    with capsys.disabled():
        print(f"\n  dwconv_ln_k C {C} dil {dil}: kernel vs oracle {worst[0]:.2e}, kernel vs float64 {worst[1]:.2e}, float32 twin vs float64 {worst[2]:.2e}")


@pytest.mark.parametrize("rows", [1, 3, 5, 58])
def test_layernorm_rows(G, rows):
    x, _, _, lw, lb = _inputs(7 + rows, 1, rows, 512)
    y = torch.full((rows, 512), float("nan"), dtype=torch.float32, device=G.DEV)
    keep = [G.dev(x), G.dev(lw), G.dev(lb)]
    _lib.check(_lib.lib().ctts_k_layernorm(*[k.data_ptr() for k in keep], EPS, y.data_ptr(), rows, None), "ctts_k_layernorm")
    err = float(np.abs(y.cpu().numpy() - codec_np.layer_norm(x[0], lw, lb, EPS)).max())
    assert err < BAR, err


def test_legacy_entry_is_the_new_one(G):
    """ctts_k_dwconv_ln (C = 512 rows, no planes, no segments) gives the bits of ctts_k_dwconv_ln_ex with the same arguments"""
    B, F = 2, 29
    x, w, b, lw, lb = _inputs(3, B, F, 512)
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    y = torch.full((B * F, 512), float("nan"), dtype=torch.float32, device=G.DEV)
    _lib.check(_lib.lib().ctts_k_dwconv_ln(x_d.data_ptr(), *[t.data_ptr() for t in P.dev], EPS, 2, y.data_ptr(), B, F, None), "ctts_k_dwconv_ln")
    _assert_same(y, _rows(x_d, P, 2, B, F), "ctts_k_dwconv_ln vs ctts_k_dwconv_ln_ex")


# ---- a. planes are the packing of the rows; b. no stray writes (inside _planes) ----------------------------------------------
@pytest.mark.parametrize("dil", [1, 2, 3, 4])
@pytest.mark.parametrize("fmt", FMTS)
def test_planes_of_the_plain_kernel_are_the_packed_rows(G, fmt, dil):
    for B, F in SMALL:
        x, w, b, lw, lb = _inputs(100 * dil + B + F, B, F, 512)
        P, x_d = Params(G, w, b, lw, lb), G.dev(x)
        rows = _rows(x_d, P, dil, B, F)
        _assert_same(_planes(x_d, P, dil, B, F, fmt, what="dwconv_ln_k"), _pack(rows, fmt), f"dwconv_ln_k {fmt} planes vs pack(rows), B {B} F {F} dil {dil}")


def _hot(lw):
    """a few LayerNorm weights of 3e4: the normalised value (O(1), up to ~4) times 3e4 leaves the half range (65504)"""
    lw = lw.copy()
    lw[[0, 7, 8, 255, 256, 511]] = 3e4
    lw[64: 448: 32] = 3e4
    return lw


@pytest.mark.parametrize("seq,dil,B,F", [("1", 1, 2, 35), ("0", 1, 342, 37), ("0", 3, 164, 75), ("1", 1, 251, 49), ("2", 2, 251, 49)],
                         ids=["plain", "run-d1", "run-d3", "seq-d1", "seq-d2"])
def test_fp16_plane_saturates_like_pack_h1p(G, monkeypatch, seq, dil, B, F):
    """outputs beyond the half range: the fp16 plane stays finite and holds pack_h1p's saturated values (+-65504), in all three kernels"""
    monkeypatch.setenv("CTTS_DWCONV_SEQ", seq)
    x, w, b, lw, lb = _inputs(11, B, F, 512)
    P, x_d = Params(G, w, b, _hot(lw), lb), G.dev(x)
    rows = _rows(x_d, P, dil, B, F)
    n_over = int((rows.abs() > 65504).sum())
    assert bool(torch.isfinite(rows).all()) and n_over > 0, "the input does not leave the half range"
    got = _planes(x_d, P, dil, B, F, "f16", what="saturating")
    assert not bool(((got & 0x7C00) == 0x7C00).any()), "an Inf / NaN in the fp16 plane"
    _assert_same(got, _pack(rows, "f16"), f"saturating fp16 plane vs pack_h1p(rows), B {B} F {F} dil {dil} CTTS_DWCONV_SEQ={seq}")
    assert int(((got & 0x7FFF) == 0x7BFF).sum()) >= n_over    # 0x7bff = 65504


# ---- c. the ring kernels equal the plain kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,dil", RING, ids=RING_IDS)
@pytest.mark.parametrize("B,F", BIG)
def test_ring_kernels_equal_the_plain_kernel(G, monkeypatch, B, F, seq, dil):
    """>= 12,288 rows: rows (dwconv_ln_run_k) and both plane formats (run_k under CTTS_DWCONV_SEQ=0 and at dilations 3, 4; seq_k under 1 at
    dilation 1 and under 2 at dilation 2) of the big launch == `dwconv_ln_k`'s on 3-utterance slices from the first and the last
    utterances, bit for bit; the planes == pack(rows) over ALL rows; the first 3 utterances within the bar of float64."""
    monkeypatch.setenv("CTTS_DWCONV_SEQ", seq)
    assert B * F >= 12288
    x, w, b, lw, lb = _inputs(B + F, B, F, 512)
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    who = f"B {B} F {F} dil {dil} CTTS_DWCONV_SEQ={seq}"
    rows = _rows(x_d, P, dil, B, F)
    err = float(np.abs(rows[: 3 * F].cpu().numpy().astype(np.float64) - _ref64(x[:3], w, b, lw, lb, dil).reshape(3 * F, 512)).max())
    assert err < BAR, (who, err)
    planes = {fmt: _planes(x_d, P, dil, B, F, fmt, what="ring") for fmt in FMTS}
    for fmt in FMTS:
        _assert_same(planes[fmt], _pack(rows, fmt), f"{who}: {fmt} planes vs pack(rows)")
    for lo in (0, B - 3):
        xs = x_d[lo: lo + 3].contiguous()
        sl = slice(lo * F, (lo + 3) * F)
        _assert_same(rows[sl], _rows(xs, P, dil, 3, F), f"{who}: rows of utterances {lo}..{lo + 2} vs dwconv_ln_k")
        for fmt in FMTS:
            _assert_same(planes[fmt][sl], _planes(xs, P, dil, 3, F, fmt, what="slice"), f"{who}: {fmt} planes of utterances {lo}..{lo + 2} vs dwconv_ln_k")


# ---- d. packed segments equal each segment alone -----------------------------------------------------------------------------
SEG_CASES = [(1000, "1", d) for d in (1, 2)] + [(t, s, d) for t in (12288, 12290) for s in ("0", "1", "2") for d in (1, 2)]


@pytest.mark.parametrize("total,seq,dil", SEG_CASES)
def test_packed_segments_equal_each_segment_alone(G, monkeypatch, total, seq, dil):
    """B = 1, seg[f] = the [lo, hi) of gpu_util.ragged_edge_layout(total) (1-token runs, boundaries on the 32 / 36 / 48 / 64 / 128 / 256
    edges): rows and both plane formats of every segment == the same frames launched alone (seg = null, F = its length).  1,000 frames
    run `dwconv_ln_k<SEG>`, the large totals `dwconv_ln_run_k<SEG>` / `dwconv_ln_seq_k<SEG>` as CTTS_DWCONV_SEQ says."""
    monkeypatch.setenv("CTTS_DWCONV_SEQ", seq)
    lens = ragged_edge_layout(total)
    edges, seg = _seg_table(G, lens)
    x, w, b, lw, lb = _inputs(total, 1, total, 512)
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    got = {"rows": _rows(x_d, P, dil, 1, total, seg=seg)}
    for fmt in FMTS:
        got[fmt] = _planes(x_d, P, dil, 1, total, fmt, seg=seg, what="packed")
    want = {k: torch.empty_like(v) for k, v in got.items()}
    for lo, hi in zip(edges[:-1], edges[1:]):
        xs, n = x_d[:, lo:hi].contiguous(), int(hi - lo)
        want["rows"][lo:hi] = _rows(xs, P, dil, 1, n)
        for fmt in FMTS:
            want[fmt][lo:hi] = _planes(xs, P, dil, 1, n, fmt, what="alone")
    for k in got:
        if not torch.equal(got[k].view(torch.int32 if k == "rows" else torch.int16), want[k].view(torch.int32 if k == "rows" else torch.int16)):
            ne = (got[k] != want[k]).reshape(total, -1).any(-1)
            r = int(torch.nonzero(ne)[0, 0])
            i = int(np.searchsorted(edges, r, side="right") - 1)
            _assert_same(got[k], want[k], f"{total} frames dil {dil} CTTS_DWCONV_SEQ={seq}: {k} of segment {i} (frames {edges[i]}..{edges[i + 1]}, "
                                          f"first bad frame {r - edges[i]} of {edges[i + 1] - edges[i]}) vs alone")


# ---- e. degenerate statistics ------------------------------------------------------------------------------------------------
DEGEN = [(None, 512, d, 3, 40) for d in (1, 2, 3, 4)] + [(None, 256, d, 3, 40) for d in (1, 2, 3, 4)] + \
        [("0", 512, d, 13, 1000) for d in (1, 2, 3, 4)] + [("1", 512, 1, 13, 1000), ("2", 512, 2, 13, 1000)]


@pytest.mark.parametrize("seq,C,dil,B,F", DEGEN)
def test_all_zero_utterance(G, monkeypatch, seq, C, dil, B, F):
    """one utterance of zeros between two random ones: each of its frames at least 3 dil from both edges sees nothing but the bias --
    all of them equal bit for bit (rows and planes) and within the bar of LN(b)"""
    if seq is not None:
        monkeypatch.setenv("CTTS_DWCONV_SEQ", seq)
    x, w, b, lw, lb = _inputs(5, B, F, C)
    x = x.copy()
    x[1] = 0
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    inner = slice(F + 3 * dil, 2 * F - 3 * dil)
    outs = {"rows": _rows(x_d, P, dil, B, F)}
    if C == 512:
        outs.update({fmt: _planes(x_d, P, dil, B, F, fmt, what="zero utterance") for fmt in FMTS})
    for k, v in outs.items():
        z = v[inner]
        _assert_same(z, z[:1].expand_as(z), f"C {C} dil {dil} B {B} F {F}: {k} of the all-zero utterance's inner frames vs the first of them")
    b64 = b.astype(np.float64)
    ln_b = (b64 - b64.mean()) / np.sqrt(b64.var() + EPS) * lw + lb
    err = float(np.abs(outs["rows"][inner].cpu().numpy() - ln_b).max())
    assert err < BAR, err


@pytest.mark.parametrize("seq,C,dil,B,F", DEGEN)
def test_zero_variance_rows_are_ln_b(G, monkeypatch, seq, C, dil, B, F):
    """x (per frame), w (per tap) and b constant over the channels: every conv output row is constant, so the variance is exactly 0 and
    the output is ln_b bit for bit -- (0 * rstd) * ln_w + ln_b with rstd = 1 / sqrt(eps) finite -- and never NaN.  The values are
    multiples of 1/8 below 4, so every product, the 7-tap sum and the 512-term channel sum are exact in float32: the mean IS the value."""
    if seq is not None:
        monkeypatch.setenv("CTTS_DWCONV_SEQ", seq)
    rs = np.random.RandomState(9)
    _, _, _, lw, lb = _inputs(5, B, F, C)
    x = np.repeat(rs.randint(-31, 32, (B, F, 1)).astype(f32) / 8, C, axis=2)
    w = np.repeat(rs.randint(-15, 16, (1, 1, 7)).astype(f32) / 8, C, axis=0)
    b = np.full(C, 0.375, f32)
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    rows = _rows(x_d, P, dil, B, F)
    want = G.dev(lb)[None].expand(B * F, C)
    assert not bool(torch.isnan(rows).any())
    _assert_same(rows, want, f"C {C} dil {dil} B {B} F {F}: zero-variance rows vs ln_b")
    if C == 512:
        for fmt in FMTS:
            _assert_same(_planes(x_d, P, dil, B, F, fmt, what="zero variance"), _pack(want.contiguous(), fmt), f"dil {dil} B {B} F {F}: zero-variance {fmt} planes vs pack(ln_b)")


# ---- f. refusals launch nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,C,B,planes,segs", [("planes at C = 256", 256, 2, True, False), ("segments with B = 2", 512, 2, False, True),
                                                  ("segments at C = 256", 256, 1, False, True), ("C = 384", 384, 2, False, False)])
def test_refusals_launch_nothing(G, what, C, B, planes, segs):
    """combinations the launcher has no kernel for: a non-zero return, ctts_last_error names the entry, and the canary-filled outputs
    (sized for C = 512, whatever C says) come back untouched"""
    F = 16
    x, w, b, lw, lb = _inputs(1, B, F, 512)
    P, x_d = Params(G, w, b, lw, lb), G.dev(x)
    y = torch.full((B * F * 512,), CANARY32, dtype=torch.int32, device=G.DEV)
    yp = torch.full((512 * 512 * 2,), CANARY16, dtype=torch.int16, device=G.DEV)
    seg = G.dev(np.tile(np.array([[0, F]], np.int32), (B * F, 1))) if segs else None
    for fmt16 in (0, 1):
        rc = _launch(x_d, P, 1, B, F, y, yp if planes else None, fmt16, seg, C=C)
        torch.cuda.synchronize()
        assert rc != 0, what
        assert "ctts_k_dwconv_ln_ex" in _lib.lib().ctts_last_error().decode(), what
        with pytest.raises(_lib.EngineError, match="ctts_k_dwconv_ln_ex"):
            _lib.check(rc, what)
        assert bool((y == CANARY32).all()) and bool((yp == CANARY16).all()), f"{what}: an output buffer was written"

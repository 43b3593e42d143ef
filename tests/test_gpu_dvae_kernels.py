"""The full DVAE's own kernels (csrc/dvae.hip) one by one: `stft_mag_k`, the log-mel epilogue of `gemm_tiled_f32_k`, the stride-2
convolution run as a k3 convolution over frame pairs, `gfsq_encode_k` (both residual loops), `gfsq_embed_k`, then the encode chain at
its shortest clips and on a poisoned workspace.  Every kernel is launched alone through the C ABI at the smallest shapes where it can
go wrong, against the float64 / numpy restatements of oracle/dvae_np.py.  Bounds are derived in the test that uses them; every output
buffer starts as NaN (or -1) and is longer than what the kernel may write.

tests/test_gpu_dvae.py keeps the end-to-end check on the golden clips; what it cannot see under the trunk's float32 noise -- a reflect
index, the index basis, the residual scale, the row guard, the pad columns, a read of uninitialised workspace -- is pinned here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from chattts_amd.dvae import DvaeEngine, pair_repack_k4s2  # noqa: E402
from oracle import codec_np, dvae_np  # noqa: E402

f32 = np.float32
DEV = torch.device("cuda:0")
NAN = float("nan")
U = 2.0 ** -24
NBIN, MAGLD, NMEL, HOP = 513, 516, 100, 256
WIN_KEY, FB_KEY = "preprocessor_mel.mel_spec.spectrogram.window", "preprocessor_mel.mel_spec.mel_scale.fb"
LEVELS = np.array([5, 5, 5, 5])
MODES = [True, False]                                  # bound_first: the current library's residual loop, and the older one


# ---- host side: inputs and oracle figures (no GPU; the caps on boundary cases are asserted from these) -------------------------
def one_hot_sd(sd):
    """`project_in` picks single input elements: group g, coordinate d <- channel 128 d + 4 g + 1 of the group's 512, bias 0, so
    that z[d] IS one input element, exactly, on the device and in the oracle"""
    out = dict(sd)
    for g in range(2):
        w = torch.zeros((4, 512), dtype=torch.float32)
        for d in range(4):
            w[d, 128 * d + 4 * g + 1] = 1.0
        out[f"vq_layer.quantizer.rvqs.{g}.project_in.weight"] = w
        out[f"vq_layer.quantizer.rvqs.{g}.project_in.bias"] = torch.zeros(4, dtype=torch.float32)
    return out


def one_hot_feat(z: np.ndarray) -> np.ndarray:
    """z [rows, 2, 4] (group, coordinate) -> features [rows, 1024] that `one_hot_sd` projects back onto z; the other channels carry
    finite noise, which meets zero weights"""
    rows = z.shape[0]
    feat = np.random.RandomState(rows).standard_normal((rows, 1024)).astype(f32)
    for g in range(2):
        for d in range(4):
            feat[:, 512 * g + 128 * d + 4 * g + 1] = z[:, g, d]
    return feat


def level_tuple_z(bound_first: bool) -> np.ndarray:
    """[625, 2, 4]: row i aims at level tuple i (coordinate 0 the fastest digit) in both groups.  The older loop rounds bound(z), so
    z = atanh(centre / half_l) lands on the level centres; the current loop bounds twice, which makes the outer centres unreachable:
    z well inside each level's interval instead"""
    digits = (np.arange(625)[:, None] // 5 ** np.arange(4)[None, :]) % 5                  # [625, 4]
    if bound_first:
        z = np.array([-3.0, -0.45, 0.0, 0.45, 3.0], dtype=f32)[digits]
    else:
        z = np.arctanh((digits - 2) / 2.002).astype(f32)
    return np.repeat(z[:, None, :], 2, axis=1).astype(f32)


SWEEP_N = 20001


def sweep_z() -> np.ndarray:
    """[20001, 2, 4]: coordinate d = g + 1 of group g runs over [-4, 4], the other three stay 0: every rounding boundary of both
    residual levels is crossed in 4e-4 steps"""
    z = np.zeros((SWEEP_N, 2, 4), dtype=f32)
    for g in range(2):
        z[:, g, g + 1] = np.linspace(-4.0, 4.0, SWEEP_N).astype(f32)
    return z


def digits_of(codes: np.ndarray) -> np.ndarray:
    return (codes[..., None] // 5 ** np.arange(4)) % 5


def real_feat() -> np.ndarray:
    return np.random.RandomState(7).standard_normal((4099, 1024)).astype(f32)


CHAIN_NS = [513, 767, 768, 1023, 1024, 1279, 1280, 2047, 2048, 2305]       # F = 3 ... 10 frames, T = 1 ... 5, odd and even F
CHAIN_KINDS = ["noise", "faint", "silence"]


def chain_clips():
    """{(n, kind): wav}: N(0, 0.3) noise, N(0, 1e-4) noise and exact silence at every length.  No tones or constants here: their far
    mel bands sit at the 1e-5 clamp, where any float32 FFT legitimately moves the log (they are covered on the mel stage alone)"""
    rs = np.random.RandomState(11)
    out = {}
    for n in CHAIN_NS:
        out[n, "noise"] = (0.3 * rs.standard_normal(n)).astype(f32)
        out[n, "faint"] = (1e-4 * rs.standard_normal(n)).astype(f32)
        out[n, "silence"] = np.zeros(n, f32)
    return out


def chain_oracle(nsd, wav):
    """-> (codes [T, 4], margins [T, 4]) of one clip, the trunk evaluated once"""
    mel = dvae_np.mel_features(wav, nsd[WIN_KEY], nsd[FB_KEY])
    feat = dvae_np.encoder_features(nsd, mel)
    return dvae_np.gfsq_encode(nsd, feat), dvae_np.gfsq_round_margin(nsd, feat)


def check_codes_by_margin(got, want, marg, thr, what):
    """the rule of tests/test_gpu_dvae.py: a code may differ from the oracle's only where one of its pre-rounding coordinates lies
    within `thr` of a rounding boundary, or (r = 1) downstream of a flipped r = 0 of the same group"""
    same = got == want
    for t, c in zip(*np.nonzero(~same)):
        near = marg[t, c] < thr
        downstream = (c % 2 == 1) and not same[t, c - 1]
        assert near or downstream, (what, int(t), int(c), int(got[t, c]), int(want[t, c]), float(marg[t, c]))
    return int((~same).sum())


def signals(n: int):
    i = np.arange(n)
    return {
        "noise": (0.3 * np.random.RandomState(n).standard_normal(n)).astype(f32),
        "ramp": (i / n).astype(f32),                     # any off-by-one or edge repeat of the reflect moves the result by O(1)
        "const": np.full(n, 0.25, f32),
        "sine": np.sin(2.0 * np.pi * 440.0 * i / 24000.0).astype(f32),
        "zeros": np.zeros(n, f32),
    }


def logmel_rows(fb: np.ndarray) -> np.ndarray:
    """[65, 516] non-negative magnitude rows: row 0 puts every mel sum within a factor 2 of the 1e-5 clamp (on both sides of it),
    row 1 is all zeros, the rest are |N(0,1)| scaled by 1e-7 ... 1e2"""
    rs = np.random.RandomState(516)
    A = np.abs(rs.standard_normal((65, MAGLD))).astype(f32)
    A[2:] *= (10.0 ** np.linspace(-7.0, 2.0, 63)).astype(f32)[:, None]
    A[1] = 0.0
    colsum = fb.astype(np.float64).sum(0)                                                # [100]
    owner = fb.argmax(1)                                                                 # the band that weighs bin k most
    g = rs.uniform(0.6, 1.6, NBIN)
    A[0, :NBIN] = np.where(colsum[owner] > 0, 1e-5 * g / np.maximum(colsum[owner], 1e-30), 0.0).astype(f32)
    A[0, NBIN:] = 0.0
    return A


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return _lib.lib()


@pytest.fixture(scope="module")
def dvae_sd():
    return W.synthetic_dvae()


@pytest.fixture(scope="module")
def nsd(dvae_sd):
    return {k: v.numpy() for k, v in dvae_sd.items()}


@pytest.fixture(scope="module")
def engs(lib, dvae_sd):
    return {bf: DvaeEngine(dvae_sd, DEV, bound_first=bf) for bf in MODES}


@pytest.fixture(scope="module")
def eng(engs):
    return engs[True]


@pytest.fixture(scope="module")
def hot(lib, dvae_sd):
    """engines on the one-hot `project_in`, and that state dict for the oracle"""
    sd = one_hot_sd(dvae_sd)
    return {bf: DvaeEngine(sd, DEV, bound_first=bf) for bf in MODES}, {k: v.numpy() for k, v in sd.items()}


@pytest.fixture(scope="module")
def chain_ref(nsd):
    return {k: chain_oracle(nsd, w) for k, w in chain_clips().items()}


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).contiguous().to(DEV)


def stft_gpu(lib, eng, wav: np.ndarray, F=None, extra_rows=1):
    """-> (rc, mag [F + extra_rows, 516] numpy); the buffer starts as NaN; window and twiddle are the engine's own"""
    n = int(wav.size)
    F = 1 + n // HOP if F is None else F
    wav_d = dev(wav)
    mag = torch.full((F + extra_rows, MAGLD), NAN, dtype=torch.float32, device=DEV)
    rc = lib.ctts_k_stft_mag(wav_d.data_ptr(), n, eng._w.mel_window, eng._w.twiddle, mag.data_ptr(), F, None)
    torch.cuda.synchronize()
    return rc, mag


def logmel_gpu(lib, eng, A_d: torch.Tensor, M: int, tiled=1, extra_rows=1):
    """the mel GEMM as ctts_dvae_encode launches it: A [M][516] x the engine's padded filterbank [100][516], epilogue 7 with coef"""
    out = torch.full((M + extra_rows, NMEL), NAN, dtype=torch.float32, device=DEV)
    rc = lib.ctts_k_gemm(tiled, A_d.data_ptr(), eng._w.mel_fb, out.data_ptr(), M, NMEL, MAGLD, MAGLD, NMEL, _lib.F32, 7, None, 0.0,
                         None, NMEL, None, eng._w.coef, 1, 0, 0, 0, 1, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def gfsq_encode_gpu(lib, eng, feat: np.ndarray, rows: int):
    """-> codes [rows + 4, 4] int32, pre-filled with -1.  `feat` carries four finite rows more than `rows`, like the codes buffer"""
    assert feat.shape[0] >= rows + 4
    feat_d = dev(feat)
    codes = torch.full((rows + 4, 4), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.ctts_k_gfsq_encode(eng.handle, feat_d.data_ptr(), codes.data_ptr(), rows, None), "ctts_k_gfsq_encode")
    torch.cuda.synchronize()
    return codes.cpu().numpy()


def pad4(feat: np.ndarray) -> np.ndarray:
    return np.concatenate([feat, np.ones((4, feat.shape[1]), f32)], 0)


# ---- (a) STFT magnitude ---------------------------------------------------------------------------------------------------------
STFT_NS = [513, 767, 768, 1023, 1024, 1025, 1279, 1280, 2305]     # 513: the shortest legal clip, F = 3, every frame reflects twice


@pytest.mark.parametrize("n", STFT_NS)
def test_stft_mag_alone(lib, eng, nsd, n):
    """Per frame || got[:513] - ref ||_2 <= 1e-5 || ref ||_2 against the float64 STFT.  Derived: a radix-2 float32 FFT of 10 stages
    has a relative L2 error of about 10 * 6.7 u (u = 2^-24) = 4e-6; sqrt(2) for keeping the one-sided half; the window product and
    the square root on top: below 1e-5 with less than 2x slack."""
    F = 1 + n // HOP
    worst = 0.0
    for name, wav in signals(n).items():
        ref = dvae_np.stft_mag(wav, nsd[WIN_KEY]).astype(np.float64)
        assert ref.shape == (F, NBIN)
        rc, mag = stft_gpu(lib, eng, wav)
        _lib.check(rc, "ctts_k_stft_mag")
        mag = mag.cpu().numpy()
        assert np.array_equal(mag[:F, NBIN:], np.zeros((F, MAGLD - NBIN), f32)), (n, name, "pad columns")
        assert np.isnan(mag[F:]).all(), (n, name, "a row beyond F was written")
        got = mag[:F, :NBIN].astype(np.float64)
        assert np.isfinite(got).all()
        if name == "zeros":
            assert not got.any(), (n, "silence must give exact zeros")
            continue
        err, nrm = np.linalg.norm(got - ref, axis=1), np.linalg.norm(ref, axis=1)
        assert (nrm > 0).all()
        ratio = float((err / nrm).max())
        worst = max(worst, ratio)
        print(f"stft_mag n={n} {name}: worst frame L2 ratio {ratio:.2e}")
        assert (err <= 1e-5 * nrm).all(), (n, name, ratio)
    print(f"stft_mag n={n}: worst L2 ratio {worst:.2e} (bound 1e-5)")


@pytest.mark.parametrize("n,F", [(512, 3), (1024, 4), (1024, 6)])
def test_stft_mag_refusals(lib, eng, n, F):
    """a clip no longer than the reflect padding, or a frame count that is not 1 + n / 256: refused, nothing launched"""
    wav = signals(n)["noise"]
    rc, mag = stft_gpu(lib, eng, wav, F=F)
    assert rc != 0 and b"launch_stft_mag" in lib.ctts_last_error()
    assert torch.isnan(mag).all().item()


# ---- (b) log-mel epilogue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 64, 65])
def test_logmel_epilogue_alone(lib, eng, nsd, M):
    """`EPI_LOG_DIV` of gemm_tiled_f32_k at the 64-row tile edges (N = 100 is a ragged second column tile).
    | got * coef - log(max(acc64, 1e-5)) | <= 4e-5.  Derived: every term is non-negative, so a 516-term float32 sum is off by at most
    516 * 2^-24 = 3.1e-5 relative; log(max(., c)) is continuous through the clamp and turns a relative error into that absolute one;
    the rest is a few ulps of the log at |log| <= 12.  The all-zero row -- what every band of a silent frame holds -- must equal
    log(float32(1e-5)) / coef to 2 ulps; the device's logf alone is about 1.4 ulp off at that argument, which the division stretched to
    2.4 ulps of the result, so the epilogue takes this log in double and rounds once."""
    fb, coef = nsd[FB_KEY], nsd["coef"].reshape(-1).astype(np.float64)
    fbt = np.zeros((NMEL, MAGLD), np.float64)
    fbt[:, :NBIN] = fb.T
    base = logmel_rows(fb)
    clamp_sums = base[0].astype(np.float64) @ fbt.T
    live = fb.sum(0) > 0
    assert ((clamp_sums[live] > 0.5e-5) & (clamp_sums[live] < 2e-5)).all() and live.sum() >= 90
    assert (clamp_sums[live] < 1e-5).sum() >= 10 and (clamp_sums[live] > 1e-5).sum() >= 10        # both sides of the clamp
    zero_ref = np.log(np.float64(f32(1e-5))) / coef
    worst = worst_ulp = 0.0
    for rot in range(3):                                  # each kind of row comes first once: M = 1 runs all three
        A = np.roll(base[: max(M, 3)], -rot, axis=0)[:M]
        rc, out = logmel_gpu(lib, eng, dev(A), M)
        _lib.check(rc, "ctts_k_gemm")
        assert np.isnan(out[M:]).all(), "a row beyond M was written"
        got = out[:M].astype(np.float64)
        assert np.isfinite(got).all()
        acc = A.astype(np.float64) @ fbt.T
        err = np.abs(got * coef - np.log(np.maximum(acc, 1e-5)))
        worst = max(worst, float(err.max()))
        assert err.max() <= 4e-5, (M, rot, float(err.max()))
        for r in np.nonzero(~A.any(1))[0]:
            ulps = np.abs(got[r] - zero_ref) / np.spacing(np.abs(zero_ref).astype(f32))
            worst_ulp = max(worst_ulp, float(ulps.max()))
            assert (ulps <= 2).all(), (M, rot, int(r), float(ulps.max()))
    print(f"log-mel epilogue M={M}: worst |log error| {worst:.2e} (bound 4e-5); silent row within {worst_ulp:.2f} ulp (bound 2)")


def test_logmel_epilogue_refused_on_split_bf16_tiles(lib, eng):
    """kernels.hpp: EPI_LOG_DIV is 'f32 tiles only'"""
    A = dev(np.ones((3, MAGLD), f32))
    rc, out = logmel_gpu(lib, eng, A, 3, tiled=2)
    assert rc != 0
    assert np.isnan(out).all()


# ---- (c) mel stage: STFT -> filterbank -> log / coef ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "sine", "const"])
def test_mel_stage_chained(lib, eng, nsd, kind):
    """GPU magnitude into the GPU epilogue against dvae_np.mel_features, in the LINEAR domain (a tone's or a constant's far bands
    sit at the clamp, where float32 FFT noise legitimately moves the log):
    | exp(got * coef) - max(mel, 1e-5) | <= 1e-5 ||fb[:, c]||_2 ||mag_frame||_2 + 4e-5 max(mel, 1e-5),
    the STFT's bound carried through the filterbank (Cauchy-Schwarz) plus the epilogue's."""
    n = 1280
    wav = signals(n)[kind]
    F = 1 + n // HOP
    rc, mag = stft_gpu(lib, eng, wav, extra_rows=0)
    _lib.check(rc, "ctts_k_stft_mag")
    rc, out = logmel_gpu(lib, eng, mag, F)
    _lib.check(rc, "ctts_k_gemm")
    assert np.isnan(out[F:]).all()
    coef = nsd["coef"].reshape(-1).astype(np.float64)
    got = np.exp(out[:F].astype(np.float64) * coef)
    ref = np.exp(dvae_np.mel_features(wav, nsd[WIN_KEY], nsd[FB_KEY]).astype(np.float64))       # == max(mel, 1e-5)
    assert ref.shape == got.shape == (F, NMEL)
    mag_n = np.linalg.norm(dvae_np.stft_mag(wav, nsd[WIN_KEY]).astype(np.float64), axis=1)       # [F]
    fb_n = np.linalg.norm(nsd[FB_KEY].astype(np.float64), axis=0)                                 # [100]
    bound = 1e-5 * mag_n[:, None] * fb_n[None, :] + 4e-5 * ref
    err = np.abs(got - ref)
    print(f"mel stage {kind}: worst error / bound {float((err / bound).max()):.3f}; {int((ref <= 1.0001e-5).sum())} of {ref.size} at the clamp")
    assert (err <= bound).all(), (kind, float((err / bound).max()))


# ---- (d) the stride-2 k4 conv as a k3 conv over frame pairs ---------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4, 5, 6, 33, 34, 129])
def test_paired_stride2_conv_on_the_kernel(lib, dvae_sd, nsd, F):
    """the launch of ctts_dvae_encode's second downsample conv: M = T rows over frames = Fe / 2 frame pairs -- one more frame than
    rows for an odd F, whose last pair ends in the appended frame.  That frame holds finite garbage here: it meets the repack's zero
    block and must not matter.  Bar: test_gemm_tiled_conv's for these tiles."""
    from tests import gpu_util as G
    Fe, T = (F + 1) & ~1, (F - 2) // 2 + 1
    rs = np.random.RandomState(F)
    x = np.full((Fe, 512), 1e3, f32)
    x[:F] = rs.standard_normal((F, 512)).astype(f32)
    w4, b = nsd["downsample_conv.2.weight"], nsd["downsample_conv.2.bias"]
    pair = pair_repack_k4s2(dvae_sd["downsample_conv.2.weight"])
    Wd, bd, xd = dev(pair.reshape(512, -1)), dev(b), dev(x)
    out = torch.full((T + 1, 512), NAN, dtype=torch.float32, device=DEV)
    rc = lib.ctts_k_gemm(1, xd.data_ptr(), Wd.data_ptr(), out.data_ptr(), T, 512, 3 * 1024, 1024, 512, _lib.F32, 4, None, 0.0, None, 512,
                         bd.data_ptr(), None, 3, 1024, Fe // 2, 1, 1, None)
    _lib.check(rc, "ctts_k_gemm")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[T]).all(), "the row beyond T was written"
    ref = codec_np.gelu(dvae_np.conv1d_k4s2_cl(x[None, :F], w4, b))[0]
    assert ref.shape == (T, 512) and np.isfinite(out[:T]).all()
    assert G.relerr(out[:T], ref) < 1e-5, G.relerr(out[:T], ref)


# ---- (e) gfsq_encode_k on exact inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound_first", MODES)
def test_gfsq_encode_every_reachable_code(lib, hot, bound_first):
    """625 rows, one per level tuple: the r = 0 codes ARE the row numbers (pins the index basis without the oracle), and all four
    columns equal the oracle's, whose rounding margins are wide here"""
    engs, hsd = hot
    feat = one_hot_feat(level_tuple_z(bound_first))
    marg = dvae_np.gfsq_round_margin(hsd, feat, bound_first=bound_first)
    assert marg.min() >= 0.1, float(marg.min())
    want = dvae_np.gfsq_encode(hsd, feat, bound_first=bound_first)
    codes = gfsq_encode_gpu(lib, engs[bound_first], pad4(feat), 625)
    assert (codes[625:] == -1).all()
    assert np.array_equal(codes[:625, 0], np.arange(625)) and np.array_equal(codes[:625, 2], np.arange(625))
    assert np.array_equal(codes[:625], want)


@pytest.mark.parametrize("bound_first", MODES)
def test_gfsq_encode_every_boundary(lib, hot, bound_first):
    """One coordinate swept over [-4, 4] in 20001 steps: a code equals the oracle's wherever the oracle's pre-rounding coordinate is at
    least 1e-4 from a boundary (with exact z the noise is tanhf's ulps times 4 at level 1, about 5e-6: 20x inside); elsewhere it may
    be one step of the swept coordinate off, and an r = 1 code may differ, in that coordinate only, where its r = 0 code did."""
    engs, hsd = hot
    feat = one_hot_feat(sweep_z())
    want = dvae_np.gfsq_encode(hsd, feat, bound_first=bound_first)
    marg = dvae_np.gfsq_round_margin(hsd, feat, bound_first=bound_first)
    for g in range(2):                                     # the sweep does cross every boundary: 4 at r = 0, 20 at r = 1
        sw = digits_of(want[:, 2 * g: 2 * g + 2])[..., g + 1]
        assert (np.diff(sw[:, 0]) != 0).sum() == 4 and (np.diff(sw[:, 1]) != 0).sum() == 20
    under = int((marg < 1e-4).sum())
    print(f"gfsq sweep bound_first={bound_first}: {under} of {marg.size} codes under the 1e-4 margin")
    assert marg.size == 4 * SWEEP_N and under <= 1e-3 * marg.size
    codes = gfsq_encode_gpu(lib, engs[bound_first], pad4(feat), SWEEP_N)
    assert (codes[SWEEP_N:] == -1).all()
    got = codes[:SWEEP_N]
    assert got.min() >= 0 and got.max() < 625
    gd, wd = digits_of(got), digits_of(want)               # [rows, 4 codes, 4 coordinates]
    n_diff = 0
    for t, c in zip(*np.nonzero(got != want)):
        d = c // 2 + 1                                     # the swept coordinate of this code's group
        others = [k for k in range(4) if k != d]
        assert np.array_equal(gd[t, c, others], wd[t, c, others]), (int(t), int(c), "a coordinate that was not swept moved")
        if c % 2 == 1 and got[t, c - 1] != want[t, c - 1]:
            n_diff += 1
            continue                                       # downstream of a flipped r = 0
        assert marg[t, c] < 1e-4 and abs(int(gd[t, c, d]) - int(wd[t, c, d])) == 1, (int(t), int(c), float(marg[t, c]))
        n_diff += 1
    print(f"gfsq sweep bound_first={bound_first}: {n_diff} codes differ from the oracle, all at a boundary")


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 4099])
def test_gfsq_encode_row_guard(lib, hot, rows):
    """four rows per workgroup: the last workgroup's spare waves must write nothing"""
    engs, hsd = hot
    feat = one_hot_feat(level_tuple_z(True))[(np.arange(rows) * 7 + 3) % 625]
    codes = gfsq_encode_gpu(lib, engs[True], pad4(feat), rows)
    assert (codes[rows:] == -1).all(), codes[rows:]
    assert np.array_equal(codes[:rows], dvae_np.gfsq_encode(hsd, feat))
    assert np.array_equal(codes[:rows, 0], (np.arange(rows) * 7 + 3) % 625)


# ---- (f) gfsq_encode_k with the real projection ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bound_first", MODES)
def test_gfsq_encode_real_weights(lib, engs, nsd, bound_first):
    """4099 rows of N(0,1) features through the synthetic `project_in`: the rule of test_gpu_dvae.py (1e-3 is the project's boundary
    for a 512-term float32 dot product in front of the rounding), with a cap on how many codes the rule may excuse"""
    feat = real_feat()
    want = dvae_np.gfsq_encode(nsd, feat, bound_first=bound_first)
    marg = dvae_np.gfsq_round_margin(nsd, feat, bound_first=bound_first)
    share = float((marg < 1e-3).mean())
    print(f"gfsq real weights bound_first={bound_first}: {100 * share:.2f} % of the oracle's codes within 1e-3 of a boundary")
    assert share <= 0.01
    codes = gfsq_encode_gpu(lib, engs[bound_first], pad4(feat), 4099)
    assert (codes[4099:] == -1).all()
    got = codes[:4099]
    assert got.min() >= 0 and got.max() < 625
    n_diff = check_codes_by_margin(got, want, marg, 1e-3, f"bound_first={bound_first}")
    distinct = [len(np.unique(got[:, c])) for c in range(4)]
    print(f"gfsq real weights bound_first={bound_first}: {n_diff} of {got.size} codes differ; distinct values per column {distinct}")
    assert min(distinct) >= 350


# ---- (g) gfsq_embed_k -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [625, 1])
def test_gfsq_embed_alone(lib, eng, nsd, rows):
    """Elementwise | got - ref | <= 8 * 2^-24 * (sum_d |zq_d w_d| + |b|): four products and four additions of at most one rounding
    each, on both sides."""
    i = np.arange(rows)
    codes = np.stack([i, (7 * i + 3) % 625, 624 - i, (11 * i) % 625], 1).astype(np.int64)
    ref = dvae_np.gfsq_embed(nsd, codes).astype(np.float64)
    codes_d = dev(codes, torch.int64)
    out = torch.full((rows + 1, 1024), NAN, dtype=torch.float32, device=DEV)
    _lib.check(lib.ctts_k_gfsq_embed(eng.handle, codes_d.data_ptr(), out.data_ptr(), rows, None), "ctts_k_gfsq_embed")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[rows]).all(), "the row beyond `rows` was written"
    got = out[:rows].astype(np.float64)
    assert np.isfinite(got).all()
    size = []
    for g in range(2):
        zq = sum(dvae_np.fsq_codes_from_index(codes[:, 2 * g + r], LEVELS).astype(np.float64) * 4.0 ** -r for r in range(2))   # [rows, 4]
        w = nsd[f"vq_layer.quantizer.rvqs.{g}.project_out.weight"].astype(np.float64)                                          # [512, 4]
        b = nsd[f"vq_layer.quantizer.rvqs.{g}.project_out.bias"].astype(np.float64)
        size.append(np.abs(zq) @ np.abs(w).T + np.abs(b))
    size = np.concatenate(size, -1)                                                                                            # [rows, 1024]
    ratio = float((np.abs(got - ref) / size).max() / U)
    print(f"gfsq_embed rows={rows}: worst |error| = {ratio:.2f} x 2^-24 x (sum |zq w| + |b|) (bound 8)")
    assert (np.abs(got - ref) <= 8 * U * size).all(), ratio


# ---- (h) the encode chain at its shortest lengths -------------------------------------------------------------------------------
def test_chain_margin_cap(chain_ref):
    """the clips of the chain test leave the margin rule little to excuse: at most 1 % of their 312 oracle codes lie within 1e-3 of
    a boundary, and silence none (its smallest margin is 2.3e-3)"""
    marg = np.concatenate([m.reshape(-1) for m in (chain_ref[n, k][1] for n in CHAIN_NS for k in CHAIN_KINDS)])
    assert marg.size == 312
    under = int((marg < 1e-3).sum())
    print(f"encode chain: {under} of {marg.size} oracle codes within 1e-3 of a boundary")
    assert under <= 0.01 * marg.size
    assert min(float(chain_ref[n, "silence"][1].min()) for n in CHAIN_NS) > 2e-3


@pytest.mark.parametrize("n", CHAIN_NS)
def test_encode_chain_short_clips(eng, chain_ref, n):
    """`sample_audio` against dvae_np.dvae_encode under the margin / downstream rule of test_gpu_dvae.py; silence exactly"""
    clips = chain_clips()
    T = (1 + n // HOP) // 2
    for kind in CHAIN_KINDS:
        want, marg = chain_ref[n, kind]
        codes = eng.sample_audio(clips[n, kind])
        assert codes.dtype == torch.int32 and tuple(codes.shape) == (4, T) and want.shape == (T, 4)
        got = codes.numpy().T
        assert got.min() >= 0 and got.max() < 625
        if kind == "silence":
            assert np.array_equal(got, want), (n, got, want)
        else:
            check_codes_by_margin(got, want, marg, 1e-3, (n, kind))


def test_encode_length_limit(eng):
    with pytest.raises(_lib.EngineError):
        eng.sample_audio(np.zeros(512, f32))
    assert tuple(eng.sample_audio(np.zeros(513, f32)).shape) == (4, 1)


# ---- (i) no read of uninitialised workspace -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [513, 768, 10257])              # 10257: the odd-F golden length
def test_encode_ignores_workspace_contents(lib, eng, n):
    wav = (0.3 * np.random.RandomState(n).standard_normal(n)).astype(f32)
    wav_d = dev(wav)
    T = int(lib.ctts_dvae_code_frames(n))
    nb = lib.ctts_dvae_encode_workspace_bytes(n)
    got = []
    for fill in (0xFF, 0x00):                                 # all NaN, all zero
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        codes = torch.full((T, 4), -1, dtype=torch.int32, device=DEV)
        _lib.check(lib.ctts_dvae_encode(eng.handle, wav_d.data_ptr(), n, codes.data_ptr(), ws.data_ptr(), nb, None), "ctts_dvae_encode")
        torch.cuda.synchronize()
        got.append(codes.cpu().numpy())
    assert got[0].min() >= 0 and got[0].max() < 625
    assert np.array_equal(got[0], got[1]), "the codes depend on what the workspace held"
    assert np.array_equal(got[0], eng.sample_audio(wav).numpy().T)


def test_decode_ignores_workspace_contents(lib, eng):
    B, T = 2, 3
    ids = dev(np.random.RandomState(5).randint(0, 625, size=(B, T, 4)), torch.int64)
    nb = lib.ctts_dvae_decode_workspace_bytes(B, T)
    got = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        mel = torch.full((B, 2 * T, NMEL), NAN, dtype=torch.float32, device=DEV)
        _lib.check(lib.ctts_dvae_decode_codes(eng.handle, ids.data_ptr(), mel.data_ptr(), B, T, ws.data_ptr(), nb, None),
                   "ctts_dvae_decode_codes")
        torch.cuda.synchronize()
        got.append(mel.cpu().numpy())
    assert np.isfinite(got[0]).all()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "the mel depends on what the workspace held"
    assert np.array_equal(got[0], eng.decode_codes(ids).cpu().numpy())

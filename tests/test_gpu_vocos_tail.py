"""The Vocos side of the acoustic decoder, kernel by kernel, from the backbone to the int16 bytes (csrc/codec.hip):

  * `CodecEngine.vocos_decode` against tests/golden/vocos_ref.npz, whose ConvNeXt blocks the reference's own class evaluated
    (oracle/make_vocos_goldens.py), in the three GEMM modes;
  * istft_frames_k / istft_ola_k / istft_ola_seg_k (ctts_k_istft, ctts_k_istft_ragged) against a float64 restatement: at the exp clip,
    with phases far beyond +-pi, below four overlapping frames, on one-hot spectra;
  * gather_windows_k (ctts_k_gather_windows), byte-exact against a numpy gather;
  * crop_pcm16_windows_k / chunks_pcm16_k (ctts_k_crop_pcm16_windows, ctts_k_chunks_pcm16), byte-exact against `audio.float_to_int16`
    of each chunk, with peaks ABOVE 1 placed where the 1024-thread reduction could lose them and chunks that start off a 16-byte boundary;
  * pcm16_scale for huge and non-finite peaks, on all five conversion paths.

Every output buffer is NaN- or canary-filled; what must not be written is asserted untouched."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, audio  # noqa: E402
from chattts_amd import engine as E  # noqa: E402

f32 = np.float32
DEV = torch.device("cuda:0")
NAN = float("nan")
CANARY16 = 0x5A5A
KEEP_FILL = 0xA5
HOP, NFFT, NBIN = 256, 1024, 513
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocos_ref.npz")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return _lib.lib()


def dev(x) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ceil8(n):
    return (int(n) + 7) // 8 * 8


# ---- the backbone against the reference-block fixture ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(lib, weights):
    return {g: E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=g) for g in ("bf16x3", "f16", "f32")}


@pytest.mark.parametrize("F", [2, 9, 66])
def test_vocos_decode_vs_reference_block_fixture(engines, F):
    """the bars of test_codec_vs_reference_golden (1e-4 RMS, north_star) and test_codec_f16_mode_holds_the_waveform_bar (f16 within 2e-5
    RMS of bf16x3, within 1e-4 of the reference) -- against a waveform whose blocks are the reference's, not our restatement's"""
    ref = np.load(GOLDEN)
    mel = torch.from_numpy(np.ascontiguousarray(ref[f"F{F}.mel"].transpose(0, 2, 1)))      # [2, F, 100] channels-last
    want = ref[f"F{F}.wav"].astype(np.float64)
    got = {g: e.vocos_decode(mel).cpu().numpy() for g, e in engines.items()}
    rms = {g: float(np.sqrt(np.mean((w - want) ** 2))) for g, w in got.items()}
    d16 = float(np.sqrt(np.mean((got["f16"].astype(np.float64) - got["bf16x3"]) ** 2)))
    print(f"vocos_decode vs reference-block fixture, F={F}: " + ", ".join(f"{g} rms {r:.2e}" for g, r in rms.items())
          + f"; f16 vs bf16x3 {d16:.2e} (signal rms {float(np.sqrt(np.mean(want ** 2))):.2e})")
    for g, w in got.items():
        assert w.shape == want.shape and np.isfinite(w).all()
        assert rms[g] < 1e-4, (g, rms[g])
    assert d16 < 2e-5, d16


# ---- ISTFT ---------------------------------------------------------------------------------------------------------------------------
LOG100 = f32(math.log(100.0))
# the clip's own edge, one float32 step each side of it, far above it, where expf overflows before the clip, and silence
SPECIAL_LOGMAGS = np.array([LOG100, np.nextafter(LOG100, f32(0)), np.nextafter(LOG100, f32(10)), 20.0, 89.0, -100.0], f32)


def hann_and_twiddle():
    window = torch.hann_window(NFFT).numpy()
    kk = np.arange(512, dtype=np.float64) * (2 * math.pi / NFFT)
    return window, np.stack([np.cos(kk), np.sin(kk)], 1).astype(f32)


def ola64(frames: np.ndarray, window: np.ndarray) -> np.ndarray:
    """float64 windowed frames [B, F, 1024] -> overlap-add, envelope division, centre trim: [B, 256 (F - 1)]"""
    B, F, _ = frames.shape
    total = NFFT + HOP * (F - 1)
    y, env, w2 = np.zeros((B, total)), np.zeros(total), window.astype(np.float64) ** 2
    for f in range(F):
        y[:, f * HOP: f * HOP + NFFT] += frames[:, f]
        env[f * HOP: f * HOP + NFFT] += w2
    return y[:, NFFT // 2: total - NFFT // 2] / env[NFFT // 2: total - NFFT // 2]


def istft64(head: np.ndarray, window: np.ndarray) -> np.ndarray:
    """the head's tail restated in float64: head [B, F, 1026] (log-magnitudes | phases) -> [B, 256 (F - 1)]"""
    h = head.astype(np.float64)
    spec = np.minimum(np.exp(h[..., :NBIN]), 100.0) * np.exp(1j * h[..., NBIN:])
    spec[..., 0] = spec[..., 0].real          # a real signal's DC and Nyquist bins are real: c2r drops what the phase puts there
    spec[..., NBIN - 1] = spec[..., NBIN - 1].real
    return ola64(np.fft.irfft(spec, n=NFFT, axis=-1) * window.astype(np.float64), window)


def edge_head(B: int, F: int, seed: int) -> np.ndarray:
    """ordinary log-magnitudes N(0.5, 0.7) with every SPECIAL_LOGMAGS value on four random bins of every frame, phases uniform in +-200;
    bins 0 and 512 carry magnitude e and such a phase too, so an imaginary part let through there shows"""
    rs = np.random.RandomState(seed)
    head = np.empty((B, F, 2 * NBIN), f32)
    head[..., :NBIN] = rs.standard_normal((B, F, NBIN)) * 0.7 + 0.5
    head[..., NBIN:] = rs.uniform(-200.0, 200.0, (B, F, NBIN))
    for b in range(B):
        for f in range(F):
            head[b, f, 1 + rs.choice(NBIN - 2, 4 * len(SPECIAL_LOGMAGS), replace=False)] = np.repeat(SPECIAL_LOGMAGS, 4)
    head[..., 0] = 1.0
    head[..., NBIN - 1] = 1.0
    return head


def run_istft(lib, head: np.ndarray, pad: int = 64):
    """ctts_k_istft on head [B, F, 1026] -> (wav [B, 256 (F - 1)], the NaN tail behind it)"""
    B, F, _ = head.shape
    window, tw = hann_and_twiddle()
    keep = [dev(head), dev(window), dev(tw)]
    frames = torch.full((B * F * NFFT,), NAN, dtype=torch.float32, device=DEV)
    wav = torch.full((B * HOP * (F - 1) + pad,), NAN, dtype=torch.float32, device=DEV)
    _lib.check(lib.ctts_k_istft(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), frames.data_ptr(), wav.data_ptr(), B, F, None),
               "ctts_k_istft")
    w = wav.cpu().numpy()
    return w[: B * HOP * (F - 1)].reshape(B, HOP * (F - 1)), w[B * HOP * (F - 1):]


def bar(ref: np.ndarray) -> float:
    return 5e-5 * max(1.0, float(np.abs(ref).max()))      # the project's own ISTFT bar (test_gpu_kernels.py test_istft)


@pytest.mark.parametrize("F", [2, 3, 4, 5, 9, 33])
def test_istft_at_the_clip_and_far_phases(lib, F):
    """below F = 5 no sample has all four overlaps; the log-magnitudes sit on the exp clip and its float32 neighbours, far above it,
    where expf overflows, and at silence; the phases reach +-200"""
    head = edge_head(2, F, seed=100 + F)
    window, _ = hann_and_twiddle()
    ref = istft64(head, window)
    got, tail = run_istft(lib, head)
    err = float(np.abs(got - ref).max())
    print(f"istft edge case B=2 F={F}: worst error {err:.3e} (max |ref| {np.abs(ref).max():.3f}, bar {bar(ref):.2e})")
    assert np.isnan(tail).all()
    assert np.isfinite(got).all()
    assert err < bar(ref), err


@pytest.mark.parametrize("k", [1, 2, 255, 511])
def test_istft_one_hot_bin_is_its_windowed_cosine(lib, k):
    """a single bin of magnitude 1 and phase 0.7, everything else at log-magnitude -100 (random phases): the frame is (2 / 1024)
    cos(2 pi k n / 1024 + 0.7) times the window -- the bit reversal and the twiddle's sign.  Row 0: the bin in every frame; row 1: in
    frame 1 only."""
    F = 4
    rs = np.random.RandomState(k)
    head = np.empty((2, F, 2 * NBIN), f32)
    head[..., :NBIN] = -100.0
    head[..., NBIN:] = rs.uniform(-200.0, 200.0, (2, F, NBIN))
    on = np.zeros((2, F), bool)
    on[0, :] = True
    on[1, 1] = True
    head[on, k] = 0.0
    head[on, NBIN + k] = 0.7
    window, _ = hann_and_twiddle()
    n = np.arange(NFFT, dtype=np.float64)
    frames = on[..., None] * ((2.0 / NFFT) * np.cos(2 * math.pi * k * n / NFFT + np.float64(f32(0.7))) * window.astype(np.float64))
    ref = ola64(frames, window)
    got, tail = run_istft(lib, head)
    err = float(np.abs(got - ref).max())
    print(f"istft one-hot bin {k}: worst error {err:.3e} (max |ref| {np.abs(ref).max():.3e}, bar {bar(ref):.2e})")
    assert np.isnan(tail).all()
    assert np.abs(ref).max() > 1e-3                       # 20 x the bar: another bin's cosine, or the mirrored one, cannot pass
    assert err < bar(ref), err


def test_istft_ragged_segments_equal_each_alone(lib):
    lens = [1, 1, 2, 1, 7]                                 # tokens; 2 frames each
    tok_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, n_seg = int(tok_off[-1]), len(lens)
    head = edge_head(1, 2 * T, seed=77)[0]                 # [24, 1026]
    window, tw = hann_and_twiddle()
    total = HOP * (2 * T - n_seg)
    keep = [dev(head), dev(window), dev(tw), dev(tok_off)]
    frames = torch.full((2 * T * NFFT,), NAN, dtype=torch.float32, device=DEV)
    wav = torch.full((total + 512,), NAN, dtype=torch.float32, device=DEV)
    _lib.check(lib.ctts_k_istft_ragged(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), frames.data_ptr(), wav.data_ptr(),
                                       keep[3].data_ptr(), n_seg, 2 * T, 2 * max(lens), None), "ctts_k_istft_ragged")
    w = wav.cpu().numpy()
    assert np.isnan(w[total:]).all()                       # nothing behind 256 (2 T - n_seg)
    for i, n_tok in enumerate(lens):
        seg = head[None, 2 * tok_off[i]: 2 * tok_off[i + 1]]
        lo = HOP * (2 * int(tok_off[i]) - i)
        got = w[lo: lo + HOP * (2 * n_tok - 1)]
        alone, _ = run_istft(lib, seg)
        assert np.array_equal(got.view(np.uint32), alone[0].view(np.uint32)), i      # the envelope counts the segment's own frames only
        ref = istft64(seg, window)[0]
        err = float(np.abs(got - ref).max())
        print(f"istft ragged segment {i} ({n_tok} tokens): worst error {err:.3e} (bar {bar(ref):.2e})")
        assert err < bar(ref), (i, err)


# ---- gather_windows_k ------------------------------------------------------------------------------------------------------------------
SLOTS, CAP, ROW = 5, 40, 772
SLOT_STRIDE = CAP * ROW + 8
CANARY32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def store():
    """[5][40][772] words of random BITS (a gather is a copy: any pattern must survive), slots SLOT_STRIDE apart"""
    rs = np.random.RandomState(5)
    return rs.randint(0, 2 ** 32, SLOTS * SLOT_STRIDE, dtype=np.uint64).astype(np.uint32)


def windows_table(rows) -> np.ndarray:
    """ctts_window[n]: slot, t_lo, t_hi, c_lo, c_hi, keep, 0, 0"""
    tab = np.zeros((len(rows), 8), np.int32)
    for i, r in enumerate(rows):
        tab[i, : len(r)] = r
    return tab


def run_gather(lib, store, tab, total_rows, extra=6):
    hid = dev(store.view(np.float32))
    packed = torch.full(((total_rows + extra) * 768,), CANARY32, dtype=torch.int32, device=DEV)
    tok_off = torch.full((len(tab) + 1 + 8,), CANARY32, dtype=torch.int32, device=DEV)
    win = dev(tab)
    _lib.check(lib.ctts_k_gather_windows(hid.data_ptr(), SLOT_STRIDE, ROW, win.data_ptr(), len(tab), total_rows, packed.data_ptr(),
                                         tok_off.data_ptr(), None), "ctts_k_gather_windows")
    return packed.cpu().numpy().view(np.uint32).reshape(-1, 768), tok_off.cpu().numpy()


def gather_ref(store, tab):
    rows = [store[s * SLOT_STRIDE + t * ROW: s * SLOT_STRIDE + t * ROW + 768] for s, lo, hi in tab[:, :3] for t in range(lo, hi)]
    return np.stack(rows), np.concatenate([[0], np.cumsum(tab[:, 2] - tab[:, 1])]).astype(np.int32)


GATHER_TABLES = {
    # out of slot order, the same slot twice (and a third time), t_lo > 0, 1-row windows, a window up to the slot's last row
    "mixed": [(3, 5, 12), (0, 0, 1), (3, 20, 40), (1, 39, 40), (4, 0, 3), (0, 10, 11), (2, 7, 9), (3, 0, 6)],
    # more windows than the 256 threads that write tok_off
    "ones300": [((7 * i) % SLOTS, (11 * i) % CAP, (11 * i) % CAP + 1) for i in range(300)],
}


@pytest.mark.parametrize("name", list(GATHER_TABLES))
def test_gather_windows_is_a_byte_exact_gather(lib, store, name):
    tab = windows_table(GATHER_TABLES[name])
    ref, tok = gather_ref(store, tab)
    got, tok_off = run_gather(lib, store, tab, len(ref))
    assert np.array_equal(tok_off[: len(tab) + 1], tok)
    assert (tok_off[len(tab) + 1:] == CANARY32).all()
    assert np.array_equal(got[: len(ref)], ref)
    assert (got[len(ref):] == CANARY32).all()


def test_gather_windows_leaves_rows_beyond_the_table(lib, store):
    """total_rows 3 above what the device table holds (the host mirror disagreed): those rows are neither read nor written"""
    tab = windows_table(GATHER_TABLES["mixed"])
    ref, tok = gather_ref(store, tab)
    got, tok_off = run_gather(lib, store, tab, len(ref) + 3)
    assert np.array_equal(tok_off[: len(tab) + 1], tok)
    assert np.array_equal(got[: len(ref)], ref)
    assert (got[len(ref):] == CANARY32).all()


# ---- crop_pcm16_windows_k / chunks_pcm16_k ---------------------------------------------------------------------------------------------
PEAKS = (np.nextafter(f32(1), f32(2)), f32(-2.5), f32(32767.0))      # ceil 2, 3, 32767
PEAK_SCALES = (16383, 10922, 1)
CHUNK_NS = (1, 7, 8, 9, 511, 8191, 8192, 8193, 12000, 16385)          # 8192 samples = one pass of 1024 threads x 8
KEEP_THR = 1e-5


def peak_positions(n: int):
    """first and last sample, the first sample of a partial last group of 8, the seam of waves 14 | 15 (7679 | 7680) and of the first
    and the second pass (8191 | 8192)"""
    pos = {0, n - 1} | {p for p in (7679, 7680, 8191, 8192) if p < n}
    if n % 8:
        pos.add(n - n % 8)
    return sorted(pos)


def chunk_table(seed: int = 2):
    """The windows both kernels are given: (tab [n, 8] ctts_window, wav: their packed decode's stand-in, start [n]: each crop's first
    sample in wav, peaks: {window: index into PEAKS}).  wav is N(0, 0.3) clipped to +-0.9 in the packed layout -- window i's 256 (2 T_i - 1)
    samples at 256 (2 tok_off[i] - i) -- so without its planted peak every chunk converts at scale 32767."""
    spec = [(n, p) for n in CHUNK_NS for p in peak_positions(n)]
    spec += [(9, None), (8193, None), (520, "zero"), (100, "denormal"), (777, "negzero")]
    rs = np.random.RandomState(seed)
    rows, peaks = [], {}
    for i, (n, what) in enumerate(spec):
        c_lo = i % 4 + 4 * ((i // 4) % 3)
        T = ((c_lo + n + HOP - 1) // HOP + 2) // 2
        assert HOP * (2 * T - 1) >= c_lo + n and 1 <= T <= 33
        rows.append((0, 0, T, c_lo, c_lo + n, 1 if i % 5 in (0, 2, 3) else 0))
    tab = windows_table(rows)
    tok = np.concatenate([[0], np.cumsum(tab[:, 2])]).astype(np.int64)
    start = HOP * (2 * tok[:-1] - np.arange(len(tab))) + tab[:, 3]
    wav = np.clip(rs.standard_normal(HOP * (2 * int(tok[-1]) - len(tab))) * 0.3, -0.9, 0.9).astype(f32)
    for i, (n, what) in enumerate(spec):
        x = wav[start[i]: start[i] + n]
        if isinstance(what, int):
            peaks[i] = i % len(PEAKS)
            x[what] = PEAKS[peaks[i]]
        elif what == "zero":
            x[:] = 0.0
            x[::3] = -0.0
        elif what == "denormal":
            x[:] = (rs.randint(1, 0x7FFFFF, n).astype(np.uint32) | (rs.randint(0, 2, n).astype(np.uint32) << 31)).view(f32)
        elif what == "negzero":
            x[::5] = -0.0
    return tab, wav, start, peaks


def chunk_reference(tab, wav, start, product: str, thr: float):
    """(out int16 [sum ceil8(n_i)], keep uint8 [sum ceil8(n_i) / 8] with KEEP_FILL where no window with .keep writes, out_off [n + 1])"""
    n = (tab[:, 4] - tab[:, 3]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum((n + 7) // 8 * 8)])
    out = np.zeros(int(oo[-1]), np.int16)
    keep = np.full(int(oo[-1]) // 8, KEEP_FILL, np.uint8)
    for i in range(len(tab)):
        x = wav[start[i]: start[i] + n[i]]
        out[oo[i]: oo[i] + n[i]] = audio.float_to_int16(x, product)
        if tab[i, 5]:
            bits = np.packbits(np.abs(x) > f32(thr))
            keep[oo[i] // 8: oo[i] // 8 + len(bits)] = bits
    return out, keep, oo


def test_chunk_table_makes_the_peak_decide():
    """the two conditions on the data, on the host: a planted peak changes more than half of its chunk's samples against scale 32767 --
    a reduction that misses it cannot pass -- and some sample tells the float64 product from the float32 one"""
    tab, wav, start, peaks = chunk_table()
    assert {int(c) % 4 for c in tab[:, 3]} == {0, 1, 2, 3} and set(peaks.values()) == {0, 1, 2} and set(tab[:, 5]) == {0, 1}
    assert {int(tab[i, 3]) % 4 for i in peaks if tab[i, 4] - tab[i, 3] > 8192} == {0, 1, 2, 3}
    f64, _, oo = chunk_reference(tab, wav, start, "f64", KEEP_THR)
    f32_, _, _ = chunk_reference(tab, wav, start, "f32", KEEP_THR)
    assert (f64 != f32_).any()
    for i, p in peaks.items():
        n = int(tab[i, 4] - tab[i, 3])
        x = wav[start[i]: start[i] + n]
        assert audio.pcm_scale(np.abs(x).max()) == PEAK_SCALES[p]
        full = (x.astype(np.float64) * 32767.0).astype(np.int64).astype(np.int16)        # what a missed peak would write
        assert 2 * int((f64[oo[i]: oo[i] + n] != full).sum()) > n, (i, n)


def call_crop(lib, wav_d, tab, out_f32, product, thr, total, with_keep=True):
    """-> (out as int16 / uint32 words incl. a canary tail of 16 elements, keep incl. a tail of 8 bytes)"""
    win = dev(tab)
    out = torch.full((total + 16,), CANARY32 if out_f32 else CANARY16, dtype=torch.int32 if out_f32 else torch.int16, device=DEV)
    keep = torch.full((total // 8 + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ctts_k_crop_pcm16_windows(wav_d.data_ptr(), win.data_ptr(), len(tab), out_f32, product, thr, out.data_ptr(),
                                             keep.data_ptr() if with_keep else None, None), "ctts_k_crop_pcm16_windows")
    return out.cpu().numpy(), keep.cpu().numpy()


def chunk_descriptors(tab, wav, start):
    """the same chunks through ctts_rs_window descriptors: even entries as `rate >= 0` chunks (copies in a second buffer, at the
    crop's own alignment mod 16 bytes, 7.0 in the gaps), odd ones as `rate < 0` crops of wav; one empty chunk in the middle"""
    n = (tab[:, 4] - tab[:, 3]).astype(np.int64)
    rs = np.zeros(len(tab) + 1, _lib.RS_WINDOW)
    keep = np.zeros((len(tab) + 1, 8), np.int32)
    chunks = np.full(int(n[::2].sum()) + 4 * len(tab) + 8, 7.0, f32)
    cur, j, EMPTY = 0, 0, 5
    for i in range(len(tab)):
        if j == EMPTY:
            rs[j] = (0, 0, 0, 0, 3, 3, 0, 0, 0)
            keep[j, 5] = 1
            j += 1
        if i % 2 == 0:
            at = cur + (int(tab[i, 3]) - cur) % 4
            chunks[at: at + n[i]] = wav[start[i]: start[i] + n[i]]
            rs[j] = (0, 0, 0, 0, 5, 5 + n[i], at, 0, 0)
            cur = at + int(n[i])
        else:
            rs[j] = (start[i], n[i], 0, 0, 0, 0, 0, -1, 0)
        keep[j, 5] = tab[i, 5]
        j += 1
    return rs, keep, chunks


@pytest.mark.parametrize("product,thr", [("f64", KEEP_THR), ("f32", 0.0)])
def test_window_pcm_kernels_are_byte_exact(lib, product, thr):
    """both kernels, every chunk length and peak position of chunk_table: the int16 bytes, the zero pad up to the next multiple of 8
    (so the next window's first element), the masks of the windows with .keep and the 0xA5 fill of the others, the canaries behind.
    keep_thr 0 (second case) also counts the denormal chunk's samples and drops -0.0."""
    tab, wav, start, _ = chunk_table()
    ref_out, ref_keep, oo = chunk_reference(tab, wav, start, product, thr)
    total, prod = int(oo[-1]), {"f64": 0, "f32": 1}[product]
    wav_d = dev(wav)
    out, keep = call_crop(lib, wav_d, tab, 0, prod, thr, total)
    for i in np.flatnonzero(out[:total] != ref_out)[:5]:
        w = int(np.searchsorted(oo, i, side="right") - 1)
        print(f"crop: element {i} (window {w}, n {tab[w, 4] - tab[w, 3]}, sample {i - oo[w]}): got {out[i]}, want {ref_out[i]}")
    assert np.array_equal(out[:total], ref_out)
    assert (out[total:].view(np.uint16) == CANARY16).all()
    assert np.array_equal(keep[: total // 8], ref_keep)
    assert (keep[total // 8:] == KEEP_FILL).all()
    # no mask buffer at all: the same samples
    out2, keep2 = call_crop(lib, wav_d, tab, 0, prod, thr, total, with_keep=False)
    assert np.array_equal(out2[:total], ref_out) and (keep2 == KEEP_FILL).all()

    rs, ckeep, chunks = chunk_descriptors(tab, wav, start)
    rs_d, ck_d, ch_d = dev(rs.view(np.uint8)), dev(ckeep), dev(chunks)
    cout = torch.full((total + 16,), CANARY16, dtype=torch.int16, device=DEV)
    ckp = torch.full((total // 8 + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ctts_k_chunks_pcm16(wav_d.data_ptr(), ch_d.data_ptr(), ck_d.data_ptr(), rs_d.data_ptr(), len(rs), 0, prod, thr,
                                       cout.data_ptr(), ckp.data_ptr(), None), "ctts_k_chunks_pcm16")
    cout, ckp = cout.cpu().numpy(), ckp.cpu().numpy()
    assert np.array_equal(cout[:total], ref_out)
    assert (cout[total:].view(np.uint16) == CANARY16).all()
    assert np.array_equal(ckp[: total // 8], ref_keep)
    assert (ckp[total // 8:] == KEEP_FILL).all()


def test_window_pcm_kernels_float32_output_is_the_crop(lib):
    """out_f32: the chunk's floats bit for bit (-0.0 and denormals included), zeros up to the next multiple of 8, the same masks"""
    tab, wav, start, _ = chunk_table()
    _, ref_keep, oo = chunk_reference(tab, wav, start, "f64", KEEP_THR)
    total = int(oo[-1])
    ref = np.zeros(total, np.uint32)
    for i in range(len(tab)):
        n = int(tab[i, 4] - tab[i, 3])
        ref[oo[i]: oo[i] + n] = wav[start[i]: start[i] + n].view(np.uint32)
    wav_d = dev(wav)
    out, keep = call_crop(lib, wav_d, tab, 1, 0, KEEP_THR, total)
    out = out.view(np.uint32)
    assert np.array_equal(out[:total], ref) and (out[total:] == CANARY32).all()
    assert np.array_equal(keep[: total // 8], ref_keep) and (keep[total // 8:] == KEEP_FILL).all()
    rs, ckeep, chunks = chunk_descriptors(tab, wav, start)
    rs_d, ck_d, ch_d = dev(rs.view(np.uint8)), dev(ckeep), dev(chunks)
    cout = torch.full((total + 16,), CANARY32, dtype=torch.int32, device=DEV)
    ckp = torch.full((total // 8 + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ctts_k_chunks_pcm16(wav_d.data_ptr(), ch_d.data_ptr(), ck_d.data_ptr(), rs_d.data_ptr(), len(rs), 1, 0, KEEP_THR,
                                       cout.data_ptr(), ckp.data_ptr(), None), "ctts_k_chunks_pcm16")
    cout, ckp = cout.cpu().numpy().view(np.uint32), ckp.cpu().numpy()
    assert np.array_equal(cout[:total], ref) and (cout[total:] == CANARY32).all()
    assert np.array_equal(ckp[: total // 8], ref_keep) and (ckp[total // 8:] == KEEP_FILL).all()


# ---- pcm16_scale for peaks whose ceiling exceeds 32767, on every conversion path -------------------------------------------------------
# finite: the quotient 32767 // ceil(peak) is 0 (audio.pcm_scale); from 2^48 the old c * 32768 wrapped (a zero divisor at 2^49), from 2^63
# the cast itself was undefined; non-finite: the reference yields garbage, this project zeros
BAD_PEAKS = np.array([32767.5, 2.0 ** 49, 1e19, 3e38, np.inf, np.nan], f32)
BAD_LENS = (777, 1003, 8, 2049, 1, 513, 1000, 4097, 64, 999, 2050, 15, 1001)     # segment 2 j + 1 carries BAD_PEAKS[j]


def bad_rows(lens, seed):
    """rows of N(0, 0.3) clipped to +-0.9; row 2 j + 1 has BAD_PEAKS[j] on one sample (first, last or inside, by turns)"""
    rs = np.random.RandomState(seed)
    rows = [np.clip(rs.standard_normal(n) * 0.3, -0.9, 0.9).astype(f32) for n in lens]
    bad = {}
    for j, v in enumerate(BAD_PEAKS):
        r = rows[2 * j + 1]
        r[(0, len(r) - 1, len(r) // 2)[j % 3]] = v
        bad[2 * j + 1] = float(v)
    return rows, bad


def mask_of(x, thr=KEEP_THR):
    with np.errstate(invalid="ignore"):
        return np.abs(x) > f32(thr)


def expect_pcm(x, is_bad, product="f64"):
    return np.zeros(len(x), np.int16) if is_bad else audio.float_to_int16(x, product)


def test_host_scale_is_zero_for_every_finite_bad_peak():
    assert [audio.pcm_scale(float(v)) for v in BAD_PEAKS[:4]] == [0, 0, 0, 0] and audio.pcm_scale(32767.0) == 1


def test_bad_peaks_float_to_int16_rows(lib):
    """ctts_float_to_int16: per_row -- a bad row is zeros, its mask is right, its neighbours are untouched; one peak over the block --
    the whole block is zeros"""
    n, ld = 1003, 1010
    rows, bad = bad_rows([n] * 13, seed=41)
    x = np.full((13, ld), 5.0, f32)                       # the stride's slack holds a value that would change every scale
    x[:, :n] = np.stack(rows)
    x_d = dev(x)
    nb = (n + 7) // 8
    pcm = torch.full((13 * n + 16,), CANARY16, dtype=torch.int16, device=DEV)
    keep = torch.full((13 * nb + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    peak = torch.zeros((13,), dtype=torch.int32, device=DEV)
    _lib.check(lib.ctts_float_to_int16(x_d.data_ptr(), pcm.data_ptr(), keep.data_ptr(), 13, n, ld, 1, 0, KEEP_THR, peak.data_ptr(), None),
               "ctts_float_to_int16")
    p, k = pcm.cpu().numpy(), keep.cpu().numpy()
    assert (p[13 * n:].view(np.uint16) == CANARY16).all() and (k[13 * nb:] == KEEP_FILL).all()
    for r in range(13):
        assert np.array_equal(p[r * n: (r + 1) * n], expect_pcm(rows[r], r in bad)), (r, bad.get(r))
        assert np.array_equal(k[r * nb: (r + 1) * nb], np.packbits(mask_of(rows[r]))), (r, bad.get(r))
    for j in range(len(BAD_PEAKS)):                       # one peak over a [2, n] block
        blk = np.ascontiguousarray(np.stack([rows[2 * j], rows[2 * j + 1]]))
        b_d = dev(blk)
        pcm.fill_(CANARY16)
        keep.fill_(KEEP_FILL)
        _lib.check(lib.ctts_float_to_int16(b_d.data_ptr(), pcm.data_ptr(), keep.data_ptr(), 2, n, n, 0, 1, KEEP_THR, peak.data_ptr(), None),
                   "ctts_float_to_int16")
        p, k = pcm.cpu().numpy(), keep.cpu().numpy()
        assert (p[: 2 * n] == 0).all() and (p[2 * n:].view(np.uint16) == CANARY16).all(), float(BAD_PEAKS[j])
        assert np.array_equal(k[: 2 * nb], np.concatenate([np.packbits(mask_of(r)) for r in blk])) and (k[2 * nb:] == KEEP_FILL).all()


def test_bad_peaks_float_to_int16_ragged_and_groups(lib, engines):
    eng = engines["bf16x3"]
    rows, bad = bad_rows(BAD_LENS, seed=42)
    off = np.concatenate([[0], np.cumsum(BAD_LENS)]).astype(np.int64)
    wav_d = dev(np.concatenate(rows))
    koff = E.keep_offsets(off)
    pcm = torch.full((int(off[-1]) + 16,), CANARY16, dtype=torch.int16, device=DEV)
    keep = torch.full((int(koff[-1]) + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    eng.float_to_int16_ragged(wav_d, off, product="f64", keep_thr=KEEP_THR, out=(pcm[: int(off[-1])], keep[: int(koff[-1])]))
    p, k = pcm.cpu().numpy(), keep.cpu().numpy()
    assert (p[off[-1]:].view(np.uint16) == CANARY16).all() and (k[koff[-1]:] == KEEP_FILL).all()
    for r in range(len(rows)):
        assert np.array_equal(p[off[r]: off[r + 1]], expect_pcm(rows[r], r in bad)), (r, bad.get(r))
        assert np.array_equal(k[koff[r]: koff[r + 1]], np.packbits(mask_of(rows[r]))), (r, bad.get(r))
    # groups: every segment its own group, but the last two (the NaN one and a normal one) share one; kept samples only, one peak per group
    grp = np.array(list(range(12)) + [13], np.int32)
    blob, starts = eng.float_to_int16_groups(wav_d, off, grp, product="f64", keep_thr=KEEP_THR)
    host = blob.cpu().numpy()
    n_grp = len(grp) - 1
    counts = host[: 8 * n_grp].view(np.int64)
    samples = host[(8 * n_grp + 15) // 16 * 16:].view(np.int16)
    for g in range(n_grp):
        x = np.concatenate(rows[grp[g]: grp[g + 1]])
        kept = x[mask_of(x)]
        assert counts[g] == len(kept), (g, bad.get(g))
        assert np.array_equal(samples[starts[g]: starts[g] + len(kept)], expect_pcm(kept, g in bad)), (g, bad.get(g))


def test_bad_peaks_window_kernels(lib):
    """the crop and the chunks kernel: a window whose crop holds a bad sample comes back as zeros under the right mask, the windows
    around it exact"""
    rows, bad = bad_rows(BAD_LENS, seed=43)
    tabrows = []
    for i, n in enumerate(BAD_LENS):
        c_lo = i % 4
        tabrows.append((0, 0, ((c_lo + n + HOP - 1) // HOP + 2) // 2, c_lo, c_lo + n, 1))
    tab = windows_table(tabrows)
    tok = np.concatenate([[0], np.cumsum(tab[:, 2])]).astype(np.int64)
    start = HOP * (2 * tok[:-1] - np.arange(len(tab))) + tab[:, 3]
    wav = np.clip(np.random.RandomState(44).standard_normal(HOP * (2 * int(tok[-1]) - len(tab))) * 0.3, -0.9, 0.9).astype(f32)
    for i, r in enumerate(rows):
        wav[start[i]: start[i] + len(r)] = r
    n = np.array(BAD_LENS, np.int64)
    oo = np.concatenate([[0], np.cumsum((n + 7) // 8 * 8)])
    total = int(oo[-1])
    ref_out, ref_keep = np.zeros(total, np.int16), np.zeros(total // 8, np.uint8)
    for i, r in enumerate(rows):
        ref_out[oo[i]: oo[i] + n[i]] = expect_pcm(r, i in bad)
        bits = np.packbits(mask_of(r))
        ref_keep[oo[i] // 8: oo[i] // 8 + len(bits)] = bits
    wav_d = dev(wav)
    out, keep = call_crop(lib, wav_d, tab, 0, 0, KEEP_THR, total)
    assert np.array_equal(out[:total], ref_out) and (out[total:].view(np.uint16) == CANARY16).all()
    assert np.array_equal(keep[: total // 8], ref_keep) and (keep[total // 8:] == KEEP_FILL).all()
    rs, ckeep, chunks = chunk_descriptors(tab, wav, start)
    rs_d, ck_d, ch_d = dev(rs.view(np.uint8)), dev(ckeep), dev(chunks)
    cout = torch.full((total + 16,), CANARY16, dtype=torch.int16, device=DEV)
    ckp = torch.full((total // 8 + 8,), KEEP_FILL, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ctts_k_chunks_pcm16(wav_d.data_ptr(), ch_d.data_ptr(), ck_d.data_ptr(), rs_d.data_ptr(), len(rs), 0, 0, KEEP_THR,
                                       cout.data_ptr(), ckp.data_ptr(), None), "ctts_k_chunks_pcm16")
    cout, ckp = cout.cpu().numpy(), ckp.cpu().numpy()
    assert np.array_equal(cout[:total], ref_out) and (cout[total:].view(np.uint16) == CANARY16).all()
    assert np.array_equal(ckp[: total // 8], ref_keep) and (ckp[total // 8:] == KEEP_FILL).all()

"""Ragged acoustic decode where its masks matter most: packs of 1-, 2-, 3-, 4- and 7-token segments between long ones, a run of 80
1-token segments and boundaries on the tile and run edges (tests/gpu_util.ragged_edge_layout), at packed totals on both sides of
every size switch of the codec kernels -- the x3p / h1p planes from 1,024 frames (CTTS_X3P_MIN_ROWS), the 256 x 256 split-bf16 tile
and the sliding-window dwconv kernels from 12,288 (CTTS_X3_TILE, CTTS_DWCONV_RUN_MIN_ROWS) -- and a C3-like pass of 40,000 frames.
Each segment of the ragged call against its alone decode (bit for bit where DESIGN.md 8 says so), under every kernel variant, against
the float64 NumPy oracle, and through Chat.decode_to_pcm16.  `pytest -m gpu`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from oracle import codec_np  # noqa: E402
from tests.gpu_util import EDGE_LONG, EDGE_ONES, ragged_edge_rows  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTALS = (1022, 1024, 1026, 12286, 12288, 12290, 40000)
BIG = 40000
EXACT = ["f32", "bf16x3"]


@functools.lru_cache(maxsize=None)
def _pack(total):
    lens, rows = ragged_edge_rows(total)
    return lens, [torch.from_numpy(r).to(DEV) for r in rows]


@pytest.fixture(scope="module")
def codecs(weights):
    """one engine per mode, built with the default thresholds (a CTTS_X3P_MIN_ROWS of the caller's environment would change them)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("CTTS_X3P_MIN_ROWS", raising=False)
        return {g: E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=g) for g in ("f32", "bf16x3", "f16")}


_RAGGED = {}


def _ragged(codec, total):
    """the default-variant ragged decode of a pack, once per (engine, total): (wav, off, mel)"""
    key = (id(codec), total)
    if key not in _RAGGED:
        _RAGGED[key] = codec.decode_ragged(_pack(total)[1], return_mel=True)
    return _RAGGED[key]


def _alone(codec, row):
    mel = codec.dvae_decode(row[None])
    return mel[0], codec.vocos_decode(mel)[0]


def _rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _first_diff(a, b):
    """index of the first element (along dim 0) where two equal-shaped tensors differ, or None"""
    ne = (a != b) if a.dim() == 1 else (a != b).any(dim=1)
    idx = torch.nonzero(ne)
    return None if idx.numel() == 0 else int(idx[0, 0])


def _against_alone(codec, total):
    """per segment of the pack: index, tokens, (mel, wav) pairs of the ragged call and of the alone decode on the same engine"""
    lens, rows = _pack(total)
    wav, off, mel = _ragged(codec, total)
    f0 = 0
    for i, r in enumerate(rows):
        m1, w1 = _alone(codec, r)
        yield i, lens[i], (mel[f0: f0 + 2 * lens[i]], m1), (wav[off[i]: off[i + 1]], w1)
        f0 += 2 * lens[i]


def _assert_bit_identical(pairs, what):
    """every segment's mel and waveform equal bit for bit; else the first differing segment, its length and the first differing
    frame (the waveform's first differing sample, in frames of 256 samples)"""
    n = 0
    for i, t, (m, m1), (w, w1) in pairs:
        if not torch.equal(m, m1):
            fr = _first_diff(m, m1)
            pytest.fail(f"{what}: segment {i} ({t} tokens): mel differs first at frame {fr} of {2 * t} "
                        f"(max |diff| {float((m - m1).abs().max()):.3e})")
        if not torch.equal(w, w1):
            s = _first_diff(w, w1)
            pytest.fail(f"{what}: segment {i} ({t} tokens): wav differs first at sample {s} (frame ~{s // 256}) of {w.numel()} "
                        f"(rms {_rms(w.cpu().numpy(), w1.cpu().numpy()):.3e})")
        n += 1
    return n


@pytest.mark.parametrize("total", TOTALS)
@pytest.mark.parametrize("gemm", EXACT)
def test_ragged_edges_bit_identical_to_alone(codecs, gemm, total):
    """f32 and bf16x3, at 1,022 / 1,024 / 1,026, 12,286 / 12,288 / 12,290 and 40,000 packed frames: every segment -- 1-token runs,
    shorts between longs, first and last -- equals its alone dvae_decode / vocos_decode bit for bit, mel and waveform"""
    n = _assert_bit_identical(_against_alone(codecs[gemm], total), f"{gemm} at {total} frames")
    assert n == len(_pack(total)[0])


@pytest.fixture(scope="module")
def f16_planes(weights):
    """gemm "f16" with CTTS_X3P_MIN_ROWS=1 (read at ctts_codec_create): every decode, however short, runs its ConvNeXt point-wise
    pairs on the fp16 planes, so an alone segment takes the same kernels as the pack around it"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CTTS_X3P_MIN_ROWS", "1")
        return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f16")


@pytest.mark.parametrize("total", TOTALS)
def test_ragged_edges_f16_on_planes_bit_identical_to_alone(f16_planes, total):
    """f16, both the ragged and the alone decodes on the fp16 planes (CTTS_X3P_MIN_ROWS=1): bit for bit per segment"""
    _assert_bit_identical(_against_alone(f16_planes, total), f"f16 (planes everywhere) at {total} frames")


@pytest.mark.parametrize("total", TOTALS)
def test_ragged_edges_f16_default_threshold_within_bar(codecs, total):
    """f16 at the default threshold: from 1,024 packed frames a short segment's point-wise pairs take the fp16 planes where alone
    they take split-bf16 tiles; per segment within the mode's 2e-5 RMS bar (waveform), and bit for bit below 1,024 frames"""
    worst = 0.0
    for i, t, (m, m1), (w, w1) in _against_alone(codecs["f16"], total):
        rms = _rms(w.cpu().numpy(), w1.cpu().numpy())
        worst = max(worst, rms)
        assert rms < 2e-5, (i, t, rms)
        if total < 1024:
            assert torch.equal(m, m1) and torch.equal(w, w1), (i, t)
    print(f"f16 ragged vs alone at {total} frames: worst segment wav rms diff {worst:.2e}")


_VARIANTS = [("CTTS_CODEC_TILE", "128"), ("CTTS_CODEC_TILE", "256"), ("CTTS_DWCONV_SEQ", "0"), ("CTTS_DWCONV_SEQ", "1"),
             ("CTTS_DWCONV_SEQ", "2")]


@pytest.mark.parametrize("gemm", EXACT)
def test_ragged_edges_kernel_variants_read_per_launch(codecs, gemm, monkeypatch):
    """the 40,000-frame edge pack under each variant read at every launch -- the 128 and 256 codec tiles, the dwconv plane writers
    0 (run kernel), 1 (seq kernel at dilation 1) and 2 (also at dilation 2) -- equals the default decode bit for bit"""
    wav, _, mel = _ragged(codecs[gemm], BIG)
    rows = _pack(BIG)[1]
    for k, v in _VARIANTS:
        monkeypatch.setenv(k, v)
        w2, _, m2 = codecs[gemm].decode_ragged(rows, return_mel=True)
        monkeypatch.delenv(k)
        assert torch.equal(m2, mel), (gemm, k, v, "mel", _first_diff(m2, mel))
        assert torch.equal(w2, wav), (gemm, k, v, "wav", _first_diff(w2, wav))


_VARIANT_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from chattts_amd import engine as E, weights as W
from tests.gpu_util import ragged_edge_rows
dec, voc = W.synthetic_decoder(), W.synthetic_vocos()
rows = [torch.from_numpy(r).cuda() for r in ragged_edge_rows(int(sys.argv[3]))[1]]
out = {}
for g in ("f32", "bf16x3"):
    wav, off, mel = E.CodecEngine(dec, voc, torch.device("cuda:0"), gemm=g).decode_ragged(rows, return_mel=True)
    out[g + ".wav"], out[g + ".mel"] = wav.cpu().numpy(), mel.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("env", [("CTTS_DWCONV_RUN_MIN_ROWS", "0"), ("CTTS_X3_TILE", "128")])
def test_ragged_edges_kernel_variants_read_once(codecs, env, tmp_path):
    """the variants read once per process, each in a fresh child: the per-frame dwconv kernel everywhere
    (CTTS_DWCONV_RUN_MIN_ROWS=0) and the 128 x 128 split-bf16 tile in place of the 256 x 256 one (CTTS_X3_TILE=128) -- the
    40,000-frame edge pack in f32 and bf16x3 equals the default decode bit for bit"""
    res = tmp_path / "out.npz"
    penv = {k: v for k, v in os.environ.items() if k not in ("CTTS_DWCONV_RUN_MIN_ROWS", "CTTS_X3_TILE", "CTTS_X3P_MIN_ROWS",
                                                               "CTTS_CODEC_TILE", "CTTS_DWCONV_SEQ")}
    penv[env[0]] = env[1]
    p = subprocess.run([sys.executable, "-c", _VARIANT_CHILD, ROOT, str(res), str(BIG)], env=penv, timeout=600, capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(res)
    for g in EXACT:
        wav, _, mel = _ragged(codecs[g], BIG)
        mel_h, wav_h = mel.cpu().numpy(), wav.cpu().numpy()
        for name, got, want in (("mel", z[g + ".mel"], mel_h), ("wav", z[g + ".wav"], wav_h)):
            if not np.array_equal(got, want):
                d = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
                pytest.fail(f"{env[0]}={env[1]}, {g}: the {name} differs from the default first at index {int(d[0])}")


def _oracle_picks(lens):
    """6-8 short segments of the pack: the first and the last (1 token), one inside the 1-token run, and the first 1, 2, 3, 4 and
    7-token segment with a long segment on both sides"""
    mid = 2 + EDGE_ONES // 2                   # the layout's 1-token run is segments 2 .. EDGE_ONES + 1
    assert lens[mid - 1] == lens[mid] == lens[mid + 1] == 1
    picks = [0, mid, len(lens) - 1]
    for s in (1, 2, 3, 4, 7):
        picks.append(next(i for i in range(1, len(lens) - 1) if lens[i] == s and min(lens[i - 1], lens[i + 1]) >= EDGE_LONG))
    return sorted(set(picks))


@pytest.mark.parametrize("gemm", ["f32", "bf16x3", "f16"])
def test_ragged_edges_short_segments_against_the_numpy_oracle(codecs, weights, gemm):
    """short segments of the 40,000-frame pack against oracle/codec_np on each segment ALONE (float32 restatement, float64 LayerNorm,
    GELU and ISTFT): the waveform within the golden comparisons' bar (1e-4 RMS; f16 2e-5), the mel within 1e-4 of max(1, peak)
    (f16 2e-3) against codec_np.dvae_decode"""
    lens, rows = _pack(BIG)
    wav, off, mel = _ragged(codecs[gemm], BIG)
    mel_bar, wav_bar = (2e-3, 2e-5) if gemm == "f16" else (1e-4, 1e-4)
    f = np.concatenate([[0], 2 * np.cumsum(lens)])
    picks = _oracle_picks(lens)
    assert 6 <= len(picks) <= 8
    dec = {k: v.numpy() for k, v in weights["decoder"].items()}
    voc = {k: v.numpy() for k, v in weights["vocos"].items()}
    for i in picks:
        seg = rows[i].cpu().numpy()
        ref_mel = codec_np.dvae_decode(dec, seg[None])[0]
        ref_wav = codec_np.decode_to_wavs(dec, voc, [seg])[0]
        m = mel[f[i]: f[i + 1]].cpu().numpy()
        merr = float(np.abs(m - ref_mel).max()) / max(1.0, float(np.abs(ref_mel).max()))
        rms = _rms(wav[off[i]: off[i + 1]].cpu().numpy(), ref_wav)
        print(f"ragged[{gemm}] segment {i} ({lens[i]} tokens) vs oracle: mel err {merr:.2e}, wav rms err {rms:.2e}")
        assert merr < mel_bar and rms < wav_bar, (i, lens[i], merr, rms)


def test_ragged_edges_decode_to_pcm16_equals_alone_strip_and_convert(weights):
    """Chat.decode_to_pcm16(rows, ragged=True), codec "f32", the 40,000-frame edge pack (above the 12,288-frame switch, 1-token rows):
    per row the alone decode, the 1e-5 silence strip and float_to_int16, bit for bit"""
    from chattts_amd.core import Chat
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32", codec_gemm="f32")
    lens, rows = _pack(BIG)
    got = chat.decode_to_pcm16(rows, ragged=True)
    assert isinstance(got, list) and len(got) == len(rows)
    for i, (r, p) in enumerate(zip(rows, got)):
        alone = chat.decode_to_wavs([r])[0]
        assert p.dtype == np.int16 and np.array_equal(p, float_to_int16(alone[np.abs(alone) > np.float32(1e-5)])), (i, lens[i])

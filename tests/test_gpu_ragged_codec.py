"""Ragged acoustic decode on the GPU: packed utterances through DVAE + Vocos in one pass, each decoded as if alone
(CodecEngine.decode_ragged, ctts_dvae_decode_ragged / ctts_vocos_decode_ragged / ctts_float_to_int16_ragged), against the reference's
own B = 1 decodes, against the padded path's alone decodes, and behind the batched speech endpoint.  `pytest -m gpu`."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from oracle import cases  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMMS = ["f32", "bf16x3", "f16"]


@pytest.fixture(scope="module", params=GEMMS)
def codec(weights, request):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=request.param)


def _alone(codec, row):
    mel = codec.dvae_decode(row[None])
    return mel[0], codec.vocos_decode(mel)[0]


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_ragged_decode_matches_the_reference_per_segment(codec, golden):
    """the reference's own B = 1 decodes (codec.npz c1x5, s1x1, s1x2, s1x7; codec_big.npz c2size, 512 tokens) packed into ONE ragged
    call: every segment's mel and waveform against its golden at the existing bars (f32 / bf16x3: mel within 1e-4 of peak, wav 1e-4
    RMS; f16: 2e-3 / 2e-5)"""
    small = ["c1x5", "s1x1", "s1x2", "s1x7"]
    rows = [torch.from_numpy(cases.codec_inputs(cases.CODEC_CASES[n])[0]) for n in small]
    hid_big, _ = cases.codec_big_inputs(cases.CODEC_BIG_CASES["c2size"], golden["generate_big"]["c2.hid0"])
    rows.append(torch.from_numpy(hid_big[0]))
    wav, off, mel = codec.decode_ragged(rows, return_mel=True)
    lens = [int(r.shape[0]) for r in rows]
    assert np.array_equal(off, 256 * (2 * np.concatenate([[0], np.cumsum(lens)]) - np.arange(len(rows) + 1)))
    assert wav.numel() == sum(256 * (2 * t - 1) for t in lens) and tuple(mel.shape) == (2 * sum(lens), 100)
    wav_h, mel_h = wav.cpu().numpy(), mel.cpu().numpy()
    mel_bar, wav_bar = (2e-3, 2e-5) if codec.gemm == "f16" else (1e-4, 1e-4)
    f0 = 0
    for i, name in enumerate(small):
        m = mel_h[f0: f0 + 2 * lens[i]]
        f0 += 2 * lens[i]
        ref_mel = golden["codec"][name + ".mel"][0].T
        merr = np.abs(m - ref_mel).max() / max(1.0, np.abs(ref_mel).max())
        rms = _rms(wav_h[off[i]: off[i + 1]], golden["codec"][name + ".wav"][0])
        print(f"ragged[{codec.gemm}] {name}: mel err {merr:.2e}, wav rms err {rms:.2e}")
        assert merr < mel_bar and rms < wav_bar, (name, merr, rms)
    Gd = golden["codec_big"]
    got = cases.codec_big_subsample(mel_h[f0:].T[None], wav_h[off[-2]: off[-1]][None])
    peak = float(Gd["c2size.mel_peak"][0])
    merr = float(np.abs(got["mel_s"] - Gd["c2size.mel_s"]).max()) / peak
    rms = _rms(got["wav_s"], Gd["c2size.wav_s"])
    wblk = float(np.abs(got["wav_blk"] - Gd["c2size.wav_blk"]).max()) / 2048
    print(f"ragged[{codec.gemm}] c2size: mel err / peak {merr:.2e}, wav rms err {rms:.2e}, block mean {wblk:.2e}")
    assert merr < mel_bar and rms < wav_bar and wblk < wav_bar, (merr, rms, wblk)


@pytest.mark.parametrize("order", ["as_listed", "shuffled"])
def test_ragged_decode_is_bit_identical_to_alone_decodes_in_f32(weights, order):
    """gemm "f32" (one GEMM kernel, no size switch), fewer than 12288 frames: every segment of the ragged call equals its alone decode
    through dvae_decode / vocos_decode bit for bit, mel and waveform, in two segment orders -- no frame reads across a boundary"""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")
    lens = [1, 2, 3, 7, 40, 50, 51, 52, 75, 150, 300]
    if order == "shuffled":
        lens = [lens[i] for i in np.random.RandomState(5).permutation(len(lens))]
    g = torch.Generator(device=DEV).manual_seed(7)
    rows = [torch.randn((t, 768), device=DEV, generator=g) for t in lens]
    assert 2 * sum(lens) < 12288
    wav, off, mel = codec.decode_ragged(rows, return_mel=True)
    f0 = 0
    for i, r in enumerate(rows):
        m1, w1 = _alone(codec, r)
        assert torch.equal(mel[f0: f0 + 2 * lens[i]], m1), (i, lens[i])
        assert torch.equal(wav[off[i]: off[i + 1]], w1), (i, lens[i])
        f0 += 2 * lens[i]
    # views work as rows, and a single segment is the alone decode itself
    big = torch.randn((60, 768), device=DEV, generator=g)
    w2, o2 = codec.decode_ragged([big[10:13], big[20:60]])
    assert torch.equal(w2[o2[0]: o2[1]], _alone(codec, big[10:13].contiguous())[1])
    assert torch.equal(w2[o2[1]: o2[2]], _alone(codec, big[20:60].contiguous())[1])
    w3, o3 = codec.decode_ragged([rows[0]])
    assert torch.equal(w3, _alone(codec, rows[0])[1])


def _bench_rows():
    rs = np.random.RandomState(17)
    lens = rs.randint(128, 513, size=40)
    return [torch.from_numpy(rs.standard_normal((int(t), 768)).astype(np.float32) * 0.5).to(DEV) for t in lens]


_RUNMIN_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from chattts_amd import engine as E, weights as W
sds = W.synthetic_all()
codec = E.CodecEngine(sds["decoder"], sds["vocos"], torch.device("cuda:0"), gemm="f32")
z = np.load(sys.argv[2])
rows = [torch.from_numpy(z["r%d" % i]).cuda() for i in range(int(z["n"]))]
wav, off = codec.decode_ragged(rows)
pad = codec.decode_to_wavs(rows[:16])
np.savez(sys.argv[3], ragged=wav.cpu().numpy(), padded=pad.cpu().numpy())
"""


def test_ragged_decode_at_bench_sizes_against_alone_decodes(weights, tmp_path):
    """40 segments of U{128..512} tokens (>= 12288 frames packed: the sliding-window dwconv kernels, the 256 x 256 split-bf16 tiles and
    the x3p / h1p planes are taken, while each segment alone runs on the small-size kernels).  Per segment against its alone decode:
    bf16x3 and f32 bit for bit, f16 within the mode's 2e-5 RMS bar.  Then, in f32, the per-frame and the
    sliding-window dwconv kernels: first the padded path with CTTS_DWCONV_RUN_MIN_ROWS=0 (per-frame kernel only) against the default
    (run kernel) bit for bit, then the ragged call likewise (a fresh process: the threshold is read once)."""
    rows = _bench_rows()
    assert 2 * sum(int(r.shape[0]) for r in rows) >= 12288
    worst = {}
    outs = {}
    for gemm in GEMMS:
        codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
        wav, off = codec.decode_ragged(rows)
        outs[gemm] = (wav, off, codec)
        errs = []
        differ = []
        for i, r in enumerate(rows):
            w1 = _alone(codec, r)[1]
            w = wav[off[i]: off[i + 1]]
            errs.append(_rms(w.cpu().numpy(), w1.cpu().numpy()))
            if not torch.equal(w, w1):
                differ.append((i, int(r.shape[0]), int(torch.nonzero(w != w1)[0, 0])))   # segment, tokens, first differing sample
        worst[gemm] = max(errs)
        print(f"ragged vs alone at bench sizes [{gemm}]: worst segment wav rms diff {worst[gemm]:.2e} (median {np.median(errs):.2e}), "
              f"{len(differ)} segments not bit-identical")
        if gemm in ("f32", "bf16x3"):
            assert not differ, (gemm, differ[:4])
    assert worst["f32"] == 0.0 and worst["bf16x3"] == 0.0, worst
    assert worst["f16"] < 2e-5, worst
    # the run-kernel check, in f32
    wav, off, codec = outs["f32"]
    pad = codec.decode_to_wavs(rows[:16]).cpu().numpy()
    assert 16 * 2 * max(int(r.shape[0]) for r in rows[:16]) >= 12288
    inp = tmp_path / "rows.npz"
    np.savez(inp, n=len(rows), **{"r%d" % i: r.cpu().numpy() for i, r in enumerate(rows)})
    res = tmp_path / "out.npz"
    env = dict(os.environ, CTTS_DWCONV_RUN_MIN_ROWS="0")
    p = subprocess.run([sys.executable, "-c", _RUNMIN_CHILD, ROOT, str(inp), str(res)], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(res)
    padded_same = np.array_equal(z["padded"], pad)
    print(f"f32, padded path: per-frame dwconv kernel == sliding-window kernel bit for bit: {padded_same}")
    assert padded_same
    assert np.array_equal(z["ragged"], wav.cpu().numpy())


def test_float_to_int16_ragged_is_bit_exact_per_segment(weights):
    """one peak per segment, the keep mask |x| > 1e-5 per segment starting on a byte boundary: bit-exact against audio.float_to_int16 of
    each segment (both products); segment lengths that are not multiples of 8, silent stretches, an all-zero segment"""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")
    rs = np.random.RandomState(9)
    lens = [1, 7, 8, 9, 256, 1000, 4099, 30000]
    segs = [(rs.standard_normal(n) * rs.choice([0.01, 0.3, 1.7, 40.0])).astype(np.float32) for n in lens]
    segs[3][:] = 0.0
    segs[5][100:600] = 1e-6
    flat = np.concatenate(segs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for product in ("f64", "f32"):
        pcm, keep, koff = codec.float_to_int16_ragged(torch.from_numpy(flat).to(DEV), off, product=product, keep_thr=1e-5)
        pcm_h, keep_h = pcm.cpu().numpy(), keep.cpu().numpy()
        assert np.array_equal(koff, np.concatenate([[0], np.cumsum([(n + 7) // 8 for n in lens])]))
        for i, s in enumerate(segs):
            assert np.array_equal(pcm_h[off[i]: off[i + 1]], float_to_int16(s, product)), (product, i)
            bits = np.unpackbits(keep_h[koff[i]: koff[i + 1]])[: lens[i]].astype(bool)
            assert np.array_equal(bits, np.abs(s) > np.float32(1e-5)), (product, i)
    pcm2, keep2, _ = codec.float_to_int16_ragged(torch.from_numpy(flat).to(DEV), off)     # no mask asked for
    assert keep2 is None
    for i, s in enumerate(segs):
        assert np.array_equal(pcm2.cpu().numpy()[off[i]: off[i + 1]], float_to_int16(s)), i


def test_decode_to_pcm16_ragged_equals_alone_strip_and_convert(weights):
    """Chat.decode_to_pcm16(rows, ragged=True) with the codec in "f32" == per row: the alone decode, the sample-level silence strip and
    float_to_int16, bit for bit; decode_to_wavs(rows, ragged=True) == the alone waveforms; use_decoder=False refuses"""
    from chattts_amd.core import Chat
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32", codec_gemm="f32")
    g = torch.Generator(device=DEV).manual_seed(21)
    rows = [torch.randn((t, 768), device=DEV, generator=g) for t in (5, 1, 64, 33, 200)]
    got = chat.decode_to_pcm16(rows, ragged=True)
    wavs = chat.decode_to_wavs(rows, ragged=True)
    assert isinstance(got, list) and len(got) == len(rows) and len(wavs) == len(rows)
    for r, p, w in zip(rows, got, wavs):
        alone = chat.decode_to_wavs([r])[0]
        assert np.array_equal(w, alone)
        assert p.dtype == np.int16 and np.array_equal(p, float_to_int16(alone[np.abs(alone) > np.float32(1e-5)]))
    unstripped = chat.decode_to_pcm16(rows, strip=False, ragged=True)
    for r, p in zip(rows, unstripped):
        assert np.array_equal(p, float_to_int16(chat.decode_to_wavs([r])[0]))
    with pytest.raises(NotImplementedError):
        chat.decode_to_wavs([torch.zeros((3, 4), dtype=torch.int64)], use_decoder=False, ragged=True)
    with pytest.raises(ValueError):
        chat.infer("hello", stream=True, ragged_decode=True)


@pytest.mark.parametrize("codec_gemm", ["f32", None])
def test_batcher_ragged_decode_matches_each_request_alone(weights, codec_gemm):
    """SpeechBatcher(ragged_decode=True) behind create_app on a loaded synthetic Chat: several concurrent requests; a recording
    subclass keeps every request's hidden states.  codec "f32": every response equals finish(hid) -- the alone decode, strip and
    convert -- of its own recorded hidden states bit for bit; default codec mode: the recorded waveforms' ragged decodes are within
    1e-6 RMS of the alone decodes.  At least one poll decoded >= 2 requests in one call; /health shows the counts."""
    import io
    import wave
    from starlette.testclient import TestClient
    from chattts_amd import server
    from chattts_amd.core import Chat
    from chattts_amd.serving import SpeechBatcher
    gold_dir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold_dir, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype="f32", tokenizer=os.path.join(gold_dir, "tokenizer"), spk_stat=spk_stat,
                     codec_gemm=codec_gemm)
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker(), "alloy": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 48})
    texts = ["Hello there.", "The quick brown fox jumps over the lazy dog.", "Good morning!", "How are you today?",
             "Numbers like 42 and 7.", "A sixth request."]
    vs = ["default", "alloy", "alloy", "default", "alloy", "default"]

    class Recording(SpeechBatcher):
        def finish_group(self, hids):
            out = super().finish_group(hids)
            for h, r in zip(hids, out):
                if not isinstance(r, BaseException):
                    self.rec.append((h.clone(), r))
            return out

    def pcm_of(r):
        with wave.open(io.BytesIO(r.content), "rb") as wf:
            return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")

    lock = threading.Lock()
    b = Recording(chat, 8, lock, ragged_decode=True)
    b.rec = []
    app = server.create_app(chat, voices, batcher=b)
    res = [None] * len(texts)
    with TestClient(app) as c:
        def one(i):
            res[i] = c.post("/v1/audio/speech", json={"input": texts[i], "voice": vs[i], "response_format": "wav"})
        ths = [threading.Thread(target=one, args=(i,)) for i in range(len(texts))]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=600)
        health = c.get("/health").json()
    b.close()
    assert all(r is not None and r.status_code == 200 for r in res), [None if r is None else r.status_code for r in res]
    occ = health["pool"]
    print(f"ragged batcher [{chat.codec.gemm}]: {occ}")
    assert occ["ragged_decode"] and occ["completed"] == len(texts) and occ["decoded"] == len(texts)
    assert occ["max_decode_group"] >= 2 and occ["decode_calls"] < len(texts)
    assert len(b.rec) == len(texts)
    bodies = [pcm_of(r) for r in res]
    for h, pcm in b.rec:
        assert any(x.shape == pcm.shape and np.array_equal(x, pcm) for x in bodies)      # the response carries what the group decode gave it
        if chat.codec.gemm == "f32":
            assert np.array_equal(pcm, b.finish(h))
    if chat.codec.gemm != "f32":
        hids = [h for h, _ in b.rec]
        wav, off = chat.codec.decode_ragged(hids)
        for i, h in enumerate(hids):
            rms = _rms(wav[off[i]: off[i + 1]].cpu().numpy(), chat.codec.decode_to_wavs([h]).cpu().numpy()[0])
            assert rms < 1e-6, (i, rms)

"""Pins both restatements of the Vocos decode (oracle/torch_port.py, oracle/codec_np.py) against tests/golden/vocos_ref.npz, whose
backbone blocks were evaluated by the reference's own `ConvNeXtBlock` (oracle/make_vocos_goldens.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import codec_np, ref_harness, torch_port

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocos_ref.npz")
FRAMES = (2, 9, 66)
# measured when the fixture was made: 4.4e-9 ... 1.5e-8 (torch_port, by the thread count torch runs it on) and 1.8e-8 ... 2.0e-8 (codec_np) on
# a signal of 3.4e-2 RMS; the bar is 50 x the worse of the two and 100 x below the 1e-4 RMS the device decoder is held to
BAR = 1e-6


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def _rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_fixture_holds_the_stated_inputs_and_rebuilds_from_the_reference(ref):
    """the fixture's inputs are the stated ones; and where the reference tree is present (the build container), the committed fixture IS
    what its class computes today, bit for bit"""
    assert sorted(ref.files) == sorted(f"F{F}.{k}" for F in FRAMES for k in ("mel", "wav"))
    for F in FRAMES:
        mel = torch.randn((2, 100, F), generator=torch.Generator().manual_seed(F), dtype=torch.float32).numpy()
        assert np.array_equal(ref[f"F{F}.mel"], mel)
        wav = ref[f"F{F}.wav"]
        assert wav.shape == (2, 256 * (F - 1)) and wav.dtype == np.float32 and np.isfinite(wav).all()
        assert 2e-2 < float(np.sqrt(np.mean(wav.astype(np.float64) ** 2))) < 5e-2
    if ref_harness.available():
        from oracle import make_vocos_goldens
        now = make_vocos_goldens.build()
        assert sorted(now) == sorted(ref.files)
        for k in ref.files:
            assert np.array_equal(now[k], ref[k]), k


@pytest.mark.parametrize("F", FRAMES)
def test_torch_port_vocos_decode_equals_the_reference_block_fixture(weights, ref, F):
    got = torch_port.vocos_decode(weights["vocos"], torch.from_numpy(ref[f"F{F}.mel"])).numpy()
    want = ref[f"F{F}.wav"]
    assert got.shape == want.shape
    rms = _rms(got, want)
    print(f"torch_port.vocos_decode vs reference-block fixture, F={F}: rms {rms:.2e}")
    assert rms < BAR, rms


@pytest.mark.parametrize("F", FRAMES)
def test_codec_np_vocos_decode_equals_the_reference_block_fixture(weights, ref, F):
    sd = {k: v.numpy() for k, v in weights["vocos"].items()}
    got = codec_np.vocos_decode(sd, np.ascontiguousarray(ref[f"F{F}.mel"].transpose(0, 2, 1)))
    want = ref[f"F{F}.wav"]
    assert got.shape == want.shape
    rms = _rms(got, want)
    print(f"codec_np.vocos_decode vs reference-block fixture, F={F}: rms {rms:.2e}")
    assert rms < BAR, rms

"""CPU: the engine's repack of `downsample_conv.2.weight` (chattts_amd/dvae.py `pair_repack_k4s2`) turns the stride-2 k4 convolution
over frames into a stride-1 k3 convolution over frame PAIRS.  Checked here on the host against the oracle's k4/s2 convolution, with the
same zero frame appended for an odd frame count and the same `T` rows kept that `ctts_dvae_encode` uses on the device."""
import numpy as np
import pytest
import torch

from chattts_amd.dvae import pair_repack_k4s2
from oracle import codec_np, dvae_np

f32 = np.float32
C_IN, C_OUT = 8, 6


def paired_conv(x: np.ndarray, w4: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x [F, C] -> [T, Cout] through the repacked weight: what the device computes, restated with the oracle's dense k3 conv"""
    F, Cin = x.shape
    Fe = (F + 1) & ~1
    xe = np.zeros((Fe, Cin), f32)
    xe[:F] = x                                                           # an odd F gets one zero frame
    pair = pair_repack_k4s2(torch.from_numpy(w4)).numpy()                # [Cout, 3, 2C]
    assert pair.shape == (w4.shape[0], 3, 2 * Cin) and pair.dtype == f32
    y = codec_np.conv1d_cl(xe.reshape(1, Fe // 2, 2 * Cin), np.ascontiguousarray(pair.transpose(0, 2, 1)), b, pad=1)[0]
    return y[: (F - 2) // 2 + 1]


@pytest.mark.parametrize("F", [3, 4, 5, 6, 7, 33, 34])
def test_pair_repack_is_the_k4_stride2_conv(F):
    rs = np.random.RandomState(100 + F)
    x = rs.standard_normal((F, C_IN)).astype(f32)
    w4 = (rs.standard_normal((C_OUT, C_IN, 4)) / np.sqrt(4 * C_IN)).astype(f32)
    b = (0.1 * rs.standard_normal(C_OUT)).astype(f32)
    ref = dvae_np.conv1d_k4s2_cl(x[None], w4, b)[0]
    got = paired_conv(x, w4, b)
    assert got.shape == ref.shape == ((F - 2) // 2 + 1, C_OUT)
    err = float(np.abs(got - ref).max())
    print(f"pair repack F={F}: max |diff| {err:.2e}")
    assert err <= 1e-5


def test_pair_repack_layout():
    """taps {[0, W0], [W1, W2], [W3, 0]}: every weight of the k4 kernel lands once, the two corner blocks are exactly zero"""
    w4 = torch.arange(1, 1 + C_OUT * C_IN * 4, dtype=torch.float32).reshape(C_OUT, C_IN, 4)
    p = pair_repack_k4s2(w4.to(torch.float64))                            # any float dtype in, float32 out
    assert p.dtype == torch.float32
    assert torch.equal(p[:, 0, :C_IN], torch.zeros(C_OUT, C_IN)) and torch.equal(p[:, 2, C_IN:], torch.zeros(C_OUT, C_IN))
    assert torch.equal(p[:, 0, C_IN:], w4[:, :, 0]) and torch.equal(p[:, 1, :C_IN], w4[:, :, 1])
    assert torch.equal(p[:, 1, C_IN:], w4[:, :, 2]) and torch.equal(p[:, 2, :C_IN], w4[:, :, 3])

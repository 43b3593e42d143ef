"""The device resampler (csrc/resample.hip, CodecEngine.resample) against the float64 oracle, sample by sample under the float32
dot-product bound, and segment independence bit for bit.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import resample as RS  # noqa: E402
from tests.resample_oracle import PAIRS, oracle_taps, reduced, resample_f64  # noqa: E402

DEV = torch.device("cuda:0")
TILE = RS.TILE          # the kernel's one tile size, in output samples


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _pack(rng, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.uniform(-1, 1, int(off[-1])).astype(np.float32), off


def _run(codec, x, off, orig, new):
    y, oo = codec.resample(torch.from_numpy(x).to(DEV), orig, new, offsets=off)
    torch.cuda.synchronize()
    return y.cpu().numpy(), np.asarray(oo)


def _edge_inputs(orig, new, t=1):
    """input lengths whose outputs end one below, at and above t tiles (every output length around the edge that the ratio can produce)"""
    M, L = reduced(orig, new)
    lo, hi = (t * TILE - 1) * M // L - 1, -(-(t * TILE + 1) * M // L) + 1
    return list(range(max(1, lo), hi + 1))


@pytest.mark.parametrize("orig,new", PAIRS)
def test_against_the_oracle_within_the_dot_product_bound(codec, orig, new):
    h, width = oracle_taps(orig, new)
    K = h.shape[1]
    lens = [1, 2, width - 1, width, width + 1, K, *_edge_inputs(orig, new), *_edge_inputs(orig, new, 2), 2049, orig]
    outs = {RS.out_len(n, *RS.ratio(orig, new)) for n in lens}
    assert any(o < TILE for o in outs) and any(o > TILE for o in outs) and (TILE in outs or new > orig)
    x, off = _pack(np.random.default_rng(orig + new), lens)
    y, oo = _run(codec, x, off, orig, new)
    worst = 0.0
    for i, n in enumerate(lens):
        want, a = resample_f64(x[off[i]: off[i + 1]], orig, new, with_bound=True)
        got = y[oo[i]: oo[i + 1]]
        assert got.shape == want.shape == (-(-n * reduced(orig, new)[1] // reduced(orig, new)[0]),), (n, got.shape, want.shape)
        bound = (K + 3) * 2.0 ** -24 * a                    # float32 dot product of K terms + the taps' rounding, per output sample
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (n, int(np.argmax(err - bound)), float(err.max()))
    print(f"{orig}->{new}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_every_segment_equals_itself_alone_bit_for_bit(codec, orig, new):
    M, L = reduced(orig, new)
    rng = np.random.default_rng(7 * orig + new)
    long_ = lambda: int(rng.integers(2500, 3500))
    e = -(-TILE * M // L)              # the input sample at which the first tile of outputs ends
    packs = [
        [v for s in range(1, 8) for v in (long_(), s)] + [long_()],                 # 1- to 7-sample segments between long ones
        [long_()] + [1] * 80 + [long_()],                                           # a run of 80 one-sample segments
        [1, long_(), 1],                                                            # a one-sample segment first and last
        [e - 1, e, e + 1, 2 * e - 1, 2 * e, 2 * e + 1, 3, e + 1, e - 1],            # segment ends 0 and +-1 input samples from the tile edges
    ]
    for lens in packs:
        x, off = _pack(rng, lens)
        y, oo = _run(codec, x, off, orig, new)
        for i in range(len(lens)):
            seg = x[off[i]: off[i + 1]]
            alone, _ = _run(codec, seg, np.array([0, len(seg)]), orig, new)
            assert y[oo[i]: oo[i + 1]].tobytes() == alone.tobytes(), (lens, i)


def test_padded_rows_equal_the_packed_rows(codec):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (5, 1237)).astype(np.float32)
    for orig, new in ((24000, 44100), (44100, 24000), (24000, 8000)):
        rows = codec.resample(torch.from_numpy(x).to(DEV), orig, new)
        packed, oo = codec.resample(torch.from_numpy(x.reshape(-1)).to(DEV), orig, new, offsets=np.arange(6) * 1237)
        one = codec.resample(torch.from_numpy(x[2]).to(DEV), orig, new)
        assert rows.shape == (5, RS.out_len(1237, *RS.ratio(orig, new))) and np.array_equal(np.diff(oo), [rows.shape[1]] * 5)
        assert rows.cpu().numpy().tobytes() == packed.cpu().numpy().tobytes()
        assert one.dim() == 1 and one.cpu().numpy().tobytes() == rows[2].cpu().numpy().tobytes()


def test_segments_at_their_own_rates_equal_each_alone(codec):
    rng = np.random.default_rng(5)
    lens, rates = [700, 1, 2300, 512, 4097], [8000, 44100, 24000, 8000, 48000]
    x, off = _pack(rng, lens)
    y, oo = codec.resample_segments(torch.from_numpy(x).to(DEV), off, rates)
    y = y.cpu().numpy()
    for i, r in enumerate(rates):
        seg = torch.from_numpy(x[off[i]: off[i + 1]]).to(DEV)
        assert y[oo[i]: oo[i + 1]].tobytes() == codec.resample(seg, 24000, r).cpu().numpy().tobytes(), i


def test_equal_rates_return_the_very_tensor(codec):
    t = torch.zeros(10, device=DEV)
    off = np.array([0, 4, 10])
    assert codec.resample(t, 24000, 24000) is t
    got = codec.resample(t, 16000, 16000, offsets=off)
    assert got[0] is t and got[1] is off


def test_refusals_reach_no_launch(codec, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a refused call was launched")
    monkeypatch.setattr(codec, "_resample_launch", boom)
    t = torch.zeros(12, device=DEV)
    for kw in (dict(orig=24000, new=24001), dict(orig=48000, new=1000), dict(orig=24000, new=8000, offsets=[0, 5, 5, 12]),
               dict(orig=24000, new=8000, offsets=[0, 9, 5, 12]), dict(orig=24000, new=8000, offsets=[0, 5]),
               dict(orig=24000, new=8000, offsets=[2, 12])):
        with pytest.raises(ValueError):
            codec.resample(t, **kw)
    with pytest.raises(ValueError):
        codec.resample(t.cpu(), 24000, 8000)
    with pytest.raises(ValueError):
        codec.resample_segments(t, [0, 5, 5, 12], [8000, 16000, 8000])

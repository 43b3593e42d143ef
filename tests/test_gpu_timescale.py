"""The device time scaler (csrc/timescale.hip, CodecEngine.time_scale) against the float64 oracle -- the search's path exactly, every
sample under the float32 bound of the overlap-add -- and segment independence bit for bit.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import timescale as TS  # noqa: E402
from tests.timescale_oracle import HOP, RAD, WIN, time_scale_f64  # noqa: E402

DEV = torch.device("cuda:0")
SPEEDS = (0.5, 0.75, 0.9, 1.1, 1.25, 1.5, 2.0)


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(scope="module")
def segments():
    segs = [np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32) for seed in range(5) for n in (1, 300, 512, 1024, 1500, 4096, 12000)]
    segs.append(np.zeros(3000, np.float32))                      # all zero: every frame is decided by the tie rule
    run = np.random.default_rng(11).uniform(-1, 1, 9000).astype(np.float32)
    run[3000:6000] = 0.0                                         # a zero run in the middle: the search walks into silence and out of it
    segs.append(run)
    return segs


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _run(codec, x, off, speed):
    y, oo, path, po = codec.time_scale(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), speed, offsets=off, return_path=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), np.asarray(oo), path.cpu().numpy(), np.asarray(po)


@pytest.mark.parametrize("speed", SPEEDS)
def test_path_and_samples_against_the_oracle(codec, segments, speed):
    num = int(round(100 * speed))
    want = [time_scale_f64(x, speed) for x in segments]
    # a condition on the fixture, on EVERY frame of every segment: the oracle's winner leads by more than float32 can blur, or the frame
    # is all zero (then the tie rule makes it exact: d = 0)
    worst, zero_frames = np.inf, 0
    for x, o in zip(segments, want):
        r = o["ratio"][1:]
        worst = min(worst, float(r.min())) if r.size else worst
        assert np.all(r > 1.0), (len(x), speed, float(r.min()), int(np.argmin(r)) + 1)
        for k in np.flatnonzero(o["zero_frame"]):
            assert o["path"][k] == (k * HOP * num) // 100 - HOP, (len(x), speed, int(k))
        zero_frames += int(o["zero_frame"].sum())
    assert zero_frames > 0
    off = _offsets([len(x) for x in segments])
    y, oo, path, po = _run(codec, np.concatenate(segments), off, speed)
    err_worst = 0.0
    for i, (x, o) in enumerate(zip(segments, want)):
        n_out = -(-len(x) * 100 // num)
        assert oo[i + 1] - oo[i] == n_out == o["y"].shape[0], (i, len(x))
        assert po[i + 1] - po[i] == -(-n_out // HOP) + 1 == o["path"].shape[0], (i, len(x))
        got_path = path[po[i]: po[i + 1]].astype(np.int64)
        assert np.array_equal(got_path, o["path"]), (i, len(x), speed, np.flatnonzero(got_path != o["path"])[:4])
        # two table roundings, two products, one sum
        bound = 4 * 2.0 ** -24 * (o["w_a"] * np.abs(o["xa"]) + o["w_b"] * np.abs(o["xb"]))
        err = np.abs(y[oo[i]: oo[i + 1]].astype(np.float64) - o["y"])
        assert np.all(err <= bound), (i, len(x), speed, int(np.argmax(err - bound)), float(err.max()))
        err_worst = max(err_worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"speed {speed}: smallest margin ratio {worst:.3f}, {zero_frames} all-zero frames, worst error / bound {err_worst:.3f}")


def test_the_host_twin_of_the_overlap_add_equals_the_device_bit_for_bit(codec, segments):
    x = segments[6]                                   # 12000 samples
    for speed in (0.75, 1.25):
        y, path = codec.time_scale(torch.from_numpy(x).to(DEV), speed, return_path=True)
        assert TS.apply(x, speed, path.cpu().numpy()).tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("speed", (0.5, 1.25, 2.0))
def test_every_segment_equals_itself_alone_bit_for_bit(codec, speed):
    rng = np.random.default_rng(int(100 * speed))
    long_ = lambda: int(rng.integers(2500, 3500))
    packs = [
        [v for s in range(1, 8) for v in (long_(), s)] + [long_()],                 # 1- to 7-sample segments between long ones
        [long_()] + [1] * 80 + [long_()],                                           # a run of 80 one-sample segments
        [1, long_(), 1],                                                            # a one-sample segment first and last
        [e + d for e in (HOP, WIN, WIN + 2 * RAD) for d in (-1, 0, 1)] + [3, HOP + 1, HOP - 1],   # 0 and +-1 around HS, N, N + 2 D
    ]
    for lens in packs:
        off = _offsets(lens)
        x = rng.uniform(-1, 1, int(off[-1])).astype(np.float32)
        y, oo, path, po = _run(codec, x, off, speed)
        for i in range(len(lens)):
            seg = x[off[i]: off[i + 1]]
            ya, _, pa, _ = _run(codec, seg, np.array([0, len(seg)]), speed)
            assert path[po[i]: po[i + 1]].tobytes() == pa.tobytes(), (lens, i)
            assert y[oo[i]: oo[i + 1]].tobytes() == ya.tobytes(), (lens, i)


def test_padded_rows_equal_the_packed_rows(codec):
    x = np.random.default_rng(3).uniform(-1, 1, (5, 1237)).astype(np.float32)
    for speed in (0.8, 1.5):
        rows, rpath = codec.time_scale(torch.from_numpy(x).to(DEV), speed, return_path=True)
        packed, oo = codec.time_scale(torch.from_numpy(x.reshape(-1)).to(DEV), speed, offsets=np.arange(6) * 1237)
        one = codec.time_scale(torch.from_numpy(x[2]).to(DEV), speed)
        n_out = TS.out_len(1237, *TS.quantize(speed))
        assert rows.shape == (5, n_out) and rpath.shape == (5, TS.frames(n_out)) and np.array_equal(np.diff(oo), [n_out] * 5)
        assert rows.cpu().numpy().tobytes() == packed.cpu().numpy().tobytes()
        assert one.dim() == 1 and one.cpu().numpy().tobytes() == rows[2].cpu().numpy().tobytes()


def test_segments_at_their_own_speeds_equal_each_alone(codec):
    rng = np.random.default_rng(5)
    lens, speeds = [700, 1, 2300, 2300, 512, 4097, 30], [1.25, 1.25, 1.0, 0.8, 1.0, 2.0, 1.0]
    off = _offsets(lens)
    x = rng.uniform(-1, 1, int(off[-1])).astype(np.float32)
    y, oo = codec.time_scale_segments(torch.from_numpy(x).to(DEV), off, speeds)
    y = y.cpu().numpy()
    for i, s in enumerate(speeds):
        seg = x[off[i]: off[i + 1]]
        want = seg if s == 1.0 else codec.time_scale(torch.from_numpy(seg).to(DEV), s).cpu().numpy()
        assert y[oo[i]: oo[i + 1]].tobytes() == want.tobytes(), i


def test_speed_one_returns_the_very_tensor(codec):
    t = torch.zeros(10, device=DEV)
    off = np.array([0, 4, 10])
    assert codec.time_scale(t, 1.0) is t
    assert codec.time_scale(t, 1.004) is t            # hundredths: 1.004 is 100 / 100
    got = codec.time_scale(t, 1.0, offsets=off)
    assert got[0] is t and got[1] is off


def test_refusals_reach_no_launch(codec, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a refused call was launched")
    monkeypatch.setattr(codec, "_time_scale_launch", boom)
    t = torch.zeros(12, device=DEV)
    for kw in (dict(speed=0.49), dict(speed=2.01), dict(speed=float("nan")), dict(speed=1.25, offsets=[0, 5, 5, 12]),
               dict(speed=1.25, offsets=[0, 9, 5, 12]), dict(speed=1.25, offsets=[0, 5]), dict(speed=1.25, offsets=[2, 12])):
        with pytest.raises(ValueError):
            codec.time_scale(t, **kw)
    with pytest.raises(ValueError):
        codec.time_scale(t.cpu(), 1.25)
    with pytest.raises(ValueError):
        codec.time_scale_segments(t, [0, 5, 5, 12], [1.25, 1.0, 0.8])
    with pytest.raises(ValueError):
        codec.time_scale_segments(t, [0, 5, 12], [1.25, 3.0])


def test_the_library_refuses_before_it_launches(codec):
    """the C entry itself, past the host's plan: every refusal returns an error and leaves y and the path untouched"""
    import ctypes as C
    from chattts_amd import _lib
    n, num = 1000, 125
    n_out = TS.out_len(n, num)
    x = torch.ones(n, device=DEV)
    y = torch.full((n_out + 8,), 7.0, device=DEV)
    path = torch.full((TS.frames(n_out) + 8,), 7, dtype=torch.int32, device=DEV)
    w = codec._time_scale_window()
    good = dict(off=[0, n], out=[0, n_out], po=[0, TS.frames(n_out)], num=num, den=100, x=x.data_ptr(), w=w.data_ptr())

    def call(**over):
        a = {**good, **over}
        tabs = [np.asarray(a[k], dtype=np.int64) for k in ("off", "out", "po")]
        dev = [torch.from_numpy(t).to(DEV) for t in tabs]
        rc = codec.lib.ctts_time_scale_ragged(a["x"], dev[0].data_ptr(), tabs[0].ctypes.data_as(C.c_void_p), y.data_ptr(), dev[1].data_ptr(),
                                              tabs[1].ctypes.data_as(C.c_void_p), path.data_ptr(), dev[2].data_ptr(),
                                              tabs[2].ctypes.data_as(C.c_void_p), len(tabs[0]) - 1, a["w"], a["num"], a["den"],
                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    for over in (dict(x=None), dict(w=None), dict(num=49), dict(num=201), dict(num=100), dict(den=50, num=100), dict(off=[0, 0], out=[0, 0]),
                 dict(off=[0, n, n - 1], out=[0, n_out, n_out + 1], po=[0, 3, 5]), dict(out=[0, n_out + 1]), dict(out=[0, n_out - 1]),
                 dict(po=[0, TS.frames(n_out) + 1]), dict(off=[0, 1 << 31], out=[0, TS.out_len(1 << 31, num)], po=[0, TS.frames(TS.out_len(1 << 31, num))]),
                 dict(off=[0, 3 << 30], out=[0, 1 << 31], num=150, po=[0, TS.frames(1 << 31)])):
        assert call(**over) != 0, over
        assert b"ctts_time_scale_ragged" in _lib.lib().ctts_last_error(), over
    assert bool((y == 7.0).all()) and bool((path == 7).all())
    assert call() == 0
    assert bool((y[:n_out] != 7.0).all()) and bool((y[n_out:] == 7.0).all()) and bool((path[TS.frames(n_out):] == 7).all())

"""The streamed resampler (csrc/resample.hip resample_stream_k, CodecEngine.resample_stream_*) against the one-shot conversion of the
whole signal (`CodecEngine.resample`, itself pinned to the float64 oracle by tests/test_gpu_resample.py), bit for bit, under every way of
cutting a signal into pushes.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, resample as RS  # noqa: E402

DEV = torch.device("cuda:0")
ORIG = 24000
RATES = (8000, 16000, 44100, 22050, 48000)     # L = 1; L = 2; L = 147, table in LDS; table through L2; upsampling, more than one tile per push
N = 20000


def geometry(new):
    L, M = RS.ratio(ORIG, new)
    width, K = RS.geometry(L, M)
    return L, M, K, width


def schedules(n, new):
    """name -> push sizes adding up to n; the last push is the final one"""
    L, M, K, width = geometry(new)
    ready = lambda j: j * M + width + M                   # the samples frame j needs
    late = max(j for j in range(1, n) if ready(j) + 1 < n)
    edges, at = [], 0
    for j in (0, late):
        for target in (ready(j) - 1, ready(j), ready(j) + 1):       # one short of frame j, exactly at it, one past it
            edges.append(target - at)
            at = target
    edges.append(n - at)
    cyc, at = [], 0
    while at < n:
        cyc.append(min((511, 512, 513)[len(cyc) % 3], n - at))
        at += cyc[-1]
    return {"whole": [n], "ones": [1] * 5 + [n - 5], "hops": cyc, "empties": [3000, 0, 0, 2000, 0, n - 5000],
            "empty_final": [5000, n - 5000, 0], "big": [12000, n - 12000], "edges": edges}


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(scope="module")
def noise():
    x = np.random.default_rng(7).uniform(-1, 1, N).astype(np.float32)
    return x, torch.from_numpy(x).to(DEV)


_ONE = {}


def one_shot(codec, xd, new, n=None):
    """CodecEngine.resample of the first n samples of the signal, computed once per (rate, n) and left unchanged"""
    n = xd.numel() if n is None else n
    if (new, n) not in _ONE:
        _ONE[new, n] = codec.resample(xd[:n].contiguous(), ORIG, new).cpu().numpy()
    return _ONE[new, n]


def stream(codec, xd, new, sizes):
    """pushes xd through a fresh stream in `sizes` -> (chunks, plans)"""
    h = codec.resample_stream_open(ORIG, new)
    chunks, plans, at = [], [], 0
    try:
        for i, n in enumerate(sizes):
            final = i == len(sizes) - 1
            plans.append(codec.resample_stream_plan(h, n, final))
            y, off = codec.resample_stream_step(xd, [(h, at, n, final)])
            assert list(off) == [0, y.numel()]
            chunks.append(y.cpu().numpy())
            at += n
    finally:
        codec.resample_stream_close(h)
    return chunks, plans


def test_the_pairs_take_the_paths_they_are_named_for(codec):
    modes = {new: codec.lib.ctts_resample_supported(*geometry(new)[:3]) for new in RATES}
    assert modes == {8000: 2, 16000: 2, 44100: 2, 22050: 1, 48000: 2}
    assert geometry(8000)[0] == 1 and geometry(44100)[0] == 147 and RS.out_len(12000, *RS.ratio(ORIG, 48000)) > 2 * RS.TILE
    assert all(geometry(new)[2] - 1 <= RS.CARRY for new in RATES) and _lib.RS_STREAM.itemsize == 80


@pytest.mark.parametrize("new", RATES)
def test_every_way_of_cutting_the_signal_gives_the_one_shot_result_bit_for_bit(codec, noise, new):
    x, xd = noise
    want = one_shot(codec, xd, new)
    assert len(want) == RS.out_len(N, *RS.ratio(ORIG, new))
    for sched, sizes in schedules(N, new).items():
        assert sum(sizes) == N and min(sizes) >= 0, sched
        chunks, plans = stream(codec, xd, new, sizes)
        assert [len(c) for c in chunks] == [p["n_out"] for p in plans], (new, sched)
        assert np.concatenate(chunks).tobytes() == want.tobytes(), (new, sched)


@pytest.mark.parametrize("new", RATES)
def test_totals_around_the_first_complete_frame(codec, noise, new):
    x, xd = noise
    L, M, K, width = geometry(new)
    for n in (1, width + M - 1, width + M, width + M + 1):
        want = one_shot(codec, xd, new, n)
        cuts = [[n]] + ([[1, n - 1], [n - 1, 1], [n - 1, 1, 0]] if n > 1 else [[1, 0]])
        for sizes in cuts:
            chunks, plans = stream(codec, xd[:n].contiguous(), new, sizes)
            assert [len(c) for c in chunks] == [p["n_out"] for p in plans], (new, n, sizes)
            assert np.concatenate(chunks).tobytes() == want.tobytes(), (new, n, sizes)


def test_many_streams_at_mixed_rates_in_one_call_equal_each_alone(codec, noise):
    x, xd = noise
    rates = [RATES[i % len(RATES)] for i in range(12)]
    start = [137 * i for i in range(12)]                      # every stream reads its own stretch of the tensor
    total = [6000 + 211 * i for i in range(12)]
    sizes = [[1500 + 97 * i, 0, 513, total[i] - 2013 - 97 * i] for i in range(12)]
    hs = [codec.resample_stream_open(ORIG, r) for r in rates]
    got = [[] for _ in hs]
    try:
        assert codec.resample_streams_in_use() >= 12
        at = list(start)
        for step in range(4):
            pushes = [(h, at[i], sizes[i][step], step == 3) for i, h in enumerate(hs)]
            want_n = [codec.resample_stream_plan(h, sizes[i][step], step == 3)["n_out"] for i, h in enumerate(hs)]
            y, off = codec.resample_stream_step(xd, pushes)
            assert list(np.diff(off)) == want_n
            yh = y.cpu().numpy()
            for i in range(12):
                got[i].append(yh[int(off[i]): int(off[i + 1])])
                at[i] += sizes[i][step]
    finally:
        for h in hs:
            codec.resample_stream_close(h)
    for i, r in enumerate(rates):
        want = codec.resample(xd[start[i]: start[i] + total[i]].contiguous(), ORIG, r).cpu().numpy()
        assert np.concatenate(got[i]).tobytes() == want.tobytes(), (i, r)


def test_a_reopened_slot_starts_fresh_and_a_refused_call_changes_nothing(codec, noise):
    x, xd = noise
    want = one_shot(codec, xd, 8000)
    h = codec.resample_stream_open(ORIG, 8000)
    codec.resample_stream_step(xd, [(h, 0, 7000, False)])      # leaves a carry in the slot
    codec.resample_stream_close(h)
    h2 = codec.resample_stream_open(ORIG, 8000)
    assert h2 == h                                              # the same slot, not cleared
    try:
        a, _ = codec.resample_stream_step(xd, [(h2, 0, 5000, False)])
        rec = codec._pool("resample").records[h2]
        with pytest.raises(ValueError, match="outside the tensor"):
            codec.resample_stream_step(xd, [(h2, N - 10, 20, False)])
        with pytest.raises(ValueError, match="twice"):
            codec.resample_stream_step(xd, [(h2, 5000, 10, False), (h2, 5010, 10, False)])
        with pytest.raises(ValueError, match="not open"):
            codec.resample_stream_step(xd, [(h2, 5000, 10, False), (h2 + 1000, 5010, 10, False)])
        assert codec._pool("resample").records[h2] == rec               # nothing was committed
        b, _ = codec.resample_stream_step(xd, [(h2, 5000, N - 5000, True)])
        assert np.concatenate([a.cpu().numpy(), b.cpu().numpy()]).tobytes() == want.tobytes()
        with pytest.raises(ValueError, match="last push"):
            codec.resample_stream_step(xd, [(h2, 0, 10, False)])
    finally:
        codec.resample_stream_close(h2)
    with pytest.raises(ValueError, match="carry up to"):
        codec.resample_stream_open(48000, 11025)                # K = 694: beyond what a slot keeps


def test_the_pool_grows_under_a_live_stream_and_keeps_its_carry():
    """a pool of 4 slots doubles while a stream is half way: the stream goes on bit for bit, and a slot of the new half works like any"""
    from chattts_amd.engine import CodecEngine

    class Small(CodecEngine):
        RS_STREAM_SLOTS = 4

    eng = Small.__new__(Small)                          # the resampler needs the library and a device, no weights
    eng.lib, eng.device = _lib.lib(), DEV
    xd = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, 3000).astype(np.float32)).to(DEV)
    want = eng.resample(xd, ORIG, 8000).cpu().numpy()
    h = eng.resample_stream_open(ORIG, 8000)
    first, _ = eng.resample_stream_step(xd, [(h, 0, 1500, False)])
    assert eng._pool("resample").slots == 4
    more = [eng.resample_stream_open(ORIG, 8000) for _ in range(4)]
    pool = eng._pool("resample")
    assert pool.slots == 8 and int(pool.buf["carry"].shape[0]) == 8 and max(more) >= 4
    rest, _ = eng.resample_stream_step(xd, [(h, 1500, 1500, True)])
    assert np.concatenate([first.cpu().numpy(), rest.cpu().numpy()]).tobytes() == want.tobytes()
    whole, _ = eng.resample_stream_step(xd, [(max(more), 0, 3000, True)])
    assert whole.cpu().numpy().tobytes() == want.tobytes()
    for m in more + [h]:
        eng.resample_stream_close(m)
    assert eng.resample_streams_in_use() == 0

"""The limiter of streams (csrc/limiter.hip limiter_stream_k, CodecEngine.peak_limit_stream_*) against the one-shot limiter of the whole
signal (`CodecEngine.peak_limit`, itself pinned to the twin by tests/test_gpu_limiter.py) and against the NumPy twin, bit for bit in
samples and in the final record, under every way of cutting a signal into pushes.  All segments of tests/limiter_cases.py at one rate
run as concurrent streams, one descriptor each per step, so a cut costs a handful of launches.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, limiter as LM  # noqa: E402
from tests import limiter_cases as LCs, limiter_stream_cases as SC  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = np.float32(-7.25)


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(autouse=True)
def no_stream_left_open(codec):
    yield
    assert codec.peak_limit_streams_in_use() == 0


_PACK = {}


def pack(codec, fs):
    """the segments of a rate packed on the device, and `peak_limit` of each as if alone: computed once per rate, left unchanged"""
    if fs not in _PACK:
        cs = LCs.cases(fs)
        off = LCs.offsets([len(x) for _, x, _ in cs])
        xd = torch.from_numpy(np.concatenate([x for _, x, _ in cs])).to(DEV)
        y, stats = codec.peak_limit(xd, offsets=off, rates=fs, gains=[g for _, _, g in cs], return_stats=True)
        _PACK[fs] = (xd, off, y.cpu().numpy(), stats)
    return _PACK[fs]


def run_streams(codec, xd, jobs):
    """jobs: [(fs, gain, in_lo, sizes)], each a stream over xd[in_lo ..] pushed in `sizes` (the last one final); stream j takes part in
    step k while it has a k-th push -> (per stream its chunks, per stream its final record).  Chunk lengths are checked against _plan."""
    hs = [codec.peak_limit_stream_open(fs, g) for fs, g, _, _ in jobs]
    chunks, at, recs = [[] for _ in jobs], [lo for _, _, lo, _ in jobs], [None] * len(jobs)
    try:
        for k in range(max(len(s) for _, _, _, s in jobs)):
            live = [j for j, job in enumerate(jobs) if k < len(job[3])]
            pushes = [(hs[j], at[j], jobs[j][3][k], k == len(jobs[j][3]) - 1) for j in live]
            want = [codec.peak_limit_stream_plan(h, n, fin)["n_out"] for h, _, n, fin in pushes]
            y, off = codec.peak_limit_stream_step(xd, pushes)
            assert [int(v) for v in np.diff(off)] == want and int(off[-1]) == y.numel()
            yh = y.cpu().numpy()
            for i, j in enumerate(live):
                chunks[j].append(yh[off[i]: off[i + 1]])
                at[j] += jobs[j][3][k]
                if pushes[i][3]:
                    recs[j] = codec.peak_limit_stream_stats(hs[j])
    finally:
        for h in hs:
            codec.peak_limit_stream_close(h)
    return chunks, recs


@pytest.mark.parametrize("cut", list(SC.cuts(24000)))
@pytest.mark.parametrize("fs", SC.RATES)
def test_every_cut_returns_the_one_shot_limiters_bits_and_record(codec, fs, cut):
    xd, off, y_one, st_one = pack(codec, fs)
    before = xd.clone()
    cs = LCs.cases(fs)
    jobs = [(fs, g, int(off[i]), SC.schedule(len(x), SC.cuts(fs)[cut], fs)) for i, (_, x, g) in enumerate(cs)]
    chunks, recs = run_streams(codec, xd, jobs)
    assert torch.equal(xd, before)                                                       # the input is never written
    for i, ((name, x, g), (y_twin, rec_twin)) in enumerate(zip(cs, LCs.twin(fs))):
        got = np.concatenate(chunks[i])
        assert got.tobytes() == y_one[off[i]: off[i + 1]].tobytes(), (fs, cut, name)
        assert got.tobytes() == y_twin.tobytes(), (fs, cut, name)
        assert recs[i].tobytes() == st_one[i].tobytes() == rec_twin.tobytes(), (fs, cut, name, recs[i], st_one[i])
        # the lag: every push but the last has emitted all but the last 2 W samples
        sizes, W = jobs[i][3], fs // 100
        assert [len(c) for c in chunks[i]][:-1] == list(np.diff([max(0, p - 2 * W) for p in np.concatenate([[0], np.cumsum(sizes[:-1])])]))
    assert any(r["n_touched"] > 0 for r in recs) and any(r["n_over"] == 0 for r in recs)


@pytest.mark.parametrize("fs", (8000, 48000))
def test_peaks_at_a_push_boundary(codec, fs):
    """one peak at b - 1, b, b +- 2 W, b +- (2 W + 1) around the push boundary b, each alone and all together: the twin's touched
    samples lie at the boundaries (the push's, b, and the emission's, b - 2 W), so the streams cannot agree with the limiter idle there"""
    W, b, n = fs // 100, 3 * LCs.TILE + 7, 6 * LCs.TILE
    base = LCs.enveloped(11, n)
    at = [b - 1, b, b - 2 * W, b + 2 * W, b - 2 * W - 1, b + 2 * W + 1]
    sigs = []
    for p in at:
        x = base.copy()
        x[p] = 1.7
        sigs.append(x)
    both = base.copy()
    both[at] = [1.7, -1.3, 1.1, -1.9, 1.5, -1.2]
    sigs.append(both)
    for x, p in zip(sigs, at):
        _, _, s = LM.gain_curve(x, fs)
        t = np.flatnonzero(s < 1)
        assert t[0] == max(0, p - 2 * W) and t[-1] == p + 2 * W and len(t) == 4 * W + 1      # the dip reaches 2 W to either side
        assert t[0] <= b + 1 and t[-1] >= b - 1                                              # .. and covers or abuts the push boundary
    _, _, s = LM.gain_curve(both, fs)
    assert all(s[i] < 1 for i in (b - 1, b, b - 2 * W - 1, b - 2 * W, b - 4 * W - 1, b + 4 * W + 1))   # it spans both boundaries
    xd = torch.from_numpy(np.concatenate(sigs)).to(DEV)
    jobs = [(fs, 1.0, i * n, [b, n - b]) for i in range(len(sigs))] + [(fs, 1.0, i * n, [b - 2 * W, 2 * W, 2 * W, n - b - 2 * W]) for i in range(len(sigs))]
    chunks, recs = run_streams(codec, xd, jobs)
    for j, (chs, rec) in enumerate(zip(chunks, recs)):
        y, want = LM.limit_segment(sigs[j % len(sigs)], fs)
        assert np.concatenate(chs).tobytes() == y.tobytes() and rec.tobytes() == want.tobytes() and rec["n_touched"] >= 4 * W + 1, j


def test_eight_streams_of_mixed_rates_and_gains_in_one_step_equal_each_alone(codec):
    rng = np.random.default_rng(5)
    n = 9000
    specs = [(8000, 1.0), (48000, 2.5), (24000, 0.5), (22050, 1.75), (16000, 2.0), (44100, 1.0), (8000, 2.25), (32000, 1.5)]
    sigs = [(rng.uniform(-1, 1, n) * rng.choice([0.05, 0.3, 1.0], n)).astype(np.float32) for _ in specs]
    xd = torch.from_numpy(np.concatenate(sigs)).to(DEV)
    sizes = [[100 + 371 * j, 2048 + 13 * j, 0, 3000 - 200 * j] for j in range(len(specs))]           # unequal positions at every step
    jobs = [(fs, g, j * n, s + [n - sum(s)]) for j, ((fs, g), s) in enumerate(zip(specs, sizes))]
    together, recs = run_streams(codec, xd, jobs)
    for j, job in enumerate(jobs):
        alone, rec = run_streams(codec, xd, [job])
        y, want = LM.limit_segment(sigs[j], job[0], job[1])
        assert [c.tobytes() for c in together[j]] == [c.tobytes() for c in alone[0]], j
        assert np.concatenate(together[j]).tobytes() == y.tobytes() and recs[j].tobytes() == rec[0].tobytes() == want.tobytes(), j
    assert sum(r["n_over"] > 0 for r in recs) >= 4


def _raw_step(codec, xd, pushes, y, mutate=None):
    """ctts_peak_limit_stream_step on the engine's pool with a caller-owned y; the host records are not committed"""
    tab, _ = codec._lm_descriptors(pushes)
    o = np.zeros(len(pushes) + 1, np.int64)
    np.cumsum(tab["n_out"], out=o[1:])
    tab["out_off"] = o[:-1] + 16
    if mutate:
        mutate(tab)
    pool = codec._pool("limiter")
    tab_d = torch.from_numpy(tab.view(np.uint8)).to(DEV)
    rc = codec.lib.ctts_peak_limit_stream_step(xd.data_ptr(), xd.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(tab), y.data_ptr(),
                                               y.numel(), pool.buf["carry"].data_ptr(), pool.buf["stats"].data_ptr(), int(pool.buf["carry"].shape[0]), None)
    torch.cuda.synchronize()
    return rc, o


def test_canaries_around_the_output_stay_and_the_input_is_unwritten(codec):
    fs = 24000
    xd, off, y_one, _ = pack(codec, fs)
    cs = LCs.cases(fs)
    before = xd.clone()
    hs = [codec.peak_limit_stream_open(fs, g) for _, _, g in cs]
    try:
        pushes = [(h, int(off[i]), len(cs[i][1]), True) for i, h in enumerate(hs)]
        y = torch.full((xd.numel() + 32,), float(CANARY), dtype=torch.float32, device=DEV)
        rc, o = _raw_step(codec, xd, pushes, y)
        assert rc == 0 and int(o[-1]) == xd.numel()
        yh = y.cpu().numpy()
        assert np.all(yh[:16] == CANARY) and np.all(yh[-16:] == CANARY) and yh[16:-16].tobytes() == y_one.tobytes()
        assert torch.equal(xd, before)
    finally:
        for h in hs:
            codec.peak_limit_stream_close(h)


def test_a_slot_is_reused_clean_and_the_pool_grows_past_its_first_size(codec):
    fs, n = 16000, 5000
    loud = (np.random.default_rng(1).uniform(-1, 1, n)).astype(np.float32)
    quiet = (loud * np.float32(0.1)).astype(np.float32)
    xd = torch.from_numpy(np.concatenate([loud, quiet])).to(DEV)
    h = codec.peak_limit_stream_open(fs, 2.0)
    y, _ = codec.peak_limit_stream_step(xd, [(h, 0, n, True)])
    assert codec.peak_limit_stream_stats(h)["n_over"] > 0
    codec.peak_limit_stream_close(h)
    h2 = codec.peak_limit_stream_open(fs, 1.5)
    assert h2 == h                                                                        # the slot just given back
    fresh = codec.peak_limit_stream_stats(h2)
    assert (fresh["g32"], fresh["min_gain"], fresh["n_over"], fresh["n_touched"]) == (np.float32(1.5), 1.0, 0, 0)
    y1, _ = codec.peak_limit_stream_step(xd, [(h2, n, 1000, False)])                      # a quiet stream in the loud one's slot
    first = int(codec._pool("limiter").buf["carry"].shape[0])
    more = [codec.peak_limit_stream_open(fs, 2.0) for _ in range(first)]                  # every slot taken: the pool doubles under the open stream
    try:
        assert int(codec._pool("limiter").buf["carry"].shape[0]) == 2 * first and max(more) >= first and codec.peak_limit_streams_in_use() == first + 1
        y2, _ = codec.peak_limit_stream_step(xd, [(h2, n + 1000, n - 1000, True), (max(more), 0, n, True)])
        want_q, rec_q = LM.limit_segment(quiet, fs, 1.5)
        want_l, rec_l = LM.limit_segment(loud, fs, 2.0)
        got = torch.cat([y1, y2[: n - y1.numel()]]).cpu().numpy()
        assert got.tobytes() == want_q.tobytes() and y2[n - y1.numel():].cpu().numpy().tobytes() == want_l.tobytes()
        assert codec.peak_limit_stream_stats(h2).tobytes() == rec_q.tobytes() and rec_q["n_over"] == 0
        assert codec.peak_limit_stream_stats(max(more)).tobytes() == rec_l.tobytes() and y.cpu().numpy().tobytes() == want_l.tobytes()
    finally:
        for s in more + [h2]:
            codec.peak_limit_stream_close(s)


def test_a_refused_step_leaves_the_records_and_the_carry_as_they_were(codec):
    fs, n = 22050, 6000
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    a, b = codec.peak_limit_stream_open(fs, 1.5), codec.peak_limit_stream_open(fs, 2.0)
    try:
        ya, _ = codec.peak_limit_stream_step(xd, [(a, 0, 2500, False), (b, 0, 100, False)])
        pool = codec._pool("limiter")
        recs = dict(pool.records)
        carry, stats = pool.buf["carry"].clone(), pool.buf["stats"].clone()
        with pytest.raises(ValueError, match="outside the tensor"):                       # the engine's own check, behind a good push
            codec.peak_limit_stream_step(xd, [(a, 2500, 100, False), (b, n - 10, 11, False)])
        with pytest.raises(ValueError, match="twice"):
            codec.peak_limit_stream_step(xd, [(a, 2500, 100, False), (a, 2600, 100, False)])
        y = torch.full((n + 32,), float(CANARY), dtype=torch.float32, device=DEV)
        for mutate, why in [(lambda t: t["c_in"].__setitem__(1, 7), "carries"), (lambda t: t["slot"].__setitem__(1, 1 << 20), "outside the pool"),
                            (lambda t: t["gain"].__setitem__(0, np.inf), "pre-gain"), (lambda t: t["n_out"].__setitem__(1, 5), "emits")]:
            rc, _ = _raw_step(codec, xd, [(a, 2500, 3500, True), (b, 100, 900, False)], y, mutate)   # the library's, on its second descriptor
            assert rc != 0 and why in codec.lib.ctts_last_error().decode()
        assert dict(pool.records) == recs
        assert torch.equal(pool.buf["carry"], carry) and torch.equal(pool.buf["stats"], stats) and bool((y == float(CANARY)).all())
        yb, _ = codec.peak_limit_stream_step(xd, [(a, 2500, n - 2500, True)])              # the stream goes on as if nothing had been asked
        want, rec = LM.limit_segment(x, fs, 1.5)
        assert torch.cat([ya, yb]).cpu().numpy().tobytes() == want.tobytes() and codec.peak_limit_stream_stats(a).tobytes() == rec.tobytes()
    finally:
        codec.peak_limit_stream_close(a)
        codec.peak_limit_stream_close(b)

"""The streamed time scaler (csrc/timescale.hip timescale_stream_k, CodecEngine.time_scale_stream_*) against the one-shot call bit for
bit and the float64 oracle's path, under every way of cutting a signal into pushes.  `pytest -m gpu`."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, timescale as TS  # noqa: E402
from tests.timescale_oracle import HOP, time_scale_f64  # noqa: E402

DEV = torch.device("cuda:0")
SPEEDS = (0.5, 0.77, 0.99, 1.01, 1.25, 1.5, 2.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timescale_one_shot_sha256.json")


def signals():
    """noise, a tone (period 96 samples under a ramp: the ramp decides between the shifts by whole periods), noise around a zero run
    longer than a window, and totals around the hop.  The seeds are chosen so that the float64 oracle's margin ratio is above 1 on
    every frame at all seven speeds (smallest: 2.9, checked on the CPU and again below)."""
    t = np.arange(8000)
    run = np.random.default_rng(1).uniform(-1, 1, 9000).astype(np.float32)
    run[3000:6000] = 0.0
    out = {"noise": np.random.default_rng(2).uniform(-1, 1, 20000).astype(np.float32),
           "tone": (np.sin(2 * np.pi * t / 96) * (0.3 + 0.7 * t / 8000)).astype(np.float32), "run": run}
    for n in (1, 511, 512, 513):
        out[f"n{n}"] = np.random.default_rng(100 + n).uniform(-1, 1, n).astype(np.float32)
    return out


def schedules(n, num):
    """name -> push sizes adding up to n; the last push is the final one"""
    need = lambda k: TS.need(k, num)
    late = max(k for k in range(2, 400) if need(k) + 1 < n)
    edges, at = [], 0
    for k in (1, late):
        for target in (need(k) - 1, need(k), need(k) + 1):          # leaves n_avail one short of frame k, exactly at it, one past it
            edges.append(target - at)
            at = target
    edges.append(n - at)
    cyc, at = [], 0
    while at < n:
        cyc.append(min((HOP - 1, HOP, HOP + 1)[len(cyc) % 3], n - at))
        at += cyc[-1]
    big = [12000] * (n // 12000) + ([n % 12000] if n % 12000 else [])
    return {"whole": [n], "ones": [1] * 5 + [n - 5], "hops": cyc, "edges": edges, "empties": [3000, 0, 0, 2000, 0, n - 5000],
            "empty_final": [5000, n - 5000, 0], "big": big}


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(scope="module")
def sig():
    return signals()


_ONE = {}


def one_shot(codec, sig, name, speed):
    """(y, path) of CodecEngine.time_scale on the whole signal, computed once per (signal, speed) and left unchanged"""
    if (name, speed) not in _ONE:
        y, path = codec.time_scale(torch.from_numpy(sig[name]).to(DEV), speed, return_path=True)
        _ONE[name, speed] = (y.cpu().numpy(), path.cpu().numpy())
    return _ONE[name, speed]


def stream(codec, x, speed, sizes):
    """pushes x through a fresh stream in `sizes` -> (chunks, path pieces, plans)"""
    xd = torch.from_numpy(x).to(DEV)
    h = codec.time_scale_stream_open(speed)
    chunks, paths, plans, at = [], [], [], 0
    try:
        for i, n in enumerate(sizes):
            final = i == len(sizes) - 1
            plans.append(codec.time_scale_stream_plan(h, n, final))
            y, off, p, po = codec.time_scale_stream_step(xd, [(h, at, n, final)], return_path=True)
            assert list(off) == [0, y.numel()] and list(po) == [0, p.numel()]
            chunks.append(y.cpu().numpy())
            paths.append(p.cpu().numpy())
            at += n
    finally:
        codec.time_scale_stream_close(h)
    return chunks, paths, plans


@pytest.mark.parametrize("speed", SPEEDS)
def test_the_oracles_winner_leads_on_every_frame_of_the_chosen_signals(sig, speed):
    worst = np.inf
    for name, x in sig.items():
        r = time_scale_f64(x, speed)["ratio"][1:]
        assert np.all(r > 1.0), (name, speed, float(r.min()), int(np.argmin(r)) + 1)
        worst = min(worst, float(r.min()))
    print(f"speed {speed}: smallest margin ratio {worst:.3f}")


@pytest.mark.parametrize("speed", SPEEDS)
def test_every_way_of_cutting_the_signal_gives_the_one_shot_result_bit_for_bit(codec, sig, speed):
    num = TS.quantize(speed)[0]
    for name in ("noise", "tone", "run"):
        x = sig[name]
        want_y, want_path = one_shot(codec, sig, name, speed)
        assert np.array_equal(want_path.astype(np.int64), time_scale_f64(x, speed)["path"]), (name, speed)
        for sched, sizes in schedules(len(x), num).items():
            assert sum(sizes) == len(x) and min(sizes) >= 0, (name, sched)
            chunks, paths, plans = stream(codec, x, speed, sizes)
            assert [len(c) for c in chunks] == [p["n_out"] for p in plans], (name, speed, sched)
            assert [len(p) for p in paths] == [p["n_path"] for p in plans], (name, speed, sched)
            assert np.concatenate(paths).tobytes() == want_path.tobytes(), (name, speed, sched)
            assert np.concatenate(chunks).tobytes() == want_y.tobytes(), (name, speed, sched)


@pytest.mark.parametrize("speed", SPEEDS)
def test_short_totals_in_one_final_push(codec, sig, speed):
    for n in (1, 511, 512, 513):
        x = sig[f"n{n}"]
        want_y, want_path = one_shot(codec, sig, f"n{n}", speed)
        assert np.array_equal(want_path.astype(np.int64), time_scale_f64(x, speed)["path"]), (n, speed)
        chunks, paths, plans = stream(codec, x, speed, [n])
        assert len(chunks[0]) == plans[0]["n_out"] == TS.out_len(n, TS.quantize(speed)[0])
        assert chunks[0].tobytes() == want_y.tobytes() and paths[0].tobytes() == want_path.tobytes(), (n, speed)


def test_eight_streams_stepped_together_equal_each_alone(codec, sig):
    jobs = [("noise", 0.5, "hops"), ("tone", 0.77, "edges"), ("run", 0.99, "empties"), ("noise", 1.01, "big"), ("tone", 1.25, "ones"),
            ("run", 1.5, "empty_final"), ("noise", 2.0, "edges"), ("tone", 2.0, "whole")]
    sizes = [schedules(len(sig[n]), TS.quantize(v)[0])[s] for n, v, s in jobs]
    alone = [stream(codec, sig[n], v, sz)[0] for (n, v, _), sz in zip(jobs, sizes)]
    hs = [codec.time_scale_stream_open(v) for _, v, _ in jobs]
    assert len(set(hs)) == 8
    got = [[] for _ in jobs]
    at = [0] * len(jobs)
    try:
        for step in range(max(len(sz) for sz in sizes)):
            live = [i for i, sz in enumerate(sizes) if step < len(sz)]
            parts = [sig[jobs[i][0]][at[i]: at[i] + sizes[i][step]] for i in live]
            starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
            x = torch.from_numpy(np.concatenate(parts + [np.zeros(0, np.float32)])).to(DEV)
            y, off = codec.time_scale_stream_step(x, [(hs[i], int(starts[q]), sizes[i][step], step == len(sizes[i]) - 1) for q, i in enumerate(live)])
            y = y.cpu().numpy()
            for q, i in enumerate(live):
                got[i].append(y[off[q]: off[q + 1]])
                at[i] += sizes[i][step]
    finally:
        for h in hs:
            codec.time_scale_stream_close(h)
    for i, (g, a) in enumerate(zip(got, alone)):
        assert len(g) == len(a) and all(u.tobytes() == v.tobytes() for u, v in zip(g, a)), jobs[i]


def test_a_slot_closed_and_reopened_gives_the_fresh_result(codec, sig):
    x = sig["noise"]
    want = one_shot(codec, sig, "noise", 1.25)[0]
    h = codec.time_scale_stream_open(0.77)
    codec.time_scale_stream_step(torch.from_numpy(x).to(DEV), [(h, 0, 7000, False)])         # leaves a carry and a state behind
    codec.time_scale_stream_close(h)
    h2 = codec.time_scale_stream_open(1.25)
    assert h2 == h                                                                              # the very slot
    codec.time_scale_stream_close(h2)
    chunks, _, _ = stream(codec, x, 1.25, [1, 0, 6000, len(x) - 6001])                        # `stream` reopens it
    assert np.concatenate(chunks).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="not open"):
        codec.time_scale_stream_step(torch.from_numpy(x).to(DEV), [(h, 0, 10, False)])


def test_refusals_leave_the_state_untouched(codec, sig):
    x = sig["noise"]
    xd = torch.from_numpy(x).to(DEV)
    want = one_shot(codec, sig, "noise", 1.5)[0]
    h, other = codec.time_scale_stream_open(1.5), codec.time_scale_stream_open(0.5)
    try:
        first, _ = codec.time_scale_stream_step(xd, [(h, 0, 6000, False)])
        codec.time_scale_stream_step(xd, [(other, 0, 100, True)])                               # `other` has had its last push
        pool = codec._pool("time_scale")
        torch.cuda.synchronize()
        carry, state, rec = pool.buf["carry"].clone(), pool.buf["state"].clone(), dict(pool.records)
        for pushes in ([(h, 0, 100, False), (h, 100, 100, False)], [(h, 19990, 100, False)], [(h, -1, 10, False)], [(h, 0, -1, False)], [],
                       [(h, 6000, 100, False), (other, 0, 10, False)], [(h, 6000, 100, False), (9999, 0, 10, False)]):
            with pytest.raises(ValueError):
                codec.time_scale_stream_step(xd, pushes)
        with pytest.raises(ValueError):
            codec.time_scale_stream_step(xd.cpu(), [(h, 6000, 100, False)])
        # past the host's plan, the library itself: descriptors that disagree with K(n_avail), a slot outside the pool, one slot twice
        p = TS.stream_plan(1.5, 6000, 5000, False)
        good = dict(in_off=6000, n_in=5000, pos=6000, total=-1, out_off=0, path_off=0, k_prev=p["k_prev"], k_now=p["k_now"], slot=h, phase=1,
                    num=150, den=100, n_out=p["n_out"], reserved=0)
        y = torch.full((p["n_out"] + 8,), 7.0, device=DEV)
        path = torch.full((64,), 7, dtype=torch.int32, device=DEV)
        for over in (dict(k_now=p["k_now"] + 1, n_out=p["n_out"] + HOP), dict(k_prev=p["k_prev"] - 1), dict(total=11001), dict(n_out=p["n_out"] - 1),
                     dict(slot=int(pool.buf["carry"].shape[0])), dict(phase=2), dict(num=100), dict(twice=True)):
            tab = np.zeros(2 if over.get("twice") else 1, _lib.TS_STREAM)
            tab[:] = tuple({**good, **over}[k] for k in _lib.TS_STREAM.names)
            tab_d = torch.from_numpy(tab.view(np.uint8)).to(DEV)
            rc = codec.lib.ctts_time_scale_stream_step(xd.data_ptr(), xd.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(tab), y.data_ptr(),
                                                       y.numel(), path.data_ptr(), path.numel(), pool.buf["carry"].data_ptr(), pool.buf["state"].data_ptr(),
                                                       int(pool.buf["carry"].shape[0]), codec._time_scale_window().data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream)
            assert rc != 0 and b"ctts_time_scale_stream_step" in _lib.lib().ctts_last_error(), over
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((path == 7).all())
        assert torch.equal(pool.buf["carry"], carry) and torch.equal(pool.buf["state"], state) and dict(pool.records) == rec
        rest, _ = codec.time_scale_stream_step(xd, [(h, 6000, len(x) - 6000, True)])
        assert np.concatenate([first.cpu().numpy(), rest.cpu().numpy()]).tobytes() == want.tobytes()
    finally:
        codec.time_scale_stream_close(h)
        codec.time_scale_stream_close(other)


def test_the_pool_grows_and_keeps_the_streams_it_holds(codec, sig):
    x = sig["tone"]
    xd = torch.from_numpy(x).to(DEV)
    want = one_shot(codec, sig, "tone", 1.25)[0]
    h = codec.time_scale_stream_open(1.25)
    first, _ = codec.time_scale_stream_step(xd, [(h, 0, 4000, False)])
    n = int(codec._pool("time_scale").buf["carry"].shape[0])
    more = [codec.time_scale_stream_open(0.5) for _ in range(n)]                                # one more than the pool held
    try:
        assert int(codec._pool("time_scale").buf["carry"].shape[0]) == 2 * n and len(set(more + [h])) == n + 1
        rest, _ = codec.time_scale_stream_step(xd, [(h, 4000, len(x) - 4000, True)])
        assert np.concatenate([first.cpu().numpy(), rest.cpu().numpy()]).tobytes() == want.tobytes()
    finally:
        for m in more + [h]:
            codec.time_scale_stream_close(m)
    assert codec.time_scale_streams_in_use() == 0


def test_the_one_shot_call_is_bit_identical_to_the_recorded_one():
    """`timescale_path_k` now calls the search as a device function it shares with the streaming kernel.  The hashes were recorded from
    the library built at the commit before that change, over the segments of test_gpu_timescale.py at its seven speeds."""
    from chattts_amd.engine import CodecEngine
    from tests.test_gpu_timescale import SPEEDS as OLD_SPEEDS, _offsets
    with open(GOLDEN) as fh:
        want = json.load(fh)
    segs = [np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32) for seed in range(5) for n in (1, 300, 512, 1024, 1500, 4096, 12000)]
    segs.append(np.zeros(3000, np.float32))
    run = np.random.default_rng(11).uniform(-1, 1, 9000).astype(np.float32)
    run[3000:6000] = 0.0
    segs.append(run)
    off = _offsets([len(s) for s in segs])
    x = torch.from_numpy(np.concatenate(segs)).to(DEV)
    ts = CodecEngine.__new__(CodecEngine)             # the scaler needs the library and a device, no weights
    ts.lib, ts.device = _lib.lib(), DEV
    for speed in OLD_SPEEDS:
        y, _, path, _ = ts.time_scale(x, speed, offsets=off, return_path=True)
        got = [hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(path.cpu().numpy().tobytes()).hexdigest()]
        assert got == want[str(speed)], speed

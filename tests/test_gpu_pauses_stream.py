"""The pause streams on the device (csrc/pauses.hip pause_stream_*_k, CodecEngine.trim_pauses_stream_*) against the NumPy twin
(`pauses.StreamPauses`, itself pinned to the serial oracle by tests/test_pauses_stream_host.py): the same count in every step, the same
bits in every chunk, the same held frames behind every step, the same record at the end.  The cases of a spec at all five rates run as
concurrent streams, one descriptor each per step, so a launch carries every frame size at once.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import pauses as PA  # noqa: E402
from tests import pauses_stream_cases as SC  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ("whole", "frames", "inside_every_frame", "random", "random+empty")


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(autouse=True)
def no_stream_left_open(codec):
    yield
    assert codec.trim_pauses_streams_in_use() == 0


def jobs_of(cases, kinds=KINDS):
    """(fs, spec, x) -> (fs, spec, x, sizes), the kind of cut rotating over the cases; an empty last size is the empty final push"""
    return [(fs, spec, x, SC.cuts(len(x), fs // 100, kinds[i % len(kinds)], seed=i)) for i, (fs, spec, x) in enumerate(cases)]


def run_streams(codec, jobs, on_step=None):
    """every job a stream, all stepped together: stream j takes part in step k while it has a k-th push.  Every chunk is compared with
    the twin's push as it comes -> the final records"""
    xd = torch.from_numpy(np.concatenate([x for _, _, x, _ in jobs])).to(DEV)
    lo = np.concatenate([[0], np.cumsum([len(x) for _, _, x, _ in jobs])])
    hs = [codec.trim_pauses_stream_open(fs, spec) for fs, spec, _, _ in jobs]
    tw = [PA.StreamPauses(fs, spec) for fs, spec, _, _ in jobs]
    at, recs = [0] * len(jobs), [None] * len(jobs)
    try:
        for k in range(max(len(s) for _, _, _, s in jobs)):
            live = [j for j, job in enumerate(jobs) if k < len(job[3])]
            pushes = [(hs[j], int(lo[j]) + at[j], jobs[j][3][k], k == len(jobs[j][3]) - 1) for j in live]
            if on_step is not None:
                on_step(k, xd, pushes)
            y, off = codec.trim_pauses_stream_step(xd, pushes)
            yh = y.cpu().numpy()
            assert int(off[-1]) == y.numel()
            for i, j in enumerate(live):
                n, fin = jobs[j][3][k], pushes[i][3]
                want = tw[j].push(jobs[j][2][at[j]: at[j] + n], fin)
                got = yh[off[i]: off[i + 1]]
                assert len(got) == len(want), (j, k, jobs[j][0], len(got), len(want))
                assert got.tobytes() == want.tobytes(), (j, k, jobs[j][0])
                at[j] += n
                st = codec.trim_pauses_stream_stats(hs[j])
                assert (st["pushed"], st["held"], st["emitted"], st["done"]) == (tw[j].pushed, tw[j].held, int(tw[j].record[7]), fin)
                if fin:
                    recs[j] = st["record"]
                    one_shot = list(PA.apply(jobs[j][2], jobs[j][0], jobs[j][1])[1]) if len(jobs[j][2]) else [0] * 8
                    assert list(st["record"]) == list(tw[j].record) == one_shot, (j, k)
    finally:
        for h in hs:
            codec.trim_pauses_stream_close(h)
    assert all(r is not None for r in recs)
    return recs


@pytest.mark.parametrize("name", list(SC.SPECS))
def test_the_edge_cases_at_every_rate_in_one_launch(codec, name):
    """80 streams of five frame sizes (F = 110 and 220 among them) and every kind of cut, a push of 0 here and there, stepped together"""
    cases = [(fs, SC.SPECS[name], x) for fs in SC.RATES for _, x in SC.edge_cases(fs, name)]
    recs = run_streams(codec, jobs_of(cases))
    assert any(r[5] > 0 for r in recs) and any(r[3] > 0 for r in recs) and any(r[4] > 0 for r in recs)      # shortened runs, lead and tail removed


def test_streams_of_different_specs_in_one_launch_and_one_that_stands_still(codec):
    rng = np.random.default_rng(7)
    cases = []
    for i, name in enumerate(SC.SPECS):
        fs = SC.RATES[i % len(SC.RATES)]
        P, lead, tail, pad = SC.frames_of(SC.SPECS[name])
        act = SC.runs((lead + 3, 0), (2, 1), (P + 2 * pad + 4, 0), (1, 1), (pad + 1, 0), (1, 1), (tail + pad + 2, 0))
        cases.append((fs, SC.SPECS[name], SC.signal(fs, act, len(act) * (fs // 100) - int(rng.integers(0, 50)), seed=i)))
    jobs = jobs_of(cases, ("random", "inside_every_frame"))
    fs, spec, x, _ = jobs[0]
    jobs[0] = (fs, spec, x, [700, 0, 0, 0, 0, 0, 0, 0, len(x) - 700])             # n_in = 0 for step after step while the others advance
    run_streams(codec, jobs)


def test_one_push_per_sample(codec):
    x = SC.signal(8000, SC.runs((1, 0), (1, 1), (2, 0)), 4 * 80 - 30)
    run_streams(codec, [(8000, SC.SPECS["bare"], x, [1] * len(x)), (11025, SC.SPECS["tail0"], SC.signal(11025, [0, 1, 0], 300, seed=2), [1] * 300)])


def test_an_empty_stream_and_a_stream_of_one_sample(codec):
    z = np.zeros(0, np.float32)
    recs = run_streams(codec, [(24000, True, z, [0, 0]), (24000, True, np.array([0.5], np.float32), [0, 1, 0]), (22050, True, z, [0])])
    assert list(recs[0]) == [0] * 8 and list(recs[1]) == [1, 1, 1, 0, 0, 0, 0, 1] and list(recs[2]) == [0] * 8


def test_a_pause_ten_times_the_capacity(codec):
    fs = 8000
    x = np.concatenate([SC.signal(fs, [0, 1, 1]), np.zeros(30 * fs, np.float32), SC.signal(fs, [1, 0, 0], seed=1)])
    sizes = [4000] * (len(x) // 4000) + [len(x) % 4000]
    held = []
    recs = run_streams(codec, [(fs, True, x, sizes), (fs, True, np.zeros(30 * fs, np.float32), [4000] * 60)],
                       on_step=lambda k, xd, pushes: held.append(max(codec.trim_pauses_stream_stats(h)["held"] for h, _, _, _ in pushes)))
    assert recs[0][5] == 1 and recs[0][6] == 3000 - 2 * 3 - 40 and recs[1][7] == 15 * 80
    assert max(held) == PA.stream_need(True) == 34


def test_a_slot_is_clean_when_it_is_used_again(codec):
    fs, F = 22050, 220
    a = SC.signal(fs, SC.runs((3, 1), (60, 0)), seed=1)
    h = codec.trim_pauses_stream_open(fs, True)
    codec.trim_pauses_stream_step(torch.from_numpy(a).to(DEV), [(h, 0, len(a), False)])          # abandoned half way: frames held, a record begun
    assert codec.trim_pauses_stream_stats(h)["held"] > 0
    codec.trim_pauses_stream_close(h)
    b = SC.signal(48000, SC.runs((9, 0), (1, 1), (70, 0), (2, 1)), seed=2)
    again = codec.trim_pauses_stream_open(48000, SC.SPECS["odd"])
    codec.trim_pauses_stream_close(again)
    assert again == h                                                                            # the slot just given back is the next one taken
    run_streams(codec, [(48000, SC.SPECS["odd"], b, SC.cuts(len(b), 480, "random", seed=3))])


def test_a_handle_given_twice_is_refused_and_every_stream_goes_on_as_it_was(codec):
    def twice(k, xd, pushes):
        if k in (1, 3):
            state = codec._pool("pauses").buf["state"].clone()
            recs = {h: {k: v for k, v in codec.trim_pauses_stream_stats(h).items() if k != "record"} for h, _, _, _ in pushes}
            with pytest.raises(ValueError, match="twice"):
                codec.trim_pauses_stream_step(xd, [*pushes, pushes[0]])
            with pytest.raises(ValueError, match="outside the tensor"):
                codec.trim_pauses_stream_step(xd, [(pushes[0][0], xd.numel(), 1, False)])
            assert torch.equal(state, codec._pool("pauses").buf["state"]) and recs == {h: {k: v for k, v in codec.trim_pauses_stream_stats(h).items() if k != "record"} for h, _, _, _ in pushes}
    cases = [(fs, SC.DEFAULT, SC.signal(fs, SC.runs((6, 0), (2, 1), (70, 0), (1, 1), (20, 0)), seed=fs)) for fs in (11025, 24000)]
    run_streams(codec, [(fs, sp, x, [len(x) // 5] * 4 + [len(x) - 4 * (len(x) // 5)]) for fs, sp, x in cases], on_step=twice)


def test_the_pool_grows_under_a_live_stream_and_keeps_its_state():
    """a pool of 4 slots doubles while a stream holds frames and a record half way: the stream goes on bit for bit"""
    from chattts_amd import _lib
    from chattts_amd.engine import CodecEngine

    class Small(CodecEngine):
        PA_STREAM_SLOTS = 4

    eng = Small.__new__(Small)                          # pause control needs the library and a device, no weights
    eng.lib, eng.device = _lib.lib(), DEV
    tone = (0.5 * np.sin(2 * np.pi * 440 / 8000 * np.arange(1250))).astype(np.float32)
    xd = torch.from_numpy(np.concatenate([tone, np.zeros(1500, np.float32), tone])).to(DEV)
    want, record = eng.trim_pauses(xd, True, rates=8000, return_stats=True)
    h = eng.trim_pauses_stream_open(8000)
    first, _ = eng.trim_pauses_stream_step(xd, [(h, 0, 2000, False)])
    assert eng._pool("pauses").slots == 4
    more = [eng.trim_pauses_stream_open(8000) for _ in range(4)]
    pool = eng._pool("pauses")
    assert pool.slots == 8 and int(pool.buf["carry"].shape[0]) == int(pool.buf["state"].shape[0]) == 8 and max(more) >= 4
    rest, _ = eng.trim_pauses_stream_step(xd, [(h, 2000, 2000, True)])
    assert np.concatenate([first.cpu().numpy(), rest.cpu().numpy()]).tobytes() == want.cpu().numpy().tobytes()
    assert list(eng.trim_pauses_stream_stats(h)["record"]) == list(record[0])
    for m in more + [h]:
        eng.trim_pauses_stream_close(m)
    assert eng.trim_pauses_streams_in_use() == 0

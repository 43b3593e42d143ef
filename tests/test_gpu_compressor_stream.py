"""The compressor of streams (csrc/compressor.hip compress_stream_*_k, CodecEngine.compress_stream_*) against the one-shot compressor of
the whole signal (`CodecEngine.compress`, itself pinned to the twin by tests/test_gpu_compressor.py) and against the NumPy twin, bit for
bit in samples and in the final record, under every way of cutting a signal into pushes (tests/compressor_stream_cases.py).  All
segments of tests/compressor_cases.py at one rate run as concurrent streams, one descriptor each per step, so a cut costs a handful of
launches.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, compressor as CP  # noqa: E402
from tests import compressor_cases as CC, compressor_stream_cases as SC  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = np.float32(-7.25)


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


@pytest.fixture(autouse=True)
def no_stream_left_open(codec):
    yield
    assert codec.compress_streams_in_use() == 0


_PACK = {}


def pack(codec, fs):
    """the segments of a rate packed on the device, and `compress` of each as if alone: computed once per rate, left unchanged"""
    if fs not in _PACK:
        cs = CC.cases(fs)
        off = CC.offsets([len(x) for _, x, _ in cs])
        xd = torch.from_numpy(np.concatenate([x for _, x, _ in cs])).to(DEV)
        y, stats = codec.compress(xd, [s for _, _, s in cs], offsets=off, rates=fs, return_stats=True)
        _PACK[fs] = (xd, off, y.cpu().numpy(), stats)
    return _PACK[fs]


def run_streams(codec, xd, jobs, handles=None):
    """jobs: [(fs, spec, in_lo, sizes)], each a stream over xd[in_lo ..] pushed in `sizes` (the last one final); stream j takes part in
    step k while it has a k-th push -> (per stream its chunks, per stream its final record).  Chunk lengths are checked against _plan."""
    hs = [codec.compress_stream_open(fs, spec) for fs, spec, _, _ in jobs] if handles is None else handles
    chunks, at, recs = [[] for _ in jobs], [lo for _, _, lo, _ in jobs], [None] * len(jobs)
    try:
        for k in range(max(len(s) for _, _, _, s in jobs)):
            live = [j for j, job in enumerate(jobs) if k < len(job[3])]
            pushes = [(hs[j], at[j], jobs[j][3][k], k == len(jobs[j][3]) - 1) for j in live]
            want = [codec.compress_stream_plan(h, n, fin)["n_out"] for h, _, n, fin in pushes]
            y, off = codec.compress_stream_step(xd, pushes)
            assert [int(v) for v in np.diff(off)] == want and int(off[-1]) == y.numel()
            yh = y.cpu().numpy()
            for i, j in enumerate(live):
                chunks[j].append(yh[off[i]: off[i + 1]])
                at[j] += jobs[j][3][k]
                if pushes[i][3]:
                    recs[j] = codec.compress_stream_stats(hs[j])
    finally:
        if handles is None:
            for h in hs:
                codec.compress_stream_close(h)
    return chunks, recs


def same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit, NaNs included"""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("cut", SC.CUT_NAMES)
@pytest.mark.parametrize("fs", SC.RATES)
def test_every_cut_returns_the_one_shot_compressors_bits_and_record(codec, fs, cut):
    xd, off, y_one, st_one = pack(codec, fs)
    before = xd.clone()
    cs = CC.cases(fs)
    jobs = [(fs, spec, int(off[i]), dict(SC.case_cuts(fs, x, spec))[cut]) for i, (_, x, spec) in enumerate(cs)]
    pool = codec._pool("compress")
    hs = [codec.compress_stream_open(fs, spec) for _, _, spec in cs]
    try:
        pool.buf["carry"].fill_(float(CANARY))                                           # a fresh stream reads neither: whatever lies there
        pool.buf["hist"].fill_(float(CANARY))
        chunks, recs = run_streams(codec, xd, jobs, hs)
    finally:
        for h in hs:
            codec.compress_stream_close(h)
    assert same_bits(xd, before)                                                       # the input is never written
    carry, hist = pool.buf["carry"].cpu().numpy(), pool.buf["hist"].cpu().numpy()
    idle = [s for s in range(pool.slots) if s not in set(hs)]
    assert np.all(carry[idle] == CANARY) and np.all(hist[idle] == CANARY)                # canaries around the slots' buffers: the other slots ..
    assert np.all(carry[hs][:, :, CP.STREAM_CARRY:] == CANARY) and np.all(hist[hs][:, :, CP.STREAM_HIST:] == CANARY)   # .. and each half's end
    for i, ((name, x, spec), (y_twin, rec_twin)) in enumerate(zip(cs, CC.twin(fs))):
        got = np.concatenate(chunks[i])
        assert same(got, y_one[off[i]: off[i + 1]]), (fs, cut, name)
        assert same(got, y_twin), (fs, cut, name)
        assert recs[i].tobytes() == st_one[i].tobytes() == rec_twin.tobytes(), (fs, cut, name, recs[i], st_one[i])
        assert [len(c) for c in chunks[i]] == SC.run_twin(fs, x, spec, jobs[i][3])[4], (fs, cut, name)          # the lag law
    assert any(r["n_touched"] > 0 for r in recs) and any(r["n_blocks"] == 0 for r in recs)


@pytest.mark.parametrize("fs", (8000, 48000))
def test_totals_under_the_lag_emit_only_at_the_end(codec, fs):
    cs = SC.totals_under_lag(fs)
    xd = torch.from_numpy(np.concatenate([x for _, x, _, _ in cs])).to(DEV)
    off = CC.offsets([len(x) for _, x, _, _ in cs])
    chunks, recs = run_streams(codec, xd, [(fs, spec, int(off[i]), cut) for i, (_, _, spec, cut) in enumerate(cs)])
    for i, (name, x, spec, cut) in enumerate(cs):
        y, rec = CP.compress_segment(x, fs, spec)
        assert [len(c) for c in chunks[i]] == [0] * (len(cut) - 1) + [len(x)]
        assert same(chunks[i][-1], y) and recs[i].tobytes() == rec.tobytes(), name


@pytest.mark.parametrize("fs", (8000, 48000))
def test_one_loud_block_at_a_push_boundary(codec, fs):
    """one loud block around the push boundary b: the block that ends at b, the one that starts there, the one A + 1 blocks before b
    (the emission edge) and the one A + H + 1 blocks before it (the last whose hold still reaches), each alone and all together.  The
    twin's gain is below 1 on both sides of b, so the streams cannot agree with the compressor idle there."""
    spec = {"attack_ms": 3, "hold_ms": 40}
    B, (A, H) = fs // 1000, CP.blocks(CP.check(spec))
    nbk = A + H + 1 + 2 * CC.TILE
    b, n = (A + H + 3 + CC.TILE) * B, nbk * B + 2 * CC.TILE * B + 5
    base = np.float32(0.01) * CC.enveloped(21, n, B)
    at = [b // B - 1, b // B, b // B - (A + 1), b // B - (A + H + 1)]
    sigs = []
    for blk in at:
        x = base.copy()
        x[blk * B + B // 2] = 0.8
        sigs.append(x)
    both = base.copy()
    both[[blk * B + 1 for blk in at]] = [0.8, -0.6, 0.7, -0.9]
    sigs.append(both)
    for x in sigs:
        g = CP.gain_curve(x, fs, spec)["g"]
        assert g[b - 1] < 1 and g[b] < 1, "the twin's gain is below 1 on both sides of the push boundary"
    xd = torch.from_numpy(np.concatenate(sigs)).to(DEV)
    jobs = [(fs, spec, i * n, [b, n - b]) for i in range(len(sigs))] + \
           [(fs, spec, i * n, [b - (A + 1) * B, (A + 1) * B, (A + 1) * B, n - b - (A + 1) * B]) for i in range(len(sigs))]
    chunks, recs = run_streams(codec, xd, jobs)
    for j, (chs, rec) in enumerate(zip(chunks, recs)):
        y, want = CP.compress_segment(sigs[j % len(sigs)], fs, spec)
        assert same(np.concatenate(chs), y) and rec.tobytes() == want.tobytes() and rec["n_touched"] > 0, j


def test_a_hold_of_500_ms_is_read_across_pushes_of_100_ms(codec):
    fs, spec = 24000, {"attack_ms": 2, "hold_ms": 500, "knee_db": 0}
    B, n = 24, 24 * 1000
    x = np.float32(0.01) * CC.enveloped(31, n, B)
    x[150 * B + 7] = 0.9                                                                 # one loud block in the second push
    xd = torch.from_numpy(x).to(DEV)
    g = CP.gain_curve(x, fs, spec)["g"]
    held = [k for k in range(10) if np.any(g[k * 100 * B: (k + 1) * 100 * B] < 1)]
    assert len(held) >= 6                                                                # the dip lives in the history for five steps and more
    chunks, recs = run_streams(codec, xd, [(fs, spec, 0, [100 * B] * 10)])
    y, want = CP.compress_segment(x, fs, spec)
    assert same(np.concatenate(chunks[0]), y) and recs[0].tobytes() == want.tobytes() and want["n_blocks"] == 1
    assert sum(bool(np.any(c != x[sum(map(len, chunks[0][:k])): sum(map(len, chunks[0][:k + 1]))])) for k, c in enumerate(chunks[0])) >= 6


def test_eight_streams_of_mixed_rates_and_specs_in_one_step_equal_each_alone(codec):
    n = 9000
    specs = [(8000, True), (48000, CC.SPECS[1]), (24000, CC.SPECS[2]), (22050, CC.SPECS[3]), (16000, CC.SPECS[4]), (44100, True),
             (8000, CC.SPECS[4]), (32000, {"attack_ms": 7, "hold_ms": 33})]
    sigs = [CC.enveloped(40 + j, n, fs // 1000) for j, (fs, _) in enumerate(specs)]
    xd = torch.from_numpy(np.concatenate(sigs)).to(DEV)
    sizes = [[100 + 371 * j, 2048 + 13 * j, 0, 3000 - 200 * j] for j in range(len(specs))]           # unequal positions at every step
    jobs = [(fs, sp, j * n, s + [n - sum(s)]) for j, ((fs, sp), s) in enumerate(zip(specs, sizes))]
    together, recs = run_streams(codec, xd, jobs)
    for j, job in enumerate(jobs):
        alone, rec = run_streams(codec, xd, [job])
        y, want = CP.compress_segment(sigs[j], job[0], job[1])
        assert [c.tobytes() for c in together[j]] == [c.tobytes() for c in alone[0]], j
        assert same(np.concatenate(together[j]), y) and recs[j].tobytes() == rec[0].tobytes() == want.tobytes(), j
    assert sum(r["n_blocks"] > 0 for r in recs) >= 4


def test_a_slot_abandoned_mid_hold_is_reused_clean_and_the_pool_grows_under_a_live_stream(codec):
    fs, n, spec = 16000, 6000, {"attack_ms": 2, "hold_ms": 300}
    loud = CC.enveloped(51, n, 16)
    loud[40 * 16 + 3] = 0.95
    quiet = (np.float32(0.01) * CC.enveloped(52, n, 16)).astype(np.float32)
    xd = torch.from_numpy(np.concatenate([loud, quiet])).to(DEV)
    h = codec.compress_stream_open(fs, spec)
    codec.compress_stream_step(xd, [(h, 0, 1600, False)])                                 # 100 ms in: the hold of the loud block is live
    assert codec.compress_stream_stats(h)["n_blocks"] > 0
    codec.compress_stream_close(h)                                                        # abandoned mid-hold
    h2 = codec.compress_stream_open(fs, spec)
    assert h2 == h                                                                        # the slot just given back
    fresh = codec.compress_stream_stats(h2)
    assert (fresh["min_gain"], fresh["n_blocks"], fresh["n_touched"], fresh["peak"]) == (1.0, 0, 0, 0.0)
    y1, _ = codec.compress_stream_step(xd, [(h2, n, 1000, False)])                        # a quiet stream in the loud one's slot
    pool = codec._pool("compress")
    first = int(pool.buf["carry"].shape[0])
    more = [codec.compress_stream_open(fs, spec) for _ in range(first)]                   # every slot taken: the pool doubles under the open stream
    try:
        assert int(codec._pool("compress").buf["carry"].shape[0]) == 2 * first == int(pool.buf["hist"].shape[0]) == int(pool.buf["stats"].shape[0])
        assert max(more) >= first and codec.compress_streams_in_use() == first + 1
        y2, _ = codec.compress_stream_step(xd, [(h2, n + 1000, n - 1000, True), (max(more), 0, n, True)])
        want_q, rec_q = CP.compress_segment(quiet, fs, spec)
        want_l, rec_l = CP.compress_segment(loud, fs, spec)
        got = torch.cat([y1, y2[: n - y1.numel()]]).cpu().numpy()
        assert same(got, want_q) and same(got, quiet) and same(y2[n - y1.numel():].cpu().numpy(), want_l)
        assert codec.compress_stream_stats(h2).tobytes() == rec_q.tobytes() and rec_q["n_blocks"] == 0
        assert codec.compress_stream_stats(max(more)).tobytes() == rec_l.tobytes() and rec_l["n_touched"] > 0
    finally:
        for s in more + [h2]:
            codec.compress_stream_close(s)


def test_nan_and_inf_pass_as_in_the_one_shot_call(codec):
    fs = 24000
    cs = [c for c in CC.cases(fs) if c[0] in ("nan", "inf")]
    assert len(cs) == 2
    xd = torch.from_numpy(np.concatenate([x for _, x, _ in cs])).to(DEV)
    off = CC.offsets([len(x) for _, x, _ in cs])
    jobs = [(fs, spec, int(off[i]), SC._fit(len(x), [5, 24 * 5 + 1, 24 * 2, 24 * CC.TILE - 24 * 7 - 6, 1])) for i, (_, x, spec) in enumerate(cs)]
    chunks, recs = run_streams(codec, xd, jobs)
    for i, (name, x, spec) in enumerate(cs):
        y, rec = CP.compress_segment(x, fs, spec)
        got = np.concatenate(chunks[i])
        assert same(got, y) and recs[i].tobytes() == rec.tobytes(), name
        assert np.array_equal(np.isnan(got), np.isnan(x)) or name == "inf"


def test_out_and_out_off_place_the_chunks(codec):
    fs, n = 24000, 5000
    x = CC.enveloped(61, 2 * n, 24)
    xd = torch.from_numpy(x).to(DEV)
    a, b = codec.compress_stream_open(fs, True), codec.compress_stream_open(fs, CC.SPECS[1])
    try:
        out = torch.full((2 * n + 64,), float(CANARY), dtype=torch.float32, device=DEV)
        na = codec.compress_stream_plan(a, 3000, False)["n_out"]
        nb = codec.compress_stream_plan(b, n, True)["n_out"]
        got, off = codec.compress_stream_step(xd, [(a, 0, 3000, False), (b, n, n, True)], out=out, out_off=[n + 40, 8])
        assert got is out and list(off) == [n + 40, 8] and nb == n
        got2, _ = codec.compress_stream_step(xd, [(a, 3000, n - 3000, True)], out=out, out_off=[n + 40 + na])
        oh = out.cpu().numpy()
        ya, _ = CP.compress_segment(x[:n], fs, True)
        yb, _ = CP.compress_segment(x[n:], fs, CC.SPECS[1])
        assert same(oh[n + 40: 2 * n + 40], ya) and same(oh[8: 8 + n], yb)
        assert np.all(oh[:8] == CANARY) and np.all(oh[8 + n: n + 40] == CANARY) and np.all(oh[2 * n + 40:] == CANARY)
        with pytest.raises(ValueError, match="outside `out`"):
            codec.compress_stream_step(xd, [(codec.compress_stream_open(fs, True), 0, n, True)], out=out[:100], out_off=[0])
    finally:
        for h in list(codec._pool("compress").records):
            codec.compress_stream_close(h)


def _raw_step(codec, xd, pushes, y, mutate=None, tabs_mutate=None, n_slots=None):
    """ctts_compress_stream_step on the engine's pool with a caller-owned y; the host records are not committed"""
    tab, tabs_h, _, n_new = codec._cp_descriptors(pushes)
    o = np.zeros(len(pushes) + 1, np.int64)
    np.cumsum(tab["n_out"], out=o[1:])
    tab["out_off"] = o[:-1] + 16
    tabs_h = tabs_h.copy()
    if mutate:
        mutate(tab)
    if tabs_mutate:
        tabs_mutate(tabs_h)
    pool = codec._pool("compress")
    up = torch.from_numpy(np.concatenate([tabs_h.view(np.uint8).reshape(-1), tab.view(np.uint8)])).to(DEV)
    sb = int(codec.lib.ctts_compress_stream_scratch_bytes(n_new))
    work = torch.empty((sb,), dtype=torch.uint8, device=DEV)
    rc = codec.lib.ctts_compress_stream_step(xd.data_ptr(), xd.numel(), up.data_ptr() + tabs_h.nbytes, tab.ctypes.data_as(C.c_void_p), len(tab),
                                             up.data_ptr(), tabs_h.ctypes.data_as(C.c_void_p), int(tabs_h.shape[0]), y.data_ptr(), y.numel(),
                                             pool.buf["carry"].data_ptr(), pool.buf["hist"].data_ptr(), pool.buf["stats"].data_ptr(),
                                             pool.slots if n_slots is None else n_slots, work.data_ptr(), sb, None)
    torch.cuda.synchronize()
    return rc, o


def test_canaries_around_the_output_stay_and_the_input_is_unwritten(codec):
    fs = 24000
    xd, off, y_one, _ = pack(codec, fs)
    cs = CC.cases(fs)
    before = xd.clone()
    hs = [codec.compress_stream_open(fs, spec) for _, _, spec in cs]
    try:
        pushes = [(h, int(off[i]), len(cs[i][1]), True) for i, h in enumerate(hs)]
        y = torch.full((xd.numel() + 32,), float(CANARY), dtype=torch.float32, device=DEV)
        rc, o = _raw_step(codec, xd, pushes, y)
        assert rc == 0 and int(o[-1]) == xd.numel()
        yh = y.cpu().numpy()
        assert np.all(yh[:16] == CANARY) and np.all(yh[-16:] == CANARY) and same(yh[16:-16], y_one)
        assert same_bits(xd, before)
    finally:
        for h in hs:
            codec.compress_stream_close(h)


def test_a_refused_step_leaves_the_output_the_records_and_the_slots_as_they_were(codec):
    fs, n = 22050, 6000
    x = CC.enveloped(71, n, 22)
    xd = torch.from_numpy(x).to(DEV)
    a, b = codec.compress_stream_open(fs, True), codec.compress_stream_open(fs, CC.SPECS[3])
    try:
        ya, oa = codec.compress_stream_step(xd, [(a, 0, 2500, False), (b, 0, 100, False)])
        ya = ya[: int(oa[1])]                                                             # a's chunk; b's lies behind it
        pool = codec._pool("compress")
        recs = dict(pool.records)
        state = {k: v.clone() for k, v in pool.buf.items()}
        with pytest.raises(ValueError, match="outside the tensor"):                       # the engine's own check, behind a good push
            codec.compress_stream_step(xd, [(a, 2500, 100, False), (b, n - 10, 11, False)])
        with pytest.raises(ValueError, match="twice"):
            codec.compress_stream_step(xd, [(a, 2500, 100, False), (a, 2600, 100, False)])
        y = torch.full((n + 32,), float(CANARY), dtype=torch.float32, device=DEV)
        good = [(a, 2500, 3500, True), (b, 100, 900, False)]
        set1 = lambda k, v: (lambda t: t[k].__setitem__(1, v))
        for kw, why in [(dict(mutate=set1("A", 0)), "attack"), (dict(mutate=set1("A", 21)), "attack"), (dict(mutate=set1("H", -1)), "hold"),
                        (dict(mutate=set1("H", 501)), "hold"), (dict(mutate=set1("rate", 22055)), "rate"), (dict(mutate=set1("rate", 7990)), "rate"),
                        (dict(tabs_mutate=lambda t: t[1].__setitem__(700, np.float32(2.0 ** -19))), "entry 700"),
                        (dict(tabs_mutate=lambda t: t[0].__setitem__(3, np.float32(1.5))), "entry 3"),
                        (dict(tabs_mutate=lambda t: t[0].__setitem__(3, np.float32(np.nan))), "entry 3"),
                        (dict(mutate=set1("slot", 1 << 20)), "outside the pool"), (dict(n_slots=1), "outside the pool"),
                        (dict(mutate=set1("tab", 2)), "gain table"), (dict(mutate=set1("c_in", 7)), "samples in"),
                        (dict(mutate=set1("c_out", 0)), "samples in"), (dict(mutate=set1("h_in", 1)), "block gains"),
                        (dict(mutate=set1("h_out", 600)), "block gains"), (dict(mutate=set1("n_out", 5)), "emits"),
                        (dict(mutate=set1("e_lo", 22)), "have emitted"), (dict(mutate=set1("cb_off", 0)), "scratch"),
                        (dict(mutate=set1("phase", 2)), "phase"), (dict(mutate=set1("total", 5)), "last push"),
                        (dict(mutate=set1("in_off", n)), "outside the input"), (dict(mutate=set1("out_off", n)), "outside the output")]:
            rc, _ = _raw_step(codec, xd, good, y, **kw)                                    # the library's, on its second descriptor
            assert rc != 0 and why in codec.lib.ctts_last_error().decode(), (why, codec.lib.ctts_last_error().decode())
        many = [(a, 0, 0, False)] * 1025
        tab = np.zeros(1025, _lib.CP_STREAM)
        rc = codec.lib.ctts_compress_stream_step(xd.data_ptr(), n, xd.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(many), xd.data_ptr(),
                                                 tab.ctypes.data_as(C.c_void_p), 1, y.data_ptr(), y.numel(), pool.buf["carry"].data_ptr(),
                                                 pool.buf["hist"].data_ptr(), pool.buf["stats"].data_ptr(), pool.slots, xd.data_ptr(), 64, None)
        assert rc != 0 and "1024" in codec.lib.ctts_last_error().decode()
        with pytest.raises(ValueError, match="at most 1024"):
            codec.compress_stream_step(xd, many)
        torch.cuda.synchronize()
        assert dict(pool.records) == recs
        assert all(same_bits(pool.buf[k], v) for k, v in state.items()) and bool((y == float(CANARY)).all())      # (a slot may hold an earlier test's NaNs)
        yb, _ = codec.compress_stream_step(xd, [(a, 2500, n - 2500, True)])               # the stream goes on as if nothing had been asked
        want, rec = CP.compress_segment(x, fs, True)
        assert same(torch.cat([ya, yb]).cpu().numpy(), want)
        assert codec.compress_stream_stats(a).tobytes() == rec.tobytes()
    finally:
        codec.compress_stream_close(a)
        codec.compress_stream_close(b)

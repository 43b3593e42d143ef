"""ctts_adpcm_stream_step on the GPU against the NumPy twin (adpcm.StreamEncoder), byte for byte and push by push: the cuts of
tests/adpcm_stream_cases.py with three rates in one step, final pushes shortened by a device count and compacted by a keep mask, junk
between the pushes and in the staging tail, slot reuse, a doubling pool, refusals, and the number of copies to the host.
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, adpcm, engine as E  # noqa: E402
from tests import adpcm_stream_cases as SC  # noqa: E402

DEV = torch.device("cuda:0")


class _Codec:
    """the members `CodecEngine.adpcm_stream_step` uses, without the decoder's weights; `to_host` counts its calls"""
    ADPCM_STREAM_SLOTS = 4                       # small, so that the tests also double the pool
    ADPCM_CARRY = E.CodecEngine.ADPCM_CARRY
    _adpcm_pool = E.CodecEngine._adpcm_pool
    _adpcm_rec = E.CodecEngine._adpcm_rec
    adpcm_stream_open = E.CodecEngine.adpcm_stream_open
    adpcm_stream_close = E.CodecEngine.adpcm_stream_close
    adpcm_streams_in_use = E.CodecEngine.adpcm_streams_in_use
    adpcm_stream_plan = E.CodecEngine.adpcm_stream_plan
    adpcm_stream_step = E.CodecEngine.adpcm_stream_step
    _copy_out = E.CodecEngine._copy_out

    def __init__(self):
        self.lib, self.device, self.copies = _lib.lib(), DEV, 0

    def to_host(self, t):
        self.copies += 1
        return E.CodecEngine.to_host(self, t)


@pytest.fixture(scope="module")
def codec():
    return _Codec()


def _run(codec, streams, together=True):
    """streams: [(rate, [(samples, final, keep or None, count or None)])] -> per stream the chunk of every push.  Round r steps the r-th
    push of every stream that has one, in ONE call (`together`) or one call per stream.  The samples of a round lie in one int16
    buffer, each push on a multiple of 8 and with junk behind it; the keep flags lie in a bit mask over that buffer."""
    handles = [codec.adpcm_stream_open(rate) for rate, _ in streams]
    out = [[] for _ in streams]
    try:
        for r in range(max(len(p) for _, p in streams)):
            due = [i for i, (_, p) in enumerate(streams) if r < len(p)]
            pcm = np.full(sum((len(streams[i][1][r][0]) + 7) // 8 * 8 + 8 for i in due) + 8, 12345, np.int16)
            keep = np.ones(len(pcm), bool)
            counts, rows, at = [], [], 8
            for i in due:
                x, final, mask, count = streams[i][1][r]
                pcm[at: at + len(x)] = x
                if mask is not None:
                    keep[at: at + len(x)] = mask
                ci = None
                if count is not None:
                    ci = len(counts)
                    counts.append(count)
                rows.append((handles[i], at, len(x), final, ci, mask is not None))
                at += (len(x) + 7) // 8 * 8 + 8
            pcm_d = torch.from_numpy(pcm).to(DEV)
            mask_d = torch.from_numpy(np.packbits(keep)).to(DEV)
            counts_d = torch.tensor(counts or [0], dtype=torch.int64, device=DEV)
            by_device = any(row[4] is not None or row[5] for row in rows)
            before = codec.copies
            got = codec.adpcm_stream_step(pcm_d, rows, counts_d, mask_d) if together else \
                [codec.adpcm_stream_step(pcm_d, [row], counts_d, mask_d)[0] for row in rows]
            if together and not by_device:
                assert codec.copies - before <= 1                               # the sizes are known on the host: the blocks, once
            for i, g in zip(due, got):
                assert g.dtype == np.uint8
                out[i].append(g.tobytes())
    finally:
        for h in handles:
            codec.adpcm_stream_close(h)
    return out


def _twin(rate, pushes):
    enc = adpcm.StreamEncoder(rate)
    out = []
    for x, final, mask, count in pushes:
        x = np.asarray(x, np.int16)
        n = len(x) if count is None else max(0, min(count, len(x)))        # a count comes in front of the mask
        keep = np.ones(n, bool) if mask is None else np.asarray(mask, bool)[:n]
        out.append(enc.push(x[:n][keep], final).tobytes())
    return out


@pytest.mark.parametrize("name", SC.SIGNALS)
def test_device_chunks_are_the_twins_push_by_push(codec, name):
    """every cut at every rate as one stream -- 30 streams, so the pool of 4 doubles three times; the r-th pushes of all of them share
    one step, which puts three rates into one launch"""
    streams, want = [], []
    for rate in SC.RATES:
        x = SC.signal(name, rate)
        for cut, lens in SC.cuts(rate).items():
            streams.append((rate, [(x[lo:hi], final, None, None) for lo, hi, final in SC.pushes(lens)]))
            want.append([c.tobytes() for c in SC.reference(name, rate, cut)])
    got = _run(codec, streams)
    for (rate, pushes), g, w in zip(streams, got, want):
        assert [len(c) for c in g] == [len(c) for c in w], (rate, [len(p[0]) for p in pushes])
        assert g == w, (rate, [len(p[0]) for p in pushes])
        assert all(len(c) <= adpcm.stream_bound(len(p[0]), rate) for c, p in zip(g, pushes))
    assert codec.adpcm_streams_in_use() == 0
    if name == "noise":                                                         # the same pushes, one call per stream: the same bytes
        few = [s for s in streams if len(s[1]) in (3, 4, 10)]
        assert _run(codec, few, together=False) == [w for s, w in zip(streams, want) if len(s[1]) in (3, 4, 10)]
        assert codec.adpcm_streams_in_use() == 0


def test_one_copy_to_the_host_when_the_host_knows_the_sizes(codec):
    x = SC.signal("noise", 8000)
    pcm_d = torch.from_numpy(x[:2048].copy()).to(DEV)
    a, b = codec.adpcm_stream_open(8000), codec.adpcm_stream_open(24000)
    try:
        ta, tb = adpcm.StreamEncoder(8000), adpcm.StreamEncoder(24000)
        before = codec.copies
        got = codec.adpcm_stream_step(pcm_d, [(a, 0, 600, False), (b, 608, 1100, False)])
        assert codec.copies == before + 1
        assert [g.tobytes() for g in got] == [ta.push(x[:600]).tobytes(), tb.push(x[608:1708]).tobytes()] and all(g.size for g in got)
        assert codec.adpcm_stream_plan(b, 1017, False) == dict(rate=24000, blocks=1, carry=83, bound=2 * 512)
        assert codec.adpcm_stream_plan(a, 0, True) == dict(rate=8000, blocks=1, carry=0, bound=256)
        before = codec.copies
        got = codec.adpcm_stream_step(pcm_d, [(a, 0, 10, False), (b, 16, 0, False)])     # samples go to a slot, no block: no copy
        assert codec.copies == before and [g.size for g in got] == [0, 0]
        ta.push(x[:10])
        before = codec.copies
        counts = torch.tensor([7], dtype=torch.int64, device=DEV)
        got = codec.adpcm_stream_step(pcm_d, [(a, 8, 100, True, 0, False), (b, 112, 5, True)], counts)
        assert codec.copies == before + 2                                                # the counts, then the blocks
        assert [g.tobytes() for g in got] == [ta.push(x[8:15], True).tobytes(), tb.push(x[112:117], True).tobytes()]
        with pytest.raises(ValueError, match="last push"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 1, False)])
    finally:
        codec.adpcm_stream_close(a)
        codec.adpcm_stream_close(b)


def test_final_pushes_with_a_device_count(codec):
    """0, negative, in range and beyond n, with and without a carry in front; the block count follows the device's length"""
    streams = []
    for rate in SC.RATES:
        S = adpcm.samples_per_block(rate)
        x = SC.signal("burst", rate)
        for first, count in ((0, 0), (7, 0), (S - 1, -5), (0, -1), (3, 1), (0, S), (S - 1, 1), (S - 1, 2), (5, 2 * S + 3), (5, 10 * S),
                             (0, 3 * S + 1)):
            pushes = [(x[:first], False, None, None)] if first else []
            pushes.append((x[first: first + 3 * S], True, None, count))
            streams.append((rate, pushes))
    got = _run(codec, streams)
    for (rate, pushes), chunks in zip(streams, got):
        assert chunks == _twin(rate, pushes), (rate, len(pushes), pushes[-1][3])
    assert got[0] == [b""] and len(got[1][1]) == 256 and len(got[2][1]) == 256     # no samples at all; 7 and S - 1 carried ones leave


def _mask(n, zero_runs, seed):
    m = np.random.default_rng(seed).random(n) < 0.8
    for lo, hi in zero_runs:
        m[lo:hi] = False
    return m


def test_final_pushes_compacted_by_a_keep_mask(codec):
    """every second sample, none kept (the carry alone leaves), everything kept behind a carry of S - 1, zero runs at the start, in the
    middle and at the end, lengths that are no multiple of 8, more than one tile of the prefix sum, and a count in front of the mask"""
    streams = []
    for rate in SC.RATES:
        S = adpcm.samples_per_block(rate)
        x, y = SC.signal("noise", rate), SC.signal("square", rate)
        streams += [
            (rate, [(x[:3 * S + 5], True, np.arange(3 * S + 5) % 2 == 0, None)]),
            (rate, [(x[:S - 1], False, None, None), (x[S - 1: S + 99], True, np.zeros(100, bool), None)]),
            (rate, [(y[:S - 1], False, None, None), (y[S - 1: 3 * S], True, np.ones(2 * S + 1, bool), None)]),
            (rate, [(x[:10], False, None, None), (x[10: 9011], True, _mask(9001, [(0, 37), (4000, 4803), (8990, 9001)], 1), None)]),
            (rate, [(y[:8197], True, _mask(8197, [(0, 1), (8192, 8197)], 2), None)]),
            (rate, [(x[:S + 4], False, None, None), (x[S + 4: S + 104], True, _mask(100, [(20, 30)], 3), 50)]),
            (rate, [(x[:3], True, np.array([False, True, False]), None)]),
            (rate, [(x[:3], True, np.zeros(3, bool), None)]),
        ]
    got = _run(codec, streams)
    for (rate, pushes), chunks in zip(streams, got):
        assert chunks == _twin(rate, pushes), (rate, [len(p[0]) for p in pushes])
    assert got[1][0] == b"" and len(got[1][1]) == 256 and got[7] == [b""]


def test_a_reused_slot_sees_no_carry_and_the_staging_tail_does_not_leak(codec):
    """a stream abandoned with S - 1 samples in its slot; the next one in that slot starts clean.  Its final push ends 3 samples into a
    16-byte unit of the staging range and 5 into one of `pcm`: the positions behind read as the last sample, not as what lies there"""
    rate = 48000
    S = adpcm.samples_per_block(rate)
    x = SC.signal("noise", rate)
    buf = np.full(4 * S + 64, 12345, np.int16)
    buf[: S - 1] = x[: S - 1]
    buf[2048: 2048 + S + 5] = x[S: 2 * S + 5]
    pcm_d = torch.from_numpy(buf).to(DEV)
    a = codec.adpcm_stream_open(rate)
    assert codec.adpcm_stream_step(pcm_d, [(a, 0, S - 1, False)])[0].size == 0           # S - 1 samples wait in the slot
    codec.adpcm_stream_close(a)
    b = codec.adpcm_stream_open(rate)
    assert b == a
    try:
        twin = adpcm.StreamEncoder(rate)
        got = codec.adpcm_stream_step(pcm_d, [(b, 2048, 6, False)])[0]
        assert got.size == 0 and twin.push(x[S: S + 6]).size == 0
        got = codec.adpcm_stream_step(pcm_d, [(b, 2048 + 8, S + 5 - 8, True)])[0].tobytes()
    finally:
        codec.adpcm_stream_close(b)
    assert got == twin.push(x[S + 8: 2 * S + 5], True).tobytes() and len(got) == 2048
    assert codec.adpcm_streams_in_use() == 0


def test_a_refused_step_changes_no_stream(codec):
    x = SC.signal("burst", 24000)
    pcm_d = torch.from_numpy(x[:8192].copy()).to(DEV)
    a, b = codec.adpcm_stream_open(24000), codec.adpcm_stream_open(8000)
    try:
        ta, tb = adpcm.StreamEncoder(24000), adpcm.StreamEncoder(8000)
        got = codec.adpcm_stream_step(pcm_d, [(a, 0, 1100, False), (b, 1104, 9, False)])
        assert [g.tobytes() for g in got] == [ta.push(x[:1100]).tobytes(), tb.push(x[1104:1113]).tobytes()]
        with pytest.raises(_lib.EngineError, match="multiples of 8"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 100, False), (b, 4, 100, False)])
        with pytest.raises(ValueError, match="twice"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 100, False), (a, 104, 100, False)])
        with pytest.raises(ValueError, match="not final"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 100, False), (b, 104, 100, False, None, True)], None, torch.zeros(1024, dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="outside"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 100, False), (b, 8000, 1000, False)])
        with pytest.raises(ValueError, match="not open"):
            codec.adpcm_stream_step(pcm_d, [(a, 0, 100, False), (63, 104, 100, False)])
        with pytest.raises(ValueError, match="55125"):
            codec.adpcm_stream_open(96000)
        got = codec.adpcm_stream_step(pcm_d, [(a, 1104, 1000, True), (b, 2104, 600, True)])
        assert [g.tobytes() for g in got] == [ta.push(x[1104:2104], True).tobytes(), tb.push(x[2104:2704], True).tobytes()]
        assert all(len(g) for g in got)
    finally:
        codec.adpcm_stream_close(a)
        codec.adpcm_stream_close(b)
    assert codec.adpcm_streams_in_use() == 0

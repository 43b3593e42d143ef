"""ctts_flac_stream_step on the GPU against the NumPy twin (flac.StreamEncoder), byte for byte and push by push, and through the independent
stream decoder: the cuts of tests/flac_stream_cases.py, first samples at every length of the coded number (the 32-bit crossing and the
36-bit end included), final pushes compacted by a keep mask on the device, several streams in one step, slot reuse, refusals.
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E, flac  # noqa: E402
from tests import flac_stream_cases as SC  # noqa: E402

DEV = torch.device("cuda:0")


class _Codec:
    """the members `CodecEngine.flac_stream_step` uses, without the decoder's weights"""
    FLAC_STREAM_SLOTS = 4                        # small, so that the tests also double the pool
    _flac_pool = E.CodecEngine._flac_pool
    _flac_rec = E.CodecEngine._flac_rec
    flac_stream_open = E.CodecEngine.flac_stream_open
    flac_stream_close = E.CodecEngine.flac_stream_close
    flac_streams_in_use = E.CodecEngine.flac_streams_in_use
    flac_stream_plan = E.CodecEngine.flac_stream_plan
    flac_stream_step = E.CodecEngine.flac_stream_step
    to_host = E.CodecEngine.to_host
    _copy_out = E.CodecEngine._copy_out

    def __init__(self):
        self.lib, self.device = _lib.lib(), DEV


@pytest.fixture(scope="module")
def codec():
    return _Codec()


def _run(codec, streams, together=True):
    """streams: [(rate, first_sample, [(samples, final, keep or None, count or None)])] -> per stream the chunk of every push.  Round r
    steps the r-th push of every stream that has one, in ONE call (`together`) or one call per stream.  The samples of a round lie in
    one int16 buffer, each push on a multiple of 8 and with junk behind it; the keep flags lie in a bit mask over that buffer."""
    handles = [codec.flac_stream_open(rate, first) for rate, first, _ in streams]
    out = [[] for _ in streams]
    try:
        for r in range(max(len(p) for _, _, p in streams)):
            due = [i for i, (_, _, p) in enumerate(streams) if r < len(p)]
            pcm = np.full(sum((len(streams[i][2][r][0]) + 7) // 8 * 8 + 8 for i in due) + 8, 12345, np.int16)
            keep = np.ones(len(pcm), bool)
            counts, rows, at = [], [], 8
            for i in due:
                x, final, mask, count = streams[i][2][r]
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
            got = codec.flac_stream_step(pcm_d, rows, counts_d, mask_d) if together else \
                [codec.flac_stream_step(pcm_d, [row], counts_d, mask_d)[0] for row in rows]
            for i, g in zip(due, got):
                assert g.dtype == np.uint8
                out[i].append(g.tobytes())
    finally:
        for h in handles:
            codec.flac_stream_close(h)
    return out


def _twin(rate, first, pushes):
    enc = flac.StreamEncoder(rate, first)
    out = []
    for x, final, mask, count in pushes:
        x = np.asarray(x, np.int16)
        n = len(x) if count is None else max(0, min(count, len(x)))        # a count comes in front of the mask
        keep = np.ones(n, bool) if mask is None else np.asarray(mask, bool)[:n]
        out.append(enc.push(x[:n][keep], final))
    return out


@pytest.mark.parametrize("rate", SC.GPU_RATES)
@pytest.mark.parametrize("name", SC.GPU_SIGNALS)
def test_device_chunks_are_the_twins_push_by_push(codec, name, rate):
    """every cut of the list as one stream; the r-th pushes of all of them share one step"""
    x = SC.signal(name)
    cuts = list(SC.CUTS)
    streams = [(rate, 0, [(x[lo:hi], final, None, None) for lo, hi, final in SC.pushes(c)]) for c in cuts]
    got = _run(codec, streams)
    for c, chunks in zip(cuts, got):
        want = SC.reference(name, rate, c)
        assert [len(g) for g in chunks] == [len(w) for w in want], c
        assert tuple(chunks) == want, c
        n = SC.pushes(c)[-1][1]
        assert all(len(g) <= flac.stream_bound(hi - lo) for g, (lo, hi, _) in zip(chunks, SC.pushes(c)))
        facts = SC.check_stream(chunks, rate, x[:n])
        if name == "noise" and n == SC.N:
            assert all(k == "VERBATIM" for k, b in zip(facts["kinds"], facts["blocks"]) if b >= 16)
    assert codec.flac_streams_in_use() == 0


@pytest.mark.parametrize("first", [(1 << 7) - 20, (1 << 11) - 20, (1 << 16) - 20, (1 << 21) - 20, (1 << 26) - 20, (1 << 31) - 20,
                                   (1 << 36) - 5000])
def test_every_length_of_the_coded_sample_number(codec, first):
    """frames start at first, first + 17 and first + 17 + 4096: below and above the boundary, so both coding lengths run; at 2^31 the
    number leaves 32 bits, at 2^36 - 5000 it takes all seven bytes.  A push that would reach 2^36 is refused and changes nothing"""
    x = SC.signal("half_silence")
    pushes = [(x[:17], False, None, None), (x[17: 17 + 4096], False, None, None), (x[4113: 4213], True, None, None)]
    got, = _run(codec, [(11025, first, pushes)])
    assert got == _twin(11025, first, pushes)
    facts = SC.check_stream(got, 11025, x[:4213], first_sample=first)
    assert facts["numbers"] == [first, first + 17, first + 17 + 4096] and facts["blocks"] == [17, 4096, 100]
    if first == (1 << 36) - 5000:
        h = codec.flac_stream_open(24000, first)
        try:
            pcm_d = torch.from_numpy(x[:5008].copy()).to(DEV)
            assert codec.flac_stream_step(pcm_d, [(h, 0, 17, False)])[0].tobytes() == _twin(24000, first, pushes[:1])[0]
            with pytest.raises(ValueError, match="2\\^36"):
                codec.flac_stream_step(pcm_d, [(h, 0, 5000, False)])
            want = _twin(24000, first, [pushes[0], (x[:100], True, None, None)])[1]
            assert codec.flac_stream_step(pcm_d, [(h, 0, 100, True)])[0].tobytes() == want
        finally:
            codec.flac_stream_close(h)


def _mask(n, zero_runs, seed):
    m = np.random.default_rng(seed).random(n) < 0.8
    for lo, hi in zero_runs:
        m[lo:hi] = False
    return m


def test_final_pushes_compacted_by_a_keep_mask(codec):
    """the last push of a stream is stripped on the device: zero runs at the start, in the middle and at the end, lengths that are no
    multiple of 8, more than one tile of the prefix sum, a carry in front, a device count in front of the mask, and a tail that loses
    every sample while 15 are carried"""
    x = SC.signal("half_silence")
    y = SC.signal("spikes")
    streams = [
        (24000, 0, [(x[:10], False, None, None), (x[10: 9011], True, _mask(9001, [(0, 37), (4000, 4803), (8990, 9001)], 1), None)]),
        (8000, 100, [(y[:8197], True, _mask(8197, [(0, 1), (8192, 8197)], 2), None)]),
        (65535, 0, [(x[:15], False, None, None), (x[15:115], True, np.zeros(100, bool), None)]),
        (24000, 0, [(y[:4100], False, None, None), (y[4100:4200], True, _mask(100, [(20, 30)], 3), 50)]),
        (24000, 0, [(x[:3], True, np.array([False, True, False]), None)]),
        (24000, 0, [(x[:5000], True, None, 4097)]),
    ]
    got = _run(codec, streams)
    for (rate, first, pushes), chunks in zip(streams, got):
        assert chunks == _twin(rate, first, pushes)
    assert len(got[2][1]) > 0 and len(got[2][0]) == 0               # the 15 carried samples leave as the stream's last block
    kept = np.concatenate([x[:10], x[10:9011][streams[0][2][1][2]]])
    SC.check_stream(got[0], 24000, kept)


def test_five_streams_in_one_step_equal_each_alone(codec):
    x, y = SC.signal("half_silence"), SC.signal("noise")
    streams = [
        (24000, 0, [(x[:5000], False, None, None), (x[5000:9000], False, None, None), (x[9000:9100], True, None, None)]),
        (8000, 7, [(y[:100], False, None, None), (y[:0], False, None, None), (y[100:4300], True, None, None)]),
        (11025, 0, [(x[:20], False, None, None), (x[20:900], True, _mask(880, [(0, 9), (870, 880)], 4), None)]),
        (65535, 1 << 31, [(y[:4096], False, None, None), (y[4096:8192], False, None, None), (y[8192:8200], False, None, None)]),
        (48000, 0, [(x[:7], False, None, None), (x[7:12], False, None, None), (x[12:16], False, None, None)]),
    ]
    together = _run(codec, streams, together=True)
    alone = _run(codec, streams, together=False)
    assert together == alone
    for (rate, first, pushes), chunks in zip(streams, together):
        assert chunks == _twin(rate, first, pushes)
    assert together[4][2] and not together[4][0] and not together[4][1]      # 7 + 5 wait; 4 more make the block of 16


def test_a_reused_slot_sees_no_carry(codec):
    x = SC.signal("noise")
    pcm_d = torch.from_numpy(x[:4104].copy()).to(DEV)
    a = codec.flac_stream_open(24000)
    assert codec.flac_stream_step(pcm_d, [(a, 0, 10, False)])[0].size == 0   # ten samples wait in the slot
    codec.flac_stream_close(a)
    b = codec.flac_stream_open(24000)
    assert b == a
    try:
        got = codec.flac_stream_step(pcm_d, [(b, 16, 4000, True)])[0].tobytes()
    finally:
        codec.flac_stream_close(b)
    assert got == flac.StreamEncoder(24000).push(x[16:4016], True)


def test_a_refused_step_changes_no_stream(codec):
    x = SC.signal("half_silence")
    pcm_d = torch.from_numpy(x[:8192].copy()).to(DEV)
    a, b = codec.flac_stream_open(24000), codec.flac_stream_open(8000)
    try:
        ta, tb = flac.StreamEncoder(24000), flac.StreamEncoder(8000)
        got = codec.flac_stream_step(pcm_d, [(a, 0, 4100, False), (b, 4104, 9, False)])
        assert [g.tobytes() for g in got] == [ta.push(x[:4100]), tb.push(x[4104:4113])]
        with pytest.raises(_lib.EngineError, match="multiples of 8"):
            codec.flac_stream_step(pcm_d, [(a, 0, 100, False), (b, 4, 100, False)])
        with pytest.raises(ValueError, match="twice"):
            codec.flac_stream_step(pcm_d, [(a, 0, 100, False), (a, 104, 100, False)])
        with pytest.raises(ValueError, match="not final"):
            codec.flac_stream_step(pcm_d, [(a, 0, 100, False), (b, 104, 100, False, None, True)], None, torch.zeros(1024, dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="outside"):
            codec.flac_stream_step(pcm_d, [(a, 0, 100, False), (b, 8000, 1000, False)])
        got = codec.flac_stream_step(pcm_d, [(a, 4104, 50, True), (b, 4120, 30, True)])
        assert [g.tobytes() for g in got] == [ta.push(x[4104:4154], True), tb.push(x[4120:4150], True)]
    finally:
        codec.flac_stream_close(a)
        codec.flac_stream_close(b)

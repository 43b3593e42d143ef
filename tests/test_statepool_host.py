"""chattts_amd/statepool.py without a device: the pool of per-stream state (slot order, reuse, growth with and without buffers, the
refusals, commit), the rule that sorts a call's pushes into rounds, the checks of a step's pushes and the parser of the int16 pushes."""
from types import SimpleNamespace

import pytest
import torch

from chattts_amd import statepool as SP

REC = SP.AdpcmRec(8000, 0, False)


def test_slots_go_out_in_order_and_a_closed_one_goes_out_next():
    pool = SP.StatePool("resample", 4)
    assert [pool.open(REC) for _ in range(3)] == [0, 1, 2] and pool.in_use == 3 and pool.slots == 4 and pool.buf == {}
    pool.close(1)
    pool.close(0)
    assert pool.in_use == 1 and [pool.open(REC), pool.open(REC), pool.open(REC)] == [0, 1, 3]      # last closed, first opened
    assert pool.in_use == 4 and pool.slots == 4


def test_a_full_pool_doubles_every_buffer_and_keeps_what_they_hold():
    pool = SP.StatePool("limiter", 4, dict(carry=((2, 3), torch.float32), stats=((5,), torch.int32)), device="cpu")
    assert pool.buf["carry"].shape == (4, 2, 3) and pool.buf["carry"].dtype == torch.float32 and not pool.buf["carry"].any()
    assert pool.buf["stats"].shape == (4, 5) and pool.buf["stats"].dtype == torch.int32 and not pool.buf["stats"].any()
    assert [pool.open(REC) for _ in range(4)] == [0, 1, 2, 3]
    pool.buf["carry"].copy_(torch.arange(1, 25, dtype=torch.float32).view(4, 2, 3))
    pool.buf["stats"].copy_(torch.arange(1, 21, dtype=torch.int32).view(4, 5))
    carry, stats = pool.buf["carry"].clone(), pool.buf["stats"].clone()
    assert [pool.open(REC), pool.open(REC)] == [4, 5] and pool.slots == 8 and pool.in_use == 6
    assert pool.buf["carry"].shape == (8, 2, 3) and pool.buf["carry"].dtype == torch.float32
    assert pool.buf["stats"].shape == (8, 5) and pool.buf["stats"].dtype == torch.int32
    assert torch.equal(pool.buf["carry"][:4], carry) and torch.equal(pool.buf["stats"][:4], stats)
    assert not pool.buf["carry"][4:].any() and not pool.buf["stats"][4:].any()
    assert [pool.open(REC), pool.open(REC)] == [6, 7] and pool.open(REC) == 8 and pool.slots == 16 and pool.buf["stats"].shape == (16, 5)


def test_a_pool_without_a_device_grows_its_free_list_only():
    pool = SP.StatePool("pauses", 4, dict(carry=((2, 3), torch.float32)))
    assert [pool.open(REC) for _ in range(9)] == list(range(9)) and pool.slots == 16 and pool.buf == {} and pool.in_use == 9
    pool.close(6)
    assert pool.open(REC) == 6 and pool.open(REC) == 9


def test_the_refusals_name_the_pool_and_the_stream():
    pool = SP.StatePool("flac", 4)
    h = pool.open(SP.FlacRec(8000, 0, 0, False))
    assert pool.get(h) == pool.live(h) == (8000, 0, 0, False)
    for call in (pool.get, pool.live, pool.close):
        with pytest.raises(ValueError, match="^flac: stream 3 is not open$"):
            call(3)
    pool.commit({h: pool.get(h)._replace(done=True)})
    assert pool.get(h).done                                          # `get` still answers: the stream is open
    with pytest.raises(ValueError, match="^flac: stream 0 has had its last push$"):
        pool.live(h)
    other = pool.open(SP.FlacRec(8000, 0, 0, False))
    with pytest.raises(ValueError, match="^flac: stream 1 has had its last push$"):               # ended by a push planned earlier in the call
        pool.live(other, {other: SP.FlacRec(8000, 16, 0, True)})
    assert pool.live(other, {h: SP.FlacRec(8000, 16, 0, True)}) == (8000, 0, 0, False)
    assert pool.live(other, {other: SP.FlacRec(8000, 16, 3, False)}) == (8000, 16, 3, False)
    pool.close(h)
    with pytest.raises(ValueError, match="^flac: stream 0 is not open$"):
        pool.close(h)
    assert pool.in_use == 1


def test_only_commit_changes_a_record():
    pool = SP.StatePool("time_scale", 4)
    a, b = pool.open(SP.TimeScaleRec(125, 100, 0, 0, False)), pool.open(SP.TimeScaleRec(50, 100, 0, 0, False))
    rec = pool.live(a)
    new = rec._replace(pushed=3000, phase=1)
    pool.live(a, {a: new})
    assert pool.records == {a: (125, 100, 0, 0, False), b: (50, 100, 0, 0, False)} and pool.get(a) is rec
    with pytest.raises(AttributeError):
        rec.pushed = 1                                               # a record is replaced, never written
    pool.commit({a: new})
    assert pool.records == {a: (125, 100, 3000, 1, False), b: (50, 100, 0, 0, False)} and pool.get(a) is new and pool.in_use == 2


def test_the_rth_push_of_a_stream_goes_to_round_r_in_the_order_given():
    assert SP.rounds([]) == ([], [])
    assert SP.rounds([5]) == ([0], [[0]])
    assert SP.rounds([5, 5, 5]) == ([0, 1, 2], [[0], [1], [2]])
    assert SP.rounds([3, 1, 3, 2, 1, 3]) == ([0, 0, 1, 0, 1, 2], [[0, 1, 3], [2, 4], [5]])                # interleaved; a round keeps the order
    assert SP.rounds(iter([2, 1, 0])) == ([0, 0, 0], [[0, 1, 2]])
    assert SP.rounds([None, 4, None, 4]) == ([-1, 0, -1, 1], [[1], [3]])                                  # None: no push, in no round
    assert SP.rounds([("flac", 1), ("adpcm", 1), ("flac", 1)]) == ([0, 0, 1], [[0, 1], [2]])              # any hashable names a stream


def test_the_checks_every_step_shares():
    ok = [(0, 0, 10, False), (1, 10, 10, True)]
    SP.check_pushes("resample", ok, 20)
    SP.check_pushes("resample", ok)
    for pushes, kw, why in [([], {}, "^limiter: nothing to step$"),
                            ([(i, 0, 0, False) for i in range(1025)], {}, "^limiter: at most 1024 streams in one step$"),
                            ([(0, 0, 1, False), (0, 1, 1, False)], {}, "^limiter: a stream appears twice in one step$"),
                            (ok, dict(n_el=19), "^limiter: a push lies outside the tensor$"),
                            ([(0, -1, 1, False)], dict(n_el=19), "outside the tensor"), ([(0, 0, -1, False)], dict(n_el=19), "outside the tensor")]:
        with pytest.raises(ValueError, match=why):
            SP.check_pushes("limiter", pushes, **kw)
    SP.check_pushes("time_scale", [(i, 0, 0, False) for i in range(1025)], 0, most=None)                   # the library's refusal, not Python's
    SP.check_pushes("pauses", [(0, 0, 1, False), (0, 1, 1, False)], 2, once=False)                         # left to the descriptor builder
    SP.check_pushes("limiter", [(i, 0, 0, False) for i in range(1024)], 0)


class _OnDevice(torch.Tensor):
    """a host tensor that says it lies on the device: all the parser asks of one"""
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def test_the_int16_pushes_are_parsed_and_checked_once_for_both_formats():
    pool = SP.StatePool("adpcm", 4)
    a, b = pool.open(SP.AdpcmRec(8000, 5, False)), pool.open(SP.AdpcmRec(16000, 0, False))
    pcm, counts, masks = _dev(torch.zeros(64, dtype=torch.int16)), _dev(torch.zeros(2, dtype=torch.int64)), _dev(torch.zeros(8, dtype=torch.uint8))
    parse = lambda pushes, p=pcm, c=counts, m=masks, label="adpcm": list(SP.int16_pushes(label, p, pushes, c, m, pool.live))
    assert parse([(a, 0, 16, False), (b, 16, 48, True, 1, True)]) == [(a, 0, 16, False, -1, False, (8000, 5, False)),
                                                                      (b, 16, 48, True, 1, True, (16000, 0, False))]
    assert parse([(a, 8, 0, 1, None, 0)], c=None, m=None) == [(a, 8, 0, True, -1, False, (8000, 5, False))]
    assert parse([(a, 0, 64, True, None, True)]) == [(a, 0, 64, True, -1, True, (8000, 5, False))]         # 8 mask bytes reach element 64
    one = [(a, 0, 8, False)]
    for kw, why in [(dict(p=torch.zeros(64, dtype=torch.int16)), "^adpcm: a contiguous int16 device tensor$"),
                    (dict(p=_dev(torch.zeros(64, dtype=torch.int32))), "a contiguous int16 device tensor"),
                    (dict(p=_dev(torch.zeros(64, 2, dtype=torch.int16))[:, 0]), "a contiguous int16 device tensor"),
                    (dict(p=SimpleNamespace(is_cuda=True)), "a contiguous int16 device tensor"),
                    (dict(c=torch.zeros(2, dtype=torch.int64)), "^adpcm: `counts` must be a contiguous int64 device tensor$"),
                    (dict(c=_dev(torch.zeros(2, dtype=torch.int32))), "`counts` must be"),
                    (dict(m=torch.zeros(8, dtype=torch.uint8)), "^adpcm: `masks` must be a contiguous uint8 device tensor$"),
                    (dict(m=_dev(torch.zeros(8, dtype=torch.int8))), "`masks` must be")]:
        with pytest.raises(ValueError, match=why):
            parse(one, **kw)
    for pushes, kw, why in [([], {}, "^flac: nothing to step$"),
                            ([(i, 0, 0, False) for i in range(1025)], {}, "^flac: at most 1024 streams in one step$"),
                            ([(a, 0, 8, False), (a, 8, 8, False)], {}, "^flac: a stream appears twice in one step$"),
                            ([(3, 0, 8, False)], {}, "^adpcm: stream 3 is not open$"),                    # the pool's own words
                            ([(a, 60, 8, False)], {}, "^flac: a push lies outside the tensor$"),
                            ([(a, -8, 8, False)], {}, "outside the tensor"), ([(a, 0, -1, False)], {}, "outside the tensor"),
                            ([(a, 0, 8, True), (b, 8, 8, True, 2)], {}, "^flac: push 1 reads count 2, beyond `counts`$"),
                            ([(a, 0, 8, True, 0)], dict(c=None), "^flac: push 0 reads count 0, beyond `counts`$"),
                            ([(a, 0, 8, True, None, True)], dict(m=None), "^flac: push 0 is masked, and `masks` does not reach its end$"),
                            ([(a, 0, 64, True, None, True)], dict(m=_dev(torch.zeros(7, dtype=torch.uint8))), "push 0 is masked, and `masks` does not"),
                            ([(a, 0, 8, False, 0)], {}, "^flac: push 0 leaves its length to the device but is not final$"),
                            ([(a, 0, 8, False, None, True)], {}, "push 0 leaves its length to the device but is not final")]:
        with pytest.raises(ValueError, match=why):
            parse(pushes, label="flac", **kw)
    pool.commit({b: SP.AdpcmRec(16000, 0, True)})
    with pytest.raises(ValueError, match="^adpcm: stream 1 has had its last push$"):
        parse([(a, 0, 8, False), (b, 8, 8, False)])
    got = SP.int16_pushes("adpcm", pcm, [(a, 0, 8, False), (b, 8, 8, False)], None, None, pool.live)       # push by push: a's row comes out
    assert next(got)[:3] == (a, 0, 8)                                                                      # before b is looked at
    with pytest.raises(ValueError, match="last push"):
        next(got)
    assert pool.records == {a: (8000, 5, False), b: (16000, 0, True)}

"""`winchain.StreamSet` on a counting fake codec: every option mix opens exactly the stages it should with the arguments the streamed
paths have always used, a failed open leaves nothing open, and a set gives every handle back once.  And the stage table itself: one
row per streamed stage, naming methods and arguments the engine has.  No GPU."""
import inspect
import itertools

import pytest

from chattts_amd import winchain as WC
from chattts_amd.engine import CodecEngine

OPENS = {"time_scale_stream_open": "time_scale", "resample_stream_open": "resample", "flac_stream_open": "flac", "adpcm_stream_open": "adpcm",
         "peak_limit_stream_open": "limiter", "trim_pauses_stream_open": "pauses", "compress_stream_open": "compress"}


class _Codec:
    """counts: every open hands out the next handle and logs (stage, arguments); every close logs (stage, handle)"""
    def __init__(self, fail_at=None):
        self.opened, self.closed, self.fail_at = [], [], fail_at

    def __getattr__(self, name):
        if name in OPENS:
            def open_(*args):
                if self.fail_at is not None and len(self.opened) == self.fail_at:
                    raise RuntimeError("no slot")
                self.opened.append((OPENS[name], args))
                return 100 + len(self.opened)
            return open_
        if name.endswith("_stream_close") and name.replace("_close", "_open") in OPENS:
            return lambda h: self.closed.append((OPENS[name.replace("_close", "_open")], h))
        raise AttributeError(name)


def _want(rate, speed, pauses, compress, limiter, gain, flac, adpcm):
    out = 24000 if rate is None else rate
    return ([("time_scale", (speed,))] if speed is not None else []) + ([("resample", (24000, rate))] if speed is not None and rate is not None else []) \
        + ([("flac", (out,))] if flac else []) + ([("adpcm", (out,))] if adpcm else []) \
        + ([("limiter", (out, 1.0 if gain is None else gain))] if limiter or gain is not None else []) \
        + ([("pauses", (out, pauses))] if pauses is not None else []) + ([("compress", (out, compress))] if compress is not None else [])


def test_every_option_mix_opens_exactly_its_stages_with_their_arguments():
    seen = set()
    for rate, speed, pauses, compress, (limiter, gain), flac, adpcm in itertools.product(
            (None, 8000), (None, 1.25), (None, {"tail_ms": 0}), (None, {"hold_ms": 100}), ((False, None), (True, None), (True, 2.0), (False, 0.5)),
            (False, True), (False, True)):
        codec = _Codec()
        s = WC.StreamSet.open(codec, rate=rate, speed=speed, pauses=pauses, compress=compress, limiter=limiter, limiter_gain=gain, flac=flac, adpcm=adpcm)
        want = _want(rate, speed, pauses, compress, limiter, gain, flac, adpcm)
        assert codec.opened == want, (codec.opened, want)                       # the stages, their arguments and the order of the opens
        assert {k: s.get(k) for k in OPENS.values()} == {**dict.fromkeys(OPENS.values()), **{st: 101 + i for i, (st, _) in enumerate(want)}}
        s.close(codec)
        assert sorted(codec.closed) == sorted((st, 101 + i) for i, (st, _) in enumerate(want))
        seen.add(len(want))
    assert seen == set(range(8))                                                # from nothing to all seven


def test_an_open_that_raises_at_the_third_stage_leaves_nothing_open():
    codec = _Codec(fail_at=2)
    with pytest.raises(RuntimeError, match="no slot"):
        WC.StreamSet.open(codec, rate=8000, speed=1.25, flac=True, limiter=True, pauses=True, compress=True)
    assert [st for st, _ in codec.opened] == ["time_scale", "resample"] and sorted(codec.closed) == [("resample", 102), ("time_scale", 101)]


def test_close_twice_closes_once_and_a_set_with_nothing_on_opens_nothing():
    codec = _Codec()
    s = WC.StreamSet.open(codec, speed=0.8, compress=True)
    s.close(codec)
    s.close(codec)
    assert codec.closed == [("time_scale", 101), ("compress", 102)] and s.get("compress") is None
    codec = _Codec()
    s = WC.StreamSet.open(codec)
    s.close(codec)
    assert codec.opened == [] and codec.closed == [] and all(s.get(k) is None for k in OPENS.values())
    assert WC.StreamSet.needed() == {} and WC.StreamSet.needed(rate=8000) == {} and WC.StreamSet.open(None, rate=8000) == {}      # the codec is not touched


def test_the_table_has_one_row_per_streamed_stage_and_names_what_the_engine_has():
    assert sorted(s.name for s in WC.STAGES) == sorted(OPENS.values()) == sorted(CodecEngine.POOLS)
    args = inspect.signature(CodecEngine.decode_windows).parameters
    for s in WC.STAGES:
        assert OPENS[s.open] == s.name and s.close == s.open.replace("_open", "_close")
        assert callable(getattr(CodecEngine, s.open)) and callable(getattr(CodecEngine, s.close)) and s.flag in args and s.streams in args
        assert s.step is None or callable(getattr(CodecEngine, s.step))
    assert [s.name for s in WC.CHECKED] == ["compress", "pauses", "limiter", "flac", "adpcm"]          # the order of the refusals
    assert [s.name for s in WC.ROUNDS] == ["pauses", "compress"] and {s.name for s in WC.STAGES if s.kind == "float"} == {"limiter", "pauses", "compress"}

"""`CodecEngine.decode_windows` behind its streamed stages, pinned absolutely: every array the calls below return for the seeded store of
test_gpu_decode_windows_pin.py, against SHA-256 hashes recorded from an earlier build.  That pin stops in front of the limiter, pause and
compressor streams, the FLAC / ADPCM epilogue and the resampler-stream entry; these cases enter all of them.  `pytest -m gpu`."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, timescale as TS  # noqa: E402
from tests.test_gpu_decode_windows_pin import EMPTY, ENCODINGS, SHORT, digest  # noqa: E402
from tests.test_gpu_stream_pool import WINDOWS, _store  # noqa: E402
from tests.test_gpu_stream_resample import RWINDOWS  # noqa: E402
from tests.test_gpu_timescale_stream_e2e import SWINDOWS  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_windows_streams_sha256.json")

# stage -> (flag argument, streams argument, open(codec, rate, speed), close)
STAGES = {"limiter": ("limiter", "lm_streams", lambda c, r: c.peak_limit_stream_open(r), "peak_limit_stream_close"),
          "pauses": ("pauses", "pa_streams", lambda c, r: c.trim_pauses_stream_open(r), "trim_pauses_stream_close"),
          "compress": ("compress", "cp_streams", lambda c, r: c.compress_stream_open(r), "compress_stream_close"),
          "flac": ("flac", "flac_streams", lambda c, r: c.flac_stream_open(r), "flac_stream_close"),
          "adpcm": ("adpcm", "adpcm_streams", lambda c, r: c.adpcm_stream_open(r), "adpcm_stream_close")}
ALL3 = ("limiter", "pauses", "compress")
IN_USE = ("time_scale", "resample", "peak_limit", "trim_pauses", "compress", "flac", "adpcm")


def call(codec, store, wins, on, rates=None, speeds=None, rs=False, share=(), **kw):
    """One `decode_windows` call with its streams opened in front of it and closed behind it.  `on`: stage -> the windows it is flagged
    for (True: all).  `share`: (i, j) pairs, window j continues window i's stream in every stage both are flagged for (and its time-scale
    and resampler streams).  `rs`: the windows at a speed and another rate get a resampler stream."""
    n = len(wins)
    first = {j: i for i, j in share}
    opened = []

    def handles(flags, open_one, close):
        hs = [None] * n
        for i in range(n):
            if flags[i]:
                if i in first and flags[first[i]]:
                    hs[i] = hs[first[i]]
                else:
                    hs[i] = open_one(i)
                    opened.append((close, hs[i]))
        return hs

    try:
        if rates is not None:
            kw["sample_rates"] = rates
        if speeds is not None:
            scaled = [TS.quantize(v)[0] != TS.quantize(v)[1] for v in speeds]
            kw["speeds"] = speeds
            kw["ts_streams"] = handles(scaled, lambda i: codec.time_scale_stream_open(speeds[i]), "time_scale_stream_close")
            if rs:
                kw["rs_streams"] = handles([s and rates[i] != 24000 for i, s in enumerate(scaled)],
                                           lambda i: codec.resample_stream_open(24000, rates[i]), "resample_stream_close")
        for stage, which in on.items():
            arg, arg_streams, open_one, close = STAGES[stage]
            flags = [which is True or i in which for i in range(n)]
            kw[arg] = flags
            kw[arg_streams] = handles(flags, lambda i: open_one(codec, 24000 if rates is None else rates[i]), close)
        return codec.decode_windows(store, wins, **kw)
    finally:
        for close, h in opened:
            getattr(codec, close)(h)


def decode_windows_streams_cases(codec):
    """name -> the arrays of one `decode_windows` call; the store, the lists and the edge windows of test_gpu_decode_windows_pin.py"""
    store = _store(5)
    store[5, 0] *= 1e-3
    plain = list(WINDOWS) + [EMPTY]
    rated = [w for w, _ in RWINDOWS] + [SHORT, EMPTY]
    rates = [8000, 16000, 24000, 8000, 8000, 16000, 24000, 16000, 8000, 16000]
    sped = [w for w, _ in SWINDOWS] + [SHORT, SHORT, EMPTY, EMPTY]
    speeds = [v for _, v in SWINDOWS] + [1.25, 1.0, 0.77, 1.0]
    # speeds with rates: scaled at 24 kHz, scaled at another rate (a resampler stream), speed 1 at another rate (the stateless window
    # path, a pass of its own), speed 1 at 24 kHz
    srates = [24000, 16000, 8000, 8000, 8000, 44100, 24000, 16000, 16000, 8000, 8000, 24000]
    half = {i for i in range(len(plain)) if i % 2 == 0}
    pcm = dict(pcm16=True, keep_thr=1e-5)
    every = {s: True for s in ALL3}
    out = {}
    for s in ALL3:
        out[s + "_only"] = call(codec, store, plain, {s: True}, **pcm)
    out["three_on_half"] = call(codec, store, plain, {s: half for s in ALL3}, **pcm)
    out["three_each_its_own_windows"] = call(codec, store, plain, {"limiter": {0, 1, 4, 5}, "pauses": {1, 2, 4, 8}, "compress": {2, 3, 4, 5}}, **pcm)
    out["three_behind_speeds"] = call(codec, store, sped, every, speeds=speeds, **pcm)
    out["three_behind_rates"] = call(codec, store, rated, every, rates=rates, **pcm)
    out["three_behind_speeds_and_rates"] = call(codec, store, sped, every, rates=srates, speeds=speeds, rs=True, **pcm)
    out["speeds_and_rates"] = call(codec, store, sped, {}, rates=srates, speeds=speeds, rs=True, **pcm)
    for fmt in ("flac", "adpcm"):
        some = {i for i in range(12) if i % 3 != 0}
        out[fmt + "_plain"] = call(codec, store, plain, {fmt: some}, **pcm)
        out[fmt + "_rates"] = call(codec, store, rated, {fmt: some}, rates=rates, **pcm)
        out[fmt + "_speeds"] = call(codec, store, sped, {fmt: some}, speeds=speeds, **pcm)
        out[fmt + "_speeds_and_rates"] = call(codec, store, sped, {fmt: True}, rates=srates, speeds=speeds, rs=True, **pcm)
        out[fmt + "_limited"] = call(codec, store, plain, {**every, fmt: True}, **pcm)
        out[fmt + "_limited_half"] = call(codec, store, plain, {"limiter": half, "compress": {0, 1, 4}, fmt: some}, **pcm)
    out["flac_and_adpcm"] = call(codec, store, plain, {"flac": {0, 3, 4, 8}, "adpcm": {1, 5, 6}, "pauses": {0, 1, 2}}, **pcm)
    out["encodings_limited"] = call(codec, store, plain, every, encodings=[ENCODINGS[i % 3] for i in range(len(plain))], **pcm)
    out["encodings_limited_half"] = call(codec, store, plain, {"limiter": half}, encodings=[ENCODINGS[(i + 1) % 3] for i in range(len(plain))], **pcm)
    out["limited_f32"] = call(codec, store, plain, every, pcm16=False)
    out["limited_f32_keep"] = call(codec, store, plain, every, pcm16=False, keep_thr=1e-5)
    out["limited_f32_half"] = call(codec, store, plain, {"pauses": half}, pcm16=False, keep_thr=1e-5)
    out["limited_pcm16_f32_product"] = call(codec, store, plain, every, pcm16=True, keep_thr=1e-5, product="f32")
    # two and three windows of one stream in one call: successive rounds, in the order given
    twice = [(0, 24, 0, 6000, False), (1, 96, 24000, 36000, False), (0, 24, 6000, None, True), (1, 96, 36000, 40000, False), (1, 96, 40000, None, True)]
    pairs = [(0, 2), (1, 3), (1, 4)]
    out["one_limiter_stream_twice"] = call(codec, store, twice, {"limiter": True}, share=pairs, **pcm)
    out["one_pause_stream_twice"] = call(codec, store, twice, {"pauses": True}, share=pairs, **pcm)
    out["every_stream_twice"] = call(codec, store, twice, {**every, "flac": True}, share=pairs, **pcm)
    out["every_stream_twice_at_speeds"] = call(codec, store, twice, {**every, "adpcm": True}, speeds=[1.25, 1.0, 1.25, 1.0, 1.0],
                                               rates=[16000, 8000, 16000, 8000, 8000], rs=True, share=pairs, **pcm)
    # a tail whose crop is empty: it ends its streams and brings what they held; alone, no window of the call has a sample
    gone = (0, 24, 12032, None, True)
    out["empty_tail"] = call(codec, store, [(0, 24, 0, 12000, False), gone, WINDOWS[1]], {**every, "flac": {0, 1}}, share=[(0, 1)], **pcm)
    out["empty_tail_f32"] = call(codec, store, [(0, 24, 0, 12000, False), gone], every, share=[(0, 1)], pcm16=False, keep_thr=1e-5)
    out["all_empty"] = call(codec, store, [gone, EMPTY], {**every, "flac": {0}, "adpcm": {1}}, **pcm)
    return out


def test_decode_windows_behind_its_streams_returns_the_recorded_arrays(weights):
    """The hashes were recorded on an MI355X at commit 4a37f9c ("Output equaliser: a biquad cascade on the device, per request"), the
    last one before `decode_windows` came to parse its lists once and to run its float stages without calling itself: gemm "f32", two
    recordings in separate processes agreed on every case listed."""
    with open(GOLDEN) as fh:
        want = json.load(fh)["cases"]
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")
    got = {k: digest(v) for k, v in decode_windows_streams_cases(codec).items() if k in want}
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert len(got[name]) == len(want[name]), name
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, i, g, w)
    # the recorded cases hold what they were chosen for: streams that emit, a lag a tail brings in, a float path that strips
    n = {k: [a["n"] for a in v] for k, v in want.items()}
    assert n["limiter_only"][0] == 12000 - 24000 // 50 and n["limiter_only"][-1] == 0
    assert n["empty_tail_f32"][0] > 0 and n["empty_tail_f32"][1] > 0
    assert all(a["dtype"] == "uint8" for a in want["flac_limited"]) and all(a["dtype"] == "float32" for a in want["limited_f32"])
    for stage in IN_USE:
        assert getattr(codec, stage + "_streams_in_use")() == 0, stage

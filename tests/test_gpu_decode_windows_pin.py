"""`CodecEngine.decode_windows` pinned absolutely: every array the plain, mixed-rate and mixed-speed calls return for a fixed seeded store
and fixed window lists, against SHA-256 hashes recorded from an earlier build.  The relative tests (test_gpu_stream_pool.py,
test_gpu_stream_resample.py, test_gpu_timescale_stream_e2e.py) compare each variant with its serial composition; this one notices a
change that moves both sides.  `pytest -m gpu`."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, timescale as TS  # noqa: E402
from tests.test_gpu_stream_pool import WINDOWS, _store  # noqa: E402
from tests.test_gpu_stream_resample import RWINDOWS  # noqa: E402
from tests.test_gpu_timescale_stream_e2e import SWINDOWS  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_windows_parent_sha256.json")

# where a shared prologue can go wrong: a range with no sample in it (24 tokens decode to 12,032 samples) and a one-token tail, next to
# the lists' own tails that the strip shortens (the fifth window of each) and the one-sample push that makes an empty chunk
EMPTY, SHORT = (0, 24, 12032, 24000, False), (5, 1, 0, None, True)
ENCODINGS = (None, "ulaw", "alaw")


def decode_windows_cases(codec):
    """name -> the arrays of one `decode_windows` call; one store for all (slot 5's first row scaled down, as test_gpu_stream_pool.py does)"""
    store = _store(5)
    store[5, 0] *= 1e-3
    plain = list(WINDOWS) + [EMPTY]
    rated = [w for w, _ in RWINDOWS] + [SHORT, EMPTY]
    rates = [8000, 16000, 24000, 8000, 8000, 16000, 24000, 16000, 8000, 16000]
    # SWINDOWS holds the one-sample push (an empty chunk); behind it a one-token tail at a speed and at speed 1, an empty range that still
    # steps its stream and one that does not
    sped = [w for w, _ in SWINDOWS] + [SHORT, SHORT, EMPTY, EMPTY]
    speeds = [v for _, v in SWINDOWS] + [1.25, 1.0, 0.77, 1.0]
    out = {"plain_f32": codec.decode_windows(store, plain, pcm16=False),
           "plain_pcm16_f64": codec.decode_windows(store, plain, pcm16=True, keep_thr=1e-5, product="f64"),
           "plain_pcm16_f32": codec.decode_windows(store, plain, pcm16=True, keep_thr=1e-5, product="f32")}
    for name, enc in (("", None), ("_encodings", ENCODINGS)):
        kw = {} if enc is None else {"encodings": [enc[i % 3] for i in range(len(rated))]}
        out["rates" + name] = codec.decode_windows(store, rated, pcm16=True, keep_thr=1e-5, sample_rates=rates, **kw)
        kw = {} if enc is None else {"encodings": [enc[i % 3] for i in range(len(sped))]}
        hs = [None if TS.quantize(v)[0] == 100 else codec.time_scale_stream_open(v) for v in speeds]
        try:
            out["speeds" + name] = codec.decode_windows(store, sped, pcm16=True, keep_thr=1e-5, speeds=speeds, ts_streams=hs, **kw)
        finally:
            for h in hs:
                if h is not None:
                    codec.time_scale_stream_close(h)
    return out


def digest(arrays):
    return [{"sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), "dtype": str(a.dtype), "n": int(a.size)} for a in arrays]


def test_decode_windows_returns_the_recorded_arrays(weights):
    """The hashes were recorded on an MI355X from the library built at commit c8e9768 ("Stream at any speed: carry the time scaler's
    path across chunks"), the last one before the three window-decode entries came to share their checks, their front half and their
    conversion body, and `decode_windows` its prologue and epilogue: gemm "f32", two recordings in separate calls agreed."""
    with open(GOLDEN) as fh:
        want = json.load(fh)["cases"]
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")
    got = {k: digest(v) for k, v in decode_windows_cases(codec).items()}
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert len(got[name]) == len(want[name]), name
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, i, g, w)
    # the recorded cases hold what they were chosen for: empty ranges, tails the strip shortened (16,608 samples from sample 20,000 of 72
    # tokens: 5,536 at 8 kHz, 21,569 at speed 0.77), the empty chunks of stepped streams
    n = {k: [a["n"] for a in v] for k, v in want.items()}
    assert n["plain_f32"][-1] == n["rates"][-1] == n["speeds"][-1] == 0 and 0 < n["plain_pcm16_f64"][4] < n["plain_f32"][4]
    assert 0 < n["rates"][4] < 5536 and 0 < n["speeds"][4] < 21569 and n["speeds"][7] == 0 and n["speeds"][10] == 0
    assert codec.time_scale_streams_in_use() == 0

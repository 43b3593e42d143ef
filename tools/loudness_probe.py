"""What the device loudness stage costs (csrc/loudness.hip, ctts_loudness_normalize_ragged), beside the decode it follows:

  * call      : 1 and 64 segments of 10 s (240 000 samples at 24 kHz), each a group of its own -- device time of one call (its three
                launches: the tiles, the groups, the scale pass), from events around `--reps` back-to-back calls on pre-uploaded tables,
                after warm calls; and the worst |L - L_twin| of the records against the NumPy float64 twin on the first segments
  * scale     : the bytes the scale pass moves (one float32 read and one written per sample) -- against the time of the whole call here;
                the three launches' own times come from a kernel trace of `--trace` (the 64-segment calls alone, nothing else on the device):
                    rocprofv3 --kernel-trace --stats -- python tools/loudness_probe.py --trace
  * decode    : `Chat.decode_to_pcm16(rows, ragged=True)` on 64 rows of 469 tokens (10 s each) without `loudness=` and with it, same
                rows; wall time including the host side

Synthetic weights, noise input under a stepped envelope (the kernels' work does not depend on the samples).  Prints one JSON line.  Not a
bench.py leg.

    python tools/loudness_probe.py [--reps 20] [--gemm f16] [--trace]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import loudness as LN  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

SEG = 240000          # 10 s at 24 kHz
TOKENS = 469          # 256 (2 T - 1) = 239 872 samples
TARGET = -16.0


def _signal(n_seg):
    r = np.random.default_rng(5)
    env = np.repeat(r.choice([0.003, 0.05, 0.3], size=n_seg * SEG // 1200), 1200)
    return (r.uniform(-1, 1, n_seg * SEG) * env).astype(np.float32)


def _call_ms(codec, n_seg, reps, check=2):
    """device time of one call over n_seg segments of 10 s, and the records' worst distance from the twin on the first `check` segments"""
    dev = codec.device
    host = _signal(n_seg)
    x = torch.from_numpy(host).to(dev)
    y = torch.empty_like(x)
    off = np.arange(n_seg + 1, dtype=np.int64) * SEG
    grp = np.arange(n_seg + 1, dtype=np.int32)
    ridx = np.zeros(n_seg, np.int32)
    tgt = np.full(n_seg, TARGET)
    coef_d, coef_h, _ = codec._loudness_coef([24000])
    tabs = [torch.from_numpy(t).to(dev) for t in (off, ridx, grp, tgt)]
    sb = int(codec.lib.ctts_loudness_normalize_ragged_scratch_bytes(off.ctypes.data_as(C.c_void_p), n_seg))
    stats = torch.empty(LN.STATS.itemsize * n_seg, dtype=torch.uint8, device=dev)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call():
        rc = codec.lib.ctts_loudness_normalize_ragged(x.data_ptr(), y.data_ptr(), tabs[0].data_ptr(), vp(off), n_seg, tabs[1].data_ptr(), vp(ridx),
                                                      coef_d.data_ptr(), vp(coef_h), 1, tabs[2].data_ptr(), vp(grp), n_seg, tabs[3].data_ptr(), vp(tgt),
                                                      stats.data_ptr(), scratch.data_ptr(), sb, st)
        assert rc == 0, codec.lib.ctts_last_error()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / reps
    rec = stats.cpu().numpy().view(LN.STATS)
    worst = 0.0
    for i in range(min(check, n_seg)):
        _, tw = LN.normalize(host[i * SEG: (i + 1) * SEG], TARGET)
        worst = max(worst, abs(float(rec["L"][i]) - float(tw["L"][0])))
        assert (rec["n_blocks"][i], rec["n_abs"][i], rec["n_rel"][i]) == (tw["n_blocks"][0], tw["n_abs"][0], tw["n_rel"][0])
    return round(ms, 4), worst


def _wall_ms(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gemm", default="f16")
    ap.add_argument("--trace", action="store_true", help="only the 64-segment calls: the run to put under a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_probe needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    if a.trace:
        from chattts_amd.engine import CodecEngine
        codec = CodecEngine(sds["decoder"], sds["vocos"], dev)
        ms, _ = _call_ms(codec, 64, a.reps, check=0)
        print(json.dumps(dict(metric="loudness_probe_trace", segments=64, call_ms=ms, reps=a.reps)))
        return
    from chattts_amd.core import Chat
    chat = Chat()
    assert chat.load(state_dicts={k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}, device=dev, dtype="f32", codec_gemm=a.gemm)
    codec = chat.codec
    out = dict(metric="loudness_probe", segment_samples=SEG, tokens_per_row=TOKENS, codec_gemm=a.gemm, reps=a.reps, call_ms={}, worst_dL_vs_twin={},
               scale_pass={}, decode_to_pcm16_ms={})
    for n_seg in (1, 64):
        ms, worst = _call_ms(codec, n_seg, a.reps)
        out["call_ms"][f"{n_seg}x"] = ms
        out["worst_dL_vs_twin"][f"{n_seg}x"] = worst
        moved = 8 * n_seg * SEG
        out["scale_pass"][f"{n_seg}x"] = dict(bytes=moved, us_at_8TBps=round(moved / 8e12 * 1e6, 3))
    rs = np.random.RandomState(3)
    rows = [torch.from_numpy(rs.standard_normal((TOKENS, 768)).astype(np.float32) * 0.5).to(dev) for _ in range(64)]
    reps = max(5, a.reps // 2)
    for name, kw in (("off", {}), ("loudness", {"loudness": TARGET}), ("off_again", {})):
        med, lo, hi = _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True, **kw), reps)
        out["decode_to_pcm16_ms"][name] = dict(median=med, min=lo, max=hi)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

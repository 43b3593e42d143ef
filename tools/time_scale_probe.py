"""What the device time scaler costs (csrc/timescale.hip, ctts_time_scale_ragged), beside the decode it follows:

  * launch    : 1, 8 and 64 segments of 10 s (240 000 samples at 24 kHz) at speeds 0.5, 1.25 and 2.0 -- device time of one call (the search
                and the overlap-add), from events around `--reps` back-to-back calls on pre-uploaded tables, after warm calls; the search
                walks ceil(n_out / 512) dependent frames per segment, the segments side by side, one workgroup each
  * decode    : `Chat.decode_to_pcm16(rows, ragged=True)` on 1, 8 and 64 rows of 469 tokens (10 s each) without `speed=` and with it, same
                rows; wall time including the host side

  * --stream  : instead, the streamed scaler (ctts_time_scale_stream_step, one launch): 1, 8 and 64 streams in their steady state, each
                pushed 12 000 samples per step, at speeds 0.5, 1.25 and 2.0 -- device time of one step from events around `--reps`
                back-to-back steps on pre-uploaded descriptor tables, after warm steps, and the frames a step runs
  * --stream --sample-rate HZ : also the streamed resampler behind it (ctts_resample_stream_step, one launch): the same streams, each
                pushed what the scaler's step emits for 12 000 samples, converted 24000 -> HZ -- device time of one step, the same way

Synthetic weights, noise input (the kernels' work does not depend on the samples).  Prints one JSON line.  Not a bench.py leg.

    python tools/time_scale_probe.py [--reps 20] [--gemm f16] [--stream [--sample-rate 8000]]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import resample as RS, timescale as TS  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

SEG = 240000          # 10 s at 24 kHz
TOKENS = 469          # 256 (2 T - 1) = 239 872 samples


def _launch_ms(codec, n_seg, speed, reps):
    dev = codec.device
    off = np.arange(n_seg + 1, dtype=np.int64) * SEG
    num, den, off_out, path_off = TS.plan(speed, off)
    x = torch.rand(n_seg * SEG, device=dev) * 2 - 1
    y = torch.empty(int(off_out[-1]), dtype=torch.float32, device=dev)
    path = torch.empty(int(path_off[-1]), dtype=torch.int32, device=dev)
    tabs = [torch.from_numpy(t).to(dev) for t in (off, off_out, path_off)]
    win = codec._time_scale_window()
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        rc = codec.lib.ctts_time_scale_ragged(x.data_ptr(), tabs[0].data_ptr(), off.ctypes.data_as(C.c_void_p), y.data_ptr(), tabs[1].data_ptr(),
                                              off_out.ctypes.data_as(C.c_void_p), path.data_ptr(), tabs[2].data_ptr(),
                                              path_off.ctypes.data_as(C.c_void_p), n_seg, win.data_ptr(), num, den, st)
        assert rc == 0
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / reps, 3), int(path_off[1]) - 1


def _stream_step_ms(codec, n_streams, speed, reps, push=12000, warm=3):
    """device time of one step of `n_streams` streams, each pushed `push` samples, and the frames it runs per stream"""
    from chattts_amd import _lib
    dev = codec.device
    pool = codec._pool("time_scale")
    assert n_streams <= int(pool.buf["carry"].shape[0])
    x = torch.rand(n_streams * push, device=dev) * 2 - 1
    tabs, frames, n_out = [], [], 0
    for r in range(warm + reps):
        p = TS.stream_plan(speed, r * push, push, False)
        tab = np.zeros(n_streams, _lib.TS_STREAM)
        for i in range(n_streams):
            tab[i] = (i * push, push, r * push, -1, i * p["n_out"], i * p["n_path"], p["k_prev"], p["k_now"], i, r & 1, p["num"], p["den"], p["n_out"], 0)
        tabs.append((tab, torch.from_numpy(tab.view(np.uint8)).to(dev)))
        frames.append(p["k_now"] - p["k_prev"])
        n_out = max(n_out, n_streams * p["n_out"])
    y = torch.empty(n_out, dtype=torch.float32, device=dev)
    path = torch.empty(n_streams * (max(frames) + 1), dtype=torch.int32, device=dev)
    win = codec._time_scale_window()
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(r):
        tab, tab_d = tabs[r]
        rc = codec.lib.ctts_time_scale_stream_step(x.data_ptr(), x.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), n_streams, y.data_ptr(),
                                                   y.numel(), path.data_ptr(), path.numel(), pool.buf["carry"].data_ptr(), pool.buf["state"].data_ptr(),
                                                   int(pool.buf["carry"].shape[0]), win.data_ptr(), st)
        assert rc == 0, codec.lib.ctts_last_error()
    for r in range(warm):
        call(r)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(warm, warm + reps):
        call(r)
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / reps, 4), round(float(np.mean(frames[warm:])), 2)


def _resample_step_ms(codec, n_streams, speed, rate, reps, push=12000, warm=3):
    """device time of one step of `n_streams` resampler streams 24000 -> `rate`, each pushed the chunk the scaler's step at `speed` emits
    for `push` samples, and the samples a step emits per stream"""
    from chattts_amd import _lib
    dev = codec.device
    pool = codec._pool("resample")
    assert n_streams <= int(pool.buf["carry"].shape[0])
    L, M = RS.ratio(24000, rate)
    K = RS.geometry(L, M)[1]
    taps = codec._resample_taps(24000, rate)
    plans, pushed, emitted = [], 0, 0
    for r in range(warm + reps):
        n_in = TS.stream_plan(speed, r * push, push, False)["n_out"]
        p = RS.stream_plan(L, M, K, pushed, emitted, n_in, False)
        plans.append((n_in, pushed, p))
        pushed, emitted = pushed + n_in, p["emitted"]
    n_max, o_max = max(n for n, _, _ in plans), max(p["n_out"] for _, _, p in plans)
    x = torch.rand(n_streams * n_max, device=dev) * 2 - 1
    y = torch.empty(max(1, n_streams * o_max), dtype=torch.float32, device=dev)
    tabs = []
    for r, (n_in, pos, p) in enumerate(plans):
        tab = np.zeros(n_streams, _lib.RS_STREAM)
        for i in range(n_streams):
            tab[i] = (i * n_max, n_in, pos, -1, p["o_lo"], p["n_out"], i * o_max, i, r & 1, p["carry_in"], p["carry_out"], 0, 0)
        tabs.append((tab, torch.from_numpy(tab.view(np.uint8)).to(dev)))
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(r):
        tab, tab_d = tabs[r]
        rc = codec.lib.ctts_resample_stream_step(x.data_ptr(), x.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), n_streams, y.data_ptr(),
                                                 y.numel(), pool.buf["carry"].data_ptr(), int(pool.buf["carry"].shape[0]), taps.data_ptr(), L, M, K, st)
        assert rc == 0, codec.lib.ctts_last_error()
    for r in range(warm):
        call(r)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for r in range(warm, warm + reps):
        call(r)
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / reps, 4), round(float(np.mean([p["n_out"] for _, _, p in plans[warm:]])), 1)


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
    return round(float(np.median(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gemm", default="f16")
    ap.add_argument("--stream", action="store_true", help="the streamed scaler's step instead")
    ap.add_argument("--sample-rate", type=int, default=None, help="--stream: also the streamed resampler's step behind it, 24000 -> this rate")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_scale_probe needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    if a.stream:
        from chattts_amd.engine import CodecEngine
        codec = CodecEngine(sds["decoder"], sds["vocos"], dev)
        out = dict(metric="time_scale_stream_probe", push_samples=12000, reps=a.reps, step_ms={}, frames_per_step={}, us_per_frame={})
        for n in (1, 8, 64):
            for speed in (0.5, 1.25, 2.0):
                ms, frames = _stream_step_ms(codec, n, speed, a.reps)
                out["step_ms"][f"{n}x@{speed}"] = ms
                out["frames_per_step"][str(speed)] = frames
                out["us_per_frame"][f"{n}x@{speed}"] = round(1e3 * ms / frames, 2)
                if a.sample_rate is not None and a.sample_rate != 24000:
                    ms, n_out = _resample_step_ms(codec, n, speed, a.sample_rate, a.reps)
                    out.setdefault("sample_rate", a.sample_rate)
                    out.setdefault("resample_step_ms", {})[f"{n}x@{speed}"] = ms
                    out.setdefault("resampled_per_step", {})[str(speed)] = n_out
        print(json.dumps(out))
        return
    chat = Chat()
    assert chat.load(state_dicts={k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}, device=dev, dtype="f32", codec_gemm=a.gemm)
    codec = chat.codec
    out = dict(metric="time_scale_probe", segment_samples=SEG, tokens_per_row=TOKENS, codec_gemm=a.gemm, reps=a.reps, launch_ms={}, frames={},
               decode_to_pcm16_ms={})
    for n_seg in (1, 8, 64):
        for speed in (0.5, 1.25, 2.0):
            ms, frames = _launch_ms(codec, n_seg, speed, a.reps)
            out["launch_ms"][f"{n_seg}x@{speed}"] = ms
            out["frames"][str(speed)] = frames
    rs = np.random.RandomState(3)
    for n_rows in (1, 8, 64):
        rows = [torch.from_numpy(rs.standard_normal((TOKENS, 768)).astype(np.float32) * 0.5).to(dev) for _ in range(n_rows)]
        r = {"speed_1": _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True), max(3, a.reps // 4))}
        for speed in (0.5, 1.25, 2.0):
            r[f"speed_{speed}"] = _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True, speed=speed), max(3, a.reps // 4))
        out["decode_to_pcm16_ms"][f"{n_rows}_rows"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()

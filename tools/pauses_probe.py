"""What the device pause stage costs (csrc/pauses.hip, ctts_trim_pauses_ragged), beside the decode it follows:

  * call      : 1 and 64 segments of 10 s (240 000 samples at 24 kHz) under the default spec -- device time of one call (its four
                launches: activity, plan, offsets, copy), from events around `--reps` back-to-back calls on pre-uploaded tables, after
                warm calls; the records and the output of the first segments are checked against the NumPy twin, bit for bit
  * bytes     : what the activity pass reads (one float32 per sample) and what the copy pass moves (one float32 read and one written
                per KEPT sample) -- against the time of the whole call here; the four launches' own times come from a kernel trace of
                `--trace` (the 64-segment calls alone, nothing else on the device):
                    rocprofv3 --kernel-trace --stats -- python tools/pauses_probe.py --trace
  * copy      : the wall time of the call's one device-to-host copy (the output offsets and the records), on an idle stream
  * decode    : `Chat.decode_to_pcm16(rows, ragged=True)` on 64 rows of 469 tokens (10 s each) without `pauses=` and with it, same rows;
                wall time including the host side.  `--root DIR` imports the package from another checkout (the parent commit, built
                there), so that the two trees can be timed alternately in one session

  * --stream  : the pause STREAMS (ctts_trim_pauses_stream_step) instead: 1 / 8 / 64 streams at 24 kHz under the default spec, each
                pushed 12 000 samples per step (half a second, a served stream's chunk) of the same stepped signal, 20 steps.  Wall
                time of `CodecEngine.trim_pauses_stream_step` -- the upload of the table, the three launches and the one copy of the
                counts it waits for -- and the device time between events around it; stream 0's chunks are checked against the
                NumPy twin, bit for bit.  `--out FILE`: the table as markdown

Synthetic weights, noise input under a stepped envelope: quiet steps at -70 dBFS, about half of the frames, in runs of 0.1 .. 1.5 s.
Prints one JSON line.  Not a bench.py leg.

    python tools/pauses_probe.py [--reps 20] [--gemm f16] [--trace] [--root DIR] [--decode-only]
    python tools/pauses_probe.py --stream [--rounds 5] [--out profiles/pauses_stream_probe.md]
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

SEG = 240000          # 10 s at 24 kHz
TOKENS = 469          # 256 (2 T - 1) = 239 872 samples
F = 240


def _signal(n_seg):
    r = np.random.default_rng(5)
    parts = []
    for _ in range(n_seg):
        env, loud = [], True
        while len(env) < SEG // F:
            m = int(r.integers(10, 150))
            env += [0.3 if loud else 10.0 ** -3.5] * m
            loud = not loud
        parts.append(np.repeat(np.array(env[: SEG // F]), F))
    env = np.concatenate(parts)
    return (r.uniform(-1, 1, n_seg * SEG) * env).astype(np.float32)


def _call_ms(codec, PA, n_seg, reps, check=2):
    """device time of one call over n_seg segments of 10 s; the first `check` segments against the twin"""
    dev = codec.device
    host = _signal(n_seg)
    x = torch.from_numpy(host).to(dev)
    y = torch.empty_like(x)
    tb = PA.tables(np.arange(n_seg + 1, dtype=np.int64) * SEG, 24000, True)
    off, rows, fbase, fade = tb["off"], tb["rows"], tb["fbase"], tb["fade"]
    tabs = [torch.from_numpy(t).to(dev) for t in (off, fbase, rows.reshape(-1), fade)]
    res_bytes = 8 * (n_seg + 1) + 4 * PA.REC * n_seg
    res = torch.empty(-(-res_bytes // 16) * 16, dtype=torch.uint8, device=dev)
    scratch = torch.empty(tb["scratch"], dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call():
        rc = codec.lib.ctts_trim_pauses_ragged(x.data_ptr(), y.data_ptr(), tabs[0].data_ptr(), vp(off), tabs[1].data_ptr(), vp(fbase), tabs[2].data_ptr(),
                                               vp(rows), n_seg, tabs[3].data_ptr(), int(fade.size), res.data_ptr(), res.data_ptr() + 8 * (n_seg + 1),
                                               scratch.data_ptr(), tb["scratch"], st)
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
    ts = []
    for _ in range(max(5, reps)):                   # the one copy of a call, on an idle stream
        t0 = time.perf_counter()
        h = res[:res_bytes].cpu()
        ts.append((time.perf_counter() - t0) * 1e6)
    h = h.numpy()
    off_out = h[: 8 * (n_seg + 1)].view(np.int64)
    rec = h[8 * (n_seg + 1):].view(np.int32).reshape(n_seg, PA.REC)
    out = y[: int(off_out[-1])].cpu().numpy()
    for i in range(min(check, n_seg)):
        yt, rt = PA.apply(host[i * SEG: (i + 1) * SEG], 24000, True)
        assert rec[i].tolist() == rt.tolist() and out[off_out[i]: off_out[i + 1]].tobytes() == yt.tobytes(), i
    return round(ms, 4), int(off_out[-1]), round(float(np.median(ts)), 1), int(rec[:, 5].sum())


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


CHUNK, STEPS = 12000, 20          # samples per push of the stream probe; pushes per stream


def _stream(codec, PA, rounds):
    """step time of 1 / 8 / 64 pause streams: per B the wall and device times of a step in ms (median, min, max over steps and rounds)"""
    dev = codec.device
    res = {}
    for B in (1, 8, 64):
        host = _signal(B)[: B * SEG].reshape(B, SEG)
        x = torch.from_numpy(np.ascontiguousarray(host[:, : CHUNK * STEPS])).to(dev)
        wall, devt, out_n, held = [], [], 0, 0
        for r in range(rounds + 1):                     # round 0 warms up
            hs = [codec.trim_pauses_stream_open(24000, True) for _ in range(B)]
            tw = PA.StreamPauses(24000, True) if r == 0 else None
            try:
                for k in range(STEPS):
                    pushes = [(h, i * CHUNK * STEPS + k * CHUNK, CHUNK, k == STEPS - 1) for i, h in enumerate(hs)]
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    a.record()
                    y, off = codec.trim_pauses_stream_step(x.view(-1), pushes)
                    b.record()
                    b.synchronize()
                    t1 = time.perf_counter()
                    if r:
                        wall.append((t1 - t0) * 1e3)
                        devt.append(a.elapsed_time(b))
                        out_n += int(off[-1])
                        held = max(held, max(codec.trim_pauses_stream_stats(h)["held"] for h in hs) if k < STEPS - 1 else 0)
                    else:
                        want = tw.push(host[0, k * CHUNK: (k + 1) * CHUNK], k == STEPS - 1)
                        assert y[: int(off[1])].cpu().numpy().tobytes() == want.tobytes(), (B, k)
            finally:
                for h in hs:
                    codec.trim_pauses_stream_close(h)
        f = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))
        res[B] = dict(wall_ms=f(wall), device_ms=f(devt), samples_in=B * CHUNK * STEPS, samples_out=out_n // rounds, held_max=held)
    return res


def _stream_markdown(res, rounds) -> str:
    rows = ["# Pause streams: step time (tools/pauses_probe.py --stream)", "",
            f"{CHUNK} samples at 24 kHz per stream and step, {STEPS} steps, default spec; median (min .. max) over the steps of {rounds} rounds. "
            "`wall` is `CodecEngine.trim_pauses_stream_step` as a caller sees it (table upload, three launches, the one copy of the counts and "
            "its wait); `device` is the time between events around it.", "",
            "| streams | wall, ms | device, ms | samples in | samples out | most frames held |", "|---|---|---|---|---|---|"]
    f = lambda d: f"{d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f})"
    for B, d in res.items():
        rows.append(f"| {B} | {f(d['wall_ms'])} | {f(d['device_ms'])} | {d['samples_in']} | {d['samples_out']} | {d['held_max']} |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gemm", default="f16")
    ap.add_argument("--trace", action="store_true", help="only the 64-segment calls: the run to put under a kernel trace")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import chattts_amd from")
    ap.add_argument("--decode-only", action="store_true", help="only the 64-row decode without the keyword (any checkout has it)")
    ap.add_argument("--stream", action="store_true", help="time the pause streams instead")
    ap.add_argument("--rounds", type=int, default=5, help="with --stream: timed rounds of 20 steps")
    ap.add_argument("--out", default=None, help="with --stream: the markdown table goes here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pauses_probe needs a GPU: nothing here can be timed without one")
    sys.path.insert(0, os.path.abspath(a.root))
    from chattts_amd.weights import synthetic_all
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    if a.stream:
        from chattts_amd import pauses as PA
        from chattts_amd.engine import CodecEngine
        res = _stream(CodecEngine(sds["decoder"], sds["vocos"], dev), PA, a.rounds)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(_stream_markdown(res, a.rounds))
        print(json.dumps(dict(metric="pauses_stream_probe", rounds=a.rounds, chunk=CHUNK, steps=STEPS, streams=res)))
        return
    if a.trace:
        from chattts_amd import pauses as PA
        from chattts_amd.engine import CodecEngine
        codec = CodecEngine(sds["decoder"], sds["vocos"], dev)
        ms, n_out, _, _ = _call_ms(codec, PA, 64, a.reps, check=0)
        print(json.dumps(dict(metric="pauses_probe_trace", segments=64, call_ms=ms, reps=a.reps, samples_in=64 * SEG, samples_out=n_out)))
        return
    from chattts_amd.core import Chat
    chat = Chat()
    assert chat.load(state_dicts={k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}, device=dev, dtype="f32", codec_gemm=a.gemm)
    rs = np.random.RandomState(3)
    rows = [torch.from_numpy(rs.standard_normal((TOKENS, 768)).astype(np.float32) * 0.5).to(dev) for _ in range(64)]
    reps = max(5, a.reps // 2)
    out = dict(metric="pauses_probe", root=os.path.abspath(a.root), segment_samples=SEG, tokens_per_row=TOKENS, codec_gemm=a.gemm, reps=a.reps,
               decode_to_pcm16_ms={})
    legs = [("off", {}), ("off_again", {})]
    if not a.decode_only:
        from chattts_amd import pauses as PA
        out.update(call_ms={}, samples_out={}, offsets_copy_us={}, runs_shortened={}, activity_pass={}, copy_pass={})
        for n_seg in (1, 64):
            ms, n_out, copy_us, runs = _call_ms(chat.codec, PA, n_seg, a.reps)
            k = f"{n_seg}x"
            out["call_ms"][k], out["samples_out"][k], out["offsets_copy_us"][k], out["runs_shortened"][k] = ms, n_out, copy_us, runs
            out["activity_pass"][k] = dict(bytes=4 * n_seg * SEG, us_at_8TBps=round(4 * n_seg * SEG / 8e12 * 1e6, 3))
            out["copy_pass"][k] = dict(bytes=8 * n_out, us_at_8TBps=round(8 * n_out / 8e12 * 1e6, 3))
        legs = [("off", {}), ("pauses", {"pauses": True}), ("off_again", {})]
    for name, kw in legs:
        med, lo, hi = _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True, **kw), reps)
        out["decode_to_pcm16_ms"][name] = dict(median=med, min=lo, max=hi)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What the dynamic range compressor costs (csrc/compressor.hip, ctts_compress_ragged, behind CodecEngine.compress), next to the nearest
existing stage, the look-ahead peak limiter, on the same packs in the same run.  Needs a GPU; writes profiles/compressor_probe.md.

    python tools/compressor_probe.py [--reps 20] [--rounds 5] [--out profiles/compressor_probe.md] [--stream]

  packs         64 rows of 10 s at 24 kHz (15.4 M samples) and at 8 kHz (5.1 M): noise under an envelope that changes every 50 ms between
                -50, -26 and -10 dBFS, so about two thirds of the blocks lie over the default knee -- the compressor's slow path on most
                tiles.  The limiter sees the same samples at unity gain (none over its threshold: its fast path, the cheapest it gets).
  timing        the C entry points on preallocated buffers (no allocation, no upload in the loop), device events around `reps` calls
                back to back, the median of `rounds`; per call.  Into a buffer of its own (in place, every call would compress what the
                one before it left, and the pack would soon lie under the knee).
  traffic       the pack read once by each launch and written once: 12 bytes per sample for the compressor (the peak launch reads 4,
                the apply launch reads 4 and writes 4) plus the block gains; the achieved rate is that over the time.
  per launch    the apply launch is not callable alone, so the split comes from two variant calls: with a table of ones, in place, the
                peak launch does all its work and every apply workgroup leaves at once (no block under 1, nothing to copy): that is
                the peak launch plus the floor; with every segment copied through in place (table index -1) both launches leave at
                once: the floor of a memset and two launches.  apply = full - peak.
  --stream      instead: ONE step of 64 compressor streams with pushes of 100 ms at 24 kHz (ctts_compress_stream_step, mid-stream: five
                pushes have gone before, so the raw carry and the history of the hold are live), next to the one-shot call over the same
                64 x 100 ms as 64 segments -- the yardstick: the step does the same work and also reads its second sources and writes
                the next carry and history.  The same descriptors are launched again and again (a step reads one half of a slot and
                writes the other, so a repeated step is the same step); the section replaces the file's `## stream` section."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import compressor as CP  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

N_SEG, SECONDS = 64, 10


def _pack(fs: int) -> np.ndarray:
    r = np.random.default_rng(5)
    n = N_SEG * SECONDS * fs
    step = fs // 20
    env = np.repeat(r.choice([0.003, 0.05, 0.3], size=n // step), step)
    return (r.uniform(-1, 1, n) * env).astype(np.float32)


def _time(fn, reps: int, rounds: int) -> float:
    """ms per call: device events around `reps` calls, the median of `rounds`"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def _measure(codec, fs: int, reps: int, rounds: int) -> dict:
    dev = codec.device
    lib = codec.lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x_h = _pack(fs)
    n = len(x_h)
    off = np.arange(N_SEG + 1, dtype=np.int64) * (n // N_SEG)
    off, rt, par, tabs, _ = CP.tables(n, True, off, fs)
    thru = par.copy()
    thru[:, 2] = -1
    x = up(x_h)
    y = torch.empty_like(x)
    ones_h = np.ones_like(tabs)
    ones_d = up(ones_h)
    off_d, rt_d, par_d, thru_d, tabs_d = up(off), up(rt), up(par), up(thru), up(tabs)
    sb = int(lib.ctts_compress_ragged_scratch_bytes(vp(off), N_SEG))
    stats = torch.empty(16 * N_SEG, dtype=torch.uint8, device=dev)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def comp(p_d, p_h, out, t_d=tabs_d, t_h=tabs):
        def call():
            rc = lib.ctts_compress_ragged(x.data_ptr(), out.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, rt_d.data_ptr(), vp(rt), p_d.data_ptr(), vp(p_h),
                                          t_d.data_ptr(), vp(t_h), int(tabs.shape[0]), stats.data_ptr(), scratch.data_ptr(), sb, st)
            assert rc == 0, lib.ctts_last_error()
        return call
    gains = torch.ones(N_SEG, dtype=torch.float32, device=dev)
    sb_l = int(lib.ctts_peak_limit_ragged_scratch_bytes(vp(off), N_SEG))
    scratch_l = torch.empty(sb_l, dtype=torch.uint8, device=dev)

    def lim():
        rc = lib.ctts_peak_limit_ragged(x.data_ptr(), y.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, rt_d.data_ptr(), vp(rt), gains.data_ptr(),
                                        stats.data_ptr(), scratch_l.data_ptr(), sb_l, st)
        assert rc == 0, lib.ctts_last_error()
    _, rec = codec.compress(x, True, offsets=off, rates=fs, return_stats=True)
    t_lim = _time(lim, reps, rounds)
    t_thru = _time(comp(thru_d, thru, x), reps, rounds)
    t_peak = _time(comp(par_d, par, x, ones_d, ones_h), reps, rounds)
    t_comp = _time(comp(par_d, par, y), reps, rounds)
    nb = n // (fs // 1000)
    traffic = 12 * n + 8 * nb
    return dict(fs=fs, n=n, ms_compress=t_comp, ms_through=t_thru, ms_peak=t_peak, ms_limit=t_lim, gbps=traffic / t_comp / 1e6, gbps_limit=8 * n / t_lim / 1e6,
                blocks_under=int(rec["n_blocks"].sum()), blocks=nb, touched=int(rec["n_touched"].sum()))


def _measure_stream(codec, reps: int, rounds: int, fs: int = 24000, ms: int = 100, before: int = 5) -> dict:
    dev, lib = codec.device, codec.lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    push, per = ms * fs // 1000, (before + 1) * ms * fs // 1000
    r = np.random.default_rng(5)
    env = np.repeat(r.choice([0.003, 0.05, 0.3], size=N_SEG * per // (fs // 20)), fs // 20)
    x_h = (r.uniform(-1, 1, N_SEG * per) * env).astype(np.float32)
    x = up(x_h)
    hs = [codec.compress_stream_open(fs, True) for _ in range(N_SEG)]
    try:
        for k in range(before):
            codec.compress_stream_step(x, [(h, i * per + k * push, push, False) for i, h in enumerate(hs)])
        tab, tabs_h, _, n_new = codec._cp_descriptors([(h, i * per + before * push, push, False) for i, h in enumerate(hs)])
        o = np.zeros(N_SEG + 1, np.int64)
        np.cumsum(tab["n_out"], out=o[1:])
        tab["out_off"] = o[:-1]
        pool = codec._pool("compress")
        both = up(np.concatenate([tabs_h.view(np.uint8).reshape(-1), tab.view(np.uint8)]))
        sb = int(lib.ctts_compress_stream_scratch_bytes(n_new))
        work = torch.empty(sb, dtype=torch.uint8, device=dev)
        y = torch.empty(int(o[-1]), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def step():
            rc = lib.ctts_compress_stream_step(x.data_ptr(), x.numel(), both.data_ptr() + tabs_h.nbytes, vp(tab), N_SEG, both.data_ptr(), vp(tabs_h),
                                               int(tabs_h.shape[0]), y.data_ptr(), y.numel(), pool.buf["carry"].data_ptr(), pool.buf["hist"].data_ptr(),
                                               pool.buf["stats"].data_ptr(), pool.slots, work.data_ptr(), sb, st)
            assert rc == 0, lib.ctts_last_error()
        t_step = _time(step, reps, rounds)
        # the yardstick: the same 64 x 100 ms as 64 segments of one one-shot call
        seg = np.concatenate([x_h[i * per + before * push: i * per + (before + 1) * push] for i in range(N_SEG)])
        off, rt, par, tabs, _ = CP.tables(len(seg), True, np.arange(N_SEG + 1, dtype=np.int64) * push, fs)
        xs, ys = up(seg), torch.empty(len(seg), dtype=torch.float32, device=dev)
        off_d, rt_d, par_d, tabs_d = up(off), up(rt), up(par), up(tabs)
        sb1 = int(lib.ctts_compress_ragged_scratch_bytes(vp(off), N_SEG))
        stats, scratch = torch.empty(16 * N_SEG, dtype=torch.uint8, device=dev), torch.empty(sb1, dtype=torch.uint8, device=dev)

        def one():
            rc = lib.ctts_compress_ragged(xs.data_ptr(), ys.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, rt_d.data_ptr(), vp(rt), par_d.data_ptr(), vp(par),
                                          tabs_d.data_ptr(), vp(tabs), int(tabs.shape[0]), stats.data_ptr(), scratch.data_ptr(), sb1, st)
            assert rc == 0, lib.ctts_last_error()
        t_one = _time(one, reps, rounds)
        t_engine = _time(lambda: codec.compress_stream_step(x, [(h, i * per + before * push, 0, False) for i, h in enumerate(hs)]), reps, rounds)
        return dict(fs=fs, ms=ms, push=push, ms_step=t_step, ms_one=t_one, ms_idle_engine=t_engine, carry=int(tab["c_in"].max()), hist=int(tab["h_in"].max()),
                    emitted=int(o[-1]))
    finally:
        for h in hs:
            codec.compress_stream_close(h)


def _stream_section(codec, a) -> str:
    r = _measure_stream(codec, a.reps, a.rounds)
    return "\n".join([
        "## stream", "",
        f"{torch.cuda.get_device_name(0)}; ONE step of {N_SEG} streams, pushes of {r['ms']} ms at {r['fs']} Hz ({r['push']} samples each, {r['emitted']} emitted), "
        f"mid-stream: each slot carries {r['carry']} raw samples and {r['hist']} block gains in; the C entry points on preallocated buffers; device events "
        f"around {a.reps} calls, median of {a.rounds} rounds.", "",
        "| what | launches | ms per call |", "|---|---|---|",
        f"| `ctts_compress_stream_step`, {N_SEG} streams x {r['ms']} ms | 2 kernels | {r['ms_step']:.4f} |",
        f"| `ctts_compress_ragged`, the same {N_SEG} x {r['ms']} ms as {N_SEG} segments (the yardstick) | a memset node and 2 kernels | {r['ms_one']:.4f} |",
        f"| `CodecEngine.compress_stream_step`, {N_SEG} empty pushes (planning, one upload, the scratch, 1 kernel) | 1 kernel | {r['ms_idle_engine']:.4f} |",
        "", f"step / one-shot = {r['ms_step'] / r['ms_one']:.2f}", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressor_probe.md"))
    ap.add_argument("--stream", action="store_true", help="measure one step of 64 streams instead, and replace the file's `## stream` section")
    a = ap.parse_args()
    from chattts_amd.engine import CodecEngine
    dev = torch.device("cuda:0")
    w = synthetic_all()
    codec = CodecEngine(w["decoder"], w["vocos"], dev)
    if a.stream:
        text = _stream_section(codec, a)
        old = open(a.out).read() if os.path.exists(a.out) else "# compressor probe\n"
        head = old.split("\n## stream\n")[0].rstrip("\n")
        with open(a.out, "w") as f:
            f.write(head + "\n\n" + text)
        print(text)
        return
    rows = [_measure(codec, fs, a.reps, a.rounds) for fs in (24000, 8000)]
    lines = ["# compressor probe", "",
             f"{torch.cuda.get_device_name(0)}; {N_SEG} rows of {SECONDS} s, x into y, the C entry points on preallocated buffers; device events around "
             f"{a.reps} calls, median of {a.rounds} rounds.  Launches per call: a memset node and 2 kernels (the limiter: 4 kernels).", "",
             "| rate | samples | compress ms | GB/s over 12 B/sample + 8 B/block | peak launch + floor ms | floor ms | peak_limit ms (fast path) | its GB/s over 8 B/sample | blocks under the curve | samples touched |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['fs']} | {r['n']} | {r['ms_compress']:.4f} | {r['gbps']:.0f} | {r['ms_peak']:.4f} | {r['ms_through']:.4f} | {r['ms_limit']:.4f} | {r['gbps_limit']:.0f} | "
                     f"{r['blocks_under']} of {r['blocks']} | {r['touched']} |")
    lines += ["", "`floor`: every segment copied through in place (table index -1): a memset and two launches that leave at once.  `peak launch + floor`: a "
              "table of ones, in place: the peak launch in full, every apply workgroup leaves at once.  apply = compress - (peak launch + floor) + floor."]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

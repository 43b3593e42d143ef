"""What the look-ahead peak limiter does to the level and what it costs (csrc/limiter.hip, ctts_peak_limit_ragged, behind
ctts_loudness_limited_ragged):

  * level     : every signal of tests/loudness_cases.py at 8000 and 24000 Hz towards -5 LUFS, with the ceiling alone
                (`loudness_normalize`) and with the limiter (`loudness_normalize(limiter=True)`): the loudness the result HAS -- the
                existing stage run over y with no target -- and the limiter's record.  Reported, not asserted: the gates make it
                non-monotone.  The same for a synthesised batch (64 rows of 64 tokens through the ragged decoder).
  * stage     : 64 segments of 10 s (240 000 samples at 24 kHz), already on the device, tables pre-uploaded -- device time of one call
                from events around `--reps` back-to-back calls, the three configurations alternated over `--rounds` rounds, median
                (min .. max) of the rounds:  `loudness_noise` the parent's ctts_loudness_normalize_ragged, in place, every segment
                towards the loudness it has (gain 1);  `exit` ctts_loudness_limited_ragged + ctts_peak_limit_ragged on the same pack and
                targets, in place: no sample is over the threshold, every tile leaves early;  `loudness_bursts` / `dense` the same
                pair towards -5 LUFS on a pack of sine bursts, out of place: every tile computes its gain curve.  The limiter call
                alone on both packs as well.

  * --stream  : the limiter of STREAMS (ctts_peak_limit_stream_step) instead: 1 / 8 / 64 streams, each pushed 12 000 samples per step
                (half a second at 24 kHz, a served stream's chunk), `quiet` (noise under 0.3: every tile leaves early) and `loud` (the
                same noise at 4x: every tile computes its curve).  The descriptors of `--reps` consecutive steps are uploaded first;
                device time of one step from events around those steps, median (min .. max) of `--rounds` rounds, alternated with the
                one-shot ctts_peak_limit_ragged on the same samples (as many segments of 12 000) and with the window decode the step
                rides behind (`decode_windows` of as many 12 000-sample chunks, 16 bit).  Writes a markdown table to `--out`.

Noise under a stepped envelope; synthetic weights.  Prints one JSON line.  Not a bench.py leg.

    python tools/limiter_probe.py [--reps 20] [--rounds 7] [--stream --out profiles/limiter_stream_probe.md]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import limiter as LM  # noqa: E402
from chattts_amd import loudness as LN  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

SEG = 240000          # 10 s at 24 kHz
N_SEG = 64
TARGET = -5.0


def _level(codec, xs, rates, target):
    """the pack of xs towards `target`, ceiling alone and with the limiter -> per segment: L, both gains, both achieved L, the record"""
    dev = codec.device
    off = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    y0, st0 = codec.loudness_normalize(x, target, offsets=off, rates=rates, return_stats=True)
    y1, st1, ls = codec.loudness_normalize(x, target, offsets=off, rates=rates, return_stats=True, limiter=True)
    a0 = codec.loudness_normalize(y0, None, offsets=off, rates=rates, return_stats=True)[1]["L"]
    a1 = codec.loudness_normalize(y1, None, offsets=off, rates=rates, return_stats=True)[1]["L"]
    peak1 = [float(y1[off[i]: off[i + 1]].abs().max()) for i in range(len(xs))]
    r3 = lambda v: None if not np.isfinite(v) else round(float(v), 3)
    return [dict(L=r3(st0["L"][i]), g_ceiling=round(float(st0["g32"][i]), 4), bound=int(st0["bound"][i]), g_limiter=round(float(st1["g32"][i]), 4),
                 L_ceiling=r3(a0[i]), L_limiter=r3(a1[i]), peak=round(peak1[i], 6), min_gain=round(float(ls["min_gain"][i]), 4),
                 n_over=int(ls["n_over"][i]), n_touched=int(ls["n_touched"][i]), n=int(off[i + 1] - off[i])) for i in range(len(xs))]


def _packs():
    r = np.random.default_rng(5)
    env = np.repeat(r.choice([0.003, 0.05, 0.3], size=N_SEG * SEG // 1200), 1200)
    noise = (r.uniform(-1, 1, N_SEG * SEG) * env).astype(np.float32)
    t = np.arange(SEG) / 24000.0
    bursts = np.tile((np.sin(2 * np.pi * 997 * t) * (np.arange(SEG) % 2400 < 240)).astype(np.float32), N_SEG)
    return noise, bursts


def _stage(codec, reps, rounds):
    dev = codec.device
    noise, bursts = _packs()
    off = np.arange(N_SEG + 1, dtype=np.int64) * SEG
    grp = np.arange(N_SEG + 1, dtype=np.int32)
    ridx = np.zeros(N_SEG, np.int32)
    hz = np.full(N_SEG, 24000, np.int32)
    lim = np.ones(N_SEG, np.int32)
    coef_d, coef_h, _ = codec._loudness_coef([24000])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    up = lambda a: torch.from_numpy(a).to(dev)
    off_d, grp_d, ridx_d, hz_d, lim_d = up(off), up(grp), up(ridx), up(hz), up(lim)
    sb_l = int(codec.lib.ctts_loudness_normalize_ragged_scratch_bytes(vp(off), N_SEG))
    sb_m = int(codec.lib.ctts_peak_limit_ragged_scratch_bytes(vp(off), N_SEG))
    stats = torch.empty(LN.STATS.itemsize * N_SEG, dtype=torch.uint8, device=dev)
    lstats = torch.empty(LM.STATS.itemsize * N_SEG, dtype=torch.uint8, device=dev)
    scr_l = torch.empty(sb_l, dtype=torch.uint8, device=dev)
    scr_m = torch.empty(sb_m, dtype=torch.uint8, device=dev)
    gains = torch.ones(N_SEG, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    xs = {"noise": up(noise), "bursts": up(bursts)}
    y = torch.empty_like(xs["noise"])
    # every segment towards the loudness it has: the gain is 1, so the calls can run in place (as the pipeline runs them) any number of
    # times on the same samples, and the noise's peak of 0.3 stays under the threshold
    L = codec.loudness_normalize(xs["noise"], None, offsets=off, return_stats=True)[1]["L"]
    assert L.min() >= -40.0 and L.max() <= -5.0
    tg = {"quiet": L.astype(np.float64).copy(), "loud": np.full(N_SEG, TARGET)}
    tg_d = {k: up(v) for k, v in tg.items()}

    def loudness(x, t, y):
        rc = codec.lib.ctts_loudness_normalize_ragged(x.data_ptr(), y.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, ridx_d.data_ptr(), vp(ridx),
                                                      coef_d.data_ptr(), vp(coef_h), 1, grp_d.data_ptr(), vp(grp), N_SEG, tg_d[t].data_ptr(), vp(tg[t]),
                                                      stats.data_ptr(), scr_l.data_ptr(), sb_l, st)
        assert rc == 0, codec.lib.ctts_last_error()

    def limit(x, out):
        rc = codec.lib.ctts_peak_limit_ragged(x.data_ptr(), out.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, hz_d.data_ptr(), vp(hz), gains.data_ptr(),
                                              lstats.data_ptr(), scr_m.data_ptr(), sb_m, st)
        assert rc == 0, codec.lib.ctts_last_error()

    def limited(x, t, y):
        rc = codec.lib.ctts_loudness_limited_ragged(x.data_ptr(), y.data_ptr(), off_d.data_ptr(), vp(off), N_SEG, ridx_d.data_ptr(), vp(ridx),
                                                    coef_d.data_ptr(), vp(coef_h), 1, grp_d.data_ptr(), vp(grp), N_SEG, tg_d[t].data_ptr(), vp(tg[t]),
                                                    lim_d.data_ptr(), vp(lim), gains.data_ptr(), stats.data_ptr(), scr_l.data_ptr(), sb_l, st)
        assert rc == 0, codec.lib.ctts_last_error()
        limit(y, y)

    z = xs["noise"]
    cfgs = {"loudness_noise": lambda: loudness(z, "quiet", z), "exit": lambda: limited(z, "quiet", z),
            "loudness_bursts": lambda: loudness(xs["bursts"], "loud", y), "dense": lambda: limited(xs["bursts"], "loud", y)}
    recs = {}
    for name in ("exit", "dense"):                    # warm, and what the limiter did in each configuration
        for _ in range(3):
            cfgs[name]()
        torch.cuda.synchronize()
        r = lstats.cpu().numpy().view(LM.STATS)
        recs[name] = dict(n_over=int(r["n_over"].sum()), n_touched=int(r["n_touched"].sum()), min_gain=round(float(r["min_gain"].min()), 4),
                          g32=[round(float(r["g32"].min()), 4), round(float(r["g32"].max()), 4)], samples=N_SEG * SEG)
    cfgs["limiter_alone_exit"] = lambda: limit(xs["noise"], y)           # gains as the last `dense` call left them are reset first
    cfgs["limiter_alone_dense"] = lambda: limit(xs["bursts"], y)
    times = {k: [] for k in cfgs}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, fn in cfgs.items():
            if name == "limiter_alone_exit":
                gains.fill_(1.0)
            if name == "limiter_alone_dense":
                gains.fill_(2.5)
            fn()
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / reps)
    ms = {k: dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4)) for k, v in times.items()}
    assert z.cpu().numpy().tobytes() == noise.tobytes(), "the in-place calls at gain 1 changed the samples"
    return dict(segments=N_SEG, segment_samples=SEG, records=recs, call_ms=ms)


CHUNK = 12000         # samples per push of the stream probe


def _stream(codec, reps, rounds):
    """step time of 1 / 8 / 64 limiter streams, quiet and loud, against the one-shot limiter on the same samples and the window decode"""
    from chattts_amd import _lib
    dev = codec.device
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = torch.cuda.current_stream(dev).cuda_stream
    r = np.random.default_rng(5)
    out = {}
    for B in (1, 8, 64):
        env = np.repeat(r.choice([0.003, 0.05, 0.3], size=B * CHUNK // 1200), 1200)
        x = torch.from_numpy((r.uniform(-1, 1, B * CHUNK) * env).astype(np.float32)).to(dev)
        y = torch.empty_like(x)
        hs = [codec.peak_limit_stream_open(24000) for _ in range(B)]
        pool = codec._pool("limiter")
        W = 240
        # step k of every stream: the same B x CHUNK samples again, at position k * CHUNK (k = 0 emits 2 W fewer: it is the warm-up)
        tabs = []
        for k in range(reps + 1):
            tab = np.zeros(B, _lib.LM_STREAM)
            for i, h in enumerate(hs):
                p = LM.stream_plan(W, k * CHUNK, max(0, k * CHUNK - 2 * W), CHUNK, False)
                tab[i] = (i * CHUNK, CHUNK, k * CHUNK, -1, p["e_lo"], p["n_out"], i * CHUNK, h, k & 1, p["carry_in"], p["carry_out"], 24000, 1.0)
            tabs.append(tab)
        tabs_d = [torch.from_numpy(t.view(np.uint8)).to(dev) for t in tabs]
        off = np.arange(B + 1, dtype=np.int64) * CHUNK
        hz = np.full(B, 24000, np.int32)
        off_d, hz_d = torch.from_numpy(off).to(dev), torch.from_numpy(hz).to(dev)
        gains = torch.ones(B, dtype=torch.float32, device=dev)
        sb = int(codec.lib.ctts_peak_limit_ragged_scratch_bytes(vp(off), B))
        scr = torch.empty(sb, dtype=torch.uint8, device=dev)
        lstats = torch.empty(LM.STATS.itemsize * B, dtype=torch.uint8, device=dev)
        store = torch.from_numpy(np.random.RandomState(3).standard_normal((B, 64, 768)).astype(np.float32) * 0.5).to(dev)
        wins = [(i, 48, 0, CHUNK, False) for i in range(B)]

        def steps(gain):
            for k in range(reps + 1):
                tabs[k]["gain"] = gain
            for t, td in zip(tabs, tabs_d):
                td.copy_(torch.from_numpy(t.view(np.uint8)))

            def run(lo=1):
                for k in range(lo, reps + 1):
                    rc = codec.lib.ctts_peak_limit_stream_step(x.data_ptr(), x.numel(), tabs_d[k].data_ptr(), vp(tabs[k]), B, y.data_ptr(), y.numel(),
                                                               pool.buf["carry"].data_ptr(), pool.buf["stats"].data_ptr(), int(pool.buf["carry"].shape[0]), st)
                    assert rc == 0, codec.lib.ctts_last_error()
            return run

        def one_shot(gain):
            def run():
                for _ in range(reps):
                    rc = codec.lib.ctts_peak_limit_ragged(x.data_ptr(), y.data_ptr(), off_d.data_ptr(), vp(off), B, hz_d.data_ptr(), vp(hz), gains.data_ptr(),
                                                          lstats.data_ptr(), scr.data_ptr(), sb, st)
                    assert rc == 0, codec.lib.ctts_last_error()
            return run

        def decode():
            for _ in range(reps):
                codec.decode_windows(store, wins)
        res = {}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for name, gain in (("quiet", 1.0), ("loud", 4.0)):
            run_s, run_o = steps(np.float32(gain)), one_shot(gain)
            gains.fill_(gain)
            run_s(0)                                       # warm: step 0 included, it resets the records
            run_o()
            decode()
            torch.cuda.synchronize()
            rec = pool.buf["stats"][hs].cpu().numpy().view(LM.STATS).reshape(-1)
            times = {"stream_step": [], "one_shot": [], "window_decode": []}
            for _ in range(rounds):
                for key, fn in (("stream_step", run_s), ("one_shot", run_o), ("window_decode", decode)):
                    torch.cuda.synchronize()
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[key].append(a.elapsed_time(b) / reps)
            res[name] = dict(n_over=int(rec["n_over"].sum()), n_touched=int(rec["n_touched"].sum()),
                             **{k: dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))
                                for k, v in times.items()})
        for h in hs:
            codec.peak_limit_stream_close(h)
        out[str(B)] = res
    return out


def _stream_markdown(res, reps, rounds, gemm) -> str:
    rows = ["# The limiter of streams: step time (tools/limiter_probe.py --stream)", "",
            f"MI355X, device events around {reps} back-to-back calls, median (min .. max) of {rounds} rounds, the three calls alternated; chunks of "
            f"{CHUNK} samples at 24 kHz per stream; `window_decode` is `decode_windows` of as many {CHUNK}-sample chunks (codec GEMM {gemm}, synthetic weights).", "",
            "| streams | signal | samples over T | stream step, ms | one-shot limiter, ms | window decode, ms | step / decode |", "|---|---|---|---|---|---|---|"]
    f = lambda d: f"{d['median']:.4f} ({d['min']:.4f} .. {d['max']:.4f})"
    for B, by in res.items():
        for name, d in by.items():
            rows.append(f"| {B} | {name} | {d['n_over']} | {f(d['stream_step'])} | {f(d['one_shot'])} | {f(d['window_decode'])} | "
                        f"{100.0 * d['stream_step']['median'] / d['window_decode']['median']:.1f} % |")
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--gemm", default="f16")
    ap.add_argument("--stream", action="store_true", help="time the limiter of streams instead")
    ap.add_argument("--out", default=None, help="with --stream: the markdown table goes here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("limiter_probe needs a GPU: nothing here can be timed without one")
    from tests import loudness_cases as LC
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    from chattts_amd.core import Chat
    chat = Chat()
    assert chat.load(state_dicts={k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}, device=dev, dtype="f32", codec_gemm=a.gemm)
    codec = chat.codec
    if a.stream:
        res = _stream(codec, a.reps, a.rounds)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(_stream_markdown(res, a.reps, a.rounds, a.gemm))
        print(json.dumps(dict(metric="limiter_stream_probe", reps=a.reps, rounds=a.rounds, codec_gemm=a.gemm, chunk=CHUNK, streams=res)))
        return
    out = dict(metric="limiter_probe", target=TARGET, reps=a.reps, rounds=a.rounds, codec_gemm=a.gemm, fixtures={}, batch={})
    sig = [s for s in LC.signals() if s[0] not in ("zeros", "silent")]
    for fs in (8000, 24000):
        rows = _level(codec, [x for _, x, _ in sig], fs, TARGET)
        out["fixtures"][str(fs)] = {name: row for (name, _, _), row in zip(sig, rows)}
    rs = np.random.RandomState(3)
    hid = [torch.from_numpy(rs.standard_normal((64, 768)).astype(np.float32) * 0.5).to(dev) for _ in range(64)]
    wav, off = codec.decode_ragged(hid)
    rows = _level(codec, [w.cpu().numpy() for w in (wav[off[i]: off[i + 1]] for i in range(64))], 24000, TARGET)
    gain_lu = [r["L_limiter"] - r["L_ceiling"] for r in rows]
    out["batch"] = dict(rows=64, tokens=64, L=[min(r["L"] for r in rows), max(r["L"] for r in rows)],
                        L_ceiling=[min(r["L_ceiling"] for r in rows), max(r["L_ceiling"] for r in rows)],
                        L_limiter=[min(r["L_limiter"] for r in rows), max(r["L_limiter"] for r in rows)],
                        gained_LU=[round(min(gain_lu), 3), round(float(np.median(gain_lu)), 3), round(max(gain_lu), 3)],
                        n_over=sum(r["n_over"] for r in rows), n_touched=sum(r["n_touched"] for r in rows), samples=int(off[-1]),
                        peak=max(r["peak"] for r in rows), min_gain=min(r["min_gain"] for r in rows))
    out["stage"] = _stage(codec, a.reps, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

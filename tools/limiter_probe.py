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

Noise under a stepped envelope; synthetic weights.  Prints one JSON line.  Not a bench.py leg.

    python tools/limiter_probe.py [--reps 20] [--rounds 7]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--gemm", default="f16")
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

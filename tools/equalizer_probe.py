"""What the output equaliser costs (csrc/equalizer.hip, ctts_equalize_ragged, behind CodecEngine.equalize) and how far it lies from its
definition.  Needs a GPU; writes profiles/equalizer_probe.md.

    python tools/equalizer_probe.py [--reps 20] [--rounds 5] [--out profiles/equalizer_probe.md]

  packs         ONE segment of 10 s at 48 kHz (480,000 samples: the longest chain of tiles the scan pass walks serially, 227 records),
                and 64 packed segments of mixed length, 0.1 s .. 10 s at 8, 24 and 48 kHz in turn (seeded), about 8 M samples: noise at
                0.3 rms.  Each with the one-section "telephone" preset and with a four-section cascade.
  timing        the C entry point on preallocated buffers (no allocation, no upload in the loop), device events around `reps` calls
                back to back, the median of `rounds`; per call, x into y.
  traffic       the algorithm's: 3 reads and 1 write of the samples, 16 bytes per sample (the tiles' end states, the true entry states
                and the output each need a pass, and the third pass reads what it filters).  The kernels stage a tile in LDS, so the
                third launch reads x once for both of its passes: 12 bytes per sample cross the memory interface (8 for a segment of
                one tile).  The share of the 8 TB/s HBM peak is the algorithm's bytes over the time.
  error         the pack of tests/equalizer_cases.py (ten segments at every length at which the route takes another path, four kinds of
                input) against `equalizer.apply`, the serial float64 loop: the largest distance in float32 ulps and the share of samples
                that differ at all, per kind of input; next to it the NumPy twin of the route against the same loop."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import equalizer as EQ  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402
from tests import equalizer_cases as K  # noqa: E402

HBM_PEAK = 8.0e12
FOUR = {"highpass_hz": 120, "lowshelf": {"hz": 250, "db": 4.5}, "highshelf": {"hz": 3000, "db": -6}, "peaks": [{"hz": 1800, "db": 7.5, "q": 3}]}   # valid at 8 kHz too
N_SEG = 64


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


def _packs():
    r = np.random.default_rng(5)
    one = ([480000], [48000])
    rates = [(8000, 24000, 48000)[i % 3] for i in range(N_SEG)]
    lens = [int(r.uniform(0.1, 10.0) * fs) for fs in rates]
    return {"one 10 s segment at 48 kHz": one, f"{N_SEG} segments of 0.1 .. 10 s at 8 / 24 / 48 kHz": (lens, rates)}


def _measure(codec, lens, rates, spec, reps: int, rounds: int) -> dict:
    dev, lib = codec.device, codec.lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = int(sum(lens))
    x_h = (0.3 * np.random.default_rng(6).standard_normal(n)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    off, sel, coef, _ = EQ.tables(n, spec, off, rates)
    x, y = up(x_h), torch.empty(n, dtype=torch.float32, device=dev)
    off_d, sel_d, coef_d = up(off), up(sel), up(coef)
    sb = int(lib.ctts_equalize_ragged_scratch_bytes(vp(off), len(lens)))
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        rc = lib.ctts_equalize_ragged(x.data_ptr(), y.data_ptr(), off_d.data_ptr(), vp(off), len(lens), sel_d.data_ptr(), vp(sel), coef_d.data_ptr(), vp(coef),
                                      int(coef.shape[0]), scratch.data_ptr(), sb, st)
        assert rc == 0, lib.ctts_last_error()
    ms = _time(call, reps, rounds)
    tiles = sum(-(-m // EQ.TILE) for m in lens)
    return dict(n=n, ms=ms, tiles=tiles, share=16.0 * n / (ms * 1e-3) / HBM_PEAK, gbps=16.0 * n / ms / 1e6, scratch=sb)


def _errors(codec) -> list:
    dev = codec.device
    rows = []
    for kind in K.KINDS:
        x = torch.from_numpy(K.pack(kind).copy()).to(dev)
        y = codec.equalize(x, K.SPECS, offsets=K.OFFSETS, rates=K.RATES).cpu().numpy()
        twin = EQ.equalize(K.pack(kind), K.SPECS, offsets=K.OFFSETS, rates=K.RATES, route=True)
        d, t = K.ulps(y, K.reference(kind)), K.ulps(twin, K.reference(kind))
        rows.append((kind, len(d), int(d.max()), int((d > 0).sum()), int(t.max()), int((t > 0).sum()), int((K.ulps(y, twin) > 0).sum())))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equalizer_probe.md"))
    a = ap.parse_args()
    from chattts_amd.engine import CodecEngine
    dev = torch.device("cuda:0")
    w = synthetic_all()
    codec = CodecEngine(w["decoder"], w["vocos"], dev)
    lines = ["# equaliser probe", "",
             f"{torch.cuda.get_device_name(0)}; x into y, the C entry point on preallocated buffers; device events around {a.reps} calls, median of "
             f"{a.rounds} rounds.  Launches per call: 3 kernels (1 where no segment is longer than a tile of {EQ.TILE} samples).  Bytes: the "
             "algorithm's 3 reads + 1 write of the samples, 16 per sample; the share is of the 8 TB/s HBM peak.", "",
             "| pack | cascade | samples | tiles | us per call | GB/s over 16 B/sample | share of HBM peak |", "|---|---|---|---|---|---|---|"]
    for name, (lens, rates) in _packs().items():
        for label, spec in (("telephone (1 section)", "telephone"), ("4 sections", FOUR)):
            r = _measure(codec, lens, rates, spec, a.reps, a.rounds)
            lines.append(f"| {name} | {label} | {r['n']} | {r['tiles']} | {1e3 * r['ms']:.1f} | {r['gbps']:.0f} | {100 * r['share']:.1f} % |")
    lines += ["", "## error", "", "The pack of tests/equalizer_cases.py against `equalizer.apply` (the serial float64 loop, rounded once to float32).", "",
              "| input | samples | device: most ulps | device: samples that differ | route twin: most ulps | route twin: samples that differ | device against the twin: samples that differ |",
              "|---|---|---|---|---|---|---|"]
    tot = dev_d = 0
    for kind, n, mx, nd, tmx, tnd, dt in _errors(codec):
        lines.append(f"| {kind} | {n} | {mx} | {nd} | {tmx} | {tnd} | {dt} |")
        tot, dev_d = tot + n, dev_d + nd
    lines += ["", f"device: {dev_d} of {tot} samples differ from the definition, a share of {dev_d / tot:.2e} (the tests' cap is {K.CAP:g})."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

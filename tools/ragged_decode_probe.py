"""Padded vs ragged acoustic decode (CodecEngine.decode_to_wavs vs CodecEngine.decode_ragged), in each codec gemm mode:

  * c3_like : 64 utterances of U{128..512} tokens -- the padded [64, Tmax] batch (the reference's semantics) vs one ragged pass over
              the same rows (no padding frames); device time of the decode only
  * short16 : 16 short utterances (U{16..96} tokens) as the batched endpoint finishes them -- one alone decode + host strip +
              float_to_int16 per utterance (SpeechBatcher.finish) vs ONE ragged decode + device PCM16 + one copy
              (Chat.decode_to_pcm16(..., ragged=True)); wall time including the host side

Synthetic weights.  Prints one JSON line.  Not a bench.py leg.

    python tools/ragged_decode_probe.py [--reps 10] [--gemm f16,bf16x3,f32]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402


def _dev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 3)


def _wall_ms(fn, reps):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gemm", default="f16,bf16x3,f32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    rs = np.random.RandomState(3)
    c3 = [torch.from_numpy(rs.standard_normal((int(t), 768)).astype(np.float32) * 0.5).to(dev) for t in rs.randint(128, 513, size=64)]
    short = [torch.from_numpy(rs.standard_normal((int(t), 768)).astype(np.float32) * 0.5).to(dev) for t in rs.randint(16, 97, size=16)]
    out = dict(metric="ragged_decode_probe", c3_tokens=int(sum(r.shape[0] for r in c3)), c3_padded_tokens=64 * max(r.shape[0] for r in c3),
               short_tokens=[int(r.shape[0]) for r in short], modes={})
    for gemm in a.gemm.split(","):
        chat = Chat()
        sd = {k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}
        assert chat.load(state_dicts=sd, device=dev, dtype="f32", codec_gemm=gemm)
        codec = chat.codec
        r = {}
        r["c3_padded_ms"] = _dev_ms(lambda: codec.decode_to_wavs(c3), a.reps)
        r["c3_ragged_ms"] = _dev_ms(lambda: codec.decode_ragged(c3), a.reps)

        def alone():
            for h in short:
                w = chat.decode_to_wavs([h])[0]
                float_to_int16(w[np.abs(w) > np.float32(1e-5)])
        r["short16_alone_ms"] = _wall_ms(alone, a.reps)
        r["short16_ragged_ms"] = _wall_ms(lambda: chat.decode_to_pcm16(short, ragged=True), a.reps)
        r["short16_ragged_decode_only_ms"] = _dev_ms(lambda: codec.decode_ragged(short), a.reps)
        out["modes"][gemm] = r
        del chat, codec
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

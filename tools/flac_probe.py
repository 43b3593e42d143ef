"""What FLAC output costs and saves (csrc/flac.hip, ctts_flac_encode_ranges), beside the PCM16 path it follows:

  * decode    : `Chat.decode_to_pcm16(rows, ragged=True)` on 1 and 8 rows of 469 tokens (10 s each) without `flac=` and with it, same rows;
                wall time including the host side (median of `--reps` calls after warm ones), the bytes that cross the bus either way, and
                the compression ratio 2 n / file bytes of the synthesised utterances (synthetic weights: the decoder's output is close to
                noise, so this ratio is the format's floor, not speech's)
  * encode    : the encoder alone on 1, 8 and 64 signals of 10 s at 24 kHz already on the device -- device time of one call (the three
                launches) from events around `--reps` back-to-back calls on pre-uploaded tables, for a speech-like signal (a noise-driven
                resonance, tests/flac_cases.py's "ar2" recipe) and for full-scale noise (every frame VERBATIM), with the ratio of each

  * --stream  : streamed FLAC instead (ctts_flac_stream_step behind `CodecEngine.decode_windows(flac=)`):
                poll  -- one poll of 1, 8 and 32 streams, each due a 24-token chunk (12,000 samples of a 48-token prefix), through
                         `decode_windows` without `flac=` and with it, the two alternating call by call: the median wall time of each and
                         the spread (min .. max) of the calls, and the bytes `to_host` brought back per call either way
                size  -- one speech-like utterance of 10 s pushed in 12,000-sample chunks (the server's) and in 3,000-sample chunks: the
                         stream's bytes, header included, against `flac.encode` of the same samples (fixed blocks of 4096)

Every file is checked against `flac.bound(n)`, every pushed chunk against `flac.stream_bound(n)`.  Prints one JSON line.  Not a bench.py leg.

    python tools/flac_probe.py [--reps 20] [--gemm f16] [--stream]
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

from chattts_amd import _lib, flac  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

SEG = 240000          # 10 s at 24 kHz
TOKENS = 469          # 256 (2 T - 1) = 239 872 samples


def _speech_like(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n) * 300
    x = np.zeros(n)
    for j in range(2, n):
        x[j] = e[j] + 1.9 * x[j - 1] - 0.92 * x[j - 2]
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _encode_ms(codec, sig: np.ndarray, n_sig: int, reps: int):
    """device time of one ctts_flac_encode_ranges call over `n_sig` copies of `sig`, and the bytes it writes"""
    dev = codec.device
    n = len(sig)
    slot = (n + 7) // 8 * 8
    pcm = torch.from_numpy(np.tile(np.concatenate([sig, np.zeros(slot - n, np.int16)]), n_sig)).to(dev)
    tab = np.zeros(n_sig, _lib.FLAC_RANGE)
    per = (n + flac.BLOCK - 1) // flac.BLOCK
    for k in range(n_sig):
        tab[k] = (k * slot, n, 24000, -1, k * per)
    sizes = (C.c_int64 * 3)()
    _lib.check(codec.lib.ctts_flac_encode_sizes(tab.ctypes.data_as(C.c_void_p), n_sig, sizes), "ctts_flac_encode_sizes")
    out = torch.empty(((int(sizes[1]) + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
    work = torch.empty((int(sizes[2]),), dtype=torch.uint8, device=dev)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        _lib.check(codec.lib.ctts_flac_encode_ranges(pcm.data_ptr(), None, tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), n_sig, out.data_ptr(),
                                                     out.numel(), work.data_ptr(), work.numel(), st), "ctts_flac_encode_ranges")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    total = int(work[: 8 * (int(sizes[0]) + 1)].view(torch.int64)[-1].item())
    assert total + n_sig * flac.HEADER_BYTES <= n_sig * flac.bound(n)
    return round(a.elapsed_time(b) / reps, 3), total


def _wall_ms(fn, reps: int):
    for _ in range(3):
        res = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), res


def _stream_probe(codec, reps: int) -> dict:
    dev = codec.device
    out = dict(poll={}, size={})
    g = torch.Generator(device=dev).manual_seed(3)
    store = torch.randn((32, 64, 768), device=dev, generator=g) * 0.5
    copied = [0]
    to_host = codec.to_host

    def counting(t):
        copied[0] += t.numel() * t.element_size()
        return to_host(t)
    codec.to_host = counting
    try:
        for S in (1, 8, 32):
            wins = [(s, 48, 12000, 24000, False) for s in range(S)]
            hs = [codec.flac_stream_open(24000) for _ in range(S)]
            calls = {"pcm16": lambda: codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5),
                     "flac": lambda: codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, flac=[True] * S, flac_streams=hs)}
            for _ in range(3):
                for fn in calls.values():
                    res = fn()
            torch.cuda.synchronize()
            ts, nbytes = {k: [] for k in calls}, {}
            for _ in range(reps):
                for k, fn in calls.items():                    # alternating: both see the same neighbours on the machine
                    copied[0] = 0
                    t0 = time.perf_counter()
                    res = fn()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
                    nbytes[k] = copied[0]
                    if k == "flac":
                        assert all(r.dtype == np.uint8 and r.size <= flac.stream_bound(12000) for r in res)
            for h in hs:
                codec.flac_stream_close(h)
            out["poll"][f"streams{S}"] = {k: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                                                 to_host_bytes=nbytes[k]) for k, v in ts.items()}
    finally:
        codec.to_host = to_host
    sig = _speech_like(SEG, 7)
    file_bytes = len(flac.encode(sig, 24000))
    pcm = torch.from_numpy(sig).to(dev)
    for chunk in (12000, 3000):
        h = codec.flac_stream_open(24000)
        total = flac.HEADER_BYTES
        for lo in range(0, SEG, chunk):
            n = min(chunk, SEG - lo)
            total += codec.flac_stream_step(pcm, [(h, lo, n, lo + n == SEG)])[0].size
        codec.flac_stream_close(h)
        out["size"][f"chunks_of_{chunk}"] = dict(stream_bytes=total, file_bytes=file_bytes, pcm16_bytes=2 * SEG,
                                                 stream_over_file=round(total / file_bytes, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gemm", default="f16")
    ap.add_argument("--stream", action="store_true", help="streamed FLAC: one poll with and without it, and the stream's size")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flac_probe needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    sds = synthetic_all()
    chat = Chat()
    assert chat.load(state_dicts={k: sds[k] for k in ("gpt", "embed", "decoder", "vocos")}, device=dev, dtype="f32", codec_gemm=a.gemm)
    codec = chat.codec
    if a.stream:
        print(json.dumps(dict(metric="flac_stream_probe", codec_gemm=a.gemm, reps=a.reps, **_stream_probe(codec, a.reps))))
        return
    out = dict(metric="flac_probe", segment_samples=SEG, tokens_per_row=TOKENS, codec_gemm=a.gemm, reps=a.reps, decode={}, encode={})
    g = torch.Generator(device=dev).manual_seed(3)
    for B in (1, 8):
        rows = [torch.randn((TOKENS, 768), device=dev, generator=g) * 0.5 for _ in range(B)]
        t_pcm, pcm = _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True), a.reps)
        t_flac, files = _wall_ms(lambda: chat.decode_to_pcm16(rows, ragged=True, flac=True), a.reps)
        assert all(f.size <= flac.bound(p.size) for f, p in zip(files, pcm))
        n_pcm, n_file = sum(2 * p.size for p in pcm), sum(f.size for f in files)
        out["decode"][f"rows{B}"] = dict(pcm16_ms=t_pcm, flac_ms=t_flac, pcm16_bytes=n_pcm, flac_bytes=n_file, ratio=round(n_pcm / n_file, 3))
    rng = np.random.default_rng(1)
    for name, sig in (("speech_like", _speech_like(SEG, 7)), ("noise", rng.integers(-32768, 32768, SEG).astype(np.int16))):
        for n_sig in (1, 8, 64):
            ms, total = _encode_ms(codec, sig, n_sig, a.reps)
            out["encode"][f"{name}_x{n_sig}"] = dict(ms=ms, bytes=total, ratio=round(2 * SEG * n_sig / total, 3),
                                                     samples_per_us=round(SEG * n_sig / (ms * 1e3), 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

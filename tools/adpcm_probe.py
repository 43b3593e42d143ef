"""What IMA ADPCM output costs (csrc/adpcm.hip, ctts_adpcm_encode_ranges), beside two yardsticks on the same buffers:

  * adpcm : one ctts_adpcm_encode_ranges call (one launch, one lane per block) over 1 / 8 / 64 signals of 10 s at 8, 24 and 48 kHz that
            are already on the device as int16
  * g711  : one ctts_g711_encode_ranges call over the same int16 buffers (one byte per sample, no dependence between samples)
  * pcm16 : one ctts_float_to_int16_ragged call over float32 buffers of the same shapes (the conversion ADPCM comes behind)

Device time from events around `--reps` back-to-back calls on pre-uploaded tables, after warm calls; `--rounds` such windows per entry, the
three entries alternating round by round so that they see the same neighbours on the machine; the figure is the median window, with the
spread (min .. max) beside it.  The ADPCM bytes are checked against the NumPy twin on the first signal.  Prints one JSON line.  Not a
bench.py leg.

    python tools/adpcm_probe.py [--reps 20] [--rounds 9]

`--stream`: the streamed form instead (ctts_adpcm_stream_step: adpcm_stage_k, then adpcm_encode_k over the staging ranges -- two
launches) for 1, 16 and 64 streams that each hold 500 samples and get a chunk of 12000 at 24 kHz, beside one ctts_adpcm_encode_ranges
call (one launch) over the same chunks as stand-alone signals -- what the step costs over the one-shot encoder for the same samples --,
and beside that call behind a device copy of the chunks (and the copy alone): the one-shot encoder over samples that a kernel has just
written, which is how both encoders meet them behind the conversion.
The same windows, alternating; `--reps` then defaults to 500 (a step is tens of microseconds).  The first stream's blocks are checked
against the twin.

    python tools/adpcm_probe.py --stream [--reps 500] [--rounds 9]
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

from chattts_amd import _lib, adpcm  # noqa: E402

SECONDS = 10


def _speech_like(n: int, rate: int, seed: int) -> np.ndarray:
    """voiced bursts: harmonics of a gliding pitch under an on / off envelope, a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    ph = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t)) / rate
    x = sum(np.exp(-((h * 120.0 - 600.0) / 500.0) ** 2) * np.sin(h * ph + h) for h in range(1, 20))
    env = np.clip(np.sin(2 * np.pi * 1.3 * t) * 3.0, 0.0, 1.0) ** 2
    x = x / np.abs(x).max() * env * 14000.0 + rng.standard_normal(n) * 8.0
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _windows(calls: dict, reps: int, rounds: int) -> dict:
    """name -> callable: `rounds` windows of `reps` back-to-back calls each, the entries alternating -> name -> median / min / max ms per call"""
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / reps)
    return {k: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ms.items()}


def _entry(lib, dev, rate: int, n_sig: int, reps: int, rounds: int) -> dict:
    n = SECONDS * rate
    slot = (n + 7) // 8 * 8
    sig = _speech_like(n, rate, 7)
    pcm = torch.from_numpy(np.tile(np.concatenate([sig, np.zeros(slot - n, np.int16)]), n_sig)).to(dev)
    wav = pcm.to(torch.float32) / 32768.0
    st = torch.cuda.current_stream(dev).cuda_stream
    # ADPCM
    A, nb = adpcm.align(rate), adpcm.n_blocks(n, rate)
    tab = np.zeros(n_sig, _lib.ADPCM_RANGE)
    for k in range(n_sig):
        tab[k] = (k * slot, n, k * nb, k * nb * A, rate, -1, 0)
    sizes = (C.c_int64 * 3)()
    _lib.check(lib.ctts_adpcm_encode_sizes(tab.ctypes.data_as(C.c_void_p), n_sig, sizes), "ctts_adpcm_encode_sizes")
    out_a = torch.empty((int(sizes[1]),), dtype=torch.uint8, device=dev)
    used = torch.empty((n_sig,), dtype=torch.int64, device=dev)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    tab_p = tab.ctypes.data_as(C.c_void_p)

    def call_adpcm():
        _lib.check(lib.ctts_adpcm_encode_ranges(pcm.data_ptr(), None, tab_d.data_ptr(), tab_p, n_sig, out_a.data_ptr(), out_a.numel(),
                                                used.data_ptr(), 8 * n_sig, st), "ctts_adpcm_encode_ranges")
    # G.711
    gtab = np.zeros(n_sig, _lib.G711_RANGE)
    for k in range(n_sig):
        gtab[k] = (k * slot, n, 0, 0, 0)
    out_g = torch.empty(((pcm.numel() + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
    gtab_d = torch.from_numpy(gtab.view(np.uint8).copy()).to(dev)
    gtab_p = gtab.ctypes.data_as(C.c_void_p)

    def call_g711():
        _lib.check(lib.ctts_g711_encode_ranges(pcm.data_ptr(), out_g.data_ptr(), gtab_d.data_ptr(), gtab_p, n_sig, st), "ctts_g711_encode_ranges")
    # the 16-bit conversion
    off = np.arange(n_sig + 1, dtype=np.int64) * slot
    off_d = torch.from_numpy(off).to(dev)
    out_p = torch.empty((wav.numel(),), dtype=torch.int16, device=dev)
    peak = torch.empty((n_sig,), dtype=torch.int32, device=dev)
    off_p = off.ctypes.data_as(C.c_void_p)

    def call_pcm16():
        _lib.check(lib.ctts_float_to_int16_ragged(wav.data_ptr(), out_p.data_ptr(), None, off_d.data_ptr(), off_p, n_sig, 0, 0.0,
                                                  peak.data_ptr(), st), "ctts_float_to_int16_ragged")
    res = _windows({"adpcm": call_adpcm, "g711": call_g711, "pcm16": call_pcm16}, reps, rounds)
    got = out_a[: nb * A].cpu().numpy()
    assert np.array_equal(got, adpcm.encode_blocks(sig, rate)), "the device's blocks differ from the twin's"
    assert used.cpu().tolist() == [n] * n_sig
    res["adpcm"].update(blocks=n_sig * nb, bytes=int(sizes[1]), samples_per_us=round(n * n_sig / (res["adpcm"]["median_ms"] * 1e3), 1))
    return res


STREAM_RATE, STREAM_CHUNK, STREAM_CARRY = 24000, 12000, 500


def _stream_entry(lib, dev, n_str: int, reps: int, rounds: int) -> dict:
    rate, n, carry = STREAM_RATE, STREAM_CHUNK, STREAM_CARRY
    slot = (n + 7) // 8 * 8
    sig = _speech_like(carry + n, rate, 7)
    pcm = torch.from_numpy(np.tile(np.concatenate([sig[carry:], np.zeros(slot - n, np.int16)]), n_str)).to(dev)
    state = torch.zeros((n_str, 2048), dtype=torch.int16, device=dev)
    state[:, :carry] = torch.from_numpy(sig[:carry].copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    A, S = adpcm.align(rate), adpcm.samples_per_block(rate)
    nb = (carry + n) // S                                    # a push that is not final: whole blocks leave, the rest goes back to the slot
    tab = np.zeros(n_str, _lib.ADPCM_PUSH)
    room = (carry + n + 7) // 8 * 8
    for k in range(n_str):
        tab[k] = (k * slot, n, k * room, k * nb, k * nb * A, rate, k, carry, 0, -1, 0)
    sizes = (C.c_int64 * 4)()
    _lib.check(lib.ctts_adpcm_stream_sizes(tab.ctypes.data_as(C.c_void_p), n_str, n_str, pcm.numel(), sizes), "ctts_adpcm_stream_sizes")
    out_s = torch.empty((int(sizes[1]),), dtype=torch.uint8, device=dev)
    work = torch.empty((int(sizes[2]),), dtype=torch.uint8, device=dev)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    tab_p = tab.ctypes.data_as(C.c_void_p)
    keep = state.clone()

    def call_stream():
        _lib.check(lib.ctts_adpcm_stream_step(pcm.data_ptr(), pcm.numel(), None, None, tab_d.data_ptr(), tab_p, n_str, state.data_ptr(), n_str,
                                              out_s.data_ptr(), out_s.numel(), work.data_ptr(), work.numel(), st), "ctts_adpcm_stream_step")
    call_stream()                                            # the check first: the timed calls go on from the carry this one leaves
    got = out_s[: nb * A].cpu().numpy()
    assert np.array_equal(got, adpcm.StreamEncoder(rate).push(sig)), "the device's blocks differ from the twin's"
    assert work[: 8 * n_str].view(torch.int64).cpu().tolist() == [nb * S] * n_str
    assert np.array_equal(state[0, : (carry + n) % S].cpu().numpy(), sig[nb * S:])
    state.copy_(keep)
    # the one-shot encoder over the same chunks
    nb1 = adpcm.n_blocks(n, rate)
    rtab = np.zeros(n_str, _lib.ADPCM_RANGE)
    for k in range(n_str):
        rtab[k] = (k * slot, n, k * nb1, k * nb1 * A, rate, -1, 0)
    out_a = torch.empty((n_str * nb1 * A,), dtype=torch.uint8, device=dev)
    used = torch.empty((n_str,), dtype=torch.int64, device=dev)
    rtab_d = torch.from_numpy(rtab.view(np.uint8).copy()).to(dev)
    rtab_p = rtab.ctypes.data_as(C.c_void_p)

    def call_one_shot():
        _lib.check(lib.ctts_adpcm_encode_ranges(pcm.data_ptr(), None, rtab_d.data_ptr(), rtab_p, n_str, out_a.data_ptr(), out_a.numel(),
                                                used.data_ptr(), 8 * n_str, st), "ctts_adpcm_encode_ranges")
    # ... and over chunks that a kernel has just written, as the conversion in front of a real encode leaves them (the buffer above is
    # read-only and stays in every L2): a device copy of the chunks, then the same call; the copy alone beside it
    fresh = torch.empty_like(pcm)

    def call_copy():
        fresh.copy_(pcm)

    def call_fresh():
        fresh.copy_(pcm)
        _lib.check(lib.ctts_adpcm_encode_ranges(fresh.data_ptr(), None, rtab_d.data_ptr(), rtab_p, n_str, out_a.data_ptr(), out_a.numel(),
                                                used.data_ptr(), 8 * n_str, st), "ctts_adpcm_encode_ranges")
    res = _windows({"stream_step": call_stream, "one_shot": call_one_shot, "copy_then_one_shot": call_fresh, "copy": call_copy}, reps, rounds)
    res["stream_step"].update(launches=2, blocks=n_str * nb, bytes=int(sizes[1]))
    res["one_shot"].update(launches=1, blocks=n_str * nb1, bytes=n_str * nb1 * A)
    res["copy_then_one_shot"].update(launches=2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--stream", action="store_true")
    a = ap.parse_args()
    a.reps = a.reps or (500 if a.stream else 20)
    if not torch.cuda.is_available():
        raise SystemExit("adpcm_probe needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    if a.stream:
        out = dict(metric="adpcm_stream_probe", rate=STREAM_RATE, chunk=STREAM_CHUNK, carry=STREAM_CARRY, reps=a.reps, rounds=a.rounds, entries={})
        for n_str in (1, 16, 64):
            out["entries"][f"x{n_str}"] = _stream_entry(lib, dev, n_str, a.reps, a.rounds)
        print(json.dumps(out))
        return
    out = dict(metric="adpcm_probe", seconds=SECONDS, reps=a.reps, rounds=a.rounds, entries={})
    for rate in (8000, 24000, 48000):
        for n_sig in (1, 8, 64):
            out["entries"][f"{rate}_x{n_sig}"] = _entry(lib, dev, rate, n_sig, a.reps, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

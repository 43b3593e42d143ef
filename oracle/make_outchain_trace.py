"""Characterisation trace of the decode calls' output options: which stage runs, in which order, with which arguments.

A device-free recorder (a `CodecEngine` subclass whose plain decodes, float32 stages, conversions and copies are recorded instead of
launched, behind a `Chat.__new__(Chat)`) walks a fixed table of calls -- every decode entry point crossed with the values of
`sample_rate`, `speed`, `loudness`, `pauses` and `limiter`, one for all and one per row, on and off -- and writes what it saw to
tests/golden/outchain_trace.json: for an accepted call every recorded call (name, arguments, offsets as lists), for a refused call the
exception's type and message.  The file keeps every distinct call once ("calls") and a case's trace as indices into that list (`pack` /
`unpack`): most calls recur in many cases.  tests/test_outchain_trace.py replays the table against the working tree.

    python -m oracle.make_outchain_trace            # rewrites the JSON: run it at the commit whose behaviour is to be pinned

The cross of the five options is pruned to a pairwise covering array (every pair of values of two options occurs in some row); the
zero-padded calls take one rate and one speed for the whole batch, so their array leaves the per-row rate and speed to single cases,
which are refused.  The refused calls of the host tests (tests/test_*_host.py) are in the table too."""
from __future__ import annotations

import dataclasses
import itertools
import json
import os
import random

import numpy as np
import torch

from chattts_amd import pauses as PA
from chattts_amd.core import Chat
from chattts_amd.engine import CodecEngine, keep_offsets
from chattts_amd.serving import SpeechBatcher

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "outchain_trace.json")


def _j(v):
    """a recorded argument as JSON: tensors as "dtype[shape]", arrays as lists, specs as their fields"""
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, PA.PauseSpec):
        return {"PauseSpec": dataclasses.asdict(v)}
    if isinstance(v, (list, tuple)):
        return [_j(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _j(x) for k, x in v.items()}
    if isinstance(v, (np.bool_, np.integer, np.floating)):
        return v.item()
    return v


def _spans(off, wav):
    """host offsets of a pack, or of the rows of a [B, n] batch"""
    return np.arange(wav.shape[0] + 1, dtype=np.int64) * wav.shape[1] if off is None else np.asarray(off, np.int64)


class _PlainDecode(Exception):
    pass


class Recorder(CodecEngine):
    """a CodecEngine without a device: the order of the calls is the real code's, the calls themselves only leave a record and
    hand back zeros of the real call's shape"""
    SAMPLES = 256

    def __init__(self):
        self.calls = []
        self.depth = 0
        self.device = torch.device("cpu")

    @property
    def lib(self):
        raise _PlainDecode                     # the real method got as far as its launches: every option was off

    def rec(self, name, **kw):
        self.calls.append([name, {k: _j(v) for k, v in kw.items()}])

    # -- the decodes: the real methods run, and the call among them that reaches the library is the plain decode; what crosses the
    #    seam from outside (depth 0) is recorded with the keywords it was given
    def _entry(self, name, plain, real, rows, first, args, kw):
        if self.depth == 0:
            self.rec("call." + name, n=len(rows), first=first, **kw, **({"positional": list(args)} if args else {}))
        self.depth += 1
        try:
            return real(rows, first, *args, **kw)
        except _PlainDecode:
            self.rec("decode." + name, rows=[int(r.shape[0]) for r in rows], first=first)
            return plain()
        finally:
            self.depth -= 1

    def decode_ragged(self, rows, return_mel=False, *args, **kw):
        def plain():
            lens = [self.SAMPLES * (2 * int(r.shape[0]) - 1) for r in rows]
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            return (torch.zeros(int(off[-1])), off, torch.zeros(2, 100)) if return_mel else (torch.zeros(int(off[-1])), off)
        return self._entry("decode_ragged", plain, super().decode_ragged, rows, return_mel, args, kw)

    def decode_to_wavs(self, rows, pad_to=None, *args, **kw):
        def plain():
            T = max(int(r.shape[0]) for r in rows) if pad_to is None else int(pad_to)
            return torch.zeros(len(rows), self.SAMPLES * (2 * T - 1))
        return self._entry("decode_to_wavs", plain, super().decode_to_wavs, rows, pad_to, args, kw)

    def vocos_decode(self, mel):
        self.rec("vocos_decode", mel=mel)
        return torch.zeros(mel.shape[0], self.SAMPLES * (mel.shape[1] - 1))

    # -- the float32 stages
    def time_scale(self, wav, speed, offsets=None, return_path=False):
        self.rec("time_scale", wav=wav, speed=speed, offsets=offsets, return_path=return_path)
        return torch.zeros(wav.shape[0], int(round(wav.shape[1] / float(speed))))

    def time_scale_segments(self, wav, off, speeds):
        self.rec("time_scale_segments", wav=wav, off=off, speeds=speeds)
        lens = [int(round(int(n) / float(s))) for n, s in zip(np.diff(off), speeds)]
        out = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return torch.zeros(int(out[-1])), out

    def resample(self, wav, orig, new, offsets=None):
        self.rec("resample", wav=wav, orig=orig, new=new, offsets=offsets)
        return torch.zeros(wav.shape[0], -(-wav.shape[1] * int(new) // int(orig)))

    def resample_segments(self, wav, off, rates, orig=24000):
        self.rec("resample_segments", wav=wav, off=off, rates=rates, orig=orig)
        lens = [-(-int(n) * int(r) // int(orig)) for n, r in zip(np.diff(off), rates)]
        out = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return torch.zeros(int(out[-1])), out

    def trim_pauses(self, wav, spec, offsets=None, rates=None, return_stats=False):
        self.rec("trim_pauses", wav=wav, spec=spec, offsets=offsets, rates=rates, return_stats=return_stats)
        off = _spans(offsets, wav)
        specs = list(spec) if isinstance(spec, (list, tuple)) else [spec] * (len(off) - 1)
        if all(s is None for s in specs):
            return wav.reshape(-1), off
        lens = [int(n) - (7 if s is not None else 0) for n, s in zip(np.diff(off), specs)]
        out = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return torch.zeros(int(out[-1])), out

    def loudness_normalize(self, wav, target, **kw):
        out = kw.get("out")
        self.rec("loudness_normalize", wav=wav, target=target, **{k: v for k, v in kw.items() if k != "out"},
                 out=None if out is None else out is wav, contiguous=wav.is_contiguous())
        return wav if out is None else out

    # -- the conversions and what follows them
    def float_to_int16(self, wav, per_row=True, product="f64", keep_thr=None):
        self.rec("float_to_int16", wav=wav, per_row=per_row, product=product, keep_thr=keep_thr)
        B, n = wav.shape
        return torch.zeros(B, n, dtype=torch.int16), None if keep_thr is None else torch.full((B, (n + 7) // 8), 255, dtype=torch.uint8)

    def float_to_int16_ragged(self, wav, off, product="f64", keep_thr=None, out=None):
        self.rec("float_to_int16_ragged", wav=wav, off=off, product=product, keep_thr=keep_thr, out=out)
        ko = keep_offsets(np.asarray(off, np.int64))
        if out is not None:
            out[0].zero_()
            if out[1] is not None:
                out[1].fill_(255)
            return out[0], out[1], ko
        return torch.zeros(wav.numel(), dtype=torch.int16), None if keep_thr is None else torch.full((int(ko[-1]),), 255, dtype=torch.uint8), ko

    def float_to_int16_groups(self, wav, off, grp, product="f64", keep_thr=1e-5, encodings=None):
        self.rec("float_to_int16_groups", wav=wav, off=off, grp=grp, product=product, keep_thr=keep_thr, encodings=encodings)
        return torch.zeros(16, dtype=torch.uint8), np.arange(len(grp), dtype=np.int64) * 8

    def float_to_int16_groups_flac(self, wav, off, grp, rates, product="f64", keep_thr=1e-5, encodings=None):
        self.rec("float_to_int16_groups_flac", wav=wav, off=off, grp=grp, rates=rates, product=product, keep_thr=keep_thr, encodings=encodings)
        return [np.zeros(3, np.int16 if r is None and (encodings is None or encodings[g] is None) else np.uint8) for g, r in enumerate(rates)]

    def unpack_groups(self, blob, starts, encodings=None):
        self.rec("unpack_groups", blob=blob.shape, starts=starts, encodings=encodings)
        return [np.zeros(3, np.int16 if encodings is None or e is None else np.uint8)
                for e in (encodings if encodings is not None else [None] * (len(starts) - 1))]

    def g711_encode(self, pcm, ranges, out=None):
        self.rec("g711_encode", pcm=pcm, ranges=ranges, out=out)
        return out.zero_() if out is not None else torch.zeros(pcm.numel(), dtype=torch.uint8)

    def to_host(self, t):
        self.rec("to_host", t=t)
        return t.numpy()


class _Dvae:
    def __init__(self, rec):
        self.rec = rec

    def decode_codes(self, rows, pad_to=None):
        self.rec.rec("dvae.decode_codes", rows=[int(r.shape[0]) for r in rows], pad_to=pad_to)
        T = max(int(r.shape[0]) for r in rows) if pad_to is None else int(pad_to)
        return torch.zeros(len(rows), 2 * T, 100)


class _FakeChat:
    """what SpeechBatcher.finish / finish_group hand to Chat"""
    def __init__(self):
        self.calls = []

    def decode_to_pcm16(self, hids, **kw):
        self.calls.append(["chat.decode_to_pcm16", {"n": len(hids), **{k: _j(v) for k, v in kw.items()}}])
        return [np.zeros(3, np.int16) for _ in hids]

    def decode_to_wavs(self, hids, **kw):
        self.calls.append(["chat.decode_to_wavs", {"n": len(hids), **{k: _j(v) for k, v in kw.items()}}])
        return [np.full(3, 0.5, np.float32) for _ in hids]


def _chat():
    chat = Chat.__new__(Chat)
    chat.codec = Recorder()
    chat.dvae = _Dvae(chat.codec)
    chat.has_loaded = lambda *a, **k: True
    return chat


def _batcher():
    b = SpeechBatcher.__new__(SpeechBatcher)
    b.chat, b.decode_calls, b.decoded, b.max_decode_group = _FakeChat(), 0, 0, 0
    return b


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
ROWS = lambda: [torch.zeros(3, 768), torch.zeros(2, 768)]
CODES = lambda: [torch.zeros(3, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64)]
GROUPS = lambda: [[torch.zeros(3, 768), torch.zeros(2, 768)], [torch.zeros(1, 768)]]       # two requests, three sentences

VALUES = {                                        # "per row" lists have two entries: two rows, or two requests
    "sample_rate": [None, 24000, 8000, [8000, 16000]],
    "speed": [None, 1.0, 1.25, [1.25, 1.0]],
    "loudness": [None, -16, [-16, None], [None, None]],
    "pauses": [None, True, [True, None], [None, None]],
    "limiter": [None, False, True, [True, False], [False, False]],
}


def covering(values: dict, seed: int = 1):
    """a pairwise covering array over `values`, greedily and reproducibly: every pair of values of two options is in some row"""
    names = list(values)
    rng = random.Random(seed)
    todo = {(a, i, b, j) for a, b in itertools.combinations(range(len(names)), 2)
            for i in range(len(values[names[a]])) for j in range(len(values[names[b]]))}
    rows = []
    while todo:
        best, gain = None, -1
        for _ in range(200):
            cand = [rng.randrange(len(values[n])) for n in names]
            g = sum((a, cand[a], b, cand[b]) in todo for a, b in itertools.combinations(range(len(names)), 2))
            if g > gain:
                best, gain = cand, g
        rows.append(best)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(range(len(names)), 2)}
    return [{n: values[n][i] for n, i in zip(names, r)} for r in rows]


FULL = covering(VALUES)                                                   # the ragged calls, the split call, the batcher
THIRD = FULL[::3]                                                         # the variants of a call: its back half is what differs
ONE = covering({k: [v for v in vs if k not in ("sample_rate", "speed") or np.ndim(v) == 0] for k, vs in VALUES.items()})   # one rate, one speed
ONE_THIRD = ONE[::3]


def _first(v):
    return v[0] if isinstance(v, list) else v


def _per_request(v, n=2):
    return None if v is None else (list(v) if isinstance(v, list) else [v] * n)


def _finish_group(b, o, **kw):
    # the batcher's jobs carry None for "off": a speed of 1.0 and a flag of False never reach it as such (serving._format_kw)
    return b.finish_group(ROWS(), sample_rates=_per_request(o["sample_rate"]), speeds=_per_request(o["speed"]), loudness=_per_request(o["loudness"]),
                          pauses=_per_request(o["pauses"]), limiter=_per_request(o["limiter"]), **kw)


def _finish(b, o, **kw):
    return b.finish(torch.zeros(3, 768), sample_rate=_first(o["sample_rate"]), speed=_first(o["speed"]), loudness=_first(o["loudness"]),
                    pauses=_first(o["pauses"]), limiter=bool(_first(o["limiter"])), **kw)


# name -> (who: "engine" | "chat" | "batcher", array, call(subject, options))
ENTRIES = {
    "eng.ragged": ("engine", FULL, lambda e, o: e.decode_ragged(ROWS(), **o)),
    "eng.ragged.mel": ("engine", THIRD, lambda e, o: e.decode_ragged(ROWS(), True, **o)),
    "eng.wavs": ("engine", ONE, lambda e, o: e.decode_to_wavs(ROWS(), **o)),
    "eng.wavs.pad": ("engine", ONE_THIRD, lambda e, o: e.decode_to_wavs(ROWS(), 4, **o)),
    "wavs.ragged": ("chat", FULL, lambda c, o: c.decode_to_wavs(ROWS(), ragged=True, **o)),
    "wavs.dec": ("chat", ONE, lambda c, o: c.decode_to_wavs(ROWS(), **o)),
    "wavs.dec.pad": ("chat", ONE_THIRD, lambda c, o: c.decode_to_wavs(ROWS(), True, 4, **o)),
    "wavs.codes": ("chat", ONE, lambda c, o: c.decode_to_wavs(CODES(), False, **o)),
    "wavs.codes.pad": ("chat", ONE_THIRD, lambda c, o: c.decode_to_wavs(CODES(), False, 4, **o)),
    "pcm.ragged": ("chat", FULL, lambda c, o: c.decode_to_pcm16(ROWS(), ragged=True, **o)),
    "pcm.ragged.nostrip": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), strip=False, product="f32", ragged=True, **o)),
    "pcm.ragged.enc": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), ragged=True, encoding="ulaw", **o)),
    "pcm.ragged.encs": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), ragged=True, encoding=["alaw", None], **o)),
    "pcm.ragged.encs2": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), strip=False, ragged=True, encoding=["ulaw", "alaw"], **o)),
    "pcm.ragged.flac": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), ragged=True, flac=True, **o)),
    "pcm.ragged.flacs": ("chat", THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), ragged=True, flac=[False, True], encoding=["ulaw", None], **o)),
    "pcm.dec": ("chat", ONE, lambda c, o: c.decode_to_pcm16(ROWS(), **o)),
    "pcm.dec.nostrip": ("chat", ONE_THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), strip=False, **o)),
    "pcm.dec.enc": ("chat", ONE_THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), encoding="alaw", **o)),
    "pcm.dec.flac": ("chat", ONE_THIRD, lambda c, o: c.decode_to_pcm16(ROWS(), flac=True, **o)),
    "pcm.codes": ("chat", ONE, lambda c, o: c.decode_to_pcm16(CODES(), False, **o)),
    "pcm.codes.enc": ("chat", ONE_THIRD, lambda c, o: c.decode_to_pcm16(CODES(), False, strip=False, encoding="ulaw", **o)),
    "pcm.codes.flac": ("chat", ONE_THIRD, lambda c, o: c.decode_to_pcm16(CODES(), False, flac=True, **o)),
    "split": ("chat", FULL, lambda c, o: c.decode_split_to_pcm16(GROUPS(), **o)),
    "split.nostrip": ("chat", THIRD, lambda c, o: c.decode_split_to_pcm16(GROUPS(), strip=False, product="f32", **o)),
    "split.enc": ("chat", THIRD, lambda c, o: c.decode_split_to_pcm16(GROUPS(), encoding="ulaw", **o)),
    "split.encs": ("chat", THIRD, lambda c, o: c.decode_split_to_pcm16(GROUPS(), encoding=[None, "alaw"], **o)),
    "split.flac": ("chat", THIRD, lambda c, o: c.decode_split_to_pcm16(GROUPS(), flac=True, **o)),
    "split.flacs": ("chat", THIRD, lambda c, o: c.decode_split_to_pcm16(GROUPS(), flac=[True, False], encoding=[None, "ulaw"], **o)),
    "finish_group": ("batcher", FULL, _finish_group),
    "finish_group.fmt": ("batcher", THIRD, lambda b, o: _finish_group(b, o, encodings=["ulaw", None], flac=[False, True])),
    "finish": ("batcher", FULL, _finish),
    "finish.enc": ("batcher", THIRD, lambda b, o: _finish(b, o, encoding="ulaw")),
}

ONE_GROUP = lambda: [[torch.zeros(3, 768), torch.zeros(2, 768)]]
D = PA.PauseSpec

# single calls: the refused calls of the host tests and of the calls' own rules, and accepted calls the arrays do not reach
SINGLES = {
    # tests/test_pauses_host.py
    "x.eng.ragged.pauses.field": ("engine", lambda e: e.decode_ragged(ROWS(), pauses=dict(x=1))),
    "x.eng.ragged.pauses.len": ("engine", lambda e: e.decode_ragged(ROWS(), pauses=[True])),
    "x.eng.ragged.pauses.rate": ("engine", lambda e: e.decode_ragged(ROWS(), pauses=True, sample_rate=7000)),
    "x.eng.ragged.pauses.rate10": ("engine", lambda e: e.decode_ragged(ROWS(), pauses=True, sample_rate=11025, loudness=-16)),
    "x.split.pauses.len": ("chat", lambda c: c.decode_split_to_pcm16([ROWS()], pauses=[True, True])),
    "ok.eng.wavs.pauses.dict": ("engine", lambda e: e.decode_to_wavs(ROWS(), sample_rate=8000, speed=1.25, loudness=-16, pauses=dict(tail_ms=0))),
    "ok.split.pauses": ("chat", lambda c: c.decode_split_to_pcm16([ROWS(), [torch.zeros(1, 768)]], pauses=[True, None], loudness=-19.0, sample_rate=8000)),
    # tests/test_limiter_host.py, tests/test_loudness_host.py
    "x.wavs.limiter.flag": ("chat", lambda c: c.decode_to_wavs(ROWS(), limiter="on")),
    "x.split.limiter.len": ("chat", lambda c: c.decode_split_to_pcm16(ONE_GROUP(), limiter=[True, False])),
    "x.wavs.loudness.range": ("chat", lambda c: c.decode_to_wavs(ROWS(), loudness=-60.0)),
    "x.split.loudness.len": ("chat", lambda c: c.decode_split_to_pcm16(ONE_GROUP(), loudness=[-19.0, -20.0])),
    "ok.split.limiter.list": ("chat", lambda c: c.decode_split_to_pcm16(ONE_GROUP(), limiter=[True], loudness=-19.0)),
    "ok.pcm.ragged.limiter.flac": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, limiter=True, loudness=[-16.0, None], flac=True, sample_rate=8000)),
    # the calls' own rules
    "x.eng.ragged.empty": ("engine", lambda e: e.decode_ragged([])),
    "ok.eng.wavs.empty": ("engine", lambda e: e.decode_to_wavs([], sample_rate=8000, limiter=True)),
    "x.eng.ragged.rate.len": ("engine", lambda e: e.decode_ragged(ROWS(), sample_rate=[8000])),
    "x.eng.ragged.rate.len.speed": ("engine", lambda e: e.decode_ragged(ROWS(), sample_rate=[8000], speed=1.25)),
    "x.eng.ragged.rate.len.loudness": ("engine", lambda e: e.decode_ragged(ROWS(), sample_rate=[8000], loudness=-16)),
    "x.eng.ragged.speed.len": ("engine", lambda e: e.decode_ragged(ROWS(), speed=[1.25])),
    "x.eng.ragged.speed.range": ("engine", lambda e: e.decode_ragged(ROWS(), speed=2.5)),
    "x.eng.ragged.loudness.len": ("engine", lambda e: e.decode_ragged(ROWS(), loudness=[-16.0])),
    "x.eng.ragged.loudness.rate": ("engine", lambda e: e.decode_ragged(ROWS(), loudness=-16.0, sample_rate=[8000, 7000])),
    "x.eng.ragged.limiter.len": ("engine", lambda e: e.decode_ragged(ROWS(), limiter=[True])),
    "x.eng.ragged.limiter.rate": ("engine", lambda e: e.decode_ragged(ROWS(), limiter=True, sample_rate=11025)),
    "x.eng.wavs.speed.range": ("engine", lambda e: e.decode_to_wavs(ROWS(), speed=0.4)),
    "x.eng.wavs.loudness.rate": ("engine", lambda e: e.decode_to_wavs(ROWS(), loudness=-16.0, sample_rate=11025)),
    "x.eng.wavs.pauses.rate": ("engine", lambda e: e.decode_to_wavs(ROWS(), pauses=True, sample_rate=50000)),
    "x.eng.wavs.limiter.len": ("engine", lambda e: e.decode_to_wavs(ROWS(), limiter=[True, False, True])),
    "x.eng.wavs.rate.rows": ("engine", lambda e: e.decode_to_wavs(ROWS(), sample_rate=[8000, 16000])),
    "x.eng.wavs.rate.rows.loudness": ("engine", lambda e: e.decode_to_wavs(ROWS(), sample_rate=[8000, 16000], loudness=-16)),
    "x.wavs.dec.rate.rows": ("chat", lambda c: c.decode_to_wavs(ROWS(), sample_rate=[8000, 16000])),
    "x.wavs.codes.rate.rows": ("chat", lambda c: c.decode_to_wavs(CODES(), False, sample_rate=[8000, 16000], limiter=True)),
    "x.pcm.dec.rate.rows": ("chat", lambda c: c.decode_to_pcm16(ROWS(), sample_rate=[8000, 16000], pauses=True)),
    "x.wavs.ragged.codes": ("chat", lambda c: c.decode_to_wavs(CODES(), False, ragged=True)),
    "x.wavs.ragged.pad": ("chat", lambda c: c.decode_to_wavs(ROWS(), True, 4, ragged=True)),
    "x.wavs.speed.range": ("chat", lambda c: c.decode_to_wavs(ROWS(), speed=2.5)),
    "x.wavs.pauses.field": ("chat", lambda c: c.decode_to_wavs(ROWS(), pauses=dict(max_pause_ms=1))),
    "x.pcm.ragged.codes": ("chat", lambda c: c.decode_to_pcm16(CODES(), False, ragged=True)),
    "x.pcm.encoding.name": ("chat", lambda c: c.decode_to_pcm16(ROWS(), encoding="mulaw")),
    "x.pcm.ragged.encoding.name": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, encoding=["mulaw", "ulaw"])),
    "x.pcm.ragged.encoding.len": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, encoding=["ulaw"])),
    "x.pcm.flac.rows": ("chat", lambda c: c.decode_to_pcm16(ROWS(), flac=[True, False])),
    "x.pcm.ragged.flac.len": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, flac=[True])),
    "x.pcm.flac.encoding": ("chat", lambda c: c.decode_to_pcm16(ROWS(), flac=True, encoding="ulaw")),
    "x.pcm.ragged.flac.encoding": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, flac=[True, False], encoding=["ulaw", None])),
    "x.pcm.ragged.flac.encoding.len": ("chat", lambda c: c.decode_to_pcm16(ROWS(), ragged=True, flac=True, encoding=[None])),
    "x.pcm.flac.rows.off": ("chat", lambda c: c.decode_to_pcm16(ROWS(), flac=[False, False], loudness=-16)),
    "ok.pcm.empty": ("chat", lambda c: c.decode_to_pcm16([], sample_rate=8000, pauses=True)),
    "ok.pcm.ragged.empty": ("chat", lambda c: c.decode_to_pcm16([], ragged=True, encoding="ulaw")),
    "ok.pcm.flac.empty": ("chat", lambda c: c.decode_to_pcm16([], flac=True)),
    "ok.wavs.empty": ("chat", lambda c: c.decode_to_wavs([], limiter=True)),
    "ok.wavs.ragged.empty": ("chat", lambda c: c.decode_to_wavs([], ragged=True, speed=1.25)),
    "ok.split.empty": ("chat", lambda c: c.decode_split_to_pcm16([], loudness=-16)),
    "x.split.group.empty": ("chat", lambda c: c.decode_split_to_pcm16([ROWS(), []])),
    "x.split.rate.len": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), sample_rate=[8000])),
    "x.split.speed.len": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), speed=[1.25])),
    "ok.split.speed.len.off": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), speed=[1.0])),
    "x.split.encoding.len": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), encoding=["ulaw"])),
    "x.split.encoding.name": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), encoding="pcm")),
    "x.split.flac.len": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), flac=[True])),
    "x.split.flac.encoding": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), flac=[True, True], encoding=[None, "ulaw"])),
    "x.split.limiter.flag": ("chat", lambda c: c.decode_split_to_pcm16(GROUPS(), limiter=[True, 1])),
    "ok.finish_group.empty.row": ("batcher", lambda b: b.finish_group([torch.zeros(0, 768), torch.zeros(2, 768)], sample_rates=[8000, 16000], pauses=[D(), None],
                                                                      limiter=[True, False], loudness=[-16.0, None], encodings=["ulaw", None], speeds=[1.25, 1.0])),
    "ok.finish_group.off.live": ("batcher", lambda b: b.finish_group([torch.zeros(0, 768), torch.zeros(2, 768)], pauses=[D(), None], limiter=[True, False],
                                                                     loudness=[-16.0, None], encodings=["ulaw", None], flac=[True, False])),
    "x.finish.empty": ("batcher", lambda b: b.finish(torch.zeros(0, 768), limiter=True)),
    "ok.finish.flac": ("batcher", lambda b: b.finish(torch.zeros(3, 768), sample_rate=8000, flac=True, limiter=True)),
}


def cases():
    """(id, who, call(subject)) of the whole table, in a fixed order"""
    out = []
    for name, (who, array, call) in ENTRIES.items():
        for i, o in enumerate(array):
            out.append((f"{name}#{i}", who, lambda s, call=call, o=o: call(s, dict(o))))
    for name, (who, call) in SINGLES.items():
        out.append((name, who, call))
    return out


def _result(r):
    """what a call handed back, as far as the fakes make it meaningful: kinds, dtypes and lengths"""
    if isinstance(r, torch.Tensor) or isinstance(r, np.ndarray):
        return f"{str(r.dtype).replace('torch.', '')}{list(r.shape)}"
    if isinstance(r, (list, tuple)):
        return [_result(x) for x in r]
    if isinstance(r, Exception):
        return {"error": [type(r).__name__, str(r)]}
    return _j(r)


def run(who: str, call):
    """one case -> {"trace": [...], "result": ...} or {"error": [type, message], "trace": [...]}"""
    subject = {"engine": Recorder, "chat": _chat, "batcher": _batcher}[who]()
    calls = subject.calls if who == "engine" else subject.codec.calls if who == "chat" else subject.chat.calls
    try:
        res = call(subject)
    except Exception as e:                                                # noqa: BLE001 -- the refusal IS the record
        return {"error": [type(e).__name__, str(e)], "trace": calls}
    return {"trace": calls, "result": _result(res)}


def record() -> dict:
    out = {}
    for cid, who, call in cases():
        r = run(who, call)
        out[cid] = {"error": r["error"]} if "error" in r else r           # a refused call: the type and the message only
    return out


def pack(table: dict) -> dict:
    """the table as it is kept on disk: every distinct recorded call and every distinct result once, the cases refer to them by index
    (most calls of the table recur in many cases)"""
    calls, results, cases_ = {}, {}, {}
    key = lambda v: json.dumps(v, separators=(",", ":"))
    for cid, r in table.items():
        cases_[cid] = r if "error" in r else {"trace": [calls.setdefault(key(c), len(calls)) for c in r["trace"]],
                                              "result": results.setdefault(key(r["result"]), len(results))}
    return {"calls": [json.loads(k) for k in calls], "results": [json.loads(k) for k in results], "cases": cases_}


def unpack(packed: dict) -> dict:
    """`pack` undone: every case with its calls and its result written out"""
    return {cid: r if "error" in r else {"trace": [packed["calls"][i] for i in r["trace"]], "result": packed["results"][r["result"]]}
            for cid, r in packed["cases"].items()}


def main():
    table = json.loads(json.dumps(record()))
    packed = pack(table)
    assert unpack(packed) == table
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(GOLDEN, "w") as f:
        lines, last = [], None                                            # the cases of one entry point share a line
        for k, v in packed["cases"].items():
            item = f"{json.dumps(k)}: {one(v)}"
            if "#" in k and k.split("#")[0] == last:
                lines[-1] += ", " + item
            else:
                lines.append(item)
            last = k.split("#")[0]
        f.write('{"calls": [\n' + ",\n".join(one(c) for c in packed["calls"]) + '\n],\n"results": ' + one(packed["results"]) + ',\n"cases": {\n'
                + ",\n".join(lines) + "\n}}\n")
    n_err = sum("error" in v for v in table.values())
    print(f"{len(table)} cases ({n_err} refused), {len(packed['calls'])} distinct calls -> {os.path.normpath(GOLDEN)} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()

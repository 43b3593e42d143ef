"""Characterisation trace of the streamed window decode: which decoder entry `CodecEngine.decode_windows` reaches with which host tables,
which stream steps follow it with which pushes, what is converted, companded and copied -- and, one layer up, which streams
`SpeechBatcher._serve_chunks` opens and closes and which keywords it hands to `decode_windows_pcm16`.

A device-free recorder (a `CodecEngine` subclass whose library entries, stream steps, conversions and copies leave a record and hand back
zeros of the real call's shape; the pause step hands back counts by a fixed rule) walks a fixed table of calls and writes what it saw to
tests/golden/windows_trace.json: for an accepted call every recorded call and the kinds and lengths of what came back, for a refused call
the exception's type and message.  tests/test_windows_trace.py replays the table against the working tree.

    python -m oracle.make_windows_trace            # rewrites the JSON: run it at the commit whose behaviour is to be pinned

The table crosses nine per-window options pairwise (rate, speed with and without resampler streams, encoding, FLAC, ADPCM, limiter,
pauses, compressor, pcm16), each on for some windows of the call and off for others, and adds single calls: streams named by two and
three windows, an empty range that still steps its streams, a one-token tail, calls whose windows are all empty, and the refused calls
of the host tests."""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from chattts_amd import _lib
from chattts_amd.engine import CodecEngine
from oracle.make_outchain_trace import _j, _result, covering, pack, unpack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "windows_trace.json")
WINDOW = "ctts_window"                            # eight int32: slot, t_lo, t_hi, c_lo, c_hi, keep, 0, 0


@contextlib.contextmanager
def no_device():
    """the two calls of torch that need a device on the way through `decode_windows`, stubbed"""
    cur, rec = torch.cuda.current_stream, torch.Tensor.record_stream
    torch.cuda.current_stream = lambda device=None: SimpleNamespace(cuda_stream=0)
    torch.Tensor.record_stream = lambda self, stream: None
    try:
        yield
    finally:
        torch.cuda.current_stream, torch.Tensor.record_stream = cur, rec


def _table(ptr, n, dtype):
    """n rows of a host table behind a ctypes pointer -> lists"""
    if ptr is None or n == 0:
        return []
    p = ptr.value if isinstance(ptr, C.c_void_p) else C.cast(ptr, C.c_void_p).value
    if dtype is WINDOW:
        return np.frombuffer(C.string_at(p, n * 32), dtype=np.int32).reshape(n, 8).tolist()
    a = np.frombuffer(C.string_at(p, n * np.dtype(dtype).itemsize), dtype=dtype)
    return [[v.item() if np.ndim(v) == 0 else v.tolist() for v in row] for row in a] if a.dtype.names else a.tolist()


def _rates(ptr, n):
    r = C.cast(ptr, C.POINTER(_lib.Rate))
    return [[r[k].L, r[k].M, r[k].K] for k in range(n)]


class _Lib:
    """the library's window entries: the host-side tables and the scalars of the call, recorded; everything else answers 0"""
    def __init__(self, rec):
        self.rec = rec

    def __getattr__(self, name):
        if not name.startswith("ctts_codec_decode_windows"):
            return lambda *a: 0
        return lambda *a: self.entry(name, a)

    def entry(self, name, a):
        out_type, out, keep_bits, product, keep_thr = a[-8:-3]
        kw = dict(strides=[a[2], a[3]], S=a[4], cap=a[5], out_type=out_type, keep_bits=None if keep_bits is None else keep_bits - out,
                  product=product, keep_thr=keep_thr)
        if name == "ctts_codec_decode_windows":
            kw.update(windows=_table(a[7], a[8], WINDOW))
        elif name == "ctts_codec_decode_windows_rate":
            kw.update(windows=_table(a[7], a[12], WINDOW), rs_windows=_table(a[9], a[12], _lib.RS_WINDOW), rates=_rates(a[13], a[14]))
            n_sel = sum(1 for r in kw["rs_windows"] if r[7] >= 0)
            kw.update(sel=_table(a[11], n_sel, np.int32))
        else:
            kw.update(windows=_table(a[7], a[8], WINDOW), conv=_table(a[10], a[13], WINDOW), rs_windows=_table(a[12], a[13], _lib.RS_WINDOW),
                      round_off=_table(a[16], a[17] + 1, np.int32), slots=a[20])
            kw.update(ts=_table(a[15], kw["round_off"][-1], _lib.TS_STREAM))
            if name == "ctts_codec_decode_windows_speed_rate":
                n_grp = a[27]
                grp_off = _table(a[25], n_grp + 1, np.int32)
                kw.update(rs=_table(a[23], grp_off[-1], _lib.RS_STREAM), rs_of_ts=_table(a[24], len(kw["ts"]), np.int32), grp_off=grp_off,
                          grp_rate=_table(a[26], n_grp, np.int32), rates=_rates(a[28], a[29]), rs_slots=a[31])
        self.rec.rec(name, **kw)
        return 0


class Recorder(CodecEngine):
    """a CodecEngine without a device: the order of the calls is the real code's"""
    def __init__(self):
        self.calls = []
        self.device = torch.device("cpu")
        self.handle = None
        self._fake = _Lib(self)

    lib = property(lambda self: self._fake)

    def rec(self, name, **kw):
        self.calls.append([name, {k: _j(v) for k, v in kw.items()}])

    @staticmethod
    def _windows_store(store):
        return int(store.size(0)), int(store.size(1))

    def _ws_bytes(self, n):
        return torch.zeros(16, dtype=torch.uint8), 16

    def _windows_layout(self, n, keep, pcm16, laws):
        lay = super()._windows_layout(n, keep, pcm16, laws)
        lay[-1].fill_(255)                              # every keep bit set: a stripped window keeps its length
        return lay

    # -- the stream steps: the pushes, recorded; chunks of zeros by fixed rules
    @staticmethod
    def _pushes(pushes):
        return [[None if v is None else int(v) if not isinstance(v, tuple) else list(v) for v in p] for p in pushes]

    def trim_pauses_stream_step(self, x, pushes):
        self.rec("trim_pauses_stream_step", x=x, pushes=self._pushes(pushes))
        counts = [int(p[2]) - int(p[2]) // 5 + (3 if p[3] else 0) for p in pushes]          # the fixed rule
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return torch.zeros(int(off[-1])), off

    def compress_stream_step(self, x, pushes, out=None, out_off=None):
        self.rec("compress_stream_step", x=x, pushes=self._pushes(pushes), out=out, out_off=out_off)
        counts = [int(p[2]) + 144 if p[3] else max(0, int(p[2]) - 144) for p in pushes]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return torch.zeros(int(off[-1])), off

    def peak_limit_stream_step(self, x, pushes, out=None, out_off=None):
        self.rec("peak_limit_stream_step", x=x, pushes=self._pushes(pushes), out=out, out_off=out_off)
        return out, np.asarray(out_off, np.int64)

    def _int16_step(self, name, pcm, pushes, counts, masks):
        self.rec(name, pcm=pcm, pushes=self._pushes(pushes), counts=counts, masks=masks)
        return [np.zeros(int(p[2]) // 4 + (7 if p[3] else 0), np.uint8) for p in pushes]

    def flac_stream_step(self, pcm, pushes, counts=None, masks=None):
        return self._int16_step("flac_stream_step", pcm, pushes, counts, masks)

    def adpcm_stream_step(self, pcm, pushes, counts=None, masks=None):
        return self._int16_step("adpcm_stream_step", pcm, pushes, counts, masks)

    # -- the conversions and the copies
    def float_to_int16_ragged(self, wav, off, product="f64", keep_thr=None, out=None):
        self.rec("float_to_int16_ragged", wav=wav, off=off, product=product, keep_thr=keep_thr, out=out)
        return out[0], out[1], None

    def g711_encode(self, pcm, ranges, out=None):
        self.rec("g711_encode", pcm=pcm, ranges=ranges, out=out)
        return out

    def to_host(self, t):
        self.rec("to_host", t=t)
        return t.contiguous().numpy()


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
# (slot, prefix tokens, s_lo, s_hi[, tail]): a first chunk, an interior chunk, one clipped by its prefix's end, a tail, a one-token tail,
# a range with no sample in it
WINS = [(0, 24, 0, 12000, False), (1, 96, 24000, 36000, False), (2, 30, 12000, 24000), (3, 72, 20000, None, True), (4, 1, 0, None, True),
        (0, 24, 12032, 24000, False)]
RATES = [8000, 16000, 24000, 8000, 24000, 16000]
SPEEDS = [1.25, 1.0, 0.5, 1.0, 1.25, 0.77]
ON = {"limiter": {0, 1, 3, 5}, "pauses": {0, 2, 3, 5}, "compress": {1, 2, 3, 5}, "flac": {0, 3}, "adpcm": {1, 4, 5}, "encoding": {2}}
STAGES = {"limiter": ("limiter", "lm_streams", lambda e, r: e.peak_limit_stream_open(r)),
          "pauses": ("pauses", "pa_streams", lambda e, r: e.trim_pauses_stream_open(r)),
          "compress": ("compress", "cp_streams", lambda e, r: e.compress_stream_open(r)),
          "flac": ("flac", "flac_streams", lambda e, r: e.flac_stream_open(r)),
          "adpcm": ("adpcm", "adpcm_streams", lambda e, r: e.adpcm_stream_open(r))}
VALUES = {"rate": [False, True], "speed": [False, "streams", "no_rs"], "encoding": [False, True], "flac": [False, True], "adpcm": [False, True],
          "limiter": [False, True], "pauses": [False, True], "compress": [False, True], "pcm16": [True, False], "keep_thr": [None, 1e-5]}


def store():
    return torch.zeros((8, 160, 768))


def call(eng, o, wins=WINS, share=(), all_on=False, **kw):
    """the `decode_windows` call of one row of options, its streams opened as the row asks (a fresh engine: nothing is closed)"""
    n = len(wins)
    first = {j: i for i, j in share}
    rates = [RATES[i % 6] for i in range(n)] if o.get("rate") else None
    for i, j in share if rates is not None else ():
        rates[j] = rates[i]
    rate = lambda i: 24000 if rates is None else rates[i]

    def handles(flags, open_one):
        hs = [None] * n
        for i in range(n):
            if flags[i]:
                hs[i] = hs[first[i]] if i in first and flags[first[i]] else open_one(i)
        return hs
    if rates is not None:
        kw["sample_rates"] = rates
    if o.get("speed"):
        speeds = [SPEEDS[i % 6] for i in range(n)]
        for i, j in share:
            speeds[j] = speeds[i]
        kw["speeds"] = speeds
        kw["ts_streams"] = handles([v != 1.0 for v in speeds], lambda i: eng.time_scale_stream_open(speeds[i]))
        if o["speed"] == "streams" and rates is not None:
            kw["rs_streams"] = handles([v != 1.0 and rate(i) != 24000 for i, v in enumerate(speeds)], lambda i: eng.resample_stream_open(24000, rate(i)))
    if o.get("encoding"):
        kw["encodings"] = [("ulaw", "alaw")[i % 2] if all_on or i in ON["encoding"] else None for i in range(n)]
    for stage, (arg, arg_streams, open_one) in STAGES.items():
        if o.get(stage):
            flags = [all_on or i % 6 in ON[stage] for i in range(n)]
            kw[arg] = flags if stage in ("limiter", "flac", "adpcm") else [True if f else None for f in flags]
            kw[arg_streams] = handles(flags, lambda i: open_one(eng, rate(i)))
    return eng.decode_windows(store(), wins, pcm16=o.get("pcm16", True), keep_thr=o.get("keep_thr"), **kw)


TWICE = [(0, 24, 0, 6000, False), (1, 96, 24000, 36000, False), (0, 24, 6000, None, True), (1, 96, 36000, 40000, False), (1, 96, 40000, None, True)]
PAIRS = [(0, 2), (1, 3), (1, 4)]
GONE = [(0, 24, 12032, None, True), (0, 24, 12032, 24000, False), (2, 0, 0, 100)]
GONE_S = [(0, 24, 12032, None, False)] + GONE[1:]          # an empty stream cannot end: the scaler refuses that tail
ALL3 = dict(limiter=True, pauses=True, compress=True)
TWO = [(0, 40, 0, 12000), (1, 40, 0, 12000, True)]
SPEC = SimpleNamespace(dim=lambda: 3, dtype=torch.float32, is_cuda=True, size=lambda i: (2, 64, 768)[i], stride=lambda i: 1)


def _refusals():
    """the refused calls of tests/test_*_stream_host.py, test_timescale_stream_host.py and test_resample_stream_host.py"""
    out = {}
    stages = {"limiter": ("limiter", "lm_streams", "peak_limit_stream_open", False), "compress": ("compress", "cp_streams", "compress_stream_open", None),
              "pauses": ("pauses", "pa_streams", "trim_pauses_stream_open", None), "flac": ("flac", "flac_streams", "flac_stream_open", False),
              "adpcm": ("adpcm", "adpcm_streams", "adpcm_stream_open", False)}
    for s, (arg, st, opener, off) in stages.items():
        def rows(e, arg=arg, st=st, opener=opener, off=off):
            h24, h8 = getattr(e, opener)(24000), getattr(e, opener)(8000)
            return {"flags.len": {arg: [True], st: [h24, None]}, "streams.none": {arg: [True, False]}, "stream.none": {arg: [True, off], st: [None, None]},
                    "stream.rate": {arg: [True, False], st: [h8, None]}, "stream.rate8": {arg: [True, False], st: [h24, None], "sample_rates": [8000, 24000]},
                    "names": {arg: [False, True], st: [h24, h24]}, "no.flag": {arg: [False, off], st: [h24, None]}, "only.streams": {st: [None, h24]},
                    "f32": {arg: [True, False], st: [h24, None], "pcm16": False}, "encoding": {arg: [True, False], st: [h24, None], "encodings": ["ulaw", None]},
                    "ok.encoding.other": {arg: [True, False], st: [h24, None], "encodings": [None, "ulaw"]},
                    "tail.then": {arg: [True, True], st: [h24, h24], "windows": [TWO[1], TWO[0]]},
                    "all.faults": {arg: [True], st: [h24], "speeds": [1.25], "encodings": ["x"], "sample_rates": [1]}}
        for k in rows(Recorder()):
            def one(e, k=k, rows=rows):
                kw = rows(e)[k]
                return e.decode_windows(store(), kw.pop("windows", TWO), **kw)
            out[f"x.{s}.{k}"] = one
    out["x.limiter.flag"] = lambda e: e.decode_windows(None, TWO, limiter=[1, False], lm_streams=[e.peak_limit_stream_open(24000), None])
    out["x.flac.and.adpcm"] = lambda e: e.decode_windows(None, TWO, flac=[True, False], flac_streams=[e.flac_stream_open(24000), None],
                                                         adpcm=[True, True], adpcm_streams=[e.adpcm_stream_open(24000), e.adpcm_stream_open(24000)])
    out["x.order"] = lambda e: e.decode_windows(None, TWO, compress=[True], pauses=[True], limiter=[True], flac=[True], adpcm=[True], speeds=[1.0], encodings=[1])
    out["x.order.pauses"] = lambda e: e.decode_windows(None, TWO, pauses=[True], limiter=[True], flac=[True], adpcm=[True], speeds=[1.0], encodings=[1])
    out["x.order.limiter"] = lambda e: e.decode_windows(None, TWO, limiter=[True], flac=[True], adpcm=[True], speeds=[1.0], encodings=[1])
    out["x.order.flac"] = lambda e: e.decode_windows(None, TWO, flac=[True], adpcm=[True], speeds=[1.0], encodings=[1])
    out["x.order.adpcm"] = lambda e: e.decode_windows(None, TWO, adpcm=[True], speeds=[1.0], encodings=[1])
    out["x.order.speeds"] = lambda e: e.decode_windows(None, TWO, speeds=[1.0], encodings=[1])
    # test_timescale_stream_host.py, test_resample_stream_host.py
    out["x.speed.rate"] = lambda e: e.decode_windows(None, TWO, speeds=[1.25, 1.0], ts_streams=[0, None], sample_rates=[24000, 8000])
    out["x.speed.no.streams"] = lambda e: e.decode_windows(None, TWO, speeds=[1.25, 1.0])
    out["x.speed.len"] = lambda e: e.decode_windows(None, TWO, speeds=[1.25])
    out["x.speed.range"] = lambda e: e.decode_windows(None, TWO, speeds=[1.25, 3.0], ts_streams=[0, None])
    out["x.speed.stream.len"] = lambda e: e.decode_windows(None, TWO, speeds=[1.25, 1.0], ts_streams=[0])
    out["x.speed.stream.none"] = lambda e: e.decode_windows(SPEC, TWO, speeds=[1.25, 1.0], ts_streams=[None, None])
    out["x.speed.stream.other"] = lambda e: e.decode_windows(SPEC, TWO, speeds=[1.25, 1.0], ts_streams=[e.time_scale_stream_open(1.5), None])
    out["x.speed.one.names"] = lambda e: e.decode_windows(SPEC, TWO, speeds=[1.25, 1.0], ts_streams=[e.time_scale_stream_open(1.25)] * 2)

    def rs(streams, speeds=(1.25, 1.0), ts=None):
        def one(e):
            t = e.time_scale_stream_open(1.25)
            r16, r8 = e.resample_stream_open(24000, 16000), e.resample_stream_open(24000, 8000)
            return e.decode_windows(SPEC, TWO, speeds=list(speeds), ts_streams=[t, t if ts else None], sample_rates=[8000, 24000],
                                    rs_streams=[{"r8": r8, "r16": r16}.get(s) for s in streams])
        return one
    out["x.rs.len"], out["x.rs.none"], out["x.rs.other"] = rs([None]), rs([None, None]), rs(["r16", None])
    out["x.rs.one.names"], out["x.rs.stays"] = rs(["r8", "r16"]), rs(["r8", "r16"], (1.25, 1.25), True)
    out["x.rs.alone.names"] = lambda e: e.decode_windows(SPEC, TWO, speeds=[1.25, 1.0], ts_streams=[e.time_scale_stream_open(1.25), None],
                                                         sample_rates=[24000, 8000], rs_streams=[None, e.resample_stream_open(24000, 8000)])
    out["x.rate.len"] = lambda e: e.decode_windows(SPEC, TWO, sample_rates=[8000])
    out["x.rate.bad"] = lambda e: e.decode_windows(store(), TWO, sample_rates=[8000, 7])
    out["x.encoding.len"] = lambda e: e.decode_windows(None, TWO, encodings=["ulaw"])
    out["x.encoding.name"] = lambda e: e.decode_windows(None, TWO, encodings=["mulaw", None])
    out["x.encoding.f32"] = lambda e: e.decode_windows(None, TWO, encodings=["ulaw", None], pcm16=False)
    out["x.window.slot"] = lambda e: e.decode_windows(store(), [(8, 4, 0, 100)])
    out["x.window.cap"] = lambda e: e.decode_windows(store(), [(0, 4, 0, 100), (1, 161, 0, 100)], limiter=[True, True],
                                                     lm_streams=[e.peak_limit_stream_open(24000), e.peak_limit_stream_open(24000)])
    out["x.window.cap.speed"] = lambda e: e.decode_windows(store(), [(0, 4, 0, 100), (1, 161, 0, 100)], speeds=[1.25, 1.0],
                                                           ts_streams=[e.time_scale_stream_open(1.25), None])
    out["x.window.cap.rate"] = lambda e: e.decode_windows(store(), [(0, 4, 0, 100), (1, 161, 0, 100)], sample_rates=[8000, 8000])
    return out


def cases():
    """(id, call(engine)) of the whole table, in a fixed order"""
    out = []
    for i, o in enumerate(covering(VALUES, seed=2)):
        out.append((f"cross#{i}", lambda e, o=o: call(e, dict(o))))
    # the rows above that pair pcm16=False with an int16 stage, or a speed and a rate without resampler streams, are refused: the
    # pairs of the options that go together, once more, among calls that are accepted
    for i, o in enumerate(covering({k: [x for x in v if x != "no_rs"] for k, v in VALUES.items() if k != "pcm16"}, seed=3)):
        out.append((f"pcm16#{i}", lambda e, o=o: call(e, dict(o))))
    every = dict(ALL3, keep_thr=1e-5)
    singles = {
        "ok.plain": lambda e: call(e, {}), "ok.plain.f32.keep": lambda e: call(e, dict(pcm16=False, keep_thr=1e-5)),
        "ok.rate.keep": lambda e: call(e, dict(rate=True, keep_thr=1e-5)), "ok.speed.keep": lambda e: call(e, dict(speed="streams", keep_thr=1e-5)),
        "ok.speed.rate.keep": lambda e: call(e, dict(speed="streams", rate=True, keep_thr=1e-5, encoding=True)),
        "ok.encoding.all": lambda e: call(e, dict(encoding=True, keep_thr=1e-5), all_on=True),
        "ok.flac.all": lambda e: call(e, dict(flac=True, keep_thr=1e-5), all_on=True),
        "ok.adpcm.all.rate": lambda e: call(e, dict(adpcm=True, rate=True), all_on=True),
        "ok.three": lambda e: call(e, every), "ok.three.all": lambda e: call(e, every, all_on=True),
        "ok.three.all.f32": lambda e: call(e, dict(every, pcm16=False), all_on=True),
        "ok.three.all.flac": lambda e: call(e, dict(every, flac=True), all_on=True),
        "ok.three.all.encoding": lambda e: call(e, dict(every, encoding=True), all_on=True),
        "ok.three.all.speed.rate": lambda e: call(e, dict(every, speed="streams", rate=True, adpcm=True), all_on=True),
        "ok.three.product": lambda e: call(e, every, product="f32"),
        "ok.twice.limiter": lambda e: call(e, dict(limiter=True, keep_thr=1e-5), TWICE, PAIRS, True),
        "ok.twice.pauses": lambda e: call(e, dict(pauses=True, keep_thr=1e-5), TWICE, PAIRS, True),
        "ok.twice.compress": lambda e: call(e, dict(compress=True), TWICE, PAIRS, True),
        "ok.twice.flac": lambda e: call(e, dict(flac=True, keep_thr=1e-5), TWICE, PAIRS, True),
        "ok.twice.adpcm.rate": lambda e: call(e, dict(adpcm=True, rate=True), TWICE, PAIRS, True),
        "ok.twice.speed": lambda e: call(e, dict(speed="streams", keep_thr=1e-5), TWICE, PAIRS),
        "ok.twice.every": lambda e: call(e, dict(every, flac=True, speed="streams", rate=True), TWICE, PAIRS, True),
        "ok.gone": lambda e: call(e, {}, GONE), "ok.gone.rate": lambda e: call(e, dict(rate=True), GONE),
        "ok.gone.speed": lambda e: call(e, dict(speed="streams", keep_thr=1e-5), GONE_S),
        "x.gone.speed.tail": lambda e: call(e, dict(speed="streams", keep_thr=1e-5), GONE),
        "ok.gone.flac": lambda e: call(e, dict(flac=True), GONE, all_on=True), "ok.gone.three": lambda e: call(e, every, GONE, all_on=True),
        "ok.gone.three.f32": lambda e: call(e, dict(every, pcm16=False), GONE, all_on=True),
        "ok.gone.three.adpcm.speed.rate": lambda e: call(e, dict(every, adpcm=True, speed="streams", rate=True), GONE_S, all_on=True),
        "ok.gone.three.some": lambda e: call(e, dict(every, flac=True), GONE),
        "ok.no.windows": lambda e: e.decode_windows(store(), []),
        "ok.flags.off": lambda e: e.decode_windows(store(), TWO, limiter=[False, None], pauses=[None, False], compress=[False, False], flac=[False, False],
                                                   adpcm=[False, False], speeds=[1.0, 1.0], encodings=[None, None], sample_rates=[24000, 24000]),
    }
    out += list(singles.items()) + list(_refusals().items())
    return out


def run(call_):
    eng = Recorder()
    try:
        with no_device():
            res = call_(eng)
    except Exception as e:                                                # noqa: BLE001 -- the refusal IS the record
        return {"error": [type(e).__name__, str(e)], "trace": eng.calls}
    return {"trace": eng.calls, "result": _result(res)}


# ---- the second section: two polls of SpeechBatcher._serve_chunks over four jobs -------------------------------------------------------
class _ServeCodec:
    """the opens and closes of the stages' streams, logged; a handle is 10 x the stage's place + the opens of that stage so far"""
    OPENS = ("time_scale_stream_open", "resample_stream_open", "flac_stream_open", "adpcm_stream_open", "peak_limit_stream_open",
             "trim_pauses_stream_open", "compress_stream_open")

    def __init__(self):
        self.log, self.count = [], {}

    def __getattr__(self, name):
        if name in self.OPENS:
            def open_(*args):
                self.count[name] = self.count.get(name, 0) + 1
                self.log.append(["open", name, _j(list(args))])
                return 10 * self.OPENS.index(name) + self.count[name]
            return open_
        if name.replace("_close", "_open") in self.OPENS:
            return lambda h: self.log.append(["close", name, h])
        raise AttributeError(name)


def serve_trace() -> dict:
    """four streamed jobs, each with its own option mix, through two polls of `_serve_chunks`, then resolved: per job the opens of its
    streams in their order (a job is known by its speed or its output rate), per poll the keywords `decode_windows_pcm16` receives,
    per job the closes, and the batcher's counts"""
    import queue
    from concurrent.futures import Future

    from chattts_amd import compressor as CP, pauses as PA, serving

    class Sink(Future):
        def __init__(self):
            super().__init__()
            self._q = queue.Queue()

    class Chat:
        codec, calls = _ServeCodec(), []

        def decode_windows_pcm16(self, store, windows, **kw):
            self.calls.append({"windows": _j(list(windows)), "kw": _j(kw)})
            return [np.zeros(3, np.int16) for _ in windows]
    b = serving.SpeechBatcher.__new__(serving.SpeechBatcher)
    b.chat, b._jobs, b._splits, b._sub = Chat(), {}, {}, {}
    b.pool = SimpleNamespace(hiddens=None, cancel=lambda rid: None)
    counts = ("stream_decode_calls", "max_stream_group", "stream_chunks", "stream_resampled_chunks", "companded", "stream_scaled_chunks",
              "stream_flac_chunks", "stream_adpcm_chunks", "stream_limited_chunks", "stream_paused_chunks", "stream_compressed_chunks",
              "cancelled", "failed", "completed", "flac_encoded", "adpcm_encoded", "trimmed")
    for k in counts:
        setattr(b, k, 0)
    mixes = {"A": dict(sample_rate=8000, speed=1.25, encoding="ulaw", compress=CP.check(True)),
             "B": dict(speed=0.8, flac=True, limiter=True, lm_gain=np.float32(2.0)),
             "C": dict(sample_rate=16000, limiter=True, pauses=PA.check(True)),
             "D": dict(sample_rate=44100, adpcm=True, compress=CP.check({"hold_ms": 100}), pauses=PA.check({"tail_ms": 0})),
             "E": dict()}
    for rid, kw in mixes.items():
        b._jobs[rid] = serving._Job(rid, "text", None, Sink(), **kw)
    key = {1.25: "A", 8000: "A", 0.8: "B", 24000: "B", 16000: "C", 44100: "D"}
    polls = [[("A", 0, 24, 0, 12000, False), ("B", 1, 24, 0, 12000, False), ("C", 2, 30, 0, 12000, False), ("E", 4, 30, 0, 12000, False)],
             [("A", 0, 48, 12000, 24000, False), ("D", 3, 24, 0, 12000, False), ("C", 2, 30, 12000, 15104, True), ("gone", 5, 9, 0, 1, False),
              ("B", 1, 30, 12000, 15104, True)]]
    for chunks in polls:
        b._serve_chunks(SimpleNamespace(chunks=chunks))
    opens = {}
    for kind, name, args in b.chat.codec.log:
        assert kind == "open"
        opens.setdefault(key[args[0] if name == "time_scale_stream_open" else args[1] if name == "resample_stream_open" else args[0]], []).append([name, args])
    closes = {}
    for rid in mixes:
        n = len(b.chat.codec.log)
        b._resolve(b._jobs[rid])
        closes[rid] = [e[1:] for e in b.chat.codec.log[n:]]
    return {"opens": opens, "calls": b.chat.calls, "closes": closes, "counts": {k: int(getattr(b, k)) for k in counts}}


def record() -> dict:
    out = {}
    for cid, c in cases():
        r = run(c)
        out[cid] = {"error": r["error"]} if "error" in r else r               # a refused call: the type and the message only
    return out


def main():
    table = json.loads(json.dumps(record()))
    packed = pack(table)
    assert unpack(packed) == table
    serve = json.loads(json.dumps(serve_trace()))
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(GOLDEN, "w") as f:
        f.write('{"calls": [\n' + ",\n".join(one(c) for c in packed["calls"]) + '\n],\n"results": ' + one(packed["results"]) + ',\n"cases": {\n'
                + ",\n".join(f"{json.dumps(k)}: {one(v)}" for k, v in packed["cases"].items()) + '\n},\n"serve": {\n'
                + ",\n".join(f"{json.dumps(k)}: {one(v)}" for k, v in serve.items()) + "\n}}\n")
    n_err = sum("error" in v for v in table.values())
    print(f"{len(table)} cases ({n_err} refused), {len(packed['calls'])} distinct calls -> {os.path.normpath(GOLDEN)} ({os.path.getsize(GOLDEN)} bytes)")
    for k, v in table.items():
        if "error" in v:
            print(" ", k, v["error"])


if __name__ == "__main__":
    main()

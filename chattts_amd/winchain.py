"""The streamed stages of the window decode, once: the table `CodecEngine.decode_windows`, `Chat.decode_windows_pcm16` and
`SpeechBatcher` read instead of spelling the stages out, the streams of one streamed utterance (`StreamSet`), the record of one window
of a `decode_windows` call and the rule that sorts a call's windows into decoder passes.  Host code only: no kernel, no library call."""
from typing import Callable, NamedTuple, Optional

from . import limiter as LM

SAMPLE_RATE = 24000


class Stage(NamedTuple):
    name: str                 # the label of the stage's state pool
    kind: str                 # "time": in front of the float chunk (inside the decoder entry); "float": on the float chunk; "int16": behind the conversion
    flag: str                 # decode_windows' per-window flag argument ...
    streams: str              # ... and its per-window stream argument
    title: str                # what the messages call the stream
    open: str                 # the engine's methods
    close: str
    flagged: Optional[Callable] = None    # a stage with flags of its own: a flag value -> the window is flagged
    step: Optional[str] = None        # a "float" stage in front of the limiter: its step method, run round by round
    counter: Optional[str] = None     # SpeechBatcher's count of the stage's chunks
    any_flag: Optional[Callable] = None   # what makes a call look at the flags at all, where that is not `flagged`
    optional: bool = False    # the stream argument may be left out with the flag given


_on = lambda f: f is not None and f is not False
# in the order a request's streams are opened and closed; the float stages among them in the order they run
STAGES = (
    Stage("time_scale", "time", "speeds", "ts_streams", "time-scale", "time_scale_stream_open", "time_scale_stream_close",
          counter="stream_scaled_chunks"),
    Stage("resample", "time", "speeds", "rs_streams", "resampler", "resample_stream_open", "resample_stream_close", optional=True),
    Stage("flac", "int16", "flac", "flac_streams", "FLAC", "flac_stream_open", "flac_stream_close", bool, counter="stream_flac_chunks"),
    Stage("adpcm", "int16", "adpcm", "adpcm_streams", "ADPCM", "adpcm_stream_open", "adpcm_stream_close", bool, counter="stream_adpcm_chunks"),
    Stage("limiter", "float", "limiter", "lm_streams", "limiter", "peak_limit_stream_open", "peak_limit_stream_close",
          lambda f: LM.check_flag(f, "decode_windows"), counter="stream_limited_chunks", any_flag=bool),
    Stage("pauses", "float", "pauses", "pa_streams", "pause", "trim_pauses_stream_open", "trim_pauses_stream_close", _on,
          step="trim_pauses_stream_step", counter="stream_paused_chunks"),
    Stage("compress", "float", "compress", "cp_streams", "compressor", "compress_stream_open", "compress_stream_close", _on,
          step="compress_stream_step", counter="stream_compressed_chunks"),
)
STAGE = {s.name: s for s in STAGES}
PLACE = {s.name: k for k, s in enumerate(STAGES)}       # a stage's place in `Window.h`
# the order `decode_windows` checks the flagged stages in: a call with several faults is refused for the first of these
CHECKED = tuple(STAGE[n] for n in ("compress", "pauses", "limiter", "flac", "adpcm"))
ROUNDS = tuple(s for s in STAGES if s.step)       # the float stages in front of the limiter, in the order they run


class StreamSet(dict):
    """The streams of one streamed utterance: stage name -> its handle; a stage that is off has no entry (`get`: None)."""

    @staticmethod
    def needed(rate=None, speed=None, pauses=None, compress=None, limiter: bool = False, limiter_gain=None, flac: bool = False,
               adpcm: bool = False) -> dict:
        """the options of one request (None / False: off; `rate` None: 24000 Hz; the limiter is on with `limiter` or a `limiter_gain`,
        its gain 1.0 when None) -> stage name -> the arguments of its open, for exactly the stages the options need: the scaler's at a
        speed, the resampler's at a speed and a rate, every other at the output rate"""
        out_rate = SAMPLE_RATE if rate is None else rate
        args = {"time_scale": speed is not None and (speed,), "resample": speed is not None and rate is not None and (SAMPLE_RATE, rate),
                "flac": flac and (out_rate,), "adpcm": adpcm and (out_rate,),
                "limiter": (limiter or limiter_gain is not None) and (out_rate, 1.0 if limiter_gain is None else limiter_gain),
                "pauses": pauses is not None and (out_rate, pauses), "compress": compress is not None and (out_rate, compress)}
        return {k: v for k, v in args.items() if v}

    @classmethod
    def open(cls, codec, **options) -> "StreamSet":
        """the streams `needed(**options)` names, opened in the table's order.  An open that fails closes what the set had opened and
        re-raises."""
        args, self = cls.needed(**options), cls()
        try:
            for s in STAGES:
                if s.name in args:
                    self[s.name] = getattr(codec, s.open)(*args[s.name])
        except BaseException:
            self.close(codec)
            raise
        return self

    def close(self, codec) -> None:
        """every held handle goes back, once, in the order of the opens; a second call finds nothing to give back"""
        for name in list(self):
            getattr(codec, STAGE[name].close)(self.pop(name))


class Window(NamedTuple):
    """one window of a `decode_windows` call, checked"""
    i: int                    # its place in the call
    slot: int
    Tn: int
    s_lo: int
    hi: int                   # s_hi, or the end of the prefix's decode
    tail: bool                # marked as one: the last push of its streams; with a `keep_thr` it is stripped
    rate: int
    q: tuple                  # the speed, quantised: (num, den)
    scaled: bool              # q is not 1
    law: int                  # -1, or the G.711 law of its encoding
    h: tuple                  # per stage, in the table's order (`PLACE`), its stream's handle or None
    staged: bool              # behind a float stage
    codec: Optional[tuple]    # (stage name, handle) of its FLAC or ADPCM stream


def _split(ws, scaled: bool, rated: bool):
    """the windows of one group -> its (kind, windows) passes: the windows at speed 1 and another rate leave a group that scales"""
    if scaled and any(w.scaled for w in ws):
        alone = [w for w in ws if not w.scaled and w.rate != SAMPLE_RATE] if rated else []
        return [("speed", [w for w in ws if w.scaled or w.rate == SAMPLE_RATE] if alone else ws)] + ([("rate", alone)] if alone else [])
    return [("rate" if rated and any(w.rate != SAMPLE_RATE for w in ws) else "plain", ws)]


def passes(ws, scaled: bool = True, rated: bool = True):
    """a call's windows -> (free, held): the decoder passes as lists of (kind, windows), kind "plain" | "rate" | "speed".  `free`: the
    windows behind no float stage, one group; `held`: the others, the scaled ones and the rest a group (and a pass) each.  A group is
    what shares the checks of the speeds' streams, the companding and the epilogue's layout.  `scaled` / `rated` False: the caller
    knows that no window is at another speed / rate, and nothing is scanned for one."""
    free, held = [], []
    for w in ws:
        (held if w.staged else free).append(w)
    groups = ([w for w in held if w.scaled], [w for w in held if not w.scaled]) if scaled else (held,)
    return (_split(free, scaled, rated) if free else []), [p for g in groups if g for p in _split(g, scaled, rated)]

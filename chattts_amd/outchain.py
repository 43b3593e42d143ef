"""The float32 stages behind the ISTFT -- time_scale, resample, trim_pauses, equalize, compress, loudness_normalize (+ limiter) -- as ONE plan and ONE
chain ("The output chain").  Every decode call builds a `Plan` from its public options, before anything is decoded: each
option is then off (None) or holds what the stages are handed, and every refusal has been carried out.  `run` takes a decoded
waveform through the stages that are on, in the one order the project guarantees.  The validators (timescale.quantize,
loudness.per_row / check_target / check_rate, pauses.per_row / check / check_rate, compressor.per_row / check, equalizer.per_row /
check, limiter.per_row / check_flag) stay the single source of each rule and each message."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from . import compressor as CP
from . import equalizer as EQ
from . import limiter as LM
from . import loudness as LN
from . import pauses as PA
from . import timescale as TS

SAMPLE_RATE = 24000                    # what the acoustic decoder produces
STAGES = ("speed", "loudness", "pauses", "compress", "limiter", "eq")


def option_kw(options: dict, rows=None) -> dict:
    """lists with one entry per row -> keyword arguments that are ABSENT WHEN OFF: a list that is None, or in which no entry (of
    `rows`, when given) is set -- None, or False for a flag -- is not passed on, so a callee that has never heard of the option is
    called as it always was"""
    out = {}
    for name, vals in options.items():
        if vals is not None:
            vals = list(vals) if rows is None else [vals[i] for i in rows]
            if any(v is not None and v is not False for v in vals):
                out[name] = vals
    return out


def _per_row(value, n: int, kind, what: str, who: str):
    """None, one for all or one per row -> None or a list of n"""
    if value is None:
        return None
    vals = [kind(value)] * n if np.ndim(value) == 0 else [kind(v) for v in value]
    if len(vals) != n:
        raise ValueError(f"{who}: one {what} per row, or one for all")
    return vals


def _given(value, check, is_list: bool, on=lambda vals: any(v is not None for v in vals)):
    """an option as it was written, one for all or a list, every entry through its validator -> None when no entry is on"""
    if value is None:
        return None
    vals = [check(v) for v in (list(value) if is_list else [value])]
    if not on(vals):
        return None
    return vals if is_list else vals[0]


def _speed(v) -> float:
    TS.quantize(v)                     # ValueError outside 0.5 .. 2.0
    return float(v)


@dataclass(frozen=True)
class Plan:
    """what one decode call does behind the ISTFT.  Every field is None when its stage is off.  The engine's plans (`rows`,
    `batch`) hold one value per row, as the stages take them; `given` holds the options as the caller wrote them, one for all or a
    list, as they cross the seam to the engine."""
    who: str
    sample_rate: object = None         # rows: one rate per row; batch, given: one rate (given with per-row rates: as written)
    speed: object = None
    loudness: object = None
    pauses: object = None
    limiter: object = None
    rates: object = SAMPLE_RATE        # the rate(s) of the result, which trim_pauses, compress and loudness_normalize are told
    compress: object = None            # the compressor's spec(s): its stage runs behind `pauses` and in front of `loudness`
    eq: object = None                  # the equaliser's spec(s): its stage runs behind `pauses` and in front of `compress`

    @property
    def on(self) -> bool:
        return any(v is not None for v in (self.sample_rate, self.speed, self.loudness, self.pauses, self.eq, self.compress, self.limiter))

    @property
    def levels(self) -> bool:
        """does the last float32 stage run (loudness_normalize, with or without the limiter behind its gain)"""
        return self.loudness is not None or self.limiter is not None

    def kwargs(self, *names) -> dict:
        """the stages that are on as keyword arguments, absent when off (`sample_rate` only when named: the decode calls take it
        always)"""
        return {k: getattr(self, k) for k in (names or STAGES) if getattr(self, k) is not None}

    def row_rates(self, n: int) -> list:
        """the result's rate, one per row"""
        return [int(self.rates)] * n if np.ndim(self.rates) == 0 else [int(r) for r in self.rates]

    # -- the engine's plans: one value per row, every refusal carried out ---------------------------------------------------------------
    @staticmethod
    def _check_rates(rates, lims, specs, targets, comps=None, eqs=None, who: str = "equalize"):
        for r in rates if lims is not None or comps is not None or eqs is not None else ():
            LN.check_rate(r)
        if eqs is not None:                # a section's frequency is held to 0.45 of ITS row's rate
            for r, e in zip(rates if len(rates) == len(eqs) else list(rates) * len(eqs), eqs):
                EQ.check(e, who, r)
        for r in rates:
            if specs is not None:
                PA.check_rate(r)
            if targets is not None:
                LN.check_rate(r)

    @classmethod
    def rows(cls, who: str, n: int, sample_rate=None, speed=None, loudness=None, pauses=None, limiter=None, compress=None, eq=None) -> "Plan":
        """packed rows, every option one for all or one per row (CodecEngine.decode_ragged).  A rate that is given is a stage that
        runs, 24000 included (resample_segments copies such rows)."""
        lims = LM.per_row(limiter, n, who)
        specs = PA.per_row(pauses, n, who)
        comps = CP.per_row(compress, n, who)
        eqs = EQ.per_row(eq, n, who)
        rates = _per_row(sample_rate, n, int, "sample rate", who)
        targets = LN.per_row(loudness, n, who)
        out_rates = [SAMPLE_RATE] * n if rates is None else rates
        cls._check_rates(out_rates, lims, specs, targets, comps, eqs, who)
        speeds = _per_row(speed, n, float, "speed", who)
        if speeds is not None and all(TS.quantize(v)[0] == TS.DEN for v in speeds):
            speeds = None
        return cls(who, rates, speeds, targets, specs, lims, out_rates, comps, eqs)

    @classmethod
    def batch(cls, who: str, n: int, sample_rate=None, speed=None, loudness=None, pauses=None, limiter=None, compress=None, eq=None) -> "Plan":
        """a zero-padded [B, n] batch: one rate and one speed for all rows, the rest one for all or one per row
        (CodecEngine.decode_to_wavs).  24000 Hz is no stage, except behind the time scaler (where `resample` hands its input back)."""
        lims = LM.per_row(limiter, n, who)
        specs = PA.per_row(pauses, n, who)
        comps = CP.per_row(compress, n, who)
        eqs = EQ.per_row(eq, n, who)
        targets = LN.per_row(loudness, n, who)
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        cls._check_rates([rate], lims, specs, targets, comps, eqs, who)
        if speed is not None and TS.quantize(speed)[0] == TS.DEN:
            speed = None
        if sample_rate is not None and speed is None and rate == SAMPLE_RATE:
            sample_rate = None
        return cls(who, None if sample_rate is None else rate, speed, targets, specs, lims, rate, comps, eqs)

    # -- Chat's plan: the options as they were written, checked value by value ---------------------------------------------------------
    @classmethod
    def given(cls, who: str, sample_rate=None, speed=None, loudness=None, pauses=None, limiter=None, one_rate: bool = False,
              compress=None, eq=None) -> "Plan":
        """the options of a Chat call: every value through its validator, a list stays a list and one for all stays one (that is how
        they cross the seam to the engine, which checks the lengths and the rates under its own name).  Off: a speed of 1.0
        everywhere, no target, no spec (of the pauses, the compressor or the equaliser), no flag.  `one_rate`: the call takes one rate for all rows (the zero-padded batch)."""
        if sample_rate is not None and (one_rate or np.ndim(sample_rate) != 0):
            sample_rate = int(sample_rate) if one_rate else [int(r) for r in sample_rate]
        return cls(who, sample_rate,
                   _given(speed, _speed, np.ndim(speed) != 0, on=lambda vals: any(TS.quantize(v)[0] != TS.DEN for v in vals)),
                   _given(loudness, LN.check_target, np.ndim(loudness) != 0),
                   _given(pauses, PA.check, isinstance(pauses, (list, tuple))),
                   _given(limiter, LM.check_flag, np.ndim(limiter) != 0, on=any),
                   SAMPLE_RATE if sample_rate is None else sample_rate,
                   _given(compress, lambda v: CP.check(v, who), isinstance(compress, list)),
                   _given(eq, lambda v: EQ.check(v, who), isinstance(eq, list)))

    def per_sentence(self, groups) -> "Plan":
        """a plan (`given`) whose options are one for all or one per REQUEST -> the plan of the requests' sentences, `groups[g]`
        holding request g's: rate, speed, pauses, eq and compress are expanded to one per sentence (every sentence goes through those
        stages alone); loudness and limiter stay one per request, because a request gets ONE gain over its sentences."""
        new = {}
        for name, what in (("sample_rate", "sample rate"), ("speed", "speed"), ("loudness", "loudness target"), ("limiter", "limiter flag"),
                           ("pauses", "pause spec"), ("compress", "compressor spec"), ("eq", "equaliser spec")):
            value = getattr(self, name)
            if isinstance(value, list):
                if len(value) != len(groups):
                    raise ValueError(f"{self.who}: one {what} per request, or one for all")
                if name in ("sample_rate", "speed", "pauses", "compress", "eq"):
                    new[name] = [v for v, g in zip(value, groups) for _ in g]
        return replace(self, **new, rates=new.get("sample_rate", self.rates))


def run(codec, wav, plan: Plan, offsets=None, in_place: bool = False):
    """A decoded float32 waveform -- [B, n], or packed with host `offsets` -- through the stages of `plan` that are on, in the order
    of DESIGN.md's "The output chain": time_scale, resample, trim_pauses, equalize, compress, loudness_normalize (with `limiter=` only when a
    flag is on).  Only the codec's public stage methods are called, and an option that is off is not passed to them.  Returns the waveform,
    or (packed, offsets) when it came packed or the pause stage has made the rows' lengths differ.  The last stage works in place
    on a pack; on a [B, n] batch with `in_place`."""
    packed = offsets is not None
    if plan.speed is not None:
        wav, offsets = codec.time_scale_segments(wav, offsets, plan.speed) if packed else (codec.time_scale(wav, plan.speed), None)
    if plan.sample_rate is not None:
        wav, offsets = codec.resample_segments(wav, offsets, plan.sample_rate) if packed else (codec.resample(wav, SAMPLE_RATE, plan.sample_rate), None)
    if plan.pauses is not None:
        wav, offsets = codec.trim_pauses(wav, plan.pauses, offsets=offsets, rates=plan.rates)
    if plan.eq is not None:
        if offsets is not None:
            wav = codec.equalize(wav, plan.eq, offsets=offsets, rates=plan.rates, out=wav)
        else:
            wav = wav.contiguous()
            wav = codec.equalize(wav, plan.eq, rates=plan.rates, **({"out": wav} if in_place else {}))
    if plan.compress is not None:
        if offsets is not None:
            wav = codec.compress(wav, plan.compress, offsets=offsets, rates=plan.rates, out=wav)
        else:
            wav = wav.contiguous()
            wav = codec.compress(wav, plan.compress, rates=plan.rates, **({"out": wav} if in_place else {}))
    if plan.levels:
        if offsets is not None:
            wav = codec.loudness_normalize(wav, plan.loudness, offsets=offsets, rates=plan.rates, out=wav, **plan.kwargs("limiter"))
        else:
            wav = wav.contiguous()
            wav = codec.loudness_normalize(wav, plan.loudness, rates=plan.rates, **({"out": wav} if in_place else {}), **plan.kwargs("limiter"))
    return wav if offsets is None else (wav, offsets)

"""Pause control, the parts that need no GPU: the NumPy twin (chattts_amd/pauses.py) against the independent serial oracle
(tests/pauses_oracle.py) bit for bit, hand-computed cases, every refusal of the host side and of ctts_trim_pauses_ragged, and the
plumbing of `pauses` through the engine's decode calls, Chat, the batcher and the endpoint on fakes."""
import ctypes as C
import logging
import threading
import types

import numpy as np
import pytest
import torch

from chattts_amd import _lib, build, pauses as PA
from chattts_amd.serving import SpeechBatcher
from tests import pauses_cases as PC
from tests import pauses_oracle as PO
from tests.test_split_pool_host import _Catch, _EndpointChat, _FakeBatcher, _FakeChat, _Params, _Pool, _spell, _wait_idle

LOUD, QUIET = np.float32(0.5), np.float32(1e-4)        # against the default threshold of -50 dB (3.16e-3)


def _steps(F, *runs, cut=0):
    """runs of (frames, level) -> float32 samples, the last `cut` samples dropped (a partial last frame)"""
    x = np.concatenate([np.full(n * F, lv, np.float32) for n, lv in runs])
    return x[: len(x) - cut] if cut else x


def _same(x, fs, spec):
    y, r = PA.apply(x, fs, spec)
    yo, ro = PO.trim(x, fs, None if spec is True else spec)
    assert y.dtype == np.float32 and r.dtype == np.int32 and r.shape == (8,)
    assert r.tolist() == list(ro), (fs, len(x), spec, r.tolist(), ro)
    assert y.tobytes() == yo.tobytes(), (fs, len(x), spec)
    return y, r.tolist()


# ---- 1. the twin against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", PC.RATES)
def test_twin_equals_oracle_on_the_edge_lengths_and_runs(fs):
    F = fs // 100
    rng = np.random.default_rng(fs)
    noise = lambda n, lv: (np.clip(rng.standard_normal(n), -3, 3) * lv).astype(np.float32)
    for n in (1, F - 1, F, F + 1, 2 * F):                                             # shorter than, equal to and just over a frame
        for lv in (0.25, 1e-4):
            for spec in (True, dict(lead_ms=0, tail_ms=0, pad_ms=0), dict(max_pause_ms=10)):
                _same(noise(n, lv), fs, spec)
    P, lead, tail, pad = PA.PauseSpec().frames()
    assert (P, lead, tail, pad) == (40, 5, 10, 3)
    for R in (P - 1, P, P + 1, 2 * pad + P, 2 * pad + P + 1, 2 * pad + P + 2, 200):   # quiet frames between two active ones
        for cut in (0, 1, F // 2):
            y, r = _same(_steps(F, (2, LOUD), (R, QUIET), (3, LOUD), cut=cut), fs, True)
            inner = R - 2 * pad                                                       # what the dilation leaves of the run
            assert r[5] == (1 if inner > P else 0) and r[6] == max(0, inner - P), (R, r)
    _same(_steps(F, (50, QUIET), cut=7), fs, True)                                    # all quiet
    _same(_steps(F, (50, LOUD), cut=7), fs, True)                                     # all active
    _same(_steps(F, (1, LOUD), (120, QUIET), (1, LOUD)), fs, True)                    # active first and last frames
    for spec in (dict(lead_ms=0), dict(tail_ms=0), dict(pad_ms=0), dict(lead_ms=0, tail_ms=0, pad_ms=0), dict(max_pause_ms=10),
                 dict(max_pause_ms=10, pad_ms=0), dict(max_pause_ms=15, lead_ms=1, tail_ms=11, pad_ms=9), dict(threshold_db=-80.0)):
        _same(_steps(F, (30, QUIET), (4, LOUD), (90, QUIET), (1, LOUD), (7, QUIET), (2, LOUD), (60, QUIET), cut=F // 3), fs, spec)
    for seed in range(12):                                                            # seeded stepped noise, every spec of the GPU fixture
        nf = int(rng.integers(1, 400))
        x = PC.stepped(nf, F, nf * F - int(rng.integers(0, F)), seed, first_loud=bool(seed & 1))
        _same(x, fs, PC.spec_of(seed % len(PC.SPECS)))


def test_a_nan_makes_its_frame_active_and_an_inf_too():
    x = _steps(80, (200, QUIET))
    x[8000] = np.nan
    x[12000] = -np.inf
    y, r = _same(x, 8000, True)
    assert r[:3] == [200, 2, 14] and np.isnan(y).sum() == 1


# ---- 2. hand-computed cases -----------------------------------------------------------------------------------------------------------
def test_hand_computed_records():
    # 8000 Hz, F = 80; the defaults are P 40, lead 5, tail 10, pad 3 frames.  100 quiet + 10 active + 100 quiet + 10 active + 100 quiet:
    # speech = 2 x (10 + 2 x 3) = 32; the leading run has 97 frames and keeps 5 (92 go); the trailing run has 97 and keeps 10 (87 go); the
    # inner run has 100 - 6 = 94 > 40 frames and keeps 20 + 20 (54 go); 320 - 92 - 87 - 54 = 87 frames of 80 samples
    x = _steps(80, (100, QUIET), (10, LOUD), (100, QUIET), (10, LOUD), (100, QUIET))
    y, r = _same(x, 8000, True)
    assert r == [320, 20, 32, 92, 87, 1, 54, 6960] and len(y) == 6960
    # the kept frames, in order: 92 .. 132 | 133 .. 186 dropped | 187 .. 232; frame 132 (k = h - 1 = 19) fades into frame 186
    w = (0.5 - 0.5 * np.cos(np.pi * (np.arange(80) + 0.5) / 80)).astype(np.float32)
    assert np.array_equal(y[: 40 * 80], x[92 * 80: 132 * 80]) and np.array_equal(y[41 * 80:], x[187 * 80: 233 * 80])
    assert np.array_equal(y[40 * 80: 41 * 80], w[::-1] * x[132 * 80: 133 * 80] + w * x[186 * 80: 187 * 80])
    # the same with a partial last frame (79 samples short of whole): the trailing run keeps frames 223 .. 232, none of them the last
    _, r2 = _same(x[:-79], 8000, True)
    assert r2 == r
    # nothing active: max(1, lead + tail) = 15 frames stay, the rest counts as tail; with lead = tail = 0 one frame stays
    assert _same(_steps(240, (50, QUIET), cut=100), 24000, True)[1] == [50, 0, 0, 0, 35, 0, 0, 15 * 240]
    assert _same(_steps(240, (50, QUIET), cut=100), 24000, dict(lead_ms=0, tail_ms=0))[1] == [50, 0, 0, 0, 49, 0, 0, 240]
    assert _same(np.full(1, QUIET), 44100, dict(lead_ms=0, tail_ms=0))[1] == [1, 0, 0, 0, 0, 0, 0, 1]
    # P = 1 (10 ms): h = 1, t = 0 -- one frame stays of the run, faded into the run's last frame; 11025 Hz has F = 110
    x = _steps(110, (1, LOUD), (9, QUIET), (1, LOUD))
    y, r = _same(x, 11025, dict(max_pause_ms=10, pad_ms=0))
    assert r == [11, 2, 2, 0, 0, 1, 8, 330]
    w = PA.fade_table(110)
    assert np.array_equal(y[110:220], w[::-1] * x[110:220] + w * x[9 * 110: 10 * 110])
    # durations round up to whole frames: 41 ms is 5 frames, 400.5 ms 41
    assert PA.PauseSpec(max_pause_ms=400.5, lead_ms=41, tail_ms=0, pad_ms=1).frames() == (41, 5, 0, 1)
    assert PA.PauseSpec().thr() == np.float32(10.0 ** -2.5)
    # a segment that is copied through
    y, r = PA.apply(x, 11025, None)
    assert y.tobytes() == x.tobytes() and r.tolist() == [11, 0, 0, 0, 0, 0, 0, 1210]


def test_a_pack_is_its_segments_alone_and_a_none_row_is_copied():
    xs = [PC.stepped(60, 80, 60 * 80 - 3, 1), PC.stepped(30, 240, 30 * 240, 2, first_loud=True), PC.stepped(45, 441, 45 * 441 - 200, 3)]
    rates, specs = [8000, 24000, 44100], [PC.spec_of(1), None, True]
    y, off, rec = PA.trim(np.concatenate(xs), specs, offsets=PC.offsets([len(x) for x in xs]), rates=rates)
    for i, (x, fs, sp) in enumerate(zip(xs, rates, specs)):
        yi, ri = PA.apply(x, fs, sp)
        assert y[off[i]: off[i + 1]].tobytes() == yi.tobytes() and rec[i].tolist() == ri.tolist()
    assert y[off[1]: off[2]].tobytes() == xs[1].tobytes() and off.dtype == np.int64 and rec.dtype == np.int32


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_specs_rates_and_tables_are_refused_on_the_host():
    assert PA.check(None) is None and PA.check(True) == PA.PauseSpec() and PA.check({}) == PA.PauseSpec()
    assert PA.check(dict(max_pause_ms=10, threshold_db=0)) == PA.PauseSpec(max_pause_ms=10, threshold_db=0)
    assert PA.check(PA.PauseSpec(pad_ms=0)).pad_ms == 0
    for bad, why in ((dict(gap_ms=3), "unknown field"), (dict(max_pause_ms="1"), "number"), (dict(max_pause_ms=True), "number"),
                     (dict(max_pause_ms=9), "10 .. 10000"), (dict(max_pause_ms=10001), "10 .. 10000"), (dict(lead_ms=-1), "0 .. 10000"),
                     (dict(tail_ms=10000.5), "0 .. 10000"), (dict(threshold_db=0.1), "-100 .. 0"), (dict(threshold_db=-101), "-100 .. 0"),
                     (dict(pad_ms=1001), "0 .. 1000"), (dict(pad_ms=float("nan")), "0 .. 1000"), (PA.PauseSpec(lead_ms=-5), "0 .. 10000"),
                     (False, "None, True"), (3, "None, True"), ("on", "None, True"), ([True], "None, True")):
        with pytest.raises(ValueError, match=why):
            PA.check(bad)
    for fs in (7999, 48001, 24000.0, "24000", None, True):
        with pytest.raises(ValueError, match="rate"):
            PA.check_rate(fs)
    assert [PA.check_rate(fs) for fs in (8000, 11025, 22050, 48000, np.int64(16000))] == [8000, 11025, 22050, 48000, 16000]
    assert PA.per_row(None, 3) is None and PA.per_row([None, None], 2) is None and PA.per_row(True, 2) == [PA.PauseSpec()] * 2
    with pytest.raises(ValueError, match="one pause spec per row"):
        PA.per_row([True], 2)
    for kw, why in ((dict(off=[1, 10]), "ascend from 0"), (dict(off=[0, 5, 5, 10]), "empty"), (dict(off=[0, 7, 5, 10]), "ascend"), (dict(off=[0]), "ascend"),
                    (dict(off=[0, 5, 10], rates=[24000]), "one rate per segment"), (dict(off=[0, 5, 10], rates=[24000, 100]), "rate"),
                    (dict(off=[0, 5, 10], specs=[True]), "one spec per segment"), (dict(off=[0, 5, 10], specs=dict(x=1)), "unknown field"),
                    (dict(off=[0, (1 << 31) - 4096]), "2\\^31"), (dict(off=np.arange(65537)), "65535")):
        with pytest.raises(ValueError, match=why):
            PA.tables(**kw)
    tb = PA.tables([0, 81, 400, 1000], rates=[8000, 24000, 8000], specs=[True, None, dict(max_pause_ms=20)])
    assert tb["fbase"].tolist() == [0, 2, 4, 12] and tb["rows"].dtype == np.int32 and tb["rows"].shape == (3, PA.ROW)
    assert tb["rows"][0].tolist()[:5] == [80, 3, 5, 10, 40] and tb["rows"][1].tolist() == [240, 0, 0, 0, 0, 0, 80, 0] and tb["rows"][2, 4] == 2
    assert tb["rows"][0, 5:6].view(np.float32)[0] == PA.PauseSpec().thr() and tb["rows"][2, 6] == 0
    assert tb["fade"].tobytes() == np.concatenate([PA.fade_table(80), PA.fade_table(240)]).tobytes()
    assert tb["scratch"] == PA.scratch_bytes(12, 3) == 2 * 48 + 16 + 16


def test_library_symbols_and_refusals_before_any_launch():
    """the C entry point checks every host table first: these calls fail without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    with open(_lib.HERE + "/../include/chattts_amd.h") as f:
        header = f.read()
    for name in ("ctts_trim_pauses_ragged", "ctts_trim_pauses_ragged_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "pauses.hip" in build.SOURCES
    assert lib.ctts_trim_pauses_ragged_scratch_bytes(12, 3) == PA.scratch_bytes(12, 3)
    assert lib.ctts_trim_pauses_ragged_scratch_bytes(1000003, 77) == PA.scratch_bytes(1000003, 77)
    assert lib.ctts_trim_pauses_ragged_scratch_bytes(0, 3) == 0 and lib.ctts_trim_pauses_ragged_scratch_bytes(5, 65536) == 0
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = 1 << 20                    # never dereferenced: every call below is refused on its host arguments
    good = PA.tables([0, 2400, 12000], rates=[24000, 8000], specs=[True, None])

    def call(off=None, fbase=None, rows=None, n_fade=None, x=fake, y=fake + (1 << 16), scratch=fake + (1 << 18), sb=1 << 20, null=None, n_seg=None):
        o = good["off"] if off is None else np.asarray(off, np.int64)
        fb = good["fbase"] if fbase is None else np.asarray(fbase, np.int64)
        rw = good["rows"] if rows is None else np.ascontiguousarray(rows, np.int32)
        p = {k: (None if k == null else fake + (1 << 19) + 4096 * i) for i, k in enumerate(("off", "fbase", "rows", "fade", "off_out", "records"))}
        rc = lib.ctts_trim_pauses_ragged(None if null == "in" else x, None if null == "out" else y, p["off"], None if null == "off_host" else vp(o),
                                         p["fbase"], None if null == "fbase_host" else vp(fb), p["rows"], None if null == "rows_host" else vp(rw),
                                         len(o) - 1 if n_seg is None else n_seg, p["fade"], int(good["fade"].size) if n_fade is None else n_fade,
                                         p["off_out"], p["records"], None if null == "scratch" else scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    def rows_with(seg, col, val):
        r = good["rows"].copy()
        r[seg, col] = val
        return r
    thr_nan = rows_with(0, 5, np.array([np.nan], np.float32).view(np.int32)[0])
    for kw, why in ([(dict(null=k), "null") for k in ("in", "out", "off", "off_host", "fbase", "fbase_host", "rows", "rows_host", "fade", "off_out",
                                                       "records", "scratch")] +
                    [(dict(off=(1, 2400, 12000)), "must be 0"), (dict(off=(0, 2400, 2400)), "empty"), (dict(off=(0, 2400, 100)), "ascend"),
                     (dict(n_seg=0), "1 <= n_seg <= 65535"), (dict(n_seg=65536), "1 <= n_seg <= 65535"),
                     (dict(off=(0, 2400, (1 << 31) - 4096)), "2^31 - 4096"),
                     (dict(rows=rows_with(0, 0, 79)), "frame of 79"), (dict(rows=rows_with(1, 0, 481)), "frame of 481"),
                     (dict(rows=rows_with(0, 4, 1001)), "P 0 (copy) .. 1000"), (dict(rows=rows_with(0, 4, -1)), "P 0 (copy) .. 1000"),
                     (dict(rows=rows_with(0, 1, 101)), "pad 0 .. 100"), (dict(rows=rows_with(0, 2, 1001)), "lead and tail"),
                     (dict(rows=rows_with(0, 3, -2)), "lead and tail"), (dict(rows=thr_nan), "threshold"),
                     (dict(rows=rows_with(0, 5, 0)), "threshold"), (dict(rows=rows_with(0, 6, 81)), "fade table"), (dict(rows=rows_with(0, 6, -1)), "fade table"),
                     (dict(n_fade=100), "fade table"), (dict(n_fade=-1), "negative"),
                     (dict(fbase=(0, 10, 25)), "the frame bases say"), (dict(fbase=(0, 10, 26)), "the frame bases say 16"), (dict(fbase=(1, 11, 26)), "first frame base"),
                     (dict(sb=100), "scratch too small"), (dict(sb=PA.scratch_bytes(25, 2) - 1), "scratch too small"),
                     (dict(x=fake + 4), "16-byte aligned"), (dict(y=fake + 8), "16-byte aligned"), (dict(scratch=fake + (1 << 18) + 4), "16-byte aligned"),
                     (dict(y=fake), "overlap"), (dict(y=fake + 16), "overlap"), (dict(y=fake + 4 * 11999 - 12), "overlap"), (dict(y=fake - 4 * 12000 + 16), "overlap")]):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_trim_pauses_ragged" in msg and why in msg, (kw, msg)


# ---- 4. the engine's decode calls: where the stage sits -----------------------------------------------------------------------------------
def _engine():
    """a CodecEngine without a device: the plain decodes and every stage behind them are recorded, the stages' ORDER is the real code's"""
    from chattts_amd.engine import CodecEngine

    class Rec(CodecEngine):
        def __init__(self):
            self.calls = []

        def decode_ragged(self, rows, return_mel=False, sample_rate=None, speed=None, loudness=None, pauses=None):
            if sample_rate is None and speed is None and loudness is None and pauses is None:
                self.calls.append("decode")
                lens = [512 * int(r.shape[0]) for r in rows]
                return torch.zeros(sum(lens)), PC.offsets(lens)
            return super().decode_ragged(rows, return_mel, sample_rate, speed, loudness, pauses)

        def decode_to_wavs(self, rows, pad_to=None, sample_rate=None, speed=None, loudness=None, pauses=None):
            if sample_rate is None and speed is None and loudness is None and pauses is None:
                self.calls.append("decode")
                return torch.zeros(len(rows), 2048)
            return super().decode_to_wavs(rows, pad_to, sample_rate, speed, loudness, pauses)

        def time_scale_segments(self, wav, off, speeds):
            self.calls.append(("time_scale", list(speeds)))
            return wav, off

        def time_scale(self, wav, speed, off=None):
            self.calls.append(("time_scale", speed))
            return wav

        def resample_segments(self, wav, off, rates):
            self.calls.append(("resample", list(rates)))
            return wav, off

        def resample(self, wav, orig, new):
            self.calls.append(("resample", new))
            return wav

        def trim_pauses(self, wav, spec, offsets=None, rates=None, return_stats=False):
            self.calls.append(("trim_pauses", spec, rates, None if offsets is None else list(offsets)))
            flat = wav.reshape(-1)
            off = np.arange(wav.shape[0] + 1, dtype=np.int64) * wav.shape[1] if wav.dim() == 2 else np.asarray(offsets, np.int64)
            return flat[: flat.numel() - 7], np.concatenate([off[:-1], off[-1:] - 7])

        def loudness_normalize(self, wav, target, offsets=None, groups=None, rates=None, return_stats=False, out=None):
            self.calls.append(("loudness", target, rates, list(offsets), None if groups is None else list(groups), out is wav))
            return wav

        def float_to_int16_ragged(self, wav, off, **kw):
            self.calls.append(("convert", list(off)))
            return None, None, None

        def float_to_int16_groups(self, wav, off, grp, **kw):
            self.calls.append(("convert_groups", list(off), list(grp)))
            return wav, [0]

        def unpack_groups(self, blob, starts, encs=None):
            return [np.zeros(3, np.int16)]

        def to_host(self, t):
            return t.numpy()
    return Rec()


def test_the_stage_sits_behind_the_resampler_and_in_front_of_loudness_and_the_conversion():
    from chattts_amd.core import Chat
    eng = _engine()
    rows = [torch.zeros(3, 768), torch.zeros(2, 768)]
    D = PA.PauseSpec()
    wav, off = eng.decode_ragged(rows, sample_rate=[8000, 16000], speed=[1.25, 1.0], loudness=[-16, None], pauses=[True, None])
    assert eng.calls == ["decode", ("time_scale", [1.25, 1.0]), ("resample", [8000, 16000]), ("trim_pauses", [D, None], [8000, 16000], [0, 1536, 2560]),
                         ("loudness", [-16.0, None], [8000, 16000], [0, 1536, 2553], None, True)]
    assert off.tolist() == [0, 1536, 2553] and wav.numel() == 2553
    eng.calls.clear()
    wav, off = eng.decode_to_wavs(rows, sample_rate=8000, speed=1.25, loudness=-16, pauses=dict(tail_ms=0))
    assert eng.calls == ["decode", ("time_scale", 1.25), ("resample", 8000), ("trim_pauses", [PA.PauseSpec(tail_ms=0)] * 2, 8000, None),
                         ("loudness", [-16.0, -16.0], 8000, [0, 2048, 4089], None, True)]
    assert off.tolist() == [0, 2048, 4089]                                            # (packed, offsets) instead of [B, n]
    eng.calls.clear()
    eng.decode_ragged(rows, pauses=None)                                              # off: not a launch, a copy or an allocation more
    eng.decode_ragged(rows, pauses=[None, None], loudness=[-16, None])
    eng.decode_to_wavs(rows, pauses=None)
    assert eng.calls == ["decode", "decode", ("loudness", [-16.0, None], [24000, 24000], [0, 1536, 2560], None, True), "decode"]
    for kw, why in ((dict(pauses=dict(x=1)), "unknown field"), (dict(pauses=[True]), "one pause spec per row"), (dict(pauses=True, sample_rate=7000), "rate"),
                    (dict(pauses=True, sample_rate=11025, loudness=-16), "multiple of 10")):
        eng.calls.clear()
        with pytest.raises(ValueError, match=why):
            eng.decode_ragged(rows, **kw)
        assert eng.calls == []                                                        # every refusal, before the decode
    # Chat: the conversion comes last, on the trimmed offsets -- on the ragged path and on the zero-padded batch's
    chat = Chat.__new__(Chat)
    chat.codec, chat.has_loaded = eng, lambda *a, **k: True
    for ragged in (True, False):
        eng.calls.clear()
        out = chat.decode_to_pcm16(rows, strip=False, ragged=ragged, sample_rate=8000, speed=1.25, loudness=-16, pauses=True)
        kinds = [c if isinstance(c, str) else c[0] for c in eng.calls]
        assert kinds == ["decode", "time_scale", "resample", "trim_pauses", "loudness", "convert"], (ragged, kinds)
        assert eng.calls[-1][1] == eng.calls[-2][3] and [len(p) for p in out] == ([1536, 1017] if ragged else [2048, 2041])
    eng.calls.clear()
    assert [len(w) for w in chat.decode_to_wavs(rows, pauses=True)] == [2048, 2041]   # a list, also without ragged
    assert [c if isinstance(c, str) else c[0] for c in eng.calls] == ["decode", "trim_pauses"]
    # a split request: every SENTENCE trimmed alone, then ONE gain over the request's trimmed sentences
    eng.calls.clear()
    chat.decode_split_to_pcm16([rows, [torch.zeros(1, 768)]], pauses=[True, None], loudness=-19.0, sample_rate=8000)
    assert eng.calls == ["decode", ("resample", [8000] * 3), ("trim_pauses", [D, D, None], [8000] * 3, [0, 1536, 2560, 3072]),
                         ("loudness", -19.0, [8000] * 3, [0, 1536, 2560, 3065], [0, 2, 3], True), ("convert_groups", [0, 1536, 2560, 3065], [0, 2, 3])]
    with pytest.raises(ValueError, match="one pause spec per request"):
        chat.decode_split_to_pcm16([rows], pauses=[True, True])


# ---- 5. Chat.infer ----------------------------------------------------------------------------------------------------------------------
def _chat():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.codec, chat.has_loaded = _engine(), lambda *a, **k: True
    chat.device = torch.device("cpu")
    chat.context, chat.logger = types.SimpleNamespace(set=lambda v: None), logging.getLogger("test_pauses_host")
    return chat


def test_chat_infer_passes_the_spec_on_and_nothing_when_it_is_none():
    chat = _chat()
    seen = []

    def fake_infer(text, *a, **kw):
        seen.append(kw)
        yield [np.full(5, 0.5, np.float32) for _ in text]
    chat._infer = fake_infer
    kw = dict(skip_refine_text=True, split_text=False)
    chat.infer(["a", "b"], pauses=True, **kw)
    chat.infer(["a", "b"], **kw)
    chat.infer(["a", "b"], pauses=None, pcm16=True, **kw)
    chat.infer(["a", "b"], pauses=[dict(tail_ms=0), None], pcm16=True, encoding="ulaw", sample_rate=8000, speed=1.25, loudness=-16, **kw)
    assert seen[0]["pauses"] == PA.PauseSpec() and "pauses" not in seen[1] and "pauses" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "pauses"} == seen[1]
    assert seen[3]["pauses"] == [PA.PauseSpec(tail_ms=0), None] and seen[3]["loudness"] == -16.0 and seen[3]["encoding"] == "ulaw"
    # a split request that is concatenated on the host: the sentences are trimmed in the decode, the ONE gain comes afterwards
    seen.clear()
    out = chat.infer("a. b. c.", pauses=True, loudness=-16.0, skip_refine_text=True)
    assert seen[0]["pauses"] == PA.PauseSpec() and "loudness" not in seen[0] and len(out) == 1
    assert chat.codec.calls[-1][0] == "loudness" and chat.codec.calls[-1][4] == [0, 3]


def test_streams_and_bad_specs_are_refused():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["hello"], stream=True, pauses=True)
    with pytest.raises(ValueError, match="10 .. 10000"):
        chat.infer(["hello"], pauses=dict(max_pause_ms=1))
    with pytest.raises(ValueError, match="one pause spec"):
        chat.infer(["a", "b"], split_text=True, pauses=[True, True])
    with pytest.raises(ValueError, match="rate"):
        chat.infer(["hello"], sample_rate=7000, pauses=True)
    lock = threading.Lock()
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _Pool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream("a#8", _Params(), pauses=True)
        with pytest.raises(ValueError, match="unknown field"):
            b.submit_stream("a#8", _Params(), pauses=dict(x=1))
        for bad in (dict(pad_ms=-1), "x", False, 3):
            with pytest.raises(ValueError):
                b.submit("a#8", _Params(), pauses=bad)
        with pytest.raises(ValueError, match="rate"):
            b.submit("a#8", _Params(), pauses=True, sample_rate=50000)
    finally:
        b.close()


# ---- 6. the batcher ---------------------------------------------------------------------------------------------------------------------
class _TrimChat(_FakeChat):
    def __init__(self):
        super().__init__()
        self.pcm_kw, self.split_kw, self.wav_kw = [], [], []

    def decode_to_pcm16(self, hids, ragged=False, **kw):
        self.pcm_kw.append(kw)
        return super().decode_to_pcm16(hids, ragged)

    def decode_split_to_pcm16(self, groups, **kw):
        self.split_kw.append(kw)
        return super().decode_split_to_pcm16(groups)

    def decode_to_wavs(self, hids, **kw):
        self.wav_kw.append(kw)
        return super().decode_to_wavs(hids)


def test_requests_with_mixed_specs_share_one_decode_and_one_trim_call():
    lock, pools = threading.Lock(), {}
    chat = _TrimChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    A, B = PA.PauseSpec(), PA.PauseSpec(max_pause_ms=100, tail_ms=0)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), pauses=p) for c, p in (("a", True), ("b", dict(max_pause_ms=100, tail_ms=0)), ("c", None), ("d", A))]
        res = [f.result(timeout=10) for f in futs]
        b.submit("e#8", _Params()).result(timeout=10)
        _wait_idle(pools)
        occ = b.occupancy()
    finally:
        b.close()
    # ONE decode call for the poll carries every spec: Chat.decode_to_pcm16(ragged=True) hands the list to ONE decode_ragged, which
    # makes ONE trim_pauses call (test_the_stage_sits_... above); the request without a spec is a None entry of it
    assert chat.pcm_kw == [{"pauses": [A, B, None, A]}, {}] and b.decode_calls == 2 and occ["trimmed"] == 3
    assert [int(r[0]) for r in res] == [ord(c) for c in "abcd"]


def test_batcher_passes_the_spec_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _TrimChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    D = PA.PauseSpec()
    try:
        b.submit("a#8", _Params(), pauses=True).result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("d#8", _Params(), pauses=dict(lead_ms=0), loudness=-20.0, sample_rate=8000, speed=1.25).result(timeout=10)
        pcm = b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, pauses=True, loudness=-23.0).result(timeout=30)
        b.submit("m#8\nn#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)
        _wait_idle(pools)
        assert b.occupancy()["trimmed"] == 3
    finally:
        b.close()
    assert chat.wav_kw == [{"pauses": D}, {}, {"sample_rate": 8000, "speed": 1.25, "loudness": -20.0, "pauses": PA.PauseSpec(lead_ms=0)}]
    assert chat.split_kw == [{"loudness": [-23.0], "pauses": [D]}, {}] and _spell(pcm) == [("k", 8), ("l", 8)]


# ---- 7. the endpoint ------------------------------------------------------------------------------------------------------------------
def _app(batcher=None, **kw):
    from chattts_amd import server
    log, catch = logging.getLogger(f"test_pauses_host.{id(kw)}"), _Catch()
    log.addHandler(catch)
    chat = _EndpointChat()
    return server.create_app(chat, {"default": "SPK-D"}, batcher=batcher, logger=log, **kw), chat, catch


def test_endpoint_pauses():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: an unknown key -- the warning, and today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "pauses": True})
        assert r.status_code == 200 and r.content == r0.content and r.headers["content-type"] == r0.headers["content-type"]
        plain = lambda call: (call[0], call[1], {k: (v if k != "params_infer_code" else vars(v)) for k, v in call[2].items()})
        assert plain(chat.calls[-1]) == plain(chat.calls[-2]) and "pauses" not in chat.calls[-1][2]
        assert catch.msgs == ["ignoring unsupported parameters: ['pauses']"]
        assert c.post("/v1/audio/speech", json={**body, "pauses": "long"}).status_code == 200        # ignored, whatever it holds
        assert c.post("/v1/audio/speech", json={**body, "pauses": True, "stream": True}).status_code == 200
        assert "pauses" not in c.get("/health").json()

    app, chat, catch = _app(pauses=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "pauses": True})
        assert r.status_code == 200 and chat.calls[-1][2]["pauses"] == PA.PauseSpec() and chat.calls[-1][1] is False
        r = c.post("/v1/audio/speech", json={**body, "pauses": {"max_pause_ms": 250, "threshold_db": -45.5}})
        assert r.status_code == 200 and chat.calls[-1][2]["pauses"] == PA.PauseSpec(max_pause_ms=250, threshold_db=-45.5)
        for off in (None, False):
            assert c.post("/v1/audio/speech", json={**body, "pauses": off}).status_code == 200 and "pauses" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "pauses" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        n = len(chat.calls)
        for bad, why in ((3, "true or an object"), ("on", "true or an object"), ([True], "true or an object"), ({"gap": 1}, "unknown field"),
                         ({"max_pause_ms": 5}, "10 .. 10000"), ({"pad_ms": 2000}, "0 .. 1000"), ({"threshold_db": "low"}, "number"),
                         ({"lead_ms": True}, "number")):
            r = c.post("/v1/audio/speech", json={**body, "pauses": bad})
            assert r.status_code == 400 and why in r.text, (bad, r.text)
        r = c.post("/v1/audio/speech", json={**body, "pauses": True, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and len(chat.calls) == n
        assert not catch.msgs and c.get("/health").json()["pauses"] is True

    app, chat, catch = _app(pauses=True, loudness=True, sample_rates=(8000, 11025, 24000), g711=True, speed=True, flac=True)      # composes
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "pauses": {"tail_ms": 0}, "loudness": -20.5, "speed": 0.8, "sample_rate": 8000, "encoding": "ulaw"})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["pauses"], kw["loudness"], kw["speed"], kw["sample_rate"], kw["encoding"]) == \
            (PA.PauseSpec(tail_ms=0), -20.5, 0.8, 8000, "ulaw")
        r = c.post("/v1/audio/speech", json={**body, "response_format": "flac", "pauses": True})
        assert r.status_code == 200 and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["pauses"] == PA.PauseSpec()
        r = c.post("/v1/audio/speech", json={**body, "pauses": True, "sample_rate": 11025})          # any rate in 8000 .. 48000
        assert r.status_code == 200 and chat.calls[-1][2]["sample_rate"] == 11025

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, pauses=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "pauses": True}).status_code == 200 and bat.calls[-1][2] == {"pauses": PA.PauseSpec()}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

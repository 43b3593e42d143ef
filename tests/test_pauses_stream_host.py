"""Host side of the pause streams: the NumPy twin (`pauses.StreamPauses`) against the independent serial oracle (tests/pauses_oracle.py) and
`pauses.apply` of the whole signal, bit for bit in samples and record, under every cut of tests/pauses_stream_cases.py; the schedule (what a
push emits, and when); the bounded state; every refusal of the host side and of ctts_trim_pauses_stream_step's host mirror (no device is
touched: every call is refused on its host arguments); the symbol, the header and `_lib`; the engine's planning."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from chattts_amd import _lib, pauses as PA, statepool as SP
from tests import pauses_oracle as ORACLE, pauses_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chattts_amd.h")


def stream(x, fs, spec, sizes, empty_final=False):
    """the twin over pushes of `sizes` -> (chunks, twin); asserts the state bound at every step"""
    tw, out, at = PA.StreamPauses(fs, spec), [], 0
    need = PA.stream_need(spec)
    for k, n in enumerate(sizes):
        out.append(tw.push(x[at: at + n], k == len(sizes) - 1 and not empty_final))
        at += n
        assert tw.held <= need <= PA.STREAM_FRAMES and len(tw.partial) < fs // 100
    if empty_final:
        out.append(tw.push(x[:0], True))
    assert at == len(x) and tw.done and tw.held == 0
    return out, tw


def check(x, fs, spec, sizes, empty_final=False, why=""):
    y, rec = ORACLE.trim(x, fs, spec)
    y2, rec2 = PA.apply(x, fs, spec)
    assert y.tobytes() == y2.tobytes() and list(rec2) == list(rec)
    out, tw = stream(x, fs, spec, sizes, empty_final)
    assert np.concatenate(out).tobytes() == y.tobytes(), (fs, why)
    assert list(tw.record) == list(rec), (fs, why, list(tw.record), rec)
    return out, tw


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", SC.RATES)
def test_the_twin_stream_is_the_oracle_on_random_streams_cut_at_random(fs):
    rng = np.random.default_rng(fs)
    F = fs // 100
    for it in range(60):
        name = list(SC.SPECS)[it % len(SC.SPECS)]
        spec = SC.SPECS[name]
        parts, quiet = [], bool(rng.integers(0, 2))
        for _ in range(int(rng.integers(1, 7))):
            parts.append((int(rng.integers(1, 70 if quiet else 6)), not quiet))
            quiet = not quiet
        act = SC.runs(*parts)
        if it % 10 == 0:
            act[:] = False                                           # no active frame at all
        n = len(act) * F - int(rng.integers(0, F))
        x = SC.signal(fs, act, n, seed=it)
        for kind in ("random", "random+empty", "inside_every_frame"):
            sizes = SC.cuts(n, F, kind, seed=it)
            check(x, fs, spec, sizes[:-1] if kind == "random+empty" else sizes, kind == "random+empty", (name, it, kind))


def test_one_push_per_sample_and_pushes_of_whole_frames():
    fs, F = 8000, 80
    x = SC.signal(fs, SC.runs((4, 0), (2, 1), (15, 0), (1, 1), (6, 0)), 28 * F - 11)
    for name in ("bare", "odd", "h1_t0"):
        check(x, fs, SC.SPECS[name], SC.cuts(len(x), F, "per_sample"), why=name)
        check(x, fs, SC.SPECS[name], SC.cuts(len(x), F, "frames"), why=name)
        check(x, fs, SC.SPECS[name], SC.cuts(len(x), F, "whole"), why=name)


@pytest.mark.parametrize("fs", SC.RATES)
@pytest.mark.parametrize("name", list(SC.SPECS))
def test_the_edge_cases_under_every_kind_of_cut(fs, name):
    F = fs // 100
    for label, x in SC.edge_cases(fs, name):
        for kind in ("whole", "frames", "inside_every_frame", "random", "random+empty"):
            sizes = SC.cuts(len(x), F, kind, seed=len(x))
            check(x, fs, SC.SPECS[name], sizes[:-1] if kind == "random+empty" else sizes, kind == "random+empty", (name, label, kind))


def test_an_empty_stream_emits_nothing_and_reports_zeros():
    tw = PA.StreamPauses(24000, True)
    assert len(tw.push(np.zeros(0, np.float32))) == 0 and len(tw.push(np.zeros(0, np.float32), True)) == 0
    assert list(tw.record) == [0] * 8 and tw.done
    with pytest.raises(ValueError, match="last push"):
        tw.push(np.zeros(1, np.float32))


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", (8000, 22050))
def test_through_speech_a_stream_withholds_less_than_a_frame(fs):
    F = fs // 100
    x = SC.signal(fs, np.ones(30, bool), 30 * F - 9, seed=2)
    tw, at, out = PA.StreamPauses(fs, True), 0, 0
    for n in SC.cuts(len(x), F, "random", seed=4)[:-1]:
        out += len(tw.push(x[at: at + n]))
        at += n
        assert at - out == at % F < F and tw.held == 0


@pytest.mark.parametrize("name", list(SC.SPECS))
def test_inside_a_pause_exactly_k0_frames_go_out_and_nothing_before_the_first_active_frame(name):
    fs, F = 11025, 110
    spec = SC.SPECS[name]
    P, lead, tail, pad = SC.frames_of(spec)
    h = -(-P // 2)
    k0 = min(h - 1, tail)
    assert PA.stream_consts(PA.check(spec))["k0"] == k0
    pre, quiet = lead + pad + 9, 3 * (P + pad + tail) + 7
    x = SC.signal(fs, SC.runs((pre, 0), (1, 1), (quiet, 0), (1, 1)))
    tw = PA.StreamPauses(fs, spec)
    for j in range(pre):                                             # a leading run: nothing is decided
        assert len(tw.push(x[j * F: (j + 1) * F])) == 0
    assert len(tw.push(x[pre * F: (pre + 1) * F])) == (min(lead, pre - pad) + pad + 1) * F          # the first active frame decides it
    for k in range(quiet):                                           # behind speech: pad frames, then k0 frames of the run, then nothing
        j = pre + 1 + k
        got = len(tw.push(x[j * F: (j + 1) * F]))
        assert got == (F if k < pad + k0 else 0), (k, got)
        assert tw.held == PA.stream_held(tw.c, *tw.state[:3])[2] - k0 + PA.stream_held(tw.c, *tw.state[:3])[4] - PA.stream_held(tw.c, *tw.state[:3])[3]
        assert tw.held <= PA.stream_need(spec)
    rest = tw.push(x[(pre + 1 + quiet) * F:], True)                  # speech resumes: the rest of the capped pause and the frame itself
    assert len(rest) == (P - k0 + pad + 1) * F


# ---- the state --------------------------------------------------------------------------------------------------------------------------
def test_stream_need_is_the_bound_and_the_capacity_holds_what_the_issue_asks():
    for spec, need in [(True, 34), (SC.SPECS["bare"], 4), (dict(max_pause_ms=1000, lead_ms=250, tail_ms=250, pad_ms=100), 86),
                       (dict(max_pause_ms=1000, lead_ms=0, tail_ms=0, pad_ms=100), 111)]:          # the most inside the promised box
        assert PA.stream_need(spec) == need <= PA.STREAM_FRAMES
    c = PA.stream_consts(PA.PauseSpec())
    assert PA.stream_need(True) == max(c["A1"] + c["A2"], c["P"] + c["pad"] - c["k0"], c["H"] - c["k0"] + c["L"])
    rng = np.random.default_rng(1)
    for _ in range(300):                                             # every spec inside the promised box fits a slot
        spec = dict(max_pause_ms=int(rng.integers(10, 1001)), lead_ms=int(rng.integers(0, 251)), tail_ms=int(rng.integers(0, 251)), pad_ms=int(rng.integers(0, 101)))
        assert PA.stream_need(spec) <= PA.STREAM_FRAMES
    assert PA.STREAM_FRAMES == 112 and (PA.STREAM_FRAMES + 1) * 480 * 4 * 2 + PA.STATE * 4 == 433984     # bytes per slot, as DESIGN.md states


def test_a_pause_ten_times_the_capacity_holds_no_more_than_the_need():
    fs, F = 8000, 80
    x = np.concatenate([SC.signal(fs, [0, 1, 1]), np.zeros(30 * fs, np.float32), SC.signal(fs, [1, 0, 0], seed=1)])
    assert len(x) // F > 10 * PA.STREAM_FRAMES
    sizes = [4000] * (len(x) // 4000) + [len(x) % 4000]
    out, tw = check(x, fs, SC.DEFAULT, sizes)
    assert tw.record[5] == 1 and tw.record[6] == 3000 - 2 * 3 - 40         # one run shortened to P frames
    seen = 0
    tw = PA.StreamPauses(fs, True)
    for k, n in enumerate(sizes[:-1]):
        tw.push(x[k * 4000: k * 4000 + n])
        seen = max(seen, tw.held)
    assert seen == PA.stream_need(True) == 34                        # the front of a long run, its back and the pad: every frame of the bound
    out, _ = stream(np.zeros(30 * fs, np.float32), fs, SC.DEFAULT, [4000] * 60)                         # no active frame ever: the first A1 frames
    assert sum(len(c) for c in out) == 15 * F and all(len(c) == 0 for c in out[:-1])


# ---- refusals of the host side ----------------------------------------------------------------------------------------------------------
def test_the_host_side_refuses_with_its_reasons():
    for args, why in [((7999, True), "rate is an integer"), ((48001, True), "rate is an integer"), ((24000.0, True), "rate is an integer"),
                      ((24000, None), "needs a spec"), ((24000, {"max_pause_ms": 5}), "max_pause_ms is a number in 10 .. 10000"),
                      ((24000, {"pause": 5}), "unknown field"), ((24000, "yes"), "None, True, a PauseSpec or a dict"),
                      ((24000, {"max_pause_ms": 2000}), "hold 194 frames, a slot holds 112"), ((24000, {"tail_ms": 1000}), "a slot holds 112"),
                      ((24000, {"lead_ms": 600}), "a slot holds 112")]:
        with pytest.raises(ValueError, match=why):
            PA.StreamPauses(*args)
    with pytest.raises(ValueError, match="submit_stream: this spec makes a stream hold"):
        PA.check_stream(8000, {"max_pause_ms": 10000}, "submit_stream")
    assert PA.check_stream(8000, {"max_pause_ms": 1000, "lead_ms": 250, "tail_ms": 250, "pad_ms": 100})[0] == 8000
    tw = PA.StreamPauses(8000, True)
    tw.pushed = (1 << 31) - 10
    with pytest.raises(ValueError, match="2\\^31"):
        tw.push(np.zeros(10, np.float32))


# ---- the symbol -------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported_declared_and_bound_and_the_layouts_agree():
    lib = _lib.lib()
    with open(HEADER) as f:
        header = f.read()
    for name, nargs in (("ctts_trim_pauses_stream_step", 16), ("ctts_trim_pauses_stream_scratch_bytes", 2)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs
    assert getattr(lib, "ctts_trim_pauses_stream_step").argtypes == _lib.SIGNATURES["ctts_trim_pauses_stream_step"][1]
    assert _lib.PA_STREAM.itemsize == 96 and "} ctts_pa_stream;" in header
    struct = header[header.index("#define CTTS_PA_STREAM_FRAMES"): header.index("} ctts_pa_stream;")]
    fields = [n for line in struct.splitlines() if line.strip().startswith(("int64_t", "int32_t", "float"))
              for n in re.sub(r"/\*.*", "", line).replace("int64_t", "").replace("int32_t", "").replace("float", "").replace(";", "").replace(" ", "").split(",")]
    assert tuple(fields) == _lib.PA_STREAM.names
    assert [_lib.PA_STREAM.fields[n][1] for n in ("slot", "F", "thr", "n_list")] == [48, 64, 84, 92]
    for name, val in (("FRAMES", PA.STREAM_FRAMES), ("CARRY", (PA.STREAM_FRAMES + 1) * 480), ("STATE", PA.STATE), ("RES", 4)):
        assert re.search(r"#define CTTS_PA_STREAM_%s %d\b" % (name, val), header)
    with open(os.path.join(ROOT, "chattts_amd", "csrc", "kernels.hpp")) as f:
        k = f.read()
    assert re.search(r"#define PA_SCAP %d\b" % PA.STREAM_FRAMES, k) and re.search(r"#define PA_STATE %d\b" % PA.STATE, k)
    assert lib.ctts_trim_pauses_stream_scratch_bytes(33, 10) == 48 + 160 and lib.ctts_trim_pauses_stream_scratch_bytes(0, 1) == 16
    assert lib.ctts_trim_pauses_stream_scratch_bytes(-1, 1) == 0 and lib.ctts_trim_pauses_stream_scratch_bytes(1, 0) == 0


# ---- the library's refusals -------------------------------------------------------------------------------------------------------------
def _desc(fs=24000, spec=True, pos=3000, n_in=5000, final=False, slot=0, phase=0, **over):
    F, pad, lead, tail, P, thr = PA.stream_row(fs, PA.check(spec))
    need, avail = PA.stream_need(spec), pos % F + n_in
    nf = avail // F + (1 if final and avail % F else 0)
    row = dict(in_off=0, n_in=n_in, pos=pos, out_off=0, fr_off=0, list_off=0, slot=slot, phase=phase, need=need, fin=int(final), F=F, pad=pad,
               lead=lead, tail=tail, P=P, thr=thr, fade=0, n_list=2 * need + nf + 1)
    row.update(over)
    return row


def test_library_refuses_before_it_launches():
    """ctts_trim_pauses_stream_step checks the host mirror first: these calls fail on a machine without a GPU, each with its reason"""
    lib = _lib.lib()
    X, Y = 1 << 24, 1 << 28            # never dereferenced: every call below is refused on its host arguments

    def call(rows, n_x=1 << 20, n_y=1 << 20, n_slots=4, null=(), y=Y, n_fade=480, scratch_bytes=1 << 20, scratch=1 << 16):
        tab = np.zeros(len(rows), _lib.PA_STREAM)
        for i, r in enumerate(rows):
            tab[i] = tuple(r[k] for k in _lib.PA_STREAM.names)
        p = {k: (None if k in null else C.c_void_p(v)) for k, v in (("x", X), ("dev", 4096), ("y", y), ("carry", 8192), ("state", 12288), ("fade", 16384),
                                                                     ("res", 20480), ("scratch", scratch))}
        rc = lib.ctts_trim_pauses_stream_step(p["x"], n_x, p["dev"], tab.ctypes.data_as(C.c_void_p), len(rows), p["y"], n_y, p["carry"], p["state"], n_slots,
                                              p["fade"], n_fade, p["res"], p["scratch"], scratch_bytes, None)
        return rc, lib.ctts_last_error().decode()

    good = lambda **o: _desc(**o)
    g = good()
    assert (g["need"], g["n_list"], g["F"], g["P"]) == (34, 2 * 34 + 21 + 1, 240, 40)                  # 120 + 5000 samples: 21 frames
    second = good(slot=1, out_off=34 * 240 + 5120, fr_off=21, list_off=90)
    cases = [
        *[(dict(rows=[good()], null=(k,)), "null") for k in ("x", "dev", "y", "carry", "state", "fade", "res", "scratch")],
        (dict(rows=[good()] * 1025), "n_streams"), (dict(rows=[]), "n_streams"), (dict(rows=[good()], n_slots=0), "no slot"),
        (dict(rows=[good()], scratch=(1 << 16) + 4), "16-byte"),
        (dict(rows=[good()], y=X + 400), "must not overlap"), (dict(rows=[good()], y=X), "must not overlap"), (dict(rows=[good()], n_fade=-1), "fade table's length"),
        (dict(rows=[good(slot=4)]), "outside the pool"), (dict(rows=[good(slot=-1)]), "outside the pool"),
        (dict(rows=[good(), second, good(slot=0)]), "twice"), (dict(rows=[good(phase=2)]), "phase"), (dict(rows=[good(fin=2)]), "last-push flag"),
        (dict(rows=[good(F=79)]), "a frame of 79 samples"), (dict(rows=[good(F=481)]), "a frame of 481 samples"),
        (dict(rows=[good(P=0)]), "P 1 .. 1000"), (dict(rows=[good(pad=101)]), "pad 0 .. 100"), (dict(rows=[good(lead=-1)]), "lead and tail"),
        (dict(rows=[good(tail=1001)]), "lead and tail"), (dict(rows=[good(thr=0.0)]), "threshold"), (dict(rows=[good(thr=np.nan)]), "threshold"),
        (dict(rows=[good(thr=1.5)]), "threshold"), (dict(rows=[good(fade=241)]), "fade table ["), (dict(rows=[good(fade=-1)]), "fade table ["),
        (dict(rows=[good()], n_fade=239), "fade table ["),
        (dict(rows=[good(P=200)]), "hold 194 frames, a slot holds 112"), (dict(rows=[good(tail=120, need=112)]), "a slot holds 112"),
        (dict(rows=[good(need=33)]), "needs 34 frames, got 33"), (dict(rows=[good(need=112)]), "needs 34 frames"),
        (dict(rows=[good(n_in=-1)]), "negative"), (dict(rows=[good(pos=-1)]), "negative"), (dict(rows=[good(out_off=-8)]), "negative"),
        (dict(rows=[good(in_off=-1)]), "negative"), (dict(rows=[good(n_in=1 << 31)]), "2^31"), (dict(rows=[good(pos=(1 << 31) - 10)]), "2^31"),
        (dict(rows=[good()], n_x=4999), "outside the input"), (dict(rows=[good(in_off=1)], n_x=5000), "outside the input"),
        (dict(rows=[good()], n_y=34 * 240 + 5119), "outside the output"), (dict(rows=[good(out_off=8)], n_y=34 * 240 + 5127), "outside the output"),
        (dict(rows=[good(fr_off=1)]), "copy list is"), (dict(rows=[good(list_off=16)]), "copy list is"), (dict(rows=[good(n_list=89)]), "copy list is"),
        (dict(rows=[good(), good(slot=1, out_off=34 * 240 + 5120)]), "copy list is"),
        (dict(rows=[good(), {**second, "out_off": 34 * 240 + 5119}]), "rooms overlap"), (dict(rows=[good(out_off=100), {**second, "out_off": 0}]), "rooms overlap"),
        (dict(rows=[good(final=True, pos=3000, n_in=5000, n_list=90)]), "copy list is"),                 # a last push counts its partial frame
        (dict(rows=[good()], scratch_bytes=32 + 90 * 16 - 1), "scratch too small"),
    ]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_trim_pauses_stream_step" in msg and why in msg, (why, msg)


# ---- the engine's planning, without a device --------------------------------------------------------------------------------------------
def _engine():
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    eng._pools = {"pauses": SP.StatePool("pauses", 4)}
    return eng


def test_the_engine_plans_a_step_and_commits_nothing_on_its_own():
    eng = _engine()
    a, b = eng.trim_pauses_stream_open(8000), eng.trim_pauses_stream_open(11025, SC.SPECS["bare"])
    assert (a, b) == (0, 1) and eng.trim_pauses_streams_in_use() == 2
    tab, fade, commit = eng._pa_descriptors([(a, 0, 1000, False), (b, 1000, 500, True)])
    assert [int(v) for v in tab["F"]] == [80, 110] and [int(v) for v in tab["need"]] == [34, 4] and [int(v) for v in tab["fin"]] == [0, 1]
    assert [int(v) for v in tab["out_off"]] == [0, 34 * 80 + 1000] and [int(v) for v in tab["fr_off"]] == [0, 12] and [int(v) for v in tab["list_off"]] == [0, 81]
    assert [int(v) for v in tab["n_list"]] == [81, 14] and [int(v) for v in tab["fade"]] == [0, 80] and len(fade) == 190
    assert fade[:80].tobytes() == PA.fade_table(80).tobytes() and fade[80:].tobytes() == PA.fade_table(110).tobytes()
    assert eng._pools["pauses"].records[a] == SP.PauseRec(8000, PA.PauseSpec(), 0, 0, False, 0, 0)
    assert commit == {a: SP.PauseRec(8000, PA.PauseSpec(), 1000, 1, False, 0, 0), b: SP.PauseRec(11025, PA.check_stream(11025, SC.SPECS["bare"])[1], 500, 1, True, 0, 0)}      # nothing committed yet
    st = eng.trim_pauses_stream_stats(a)                             # before the first sample: zeros, no device read
    assert list(st["record"]) == [0] * 8 and (st["pushed"], st["emitted"], st["held"], st["done"]) == (0, 0, 0, False)
    for pushes, why in [([(a, 0, 10, False), (a, 10, 10, False)], "twice"), ([(3, 0, 10, False)], "not open"), ([(a, 0, -1, False)], "negative"),
                        ([(a, 0, 1 << 31, False)], "2\\^31")]:
        with pytest.raises(ValueError, match=why):
            eng._pa_descriptors(pushes)
    for rate, spec, why in [(7000, True, "rate"), (24000, None, "needs a spec"), (24000, {"max_pause_ms": 2000}, "a slot holds 112"), (24000, {"x": 1}, "unknown field")]:
        with pytest.raises(ValueError, match=why):
            eng.trim_pauses_stream_open(rate, spec)
    assert eng.trim_pauses_streams_in_use() == 2                     # a refused open takes no slot
    eng._pools["pauses"].commit({b: eng._pools["pauses"].get(b)._replace(done=True)})
    with pytest.raises(ValueError, match="last push"):
        eng._pa_descriptors([(b, 0, 1, False)])
    eng.trim_pauses_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.trim_pauses_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.trim_pauses_stream_stats(a)
    assert eng.trim_pauses_stream_open(48000) == a and eng._pools["pauses"].records[a] == SP.PauseRec(48000, PA.PauseSpec(), 0, 0, False, 0, 0)


# ---- the default-off plumbing, on fakes -------------------------------------------------------------------------------------------------
TODAY = "a stream would need the run state carried across chunks"


def test_chat_infer_takes_the_paused_stream_when_opted_in_and_keeps_todays_refusal_otherwise():
    from tests.test_resample_stream_host import _bare_chat
    chat = _bare_chat()
    with pytest.raises(ValueError, match="pauses applies to non-streamed inference only \\(" + TODAY + "\\)"):
        chat.infer(["hello"], stream=True, pauses=True, split_text=False)
    assert not chat.calls
    chat.infer(["hello"], stream=True, pauses=True, stream_pauses=True, split_text=False)
    (a, kw), = chat.calls
    assert a[1] is True and kw["pa_spec"] == PA.PauseSpec() and "pauses" not in kw
    chat.infer(["hello"], stream=True, pauses={"max_pause_ms": 200}, stream_pauses=True, split_text=False, sample_rate=8000, stream_resample=True,
               pcm16=True, encoding="ulaw", limiter=True, stream_limiter=True)
    kw = chat.calls[-1][1]
    assert kw["pa_spec"].max_pause_ms == 200 and kw["sample_rate"] == 8000 and kw["encoding"] == "ulaw" and "lm_gain" in kw
    on = dict(stream=True, pauses=True, stream_pauses=True)
    n = len(chat.calls)
    for extra, why in [(dict(split_text=True), "split_text"), (dict(split_text=False, use_decoder=False), "use_decoder=True"),
                       (dict(split_text=False, pauses=[True]), "one pause spec for the whole batch"),
                       (dict(split_text=False, pauses={"max_pause_ms": 2000}), "infer: this spec makes a stream hold 194 frames, a slot holds 112"),
                       (dict(split_text=False, pauses={"tail": 1}), "unknown field"),
                       (dict(split_text=False, sample_rate=7000, stream_resample=True), "rate")]:
        with pytest.raises(ValueError, match=why):
            chat.infer(["hello"], **{**on, **extra})
    assert len(chat.calls) == n                                                 # refused before anything is generated
    chat.infer(["hello"], stream=True, stream_pauses=True, split_text=False)    # the switch alone changes nothing
    assert "pa_spec" not in chat.calls[-1][1]
    chat.infer(["hello"], pauses=True, stream_pauses=True, split_text=False)    # a non-streamed call is today's
    assert chat.calls[-1][1]["pauses"] == PA.PauseSpec() and "pa_spec" not in chat.calls[-1][1]


def test_the_endpoint_serves_a_paused_stream_when_switched_on_and_is_todays_otherwise():
    import logging
    from starlette.testclient import TestClient
    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    from tests.test_stream_resample_host import _StreamBatcher
    body = {"input": "hello", "response_format": "pcm", "stream": True, "pauses": {"max_pause_ms": 200}}

    def app(chat, **kw):
        return TestClient(server.create_app(chat, {"default": "SPK-D"}, logger=logging.getLogger("test_pauses_stream_host"), **kw))

    chat = _EndpointChat()
    with app(chat, pauses=True) as c:                                      # today: the 400 with its text
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "pauses is served for non-streamed requests only" in r.text and not chat.calls
        assert "stream_pauses" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, stream_pauses=True) as c:                               # without `pauses` the switch does nothing
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "pauses" not in chat.calls[-1][2]
        assert "stream_pauses" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, pauses=True, stream_pauses=True) as c:                  # served, serially here
        r = c.post("/v1/audio/speech", json=body)
        text, stream, kw = chat.calls[-1]
        assert r.status_code == 200 and stream and (kw["pauses"].max_pause_ms, kw["stream_pauses"], kw["split_text"]) == (200, True, False)
        n = len(chat.calls)
        for bad in ({**body, "pauses": {"max_pause_ms": 2000}}, {**body, "pauses": {"pause": 1}}, {**body, "pauses": "yes"}):
            assert c.post("/v1/audio/speech", json=bad).status_code == 400, bad
        assert len(chat.calls) == n
        assert c.post("/v1/audio/speech", json={**body, "pauses": False}).status_code == 200 and "stream_pauses" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "pauses": True}).status_code == 200
        assert chat.calls[-1][1] is False and "stream_pauses" not in chat.calls[-1][2]
        assert c.get("/health").json()["stream_pauses"] is True
    chat, bat = _EndpointChat(), _StreamBatcher()                          # through the pool when the pool can take it
    bat.stream_pauses = True
    with app(chat, batcher=bat, batch_streams=True, pauses=True, stream_pauses=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and bat.calls[-1][0] == "hello" and bat.calls[-1][1]["pauses"].max_pause_ms == 200 and not chat.calls
    chat, bat = _EndpointChat(), _StreamBatcher()                          # a pool built without stream_pauses: served serially
    with app(chat, batcher=bat, batch_streams=True, pauses=True, stream_pauses=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and not bat.calls and chat.calls[-1][2]["stream_pauses"] is True

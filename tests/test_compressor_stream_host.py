"""The compressor of streams, the host side (no GPU): `stream_plan`'s arithmetic and refusals, the NumPy twin `StreamCompressor` against
`compress_segment` bit for bit under every cut of tests/compressor_stream_cases.py, the bounds on what a stream carries, the lag law, the
record and the pool, the new symbols, the library's refusals (each comes before any launch), the engine's planning and the plumbing of
Plan-free `decode_windows`, Chat, SpeechBatcher and the endpoint on fakes."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from chattts_amd import _lib, compressor as CP, statepool as SP
from tests import compressor_cases as CC, compressor_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "chattts_amd.h")
TODAY = "a compressed stream would need the block state carried across chunks"


# ---- stream_plan ------------------------------------------------------------------------------------------------------------------------
def test_stream_plan_sums_and_refusals():
    B, A, H = 24, 5, 60
    p = CP.stream_plan(B, A, 0, 0, 1000, False, H)                                       # 41 whole blocks: 35 are out
    assert p == dict(total=1000, e_lo=0, n_out=35 * B, emitted=35 * B, carry_in=0, carry_out=1000 - 35 * B, c_keep=41)
    p = CP.stream_plan(B, A, 1000, 35 * B, 2400, False, H)                               # 141 whole blocks: 135 out, the c of 135 - 66 .. 140 kept
    assert p == dict(total=3400, e_lo=840, n_out=100 * B, emitted=135 * B, carry_in=160, carry_out=3400 - 135 * B, c_keep=141 - 69)
    p = CP.stream_plan(B, A, 3400, 135 * B, 7, True, H)
    assert p == dict(total=3407, e_lo=135 * B, n_out=3407 - 135 * B, emitted=3407, carry_in=160, carry_out=0, c_keep=0)
    assert CP.stream_plan(B, A, 0, 0, 0, True, H) == dict(total=0, e_lo=0, n_out=0, emitted=0, carry_in=0, carry_out=0, c_keep=0)
    assert CP.stream_plan(B, A, 0, 0, (A + 1) * B + B - 1, False, H)["n_out"] == 0       # the lag: A + 1 blocks and the open one
    assert CP.stream_plan(B, A, 0, 0, (A + 2) * B, False, H)["n_out"] == B
    assert CP.stream_plan(B, A, 0, 0, 10 ** 6, False)["c_keep"] == 2 * A + CP.H_MAX + 2  # without H: the longest hold, the bound
    rng = np.random.default_rng(0)
    for _ in range(300):                                                                 # the sums, over random schedules
        B, A, H = int(rng.integers(8, 49)), int(rng.integers(1, 21)), int(rng.integers(0, 501))
        pushed = emitted = 0
        for k in range(6):
            n, fin = int(rng.integers(0, 3000)), k == 5
            p = CP.stream_plan(B, A, pushed, emitted, n, fin, H)
            assert p["total"] == pushed + n and p["e_lo"] == emitted and p["emitted"] == emitted + p["n_out"] and p["carry_in"] == pushed - emitted
            assert p["carry_out"] == (0 if fin else p["total"] - p["emitted"]) <= CP.STREAM_CARRY and 0 <= p["c_keep"] <= CP.STREAM_HIST
            assert fin or p["emitted"] % B == 0
            pushed, emitted = p["total"], p["emitted"]
        assert emitted == pushed
    for args, why in [((7, 5, 0, 0, 1, False), "B = fs // 1000"), ((49, 5, 0, 0, 1, False), "B = fs // 1000"), ((24, 0, 0, 0, 1, False), "attack"),
                      ((24, 21, 0, 0, 1, False), "attack"), ((24, 5, 0, 0, 1, False, 501), "hold"), ((24, 5, -1, 0, 1, False), "negative"),
                      ((24, 5, 0, 0, -1, False), "negative"), ((24, 5, 0, -24, 1, False), "negative"), ((24, 5, 1000, 0, 1, False), "has emitted 840, not 0"),
                      ((24, 5, 100, 24, 1, False), "has emitted 0, not 24"), ((24, 5, 0, 0, 1 << 31, False), "2\\^31"),
                      ((24, 5, (1 << 31) - 24, ((1 << 31) - 24) // 24 * 24 - 6 * 24, 24, True), "2\\^31")]:
        with pytest.raises(ValueError, match=why):
            CP.stream_plan(*args)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", SC.RATES)
def test_the_twin_stream_equals_the_one_shot_twin_under_every_cut(fs):
    seen_c = seen_h = runs = 0
    for (name, x, spec), (y, rec) in zip(CC.cases(fs), CC.twin(fs)):
        for cut_name, cut in SC.case_cuts(fs, x, spec):
            chunks, st, most_c, most_h, n_out = SC.run_twin(fs, x, spec, cut)
            got = np.concatenate(chunks)
            assert got.dtype == np.float32 and got.tobytes() == y.tobytes(), (fs, name, cut_name)
            assert st.tobytes() == rec.tobytes(), (fs, name, cut_name, st, rec)
            assert [len(c) for c in chunks] == n_out, (fs, name, cut_name)               # the lag law: every push emits exactly n_out
            assert most_c <= CP.STREAM_CARRY and most_h <= CP.STREAM_HIST
            seen_c, seen_h, runs = max(seen_c, most_c), max(seen_h, most_h), runs + 1
    assert runs == len(CC.cases(fs)) * len(SC.CUT_NAMES)
    for name, x, spec, cut in SC.totals_under_lag(fs):
        chunks, st, _, _, n_out = SC.run_twin(fs, x, spec, cut)
        y, rec = CP.compress_segment(x, fs, spec)
        assert n_out[:-1] == [0] * (len(cut) - 1) and chunks[-1].tobytes() == y.tobytes() and st.tobytes() == rec.tobytes(), name
    if fs == 48000:                                                                      # the bounds are reached, not only respected
        assert seen_c == CP.STREAM_CARRY == 1055 and seen_h == CP.STREAM_HIST == 542


def test_the_longest_spec_at_48_khz_fills_at_least_half_of_each_bound():
    fs, spec = 48000, {"attack_ms": 20, "hold_ms": 500}
    x = CC.enveloped(3, 800 * 48 + 17, 48)
    _, st, most_c, most_h, _ = SC.run_twin(fs, x, spec, [100 * 48 + 47] * 7 + [len(x) - 7 * (100 * 48 + 47)])
    assert 2 * most_c >= CP.STREAM_CARRY and 2 * most_h >= CP.STREAM_HIST and most_c <= CP.STREAM_CARRY and most_h <= CP.STREAM_HIST
    assert st.tobytes() == CP.compress_segment(x, fs, spec)[1].tobytes()


def test_the_twin_carries_no_sample_older_than_what_it_has_emitted_and_refuses_with_reasons():
    sc = CP.StreamCompressor(24000, {"attack_ms": 2, "hold_ms": 500})
    x = CC.enveloped(4, 24000, 24)
    for k in range(9):
        sc.push(x[k * 2400: (k + 1) * 2400])
        assert len(sc.carry) == sc.pushed - sc.emitted < (sc.A + 2) * sc.B and len(sc.hist) <= 2 * sc.A + sc.H + 2
        assert sc.carry.tobytes() == x[sc.emitted: sc.pushed].tobytes()
    left = sc.pushed - sc.emitted
    assert sc.push(np.zeros(0, np.float32), True).size == left and sc.carry.size == 0 and sc.hist.size == 0      # an empty last push brings the rest
    with pytest.raises(ValueError, match="last push"):
        sc.push(x[:1])
    empty = CP.StreamCompressor(8000, True)
    assert empty.push(np.zeros(0, np.float32), True).size == 0
    assert (empty.stats["min_gain"], empty.stats["n_blocks"], empty.stats["n_touched"], empty.stats["peak"]) == (1.0, 0, 0, 0.0)
    for args, why in [((7999, True), "rate"), ((24000, None), "spec is off"), ((24000, False), "spec is off"), ((24000, {"hold": 1}), "unknown compressor field"),
                      ((24000, {"attack_ms": 21}), "attack_ms is a number in 1 .. 20")]:
        with pytest.raises(ValueError, match=why):
            CP.StreamCompressor(*args)


# ---- the record and the pool ------------------------------------------------------------------------------------------------------------
def test_compress_rec_and_the_pools_doubling():
    from chattts_amd.engine import CodecEngine
    label, (slots, buffers) = "compress", CodecEngine.POOLS["compress"]
    assert getattr(CodecEngine, slots) == 64 and set(buffers) == {"carry", "hist", "stats"}
    assert buffers["carry"][0] == (2, 1056) and buffers["hist"][0] == (2, 544) and buffers["stats"][0] == (4,)
    assert buffers["carry"][0][1] >= CP.STREAM_CARRY and buffers["hist"][0][1] >= CP.STREAM_HIST
    assert SP.CompressRec._fields == ("rate", "spec", "pushed", "emitted", "phase", "done")
    import torch
    pool = SP.StatePool(label, 2, buffers, torch.device("cpu"))
    a, b = pool.open(SP.CompressRec(8000, CP.check(True), 0, 0, 0, False)), pool.open(SP.CompressRec(48000, CP.check(True), 0, 0, 0, False))
    pool.buf["carry"][b].fill_(3.0)
    pool.buf["stats"][b].fill_(7)
    c = pool.open(SP.CompressRec(24000, CP.check(True), 0, 0, 0, False))                 # full: every buffer doubles and keeps its rows
    assert (a, b, c) == (0, 1, 2) and pool.slots == 4 and pool.in_use == 3
    assert all(int(v.shape[0]) == 4 for v in pool.buf.values()) and bool((pool.buf["carry"][b] == 3.0).all()) and bool((pool.buf["stats"][b] == 7).all())
    assert bool((pool.buf["carry"][2:] == 0).all()) and bool((pool.buf["hist"][2:] == 0).all())
    pool.commit({b: pool.get(b)._replace(done=True)})
    with pytest.raises(ValueError, match="last push"):
        pool.live(b)
    pool.close(a)
    assert pool.open(SP.CompressRec(8000, CP.check(True), 0, 0, 0, False)) == a


# ---- the symbol -------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported_declared_and_bound_and_the_layouts_agree():
    lib = _lib.lib()
    with open(HEADER) as f:
        header = f.read()
    for name, nargs in (("ctts_compress_stream_step", 17), ("ctts_compress_stream_scratch_bytes", 1)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs
    assert lib.ctts_compress_stream_step.argtypes == _lib.SIGNATURES["ctts_compress_stream_step"][1]
    assert _lib.CP_STREAM.itemsize == 104 and "} ctts_cp_stream;" in header
    struct = header[header.index("#define CTTS_CP_SHIST"): header.index("} ctts_cp_stream;")]
    fields = [n for line in struct.splitlines() if line.strip().startswith(("int64_t", "int32_t"))
              for n in re.sub(r"/\*.*", "", line).replace("int64_t", "").replace("int32_t", "").replace(";", "").replace(" ", "").split(",")]
    assert tuple(fields) == _lib.CP_STREAM.names
    assert [_lib.CP_STREAM.fields[n][1] for n in ("cb_off", "slot", "tab", "h_out")] == [56, 64, 84, 100]
    from chattts_amd.engine import CodecEngine
    assert re.search(r"#define CTTS_CP_SCARRY %d\b" % CodecEngine.CP_CARRY, header) and re.search(r"#define CTTS_CP_SHIST %d\b" % CodecEngine.CP_HIST, header)
    with open(os.path.join(ROOT, "chattts_amd", "csrc", "kernels.hpp")) as f:
        k = f.read()
    assert re.search(r"#define CP_SCARRY %d\b" % CodecEngine.CP_CARRY, k) and re.search(r"#define CP_SHIST %d\b" % CodecEngine.CP_HIST, k)
    assert lib.ctts_compress_stream_scratch_bytes(0) == 16 and lib.ctts_compress_stream_scratch_bytes(5) == 32
    assert lib.ctts_compress_stream_scratch_bytes(1000) == 4000 and lib.ctts_compress_stream_scratch_bytes(-1) == 0 == lib.ctts_compress_stream_scratch_bytes(1 << 31)


# ---- the library's refusals -------------------------------------------------------------------------------------------------------------
def _desc(fs=24000, att=5, hold=60, at=1000, n=2400, final=False, slot=0, phase=0, tab=0, **over):
    """a descriptor that agrees with `stream_plan` (n samples arrive at position `at`), then `over` written over its fields"""
    B, A, H, pos, n_in = fs // 1000, att, hold, at, n
    p = CP.stream_plan(B, A, pos, max(0, pos // B - A - 1) * B, n_in, final, H)
    h_in = pos // B - max(0, p["e_lo"] // B - A - H - 1)
    row = dict(in_off=0, n_in=n_in, pos=pos, total=p["total"] if final else -1, e_lo=p["e_lo"], n_out=p["n_out"], out_off=0, cb_off=0, slot=slot,
               phase=phase, rate=fs, A=A, H=H, tab=tab, c_in=p["carry_in"], c_out=p["carry_out"], h_in=h_in, h_out=p["c_keep"])
    row.update(over)
    return row


def test_library_refuses_before_it_launches():
    """ctts_compress_stream_step checks the host mirror first: these calls fail on a machine without a GPU, each with its reason"""
    lib = _lib.lib()
    X, Y = 1 << 24, 1 << 28            # never dereferenced: every call below is refused on its host arguments
    tabs = np.stack([CP.table(CP.check(True)), CP.table(CP.check(CC.SPECS[4]))])

    def call(rows, n_x=1 << 20, n_y=1 << 20, n_slots=4, null=(), x=X, y=Y, n_tab=1, tab_host=tabs, scratch_bytes=1 << 20, scratch=1 << 16, tab_dev=1 << 12):
        tab = np.zeros(len(rows), _lib.CP_STREAM)
        for i, r in enumerate(rows):
            tab[i] = tuple(r[k] for k in _lib.CP_STREAM.names)
        p = {k: (None if k in null else C.c_void_p(v)) for k, v in (("x", x), ("dev", 4096 * 3), ("tab_dev", tab_dev), ("y", y), ("carry", 8192),
                                                                     ("hold", 8192 * 3), ("stats", 12288), ("scratch", scratch))}
        th = None if "tab_host" in null else np.ascontiguousarray(tab_host).ctypes.data_as(C.c_void_p)
        rc = lib.ctts_compress_stream_step(p["x"], n_x, p["dev"], None if "host" in null else tab.ctypes.data_as(C.c_void_p), len(rows), p["tab_dev"], th,
                                           n_tab, p["y"], n_y, p["carry"], p["hold"], p["stats"], n_slots, p["scratch"], scratch_bytes, None)
        return rc, lib.ctts_last_error().decode()

    good = lambda **o: _desc(**o)
    g = good()
    assert (g["e_lo"], g["n_out"], g["c_in"], g["c_out"], g["h_in"], g["h_out"]) == (840, 2400, 160, 160, 41, 72)
    second = good(slot=1, out_off=2400, cb_off=100)
    bad_tab = lambda q, v: (lambda t: (t.__setitem__((0, q), v), t)[1])(tabs.copy())
    cases = [
        *[(dict(rows=[good()], null=(k,)), "null") for k in ("x", "dev", "host", "tab_dev", "tab_host", "y", "carry", "hold", "stats", "scratch")],
        (dict(rows=[good()] * 1025), "n_streams"), (dict(rows=[]), "n_streams"), (dict(rows=[good()], n_slots=0), "no slot"),
        (dict(rows=[good()], scratch=(1 << 16) + 4), "16-byte"), (dict(rows=[good()], x=X + 4), "16-byte"), (dict(rows=[good()], tab_dev=(1 << 12) + 8), "16-byte"),
        (dict(rows=[good()], y=X + 400), "must not overlap"), (dict(rows=[good()], y=X), "must not overlap"),
        (dict(rows=[good()], n_tab=0), "n_tab"), (dict(rows=[good()], n_tab=2), "n_tab"),
        (dict(rows=[good()], tab_host=bad_tab(0, np.float32(2.0 ** -19))), "table 0: entry 0"), (dict(rows=[good()], tab_host=bad_tab(1023, np.float32(1.0001))), "entry 1023"),
        (dict(rows=[good()], tab_host=bad_tab(5, np.float32(np.nan))), "entry 5"),
        (dict(rows=[good(slot=4)]), "outside the pool"), (dict(rows=[good(slot=-1)]), "outside the pool"),
        (dict(rows=[good(), second, good(slot=0, cb_off=200)], n_tab=1), "twice"), (dict(rows=[good(phase=2)]), "phase"),
        (dict(rows=[good(rate=7990)]), "rate"), (dict(rows=[good(rate=48010)]), "rate"), (dict(rows=[good(rate=24005)]), "rate"),
        (dict(rows=[good(A=0)]), "attack is 1 .. 20"), (dict(rows=[good(A=21)]), "attack is 1 .. 20"), (dict(rows=[good(H=-1)]), "hold is 0 .. 500"),
        (dict(rows=[good(H=501)]), "hold is 0 .. 500"), (dict(rows=[good(tab=1)]), "gain table 1 is outside the 1 given"), (dict(rows=[good(tab=-1)]), "gain table"),
        (dict(rows=[good(n_in=-1)]), "negative"), (dict(rows=[good(pos=-1)]), "negative"), (dict(rows=[good(out_off=-8)]), "negative"),
        (dict(rows=[good(in_off=-1)]), "negative"), (dict(rows=[good(n_in=1 << 31)]), "2^31"), (dict(rows=[good(pos=(1 << 31) - 10, e_lo=0)]), "2^31"),
        (dict(rows=[good()], n_x=2399), "outside the input"), (dict(rows=[good(in_off=1)], n_x=2400), "outside the input"),
        (dict(rows=[good(total=3401)]), "a last push ends the stream at pos + n_in = 3400"), (dict(rows=[good(total=0)]), "a last push"),
        (dict(rows=[good(e_lo=816)]), "have emitted 840"), (dict(rows=[good(n_out=2399)]), "emits 2400"), (dict(rows=[good(n_out=2424)]), "emits 2400"),
        (dict(rows=[good()], n_y=2399), "outside the output"), (dict(rows=[good(out_off=8)], n_y=2407), "outside the output"),
        (dict(rows=[good(c_in=159)]), "carries 160 samples in and 160 out"), (dict(rows=[good(c_out=0)]), "carries 160 samples in and 160 out"),
        (dict(rows=[good(h_in=40)]), "carries 41 block gains in and 72 out"), (dict(rows=[good(h_out=141)]), "carries 41 block gains in and 72 out"),
        (dict(rows=[good(final=True, c_out=1)]), "samples in and 0 out"), (dict(rows=[good(final=True, h_out=1)]), "block gains in and 0 out"),
        (dict(rows=[good(cb_off=4)]), "start at float 0"), (dict(rows=[good(), {**second, "cb_off": 99}]), "start at float 100"),
        (dict(rows=[good()], scratch_bytes=399), "scratch too small"), (dict(rows=[good(), second], scratch_bytes=799), "scratch too small"),
    ]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_compress_stream_step" in msg and why in msg, (why, msg)


# ---- the engine's planning, without a device --------------------------------------------------------------------------------------------
def _engine():
    import torch
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    eng.device = torch.device("cpu")
    eng._pools = {"compress": SP.StatePool("compress", 4, CodecEngine.POOLS["compress"][1], eng.device)}
    return eng


def test_the_engine_plans_a_step_and_commits_nothing_on_its_own():
    eng = _engine()
    a, b = eng.compress_stream_open(8000, {"attack_ms": 2, "hold_ms": 0}), eng.compress_stream_open(48000)
    assert (a, b) == (0, 1) and eng.compress_streams_in_use() == 2
    st = eng.compress_stream_stats(a)                                                    # the record is set when the stream is opened
    assert (st["min_gain"], st["n_blocks"], st["n_touched"], st["peak"]) == (1.0, 0, 0, 0.0)
    tab, tabs, commit, n_new = eng._cp_descriptors([(a, 0, 1000, False), (b, 1000, 500, True)])
    assert [int(v) for v in tab["n_out"]] == [(125 - 3) * 8, 500] and [int(v) for v in tab["total"]] == [-1, 500] and [int(v) for v in tab["c_out"]] == [24, 0]
    assert [int(v) for v in tab["rate"]] == [8000, 48000] and [int(v) for v in tab["A"]] == [2, 5] and [int(v) for v in tab["H"]] == [0, 60]
    assert [int(v) for v in tab["tab"]] == [0, 1] and [int(v) for v in tab["cb_off"]] == [0, 125] and n_new == 125 + 11 and tabs.shape == (2, CP.TABLE)
    assert [int(v) for v in tab["h_in"]] == [0, 0] and [int(v) for v in tab["h_out"]] == [125 - (122 - 3), 0] and [int(v) for v in tab["slot"]] == [a, b]
    assert tabs[0].tobytes() == CP.table(CP.check({"attack_ms": 2, "hold_ms": 0})).tobytes() and tabs[1].tobytes() == CP.table(CP.check(True)).tobytes()
    assert eng._pools["compress"].records[a] == SP.CompressRec(8000, CP.check({"attack_ms": 2, "hold_ms": 0}), 0, 0, 0, False)      # nothing committed yet
    assert commit[a] == SP.CompressRec(8000, CP.check({"attack_ms": 2, "hold_ms": 0}), 1000, 976, 1, False)
    assert commit[b] == SP.CompressRec(48000, CP.check(True), 500, 500, 1, True)
    assert eng.compress_stream_plan(a, 1000, False)["n_out"] == 976
    same = eng._cp_descriptors([(a, 0, 10, False), (b, 0, 10, False), (eng.compress_stream_open(24000, True), 0, 10, False)])[0]
    assert [int(v) for v in same["tab"]] == [0, 1, 1]                                    # equal specs share one table
    with pytest.raises(ValueError, match="twice"):
        eng._cp_descriptors([(a, 0, 10, False), (a, 10, 10, False)])
    with pytest.raises(ValueError, match="not open"):
        eng._cp_descriptors([(3, 0, 10, False)])
    with pytest.raises(ValueError, match="2\\^31"):
        eng._cp_descriptors([(a, 0, 1 << 31, False)])
    for rate, spec, why in [(7000, True, "rate"), (24005, True, "rate"), (24000, None, "spec is off"), (24000, False, "spec is off"),
                            (24000, {"x": 1}, "unknown compressor field"), (24000, {"hold_ms": 501}, "hold_ms is a number in 0 .. 500")]:
        with pytest.raises(ValueError, match=why):
            eng.compress_stream_open(rate, spec)
    assert eng.compress_streams_in_use() == 3                                            # a refused open takes no slot
    eng._pools["compress"].commit({b: eng._pools["compress"].get(b)._replace(done=True)})
    with pytest.raises(ValueError, match="last push"):
        eng.compress_stream_plan(b, 1, False)
    eng._pools["compress"].buf["stats"][a].fill_(9)
    eng.compress_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.compress_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.compress_stream_stats(a)
    assert eng.compress_stream_open(22050, True) == a and eng.compress_stream_stats(a)["min_gain"] == 1.0 and eng.compress_stream_stats(a)["n_blocks"] == 0


def test_decode_windows_checks_the_compressor_streams_before_anything_else():
    eng = _engine()
    wins = [(0, 40, 0, 12000), (1, 40, 0, 12000, True)]
    h24, h8 = eng.compress_stream_open(24000), eng.compress_stream_open(8000)
    for kw, why in [(dict(compress=[True], cp_streams=[h24, None]), "one compress flag and one cp_streams entry per window"),
                    (dict(compress=[True, False]), "one compress flag and one cp_streams entry per window"),
                    (dict(compress=[True, None], cp_streams=[None, None]), "needs an open compressor stream at 24000 Hz"),
                    (dict(compress=[True, False], cp_streams=[h8, None]), "needs an open compressor stream at 24000 Hz"),
                    (dict(compress=[True, False], cp_streams=[h24, None], sample_rates=[8000, 24000]), "needs an open compressor stream at 8000 Hz"),
                    (dict(compress=[False, True], cp_streams=[h24, h24]), "no compress flag but names"),
                    (dict(compress=[False, None], cp_streams=[h24, None]), "cp_streams without a compress flag"),
                    (dict(cp_streams=[None, h24]), "cp_streams without a compress flag")]:
        with pytest.raises(ValueError, match=why):
            eng.decode_windows(None, wins, **kw)
    with pytest.raises(ValueError, match="has had its last push"):                      # a tail, then another window of the stream
        eng.decode_windows(None, [wins[1], wins[0]], compress=[True, True], cp_streams=[h24, h24])
    assert eng._pools["compress"].records[h24] == SP.CompressRec(24000, CP.check(True), 0, 0, 0, False)


# ---- the default-off plumbing, on fakes -------------------------------------------------------------------------------------------------
def test_chat_infer_takes_the_compressed_stream_when_opted_in_and_keeps_todays_refusal_otherwise():
    from tests.test_resample_stream_host import _bare_chat
    chat = _bare_chat()
    with pytest.raises(ValueError, match="compress applies to non-streamed inference only \\(" + TODAY + "\\)"):
        chat.infer(["hello"], stream=True, compress=True, split_text=False)
    assert not chat.calls
    chat.infer(["hello"], stream=True, compress=True, stream_compress=True, split_text=False)
    (a, kw), = chat.calls
    assert a[1] is True and kw["cp_spec"] == CP.check(True) and "compress" not in kw
    chat.infer(["hello"], stream=True, compress={"hold_ms": 200}, stream_compress=True, split_text=False, sample_rate=8000, stream_resample=True,
               pcm16=True, encoding="ulaw", limiter=True, stream_limiter=True, pauses=True, stream_pauses=True)
    kw = chat.calls[-1][1]
    assert kw["cp_spec"][4] == 200.0 and kw["sample_rate"] == 8000 and kw["encoding"] == "ulaw" and "lm_gain" in kw and "pa_spec" in kw
    on = dict(stream=True, compress=True, stream_compress=True)
    n = len(chat.calls)
    for extra, why in [(dict(split_text=True), "split_text"), (dict(split_text=False, use_decoder=False), "use_decoder=True"),
                       (dict(split_text=False, compress=[True]), "one compressor spec for the whole batch"),
                       (dict(split_text=False, compress={"hold_ms": 2000}), "hold_ms is a number in 0 .. 500"),
                       (dict(split_text=False, compress={"hold": 1}), "unknown compressor field"),
                       (dict(split_text=False, sample_rate=7000, stream_resample=True), "rate")]:
        with pytest.raises(ValueError, match=why):
            chat.infer(["hello"], **{**on, **extra})
    assert len(chat.calls) == n                                                          # refused before anything is generated
    chat.infer(["hello"], stream=True, compress=CP.check({"hold_ms": 10}), stream_compress=True, split_text=False)      # a checked spec, as the endpoint passes it
    assert chat.calls[-1][1]["cp_spec"] == CP.check({"hold_ms": 10})
    chat.infer(["hello"], stream=True, stream_compress=True, split_text=False)           # the switch alone changes nothing
    assert "cp_spec" not in chat.calls[-1][1]
    chat.infer(["hello"], stream=True, compress=False, stream_compress=True, split_text=False)
    assert "cp_spec" not in chat.calls[-1][1]
    chat.infer(["hello"], compress=True, stream_compress=True, split_text=False)         # a non-streamed call is today's
    assert chat.calls[-1][1]["compress"] == CP.check(True) and "cp_spec" not in chat.calls[-1][1]


class _CpCodec:
    """the part of CodecEngine the compressed streams touch, recorded"""
    SAMPLE_RATE = 24000

    def __init__(self):
        self.log, self.free = [], [33, 32, 31, 30]

    def compress_stream_open(self, rate, spec=True):
        self.log.append(("cp_open", rate, CP.check(spec)))
        return self.free.pop()

    def compress_stream_close(self, h):
        self.log.append(("cp_close", h))
        self.free.append(h)

    def decode_window(self, hiddens, a, b, sample_rate=None):
        import torch
        self.log.append(("window", a, b, sample_rate))
        return torch.arange(len(hiddens) * (b - a), dtype=torch.float32).view(len(hiddens), b - a)

    def compress_stream_step(self, x, pushes):
        import torch
        self.log.append(("cp_step", [tuple(p) for p in pushes]))
        B = len(pushes)
        return torch.ones(B * 60), np.arange(B + 1, dtype=np.int64) * 60

    def to_host(self, t):
        return t.numpy()


def test_the_serial_stream_steps_the_rows_compressor_streams_and_closes_them():
    import torch
    from types import SimpleNamespace
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.codec, chat.device, chat.incremental_stream = _CpCodec(), torch.device("cpu"), True
    hid = [torch.zeros((10, 768)), torch.zeros((10, 768))]
    rows = chat._stream_rows_paused(hid, 0, 3000, False, None, cp_handles=[30, 31])
    assert [r.shape for r in rows] == [(60,), (60,)] and rows[0].dtype == np.float32
    assert chat.codec.log == [("window", 0, 3000, None), ("cp_step", [(30, 0, 3000, False), (31, 3000, 3000, False)])]
    chat.codec.log.clear()
    rows = chat._stream_rows_paused(hid, 256 * 19, None, True, None, 8000, cp_handles=[30, 31])      # nothing left: the streams are stepped all the same
    assert [r.shape for r in rows] == [(60,), (60,)] and chat.codec.log == [("cp_step", [(30, 0, 0, True), (31, 0, 0, True)])]
    chat.codec.log.clear()
    chat.has_loaded = lambda use_decoder=True: True
    chat.normalizer = lambda t, *a: t
    seen = {}

    def batches(text, step, stream, use_decoder, split_text, params, pcm16, ragged, raw, sample_rate, encoding, speed, sets, cp_spec=None):
        from chattts_amd.winchain import StreamSet
        seen.update(sets=sets, spec=cp_spec)
        sets.extend(StreamSet.open(chat.codec, rate=sample_rate, speed=speed, compress=cp_spec) for _ in text)
        yield "chunk"
        raise RuntimeError("the consumer's problem")
    chat._infer_batches = batches
    spec = CP.check({"hold_ms": 100})
    gen = chat._infer(["a", "b"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None), sample_rate=8000, cp_spec=spec)
    assert next(gen) == "chunk" and [dict(st) for st in seen["sets"]] == [{"compress": 30}, {"compress": 31}] and seen["spec"] == spec      # no other stream
    with pytest.raises(RuntimeError):
        next(gen)
    assert chat.codec.log == [("cp_open", 8000, spec), ("cp_open", 8000, spec), ("cp_close", 30), ("cp_close", 31)]
    chat._infer_batches = lambda *a, **kw: iter([kw])
    assert next(chat._infer(["a"], True, None, True, False, True, True, True, False, 4, None, SimpleNamespace(spk_smp=None))) == {}   # today's call


def _compressed_chat():
    from tests.test_resample_stream_host import _RsCodec
    from tests.test_stream_pool_host import _FakeChat, _piece

    class _Codec(_RsCodec, _CpCodec):
        def __init__(self):
            _RsCodec.__init__(self)
            self.free = [33, 32, 31, 30]

    class _Chat(_FakeChat):
        def __init__(self):
            super().__init__()
            self.codec, self.kw_calls = _Codec(), []

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            return [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]
    return _Chat()


def test_submit_stream_takes_the_compressor_when_opted_in_and_gives_the_stream_back():
    from chattts_amd.serving import SpeechBatcher
    from tests.test_resample_stream_host import _wait
    from tests.test_stream_pool_host import _FakePool, _Params
    lock, holder = threading.Lock(), {}
    chat = _compressed_chat()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_compress=True)
    try:
        for kw, why in [(dict(compress={"ratio": 1}), "ratio is a number in 1.5 .. 20"), (dict(compress="yes"), "takes True, False, None or a dict"),
                        (dict(compress=True, sample_rate=7000), "rate")]:
            with pytest.raises(ValueError, match=why):
                b.submit_stream("x", _Params(48), **kw)
        with lock:
            streams = [b.submit_stream("A", _Params(96), compress={"hold_ms": 100}, sample_rate=8000, encoding="ulaw"), b.submit_stream("B", _Params(96)),
                       b.submit_stream("C", _Params(96), compress=True)]
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in enumerate(streams)]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        assert all(len(got[k]) > 0 for k in range(3))
        full = [(w, kw) for w, kw in zip(chat.window_calls, chat.kw_calls) if len(w) == 3]
        assert full
        for w, kw in full:
            by = {x[0]: k for k, x in enumerate(w)}
            assert set(kw) == {"sample_rates", "encodings", "compress", "cp_streams"}, kw
            assert [kw["compress"][by[k]] for k in range(3)] == [CP.check({"hold_ms": 100}), None, CP.check(True)]
            assert kw["cp_streams"][by[0]] == 30 and kw["cp_streams"][by[1]] is None and kw["cp_streams"][by[2]] == 31
        _wait(lambda: sum(e[0] == "cp_close" for e in chat.codec.log) == 2)
        opens = [e for e in chat.codec.log if e[0] == "cp_open"]
        assert opens == [("cp_open", 8000, CP.check({"hold_ms": 100})), ("cp_open", 24000, CP.check(True))]
        s = b.submit_stream("D", _Params(400), compress=True)                      # a cancelled one gives its stream back too
        assert len(next(s)) > 0
        s.close()
        _wait(lambda: sum(e[0] == "cp_close" for e in chat.codec.log) == 3)
        n = len(chat.kw_calls)
        assert len(list(b.submit_stream("E", _Params(48)))) > 0                    # without the spec: the call before this option
        assert len(list(b.submit_stream("F", _Params(48), compress=False))) > 0
        assert all("compress" not in kw and "cp_streams" not in kw for kw in chat.kw_calls[n:])
        assert b.occupancy()["stream_compressed_chunks"] > 0
    finally:
        b.close()
    off = SpeechBatcher(_compressed_chat(), 2, lock, make_pool=lambda: _FakePool(2, lock), streams=True)
    try:
        with pytest.raises(TypeError, match="block state carried across chunks"):
            off.submit_stream("x", _Params(48), compress=True)
        assert "stream_compressed_chunks" not in off.occupancy()
    finally:
        off.close()
    assert not lock.locked()


def test_the_endpoint_serves_a_compressed_stream_when_switched_on_and_is_todays_otherwise():
    import logging
    from starlette.testclient import TestClient
    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    from tests.test_stream_resample_host import _StreamBatcher
    body = {"input": "hello", "response_format": "pcm", "stream": True, "compress": {"hold_ms": 200}}

    def app(chat, **kw):
        return TestClient(server.create_app(chat, {"default": "SPK-D"}, logger=logging.getLogger("test_compressor_stream_host"), **kw))

    chat = _EndpointChat()
    with app(chat, compress=True) as c:                                    # today: the 400 with its text
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "compress is served for non-streamed requests only" in r.text and TODAY in r.text and not chat.calls
        assert "stream_compress" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, stream_compress=True) as c:                             # without `compress` the switch does nothing
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "compress" not in chat.calls[-1][2]
        assert "stream_compress" not in c.get("/health").json() and "compress" not in c.get("/health").json()
    chat = _EndpointChat()
    with app(chat, compress=True, stream_compress=True) as c:              # served, serially here
        r = c.post("/v1/audio/speech", json=body)
        text, stream, kw = chat.calls[-1]
        assert r.status_code == 200 and stream and (kw["compress"][4], kw["stream_compress"], kw["split_text"]) == (200.0, True, False)
        n = len(chat.calls)
        for bad in ({**body, "compress": {"hold_ms": 2000}}, {**body, "compress": {"hold": 1}}, {**body, "compress": "yes"}):
            assert c.post("/v1/audio/speech", json=bad).status_code == 400, bad
        assert len(chat.calls) == n
        assert c.post("/v1/audio/speech", json={**body, "compress": False}).status_code == 200 and "stream_compress" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "compress": True}).status_code == 200
        assert chat.calls[-1][1] is False and "stream_compress" not in chat.calls[-1][2]
        assert c.get("/health").json()["stream_compress"] is True and c.get("/health").json()["compress"] is True
    chat, bat = _EndpointChat(), _StreamBatcher()                          # through the pool when the pool can take it
    bat.stream_compress = True
    with app(chat, batcher=bat, batch_streams=True, compress=True, stream_compress=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and bat.calls[-1][0] == "hello" and bat.calls[-1][1]["compress"][4] == 200.0 and not chat.calls
    chat, bat = _EndpointChat(), _StreamBatcher()                          # a pool built without stream_compress: served serially
    with app(chat, batcher=bat, batch_streams=True, compress=True, stream_compress=True) as c:
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and not bat.calls and chat.calls[-1][2]["stream_compress"] is True

"""Loudness normalisation, the parts that need no GPU: the K-weighting's coefficients and calibration tones, the NumPy twin
(chattts_amd/loudness.py) against the independent serial oracle (tests/loudness_oracle.py), the block, gate, gain and group rules, every
refusal of the host side and of ctts_loudness_normalize_ragged, and the plumbing of `loudness` through Chat, the batcher and the endpoint
on fakes."""
import ctypes as C
import logging
import math
import threading
import types

import numpy as np
import pytest
import torch

from chattts_amd import _lib, build, loudness as LN
from chattts_amd.serving import SpeechBatcher
from tests import loudness_cases as LC
from tests import loudness_oracle as O
from tests.test_split_pool_host import _Catch, _EndpointChat, _FakeBatcher, _FakeChat, _Params, _Pool, _spell, _wait_idle


# ---- 1. the filter ----------------------------------------------------------------------------------------------------------------------
def test_shelf_coefficients_at_48_khz_are_the_standards_table():
    b1, a1, b2, a2 = LN.coefficients(48000)
    assert np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() < 1e-12
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() < 1e-12
    assert list(b2) == [1.0, -2.0, 1.0] and np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() < 1e-8      # BS.1770-4 table 2
    ob = O.k_coefficients(48000)
    assert all(np.abs(np.asarray(p) - np.asarray(q)).max() < 1e-15 for p, q in zip((b1, a1, b2, a2), ob))
    assert abs(abs(np.roots(LN.coefficients(24000)[3])).max() - 0.99007) < 1e-5      # why a truncated warm-up would need ~2000 samples


def test_calibration_tones():
    t = np.arange(240000) / 24000.0
    _, st = LN.normalize(np.sin(2 * np.pi * 997 * t).astype(np.float32), -16.0)
    assert abs(st["L"][0] - (-2.984)) < 0.01 and st["n_blocks"][0] == 97 and st["peak"][0] == 1.0
    t = np.arange(480000) / 48000.0
    _, st = LN.normalize(np.sin(2 * np.pi * 997 * t).astype(np.float32), -16.0, rates=48000)
    assert abs(st["L"][0] - (-3.01)) < 0.1


def test_the_state_space_tables_reproduce_the_filter():
    """A^H, h_i = C A^i and M of `rate_row` against a serial run of `step`: what the kernels rely on"""
    for fs in (8000, 22050, 48000):
        H = fs // 10
        row = LN.rate_row(fs)
        assert row.shape == (LN.ROW,) and row[0] == H and row[1] == LN.chunk(H) == (-(-H // 64) | 1) and np.array_equal(row[2:12], LN._k10(fs))
        k = row[2:12]
        s0 = np.array([0.3, -0.2, 0.1, 0.05])
        s, ys = list(s0), []
        for _ in range(H):
            ys.append(LN.step(k, 0.0, s))
        AH = row[16:32].reshape(4, 4)
        assert np.abs(AH @ s0 - np.array(s)).max() < 1e-12
        tri = row[32:42]
        M = np.zeros((4, 4))
        M[np.triu_indices(4)] = tri
        M = M + M.T - np.diag(np.diag(M))
        assert abs(s0 @ M @ s0 - np.dot(ys, ys)) < 1e-12 * max(1.0, np.dot(ys, ys))
        c = int(row[1])
        P = row[48:].reshape(64, 4, 4)
        big = np.abs(P).max()                      # the high-pass's two poles nearly coincide: entries of A^m reach the tens
        assert np.array_equal(P[0], np.eye(4)) and np.abs(P[2] - P[1] @ P[1]).max() < 1e-13 * big
        assert np.abs(P[63] - np.linalg.matrix_power(P[1], 63)).max() < 1e-11 * big
        s = list(s0)
        for _ in range(c):
            LN.step(k, 0.0, s)
        assert np.abs(P[1] @ s0 - np.array(s)).max() < 1e-13 * big


# ---- 2. the twin against the oracle ---------------------------------------------------------------------------------------------------
def _cases():
    sig = LC.signals()
    out = [(i, 24000) for i in range(len(sig)) if len(sig[i][1]) < 100000]      # (the longest one: on the device, tests/test_gpu_loudness.py)
    out += [(i, fs) for i, (name, x, _) in enumerate(sig) for fs in (8000, 22050, 48000) if len(x) < 15000 or name == "gap"]
    return out


def test_twin_and_oracle_agree_on_the_fixtures():
    sig = LC.signals()
    worst = 0.0
    for i, fs in _cases():
        name, x, target = sig[i]
        y, st = LN.normalize(x, target, rates=fs)
        o = LC.alone(i, fs)
        assert (st["n_blocks"][0], st["n_abs"][0], st["n_rel"][0], st["bound"][0]) == (o["n_blocks"], o["n_abs"], o["n_rel"], o["bound"]), (name, fs)
        assert st["peak"][0] == np.float32(o["peak"])
        if o["n_abs"] == 0:
            assert st["L"][0] == -math.inf and st["g32"][0] == 1.0 and y.tobytes() == x.tobytes()
            continue
        worst = max(worst, abs(st["L"][0] - o["L"]))
        assert abs(st["L"][0] - o["L"]) <= 1e-9, (name, fs, st, o)
        assert abs(float(st["g32"][0]) / o["g"] - 1.0) <= 2.0 ** -23
        assert y.tobytes() == (st["g32"][0] * x).tobytes()
    print(f"worst |L_twin - L_oracle|: {worst:.3e} LU")


def test_the_tile_route_reproduces_the_serial_filter():
    for fs, n in ((8000, 5000), (24000, 2400), (24000, 7201), (48000, 4799)):
        x = LC.enveloped(3, n) + np.float32(0.01)
        y = O.k_weight(x, fs)
        H = fs // 10
        want = [float(np.dot(y[j: j + H], y[j: j + H])) for j in range(0, n, H)]
        got = LN.sub_block_energies(x, fs)
        # the closed form cancels the carried state's response against the tile's own: the error scales with the segment's
        # largest tile, not with the tile (a quiet tile behind a loud one keeps ~1e-16 of the LOUD one's energy as error)
        assert got.shape == (len(want),) and np.abs(got - np.array(want)).max() < 1e-12 * max(want), (fs, n)


# ---- 3. the rules -----------------------------------------------------------------------------------------------------------------------
def test_short_segments_are_one_block_over_all_their_samples():
    for n in (1, 2399, 9599):                       # fewer than 4 complete sub-blocks at 24 kHz
        x = LC.enveloped(1, n) + np.float32(0.01)
        y = O.k_weight(x, 24000)
        z = LN.blocks(x, 24000)
        assert z.shape == (1,) and abs(z[0] / (np.dot(y, y) / n) - 1.0) < 1e-11
        assert len(O.segment_blocks(x, 24000)) == 1
    assert LN.blocks(LC.enveloped(1, 9600), 24000).shape == (1,) and LN.blocks(LC.enveloped(1, 12000), 24000).shape == (2,)
    assert LN.blocks(LC.enveloped(1, 11999), 24000).shape == (1,)      # the incomplete fifth sub-block does not count


def test_silence_has_no_loudness_and_gain_one():
    for x in (np.zeros(12000, np.float32), (1e-4 * np.random.default_rng(7).uniform(-1, 1, 12000)).astype(np.float32)):
        y, st = LN.normalize(x, -16.0)
        assert st["L"][0] == -math.inf and st["g32"][0] == 1.0 and st["n_abs"][0] == 0 and st["bound"][0] == LN.BOUND_NONE and y.tobytes() == x.tobytes()
    assert LN.gate(np.array([0.0, 0.0])) == (-math.inf, 2, 0, 0)


def test_each_of_the_three_gain_terms_binds():
    assert LN.gain(-20.0, 0.1, -16.0) == (np.float32(10 ** 0.2), LN.BOUND_TARGET)
    assert LN.gain(-60.0, 0.001, -10.0) == (np.float32(10 ** 1.5), LN.BOUND_CAP)
    g, b = LN.gain(-13.0, 1.0, -5.0)
    assert b == LN.BOUND_CEILING and g == np.float32(LN.CEILING) and abs(LN.CEILING - 0.8912509381337456) < 1e-15
    assert LN.gain(-20.0, 0.1, None) == (np.float32(1.0), LN.BOUND_NONE) and LN.gain(-math.inf, 0.0, -16.0) == (np.float32(1.0), LN.BOUND_NONE)
    names = [s[0] for s in LC.signals()]
    assert [LC.alone(names.index(n), 24000)["bound"] for n in ("sine", "faint", "bursts", "zeros")] == [0, 1, 2, -1]
    # under the ceiling the 16-bit conversion's multiplier is the plain 32767: ceil(peak) == 1
    i = names.index("bursts")
    y, st = LN.normalize(LC.signals()[i][1], -5.0)
    assert st["bound"][0] == LN.BOUND_CEILING and np.abs(y).max() <= np.float32(LN.CEILING) * np.float32(1.0 + 2.0 ** -23)


def test_a_group_pools_its_blocks_and_takes_one_gain():
    names = [s[0] for s in LC.signals()]
    idx = [names.index(n) for n in ("env4_24000", "env0_1", "silent", "env0_11999")]
    xs = [LC.signals()[i][1] for i in idx]
    off = LC.offsets([len(x) for x in xs])
    y, st = LN.normalize(np.concatenate(xs), -20.0, offsets=off, groups=[0, 4])
    o = LC.grouped(idx, [24000] * 4, -20.0)
    assert len(st) == 1 and (st["n_blocks"][0], st["n_abs"][0], st["n_rel"][0]) == (o["n_blocks"], o["n_abs"], o["n_rel"])
    assert st["n_blocks"][0] == sum(len(LC.blocks(i, 24000)) for i in idx)            # blocks never span sentences
    assert abs(st["L"][0] - o["L"]) <= 1e-9 and st["peak"][0] == max(np.abs(x).max() for x in xs)
    assert y.tobytes() == (st["g32"][0] * np.concatenate(xs)).tobytes()
    _, each = LN.normalize(np.concatenate(xs), -20.0, offsets=off)                    # without the table: every segment its own group
    assert len(each) == 4 and each["L"][2] == -math.inf and len(set(each["g32"].tolist())) == 4
    _, mixed = LN.normalize(np.concatenate(xs), [-20.0, None], offsets=off, groups=[0, 1, 4], rates=[24000, 8000, 8000, 48000])
    assert mixed["bound"][1] == LN.BOUND_NONE and mixed["g32"][1] == 1.0 and mixed["L"][1] > -70.0


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_rates_targets_and_tables_are_refused_on_the_host():
    for fs in (7990, 48010, 24005, 22051, 24000.0, "24000", None, True):
        with pytest.raises(ValueError, match="rate"):
            LN.check_rate(fs)
    assert [LN.check_rate(fs) for fs in (8000, 22050, 44100, 48000, np.int64(16000))] == [8000, 22050, 44100, 48000, 16000]
    for t in (-40.01, -4.99, 0, "loud", True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target"):
            LN.check_target(t)
    assert LN.check_target(None) is None and LN.check_target(-40) == -40.0 and LN.check_target(-5.0) == -5.0
    assert LN.per_row(None, 3) is None and LN.per_row([None, None], 2) is None and LN.per_row(-16, 2) == [-16.0, -16.0]
    with pytest.raises(ValueError, match="one loudness target per row"):
        LN.per_row([-16.0], 2)
    for kw, why in ((dict(offsets=[1, 10]), "ascend from 0"), (dict(offsets=[0, 5, 5, 10]), "empty"), (dict(offsets=[0, 7, 5, 10]), "ascend"),
                    (dict(offsets=[0, 9]), "cover"), (dict(offsets=[0]), "ascend"), (dict(offsets=[0, 5, 10], groups=[0, 1]), "group table"),
                    (dict(offsets=[0, 5, 10], groups=[0, 0, 2]), "group table"), (dict(offsets=[0, 5, 10], groups=[1, 2]), "group table"),
                    (dict(offsets=[0, 5, 10], rates=[24000]), "one rate per segment"), (dict(offsets=[0, 5, 10], targets=[-16.0] * 3), "one target per group"),
                    (dict(offsets=[0, 5, 10], rates=[24000, 100]), "rate"), (dict(targets=-3.0), "target")):
        with pytest.raises(ValueError, match=why):
            LN.tables(10, **kw)
    with pytest.raises(ValueError, match="2\\^31"):
        LN.tables((1 << 31) - 4096)
    with pytest.raises(ValueError, match="65535"):
        LN.tables(65536, offsets=np.arange(65537))
    off, grp, rates, tg = LN.tables(10, offsets=[0, 4, 10], targets=[None, -16])
    assert grp.tolist() == [0, 1, 2] and rates == [24000, 24000] and tg == [None, -16.0] and off.dtype == np.int64 and grp.dtype == np.int32


def test_library_symbols_and_refusals_before_any_launch():
    """the C entry point checks every host table first: these calls fail without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    with open(_lib.HERE + "/../include/chattts_amd.h") as f:
        header = f.read()
    for name in ("ctts_loudness_normalize_ragged", "ctts_loudness_normalize_ragged_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "loudness.hip" in build.SOURCES and lib.ctts_version() == 1
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    off = i64([0, 2400, 12000])
    assert lib.ctts_loudness_normalize_ragged_scratch_bytes(vp(off), 2) == (12000 // 800 + 2 + 1) * LN.REC * 8 + 16
    assert lib.ctts_loudness_normalize_ragged_scratch_bytes(vp(i64([0, 5, 5])), 2) == 0 and b"empty" in lib.ctts_last_error()
    assert lib.ctts_loudness_normalize_ragged_scratch_bytes(vp(i64([0, (1 << 31) - 4096])), 1) == 0 and b"2^31" in lib.ctts_last_error()
    coef, _ = LN.coef_table([24000, 8000])
    fake = 4096                       # never dereferenced: every call below is refused on its host arguments

    def call(off=(0, 2400, 12000), rate=(1, 0), grp=(0, 1, 2), target=(-16.0, math.nan), coef=coef, x=fake, y=fake, scratch=fake, sb=1 << 20,
             null=None, n_seg=None):
        o, r, g, t = i64(off), np.asarray(rate, np.int32), np.asarray(grp, np.int32), np.asarray(target, np.float64)
        p = {k: (None if k == null else fake) for k in ("off", "rate", "coef", "grp", "target", "stats")}
        rc = lib.ctts_loudness_normalize_ragged(None if null == "x" else x, y, p["off"], vp(o), len(o) - 1 if n_seg is None else n_seg, p["rate"], vp(r),
                                                p["coef"], vp(coef), coef.shape[0], p["grp"], vp(g), len(g) - 1, p["target"], vp(t), p["stats"],
                                                scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    bad_h, bad_c, frac_h = coef.copy(), coef.copy(), coef.copy()
    bad_h[0, 0], bad_c[1, 1], frac_h[1, 0] = 700.0, 38.0, 2400.5
    for kw, why in ((dict(null="x"), "null"), (dict(null="stats"), "null"), (dict(null="grp"), "null"), (dict(null="target"), "null"),
                    (dict(off=(1, 2400, 12000)), "must be 0"), (dict(off=(0, 2400, 2400)), "empty"), (dict(off=(0, 2400, 100)), "ascend"),
                    (dict(n_seg=0), "1 <= n_seg <= 65535"), (dict(n_seg=65536), "1 <= n_seg <= 65535"),
                    (dict(off=(0, 2400, (1 << 31) - 4096)), "2^31 - 4096"), (dict(rate=(2, 0)), "outside the table"), (dict(rate=(0, -1)), "outside the table"),
                    (dict(coef=bad_h), "sub-block"), (dict(coef=frac_h), "sub-block"), (dict(coef=bad_c), "chunk"),
                    (dict(grp=(1, 2)), "from 0 to n_seg"), (dict(grp=(0, 1)), "from 0 to n_seg"), (dict(grp=(0, 0, 2)), "group 0 is empty"),
                    (dict(target=(-41.0, -16.0)), "-40 .. -5"), (dict(target=(-16.0, -4.0)), "-40 .. -5"), (dict(target=(math.inf, -16.0)), "-40 .. -5"),
                    (dict(sb=100), "scratch"), (dict(scratch=None), "scratch"), (dict(x=4100), "16-byte aligned"), (dict(y=4104), "16-byte aligned"),
                    (dict(y=4096 + 160), "overlap")):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_loudness_normalize_ragged" in msg and why in msg, (kw, msg)


def test_streams_are_refused():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["hello"], stream=True, loudness=-16.0)
    with pytest.raises(ValueError, match="-40 .. -5"):
        chat.infer(["hello"], loudness=-3.0)
    with pytest.raises(ValueError, match="one loudness target"):
        chat.infer(["a", "b"], split_text=True, loudness=[-16.0, -20.0])
    with pytest.raises(ValueError, match="rate"):
        chat.infer(["hello"], sample_rate=11025, loudness=-16.0)
    lock = threading.Lock()
    b = SpeechBatcher(_FakeChat(), 2, lock, make_pool=lambda: _Pool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream("a#8", _Params(), loudness=-16.0)
        with pytest.raises(ValueError, match="-40 .. -5"):
            b.submit_stream("a#8", _Params(), loudness=-50.0)
        for bad in (-41.0, -4.0, "x", True):
            with pytest.raises(ValueError):
                b.submit("a#8", _Params(), loudness=bad)
        with pytest.raises(ValueError, match="rate"):
            b.submit("a#8", _Params(), loudness=-16.0, sample_rate=11025)
    finally:
        b.close()


# ---- 5. Chat: the argument reaches the decode, and nothing does without it -------------------------------------------------------------
class _Codec:
    """a CodecEngine without a device: what it is called with is recorded"""
    SAMPLE_RATE = 24000

    def __init__(self):
        self.calls = []

    def decode_ragged(self, rows, **kw):
        self.calls.append(("decode_ragged", kw))
        lens = [4 * int(r.shape[0]) for r in rows]
        return torch.arange(sum(lens), dtype=torch.float32) / 100, LC.offsets(lens)

    def decode_to_wavs(self, rows, **kw):
        self.calls.append(("decode_to_wavs", kw))
        return torch.ones((len(rows), 8))

    def loudness_normalize(self, wav, target, **kw):
        self.calls.append(("loudness_normalize", target, {k: (v if k != "out" else v is wav) for k, v in kw.items()}))
        return wav

    def float_to_int16_groups(self, wav, off, grp, **kw):
        self.calls.append(("float_to_int16_groups", list(grp)))
        return wav, [0]

    def unpack_groups(self, blob, starts, encs=None):
        return [np.zeros(3, np.int16)]

    def to_host(self, t):
        return t.numpy()


def _chat():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    chat.codec, chat.has_loaded = _Codec(), lambda *a, **k: True
    chat.device = torch.device("cpu")
    chat.context, chat.logger = types.SimpleNamespace(set=lambda v: None), logging.getLogger("test_loudness_host")
    return chat


def test_chat_decode_calls_pass_the_target_on_and_nothing_when_it_is_none():
    chat = _chat()
    rows = [torch.zeros(3, 768), torch.zeros(2, 768)]
    chat.decode_to_wavs(rows, ragged=True, loudness=[-16, None])
    chat.decode_to_wavs(rows, ragged=True)
    chat.decode_to_wavs(rows, ragged=True, loudness=[None, None])
    chat.decode_to_wavs(rows, loudness=-23.0, sample_rate=8000)
    chat.decode_to_wavs(rows)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": None, "loudness": [-16.0, None]}), ("decode_ragged", {"sample_rate": None}),
                                ("decode_ragged", {"sample_rate": None}), ("decode_to_wavs", {"pad_to": None, "sample_rate": 8000, "loudness": -23.0}),
                                ("decode_to_wavs", {"pad_to": None, "sample_rate": None})]
    with pytest.raises(ValueError, match="-40 .. -5"):
        chat.decode_to_wavs(rows, loudness=-60.0)
    chat.codec.calls.clear()
    groups = [[torch.zeros(3, 768), torch.zeros(2, 768)]]
    chat.decode_split_to_pcm16(groups, loudness=-19.0, sample_rate=8000)
    chat.decode_split_to_pcm16(groups)
    assert chat.codec.calls == [("decode_ragged", {"sample_rate": 8000}),
                                ("loudness_normalize", -19.0, {"offsets": pytest.approx([0, 12, 20]), "groups": pytest.approx([0, 2]), "out": True, "rates": [8000, 8000]}),
                                ("float_to_int16_groups", [0, 2]), ("decode_ragged", {"sample_rate": None}), ("float_to_int16_groups", [0, 2])]
    with pytest.raises(ValueError, match="one loudness target per request"):
        chat.decode_split_to_pcm16(groups, loudness=[-19.0, -20.0])


def test_chat_infer_passes_the_target_on_and_nothing_when_it_is_none():
    chat = _chat()
    seen = []

    def fake_infer(text, *a, **kw):
        seen.append(kw)
        yield [np.full(5, 0.5, np.float32) for _ in text]
    chat._infer = fake_infer
    kw = dict(skip_refine_text=True, split_text=False)
    chat.infer(["a", "b"], loudness=[-16.0, None], **kw)
    chat.infer(["a", "b"], **kw)
    chat.infer(["a", "b"], loudness=None, pcm16=True, **kw)
    assert seen[0]["loudness"] == [-16.0, None] and "loudness" not in seen[1] and "loudness" not in seen[2]
    assert {k: v for k, v in seen[0].items() if k != "loudness"} == seen[1]
    # a split request that is concatenated on the host: the decode stays untouched, ONE group over the sentences afterwards
    seen.clear()
    out = chat.infer("a. b. c.", loudness=-16.0, skip_refine_text=True)
    assert "loudness" not in seen[0] and len(out) == 1 and len(out[0]) == 15
    call = chat.codec.calls[-1]
    assert call[0] == "loudness_normalize" and call[1] == -16.0 and list(call[2]["groups"]) == [0, 3] and list(call[2]["offsets"]) == [0, 5, 10, 15]
    assert call[2]["rates"] == 24000


# ---- 6. the batcher ---------------------------------------------------------------------------------------------------------------------
class _LoudChat(_FakeChat):
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


def test_requests_with_mixed_targets_share_one_decode():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), loudness=t) for c, t in (("a", -16), ("b", -23.0), ("c", None), ("d", -16.0))]
        res = [f.result(timeout=10) for f in futs]
        b.submit("e#8", _Params()).result(timeout=10)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.pcm_kw == [{"loudness": [-16.0, -23.0, None, -16.0]}, {}] and b.decode_calls == 2
    assert [int(r[0]) for r in res] == [ord(c) for c in "abcd"]


def test_batcher_passes_the_target_on_every_completion_path_and_nothing_without_it():
    lock, pools = threading.Lock(), {}
    chat = _LoudChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)))      # every request alone: `finish`
    try:
        b.submit("a#8", _Params(), loudness=-16).result(timeout=10)
        b.submit("b#8", _Params()).result(timeout=10)
        b.submit("d#8", _Params(), loudness=-20.0, sample_rate=8000, speed=1.25).result(timeout=10)
        pcm = b.submit("k#8\nl#8", _Params(spk_smp="V"), split_text=True, loudness=-23.0).result(timeout=30)
        b.submit("m#8\nn#8", _Params(spk_smp="V"), split_text=True).result(timeout=30)
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.wav_kw == [{"loudness": -16.0}, {}, {"sample_rate": 8000, "speed": 1.25, "loudness": -20.0}]
    assert chat.split_kw == [{"loudness": [-23.0]}, {}] and _spell(pcm) == [("k", 8), ("l", 8)]


# ---- 7. the endpoint ------------------------------------------------------------------------------------------------------------------
def _app(batcher=None, **kw):
    from chattts_amd import server
    log, catch = logging.getLogger(f"test_loudness_host.{id(kw)}"), _Catch()
    log.addHandler(catch)
    chat = _EndpointChat()
    return server.create_app(chat, {"default": "SPK-D"}, batcher=batcher, logger=log, **kw), chat, catch


def test_endpoint_loudness():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app()                          # off: an unknown key -- the warning, and today's call argument for argument
    with TestClient(app) as c:
        r0 = c.post("/v1/audio/speech", json=body)
        r = c.post("/v1/audio/speech", json={**body, "loudness": -16})
        assert r.status_code == 200 and r.content == r0.content and sorted(chat.calls[-1][2]) == sorted(chat.calls[-2][2]) and "loudness" not in chat.calls[-1][2]
        assert catch.msgs == ["ignoring unsupported parameters: ['loudness']"]
        assert c.post("/v1/audio/speech", json={**body, "loudness": "loud"}).status_code == 200      # ignored, whatever it holds
        assert "loudness" not in c.get("/health").json()

    app, chat, catch = _app(loudness=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "loudness": -16})
        assert r.status_code == 200 and chat.calls[-1][2]["loudness"] == -16.0 and chat.calls[-1][1] is False
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and "loudness" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "loudness": None}).status_code == 200 and "loudness" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "stream": True}).status_code == 200 and chat.calls[-1][1] is True
        n = len(chat.calls)
        for bad in (-41, -4.5, 0, "loud", True, [-16]):
            r = c.post("/v1/audio/speech", json={**body, "loudness": bad})
            assert r.status_code == 400 and "-40 .. -5" in r.text, bad
        r = c.post("/v1/audio/speech", json={**body, "loudness": -16, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and len(chat.calls) == n
        assert not catch.msgs and c.get("/health").json()["loudness"] is True

    app, chat, catch = _app(loudness=True, sample_rates=(8000, 11025, 24000), g711=True, speed=True, flac=True)      # composes with the other options
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "loudness": -20.5, "speed": 0.8, "sample_rate": 8000, "encoding": "ulaw"})
        kw = chat.calls[-1][2]
        assert r.status_code == 200 and (kw["loudness"], kw["speed"], kw["sample_rate"], kw["encoding"]) == (-20.5, 0.8, 8000, "ulaw")
        r = c.post("/v1/audio/speech", json={**body, "response_format": "flac", "loudness": -16})
        assert r.status_code == 200 and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["loudness"] == -16.0
        assert c.post("/v1/audio/speech", json={**body, "loudness": -16, "sample_rate": 11025}).status_code == 400      # no multiple of 10 Hz

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, loudness=True)
    with TestClient(app) as c:
        assert c.post("/v1/audio/speech", json={**body, "loudness": -16}).status_code == 200 and bat.calls[-1][2] == {"loudness": -16.0}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

"""`ctts_float_to_int16_groups` on the GPU: one peak per group of packed segments, the silent samples dropped and the rest compacted on
the device, against NumPy byte for byte (kept counts included); and the refusals of the entry point.  `pytest -m gpu`."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib  # noqa: E402
from chattts_amd import engine as E  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402

DEV = torch.device("cuda:0")
f32 = np.float32
LENS = [1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049]      # on and beside every vector (8) and workgroup (2048) edge, and wave-sized runs
THR = 1e-5


def _codec():
    return types.SimpleNamespace(lib=_lib.lib())     # float_to_int16_groups needs the library only, not a loaded decoder


def _waves(lens, rs):
    """segments of audio-like samples with silence where the strip bites: exact zeros, |x| below and exactly AT the threshold (kept is
    |x| > thr, strictly), alone and in runs"""
    out = []
    for n in lens:
        w = (rs.standard_normal(n) * 0.3).astype(f32)
        quiet = rs.rand(n) < 0.15
        w[quiet] = rs.choice(np.array([0.0, 1e-6, -9e-6, 1e-5, -1e-5], f32), size=int(quiet.sum()))
        if n >= 255:
            a = int(rs.randint(0, n - 100))
            w[a: a + int(rs.randint(1, 100))] = 0.0
        out.append(w)
    return out


def _reference(segs, grp, thr, product):
    """the host lines of Chat.infer(split_text=True, pcm16=True): strip every sentence, concatenate, ONE float_to_int16"""
    res = []
    for g in range(len(grp) - 1):
        ws = segs[grp[g]: grp[g + 1]]
        kept = np.concatenate([w[np.abs(w) > f32(thr)] for w in ws]) if thr is not None else np.concatenate(ws)
        whole = np.concatenate(ws)
        if kept.size and np.abs(kept).max() != np.abs(whole).max():      # (only if the peak itself were stripped: it never is)
            raise AssertionError("test data: the group's peak must survive the strip")
        res.append(float_to_int16(kept, product))
    return res


def _run(segs, grp, thr, product):
    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([len(w) for w in segs], out=off[1:])
    wav = torch.from_numpy(np.concatenate(segs)).to(DEV)
    blob, starts = E.CodecEngine.float_to_int16_groups(_codec(), wav, off, np.asarray(grp, np.int32), product=product, keep_thr=thr)
    torch.cuda.synchronize()
    host = blob.cpu().numpy()
    n_grp = len(grp) - 1
    n_kept = host[: 8 * n_grp].view(np.int64).copy()
    return E.CodecEngine.unpack_groups(host, starts), n_kept, starts, off


def _mixed_case():
    """groups of 1, 2 and 5 segments; every length of LENS three times, so that group and segment boundaries fall at every residue; then
    the special groups"""
    rs = np.random.RandomState(31)
    lens = LENS + LENS[3:] + LENS[:3] + LENS[7:] + LENS[:7]
    sizes = [1, 2, 5, 2, 5, 1, 5, 1, 2, 1, 5]
    assert sum(sizes) == len(lens) == 30
    segs = _waves(lens, rs)
    names = {}
    def add(name, ws):
        names[name] = len(sizes)
        segs.extend(ws)
        sizes.append(len(ws))
    a, b, c = _waves([257, 2049, 9], rs)
    b[:] = f32(1e-6) * np.sign(b)                         # a segment that is stripped entirely, between two that are not
    add("segment_stripped", [a, b, c])
    add("group_stripped", [np.full(n, 5e-6, f32) for n in (7, 2048, 1)])     # count 0, peak > 0
    add("all_zero", [np.zeros(n, f32) for n in (9, 256)])
    ws = _waves([2047, 8, 255], rs)
    ws[2][254] = f32(-3.7)                                # the group's peak is the last sample of its last segment: ceil -> 4
    add("peak_last", ws)
    add("one_sample", [np.array([0.25], f32)])
    grp = np.zeros(len(sizes) + 1, np.int32)
    np.cumsum(sizes, out=grp[1:])
    return segs, grp, names


@pytest.fixture(scope="module")
def mixed():
    return _mixed_case()


@pytest.mark.parametrize("product", ["f64", "f32"])
@pytest.mark.parametrize("thr", [THR, None])
def test_groups_equal_numpy_byte_for_byte(mixed, product, thr):
    segs, grp, names = mixed
    got, n_kept, starts, off = _run(segs, grp, thr, product)
    want = _reference(segs, grp, thr, product)
    assert list(starts[:-1] % 8) == [0] * (len(grp) - 1)
    for g, (a, b) in enumerate(zip(got, want)):
        assert int(n_kept[g]) == b.size, (g, int(n_kept[g]), b.size)
        assert a.dtype == np.int16 and a.tobytes() == b.tobytes(), (g, a.size, b.size)
    g = names["group_stripped"]
    assert int(n_kept[g]) == (0 if thr is not None else 7 + 2048 + 1)
    g = names["all_zero"]
    assert int(n_kept[g]) == (0 if thr is not None else 9 + 256) and not got[g].any()
    g = names["peak_last"]
    assert np.abs(got[g]).max() == int(3.7 * (32767 // 4))       # scaled by the peak of the LAST segment
    if thr is not None:
        assert sum(int(n) for n in n_kept) < int(off[-1])          # the strip did bite
    else:
        assert [int(n) for n in n_kept] == [int(off[grp[g + 1]] - off[grp[g]]) for g in range(len(grp) - 1)]


def test_one_group_is_float_to_int16_of_the_concatenation():
    """n_grp = 1 over 5 segments with keep_thr < 0: a plain concatenation under one peak"""
    rs = np.random.RandomState(5)
    segs = _waves([2049, 1, 256, 7, 2047], rs)
    got, n_kept, _, off = _run(segs, [0, 5], None, "f64")
    assert int(n_kept[0]) == int(off[-1]) and got[0].tobytes() == float_to_int16(np.concatenate(segs)).tobytes()


def test_a_group_of_more_than_256_tiles():
    """the per-group scan walks its tile counts 256 at a time: a group of 257 tiles + 9 samples beside a short one"""
    rs = np.random.RandomState(6)
    segs = _waves([2048 * 200 + 1, 2048 * 57 + 8, 255], rs)
    grp = [0, 2, 3]
    got, n_kept, _, _ = _run(segs, grp, THR, "f64")
    for g, b in enumerate(_reference(segs, grp, THR, "f64")):
        assert int(n_kept[g]) == b.size and got[g].tobytes() == b.tobytes(), g


def test_refusals_launch_nothing():
    lib = _lib.lib()
    n = 64
    wav = torch.full((n,), 0.5, dtype=torch.float32, device=DEV)
    pcm = torch.full((n + 16,), 0x7777, dtype=torch.int16, device=DEV)
    cnt = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    peak = torch.zeros((4,), dtype=torch.int32, device=DEV)
    work = torch.zeros((64,), dtype=torch.uint8, device=DEV)

    def call(off, grp, n_grp=None, peak_p=None, cnt_p=None, n_seg=None):
        off, grp = np.asarray(off, np.int64), np.asarray(grp, np.int32)
        off_d, grp_d = torch.from_numpy(off).to(DEV), torch.from_numpy(grp).to(DEV)
        rc = lib.ctts_float_to_int16_groups(wav.data_ptr(), pcm.data_ptr(), cnt.data_ptr() if cnt_p is None else cnt_p, off_d.data_ptr(),
                                            off.ctypes.data_as(C.c_void_p), len(off) - 1 if n_seg is None else n_seg, grp_d.data_ptr(),
                                            grp.ctypes.data_as(C.c_void_p), len(grp) - 1 if n_grp is None else n_grp, 0, 1e-5,
                                            peak.data_ptr() if peak_p is None else peak_p, work.data_ptr(), work.numel(), None)
        torch.cuda.synchronize()
        return rc, (lib.ctts_last_error() or b"").decode()

    good_off, good_grp = [0, 16, 40, 64], [0, 1, 3]
    bad = {
        "n_grp < 1": call(good_off, [0], n_grp=0),
        "empty group": call(good_off, [0, 1, 1, 3]),
        "group table past n_seg": call(good_off, [0, 1, 2]),
        "non-ascending offsets": call([0, 40, 16, 64], good_grp),
        "empty segment": call([0, 16, 16, 64], good_grp),
        "null peak": call(good_off, good_grp, peak_p=0),
        "null count": call(good_off, good_grp, cnt_p=0),
    }
    for what, (rc, msg) in bad.items():
        assert rc != 0 and "ctts_float_to_int16_groups" in msg, (what, rc, msg)
    assert (pcm.cpu().numpy() == 0x7777).all() and (cnt.cpu().numpy() == -1).all()       # nothing ran
    assert lib.ctts_float_to_int16_groups_scratch_bytes(np.asarray(good_off, np.int64).ctypes.data_as(C.c_void_p), 3,
                                                        np.asarray([0, 1, 1, 3], np.int32).ctypes.data_as(C.c_void_p), 3) == 0
    rc, msg = call(good_off, good_grp)                                                   # the same buffers, accepted
    assert rc == 0, msg
    assert cnt.cpu().numpy()[:2].tolist() == [16, 48] and (pcm.cpu().numpy()[:64] == int(0.5 * 32767)).all()

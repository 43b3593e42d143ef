"""ctts_flac_encode_ranges on the GPU against the NumPy twin, byte for byte, and through the independent decoder: every length and signal
of tests/flac_cases.py, several ranges in one call (different rates, nonzero starts, a skipped range, device counts below the capacity)
with a canary behind the bytes used, and fed from float_to_int16_groups with and without stripping.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E, flac  # noqa: E402
from tests import flac_cases as FC  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 0xA5


class _Codec:
    """the two members `CodecEngine.flac_encode` and `float_to_int16_groups` use, without the decoder's weights"""
    flac_encode = E.CodecEngine.flac_encode
    float_to_int16_groups = E.CodecEngine.float_to_int16_groups
    float_to_int16_groups_flac = E.CodecEngine.float_to_int16_groups_flac
    unpack_groups = staticmethod(E.CodecEngine.unpack_groups)
    to_host = E.CodecEngine.to_host
    _copy_out = E.CodecEngine._copy_out

    def __init__(self):
        self.lib, self.device = _lib.lib(), DEV


@pytest.fixture(scope="module")
def codec():
    return _Codec()


def _raw(pcm_d, rows, counts_d=None, slack=64):
    """the C entry over (start, n, rate, count_idx) rows with a canary-filled `out` -> (out bytes, slot offsets + total, lengths)"""
    lib = _lib.lib()
    tab = np.zeros(len(rows), _lib.FLAC_RANGE)
    slots = 0
    for i, (start, n, rate, ci) in enumerate(rows):
        tab[i] = (start, n, rate, ci, slots)
        slots += (n + 4095) // 4096 if rate else 0
    sizes = (C.c_int64 * 3)()
    assert lib.ctts_flac_encode_sizes(tab.ctypes.data_as(C.c_void_p), len(rows), sizes) == 0, lib.ctts_last_error()
    assert sizes[0] == slots and sizes[1] == sum(2 * n + 16 * ((n + 4095) // 4096) for _, n, rate, _ in rows if rate)
    out_d = torch.full(((int(sizes[1]) + 15) // 16 * 16 + slack,), CANARY, dtype=torch.uint8, device=DEV)
    work_d = torch.zeros((int(sizes[2]),), dtype=torch.uint8, device=DEV)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    rc = lib.ctts_flac_encode_ranges(pcm_d.data_ptr(), _lib.ptr(counts_d), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(rows),
                                     out_d.data_ptr(), out_d.numel() - slack, work_d.data_ptr(), work_d.numel(),
                                     torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, lib.ctts_last_error()
    torch.cuda.synchronize()
    meta = work_d.cpu().numpy()[: 8 * (slots + 1 + len(rows))].view(np.int64)
    return out_d.cpu().numpy(), meta[: slots + 1], meta[slots + 1:]


@pytest.mark.parametrize("name", FC.SIGNALS)
@pytest.mark.parametrize("n", FC.LENGTHS)
def test_device_bytes_are_the_twins(codec, n, name):
    x, rate, body, lens = FC.reference(name, n)
    pcm_d = torch.from_numpy(np.concatenate([x, np.zeros((-n) % 8 + 8, np.int16)])).to(DEV)
    (got, got_lens, got_n), = codec.flac_encode(pcm_d, [(0, n, rate)], info=True)
    assert got_n == n and got_lens.tolist() == lens.tolist()
    assert got.dtype == np.uint8 and got.tobytes() == body
    file = flac.file_bytes(got, got_lens, got_n, rate)
    assert file.size <= flac.bound(n)
    y, r, facts = FC.decoded(file)
    assert r == rate and np.array_equal(y, x)
    if name == "noise":
        assert all(k == "VERBATIM" for k, b in zip(facts["kinds"], facts["blocks"]) if b >= 16)


def test_several_ranges_in_one_call_and_the_canary():
    """six ranges: different rates (table codes and the 16-bit form), starts that are no multiples of 16, a skipped range, an empty one,
    two whose lengths come from device counts below the capacity (one of them 0) -- the frames lie back to back in range order, the
    lengths are the twin's, and no byte behind the total is written"""
    sig = [FC.signal("ar2", 9000), FC.signal("chirp", 4097), FC.signal("noise", 300), FC.signal("small_noise", 5000),
           FC.signal("ramp", 4096), FC.signal("spikes", 100)]
    rows, parts, pos = [], [], 8
    rates = [24000, 11025, 0, 8000, 44100, 16000]
    count_idx = [-1, 3, -1, 0, -1, 2]
    counts = np.array([4097, -5, 0, 4000], np.int64)             # range 1 -> 4000 of its 4097, range 3 -> 4097 of 5000, range 5 -> 0
    for x, rate, ci in zip(sig, rates, count_idx):
        rows.append((pos, len(x), rate, ci))
        parts.append((pos, x))
        pos = (pos + len(x) + 7) // 8 * 8 + 8
    rows.insert(3, (rows[2][0] + 304, 0, 22050, -1))             # an empty range among them
    pcm = np.full(pos, 77, np.int16)
    for p, x in parts:
        pcm[p: p + len(x)] = x
    out, offs, n_act = _raw(torch.from_numpy(pcm).to(DEV), rows, torch.from_numpy(counts).to(DEV))
    want_n = [9000, 4000, 0, 0, 4097, 4096, 0]
    assert n_act.tolist() == want_n
    want, want_lens = b"", []
    for (start, n, rate, ci), m in zip(rows, want_n):
        if rate:
            body, lens = flac.frames(pcm[start: start + m], rate)
            want += body
            want_lens += lens.tolist() + [0] * ((n + 4095) // 4096 - len(lens))     # the slots the capacity reserved and the count left empty
    assert np.diff(offs).tolist() == want_lens and int(offs[-1]) == len(want)
    assert out[: len(want)].tobytes() == want
    assert (out[len(want):] == CANARY).all()


@pytest.mark.parametrize("keep_thr", [None, 1e-5])
def test_fed_from_the_grouped_conversion(codec, keep_thr):
    """float_to_int16_groups' slots and its device count header go straight into the encoder: group g's file holds exactly the samples
    the conversion hands out for it, stripped or not; a group without the flag comes back as before"""
    rng = np.random.default_rng(11)
    segs = [5000, 3000, 4096, 700, 9000]
    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([(s + 7) // 8 * 8 for s in segs], out=off[1:])
    wav = np.zeros(int(off[-1]), np.float32)
    for k, s in enumerate(segs):
        w = (np.sin(np.arange(s) * 0.05 * (k + 1)) * 0.4 + rng.standard_normal(s) * 0.01).astype(np.float32)
        w[rng.random(s) < 0.3] = 0.0                              # what the strip removes
        wav[int(off[k]): int(off[k]) + s] = w
    grp = np.array([0, 2, 3, 5], np.int32)
    wav_d = torch.from_numpy(wav).to(DEV)
    blob, starts = codec.float_to_int16_groups(wav_d, off, grp, keep_thr=keep_thr)
    plain = E.CodecEngine.unpack_groups(codec.to_host(blob), starts)
    rates = [24000, None, 8000]
    files = codec.float_to_int16_groups_flac(wav_d, off, grp, rates, keep_thr=keep_thr)
    assert len(files) == 3 and files[1].dtype == np.int16 and np.array_equal(files[1], plain[1])
    for g in (0, 2):
        assert files[g].dtype == np.uint8 and files[g].size <= flac.bound(len(plain[g]))
        y, r, _ = FC.decoded(files[g])
        assert r == rates[g] and np.array_equal(y, plain[g]) and files[g].tobytes() == flac.encode(plain[g], rates[g])
    if keep_thr is not None:
        assert len(plain[0]) < segs[0] + segs[1]                  # something was stripped: the count came from the device

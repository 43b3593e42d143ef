"""g711_ranges_k on the GPU against the NumPy twin: every int16 value under both laws, ranges whose lengths sit on the edges of a thread's
16-sample group and of a workgroup's 4096-sample tile with a canary around them, 1024 ranges in one call, and refusals that reach no
launch.  (A range that starts beyond 2^31 bytes is not run here: the kernel's positions are 64-bit by reading, DESIGN.md says so.)
`pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E, g711  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 0xA5


def _call(pcm_d, out_d, rows, n_rng=None):
    """ctts_g711_encode_ranges over (start, n, law) rows -> rc"""
    lib = _lib.lib()
    tab = np.zeros(len(rows), _lib.G711_RANGE)
    for i, r in enumerate(rows):
        tab[i] = (*r, 0, 0)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    rc = lib.ctts_g711_encode_ranges(pcm_d.data_ptr(), out_d.data_ptr(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p),
                                     len(rows) if n_rng is None else n_rng, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return rc


def _check(pcm, rows, got):
    """every byte of a converted range is the twin's, every other byte is still the canary"""
    want = np.full(got.shape, CANARY, np.uint8)
    for start, n, law in rows:
        if law >= 0:
            want[start: start + n] = g711.encode(pcm[start: start + n], law)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def test_all_int16_values_under_both_laws():
    x = np.arange(-32768, 32768).astype(np.int16)
    pcm = np.concatenate([x, x[::-1]])
    pcm_d = torch.from_numpy(pcm).to(DEV)
    out_d = torch.full((pcm.size,), CANARY, dtype=torch.uint8, device=DEV)
    assert _call(pcm_d, out_d, [(0, 65536, 0), (65536, 65536, 1)]) == 0, _lib.lib().ctts_last_error()
    got = out_d.cpu().numpy()
    assert np.array_equal(got[:65536], g711.encode(x, 0)) and np.array_equal(got[65536:], g711.encode(x[::-1], 1))


@pytest.mark.parametrize("shift", [0, 8])
def test_ranges_at_group_and_tile_edges_leave_the_canary(shift):
    """lengths 1 .. 70001 at starts that are multiples of 8 (`shift` 8: most of them no multiples of 16, the store's weaker alignment), a
    gap behind each, a skipped range and an empty one among them"""
    lens = [1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, 70001]
    rows, pos = [], shift
    for i, n in enumerate(lens):
        rows.append((pos, n, i % 2))
        pos = (pos + n + 7) // 8 * 8 + (8 if i % 3 else 24)
    rows.insert(4, (rows[3][0] + rows[3][1] + 7 & ~7, 0, 1))          # an empty range
    skip = (pos, 5000, -1)
    rows.append(skip)
    pos += 5000 + 11
    rows.append(((pos + 7) // 8 * 8, 33, 1))
    total = rows[-1][0] + 33 + 100
    pcm = np.random.default_rng(7 + shift).integers(-32768, 32768, total).astype(np.int16)
    pcm_d = torch.from_numpy(pcm).to(DEV)
    out_d = torch.full((total,), CANARY, dtype=torch.uint8, device=DEV)
    assert _call(pcm_d, out_d, rows) == 0, _lib.lib().ctts_last_error()
    _check(pcm, rows, out_d.cpu().numpy())


def test_1024_ranges_of_mixed_laws_and_lengths_in_one_call():
    rng = np.random.default_rng(19)
    lens = rng.integers(0, 300, 1024)
    lens[[5, 500, 1023]] = [4096, 9000, 4097]
    laws = rng.integers(-1, 2, 1024)
    rows, pos = [], 0
    for n, law in zip(lens, laws):
        rows.append((pos, int(n), int(law)))
        pos = (pos + int(n) + 7) // 8 * 8 + 8 * int(rng.integers(0, 3))
    pcm = rng.integers(-32768, 32768, pos + 64).astype(np.int16)
    pcm_d = torch.from_numpy(pcm).to(DEV)
    out_d = torch.full((pcm.size,), CANARY, dtype=torch.uint8, device=DEV)
    assert _call(pcm_d, out_d, rows) == 0, _lib.lib().ctts_last_error()
    _check(pcm, rows, out_d.cpu().numpy())


def test_refusals_reach_no_launch():
    pcm_d = torch.zeros((4096,), dtype=torch.int16, device=DEV)
    out_d = torch.full((4096,), CANARY, dtype=torch.uint8, device=DEV)
    lib = _lib.lib()
    for rows, kw, msg in (([(4, 100, 0)], {}, b"multiples of 8"), ([(0, -1, 0)], {}, b"negative"), ([(0, 100, 2)], {}, b"law"),
                          ([(0, 100, 0), (96, 8, 1)], {}, b"overlapping"), ([(512, 8, 0), (0, 8, 0)], {}, b"descending"),
                          ([(0, 100, 0)], {"n_rng": 0}, b"n_rng"), ([(8 * i, 8, 0) for i in range(1025)], {}, b"1024")):
        assert _call(pcm_d, out_d, rows, **kw) != 0 and msg in lib.ctts_last_error(), (rows[:2], lib.ctts_last_error())
    assert _call(pcm_d, pcm_d.view(torch.uint8), [(0, 100, 0)]) != 0 and b"aliases" in lib.ctts_last_error()
    assert bool((out_d == CANARY).all()) and bool((pcm_d == 0).all())


def test_engine_wrapper_equals_the_twin(weights):
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV)
    pcm = np.random.default_rng(2).integers(-32768, 32768, 5003).astype(np.int16)
    pcm_d = torch.from_numpy(pcm).to(DEV)
    got = codec.g711_encode(pcm_d, [(0, 5003, "alaw")])
    assert got.dtype == torch.uint8 and got.numel() == 5008 and np.array_equal(codec.to_host(got)[:5003], g711.encode(pcm, "alaw"))
    out = torch.full((5008,), CANARY, dtype=torch.uint8, device=DEV)
    codec.g711_encode(pcm_d, [(0, 1000, "ulaw"), (1000, 3000, None), (4000, 1003, 1)], out=out)
    h = out.cpu().numpy()
    assert np.array_equal(h[:1000], g711.encode(pcm[:1000], 0)) and np.array_equal(h[4000:5003], g711.encode(pcm[4000:], 1))
    assert bool((h[1000:4000] == CANARY).all()) and bool((h[5003:] == CANARY).all())
    with pytest.raises(_lib.EngineError, match="multiples of 8"):
        codec.g711_encode(pcm_d, [(3, 10, 0)])
    with pytest.raises(ValueError):
        codec.g711_encode(pcm_d, [(0, 5004, 0)])
    with pytest.raises(ValueError):
        codec.g711_encode(pcm_d.float(), [(0, 8, 0)])

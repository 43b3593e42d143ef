"""ctts_adpcm_encode_ranges on the GPU against the NumPy twin, byte for byte: every signal and length of tests/adpcm_cases.py packed into
ONE call with mixed rates, a skipped range, device counts below the capacity (one that ends a block exactly, one that leaves a single
sample in the last block, one that is 0), 70 blocks followed by one block of the next range (a partly filled wave, a workgroup that
spans two ranges), canaries in front of, between and behind the byte spans, every range alone against the same range in the pack, the
per-range sample records, and the refusals.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, adpcm, engine as E  # noqa: E402
from tests import adpcm_cases as AC  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 0xA5
FRONT = 256                  # canary bytes in front of the output


class _Codec:
    """the members `CodecEngine.adpcm_encode` and the grouped conversion use, without the decoder's weights"""
    adpcm_encode = E.CodecEngine.adpcm_encode
    float_to_int16_groups = E.CodecEngine.float_to_int16_groups
    float_to_int16_groups_adpcm = E.CodecEngine.float_to_int16_groups_adpcm
    g711_encode = E.CodecEngine.g711_encode
    unpack_groups = staticmethod(E.CodecEngine.unpack_groups)
    to_host = E.CodecEngine.to_host
    _copy_out = E.CodecEngine._copy_out

    def __init__(self):
        self.lib, self.device = _lib.lib(), DEV


@pytest.fixture(scope="module")
def codec():
    return _Codec()


def _raw(pcm_d, rows, counts_d=None, slack=4096):
    """the C entry over (start, n, rate, count_idx) rows with a canary-filled `out` -> (all bytes of the buffer, canaries included, the
    table, the per-range sample records)"""
    lib = _lib.lib()
    tab = np.zeros(len(rows), _lib.ADPCM_RANGE)
    blocks = nbytes = 0
    for i, (start, n, rate, ci) in enumerate(rows):
        tab[i] = (start, n, blocks, nbytes, rate, ci, 0)
        if rate:
            nb = adpcm.n_blocks(n, rate)
            blocks, nbytes = blocks + nb, nbytes + nb * adpcm.align(rate)
    sizes = (C.c_int64 * 3)()
    assert lib.ctts_adpcm_encode_sizes(tab.ctypes.data_as(C.c_void_p), len(rows), sizes) == 0, lib.ctts_last_error()
    assert list(sizes) == [blocks, nbytes, (8 * len(rows) + 15) // 16 * 16]
    buf_d = torch.full((FRONT + nbytes + slack,), CANARY, dtype=torch.uint8, device=DEV)
    used_d = torch.full((len(rows) + 2,), -77, dtype=torch.int64, device=DEV)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    rc = lib.ctts_adpcm_encode_ranges(pcm_d.data_ptr(), _lib.ptr(counts_d), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(rows),
                                      buf_d.data_ptr() + FRONT, nbytes, used_d.data_ptr(), 8 * len(rows),
                                      torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, lib.ctts_last_error()
    torch.cuda.synchronize()
    return buf_d.cpu().numpy(), tab, used_d.cpu().numpy()


@pytest.fixture(scope="module")
def packed():
    """every case at every rate in one buffer -> (pcm, [(start, n, rate)], [name], the twin's blocks per range): computed once"""
    items, names = [], []
    for rate in AC.RATES:
        for name, x in AC.cases(rate):
            items.append((x, rate))
            names.append(f"{rate}/{name}")
    order = np.random.default_rng(5).permutation(len(items))     # the rates mixed through the call
    items, names = [items[i] for i in order], [names[i] for i in order]
    pcm, ranges = AC.pack(items)
    want = [adpcm.encode_blocks(x, rate) for x, rate in items]
    return pcm, ranges, names, want


def test_all_cases_in_one_call_with_mixed_rates(packed):
    pcm, ranges, names, want = packed
    assert len(ranges) <= 1024 and len({r for _, _, r in ranges}) == 3
    out, tab, used = _raw(torch.from_numpy(pcm).to(DEV), [(s, n, r, -1) for s, n, r in ranges])
    assert (out[:FRONT] == CANARY).all()
    for k, (name, w) in enumerate(zip(names, want)):
        b0 = FRONT + int(tab["byte0"][k])
        assert np.array_equal(out[b0: b0 + w.size], w), name
    end = FRONT + sum(w.size for w in want)
    assert (out[end:] == CANARY).all() and out.size - end == 4096
    assert used[: len(ranges)].tolist() == [n for _, n, _ in ranges] and used[len(ranges):].tolist() == [-77, -77]


def test_counts_skips_and_the_canaries_between():
    """S = 505 at 8000 Hz, 1017 at 24000 Hz.  Range 0: 70 blocks, range 1 (next rate): one block -- blocks 64 .. 69 fill a wave partly
    and share their workgroup with range 1's.  Range 2 is skipped; range 3's count ends a block exactly (2 of its 3 blocks are
    written); range 4's count leaves ONE sample in its last block; range 5's count is 0, range 6's negative, range 7's beyond n;
    range 8 is empty.  Blocks a count left out keep their canaries: nothing outside a range's written blocks is written."""
    S8, S24 = 505, 1017
    sig = [(AC.noise(70 * S8, 1), 8000), (AC.noise(S24 - 3, 2), 24000), (AC.noise(900, 3), 0), (AC.noise(3 * S24, 4), 24000),
           (AC.noise(4 * S8, 5), 8000), (AC.noise(600, 6), 48000), (AC.noise(600, 7), 8000), (AC.burst(48000, 0.1), 48000)]
    pcm, ranges = AC.pack(sig)
    rows = [(s, n, r, ci) for (s, n, r), ci in zip(ranges, [-1, -1, -1, 0, 1, 2, 3, 4])]
    rows.append((len(pcm) - 8, 0, 24000, -1))
    counts = np.array([2 * S24, 2 * S8 + 1, 0, -5, 1 << 40], np.int64)
    want_n = [70 * S8, S24 - 3, 0, 2 * S24, 2 * S8 + 1, 0, 0, 4800, 0]
    out, tab, used = _raw(torch.from_numpy(pcm).to(DEV), rows, torch.from_numpy(counts).to(DEV))
    assert used[: len(rows)].tolist() == want_n
    assert tab["block0"].tolist() == [0, 70, 71, 71, 74, 78, 79, 81, 84] and int(tab["byte0"][1]) == 70 * 256
    want = np.full(out.size, CANARY, np.uint8)
    for (start, n, rate, _), m, b0 in zip(rows, want_n, tab["byte0"]):
        if rate and m:
            w = adpcm.encode_blocks(pcm[start: start + m], rate)
            want[FRONT + int(b0): FRONT + int(b0) + w.size] = w
    assert np.array_equal(out, want)
    owned = sum(adpcm.n_blocks(n, r) * adpcm.align(r) for _, n, r, _ in rows if r)
    assert owned == out.size - FRONT - 4096


def test_each_range_alone_equals_the_range_in_the_pack(codec, packed):
    pcm, ranges, names, want = packed
    pcm_d = torch.from_numpy(pcm).to(DEV)
    pick = [k for k, nm in enumerate(names) if nm.split("/")[1] in ("noise1", "noise2", "square", "lo_hi", "burst", "step88+1", "zeros")]
    pick += [k for k, nm in enumerate(names) if nm.startswith("24000/noise") and nm not in ("24000/noise1", "24000/noise2")]
    assert len(pick) >= 25
    for k in pick:
        s, n, r = ranges[k]
        (got, m), = codec.adpcm_encode(pcm_d, [(s, n, r)], info=True)
        assert m == n and got.dtype == np.uint8 and np.array_equal(got, want[k]), names[k]
        assert adpcm.wav_bytes(got, m, r).tobytes() == adpcm.wav_header(n, r) + want[k].tobytes()


def test_engine_entry_results_and_refusals(codec):
    x = AC.noise(3000, 9)
    pcm = np.concatenate([x, np.zeros(8, np.int16)])
    pcm_d = torch.from_numpy(pcm).to(DEV)
    counts = torch.tensor([1500, 0], dtype=torch.int64, device=DEV)
    res = codec.adpcm_encode(pcm_d, [(0, 1000, 8000), (1000, 504, None), (1504, 1400, 24000, 0), (2904, 96, 48000, 1)], counts=counts, info=True)
    assert res[1] is None and res[0][1] == 1000 and res[2][1] == 1400 and res[3][1] == 0 and res[3][0].size == 0
    assert np.array_equal(res[0][0], adpcm.encode_blocks(x[:1000], 8000)) and np.array_equal(res[2][0], adpcm.encode_blocks(x[1504:2904], 24000))
    plain = codec.adpcm_encode(pcm_d, [(0, 1000, 8000), (1000, 504, 0)])
    assert plain[1] is None and np.array_equal(plain[0], res[0][0])
    none = codec.adpcm_encode(pcm_d, [(0, 0, 8000), (8, 16, None)])                 # nothing to encode: no launch
    assert none[0].size == 0 and none[0].dtype == np.uint8 and none[1] is None
    assert adpcm.behind_decode(res[3][0], res[3][1], 48000).size == 60
    with pytest.raises(ValueError, match="int16"):
        codec.adpcm_encode(pcm_d.float(), [(0, 8, 8000)])
    with pytest.raises(ValueError, match="beyond the"):
        codec.adpcm_encode(pcm_d, [(0, 4000, 8000)])
    with pytest.raises(ValueError, match="beyond `counts`"):
        codec.adpcm_encode(pcm_d, [(0, 100, 8000, 2)], counts=counts)
    with pytest.raises(ValueError, match="beyond `counts`"):
        codec.adpcm_encode(pcm_d, [(0, 100, 8000, 0)])
    # the library's refusals come before any launch: nothing is written
    for rows, word in (([(4, 100, 8000)], "multiples of 8"), ([(0, 100, 8000), (96, 100, 8000)], "overlapping"), ([(0, 100, -3)], "rate"),
                       ([(8 * i, 8, 8000) for i in range(1025)], "1024")):
        big = torch.from_numpy(np.zeros(9000, np.int16)).to(DEV)
        with pytest.raises(_lib.EngineError, match=word):
            codec.adpcm_encode(big, rows)


@pytest.mark.parametrize("keep_thr", [None, 1e-5])
def test_fed_from_the_grouped_conversion(codec, keep_thr):
    """float_to_int16_groups' slots and its device count header go straight into the encoder: group g's file is `adpcm.encode` of exactly
    the samples the conversion hands out for it, stripped or not; a group without a rate comes back as before; an all-silent group
    that the strip empties comes back as the bare header"""
    rng = np.random.default_rng(11)
    segs = [5000, 3000, 4096, 700, 9000, 640]
    off = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([(s + 7) // 8 * 8 for s in segs], out=off[1:])
    wav = np.zeros(int(off[-1]), np.float32)
    for k, s in enumerate(segs[:-1]):
        w = (np.sin(np.arange(s) * 0.05 * (k + 1)) * 0.4 + rng.standard_normal(s) * 0.01).astype(np.float32)
        w[rng.random(s) < 0.3] = 0.0                              # what the strip removes
        wav[int(off[k]): int(off[k]) + s] = w
    grp = np.array([0, 2, 3, 5, 6], np.int32)
    wav_d = torch.from_numpy(wav).to(DEV)
    blob, starts = codec.float_to_int16_groups(wav_d, off, grp, keep_thr=keep_thr)
    plain = E.CodecEngine.unpack_groups(codec.to_host(blob), starts)
    rates = [24000, None, 8000, 48000]
    files = codec.float_to_int16_groups_adpcm(wav_d, off, grp, rates, keep_thr=keep_thr)
    assert len(files) == 4 and files[1].dtype == np.int16 and np.array_equal(files[1], plain[1])
    for g in (0, 2, 3):
        assert files[g].dtype == np.uint8 and files[g].tobytes() == adpcm.encode_result(plain[g], rates[g]).tobytes(), g
    if keep_thr is not None:
        assert len(plain[0]) < segs[0] + segs[1] and len(plain[3]) == 0 and files[3].size == 60
    mixed = codec.float_to_int16_groups_adpcm(wav_d, off, grp, [8000, None, None, 8000], keep_thr=keep_thr, encodings=[None, "ulaw", None, None])
    assert mixed[1].dtype == np.uint8 and mixed[1].size == len(plain[1]) and np.array_equal(mixed[2], plain[2])
    assert mixed[0].tobytes() == adpcm.encode_result(plain[0], 8000).tobytes()
    with pytest.raises(ValueError, match="not both"):
        codec.float_to_int16_groups_adpcm(wav_d, off, grp, [8000, None, None, None], encodings=["ulaw", None, None, None])
    with pytest.raises(ValueError, match="one rate"):
        codec.float_to_int16_groups_adpcm(wav_d, off, grp, [8000, None])

"""The device pause stage (csrc/pauses.hip, ctts_trim_pauses_ragged, CodecEngine.trim_pauses) against the independent serial oracle
(tests/pauses_oracle.py): samples, output offsets and records bit for bit, at segment lengths around the plan kernel's chunk, at every
packed alignment, alone and packed, with canaries behind the output and the scratch.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib  # noqa: E402
from chattts_amd import pauses as PA  # noqa: E402
from tests import pauses_cases as PC  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 4096


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _specs(ks):
    return [None if k is None else PC.spec_of(k) for k in ks]


def _raw(xs, rates, ks, out=None, src=None):
    """the pack of xs through the C entry with buffers of this test's own: a canary behind the output, behind the results and behind
    the scratch -> (return code, samples per segment, off_out, records)"""
    lib = _lib.lib()
    tb = PA.tables(PC.offsets([len(x) for x in xs]), rates, _specs(ks))
    off, rows, fbase, fade = tb["off"], tb["rows"], tb["fbase"], tb["fade"]
    n, n_seg = int(off[-1]), len(xs)
    if src is None:
        src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    buf = torch.full((n + CANARY,), 123.0, dtype=torch.float32, device=DEV) if out is None else out
    tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), fbase.view(np.uint8), rows.reshape(-1).view(np.uint8), fade.view(np.uint8)])).to(DEV)
    res_bytes = 8 * (n_seg + 1) + 4 * PA.REC * n_seg
    res_pad = -(-res_bytes // 16) * 16
    assert tb["scratch"] == int(lib.ctts_trim_pauses_ragged_scratch_bytes(int(fbase[-1]), n_seg))
    work = torch.full((res_pad + tb["scratch"] + CANARY,), 0x5A, dtype=torch.uint8, device=DEV)
    base, wp = tabs.data_ptr(), work.data_ptr()
    rc = lib.ctts_trim_pauses_ragged(src.data_ptr(), buf.data_ptr(), base, off.ctypes.data_as(C.c_void_p), base + off.nbytes,
                                     fbase.ctypes.data_as(C.c_void_p), base + off.nbytes + fbase.nbytes, rows.ctypes.data_as(C.c_void_p), n_seg,
                                     base + off.nbytes + fbase.nbytes + rows.nbytes, int(fade.size), wp, wp + 8 * (n_seg + 1), wp + res_pad,
                                     tb["scratch"], None)
    torch.cuda.synchronize()
    if rc != 0:
        return rc, buf, None, None
    host, w = buf.cpu().numpy(), work.cpu().numpy()
    off_out = w[: 8 * (n_seg + 1)].view(np.int64)
    rec = w[8 * (n_seg + 1): res_bytes].view(np.int32).reshape(n_seg, PA.REC)
    assert np.all(w[res_bytes: res_pad] == 0x5A) and np.all(w[res_pad + tb["scratch"]:] == 0x5A), "the canary behind the scratch was written"
    assert np.all(host[n:] == np.float32(123.0)), "the canary behind the output was written"
    assert np.all(host[int(off_out[-1]): n] == np.float32(123.0)), "samples were written behind the last segment's output"
    return rc, [host[off_out[i]: off_out[i + 1]] for i in range(n_seg)], off_out, rec


def _check(xs, rates, ks, ys, off_out, rec, tag):
    want = [PC.answer(x, fs, k) for x, fs, k in zip(xs, rates, ks)]
    assert off_out.tolist() == PC.offsets([len(y) for y, _ in want]).tolist(), tag
    for i, (y, r) in enumerate(want):
        assert rec[i].tolist() == list(r), (tag, i, rec[i].tolist(), r)
        assert ys[i].tobytes() == y.tobytes(), (tag, i)


def _pack(fs):
    seg = PC.segments(fs)
    return [x for x, _ in seg], [fs] * len(seg), [k for _, k in seg]


def test_the_fixture_keeps_every_sample_away_from_the_threshold_and_covers_the_paths():
    """conditions on the fixture, checked on the host: no sample within a factor of 2 of the threshold; packed offsets at every residue
    mod 4; crossfade frames at a misaligned source and at a misaligned destination; rows that lose samples at every rate"""
    for fs in PC.RATES:
        xs, rates, ks = _pack(fs)
        worst = min(PC.margin(x) for x in xs)
        print(f"{fs} Hz: the closest sample is a factor of {worst:.3f} from the threshold")
        assert worst >= 2.0
        off = PC.offsets([len(x) for x in xs])
        assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3}, fs
        F = fs // 100
        src_mis = dst_mis = runs = 0
        off_out = PC.offsets([len(PC.answer(x, fs, k)[0]) for x, k in zip(xs, ks)])
        for s, (x, k) in enumerate(zip(xs, ks)):
            keep, mix, rec = PA.plan(PA.activity(x, F, PC.THR), len(x), F, PA.check(PC.spec_of(k)))
            assert rec == list(PC.answer(x, fs, k)[1])
            runs += rec[5]
            start = np.cumsum(keep * F) - keep * F
            for a in np.nonzero(mix >= 0)[0]:
                src_mis += (off[s] + a * F) % 4 != 0 or (off[s] + mix[a] * F) % 4 != 0
                dst_mis += (off_out[s] + start[a]) % 4 != 0
        assert runs >= 4 and src_mis >= 1 and dst_mis >= 1, (fs, runs, src_mis, dst_mis)
        assert any(len(PC.answer(x, fs, k)[0]) < len(x) for x, k in zip(xs, ks))


@pytest.mark.parametrize("fs", PC.RATES)
def test_every_length_at_one_rate_against_the_oracle(fs):
    xs, rates, ks = _pack(fs)
    rc, ys, off_out, rec = _raw(xs, rates, ks)
    assert rc == 0, _lib.lib().ctts_last_error()
    _check(xs, rates, ks, ys, off_out, rec, f"{fs} Hz")


def test_rates_mixed_in_one_pack_none_rows_and_alone_versus_packed():
    xs, rates, ks = [], [], []
    for i in range(10):                                      # segment i of rate i mod 4, every other odd one copied through
        fs = PC.RATES[i % 4]
        x, k = PC.segments(fs)[i]
        xs.append(x)
        rates.append(fs)
        ks.append(None if i % 4 == 1 else k)
    rc, ys, off_out, rec = _raw(xs, rates, ks)
    assert rc == 0, _lib.lib().ctts_last_error()
    _check(xs, rates, ks, ys, off_out, rec, "mixed")
    for i, k in enumerate(ks):
        if k is None:
            assert ys[i].tobytes() == xs[i].tobytes()
    for i in range(len(xs)):                                 # every segment alone: the record and the samples bit for bit
        for lead in (0, 1, 2, 3):                            # .. at every alignment of its first sample
            if lead and i % 3:
                continue
            pre = [np.full(lead, 0.5, np.float32)] if lead else []
            rc, y1, o1, r1 = _raw(pre + [xs[i]], [24000] * len(pre) + [rates[i]], [None] * len(pre) + [ks[i]])
            assert rc == 0
            assert y1[-1].tobytes() == ys[i].tobytes() and r1[-1].tolist() == rec[i].tolist(), (i, lead)


def test_an_output_that_overlaps_the_input_is_refused_and_nothing_is_written():
    xs, rates, ks = _pack(8000)
    n = sum(len(x) for x in xs)
    n4 = (n + 3) & ~3                                        # the next 16-byte aligned place behind the input
    both = torch.full((n4 + n + CANARY,), 123.0, dtype=torch.float32, device=DEV)
    both[:n].copy_(torch.from_numpy(np.concatenate(xs)))
    before = both.cpu().numpy().copy()
    for shift in (0, 4, n4 - 4):                             # the same buffer, a little behind it, its last samples
        rc, _, _, _ = _raw(xs, rates, ks, out=both[shift:], src=both[:n])
        assert rc != 0 and b"overlap" in _lib.lib().ctts_last_error()
        assert both.cpu().numpy().tobytes() == before.tobytes()
    rc, ys, off_out, rec = _raw(xs, rates, ks, out=both[n4:], src=both[:n])     # directly behind it: accepted
    assert rc == 0
    _check(xs, rates, ks, ys, off_out, rec, "behind")


def test_the_engine_call_in_its_three_forms(codec):
    fs = 24000
    xs, rates, ks = _pack(fs)
    off = PC.offsets([len(x) for x in xs])
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    y, off_out, rec = codec.trim_pauses(src, _specs(ks), offsets=off, rates=fs, return_stats=True)
    assert y.numel() == off_out[-1] and isinstance(off_out, np.ndarray) and off_out.dtype == np.int64
    host = y.cpu().numpy()
    _check(xs, rates, ks, [host[off_out[i]: off_out[i + 1]] for i in range(len(xs))], off_out, rec, "engine")
    y2, off2 = codec.trim_pauses(src, _specs(ks), offsets=off, rates=fs)
    assert off2.tolist() == off_out.tolist() and y2.cpu().numpy().tobytes() == host.tobytes()
    one = codec.trim_pauses(torch.from_numpy(xs[7]).to(DEV), PC.spec_of(ks[7]), rates=fs)                # 1-D: a tensor
    assert isinstance(one, torch.Tensor) and one.cpu().numpy().tobytes() == PC.answer(xs[7], fs, ks[7])[0].tobytes()
    rows = torch.from_numpy(np.stack([xs[5], xs[5][::-1].copy()])).to(DEV)                                # [B, n]: every row alone
    yr, offr = codec.trim_pauses(rows, PC.spec_of(0), rates=fs)
    w0, w1 = PC.answer(xs[5], fs, 0)[0], PC.answer(xs[5][::-1].copy(), fs, 0)[0]
    assert offr.tolist() == [0, len(w0), len(w0) + len(w1)] and yr.cpu().numpy().tobytes() == np.concatenate([w0, w1]).tobytes()
    same, off3 = codec.trim_pauses(src, None, offsets=off)                                                # nothing asked: no launch
    assert same.data_ptr() == src.data_ptr() and off3.tolist() == off.tolist()
    assert codec.trim_pauses(src, [None] * len(xs), offsets=off)[0].data_ptr() == src.data_ptr()
    assert codec.trim_pauses(src[:4800], None) is not None


def test_refusals_come_before_any_launch(codec):
    x = torch.zeros(4800, dtype=torch.float32, device=DEV)
    for kw in (dict(spec=dict(max_pause_ms=5)), dict(spec=dict(gap=1)), dict(spec="x"), dict(spec=True, rates=7999), dict(spec=True, rates=48001),
               dict(spec=True, offsets=[0, 4800, 4800]), dict(spec=True, offsets=[0, 4000]), dict(spec=[True, True]),
               dict(spec=True, offsets=[0, 2400, 4800], rates=[8000])):
        with pytest.raises(ValueError):
            codec.trim_pauses(x, **kw)
    with pytest.raises(ValueError):
        codec.trim_pauses(x.double(), True)

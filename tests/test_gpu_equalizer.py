"""The device equaliser (csrc/equalizer.hip, CodecEngine.equalize) against the serial definition (`equalizer.apply`, pinned by
tests/test_equalizer_host.py) on the pack of tests/equalizer_cases.py: every sample within one float32 ulp and at most 1e-3 of them
different at all, the off segment bit for bit, a segment's independence of what it is packed with, in place against out of place, rows
against the pack, canaries on both sides of every buffer, the scratch at exactly its declared size on poisoned memory, and every
refusal before any launch.  `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import equalizer as EQ  # noqa: E402
from tests import equalizer_cases as K  # noqa: E402
from tests.test_gpu_workspace_contract import _stage_contract, stage_codec  # noqa: E402,F401

DEV = torch.device("cuda:0")
CANARY = 4096


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _run(codec, flat, off, rates, specs, inplace=False, shift=0):
    """a pack through the device -> the packed result on the host; the canaries in front of and behind the input and the output must
    survive, and so must the input when the call is not in place.  `shift`: floats the pack sits off the buffers' 16-byte alignment"""
    n = len(flat)
    lo = CANARY + shift
    buf = torch.full((n + 2 * CANARY + 4,), 123.0, dtype=torch.float32, device=DEV)
    src_buf = buf if inplace else torch.full((n + 2 * CANARY + 4,), 321.0, dtype=torch.float32, device=DEV)
    src = src_buf[lo: lo + n]
    src.copy_(torch.from_numpy(np.array(flat, dtype=np.float32)))
    dst = buf[lo: lo + n]
    y = codec.equalize(src, specs, offsets=off, rates=rates, out=dst)
    torch.cuda.synchronize()
    assert y.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(host[:lo] == np.float32(123.0)) and np.all(host[lo + n:] == np.float32(123.0)), "a canary around the output was written"
    if not inplace:
        h = src_buf.cpu().numpy()
        assert np.all(h[:lo] == np.float32(321.0)) and np.all(h[lo + n:] == np.float32(321.0)), "a canary around the input was written"
        assert h[lo: lo + n].tobytes() == np.ascontiguousarray(flat).tobytes(), "the input was written"
    return host[lo: lo + n].copy()


@pytest.fixture(scope="module")
def packed(codec):
    """the pack of every kind of input through the device, once"""
    return {kind: _run(codec, K.pack(kind), K.OFFSETS, K.RATES, K.SPECS) for kind in K.KINDS}


def test_the_kernels_are_the_definition_but_for_rounding_boundaries(packed):
    """every sample within one float32 ulp of `equalizer.apply`, at most 1e-3 of them different at all, the off segment bit for bit.
    Observed on an MI355X: 9 of 51516 samples differ, a share of 1.75e-4, all of them in the 20 Hz high-pass at 48 kHz under the two
    impulses (7 and 2); none under the noise or the DC + sine input."""
    K.compare("device", packed)


def test_the_kernels_against_their_twin(packed):
    """the NumPy twin of the route computes what the launches compute, up to the fused multiply-adds of the device: the same bound"""
    for kind in K.KINDS:
        twin = EQ.equalize(K.pack(kind), K.SPECS, offsets=K.OFFSETS, rates=K.RATES, route=True)
        d = K.ulps(packed[kind], twin)
        print(f"device against the route twin, {kind}: {int((d > 0).sum())} of {len(d)} differ")
        assert int(d.max()) <= 1 and float((d > 0).mean()) <= K.CAP


@pytest.mark.parametrize("kind", ["noise", "impulse_chunk_end"])
def test_alone_in_place_and_off_the_alignment_give_the_packs_bits(codec, packed, kind):
    x, want = K.pack(kind), packed[kind]
    assert _run(codec, x, K.OFFSETS, K.RATES, K.SPECS, inplace=True).tobytes() == want.tobytes(), "in place differs from out of place"
    for i, (n, rate, spec) in enumerate(K.SEGMENTS):               # every segment alone: the tiles are anchored at its first sample
        if spec is not None:
            a, b = K.OFFSETS[i], K.OFFSETS[i + 1]
            alone = _run(codec, x[a:b], np.array([0, n], np.int64), rate, spec, inplace=bool(i & 1))
            assert alone.tobytes() == want[a:b].tobytes(), f"segment {i} ({n} samples) alone differs from the pack"
    one = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), x])).to(DEV)[1:]             # 4 bytes off the allocation's alignment
    y2 = codec.equalize(one, K.SPECS, offsets=K.OFFSETS, rates=K.RATES)                          # no `out`: a tensor of its own
    assert y2.data_ptr() != one.data_ptr() and y2.cpu().numpy().tobytes() == want.tobytes() and one.cpu().numpy().tobytes() == x.tobytes()
    y1 = codec.equalize(one, K.SPECS, offsets=K.OFFSETS, rates=K.RATES, out=one)
    assert y1.data_ptr() == one.data_ptr() and y1.cpu().numpy().tobytes() == want.tobytes()


def test_rows_equal_the_same_rows_packed(codec):
    n = K.T + 7
    rows = np.stack([K.signal("noise", n, 24000, 1), K.signal("dc_sine", n, 24000, 2), K.signal("noise", n, 24000, 3)])
    specs = [K.MAX4, None, "telephone"]
    t = torch.from_numpy(rows).to(DEV)
    y = codec.equalize(t, specs, rates=24000)
    assert y.shape == t.shape and y.data_ptr() != t.data_ptr() and t.cpu().numpy().tobytes() == rows.tobytes(), "the input was written"
    flat = codec.equalize(t.view(-1).clone(), specs, offsets=np.arange(4, dtype=np.int64) * n, rates=[24000] * 3)
    assert y.cpu().numpy().tobytes() == flat.cpu().numpy().tobytes()
    assert y[1].cpu().numpy().tobytes() == rows[1].tobytes()                                       # the row that is off
    for b in (0, 2):
        d = K.ulps(y[b].cpu().numpy(), EQ.apply(rows[b], 24000, specs[b]))
        assert int(d.max()) <= 1
    z = codec.equalize(t, specs, rates=24000, out=t)                                               # [B, n] in place
    assert z.data_ptr() == t.data_ptr() and z.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    single = codec.equalize(torch.from_numpy(rows[0]).to(DEV), K.MAX4)                             # 1-D, one signal, the default rate
    assert single.cpu().numpy().tobytes() == y[0].cpu().numpy().tobytes()


def test_the_scratch_at_its_declared_size_on_poisoned_memory(monkeypatch, stage_codec):
    """the call inside an arena that hands out exactly ctts_equalize_ragged_scratch_bytes, pre-filled with zeros, 0x7F and 0xFF, guards
    on both sides: no guard byte changes, and the results are bit-identical under the three patterns and to an un-instrumented run"""
    x = torch.from_numpy(K.pack("noise").copy()).to(DEV)
    y = _stage_contract(monkeypatch, lambda: stage_codec.equalize(x, K.SPECS, offsets=K.OFFSETS, rates=K.RATES), "equalize")
    assert int(K.ulps(y.cpu().numpy(), K.reference("noise")).max()) <= 1
    short = torch.from_numpy(K.signal("noise", 3 * 50, 8000, 9)).to(DEV)                           # no segment longer than a tile: one launch
    _stage_contract(monkeypatch, lambda: stage_codec.equalize(short, "telephone", offsets=[0, 50, 100, 150], rates=8000), "equalize, short segments")


def test_refusals_come_before_any_launch(codec):
    x = torch.zeros(4800, dtype=torch.float32, device=DEV)
    for kw in (dict(rates=24005), dict(rates=7990), dict(rates=48010), dict(offsets=[0, 4800, 4800]), dict(offsets=[0, 4000]),
               dict(offsets=[0, 2400, 4800], rates=[24000])):
        with pytest.raises(ValueError):
            codec.equalize(x, "telephone", **kw)
    five = {"peaks": [{"hz": 1000, "db": 1, "q": 1}] * 5}
    for spec in (None, False, {}, True, 1, "phone", five, {"highpass_hz": 19}, {"highpass_hz": 11000}, {"gain": 3}, ["telephone", "telephone"]):
        with pytest.raises(ValueError):
            codec.equalize(x, spec)
    with pytest.raises(ValueError):
        codec.equalize(x.double(), "telephone")
    with pytest.raises(ValueError):
        codec.equalize(x, "telephone", out=torch.zeros(4801, dtype=torch.float32, device=DEV))
    # the C entry itself, on live device buffers: a null pointer, a misaligned buffer, an empty segment, five sections, a rate out of range
    lib = codec.lib
    off = np.array([0, 2400, 4800], np.int64)
    sel = np.array([0, 0], np.int32)
    good = np.ascontiguousarray(EQ.row(24000, "telephone")[None])
    tabs = torch.from_numpy(np.concatenate([good.view(np.uint8).reshape(-1), off.view(np.uint8), sel.view(np.uint8)])).to(DEV)
    sb = int(lib.ctts_equalize_ragged_scratch_bytes(off.ctypes.data_as(C.c_void_p), 2))
    work = torch.empty(sb + 16, dtype=torch.uint8, device=DEV)
    x.fill_(0.25)
    torch.cuda.synchronize()

    def call(xp=x.data_ptr(), yp=x.data_ptr(), off_h=off, coef_h=good, scratch=work.data_ptr()):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        p_off = tabs.data_ptr() + good.nbytes
        rc = lib.ctts_equalize_ragged(xp, yp, p_off, vp(off_h), len(off_h) - 1, p_off + off.nbytes, vp(sel), tabs.data_ptr(), vp(coef_h), 1, scratch, sb, None)
        return rc, lib.ctts_last_error().decode()

    def row_with(at, v):
        r = good.copy()
        r[0, at] = v
        return r

    for kw, why in ((dict(xp=None), "null"), (dict(yp=None), "null"), (dict(xp=x.data_ptr() + 4), "16-byte aligned"), (dict(scratch=work.data_ptr() + 8), "scratch"),
                    (dict(off_h=np.array([0, 2400, 2400], np.int64)), "empty"), (dict(coef_h=row_with(0, 5.0)), "1 .. 4 second-order sections (got 5)"),
                    (dict(coef_h=row_with(1, 48010.0)), "multiple of 10 Hz in 8000 .. 48000"), (dict(coef_h=row_with(1, 7000.0)), "multiple of 10 Hz in 8000 .. 48000")):
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_equalize_ragged" in msg and why in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((x == 0.25).all()), "a refused call wrote its output"
    rc, msg = call()                                                                               # the same call, unrefused, runs
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert not bool((x == 0.25).any()), "the call that passes every check did not filter both segments"

"""The device compressor (csrc/compressor.hip, CodecEngine.compress) against the NumPy twin (chattts_amd/compressor.py, pinned by
tests/test_compressor_host.py): every sample and every record bit for bit, a segment's independence of what it is packed with, in
place against out of place, canaries on both sides of every buffer.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import compressor as CP  # noqa: E402
from tests import compressor_cases as C  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 4096


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _run(codec, xs, rates, specs, inplace=False):
    """the pack of xs through the device -> (samples per segment, records); the canaries in front of and behind the input and the
    output must survive, and so must the input when the call is not in place"""
    off = C.offsets([len(x) for x in xs])
    n = int(off[-1])
    flat = np.concatenate(xs)
    buf = torch.full((n + 2 * CANARY,), 123.0, dtype=torch.float32, device=DEV)
    src_buf = buf if inplace else torch.full((n + 2 * CANARY,), 321.0, dtype=torch.float32, device=DEV)
    src = src_buf[CANARY: CANARY + n]
    src.copy_(torch.from_numpy(flat))
    dst = buf[CANARY: CANARY + n]
    y, st = codec.compress(src, specs, offsets=off, rates=rates, return_stats=True, out=dst)
    torch.cuda.synchronize()
    assert y.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(host[:CANARY] == np.float32(123.0)) and np.all(host[CANARY + n:] == np.float32(123.0)), "a canary around the output was written"
    if not inplace:
        h = src_buf.cpu().numpy()
        assert np.all(h[:CANARY] == np.float32(321.0)) and np.all(h[CANARY + n:] == np.float32(321.0)), "a canary around the input was written"
        assert h[CANARY: CANARY + n].tobytes() == flat.tobytes(), "the input was written"
    return [host[CANARY + off[i]: CANARY + off[i + 1]] for i in range(len(xs))], st


def _same(tag, y, st, twin):
    ty, trec = twin
    assert st.tobytes() == trec.tobytes(), (tag, st, trec)
    if y.tobytes() != ty.tobytes():
        bad = np.flatnonzero(y.view(np.uint32) != ty.view(np.uint32))
        raise AssertionError(f"{tag}: {len(bad)} of {len(y)} samples differ from the twin, the first at {bad[0]}: {y[bad[0]]!r} against {ty[bad[0]]!r}")


@pytest.mark.parametrize("fs", C.RATES)
def test_every_case_at_one_rate_against_the_twin(codec, fs):
    cs = C.cases(fs)
    ys, st = _run(codec, [x for _, x, _ in cs], fs, [s for _, _, s in cs])
    for i, (name, _, _) in enumerate(cs):
        _same(f"{name}@{fs}", ys[i], st[i], C.twin(fs)[i])
    recs = {name: st[i] for i, (name, _, _) in enumerate(cs)}
    assert recs["quiet"]["n_blocks"] == 0 and recs["quiet"]["n_touched"] == 0 and recs["quiet"]["min_gain"] == 1.0
    assert recs["silence"].tobytes() == np.array((1.0, 0, 0, 0.0), dtype=CP.STATS).tobytes()
    assert recs["nan"]["n_touched"] > 0 and recs["nan"]["peak"] <= 0.9 and np.isinf(recs["inf"]["peak"])
    long = 5 * C.TILE * (fs // 1000) + 3
    assert recs[f"held_{long}"]["n_blocks"] == 1 and recs[f"held_{long}"]["n_touched"] > 3 * C.TILE * (fs // 1000)      # one block, held across tiles
    assert sum(int(np.isnan(y).sum()) for y in ys) == 4 + fs // 1000


def test_rates_and_specs_mixed_in_one_pack_in_place_and_alone_versus_packed(codec):
    pick = [(fs, i) for k, fs in enumerate(C.RATES) for i in range(k, len(C.cases(fs)), 4)]     # every case once, the rates in turn
    pick.sort(key=lambda p: p[1])
    xs = [C.cases(fs)[i][1] for fs, i in pick]
    specs = [C.cases(fs)[i][2] for fs, i in pick]
    rates = [fs for fs, _ in pick]
    specs[3] = None                                                                               # copied through, among the others
    ys, st = _run(codec, xs, rates, specs)
    for k, (fs, i) in enumerate(pick):
        if k == 3:
            assert ys[k].tobytes() == xs[k].tobytes() and st[k].tobytes() == np.array((1.0, 0, 0, 0.0), dtype=CP.STATS).tobytes()
        else:
            _same(f"{C.cases(fs)[i][0]}@{fs} mixed", ys[k], st[k], C.twin(fs)[i])
    ys2, st2 = _run(codec, xs, rates, specs, inplace=True)
    assert st2.tobytes() == st.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(ys, ys2)), "in place differs from out of place"
    for k in range(0, len(pick), 5):               # segments alone, at the pack's other alignments too: the record and the samples bit for bit
        if specs[k] is not None:
            y1, s1 = _run(codec, [xs[k]], [rates[k]], [specs[k]])
            assert s1.tobytes() == st[k: k + 1].tobytes() and y1[0].tobytes() == ys[k].tobytes(), pick[k]


def test_rows_a_single_signal_and_a_misaligned_view(codec):
    fs = 24000
    cs = C.cases(fs)
    i = next(k for k, c in enumerate(cs) if c[0].startswith("env_default_"))
    x = cs[i][1]
    rows = torch.from_numpy(np.stack([x, x[::-1].copy()])).to(DEV)                               # [B, n]: every row alone
    y, st = codec.compress(rows, True, rates=fs, return_stats=True)
    assert y.shape == rows.shape and y.data_ptr() != rows.data_ptr()
    assert y[0].cpu().numpy().tobytes() == C.twin(fs)[i][0].tobytes() and st[0].tobytes() == C.twin(fs)[i][1].tobytes()
    assert y[1].cpu().numpy().tobytes() == CP.compress_segment(x[::-1], fs)[0].tobytes()
    assert rows[0].cpu().numpy().tobytes() == x.tobytes(), "the input was written"
    one = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), x])).to(DEV)[1:]             # 4 bytes off the allocation's alignment
    y1 = codec.compress(one, True, rates=fs, out=one)
    assert y1.data_ptr() == one.data_ptr() and y1.cpu().numpy().tobytes() == C.twin(fs)[i][0].tobytes()


def test_refusals_come_before_any_launch(codec):
    x = torch.zeros(4800, dtype=torch.float32, device=DEV)
    for kw in (dict(rates=24005), dict(rates=7990), dict(rates=48010), dict(offsets=[0, 4800, 4800]), dict(offsets=[0, 4000]),
               dict(offsets=[0, 2400, 4800], rates=[24000])):
        with pytest.raises(ValueError):
            codec.compress(x, True, **kw)
    for spec in (None, False, 1, "on", {"ratio": 1.0}, {"gain": 3}, {"attack_ms": True}, [True, True]):
        with pytest.raises(ValueError):
            codec.compress(x, spec)
    with pytest.raises(ValueError):
        codec.compress(x.double(), True)

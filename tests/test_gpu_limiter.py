"""The device limiter (csrc/limiter.hip, CodecEngine.peak_limit and loudness_normalize(limiter=)) against the NumPy twin
(chattts_amd/limiter.py, itself pinned to the brute-force oracle by tests/test_limiter_host.py): every sample and every record bit for
bit, a segment's independence of what it is packed with, in place against out of place, and the loudness stage in front of it.
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import limiter as LM  # noqa: E402
from chattts_amd import loudness as LN  # noqa: E402
from tests import limiter_cases as C  # noqa: E402
from tests import loudness_cases as LC  # noqa: E402
from tests.test_gpu_loudness import G_BOUND, L_BOUND  # noqa: E402

DEV = torch.device("cuda:0")
CANARY = 4096


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _run(codec, xs, rates, gains, inplace=False, **kw):
    """the pack of xs through the device -> (samples per segment, records); a canary behind the output must survive"""
    off = C.offsets([len(x) for x in xs])
    n = int(off[-1])
    buf = torch.full((n + CANARY,), 123.0, dtype=torch.float32, device=DEV)
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    if inplace:
        buf[:n].copy_(src)
        src = buf[:n]
    y, st = codec.peak_limit(src, offsets=off, rates=rates, gains=gains, return_stats=True, out=buf[:n], **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(host[n:] == np.float32(123.0)), "the canary behind the output was written"
    if not inplace:
        assert src.cpu().numpy().tobytes() == np.concatenate(xs).tobytes(), "the input was written"
    return [host[off[i]: off[i + 1]] for i in range(len(xs))], st


def _same(tag, y, st, twin):
    ty, trec = twin
    assert st.tobytes() == trec.tobytes(), (tag, st, trec)
    if y.tobytes() != ty.tobytes():
        bad = np.flatnonzero(y.view(np.uint32) != ty.view(np.uint32))
        raise AssertionError(f"{tag}: {len(bad)} of {len(y)} samples differ from the twin, the first at {bad[0]}: {y[bad[0]]!r} against {ty[bad[0]]!r}")


@pytest.mark.parametrize("fs", C.RATES)
def test_every_case_at_one_rate_against_the_twin(codec, fs):
    cs = C.cases(fs)
    ys, st = _run(codec, [x for _, x, _ in cs], fs, [g for _, _, g in cs])
    for i, (name, _, _) in enumerate(cs):
        _same(f"{name}@{fs}", ys[i], st[i], C.twin(fs)[i])
    assert max(np.abs(y).max() for y in ys) <= LM.C32


def test_rates_mixed_in_one_pack_in_place_and_alone_versus_packed(codec):
    pick = [(fs, i) for k, fs in enumerate(C.RATES) for i in range(k, len(C.cases(fs)), 4)]     # every case once, the rates in turn
    pick.sort(key=lambda p: p[1])
    xs = [C.cases(fs)[i][1] for fs, i in pick]
    gs = [C.cases(fs)[i][2] for fs, i in pick]
    rates = [fs for fs, _ in pick]
    ys, st = _run(codec, xs, rates, gs)
    for k, (fs, i) in enumerate(pick):
        _same(f"{C.cases(fs)[i][0]}@{fs} mixed", ys[k], st[k], C.twin(fs)[i])
    ys2, st2 = _run(codec, xs, rates, gs, inplace=True)
    assert st2.tobytes() == st.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(ys, ys2)), "in place differs from out of place"
    for k in range(len(pick)):                     # every segment alone: the record and the samples bit for bit
        y1, s1 = _run(codec, [xs[k]], [rates[k]], [gs[k]])
        assert s1.tobytes() == st[k: k + 1].tobytes() and y1[0].tobytes() == ys[k].tobytes(), pick[k]


def test_rows_a_single_signal_a_nan_and_device_gains(codec):
    fs = 24000
    cs = C.cases(fs)
    i = next(k for k, c in enumerate(cs) if c[0] == f"pair2W_{2 * C.TILE + 1}")
    x = cs[i][1]
    rows = torch.from_numpy(np.stack([x, x[::-1].copy()])).to(DEV)                            # [B, n]: every row alone
    y, st = codec.peak_limit(rows, rates=fs, gains=2.0, return_stats=True)
    assert y.shape == rows.shape and y.data_ptr() != rows.data_ptr()
    assert y[0].cpu().numpy().tobytes() == C.twin(fs)[i][0].tobytes() and st[0].tobytes() == C.twin(fs)[i][1].tobytes()
    assert y[1].cpu().numpy().tobytes() == LM.limit_segment(x[::-1], fs, 2.0)[0].tobytes()
    assert rows[0].cpu().numpy().tobytes() == x.tobytes(), "the input was written"
    g = torch.tensor([2.0], dtype=torch.float32, device=DEV)                                   # the gains where the loudness stage leaves them
    y1 = codec.peak_limit(torch.from_numpy(x).to(DEV), rates=fs, gains=g)
    assert y1.cpu().numpy().tobytes() == C.twin(fs)[i][0].tobytes()
    xn = x.copy()
    xn[100] = np.nan                                                                           # a NaN passes through and asks for no gain
    yn, sn = codec.peak_limit(torch.from_numpy(xn).to(DEV), rates=fs, gains=2.0, return_stats=True)
    tn, trec = LM.limit_segment(xn, fs, 2.0)
    assert yn.cpu().numpy().tobytes() == tn.tobytes() and sn[0].tobytes() == trec.tobytes() and np.isnan(tn[100]) and np.isnan(tn).sum() == 1


def _loud(codec, xs, targets, rates, lim, groups=None):
    off = LC.offsets([len(x) for x in xs])
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    y, st, ls = codec.loudness_normalize(src, targets, offsets=off, groups=groups, rates=rates, return_stats=True, out=src, limiter=lim)
    torch.cuda.synchronize()
    host = y.cpu().numpy()
    return [host[off[i]: off[i + 1]] for i in range(len(xs))], st, ls


def test_loudness_in_front_of_the_limiter_against_the_twins(codec):
    """L and g32 under the loudness tests' bounds; the samples bit for bit the twin limiter at the device's own g32"""
    sig = LC.signals()
    names = [s[0] for s in sig]
    idx = [names.index(n) for n in ("bursts", "env4_9600", "env4_24000", "sine", "silent", "faint", "env5_50000")]
    xs = [sig[i][1] for i in idx]
    tg = [-5.0, -5.0, -5.0, -16.0, -16.0, -10.0, None]
    rates = [24000, 8000, 24000, 48000, 22050, 24000, 8000]
    lim = [True, True, True, True, True, False, True]
    ys, st, ls = _loud(codec, xs, tg, rates, lim)
    _, tst, _ = LN.normalize(np.concatenate(xs), tg, offsets=LC.offsets([len(x) for x in xs]), rates=rates, limiter=lim)
    plain = LN.normalize(np.concatenate(xs), tg, offsets=LC.offsets([len(x) for x in xs]), rates=rates)[1]
    assert plain["bound"][0] == LN.BOUND_CEILING and st["bound"][0] == LN.BOUND_TARGET and st["g32"][0] > plain["g32"][0]
    for k in range(len(xs)):
        tag = f"{names[idx[k]]}@{rates[k]}"
        assert (st["n_blocks"][k], st["n_abs"][k], st["n_rel"][k], st["bound"][k]) == (tst["n_blocks"][k], tst["n_abs"][k], tst["n_rel"][k], tst["bound"][k]), tag
        assert st["bound"][k] in (-1, 0, 1) or not lim[k], tag
        if tst["n_abs"][k]:
            print(f"{tag}: L {st['L'][k]:.9f} twin {tst['L'][k]:.9f} g32 {st['g32'][k]:.7g} twin {tst['g32'][k]:.7g} bound {st['bound'][k]}")
            assert abs(st["L"][k] - tst["L"][k]) <= L_BOUND and abs(float(st["g32"][k]) / float(tst["g32"][k]) - 1.0) <= G_BOUND, tag
        else:
            assert st["g32"][k] == 1.0, tag
        if lim[k]:
            ty, trec = LM.limit_segment(xs[k], rates[k], st["g32"][k])
            assert ls[k].tobytes() == trec.tobytes(), (tag, ls[k], trec)
            assert ys[k].tobytes() == ty.tobytes(), tag
        else:
            assert ys[k].tobytes() == (np.float32(st["g32"][k]) * xs[k]).tobytes() and ls[k].tobytes() == np.zeros((), LM.STATS).tobytes(), tag
    assert ls["n_over"][0] > 0 and ls["n_over"][4] == 0 and ls["g32"][6] == 1.0
    assert max(np.abs(ys[k]).max() for k in range(len(xs)) if lim[k]) <= LM.C32
    # the same rows without measurement: the limiter at unity gain, only where it is asked for
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    y = codec.loudness_normalize(src, None, offsets=LC.offsets([len(x) for x in xs]), rates=rates, limiter=[k == 3 for k in range(len(xs))])
    assert y.data_ptr() != src.data_ptr()
    want = np.concatenate([LM.limit_segment(x, rates[k])[0] if k == 3 else x for k, x in enumerate(xs)])
    assert y.cpu().numpy().tobytes() == want.tobytes() and src.cpu().numpy().tobytes() == np.concatenate(xs).tobytes()


def test_a_group_gets_one_gain_and_the_limiter_runs_per_sentence(codec):
    sig = LC.signals()
    names = [s[0] for s in sig]
    members = [["bursts", "env4_9600", "env0_1"], ["env1_2399"], ["env4_24000", "bursts"]]
    idx = [[names.index(m) for m in g] for g in members]
    flat = [i for g in idx for i in g]
    grp = np.array([0, 3, 4, 6], np.int32)
    rates = [24000, 8000, 48000, 22050, 24000, 24000]
    tg = [-5.0, -16.0, -6.0]
    lim = [True, False, True]
    xs = [sig[i][1] for i in flat]
    ys, st, ls = _loud(codec, xs, tg, rates, lim, groups=grp)
    _, tst, _ = LN.normalize(np.concatenate(xs), tg, offsets=LC.offsets([len(x) for x in xs]), groups=grp, rates=rates, limiter=lim)
    for g in range(3):
        assert abs(st["L"][g] - tst["L"][g]) <= L_BOUND and abs(float(st["g32"][g]) / float(tst["g32"][g]) - 1.0) <= G_BOUND and st["bound"][g] == tst["bound"][g], g
        for k in range(int(grp[g]), int(grp[g + 1])):
            if lim[g]:
                ty, trec = LM.limit_segment(xs[k], rates[k], st["g32"][g])          # the sentence alone: no window spans two
                assert ys[k].tobytes() == ty.tobytes() and ls[k].tobytes() == trec.tobytes(), (g, k)
            else:
                assert ys[k].tobytes() == (np.float32(st["g32"][g]) * xs[k]).tobytes(), (g, k)
    y1, s1, l1 = _loud(codec, xs[4:6], [tg[2]], rates[4:6], True, groups=np.array([0, 2], np.int32))     # the last group alone
    assert s1.tobytes() == st[2:3].tobytes() and l1.tobytes() == ls[4:6].tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(y1, ys[4:6]))


def test_refusals_come_before_any_launch(codec):
    x = torch.zeros(4800, dtype=torch.float32, device=DEV)
    for kw in (dict(rates=24005), dict(rates=7990), dict(rates=48010), dict(offsets=[0, 4800, 4800]), dict(offsets=[0, 4000]),
               dict(gains=[1.0, 2.0]), dict(gains=0.0), dict(gains=float("nan")), dict(offsets=[0, 2400, 4800], rates=[24000])):
        with pytest.raises(ValueError):
            codec.peak_limit(x, **kw)
    with pytest.raises(ValueError):
        codec.peak_limit(x.double())
    for lim in (1, "yes", [True, False]):
        with pytest.raises(ValueError):
            codec.loudness_normalize(x, -16.0, limiter=lim)

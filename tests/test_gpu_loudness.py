"""The device loudness stage (csrc/loudness.hip, CodecEngine.loudness_normalize) against the independent float64 oracle
(tests/loudness_oracle.py): block counts exactly, the loudness and the gain under their bounds, every sample and the peak bit for bit,
and a group's independence of what it is packed with.  `pytest -m gpu`."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import loudness as LN  # noqa: E402
from tests import loudness_cases as LC  # noqa: E402

DEV = torch.device("cuda:0")
# |L - L_oracle|: the condition is 1e-4 LU (100 times under the fixture's gate margin).  The device carries states and energies in
# float64; the worst value measured on the MI355X over every case of this file is 3.2e-14 LU (profiles/loudness_probe.md), and the bound
# is 100 times that
L_BOUND = 3.2e-12
G_BOUND = math.log(10.0) / 20.0 * 1e-4 + 2.0 ** -23
CANARY = 4096


@pytest.fixture(scope="module")
def codec(weights):
    from chattts_amd.engine import CodecEngine
    return CodecEngine(weights["decoder"], weights["vocos"], DEV)


def _run(codec, xs, targets, rates, groups=None, inplace=False):
    """the pack of xs through the device -> (samples per segment, records); a canary behind the output must survive"""
    off = LC.offsets([len(x) for x in xs])
    n = int(off[-1])
    buf = torch.full((n + CANARY,), 123.0, dtype=torch.float32, device=DEV)
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    if inplace:
        buf[:n].copy_(src)
        src = buf[:n]
    y, st = codec.loudness_normalize(src, targets, offsets=off, groups=groups, rates=rates, return_stats=True, out=buf[:n])
    torch.cuda.synchronize()
    assert y.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(host[n:] == np.float32(123.0)), "the canary behind the output was written"
    return [host[off[i]: off[i + 1]] for i in range(len(xs))], st


def _check(st, o, x_list, y_list, tag):
    """one group's record and samples against the oracle's record o -> |L - L_oracle|"""
    assert (st["n_blocks"], st["n_abs"], st["n_rel"]) == (o["n_blocks"], o["n_abs"], o["n_rel"]), (tag, st, o)
    assert st["peak"] == np.float32(max(np.abs(x).max() for x in x_list)), tag
    assert st["bound"] == o["bound"], (tag, st, o)
    err = 0.0
    if o["n_abs"] == 0:
        assert st["L"] == -math.inf and st["g32"] == np.float32(1.0), (tag, st)
    else:
        err = abs(float(st["L"]) - o["L"])
        print(f"{tag}: L {st['L']:.9f} oracle {o['L']:.9f} |dL| {err:.3e} g32 {st['g32']:.7g} g_oracle {o['g']:.7g} bound {st['bound']}")
        assert err <= L_BOUND, (tag, st, o)
        assert abs(float(st["g32"]) / o["g"] - 1.0) <= G_BOUND, (tag, st, o)
    for x, y in zip(x_list, y_list):
        assert y.tobytes() == (np.float32(st["g32"]) * x).tobytes(), tag
    return err


def test_the_fixture_keeps_every_block_away_from_both_gates():
    """a condition on the fixture, not on the device: no block of any case within 0.01 LU of a gate"""
    worst = min(LC.alone(i, fs)["margin"] for i in range(len(LC.signals())) for fs in LC.RATES)
    print(f"smallest gate distance over the fixture: {worst:.4f} LU")
    assert worst >= 0.01
    kinds = {name: LC.alone(i, 24000) for i, (name, _, _) in enumerate(LC.signals())}
    assert kinds["bursts"]["bound"] == 2 and kinds["sine"]["bound"] == 0 and kinds["faint"]["bound"] == 1 and kinds["silent"]["n_abs"] == 0 and kinds["zeros"]["n_abs"] == 0
    every = [LC.alone(i, fs) for i in range(len(LC.signals())) for fs in LC.RATES]
    assert sum(0 < o["n_abs"] < o["n_blocks"] for o in every) >= 4 and sum(0 < o["n_rel"] < o["n_abs"] for o in every) >= 4


@pytest.mark.parametrize("fs", LC.RATES)
def test_every_case_at_one_rate_against_the_oracle(codec, fs):
    sig = LC.signals()
    xs = [x for _, x, _ in sig]
    ys, st = _run(codec, xs, [t for _, _, t in sig], fs)
    worst = max(_check(st[i], LC.alone(i, fs), [xs[i]], [ys[i]], f"{sig[i][0]}@{fs}") for i in range(len(sig)))
    print(f"worst |L - L_oracle| at {fs} Hz: {worst:.3e} LU")


def test_rates_mixed_in_one_pack_and_alone_versus_packed(codec):
    sig = LC.signals()
    xs = [x for _, x, _ in sig]
    tg = [t for _, _, t in sig]
    rates = [LC.RATES[i % 4] for i in range(len(sig))]
    ys, st = _run(codec, xs, tg, rates)
    for i in range(len(sig)):
        _check(st[i], LC.alone(i, rates[i]), [xs[i]], [ys[i]], f"{sig[i][0]}@{rates[i]} mixed")
    ys2, st2 = _run(codec, xs, tg, rates, inplace=True)
    assert st2.tobytes() == st.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(ys, ys2)), "in place differs from out of place"
    for i in range(len(sig)):                      # every segment alone: the record and the samples bit for bit
        y1, s1 = _run(codec, [xs[i]], [tg[i]], [rates[i]])
        assert s1.tobytes() == st[i: i + 1].tobytes() and y1[0].tobytes() == ys[i].tobytes(), sig[i][0]


def test_groups_pool_their_blocks_and_share_one_gain(codec):
    sig = LC.signals()
    names = [s[0] for s in sig]
    members = [["env5_50000", "env0_1", "zeros", "env5_9601"], ["env1_2399"], ["silent", "env4_24000", "silent"], ["zeros", "silent"],
               ["sine", "env2_2400"], ["env3_123457", "faint"]]
    idx = [[names.index(m) for m in g] for g in members]
    rates = [[LC.RATES[(k + j) % 4] for j in range(len(g))] for k, g in enumerate(idx)]
    tg = [-16.0, -23.0, -16.0, -16.0, -16.0, -10.0]
    flat = [i for g in idx for i in g]
    flat_r = [r for g in rates for r in g]
    grp = np.concatenate([[0], np.cumsum([len(g) for g in idx])]).astype(np.int32)
    xs = [sig[i][1] for i in flat]
    ys, st = _run(codec, xs, tg, flat_r, groups=grp)
    for k, g in enumerate(idx):
        a, b = int(grp[k]), int(grp[k + 1])
        o = LC.grouped(g, rates[k], tg[k])
        assert o["margin"] >= 0.01, (k, o)
        _check(st[k], o, xs[a:b], ys[a:b], f"group {k}")
        y1, s1 = _run(codec, xs[a:b], [tg[k]], rates[k], groups=np.array([0, b - a], np.int32))     # the group alone
        assert s1.tobytes() == st[k: k + 1].tobytes() and all(p.tobytes() == q.tobytes() for p, q in zip(y1, ys[a:b])), k
    assert st["n_abs"][3] == 0 and st["g32"][3] == 1.0 and st["bound"][0] == 0


def test_a_null_target_leaves_its_rows_alone_and_rows_are_segments(codec):
    sig = LC.signals()
    xs = [sig[i][1] for i in (9, 13, 4, 16)]
    tg = [None, -16.0, None, -10.0]
    ys, st = _run(codec, xs, tg, 24000)
    for i in (0, 2):
        assert ys[i].tobytes() == xs[i].tobytes() and st["g32"][i] == 1.0 and st["bound"][i] == -1
        assert st["L"][i] == _run(codec, [xs[i]], [-16.0], 24000)[1]["L"][0]                        # measured all the same
    assert ys[1].tobytes() != xs[1].tobytes() and ys[3].tobytes() != xs[3].tobytes()
    src = torch.from_numpy(np.concatenate(xs)).to(DEV)
    assert codec.loudness_normalize(src, [None] * 4, offsets=LC.offsets([len(x) for x in xs])) is src      # nothing asked: no launch
    rows = torch.from_numpy(np.stack([sig[9][1], sig[13][1]])).to(DEV)                                   # [B, n]: every row alone
    y, s2 = codec.loudness_normalize(rows, -16.0, return_stats=True)
    assert y.shape == rows.shape and s2[1:].tobytes() == st[1:2].tobytes() and y[1].cpu().numpy().tobytes() == ys[1].tobytes()
    twin_y, twin_st = LN.normalize(np.concatenate(xs), tg, offsets=LC.offsets([len(x) for x in xs]))
    assert np.array_equal(twin_st["n_rel"], st["n_rel"]) and np.array_equal(twin_st["bound"], st["bound"])
    assert np.max(np.abs(twin_st["L"] - st["L"])) <= L_BOUND


def test_refusals_come_before_any_launch(codec):
    x = torch.zeros(4800, dtype=torch.float32, device=DEV)
    for kw in (dict(target=-4.0), dict(target=-41.0), dict(target="x"), dict(target=-16.0, rates=24005), dict(target=-16.0, rates=7990),
               dict(target=-16.0, rates=48010), dict(target=-16.0, offsets=[0, 4800, 4800]), dict(target=-16.0, offsets=[0, 4000]),
               dict(target=-16.0, offsets=[0, 2400, 4800], groups=[0, 1]), dict(target=[-16.0, -16.0])):
        with pytest.raises(ValueError):
            codec.loudness_normalize(x, **kw)
    with pytest.raises(ValueError):
        codec.loudness_normalize(x.double(), -16.0)

"""The prompt-pass attention tests, the parts that need no GPU: the derived bounds of tests/prompt_pass_oracle.py hold for numpy
emulations of the two kernels' arithmetic; a mask that is off by one key at its lower end breaks them on the same inputs (the trap
rows); the case table of tests/prompt_pass_cases.py reaches every edge it is meant to reach; the test-only entry points refuse what
they must."""
import numpy as np
import pytest

from tests import prompt_pass_cases as PC
from tests import prompt_pass_oracle as PO

EMU = {"mfma": PO.emulate_mfma, "wave": PO.emulate_wave}


def _naive_row(q, K, V, c, g, t):
    """one row of one group, written out plainly: the oracle's own check"""
    slot = c.slot0 + t
    lo = min(c.kv_start[g], slot)
    qr = q[g * c.T + t, :PO.H].astype(np.float64).reshape(PO.NH, PO.HD)
    Kb, Vb = K[g, :, lo: slot + 1].astype(np.float64), V[g, :, lo: slot + 1].astype(np.float64)
    s = np.einsum("hd,hjd->hj", qr, Kb) / 8.0
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("hj,hjd->hd", p, Vb).reshape(PO.H), slot - lo + 1


@pytest.mark.parametrize("name", ["t129_s33", "t33_s200", "t2_s7"])
def test_oracle_equals_a_plain_row_loop(name):
    c = PC.BY_NAME[name]
    q, K, V, _ = PC.inputs(c)
    r = PC.answer(c)
    for g in range(PC.groups(c)):
        for t in sorted({0, 1, c.T // 2, c.T - 1}):
            ref, n = _naive_row(q, K, V, c, g, t)
            m = g * c.T + t
            assert r["n"][m] == n and r["valid"][m] == (c.slot0 + t >= c.kv_start[g])
            assert np.abs(r["ref"][m] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (name, g, t)
    assert np.isfinite(r["ref"]).all() and (r["a"] >= np.abs(r["ref"]) * (1 - 1e-12)).all() and (r["delta"] >= 0).all()


def test_bf16_round_is_round_to_nearest_even():
    from tests import gpu_util
    x = np.random.RandomState(3).standard_normal(100000).astype(np.float32) * np.float32(37.0)
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 2.0 ** -8, 0.0], np.float32)   # halfway cases
    for v in (x, ties):
        assert PO.bf16_round(v).tobytes() == gpu_util.bf16_round(v).tobytes()
    assert PO.bf16_round(ties)[:2].tolist() == [1.0, 1.0 + 2.0 ** -6]


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.name)
def test_emulated_kernel_stays_under_the_bound(c):
    """the kernel's arithmetic, restated in numpy, uses at most 0.9 of the derived f32-out bound on every valid row of the case; its
    bf16 rounding stays inside the bf16-out bound (which a value just above a power of two uses up: half an ulp there is 2^-8 of it)"""
    q, K, V, ks = PC.inputs(c)
    r = PC.answer(c)
    kern = PO.kernel_of(c.T)
    got = EMU[kern](q, K, V, c.T, c.slot0, ks)
    assert np.isfinite(got).all()
    ratio = PO.worst_ratio(got, r, kern)
    ratio16 = PO.worst_ratio(PO.bf16_round(got), r, kern, out_bf16=True)
    print(f"{c.name}: {kern} emulation worst |err| / bound = {ratio:.3f} (f32 out), {ratio16:.3f} (bf16 out)")
    assert ratio <= 0.9 and ratio16 <= 1.0, (c.name, ratio, ratio16)


@pytest.mark.parametrize("c", [c for c in PC.CASES if max(c.kv_start) > 0], ids=lambda c: c.name)
def test_a_leaked_pad_key_breaks_the_bound(c):
    """the first visible key moved down by one: every utterance with pad rows in reach shows it through its trap V"""
    q, K, V, ks = PC.inputs(c)
    r = PC.answer(c)
    kern = PO.kernel_of(c.T)
    got = EMU[kern](q, K, V, c.T, c.slot0, ks, lo_shift=-1)
    err = np.abs(got.astype(np.float64) - r["ref"]) / PO.bound(r, kern)
    for g, kvs in enumerate(c.kv_start):
        rows = np.arange(g * c.T, (g + 1) * c.T)
        rows = rows[r["valid"][rows]]
        if kvs > 0 and len(rows):
            assert err[rows].max() > 1.0, (c.name, g)


def test_case_table_reaches_every_edge():
    mf, wv = PC.MFMA_CASES, PC.WAVE_CASES
    assert all(c.T >= 128 and PO.kernel_of(c.T) == "mfma" and 3 <= PC.groups(c) <= 4 and c.T <= 200 for c in mf)
    assert all(2 <= c.T < 128 and PO.kernel_of(c.T) == "wave" for c in wv)
    for c in PC.CASES:   # what keeps a launch inside its buffers
        assert c.slot0 >= 0 and c.slot0 + c.T <= c.cmax and all(0 <= k <= c.slot0 + c.T - 1 for k in c.kv_start), c.name
    assert len({c.name for c in PC.CASES}) == len(PC.CASES) and len({c.seed for c in PC.CASES}) == len(PC.CASES)
    # MFMA kernel: ragged tiles and waves
    assert {c.T % 64 for c in mf} >= {0, 1, 16, 17, 63}
    assert any(c.T % 64 == 1 for c in mf)                                     # a last query tile of a single row
    assert {k % 32 for c in mf for k in c.kv_start} >= {0, 1, 31}
    assert {c.slot0 % 32 for c in mf} >= {0, 1, 31}
    rel = set()
    for c in mf:
        firsts = [c.slot0 + 64 * i for i in range((c.T + 63) // 64)]
        for k in c.kv_start:
            for f in firsts:
                last = min(f + 63, c.slot0 + c.T - 1)
                rel.add("before" if k < f else "first" if k == f else "inside" if k <= last else "behind")
            if k == c.slot0 + c.T - 1:
                rel.add("last_row")
            if k < c.slot0:
                rel.add("below_chunk")
    assert rel >= {"before", "first", "inside", "behind", "last_row", "below_chunk"}
    assert any(c.cmax == c.slot0 + c.T and c.cmax % 32 != 0 for c in mf)      # the staging loop's clamp onto the last cache row
    assert any(c.cmax > c.slot0 + c.T for c in mf)                            # ... and NaN rows behind the chunk
    # one-wave kernel
    assert {127, 33} <= {c.T for c in wv} and min(c.T for c in wv) == 2
    counts = set()
    for c in wv:
        r = PC.answer(c)
        counts |= set(r["n"][r["valid"]].tolist())
    assert counts >= {1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65}
    assert any(c.slot0 == 200 for c in wv)
    # both: flat and peaked softmax, pad rows, trap and NaN rows in the inputs
    for cs in (mf, wv):
        assert {c.qscale for c in cs} == {1.0, 12.0}
        assert any(max(c.kv_start) > c.slot0 for c in cs)
    for c in PC.CASES:
        q, K, V, ks = PC.inputs(c)
        assert K.tobytes() == PO.bf16_round(np.nan_to_num(K)).tobytes() or np.isnan(K).any()
        for g, k in enumerate(c.kv_start):
            assert (V[g, :, :k] == PC.TRAP_V).all() and np.isfinite(K[g, :, : c.slot0 + c.T]).all()
            assert np.isnan(K[g, :, c.slot0 + c.T:]).all() and np.isnan(V[g, :, c.slot0 + c.T:]).all()
            Kv, Vv = K[g, :, k: c.slot0 + c.T], V[g, :, k: c.slot0 + c.T]
            assert Kv.tobytes() == PO.bf16_round(Kv).tobytes() and Vv.tobytes() == PO.bf16_round(Vv).tobytes()
        assert all(0 < s < c.T for s in PC.cuts(c)) and (c.T - 1 in PC.cuts(c) or c.T == 1)
    # chunked prompts: same kernel for every chunk as for the whole, and a boundary off every block / tile edge
    for name, kvs, chunks, _ in PC.CHUNKED:
        T = sum(chunks)
        assert all(PO.kernel_of(n) == PO.kernel_of(T) and n >= 2 for n in chunks), name
    assert any(PO.kernel_of(sum(ch)) == "mfma" and any(b % 32 for b in np.cumsum(ch)[:-1]) for _, _, ch, _ in PC.CHUNKED)
    assert any(PO.kernel_of(sum(ch)) == "wave" for _, _, ch, _ in PC.CHUNKED)


def test_entry_points_refuse_bad_arguments():
    """no launch happens for any of these: the checks sit in front of it"""
    from chattts_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data
    att = lambda **kw: lib.ctts_k_attention_prefill_ex(*[kw.get(k, d) for k, d in (
        ("qkv", p), ("kc", p), ("vc", p), ("cmax", 300), ("out", p), ("out_bf16", 0), ("T", 130), ("slot0", 0), ("ks", p), ("rm", None),
        ("M", 260), ("st", None))])
    for bad in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(out=None), dict(ks=None), dict(out_bf16=2), dict(out_bf16=-1),
                dict(T=1, M=2), dict(M=261), dict(M=0), dict(slot0=-1), dict(slot0=171)):
        assert att(**bad) != 0, bad
        assert b"ctts_k_attention_prefill_ex" in lib.ctts_last_error(), bad
    qk = lambda **kw: lib.ctts_k_qkv_rope_ex(*[kw.get(k, d) for k, d in (
        ("A", p), ("W", p), ("M", 46), ("ssq", p), ("eps", 1e-6), ("qkv", p), ("kc", p), ("vc", p), ("cmax", 60), ("cos", p), ("sin", p),
        ("T", 23), ("len", None), ("ks", p), ("slot0", 0), ("rm", None), ("mb", 0), ("st", None))])
    for bad in (dict(A=None), dict(W=None), dict(ssq=None), dict(qkv=None), dict(kc=None), dict(vc=None), dict(cos=None), dict(sin=None),
                dict(ks=None), dict(T=1), dict(M=47), dict(M=0), dict(slot0=-1), dict(slot0=38)):
        assert qk(**bad) != 0, bad
        assert b"ctts_k_qkv_rope_ex" in lib.ctts_last_error(), bad

"""The test-only entry points of the step's end (tests/test_gpu_step_back.py), the parts that need no GPU: the three symbols are exported,
declared and bound with the same argument count, and every documented refusal comes back non-zero from the host arguments alone."""
import ctypes as C
import os
import re

from chattts_amd import _lib

NAMES = ("ctts_k_final_norm_rows", "ctts_k_fnorm_heads", "ctts_k_sample_rows")


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        raw = f.read()
    assert '"fnorm16"' in raw                                   # the variant string the fused launch reports is documented
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, flags=re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is C.c_int


def _why():
    return _lib.lib().ctts_last_error()


def test_final_norm_rows_refuses_without_a_device():
    """the pointers below are never dereferenced: every refusal is decided before anything is launched"""
    lib = _lib.lib()
    p = lambda i: C.c_void_p(0x1000 * (i + 1))

    def call(x=p(0), qpb=1, w=p(1), hfin=p(2), hid=p(3), max_new=4, lens=p(4), T=3, B=2, row_map=None, n_active=None, prompt_len=None,
             packed=None, last_row=None):
        return lib.ctts_k_final_norm_rows(x, qpb, w, 1e-6, hfin, hid, max_new, lens, T, B, row_map, n_active, prompt_len, packed, last_row, None)

    for kw in (dict(x=None), dict(w=None), dict(hfin=None), dict(lens=None), dict(B=0), dict(B=-3), dict(qpb=0), dict(T=-1)):
        assert call(**kw) != 0 and b"bad arguments" in _why(), kw
    assert call(max_new=0) != 0 and b"max_new" in _why()
    assert call(qpb=3, n_active=p(5)) != 0 and b"n_active" in _why() and b"decode layout" in _why()
    assert call(n_active=p(5), last_row=p(6)) != 0 and b"last_row" in _why()


def test_fnorm_heads_refuses_without_a_device():
    lib = _lib.lib()
    p = lambda i: C.c_void_p(0x1000 * (i + 1))

    def call(Ap=p(0), Wp=p(1), M=16, N=32, n_cols=20, n_active=None, nw=p(2), Cc=p(3), ldc=20, desc=p(4), hid=p(5), hid_cap=4, T=3,
             prompt_len=None):
        return lib.ctts_k_fnorm_heads(Ap, Wp, M, N, n_cols, n_active, nw, 1e-6, Cc, ldc, desc, hid, hid_cap, T, prompt_len, None)

    for kw in (dict(Ap=None), dict(Wp=None), dict(nw=None), dict(Cc=None), dict(M=0), dict(M=-1)):
        assert call(**kw) != 0 and b"bad arguments" in _why(), kw
    for kw in (dict(N=0), dict(N=24), dict(n_cols=0), dict(n_cols=33), dict(ldc=19)):
        assert call(**kw) != 0 and b"multiple of 16" in _why(), kw
    for kw in (dict(desc=None), dict(hid_cap=0)):
        assert call(**kw) != 0 and b"hidden capture needs" in _why(), kw
    assert call(hid=None, prompt_len=p(6)) != 0 and b"prompt_len" in _why()


def test_sample_rows_refuses_without_a_device():
    lib = _lib.lib()
    p = lambda i: C.c_void_p(0x1000 * (i + 1))

    def state(**kw):
        s = _lib.GenState()
        s.B, s.T, s.max_new, s.nq, s.eos = 4, 1, 8, 1, 625
        s.ids_buf, s.len, s.finish, s.end_idx, s.q, s.temperature = (0x1000 * i for i in range(20, 26))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    fold = dict(desc=p(2), emb=p(3), x=p(4), desc_out=p(5), kv_start=p(6))

    def call(s=None, null_state=False, logits=p(0), n_text=0, rows=4, row_map=None, n_active=None, desc=None, emb=None, x=None, xb=None, ssq=None,
             desc_out=None, kv_start=None, xb_packed=0, xp32=None, lo=0, rope=None, cos=None, sin=None):
        st = None if null_state else C.byref(state() if s is None else s)
        return lib.ctts_k_sample_rows(st, logits, n_text, rows, row_map, n_active, desc, emb, x, xb, ssq, desc_out, kv_start, xb_packed, xp32, lo,
                                      rope, cos, sin, None)

    for kw in (dict(null_state=True), dict(logits=None), dict(rows=0), dict(rows=-1), dict(n_text=-1), dict(n_text=1 << 20)):
        assert call(**kw) != 0 and b"bad arguments" in _why(), kw
    assert call(rows=5) != 0 and b"more rows" in _why()
    for k in ("ids_buf", "len", "finish", "end_idx"):
        assert call(s=state(**{k: None})) != 0 and b"are needed" in _why(), k
    assert call(s=state(q=None)) != 0 and b"q draws" in _why()
    assert call(s=state(nq=0)) != 0 and b"q draws" in _why()
    assert call(n_text=300, desc=p(2)) != 0 and b"no descriptors" in _why()
    for k in ("emb", "xb", "ssq", "desc_out", "xp32", "rope"):
        assert call(**{k: p(7)}) != 0 and b"without x" in _why(), k
    # the fold: descriptors in and out, kv_start, codes only -- what run_step and decode_body impose
    assert call(**{**fold, "desc": None}, n_text=300) != 0 and b"no fold" in _why()
    assert call(**{**fold, "emb": None}) != 0 and b"emb_code" in _why()
    for k in ("desc", "desc_out"):
        assert call(**{**fold, k: None}) != 0 and b"descriptors in and out" in _why(), k
    assert call(**{**fold, "kv_start": None}) != 0 and b"kv_start" in _why()
    assert call(**fold, rope=p(8)) != 0 and b"cos / sin" in _why()
    assert call(**fold, rope=p(8), cos=p(9)) != 0 and b"cos / sin" in _why()
    for kw in (dict(lo=-8), dict(lo=12, xb=p(10), xb_packed=1), dict(lo=16), dict(lo=16, xb=p(10))):
        assert call(**fold, **kw) != 0 and b"lo plane" in _why(), kw

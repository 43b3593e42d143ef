"""The host side of the workspace contract (no GPU): the library's size functions never shrink when an argument grows, the derived
sizes reduce to their bases, `tests/ws_arena.Arena` does the arithmetic the GPU tests rely on (on a CPU tensor), and every workspace
or scratch allocation of the package goes through `chattts_amd.engine.device_scratch`."""
import ast
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from chattts_amd import _lib
from tests import ws_arena
from tests.ws_arena import ALIGN, GUARD_BYTE, GUARD_MIN, Arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _monotone(f, grids):
    """f over the product of `grids` (ascending values per argument): never smaller when ONE argument takes its next value, never 0"""
    import itertools
    vals = {a: int(f(*a)) for a in itertools.product(*grids)}
    assert all(v > 0 for v in vals.values()), [a for a, v in vals.items() if v <= 0]
    for a, v in vals.items():
        for k, g in enumerate(grids):
            i = g.index(a[k])
            if i + 1 < len(g):
                b = (*a[:k], g[i + 1], *a[k + 1:])
                assert vals[b] >= v, (a, v, b, vals[b])


# ---- the size functions --------------------------------------------------------------------------------------------------------
BS = [1, 2, 3, 8, 15, 16, 17, 32, 33, 64]
TS = [1, 2, 5, 16, 21, 63, 64, 65]


def test_gpt_workspace_is_monotone_and_holds_the_decode_carve(lib):
    _monotone(lib.ctts_gpt_workspace_bytes, [BS, TS])
    for B in BS:
        for T in TS:
            n = lib.ctts_gpt_workspace_bytes(B, T)
            assert n >= lib.ctts_gpt_workspace_bytes(B, 1) and n % ALIGN == 0, (B, T)
    assert lib.ctts_gpt_workspace_bytes(4, 0) == lib.ctts_gpt_workspace_bytes(4, 1)      # carve: M = B * max(T, 1)


def test_codec_workspaces_are_monotone_in_256_row_tiles(lib):
    FS = [2, 4, 254, 256, 258, 1022, 1024, 1026, 12288, 12290]
    _monotone(lib.ctts_codec_workspace_bytes, [[1, 2, 3], FS])
    row = (512 + 512 + 2048 + 384 + 1024) * 4                                           # carve_codec's five fields, per frame
    for B in (1, 2, 3):
        for F in FS:
            R = -(-B * F // 256) * 256
            assert lib.ctts_codec_workspace_bytes(B, F) == R * row, (B, F)
    _monotone(lib.ctts_dvae_decode_workspace_bytes, [[1, 2, 3], [1, 2, 33, 127, 128, 129]])
    _monotone(lib.ctts_dvae_encode_workspace_bytes, [[513, 767, 768, 1023, 1024, 10257, 24000]])


def test_ragged_and_window_workspaces_are_monotone_and_reduce_to_their_bases(lib):
    NW, TT = [1, 2, 3, 5], [5, 6, 40, 127, 513, 6145]
    _monotone(lib.ctts_codec_ragged_workspace_bytes, [NW, TT])
    # A window workspace ends in the packed waveforms, 256 (2 T - n_win) samples (carve_windows): at a fixed token total every further
    # window is one 256-sample frame LESS, so the size itself falls by 1024 bytes per window by design.  What never shrinks is the
    # size with those frames added back; in the token total and in the chunk area the size itself is monotone.
    back = lambda f: (lambda n, *a: f(n, *a) + 1024 * n if f(n, *a) else 0)
    _monotone(back(lib.ctts_codec_windows_workspace_bytes), [NW, TT])
    for n in NW:
        _monotone(lambda t: lib.ctts_codec_windows_workspace_bytes(n, t), [TT])
    CH = [0, 1, 63, 64, 4096, 100001]
    for f in (lib.ctts_codec_windows_rate_workspace_bytes, lib.ctts_codec_windows_speed_workspace_bytes,
              lib.ctts_codec_windows_speed_rate_workspace_bytes):
        _monotone(back(f), [NW, TT, CH])
        for n in NW:
            _monotone(lambda t, c: f(n, t, c), [TT, CH])
    for n in NW:
        for t in TT:
            base = lib.ctts_codec_windows_workspace_bytes(n, t)
            assert base >= lib.ctts_codec_ragged_workspace_bytes(n, t) >= lib.ctts_codec_workspace_bytes(1, 2 * t), (n, t)
            assert lib.ctts_codec_windows_rate_workspace_bytes(n, t, 0) == base
            # the time-scaled entries keep 16 bytes of path entries behind the chunk area, whatever its size: one 256-byte granule
            assert lib.ctts_codec_windows_speed_workspace_bytes(n, t, 0) == base + ALIGN
            assert lib.ctts_codec_windows_speed_rate_workspace_bytes(n, t, 0) == base + ALIGN
            for c in CH:
                assert lib.ctts_codec_windows_rate_workspace_bytes(n, t, c) == base + -(-4 * c // ALIGN) * ALIGN
                assert lib.ctts_codec_windows_speed_workspace_bytes(n, t, c) == base + -(-(4 * c + 16) // ALIGN) * ALIGN
                assert lib.ctts_codec_windows_speed_rate_workspace_bytes(n, t, c) == lib.ctts_codec_windows_speed_workspace_bytes(n, t, c)


def test_stage_scratch_sizes_are_monotone_in_the_pack(lib):
    """the offsets-based sizes over packs that grow by one sample across a tile edge and by one segment; the frame-based ones over
    their two arguments"""
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    by_off = (lib.ctts_loudness_normalize_ragged_scratch_bytes, lib.ctts_peak_limit_ragged_scratch_bytes, lib.ctts_compress_ragged_scratch_bytes)
    for f in by_off:
        last = 0
        for n in (1, 7, 8, 799, 800, 801, 2047, 2048, 2049, 24000):                     # one segment, longer and longer
            off = i64([0, n])
            v = int(f(_vp(off), 1))
            assert v >= last and v > 0, (f, n, v, last)
            last = v
        for n_seg in (1, 2, 3, 9):                                                       # the same samples in more segments
            off = i64(np.linspace(0, 9000, n_seg + 1).astype(np.int64))
            v = int(f(_vp(off), n_seg))
            assert v >= int(f(_vp(i64([0, 9000])), 1)), (f, n_seg)
    last = 0
    for n in (1, 2047, 2048, 2049, 4097, 24000):                                         # the grouped conversion: tiles of 2048
        off, grp = i64([0, n]), np.ascontiguousarray([0, 1], dtype=np.int32)
        v = int(lib.ctts_float_to_int16_groups_scratch_bytes(_vp(off), 1, _vp(grp), 1))
        assert v == 4 * -(-n // 2048) and v >= last
        last = v
    off, grp = i64([0, 1, 2048, 4097]), np.ascontiguousarray([0, 2, 3], dtype=np.int32)
    assert int(lib.ctts_float_to_int16_groups_scratch_bytes(_vp(off), 3, _vp(grp), 2)) == 4 * 2 * 2   # two groups x the longest one's tiles
    _monotone(lib.ctts_trim_pauses_ragged_scratch_bytes, [[1, 2, 15, 16, 17, 1000], [1, 2, 3, 4, 5, 77]])
    _monotone(lib.ctts_trim_pauses_stream_scratch_bytes, [[0, 1, 15, 16, 17, 1000], [1, 2, 3, 100]])


# ---- the arena's own arithmetic ------------------------------------------------------------------------------------------------
CPU = torch.device("cpu")


def test_arena_views_are_exact_aligned_prefilled_and_apart():
    sizes = [1, 255, 256, 257, 0, 100000]
    a = Arena(Arena.room(sizes), 0xFF, CPU)
    views = [a.take(n) for n in sizes]
    assert a.takes == len(sizes) and a.sizes == sizes
    prev_end = 0
    for i, (v, n) in enumerate(zip(views, sizes)):
        assert v.dtype == torch.uint8 and v.numel() == n
        lo = a.regions[i][0]
        assert a.regions[i][1] == n and (a.buf.data_ptr() + lo) % ALIGN == 0
        if n:                                                                            # (an empty view has no address)
            assert v.data_ptr() == a.buf.data_ptr() + lo
        assert lo - prev_end >= (GUARD_MIN if i == 0 else 2 * GUARD_MIN), (i, lo, prev_end)   # guards of its own on both sides
        assert bool((v == 0xFF).all())
        prev_end = lo + n
    assert a.buf.numel() - prev_end >= GUARD_MIN
    a.assert_guards_intact()
    payload = sum(sizes)
    assert int((a.buf == GUARD_BYTE).sum()) == a.buf.numel() - payload
    views[3].fill_(0)                                                                    # writing the payload is what it is for
    a.assert_guards_intact()


def test_arena_refuses_what_does_not_fit_and_bad_patterns():
    a = Arena(Arena.room([1000]), 0x00, CPU)
    a.take(1000)
    with pytest.raises(MemoryError):
        a.take(1000)
    assert a.takes == 1
    with pytest.raises(ValueError):
        Arena(1 << 20, GUARD_BYTE, CPU)
    with pytest.raises(ValueError):
        Arena(1 << 20, 0x00, CPU, guard=1024)
    with pytest.raises(ValueError):
        a.take(-1)


@pytest.mark.parametrize("fill", ws_arena.PATTERNS)
def test_arena_names_the_first_damaged_byte_and_its_take(fill):
    sizes = [300, 4096, 77]
    for which, delta, word in ((0, -1, "in front of take 0"), (0, 0, "behind the end of take 0"), (1, -1, "in front of take 1"),
                               (1, 0, "behind the end of take 1"), (2, 0, "behind the end of take 2"),
                               (2, GUARD_MIN + 5000, "behind the end of take 2"), (1, -2 * GUARD_MIN + 10, "behind the end of take 0")):
        a = Arena(Arena.room(sizes) + 8192, fill, CPU)
        for n in sizes:
            a.take(n)
        lo, n = a.regions[which]
        at = lo - 1 if delta == -1 else lo + n + delta if delta >= 0 else lo + delta
        assert a.first_damage() is None
        a.buf[at] = fill                                                                 # one byte of payload pattern in a guard
        hit = a.first_damage()
        assert hit is not None and hit[0] == at and word in hit[1], (which, delta, hit)
        with pytest.raises(AssertionError, match=f"offset {at} "):
            a.assert_guards_intact()
    empty = Arena(1 << 20, fill, CPU)
    empty.buf[5] = 0x11
    assert empty.first_damage()[0] == 5


def test_arena_stands_in_for_the_seam_and_for_the_codec_buffer(monkeypatch):
    from chattts_amd import engine as E
    a = Arena(Arena.room([512, 1024]), 0x7F, CPU)
    monkeypatch.setattr(E, "device_scratch", a.device_scratch)
    t = E.device_scratch(512, CPU)
    assert t.numel() == 512 and a.takes == 1 and bool((t == 0x7F).all())
    ws, n = a.codec_ws_bytes(1000)
    assert n == 1000 and ws.numel() == 1000 and a.sizes == [512, 1000]


# ---- every allocation goes through the seam ------------------------------------------------------------------------------------
def _is_sized_call(node):
    """a call of a `*_workspace_bytes` / `*_scratch_bytes` function (or method)"""
    if not isinstance(node, ast.Call):
        return False
    f = node.func
    name = f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else ""
    return name.endswith("_workspace_bytes") or name.endswith("scratch_bytes")


def _is_uint8_empty(node):
    """torch.empty(..., dtype=torch.uint8, ...)"""
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "empty"
            and isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"):
        return False
    return any(k.arg == "dtype" and isinstance(k.value, ast.Attribute) and k.value.attr == "uint8" for k in node.keywords)


def _bypasses(tree):
    """(function, line) of every torch.empty(uint8) whose size comes from a size function called in the same function -- directly, or
    through a name assigned from one -- the seam itself excepted: that byte buffer is the workspace (or holds it behind the stage's
    records)"""
    out = []
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)) or fn.name == "device_scratch":
            continue
        body = list(ast.walk(fn))
        if not any(_is_sized_call(n) for n in body):
            continue
        # (the byte buffers a stage allocates for its OUTPUT -- blobs, masks -- are sized by other names)
        out += [(fn.name, n.lineno) for n in body if _is_uint8_empty(n) and _names_size(n, fn)]
    return out


def _names_size(call, fn):
    """the allocation's size expression uses a name bound from a size call in this function, or holds a size call itself"""
    if any(_is_sized_call(n) for n in ast.walk(call)):
        return True
    bound = set()
    for n in ast.walk(fn):
        if isinstance(n, ast.Assign) and any(_is_sized_call(m) for m in ast.walk(n.value)):
            for t in n.targets:
                bound |= {m.id for m in ast.walk(t) if isinstance(m, ast.Name)} | {m.attr for m in ast.walk(t) if isinstance(m, ast.Attribute)}
    used = {m.id for m in ast.walk(call) if isinstance(m, ast.Name)} | {m.attr for m in ast.walk(call) if isinstance(m, ast.Attribute)}
    return bool(bound & used)


def test_no_workspace_allocation_bypasses_the_seam():
    files = sorted(glob.glob(os.path.join(ROOT, "chattts_amd", "*.py")))
    assert len(files) > 10
    hits = []
    for path in files:
        with open(path, encoding="utf-8") as f:
            tree = ast.parse(f.read(), path)
        hits += [(os.path.basename(path), *h) for h in _bypasses(tree)]
    assert not hits, f"workspace / scratch buffers allocated outside engine.device_scratch: {hits}"


def test_the_bypass_check_sees_the_allocations_it_is_for():
    """the shapes the package had before the seam are caught, the seam and unrelated byte buffers are not"""
    old = '''
def a(self, n):
    nb = self.lib.ctts_dvae_encode_workspace_bytes(n)
    ws = torch.empty((nb,), dtype=torch.uint8, device=self.device)
def b(self):
    sb = int(self.lib.ctts_compress_ragged_scratch_bytes(off_p, n_seg))
    rec_bytes = 16
    work = torch.empty((rec_bytes + sb,), dtype=torch.uint8, device=dev)
def c(self):
    ws = torch.empty((self.lib.ctts_gpt_workspace_bytes(n, Tg),), dtype=torch.uint8, device=dev)
def d(ln):
    ln.ws_bytes = max(lib.ctts_gpt_workspace_bytes(Bl, tc_ws), lib.ctts_gpt_workspace_bytes(Bl, 1))
    ln.workspace = torch.empty((ln.ws_bytes,), dtype=torch.uint8, device=dev)
'''
    assert [h[0] for h in _bypasses(ast.parse(old))] == ["a", "b", "c", "d"]
    new = '''
def device_scratch(nbytes, device):
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)
def a(self, n):
    nb = self.lib.ctts_dvae_encode_workspace_bytes(n)
    ws = device_scratch(nb, self.device)
    blob = torch.empty((hdr + 2 * E,), dtype=torch.uint8, device=dev)
    f = torch.empty((nb,), dtype=torch.float32, device=dev)
'''
    assert _bypasses(ast.parse(new)) == []

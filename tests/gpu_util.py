"""Helpers for the `-m gpu` parity tests: thin wrappers that call single kernels through the C ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from chattts_amd import _lib

DEV = torch.device("cuda:0")


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous().to(DEV)


def bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def gemm(A, W, *, wt="f32", tiled=False, epi=0, norm_w=None, eps=1e-6, res=None, bias=None, gamma=None,
         taps=1, cin=0, frames=0, pad=0, dil=1, n_out=None):
    """A [M(or B*F), lda] f32, W [N(,2N),K].  Returns C [M, N] numpy."""
    lib = _lib.lib()
    A_d = dev(A, torch.float32)
    if tiled == 2:  # split-bf16 tiles: weights packed [2][N][Kp]
        from chattts_amd.engine import split_bf16
        Wt = torch.as_tensor(np.ascontiguousarray(W), dtype=torch.float32)
        W_d = split_bf16(Wt).to(DEV)
        K = Wt.shape[1]
        N = n_out if n_out is not None else Wt.shape[0]
    else:
        W_d = dev(W, torch.bfloat16 if wt == "bf16" else torch.float32)
        K = W_d.shape[1]
        N = n_out if n_out is not None else W_d.shape[0]
    M = A_d.shape[0]
    C_d = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    nw = None if norm_w is None else dev(norm_w, torch.float32)
    r = None if res is None else dev(res, torch.float32)
    b = None if bias is None else dev(bias, torch.float32)
    g = None if gamma is None else dev(gamma, torch.float32)
    rc = lib.ctts_k_gemm(int(tiled), A_d.data_ptr(), W_d.data_ptr(), C_d.data_ptr(), M, N, K, A_d.shape[1], N,
                         _lib.BF16 if wt == "bf16" else _lib.F32, epi, _lib.ptr(nw), eps, _lib.ptr(r), N, _lib.ptr(b), _lib.ptr(g),
                         taps, cin, frames, pad, dil, None)
    _lib.check(rc, "ctts_k_gemm")
    torch.cuda.synchronize()
    return C_d.cpu().numpy()


def relerr(got: np.ndarray, ref: np.ndarray) -> float:
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / max(1e-30, np.abs(ref).max()))


# ---- row descriptors (csrc/kernels.hpp RowDesc) ---------------------------------------------------------------------------------
DESC_ABSENT = (-1, 0, 0, 0)      # what the step's first kernel writes for a compact row that does not exist this step
CANARY32 = 0x5A5A5A5A            # int32 pattern of an output word no kernel may write
CANARY16 = 0x5A5A


def row_desc(b: int, slot: int, ks: int, finished: bool = False):
    """numpy restatement of write_desc (csrc/gpt.hip): {utterance or -1, KV slot, RoPE position, first visible key}; a slot in front
    of the utterance's first valid one (ks > slot) is a pad row: position 1, and it sees itself only"""
    return (-1 if finished else int(b), int(slot), 1 if slot - ks < 0 else int(slot - ks), int(slot) if ks > slot else int(ks))


def live_rows(finish: np.ndarray, order=None):
    """numpy restatement of the device-side compaction (nth_unfinished): the utterances with finish == 0 in visiting order"""
    seq = np.arange(len(finish)) if order is None else np.asarray(order)
    return [int(s) for s in seq if finish[s] == 0]


# ---- ragged decode: packed layouts whose segment boundaries fall where the codec kernels switch, tile and run -------------------
EDGE_MODS = (32, 36, 48, 64, 128, 256)   # GEMM row tiles 32 / 64 / 128 / 256; dwconv runs of 36 frames (dilation 1) and 48 (seq, dilation 2)
EDGE_SHORTS = (1, 2, 3, 4, 7)            # tokens: 2 - 14 frames, inside the k7 conv's reach, the dilation-2 dwconv's 13-frame span, one run
EDGE_LONG = 8                            # tokens: a "long" neighbour is at least 16 frames, wider than any of those spans
EDGE_ONES = 80                           # the run of 1-token segments: 160 frames from frame 256, 80 boundaries in one 256-row tile


def edge_residues(m: int):
    """the boundary residues mod m the layouts hit: 0 and +-2 frames.  A boundary sits at 2 x (a token offset), so with every m in
    EDGE_MODS even, +-1 frame is unreachable; +-2 frames (+-1 token) is the nearest a real pack can come."""
    return sorted({0, 2 % m, (-2) % m})


def _edge_hits(lens):
    """(m, residue) of every boundary with a long segment on at least one side"""
    f = np.concatenate([[0], 2 * np.cumsum(lens)])
    return {(m, int(f[i]) % m) for i in range(1, len(lens)) if max(lens[i - 1], lens[i]) >= EDGE_LONG for m in EDGE_MODS}


def ragged_edge_layout(total_frames: int, seed: int = 0):
    """Token lengths of a packed ragged-decode batch of exactly `total_frames` frames (2 per token), built to put segment boundaries
    where a wrong mask would show:
      * a 1-token segment first and last;
      * a long segment, then EDGE_ONES 1-token segments from frame 256 on (one dwconv run and every 32 ... 256-row tile over them
        holds many boundaries), closed by a long segment;
      * then long / short pairs, the shorts cycling through EDGE_SHORTS, each long sized so that its end lands on a residue
        0, +2 or -2 mod every m in EDGE_MODS that no boundary next to a long segment has hit yet;
      * the rest: long segments of U{128..512} tokens (the bench's utterance lengths) with a short between each two.
    Deterministic for (total_frames, seed); tests/test_ragged_codec_host.py checks these properties."""
    if total_frames % 2 or total_frames < 1000:
        raise ValueError("total_frames: an even number of at least 1000")
    T = total_frames // 2
    lens = [1, 127] + [1] * EDGE_ONES + [EDGE_LONG]   # the last entry is the open long segment: it grows before it is closed
    want = {(m, r) for m in EDGE_MODS for r in edge_residues(m)}
    si = 0
    while True:
        todo = want - _edge_hits(lens + [EDGE_LONG])
        if not todo:
            break
        pos = 2 * sum(lens)
        lens[-1] += min(((r - pos) % m) // 2 for m, r in todo)
        lens += [EDGE_SHORTS[si % len(EDGE_SHORTS)], EDGE_LONG]
        si += 1
    rs = np.random.RandomState(seed)
    while True:
        rem = T - sum(lens) - 1                       # the closing 1-token segment
        if rem < 0:
            raise ValueError(f"total_frames {total_frames} is too small for the edge layout")
        nxt = int(rs.randint(128, 513))
        if rem < nxt + 2 * EDGE_LONG + max(EDGE_SHORTS):
            lens[-1] += rem
            break
        lens += [EDGE_SHORTS[si % len(EDGE_SHORTS)], nxt]
        si += 1
    lens.append(1)
    assert sum(lens) == T
    return lens


def ragged_edge_rows(total_frames: int, seed: int = 0):
    """(lens, host float32 rows [T_i, 768]) of ragged_edge_layout(total_frames, seed); hidden states N(0, 0.25) like the bench test's"""
    lens = ragged_edge_layout(total_frames, seed)
    hid = np.random.RandomState(1000 + seed).standard_normal((sum(lens), 768)).astype(np.float32) * np.float32(0.5)
    cut = np.cumsum(lens)[:-1]
    return lens, np.split(hid, cut)

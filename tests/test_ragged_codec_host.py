"""Ragged acoustic decode, the parts that need no GPU: the C ABI's new symbols, workspace sizes and refusals, the packed-segment
offset arithmetic, SlotPool.run's grouped hand-out and SpeechBatcher(ragged_decode=True) on fakes."""
import ctypes as C
import threading
import time

import numpy as np
import pytest
import torch

from chattts_amd import _lib
from chattts_amd.audio import float_to_int16
from chattts_amd.engine import keep_offsets, ragged_offsets, ragged_views
from chattts_amd.serving import SlotPool, SpeechBatcher

NEW_SYMBOLS = ("ctts_codec_ragged_workspace_bytes", "ctts_dvae_decode_ragged", "ctts_vocos_decode_ragged", "ctts_float_to_int16_ragged")


def test_ragged_symbols_are_exported_and_declared():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    import os
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header


def test_ragged_workspace_grows_monotonically():
    lib = _lib.lib()
    f = lib.ctts_codec_ragged_workspace_bytes
    assert f(0, 10) == 0 and f(5, 4) == 0                      # no segment, or fewer tokens than segments: refused
    prev = 0
    for total in (1, 2, 3, 7, 64, 100, 128, 129, 1000, 6144, 6145, 20000):
        n = f(1, total)
        assert n >= prev and n % 256 == 0, (total, n)       # non-decreasing (whole 256-row tiles), growing across a tile boundary
        # at least the padded path's [1, 2T] workspace plus one (lo, hi) pair per mel frame
        assert n >= lib.ctts_codec_workspace_bytes(1, 2 * total) + 2 * total * 8
        prev = n
    assert f(1, 129) > f(1, 128) and f(1, 20000) > f(1, 6145)
    assert f(3, 1000) == f(1, 1000)                           # the table is per frame, not per segment


def test_ragged_offset_arithmetic():
    lens = [1, 2, 7, 40, 512]
    tok, off, koff = ragged_offsets(lens)
    assert tok.dtype == np.int32 and tok.tolist() == [0, 1, 3, 10, 50, 562]
    assert off.dtype == np.int64 and off[-1] == sum(256 * (2 * t - 1) for t in lens)
    assert np.array_equal(np.diff(off), [256 * (2 * t - 1) for t in lens])
    assert np.array_equal(off, 256 * (2 * tok.astype(np.int64) - np.arange(len(lens) + 1)))
    assert np.array_equal(np.diff(koff), [(256 * (2 * t - 1) + 7) // 8 for t in lens])
    assert keep_offsets([0, 1, 9, 17, 24]).tolist() == [0, 1, 2, 3, 4]
    assert keep_offsets([0, 7, 8, 8 + 13]).tolist() == [0, 1, 2, 4]
    flat = np.arange(off[-1])
    views = ragged_views(flat, off)
    assert [v.size for v in views] == [256 * (2 * t - 1) for t in lens] and views[2][0] == off[2]
    assert np.shares_memory(views[1], flat)


def _arr(vals, ctype):
    a = (ctype * len(vals))(*vals)
    return a, C.cast(a, C.c_void_p)


def test_ragged_entry_points_refuse_bad_offsets():
    """n_seg < 1, empty segments, offsets that do not ascend or do not start at 0, a workspace that is too small -- refused before any
    device work (the pointers below are never dereferenced)"""
    lib = _lib.lib()
    fake = C.c_void_p(16)
    for fn in (lib.ctts_dvae_decode_ragged, lib.ctts_vocos_decode_ragged):
        def call(offs, n_seg, ws_bytes=1 << 40):
            keep, p = _arr(offs, C.c_int32)
            return fn(fake, fake, fake, p, n_seg, fake, fake, ws_bytes, None)
        for offs, n_seg, msg in (([0], 0, b"n_seg"), ([0, 3, 3, 5], 3, b"empty"), ([0, 4, 2], 2, b"ascend"), ([1, 4], 1, b"first"),
                                 ([0, 5, 9], 2, b"workspace")):
            rc = call(offs, n_seg, 1 << 40 if msg != b"workspace" else 1024)
            assert rc != 0 and msg in lib.ctts_last_error(), (offs, lib.ctts_last_error())
        assert fn(None, fake, fake, fake, 1, fake, fake, 1 << 40, None) != 0
    f16 = lib.ctts_float_to_int16_ragged
    for offs, n_seg in (([0, 256, 256], 2), ([0, 10, 5], 2), ([3, 10], 1), ([0], 0)):
        keep, p = _arr(offs, C.c_int64)
        assert f16(fake, fake, None, fake, p, n_seg, 0, 1e-5, fake, None) != 0, offs
    keep, p = _arr([0, 8], C.c_int64)
    assert f16(fake, fake, None, fake, p, 1, 2, 1e-5, fake, None) != 0          # product must be 0 or 1


# ---- SlotPool.run(grouped=True) -----------------------------------------------------------------------------------------------
def test_slot_pool_grouped_hand_out():
    outs = [[("a", 1, 2), ("b", 3, 4)], [], [("c", 5, 6)]]
    assert [g for o in outs for g in SlotPool._hand_out(o, True)] == [outs[0], outs[2]]
    assert [x for o in outs for x in SlotPool._hand_out(o, False)] == [("a", 1, 2), ("b", 3, 4), ("c", 5, 6)]


# ---- SpeechBatcher(ragged_decode=True) on fakes --------------------------------------------------------------------------------
class _Params:
    def __init__(self, spk, max_new_token=32):
        self.spk_emb, self.max_new_token = spk, max_new_token


class _Tok:
    spk_emb_ids = 7


class _FakeChat:
    """prompt = the text's bytes; a request's decoded waveform = its hidden rows' first column / 256; "empty" yields no tokens (step 0
    drew EOS); decode_to_pcm16(ragged=True) is what the ragged path calls, once per group"""
    tokenizer = _Tok()

    def __init__(self):
        self.pcm_calls = []
        self.wav_calls = 0

    def normalizer(self, text, norm, homophones, lang):
        return text

    def code_prompt(self, texts, params):
        t = np.frombuffer(texts[0].encode(), dtype=np.uint8).astype(np.int64)
        ids = torch.from_numpy(np.repeat(t[None, :, None], 4, axis=2))
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def prompt_embedding(self, ids, tmask, params, spk_emb_ids):
        return ids[..., :1].float().expand(*ids.shape[:2], 768).clone()

    def decode_to_wavs(self, hids):
        self.wav_calls += 1
        return np.stack([hids[0][:, 0].numpy().astype(np.float32) / 256.0])

    def decode_to_pcm16(self, hids, ragged=False):
        assert ragged
        self.pcm_calls.append(len(hids))
        out = []
        for h in hids:
            assert h.shape[0] > 0
            w = h[:, 0].numpy().astype(np.float32) / 256.0
            out.append(float_to_int16(w[np.abs(w) > np.float32(1e-5)]))
        return out


class _FakePool:
    """S slots; every request completes after 3 chunks; a request whose text is "empty" completes with no tokens.  run(grouped=True)
    hands out the requests of one chunk as one list"""

    def __init__(self, S, lock):
        self.S, self.lock = S, lock
        self.queue, self.active, self.free = [], {}, list(range(S))
        self.grouped_calls = 0

    def submit(self, rid, ids, tmask, max_new_token, *, params, emb):
        self.queue.append((rid, ids, emb))

    def run(self, between=None, grouped=False):
        self.grouped_calls += int(grouped)
        while self.queue or self.active:
            if between is not None:
                between()
            assert self.lock.locked()
            while self.queue and self.free:
                rid, ids, emb = self.queue.pop(0)
                self.active[self.free.pop(0)] = [rid, ids, emb, 0]
            time.sleep(0.002)
            done = []
            for s, a in list(self.active.items()):
                a[3] += 1
                if a[3] >= 3:
                    del self.active[s]
                    self.free.append(s)
                    text = bytes(a[1][:, 0].numpy().astype(np.uint8)).decode()
                    hid = a[2][:0] if text == "empty" else a[2]
                    done.append((a[0], a[1], hid))
            if grouped:
                if done:
                    yield done
            else:
                yield from done


def test_ragged_batcher_groups_a_poll_routes_results_and_isolates_an_empty_result():
    lock = threading.Lock()
    chat = _FakeChat()
    holder = {}
    texts = ["alpha", "empty", "bravo charlie", "delta", "echo"]
    b = SpeechBatcher(chat, 8, lock, make_pool=lambda: holder.setdefault("p", _FakePool(8, lock)), ragged_decode=True)
    try:
        # submitted together: they are admitted in one chunk and finish in one poll
        with lock:
            futs = [(t, b.submit(t, _Params("spk-" + t))) for t in texts]
        for t, f in futs:
            if t == "empty":
                with pytest.raises(RuntimeError, match="no audio"):
                    f.result(timeout=30)
                continue
            w = np.frombuffer(t.encode(), dtype=np.uint8).astype(np.float32) / 256.0
            assert np.array_equal(f.result(timeout=30), float_to_int16(w[np.abs(w) > np.float32(1e-5)])), t   # its own result
        occ = b.occupancy()
        assert occ["ragged_decode"] and occ["completed"] == 4 and occ["failed"] == 1
        assert occ["decoded"] == 4 and occ["decode_calls"] == len(chat.pcm_calls) and sum(chat.pcm_calls) == 4
        assert occ["max_decode_group"] >= 2 and occ["decode_calls"] < 4                   # grouped: fewer decodes than requests
        assert chat.wav_calls == 0 and holder["p"].grouped_calls >= 1
        # the worker still serves after the failure
        assert np.asarray(b.submit("zulu", _Params("z")).result(timeout=30)).size == 4
    finally:
        b.close()
    assert not lock.locked()


def test_batcher_default_still_decodes_each_request_alone():
    lock = threading.Lock()
    chat = _FakeChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: _FakePool(4, lock))
    try:
        with lock:
            futs = [b.submit(t, _Params(t)) for t in ("one", "two", "three")]
        for f in futs:
            f.result(timeout=30)
        occ = b.occupancy()
        assert not occ["ragged_decode"] and occ["decode_calls"] == 3 and occ["max_decode_group"] == 1
        assert chat.pcm_calls == [] and chat.wav_calls == 3
    finally:
        b.close()


EDGE_TOTALS = (1022, 1024, 1026, 12286, 12288, 12290, 40000)


@pytest.mark.parametrize("total", EDGE_TOTALS)
def test_ragged_edge_layout_puts_short_segments_at_every_kernel_edge(total):
    """tests/gpu_util.ragged_edge_layout, the packs of tests/test_gpu_ragged_codec_edges.py: exactly `total` frames; 1-token segments
    first and last; every short length (1, 2, 3, 4, 7 tokens) between two long segments (>= 8 tokens); aligned 32 / 36 / 48 / 64 /
    128 / 256-frame windows holding many boundaries (the 1-token run); boundaries with a long neighbour at frame offsets 0, +2 and
    -2 mod each of those (every boundary is at an even frame, so +-1 is out of reach); deterministic"""
    from tests.gpu_util import EDGE_LONG, EDGE_MODS, EDGE_SHORTS, edge_residues, ragged_edge_layout, ragged_edge_rows
    lens = ragged_edge_layout(total)
    assert lens == ragged_edge_layout(total)
    assert all(isinstance(t, int) and t >= 1 for t in lens) and 2 * sum(lens) == total
    assert lens[0] == 1 and lens[-1] == 1
    for s in EDGE_SHORTS:
        assert any(lens[i] == s and lens[i - 1] >= EDGE_LONG and lens[i + 1] >= EDGE_LONG for i in range(1, len(lens) - 1)), s
    assert EDGE_LONG * 2 > 13
    bnd = 2 * np.cumsum(lens)[:-1]                         # frame offsets of the boundaries between segments
    assert np.all(bnd % 2 == 0)
    for m in EDGE_MODS:
        inside = max(int(np.sum((bnd > j * m) & (bnd < (j + 1) * m))) for j in range(total // m))
        assert inside >= min(m // 2 - 1, 64), (m, inside)  # every other frame of one aligned window is a boundary
        long_nb = {int(bnd[i]) % m for i in range(len(bnd)) if max(lens[i], lens[i + 1]) >= EDGE_LONG}
        for r in edge_residues(m):
            assert r in long_nb, (m, r)
    assert sorted(edge_residues(32)) == [0, 2, 30]
    ones = max(len(run) for run in "".join("1" if t == 1 else "." for t in lens).split("."))
    assert ones >= 64
    lens2, rows = ragged_edge_rows(total)
    assert lens2 == lens and [r.shape for r in rows] == [(t, 768) for t in lens] and rows[0].dtype == np.float32
    if total >= 12288:
        assert max(lens) >= 128                            # long segments of the bench's utterance lengths

"""Streamed IMA ADPCM, the parts that need no GPU: the cutting rule over every carry, the NumPy twin over every signal and cut of
tests/adpcm_stream_cases.py against the one-shot encoder, the open-ended header through `parse_wav` and `audio.load_wav`, the new symbols,
and every refusal of ctts_adpcm_stream_step.  Everything is exact."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from chattts_amd import _lib, adpcm, audio
from tests import adpcm_stream_cases as SC


# ---- 1. the cutting rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (8000, 16000, 24000, 48000))
def test_stream_plan_over_every_carry(rate):
    S = adpcm.samples_per_block(rate)
    for final in (False, True):
        for carry in (0, 1, 2, S // 2, S - 2, S - 1):
            for n in (0, 1, 2, S - carry - 1, S - carry, S - carry + 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 12000, 70 * S + 3):
                if n < 0:
                    continue
                blocks, held = adpcm.stream_plan(carry, n, final, rate)
                avail = carry + n
                if final:
                    assert (blocks, held) == ((avail + S - 1) // S, 0), (carry, n)
                else:
                    assert (blocks, held) == (avail // S, avail % S) and blocks * S + held == avail, (carry, n)
                assert blocks * adpcm.align(rate) <= adpcm.stream_bound(n, rate), (carry, n, final)
    assert adpcm.stream_plan(0, 0, True, rate) == (0, 0) and adpcm.stream_plan(S - 1, 0, True, rate) == (1, 0)
    assert adpcm.stream_plan(S - 1, 1, False, rate) == (1, 0) and adpcm.stream_plan(S - 2, 1, False, rate) == (0, S - 1)
    assert adpcm.stream_bound(0, rate) == adpcm.align(rate) and adpcm.stream_bound(1, rate) == adpcm.align(rate)
    assert adpcm.stream_bound(2, rate) == 2 * adpcm.align(rate)                          # S - 1 carried, 2 more: S + 1 samples, final
    for bad in ((S, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            adpcm.stream_plan(*bad, False, rate)
    with pytest.raises(ValueError):
        adpcm.stream_plan(0, 1, False, 0)


def test_the_lag_of_a_stream_is_what_the_docstring_says():
    for rate, ms in ((8000, 63.0), (16000, 31.5), (24000, 42.3), (48000, 42.5)):
        assert round((adpcm.samples_per_block(rate) - 1) * 1000.0 / rate, 1) == ms
        assert f"{ms:g} ms at {rate // 1000} kHz" in adpcm.__doc__


# ---- 2. the twin against the one-shot encoder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", SC.RATES)
@pytest.mark.parametrize("name", SC.SIGNALS)
def test_twin_equals_the_one_shot_encoder_over_every_cut(name, rate):
    """push by push: the twin's chunk is the one-shot encoder's blocks that the cutting rule deals to that push"""
    x = SC.signal(name, rate)
    A, S = adpcm.align(rate), adpcm.samples_per_block(rate)
    for cut, lens in SC.cuts(rate).items():
        want = SC.reference(name, rate, cut)
        enc = adpcm.StreamEncoder(rate)
        carry, got = 0, []
        for w, (lo, hi, final) in zip(want, SC.pushes(lens)):
            c = enc.push(x[lo:hi], final)
            blocks, carry = adpcm.stream_plan(carry, hi - lo, final, rate)
            assert c.dtype == np.uint8 and c.size == A * blocks and c.size <= adpcm.stream_bound(hi - lo, rate), (cut, lo, hi)
            assert np.array_equal(c, w), (cut, lo, hi)
            assert len(enc.held) == carry
            got.append(c)
        n = sum(lens)
        got = np.concatenate(got)
        assert got.size == adpcm.n_blocks(n, rate) * A
    cut = "every_path"                                     # once against the one-shot encoder outright, and through the decoder
    n = sum(SC.cuts(rate)[cut])
    blob, trace = adpcm.encode_blocks(x[:n], rate, trace=True)
    got = np.concatenate(SC.reference(name, rate, cut))
    assert np.array_equal(got, blob) and np.array_equal(adpcm.decode_blocks(got, n, rate), trace[:n])
    assert np.array_equal(adpcm.decode_blocks(got, len(trace), rate), trace)               # the padding: the coder goes on towards x[n - 1]


def test_the_pushes_that_emit_and_the_ones_that_wait():
    rate = 8000
    S = adpcm.samples_per_block(rate)
    enc = adpcm.StreamEncoder(rate)
    x = SC.signal("noise", rate)
    got = [enc.push(x[lo:hi], final).size // 256 for lo, hi, final in SC.pushes(SC.cuts(rate)["every_path"])]
    assert got == [0, 0, 1, 0, 0, 1, 1, 2, 3, 1]           # 0; 1 waits; S - 1 more: a block; 1 waits; 0; S: a block, 1 waits; ...
    assert [c.size for c in SC.reference("noise", rate, "one_block_then_nothing")] == [0, 256, 0]
    assert [c.size for c in SC.reference("noise", rate, "no_samples")] == [0, 0]
    assert [c.size for c in SC.reference("noise", rate, "block_reached_by_ones")] == [0, 0, 256, 256]
    enc = adpcm.StreamEncoder(rate)
    enc.push(np.zeros(3, np.int16), True)
    with pytest.raises(ValueError, match="last push"):
        enc.push(np.zeros(1, np.int16))
    with pytest.raises(ValueError, match="int16"):
        adpcm.StreamEncoder(rate).push(np.zeros(3, np.float32))
    assert S == 505


# ---- 3. the open-ended header -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", SC.RATES)
def test_stream_header_round_trips_and_an_over_count_still_raises(rate):
    h = adpcm.stream_header(rate)
    ref = adpcm.wav_header(1, rate)
    assert len(h) == 60 == adpcm.HEADER_BYTES
    assert [i for i in range(60) if h[i] != ref[i]] == [4, 5, 6, 7, 48, 49, 50, 51, 56, 57, 58, 59]
    assert h[4:8] == h[48:52] == h[56:60] == b"\xFF" * 4
    S = adpcm.samples_per_block(rate)
    n = 2 * S + 9
    x = SC.signal("noise", rate)[:n]
    blocks, trace = adpcm.encode_blocks(x, rate, trace=True)
    y, r = adpcm.parse_wav(h + blocks.tobytes())
    assert r == rate and len(y) == 3 * S and np.array_equal(y, trace)                      # every whole block that follows
    assert np.array_equal(y[:n], adpcm.decode_blocks(blocks, n, rate))
    y2, _ = adpcm.parse_wav(h + blocks.tobytes() + b"\x00" * 100)                          # a torn last block is not read
    assert np.array_equal(y2, y)
    f, r = audio.load_wav(h + blocks.tobytes(), adpcm=True)
    assert r == rate and np.array_equal(f, (y.astype(np.float64) / 32768.0).astype(np.float32))
    with pytest.raises(ValueError, match="no samples"):
        adpcm.parse_wav(h)
    whole = bytearray(adpcm.encode(x, rate))
    for fact in (3 * S + 1, 0xFFFFFFFE, 1 << 31):
        whole[48:52] = struct.pack("<I", fact)
        with pytest.raises(ValueError, match="`fact` chunk counts"):
            adpcm.parse_wav(bytes(whole))
    whole[48:52] = struct.pack("<I", 0xFFFFFFFF)                                           # open-ended `fact`, a closed `data` chunk
    assert len(adpcm.parse_wav(bytes(whole))[0]) == 3 * S
    with pytest.raises(ValueError):
        adpcm.stream_header(0)


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------------------
def _pushes(rows):
    """rows (start, n, rate, slot, carry, flags, count_idx[, stage, block0, byte0]) -> a ctts_adpcm_push table with the running sums"""
    tab = np.zeros(len(rows), _lib.ADPCM_PUSH)
    stage = blocks = nbytes = 0
    for i, r in enumerate(rows):
        start, n, rate, slot, carry, flags, ci = r[:7]
        tab[i] = (start, n, r[7] if len(r) > 7 else stage, r[8] if len(r) > 8 else blocks, r[9] if len(r) > 9 else nbytes, rate, slot,
                  carry, flags, ci, 0)
        A = 256 * max(1, rate // 11025)
        S = 2 * (A - 4) + 1
        cap = max(carry + n, 0)
        nb = (cap + S - 1) // S if flags & 1 else cap // S
        stage += (cap + 7) // 8 * 8
        blocks += nb
        nbytes += nb * A
    return tab


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in ("ctts_adpcm_stream_sizes", "ctts_adpcm_stream_step"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "} ctts_adpcm_push;        /* 64 bytes */" in header and _lib.ADPCM_PUSH.itemsize == 64
    names = ("start", "n", "stage", "block0", "byte0", "rate", "slot", "carry", "flags", "count_idx", "reserved")
    assert [_lib.ADPCM_PUSH.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    assert "int64_t start, n;" in header and "int64_t stage;" in header and "int64_t block0, byte0;" in header
    assert "int32_t rate, slot, carry, flags;" in header and "int32_t count_idx, reserved;" in header
    sizes = (C.c_int64 * 4)()
    # 504 carried + 507 at 8 kHz, not final: 2 blocks, 1 held; a final push of nothing onto nothing; 2040 + 2 at 48 kHz, final: 2 blocks
    tab = _pushes([(0, 507, 8000, 0, 504, 0, -1), (512, 0, 24000, 1, 0, 1, -1), (512, 2, 48000, 2, 2040, 1, -1)])
    assert lib.ctts_adpcm_stream_sizes(tab.ctypes.data_as(C.c_void_p), 3, 4, 600, sizes) == 0, lib.ctts_last_error()
    assert list(sizes)[:2] == [4, 2 * 256 + 2 * 1024] and sizes[3] == 1016 + 0 + 2048
    assert sizes[2] >= 16 * 3 + 48 * 3 + 2 * sizes[3] and sizes[2] % 16 == 0
    assert sizes[1] <= adpcm.stream_bound(507, 8000) + adpcm.stream_bound(0, 24000) + adpcm.stream_bound(2, 48000)


def test_stream_step_refuses_bad_tables_without_a_device():
    """every refusal comes from the host table before anything is launched: the pointers below are never dereferenced, and the message
    names the refusal"""
    lib = _lib.lib()
    pcm, out, work, state = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 16)

    def call(rows, n_push=None, pcm=pcm, out=out, work=work, state=state, dev=C.c_void_p(4096), host=True, counts=None, mask=None,
             n_slots=8, n_pcm=1 << 16, out_bytes=1 << 20, work_bytes=1 << 20):
        tab = _pushes(rows)
        return lib.ctts_adpcm_stream_step(pcm, n_pcm, mask, counts, dev, tab.ctypes.data_as(C.c_void_p) if host else None,
                                          len(rows) if n_push is None else n_push, state, n_slots, out, out_bytes, work, work_bytes, None)

    def why():
        return lib.ctts_last_error()
    ok = (0, 100, 24000, 0, 0, 0, -1)
    for kw in (dict(pcm=None), dict(out=None), dict(dev=None), dict(host=False), dict(work=None), dict(state=None)):
        assert call([ok], **kw) != 0 and b"null" in why(), kw
    assert call([(0, 100, 24000, 0, 0, 1, 0)]) != 0 and b"null" in why() and b"counts" in why()
    assert call([(0, 100, 24000, 0, 0, 3, -1)]) != 0 and b"null" in why() and b"mask" in why()
    assert call([ok], n_push=0) != 0 and b"n_push" in why()
    assert call([(8 * i, 8, 24000, i, 0, 0, -1) for i in range(1025)], n_slots=2048) != 0 and b"1024" in why()
    for slot in (-1, 8, 1 << 20):
        assert call([(0, 100, 24000, slot, 0, 0, -1)]) != 0 and b"outside the pool" in why(), slot
    assert call([ok, (104, 100, 24000, 1, 0, 0, -1), (208, 10, 8000, 0, 0, 0, -1)]) != 0 and b"twice" in why()
    for start in (4, 7, 9, 1001, -8):
        assert call([(start, 10, 24000, 0, 0, 0, -1)]) != 0 and b"multiples of 8" in why(), start
    assert call([(8, -1, 24000, 0, 0, 0, -1)]) != 0 and b"negative" in why()
    assert call([(8, 1 << 31, 24000, 0, 0, 0, -1)], n_pcm=1 << 33) != 0 and b"beyond" in why()
    assert call([(65536 - 8, 9, 24000, 0, 0, 0, -1)]) != 0 and b"beyond" in why()                    # one sample past pcm
    for rate in (0, -1, -(1 << 31)):
        assert call([(0, 8, rate, 0, 0, 0, -1)]) != 0 and b"positive rate" in why(), rate
    for rate in (55125, 96000, (1 << 31) - 1):
        assert call([(0, 8, rate, 0, 0, 0, -1)]) != 0 and b"slot" in why() and b"55125" in why(), rate
    for rate, carry in ((8000, -1), (8000, 505), (24000, 1017), (48000, 2041), (11024, 505), (11025, 505), (55124, 2041)):
        assert call([(0, 8, rate, 0, carry, 0, -1)]) != 0 and b"carries" in why(), (rate, carry)
    sizes = (C.c_int64 * 4)()
    for rate, carry in ((8000, 504), (24000, 1016), (48000, 2040), (55124, 2040)):                    # the most a slot holds: the table passes
        assert lib.ctts_adpcm_stream_sizes(_pushes([(0, 8, rate, 0, carry, 0, -1)]).ctypes.data_as(C.c_void_p), 1, 8, 100, sizes) == 0, why()
    assert call([(0, 8, 24000, 0, 0, 4, -1)]) != 0 and b"flag" in why()
    for ci in (-2, 65536):
        assert call([(0, 8, 24000, 0, 0, 1, ci)], counts=C.c_void_p(1 << 12)) != 0 and b"count_idx" in why(), ci
    assert call([(0, 8, 24000, 0, 0, 0, 0)], counts=C.c_void_p(1 << 12)) != 0 and b"not final" in why() and b"count_idx" in why()
    assert call([(0, 8, 24000, 0, 0, 2, -1)], mask=C.c_void_p(1 << 12)) != 0 and b"not final" in why() and b"mask" in why()
    assert call([(0, 8, 24000, 0, 0, 0, -1, 8, 0, 0)]) != 0 and b"stage" in why()
    assert call([(0, 8, 24000, 0, 0, 0, -1, 0, 1, 0)]) != 0 and b"block0" in why()
    assert call([(0, 8, 24000, 0, 0, 0, -1, 0, 0, 512)]) != 0 and b"byte0" in why()
    assert call([(0, 1017, 24000, 0, 0, 0, -1, 0, 0, 0), (1024, 8, 24000, 1, 0, 0, -1, 1024, 2, 512)]) != 0 and b"block0" in why()
    assert call([(0, 1017, 24000, 0, 0, 0, -1, 0, 0, 0), (1024, 8, 24000, 1, 0, 0, -1, 1024, 1, 1024)]) != 0 and b"byte0" in why()
    assert call([(0, 1017, 24000, 0, 0, 0, -1)], out_bytes=511) != 0 and b"out of capacity" in why() and b"out holds" in why()
    assert call([(0, 1017, 24000, 0, 0, 0, -1)], work_bytes=64 + 2 * 1024 - 1) != 0 and b"out of capacity" in why() and b"work holds" in why()
    assert call([ok], pcm=C.c_void_p((1 << 20) + 2)) != 0 and b"aligned" in why()
    assert call([ok], out=C.c_void_p((1 << 24) + 8)) != 0 and b"aligned" in why()
    assert call([ok], work=C.c_void_p((1 << 28) + 8)) != 0 and b"aligned" in why()
    assert call([ok], dev=C.c_void_p(4100)) != 0 and b"aligned" in why()
    assert call([(0, 8, 24000, 0, 0, 1, 0)], counts=C.c_void_p((1 << 12) + 4)) != 0 and b"aligned" in why()
    assert call([ok], out=pcm) != 0 and b"aliases" in why()
    assert call([ok], out=C.c_void_p((1 << 20) + 64)) != 0 and b"aliases" in why()
    assert call([ok], out=C.c_void_p((1 << 20) - 64), out_bytes=128) != 0 and b"aliases" in why()
    sizes = (C.c_int64 * 4)()
    assert lib.ctts_adpcm_stream_sizes(None, 1, 8, 100, sizes) != 0 and b"null" in why()
    assert lib.ctts_adpcm_stream_sizes(_pushes([ok]).ctypes.data_as(C.c_void_p), 1, 8, 100, None) != 0 and b"null" in why()
    assert lib.ctts_adpcm_stream_sizes(_pushes([ok]).ctypes.data_as(C.c_void_p), 1, 8, 99, sizes) != 0 and b"beyond" in why()
    # streams that hold and get nothing launch nothing, and say so by succeeding on pointers no kernel could touch
    assert call([(0, 0, 24000, 0, 0, 1, -1), (8, 0, 8000, 3, 0, 0, -1)]) == 0


# ---- 5. Chat, the batcher and the endpoint on fakes ---------------------------------------------------------------------------------------
def test_infer_refuses_a_streamed_adpcm_without_the_option_and_with_what_does_not_go_with_it():
    from chattts_amd.core import Chat
    chat = Chat()
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True)
    with pytest.raises(ValueError, match="split_text"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True, stream_adpcm=True)
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(["x"], adpcm=True, stream=True, stream_adpcm=True, split_text=False)
    with pytest.raises(ValueError, match="encoding"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True, stream_adpcm=True, split_text=False, encoding="ulaw")
    with pytest.raises(ValueError, match="flac"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True, stream_adpcm=True, split_text=False, flac=True, stream_flac=True)
    with pytest.raises(ValueError, match="use_decoder"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True, stream_adpcm=True, split_text=False, use_decoder=False)
    with pytest.raises(ValueError, match="55125"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True, stream_adpcm=True, split_text=False, sample_rate=96000, stream_resample=True)


class _AdpcmCodec:
    """the ADPCM streams of a fake engine: the host twin behind the engine's handles"""

    def __init__(self):
        self.enc, self.opened, self.closed = {}, [], []

    def adpcm_stream_open(self, rate):
        h = len(self.opened)
        self.opened.append((h, rate))
        self.enc[h] = adpcm.StreamEncoder(rate)
        return h

    def adpcm_stream_close(self, h):
        del self.enc[h]
        self.closed.append(h)

    def adpcm_streams_in_use(self):
        return len(self.enc)


def _fake_chat():
    from tests.test_g711_host import _EncChat
    from tests.test_stream_pool_host import _piece

    class _StreamAdpcmChat(_EncChat):
        """as _EncChat; a flagged window's piece is pushed into its stream of the fake engine and comes back as that push's blocks"""

        def __init__(self):
            super().__init__()
            self.codec = _AdpcmCodec()

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            flags = kw.get("adpcm", [False] * len(windows))
            hs = kw.get("adpcm_streams", [None] * len(windows))
            out = []
            for (slot, prefix, a, b, tail), f, h in zip(windows, flags, hs):
                p = _piece(store[slot], prefix, a, b)
                out.append(self.codec.enc[h].push(p, bool(tail)) if f else p)
            return out
    return _StreamAdpcmChat()


def test_adpcm_streams_due_at_one_poll_share_one_call_and_free_their_slots():
    import threading
    import time

    from chattts_amd.serving import SpeechBatcher
    from chattts_amd.serving import StreamSpec, stream_schedule
    from tests.test_stream_pool_host import _FakePool, _Params, _piece
    lock = threading.Lock()
    chat = _fake_chat()
    holder = {}
    off = SpeechBatcher(chat, 3, lock, make_pool=lambda: _FakePool(3, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="stream_adpcm=True"):
            off.submit_stream("x", _Params(48), adpcm_blocks=True)                           # without the option: refused
        with pytest.raises(TypeError):
            off.submit_stream("x", _Params(48), adpcm=True)                                  # the file's keyword is no stream's
        assert "stream_adpcm_chunks" not in off.occupancy()
    finally:
        off.close()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_adpcm=True,
                      stream_flac=True)
    try:
        with pytest.raises(ValueError, match="encoding"):
            b.submit_stream("x", _Params(48), adpcm_blocks=True, encoding="ulaw")
        with pytest.raises(ValueError, match="flac"):
            b.submit_stream("x", _Params(48), adpcm_blocks=True, flac=True)
        with pytest.raises(ValueError, match="55125"):
            b.submit_stream("x", _Params(48), adpcm_blocks=True, sample_rate=96000)
        with lock:       # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = {"A": b.submit_stream("A", _Params(96), adpcm_blocks=True), "B": b.submit_stream("B", _Params(96)),
                       "C": b.submit_stream("C", _Params(96), adpcm_blocks=True, sample_rate=8000)}
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in streams.items()]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        sched = stream_schedule([], 96, True, StreamSpec(24, 12000, 0))
        for tag, rate in (("A", 24000), ("B", None), ("C", 8000)):
            want = [_piece(ord(tag), p, lo, hi) for p, lo, hi, _ in sched]
            assert len(got[tag]) == len(want), tag
            if rate is None:
                assert all(g.dtype == np.int16 and np.array_equal(g, w) for g, w in zip(got[tag], want))
                continue
            assert all(g.dtype == np.uint8 and g.size % adpcm.align(rate) == 0 for g in got[tag])
            assert np.array_equal(np.concatenate(got[tag]), adpcm.encode_blocks(np.concatenate(want), rate))   # the PCM stream's samples
        polls = sorted({p for p, _, _, _ in sched})
        assert len(chat.window_calls) == len(polls) < len(sched)                             # one call per poll for the three streams
        for w, kw in zip(chat.window_calls, chat.kw_calls):
            slots = [x[0] for x in w]
            assert kw["adpcm"] == [s != 1 for s in slots] and kw["sample_rates"] == [8000 if s == 2 else 24000 for s in slots]
            assert [h is not None for h in kw["adpcm_streams"]] == kw["adpcm"] and set(kw) == {"adpcm", "adpcm_streams", "sample_rates"}
        assert sorted(chat.codec.opened) == [(0, 24000), (1, 8000)]
        deadline = time.time() + 10
        while chat.codec.adpcm_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.adpcm_streams_in_use() == 0 and sorted(chat.codec.closed) == [0, 1]
        occ = b.occupancy()
        assert occ["stream_adpcm_chunks"] == 2 * len(sched) and occ["completed"] == 3 and "adpcm_encoded" not in occ
        assert occ["stream_flac_chunks"] == 0
        s = b.submit_stream("D", _Params(400), adpcm_blocks=True)                            # cancelled mid-stream: its slot is freed
        first = next(s)
        s.close()
        assert first.dtype == np.uint8 and list(s) == []
        deadline = time.time() + 10
        while chat.codec.adpcm_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.adpcm_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1
        n_calls = len(chat.kw_calls)
        assert sum(len(c) for c in b.submit_stream("E", _Params(48))) == 256 * 95            # no flag: today's call, no keyword
        assert all(kw == {} for kw in chat.kw_calls[n_calls:])
    finally:
        b.close()
    assert not lock.locked()


def test_endpoint_streams_adpcm_only_with_the_option():
    import threading

    from starlette.testclient import TestClient

    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    full = np.arange(600, dtype=np.int16)                                                    # what _EndpointChat hands out

    class _Chat(_EndpointChat):
        def infer(self, text, stream=False, **kw):
            out = super().infer(text, stream, **kw)
            if not kw.get("adpcm"):
                return out
            if not stream:
                return [np.frombuffer(adpcm.encode(w, kw.get("sample_rate", 24000)), np.uint8) for w in out]
            assert kw["stream_adpcm"] is True and kw["split_text"] is False
            enc = adpcm.StreamEncoder(kw.get("sample_rate", 24000))
            chunks = list(out)
            return ([enc.push(c[0], i == len(chunks) - 1)] for i, c in enumerate(chunks))

    class _Batcher:
        streams, refine, stream_adpcm = True, False, True

        def __init__(self):
            self.lock, self.calls = threading.Lock(), []

        def submit_stream(self, text, params, **kw):
            self.calls.append(("stream", text, kw))
            enc = adpcm.StreamEncoder(kw.get("sample_rate", 24000))
            parts = [full[:10], full[10:10], full[10:250]]
            outer = self

            class _It:
                def __init__(self):
                    self.it = iter([enc.push(p, i == 2) if kw.get("adpcm_blocks") else p for i, p in enumerate(parts)])

                def __iter__(self):
                    return self

                def __next__(self):
                    return next(self.it)

                def close(self):
                    outer.calls.append(("closed",))
            return _It()

        def occupancy(self):
            return {}
    chat = _Chat()
    body = {"input": "hello", "response_format": "adpcm", "stream": True}
    with TestClient(server.create_app(chat, adpcm=True)) as c:                               # option off: today's 400
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "non-streamed" in r.text and "block's samples" in r.text and not chat.calls
        assert "stream_adpcm" not in c.get("/health").json()
    with TestClient(server.create_app(chat, stream_adpcm=True)) as c:                        # without adpcm the format does not exist
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "Unsupported audio format: adpcm" in r.text and "stream_adpcm" not in c.get("/health").json()
    with TestClient(server.create_app(chat, adpcm=True, stream_adpcm=True, stream_sample_rates=(8000,), g711=True)) as c:
        assert c.get("/health").json()["stream_adpcm"] is True
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content[:60] == adpcm.stream_header(24000)
        y, rate = adpcm.parse_wav(r.content)
        n = len(r.content) - 60
        assert rate == 24000 and n % 512 == 0 and n > 0 and chat.calls[-1][1] is True and chat.calls[-1][2]["adpcm"] is True
        file = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm"}).content      # the file, as before
        assert "stream_adpcm" not in chat.calls[-1][2] and file[60:] == r.content[60:]                        # the same blocks
        x, _ = adpcm.parse_wav(file)
        trace = adpcm.encode_blocks(full, 24000, trace=True)[1]
        assert len(x) == 600 and np.array_equal(y[:600], x) and np.array_equal(y, trace) and len(y) == 1017   # the padding follows
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        y8, rate = adpcm.parse_wav(r.content)
        assert r.status_code == 200 and rate == 8000 and r.content[:60] == adpcm.stream_header(8000)
        assert chat.calls[-1][2]["stream_resample"] is True and chat.calls[-1][2]["stream_adpcm"] is True
        n_calls = len(chat.calls)
        r = c.post("/v1/audio/speech", json={**body, "encoding": "ulaw"})
        assert r.status_code == 400 and "ncoding" in r.text and len(chat.calls) == n_calls
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "stream": True})     # no adpcm: today's call
        assert "adpcm" not in chat.calls[-1][2] and "stream_adpcm" not in chat.calls[-1][2]
    chat, bat = _Chat(), _Batcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, adpcm=True, stream_adpcm=True, stream_sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content[:60] == adpcm.stream_header(8000)
        blocks, trace = adpcm.encode_blocks(full[:250], 8000, trace=True)
        assert r.content[60:] == blocks.tobytes() and not chat.calls
        y, rate = adpcm.parse_wav(r.content)
        assert rate == 8000 and np.array_equal(y, trace) and len(y) == 505
        assert bat.calls[-2:] == [("stream", "hello", {"sample_rate": 8000, "adpcm_blocks": True}), ("closed",)]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "stream": True})
        assert r.content == full[:250].tobytes() and bat.calls[-2] == ("stream", "hello", {})

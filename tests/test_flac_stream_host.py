"""Streamed FLAC, the parts that need no GPU: the cutting rule over every carry and length, the variable-block-size header at the
boundaries of the coded sample number, the NumPy twin through the independent stream decoder (tests/flac_stream_oracle.py) over every
signal and cut of tests/flac_stream_cases.py, the new symbols, and every refusal of ctts_flac_stream_step."""
import ctypes as C
import os

import numpy as np
import pytest

from chattts_amd import _lib, flac
from tests import flac_cases as FC
from tests import flac_oracle
from tests import flac_stream_cases as SC
from tests import flac_stream_oracle as SO


# ---- 1. the cutting rule --------------------------------------------------------------------------------------------------------------
def test_stream_plan_over_every_carry_and_length():
    for final in (False, True):
        for carry in range(16):
            for n_in in range(8233):
                blocks, held = flac.stream_plan(carry, n_in, final)
                avail = carry + n_in
                assert sum(blocks) + held == avail and 0 <= held <= 15, (carry, n_in, final)
                assert all(b == 4096 for b in blocks[:-1]) and all(1 <= b <= 4096 for b in blocks[-1:]), (carry, n_in, final)
                if final:
                    assert held == 0
                else:
                    assert all(16 <= b for b in blocks) and held == (avail if avail < 16 else avail % 4096 if avail % 4096 < 16 else 0)
    assert flac.stream_plan(15, 1, False) == ([16], 0) and flac.stream_plan(14, 1, False) == ([], 15)
    assert flac.stream_plan(15, 0, True) == ([15], 0) and flac.stream_plan(0, 0, True) == ([], 0)
    assert flac.stream_plan(0, 4111, False) == ([4096], 15) and flac.stream_plan(0, 4112, False) == ([4096, 16], 0)
    for bad in ((16, 0), (-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            flac.stream_plan(*bad, False)


def test_stream_bound_holds_and_fits_the_kernels_frame_buffer():
    """a frame is at most 16 bytes of header, the subframe's byte, 2 n bytes and the CRC-16; the kernel packs a frame into FLAC_WORDS
    words of LDS, and its store loop and the CRC's second word reach one word beyond the frame"""
    for n_in in (0, 1, 15, 16, 4081, 4082, 4096, 8192, 100000):
        worst = 0
        for carry in range(16):
            for final in (False, True):
                blocks, _ = flac.stream_plan(carry, n_in, final)
                worst = max(worst, sum(19 + 2 * b for b in blocks))
        assert worst <= flac.stream_bound(n_in), n_in
    src = open(os.path.join(_lib.HERE, "csrc", "flac.hip")).read()
    assert "#define FLAC_WORDS (FLAC_BLOCK / 2 + 8)" in src
    words = 4096 // 2 + 8
    longest = max(len(flac.frame_header_variable((1 << 36) - 1, n, 65535)) + 1 + 2 * n + 2 for n in (4095, 4096))
    assert longest == 8209 and (longest + 3) // 4 + 1 <= words


# ---- 2. the header ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [0, (1 << 7) - 1, (1 << 7) + 1, 1 << 11, 1 << 16, 1 << 21, 1 << 26, (1 << 31) - 1, 1 << 31, (1 << 36) - 1])
def test_variable_header_at_the_boundaries_of_the_sample_number(sample):
    want_len = 1 if sample < 1 << 7 else 2 if sample < 1 << 11 else 3 if sample < 1 << 16 else 4 if sample < 1 << 21 else \
        5 if sample < 1 << 26 else 6 if sample < 1 << 31 else 7
    for n, rate in ((4096, 24000), (17, 11025), (1, 65535), (4095, 8000)):
        h = flac.frame_header_variable(sample, n, rate)
        assert h[:2] == b"\xFF\xF9" and len(h) == 4 + want_len + (2 if n != 4096 else 0) + (2 if rate not in flac.RATE_CODES else 0) + 1
        assert h[2] >> 4 == (0xC if n == 4096 else 0x7) and h[3] == 0x08
        got = SO.read_header(h + b"\x00" * 8)
        assert got == dict(sample=sample, n=n, rate=rate, end=len(h))
        assert h[-1] == flac_oracle._crc8(h[:-1])
    if want_len == 7:
        assert flac.frame_header_variable(sample, 4096, 24000)[4] == 0xFE
    with pytest.raises(flac_oracle.FlacError):
        SO.read_header(flac.frame_header(0, 4096, 24000) + b"\x00" * 8)           # FF F8: the file encoder's frames are no stream's


def test_header_refusals_and_the_stream_header():
    for bad in (-1, 1 << 36):
        with pytest.raises(ValueError, match="36 bits"):
            flac.frame_header_variable(bad, 16, 24000)
        with pytest.raises(ValueError, match="36 bits"):
            flac.StreamEncoder(24000, bad)
    for n in (0, 4097):
        with pytest.raises(ValueError):
            flac.frame_header_variable(0, n, 24000)
    with pytest.raises(ValueError, match="sample rate"):
        flac.stream_header(70000)
    h = flac.stream_header(11025)
    assert len(h) == 42 == flac.HEADER_BYTES and h[:8] == b"fLaC\x80\x00\x00\x22" and h[8:12] == bytes([0x00, 0x10, 0x10, 0x00])
    assert h[12:18] == bytes(6) and h[18:26] == bytes([0x02, 0xB1, 0x10, 0xF0, 0, 0, 0, 0]) and h[26:] == bytes(16)
    enc = flac.StreamEncoder(24000, (1 << 36) - 100)
    assert enc.push(np.zeros(50, np.int16)) != b""
    with pytest.raises(ValueError, match="2\\^36"):
        enc.push(np.zeros(50, np.int16))
    assert enc.push(np.zeros(49, np.int16), True) != b""
    with pytest.raises(ValueError, match="last push"):
        enc.push(np.zeros(1, np.int16))


# ---- 3. the twin through the independent decoder ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.SIGNALS)
def test_twin_round_trip_over_every_cut(name):
    x = SC.signal(name)
    rate = FC.RATES[FC.SIGNALS.index(name) % len(FC.RATES)]
    for cut in SC.CUTS:
        chunks = SC.reference(name, rate, cut)
        pushes = SC.pushes(cut)
        n = pushes[-1][1]
        facts = SC.check_stream(chunks, rate, x[:n])
        assert sum(facts["blocks"]) == n and all(16 <= b <= 4096 for b in facts["blocks"][:-1])
        assert all(len(c) <= flac.stream_bound(hi - lo) for c, (lo, hi, _) in zip(chunks, pushes)), cut
    lens, last = SC.CUTS["carry_reaches_16"]
    got = [len(c) > 0 for c in SC.reference(name, rate, "carry_reaches_16")]
    assert got[:6] == [False, False, True, False, False, True]                 # 1, 14 wait; 1 more: a block of 16; 0; 15 waits; 16 more: 31
    assert SC.reference(name, rate, "no_samples") == (b"",) and SC.reference(name, rate, "empty_pushes_only") == (b"", b"", b"")
    assert [len(c) > 0 for c in SC.reference(name, rate, "final_empty_carry_15")] == [False, True]


def test_the_decoded_samples_do_not_depend_on_the_cut_and_the_first_sample_moves_the_numbers():
    x = SC.signal("ar2")
    first = (1 << 31) - 4100
    enc = flac.StreamEncoder(48000, first)
    chunks = [enc.push(x[:5000]), enc.push(x[5000:5010]), enc.push(x[5010:], True)]
    assert chunks[0] and not chunks[1] and chunks[2]
    facts = SC.check_stream(chunks, 48000, x, first_sample=first)
    assert facts["numbers"][0] == first and facts["numbers"][1] == first + 4096 and facts["numbers"][-1] > 1 << 31
    with pytest.raises(flac_oracle.FlacError, match="was due"):
        SO.decode(flac.stream_header(48000) + b"".join(chunks), first_sample=0)
    with pytest.raises(flac_oracle.FlacError, match="was due"):
        SO.decode(flac.stream_header(48000) + chunks[2], first_sample=first)                  # a lost chunk shows
    file_y, _ = flac_oracle.decode(flac.encode(x, 48000))
    assert np.array_equal(file_y, x)
    bad = bytearray(flac.stream_header(48000) + chunks[0])
    bad[60] ^= 1
    with pytest.raises(flac_oracle.FlacError):
        SO.decode(bytes(bad), first_sample=first)


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------------------------
def _pushes(rows):
    """rows (start, n, rate, slot, carry, flags, count_idx, sample[, stage, frame0]) -> a ctts_flac_push table with the running sums"""
    tab = np.zeros(len(rows), _lib.FLAC_PUSH)
    stage = slots = 0
    for i, r in enumerate(rows):
        start, n, rate, slot, carry, flags, ci, sample = r[:8]
        tab[i] = (start, n, sample, r[8] if len(r) > 8 else stage, r[9] if len(r) > 9 else slots, rate, slot, carry, flags, ci, 0)
        stage += (max(carry + n, 0) + 7) // 8 * 8
        slots += (max(carry + n, 0) + 4095) // 4096
    return tab


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in ("ctts_flac_stream_sizes", "ctts_flac_stream_step"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "} ctts_flac_push;" in header and _lib.FLAC_PUSH.itemsize == 64
    names = ("start", "n", "sample", "stage", "frame0", "rate", "slot", "carry", "flags", "count_idx", "reserved")
    assert [_lib.FLAC_PUSH.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    sizes = (C.c_int64 * 4)()
    tab = _pushes([(0, 4097, 24000, 0, 15, 0, -1, 0), (4104, 0, 8000, 1, 0, 1, -1, 5), (4104, 10, 11025, 2, 3, 0, -1, 0)])
    assert lib.ctts_flac_stream_sizes(tab.ctypes.data_as(C.c_void_p), 3, 4, 5000, sizes) == 0, lib.ctts_last_error()
    assert list(sizes)[:2] == [3, 2 * 4112 + 2 * 19 + 2 * 13 + 19] and sizes[3] == 4112 + 0 + 16
    assert sizes[2] >= 8 * (3 + 1 + 9) + 3 * 32 + 3 * 96 + 2 * sizes[3] and sizes[2] % 16 == 0
    assert sizes[1] >= flac.stream_bound(4097) + flac.stream_bound(0) - 19 + 2 * 13 + 19 - 2 * 15   # the carries that are not there


def test_stream_step_refuses_bad_tables_without_a_device():
    """every refusal comes from the host table before anything is launched: the pointers below are never dereferenced, and the message
    names the refusal"""
    lib = _lib.lib()
    pcm, out, work, state = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28), C.c_void_p(1 << 16)

    def call(rows, n_push=None, pcm=pcm, out=out, work=work, state=state, dev=C.c_void_p(4096), host=True, counts=None, mask=None,
             n_slots=8, n_pcm=1 << 16, out_bytes=1 << 20, work_bytes=1 << 20):
        tab = _pushes(rows)
        return lib.ctts_flac_stream_step(pcm, n_pcm, mask, counts, dev, tab.ctypes.data_as(C.c_void_p) if host else None,
                                         len(rows) if n_push is None else n_push, state, n_slots, out, out_bytes, work, work_bytes, None)

    def why():
        return lib.ctts_last_error()
    ok = (0, 100, 24000, 0, 0, 0, -1, 0)
    for kw in (dict(pcm=None), dict(out=None), dict(dev=None), dict(host=False), dict(work=None), dict(state=None)):
        assert call([ok], **kw) != 0 and b"null" in why(), kw
    assert call([(0, 100, 24000, 0, 0, 1, 0, 0)]) != 0 and b"null" in why() and b"counts" in why()
    assert call([(0, 100, 24000, 0, 0, 3, -1, 0)]) != 0 and b"null" in why() and b"mask" in why()
    assert call([ok], n_push=0) != 0 and b"n_push" in why()
    assert call([(8 * i, 8, 24000, i, 0, 0, -1, 0) for i in range(1025)], n_slots=2048) != 0 and b"1024" in why()
    for slot in (-1, 8, 1 << 20):
        assert call([(0, 100, 24000, slot, 0, 0, -1, 0)]) != 0 and b"outside the pool" in why(), slot
    assert call([ok, (104, 100, 24000, 1, 0, 0, -1, 0), (208, 10, 8000, 0, 0, 0, -1, 0)]) != 0 and b"twice" in why()
    for start in (4, 7, 9, 1001, -8):
        assert call([(start, 10, 24000, 0, 0, 0, -1, 0)]) != 0 and b"multiples of 8" in why(), start
    assert call([(8, -1, 24000, 0, 0, 0, -1, 0)]) != 0 and b"negative" in why()
    assert call([(8, 1 << 31, 24000, 0, 0, 0, -1, 0)], n_pcm=1 << 33) != 0 and b"beyond" in why()
    assert call([(65536 - 8, 9, 24000, 0, 0, 0, -1, 0)]) != 0 and b"beyond" in why()                 # one sample past pcm
    for rate in (0, -1, 65536, 100000, 1 << 20):
        assert call([(0, 8, rate, 0, 0, 0, -1, 0)]) != 0 and b"cannot be coded" in why(), rate
    for carry in (-1, 16):
        assert call([(0, 8, 24000, 0, carry, 0, -1, 0)]) != 0 and b"carries" in why(), carry
    assert call([(0, 8, 24000, 0, 0, 4, -1, 0)]) != 0 and b"flag" in why()
    for ci in (-2, 65536):
        assert call([(0, 8, 24000, 0, 0, 1, ci, 0)], counts=C.c_void_p(1 << 12)) != 0 and b"count_idx" in why(), ci
    assert call([(0, 8, 24000, 0, 0, 0, 0, 0)], counts=C.c_void_p(1 << 12)) != 0 and b"not final" in why() and b"count_idx" in why()
    assert call([(0, 8, 24000, 0, 0, 2, -1, 0)], mask=C.c_void_p(1 << 12)) != 0 and b"not final" in why() and b"mask" in why()
    for sample, n, carry in ((-1, 8, 0), (1 << 36, 0, 0), ((1 << 36) - 8, 8, 0), ((1 << 36) - 20, 8, 12), ((1 << 36) - 1, 1, 0)):
        assert call([(0, n, 24000, 0, carry, 0, -1, sample)]) != 0 and b"2^36" in why(), sample
    assert call([(0, 5000, 24000, 0, 0, 0, -1, 0, 0, 0), (5000, 8, 24000, 1, 0, 0, -1, 0, 5000, 1)]) != 0 and b"frame0" in why()
    assert call([(0, 8, 24000, 0, 0, 0, -1, 0, 0, 3)]) != 0 and b"frame0" in why()
    assert call([(0, 8, 24000, 0, 0, 0, -1, 0, 8, 0)]) != 0 and b"stage" in why()
    assert call([(0, 4096, 24000, 0, 0, 0, -1, 0)], out_bytes=2 * 4096 + 18) != 0 and b"out of capacity" in why()
    assert call([(0, 4096, 24000, 0, 0, 0, -1, 0)], work_bytes=2 * 4096 + 64) != 0 and b"out of capacity" in why()
    assert call([ok], pcm=C.c_void_p((1 << 20) + 2)) != 0 and b"aligned" in why()
    assert call([ok], out=C.c_void_p((1 << 24) + 8)) != 0 and b"aligned" in why()
    sizes = (C.c_int64 * 4)()
    assert lib.ctts_flac_stream_sizes(None, 1, 8, 100, sizes) != 0 and b"null" in why()
    assert lib.ctts_flac_stream_sizes(_pushes([ok]).ctypes.data_as(C.c_void_p), 1, 8, 100, None) != 0 and b"null" in why()
    assert lib.ctts_flac_stream_sizes(_pushes([ok]).ctypes.data_as(C.c_void_p), 1, 8, 99, sizes) != 0 and b"beyond" in why()
    # streams that hold and get nothing launch nothing, and say so by succeeding on pointers no kernel could touch
    assert call([(0, 0, 24000, 0, 0, 1, -1, 0), (8, 0, 8000, 3, 0, 0, -1, 77)]) == 0


# ---- 5. Chat, the batcher and the endpoint on fakes ---------------------------------------------------------------------------------------
def test_infer_refuses_a_streamed_flac_without_the_option_and_with_split_text():
    from chattts_amd.core import Chat
    chat = Chat()
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["x"], pcm16=True, flac=True, stream=True)
    with pytest.raises(ValueError, match="split_text"):
        chat.infer(["x"], pcm16=True, flac=True, stream=True, stream_flac=True)
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(["x"], flac=True, stream=True, stream_flac=True, split_text=False)
    with pytest.raises(ValueError, match="encoding"):
        chat.infer(["x"], pcm16=True, flac=True, stream=True, stream_flac=True, split_text=False, encoding="ulaw")
    with pytest.raises(ValueError, match="sample rate"):
        chat.infer(["x"], pcm16=True, flac=True, stream=True, stream_flac=True, split_text=False, sample_rate=70000, stream_resample=True)


class _FlacCodec:
    """the FLAC streams of a fake engine: the host twin behind the engine's handles"""

    def __init__(self):
        self.enc, self.opened, self.closed = {}, [], []

    def flac_stream_open(self, rate, first_sample=0):
        h = len(self.opened)
        self.opened.append((h, rate))
        self.enc[h] = flac.StreamEncoder(rate, first_sample)
        return h

    def flac_stream_close(self, h):
        del self.enc[h]
        self.closed.append(h)

    def flac_streams_in_use(self):
        return len(self.enc)


def _fake_chat():
    from tests.test_g711_host import _EncChat
    from tests.test_stream_pool_host import _piece

    class _StreamFlacChat(_EncChat):
        """as _EncChat; a flagged window's piece is pushed into its stream of the fake engine and comes back as that push's frames"""

        def __init__(self):
            super().__init__()
            self.codec = _FlacCodec()

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            flags = kw.get("flac", [False] * len(windows))
            hs = kw.get("flac_streams", [None] * len(windows))
            out = []
            for (slot, prefix, a, b, tail), f, h in zip(windows, flags, hs):
                p = _piece(store[slot], prefix, a, b)
                out.append(np.frombuffer(self.codec.enc[h].push(p, bool(tail)), np.uint8) if f else p)
            return out
    return _StreamFlacChat()


def test_flac_streams_due_at_one_poll_share_one_call_and_free_their_slots():
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
        with pytest.raises(ValueError, match="non-streamed"):
            off.submit_stream("x", _Params(48), flac=True)                                   # without the option: today's refusal
        assert "stream_flac_chunks" not in off.occupancy()
    finally:
        off.close()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_flac=True)
    try:
        with pytest.raises(ValueError, match="encoding"):
            b.submit_stream("x", _Params(48), flac=True, encoding="ulaw")
        with pytest.raises(ValueError, match="sample rate"):
            b.submit_stream("x", _Params(48), flac=True, sample_rate=70000)
        with lock:       # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = {"A": b.submit_stream("A", _Params(96), flac=True), "B": b.submit_stream("B", _Params(96)),
                       "C": b.submit_stream("C", _Params(96), flac=True, sample_rate=8000)}
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
            assert all(g.dtype == np.uint8 for g in got[tag])
            SC.check_stream([g.tobytes() for g in got[tag]], rate, np.concatenate(want))     # header, then the chunks: the PCM stream's samples
        polls = sorted({p for p, _, _, _ in sched})
        assert len(chat.window_calls) == len(polls) < len(sched)                             # one call per poll for the three streams
        for w, kw in zip(chat.window_calls, chat.kw_calls):
            slots = [x[0] for x in w]
            assert kw["flac"] == [s != 1 for s in slots] and kw["sample_rates"] == [8000 if s == 2 else 24000 for s in slots]
            assert [h is not None for h in kw["flac_streams"]] == kw["flac"] and set(kw) == {"flac", "flac_streams", "sample_rates"}
        assert sorted(chat.codec.opened) == [(0, 24000), (1, 8000)]
        deadline = time.time() + 10
        while chat.codec.flac_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.flac_streams_in_use() == 0 and sorted(chat.codec.closed) == [0, 1]
        occ = b.occupancy()
        assert occ["stream_flac_chunks"] == 2 * len(sched) and occ["flac_encoded"] == 0 and occ["completed"] == 3
        s = b.submit_stream("D", _Params(400), flac=True)                                    # cancelled mid-stream: its slot is freed
        first = next(s)
        s.close()
        assert first.dtype == np.uint8 and list(s) == []
        deadline = time.time() + 10
        while chat.codec.flac_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.flac_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1
        n_calls = len(chat.kw_calls)
        assert sum(len(c) for c in b.submit_stream("E", _Params(48))) == 256 * 95            # no flag: today's call, no keyword
        assert all(kw == {} for kw in chat.kw_calls[n_calls:])
    finally:
        b.close()
    assert not lock.locked()


def test_endpoint_streams_flac_only_with_the_option():
    import threading

    from starlette.testclient import TestClient

    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    full = np.arange(600, dtype=np.int16)

    class _Chat(_EndpointChat):
        def infer(self, text, stream=False, **kw):
            out = super().infer(text, stream, **kw)
            if not kw.get("flac"):
                return out
            if not stream:
                return [np.frombuffer(flac.encode(w, kw.get("sample_rate", 24000)), np.uint8) for w in out]
            assert kw["stream_flac"] is True and kw["split_text"] is False
            enc = flac.StreamEncoder(kw.get("sample_rate", 24000))
            chunks = list(out)
            return ([np.frombuffer(enc.push(c[0], i == len(chunks) - 1), np.uint8)] for i, c in enumerate(chunks))

    class _Batcher:
        streams, refine, stream_flac = True, False, True

        def __init__(self):
            self.lock, self.calls = threading.Lock(), []

        def submit_stream(self, text, params, **kw):
            self.calls.append(("stream", text, kw))
            enc = flac.StreamEncoder(kw.get("sample_rate", 24000))
            parts = [full[:10], full[10:10], full[10:250]]
            outer = self

            class _It:
                def __init__(self):
                    self.it = iter([np.frombuffer(enc.push(p, i == 2), np.uint8) if kw.get("flac") else p for i, p in enumerate(parts)])

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
    body = {"input": "hello", "response_format": "flac", "stream": True}
    with TestClient(server.create_app(chat, flac=True)) as c:                                # option off: today's 400
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "non-streamed" in r.text and "variable-block-size" in r.text and not chat.calls
        assert "stream_flac" not in c.get("/health").json()
    with TestClient(server.create_app(chat, stream_flac=True)) as c:                         # without flac the format does not exist
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 400 and "Unsupported audio format: flac" in r.text and "stream_flac" not in c.get("/health").json()
    with TestClient(server.create_app(chat, flac=True, stream_flac=True, stream_sample_rates=(8000,), g711=True)) as c:
        assert c.get("/health").json()["stream_flac"] is True
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content[:42] == flac.stream_header(24000)
        y, rate = SO.decode(r.content)
        assert rate == 24000 and np.array_equal(y, full) and chat.calls[-1][1] is True and chat.calls[-1][2]["flac"] is True
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        y, rate = SO.decode(r.content)
        assert r.status_code == 200 and rate == 8000 and np.array_equal(y, full) and chat.calls[-1][2]["stream_resample"] is True
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={**body, "encoding": "ulaw"})
        assert r.status_code == 400 and "ncoding" in r.text and len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "stream": True})     # no flac: today's call
        assert r.content == full.tobytes() and "flac" not in chat.calls[-1][2] and "stream_flac" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac"})                    # the file, as before
        assert r.content == flac.encode(full, 24000) and "stream_flac" not in chat.calls[-1][2]
    chat, bat = _Chat(), _Batcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, flac=True, stream_flac=True, stream_sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and r.content[:42] == flac.stream_header(8000)
        y, rate = SO.decode(r.content)
        assert rate == 8000 and np.array_equal(y, full[:250]) and not chat.calls
        assert bat.calls[-2:] == [("stream", "hello", {"sample_rate": 8000, "flac": True}), ("closed",)]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "stream": True})
        assert r.content == full[:250].tobytes() and bat.calls[-2] == ("stream", "hello", {})

"""Streams at other sample rates, the parts that need no GPU: the window a chunk's outputs read (`resample.window_inputs`) against the
float64 oracle, the tiling of a stream's chunks, the new C entries' refusals, `SpeechBatcher.submit_stream(sample_rate=)` on a fake
pool and the endpoint's `stream_sample_rates` on a fake chat."""
import ctypes as C
import os
import struct
import threading

import numpy as np
import pytest

from chattts_amd import _lib, resample as RS
from chattts_amd.serving import SpeechBatcher, StreamSpec, stream_schedule
from tests.resample_oracle import PAIRS, oracle_taps, reduced, resample_f64
from tests.test_split_pool_host import _EndpointChat
from tests.test_stream_pool_host import _FakeChat, _FakePool, _Params

N = 600


def _geometry(orig, new):
    M, L = reduced(orig, new)
    h, width = oracle_taps(orig, new)
    return L, M, h.shape[1], width


def _ranges(L, n_out):
    """every (o_lo, o_hi): o_lo in {0, 1, L-1, L, L+1} or at the output's end, lengths {0, 1, L, 2L+1}; the last output and n_out itself"""
    out = set()
    for o_lo in {0, 1, L - 1, L, L + 1, n_out - 2 * L - 1, n_out - L, n_out - 1, n_out}:
        for n in (0, 1, L, 2 * L + 1):
            if 0 <= o_lo and o_lo + n <= n_out:
                out.add((o_lo, o_lo + n))
    out.add((n_out - 1, n_out))
    out.add((n_out, n_out))
    return sorted(out)


# ---- 1. a window equals the slice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_window_equals_slice_of_the_whole_signal(orig, new):
    """the oracle on x[a:b] alone (placed at its own position, zeros elsewhere) gives outputs [o_lo, o_hi) of the oracle on all of x"""
    L, M, K, width = _geometry(orig, new)
    assert RS.geometry(L, M) == (width, K)
    x = np.random.default_rng(orig + new).standard_normal(N)
    whole = resample_f64(x, orig, new)
    n_out = RS.out_len(N, L, M)
    assert whole.shape[0] == n_out
    for o_lo, o_hi in _ranges(L, n_out):
        a, b = RS.window_inputs(L, M, K, o_lo, o_hi, N)
        assert 0 <= a <= b <= N and (a < b) == (o_hi > o_lo)
        xz = np.zeros(N)
        xz[a:b] = x[a:b]
        assert np.array_equal(resample_f64(xz, orig, new)[o_lo:o_hi], whole[o_lo:o_hi]), (o_lo, o_hi, a, b)


@pytest.mark.parametrize("orig,new", PAIRS)
def test_window_is_tight(orig, new):
    """one sample less at either end changes some output of a signal of ones -- unless that end is the signal's own.  The filter's
    outermost taps are ~1e-49 or smaller (the Hann window's zero at t = +-6, where `width` puts k = 0) and vanish in a float64 sum,
    so the outputs are compared through the taps' SUPPORT: the oracle's table with every tap set to one counts the samples an output
    reads, which is what `window_inputs` states."""
    L, M, K, width = _geometry(orig, new)
    n_out = RS.out_len(N, L, M)

    def reads(x, o_lo, o_hi):      # y[o] = sum_k x[j M + k - width], the oracle's formula with h = 1
        xp = np.zeros(width + N + K + M)
        xp[width: width + N] = x
        return np.array([xp[(o // L) * M: (o // L) * M + K].sum() for o in range(o_lo, o_hi)])
    ones = np.ones(N)
    for o_lo, o_hi in _ranges(L, n_out):
        if o_hi == o_lo:
            continue
        a, b = RS.window_inputs(L, M, K, o_lo, o_hi, N)
        full = reads(ones, o_lo, o_hi)
        for lo, hi, clipped in ((a + 1, b, a == 0), (a, b - 1, b == N)):
            xz = np.zeros(N)
            xz[lo:hi] = 1.0
            changed = not np.array_equal(reads(xz, o_lo, o_hi), full)
            assert changed or clipped, (o_lo, o_hi, a, b, lo, hi)
        xz = np.zeros(N)
        xz[a:b] = 1.0
        assert np.array_equal(reads(xz, o_lo, o_hi), full)
        # with the real taps, too, the window is sufficient for a signal of ones
        assert np.array_equal(resample_f64(xz, orig, new)[o_lo:o_hi], resample_f64(ones, orig, new)[o_lo:o_hi])


# ---- 2. a stream's chunks tile the resampled output ------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", (0, 1, 12000))
def test_chunks_tile_the_output(speed):
    for orig, new in PAIRS[:4]:                      # the conversions from 24 kHz
        L, M, K, _ = _geometry(orig, new)
        # EOS exactly on a stream_batch multiple (the duplicate yield), fewer yields than pass_first_n_batches, an ordinary end
        for n, eos, passed, counts in ((48, True, 0, [8, 16, 24, 32, 40, 48]), (30, True, 5, [16, 30]), (80, False, 1, [8, 24, 50, 80]),
                                       (1, True, 0, []), (96, True, 2, [])):
            sched = stream_schedule(counts, n, eos, StreamSpec(24, speed, passed))
            total = 256 * (2 * n - 1)
            at = 0
            for prefix, s_lo, s_hi, tail in sched:
                o_lo, o_hi = RS.out_len(s_lo, L, M), RS.out_len(s_hi, L, M)
                assert o_lo == at and o_hi >= o_lo, (new, n, speed, prefix, s_lo, s_hi)
                at = o_hi
                ptotal = 256 * (2 * prefix - 1)
                a, b = RS.window_inputs(L, M, K, o_lo, o_hi, ptotal)      # never refused: the chunk ends inside its prefix's outputs
                assert 0 <= a <= b <= ptotal
                if o_hi > o_lo:
                    assert a <= s_lo and b >= min(s_hi, ptotal) - M      # the widened window holds the chunk's own samples
            assert sched[-1][3] and at == RS.out_len(total, L, M), (new, n, speed)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_window_inputs_refusals():
    L, M, K, width = _geometry(24000, 8000)
    n_out = RS.out_len(N, L, M)
    assert RS.window_inputs(L, M, K, 0, n_out, N) == (0, N)
    assert RS.window_inputs(L, M, K, 50, 50, N) == (50 * M - width, 50 * M - width)        # an empty chunk reads nothing
    assert RS.window_inputs(L, M, K, 50, 51, N) == (50 * M - width, 50 * M + width + M)
    for o_lo, o_hi in ((-1, 4), (5, 4), (0, n_out + 1), (n_out + 1, n_out + 1)):
        with pytest.raises(ValueError):
            RS.window_inputs(L, M, K, o_lo, o_hi, N)
    with pytest.raises(ValueError):
        RS.window_inputs(L, M, M, 0, 1, N)           # no table has K <= M
    with pytest.raises(ValueError):
        RS.window_inputs(L, M, K + 1, 0, 1, N)       # K - M must be even


def _rs_table(rows):
    tab = np.zeros(len(rows), _lib.RS_WINDOW)
    for i, r in enumerate(rows):
        tab[i] = r
    return tab, tab.ctypes.data_as(C.c_void_p)


def test_new_symbols_are_exported_and_declared():
    lib = _lib.lib()
    names = ("ctts_resample_windows", "ctts_codec_windows_rate_workspace_bytes", "ctts_codec_decode_windows_rate")
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "} ctts_rs_window;" in header and _lib.RS_WINDOW.itemsize == 64 and C.sizeof(_lib.Rate) == 24
    f = lib.ctts_codec_windows_rate_workspace_bytes
    assert f(0, 10, 8) == 0 and f(2, 80, -1) == 0
    assert f(2, 80, 0) == lib.ctts_codec_windows_workspace_bytes(2, 80) and f(2, 80, 4096) >= f(2, 80, 0) + 4096 * 4


def test_resample_windows_refuses_bad_tables_without_a_device():
    """every refusal comes from the host mirror before anything is launched: the pointers below are never dereferenced"""
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    L, M, K, width = _geometry(24000, 8000)
    total = 6000
    n_out = RS.out_len(total, L, M)

    def call(rows, n_win=None, taps=fake, lmk=(L, M, K), n_x=1 << 30, n_y=1 << 30, sel=None):
        tab, p = _rs_table(rows)
        sp = None if sel is None else np.asarray(sel, np.int32).ctypes.data_as(C.c_void_p)
        return lib.ctts_resample_windows(fake, n_x, fake, p, len(rows) if n_win is None else n_win, fake, n_y, None if sel is None else fake, sp,
                                         0 if sel is None else len(sel), taps, *lmk, None)
    a, b = RS.window_inputs(L, M, K, 100, 200, total)
    ok = (0, b - a, a, total, 100, 200, 0, 0, 0)     # in_off, n_in, origin, total, o_lo, o_hi, out_off, rate, pad
    for rows, msg in (([(0, b - a, a, total, 200, 100, 0, 0, 0)], b"outputs"), ([(0, b - a, a, total, -1, 100, 0, 0, 0)], b"outputs"),
                      ([(0, b - a, a, total, 100, n_out + 1, 0, 0, 0)], b"beyond"), ([(0, b - a - 1, a, total, 100, 200, 0, 0, 0)], b"read"),
                      ([(0, b - a - 1, a + 1, total, 100, 200, 0, 0, 0)], b"read"), ([(0, total + 1, 0, total, 100, 200, 0, 0, 0)], b"signal"),
                      ([(0, b - a, -1, total, 100, 200, 0, 0, 0)], b"signal"), ([(0, b - a, a, total, 100, 200, 0, 0, 256)], b"pad")):
        assert call(rows) != 0 and msg in lib.ctts_last_error(), (rows, lib.ctts_last_error())
    assert call([ok], taps=None) != 0 and b"null" in lib.ctts_last_error()
    assert call([ok], lmk=(L, M, K + M * 4000)) != 0 and b"not supported" in lib.ctts_last_error()
    assert call([ok], lmk=(3, 3, 9)) != 0
    assert call([ok] * 1025) != 0 and b"1024" in lib.ctts_last_error()
    assert call([ok], n_win=0) != 0
    assert call([ok], n_x=b - a - 1) != 0 and b"outside" in lib.ctts_last_error()
    assert call([ok], n_y=99) != 0 and b"outside" in lib.ctts_last_error()
    assert call([ok], sel=[1]) != 0 and b"selected" in lib.ctts_last_error()


def test_decode_windows_rate_refuses_bad_tables_without_a_device():
    lib = _lib.lib()
    fake = C.c_void_p(4096)
    S, cap = 8, 64
    L, M, K, width = _geometry(24000, 8000)
    Tn = 40
    total = 256 * (2 * Tn - 1)
    o_lo, o_hi = RS.out_len(0, L, M), RS.out_len(12000, L, M)
    a, b = RS.window_inputs(L, M, K, o_lo, o_hi, total)
    n = o_hi - o_lo
    win_ok = (0, 0, Tn, a, b, 0)
    rs_ok = (a, b - a, a, total, o_lo, o_hi, 0, 0, -n % 8)

    def call(win=win_ok, rs=rs_ok, taps=fake, lmk=(L, M, K), n_rates=1, sel=(0,), n_win=1):
        tab = np.ascontiguousarray(np.array([[*win, 0, 0]], dtype=np.int32))
        rtab, rp = _rs_table([rs])
        rates = (_lib.Rate * 1)()
        rates[0].taps, rates[0].L, rates[0].M, rates[0].K = taps, *lmk
        s = np.asarray(sel, np.int32)
        return lib.ctts_codec_decode_windows_rate(fake, fake, cap * 768, 768, S, cap, fake, tab.ctypes.data_as(C.c_void_p), fake, rp, fake,
                                                  s.ctypes.data_as(C.c_void_p), n_win, C.cast(rates, C.c_void_p), n_rates, 1, fake, fake, 0, 1e-5,
                                                  fake, 1024, None)
    # the valid tables get as far as the workspace check: everything before it passed
    assert call() != 0 and b"workspace" in lib.ctts_last_error(), lib.ctts_last_error()
    assert call(taps=None) != 0 and b"null" in lib.ctts_last_error()
    assert call(lmk=(L, M, K + M * 4000)) != 0 and b"not supported" in lib.ctts_last_error()
    assert call(rs=(a, b - a, a, total, o_hi, o_lo, 0, 0, 0)) != 0 and b"outputs" in lib.ctts_last_error()
    assert call(rs=(a, b - a, a, total, o_lo, o_lo, 0, 0, 0)) != 0 and b"outputs" in lib.ctts_last_error()
    # a crop one sample short of what the outputs read (both tables agree with each other, the window does not hold the inputs)
    assert call(win=(0, 0, Tn, a, b - 1, 0), rs=(a, b - a - 1, a, total, o_lo, o_hi, 0, 0, -n % 8)) != 0 and b"read" in lib.ctts_last_error()
    assert call(rs=(a + 1, b - a, a, total, o_lo, o_hi, 0, 0, -n % 8)) != 0 and b"crop" in lib.ctts_last_error()
    assert call(rs=(a, b - a, a, total, o_lo, o_hi, 8, 0, -n % 8)) != 0 and b"multiples of 8" in lib.ctts_last_error()
    assert call(rs=(a, b - a, a, total, o_lo, o_hi, 0, 1, -n % 8)) != 0 and b"rate" in lib.ctts_last_error()
    assert call(sel=(1,)) != 0 and b"selection" in lib.ctts_last_error()
    assert call(n_win=1025) != 0 and b"1024" in lib.ctts_last_error()
    assert call(n_win=0) != 0


# ---- 4. the batcher on fakes -----------------------------------------------------------------------------------------------------------
class _RateChat(_FakeChat):
    """as _FakeChat; a call with rates is recorded with them and a resampled window's audio is a ramp over its OUTPUT range"""

    def __init__(self):
        super().__init__()
        self.rate_calls = []

    def decode_windows_pcm16(self, store, windows, **kw):
        self.window_calls.append(list(windows))
        self.rate_calls.append(dict(kw))
        rates = kw.get("sample_rates", [24000] * len(windows))
        return [_rate_piece(store[slot], prefix, a, b, r) for (slot, prefix, a, b, tail), r in zip(windows, rates)]


def _rate_piece(tag, prefix, a, b, rate):
    L, M = RS.ratio(24000, rate) if rate != 24000 else (1, 1)
    return ((np.arange(RS.out_len(a, L, M), RS.out_len(b, L, M)) + 1000 * prefix + tag) % 30000).astype(np.int16)


def test_streams_at_three_rates_due_at_one_poll_share_one_decode_call():
    lock = threading.Lock()
    chat = _RateChat()
    holder = {}
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True)
    try:
        with pytest.raises(ValueError):
            b.submit_stream("x", _Params(48), sample_rate=24001)        # 8000/8001: beyond the kernel, refused at submit
        with lock:       # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = {8000: b.submit_stream("A", _Params(96), sample_rate=8000), 16000: b.submit_stream("B", _Params(96), sample_rate=16000),
                       24000: b.submit_stream("C", _Params(96), sample_rate=24000)}
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in streams.items()]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        sched = stream_schedule([], 96, True, StreamSpec(24, 12000, 0))
        for (rate, _), tag in zip(streams.items(), "ABC"):
            want = [_rate_piece(ord(tag), p, lo, hi, rate) for p, lo, hi, _ in sched]
            assert len(got[rate]) == len(want) and all(np.array_equal(g, w) for g, w in zip(got[rate], want)), rate
            L, M = RS.ratio(24000, rate) if rate != 24000 else (1, 1)
            assert sum(len(g) for g in got[rate]) == RS.out_len(256 * (2 * 96 - 1), L, M)       # the chunks tile the stream
        # one call per poll for the three streams, with one rate per window in the windows' order
        full = [(w, kw) for w, kw in zip(chat.window_calls, chat.rate_calls) if len(w) == 3]
        assert full and len(chat.window_calls) == b.occupancy()["stream_decode_calls"]
        for w, kw in full:
            assert kw == {"sample_rates": [{0: 8000, 1: 16000, 2: 24000}[x[0]] for x in w]}, kw
        occ = b.occupancy()
        assert occ["stream_resampled_chunks"] == 2 * len(sched) and occ["stream_chunks"] == 3 * len(sched)
        # sample_rate=24000 (or none) passes no rate: the call is today's
        n_calls = len(chat.rate_calls)
        assert [len(c) for c in b.submit_stream("D", _Params(48), sample_rate=24000)] == \
            [hi - lo for _, lo, hi, _ in stream_schedule([], 48, True, StreamSpec(24, 12000, 0))]
        assert len(chat.rate_calls) > n_calls and all(kw == {} for kw in chat.rate_calls[n_calls:])
        plain = _FakeChat()                      # a chat whose decode_windows_pcm16 takes no keyword at all
        holder2 = {}
        b2 = SpeechBatcher(plain, 2, lock, make_pool=lambda: holder2.setdefault("p", _FakePool(2, lock)), streams=True)
        try:
            assert sum(len(c) for c in b2.submit_stream("E", _Params(48))) == 256 * 95
            assert b2.occupancy()["stream_resampled_chunks"] == 0
        finally:
            b2.close()
    finally:
        b.close()
    assert not lock.locked()


# ---- 5. the endpoint on a fake chat ----------------------------------------------------------------------------------------------------
class _StreamBatcher:
    streams, refine = True, False

    def __init__(self):
        self.lock, self.calls = threading.Lock(), []

    def submit_stream(self, text, params, **kw):
        self.calls.append((text, kw))

        class _It:
            def __init__(self):
                self.it = iter([np.arange(100, dtype=np.int16), np.zeros((0,), np.int16), np.arange(100, 250, dtype=np.int16)])

            def __iter__(self):
                return self

            def __next__(self):
                return next(self.it)

            def close(self):
                pass
        return _It()

    def occupancy(self):
        return {}


def test_endpoint_serves_streams_at_the_configured_rates_only():
    from starlette.testclient import TestClient
    from chattts_amd import server
    body = {"input": "hello", "response_format": "wav", "stream": True}
    old_text = ("sample_rate 8000 is served for non-streamed requests only: a stream's chunks are produced at 24000 Hz (the resampling "
                "filter's state is not carried across chunks)")
    chat = _EndpointChat()
    with TestClient(server.create_app(chat, sample_rates=(8000, 24000))) as c:          # without the option: today's 400, today's text
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 400 and old_text in r.text and not chat.calls
    chat = _EndpointChat()
    with TestClient(server.create_app(chat, sample_rates=(8000, 16000, 24000), stream_sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 16000})             # a rate outside the option: the same 400
        assert r.status_code == 400 and old_text.replace("8000", "16000") in r.text and not chat.calls
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 44100})
        assert r.status_code == 400 and "Unsupported sample_rate" in r.text and not chat.calls
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200
        assert r.content[:44] == server.wav_stream_header(8000) and struct.unpack("<I", r.content[24:28])[0] == 8000
        assert np.array_equal(np.frombuffer(r.content[44:], "<i2"), np.arange(600, dtype=np.int16))       # the fake's chunks
        text, stream, kw = chat.calls[-1]
        assert stream and kw["sample_rate"] == 8000 and kw["stream_resample"] is True and kw["split_text"] is False
        r = c.post("/v1/audio/speech", json=body)                                       # no rate: today's call, today's header
        assert r.status_code == 200 and r.content[:44] == server.wav_stream_header()
        assert "sample_rate" not in chat.calls[-1][2] and "stream_resample" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={**body, "stream": False, "sample_rate": 16000})      # non-streamed: as before
        assert r.status_code == 200 and chat.calls[-1][2]["sample_rate"] == 16000 and "stream_resample" not in chat.calls[-1][2]
    chat, bat = _EndpointChat(), _StreamBatcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, stream_sample_rates=(8000, 16000))) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 16000})             # through the pool
        assert r.status_code == 200 and r.content[:44] == server.wav_stream_header(16000)
        assert np.array_equal(np.frombuffer(r.content[44:], "<i2"), np.arange(250, dtype=np.int16))
        assert bat.calls[-1] == ("hello", {"sample_rate": 16000}) and not chat.calls
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and r.content[:44] == server.wav_stream_header() and bat.calls[-1] == ("hello", {})
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 48000})             # only stream rates configured, a rate outside them
        assert r.status_code == 400 and "non-streamed requests only" in r.text and len(bat.calls) == 2

"""FLAC output, the parts that need no GPU: the CRCs, one stream written out by hand, the NumPy twin through the independent decoder
(tests/flac_oracle.py) over every length and signal of tests/flac_cases.py, the exact search against a brute-force count, every refusal of
ctts_flac_encode_ranges, the endpoint on a fake chat and the batcher on fake pools."""
import ctypes as C
import itertools
import os
import threading

import numpy as np
import pytest

from chattts_amd import _lib, flac
from chattts_amd.serving import SpeechBatcher
from tests import flac_cases as FC
from tests import flac_oracle
from tests.test_g711_host import _EncChat, _GroupPool
from tests.test_split_pool_host import _EndpointChat
from tests.test_stream_pool_host import _FakePool, _Params


# ---- 1. checksums and one stream by hand ------------------------------------------------------------------------------------------------
def test_crc_check_values():
    assert flac.crc8(b"123456789") == 0xF4 and flac.crc16(b"123456789") == 0xFEE8
    assert flac_oracle._crc8(b"123456789") == 0xF4 and flac_oracle._crc16(b"123456789") == 0xFEE8
    assert flac.crc8(b"") == 0 and flac.crc16(b"") == 0
    data = bytes(range(256)) * 3
    assert flac.crc16(data) == flac_oracle._crc16(data) and flac.crc8(data) == flac_oracle._crc8(data)
    assert flac_oracle._crc16_many(data, [(0, 9), (5, 700), (0, 0)]) == [flac.crc16(data[0:9]), flac.crc16(data[5:700]), 0]


def test_a_constant_block_byte_by_byte():
    """five samples of value 7 at 11025 Hz: a rate outside the table (code 1101, Hz in 16 bits), a short block (code 0111, n - 1 in 16
    bits), frame number 0, a CONSTANT subframe"""
    x = np.full(5, 7, np.int16)
    head = bytes([0xFF, 0xF8, 0x7D, 0x08, 0x00, 0x00, 0x04, 0x2B, 0x11])
    frame = head + bytes([flac_oracle._crc8(head)]) + bytes([0x00, 0x00, 0x07])
    frame += flac_oracle._crc16(frame).to_bytes(2, "big")
    assert len(frame) == 15
    body, lens = flac.frames(x, 11025)
    assert body == frame and lens.tolist() == [15]
    info = (b"fLaC" + bytes([0x80, 0x00, 0x00, 0x22]) + bytes([0x10, 0x00, 0x10, 0x00]) + bytes([0, 0, 15, 0, 0, 15])
            + bytes([0x02, 0xB1, 0x10, 0xF0, 0x00, 0x00, 0x00, 0x05]) + bytes(16))
    assert len(info) == 42 == flac.HEADER_BYTES and flac.stream_info(5, 11025, lens) == info
    assert flac.encode(x, 11025) == info + frame
    assert flac.encode(np.zeros(0, np.int16), 24000) == flac.stream_info(0, 24000, []) and len(flac.encode(np.zeros(0, np.int16), 24000)) == 42
    assert flac.stream_info(0, 24000, [])[8:18] == bytes([0x10, 0x00, 0x10, 0x00, 0, 0, 0, 0, 0, 0])


def test_frame_header_fields():
    h = flac.frame_header(0, 4096, 24000)
    assert h[:5] == bytes([0xFF, 0xF8, 0xC7, 0x08, 0x00]) and len(h) == 6 and h[5] == flac_oracle._crc8(h[:5])
    h = flac.frame_header(127, 4096, 48000)
    assert h[2] == 0xCA and h[4] == 0x7F and len(h) == 6
    h = flac.frame_header(128, 4096, 8000)                      # two bytes of frame number from frame 128 on
    assert h[2] == 0xC4 and h[4:6] == bytes([0xC2, 0x80]) and len(h) == 7 and h[6] == flac_oracle._crc8(h[:6])
    h = flac.frame_header(2048, 100, 65535)                     # three bytes; the short block and the rate in Hz behind it
    assert h[2] == 0x7D and h[4:7] == bytes([0xE0, 0xA0, 0x80]) and h[7:11] == bytes([0x00, 0x63, 0xFF, 0xFF]) and len(h) == 12
    codes = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 88200: 1, 176400: 2, 192000: 3, 96000: 11}
    assert all(flac.rate_code(r) == c for r, c in codes.items()) and flac.rate_code(11025) == 13 and flac.rate_code(1) == 13
    for bad in (0, -8000, 65536, 100000, 24000.5, True, 1 << 20):
        with pytest.raises(ValueError):
            flac.rate_code(bad)
    assert flac.bound(0) == 42 and flac.bound(1) == 42 + 2 + 16 and flac.bound(4097) == 42 + 2 * 4097 + 32


def test_twin_refuses_other_inputs():
    with pytest.raises(ValueError):
        flac.encode(np.zeros(4, np.int32), 24000)
    with pytest.raises(ValueError):
        flac.encode(np.zeros((2, 4), np.int16), 24000)
    with pytest.raises(ValueError):
        flac.encode(np.zeros(4, np.int16), 70000)


# ---- 2. the twin through the independent decoder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.SIGNALS)
@pytest.mark.parametrize("n", FC.LENGTHS)
def test_round_trip_and_bound(n, name):
    x, rate, body, lens = FC.reference(name, n)
    file = flac.stream_info(n, rate, lens) + body
    assert file == flac.encode(x, rate) if n <= 4097 else True
    assert len(file) <= flac.bound(n) and len(lens) == (n + 4095) // 4096 and int(lens.sum()) == len(body)
    y, r, facts = FC.decoded(file)
    assert r == rate and y.dtype == np.int16 and np.array_equal(y, x)
    assert facts["md5"] == bytes(16) and facts["total"] == n
    if name == "noise":                                         # nothing to gain: every block of 16 samples or more stays VERBATIM
        assert all(k == "VERBATIM" for k, b in zip(facts["kinds"], facts["blocks"]) if b >= 16)
    if name in ("silence", "dc_min", "dc_max"):
        assert all(k == "CONSTANT" for k in facts["kinds"])
    if n > 128 * 4096:
        assert len(lens) == 129 and body[int(lens[:128].sum()) + 4: int(lens[:128].sum()) + 6] == bytes([0xC2, 0x80])


def test_the_decoder_refuses_damage():
    x, rate, body, lens = FC.reference("ar2", 4097)
    file = bytearray(flac.stream_info(4097, rate, lens) + body)
    for at in (0, 42, 42 + 3, 42 + 100, len(file) - 1, 42 + int(lens[0]) + 1):
        bad = bytearray(file)
        bad[at] ^= 0x10
        with pytest.raises(ValueError):
            flac_oracle.decode(bytes(bad))
    with pytest.raises(ValueError):
        flac_oracle.decode(bytes(file[:-3]))
    with pytest.raises(ValueError):                             # a frame number out of order
        flac_oracle.decode(bytes(file[:42]) + body[int(lens[0]):] + body[: int(lens[0])])


# ---- 3. the exact search --------------------------------------------------------------------------------------------------------------------
def _brute(x):
    """the smallest subframe by counting, written without the twin's arrays: every order, every partition order, every parameter, code
    by code; for up to two partitions every COMBINATION of parameters (the minimum is separable, this shows it) -> (bits, o, p)"""
    n = len(x)
    x = [int(v) for v in x]
    if all(v == x[0] for v in x):
        return 24, "CONSTANT"
    best, tag = 8 + 16 * n, "VERBATIM"
    ctz = (n & -n).bit_length() - 1
    for o in range(min(4, n - 1) + 1):
        r = list(x)
        for _ in range(o):
            r = [b - a for a, b in zip(r[:-1], r[1:])]          # len n - o: r[i] belongs to sample i + o
        u = [(v << 1) ^ (v >> 31) if v >= 0 else ((v << 1) ^ -1) for v in r]
        for p in range(min(6, ctz) + 1):
            size = n >> p
            if size <= o:
                continue
            parts = [u[max(j * size - o, 0): (j + 1) * size - o] for j in range(1 << p)]

            def cost(part, k):
                return sum((v >> k) + 1 + k for v in part)
            if p <= 1:
                body = min(sum(4 + cost(part, k) for part, k in zip(parts, ks)) for ks in itertools.product(range(15), repeat=1 << p))
            else:
                body = sum(4 + min(cost(part, k) for k in range(15)) for part in parts)
            bits = 8 + 16 * o + 6 + body
            if bits < best:
                best, tag = bits, f"FIXED{o}/{p}"
    return best, tag


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 64, 192])
def test_exact_search_against_a_brute_force_count(n):
    rng = np.random.default_rng(n)
    blocks = [rng.integers(-40, 41, n), np.cumsum(rng.integers(-9, 10, n)), (np.arange(n) ** 2) // 3 - 7, rng.integers(-32768, 32768, n),
              np.cumsum(np.cumsum(rng.integers(-2, 3, n))), np.where(np.arange(n) < n // 2, 0, rng.integers(-2000, 2001, n)),
              np.full(n, -3), np.r_[np.zeros(n - 1), 32767]]
    for b in blocks:
        x = np.clip(b, -32768, 32767).astype(np.int16)
        bits, tag = _brute(x)
        body, lens = flac.frames(x, 24000)
        hdr = len(flac.frame_header(0, n, 24000))
        assert int(lens[0]) == hdr + (bits + 7) // 8 + 2, (n, x[:8], tag)
        _, _, facts = flac_oracle.decode(flac.encode(x, 24000), info=True)
        assert facts["kinds"] == [tag], (n, x[:8])              # the ties too: the lowest order, then the lowest partition order


def test_ties_go_to_the_lowest_order_partition_and_parameter():
    x = np.array([0, 0, 0, 0, 0, 0, 0, 1], np.int16)           # orders 0 and 1 cost the same at p = 0: order 0 wins; k = 0 beats k = 1
    _, _, facts = flac_oracle.decode(flac.encode(x, 24000), info=True)
    assert facts["kinds"] == ["FIXED0/0"] and _brute(x)[1] == "FIXED0/0"
    order, part, ks, bits = flac._analyse(x.astype(np.int64)[None, :])
    assert (int(order[0]), int(part[0]), int(ks[0, 0])) == (0, 0, 0)


# ---- 4. the C entry ---------------------------------------------------------------------------------------------------------------------------
def _table(rows):
    tab = np.zeros(len(rows), _lib.FLAC_RANGE)
    slots = 0
    for i, r in enumerate(rows):
        start, n, rate = r[:3]
        ci = r[3] if len(r) > 3 else -1
        tab[i] = (start, n, rate, ci, r[4] if len(r) > 4 else slots)
        slots += (max(n, 0) + 4095) // 4096 if rate > 0 else 0
    return tab


def test_symbol_is_exported_and_declared():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in ("ctts_flac_encode_ranges", "ctts_flac_encode_sizes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "} ctts_flac_range;" in header and _lib.FLAC_RANGE.itemsize == 32
    assert [_lib.FLAC_RANGE.fields[k][1] for k in ("start", "n", "rate", "count_idx", "frame0")] == [0, 8, 16, 20, 24]
    from chattts_amd import build
    assert "flac.hip" in build.SOURCES
    sizes = (C.c_int64 * 3)()
    tab = _table([(0, 4097, 24000), (4104, 10, 0), (4120, 4096, 8000)])
    assert lib.ctts_flac_encode_sizes(tab.ctypes.data_as(C.c_void_p), 3, sizes) == 0
    assert list(sizes)[:2] == [3, 2 * 4097 + 32 + 2 * 4096 + 16] and sizes[2] >= 8 * (3 + 1 + 3) and sizes[2] % 16 == 0
    assert sizes[1] == flac.bound(4097) + flac.bound(4096) - 2 * flac.HEADER_BYTES


def test_encode_ranges_refuses_bad_tables_without_a_device():
    """every refusal comes from the host table before anything is launched: the pointers below are never dereferenced, and the message
    names the refusal"""
    lib = _lib.lib()
    pcm, out, work = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)

    def call(rows, n_rng=None, pcm=pcm, out=out, work=work, dev=C.c_void_p(4096), host=True, counts=None, out_bytes=1 << 20, work_bytes=1 << 20):
        tab = _table(rows)
        return lib.ctts_flac_encode_ranges(pcm, counts, dev, tab.ctypes.data_as(C.c_void_p) if host else None,
                                           len(rows) if n_rng is None else n_rng, out, out_bytes, work, work_bytes, None)
    ok = (0, 100, 24000)
    for kw in (dict(pcm=None), dict(out=None), dict(dev=None), dict(host=False), dict(work=None)):
        assert call([ok], **kw) != 0 and b"null" in lib.ctts_last_error(), kw
    assert call([(0, 100, 24000, 0)]) != 0 and b"null" in lib.ctts_last_error() and b"counts" in lib.ctts_last_error()
    assert call([ok], n_rng=0) != 0 and b"n_rng" in lib.ctts_last_error()
    assert call([ok] * 2, n_rng=-1) != 0 and b"n_rng" in lib.ctts_last_error()
    assert call([(8 * i, 8, 24000) for i in range(1025)]) != 0 and b"1024" in lib.ctts_last_error()
    for start in (4, 7, 9, 1001, -8):
        assert call([(start, 10, 24000)]) != 0 and b"multiples of 8" in lib.ctts_last_error(), start
    assert call([(8, -1, 24000)]) != 0 and b"negative" in lib.ctts_last_error()
    assert call([(8, 1 << 31, 24000)]) != 0 and b"beyond" in lib.ctts_last_error()
    assert call([(0, 17, 24000), (16, 8, 8000)]) != 0 and b"overlapping" in lib.ctts_last_error()      # overlap by one sample
    assert call([(64, 8, 24000), (0, 8, 24000)]) != 0 and b"descending" in lib.ctts_last_error()
    assert call([(0, 16, 0), (8, 8, 24000)]) != 0 and b"overlapping" in lib.ctts_last_error()          # a skipped range counts too
    for rate in (-1, 65536, 100000, 1 << 20):
        assert call([(0, 8, rate)]) != 0 and b"cannot be coded" in lib.ctts_last_error(), rate
    for ci in (-2, 65536):
        assert call([(0, 8, 24000, ci)], counts=C.c_void_p(1 << 12)) != 0 and b"count_idx" in lib.ctts_last_error(), ci
    assert call([(0, 5000, 24000, -1, 0), (5000, 8, 24000, -1, 1)]) != 0 and b"frame0" in lib.ctts_last_error()   # the first owns two slots
    assert call([(0, 8, 24000, -1, 3)]) != 0 and b"frame0" in lib.ctts_last_error()
    assert call([(0, 4096, 24000)], out_bytes=2 * 4096 + 15) != 0 and b"out of capacity" in lib.ctts_last_error()
    assert call([(0, 4096, 24000)], work_bytes=64) != 0 and b"out of capacity" in lib.ctts_last_error()
    assert call([ok], out=pcm) != 0 and b"aliases" in lib.ctts_last_error()
    assert call([(0, 4096, 24000)], out=C.c_void_p((1 << 20) + 4096)) != 0 and b"aliases" in lib.ctts_last_error()     # inside the samples
    assert call([(0, 4096, 24000)], pcm=C.c_void_p((1 << 24) + 2048)) != 0 and b"aliases" in lib.ctts_last_error()      # samples inside out
    assert call([ok], pcm=C.c_void_p((1 << 20) + 2)) != 0 and b"aligned" in lib.ctts_last_error()
    assert call([ok], out=C.c_void_p((1 << 24) + 8)) != 0 and b"aligned" in lib.ctts_last_error()
    sizes = (C.c_int64 * 3)()
    assert lib.ctts_flac_encode_sizes(None, 1, sizes) != 0 and b"null" in lib.ctts_last_error()
    assert lib.ctts_flac_encode_sizes(_table([ok]).ctypes.data_as(C.c_void_p), 1, None) != 0 and b"null" in lib.ctts_last_error()
    assert lib.ctts_flac_encode_sizes(_table([(4, 8, 24000)]).ctypes.data_as(C.c_void_p), 1, sizes) != 0 and b"multiples of 8" in lib.ctts_last_error()
    # nothing to encode launches nothing either, and says so by succeeding on pointers no kernel could touch
    assert call([(0, 0, 24000), (8, 50, 0)]) == 0


def test_infer_refuses_flac_without_pcm16_with_an_encoding_or_streamed():
    from chattts_amd.core import Chat
    chat = Chat()
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(["x"], flac=True)
    with pytest.raises(ValueError, match="encoding"):
        chat.infer(["x"], pcm16=True, flac=True, encoding="ulaw")
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["x"], pcm16=True, flac=True, stream=True)
    with pytest.raises(ValueError, match="sample rate"):
        chat.infer(["x"], pcm16=True, flac=True, sample_rate=70000)
    assert Chat._flac_flags(None, 3, None, True, "t") is None and Chat._flac_flags([False] * 3, 3, "ulaw", True, "t") is None
    assert Chat._flac_flags(True, 2, None, False, "t") == [True, True]
    assert Chat._flac_flags([True, False], 2, [None, "alaw"], True, "t") == [True, False]      # a row is one or the other
    for args in ((True, 2, "ulaw", True), ([True, False], 2, ["ulaw", None], True), ([True], 2, None, True), ([True, False], 2, None, False)):
        with pytest.raises(ValueError):
            Chat._flac_flags(*args, "t")


# ---- 5. the endpoint on a fake chat ----------------------------------------------------------------------------------------------------------
class _FlacChat(_EndpointChat):
    """as _EndpointChat; with `flac` the results are the files of the same samples at the call's rate"""

    def infer(self, text, stream=False, **kw):
        out = super().infer(text, stream, **kw)
        if not kw.get("flac"):
            return out
        assert not stream
        return [np.frombuffer(flac.encode(w, kw.get("sample_rate", 24000)), np.uint8) for w in out]


class _FileBatcher:
    streams, refine = True, False

    def __init__(self):
        self.lock, self.calls = threading.Lock(), []

    def submit(self, text, params, **kw):
        from concurrent.futures import Future
        self.calls.append(("submit", text, kw))
        pcm = np.arange(100, dtype=np.int16)
        f = Future()
        f.set_result(np.frombuffer(flac.encode(pcm, kw.get("sample_rate", 24000)), np.uint8) if kw.get("flac") else pcm)
        return f

    def submit_stream(self, text, params, **kw):
        raise AssertionError("a flac request never reaches the streamed path")

    def occupancy(self):
        return {}


def test_endpoint_without_the_option_is_todays():
    from starlette.testclient import TestClient
    from chattts_amd import server
    chat = _FlacChat()
    with TestClient(server.create_app(chat)) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac"})
        assert r.status_code == 400 and "Unsupported audio format: flac, supported formats: pcm, wav" in r.text and not chat.calls
        assert c.get("/health").json()["formats"] == ["pcm", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav"})
        assert r.status_code == 200 and "flac" not in chat.calls[-1][2]
    with TestClient(server.create_app(chat, g711=True)) as c:
        assert c.get("/health").json()["formats"] == ["alaw", "pcm", "ulaw", "wav"]


def test_endpoint_serves_flac_serially_and_batched():
    from starlette.testclient import TestClient
    from chattts_amd import server
    full = np.arange(600, dtype=np.int16)
    chat = _FlacChat()
    with TestClient(server.create_app(chat, flac=True, sample_rates=(8000, 24000), speed=True, g711=True)) as c:
        assert c.get("/health").json()["formats"] == ["alaw", "flac", "pcm", "ulaw", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac" and "output.flac" in r.headers["content-disposition"]
        assert r.content == flac.encode(full, 24000) and chat.calls[-1][2]["flac"] is True and chat.calls[-1][2]["pcm16"] is True
        assert "sample_rate" not in chat.calls[-1][2] and "speed" not in chat.calls[-1][2] and "encoding" not in chat.calls[-1][2]
        y, rate = flac_oracle.decode(r.content)
        assert rate == 24000 and np.array_equal(y, full)
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "sample_rate": 8000, "speed": 1.25})
        assert r.status_code == 200 and r.content == flac.encode(full, 8000)
        assert chat.calls[-1][2]["sample_rate"] == 8000 and chat.calls[-1][2]["speed"] == 1.25 and chat.calls[-1][2]["flac"] is True
        assert flac_oracle.decode(r.content)[1] == 8000
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "variable-block-size" in r.text
        for enc in ("ulaw", "alaw", "flac", 7):
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "encoding": enc})
            assert r.status_code == 400 and "ncoding" in r.text, enc
        assert len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav"})                          # no flac: today's call
        assert r.status_code == 200 and r.content == server.pcm16_to_wav_bytes(full) and "flac" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "ulaw"})
        assert r.status_code == 200 and chat.calls[-1][2]["encoding"] == "ulaw" and "flac" not in chat.calls[-1][2]
    with TestClient(server.create_app(chat, flac=True)) as c:                                                      # without g711 too
        assert c.get("/health").json()["formats"] == ["flac", "pcm", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "encoding": "ulaw"})
        assert r.status_code == 400 and "ncoding" in r.text
    chat, bat = _FlacChat(), _FileBatcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, flac=True, sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "sample_rate": 8000})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
        assert r.content == flac.encode(np.arange(100, dtype=np.int16), 8000) and bat.calls[-1] == ("submit", "hello", {"sample_rate": 8000, "flac": True})
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "flac", "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm"})
        assert r.content == np.arange(100, dtype=np.int16).tobytes() and bat.calls[-1] == ("submit", "hello", {}) and not chat.calls


# ---- 6. the batcher on fake pools --------------------------------------------------------------------------------------------------------------
class _FileChat(_EncChat):
    """as _EncChat; a row with the flac flag comes back as the file of the fake's ramp at the row's rate"""

    def decode_to_pcm16(self, hids, ragged=False, **kw):
        out = super().decode_to_pcm16(hids, ragged, **{k: v for k, v in kw.items() if k != "flac"})
        self.group_calls[-1] = (len(hids), ragged, dict(kw))
        flags = kw.get("flac", [False] * len(hids))
        rates = kw.get("sample_rate", [24000] * len(hids))
        return [np.frombuffer(flac.encode(p, r), np.uint8) if f else p for p, f, r in zip(out, flags, rates)]


def test_requests_with_and_without_flac_due_at_one_poll_share_one_decode():
    lock = threading.Lock()
    chat = _FileChat()
    holder = {}
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _GroupPool(3, lock)), streams=True, ragged_decode=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            b.submit_stream("x", _Params(48), flac=True)
        with pytest.raises(ValueError, match="encoding"):
            b.submit("x", _Params(48), flac=True, encoding="ulaw")
        with pytest.raises(ValueError, match="sample rate"):
            b.submit("x", _Params(48), flac=True, sample_rate=70000)
        with lock:       # admitted together, the same length: they finish at the same poll
            futs = [b.submit("A", _Params(40)), b.submit("B", _Params(40), flac=True), b.submit("C", _Params(40), encoding="alaw")]
        res = [f.result(timeout=30) for f in futs]
        pcm = (np.arange(40) * 100).astype(np.int16)
        assert np.array_equal(res[0], pcm) and res[0].dtype == np.int16 and res[2].dtype == np.uint8 and len(res[2]) == 40
        assert res[1].dtype == np.uint8 and res[1].tobytes() == flac.encode(pcm, 24000)
        assert chat.group_calls == [(3, True, {"encoding": [None, None, "alaw"], "flac": [False, True, False]})]      # ONE decode call
        occ = b.occupancy()
        assert occ["decode_calls"] == 1 and occ["flac_encoded"] == 1 and occ["companded"] == 1
        assert np.array_equal(b.submit("D", _Params(16)).result(timeout=30), (np.arange(16) * 100).astype(np.int16))
        assert chat.group_calls[-1] == (1, True, {})                                            # no flag: today's call, no keyword
        assert b.occupancy()["flac_encoded"] == 1
    finally:
        b.close()
    assert not lock.locked()


def test_a_request_decoded_alone_is_encoded_by_the_host_twin():
    from tests.test_stream_pool_host import _FakeChat

    class _WavChat(_FakeChat):
        def __init__(self):
            super().__init__()
            self.wav_calls = []

        def decode_to_wavs(self, hids, **kw):
            self.wav_calls.append(dict(kw))
            return [np.sin(np.arange(5000) * 0.01).astype(np.float32) * 0.25]
    lock = threading.Lock()
    chat = _WavChat()
    holder = {}
    b = SpeechBatcher(chat, 2, lock, make_pool=lambda: holder.setdefault("p", _FakePool(2, lock)), streams=True)
    try:
        plain = b.submit("A", _Params(16)).result(timeout=30)
        file = b.submit("B", _Params(16), flac=True, sample_rate=8000).result(timeout=30)
        assert plain.dtype == np.int16 and file.dtype == np.uint8 and chat.wav_calls == [{}, {"sample_rate": 8000}]
        y, rate = flac_oracle.decode(file.tobytes())
        assert rate == 8000 and np.array_equal(y, plain) and file.size <= flac.bound(plain.size)
    finally:
        b.close()
    assert not lock.locked()

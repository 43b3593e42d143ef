"""G.711 output, the parts that need no GPU: the NumPy twin against the issue's table hashes, `audioop` and the map's own properties; the
WAV writers field by field and `load_wav(g711=True)`; every refusal of ctts_g711_encode_ranges; the layout code behind the one
device-to-host copy driven with a host stand-in for the kernel; the endpoint on a fake chat; the batcher on fake pools."""
import ctypes as C
import hashlib
import os
import struct
import threading

import numpy as np
import pytest
import torch

from chattts_amd import _lib, audio, g711
from chattts_amd.engine import CodecEngine
from chattts_amd.serving import SpeechBatcher, StreamSpec, stream_schedule
from tests.test_split_pool_host import _EndpointChat
from tests.test_stream_pool_host import _FakeChat, _FakePool, _Params, _piece

ALL = np.arange(-32768, 32768).astype(np.int16)
CODES = np.arange(256, dtype=np.uint8)
SHA = {0: "90c29de505fb68e766118303bd552a16005dcf810873698bee1d8f3b247ce28c", 1: "38488f6fd710f4686360edc4d38639f96c491595ef93f8eb8d62d5e07ca6ce7b"}


# ---- 1. the host twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", [0, 1])
def test_code_table_hash(law):
    t = g711.encode(ALL, law)
    assert t.dtype == np.uint8 and t.shape == ALL.shape and hashlib.sha256(t.tobytes()).hexdigest() == SHA[law]
    assert np.array_equal(t, g711.encode(ALL, ("ulaw", "alaw")[law])) and len(np.unique(t)) == 256


def _scalar(lin: int, law: int) -> int:
    """the issue's definition, step by step, one sample at a time"""
    mag = ~lin if lin < 0 else lin
    if law == 0:
        a = min((mag >> 2) + 33, 0x1FFF)
        seg = 1 + (a >> 6).bit_length()
        code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF))
        return code | (0x80 if lin >= 0 else 0)
    ix = mag >> 4
    if ix > 15:
        e = 1
        while ix > 31:
            ix >>= 1
            e += 1
        ix = ix - 16 + (e << 4)
    return (ix | (0x80 if lin >= 0 else 0)) ^ 0x55


@pytest.mark.parametrize("law", [0, 1])
def test_twin_is_the_definition_sample_by_sample(law):
    xs = np.concatenate([ALL[::37], ALL[:40], ALL[-40:], np.arange(-70, 70).astype(np.int16)])
    assert g711.encode(xs, law).tolist() == [_scalar(int(x), law) for x in xs]


@pytest.mark.parametrize("law", [0, 1])
def test_symmetry_and_idempotence(law):
    t = g711.encode(ALL, law)
    assert np.array_equal(g711.encode(~ALL, law), t ^ 0x80)
    back = g711.encode(g711.expand(CODES, law), law)
    bad = np.nonzero(back != CODES)[0].tolist()
    assert bad == ([0x7F] if law == 0 else [])            # mu-law's negative zero expands to 0, which maps to 0xFF
    if law == 0:
        assert int(g711.expand(CODES, 0)[0x7F]) == 0 and int(back[0x7F]) == 0xFF
    assert g711.expand(CODES, law).dtype == np.int16


def test_agreement_with_audioop():
    audioop = pytest.importorskip("audioop")
    mu = np.frombuffer(audioop.lin2ulaw(ALL.tobytes(), 2), np.uint8)
    diff = np.nonzero(mu != g711.encode(ALL, 0))[0]
    assert len(diff) == 508 and (ALL[diff] < 0).all()      # audioop shifts the two's complement, G.191 the ones' complement
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(ALL.tobytes(), 2), np.uint8), g711.encode(ALL, 1))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(CODES.tobytes(), 2), np.int16), g711.expand(CODES, 0))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(CODES.tobytes(), 2), np.int16), g711.expand(CODES, 1))


def test_twin_refuses_other_types_and_laws():
    for bad in ("mulaw", 2, -1, None, True):
        with pytest.raises(ValueError):
            g711.encode(ALL[:4], bad)
    with pytest.raises(ValueError):
        g711.encode(ALL[:4].astype(np.int32), 0)
    with pytest.raises(ValueError):
        g711.expand(ALL[:4], 0)
    assert g711.encode(np.zeros((2, 0), np.int16), 1).shape == (2, 0)
    assert g711.check_encoding(None) is None and g711.check_encoding("alaw") == "alaw"
    with pytest.raises(ValueError):
        g711.check_encoding("pcm")


# ---- 2. WAV in and out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [100, 101])
def test_wav_bytes_field_by_field(law, tag, n):
    codes = g711.encode(((np.arange(n) * 613) % 60000 - 30000).astype(np.int16), law)
    b = audio.g711_to_wav_bytes(codes, law, 8000)
    assert b[:4] == b"RIFF" and b[8:16] == b"WAVEfmt " and struct.unpack_from("<I", b, 4)[0] == len(b) - 8 and len(b) % 2 == 0
    size, fmt, ch, rate, byte_rate, align, bits, cb = struct.unpack_from("<IHHIIHHH", b, 16)
    assert (size, fmt, ch, rate, byte_rate, align, bits, cb) == (18, tag, 1, 8000, 8000, 1, 8, 0)
    assert b[38:42] == b"fact" and struct.unpack_from("<II", b, 42) == (4, n)
    assert b[50:54] == b"data" and struct.unpack_from("<I", b, 54)[0] == n
    assert b[58: 58 + n] == codes.tobytes() and b[58 + n:] == (b"\0" if n & 1 else b"")      # the pad byte behind an odd chunk
    wav, r = audio.load_wav(b, g711=True)
    assert r == 8000 and wav.dtype == np.float32 and np.array_equal(wav, (g711.expand(codes, law).astype(np.float64) / 32768).astype(np.float32))
    with pytest.raises(ValueError, match="unknown format"):
        audio.load_wav(b)                                  # the default keeps refusing the tag


def test_open_ended_header_and_other_files():
    from chattts_amd import server
    h = server.g711_wav_stream_header("alaw", 16000)
    assert len(h) == 58 and h[4:8] == h[46:50] == h[54:58] == b"\xff" * 4 and struct.unpack_from("<HHI", h, 20) == (6, 1, 16000)
    assert h == audio.g711_wav_header("alaw", 16000, None)
    codes = g711.encode(ALL[::64], "alaw")
    wav, r = audio.load_wav(h + codes.tobytes(), g711=True)            # a stored stream: the data chunk runs to the end
    assert r == 16000 and np.array_equal(wav, g711.expand(codes, 1).astype(np.float32) / 32768)
    stereo = np.stack([codes, codes[::-1]], axis=1).reshape(-1)
    b = bytearray(audio.g711_to_wav_bytes(stereo, "alaw", 8000))
    struct.pack_into("<H", b, 22, 2)
    wav, _ = audio.load_wav(bytes(b), g711=True)
    assert wav.shape == (codes.size,) and np.allclose(wav, (g711.expand(codes, 1) / 32768.0 + g711.expand(codes[::-1], 1) / 32768.0) / 2)
    pcm = server.pcm16_to_wav_bytes(ALL[::64], 8000)                   # integer PCM goes on through the stdlib, with the option too
    a, b2 = audio.load_wav(pcm, g711=True), audio.load_wav(pcm)
    assert a[1] == b2[1] == 8000 and np.array_equal(a[0], b2[0])
    with pytest.raises(ValueError):
        audio.load_wav(b"junk", g711=True)
    with pytest.raises(ValueError, match="no samples"):
        audio.load_wav(audio.g711_to_wav_bytes(np.zeros((0,), np.uint8), "ulaw"), g711=True)


# ---- 3. the C entry's refusals ---------------------------------------------------------------------------------------------------------
def _ranges(rows):
    tab = np.zeros(len(rows), _lib.G711_RANGE)
    for i, r in enumerate(rows):
        tab[i] = (*r, 0, 0)
    return tab, tab.ctypes.data_as(C.c_void_p)


def test_symbol_is_exported_and_declared():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    assert "ctts_g711_encode_ranges" in _lib.SIGNATURES and lib.ctts_g711_encode_ranges is not None
    assert "ctts_g711_encode_ranges(" in header and "} ctts_g711_range;" in header and _lib.G711_RANGE.itemsize == 32
    assert [(_lib.G711_RANGE.fields[k][1]) for k in ("start", "n", "law")] == [0, 8, 16]


def test_encode_ranges_refuses_bad_tables_without_a_device():
    """every refusal comes from the host mirror before anything is launched: the pointers below are never dereferenced, and the
    message names the refusal (a launch on this host would fail with a HIP error instead)"""
    lib = _lib.lib()
    pcm, out = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(rows, n_rng=None, pcm=pcm, out=out, dev=C.c_void_p(4096), host=True):
        tab, p = _ranges(rows)
        return lib.ctts_g711_encode_ranges(pcm, out, dev, p if host else None, len(rows) if n_rng is None else n_rng, None)
    ok = (0, 100, 0)
    for kw in (dict(pcm=None), dict(out=None), dict(dev=None), dict(host=False)):
        assert call([ok], **kw) != 0 and b"null" in lib.ctts_last_error(), kw
    assert call([ok], n_rng=0) != 0 and b"n_rng" in lib.ctts_last_error()
    assert call([ok] * 2, n_rng=-1) != 0 and b"n_rng" in lib.ctts_last_error()
    assert call([(8 * i, 8, 0) for i in range(1025)]) != 0 and b"1024" in lib.ctts_last_error()
    for start in (4, 7, 9, 1001, -8):
        assert call([(start, 10, 1)]) != 0 and b"multiples of 8" in lib.ctts_last_error(), start
    assert call([(8, -1, 0)]) != 0 and b"negative" in lib.ctts_last_error()
    assert call([(0, 17, 0), (16, 8, 1)]) != 0 and b"overlapping" in lib.ctts_last_error()       # overlap by one sample
    assert call([(64, 8, 0), (0, 8, 0)]) != 0 and b"descending" in lib.ctts_last_error()
    assert call([(0, 16, -1), (8, 8, 0)]) != 0 and b"overlapping" in lib.ctts_last_error()       # a skipped range counts too
    for law in (2, -2, 7):
        assert call([(0, 8, law)]) != 0 and b"law" in lib.ctts_last_error(), law
    assert call([ok], out=pcm) != 0 and b"aliases" in lib.ctts_last_error()
    assert call([(0, 4096, 0)], out=C.c_void_p((1 << 20) + 4096)) != 0 and b"aliases" in lib.ctts_last_error()     # inside the samples
    assert call([(0, 4096, 0)], pcm=C.c_void_p((1 << 24) + 2048), out=out) != 0 and b"aliases" in lib.ctts_last_error()   # samples inside out
    assert call([ok], pcm=C.c_void_p((1 << 20) + 2)) != 0 and b"aligned" in lib.ctts_last_error()
    # nothing to convert launches nothing either, and says so by succeeding on pointers no kernel could touch
    assert call([(0, 0, 0), (8, 50, -1)]) == 0


# ---- 4. the layouts behind the one copy, with the host twin standing in for the kernel ----------------------------------------------------
class _HostCodec:
    """the two engine calls the layout code makes, on host tensors: the launch (through the twin, honouring the ranges) and the copy"""

    def __init__(self):
        self.launches, self.copies = [], []

    def g711_encode(self, pcm, ranges, out=None):
        self.launches.append(list(ranges))
        for start, n, law in ranges:
            if law is not None and law != -1:
                assert start % 8 == 0
                out[start: start + n] = torch.from_numpy(g711.encode(pcm[start: start + n].numpy(), law))
        return out

    def to_host(self, t):
        self.copies.append(int(t.numel()))
        return t.numpy().copy()


@pytest.mark.parametrize("laws", [[0, 1, 0], [-1, 0, 1], None])
def test_windows_layout_one_launch_one_copy(laws):
    rng = np.random.default_rng(5)
    n = np.array([9, 4097, 16])
    off = np.zeros(4, np.int64)
    np.cumsum((n + 7) // 8 * 8, out=off[1:])
    keep = [0, 1, 0]
    n_out, n_g, n_keep = int(off[-1]) * 2, ((int(off[-1]) + 15) // 16 * 16 if laws else 0), (int(off[-1]) // 8 + 15) // 16 * 16
    buf = torch.full((n_out + n_g + n_keep,), 0xAA, dtype=torch.uint8)
    pcm = rng.integers(-32768, 32768, int(off[-1])).astype(np.int16)
    buf[:n_out] = torch.from_numpy(pcm.view(np.uint8))
    mask = rng.integers(0, 2, int(n[1])).astype(bool)
    kb = n_out + n_g + int(off[1]) // 8
    buf[kb: kb + (int(n[1]) + 7) // 8] = torch.from_numpy(np.packbits(mask))
    fake = _HostCodec()
    out = CodecEngine._windows_to_host(fake, buf, n_out, n_g, off, n, keep, [0, 1, 2], laws, np.int16, [None] * 3)
    assert len(fake.copies) == 1 and len(fake.launches) == (1 if laws else 0)
    assert fake.copies[0] == (n_g + n_keep if laws and min(laws) >= 0 else buf.numel())      # all companded: the samples stay on the device
    for k in range(3):
        want = pcm[int(off[k]): int(off[k]) + int(n[k])]
        if laws and laws[k] >= 0:
            want = g711.encode(want, laws[k])
        if keep[k]:
            want = want[mask]
        assert out[k].dtype == want.dtype and np.array_equal(out[k], want), k


@pytest.mark.parametrize("encs", [["ulaw", "alaw"], [None, "alaw"]])
def test_groups_blob_unpacks_codes_and_samples(encs):
    starts, kept = np.array([0, 24, 40]), np.array([19, 16], np.int64)
    E, hdr = 40, 16
    pcm = (np.arange(E) * 777 - 15000).astype(np.int16)
    codes = np.concatenate([g711.encode(pcm[0:24], encs[0] or 0), g711.encode(pcm[24:40], encs[1])])
    tail = np.concatenate([kept.view(np.uint8), codes, np.zeros(8, np.uint8)])
    blob = tail if all(encs) else np.concatenate([pcm.view(np.uint8), tail])
    got = CodecEngine.unpack_groups(blob, starts, encs)
    for g, e in enumerate(encs):
        want = pcm[int(starts[g]): int(starts[g]) + int(kept[g])]
        assert np.array_equal(got[g], want if e is None else g711.encode(want, e)) and got[g].dtype == (np.int16 if e is None else np.uint8)
    plain = np.concatenate([kept.view(np.uint8), pcm.view(np.uint8)])
    assert all(np.array_equal(a, pcm[int(s): int(s) + int(k)]) for a, s, k in zip(CodecEngine.unpack_groups(plain, starts), starts, kept))


def test_infer_refuses_encoding_without_pcm16():
    from chattts_amd.core import Chat
    chat = Chat()
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(["x"], encoding="ulaw")
    with pytest.raises(ValueError, match="unknown encoding"):
        chat.infer(["x"], pcm16=True, encoding="mulaw")


# ---- 5. the endpoint on a fake chat ----------------------------------------------------------------------------------------------------
class _G711Chat(_EndpointChat):
    """as _EndpointChat; with `encoding` the results are the codes of the same samples"""

    def infer(self, text, stream=False, **kw):
        out = super().infer(text, stream, **kw)
        enc = kw.get("encoding")
        if enc is None:
            return out
        return (g711.encode(c, enc) for c in out) if stream else [g711.encode(w, enc) for w in out]


class _CodeBatcher:
    streams, refine = True, False

    def __init__(self):
        self.lock, self.calls = threading.Lock(), []

    def submit(self, text, params, **kw):
        from concurrent.futures import Future
        self.calls.append(("submit", text, kw))
        f = Future()
        f.set_result(g711.encode(np.arange(100, dtype=np.int16), kw["encoding"]) if "encoding" in kw else np.arange(100, dtype=np.int16))
        return f

    def submit_stream(self, text, params, **kw):
        self.calls.append(("stream", text, kw))
        parts = [np.arange(100, dtype=np.int16), np.zeros((0,), np.int16), np.arange(100, 250, dtype=np.int16)]

        class _It:
            def __init__(self):
                self.it = iter([g711.encode(p, kw["encoding"]) if "encoding" in kw else p for p in parts])

            def __iter__(self):
                return self

            def __next__(self):
                return next(self.it)

            def close(self):
                pass
        return _It()

    def occupancy(self):
        return {}


def test_endpoint_without_the_option_is_todays():
    from starlette.testclient import TestClient
    from chattts_amd import server
    chat = _G711Chat()
    with TestClient(server.create_app(chat)) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "ulaw"})
        assert r.status_code == 400 and "Unsupported audio format: ulaw, supported formats: pcm, wav" in r.text and not chat.calls
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": "ulaw"})     # an unknown key: ignored
        assert r.status_code == 200 and "encoding" not in chat.calls[-1][2]
        assert r.content == server.pcm16_to_wav_bytes(np.arange(600, dtype=np.int16))
        assert c.get("/health").json()["formats"] == ["pcm", "wav"]


def test_endpoint_serves_g711_raw_and_wav():
    from starlette.testclient import TestClient
    from chattts_amd import server
    full = np.arange(600, dtype=np.int16)
    chat = _G711Chat()
    with TestClient(server.create_app(chat, g711=True, sample_rates=(8000, 24000), stream_sample_rates=(8000,))) as c:
        assert c.get("/health").json()["formats"] == ["alaw", "pcm", "ulaw", "wav"]
        for law, media in (("ulaw", "audio/pcmu"), ("alaw", "audio/pcma")):
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": law, "sample_rate": 8000})
            assert r.status_code == 200 and r.headers["content-type"].lower() == media and r.content == g711.encode(full, law).tobytes()
            assert chat.calls[-1][2]["encoding"] == law and chat.calls[-1][2]["sample_rate"] == 8000 and chat.calls[-1][2]["pcm16"] is True
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": law, "sample_rate": 8000})
            assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
            assert r.content == audio.g711_to_wav_bytes(g711.encode(full, law), law, 8000)
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": law, "sample_rate": 8000, "stream": True})
            assert r.status_code == 200 and r.content == server.g711_wav_stream_header(law, 8000) + g711.encode(full, law).tobytes()
            assert chat.calls[-1][1] and chat.calls[-1][2]["encoding"] == law and chat.calls[-1][2]["stream_resample"] is True
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": law, "stream": True})       # raw stream at 24 kHz
            assert r.status_code == 200 and r.content == g711.encode(full, law).tobytes() and "sample_rate" not in chat.calls[-1][2]
        n = len(chat.calls)
        for body in ({"response_format": "wav", "encoding": "mp3"}, {"response_format": "ulaw", "encoding": "alaw"},
                     {"response_format": "pcm", "encoding": "ulaw"}, {"response_format": "wav", "encoding": 7}):
            r = c.post("/v1/audio/speech", json={"input": "hello", **body})
            assert r.status_code == 400 and "ncoding" in r.text, body
        assert len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav"})                         # no encoding: today's call
        assert r.status_code == 200 and r.content == server.pcm16_to_wav_bytes(full) and "encoding" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm", "stream": True})
        assert r.status_code == 200 and r.content == full.tobytes() and "encoding" not in chat.calls[-1][2]
    chat, bat = _G711Chat(), _CodeBatcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, g711=True, stream_sample_rates=(8000,), sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "ulaw", "sample_rate": 8000, "stream": True})
        assert r.status_code == 200 and r.content == g711.encode(np.arange(250, dtype=np.int16), "ulaw").tobytes()
        assert bat.calls[-1] == ("stream", "hello", {"sample_rate": 8000, "encoding": "ulaw"})
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": "alaw", "stream": True})
        assert r.content == server.g711_wav_stream_header("alaw", 24000) + g711.encode(np.arange(250, dtype=np.int16), "alaw").tobytes()
        assert bat.calls[-1] == ("stream", "hello", {"encoding": "alaw"})
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": "alaw", "sample_rate": 8000})
        assert r.content == audio.g711_to_wav_bytes(g711.encode(np.arange(100, dtype=np.int16), "alaw"), "alaw", 8000)
        assert bat.calls[-1] == ("submit", "hello", {"sample_rate": 8000, "encoding": "alaw"})
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm"})
        assert r.content == np.arange(100, dtype=np.int16).tobytes() and bat.calls[-1] == ("submit", "hello", {}) and not chat.calls


def test_voice_upload_takes_telephone_recordings_only_with_the_option():
    from starlette.testclient import TestClient
    from chattts_amd import server

    class _VoiceChat(_EndpointChat):
        def sample_audio_speaker(self, wav, rate):
            self.clip = (np.asarray(wav), rate)
            raise ValueError("stop here")              # the route answers 400 with this text: the clip got through load_wav
    codes = g711.encode(ALL[::16], "ulaw")
    body = audio.g711_to_wav_bytes(codes, "ulaw", 8000)
    chat = _VoiceChat()
    with TestClient(server.create_app(chat, voice_upload=True)) as c:
        r = c.post("/v1/audio/voices?name=tel", content=body)
        assert r.status_code == 400 and "bad WAV upload" in r.text and "unknown format: 7" in r.text
    with TestClient(server.create_app(chat, voice_upload=True, g711=True)) as c:
        r = c.post("/v1/audio/voices?name=tel", content=body)
        assert r.status_code == 400 and "stop here" in r.text
        assert chat.clip[1] == 8000 and np.array_equal(chat.clip[0], g711.expand(codes, 0).astype(np.float32) / 32768)


# ---- 6. the batcher on fake pools ------------------------------------------------------------------------------------------------------
class _EncChat(_FakeChat):
    """as _FakeChat; every decode call is recorded with its keywords, and a companded piece is the twin's codes of the fake's ramp.  One
    call stands for one decoder pass and -- on the real Chat -- one ctts_g711_encode_ranges launch (CodecEngine.decode_windows /
    Chat._decode_to_g711_ragged convert all ranges of a call together)."""

    def __init__(self):
        super().__init__()
        self.kw_calls, self.group_calls = [], []

    def decode_windows_pcm16(self, store, windows, **kw):
        self.window_calls.append(list(windows))
        self.kw_calls.append(dict(kw))
        encs = kw.get("encodings", [None] * len(windows))
        pieces = [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]
        return [p if e is None else g711.encode(p, e) for p, e in zip(pieces, encs)]

    def decode_to_pcm16(self, hids, ragged=False, **kw):
        self.group_calls.append((len(hids), ragged, dict(kw)))
        encs = kw.get("encoding", [None] * len(hids))
        pcm = [(np.arange(int(h.shape[0])) * 100).astype(np.int16) for h in hids]
        return [p if e is None else g711.encode(p, e) for p, e in zip(pcm, encs)]


class _GroupPool(_FakePool):
    """as _FakePool, for a batcher with ragged_decode: the results of a poll are handed out as one group"""

    def run(self, between=None, grouped=False, events=False):
        for got in _FakePool.run(self, between, grouped, events=True):
            if isinstance(got, tuple):
                self._late = getattr(self, "_late", []) + [got]
                continue
            if getattr(self, "_late", None):
                late, self._late = self._late, []
                yield late
            yield got
        if getattr(self, "_late", None):
            yield self._late
            self._late = []


def test_streams_with_three_encodings_due_at_one_poll_share_one_call():
    lock = threading.Lock()
    chat = _EncChat()
    holder = {}
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True)
    try:
        with pytest.raises(ValueError):
            b.submit_stream("x", _Params(48), encoding="g711")
        with pytest.raises(ValueError):
            b.submit("x", _Params(48), encoding="mulaw")
        with lock:       # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = {None: b.submit_stream("A", _Params(96)), "ulaw": b.submit_stream("B", _Params(96), encoding="ulaw"),
                       "alaw": b.submit_stream("C", _Params(96), encoding="alaw")}
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in streams.items()]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        sched = stream_schedule([], 96, True, StreamSpec(24, 12000, 0))
        for enc, tag in zip(streams, "ABC"):
            want = [_piece(ord(tag), p, lo, hi) for p, lo, hi, _ in sched]
            want = want if enc is None else [g711.encode(w, enc) for w in want]
            assert len(got[enc]) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[enc], want)), enc
        # one decode call per poll for the three streams -- hence one companding call --, one encoding per window in the windows' order
        occ = b.occupancy()
        polls = sorted({p for p, _, _, _ in sched})             # the prefixes at which chunks fall due (the last one: two per stream)
        assert len(chat.window_calls) == occ["stream_decode_calls"] == len(polls) < len(sched)
        for w, kw in zip(chat.window_calls, chat.kw_calls):
            assert {x[0] for x in w} == {0, 1, 2} and kw == {"encodings": [{0: None, 1: "ulaw", 2: "alaw"}[x[0]] for x in w]}, kw
        assert occ["companded"] == 2 * len(sched) and occ["stream_chunks"] == 3 * len(sched)
        n_calls = len(chat.kw_calls)
        assert sum(len(c) for c in b.submit_stream("D", _Params(48))) == 256 * 95             # no encoding: today's call, no keyword
        assert len(chat.kw_calls) > n_calls and all(kw == {} for kw in chat.kw_calls[n_calls:])
        assert b.occupancy()["companded"] == 2 * len(sched)
    finally:
        b.close()
    assert not lock.locked()


def test_three_requests_with_three_encodings_due_at_one_poll_share_one_decode():
    lock = threading.Lock()
    chat = _EncChat()
    holder = {}
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _GroupPool(3, lock)), streams=True, ragged_decode=True)
    try:
        with lock:       # admitted together, the same length: they finish at the same poll
            futs = [b.submit("A", _Params(40)), b.submit("B", _Params(40), encoding="ulaw"), b.submit("C", _Params(40), encoding="alaw")]
        res = [f.result(timeout=30) for f in futs]
        pcm = (np.arange(40) * 100).astype(np.int16)
        assert np.array_equal(res[0], pcm) and res[0].dtype == np.int16
        assert np.array_equal(res[1], g711.encode(pcm, "ulaw")) and np.array_equal(res[2], g711.encode(pcm, "alaw")) and res[1].dtype == np.uint8
        assert chat.group_calls == [(3, True, {"encoding": [None, "ulaw", "alaw"]})]            # ONE decode call, one companding call
        occ = b.occupancy()
        assert occ["decode_calls"] == 1 and occ["companded"] == 2
        assert np.array_equal(b.submit("D", _Params(16)).result(timeout=30), (np.arange(16) * 100).astype(np.int16))
        assert chat.group_calls[-1] == (1, True, {})                                            # no encoding: today's call
    finally:
        b.close()
    assert not lock.locked()

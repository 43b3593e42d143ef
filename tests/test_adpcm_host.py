"""IMA ADPCM output, the parts that need no GPU: the tables and the step against CPython's `audioop` (a codec this project did not write),
the NumPy twin block by block over tests/adpcm_cases.py, the WAV container and its reader, the quality of the block rule against
`audioop`'s single carried chain, every refusal of ctts_adpcm_encode_ranges, the argument rules of Chat and the batcher, the endpoint on
a fake chat."""
import audioop
import ctypes as C
import os
import struct
import threading

import numpy as np
import pytest

from chattts_amd import _lib, adpcm, audio
from chattts_amd.serving import SpeechBatcher
from tests import adpcm_cases as AC
from tests.test_g711_host import _EncChat, _GroupPool
from tests.test_split_pool_host import _EndpointChat
from tests.test_stream_pool_host import _FakePool, _Params


def _swap(b: bytes) -> np.ndarray:
    """audioop puts the first sample of a byte in the high nibble, the WAV form in the low one"""
    a = np.frombuffer(b, np.uint8)
    return (a >> 4) | ((a & 15) << 4)


# ---- 1. the tables and the step ---------------------------------------------------------------------------------------------------------
def test_tables_and_decoder_against_audioop_at_every_index():
    assert len(adpcm.STEP) == 89 and adpcm.IDX == (-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8)
    assert list(adpcm.STEP) == sorted(set(adpcm.STEP)) and adpcm.STEP[0] == 7 and adpcm.STEP[88] == 32767
    for idx in range(89):
        for code in range(16):
            # two samples from (0, idx): the first shows STEP[idx], the second (code 7) the index the first code led to
            ref, state = audioop.adpcm2lin(bytes([(code << 4) | 7]), 2, (0, idx))
            blk = np.zeros(256, np.uint8)
            blk[2], blk[4] = idx, code | (7 << 4)
            got = adpcm.decode_blocks(blk, 3, 8000)
            assert got[0] == 0 and got[1:].tolist() == np.frombuffer(ref, np.int16).tolist(), (idx, code)
    assert [adpcm.index0(d) for d in (0, 7, 8, 9, 32767, 32768, 65535, -9)] == [0, 0, 1, 2, 88, 88, 88, 2]
    for i, s in enumerate(adpcm.STEP):
        assert adpcm.index0(s) == i and adpcm.index0(s + 1) == min(i + 1, 88)


def test_block_sizes():
    assert [adpcm.align(r) for r in (8000, 11025, 16000, 22049, 22050, 24000, 32000, 33074, 33075, 44100, 48000)] == \
        [256, 256, 256, 256, 512, 512, 512, 512, 768, 1024, 1024]
    assert [adpcm.samples_per_block(r) for r in AC.RATES] == [505, 1017, 2041]
    assert [adpcm.n_blocks(n, 8000) for n in (0, 1, 505, 506, 1010, 1011)] == [0, 1, 1, 2, 2, 3]
    for bad in (0, -8000, 24000.0, True, None, "8000", 1 << 31):
        with pytest.raises(ValueError, match="sample rate"):
            adpcm.align(bad)


# ---- 2. the twin, block by block, against audioop ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", AC.RATES)
def test_every_block_equals_audioop_from_its_header_state(rate):
    A, S = adpcm.align(rate), adpcm.samples_per_block(rate)
    for name, x in AC.cases(rate):
        blocks, preds = adpcm.encode_blocks(x, rate, trace=True)
        nb = adpcm.n_blocks(len(x), rate)
        assert blocks.dtype == np.uint8 and blocks.size == nb * A and nb == -(-len(x) // S), name
        xp = np.concatenate([x, np.full(nb * S - len(x), x[-1], np.int16)])                # positions at or beyond n read as x[n - 1]
        dec = adpcm.decode_blocks(blocks, nb * S, rate)
        for b in range(nb):
            blk, B = xp[b * S: (b + 1) * S], blocks[b * A: (b + 1) * A]
            i0 = adpcm.index0(int(blk[1]) - int(blk[0]))
            assert struct.unpack("<hBB", B[:4].tobytes()) == (int(blk[0]), i0, 0), (name, b)
            ref, _ = audioop.lin2adpcm(blk[1:].tobytes(), 2, (int(blk[0]), i0))
            assert np.array_equal(B[4:], _swap(ref)), (name, b)
            back, _ = audioop.adpcm2lin(ref, 2, (int(blk[0]), i0))
            assert np.array_equal(dec[b * S + 1: (b + 1) * S], np.frombuffer(back, np.int16)) and dec[b * S] == blk[0], (name, b)
        assert np.array_equal(preds, dec), name                                              # the encoder's predictor is the decoder's output
        assert np.array_equal(adpcm.decode_blocks(blocks, len(x), rate), dec[: len(x)])
        if name == "zeros":
            assert not blocks.any()
        if name == "lo_hi":
            assert blocks[2] == 88
        if name == "square":
            assert dec.max() == 32767 and dec.min() == -32768 and blocks[2] == 0          # the predictor reaches both rails from index0 0


def test_twin_refusals():
    with pytest.raises(ValueError, match="no samples"):
        adpcm.encode_blocks(np.zeros(0, np.int16), 8000)
    with pytest.raises(ValueError, match="no samples"):
        adpcm.encode(np.zeros(0, np.int16), 8000)
    with pytest.raises(ValueError, match="int16"):
        adpcm.encode(np.zeros(4, np.float32), 8000)
    with pytest.raises(ValueError, match="int16"):
        adpcm.encode_blocks(np.zeros((2, 4), np.int16), 8000)
    with pytest.raises(ValueError, match="multiples"):
        adpcm.decode_blocks(np.zeros(255, np.uint8), 1, 8000)
    with pytest.raises(ValueError, match="hold up to"):
        adpcm.decode_blocks(np.zeros(256, np.uint8), 506, 8000)
    bad = np.zeros(256, np.uint8)
    bad[2] = 89
    with pytest.raises(ValueError, match="beyond 88"):
        adpcm.decode_blocks(bad, 5, 8000)
    with pytest.raises(ValueError, match="blocks of"):
        adpcm.wav_bytes(np.zeros(256, np.uint8), 506, 8000)
    with pytest.raises(ValueError):
        adpcm.wav_bytes(np.zeros(0, np.uint8), 0, 8000)
    # behind a decode an empty result is the bare header, as FLAC's is
    bare = adpcm.behind_decode(np.zeros(0, np.uint8), 0, 24000)
    assert bare.dtype == np.uint8 and bare.size == 60 and bare.tobytes() == adpcm.encode_result(np.zeros(0, np.int16), 24000).tobytes()
    assert struct.unpack_from("<I", bare.tobytes(), 4)[0] == 52 and struct.unpack_from("<I", bare.tobytes(), 48)[0] == 0
    assert struct.unpack_from("<I", bare.tobytes(), 56)[0] == 0


# ---- 3. the file ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", AC.RATES)
def test_file_header_byte_by_byte_and_the_reader(rate):
    A, S = adpcm.align(rate), adpcm.samples_per_block(rate)
    for n in (1, S, S + 1, 3 * S + 11):
        x = AC.noise(n, n)
        f = adpcm.encode(x, rate)
        nb = -(-n // S)
        assert len(f) == 60 + nb * A == adpcm.HEADER_BYTES + nb * A
        assert f[:4] == b"RIFF" and struct.unpack_from("<I", f, 4)[0] == len(f) - 8 and f[8:16] == b"WAVEfmt "
        assert struct.unpack_from("<IHHIIHHHH", f, 16) == (20, 0x0011, 1, rate, rate * A // S, A, 4, 2, S)
        assert f[40:44] == b"fact" and struct.unpack_from("<II", f, 44) == (4, n)
        assert f[52:56] == b"data" and struct.unpack_from("<I", f, 56)[0] == nb * A
        assert f[60:] == adpcm.encode_blocks(x, rate).tobytes()
        assert adpcm.wav_bytes(adpcm.encode_blocks(x, rate), n, rate).tobytes() == f
        y, r = adpcm.parse_wav(f)
        assert r == rate and y.dtype == np.int16 and np.array_equal(y, adpcm.decode_blocks(f[60:], n, rate))
        w, r2 = audio.load_wav(f, adpcm=True)
        assert r2 == rate and w.dtype == np.float32 and np.array_equal(w, (y.astype(np.float64) / 32768.0).astype(np.float32))


def test_load_wav_refusals_and_the_default():
    x = AC.noise(700, 3)
    f = bytearray(adpcm.encode(x, 8000))
    with pytest.raises(ValueError, match="not an integer-PCM WAV"):             # without the flag: as today
        audio.load_wav(bytes(f))
    with pytest.raises(ValueError, match="not an integer-PCM WAV"):
        audio.load_wav(bytes(f), g711=True)
    stereo = bytearray(f)
    struct.pack_into("<H", stereo, 22, 2)
    with pytest.raises(ValueError, match="2 channels"):
        audio.load_wav(bytes(stereo), adpcm=True)
    for at, fmt, val in ((32, "<H", 512), (34, "<H", 8), (38, "<H", 504), (38, "<H", 1017)):      # align, bits, samples per block
        bad = bytearray(f)
        struct.pack_into(fmt, bad, at, val)
        with pytest.raises(ValueError, match="disagrees with its block size"):
            audio.load_wav(bytes(bad), adpcm=True)
    short = bytearray(f)
    struct.pack_into("<I", short, 48, 2 * 505 + 1)                             # `fact` beyond the blocks
    with pytest.raises(ValueError, match="fact"):
        audio.load_wav(bytes(short), adpcm=True)
    with pytest.raises(ValueError, match="no samples"):
        audio.load_wav(bytes(f[:60]), adpcm=True)
    assert adpcm.parse_wav(b"RIFFxxxxWAVE") is None and adpcm.parse_wav(b"nothing") is None
    # an integer-PCM file goes on as without the option
    pcm_file = audio.pcm_to_wav_bytes(np.linspace(-0.5, 0.5, 64, dtype=np.float32), 16000)
    a, b = audio.load_wav(pcm_file, adpcm=True), audio.load_wav(pcm_file)
    assert a[1] == b[1] == 16000 and np.array_equal(a[0], b[0])
    # a file of another encoder: another block size, no `fact` chunk
    blocks = adpcm.encode_blocks(x, 8000)[:256]
    other = (b"RIFF" + struct.pack("<I", 4 + 28 + 8 + 256) + b"WAVEfmt " + struct.pack("<IHHIIHHHH", 20, 0x11, 1, 44100, 22000, 256, 4, 2, 505)
             + b"data" + struct.pack("<I", 256) + blocks.tobytes())
    y, r = adpcm.parse_wav(other)
    assert r == 44100 and np.array_equal(y, adpcm.decode_blocks(blocks, 505, 8000))


# ---- 4. the quality of the block rule -------------------------------------------------------------------------------------------------------
def _snr(x, y) -> float:
    x, y = x.astype(np.float64), y.astype(np.float64)
    return float(10.0 * np.log10((x ** 2).sum() / ((x - y) ** 2).sum()))


@pytest.mark.parametrize("rate", AC.RATES)
def test_block_rule_costs_at_most_3_db_against_audioops_carried_chain(rate):
    """The start index of every block is a function of its first difference instead of the chain's running index: a block spends a few
    samples adapting.  The bar is a condition on the definition: on the 4 s burst signal the SNR of decode(encode(x)) is at most 3 dB
    below that of audioop's single chain over the same samples.  Measured: 12.60 / 30.43 / 38.15 dB against the chain's 12.57 / 30.43 /
    38.13 dB at 8000 / 24000 / 48000 Hz (505 / 1017 / 2041 samples per block)."""
    x = AC.burst(rate)
    ours = adpcm.decode_blocks(adpcm.encode_blocks(x, rate), len(x), rate)
    codes, _ = audioop.lin2adpcm(x.tobytes(), 2, None)
    chain = np.frombuffer(audioop.adpcm2lin(codes, 2, None)[0], np.int16)
    a, b = _snr(x, ours), _snr(x, chain)
    print(f"adpcm block rule at {rate} Hz: {a:.2f} dB, audioop's carried chain: {b:.2f} dB")
    assert a >= b - 3.0, (rate, a, b)


# ---- 5. the C entry -------------------------------------------------------------------------------------------------------------------------
def _table(rows):
    tab = np.zeros(len(rows), _lib.ADPCM_RANGE)
    blocks = nbytes = 0
    for i, r in enumerate(rows):
        start, n, rate = r[:3]
        ci = r[3] if len(r) > 3 else -1
        tab[i] = (start, n, r[4] if len(r) > 4 else blocks, r[5] if len(r) > 5 else nbytes, rate, ci, 0)
        if rate > 0:
            nb = adpcm.n_blocks(n, rate)
            blocks, nbytes = blocks + nb, nbytes + nb * adpcm.align(rate)
    return tab


def test_symbol_is_exported_and_declared():
    lib = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "chattts_amd.h")) as f:
        header = f.read()
    for name in ("ctts_adpcm_encode_ranges", "ctts_adpcm_encode_sizes"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert "} ctts_adpcm_range;" in header and _lib.ADPCM_RANGE.itemsize == 48
    assert [_lib.ADPCM_RANGE.fields[k][1] for k in ("start", "n", "block0", "byte0", "rate", "count_idx", "reserved")] == [0, 8, 16, 24, 32, 36, 40]
    from chattts_amd import build
    assert "adpcm.hip" in build.SOURCES
    with open(os.path.join(_lib.HERE, "csrc", "kernels.hpp")) as f:
        assert "struct AdpcmRange" in f.read()
    sizes = (C.c_int64 * 3)()
    tab = _table([(0, 506, 8000), (512, 10, 0), (528, 2041, 48000), (2576, 1, 24000)])
    assert tab["block0"].tolist() == [0, 2, 2, 3] and tab["byte0"].tolist() == [0, 512, 512, 1536]
    assert lib.ctts_adpcm_encode_sizes(tab.ctypes.data_as(C.c_void_p), 4, sizes) == 0
    assert list(sizes) == [4, 2 * 256 + 1024 + 512, 32]


def test_encode_ranges_refuses_bad_tables_without_a_device():
    """every refusal comes from the host table before anything is launched: the pointers below are never dereferenced, and the message
    names the refusal"""
    lib = _lib.lib()
    pcm, out, used = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)

    def call(rows, n_rng=None, pcm=pcm, out=out, used=used, dev=C.c_void_p(4096), host=True, counts=None, out_bytes=1 << 20, used_bytes=1 << 16):
        tab = _table(rows)
        return lib.ctts_adpcm_encode_ranges(pcm, counts, dev, tab.ctypes.data_as(C.c_void_p) if host else None,
                                            len(rows) if n_rng is None else n_rng, out, out_bytes, used, used_bytes, None)
    ok = (0, 100, 24000)
    for kw in (dict(pcm=None), dict(out=None), dict(dev=None), dict(host=False), dict(used=None)):
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
    assert call([(0, 8, -1)]) != 0 and b"rate" in lib.ctts_last_error()
    for ci in (-2, 65536):
        assert call([(0, 8, 24000, ci)], counts=C.c_void_p(1 << 12)) != 0 and b"count_idx" in lib.ctts_last_error(), ci
    assert call([(0, 1018, 24000, -1, 0, 0), (1024, 8, 24000, -1, 1, 1024)]) != 0 and b"block0" in lib.ctts_last_error()   # the first owns two blocks
    assert call([(0, 8, 24000, -1, 3, 0)]) != 0 and b"block0" in lib.ctts_last_error()
    assert call([(0, 1018, 24000, -1, 0, 0), (1024, 8, 8000, -1, 2, 512)]) != 0 and b"byte0" in lib.ctts_last_error()      # ... and 1024 bytes
    assert call([(0, 8, 24000, -1, 0, 256)]) != 0 and b"byte0" in lib.ctts_last_error()
    big = [(i * (1 << 31), (1 << 31) - 8, 8000) for i in range(512)]                                                      # 2^31 blocks or more
    assert call(big, out_bytes=1 << 60) != 0 and b"2^31" in lib.ctts_last_error()
    assert call([(0, 1017, 24000)], out_bytes=511) != 0 and b"out of capacity" in lib.ctts_last_error()
    assert call([(0, 8, 24000), (8, 8, 24000)], used_bytes=8) != 0 and b"out of capacity" in lib.ctts_last_error()
    assert call([ok], out=pcm) != 0 and b"aliases" in lib.ctts_last_error()
    assert call([(0, 4096, 24000)], out=C.c_void_p((1 << 20) + 4096)) != 0 and b"aliases" in lib.ctts_last_error()     # inside the samples
    assert call([(0, 4096, 24000)], pcm=C.c_void_p((1 << 24) + 2048)) != 0 and b"aliases" in lib.ctts_last_error()      # samples inside out
    assert call([ok], pcm=C.c_void_p((1 << 20) + 2)) != 0 and b"aligned" in lib.ctts_last_error()
    assert call([ok], out=C.c_void_p((1 << 24) + 8)) != 0 and b"aligned" in lib.ctts_last_error()
    assert call([ok], used=C.c_void_p((1 << 28) + 4)) != 0 and b"aligned" in lib.ctts_last_error()
    sizes = (C.c_int64 * 3)()
    assert lib.ctts_adpcm_encode_sizes(None, 1, sizes) != 0 and b"null" in lib.ctts_last_error()
    assert lib.ctts_adpcm_encode_sizes(_table([ok]).ctypes.data_as(C.c_void_p), 1, None) != 0 and b"null" in lib.ctts_last_error()
    assert lib.ctts_adpcm_encode_sizes(_table([(4, 8, 24000)]).ctypes.data_as(C.c_void_p), 1, sizes) != 0 and b"multiples of 8" in lib.ctts_last_error()
    # nothing to encode launches nothing either, and says so by succeeding on pointers no kernel could touch
    assert call([(0, 0, 24000), (8, 50, 0)]) == 0


# ---- 6. the argument rules ------------------------------------------------------------------------------------------------------------------
def test_infer_and_decode_calls_refuse_adpcm_without_pcm16_with_an_encoding_flac_or_streamed():
    from chattts_amd import g711
    from chattts_amd.core import Chat
    chat = Chat()
    with pytest.raises(ValueError, match="pcm16"):
        chat.infer(["x"], adpcm=True)
    with pytest.raises(ValueError, match="encoding"):
        chat.infer(["x"], pcm16=True, adpcm=True, encoding="ulaw")
    with pytest.raises(ValueError, match="flac"):
        chat.infer(["x"], pcm16=True, adpcm=True, flac=True)
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(["x"], pcm16=True, adpcm=True, stream=True)
    with pytest.raises(ValueError, match="sample rate"):
        chat.infer(["x"], pcm16=True, adpcm=True, sample_rate=0)
    f = Chat._adpcm_flags
    assert f(None, 3, None, None, True, "t") is None and f(False, 3, None, None, True, "t") is None and f([False] * 3, 3, "ulaw", None, True, "t") is None
    assert f(True, 2, None, None, False, "t") == [True, True]
    assert f([True, False], 2, [None, "alaw"], None, True, "t") == [True, False]          # a row is one or the other
    for args in ((True, 2, "ulaw", None, True), ([True, False], 2, ["ulaw", None], None, True), ([True], 2, None, None, True),
                 ([True, False], 2, None, None, False), (True, 2, None, [True, False], True), ([False, True], 2, None, [True, False], True)):
        with pytest.raises(ValueError):
            f(*args, "t")
    # the unknown-encoding messages are what they were: adpcm is a flag of its own, no encoding value
    with pytest.raises(ValueError) as e:
        g711.check_encoding("adpcm")
    assert str(e.value) == "unknown encoding 'adpcm': None (16-bit PCM), \"ulaw\" or \"alaw\""
    with pytest.raises(ValueError) as e:
        chat.infer(["x"], pcm16=True, encoding="adpcm")
    assert str(e.value) == "unknown encoding 'adpcm': None (16-bit PCM), \"ulaw\" or \"alaw\""


# ---- 7. the endpoint on a fake chat ------------------------------------------------------------------------------------------------------------
class _AdpcmChat(_EndpointChat):
    """as _EndpointChat; with `adpcm` the results are the files of the same samples at the call's rate"""

    def infer(self, text, stream=False, **kw):
        out = super().infer(text, stream, **{k: v for k, v in kw.items() if k != "adpcm"})
        self.calls[-1] = (*self.calls[-1][:2], dict(kw), *self.calls[-1][3:])
        if not kw.get("adpcm"):
            return out
        assert not stream
        return [np.frombuffer(adpcm.encode(w, kw.get("sample_rate", 24000)), np.uint8) for w in out]


class _FileBatcher:
    streams, refine = True, False

    def __init__(self):
        self.lock, self.calls = threading.Lock(), []

    def submit(self, text, params, **kw):
        from concurrent.futures import Future
        self.calls.append(("submit", text, kw))
        pcm = np.arange(100, dtype=np.int16)
        f = Future()
        f.set_result(np.frombuffer(adpcm.encode(pcm, kw.get("sample_rate", 24000)), np.uint8) if kw.get("adpcm") else pcm)
        return f

    def submit_stream(self, text, params, **kw):
        raise AssertionError("an adpcm request never reaches the streamed path")

    def occupancy(self):
        return {}


def test_endpoint_without_the_switch_is_todays():
    from starlette.testclient import TestClient
    from chattts_amd import server
    chat = _AdpcmChat()
    with TestClient(server.create_app(chat)) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm"})
        assert r.status_code == 400 and "Unsupported audio format: adpcm, supported formats: pcm, wav" in r.text and not chat.calls
        assert c.get("/health").json() == {"status": "healthy", "model_loaded": True, "formats": ["pcm", "wav"]}
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav"})
        assert r.status_code == 200 and "adpcm" not in chat.calls[-1][2]
    with TestClient(server.create_app(chat, g711=True, flac=True)) as c:
        assert c.get("/health").json()["formats"] == ["alaw", "flac", "pcm", "ulaw", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav", "encoding": "adpcm"})
        assert r.status_code == 400 and "Unsupported encoding: adpcm, supported: alaw, ulaw" in r.text


def test_endpoint_serves_adpcm_serially_and_batched():
    from starlette.testclient import TestClient
    from chattts_amd import server
    full = np.arange(600, dtype=np.int16)
    chat = _AdpcmChat()
    with TestClient(server.create_app(chat, adpcm=True, sample_rates=(8000, 24000), speed=True, g711=True, loudness=True)) as c:
        assert c.get("/health").json()["formats"] == ["adpcm", "alaw", "pcm", "ulaw", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm"})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and "output.wav" in r.headers["content-disposition"]
        assert r.content == adpcm.encode(full, 24000) and chat.calls[-1][2]["adpcm"] is True and chat.calls[-1][2]["pcm16"] is True
        assert "sample_rate" not in chat.calls[-1][2] and "speed" not in chat.calls[-1][2] and "encoding" not in chat.calls[-1][2]
        y, rate = adpcm.parse_wav(r.content)
        assert rate == 24000 and len(y) == 600 and np.abs(y.astype(int) - full).max() < 64
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "sample_rate": 8000, "speed": 1.25, "loudness": -20})
        assert r.status_code == 200 and r.content == adpcm.encode(full, 8000)
        kw = chat.calls[-1][2]
        assert kw["sample_rate"] == 8000 and kw["speed"] == 1.25 and kw["adpcm"] is True and kw["loudness"] == -20.0
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text
        for enc in ("ulaw", "alaw", "adpcm", 7):
            r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "encoding": enc})
            assert r.status_code == 400 and "ncoding" in r.text, enc
        assert len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "wav"})                          # no adpcm: today's call
        assert r.status_code == 200 and r.content == server.pcm16_to_wav_bytes(full) and "adpcm" not in chat.calls[-1][2]
    with TestClient(server.create_app(chat, adpcm=True)) as c:                                                     # without g711 too
        assert c.get("/health").json()["formats"] == ["adpcm", "pcm", "wav"]
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "encoding": "ulaw"})
        assert r.status_code == 400 and "ncoding" in r.text
    chat, bat = _AdpcmChat(), _FileBatcher()
    with TestClient(server.create_app(chat, batcher=bat, batch_streams=True, adpcm=True, sample_rates=(8000,))) as c:
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "sample_rate": 8000})
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        assert r.content == adpcm.encode(np.arange(100, dtype=np.int16), 8000) and bat.calls[-1] == ("submit", "hello", {"sample_rate": 8000, "adpcm": True})
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "adpcm", "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text
        r = c.post("/v1/audio/speech", json={"input": "hello", "response_format": "pcm"})
        assert r.content == np.arange(100, dtype=np.int16).tobytes() and bat.calls[-1] == ("submit", "hello", {}) and not chat.calls


# ---- 8. the batcher on fake pools ------------------------------------------------------------------------------------------------------------
class _FileChat(_EncChat):
    """as _EncChat; a row with the adpcm flag comes back as the file of the fake's ramp at the row's rate"""

    def decode_to_pcm16(self, hids, ragged=False, **kw):
        out = super().decode_to_pcm16(hids, ragged, **{k: v for k, v in kw.items() if k not in ("adpcm", "flac")})
        self.group_calls[-1] = (len(hids), ragged, dict(kw))
        assert not (kw.get("adpcm") and kw.get("flac")), "a decode call hands out one kind of file"
        flags = kw.get("adpcm", [False] * len(hids))
        rates = kw.get("sample_rate", [24000] * len(hids))
        return [np.frombuffer(adpcm.encode(p, r), np.uint8) if f else p for p, f, r in zip(out, flags, rates)]


def test_batcher_argument_rules_and_one_decode_for_mixed_requests():
    lock = threading.Lock()
    chat = _FileChat()
    holder = {}
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: holder.setdefault("p", _GroupPool(4, lock)), streams=True, ragged_decode=True)
    try:
        assert "adpcm_encoded" not in b.occupancy()                                  # never asked for: the report of today
        with pytest.raises(TypeError):
            b.submit_stream("x", _Params(48), adpcm=True)                            # a stream has no such option
        with pytest.raises(ValueError, match="encoding"):
            b.submit("x", _Params(48), adpcm=True, encoding="ulaw")
        with pytest.raises(ValueError, match="flac"):
            b.submit("x", _Params(48), adpcm=True, flac=True)
        with pytest.raises(ValueError, match="sample rate"):
            b.submit("x", _Params(48), adpcm=True, sample_rate=-5)
        with pytest.raises(ValueError) as e:
            b.submit("x", _Params(48), encoding="adpcm")
        assert str(e.value) == "unknown encoding 'adpcm': None (16-bit PCM), \"ulaw\" or \"alaw\""
        with lock:       # admitted together, the same length: they finish at the same poll
            futs = [b.submit("A", _Params(40)), b.submit("B", _Params(40), adpcm=True), b.submit("C", _Params(40), encoding="alaw")]
        res = [f.result(timeout=30) for f in futs]
        pcm = (np.arange(40) * 100).astype(np.int16)
        assert np.array_equal(res[0], pcm) and res[0].dtype == np.int16 and res[2].dtype == np.uint8 and len(res[2]) == 40
        assert res[1].dtype == np.uint8 and res[1].tobytes() == adpcm.encode(pcm, 24000)
        assert chat.group_calls == [(3, True, {"encoding": [None, None, "alaw"], "adpcm": [False, True, False]})]      # ONE decode call
        occ = b.occupancy()
        assert occ["decode_calls"] == 1 and occ["adpcm_encoded"] == 1 and occ["companded"] == 1 and occ["flac_encoded"] == 0
        assert np.array_equal(b.submit("D", _Params(16)).result(timeout=30), (np.arange(16) * 100).astype(np.int16))
        assert chat.group_calls[-1] == (1, True, {})                                            # no flag: today's call, no keyword
        assert b.occupancy()["adpcm_encoded"] == 1
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
        file = b.submit("B", _Params(16), adpcm=True, sample_rate=8000).result(timeout=30)
        assert plain.dtype == np.int16 and file.dtype == np.uint8 and chat.wav_calls == [{}, {"sample_rate": 8000}]
        assert file.tobytes() == adpcm.encode(plain, 8000)
    finally:
        b.close()
    assert not lock.locked()

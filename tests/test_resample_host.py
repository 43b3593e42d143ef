"""Host side of the device resampler: the float64 oracle against closed forms, the output length, `load_wav`, the refusals that must
reach no launch, the endpoint's `sample_rate` / voice upload on a fake chat, and the batcher's one-decode-per-poll at mixed rates."""
import ctypes as C
import io
import logging
import struct
import threading
import wave

import numpy as np
import pytest
import torch

from chattts_amd import _lib, resample as RS
from chattts_amd.audio import load_wav, pcm_to_wav_bytes
from chattts_amd.engine import CodecEngine
from chattts_amd.serving import SpeechBatcher
from tests.resample_oracle import PAIRS, oracle_taps, reduced, resample_f64
from tests.test_split_pool_host import _Catch, _EndpointChat, _FakeBatcher, _FakeChat, _Params, _Pool, _wait_idle

# properties of the stated filter, measured once from the oracle (0.4 s of input; the first and last 2 width input samples' worth of
# output left out): |y - 1| for a constant 1, |y - sin| for a 1 kHz sine.  The tests assert twice these.
CONST_DEV = {(24000, 8000): 4.66e-4, (24000, 16000): 5.10e-4, (24000, 48000): 8.76e-4, (24000, 44100): 8.76e-4, (44100, 24000): 4.81e-4,
             (16000, 24000): 6.80e-4, (48000, 24000): 4.57e-4}
SINE_DEV = {(24000, 8000): 1.36e-4, (24000, 16000): 3.96e-4, (24000, 48000): 4.66e-5, (24000, 44100): 1.01e-4, (44100, 24000): 3.62e-5,
            (16000, 24000): 5.53e-4, (48000, 24000): 3.42e-5}
TONE_RMS_OUT = 2.55e-5      # a unit sine at 0.9 x 12 kHz through 24k -> 8k: RMS of the interior (in: 0.7071); asserted at twice this


def _interior(orig, new):
    """output samples that the zero padding at the signal's ends reaches"""
    M, L = reduced(orig, new)
    _, width = oracle_taps(orig, new)
    return int(np.ceil(2 * width / M * L)) + 2


# ---- the oracle against closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_oracle_constant_stays_constant(orig, new):
    e = _interior(orig, new)
    y = resample_f64(np.ones(4 * orig // 10), orig, new)[e:-e]
    dev = float(np.abs(y - 1).max())
    print(f"{orig}->{new}: constant deviates by {dev:.3e}")
    assert dev <= 2 * CONST_DEV[(orig, new)]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_oracle_1khz_sine_is_the_sine_at_the_new_rate(orig, new):
    e = _interior(orig, new)
    y = resample_f64(np.sin(2 * np.pi * 1000 * np.arange(4 * orig // 10) / orig), orig, new)
    dev = float(np.abs(y - np.sin(2 * np.pi * 1000 * np.arange(len(y)) / new))[e:-e].max())
    print(f"{orig}->{new}: 1 kHz sine deviates by {dev:.3e}")
    assert dev <= 2 * SINE_DEV[(orig, new)]


def test_oracle_attenuates_a_tone_above_the_new_nyquist():
    y = resample_f64(np.sin(2 * np.pi * 0.9 * 12000 * np.arange(9600) / 24000), 24000, 8000)[60:-60]
    rms = float(np.sqrt(np.mean(y ** 2)))
    print(f"10.8 kHz through 24k->8k: rms {rms:.3e} (in {np.sqrt(0.5):.4f})")
    assert rms <= 2 * TONE_RMS_OUT


@pytest.mark.parametrize("orig,new", PAIRS)
def test_module_taps_equal_the_oracles(orig, new):
    h, width = oracle_taps(orig, new)
    L, M = RS.ratio(orig, new)
    assert (M, L) == reduced(orig, new) and RS.geometry(L, M) == (width, h.shape[1])
    t = RS.taps(orig, new)
    assert t.shape == h.shape and t.dtype == np.float64 and np.abs(t - h).max() <= 4 * np.finfo(np.float64).eps


def test_table_sizes_of_the_stated_pairs():
    assert [RS.geometry(*RS.ratio(o, n))[1] for o, n in ((24000, 8000), (24000, 44100), (44100, 24000))] == [41, 94, 171]
    assert RS.ratio(24000, 44100) == (147, 80) and RS.ratio(44100, 24000) == (80, 147)


@pytest.mark.parametrize("orig,new", PAIRS)
def test_output_length(orig, new):
    L, M = RS.ratio(orig, new)
    for n in range(1, 51):
        want = -(-n * L // M)
        assert RS.out_len(n, L, M) == want == len(resample_f64(np.ones(n), orig, new))
        assert RS.plan(orig, new, [0, n])[3].tolist() == [0, want]


# ---- load_wav ----------------------------------------------------------------------------------------------------------------------
def _wav_bytes(frames: np.ndarray, width: int, rate: int) -> bytes:
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(frames.shape[1])
        wf.setsampwidth(width)
        wf.setframerate(rate)
        wf.writeframes(frames.astype({1: np.uint8, 2: "<i2", 4: "<i4"}[width]).tobytes())
    return buf.getvalue()


@pytest.mark.parametrize("width", [1, 2, 4])
def test_load_wav_integer_pcm(width):
    x = np.array([[0.0], [0.5], [-0.5], [0.25], [-1.0]])
    full = float(1 << (8 * width - 1))
    ints = x * full + (128 if width == 1 else 0)
    wav, rate = load_wav(_wav_bytes(ints, width, 16000))
    assert rate == 16000 and wav.dtype == np.float32 and wav.shape == (5,)
    assert np.array_equal(wav, x[:, 0].astype(np.float32))


def test_load_wav_averages_channels():
    st = np.array([[16384, -16384], [8192, 24576], [-32768, 0]])
    wav, rate = load_wav(_wav_bytes(st, 2, 44100))
    assert rate == 44100 and np.array_equal(wav, np.array([0.0, 0.5, -0.5], np.float32))
    assert np.array_equal(load_wav(pcm_to_wav_bytes(np.array([0.5, -0.25], np.float32), 8000))[0] > 0, [True, False])


def _riff(fmt_tag: int, bits: int, payload: bytes) -> bytes:
    fmt = struct.pack("<HHIIHH", fmt_tag, 1, 16000, 16000 * bits // 8, bits // 8, bits)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(payload)) + b"WAVEfmt " + struct.pack("<I", len(fmt)) + fmt + \
        b"data" + struct.pack("<I", len(payload)) + payload


@pytest.mark.parametrize("what,data,names", [
    ("float", _riff(3, 32, np.zeros(8, np.float32).tobytes()), "3"),
    ("mu-law", _riff(7, 8, bytes(16)), "7"),
    ("24-bit", _riff(1, 24, bytes(24)), "24"),
    ("garbage", b"ID3\x03 not a wave file at all", "RIFF"),
    ("empty", _riff(1, 16, b""), "no samples"),
])
def test_load_wav_refuses_what_it_cannot_read(what, data, names):
    with pytest.raises(ValueError, match=names):
        load_wav(data)


# ---- refusals, before any launch ---------------------------------------------------------------------------------------------------
def test_plan_refusals():
    with pytest.raises(ValueError, match="equal"):
        RS.plan(24000, 24000, [0, 10])
    with pytest.raises(ValueError, match="equal"):
        RS.plan(48000, 48000, [0, 10])
    with pytest.raises(ValueError, match="beyond what the kernel supports"):
        RS.plan(24000, 24001, [0, 10])             # 24001/24000: a table of 24001 x 24014 floats
    with pytest.raises(ValueError, match="beyond what the kernel supports"):
        RS.plan(48000, 1000, [0, 10])              # 1/48: one tile would read 2048 x 48 input samples
    with pytest.raises(ValueError, match="empty"):
        RS.plan(24000, 8000, [0, 5, 5, 9])
    with pytest.raises(ValueError, match="ascend"):
        RS.plan(24000, 8000, [0, 9, 5])
    with pytest.raises(ValueError, match="start at 0"):
        RS.plan(24000, 8000, [3, 9])
    with pytest.raises(ValueError, match="2\\^31"):
        RS.plan(24000, 48000, [0, 1 << 30])
    assert int(RS.plan(24000, 48000, [0, (1 << 30) - 1])[3][-1]) == (1 << 31) - 2


def test_python_and_library_agree_on_what_is_supported():
    lib = _lib.lib()
    pairs = PAIRS + [(22050, 24000), (11025, 24000), (8000, 24000), (32000, 24000), (24000, 24001), (48000, 1000), (48000, 8000), (8000, 44100)]
    for orig, new in pairs:
        L, M = RS.ratio(orig, new)
        K = RS.geometry(L, M)[1]
        assert lib.ctts_resample_supported(L, M, K) == RS.mode(L, M, K), (orig, new)
    assert RS.mode(*RS.ratio(24000, 44100), 94) == 2 and RS.mode(*RS.ratio(44100, 24000), 171) == 1      # both table paths are in use
    assert lib.ctts_resample_supported(1, 1, 15) == 0 and lib.ctts_resample_supported(2, 1, 14) == 0


def test_library_refuses_before_it_launches():
    """the C entry point checks the host tables first: these calls fail on a machine without a GPU, with the reason, not with a HIP error"""
    lib = _lib.lib()
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused on its host arguments

    def call(off_in, off_out, L, M, K, sel=None):
        oi, oo = i64(off_in), i64(off_out)
        s = None if sel is None else np.asarray(sel, dtype=np.int32)
        rc = lib.ctts_resample_ragged(fake, fake, oi.ctypes.data_as(C.c_void_p), fake, fake, oo.ctypes.data_as(C.c_void_p), len(oi) - 1,
                                      None if s is None else fake, None if s is None else s.ctypes.data_as(C.c_void_p),
                                      0 if s is None else len(s), fake, L, M, K, None)
        return rc, lib.ctts_last_error().decode()

    for args, why in [(([0, 9], [0, 9], 1, 1, 15), "L != M"), (([0, 9], [0, 1], 1, 48, 680), "not supported"),
                      (([0, 9, 9], [0, 3, 6], 1, 3, 41), "empty"), (([0, 9, 5], [0, 3, 6], 1, 3, 41), "ascend"),
                      (([0, 9], [0, 4], 1, 3, 41), "ceil"), (([0, 1 << 30], [0, 1 << 31], 2, 1, 15), "2^31"),
                      (([0, 9], [0, 3], 1, 3, 41, [1]), "outside the pack")]:
        rc, msg = call(*args)
        assert rc != 0 and why in msg, (args, msg)


# ---- the endpoint on a fake chat ---------------------------------------------------------------------------------------------------
class _VoiceChat(_EndpointChat):
    def __init__(self, tokens=30):
        super().__init__()
        self.tokens, self.clips = tokens, []

    def sample_audio_speaker(self, wav, sample_rate=None):
        from chattts_amd.frontend import Speaker
        self.clips.append((np.asarray(wav).copy(), sample_rate))
        return Speaker.encode_prompt(torch.arange(4 * self.tokens, dtype=torch.int32).view(4, self.tokens) % 600)


def _app(chat=None, batcher=None, **kw):
    from chattts_amd import server
    log, catch = logging.getLogger(f"test_resample_host.{id(kw)}"), _Catch()
    log.addHandler(catch)
    chat = chat or _VoiceChat()
    return server.create_app(chat, {"default": "SPK-D"}, batcher=batcher, logger=log, **kw), chat, catch


def _header_rate(body: bytes) -> int:
    with wave.open(io.BytesIO(body), "rb") as wf:
        return wf.getframerate()


def test_endpoint_sample_rate():
    from starlette.testclient import TestClient
    body = {"input": "hello", "response_format": "wav"}
    app, chat, catch = _app(sample_rates=(8000, 16000, 24000, 44100, 48000))
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200 and _header_rate(r.content) == 8000 and chat.calls[-1][2]["sample_rate"] == 8000
        r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and _header_rate(r.content) == 24000 and "sample_rate" not in chat.calls[-1][2]
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 24000})
        assert r.status_code == 200 and _header_rate(r.content) == 24000 and "sample_rate" not in chat.calls[-1][2]
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 11025})
        assert r.status_code == 400 and "11025" in r.text and "44100" in r.text and len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000, "stream": True})
        assert r.status_code == 400 and "non-streamed" in r.text and "state" in r.text and len(chat.calls) == n
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 24000, "stream": True})
        assert r.status_code == 200 and chat.calls[-1][1] is True
        assert not catch.msgs

    bat = _FakeBatcher()
    app, chat, catch = _app(batcher=bat, sample_rates=(8000, 24000))
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200 and _header_rate(r.content) == 8000 and bat.calls[-1][2] == {"sample_rate": 8000}
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1][2] == {}

    app, chat, catch = _app()                      # off: the key is unknown, the response is today's
    with TestClient(app) as c:
        r = c.post("/v1/audio/speech", json={**body, "sample_rate": 8000})
        assert r.status_code == 200 and _header_rate(r.content) == 24000 and "sample_rate" not in chat.calls[-1][2]
        assert any("unsupported parameters" in m and "sample_rate" in m for m in catch.msgs), catch.msgs


def test_endpoint_voice_upload_then_speech():
    from starlette.testclient import TestClient
    clip = pcm_to_wav_bytes(0.5 * np.sin(np.arange(16000) / 9).astype(np.float32), 16000)
    app, chat, _ = _app(voice_upload=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/voices", params={"name": "anna", "text": "what the clip says"}, content=clip)
        assert r.status_code == 200, r.text
        assert r.json() == {"name": "anna", "seconds": 1.0, "sample_rate": 16000, "tokens": 30}
        assert chat.clips[-1][1] == 16000 and chat.clips[-1][0].shape == (16000,)
        assert c.post("/v1/audio/speech", json={"input": "hi", "voice": "anna", "response_format": "pcm"}).status_code == 200
        p = chat.calls[-1][2]["params_infer_code"]
        assert p.spk_smp == chat.sample_audio_speaker(np.zeros(1)) and p.txt_smp == "what the clip says" and p.spk_emb is None
        assert c.post("/v1/audio/voices", params={"name": "default"}, content=clip).status_code == 400
        r = c.post("/v1/audio/voices", params={"name": "x"}, content=b"RIFFnope")
        assert r.status_code == 400 and "bad WAV" in r.text
        chat.tokens = 0
        r = c.post("/v1/audio/voices", params={"name": "short"}, content=clip)
        assert r.status_code == 400 and "too short" in r.text

    class _Bat(_FakeBatcher):
        pool = _Pool(2, threading.Lock(), cap=2048 + 1 + 2 * _Pool.POLL + 64 + 20)      # room for 20 prompt tokens of a voice

    app, chat, _ = _app(batcher=_Bat(), voice_upload=True)
    with TestClient(app) as c:
        r = c.post("/v1/audio/voices", params={"name": "long"}, content=clip)
        assert r.status_code == 400 and "30 audio tokens" in r.text and "20" in r.text
        chat.tokens = 20
        assert c.post("/v1/audio/voices", params={"name": "fits"}, content=clip).status_code == 200

    app, _, _ = _app()                              # without voice_upload the route does not exist
    with TestClient(app) as c:
        assert c.post("/v1/audio/voices", params={"name": "anna"}, content=clip).status_code == 404


# ---- the batcher: requests at two rates that finish at one poll ---------------------------------------------------------------------
class _Codec:
    """a CodecEngine without a device: `decode_ragged` hands out one sample per token at "24 kHz" and goes through the engine's own
    `resample_segments`; the launches are counted instead of made"""
    SAMPLE_RATE = CodecEngine.SAMPLE_RATE
    resample, resample_segments = CodecEngine.resample, CodecEngine.resample_segments

    def __init__(self):
        self.decodes, self.launches = [], []

    def decode_ragged(self, rows, return_mel=False, sample_rate=None):
        self.decodes.append(len(rows))
        lens = [48 * int(r.shape[0]) for r in rows]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        wav = torch.cat([torch.full((n,), float(r[0, 0])) for n, r in zip(lens, rows)])
        return self.resample_segments(wav, off, [int(r) for r in sample_rate])

    def _resample_launch(self, x, off, y, off_out, sel, orig, new):
        self.launches.append((new, list(sel)))
        for i in sel:
            y[int(off_out[i]): int(off_out[i + 1])] = x[int(off[i])]


class _RateChat(_FakeChat):
    def __init__(self):
        super().__init__()
        self.codec = _Codec()

    def decode_to_pcm16(self, hids, ragged=False, sample_rate=None):
        assert ragged
        wav, off = self.codec.decode_ragged(list(hids), sample_rate=sample_rate or [24000] * len(hids))
        return [wav[int(off[i]): int(off[i + 1])].numpy().astype(np.int16) for i in range(len(hids))]


def test_two_rates_at_one_poll_share_the_decode():
    lock, pools = threading.Lock(), {}
    chat = _RateChat()
    b = SpeechBatcher(chat, 4, lock, make_pool=lambda: pools.setdefault("code", _Pool(4, lock)), ragged_decode=True)
    try:
        with lock:                  # all four are in the pool before its first launch: they finish at the same poll
            futs = [b.submit(f"{c}#8", _Params(), sample_rate=r) for c, r in (("a", 8000), ("b", 16000), ("c", 8000), ("d", None))]
        res = [f.result(timeout=10) for f in futs]
        _wait_idle(pools)
    finally:
        b.close()
    assert chat.codec.decodes == [4], "the four requests were not decoded together"
    assert sorted(chat.codec.launches) == [(8000, [0, 2]), (16000, [1])], chat.codec.launches      # one launch per distinct rate
    assert [len(r) for r in res] == [128, 256, 128, 384] and [int(r[0]) for r in res] == [ord(c) for c in "abcd"]

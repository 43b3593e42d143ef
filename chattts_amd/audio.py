"""Host back end of the path: float32 waveform -> 16-bit PCM / WAV bytes, what the reference's
examples do with `Chat.infer`'s output (/root/reference/tools/audio/np.py:7-12, pcm.py:8-33; examples/cmd/run.py).
The device twin of `float_to_int16` is `CodecEngine.float_to_int16` (csrc/codec.hip pcm16_k, C ABI ctts_float_to_int16); this host
form serves the odd pieces (a stream's last chunk after its column filter, split_text concatenations) and the tests.
mp3 / ogg go through PyAV in the reference (tools/audio/av.py), which is not part of this engine."""
from __future__ import annotations

import math
import struct
import wave
from io import BytesIO

import numpy as np


def pcm_scale(peak: float) -> int:
    """np.py:9-10: am = 32767 * 32768 // (int(ceil(peak)) * 32768); 0 for a silent clip (the reference divides by zero there)"""
    c = int(math.ceil(float(peak))) * 32768
    return 32767 * 32768 // c if c else 0


def float_to_int16(audio: np.ndarray, product: str = "f64") -> np.ndarray:
    """np.py:7-11: scale by 32767 / ceil(max|x|) in integer arithmetic, truncate toward zero; ONE peak over the whole array, whatever its
    rank.  `product`: "f64" = the reference as it RUNS (the function is numba-jitted, and numba types float32[:] * int64 as float64: the
    product is exact before the truncation); "f32" = what plain NumPy >= 2 makes of the same source line (python int = weak scalar: the
    float32 product is rounded first).  The two differ by one count on roughly one sample in 10^4.  A silent clip returns zeros."""
    audio = np.asarray(audio)
    am = pcm_scale(np.abs(audio).max()) if audio.size else 0
    if am == 0:
        return np.zeros(audio.shape, dtype=np.int16)
    if product == "f32":
        return np.multiply(audio.astype(np.float32, copy=False), np.float32(am)).astype(np.int16)
    return np.multiply(audio.astype(np.float64), float(am)).astype(np.int16)


def pcm_to_wav_bytes(wav: np.ndarray, sample_rate: int = 24000) -> bytes:
    """pcm.py:8-33: mono, 16-bit little-endian RIFF/WAVE."""
    buf = BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(sample_rate)
        wf.writeframes(float_to_int16(np.asarray(wav, dtype=np.float32).reshape(-1)).astype("<i2").tobytes())
    return buf.getvalue()


WAVE_FORMAT_ALAW, WAVE_FORMAT_MULAW = 6, 7


def g711_wav_header(law, sample_rate: int, n_samples=None) -> bytes:
    """everything in front of the samples of a mono G.711 RIFF/WAVE file: format tag 7 (mu-law) / 6 (A-law), 8 bits, block align 1, an
    18-byte `fmt ` chunk with cbSize = 0, a `fact` chunk holding the sample count, the `data` chunk's header.  `n_samples` None: the
    open-ended form of a stream -- 0xFFFFFFFF in the RIFF, `fact` and `data` lengths, like `server.wav_stream_header`."""
    from .g711 import law_of
    tag = (WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW)[law_of(law)]
    if n_samples is None:
        riff = fact = data = 0xFFFFFFFF
    else:
        fact = data = int(n_samples)
        riff = 4 + (8 + 18) + (8 + 4) + 8 + data + (data & 1)
    return (b"RIFF" + struct.pack("<I", riff) + b"WAVEfmt " + struct.pack("<IHHIIHHH", 18, tag, 1, int(sample_rate), int(sample_rate), 1, 8, 0)
            + b"fact" + struct.pack("<II", 4, fact) + b"data" + struct.pack("<I", data))


def g711_to_wav_bytes(codes: np.ndarray, law, sample_rate: int = 8000) -> bytes:
    """G.711 codes (uint8, `g711.encode`'s or the device's) -> a mono WAVE_FORMAT_MULAW / WAVE_FORMAT_ALAW file; an odd-length `data` chunk
    is followed by one pad byte (RIFF chunks are word aligned)"""
    codes = np.ascontiguousarray(np.asarray(codes).reshape(-1))
    if codes.dtype != np.uint8:
        raise ValueError(f"g711_to_wav_bytes takes uint8 codes, got {codes.dtype}")
    return g711_wav_header(law, sample_rate, codes.size) + codes.tobytes() + (b"\0" if codes.size & 1 else b"")


def _load_g711_wav(data: bytes):
    """a WAVE_FORMAT_MULAW / WAVE_FORMAT_ALAW file parsed chunk by chunk (stdlib `wave` refuses the tags) -> (float32 mono, rate), or None
    when the bytes are no RIFF/WAVE with one of those two tags -- then `load_wav` goes on as without the option"""
    from .g711 import expand
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        return None
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data) and (fmt is None or body is None):
        cid, size = data[pos: pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if cid == b"fmt " and size >= 16 and pos + 8 + 16 <= len(data):
            fmt = struct.unpack_from("<HHIIHH", data, pos + 8)
        elif cid == b"data":
            body = data[pos + 8: pos + 8 + size]       # an open-ended stream's 0xFFFFFFFF: everything that follows
        pos += 8 + size + (size & 1)
    if fmt is None or fmt[0] not in (WAVE_FORMAT_ALAW, WAVE_FORMAT_MULAW):
        return None
    tag, ch, rate, _, _, bits = fmt
    if bits != 8:
        raise ValueError(f"a G.711 WAV file holds 8-bit samples, this one says {bits}")
    if ch < 1 or rate <= 0:
        raise ValueError(f"bad WAV header: {ch} channels at {rate} Hz")
    frames = len(body or b"") // ch
    if frames == 0:
        raise ValueError("the WAV file holds no samples")
    x = expand(np.frombuffer(body[: frames * ch], dtype=np.uint8), 0 if tag == WAVE_FORMAT_MULAW else 1).astype(np.float64) / 32768.0
    return x.reshape(frames, ch).mean(axis=1).astype(np.float32), int(rate)


def _load_adpcm_wav(data: bytes):
    """a mono WAVE_FORMAT_IMA_ADPCM file (`adpcm.parse_wav`) -> (float32 mono, rate), or None when the bytes are no RIFF/WAVE with that tag"""
    from .adpcm import parse_wav
    got = parse_wav(data)
    if got is None:
        return None
    return (got[0].astype(np.float64) / 32768.0).astype(np.float32), got[1]


def load_wav(data: bytes, *, g711: bool = False, adpcm: bool = False):
    """RIFF/WAVE bytes -> (float32 mono samples in [-1, 1), sample rate): the front door of voice cloning from an uploaded clip
    (`Chat.sample_audio_speaker(wav, rate)`, the endpoint's POST /v1/audio/voices).  Integer PCM of 8 (unsigned), 16 or 32 bits, any
    number of channels (averaged to mono), read with the stdlib `wave` module.  Anything else -- a float or compressed WAVE, 24-bit
    samples, no RIFF at all, no frames -- raises ValueError naming what was found.  `g711=True` (keyword-only; the default refuses them
    like any compressed file): mu-law and A-law files (format tags 7 / 6, 8 bits, any channel count, any rate) -- telephone recordings --
    are parsed from the RIFF chunks by hand and expanded through `g711.expand`'s tables to int16 / 32768.  `adpcm=True` (keyword-only;
    the default refuses them likewise): mono IMA ADPCM files (format tag 0x0011, 4 bits, any block size, any rate) are decoded through
    `adpcm.parse_wav` to int16 / 32768; another channel count, or a `fmt ` chunk that disagrees with its block size, raises ValueError."""
    if adpcm:
        got = _load_adpcm_wav(bytes(data))
        if got is not None:
            return got
    if g711:
        got = _load_g711_wav(bytes(data))
        if got is not None:
            return got
    try:
        with wave.open(BytesIO(bytes(data)), "rb") as wf:
            ch, width, rate, n = wf.getnchannels(), wf.getsampwidth(), wf.getframerate(), wf.getnframes()
            raw = wf.readframes(n)
    except (wave.Error, EOFError) as e:     # `wave` reads integer PCM only: "unknown format: 3" is a float file, 85 an mp3 in a RIFF
        raise ValueError(f"not an integer-PCM WAV file: {e or 'truncated or empty input'}") from None
    if width not in (1, 2, 4):
        raise ValueError(f"unsupported WAV sample width: {8 * width} bits (8-, 16- and 32-bit PCM are supported)")
    if ch < 1 or rate <= 0:
        raise ValueError(f"bad WAV header: {ch} channels at {rate} Hz")
    frames = len(raw) // (width * ch)
    if frames == 0:
        raise ValueError("the WAV file holds no samples")
    raw = raw[: frames * width * ch]
    if width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    else:
        x = np.frombuffer(raw, dtype="<i2" if width == 2 else "<i4").astype(np.float64) / float(1 << (8 * width - 1))
    return x.reshape(frames, ch).mean(axis=1).astype(np.float32), int(rate)

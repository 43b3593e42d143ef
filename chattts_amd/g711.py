"""G.711 companding on the host: the NumPy twin of csrc/g711.hip (ctts_g711_encode_ranges) and the expansion tables.

The map is the ITU-T G.191 one: a negative sample is companded from its ONES' complement, so the map is sign-symmetric
(`encode(~x) == encode(x) ^ 0x80`).  With `lin` an int16 in 32-bit arithmetic, `mag = ~lin if lin < 0 else lin`:

    mu-law: a = min((mag >> 2) + 33, 0x1FFF); seg = 1 + bits(a >> 6); code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)); | 0x80 if lin >= 0
    A-law:  ix = mag >> 4; if ix > 15: e = 1; while ix > 31: ix >>= 1, e += 1; ix = ix - 16 + (e << 4); | 0x80 if lin >= 0; ^ 0x55

The device converts whole results; this form serves the odd pieces that are converted on the host (a serial stream's last chunk after its
column filter, a split request concatenated on the host), `audio.load_wav(g711=True)` and the tests."""
from __future__ import annotations

import numpy as np

LAWS = {"ulaw": 0, "alaw": 1}


def law_of(law) -> int:
    """"ulaw" / "alaw" / 0 / 1 -> 0 (mu-law) or 1 (A-law); anything else raises ValueError"""
    if isinstance(law, str):
        if law in LAWS:
            return LAWS[law]
    elif law is not None and not isinstance(law, bool) and int(law) in (0, 1):
        return int(law)
    raise ValueError(f"unknown G.711 law {law!r}: \"ulaw\" (0) or \"alaw\" (1)")


def check_encoding(encoding):
    """the `encoding=` option of the output paths: None, "ulaw" or "alaw" -> the same; anything else raises ValueError"""
    if encoding is None or encoding in LAWS:
        return encoding
    raise ValueError(f"unknown encoding {encoding!r}: None (16-bit PCM), \"ulaw\" or \"alaw\"")


def _bits(v: np.ndarray) -> np.ndarray:
    """number of significant bits of the non-negative int32 values (< 2^13)"""
    n = np.zeros(v.shape, np.int32)
    for k in range(13):
        n += (v >> k) > 0
    return n


def encode(pcm, law) -> np.ndarray:
    """int16 samples -> G.711 codes (uint8, same shape)"""
    law = law_of(law)
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise ValueError(f"g711.encode takes int16 samples, got {pcm.dtype}")
    lin = pcm.astype(np.int32)
    mag = np.where(lin < 0, ~lin, lin)
    sign = np.where(lin >= 0, 0x80, 0).astype(np.int32)
    if law == 0:
        a = np.minimum((mag >> 2) + 33, 0x1FFF)
        seg = 1 + _bits(a >> 6)
        code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)) | sign
    else:
        ix = mag >> 4
        e = np.maximum(_bits(ix) - 4, 0)          # ix > 15: 1 + the halvings that bring it to <= 31
        sh = np.maximum(e - 1, 0)
        code = (np.where(e > 0, (ix >> sh) - 16 + (e << 4), ix) | sign) ^ 0x55
    return code.astype(np.uint8)


def _tables():
    c = np.arange(256, dtype=np.int32)
    m = ~c & 0xFF
    e = (m >> 4) & 7
    step = 4 << (e + 1)
    v = (0x80 << e) + step * (m & 0xF) + step // 2 - 132
    mu = np.where(c < 0x80, -v, v)
    i = (c ^ 0x55) & 0x7F
    e = i >> 4
    t = (i & 0xF) + np.where(e > 0, 16, 0)
    v = ((t << 4) + 8) << np.maximum(e - 1, 0)
    al = np.where(((c ^ 0x55) & 0x80) == 0, -v, v)
    return mu.astype(np.int16), al.astype(np.int16)


EXPAND = _tables()      # [law][code] -> int16


def expand(codes, law) -> np.ndarray:
    """G.711 codes (uint8) -> int16 samples (same shape), through the 256-entry tables"""
    law = law_of(law)
    codes = np.asarray(codes)
    if codes.dtype != np.uint8:
        raise ValueError(f"g711.expand takes uint8 codes, got {codes.dtype}")
    return EXPAND[law][codes]

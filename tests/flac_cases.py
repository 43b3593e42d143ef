"""The lengths and signals of the FLAC tests (host and GPU share them) and their references, each computed once per session: the twin's
encoding of a case and the independent decoder's reading of a file (keyed by the file's bytes, so a device result that equals the twin's
is decoded once)."""
import functools
import hashlib
import zlib

import numpy as np

from chattts_amd import flac
from tests import flac_oracle

LENGTHS = [0, 1, 2, 4, 5, 15, 16, 4095, 4096, 4097, 2 * 4096 + 17, 128 * 4096 + 1]        # the last: two-byte frame numbers
SIGNALS = ["silence", "dc_min", "dc_max", "alternating", "noise", "small_noise", "ramp", "chirp", "ar2", "spikes", "half_silence"]
RATES = [24000, 8000, 11025, 48000, 192000, 65535]


def signal(name: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(zlib.crc32(f"{name}/{n}".encode()))
    i = np.arange(n)
    if name == "silence":
        x = np.zeros(n)
    elif name == "dc_min":
        x = np.full(n, -32768)
    elif name == "dc_max":
        x = np.full(n, 32767)
    elif name == "alternating":
        x = np.where(i % 2, -32767, 32767)
    elif name == "noise":
        x = rng.integers(-32768, 32768, n)
    elif name == "small_noise":
        x = rng.integers(-3, 4, n)
    elif name == "ramp":
        x = (i * 7) % 65536 - 32768
    elif name == "chirp":
        x = np.round(30000 * np.sin(2 * np.pi * (50 * i / 24000 + 1500 * (i / 24000) ** 2)))
    elif name == "ar2":                                  # a resonance near 500 Hz at 24 kHz, driven by noise: "speech-like"
        e = rng.standard_normal(n) * 300
        x = np.zeros(n)
        for j in range(n):
            x[j] = e[j] + 1.9 * (x[j - 1] if j > 0 else 0) - 0.92 * (x[j - 2] if j > 1 else 0)
        x = np.clip(np.round(x), -32768, 32767)
    elif name == "spikes":                               # long unary runs that cross words
        x = np.zeros(n)
        at = rng.choice(n, size=min(n, max(1, n // 700)), replace=False) if n else []
        x[at] = rng.choice([-32767, 32767], size=len(at))
    elif name == "half_silence":                         # each block: silence, then noise of a few hundred counts
        x = rng.integers(-400, 401, n)
        x[(i % 4096) < 2048] = 0
    else:
        raise KeyError(name)
    return np.asarray(x).astype(np.int16)


def rate_of(name: str, n: int) -> int:
    return RATES[(SIGNALS.index(name) + LENGTHS.index(n)) % len(RATES)] if n in LENGTHS else 24000


@functools.lru_cache(maxsize=None)
def reference(name: str, n: int):
    """(samples, rate, the twin's frames, their lengths)"""
    x = signal(name, n)
    x.setflags(write=False)
    body, lens = flac.frames(x, rate_of(name, n))
    return x, rate_of(name, n), body, lens


_DECODED = {}


def decoded(file_bytes):
    """flac_oracle.decode(file, info=True), once per distinct file"""
    file_bytes = bytes(file_bytes)
    key = hashlib.sha1(file_bytes).digest()
    if key not in _DECODED:
        _DECODED[key] = flac_oracle.decode(file_bytes, info=True)
    return _DECODED[key]

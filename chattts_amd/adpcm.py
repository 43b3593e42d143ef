"""IMA/DVI ADPCM on the host: the NumPy twin of csrc/adpcm.hip (ctts_adpcm_encode_ranges), byte for byte, the decoder and the WAV
container (WAVE_FORMAT_IMA_ADPCM, tag 0x0011: 4 bits per sample, mono).

One sample, state (pred, idx), the sample v an int16 in 32-bit arithmetic:

    step = STEP[idx]; d = v - pred; sign = 8 if d < 0 else 0; d = |d|; code = 0; vp = step >> 3
    if d >= step:       code = 4;  d -= step;      vp += step
    if d >= step >> 1:  code |= 2; d -= step >> 1; vp += step >> 1
    if d >= step >> 2:  code |= 1;                 vp += step >> 2
    pred = clamp(pred -+ vp, -32768, 32767); code |= sign; idx = clamp(idx + IDX[code], 0, 88)

The decoder makes the same vp from the code alone, so the encoder's pred is the decoder's output.  It is CPython's `audioop`
(`lin2adpcm` / `adpcm2lin`) step for step; tests/test_adpcm_host.py pins the tables and the codes against it.

Blocks: `align(rate)` = 256 * max(1, rate // 11025) bytes hold S = 2 * (align - 4) + 1 samples (505 / 1017 / 2041).  A signal of n >= 1
samples is ceil(n / S) full blocks; positions at or beyond n read as x[n - 1].  Block b: bytes 0-1 x[bS] (little-endian int16, the start
predictor), byte 2 index0, byte 3 zero, byte 4 + j the code of sample 1 + 2j in bits 0-3 and that of sample 2 + 2j in bits 4-7.
index0 = min{i : STEP[i] >= |x[bS + 1] - x[bS]|}, 88 when there is none: a block's bytes depend on its own samples and the rate only,
which is what makes every block of every signal independent work on the device.  A decoder takes the state from the header, so the
choice is a legal one; it is the one place where this encoder differs from a chain carried through the whole signal.

The device encodes whole results; this form serves the odd pieces that are converted on the host (SpeechBatcher.finish, a split request
concatenated on the host), `audio.load_wav(adpcm=True)` and the tests.

Streams (`stream_plan`, `StreamEncoder`; on the device `CodecEngine.adpcm_stream_step`, csrc/adpcm.hip adpcm_stage_k): because a block's
bytes depend on its own S samples and the rate only, a stream cut anywhere emits the bytes of the one-shot encoder as long as only whole
blocks leave and the rest waits.  A stream holds `carry` samples (0 .. S - 1) of its earlier pushes; a push of n samples makes
avail = carry + n.  Not final: avail // S blocks leave, from the front, and avail % S samples are held.  Final: ceil(avail / S) blocks
leave, the last one padded as the one-shot encoder pads (positions beyond the end read as the last sample), and none are held; a final
push with avail = 0 emits nothing.  The pushes of a stream, concatenated, are `encode_blocks` of its samples, however they were cut.  A
stream's blocks are at most S - 1 samples behind its PCM: 63 ms at 8 kHz, 31.5 ms at 16 kHz, 42.3 ms at 24 kHz, 42.5 ms at 48 kHz.
`stream_header` is the header of a file whose length is not known yet (0xFFFFFFFF in the RIFF, `fact` and `data` lengths); `parse_wav`
reads such a file as every whole block that follows.  The consequence: a receiver of an open-ended stream cannot know the true length --
behind the last real sample it decodes up to S - 1 padded samples, which hold the last value (as closely as the coder follows it)."""
from __future__ import annotations

import struct

import numpy as np

WAVE_FORMAT_IMA_ADPCM = 0x0011
HEADER_BYTES = 60          # RIFF/WAVE, a 20-byte `fmt `, `fact`, the `data` chunk's header
IDX = (-1, -1, -1, -1, 2, 4, 6, 8) * 2
STEP = (7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
        157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552,
        1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487,
        12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767)
_STEP = np.asarray(STEP, np.int64)
_IDX = np.asarray(IDX, np.int64)


def check_rate(rate) -> int:
    """the rate as the `fmt ` chunk holds it: an integer number of Hz in 1 .. 2^31 - 1; anything else raises ValueError"""
    if isinstance(rate, (bool, np.bool_)) or not isinstance(rate, (int, np.integer)) or not 1 <= int(rate) < 1 << 31:
        raise ValueError(f"adpcm: the sample rate is an integer number of Hz in 1 .. 2^31 - 1, got {rate!r}")
    return int(rate)


def align(rate) -> int:
    """bytes per block: 256 up to 22049 Hz, 512 up to 33074 Hz, 1024 at 44100 and 48000 Hz"""
    return 256 * max(1, check_rate(rate) // 11025)


def samples_per_block(rate) -> int:
    return 2 * (align(rate) - 4) + 1


def n_blocks(n, rate) -> int:
    """the blocks of a signal of n samples (0 for none)"""
    S = samples_per_block(rate)
    return (max(int(n), 0) + S - 1) // S


def index0(d) -> int:
    """a block's start index from the magnitude of its first difference: the least i with STEP[i] >= d, 88 when there is none"""
    return int(min(np.searchsorted(_STEP, abs(int(d)), side="left"), 88))


def _pcm(pcm) -> np.ndarray:
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError(f"adpcm takes a 1-D int16 array, got {pcm.dtype} {pcm.shape}")
    return pcm


def _vp(step: np.ndarray, code: np.ndarray) -> np.ndarray:
    return (step >> 3) + np.where(code & 4, step, 0) + np.where(code & 2, step >> 1, 0) + np.where(code & 1, step >> 2, 0)


def encode_blocks(pcm, rate, trace: bool = False):
    """int16 samples (n >= 1) -> the blocks back to back, a uint8 array of n_blocks * align bytes: what ctts_adpcm_encode_ranges writes
    for one range.  `trace`: (blocks, the predictor behind every sample, int16 [n_blocks * S]) -- what a decoder makes of the blocks."""
    x = _pcm(pcm)
    A, S = align(rate), samples_per_block(rate)
    n = len(x)
    if n < 1:
        raise ValueError("adpcm: a signal of no samples has no blocks")
    nb = (n + S - 1) // S
    X = np.full(nb * S, int(x[-1]), np.int64)
    X[:n] = x
    X = X.reshape(nb, S)
    pred = X[:, 0].copy()
    idx = np.minimum(np.searchsorted(_STEP, np.abs(X[:, 1] - pred), side="left"), 88).astype(np.int64)
    out = np.zeros((nb, A), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = pred & 0xFF, (pred >> 8) & 0xFF, idx
    codes = np.zeros((nb, S - 1), np.uint8)
    preds = np.zeros((nb, S), np.int64)
    preds[:, 0] = pred
    for s in range(1, S):
        step = _STEP[idx]
        d = X[:, s] - pred
        sign = np.where(d < 0, 8, 0)
        d = np.abs(d)
        c4 = d >= step
        d = d - np.where(c4, step, 0)
        c2 = d >= (step >> 1)
        d = d - np.where(c2, step >> 1, 0)
        c1 = d >= (step >> 2)
        code = c4 * 4 + c2 * 2 + c1 * 1
        vp = _vp(step, code)
        pred = np.clip(np.where(sign, pred - vp, pred + vp), -32768, 32767)
        code = code | sign
        idx = np.clip(idx + _IDX[code], 0, 88)
        codes[:, s - 1] = code
        preds[:, s] = pred
    out[:, 4:] = codes[:, 0::2] | (codes[:, 1::2] << 4)
    out = out.reshape(-1)
    return (out, preds.reshape(-1).astype(np.int16)) if trace else out


def _decode(B: np.ndarray) -> np.ndarray:
    """blocks [nb, A] (int64 bytes, step indices within 0 .. 88) -> their samples [nb, 2 * (A - 4) + 1] (int64)"""
    nb, S = B.shape[0], 2 * (B.shape[1] - 4) + 1
    pred = B[:, 0] | (B[:, 1] << 8)
    pred = np.where(pred >= 32768, pred - 65536, pred)
    idx = np.minimum(B[:, 2], 88)
    codes = np.zeros((nb, S - 1), np.int64)
    codes[:, 0::2], codes[:, 1::2] = B[:, 4:] & 15, B[:, 4:] >> 4
    out = np.zeros((nb, S), np.int64)
    out[:, 0] = pred
    for s in range(1, S):
        code = codes[:, s - 1]
        vp = _vp(_STEP[idx], code)
        pred = np.clip(np.where(code & 8, pred - vp, pred + vp), -32768, 32767)
        idx = np.clip(idx + _IDX[code], 0, 88)
        out[:, s] = pred
    return out


def decode_blocks(data, n, rate) -> np.ndarray:
    """blocks (bytes or uint8, whole blocks of align(rate) bytes) -> the first n int16 samples they hold"""
    A, S = align(rate), samples_per_block(rate)
    b = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data)
    if b.dtype != np.uint8 or b.ndim != 1 or b.size % A:
        raise ValueError(f"adpcm: blocks at {rate} Hz are whole multiples of {A} bytes of uint8")
    nb = b.size // A
    n = int(n)
    if not 0 <= n <= nb * S:
        raise ValueError(f"adpcm: {nb} blocks hold up to {nb * S} samples, not {n}")
    B = b.reshape(nb, A).astype(np.int64)
    if nb and int(B[:, 2].max()) > 88:
        raise ValueError("adpcm: a block header's step index is beyond 88")
    return _decode(B).reshape(-1)[:n].astype(np.int16)


def wav_header(n, rate, bare: bool = False) -> bytes:
    """the 60 bytes in front of the blocks of a file of n >= 1 samples (`bare`: n = 0 too, `behind_decode`'s empty result)"""
    rate, n = check_rate(rate), int(n)
    A, S = align(rate), samples_per_block(rate)
    data = n_blocks(n, rate) * A
    if n < (0 if bare else 1) or n >= 1 << 32 or HEADER_BYTES - 8 + data >= 1 << 32:
        raise ValueError(f"adpcm: a file holds 1 .. 2^32 - 1 samples in under 4 GiB, got {n}")
    return (b"RIFF" + struct.pack("<I", HEADER_BYTES - 8 + data) + b"WAVEfmt "
            + struct.pack("<IHHIIHHHH", 20, WAVE_FORMAT_IMA_ADPCM, 1, rate, rate * A // S, A, 4, 2, S)
            + b"fact" + struct.pack("<II", 4, n) + b"data" + struct.pack("<I", data))


def stream_header(rate) -> bytes:
    """the 60 bytes in front of a stream's blocks: `wav_header` with 0xFFFFFFFF in the RIFF, `fact` and `data` lengths (the convention of
    the server's streamed PCM and G.711 headers).  `parse_wav` reads every whole block that follows: up to S - 1 samples more than the
    stream held, all of them coding the last value."""
    h = bytearray(wav_header(1, rate))
    for at in (4, 48, 56):
        h[at: at + 4] = b"\xFF\xFF\xFF\xFF"
    return bytes(h)


def stream_plan(carry, n, final, rate):
    """the cutting rule: a stream at `rate` that holds `carry` samples gets n more -> (blocks emitted, samples held afterwards)"""
    S = samples_per_block(rate)
    carry, n = int(carry), int(n)
    if not 0 <= carry < S or n < 0:
        raise ValueError(f"adpcm: a stream at {rate} Hz carries 0 .. {S - 1} samples and a push has 0 or more (got {carry}, {n})")
    avail = carry + n
    return ((avail + S - 1) // S, 0) if final else (avail // S, avail % S)


def stream_bound(n, rate) -> int:
    """the most bytes a push of n samples can emit: a final push onto a carry of S - 1"""
    S = samples_per_block(rate)
    return (S - 1 + max(int(n), 0) + S - 1) // S * align(rate)


class StreamEncoder:
    """The NumPy twin of `CodecEngine.adpcm_stream_step` for one stream: `push(x, final)` -> the blocks that push completes (a uint8
    array, possibly empty).  The concatenated pushes are `encode_blocks` of the concatenated samples."""

    def __init__(self, rate):
        self.rate = check_rate(rate)
        self.S = samples_per_block(rate)
        self.held = np.zeros((0,), np.int16)
        self.done = False

    def push(self, x, final: bool = False) -> np.ndarray:
        x = _pcm(x)
        if self.done:
            raise ValueError("adpcm: the stream has had its last push")
        blocks, held = stream_plan(len(self.held), len(x), final, self.rate)
        buf = np.concatenate([self.held, x])
        self.held = buf[len(buf) - held:].copy() if held else np.zeros((0,), np.int16)
        self.done = bool(final)
        if not blocks:
            return np.zeros((0,), np.uint8)
        return encode_blocks(buf[: len(buf) - held], self.rate)


def wav_bytes(blocks, n, rate) -> np.ndarray:
    """the complete file around blocks that are already encoded (the device's): a uint8 array"""
    blocks = np.asarray(blocks)
    if blocks.dtype != np.uint8 or blocks.ndim != 1 or blocks.size != n_blocks(n, rate) * align(rate):
        raise ValueError(f"adpcm: {int(n)} samples at {rate} Hz are {n_blocks(n, rate)} blocks of {align(rate)} bytes, got {blocks.size} bytes")
    return np.concatenate([np.frombuffer(wav_header(n, rate), np.uint8), blocks])


def behind_decode(blocks, n, rate) -> np.ndarray:
    """`wav_bytes` behind a decode, where a result can be empty (silence stripped to nothing): then the bare 60-byte header -- `fact` 0, a
    `data` chunk of no bytes -- as the FLAC path hands out a bare `fLaC` header there.  Called directly, `wav_bytes` and `encode` refuse
    n = 0."""
    if int(n) > 0:
        return wav_bytes(blocks, n, rate)
    return np.frombuffer(wav_header(0, rate, bare=True), np.uint8)


def encode_result(pcm, rate) -> np.ndarray:
    """a result converted on the host -> its file as a uint8 array: `encode`, or `behind_decode`'s bare header for no samples"""
    x = _pcm(pcm)
    return np.frombuffer(encode(x, rate), np.uint8) if len(x) else behind_decode(None, 0, rate)


def encode(pcm, rate) -> bytes:
    """int16 samples (n >= 1) -> the whole WAV file"""
    x = _pcm(pcm)
    if len(x) < 1:
        raise ValueError("adpcm: a file of no samples is refused (n >= 1)")
    return wav_header(len(x), rate) + encode_blocks(x, rate).tobytes()


def parse_wav(data):
    """a mono WAVE_FORMAT_IMA_ADPCM file -> (int16 samples, rate), or None when the bytes are no RIFF/WAVE with that tag.  Another channel
    count, a `fmt ` chunk that disagrees with its block size (4 bits, samples per block 2 * (align - 4) + 1), no whole block, a `fact`
    count beyond the blocks: ValueError -- but a `fact` of 0xFFFFFFFF (`stream_header`: an open-ended file) is read as every whole block
    that follows, the `data` chunk's 0xFFFFFFFF being cut to the bytes that are there.  Any block size of 5 bytes or more is read (files of other encoders), not only `align(rate)`."""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        return None
    pos, fmt, body, fact = 12, None, None, None
    while pos + 8 <= len(data) and (fmt is None or body is None):
        cid, size = data[pos: pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if cid == b"fmt " and size >= 16 and pos + 8 + 16 <= len(data):
            fmt = struct.unpack_from("<HHIIHH", data, pos + 8)
            extra = struct.unpack_from("<HH", data, pos + 24) if size >= 20 and pos + 28 <= len(data) else None
        elif cid == b"fact" and size >= 4 and pos + 12 <= len(data):
            fact = struct.unpack_from("<I", data, pos + 8)[0]
        elif cid == b"data":
            body = data[pos + 8: pos + 8 + size]
        pos += 8 + size + (size & 1)
    if fmt is None or fmt[0] != WAVE_FORMAT_IMA_ADPCM:
        return None
    _, ch, rate, _, A, bits = fmt
    if ch != 1:
        raise ValueError(f"an IMA ADPCM WAV file is read as mono, this one has {ch} channels")
    if rate <= 0 or rate >= 1 << 31:
        raise ValueError(f"bad WAV header: {rate} Hz")
    if bits != 4 or A < 5 or extra is None or extra[0] < 2 or extra[1] != 2 * (A - 4) + 1:
        raise ValueError(f"the `fmt ` chunk of this IMA ADPCM file disagrees with its block size of {A} bytes "
                         f"(4 bits and {2 * (A - 4) + 1} samples per block are expected)")
    S = extra[1]
    nb = len(body or b"") // A
    n = nb * S if fact is None or fact == 0xFFFFFFFF else int(fact)
    if nb == 0 or n == 0:
        raise ValueError("the WAV file holds no samples")
    if n > nb * S:
        raise ValueError(f"the `fact` chunk counts {n} samples, the {nb} blocks hold {nb * S}")
    B = np.frombuffer(body[: nb * A], np.uint8).reshape(nb, A).astype(np.int64)
    B[:, 2] = np.minimum(B[:, 2], 88)
    return _decode(B).reshape(-1)[:n].astype(np.int16), int(rate)

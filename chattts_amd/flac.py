"""FLAC on the host: the NumPy twin of csrc/flac.hip (ctts_flac_encode_ranges), byte for byte, and the file container.

The subset is fixed so that two integer-only encoders cannot differ: mono, 16 bits per sample, fixed block size 4096 (frames start
FF F8; the last block may be shorter and then carries its length - 1 in 16 bits), the sample rate by its table code or in Hz (16 bits).
A block is CONSTANT when all its samples are equal, else FIXED of order o in 0 .. min(4, n - 1) with Rice partition order p in
0 .. min(6, ctz(n)), (n >> p) > o, and 4-bit parameters k in 0 .. 14 (no escape), when that is STRICTLY smaller than VERBATIM.  The choice
is an exact search over every (o, p, k per partition): the smallest subframe in bits, ties to the lowest o, then the lowest p, then the
lowest k.  So a frame never exceeds its VERBATIM size, 16 + 2 n bytes, which gives `bound`.  The sums here are exact (int64); the kernel's
are 64-bit too.  The file is `fLaC`, one STREAMINFO block (MD5 all zero: "not computed", the samples never reach the host) and the frames.

The device encodes whole results; this form serves the odd pieces that are converted on the host (SpeechBatcher.finish, a split request
concatenated on the host) and the tests.

Streams (the second half of this file; ctts_flac_stream_step) arrive in pushes and leave as variable-block-size frames (FF F9) that carry
the number of their first sample: `stream_header`, `frame_header_variable`, `stream_plan` (the cutting rule), `stream_bound`,
`StreamEncoder`."""
from __future__ import annotations

import numpy as np

BLOCK = 4096
MAX_ORDER = 4
MAX_PART_ORDER = 6
MAX_RICE = 14
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
HEADER_BYTES = 42          # "fLaC" + the metadata block header + STREAMINFO


def crc8(data) -> int:
    """CRC-8, polynomial 0x07, initial value 0 (the frame header's)"""
    c = 0
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _crc16_table():
    t = np.zeros(256, np.uint16)
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        t[i] = c
    return [int(v) for v in t]


_CRC16 = _crc16_table()


def crc16(data) -> int:
    """CRC-16, polynomial 0x8005, initial value 0, not reflected (the frame footer's)"""
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def rate_code(rate) -> int:
    """the frame header's 4-bit sample-rate code: the table's, else 0b1101 (Hz in 16 bits); a rate in neither form raises ValueError"""
    if isinstance(rate, bool) or int(rate) != rate:
        raise ValueError(f"flac: the sample rate is an integer number of Hz, got {rate!r}")
    rate = int(rate)
    if rate in RATE_CODES:
        return RATE_CODES[rate]
    if 1 <= rate <= 65535:
        return 13
    raise ValueError(f"flac: sample rate {rate} Hz is neither in the format's table nor codable in 16 bits")


def bound(n: int) -> int:
    """the largest file of n samples: every frame is at most its VERBATIM form, 16 + 2 n_block bytes"""
    n = int(n)
    return HEADER_BYTES + 2 * n + 16 * ((n + BLOCK - 1) // BLOCK)


def _frame_number(f: int) -> bytes:
    """the UTF-8-like coding of the frame number"""
    if f < 0x80:
        return bytes([f])
    n = 2
    while f >= 1 << (5 * n + 1):
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (f >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((f >> (6 * i)) & 0x3F))
    return bytes(out)


def frame_header(f: int, n: int, rate: int) -> bytes:
    """the header of frame f, a block of n samples, with its CRC-8"""
    rc = rate_code(rate)
    h = bytearray([0xFF, 0xF8, ((0x0C if n == BLOCK else 0x07) << 4) | rc, 0x08])
    h += _frame_number(f)
    if n != BLOCK:
        h += bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    if rc == 13:
        h += bytes([rate >> 8, rate & 0xFF])
    h.append(crc8(h))
    return bytes(h)


def _ctz(n: int) -> int:
    return (n & -n).bit_length() - 1


def _analyse(X: np.ndarray):
    """blocks [nb, n] (int64) -> per block (order, p, ks, subframe bits); order -2 CONSTANT, -1 VERBATIM, else FIXED"""
    nb, n = X.shape
    P = min(MAX_PART_ORDER, _ctz(n))
    best = np.full(nb, 8 + 16 * n, np.int64)
    order = np.full(nb, -1, np.int64)
    part = np.zeros(nb, np.int64)
    ks = np.zeros((nb, 1 << MAX_PART_ORDER), np.int64)
    kk = np.arange(MAX_RICE + 1, dtype=np.int64)
    r = X
    for o in range(min(MAX_ORDER, n - 1) + 1):
        if o:
            r = r[:, 1:] - r[:, :-1]
        u = np.zeros((nb, n), np.int64)
        u[:, o:] = (r << 1) ^ (r >> 63)
        sums = np.stack([(u >> k).reshape(nb, 1 << P, n >> P).sum(2) for k in range(MAX_RICE + 1)])      # [k][block][partition]
        levels = {}
        for p in range(P, -1, -1):
            levels[p] = sums
            sums = sums[:, :, 0::2] + sums[:, :, 1::2] if p else sums
        for p in range(P + 1):
            if (n >> p) <= o:
                break
            cnt = np.full(1 << p, n >> p, np.int64)
            cnt[0] -= o
            cost = levels[p] + (kk[:, None, None] + 1) * cnt[None, None, :]
            k_min = cost.argmin(0)                                      # the first minimum: the lowest k
            bits = 8 + 16 * o + 6 + (4 + cost.min(0)).sum(1)
            win = bits < best
            best[win], order[win], part[win] = bits[win], o, p
            ks[win, : 1 << p] = k_min[win]
    const = (X == X[:, :1]).all(1)
    best[const], order[const] = 24, -2
    return order, part, ks, best


def _put(bits: np.ndarray, pos, val, width: int) -> None:
    """writes the `width` low bits of each val, most significant first, at bit positions pos (arrays)"""
    for j in range(width):
        bits[pos + j] = (val >> (width - 1 - j)) & 1


def _subframe(x: np.ndarray, o: int, p: int, ks: np.ndarray, nbits: int) -> bytes:
    n = len(x)
    bits = np.zeros((nbits + 7) // 8 * 8, np.uint8)
    one = np.zeros(1, np.int64)
    if o == -2:
        _put(bits, one, np.array([0]), 8)
        _put(bits, one + 8, x[:1] & 0xFFFF, 16)
    elif o == -1:
        _put(bits, one, np.array([2]), 8)
        _put(bits, 8 + 16 * np.arange(n), x & 0xFFFF, 16)
    else:
        _put(bits, one, np.array([(8 | o) << 1]), 8)
        _put(bits, 8 + 16 * np.arange(o), x[:o] & 0xFFFF, 16)
        _put(bits, one + 8 + 16 * o, np.array([p]), 6)                  # coding method 00, then the partition order
        r = x
        for _ in range(o):
            r = r[1:] - r[:-1]
        u = (r << 1) ^ (r >> 63)
        i = np.arange(o, n)
        S = n >> p
        k = ks[i // S]
        first = (i % S == 0) | (i == o)                                 # a partition's first residual carries the parameter in front
        q = u >> k
        length = q + 1 + k + 4 * first
        pos = 8 + 16 * o + 6 + np.concatenate([[0], np.cumsum(length)[:-1]])
        _put(bits, pos[first], k[first], 4)
        stop = pos + 4 * first + q
        bits[stop] = 1
        for j in range(MAX_RICE):
            m = k > j
            bits[stop[m] + 1 + j] = (u[m] >> (k[m] - 1 - j)) & 1
        assert int(pos[-1] + length[-1]) == nbits
    return np.packbits(bits).tobytes()


def frames(pcm, rate):
    """int16 samples -> (the frames back to back, their lengths in bytes): what ctts_flac_encode_ranges writes for one range"""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise ValueError(f"flac takes a 1-D int16 array, got {pcm.dtype} {pcm.shape}")
    rate_code(rate)
    x = pcm.astype(np.int64)
    n = len(x)
    nf, tail = n // BLOCK, n % BLOCK
    out, lens = [], []
    groups = ([x[: nf * BLOCK].reshape(nf, BLOCK)] if nf else []) + ([x[nf * BLOCK:].reshape(1, tail)] if tail else [])
    f = 0
    for X in groups:
        order, part, ks, nbits = _analyse(X)
        for b in range(len(X)):
            body = frame_header(f, X.shape[1], int(rate)) + _subframe(X[b], int(order[b]), int(part[b]), ks[b], int(nbits[b]))
            body += crc16(body).to_bytes(2, "big")
            out.append(body)
            lens.append(len(body))
            f += 1
    return b"".join(out), np.asarray(lens, np.int64)


def stream_info(n_samples: int, rate: int, frame_lengths) -> bytes:
    """`fLaC` and the one metadata block (34 bytes of STREAMINFO, last-block flag set): 42 bytes"""
    rate_code(rate)
    fl = np.asarray(frame_lengths, np.int64)
    lo, hi = (int(fl.min()), int(fl.max())) if len(fl) else (0, 0)
    if not 0 <= int(n_samples) < 1 << 36:
        raise ValueError("flac: the total sample count takes 36 bits")
    v = (int(rate) << 44) | (0 << 41) | (15 << 36) | int(n_samples)            # 20 bits rate, 3 channels - 1, 5 bits - 1, 36 samples
    return (b"fLaC\x80\x00\x00\x22" + BLOCK.to_bytes(2, "big") * 2 + lo.to_bytes(3, "big") + hi.to_bytes(3, "big") + v.to_bytes(8, "big")
            + bytes(16))


def file_bytes(frame_bytes, frame_lengths, n_samples: int, rate: int) -> np.ndarray:
    """the complete file around frames that are already encoded (the device's): a uint8 array"""
    return np.frombuffer(stream_info(n_samples, rate, frame_lengths) + bytes(frame_bytes), np.uint8)


def encode(pcm, rate) -> bytes:
    """int16 samples -> the whole FLAC file"""
    body, lens = frames(pcm, rate)
    return stream_info(len(pcm), rate, lens) + body


# ---- streams: variable-block-size frames (sync FF F9) that carry the number of their first sample ------------------------------------
# A stream is cut where its pushes end, so its blocks have 16 .. 4096 samples (the last: 1 .. 4096) and a frame says where it starts.  Up
# to 15 samples wait for the next push (a block under 16 samples may only end a stream).  The subframes are the file encoder's, search
# and all; the bytes depend on the cut, the decoded samples do not.  csrc/flac.hip (ctts_flac_stream_step) agrees byte for byte.
MIN_BLOCK = 16
MAX_SAMPLES = 1 << 36


def stream_header(rate) -> bytes:
    """`fLaC` and STREAMINFO of a stream whose end is not known: blocks of 16 .. 4096 samples, frame sizes, total and MD5 unknown (0)"""
    rate_code(rate)
    v = (int(rate) << 44) | (0 << 41) | (15 << 36)
    return b"fLaC\x80\x00\x00\x22" + MIN_BLOCK.to_bytes(2, "big") + BLOCK.to_bytes(2, "big") + bytes(6) + v.to_bytes(8, "big") + bytes(16)


def frame_header_variable(sample: int, n: int, rate: int) -> bytes:
    """the header of the block of n samples whose first is sample `sample` of the stream (up to 36 bits: 1 .. 7 bytes), with its CRC-8"""
    sample, n = int(sample), int(n)
    if not 0 <= sample < MAX_SAMPLES:
        raise ValueError(f"flac: sample number {sample} does not fit 36 bits")
    if not 1 <= n <= BLOCK:
        raise ValueError(f"flac: a block of {n} samples")
    rc = rate_code(rate)
    h = bytearray([0xFF, 0xF9, ((0x0C if n == BLOCK else 0x07) << 4) | rc, 0x08])
    h += _frame_number(sample)
    if n != BLOCK:
        h += bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    if rc == 13:
        h += bytes([int(rate) >> 8, int(rate) & 0xFF])
    h.append(crc8(h))
    return bytes(h)


def stream_plan(carry: int, n_in: int, final: bool):
    """the cutting rule: a stream that holds `carry` samples (0 .. 15) gets n_in more -> (the lengths of the blocks it emits, the samples
    it holds afterwards).  Blocks of 4096 from the front; a rest of 16 or more is one more block; a rest of 1 .. 15 waits, unless the
    push is the last, which emits it."""
    carry, n_in = int(carry), int(n_in)
    if not 0 <= carry < MIN_BLOCK or n_in < 0:
        raise ValueError(f"flac: a stream carries 0 .. 15 samples and is pushed 0 or more (got {carry}, {n_in})")
    avail = carry + n_in
    blocks = [BLOCK] * (avail // BLOCK)
    r = avail % BLOCK
    if not final and (avail < MIN_BLOCK or 0 < r < MIN_BLOCK):
        return (blocks if avail >= MIN_BLOCK else []), (r if avail >= MIN_BLOCK else avail)
    if r:
        blocks.append(r)
    return blocks, 0


def stream_bound(n_in: int) -> int:
    """the most bytes one push of n_in samples emits: with the carry up to n_in + 15 samples in at most (n_in + 15) // 4096 + 1 frames,
    each at most its VERBATIM form -- a header of up to 16 bytes (7 of them the sample number), the subframe's byte, 2 n, the CRC-16"""
    n = int(n_in) + MIN_BLOCK - 1
    return 2 * n + 19 * (n // BLOCK + 1)


def stream_frames(pcm, rate, sample: int, blocks) -> bytes:
    """the frames of consecutive blocks (their lengths in `blocks`) of int16 samples, the first of which is sample `sample`"""
    x = np.asarray(pcm).astype(np.int64)
    out, at = [], 0
    for n in blocks:
        X = x[at: at + n].reshape(1, n)
        order, part, ks, nbits = _analyse(X)
        body = frame_header_variable(sample + at, n, int(rate)) + _subframe(X[0], int(order[0]), int(part[0]), ks[0], int(nbits[0]))
        out.append(body + crc16(body).to_bytes(2, "big"))
        at += n
    assert at == len(x)
    return b"".join(out)


class StreamEncoder:
    """One stream on the host: push(pcm, final=False) -> the bytes of the frames that push completes (possibly none).  The frames of all
    pushes behind `stream_header(rate)` are a FLAC stream whose samples are the pushes, concatenated."""

    def __init__(self, rate, first_sample: int = 0):
        rate_code(rate)
        if not 0 <= int(first_sample) < MAX_SAMPLES:
            raise ValueError(f"flac: sample number {first_sample} does not fit 36 bits")
        self.rate, self.sample, self.done = int(rate), int(first_sample), False        # sample: the number of the first sample held
        self.held = np.zeros((0,), np.int16)

    def push(self, pcm, final: bool = False) -> bytes:
        pcm = np.asarray(pcm)
        if pcm.dtype != np.int16 or pcm.ndim != 1:
            raise ValueError(f"flac takes a 1-D int16 array, got {pcm.dtype} {pcm.shape}")
        if self.done:
            raise ValueError("flac: the stream has had its last push")
        if self.sample + len(self.held) + len(pcm) >= MAX_SAMPLES:
            raise ValueError("flac: the push would take the stream's sample number to 2^36")
        blocks, carry = stream_plan(len(self.held), len(pcm), final)
        x = np.concatenate([self.held, pcm])
        n = sum(blocks)
        out = stream_frames(x[:n], self.rate, self.sample, blocks)
        self.held, self.sample, self.done = x[n:].copy(), self.sample + n, bool(final)
        assert len(self.held) == carry
        return out

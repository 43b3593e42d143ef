"""An independent FLAC decoder for the tests, written from the format description (RFC 9639): it shares no code with chattts_amd/flac.py.
Mono, CONSTANT / VERBATIM / FIXED 0-4 subframes with 4- or 5-bit Rice partitions (escape partitions included);
anything else (LPC subframes, reserved codes, wasted bits, stereo decorrelation) raises, and so does every sync, CRC-8 or CRC-16 mismatch.
On top of the format it checks what this project's streams promise: the frame numbers count up from 0, every block but the last has
4096 samples, and the total matches STREAMINFO (also the frame-size bounds where STREAMINFO gives them).

    decode(data) -> (int16 samples, rate);  decode(data, info=True) -> (samples, rate, dict with the STREAMINFO fields and per-frame facts)
"""
import numpy as np


class FlacError(ValueError):
    pass


def _crc8(data):
    crc = 0
    for byte in data:
        for bit in range(7, -1, -1):
            top = (crc >> 7) & 1
            crc = (crc << 1) & 0xFF
            if top ^ ((byte >> bit) & 1):
                crc ^= 0x07
    return crc


def _crc16(data):
    crc = 0
    for byte in data:
        for bit in range(7, -1, -1):
            top = (crc >> 15) & 1
            crc = (crc << 1) & 0xFFFF
            if top ^ ((byte >> bit) & 1):
                crc ^= 0x8005
    return crc


class _Bits:
    """big-endian bit reader over one frame's bytes (a Python integer; the positions of the one bits serve the unary runs)"""

    def __init__(self, data):
        self.total = 8 * len(data)
        self.big = int.from_bytes(data, "big")
        self.ones = np.flatnonzero(np.unpackbits(np.frombuffer(data, np.uint8))).tolist() + [1 << 62]
        self.oi = 0
        self.pos = 0

    def read(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.total:
            raise FlacError("the stream ends inside a frame")
        self.pos += n
        return (self.big >> (self.total - self.pos)) & ((1 << n) - 1)

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        ones, oi, pos = self.ones, self.oi, self.pos
        while ones[oi] < pos:
            oi += 1
        if ones[oi] >= self.total:
            raise FlacError("the stream ends inside a unary run")
        self.oi, self.pos = oi, ones[oi] + 1
        return ones[oi] - pos

    def align(self):
        while self.pos & 7:
            if self.read(1):
                raise FlacError("non-zero padding bit")


def _crc16_many(data, spans):
    """the bitwise CRC-16 of every span at once: the frames are right-aligned in a matrix (leading zero bytes leave a CRC with
    initial value 0 unchanged) and all registers step together, bit by bit"""
    if not spans:
        return []
    width = max(e - s for s, e in spans)
    m = np.zeros((len(spans), width), np.uint8)
    for i, (s, e) in enumerate(spans):
        m[i, width - (e - s):] = np.frombuffer(data[s:e], np.uint8)
    crc = np.zeros(len(spans), np.uint32)
    for col in range(width):
        byte = m[:, col].astype(np.uint32)
        for bit in range(7, -1, -1):
            top = ((crc >> 15) ^ (byte >> bit)) & 1
            crc = ((crc << 1) & 0xFFFF) ^ (top * 0x8005)
    return [int(c) for c in crc]


_BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _residual(br, n, order):
    method = br.read(2)
    if method > 1:
        raise FlacError(f"reserved residual coding method {method}")
    width, escape = (4, 15) if method == 0 else (5, 31)
    p = br.read(4)
    if n % (1 << p) or (n >> p) < order:
        raise FlacError(f"partition order {p} does not fit a block of {n} with predictor order {order}")
    out = []
    for j in range(1 << p):
        count = (n >> p) - (order if j == 0 else 0)
        if count < 0:
            raise FlacError("a partition shorter than the predictor order")
        k = br.read(width)
        if k == escape:
            raw = br.read(5)
            out.extend(br.signed(raw) if raw else 0 for _ in range(count))
            continue
        for _ in range(count):
            q = br.unary()
            u = (q << k) | (br.read(k) if k else 0)
            out.append((u >> 1) ^ -(u & 1))
    return out, p


def _subframe(br, n, bps):
    if br.read(1):
        raise FlacError("subframe padding bit set")
    kind = br.read(6)
    if br.read(1):
        raise FlacError("wasted bits are not supported")
    if kind == 0:
        return [br.signed(bps)] * n, "CONSTANT"
    if kind == 1:
        return [br.signed(bps) for _ in range(n)], "VERBATIM"
    if 8 <= kind <= 12:
        order = kind - 8
        if order > n:
            raise FlacError("more warm-up samples than the block holds")
        s = [br.signed(bps) for _ in range(order)]
        res, p = _residual(br, n, order)
        coef = _FIXED[order]
        for r in res:
            s.append(r + sum(c * s[-1 - i] for i, c in enumerate(coef)))
        return s, f"FIXED{order}/{p}"
    raise FlacError(f"unsupported subframe type {kind:#08b}")


def _utf8(data, pos):
    b0 = data[pos]
    if b0 < 0x80:
        return b0, pos + 1
    n = 0
    while b0 & (0x80 >> n):
        n += 1
    if n < 2 or n > 7:
        raise FlacError("bad frame-number lead byte")
    v = b0 & (0x7F >> n)
    for i in range(1, n):
        c = data[pos + i]
        if c & 0xC0 != 0x80:
            raise FlacError("bad frame-number continuation byte")
        v = (v << 6) | (c & 0x3F)
    return v, pos + n


def decode(data, info=False, block=4096):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, si = 4, None
    while True:
        if pos + 4 > len(data):
            raise FlacError("the metadata ends early")
        last, kind, size = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1: pos + 4], "big")
        body = data[pos + 4: pos + 4 + size]
        if len(body) != size:
            raise FlacError("a metadata block runs past the end")
        if kind == 0:
            if size != 34 or si is not None or pos != 4:
                raise FlacError("STREAMINFO must come first, once, with 34 bytes")
            v = int.from_bytes(body[10:18], "big")
            si = dict(min_block=int.from_bytes(body[0:2], "big"), max_block=int.from_bytes(body[2:4], "big"),
                      min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"), rate=v >> 44,
                      channels=((v >> 41) & 7) + 1, bps=((v >> 36) & 31) + 1, total=v & ((1 << 36) - 1), md5=body[18:34])
        pos += 4 + size
        if last:
            break
    if si is None:
        raise FlacError("no STREAMINFO")
    if si["channels"] != 1:
        raise FlacError("only mono streams are supported")
    bps = si["bps"]
    samples, kinds, sizes, blocks, spans = [], [], [], [], []
    want = 0
    while pos < len(data):
        start = pos
        if len(data) - pos < 6 or data[pos] != 0xFF or data[pos + 1] & 0xFE != 0xF8:
            raise FlacError(f"no frame sync at byte {pos}")
        if data[pos + 1] & 1:
            raise FlacError("variable block size stream")
        bs_code, sr_code = data[pos + 2] >> 4, data[pos + 2] & 15
        ch, ss, rsv = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7, data[pos + 3] & 1
        if rsv or ch != 0:
            raise FlacError("reserved bit or a channel assignment other than mono")
        if {0: bps, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}.get(ss) != bps:
            raise FlacError(f"sample-size code {ss} disagrees with STREAMINFO's {bps} bits")
        number, pos = _utf8(data, pos + 4)
        if bs_code == 0:
            raise FlacError("reserved block-size code")
        if bs_code == 6:
            n, pos = data[pos] + 1, pos + 1
        elif bs_code == 7:
            n, pos = int.from_bytes(data[pos: pos + 2], "big") + 1, pos + 2
        else:
            n = _BLOCK_SIZES[bs_code]
        if sr_code == 0:
            rate = si["rate"]
        elif sr_code == 12:
            rate, pos = data[pos] * 1000, pos + 1
        elif sr_code == 13:
            rate, pos = int.from_bytes(data[pos: pos + 2], "big"), pos + 2
        elif sr_code == 14:
            rate, pos = int.from_bytes(data[pos: pos + 2], "big") * 10, pos + 2
        elif sr_code == 15:
            raise FlacError("invalid sample-rate code")
        else:
            rate = _RATES[sr_code]
        if _crc8(data[start: pos]) != data[pos]:
            raise FlacError(f"frame {number}: header CRC-8 mismatch")
        pos += 1
        if rate != si["rate"]:
            raise FlacError(f"frame {number}: rate {rate} differs from STREAMINFO's {si['rate']}")
        if number != want:
            raise FlacError(f"frame number {number} where {want} was due")
        want += 1
        if blocks and blocks[-1] != block:
            raise FlacError("a block other than the last is not 4096 samples long")
        if n > block:
            raise FlacError(f"a block of {n} samples")
        br = _Bits(data[pos: pos + (n * bps + 7) // 8 + 64])
        s, kind = _subframe(br, n, bps)
        if len(s) != n:
            raise FlacError("subframe length")
        br.align()
        pos += br.pos >> 3
        if pos + 2 > len(data):
            raise FlacError(f"frame {number}: the stream ends before the CRC-16")
        spans.append((start, pos))
        pos += 2
        samples.extend(s)
        kinds.append(kind)
        sizes.append(pos - start)
        blocks.append(n)
    for f, ((a, b), crc) in enumerate(zip(spans, _crc16_many(data, spans))):
        # (short frames also go through the scalar loop: the two forms of the bitwise CRC check each other)
        if crc != int.from_bytes(data[b: b + 2], "big") or (b - a < 64 and crc != _crc16(data[a:b])):
            raise FlacError(f"frame {f}: CRC-16 mismatch")
    if len(samples) != si["total"]:
        raise FlacError(f"{len(samples)} samples decoded, STREAMINFO says {si['total']}")
    if si["min_block"] != block or si["max_block"] != block:
        raise FlacError("STREAMINFO's block sizes are not 4096")
    if sizes and (si["min_frame"], si["max_frame"]) != (min(sizes), max(sizes)):
        raise FlacError("STREAMINFO's frame sizes are not the stream's")
    lim = 1 << (bps - 1)
    if any(v < -lim or v >= lim for v in samples):
        raise FlacError("a decoded sample leaves the sample size")
    pcm = np.asarray(samples, np.int64).astype(np.int16 if bps == 16 else np.int32)
    if info:
        return pcm, si["rate"], dict(si, kinds=kinds, frame_sizes=sizes, blocks=blocks)
    return pcm, si["rate"]

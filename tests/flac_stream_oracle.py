"""The independent decoder of tests/flac_oracle.py for STREAMED FLAC: variable-block-size frames (sync FF F9) whose header carries the
number of the block's first sample in up to 36 bits.  Written from the format description (RFC 9639); it shares no code with
chattts_amd/flac.py -- the CRCs, the bit reader and the subframe decoder are flac_oracle's.  On top of the format it checks what this
project's streams promise: STREAMINFO says blocks of 16 .. 4096 samples, frame sizes, total and MD5 unknown; the first frame's number is
the stream's first sample and every later one the previous number plus the previous block size; every block but the last has 16 .. 4096
samples (the last 1 .. 4096).

    read_header(data, pos) -> dict(sample, n, rate, end): one frame header, CRC-8 checked
    decode(data, first_sample=0) -> (int16 samples, rate);  info=True adds a dict with the STREAMINFO fields and per-frame facts
"""
import numpy as np

from tests.flac_oracle import FlacError, _Bits, _crc8, _crc16, _crc16_many, _subframe, _utf8, _BLOCK_SIZES, _RATES

MIN_BLOCK, MAX_BLOCK = 16, 4096


def read_header(data, pos=0, bps=16):
    data = bytes(data)
    start = pos
    if len(data) - pos < 6 or data[pos] != 0xFF or data[pos + 1] != 0xF9:
        raise FlacError(f"no variable-block-size frame sync (FF F9) at byte {pos}")
    bs_code, sr_code = data[pos + 2] >> 4, data[pos + 2] & 15
    ch, ss, rsv = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7, data[pos + 3] & 1
    if rsv or ch != 0:
        raise FlacError("reserved bit or a channel assignment other than mono")
    if {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}.get(ss) != bps:
        raise FlacError(f"sample-size code {ss} is not {bps} bits (a streamable frame says its sample size itself)")
    sample, pos = _utf8(data, pos + 4)
    if sample >= 1 << 36:
        raise FlacError("a sample number beyond 36 bits")
    if bs_code == 0:
        raise FlacError("reserved block-size code")
    if bs_code == 6:
        n, pos = data[pos] + 1, pos + 1
    elif bs_code == 7:
        n, pos = int.from_bytes(data[pos: pos + 2], "big") + 1, pos + 2
    else:
        n = _BLOCK_SIZES[bs_code]
    if sr_code == 12:
        rate, pos = data[pos] * 1000, pos + 1
    elif sr_code == 13:
        rate, pos = int.from_bytes(data[pos: pos + 2], "big"), pos + 2
    elif sr_code == 14:
        rate, pos = int.from_bytes(data[pos: pos + 2], "big") * 10, pos + 2
    elif sr_code in (0, 15):
        raise FlacError("a streamable frame says its rate itself (code 0), and code 15 is invalid")
    else:
        rate = _RATES[sr_code]
    if _crc8(data[start: pos]) != data[pos]:
        raise FlacError(f"the frame at sample {sample}: header CRC-8 mismatch")
    return dict(sample=sample, n=n, rate=rate, end=pos + 1)


def decode(data, first_sample=0, info=False):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if len(data) < 42 or data[4:8] != b"\x80\x00\x00\x22":
        raise FlacError("STREAMINFO must be the one metadata block: 34 bytes, last-block flag set")
    body = data[8:42]
    v = int.from_bytes(body[10:18], "big")
    si = dict(min_block=int.from_bytes(body[0:2], "big"), max_block=int.from_bytes(body[2:4], "big"),
              min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"), rate=v >> 44,
              channels=((v >> 41) & 7) + 1, bps=((v >> 36) & 31) + 1, total=v & ((1 << 36) - 1), md5=body[18:34])
    want = dict(min_block=MIN_BLOCK, max_block=MAX_BLOCK, min_frame=0, max_frame=0, channels=1, bps=16, total=0, md5=bytes(16))
    for key, val in want.items():
        if si[key] != val:
            raise FlacError(f"STREAMINFO of a stream: {key} is {si[key]!r}, not {val!r}")
    if not 1 <= si["rate"] < 1 << 20:
        raise FlacError("STREAMINFO's rate")
    pos = 42
    samples, kinds, sizes, blocks, numbers, spans = [], [], [], [], [], []
    due = int(first_sample)
    while pos < len(data):
        start = pos
        h = read_header(data, pos)
        pos, n = h["end"], h["n"]
        if h["rate"] != si["rate"]:
            raise FlacError(f"the frame at sample {h['sample']}: rate {h['rate']} differs from STREAMINFO's {si['rate']}")
        if h["sample"] != due:
            raise FlacError(f"a frame says it starts at sample {h['sample']} where {due} was due")
        if blocks and not MIN_BLOCK <= blocks[-1] <= MAX_BLOCK:
            raise FlacError(f"a block other than the last has {blocks[-1]} samples")
        if not 1 <= n <= MAX_BLOCK:
            raise FlacError(f"a block of {n} samples")
        due += n
        br = _Bits(data[pos: pos + (n * 16 + 7) // 8 + 64])
        s, kind = _subframe(br, n, 16)
        if len(s) != n:
            raise FlacError("subframe length")
        br.align()
        pos += br.pos >> 3
        if pos + 2 > len(data):
            raise FlacError(f"the frame at sample {h['sample']}: the stream ends before the CRC-16")
        spans.append((start, pos))
        pos += 2
        samples.extend(s)
        kinds.append(kind)
        sizes.append(pos - start)
        blocks.append(n)
        numbers.append(h["sample"])
    for (a, b), crc in zip(spans, _crc16_many(data, spans)):
        if crc != int.from_bytes(data[b: b + 2], "big") or (b - a < 64 and crc != _crc16(data[a:b])):
            raise FlacError(f"the frame at byte {a}: CRC-16 mismatch")
    if any(v < -32768 or v > 32767 for v in samples):
        raise FlacError("a decoded sample leaves 16 bits")
    pcm = np.asarray(samples, np.int64).astype(np.int16)
    if info:
        return pcm, si["rate"], dict(si, kinds=kinds, frame_sizes=sizes, blocks=blocks, numbers=numbers)
    return pcm, si["rate"]

"""What the streamed output stages of `CodecEngine` share on the host: the pool of per-stream device state, the stages' records, the checks
of a step's pushes, the parser of the int16 pushes, and the rule that sorts a call's pushes into rounds.  Python integers and, in the pool,
`torch.zeros` / `torch.cat` only: no kernel and no library call, so all of it runs without a device."""
from typing import Any, NamedTuple, Optional

import torch


# -- the host record of an open stream, one kind per stage; `done`: the stream has had its last push ----------------------------------
class TimeScaleRec(NamedTuple):
    num: int              # the speed, quantised: num / den
    den: int
    pushed: int           # samples pushed
    phase: int            # which half of the slot's carry the next step reads
    done: bool


class ResampleRec(NamedTuple):
    orig: int
    new: int
    pushed: int
    emitted: int          # outputs emitted
    phase: int
    done: bool


class LimiterRec(NamedTuple):
    rate: int
    gain: Any             # the float32 pre-gain
    pushed: int
    emitted: int
    phase: int
    done: bool


class CompressRec(NamedTuple):
    rate: int
    spec: Any             # a checked compressor spec (compressor.check)
    pushed: int
    emitted: int
    phase: int
    done: bool


class PauseRec(NamedTuple):
    rate: int
    spec: Any             # pauses.PauseSpec
    pushed: int
    phase: int
    done: bool
    held: int             # frames that wait, as the last step's copy told
    emitted: int


class FlacRec(NamedTuple):
    rate: int
    sample: int           # the number of the first sample the stream holds
    carry: int            # samples held (0 .. 15)
    done: bool


class AdpcmRec(NamedTuple):
    rate: int
    carry: int            # samples held (0 .. S - 1)
    done: bool


class StatePool:
    """The state of one stage's open streams: named device buffers [slots, *tail], the free list and one host record per open handle
    (a handle is a slot).  `buffers`: {name: (tail, dtype)}.  Without a `device` nothing is allocated (`buf` stays empty) and the pool
    only counts its slots: what the planning code needs."""

    def __init__(self, label: str, slots: int, buffers: Optional[dict] = None, device=None):
        self.label, self.slots, self.records = label, int(slots), {}
        self.free = list(range(self.slots - 1, -1, -1))
        self.buf = {} if device is None else {k: torch.zeros((self.slots, *tail), dtype=dt, device=device) for k, (tail, dt) in (buffers or {}).items()}

    def open(self, record) -> int:
        """-> a free slot, now `record`'s; a slot just closed goes out first.  A full pool doubles first: every buffer keeps its rows and
        gets as many zero rows (`torch.cat`: stream-ordered behind every step so far)."""
        if not self.free:
            self.buf = {k: torch.cat([b, torch.zeros_like(b)]) for k, b in self.buf.items()}
            self.free = list(range(2 * self.slots - 1, self.slots - 1, -1))
            self.slots *= 2
        slot = self.free.pop()
        self.records[slot] = record
        return slot

    def close(self, handle: int) -> None:
        if self.records.pop(int(handle), None) is None:
            raise ValueError(f"{self.label}: stream {handle} is not open")
        self.free.append(int(handle))

    @property
    def in_use(self) -> int:
        return len(self.records)

    def get(self, handle: int):
        rec = self.records.get(int(handle))
        if rec is None:
            raise ValueError(f"{self.label}: stream {handle} is not open")
        return rec

    def live(self, handle: int, ahead=None):
        """the record the stream's next push continues -- `ahead[handle]` where the call has planned a push of it already --, refused
        once that record is done"""
        rec = self.get(handle)
        if ahead:
            rec = ahead.get(int(handle), rec)
        if rec.done:
            raise ValueError(f"{self.label}: stream {handle} has had its last push")
        return rec

    def commit(self, records: dict) -> None:
        """{handle: its new record}, behind the launch: the only way a record changes"""
        self.records.update(records)


def rounds(handles):
    """the handles of a call's pushes, in order (None: no push) -> (rnd, members): the r-th push of a stream goes to round r -- rnd[i] is
    push i's round (-1 for None), members[r] the pushes of round r in the order given"""
    seen, rnd, members = {}, [], []
    for i, h in enumerate(handles):
        if h is None:
            rnd.append(-1)
            continue
        r = seen[h] = seen.get(h, -1) + 1
        if r == len(members):
            members.append([])
        members[r].append(i)
        rnd.append(r)
    return rnd, members


def check_pushes(label: str, pushes, n_el: Optional[int] = None, most: Optional[int] = 1024, once: bool = True) -> None:
    """what every `*_stream_step` refuses before it plans: no push, more than `most`, a stream twice (`once`), and with `n_el`, the
    tensor's elements, a push [(handle, start, n, ..)] outside them"""
    if len(pushes) < 1:
        raise ValueError(f"{label}: nothing to step")
    if most is not None and len(pushes) > most:
        raise ValueError(f"{label}: at most {most} streams in one step")
    if once and len({int(p[0]) for p in pushes}) != len(pushes):
        raise ValueError(f"{label}: a stream appears twice in one step")
    if n_el is not None:
        for p in pushes:
            if int(p[1]) < 0 or int(p[2]) < 0 or int(p[1]) + int(p[2]) > n_el:
                raise ValueError(f"{label}: a push lies outside the tensor")


def int16_pushes(label: str, pcm, pushes, counts, masks, live):
    """The arguments of a step of int16 streams (FLAC, ADPCM), checked: `pushes` = [(handle, start, n, final[, count_idx, masked])] ->
    per push (handle, start, n, final, count_idx or -1, masked, the stream's record).  `live`: handle -> its record, refusing a stream
    that is not open or has had its last push.  A generator: the call's checks run with the first push, those of push k when it is
    asked for, so a stage's own refusal of push k - 1 still comes first."""
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()):
        raise ValueError(f"{label}: a contiguous int16 device tensor")
    if counts is not None and not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()):
        raise ValueError(f"{label}: `counts` must be a contiguous int64 device tensor")
    if masks is not None and not (masks.is_cuda and masks.dtype == torch.uint8 and masks.is_contiguous()):
        raise ValueError(f"{label}: `masks` must be a contiguous uint8 device tensor")
    check_pushes(label, pushes)
    n_el = pcm.numel()
    for k, p in enumerate(pushes):
        h, start, n, final = int(p[0]), int(p[1]), int(p[2]), bool(p[3])
        ci = int(p[4]) if len(p) > 4 and p[4] is not None else -1
        masked = len(p) > 5 and bool(p[5])
        rec = live(h)
        if n < 0 or start < 0 or start + n > n_el:
            raise ValueError(f"{label}: a push lies outside the tensor")
        if ci >= 0 and (counts is None or ci >= counts.numel()):
            raise ValueError(f"{label}: push {k} reads count {ci}, beyond `counts`")
        if masked and (masks is None or masks.numel() * 8 < start + n):
            raise ValueError(f"{label}: push {k} is masked, and `masks` does not reach its end")
        if (ci >= 0 or masked) and not final:
            raise ValueError(f"{label}: push {k} leaves its length to the device but is not final")
        yield h, start, n, final, ci, masked, rec

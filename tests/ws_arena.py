"""Guarded, pre-filled device memory for the workspace-contract tests (tests/test_gpu_workspace_contract.py).

Every hot path of the library runs inside a caller-supplied byte buffer it carves itself; `chattts_amd.engine.device_scratch` is the
one place the package allocates such buffers.  An `Arena` stands in for it: ONE allocation, cut into

    front guard | payload | back guard | front guard | payload | back guard | ... | unused rest

`take(nbytes)` hands out a view of EXACTLY `nbytes` whose first byte sits on a 256-byte boundary (the granule of `align_up`,
csrc/capi.hip), pre-filled with the arena's payload pattern; everything that is not payload holds the guard pattern and is compared
byte for byte by `assert_guards_intact()`.  So a size function that is short, or a kernel that writes past its last field, shows as a
damaged guard, and a kernel that reads what it never wrote shows as a result that depends on the payload pattern.

Works on any torch device: the arithmetic is tested on the CPU (tests/test_workspace_contract_host.py)."""
from __future__ import annotations

import torch

GUARD_BYTE = 0x5A                 # tests/gpu_util.CANARY32, byte by byte
GUARD_MIN = 64 * 1024             # bytes of guard on each side of every payload, at least
ALIGN = 256                       # align_up's granule (csrc/capi.hip)
# payload patterns: zeros; all ones (NaN as f32 / bf16 / f16, -1 as int32); 0x7F (3.4e38 as f32 and bf16, a NaN as f16, 2139062143 as int32)
PATTERNS = (0x00, 0xFF, 0x7F)


class Arena:
    def __init__(self, capacity: int, fill: int, device, guard: int = GUARD_MIN):
        """`capacity`: payload bytes the arena must be able to hand out in all -- `takes` regions of guards and alignment come on
        top per take (see `room`); `fill`: the payload pattern, a byte; `guard`: bytes of each guard, at least GUARD_MIN"""
        if not 0 <= int(fill) <= 0xFF or int(fill) == GUARD_BYTE:
            raise ValueError("the payload pattern is a byte other than the guard's")
        if guard < GUARD_MIN:
            raise ValueError(f"a guard is at least {GUARD_MIN} bytes")
        self.fill, self.guard, self.device = int(fill), int(guard), torch.device(device)
        self.buf = torch.full((int(capacity),), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        self._base = self.buf.data_ptr()
        self._end = 0                 # offset behind the last payload handed out
        self.regions = []             # (offset, nbytes) of every payload, in order
        self.sizes = []               # the sizes requested, in order

    @staticmethod
    def room(sizes, guard: int = GUARD_MIN) -> int:
        """a capacity that holds takes of `sizes` bytes, whatever the allocation's own alignment"""
        return sum(int(n) + 2 * guard + ALIGN for n in sizes) + ALIGN

    @property
    def takes(self) -> int:
        return len(self.sizes)

    def take(self, nbytes: int) -> torch.Tensor:
        """a uint8 view of exactly `nbytes`, 256-byte aligned, pre-filled, with at least `guard` bytes of guard pattern on either side
        that no other take shares"""
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError("a negative size")
        lo = self._end + (2 if self.regions else 1) * self.guard      # the previous take's back guard, then this one's front guard
        lo += (-(self._base + lo)) % ALIGN
        if lo + nbytes + self.guard > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes: take {self.takes} of {nbytes} bytes does not fit behind {self._end}")
        view = self.buf[lo: lo + nbytes]
        view.fill_(self.fill)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()       # whichever stream the caller goes on with finds the pattern
        self.regions.append((lo, nbytes))
        self.sizes.append(nbytes)
        self._end = lo + nbytes
        return view

    def device_scratch(self, nbytes: int, device) -> torch.Tensor:
        """the signature of `chattts_amd.engine.device_scratch`: what a test puts in its place"""
        assert torch.device(device).type == self.device.type, (device, self.device)
        return self.take(nbytes)

    def codec_ws_bytes(self, n: int):
        """the body of an override of `CodecEngine._ws_bytes`: a view of exactly the `n` bytes asked for, and `n` as its size (the
        engine's own grow-only buffer hands the library whatever it has grown to)"""
        return self.take(n), int(n)

    def _gaps(self):
        """(lo, hi, owner) of every stretch of guard: `owner(offset)` names the take a damaged byte belongs to"""
        prev_end, out = 0, []
        for i, (lo, n) in enumerate(self.regions):
            out.append((prev_end, lo, i))
            prev_end = lo + n
        out.append((prev_end, self.buf.numel(), len(self.regions)))
        return out

    def first_damage(self):
        """None, or (offset, text) of the first guard byte that no longer holds the pattern"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for lo, hi, i in self._gaps():
            bad = self.buf[lo:hi] != GUARD_BYTE
            if not bool(bad.any()):
                continue
            at = lo + int(torch.nonzero(bad)[0, 0])
            val = int(self.buf[at])
            if not self.regions:
                where = "nothing was handed out"
            elif i > 0 and (i == len(self.regions) or at < self.regions[i - 1][0] + self.regions[i - 1][1] + self.guard):
                p_lo, p_n = self.regions[i - 1]
                where = f"{at - (p_lo + p_n)} bytes behind the end of take {i - 1} ({p_n} bytes)"
            else:
                p_lo, p_n = self.regions[i]
                where = f"{p_lo - at} bytes in front of take {i} ({p_n} bytes)"
            return at, f"guard byte at arena offset {at} is 0x{val:02X}, not 0x{GUARD_BYTE:02X}: {where}"
        return None

    def assert_guards_intact(self):
        hit = self.first_damage()
        assert hit is None, hit[1]

"""The cuts of the compressor stream tests: every way of cutting a signal of n samples into pushes at which a stream can go wrong, sized by
the stream's own B, A and H.  A cut is a list of push sizes that sum to n; the last push is the final one.  The signals are those of
`compressor_cases`."""
from functools import lru_cache

import numpy as np

from chattts_amd import compressor as CP

from tests import compressor_cases as CC

RATES = CC.RATES
TILE = CC.TILE


def _fit(n: int, sizes, tail: bool = True):
    """the sizes, cut off where the signal ends, then (with `tail`) the rest as the last push"""
    out, left = [], n
    for s in sizes:
        s = min(int(s), left)
        out.append(s)
        left -= s
    if tail or left:
        out.append(left)
    return out


def cuts(n: int, B: int, A: int, H: int):
    """[(name, [push sizes])] for a signal of n samples"""
    lag, reach = (A + 1) * B, (A + H + 2) * B
    out = [("whole", [n]),
           ("singles", _fit(n, [1] * 5)),
           ("block", _fit(n, [B - 1, B, B + 1])),
           ("lag", _fit(n, [lag - 1, lag, lag + B, lag + B + 1])),
           ("reach_lo", _fit(n, [reach - 1])),
           ("reach_hi", _fit(n, [reach + 1])),
           ("tile_lo", _fit(n, [TILE * B - 1])),
           ("tile", _fit(n, [TILE * B])),
           ("tile_hi", _fit(n, [TILE * B + 1])),
           ("empties", _fit(n, [B + 3, 0, 0, lag, 0, 2 * B])),
           ("all_then_empty", [n, 0]),
           ("short_final", _fit(n, [max(0, n - (B - 1))])),
           ("under_lag", _fit(n, [B // 2, 1, lag - B - 2, 0], tail=True))]
    for name, c in out:
        assert sum(c) == n and all(v >= 0 for v in c), (name, c)
    return out


CUT_NAMES = [name for name, _ in cuts(10000, 24, 5, 60)]


def case_cuts(fs: int, x: np.ndarray, spec):
    A, H = CP.blocks(CP.check(spec))
    return cuts(len(x), fs // 1000, A, H)


def run_twin(fs: int, x: np.ndarray, spec, cut):
    """the twin over one cut -> (chunks, record, the most raw samples and block gains it carried, the plans' n_out)"""
    sc = CP.StreamCompressor(fs, spec)
    chunks, most_c, most_h, n_out, at = [], 0, 0, [], 0
    for k, n in enumerate(cut):
        final = k == len(cut) - 1
        p = CP.stream_plan(sc.B, sc.A, sc.pushed, sc.emitted, n, final, sc.H)
        chunks.append(sc.push(x[at: at + n], final))
        at += n
        n_out.append(p["n_out"])
        assert len(sc.carry) == p["carry_out"] and len(sc.hist) == p["c_keep"]
        most_c, most_h = max(most_c, len(sc.carry)), max(most_h, len(sc.hist))
    return chunks, sc.stats.copy(), most_c, most_h, n_out


@lru_cache(maxsize=None)
def totals_under_lag(fs: int):
    """signals shorter than (A + 1) B, spread over several pushes: nothing is emitted before the last"""
    B = fs // 1000
    out = []
    for k, spec in enumerate(CC.SPECS):
        A, H = CP.blocks(CP.check(spec))
        n = (A + 1) * B - 1
        out.append((f"under_{k}", CC.enveloped(50 + k, n, B), spec, [B // 2, 0, B, n - B - B // 2]))
    return out

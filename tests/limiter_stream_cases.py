"""How the limiter-stream tests cut a segment into pushes: every family of the issue, sized by the stream's own W = fs // 100.  A cut is a
list of push sizes whose last entry, None, takes what is left (possibly nothing: an empty final push); sizes are clipped to what the
segment still has, so a short segment sees empty pushes in the middle and totals of 1 or of less than 2 W spread over several pushes."""
from tests import limiter_cases as LCs

RATES = LCs.RATES
TILE = LCs.TILE


def cuts(fs: int) -> dict:
    W = fs // 100
    return {
        "whole": [None],
        "ones": [1, 1, 1, 1, 1, None],                                  # single samples, then the rest
        "w2": [2 * W - 1, 2 * W, 2 * W + 1, None],                      # around the lag
        "w4": [4 * W - 1, 4 * W, 4 * W + 1, None],                      # around the carry
        "tile": [TILE - 1, TILE, TILE + 1, None],                       # around the kernel's tile: 2047 / 2048 / 2049
        "empties": [W + 3, 0, 0, 3 * W, 0, None],                       # empty pushes in the middle
        "empty_final": [TILE + 5, 1 << 30, None],                       # everything is in before the last push, which is empty
        "short_final": ["-", None],                                     # all but W + 1 samples, then a final push shorter than 2 W
        "small": [W // 3, 0, W // 3, 1, None],                          # totals under 2 W over several pushes (the segments of 1 and W)
    }


def schedule(n: int, cut, fs: int):
    """the push sizes of a segment of n samples under `cut`: they add up to n, the last one is the final push"""
    W = fs // 100
    left, out = n, []
    for c in cut[:-1]:
        c = max(0, n - (W + 1)) if c == "-" else c
        out.append(min(c, left))
        left -= out[-1]
    return out + [left]

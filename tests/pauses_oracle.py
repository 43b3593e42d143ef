"""An independent, serial definition of pause control (chattts_amd/pauses.py states it; this file shares no code with it): ONE Python
loop over a segment's frames with an explicit run state machine.  Dilation is a countdown from the last active frame (forwards) and to
the next one (a second loop, backwards); the quiet runs are then classified leading / inner / trailing / alone as the loop meets
them.  Its own crossfade, its own record."""
import math

import numpy as np

DEFAULTS = dict(max_pause_ms=400, lead_ms=50, tail_ms=100, threshold_db=-50.0, pad_ms=30)


def _frames(ms):
    return int(math.ceil(ms / 10))


def trim(x, fs, spec=None):
    """x float32 [n >= 1] at fs Hz, spec a dict of the five fields (missing ones default) -> (y float32, record: list of 8 ints)"""
    p = dict(DEFAULTS)
    p.update(spec or {})
    x = np.asarray(x, dtype=np.float32)
    n, F = len(x), fs // 100
    nF = (n + F - 1) // F
    P, lead, tail, pad = _frames(p["max_pause_ms"]), _frames(p["lead_ms"]), _frames(p["tail_ms"]), _frames(p["pad_ms"])
    thr = np.float32(10.0 ** (p["threshold_db"] / 20.0))
    # activity
    active = []
    for j in range(nF):
        hit = False
        for v in x[j * F: min((j + 1) * F, n)]:
            if not (abs(v) < thr):
                hit = True
                break
        active.append(hit)
    # dilation by countdown
    speech = [False] * nF
    left = 0                                        # frames the last active one still covers
    for j in range(nF):
        if active[j]:
            left = pad + 1
        if left > 0:
            speech[j] = True
            left -= 1
    left = 0
    for j in range(nF - 1, -1, -1):
        if active[j]:
            left = pad + 1
        if left > 0:
            speech[j] = True
            left -= 1
    # the state machine over frames: out is a list of ("copy", frame) / ("fade", frame, partner)
    out = []
    rec = dict(lead=0, tail=0, runs=0, inner=0)
    seen_speech = False
    run = []                                        # the quiet frames of the run being collected

    def close(run, followed):
        R = len(run)
        if R == 0:
            return
        if not seen_speech and not followed:        # the whole segment is quiet
            keep = max(1, lead + tail)
            out.extend(("copy", j) for j in run[:keep])
            rec["tail"] += max(0, R - keep)
        elif not seen_speech:                       # leading
            keep = min(R, lead)
            out.extend(("copy", j) for j in run[R - keep:])
            rec["lead"] += R - keep
        elif not followed:                          # trailing
            keep = min(R, tail)
            out.extend(("copy", j) for j in run[:keep])
            rec["tail"] += R - keep
        elif R <= P:
            out.extend(("copy", j) for j in run)
        else:
            h = (P + 1) // 2
            t = P - h
            out.extend(("copy", j) for j in run[:h - 1])
            out.append(("fade", run[h - 1], run[R - t - 1]))
            out.extend(("copy", j) for j in run[R - t:])
            rec["runs"] += 1
            rec["inner"] += R - P

    for j in range(nF):
        if speech[j]:
            close(run, True)
            run = []
            seen_speech = True
            out.append(("copy", j))
        else:
            run.append(j)
    close(run, False)
    w_in = np.array([np.float32(0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / F)) for i in range(F)], dtype=np.float32)
    parts = []
    for item in out:
        a = item[1]
        if item[0] == "copy":
            parts.append(x[a * F: min((a + 1) * F, n)])
        else:
            b = item[2]
            fr = np.empty(F, dtype=np.float32)
            for i in range(F):
                fr[i] = np.float32(np.float32(w_in[F - 1 - i] * x[a * F + i]) + np.float32(w_in[i] * x[b * F + i]))
            parts.append(fr)
    y = np.concatenate(parts).astype(np.float32, copy=False)
    return y, [nF, sum(active), sum(speech), rec["lead"], rec["tail"], rec["runs"], rec["inner"], len(y)]


def passthrough(x, fs):
    n, F = len(x), fs // 100
    return np.array(x, dtype=np.float32), [(n + F - 1) // F, 0, 0, 0, 0, 0, 0, n]

"""The streamed window decode against its characterisation trace (tests/golden/windows_trace.json, written by
oracle/make_windows_trace.py at the commit before `decode_windows` came to parse its lists once): for every call of the table the same
library entry with the same host tables, the same stream steps with the same pushes in the same order, the same conversions, companding
ranges and copies -- no launch, upload or device-to-host copy more or fewer on any path -- and for every refused call the same
exception, word for word, before anything has run.  No GPU: the recorder is a CodecEngine whose library, steps, conversions and copies
only leave a record."""
import itertools
import json

import pytest

from oracle import make_windows_trace as M

with open(M.GOLDEN) as f:
    GOLD = M.unpack(json.load(f))         # every distinct call is kept once; the cases refer to it
CASES = M.cases()


def test_the_table_is_the_recorded_one():
    assert [c[0] for c in CASES] == list(GOLD) and len(GOLD) == 147
    assert sum("error" in v for v in GOLD.values()) == 89
    # the accepted calls reach every entry and every step
    names = {c[0] for v in GOLD.values() if "error" not in v for c in v["trace"]}
    assert names == {"ctts_codec_decode_windows", "ctts_codec_decode_windows_rate", "ctts_codec_decode_windows_speed",
                     "ctts_codec_decode_windows_speed_rate", "trim_pauses_stream_step", "compress_stream_step", "peak_limit_stream_step",
                     "flac_stream_step", "adpcm_stream_step", "float_to_int16_ragged", "g711_encode", "to_host"}


def test_every_pair_of_option_values_is_in_the_array():
    rows = M.covering(M.VALUES, seed=2)
    for a, b in itertools.combinations(M.VALUES, 2):
        for va, vb in itertools.product(M.VALUES[a], M.VALUES[b]):
            assert any(row[a] == va and row[b] == vb for row in rows), (a, va, b, vb)


@pytest.mark.parametrize("entry", ["cross", "pcm16", "ok", "x"])
def test_replay(entry):
    ran = 0
    for cid, call in CASES:
        if cid.replace("#", ".").split(".")[0] != entry:
            continue
        got = json.loads(json.dumps(M.run(call)))
        want = GOLD[cid]
        if "error" in want:
            assert got.get("error") == want["error"], (cid, got)
            assert got["trace"] == [], (cid, got["trace"])              # refused before anything has run
        else:
            assert "error" not in got, (cid, got["error"])
            assert got["trace"] == want["trace"] and got["result"] == want["result"], cid
        ran += 1
    assert ran


def test_the_batcher_opens_closes_and_forwards_what_it_did():
    """two polls of `SpeechBatcher._serve_chunks` over four jobs with different option mixes and one with none: per job the opens of its
    streams in their order and with their arguments, per poll the keywords `decode_windows_pcm16` receives (absent when off), per job
    its closes, and every count"""
    with open(M.GOLDEN) as f:
        want = json.load(f)["serve"]
    got = json.loads(json.dumps(M.serve_trace()))
    assert got["opens"] == want["opens"] and got["closes"] == want["closes"] and got["counts"] == want["counts"]
    assert len(got["calls"]) == len(want["calls"]) == 2
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w, (g, w)
    assert "adpcm" not in want["calls"][0]["kw"] and want["closes"]["E"] == [] and "E" not in want["opens"]

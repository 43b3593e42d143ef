"""The decode calls' output options against the characterisation trace (tests/golden/outchain_trace.json, written by
oracle/make_outchain_trace.py at the commit before the stages got one plan and one chain): for every call of the table the same
stage calls with the same arguments in the same order -- no launch, copy, allocation or device-to-host read more or fewer on any
path -- and for every refused call the same exception, word for word, before anything has run.  No GPU: the recorder is a
CodecEngine whose decodes, stages, conversions and copies only leave a record."""
import json

import pytest

from oracle import make_outchain_trace as M

with open(M.GOLDEN) as f:
    GOLD = M.unpack(json.load(f))         # every distinct call is kept once; the cases refer to it
CASES = M.cases()


def test_the_table_is_the_recorded_one():
    assert [c[0] for c in CASES] == list(GOLD) and len(GOLD) == 533
    assert sum("error" in v for v in GOLD.values()) == 51


def test_every_pair_of_option_values_is_in_the_arrays():
    import itertools
    for array, values in ((M.FULL, M.VALUES), (M.ONE, {k: [v for v in vs if k not in ("sample_rate", "speed") or not isinstance(v, list)]
                                                      for k, vs in M.VALUES.items()})):
        for a, b in itertools.combinations(values, 2):
            for va, vb in itertools.product(values[a], values[b]):
                assert any(row[a] == va and row[b] == vb and type(row[a]) is type(va) and type(row[b]) is type(vb) for row in array), (a, va, b, vb)


@pytest.mark.parametrize("entry", sorted({c[0].split("#")[0] for c in CASES if "#" in c[0]}) + ["singles"])
def test_replay(entry):
    ran = 0
    for cid, who, call in CASES:
        if (cid.split("#")[0] if "#" in cid else "singles") != entry:
            continue
        got = json.loads(json.dumps(M.run(who, call)))
        want = GOLD[cid]
        if "error" in want:
            assert got.get("error") == want["error"], (cid, got)
            # every refusal, before anything runs: the options may have crossed the seam to the engine's decode call ("call."
            # records what arrived there), which refuses under its own name -- but no decode, stage, conversion or copy has run
            assert [c for c in got["trace"] if not c[0].startswith("call.")] == [], (cid, got["trace"])
        else:
            assert "error" not in got, (cid, got["error"])
            assert got["trace"] == want["trace"] and got["result"] == want["result"], cid
        ran += 1
    assert ran

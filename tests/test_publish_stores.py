"""The decode step's results leave through write-through stores ("results published write-through"): same values,
same addresses, only the cache policy differs -- so every bit the PARENT of that change produced must still be produced.

tests/golden/publish_parent.npz was written by tools/make_publish_golden.py on the parent commit's library: the 2-layer synthetic
model, prompts of 3-5 tokens, 10 decode steps, 1 / 16 / 17 / 64 utterances (the projections' 16-row tile edges), one utterance forced
to finish at step 3 (compaction moves rows), seeded sampling, all three arithmetics.  Stored: the token ids, and per utterance a digest
of its captured hidden rows, its row of the last step's logits and its layer-1 K / V rows (+ the certificate's margins).  This runs the
same cases on the tree's library, eagerly and on the captured 8-step graph, and requires np.array_equal on every array."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_publish_golden", os.path.join(ROOT, "tools", "make_publish_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(G.GOLDEN))


def test_golden_covers_every_case(parent):
    assert os.path.getsize(G.GOLDEN) < 200 * 1024
    for dtype in G.DTYPES:
        for B in G.BATCHES:
            for arr in ("ids", "n_gen", "hidden", "logits", "k1", "v1"):
                assert f"{dtype}/B{B}/{arr}" in parent
            # the workload does what it is there for: the forced finish leaves rows to compact, the others run all ten steps
            n_gen = parent[f"{dtype}/B{B}/n_gen"]
            assert int(n_gen.max()) == G.STEPS
            if B > 1:
                assert int(n_gen[G.FINISH_ROW]) <= G.FINISH_AT < int(n_gen[G.FINISH_ROW + 1:].max())


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", G.DTYPES)
def test_every_bit_of_the_parent(parent, dtype, use_graph):
    eng = G.make_engine(dtype, torch.device("cuda:0"))
    for B in G.BATCHES:
        got = G.run_case(eng, B, use_graph)
        want = {k.split("/")[2]: v for k, v in parent.items() if k.startswith(f"{dtype}/B{B}/")}
        assert sorted(got) == sorted(want), (dtype, B)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (dtype, B, "eager" if not use_graph else "graph", k,
                                                                                       np.argwhere(got[k] != want[k])[:4].tolist())

"""The compressor stream step inside its declared scratch (ctts_compress_stream_scratch_bytes), on guarded, poisoned memory: the contract
of tests/test_gpu_workspace_contract.py for the new entry.  A buffer is handed out through `engine.device_scratch`, its guards stay intact,
and the chunks and records are bit-identical for every payload pattern and to a plain run.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import compressor as CP  # noqa: E402
from tests.test_gpu_workspace_contract import _codec, _pack, _stage_contract  # noqa: E402


@pytest.fixture()
def stage_codec(weights):
    return _codec(weights, "f32")


def test_stage_compress_stream_step(monkeypatch, stage_codec):
    """three streams stepped together, three times: signals of 1, tile - 1 and tile + 1 samples (a sample tile of 128 blocks at 24 kHz),
    cut so that the second step reads the raw carry and the history and the third is the last (for the 1-sample stream an empty one)"""
    x, off = _pack(CP.TILE_BLOCKS * 24, 7)
    lens = [int(off[i + 1] - off[i]) for i in range(3)]
    cuts = [[min(n, 1000), max(0, min(n - 1000, 1500)), max(0, n - 2500)] for n in lens]

    def call():
        hs = [stage_codec.compress_stream_open(24000, True) for _ in range(3)]
        try:
            out, at = [], [int(off[i]) for i in range(3)]
            for k in range(3):
                y, o = stage_codec.compress_stream_step(x, [(h, at[i], cuts[i][k], k == 2) for i, h in enumerate(hs)])
                at = [a + cuts[i][k] for i, a in enumerate(at)]
                out += [y, o]
            return out + [np.stack([stage_codec.compress_stream_stats(h) for h in hs])]
        finally:
            for h in hs:
                stage_codec.compress_stream_close(h)

    got = _stage_contract(monkeypatch, call, "compress_stream_step", min_takes=3)
    xh = x.cpu().numpy()
    for i in range(3):
        want, rec = CP.compress_segment(xh[off[i]: off[i + 1]], 24000, True)
        chunks = [got[2 * k][int(got[2 * k + 1][i]): int(got[2 * k + 1][i + 1])].cpu().numpy() for k in range(3)]
        assert np.concatenate(chunks).tobytes() == want.tobytes() and got[6][i].tobytes() == rec.tobytes(), i
    assert int(got[6]["n_blocks"].sum()) > 0

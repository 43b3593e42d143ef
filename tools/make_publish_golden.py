"""Pins the decode step's bits across the change of its stores' cache policy ("results published write-through").

`python tools/make_publish_golden.py [OUT.npz]` writes tests/golden/publish_parent.npz (or OUT.npz) from whatever library is loaded -- run it on the PARENT of
the change (a worktree of the parent commit, or CTTS_LIB pointing at the parent's libchattts_amd.so); tests/test_publish_stores.py
imports `workload` / `run_case` from here, runs the same cases on the tree's own library and requires np.array_equal on every array.

Workload: the 2-layer synthetic model, prompts of 3-5 tokens (left-padded), 10 decode steps, seeded sampling, batches of 1, 16, 17 and
64 utterances -- the row-tile edges of the projections (16-row tiles; 17 leaves a tile of one row; 64 fills the four tiles of a 64-row
workgroup).  In the batches of more than one utterance, utterance 1 is forced to finish at step 3, so that from step 4 on the device-side
compaction moves every later utterance up by one row.  All three arithmetics ("bf16", "f32x3", "f32"); every case runs eagerly and on
the captured 8-step graph, and both must give the stored arrays.

Stored per case: the token ids in full (int16), and one 16-byte sha256 prefix PER UTTERANCE of the bytes of (a) its captured hidden rows,
(b) its row of the logits buffer as the last step left it, (c) / (d) its K / V rows of layer 1 (the slots of valid prompt tokens and of decode steps
that were written) -- the arrays themselves (1.9 MB of hidden rows at 64 utterances alone) would not fit a committed fixture; a digest row that
differs names the utterance and the array.  The certificate's margins are stored as they are where the engine certifies."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chattts_amd import engine as E, synth, weights as W  # noqa: E402
from chattts_amd.config import GPT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "publish_parent.npz")
DTYPES = ("bf16", "f32x3", "f32")
BATCHES = (1, 16, 17, 64)
STEPS = 10
FINISH_AT, FINISH_ROW = 3, 1


def make_engine(dtype, dev):
    return E.GptEngine(W.synthetic_gpt(n_layers=2), W.synthetic_embed(), dev, dtype=dtype, exact_fallback=False)


def _digest(t: torch.Tensor) -> np.ndarray:
    raw = t.contiguous().cpu().view(torch.uint8).numpy().tobytes()   # (the bytes: a bf16 KV cache has no numpy dtype)
    return np.frombuffer(hashlib.sha256(raw).digest()[:16], dtype=np.uint8)


def _logits_offset(B: int) -> int:
    """byte offset of the logits rows in the decode step's workspace (csrc/capi.hip carve(base, B, 1): x, qkv, ao, act, hfin in front)"""
    al = lambda n: (n + 255) & ~255
    return al(B * GPT.hidden * 4) + al(B * 3 * GPT.hidden * 4) + al(B * GPT.hidden * 4) + al(B * GPT.inter * 4) + al(B * GPT.hidden * 4)


def run_case(eng, B: int, use_graph: bool) -> dict:
    ids, mask, tmask = synth.make_prompts(B, 3, 5, seed=5 + B)
    T = ids.shape[1]
    warpers, procs = E.gen_logits(GPT.n_audio - 1, 0.7, 20, 1.05)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    stop = torch.full((B,), STEPS, dtype=torch.int32)
    if B > 1:
        stop[FINISH_ROW] = FINISH_AT
    emb = eng.embed_prompt(ids_t, torch.from_numpy(tmask))
    out = list(eng.generate(emb, ids_t, torch.tensor([0.3] * GPT.n_vq), GPT.n_audio - 1, mask_t, STEPS, 0, (*procs, *warpers),
                            return_hidden=True, manual_seed=11, use_graph=use_graph, stop_at=stop, lanes=1))[-1]
    torch.cuda.synchronize()
    ln = eng._session["lanes"][0]
    n_gen = [int(r.shape[0]) for r in out.ids]
    tok = np.full((B, STEPS, GPT.n_vq), -1, dtype=np.int16)
    for b, r in enumerate(out.ids):
        tok[b, :n_gen[b]] = r.cpu().numpy().astype(np.int16)
    pad = (T - mask.sum(axis=1)).astype(int).tolist()   # left padding of every prompt
    off = _logits_offset(B)
    logits = ln.workspace[off: off + B * GPT.n_vq * GPT.n_audio * 4].view(torch.float32).reshape(B, GPT.n_vq * GPT.n_audio)
    res = {"ids": tok, "n_gen": np.asarray(n_gen, dtype=np.int16),
           "hidden": np.stack([_digest(h) for h in out.hiddens]),
           "logits": np.stack([_digest(logits[m]) for m in range(B)]),
           # K / V of the layer-1 slots that were written: the valid prompt tokens' (the f32x3 prompt pass skips the left padding) and one
           # per embedded token (the last sampled token never is)
           "k1": np.stack([_digest(ln.kcache[1, b, :, pad[b]:T + max(n_gen[b], 1) - 1]) for b in range(B)]),
           "v1": np.stack([_digest(ln.vcache[1, b, :, pad[b]:T + max(n_gen[b], 1) - 1]) for b in range(B)])}
    if eng.certify:   # the parity certificate's per-utterance minimum margins (written by the sampler step by step)
        res["margin"] = np.asarray(eng.last_margins, dtype=np.float32).reshape(-1)
    return res


def workload(dev, use_graph: bool) -> dict:
    """every case of one launch mode: {"<dtype>/B<batch>/<array>": ndarray}"""
    out = {}
    for dtype in DTYPES:
        eng = make_engine(dtype, dev)
        for B in BATCHES:
            for k, v in run_case(eng, B, use_graph).items():
                out[f"{dtype}/B{B}/{k}"] = v
        del eng
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    eager, graph = workload(dev, False), workload(dev, True)
    bad = [k for k in eager if not np.array_equal(eager[k], graph[k])]
    assert not bad, ("eager and graph disagree on the library that writes the golden", bad)
    dst = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    np.savez_compressed(dst, **eager)
    print(f"{dst}: {len(eager)} arrays, {os.path.getsize(dst)} bytes")

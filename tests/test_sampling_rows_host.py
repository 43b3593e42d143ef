"""CPU tests of per-request sampling: the C ABI of the per-slot sampling table (ctts_sampling_row, ctts_gen_state.row_sampling), the
host packing of a request's parameters into it, and the serving batcher's routing / error isolation / lock discipline on fakes."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest
import torch

from chattts_amd import _lib, rng
from chattts_amd.serving import SpeechBatcher, request_params, sampling_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampling_row_and_gen_state_match_the_header_layout(tmp_path):
    """sizeof and every field offset of ctts_sampling_row and of the extended ctts_gen_state as gcc lays out include/chattts_amd.h ==
    what chattts_amd/_lib.py tells ctypes; row_sampling is the LAST field of ctts_gen_state and the row is 128 bytes"""
    pairs = [("ctts_sampling_row", _lib.SamplingRow), ("ctts_gen_state", _lib.GenState)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "chattts_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("%zu\\n", sizeof({cname}));')
        for fname, *_ in cls._fields_:
            lines.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, cls in pairs:
        want.append(C.sizeof(cls))
        want += [getattr(cls, fname).offset for fname, *_ in cls._fields_]
    assert got == want
    assert C.sizeof(_lib.SamplingRow) == 128
    assert _lib.GenState._fields_[-1][0] == "row_sampling"


def test_sampling_row_packing():
    p = request_params(dict(temperature=[0.05, 0.3, 0.7, 1.5], top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=7,
                            manual_seed=5))
    r = sampling_row(p, rng_seed=2 ** 63 + 5, rng_per_step=True)
    assert list(r.temperature) == [float(np.float32(t)) for t in (0.05, 0.3, 0.7, 1.5)]
    thr = np.float32(1.0 - 0.7)                    # `cum <= 1 - top_p` on a float32 tensor: the scalar rounded to float32 once
    assert np.float32(r.top_p_thr) == thr and r.top_p_thr == float(thr) and r.use_top_p == 1
    assert (r.top_k, r.use_top_k, r.min_new, r.use_penalty) == (20, 1, 7, 1)
    assert np.array_equal(np.array(list(r.pow_table), np.float32), rng.penalty_table(1.05).numpy())
    assert (r.rng_seed, r.rng_per_step) == (2 ** 63 + 5, 1)
    # None -> use flags 0; penalty 1 creates no processor (processors.py:52) -> no table; a scalar temperature covers the 4 codebooks
    p = request_params(dict(temperature=0.3, top_P=None, top_K=None, repetition_penalty=1.0))
    r = sampling_row(p)
    assert (r.use_top_p, r.use_top_k, r.use_penalty, r.top_k, r.top_p_thr, r.rng_per_step) == (0, 0, 0, 0, 0.0, 0)
    assert list(r.pow_table) == [0.0] * 17 and list(r.temperature) == [float(np.float32(0.3))] * 4
    # the defaults are InferCodeParams' (core.py:48-64)
    from chattts_amd.core import InferCodeParams
    d = request_params(None)
    assert d == request_params(InferCodeParams())
    assert (d.temperature, d.plan.top_p, d.plan.top_k, d.plan.penalty, d.manual_seed) == ((0.3,) * 4, 0.7, 20, 1.05, None)


def test_request_params_refuse_what_generate_refuses():
    with pytest.raises(ValueError):
        request_params(dict(temperature=[0.3, 0.3]))
    # a penalty processor is validated like GptEngine.generate's (gen_logits -> plan_from_processors): any value builds a plan ...
    assert request_params(dict(repetition_penalty=0.9)).plan.penalty == 0.9
    # ... and the plan is the one generate derives for the same arguments
    from chattts_amd.engine import gen_logits, plan_from_processors
    w, p = gen_logits(625, 0.5, 3, 2.0)
    assert request_params(dict(top_P=0.5, top_K=3, repetition_penalty=2.0)).plan == plan_from_processors((*p, *w))


# ---- SpeechBatcher on fakes -----------------------------------------------------------------------------------------------
class _Params:
    def __init__(self, spk, max_new_token=32):
        self.spk_emb, self.max_new_token = spk, max_new_token


class _Tok:
    spk_emb_ids = 7


class _FakeChat:
    """prompt = the text's bytes; the decoded waveform of a request = its token ids, as floats; "boom" fails at tokenisation,
    "crash" fails at decode"""
    tokenizer = _Tok()

    def __init__(self):
        self.norm_calls = []

    def normalizer(self, text, norm, homophones, lang):
        self.norm_calls.append((text, norm, homophones, lang))
        return text

    def code_prompt(self, texts, params):
        if texts[0] == "boom":
            raise ValueError("cannot tokenise boom")
        t = np.frombuffer(texts[0].encode(), dtype=np.uint8).astype(np.int64)
        ids = torch.from_numpy(np.repeat(t[None, :, None], 4, axis=2))
        return ids, torch.ones(ids.shape[:2], dtype=torch.bool), torch.ones(ids.shape[:2], dtype=torch.bool)

    def prompt_embedding(self, ids, tmask, params, spk_emb_ids):
        assert spk_emb_ids == 7
        return ids[..., :1].float().expand(*ids.shape[:2], 768).clone()

    def decode_to_wavs(self, hids):
        h = hids[0]
        if float(h[0, 0]) == float(ord("c")) and h.shape[0] == len("crash"):
            raise RuntimeError("decoder failed")
        return np.stack([h[:, 0].numpy().astype(np.float32) / 256.0])


class _FakePool:
    """a pool of S slots that 'generates' the prompt itself, one token per chunk of `between` calls"""

    def __init__(self, S, lock, chunk_log):
        self.S, self.lock, self.log = S, lock, chunk_log
        self.queue, self.active, self.free = [], {}, list(range(S))
        self.submitted = []

    def submit(self, rid, ids, tmask, max_new_token, *, params, emb):
        assert ids.shape[1] == 4 and emb.shape == (ids.shape[0], 768)
        self.submitted.append((rid, params.spk_emb))
        self.queue.append((rid, ids, emb))

    def run(self, between=None):
        while self.queue or self.active:
            if between is not None:
                between()
            assert self.lock.locked()                   # every chunk runs with the GPU lock held
            self.log.append(threading.current_thread().name)
            while self.queue and self.free:
                rid, ids, emb = self.queue.pop(0)
                self.active[self.free.pop(0)] = [rid, ids, emb, 0]
            time.sleep(0.002)
            for s, a in list(self.active.items()):
                a[3] += 1
                if a[3] >= 3:
                    del self.active[s]
                    self.free.append(s)
                    yield a[0], a[1], a[2]


def test_batcher_routes_results_isolates_errors_and_shares_the_lock():
    lock = threading.Lock()
    chunks = []
    holder = {}
    b = SpeechBatcher(_FakeChat(), 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock, chunks)))
    texts = ["alpha", "boom", "bravo charlie", "crash", "delta", "echo", "foxtrot golf"]
    try:
        futs = [(t, b.submit(t, _Params("spk-" + t))) for t in texts]
        # another GPU user (a streamed request) gets the lock between chunks while the pool is busy
        got_lock = []

        def streamer():
            for _ in range(5):
                with lock:
                    got_lock.append(len(chunks))
                time.sleep(0.001)
        th = threading.Thread(target=streamer)
        th.start()
        for t, f in futs:
            if t in ("boom", "crash"):
                with pytest.raises((ValueError, RuntimeError)):
                    f.result(timeout=30)
                continue
            pcm = f.result(timeout=30)
            from chattts_amd.audio import float_to_int16
            w = np.frombuffer(t.encode(), dtype=np.uint8).astype(np.float32) / 256.0
            assert np.array_equal(pcm, float_to_int16(w[np.abs(w) > np.float32(1e-5)])), t     # routed to ITS request
        th.join(timeout=30)
        assert len(got_lock) == 5
        # the worker is still serving after both failures
        assert np.asarray(b.submit("zulu", _Params("z")).result(timeout=30)).size == 4
        occ = b.occupancy()
        assert occ["failed"] == 2 and occ["completed"] == 6 and occ["admissions"] == 7
        assert 2 <= occ["max_coresident"] <= 3
        assert set(chunks) == {"speech-batcher"}                   # only the worker ran pool chunks
        assert [r[1] for r in holder["p"].submitted] == ["spk-" + t for t in texts if t != "boom"] + ["z"]
    finally:
        b.close()
    assert not lock.locked()

"""Continuous batching over a pool of utterance slots.

The reference's default path generates one fixed batch to completion (`GPT.generate`, gpt.py:316-618; rows that
finish early idle until the last one is done, :592); only its optional vLLM fork schedules requests continuously
(/root/reference/ChatTTS/model/velocity/scheduler.py:130-293, block_manager.py:73-296).  `SlotPool` is the
MI355X-native equivalent for this engine: a fixed pool of S utterance slots with a dense KV cache per slot
(288 GB of HBM make paging unnecessary: 64 slots x 2560 positions x 61 KB = 10 GB), ONE captured decode graph
for the whole session, and device-side state that makes admission / retirement free of re-capture: the `finish` flags
(a free or retired slot looks finished; the first kernel of every decode step ranks the unfinished slots and computes exactly
those -- device-side compaction, include/chattts_amd.h) and `prompt_len` (where each slot's generated part starts).  Admission
is: write the slot's state, clear its flag.  Newly admitted requests are prefilled as a group straight into their slots' KV cache.

Parity contract: a request produces exactly the tokens `GptEngine.generate` produces for it alone with
`row_offset = 4*slot, total_rows = 4*S` (the Exp(1) draw of a sampling row is the pool row's), because nothing
in the step mixes utterances.  With the host generator, seeded sampling only (`manual_seed`: the reference re-seeds its CPU
generator every step, so the draw is one constant tensor for the whole session); `rng="device"` serves unseeded sampling too.

Per-request sampling parameters (`SlotPool(..., per_request=True)`): every request carries its own `InferCodeParams` sampling fields
and seed (the role of the reference's per-request `SamplingParams` in its vLLM engine, velocity/sampling_params.py:24), written into
the slot's entry of the sampling kernel's per-slot table (include/chattts_amd.h, ctts_sampling_row) at admission, with its own Exp(1)
rows and its own global sampling row.  Contract there: a request yields the tokens `GptEngine.generate` yields for it ALONE with the same
parameters, `row_offset` and `total_rows` -- whatever runs beside it and whichever slot it lands in.
"""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
import itertools
import queue
import threading
import time
from collections import deque
from concurrent.futures import Future
from dataclasses import dataclass, field
from typing import Deque, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from . import adpcm as ADPCM
from . import flac as FLAC
from . import g711 as G711
from . import loudness as LN
from . import limiter as LM
from . import compressor as CP
from . import equalizer as EQ
from . import pauses as PA
from . import resample as RS
from . import timescale as TS
from ._sync import wait_event, wait_stream
from .config import GPT
from .engine import GptEngine, gen_logits, plan_from_processors
from .outchain import option_kw
from .winchain import STAGES, StreamSet
from .rng import ExpDraws, penalty_table


@dataclass
class _Req:
    rid: object
    ids: torch.Tensor        # [T, 4] int64
    tmask: torch.Tensor      # [T] bool
    max_new: int
    stop_at: int             # -1: none (benchmark hook, see engine.generate)
    params: Optional["RequestParams"] = None   # per_request pools only
    row_offset: int = 0
    total_rows: int = GPT.n_vq
    emb: Optional[torch.Tensor] = None         # [T, 768] prompt embedding (speaker applied), or None: embedded at admission
    stream: Optional["StreamSpec"] = None      # a streamed request: its chunk schedule (run(events=True))
    cursor: Optional["StreamCursor"] = None    # where that schedule stands (fresh at every admission)
    cancelled: bool = False                    # cancel(rid): retired at the next poll, nothing is handed out


# InferCodeParams' sampling fields and their defaults (core.py:48-64)
_PARAM_DEFAULTS = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=None,
                       ensure_non_empty=True)


# RefineTextParams' sampling fields and their defaults (core.py:33-44)
_TEXT_PARAM_DEFAULTS = dict(temperature=0.7, top_P=0.7, top_K=20, repetition_penalty=1.0, min_new_token=0, manual_seed=None,
                            ensure_non_empty=True)


@dataclass
class RequestParams:
    """the sampling parameters of one pooled request, validated: `temperature` has one entry per codebook (text mode: one entry)"""
    temperature: Tuple[float, ...]
    plan: object             # engine.SamplingPlan
    min_new_token: int
    manual_seed: Optional[int]
    ensure_non_empty: bool
    infer_text: bool = False


def request_params(params=None, infer_text: bool = False, num_code: int = GPT.n_text) -> RequestParams:
    """`params`: an `InferCodeParams`, a dict of its fields, or None (the defaults).  Validated the way `GptEngine.generate` validates
    them (gen_logits -> plan_from_processors), so a pool refuses exactly what a plain call refuses.
    `infer_text=True`: `params` is a `RefineTextParams` (or a dict of its fields) -- ONE temperature (the text mode has one sampling row per
    utterance, core.py refine_text_ids), `gen_logits(num_code, ...)`, `plan_from_processors(..., infer_text=True)`: a text pool refuses
    what `Chat.refine_text_ids` refuses (a repetition penalty other than 1 above all)."""
    defaults, n_temp, wrong, codes = ((_TEXT_PARAM_DEFAULTS, 1, "refine-text mode takes one temperature (a scalar)", int(num_code)) if infer_text else
                                      (_PARAM_DEFAULTS, GPT.n_vq, "temperature must be a scalar or one value per codebook", GPT.n_audio - 1))
    get = (lambda k: params.get(k, defaults[k])) if isinstance(params, dict) else (lambda k: getattr(params, k, defaults[k]))
    t = get("temperature")
    temp = tuple(float(x) for x in t) if isinstance(t, (list, tuple)) else (float(t),) * n_temp   # core.py:558-561
    if len(temp) != n_temp:
        raise ValueError(wrong)
    warpers, procs = gen_logits(codes, get("top_P"), get("top_K"), get("repetition_penalty"))
    plan = plan_from_processors((*procs, *warpers), infer_text=bool(infer_text))
    seed = get("manual_seed")
    return RequestParams(temp, plan, int(get("min_new_token")), None if seed is None else int(seed), bool(get("ensure_non_empty")), bool(infer_text))


def sampling_row(p: RequestParams, rng_seed: int = 0, rng_per_step: bool = False) -> _lib.SamplingRow:
    """the ctts_sampling_row of one request: the values `GptEngine.generate` puts into the call-wide fields for the same parameters"""
    if p.infer_text and p.plan.penalty is not None:     # (the sampling kernel's text mode never reads use_penalty / pow_table)
        raise NotImplementedError("refine-text mode supports repetition_penalty = 1.0 only (reference default)")
    r = _lib.SamplingRow()
    for i, t in enumerate(p.temperature):
        r.temperature[i] = float(np.float32(t))
    ptab = penalty_table(p.plan.penalty)
    r.use_penalty = int(ptab is not None)
    if ptab is not None:
        for i, v in enumerate(ptab.tolist()):
            r.pow_table[i] = v
    r.top_p_thr = float(np.float32(1.0 - p.plan.top_p)) if p.plan.top_p is not None else 0.0
    r.use_top_p = int(p.plan.top_p is not None)
    r.top_k, r.use_top_k = int(p.plan.top_k or 0), int(p.plan.top_k is not None)
    r.min_new = int(p.min_new_token)
    r.rng_seed = int(rng_seed) & (2 ** 64 - 1)
    r.rng_per_step = int(bool(rng_per_step))
    return r


@dataclass
class StreamSpec:
    """the streaming fields of a request's `InferCodeParams` (core.py:62-64)"""
    stream_batch: int = 24
    stream_speed: int = 12000
    pass_first_n_batches: int = 2


class StreamCursor:
    """The chunk schedule of ONE streamed request, advanced by the token counts a pool reads at its polls.  It is the schedule
    `GptEngine.generate(stream=True)` + the `stream` branch of `Chat._infer` produce for the request run alone as a batch of one:
      * a yield at every multiple of `stream_batch` tokens the request reaches (generate yields there while the row is live), the
        reference's duplicate yield when the row ends by EOS exactly on such a multiple (engine.py, "stream_iter quirk"), and
        generate's final result, which passes through the same loop of `_infer`;
      * the first `pass_first_n_batches` yields are dropped; every other one emits samples [length, length + stream_speed) of the
        decode of the prefix of exactly that many tokens, clipped to its 256 (2 n - 1) samples, and moves `length` to the clipped end;
      * the tail: everything from `length` to the end of the full decode.
    Every method returns the chunks that became due, in order: (prefix_tokens, s_lo, s_hi, is_tail).  A chunk may be empty
    (s_lo == s_hi): the serial path yields an empty array there."""

    def __init__(self, spec: StreamSpec):
        if int(spec.stream_batch) < 1 or int(spec.stream_speed) < 0:
            raise ValueError("stream_batch must be positive, stream_speed non-negative")
        self.spec = spec
        self.boundary = int(spec.stream_batch)     # the next token count at which a live request yields
        self.yields = 0
        self.length = 0                            # samples emitted so far

    def _yield(self, prefix: int, out: list) -> None:
        self.yields += 1
        if self.yields <= int(self.spec.pass_first_n_batches):
            return
        s_hi = max(self.length, min(self.length + int(self.spec.stream_speed), 256 * (2 * prefix - 1)))
        out.append((prefix, self.length, s_hi, False))
        self.length = s_hi

    def advance(self, count: int) -> list:
        """the request is live and holds `count` tokens"""
        out: list = []
        while self.boundary <= count:
            self._yield(self.boundary, out)
            self.boundary += int(self.spec.stream_batch)
        return out

    def finish(self, n: int, eos: bool) -> list:
        """the request ended with `n` tokens; `eos`: by its finish flag (EOS), not by max_new_token"""
        if n <= 0:
            return []                              # step 0 drew EOS: no audio, no chunks
        out = self.advance(n)
        if eos and n % int(self.spec.stream_batch) == 0:
            self._yield(n, out)                    # the duplicate yield
        self._yield(n, out)                        # generate's final result
        out.append((n, self.length, 256 * (2 * n - 1), True))
        return out


def stream_schedule(counts, n: int, eos: bool, spec: StreamSpec) -> list:
    """Pure host function: the token counts a streamed request showed at successive polls while live (`counts`), then its end (`n`
    tokens, `eos`) -> every chunk of its stream, [(prefix_tokens, s_lo, s_hi, is_tail)].  The result does not depend on where the polls
    fell (a boundary passed between two polls is served at the later one, from the prefix of exactly that many tokens)."""
    cur = StreamCursor(spec)
    out: list = []
    for c in counts:
        out += cur.advance(min(int(c), int(n)))
    return out + cur.finish(int(n), bool(eos))


class StreamEvents:
    """what `SlotPool.run(events=True)` yields at a poll at which chunks of streamed requests became due: `chunks` = [(request id,
    slot, prefix_tokens, s_lo, s_hi, is_tail)].  The consumer decodes them from `pool.hiddens` BEFORE it resumes the generator (rows
    below a live slot's prefix are final; a finished slot is freed, and may be re-admitted, only after the generator resumes)."""

    def __init__(self, chunks: list):
        self.chunks = chunks


class SlotPool:
    POLL = 8   # decode steps between two looks at the finish flags (= admission / retirement granularity)

    def __init__(self, engine: GptEngine, slots: int = 64, cap: int = 1536, hid_cap: int = 1024, *, temperature=(0.3,) * 4,
                 top_P: Optional[float] = 0.7, top_K: Optional[int] = 20, repetition_penalty: float = 1.05, manual_seed: int = 42,
                 min_new_token: int = 0, eos_token: Optional[int] = None, rng: str = "host", rng_seed: Optional[int] = None,
                 per_request: bool = False, infer_text: bool = False):
        """`per_request=True`: the sampling keywords above are not used; every request brings its own (`submit(params=...)`), with
        the host generator each its own `manual_seed`; with the device generator seeded and unseeded requests share the pool (unseeded
        ones draw from `rng_seed` -- random if None -- with a fresh counter word per admission, `nonce_of[rid]`).
        `rng="device"`: the Exp(1) draws come from the sampling kernel's own generator (engine.generate's `rng`), which is what
        makes the reference's DEFAULT `manual_seed=None` servable here: a fresh draw per (admission, request step, pool row) without any
        per-step host work -- every admission gets its own number as the fourth word of the generator's counter, so a request never
        replays the stream of the slot's previous occupant (`nonce_of[rid]`; `generate(rng_nonce=...)` reproduces it in isolation).  The host stream (`rng="host"`) needs `manual_seed` (one constant tensor per session)."""
        if rng not in ("host", "device"):
            raise ValueError("rng must be 'host' or 'device'")
        self.per_request = bool(per_request)
        # infer_text=True: a REFINE-TEXT pool (the generator in text mode, core.py refine_text_ids): prompts are [T, 4] text ids
        # (replicated), requests bring `RefineTextParams`-shaped parameters, a sampling row is ONE per utterance (`row_offset` /
        # `total_rows` count those), `eos_token` is the tokenizer's [Ebreak] and must be given, results are (rid, ids [n] int64, empty).
        # No hidden states are kept: `hid_cap` is not used (the store is the one row per slot the C side writes through its bound check).
        self.infer_text = bool(infer_text)
        if self.infer_text:
            if not self.per_request:
                raise ValueError("a text-mode pool is a per-request pool: SlotPool(per_request=True, infer_text=True)")
            if eos_token is None:
                raise ValueError("a text-mode pool needs eos_token (tokenizer.eos_token, [Ebreak])")
            hid_cap = 1
        eos_token = GPT.n_audio - 1 if eos_token is None else int(eos_token)
        self.nrow = 1 if self.infer_text else GPT.n_vq          # sampling rows per utterance (gpt.py:459-464 vs :439-440)
        self.V = GPT.n_text if self.infer_text else GPT.n_audio
        if manual_seed is None and rng != "device" and not self.per_request:
            raise NotImplementedError("SlotPool with the host generator needs manual_seed (one constant Exp(1) draw per session); "
                                      "use rng='device' for unseeded sampling")
        if cap > engine.max_pos:
            raise ValueError("slot capacity exceeds max_position_embeddings")
        self.eng, self.S, self.cap, self.hid_cap = engine, slots, cap, hid_cap
        self.lib = engine.lib
        dev = self.dev = engine.device
        if self.infer_text:
            plan = plan_from_processors(())       # (per request: the call-wide fields are not read)
        else:
            warpers, procs = gen_logits(GPT.n_audio - 1, top_P, top_K, repetition_penalty)
            plan = plan_from_processors((*procs, *warpers))
        h = C.c_void_p()
        _lib.check(self.lib.ctts_gpt_create(C.byref(h), C.byref(engine._w)), "ctts_gpt_create")
        self.handle = h
        self.st = torch.cuda.Stream(device=dev)
        nvq = GPT.n_vq
        with torch.cuda.stream(self.st):
            self.ids_buf = torch.zeros((slots, cap, nvq), dtype=torch.int64, device=dev)
            self.len = torch.ones((slots,), dtype=torch.int32, device=dev)
            self.kv_start = torch.zeros((slots,), dtype=torch.int32, device=dev)
            # finish flags + end_idx in one padded block: a poll is one shader copy of it into pinned memory (engine.snapshot)
            self._Sp = (slots + 15) // 16 * 16
            self.state_blk = torch.zeros((5 * self._Sp,), dtype=torch.uint8, device=dev)
            self.finish = self.state_blk[:slots]
            self.finish.fill_(1)                                                    # free slots look finished
            self.end_idx = self.state_blk[self._Sp:].view(torch.int32)[:slots]
            self.prompt_len = torch.ones((slots,), dtype=torch.int32, device=dev)
            self.stop_at = torch.full((slots,), -1, dtype=torch.int32, device=dev)
            self.hiddens = torch.empty((slots, hid_cap, GPT.hidden), dtype=torch.float32, device=dev)
            kv_shape = (engine.n_layers, slots, GPT.n_heads, cap, GPT.head_dim)
            self.kcache = torch.zeros(kv_shape, dtype=engine.wdt, device=dev)
            self.vcache = torch.zeros(kv_shape, dtype=engine.wdt, device=dev)
            self.n_active = torch.zeros((1,), dtype=torch.int32, device=dev)   # written by the step's first kernel
            self.device_rng, self.rng_per_step = rng == "device", manual_seed is None
            self.rows = self.row_base = None
            if self.per_request:
                # the per-slot sampling table and global sampling rows, written at admission (ctts_gen_state.row_sampling / row_base)
                self.rows = torch.zeros((slots, C.sizeof(_lib.SamplingRow)), dtype=torch.uint8, device=dev)
                self.row_base = torch.zeros((slots,), dtype=torch.int32, device=dev)
                self.q = (torch.zeros((1,), dtype=torch.float32, device=dev) if self.device_rng else
                          torch.ones((1, slots * self.nrow, self.V), dtype=torch.float32, device=dev))   # host: each slot's rows at admission
                self.rng_seed = None
                self.pool_seed = int(rng_seed) if rng_seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
                self.rng_nonce = torch.zeros((slots,), dtype=torch.int32, device=dev) if self.device_rng else None
            elif self.device_rng:
                self.q = torch.zeros((1,), dtype=torch.float32, device=dev)
                seed = int(rng_seed) if rng_seed is not None else (int(manual_seed) if manual_seed is not None
                                                                   else int(torch.randint(0, 2 ** 62, (1,)).item()))
                self.rng_seed = torch.tensor([seed], dtype=torch.int64, device=dev)
                # unseeded (manual_seed=None): a request's step index restarts at 0, so the Philox counter (token group, pool row, step)
                # alone would replay the previous occupant's stream in the same slot.  A per-slot admission number is the fourth counter
                # word (ctts_gen_state.rng_nonce): every (admission, step, row, token) draws fresh.  Seeded pools keep the constant word --
                # the reference re-seeds at every step there, the same draw for every request IS its semantics.
                self.rng_nonce = torch.zeros((slots,), dtype=torch.int32, device=dev) if manual_seed is None else None
            else:
                self.q = ExpDraws(slots * nvq, GPT.n_audio, manual_seed).step(0).to(dev).reshape(1, slots * nvq, GPT.n_audio).contiguous()
                self.rng_seed = None
                self.rng_nonce = None
            self.temp = None if self.per_request else torch.tensor(list(temperature), dtype=torch.float32, device=dev)
            ptab = None if self.per_request else penalty_table(plan.penalty)
            self.ptab = None if ptab is None else ptab.to(dev)
            ws_bytes = self.lib.ctts_gpt_workspace_bytes(slots, 1)
            self.ws = _engine.device_scratch(ws_bytes, dev)
        self.plan, self.min_new, self.eos = plan, int(min_new_token), int(eos_token)
        self.dec = self._state(B=slots, T=1, workspace=self.ws, row_map=None, n_active=self.n_active)
        self.st.synchronize()
        _lib.check(self.lib.ctts_gpt_graph_build(self.handle, C.byref(self.dec), self.st.cuda_stream), "ctts_gpt_graph_build")
        # a poll's target: two pinned blocks (state_blk's size) used in turn, each with the event behind its copy (_snapshot)
        self._snaps = [(torch.empty((5 * self._Sp,), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]
        self._snap_seq = 0                    # snapshots enqueued so far
        self._admit_no = 0                    # admissions numbered so far (rng_nonce)
        self._pending: Deque = deque()        # snapshots enqueued, not read yet (launch / poll)
        self._ready: Deque = deque()          # (event behind the result copies, results) of the previous poll
        self.free: List[int] = list(range(slots))
        self.active: dict = {}                 # slot -> (_Req, Tg, first snapshot sequence number that reflects this request)
        self.queue: Deque[_Req] = deque()
        self.steps = 0
        self.admissions = 0                   # prefill groups so far (bench.py reports it)
        self._keep = None
        self.slot_of: dict = {}               # request id -> slot it ran in (parity tests / tracing)
        self.nonce_of: dict = {}              # request id -> its admission number (device generator, unseeded: ctts_gen_state.rng_nonce)

    def close(self):
        if getattr(self, "handle", None):
            self.st.synchronize()
            self.lib.ctts_gpt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _state(self, B, T, workspace, row_map, n_active) -> _lib.GenState:
        s = _lib.GenState()
        s.B, s.T, s.max_new = B, T, self.cap - T
        s.ids_buf, s.len, s.kv_start = self.ids_buf.data_ptr(), self.len.data_ptr(), self.kv_start.data_ptr()
        s.finish, s.end_idx, s.hiddens = self.finish.data_ptr(), self.end_idx.data_ptr(), self.hiddens.data_ptr()
        s.kcache, s.vcache, s.q, s.nq = self.kcache.data_ptr(), self.vcache.data_ptr(), self.q.data_ptr(), 1
        s.temperature, s.pow_table = _lib.ptr(self.temp), _lib.ptr(self.ptab)
        p = self.plan
        s.top_p_thr = float(np.float32(1.0 - p.top_p)) if p.top_p is not None else 0.0
        s.use_top_p, s.top_k, s.use_top_k = int(p.top_p is not None), int(p.top_k or 0), int(p.top_k is not None)
        s.min_new, s.eos, s.row_offset = self.min_new, self.eos, 0
        s.stop_at = self.stop_at.data_ptr()
        s.workspace, s.workspace_bytes = workspace.data_ptr(), workspace.numel()
        s.row_map, s.n_active = _lib.ptr(row_map), _lib.ptr(n_active)
        s.cap, s.hid_cap, s.kv_batch, s.q_batch = self.cap, self.hid_cap, self.S, self.S
        s.prompt_len = self.prompt_len.data_ptr()
        s.infer_text = int(self.infer_text)
        s.rng_device, s.rng_per_step, s.rng_seed = int(self.device_rng), int(self.rng_per_step), _lib.ptr(self.rng_seed)
        s.rng_nonce = _lib.ptr(self.rng_nonce)
        if self.per_request:
            s.temperature, s.pow_table = None, None
            s.row_sampling, s.row_base = self.rows.data_ptr(), self.row_base.data_ptr()
        return s

    # -- request intake ---------------------------------------------------------------------------------------
    def submit(self, rid, input_ids, text_mask=None, max_new_token: int = 512, stop_at: int = -1, *, params=None, row_offset: int = 0,
               total_rows: Optional[int] = None, emb: Optional[torch.Tensor] = None, stream: Optional[StreamSpec] = None) -> None:
        """Queues one request.  Per-request pools only: `params` (an `InferCodeParams` or a dict of its sampling fields: temperature,
        top_P, top_K, repetition_penalty, min_new_token, manual_seed, ensure_non_empty), `row_offset` / `total_rows` (the request's
        sampling rows inside the batch whose tokens it must reproduce -- (0, 4): alone at batch 1, what `Chat.infer` does for one text),
        `emb` ([T, 768] prompt embedding with the speaker applied, `Chat.prompt_embedding`; None: the plain embedding of input_ids).
        The request then yields exactly the tokens `GptEngine.generate` yields for it alone with those arguments.  Step 0 follows
        generate's rule (gpt.py:527-570): a request whose first token is EOS yields no tokens (an empty result) -- unless it is unseeded
        with `ensure_non_empty`, then it is generated again with a fresh draw.
        `stream` (any pool): the request is streamed -- `run(events=True)` also yields its chunk events (StreamEvents).
        Text-mode pools: `input_ids` are [T, 4] text ids (replicated), `params` a `RefineTextParams` (or a dict of its sampling fields),
        `row_offset` / `total_rows` count one sampling row per utterance ((0, 1): alone at batch 1), the request yields the tokens
        `GptEngine.generate(infer_text=True)` yields for it alone; no `emb`, no `stream` (a text row has no audio)."""
        total_rows = self.nrow if total_rows is None else total_rows
        ids = torch.as_tensor(input_ids).to(torch.int64)
        assert ids.dim() == 2 and ids.shape[1] == GPT.n_vq
        tm = torch.ones(ids.shape[0], dtype=torch.bool) if text_mask is None else torch.as_tensor(text_mask).bool()
        # 2 * POLL positions of slack: a request that ends by max_new_token (no EOS) is retired by the HOST, up to two chunks late
        if ids.shape[0] + max_new_token + 1 + 2 * self.POLL > self.cap or (max_new_token > self.hid_cap and not self.infer_text):
            raise ValueError("request does not fit a slot (prompt + max_new_token + 2 * POLL vs cap, max_new_token vs hid_cap)")
        p = None
        if self.per_request:
            p = request_params(params, infer_text=True) if self.infer_text else request_params(params)
            if self.infer_text and (emb is not None or stream is not None):
                raise ValueError("a text-mode pool takes token ids only (no emb, no stream)")
            if p.manual_seed is None and not self.device_rng:
                raise NotImplementedError("a request without manual_seed needs a pool with the device generator (rng='device')")
            if not (0 <= int(row_offset) and int(row_offset) + self.nrow <= int(total_rows)):
                raise ValueError("row_offset / total_rows: the request's sampling rows (4, text mode: 1) must lie inside the batch")
            if emb is not None and tuple(emb.shape) != (ids.shape[0], GPT.hidden):
                raise ValueError("emb must be [T, 768] for a [T, 4] prompt")
        elif params is not None or row_offset != 0 or total_rows != GPT.n_vq or emb is not None:
            raise ValueError("params / row_offset / total_rows / emb need SlotPool(per_request=True)")
        if stream is not None:
            StreamCursor(stream)      # validates the spec
        self.queue.append(_Req(rid, ids, tm, int(max_new_token), int(stop_at), p, int(row_offset), int(total_rows), emb, stream))

    def cancel(self, rid) -> bool:
        """Drops a request: a queued one leaves the queue, an admitted one is retired at the next poll (its finish flag is set, its slot
        freed, nothing more is handed out for it).  False when the pool does not know the request (it completed already)."""
        for r in self.queue:
            if r.rid == rid:
                self.queue.remove(r)
                return True
        for r, _, _ in self.active.values():
            if r.rid == rid:
                r.cancelled = True
                return True
        return False

    def _admit_rows(self, slots: List[int], reqs: List[_Req], sl: torch.Tensor) -> None:
        """per-request pools: the admitted slots' sampling table entries, global sampling rows and Exp(1) rows (stream-ordered)"""
        dev, nvq = self.dev, self.nrow
        tab = []
        for r in reqs:
            seeded = r.params.manual_seed is not None
            seed = (r.params.manual_seed if seeded else self.pool_seed) if self.device_rng else 0
            row = sampling_row(r.params, seed, self.device_rng and not seeded)
            tab.append(np.frombuffer(bytes(row), dtype=np.uint8))
        self.rows[sl] = torch.from_numpy(np.stack(tab)).to(dev)
        self.row_base[sl] = torch.tensor([r.row_offset for r in reqs], dtype=torch.int32, device=dev)
        if not self.device_rng:
            for s_, r in zip(slots, reqs):    # the request's rows of the draw of a total_rows batch (what generate uploads for it)
                q = ExpDraws(r.total_rows, self.V, r.params.manual_seed, row_begin=r.row_offset, row_end=r.row_offset + nvq).step(0)
                self.q[0, s_ * nvq: (s_ + 1) * nvq] = q.to(dev)

    def _admit(self) -> None:
        # A group is left-padded to its longest prompt Tg, and every member then needs Tg + max_new_token + 1 <= cap (not just
        # its own prompt length, which is all submit() can check): take queued requests in FIFO order while that holds for the
        # whole group; the first one that does not fit waits for the next round (alone it always fits).  Nothing is popped
        # from the queue / the free list before the group is known to be valid.
        n, Tg, need = 0, 0, 0
        for r in list(self.queue)[: len(self.free)]:
            t_new = max(Tg, int(r.ids.shape[0]))
            need_new = max(need, r.max_new)
            if n > 0 and t_new + need_new + 1 + 2 * self.POLL > self.cap:
                break
            n, Tg, need = n + 1, t_new, need_new
        if n == 0:
            return
        assert Tg + need + 1 + 2 * self.POLL <= self.cap
        reqs = [self.queue.popleft() for _ in range(n)]
        self.admissions += 1
        slots = [self.free.pop(0) for _ in range(n)]              # lowest free slots first (deterministic)
        ids = torch.zeros((n, Tg, GPT.n_vq), dtype=torch.int64)
        mask = torch.zeros((n, Tg), dtype=torch.bool)
        tmask = torch.zeros((n, Tg), dtype=torch.bool)
        for i, r in enumerate(reqs):                               # left padding, like Tokenizer.encode (tokenizer.py:73-110)
            t = int(r.ids.shape[0])
            ids[i, Tg - t:], mask[i, Tg - t:], tmask[i, Tg - t:] = r.ids, True, r.tmask
        dev = self.dev
        with torch.cuda.stream(self.st):
            sl = torch.tensor(slots, dtype=torch.long, device=dev)
            emb = self.eng.embed_prompt(ids, tmask)
            for i, r in enumerate(reqs):
                if r.emb is not None:
                    t = int(r.ids.shape[0])
                    emb[i, Tg - t:] = r.emb.to(device=dev, dtype=emb.dtype)
            if self.per_request:
                self._admit_rows(slots, reqs, sl)
            self.ids_buf[sl, :Tg] = ids.to(dev)
            self.len[sl] = Tg
            self.prompt_len[sl] = Tg
            self.kv_start[sl] = (Tg - mask.sum(1)).to(torch.int32).to(dev)
            self.finish[sl] = 0
            self.end_idx[sl] = 0
            self.stop_at[sl] = torch.tensor([r.stop_at for r in reqs], dtype=torch.int32, device=dev)
            if self.rng_nonce is not None:   # (per-request pools: every admission; only unseeded rows read it)
                self._admit_no += n
                # globally unique admission numbers (never the constant word of a plain generate() call)
                self.rng_nonce[sl] = torch.arange(self._admit_no - n + 1, self._admit_no + 1, dtype=torch.int32, device=dev)
                for i, r in enumerate(reqs):
                    self.nonce_of[r.rid] = self._admit_no - n + 1 + i
            rmap = sl.to(torch.int32)
            ws = _engine.device_scratch(self.lib.ctts_gpt_workspace_bytes(n, Tg), dev)
            pre = self._state(B=n, T=Tg, workspace=ws, row_map=rmap, n_active=None)
            _lib.check(self.lib.ctts_gpt_prefill(self.handle, C.byref(pre), emb.data_ptr(), self.st.cuda_stream), "ctts_gpt_prefill")
            self._keep = (ws, emb, rmap, sl)  # stream-ordered: stay alive until the next poll's sync, no extra sync here
        since = self._snap_seq      # snapshots enqueued before this admission still show the previous occupant
        for s_, r in zip(slots, reqs):
            r.cursor = StreamCursor(r.stream) if r.stream is not None else None
            self.active[s_] = (r, Tg, since)
            self.slot_of[r.rid] = s_

    # -- main loop --------------------------------------------------------------------------------------------
    def _snapshot(self):
        """stream-ordered shader copy of the finish flags + end_idx into one of two pinned blocks, and the event behind it"""
        blk, ev = self._snaps[self._snap_seq % 2]
        _lib.check(self.lib.ctts_copy_bytes(blk.data_ptr(), self.state_blk.data_ptr(), blk.numel(), self.st.cuda_stream), "ctts_copy_bytes")
        ev.record(self.st)
        self._snap_seq += 1
        return self._snap_seq - 1, blk, ev

    def run(self, between=None, grouped: bool = False, events: bool = False) -> Iterator:
        """Yields (request id, ids [n,4] int64, hiddens [n,768] float32) as requests complete, admitting queued
        requests into freed slots between decode chunks.  ONE chunk runs ahead: the next POLL steps are enqueued before the host
        looks at the previous chunk's flags, so the device never waits for the poll, the admission prefill or the result copies
        (a freed slot idles for at most two chunks instead of one).  A slot's entry only listens to snapshots enqueued after its
        admission -- an older one still shows the previous occupant's flag.  `between` (optional callable): called once per chunk, before
        admission -- a server submits newly arrived requests there and lets other GPU users in (SpeechBatcher).  `grouped=True`: yields
        instead ONE list of those triples per poll -- the requests that completed together (SpeechBatcher's ragged decode).
        `events=True`: at a poll at which chunks of streamed requests (`submit(stream=...)`) became due, a `StreamEvents` is yielded
        first -- at once, not one chunk later like the results: the consumer decodes the chunks from `self.hiddens` while the generator
        is suspended, so a finished slot's rows are still its own (the slot is freed, and re-admitted, only after the generator resumes;
        the device meanwhile runs the chunk that was enqueued ahead)."""
        while self.busy():
            if between is not None:
                between()
            yield from self.tick(grouped, events)

    # The loop body of run() in three pieces, so that ONE worker can drive several pools (SpeechBatcher(refine=True): the text pool and
    # the code pool): `launch()` of every pool first -- one chunk of each enqueued on its own stream -- and only then the waits.
    def busy(self) -> bool:
        """requests queued or resident, a snapshot not read yet, or results not handed out yet"""
        return bool(self.queue or self.active or self._pending or self._ready)

    def tick(self, grouped: bool = False, events: bool = False) -> Iterator:
        """one iteration of run(): admit + enqueue a chunk, hand out the previous poll's results, read the oldest snapshot"""
        self.launch()
        yield from self.results(grouped)
        yield from self.poll(events)

    def launch(self) -> bool:
        """admits queued requests into free slots and enqueues one POLL-step chunk + its snapshot when slots are live (True then)"""
        self._admit()
        if not self.active:
            return False
        _lib.check(self.lib.ctts_gpt_graph_launch(self.handle, self.POLL, self.st.cuda_stream), "ctts_gpt_graph_launch")
        self.steps += self.POLL
        self._pending.append(self._snapshot())
        return True

    def results(self, grouped: bool = False) -> Iterator:
        """the results of the previous poll: their copies were enqueued in front of the chunk launched last, so the device stays busy
        while the host waits for them"""
        while self._ready:
            ev_out, outs = self._ready.popleft()
            wait_event(ev_out)
            yield from self._hand_out(outs, grouped)

    def poll(self, events: bool = False) -> Iterator:
        """reads the oldest snapshot once a second chunk runs ahead of it (or nothing is live any more): retires cancelled and finished
        slots, yields the due StreamEvents at once, queues the finished requests' results for the next `results()`"""
        pending, ready = self._pending, self._ready
        if len(pending) < 2 and self.active:
            return            # keep one chunk running ahead of the snapshot the host is about to read
        if not pending:
            return
        seq, blk, ev = pending.popleft()
        wait_event(ev)        # polled, not an interrupt wait (chattts_amd/_sync.py)
        fin = blk[: self.S]
        end = blk[self._Sp:].view(torch.int32)[: self.S]
        gone = [s for s, (r, _, _) in self.active.items() if r.cancelled]
        if gone:                  # cancel(rid): the slot stops computing and is free for the next admission
            with torch.cuda.stream(self.st):
                for s in gone:
                    self.active.pop(s)
                    self.finish[s] = 1
            self.free.extend(gone)
            self.free.sort()
        done = [s for s, (r, _, since) in self.active.items() if seq >= since and (bool(fin[s]) or int(end[s]) >= r.max_new)]
        if events:
            chunks = []
            for s, (r, _, since) in self.active.items():
                if r.cursor is None or seq < since:
                    continue
                n = min(int(end[s]), r.max_new)
                due = r.cursor.finish(n, bool(fin[s]) and int(end[s]) < r.max_new) if s in done else r.cursor.advance(n)
                chunks += [(r.rid, s, *c) for c in due]
            if chunks:
                yield StreamEvents(chunks)
        if not done:
            return
        outs = []
        with torch.cuda.stream(self.st):
            for s in done:
                r, Tg, _ = self.active.pop(s)
                n = min(int(end[s]), r.max_new)
                if self.per_request and n == 0 and bool(fin[s]) and r.stop_at < 0 and r.max_new > 0:
                    # step 0 drew EOS: generate's rule (engine.py, gpt.py:527-570) -- an unseeded request with ensure_non_empty is
                    # generated again (fresh admission number / draw), any other yields nothing
                    self.finish[s] = 1
                    if r.params.manual_seed is None and r.params.ensure_non_empty:
                        self.queue.appendleft(r)
                        continue
                    outs.append((r.rid, self.ids_buf[s, :0, 0].clone() if self.infer_text else self.ids_buf[s, :0].clone(),
                                 self.hiddens[s, :0].clone()))
                    continue
                if self.infer_text:     # gpt.py:300-301: the text row is slot 0 of the replicated ids; no hidden states are kept
                    outs.append((r.rid, self.ids_buf[s, Tg: Tg + n, 0].clone(), self.hiddens[s, :0].clone()))
                else:
                    outs.append((r.rid, self.ids_buf[s, Tg: Tg + n].clone(), self.hiddens[s, :n].clone()))
                self.finish[s] = 1      # a request cut at max_new_token stops costing attention bandwidth
            ev_out = torch.cuda.Event()
            ev_out.record(self.st)
        ready.append((ev_out, outs))    # handed out after the next chunk has been enqueued; the slots are free now (re-admission
        self.free.extend(done)          # writes are stream-ordered behind the copies)
        self.free.sort()

    @staticmethod
    def _hand_out(outs: list, grouped: bool):
        if not grouped:
            yield from outs
        elif outs:
            yield outs


class _Cancel:
    def __init__(self, rid):
        self.rid = rid


class SpeechStream:
    """`SpeechBatcher.submit_stream`'s result: an iterator over one streamed request's int16 chunks, fed by the worker through a
    thread-safe queue.  It ends when the request is complete; an error (an empty result too) is raised from `next`.  `close()` before
    the end cancels the request: its slot is retired at the pool's next poll."""

    def __init__(self, batcher: "SpeechBatcher", rid):
        self._b, self.rid, self._q, self._done = batcher, rid, queue.Queue(), False

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        if self._done:
            raise StopIteration
        item = self._q.get()
        if item is None or isinstance(item, BaseException):
            self._done = True
            if item is None:
                raise StopIteration
            raise item
        return item

    def close(self) -> None:
        if not self._done:
            self._done = True
            self._b._in.put(_Cancel(self.rid))


def split_rows(n: int, max_split_batch: int) -> List[Tuple[int, int]]:
    """(row_offset, total_rows) of every sentence of an n-sentence split_text call: `Chat._infer` generates the sentences in batches of
    `max_split_batch`, so sentence i holds sampling rows 4 (i % max_split_batch) .. + 3 of a batch of 4 * (its batch's size) rows"""
    m = int(max_split_batch)
    if m < 1:
        raise ValueError("max_split_batch must be positive")
    return [(GPT.n_vq * (i % m), GPT.n_vq * min(m, n - (i - i % m))) for i in range(n)]


@dataclass(eq=False)
class _Job:
    """one request of a SpeechBatcher, from `submit` / `submit_stream` to its resolution: what travels on the worker's queue and what
    `SpeechBatcher._jobs` holds while the request is wanted"""
    rid: object
    text: str                              # as the endpoint received it
    params: object                         # its InferCodeParams (never modified)
    sink: object                           # the caller's end: a Future, or a SpeechStream
    refine: object = None                  # its RefineTextParams: the refine-text pass runs first
    max_split_batch: Optional[int] = None  # None unless the request is split_text
    sample_rate: Optional[int] = None      # None: 24 kHz
    encoding: Optional[str] = None         # None: int16
    code_text: Optional[str] = None        # the text of the code stage: normalised, with `refine` then refined
    in_text_pool: bool = False             # the refine-text pass of an unsplit request is queued or resident
    speed: Optional[float] = None          # None: 1.0 (on a stream only with SpeechBatcher(stream_speeds=True))
    flac: bool = False                     # the result is the FLAC file of the int16 waveform; a stream: its chunks are FLAC frames
    adpcm: bool = False                    # the result is the IMA ADPCM WAV file of the int16 waveform; a stream: its chunks are ADPCM blocks
    loudness: Optional[float] = None       # a target in LUFS (non-streamed only); None: the level is left alone
    pauses: object = None                  # a pauses.PauseSpec (non-streamed only); None: the silence is left alone
    limiter: bool = False                  # the look-ahead peak limiter behind the loudness stage's gain; a stream: in front of the conversion
    lm_gain: Optional[float] = None        # ... and the float32 pre-gain of its `gain_db` (None: 1)
    compress: object = None                # a checked compressor spec; None: the dynamics are left alone
    eq: object = None                      # a checked equaliser spec (non-streamed only); None: the spectrum is left alone
    streams: Optional[StreamSet] = None    # a stream: the streams of its stages (winchain.STAGES), opened at its first chunk

    @property
    def is_stream(self) -> bool:
        return isinstance(self.sink, SpeechStream)

    def __getitem__(self, i):
        """the queue item was a tuple that began (rid, text, params, sink): wrappers of `_take` that index it keep working"""
        return (self.rid, self.text, self.params, self.sink)[i]


@dataclass(eq=False)
class _SplitReq:
    """one split_text request in flight (SpeechBatcher.submit(split_text=True)).  Its pool requests carry tuple ids: (rid, "r", i) sentence
    i in the text pool, (rid, "A") the refer sentence alone (stage A), (rid, i) sentence i of stage B."""
    job: _Job
    params: object                 # the caller's object until stage A ends, then a COPY with spk_smp / txt_smp filled
    texts: list                    # per sentence: its normalised (refine: refined) text, None while it is in the text pool
    hids: list                     # per sentence: its hidden states, None until stage B delivered them
    need_a: bool
    keys: set = field(default_factory=set)     # its pool requests that are queued or resident
    a_started: bool = False
    a_done: bool = False
    b_started: bool = False


_NO_AUDIO = "the engine returned no audio (the first token was EOS)"
_NO_TEXT = "the refine-text pass returned no tokens (the first token was EOS)"


def _job_speed(speed) -> Optional[float]:
    """a request's speed as its job carries it: in hundredths, None for 1.0; ValueError outside 0.5 .. 2.0"""
    if speed is None:
        return None
    num, den = TS.quantize(speed)
    return None if num == den else num / den


def _format_kw(jobs, rate_kw: str = "sample_rate", encoding_kw: str = "encoding", speed_kw: str = "speed") -> dict:
    """the output-format keywords of ONE decode that serves `jobs`, one list entry per job.  Nothing when every job wants 24 kHz int16
    at speed 1: the collaborator is then called exactly as it was before it knew rates, encodings and speeds (the host fakes pin that)."""
    kw = option_kw({rate_kw: [j.sample_rate for j in jobs], encoding_kw: [j.encoding for j in jobs], speed_kw: [j.speed for j in jobs],
                    "flac": [j.flac for j in jobs], "loudness": [j.loudness for j in jobs], "pauses": [j.pauses for j in jobs],
                    "limiter": [j.limiter for j in jobs], "adpcm": [j.adpcm for j in jobs], "compress": [j.compress for j in jobs],
                    "eq": [j.eq for j in jobs]})
    if rate_kw in kw:
        kw[rate_kw] = [24000 if r is None else r for r in kw[rate_kw]]
    if speed_kw in kw:
        kw[speed_kw] = [1.0 if v is None else v for v in kw[speed_kw]]
    return kw


def _file_parts(items: list) -> list:
    """(job, ...) items of one poll -> the lists that are decoded together: one, unless the poll holds FLAC and ADPCM requests -- a
    decode call hands out one kind of file, so the ADPCM requests then get a decode of their own"""
    if any(it[0].adpcm for it in items) and any(it[0].flac for it in items):
        return [[it for it in items if not it[0].adpcm], [it for it in items if it[0].adpcm]]
    return [items]


class SpeechBatcher:
    """Serves many non-streamed speech requests from ONE per-request slot pool (continuous batching behind `server.create_app(...,
    batch_slots=N)`).  A single worker thread owns the pool and all GPU work of pooled requests: requests arrive through a thread-safe
    queue (`submit` returns a Future), the worker builds their prompts with the code `Chat.infer` uses (normalise -> `Chat.code_prompt`
    -> `Chat.prompt_embedding`), submits them between decode chunks, and decodes every finished request ALONE through the serial path's
    decoder and silence strip (a padded batch decode would let the DVAE conv biases of padded frames into the tails of shorter rows).
    `ragged_decode=True`: the requests that finish in one poll are decoded TOGETHER instead, each still as if alone -- one ragged
    decode (Chat.decode_to_pcm16(..., ragged=True)), one PCM16 pass and one device-to-host copy per poll.
    `gpu_lock` (a threading.Lock shared with the streamed path) is taken per decode chunk and per decode, never per request.
    An error in one request fails that request's Future only (an empty result -- step 0 drew EOS -- too).  `decode_calls` counts the
    decodes, `decoded` the requests they served, `max_decode_group` the most requests one decode served.

    `streams=True`: `submit_stream` serves streamed requests from the same pool.  The chunks of all streams that are due at one poll
    are decoded by ONE window decode straight from the pool's hidden-state store (`Chat.decode_windows_pcm16` ->
    `CodecEngine.decode_windows`), each what the serial streamed path yields for that request; `stream_decode_calls` counts those
    decodes, `stream_chunks` the chunks they served, `max_stream_group` the most one decode served.

    `stream_speeds=True` (with `streams`; off: `submit_stream(speed=)` is refused as before): a streamed request may carry a speed.
    Its job record holds a stream of the time scaler (`CodecEngine.time_scale_stream_open`, opened at its first chunk, given back
    in `_resolve` however the request ends); the chunks due at one poll -- at whatever speeds, speed 1 among them -- still come from
    one window decode (`CodecEngine.decode_windows(speeds=, ts_streams=)`); `occupancy()["stream_scaled_chunks"]` counts them.
    `stream_speed_rates=True` (with `stream_speeds`; off: a streamed speed at another rate than 24000 is refused as before): such a
    request's job also holds a stream of the resampler (`CodecEngine.resample_stream_open(24000, rate)`, opened and given back where
    the time scaler's is) and its chunks are the scaler's chunks resampled with the filter's history and look-ahead carried
    (`decode_windows(..., rs_streams=)`): those of the serial call with `stream_scaled_resample=True`.
    `stream_flac=True` (with `streams`; off: `submit_stream(flac=True)` is refused as before): a streamed request may ask for FLAC.
    Its job holds a stream of the encoder (`CodecEngine.flac_stream_open(rate)`, opened at its first chunk, given back in `_resolve`
    however the request ends); the chunks of all FLAC streams due at one poll are the pushes of ONE encoder step behind the one
    window decode (`decode_windows(flac=, flac_streams=)`); `occupancy()["stream_flac_chunks"]` counts them.
    `stream_adpcm=True` (with `streams`; off: `submit_stream(adpcm_blocks=True)` is refused): likewise for IMA ADPCM -- the job holds
    a stream of that encoder (`CodecEngine.adpcm_stream_open(rate)`), the chunks of all ADPCM streams due at one poll are the pushes
    of ONE encoder step (`decode_windows(adpcm=, adpcm_streams=)`), and `occupancy()["stream_adpcm_chunks"]` counts them.

    `refine=True`: requests may ask for the reference's DEFAULT behaviour, the refine-text pass in front of the code pass
    (`submit(text, params, refine=RefineTextParams(...))`).  A second, TEXT-mode per-request pool (SlotPool(infer_text=True), its own
    handle and stream, `text_cap` positions per slot: the endpoint's 2048-character inputs + 384 new tokens by default) serves that stage:
    the request is admitted there first; when its text row completes the worker turns it into the code-stage text with the helpers
    `Chat._infer` uses (`Chat.refined_text`, then `Chat.code_prompt` / `Chat.prompt_embedding`) and submits it to the code pool, as a
    stream if it was one.  The result is what `Chat.infer([text], skip_refine_text=False, params_refine_text=refine,
    params_infer_code=params, pcm16=True[, stream=True])` returns for the request alone.  ONE worker owns both pools: every iteration
    enqueues one chunk of every pool that has work -- on their two streams, so the text chain overlaps the code chain on the device --
    before it waits for any snapshot.  The text pool draws from the HOST generator (`refine_rng="host"`: what the serial refine pass
    draws from whatever the engine's `rng` is -- seeded requests only); `refine_rng="device"` serves unseeded refine requests too, from
    the sampling kernel's generator (`GptEngine.generate(text_rng="device")` is that request alone).  `occupancy()["refine"]` counts
    text admissions, the most co-resident text requests, text steps, hand-offs, and the polls at which both pools had live slots.
    A request without `refine` takes the code pool directly, as without the option.

    `submit(..., split_text=True)`: the reference's default handling of a long input (`Chat.infer(text: str, split_text=True)`), with the
    request's sentences side by side in the slots.  The worker cuts the text with `core.split_sentences`; one sentence is an ordinary
    request.  Otherwise: stage A (only without `params.spk_smp`) -- sentence 0 alone, its decode through the DVAE encoder on the device
    (`Chat.refer_speaker`) becomes the `spk_smp` prompt of a COPY of the parameters; stage B -- every sentence (sentence 0 again) with the
    sampling rows it has in the serial call's batches of `max_split_batch` (`split_rows`), in as many slots as are free, other requests
    interleaving; when the last one is done the request is decoded by `Chat.decode_split_to_pcm16` -- with `ragged_decode`, together
    with everything else that finished at that poll.  With `refine` the sentences pass the text pool first, as rows i of n; stage A
    starts when sentence 0's text is back.  A sentence whose first token is EOS, one that does not fit a slot, or any other error fails
    that request alone and frees all its slots; `cancel(future)` drops every sentence.  `occupancy()["split"]`: split requests,
    stage-B sentences, the most sentences of one request co-resident.

    `make_pool` / `make_text_pool` (tests: fakes) build the pools; by default a per-request SlotPool on `chat.gpt` with the engine's generator mode,
    `cap` = the engine's position limit (the longest accepted prompt + max_new_token 2048 + slack), `hid_cap` 2048."""

    def __init__(self, chat, slots: int, gpu_lock: threading.Lock, *, make_pool=None, cap: Optional[int] = None, hid_cap: int = 2048,
                 logger=None, ragged_decode: bool = False, streams: bool = False, refine: bool = False, make_text_pool=None,
                 text_cap: Optional[int] = None, refine_rng: str = "host", stream_speeds: bool = False, stream_speed_rates: bool = False,
                 stream_flac: bool = False, stream_limiter: bool = False, stream_pauses: bool = False, stream_adpcm: bool = False,
                 stream_compress: bool = False):
        import logging
        self.chat, self.lock, self.S = chat, gpu_lock, int(slots)
        self.ragged_decode = bool(ragged_decode)
        self.decode_calls = 0        # decoder passes over finished requests
        self.decoded = 0             # requests those passes served
        self.max_decode_group = 0    # most requests one pass served
        self.streams = bool(streams)
        self.stream_decode_calls = 0  # window decodes over the due chunks of streamed requests
        self.stream_chunks = 0        # chunks those decodes served (empty chunks included)
        self.stream_resampled_chunks = 0   # those of them at another rate than 24 kHz
        self.stream_speeds = bool(stream_speeds)   # submit_stream(speed=) is accepted
        self.stream_speed_rates = bool(stream_speeds and stream_speed_rates)   # ... at another rate than 24000 too
        self.stream_scaled_chunks = 0      # chunks of streams at another speed than 1
        self.stream_flac = bool(stream_flac)       # submit_stream(flac=True) is accepted
        self.stream_flac_chunks = 0        # chunks handed out as FLAC frames (empty ones included)
        self.stream_adpcm = bool(stream_adpcm)     # submit_stream(adpcm_blocks=True) is accepted
        self.stream_adpcm_chunks = 0       # chunks handed out as IMA ADPCM blocks (empty ones included)
        self.stream_limiter = bool(stream_limiter)   # submit_stream(limiter=True) is accepted
        self.stream_limited_chunks = 0     # chunks that came out of a limiter stream (empty ones included)
        self.stream_pauses = bool(stream_pauses)     # submit_stream(pauses=) is accepted
        self.stream_paused_chunks = 0      # chunks that came out of a pause stream (empty ones included)
        self.stream_compress = bool(stream_compress)   # submit_stream(compress=) is accepted
        self.stream_compressed_chunks = 0  # chunks that came out of a compressor stream (empty ones included)
        self.companded = 0                 # outputs handed out as G.711 (results and streamed chunks)
        self.flac_encoded = 0              # results handed out as FLAC files
        self.adpcm_encoded = 0             # results handed out as IMA ADPCM WAV files
        self.adpcm_asked = False           # some request has asked for one: only then does occupancy() carry the counter
        self.trimmed = 0                   # results handed out with their pauses trimmed
        self.max_stream_group = 0     # most chunks one window decode served
        self.cancelled = 0            # streams closed by their consumer before the end
        self.log = logger or logging.getLogger("chattts_amd.serving")
        self._in: "queue.Queue" = queue.Queue()      # _Job | _Cancel | None (close)
        self._jobs: dict = {}        # request id -> its _Job, from `_take` until `_resolve`: the requests that are still wanted
        self._ids = itertools.count()
        self.admissions = 0          # requests admitted into the pool
        self.max_coresident = 0      # most requests resident in the pool at once
        self.completed = 0
        self.failed = 0
        self._stop = False
        self._splits: dict = {}          # request id -> its _SplitReq
        self._sub: dict = {}             # pool request id (a tuple) -> the _SplitReq it belongs to
        self.split_requests = 0          # split_text requests of more than one sentence
        self.split_sentences = 0         # sentences submitted to stage B
        self.split_max_coresident = 0    # most stage-B sentences of ONE request resident at once
        if make_pool is None:
            def make_pool():
                eng = chat.gpt
                return SlotPool(eng, slots=self.S, cap=cap if cap is not None else eng.max_pos, hid_cap=hid_cap,
                                rng=getattr(eng, "rng", "host"), per_request=True)
        self._make_pool = make_pool
        self.refine = bool(refine)
        self.text_pool = None
        self.refine_admissions = 0       # requests admitted into the text pool
        self.refine_max_coresident = 0   # most requests resident in the text pool at once
        self.handed = 0                  # requests handed from the text pool to the code pool
        self.both_live_polls = 0         # worker iterations at which both pools had live slots
        if self.refine and make_text_pool is None:
            def make_text_pool():
                eng = chat.gpt
                # the endpoint accepts 2048 characters (<= 2048 text tokens + the prompt's decoration) and refines with max_new_token 384
                tc = text_cap if text_cap is not None else min(eng.max_pos, 2048 + 64 + 384 + 1 + 2 * SlotPool.POLL)
                return SlotPool(eng, slots=self.S, cap=tc, rng=refine_rng, per_request=True, infer_text=True,
                                eos_token=chat.tokenizer.eos_token)
        self._make_text_pool = make_text_pool
        with self.lock:
            self.pool = make_pool()
            if self.refine:
                self.text_pool = make_text_pool()
        self._thread = threading.Thread(target=self._loop2 if self.refine else self._loop, name="speech-batcher", daemon=True)
        self._thread.start()

    # -- public -------------------------------------------------------------------------------------------------------------
    def submit(self, text: str, params, refine=None, split_text: bool = False, max_split_batch: int = 4, sample_rate=None,
               encoding=None, speed=None, flac: bool = False, loudness=None, pauses=None, limiter: bool = False,
               adpcm: bool = False, compress=None, eq=None) -> Future:
        """one non-streamed request: `text` as the endpoint received it, `params` its InferCodeParams.  The Future resolves to the
        int16 waveform `Chat.infer([text], skip_refine_text=True, params_infer_code=params, pcm16=True)[0]` would return.
        `refine` (a `RefineTextParams`; batchers built with refine=True): the refine-text pass runs first, in the text pool -- the
        result is that of `Chat.infer([text], skip_refine_text=False, params_refine_text=refine, ...)`.
        `split_text=True`: the result is that of `Chat.infer(text, split_text=True, max_split_batch=..., ragged_decode=True,
        pcm16=True, ...)[0]` -- the same tokens per sentence, ONE waveform under one peak (see the class text).  `params` is never
        modified (the serial call writes the speaker prompt into it).  `sample_rate` (None: 24000): the rate of the returned audio, the
        serial call's `sample_rate=`; requests that finish together at different rates are decoded together and resampled in one
        launch per distinct rate (CodecEngine.resample_segments).  `encoding` (None: int16; "ulaw" / "alaw"): the serial call's
        `encoding=` -- the Future resolves to the uint8 G.711 codes of that waveform; requests that finish together with different
        encodings still share the one decode, and one companding launch (ctts_g711_encode_ranges).  `speed` (None: 1.0; 0.5 .. 2.0):
        the serial call's `speed=` -- the same tokens, time-scaled on the device behind the decode; requests that finish together at
        different speeds still share the one ragged decode (CodecEngine.time_scale_segments: rows at speed 1 are copied through).
        `flac=True`: the serial call's `flac=` -- the Future resolves to a uint8 array, the complete FLAC file of that int16 waveform
        at its rate; not together with `encoding`.  Requests that finish together, with and without it, still share the one decode;
        the encoder runs on the device behind the grouped conversion (CodecEngine.flac_encode), in `finish` by the host twin.
        `loudness` (None: untouched; a target in LUFS, -40 .. -5): the serial call's `loudness=` -- the waveform is brought to that
        BS.1770 integrated loudness on the device, in front of the strip and the conversion; requests that finish together with
        different targets, or none, still share the one ragged decode and ONE normalisation call (a split request is one group of
        it: one gain over its sentences).
        `pauses` (None: untouched; True, a pauses.PauseSpec or a dict of its fields): the serial call's `pauses=` -- edge silence
        trimmed and long pauses capped on the device, behind the resampler and in front of the loudness stage; requests that finish
        together with different specs, or none, still share the one ragged decode and ONE `CodecEngine.trim_pauses` call (a request
        without a spec is copied through it; every sentence of a split request is trimmed alone).
        `limiter=True`: the serial call's `limiter=` -- the look-ahead peak limiter behind the loudness stage's gain, which then drops
        its ceiling term (at unity gain without `loudness`); requests that finish together, with and without it, still share the one
        decode, and the ones without it are not touched by it (every sentence of a split request is limited alone).
        `adpcm=True`: the serial call's `adpcm=` -- the Future resolves to a uint8 array, the complete WAVE_FORMAT_IMA_ADPCM file
        (4 bits per sample) of that int16 waveform at its rate; not together with `encoding` or `flac`.  Requests that finish
        together, with and without it, still share the one decode; the encoder runs on the device behind the grouped conversion
        (CodecEngine.adpcm_encode), in `finish` by the host twin; `occupancy()["adpcm_encoded"]` counts them from the first such request on.  A poll whose requests ask for FLAC and for ADPCM is decoded in two
        groups, one per kind of file.
        `compress` (None / False: off; True or a dict of compressor.RANGES' fields): the serial call's `compress=` -- the look-ahead
        compressor on the device, behind `pauses` and in front of the loudness stage; requests that finish together with different
        specs, or none, still share the one ragged decode and ONE `CodecEngine.compress` call (a request without a spec is copied
        through it; every sentence of a split request is compressed alone).
        `eq` (None / False: off; an equaliser preset name or a dict of equalizer.FIELDS): the serial call's `eq=` -- the biquad
        cascade on the device, behind `pauses` and in front of `compress`; requests that finish together with different specs, or
        none, still share the one ragged decode and ONE `CodecEngine.equalize` call (a request without a spec is copied through it;
        every sentence of a split request is filtered alone from zero state)."""
        eq = EQ.check(eq, "submit")
        if eq is not None:
            eq = EQ.check(eq, "submit", LN.check_rate(24000 if sample_rate is None else sample_rate))
        compress = CP.check(compress, "submit")
        if compress is not None:
            LN.check_rate(24000 if sample_rate is None else sample_rate)
        limiter = LM.check_flag(limiter, "submit")
        if limiter:
            LN.check_rate(24000 if sample_rate is None else sample_rate)
        pauses = PA.check(pauses)
        if pauses is not None:
            PA.check_rate(24000 if sample_rate is None else sample_rate)
        loudness = LN.check_target(loudness)
        if loudness is not None:
            LN.check_rate(24000 if sample_rate is None else sample_rate)
        G711.check_encoding(encoding)
        if flac:
            if encoding is not None:
                raise ValueError("flac does not go with an encoding (a FLAC file holds the 16-bit samples)")
            FLAC.rate_code(24000 if sample_rate is None else sample_rate)
        if adpcm:
            if encoding is not None:
                raise ValueError("adpcm does not go with an encoding (an ADPCM file is coded from the 16-bit samples)")
            if flac:
                raise ValueError("adpcm does not go with flac (a request is answered with one kind of file)")
            ADPCM.check_rate(24000 if sample_rate is None else sample_rate)
            self.adpcm_asked = True
        speed = _job_speed(speed)
        self._check_refine(refine)
        if split_text and int(max_split_batch) < 1:
            raise ValueError("max_split_batch must be positive")
        fut: Future = Future()
        fut.rid = next(self._ids)
        self._in.put(_Job(fut.rid, text, params, fut, refine, int(max_split_batch) if split_text else None, self._rate(sample_rate), encoding,
                          speed=speed, flac=bool(flac), loudness=loudness, pauses=pauses, limiter=limiter, adpcm=bool(adpcm),
                          compress=compress, eq=eq))
        return fut

    def cancel(self, fut: Future) -> None:
        """drops a non-streamed request (every sentence of a split one, in whichever pool): its slots are retired at the next poll and
        the Future is cancelled.  Nothing happens when it has completed already."""
        self._in.put(_Cancel(fut.rid))

    def submit_stream(self, text: str, params, refine=None, split_text: bool = False, sample_rate=None, encoding=None,
                      speed=None, flac: bool = False, loudness=None, pauses=None, limiter: bool = False, gain_db=None,
                      adpcm_blocks: bool = False, compress=None) -> SpeechStream:
        """one streamed request: an iterator over the int16 chunks `Chat.infer([text], stream=True, skip_refine_text=True,
        params_infer_code=params, pcm16=True)` yields (each chunk flat, [n] instead of [1, n]).  Closing it cancels the request, in
        whichever pool it is.  `refine`: as in `submit`.  `split_text` is refused: the serial streamed schedule across split batches
        is not served from the pool.  `sample_rate` (None: 24000): the serial call's `sample_rate=` with `stream_resample=True` --
        every chunk is its range of the prefix's decode resampled as one signal; the chunks of streams at different rates that are
        due at one poll still come from one decoder pass (CodecEngine.decode_windows(sample_rates=)).  `encoding` (None: int16;
        "ulaw" / "alaw"): the serial call's `encoding=` -- the chunks are uint8 G.711 codes; the chunks of one poll share the decoder
        pass and ONE companding launch whatever their encodings (CodecEngine.decode_windows(encodings=)).  `speed` other than 1 is
        refused: a chunk's frames depend on the path of everything before it, which is not carried across chunks -- unless the
        batcher was built with `stream_speeds=True`: then the chunks are those of the serial call with `speed=, stream_time_scale=True`
        (the path and a tail of samples are carried on the device, per stream), at 24000 Hz only -- unless it was also built with
        `stream_speed_rates=True`: then `speed` goes with `sample_rate`, the serial call's `stream_scaled_resample=True`.  `flac` is
        refused: a streamed FLAC needs a variable-block-size stream and carried sample numbers -- unless the batcher was built with
        `stream_flac=True`: then the chunks are uint8, the FLAC frames each chunk completes (possibly none: up to 15 samples wait for
        the next chunk), the serial call's `flac=True, stream_flac=True`; behind `flac.stream_header(rate)` they decode to the int16
        chunks of the same request without `flac`.  The chunks of all FLAC streams due at one poll share ONE encoder step behind the
        one decoder pass (CodecEngine.decode_windows(flac=)); it combines with `sample_rate` and `speed` as far as the batcher serves
        those, not with `encoding`.  `loudness` is refused: an integrated loudness needs the whole utterance.  `pauses` is refused: the
        run state would have to be carried across chunks -- unless the batcher was built with `stream_pauses=True`: then the request
        gets a pause stream (opened at its first chunk, given back where its other streams are) and its chunks are those of the serial
        call with `pauses=, stream_pauses=True`, possibly empty (CodecEngine.decode_windows(pauses=); a spec that would make a stream
        hold more than `pauses.STREAM_FRAMES` frames is refused here).  `limiter` is refused: the look-ahead is not carried across chunks -- unless
        the batcher was built with `stream_limiter=True`: then the request gets a limiter stream (opened at its first chunk, given back
        where its other streams are) and its chunks are those of the serial call with `limiter=True, stream_limiter=True`: converted,
        companded or FLAC-encoded from limited samples, 20 ms behind.  The limiter streams due at one poll share one step per round
        behind their decoder pass (CodecEngine.decode_windows(limiter=)).  `gain_db` (with `limiter` only): the serial call's fixed
        make-up gain in front of the limiter, -30 .. +30 dB.  `adpcm_blocks` (accepted by a batcher built with `stream_adpcm=True`;
        refused otherwise, and together with `encoding` or `flac`): the chunks are uint8, the whole IMA ADPCM blocks each chunk
        completes (possibly none: up to S - 1 samples of an open block wait for the next chunk), the serial call's `adpcm=True,
        stream_adpcm=True`; concatenated they are `adpcm.encode_blocks` of the int16 chunks of the same request without it, and behind
        `adpcm.stream_header(rate)` an open-ended WAV file.  The request gets an ADPCM stream (opened at its first chunk, given back
        where its other streams are); the chunks of all ADPCM streams due at one poll share ONE encoder step behind the one decoder
        pass (CodecEngine.decode_windows(adpcm=)).  `compress` (None / False: off; True or a dict of compressor.RANGES' fields; one spec
        per request) is refused, with the TypeError of the time before the option: the block state would have to be carried across chunks -- unless the batcher was built with
        `stream_compress=True`: then the request gets a compressor stream (opened at its first chunk, given back where its other
        streams are) and its chunks are those of the serial call with `compress=, stream_compress=True`: converted, companded or
        encoded from compressed samples, the attack and at most two milliseconds behind.  The compressor streams due at one poll
        share one step per round behind their decoder pass and their pause streams, in front of their limiter streams
        (CodecEngine.decode_windows(compress=))."""
        if compress is not None and compress is not False and not self.stream_compress:     # as before the option existed: not an argument of this call
            raise TypeError("submit_stream() got an unexpected keyword argument 'compress': it applies to non-streamed requests only "
                            "(a stream would need the block state carried across chunks) unless the batcher is built with stream_compress=True")
        compress = CP.check(compress, "submit_stream")
        if compress is not None:
            LN.check_rate(24000 if sample_rate is None else sample_rate)
        if adpcm_blocks:
            if not self.stream_adpcm:
                raise ValueError("adpcm_blocks needs a batcher built with stream_adpcm=True (an ADPCM file is served for non-streamed "
                                 "requests only otherwise)")
            if encoding is not None:
                raise ValueError("adpcm_blocks does not go with an encoding (an ADPCM stream is coded from the 16-bit samples)")
            if flac:
                raise ValueError("adpcm_blocks does not go with flac (a stream is answered in one format)")
            if ADPCM.samples_per_block(24000 if sample_rate is None else sample_rate) - 1 > 2048:
                raise ValueError(f"a streamed ADPCM file at {sample_rate} Hz would carry more than a stream keeps: streams run below 55125 Hz")
        limiter = LM.check_flag(limiter, "submit_stream")
        if limiter and not self.stream_limiter:
            raise ValueError("limiter applies to non-streamed requests only (the look-ahead is not carried across chunks)")
        g32 = LM.check_gain_db(gain_db)
        if g32 is not None and not limiter:
            raise ValueError("gain_db is the make-up gain in front of the limiter: it needs limiter=True")
        if limiter:
            LN.check_rate(24000 if sample_rate is None else sample_rate)
        pauses = PA.check(pauses)
        if pauses is not None and not self.stream_pauses:
            raise ValueError("pauses applies to non-streamed requests only (a stream would need the run state carried across chunks)")
        if pauses is not None:
            PA.check_stream(24000 if sample_rate is None else sample_rate, pauses, "submit_stream")
        if LN.check_target(loudness) is not None:
            raise ValueError("loudness applies to non-streamed requests only (an integrated loudness needs the whole utterance; a stream "
                             "would need a running measure)")
        if flac and not self.stream_flac:
            raise ValueError("flac is served for non-streamed requests only (a streamed FLAC needs a variable-block-size stream and "
                             "carried sample numbers)")
        if flac:
            if encoding is not None:
                raise ValueError("flac does not go with an encoding (a FLAC stream holds the 16-bit samples)")
            FLAC.rate_code(24000 if sample_rate is None else sample_rate)
        G711.check_encoding(encoding)
        speed = _job_speed(speed)
        if speed is not None and not self.stream_speeds:
            raise ValueError("speed applies to non-streamed requests only (a chunk's frames depend on the path of everything before it)")
        if speed is not None and self._rate(sample_rate) is not None and not self.stream_speed_rates:
            raise ValueError("a streamed speed is served at 24000 Hz only (resampling the scaled stream would need its history and a "
                             "look-ahead carried too)")
        if split_text:
            raise ValueError("split_text is served for non-streamed requests only")
        if not self.streams:
            raise RuntimeError("this SpeechBatcher was built without streams=True")
        self._check_refine(refine)
        rate = self._rate(sample_rate)
        if rate is not None:
            K = RS.plan(24000, rate, [0, 1])[2]       # an unsupported pair is refused here, not at the first chunk
            if speed is not None and K - 1 > RS.CARRY:
                raise ValueError(f"a streamed speed at {rate} Hz would carry up to {K - 1} samples, a resampler stream keeps {RS.CARRY}")
        h = SpeechStream(self, next(self._ids))
        self._in.put(_Job(h.rid, text, params, h, refine, None, rate, encoding, speed=speed, flac=bool(flac),
                          **({"limiter": True, "lm_gain": g32} if limiter else {}), **({} if pauses is None else {"pauses": pauses}),
                          **({"adpcm": True} if adpcm_blocks else {}), **({} if compress is None else {"compress": compress})))
        return h

    def _check_refine(self, refine) -> None:
        if refine is not None and not self.refine:
            raise RuntimeError("this SpeechBatcher was built without refine=True")

    @staticmethod
    def _rate(sample_rate) -> Optional[int]:
        return None if sample_rate is None or int(sample_rate) == 24000 else int(sample_rate)

    def occupancy(self) -> dict:
        pool, tp = self.pool, self.text_pool
        occ = {"slots": self.S, "active": len(getattr(pool, "active", {})), "queued": self._in.qsize() + len(getattr(pool, "queue", ())),
               "admissions": self.admissions, "max_coresident": self.max_coresident, "completed": self.completed, "failed": self.failed,
               "ragged_decode": self.ragged_decode, "decode_calls": self.decode_calls, "decoded": self.decoded,
               "max_decode_group": self.max_decode_group, "companded": self.companded, "flac_encoded": self.flac_encoded,
               "trimmed": self.trimmed,
               "split": {"requests": self.split_requests, "sentences": self.split_sentences, "max_coresident": self.split_max_coresident}}
        if self.adpcm_asked:  # (a batcher that was never asked for the format reports as it always did)
            occ["adpcm_encoded"] = self.adpcm_encoded
        if self.streams:      # (list(): the worker changes the registry meanwhile)
            occ.update({"streams": sum(j.is_stream for j in list(self._jobs.values())), "stream_decode_calls": self.stream_decode_calls,
                        "stream_chunks": self.stream_chunks, "max_stream_group": self.max_stream_group, "cancelled": self.cancelled,
                        "stream_resampled_chunks": self.stream_resampled_chunks, "stream_scaled_chunks": self.stream_scaled_chunks})
            if self.stream_flac:
                occ["stream_flac_chunks"] = self.stream_flac_chunks
            if self.stream_adpcm:
                occ["stream_adpcm_chunks"] = self.stream_adpcm_chunks
            if self.stream_limiter:
                occ["stream_limited_chunks"] = self.stream_limited_chunks
            if self.stream_pauses:
                occ["stream_paused_chunks"] = self.stream_paused_chunks
            if self.stream_compress:
                occ["stream_compressed_chunks"] = self.stream_compressed_chunks
        if self.refine:
            occ["refine"] = {"active": len(getattr(tp, "active", {})), "queued": len(getattr(tp, "queue", ())),
                             "admissions": self.refine_admissions, "max_coresident": self.refine_max_coresident,
                             "steps": int(getattr(tp, "steps", 0)), "handed": self.handed, "both_live_polls": self.both_live_polls}
        return occ

    def close(self):
        self._stop = True
        self._in.put(None)
        self._thread.join(timeout=60)

    # -- worker -------------------------------------------------------------------------------------------------------------
    def _resolve(self, job: _Job, result=None, cancelled: bool = False) -> None:
        """The ONE exit of a request.  `result`: its waveform, or the exception that fails it; a stream: None, its end (its chunks went
        out already).  `cancelled`: its consumer dropped it.  A request that is not wanted any more (resolved already) is left alone."""
        sp = self._splits.pop(job.rid, None)
        if sp is not None:
            for k in sp.keys:
                self._sub.pop(k, None)
        if self._jobs.pop(job.rid, None) is None:
            return
        if job.streams:                    # finished, failed or cancelled: the streams of its stages go back to their pools
            job.streams.close(self.chat.codec)
        failed = isinstance(result, BaseException)
        if cancelled:
            self.cancelled += job.is_stream
        elif failed:
            self.failed += 1
        else:
            self.completed += 1
            self.flac_encoded += job.flac and not job.is_stream                  # (a stream's chunks are counted as they go out)
            self.adpcm_encoded += job.adpcm and not job.is_stream               # (likewise)
            self.trimmed += job.pauses is not None and not job.is_stream
            self.companded += not job.is_stream and job.encoding is not None      # (a stream's chunks are counted as they go out)
        if job.is_stream:
            job.sink._q.put(None if cancelled else result)
        elif cancelled:
            job.sink.cancel()
        elif job.sink.done():
            pass                       # the caller cancelled the Future itself
        elif failed:
            job.sink.set_exception(result)
        else:
            job.sink.set_result(result)

    def _take(self, job: _Job) -> None:
        """prompt of one request -> pool.submit (worker thread, GPU lock held)"""
        self._jobs[job.rid] = job
        text = job.text
        if job.max_split_batch is not None:
            try:
                from .core import split_sentences
                sents = split_sentences(text)
                if len(sents) == 0:
                    raise ValueError("split_text: the input holds no sentence")
            except Exception as e:
                self._resolve(job, e)
                return
            if len(sents) > 1:
                self._take_split(job, sents)
                return
            text = sents[0]               # one sentence: an ordinary request
        try:
            job.code_text = self.chat.normalizer(text, True, True, None)        # what Chat._infer does with do_text_normalization / homophones
            if job.refine is not None:       # stage 1: the refine-text pass, in the text pool (Chat._refine_text's prompt)
                ids, attn, _ = self.chat.refine_prompt([job.code_text], job.refine)
                self.text_pool.submit(job.rid, ids[0][attn[0].bool()], max_new_token=job.refine.max_new_token, params=job.refine)
                job.in_text_pool = True
                self.refine_admissions += 1
                return
        except Exception as e:        # this request's error, not the worker's
            self._resolve(job, e)
            return
        self._to_code(job)

    def _refined(self, rid, row: torch.Tensor) -> None:
        """a request's text row completed: hand it to the code pool (exactly once), as the text `Chat._infer` would synthesise"""
        if rid in self._sub:
            self._sentence_refined(rid, row)
            return
        job = self._jobs.get(rid)
        if job is None or not job.in_text_pool:
            return                        # cancelled or failed meanwhile
        job.in_text_pool = False
        try:
            if row.shape[0] == 0:         # the serial path's refine pass yields nothing there (gpt.py:570)
                raise RuntimeError(_NO_TEXT)
            job.code_text = self.chat.refined_text([row.cpu()])[0]
        except Exception as e:
            self._resolve(job, e)
            return
        self.handed += 1
        self._to_code(job)

    def _to_code(self, job: _Job) -> None:
        """the code-stage prompt of one normalised (or refined) text -> pool.submit"""
        kw, p = {}, job.params
        if job.is_stream:
            kw["stream"] = StreamSpec(int(p.stream_batch), int(p.stream_speed), int(p.pass_first_n_batches))
        try:
            self._code_submit(job.rid, job.code_text, p, **kw)
        except Exception as e:        # this request's error, not the worker's
            self._resolve(job, e)

    def _code_submit(self, key, t: str, params, **kw) -> None:
        chat = self.chat
        ids, attn, tmask = chat.code_prompt([t], params)
        emb = chat.prompt_embedding(ids, tmask, params, chat.tokenizer.spk_emb_ids)
        keep = attn[0].bool()
        self.pool.submit(key, ids[0][keep], tmask[0][keep], max_new_token=params.max_new_token, params=params, emb=emb[0][keep.to(emb.device)],
                         **kw)
        self.admissions += 1

    # -- split_text requests ------------------------------------------------------------------------------------------------
    def _take_split(self, job: _Job, sents: list) -> None:
        """a request of several sentences: normalise them like `Chat._infer`, then the text pool (refine) or stage A / B"""
        n, refine = len(sents), job.refine
        sp = _SplitReq(job, job.params, [None] * n, [None] * n, need_a=getattr(job.params, "spk_smp", None) is None)
        self._splits[job.rid] = sp
        self.split_requests += 1
        try:
            ts = [self.chat.normalizer(s_, True, True, None) for s_ in sents]
            if refine is None:
                sp.texts = ts
                self._split_advance(sp)
                return
            for i, t in enumerate(ts):      # the serial call refines the sentences as ONE batch: row i of n
                ids, attn, _ = self.chat.refine_prompt([t], refine)
                key = (job.rid, "r", i)
                self.text_pool.submit(key, ids[0][attn[0].bool()], max_new_token=refine.max_new_token, params=refine, row_offset=i, total_rows=n)
                self._sub[key] = sp
                sp.keys.add(key)
                self.refine_admissions += 1
        except Exception as e:
            self._fail_split(sp, e)

    def _split_advance(self, sp: _SplitReq) -> None:
        """submits what has become possible: stage A once sentence 0's text is there, stage B once every text and the speaker prompt are.
        Raises what the prompt builder or the pool raises (a sentence that does not fit a slot): the caller fails the request."""
        rid = sp.job.rid
        if sp.need_a and not sp.a_started and sp.texts[0] is not None:
            sp.a_started = True
            self._split_submit(sp, (rid, "A"), sp.texts[0], 0, GPT.n_vq)      # alone: a batch of one
        if not sp.b_started and (sp.a_done or not sp.need_a) and all(t is not None for t in sp.texts):
            sp.b_started = True
            for i, ((ro, tr), t) in enumerate(zip(split_rows(len(sp.texts), sp.job.max_split_batch), sp.texts)):
                self._split_submit(sp, (rid, i), t, ro, tr)
                self.split_sentences += 1

    def _split_submit(self, sp: _SplitReq, key, t: str, row_offset: int, total_rows: int) -> None:
        self._code_submit(key, t, sp.params, row_offset=row_offset, total_rows=total_rows)
        self._sub[key] = sp
        sp.keys.add(key)

    def _fail_split(self, sp: _SplitReq, e: BaseException) -> None:
        """fails ONE split request: every sentence of it leaves its pool (queued ones at once, resident ones at the next poll)"""
        self._drop_split(sp)
        self._resolve(sp.job, e)

    def _drop_split(self, sp: _SplitReq) -> None:
        for k in list(sp.keys):
            self._sub.pop(k, None)
            (self.text_pool if len(k) == 3 else self.pool).cancel(k)
        sp.keys.clear()
        self._splits.pop(sp.job.rid, None)

    def _sentence_refined(self, key, row: torch.Tensor) -> None:
        sp = self._sub.pop(key)
        sp.keys.discard(key)
        try:
            if row.shape[0] == 0:
                raise RuntimeError(_NO_TEXT)
            sp.texts[key[2]] = self.chat.refined_text([row.cpu()])[0]
            if all(t is not None for t in sp.texts):
                self.handed += 1
            self._split_advance(sp)
        except Exception as e:
            self._fail_split(sp, e)

    def _sentence_done(self, key, hid: torch.Tensor) -> Optional[_SplitReq]:
        """a stage-A / stage-B pool request completed -> the split request, once ALL its sentences are generated"""
        sp = self._sub.pop(key)
        sp.keys.discard(key)
        try:
            if hid.shape[0] == 0:       # (the serial call drops the whole split batch silently there)
                raise RuntimeError(_NO_AUDIO)
            if key[1] == "A":           # core.py:435-453: the refer sentence's audio becomes the speaker prompt of all sentences
                smp = self.chat.refer_speaker([hid], on_device=True)
                new = dict(spk_smp=smp, txt_smp=sp.texts[0])
                if dataclasses.is_dataclass(sp.params):
                    sp.params = dataclasses.replace(sp.params, **new)
                else:
                    sp.params = copy.copy(sp.params)
                    for k, v in new.items():
                        setattr(sp.params, k, v)
                sp.a_done = True
                self._split_advance(sp)
                return None
            sp.hids[key[1]] = hid
        except Exception as e:
            self._fail_split(sp, e)
            return None
        return sp if all(h is not None for h in sp.hids) else None

    def _finish_splits(self, ready: list, plain: list = ()) -> None:
        """ONE decode for the split requests that completed at this poll (+ `plain`: (job, hid) of the ordinary requests of the same
        poll, each a group of one sentence): Chat.decode_split_to_pcm16"""
        live = [(job, [hid]) for job, hid in plain if hid.shape[0] > 0] + [(sp.job, sp.hids) for sp in ready]
        for job, hid in plain:
            if hid.shape[0] == 0:
                self._resolve(job, RuntimeError(_NO_AUDIO))
        for part in _file_parts(live):
            try:
                self._count_decode(len(part))
                results = self.chat.decode_split_to_pcm16([g for _, g in part], **_format_kw([job for job, _ in part]))
            except Exception as e:     # the decode failed: its requests fail, the worker goes on
                results = [e] * len(part)
            for (job, _), r in zip(part, results):
                self._resolve(job, r)

    def _drain(self, block: bool) -> bool:
        """moves arrived requests into the pool; False once close() was called"""
        while True:
            try:
                item = self._in.get(block=block, timeout=0.5 if block else None)
            except queue.Empty:
                return not self._stop
            if item is None:
                return False
            block = False
            with self.lock:
                if isinstance(item, _Cancel):
                    self._cancel(item.rid)
                else:
                    self._take(item)

    def _cancel(self, rid) -> None:
        """cancel(future) / SpeechStream.close(): the request leaves whichever pool it is in (every sentence of a split one)"""
        job = self._jobs.get(rid)
        if job is None:
            return
        sp = self._splits.get(rid)
        if sp is not None:
            self._drop_split(sp)
        else:
            (self.text_pool if job.in_text_pool else self.pool).cancel(rid)
        self._resolve(job, cancelled=True)

    def _serve_chunks(self, ev: StreamEvents) -> None:
        """the chunks of one poll: ONE window decode, every piece to its own stream's queue"""
        live = [c for c in ev.chunks if c[0] in self._jobs]
        if not live:
            return
        jobs = [self._jobs[c[0]] for c in live]
        try:
            if any(c[4] > c[3] for c in live):
                self.stream_decode_calls += 1
                self.max_stream_group = max(self.max_stream_group, len(live))
            self.stream_chunks += len(live)
            self.stream_resampled_chunks += sum(j.sample_rate is not None for j in jobs)
            self.companded += sum(j.encoding is not None for j in jobs)
            kw = _format_kw(jobs, "sample_rates", "encodings", "speeds")
            for j in jobs:                # a job's streams are opened at its first chunk: exactly those its options need
                if j.streams is None:
                    opts = dict(rate=j.sample_rate, speed=j.speed, pauses=j.pauses, compress=j.compress, limiter=j.limiter, limiter_gain=j.lm_gain,
                                flac=j.flac, adpcm=j.adpcm)
                    j.streams = StreamSet.open(self.chat.codec, **opts) if StreamSet.needed(**opts) else StreamSet()
            for st in STAGES:             # a stage some job of the poll is in: its handles, one entry per job, and its count
                hs = [j.streams.get(st.name) for j in jobs]
                if any(h is not None for h in hs):
                    kw[st.streams] = hs
                    if st.counter:
                        setattr(self, st.counter, getattr(self, st.counter) + sum(h is not None for h in hs))
            pieces = self.chat.decode_windows_pcm16(self.pool.hiddens, [c[1:] for c in live], **kw)
        except Exception as e:        # the decode failed: these streams fail, the worker and the other requests go on
            for job in dict.fromkeys(jobs):
                self.pool.cancel(job.rid)
                self._resolve(job, e)
            return
        for job, pcm in zip(jobs, pieces):
            job.sink._q.put(pcm)

    def _between(self):
        self.max_coresident = max(self.max_coresident, len(self.pool.active))
        if self._splits:
            per: dict = {}
            for v in self.pool.active.values():
                k = getattr(v[0], "rid", v[0])
                if isinstance(k, tuple) and len(k) == 2 and k[1] != "A" and k in self._sub:
                    per[k[0]] = per.get(k[0], 0) + 1
            self.split_max_coresident = max([self.split_max_coresident, *per.values()])
        self.lock.release()           # one decode chunk done: a streamed request may take the GPU now
        time.sleep(0)
        self._drain(block=False)
        self.lock.acquire()

    def finish(self, hid: torch.Tensor, sample_rate=None, encoding=None, speed=None, flac: bool = False, loudness=None,
               pauses=None, limiter: bool = False, adpcm: bool = False, compress=None, eq=None) -> np.ndarray:
        """the serial server's path for one utterance (Chat.infer, pcm16, split_text): decode -> sample-level strip -> float_to_int16"""
        from .audio import float_to_int16
        if hid.shape[0] == 0:
            raise RuntimeError(_NO_AUDIO)
        self._count_decode(1)
        kw = option_kw({"sample_rate": [sample_rate], "speed": [speed], "loudness": [loudness], "pauses": [pauses], "limiter": [bool(limiter)],
                        "compress": [compress], "eq": [eq]})
        wav = self.chat.decode_to_wavs([hid], **{k: v[0] for k, v in kw.items()})[0]
        pcm = float_to_int16(wav[np.abs(wav) > np.float32(1e-5)])
        if flac:                                                            # converted on the host, encoded by the host twin
            return np.frombuffer(FLAC.encode(pcm, 24000 if sample_rate is None else int(sample_rate)), np.uint8)
        if adpcm:                                                           # likewise
            return ADPCM.encode_result(pcm, 24000 if sample_rate is None else int(sample_rate))
        return pcm if encoding is None else G711.encode(pcm, encoding)      # converted on the host, companded by the host twin

    def finish_group(self, hids: List[torch.Tensor], sample_rates=None, encodings=None, speeds=None, flac=None, loudness=None,
                     pauses=None, limiter=None, adpcm=None, compress=None, eq=None) -> list:
        """ragged_decode: the requests of one poll in ONE decode, each as if alone -> per request its int16 waveform (what `finish`
        returns for it) or the exception that fails it alone (an empty result).  `sample_rates`: one rate per request (None: 24000);
        `speeds`: one speed per request (None: 1.0); `loudness`: one target per request (None entries: left alone); `pauses`: one spec
        per request (None entries: copied through the one `trim_pauses` call); `limiter`: one flag per request; `flac`, `adpcm`: one flag per request (no request has both);
        `compress`: one spec per request (None entries: copied through the one `compress` call); `eq`: one equaliser spec per request
        (None entries: copied through the one `equalize` call)"""
        out: list = [RuntimeError(_NO_AUDIO) if h.shape[0] == 0 else None for h in hids]
        live = [i for i, h in enumerate(hids) if h.shape[0] > 0]
        if live:
            self._count_decode(len(live))
            kw = option_kw({"sample_rate": sample_rates, "encoding": encodings, "speed": speeds, "flac": flac, "loudness": loudness,
                            "pauses": pauses, "limiter": limiter, "adpcm": adpcm, "compress": compress, "eq": eq}, rows=live)
            for i, pcm in zip(live, self.chat.decode_to_pcm16([hids[i] for i in live], ragged=True, **kw)):
                out[i] = pcm
        return out

    def _count_decode(self, n: int) -> None:
        self.decode_calls += 1
        self.decoded += n
        self.max_decode_group = max(self.max_decode_group, n)

    def _pools_failed(self, e: BaseException) -> None:
        """a pool itself failed: the requests in flight fail, fresh pools serve the next ones"""
        self.log.error("slot pool failed: %s", e)
        for job in list(self._jobs.values()):
            self._resolve(job, e)
        for p in (self.text_pool, self.pool):
            close = getattr(p, "close", None)
            if close is not None:
                close()
        self.pool = self._make_pool()
        if self.refine:
            self.text_pool = self._make_text_pool()

    def _loop(self):
        while self._drain(block=True) or self.pool.queue:
            if not self.pool.queue:
                continue
            self.lock.acquire()
            try:
                if self.streams:
                    it = self.pool.run(between=self._between, grouped=self.ragged_decode, events=True)
                else:
                    it = self.pool.run(between=self._between, grouped=True) if self.ragged_decode else self.pool.run(between=self._between)
                while True:
                    try:
                        got = next(it)
                    except StopIteration:
                        break
                    except Exception as e:
                        self._pools_failed(e)
                        break
                    self._handle(got)
            finally:
                self.lock.release()

    def _handle(self, got) -> None:
        """one item of the code pool's output: the due chunks of a poll, or finished requests (one, or the group of a poll)"""
        if isinstance(got, StreamEvents):
            self._serve_chunks(got)
            return
        ready, plain = [], []          # split requests that became complete; (job, hidden states) of the ordinary finished requests
        for rid, _, hid in (got if self.ragged_decode else [got]):
            if rid in self._sub:       # a sentence of a split request: collected until its request is complete
                sp = self._sentence_done(rid, hid)
                if sp is not None:
                    ready.append(sp)
                continue
            job = self._jobs.get(rid)
            if job is None:
                continue               # cancelled or failed meanwhile
            if job.is_stream:          # a stream's result: its chunks went out already
                self._resolve(job, RuntimeError(_NO_AUDIO) if hid.shape[0] == 0 else None)
            else:
                plain.append((job, hid))
        if not self.ragged_decode:     # every request alone
            for job, hid in plain:
                try:
                    pcm = self.finish(hid, **{k: v[0] for k, v in _format_kw([job]).items()})
                except Exception as e:
                    pcm = e
                self._resolve(job, pcm)
            if ready:
                self._finish_splits(ready)
        elif ready:                    # one decode for everything that finished at this poll
            self._finish_splits(ready, plain)
        elif plain:
            for part in _file_parts(plain):
                try:
                    results = self.finish_group([hid for _, hid in part], **_format_kw([job for job, _ in part], "sample_rates", "encodings", "speeds"))
                except Exception as e:     # the group's decode failed: its requests fail, the worker goes on
                    results = [e] * len(part)
                for (job, _), r in zip(part, results):
                    self._resolve(job, r)

    def _loop2(self):
        """refine=True: ONE worker over the text pool and the code pool.  Every iteration: let other GPU users in and take arrived
        requests (`_between`), then enqueue one chunk of EVERY pool that has work -- each on its own stream -- and only then wait:
        for the previous poll's results, then for the oldest snapshot of each.  A finished text row goes to the code pool at once
        and is admitted there at the next iteration."""
        def busy():
            return self.text_pool.busy() or self.pool.busy()
        while self._drain(block=True) or busy():
            if not busy():
                continue
            self.lock.acquire()
            try:
                while busy():
                    self._between()
                    try:
                        live = [p for p in (self.text_pool, self.pool) if p.busy()]      # only the pools that have work
                        n_live = sum(bool(p.launch()) for p in live)
                        self.both_live_polls += int(n_live == 2)
                        self.refine_max_coresident = max(self.refine_max_coresident, len(self.text_pool.active))
                        for p in live:
                            for got in p.results(self.ragged_decode and p is self.pool):
                                self._route(p, got)
                        for p in live:
                            for got in p.poll(self.streams and p is self.pool):
                                self._route(p, got)
                    except Exception as e:
                        self._pools_failed(e)
                        break
            finally:
                self.lock.release()

    def _route(self, pool, got) -> None:
        if pool is self.text_pool:
            self._refined(got[0], got[1])
        else:
            self._handle(got)

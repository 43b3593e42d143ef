"""Host side of the hot path: weight repacking, per-call device state, the generate loop
(mirror of `GPT.generate`, /root/reference/ChatTTS/model/gpt.py:316-618) and the acoustic decoder
(mirror of `Chat._decode_to_wavs`, /root/reference/ChatTTS/core.py:513-539).

PyTorch is used for device memory, streams and host<->device copies only; every arithmetic op of
the path runs in libchattts_amd.so (hand-written gfx950 kernels) through the C ABI in
include/chattts_amd.h.  There is no eager/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import logging
import math
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import adpcm as ADPCM
from . import compressor as CP
from . import equalizer as EQ
from . import flac as FLAC
from . import g711 as G711
from . import loudness as LN
from . import limiter as LM
from . import outchain as OC
from . import pauses as PA
from . import resample as RS
from . import statepool as SP
from . import timescale as TS
from . import winchain as WC
from ._sync import wait_event, wait_stream
from .config import DVAE, GPT, VOCOS
from .rng import ExpDraws, penalty_table
from .weights import fold_weight_norm, gpt_layer_count

log = logging.getLogger("chattts_amd")


def device_scratch(nbytes: int, device) -> torch.Tensor:
    """The ONE place that allocates memory the library carves itself: every workspace (`ctts_*_workspace_bytes`) and every stage
    scratch (`ctts_*_scratch_bytes`) of this package comes from here, as `nbytes` uninitialised bytes on `device`.  The library may
    assume nothing about their contents.  Callers reach it as `engine.device_scratch` (a module attribute looked up per call), so a
    test can replace it and hand out guarded, pre-filled memory of exactly the declared size (tests/ws_arena.py)."""
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------------------
# logits-processor descriptors (mirror of gen_logits, /root/reference/ChatTTS/model/processors.py:38-58)
# ---------------------------------------------------------------------------------------------
@dataclass
class RepetitionPenalty:          # CustomRepetitionPenaltyLogitsProcessorRepeat, processors.py:6-35
    penalty: float
    max_input_ids: int
    past_window: int = 16


@dataclass
class TopP:                       # transformers TopPLogitsWarper(top_p, min_tokens_to_keep=3)
    top_p: float
    min_tokens_to_keep: int = 3


@dataclass
class TopK:                       # transformers TopKLogitsWarper(top_k, min_tokens_to_keep=3)
    top_k: int
    min_tokens_to_keep: int = 3


def gen_logits(num_code: int, top_P=0.7, top_K=20, repetition_penalty=1.0):
    """Same signature / return shape as the reference's `gen_logits` (processors.py:38-58); returns
    descriptors the fused sampling kernel understands instead of Python callables."""
    warpers, procs = [], []
    if top_P is not None:
        warpers.append(TopP(top_P, 3))
    if top_K is not None:
        warpers.append(TopK(top_K, 3))
    if repetition_penalty is not None and repetition_penalty != 1:
        procs.append(RepetitionPenalty(repetition_penalty, num_code, 16))
    return warpers, procs


@dataclass
class SamplingPlan:
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    penalty: Optional[float] = None


def plan_from_processors(processors: Sequence, infer_text: bool = False) -> SamplingPlan:
    """Accepts this module's descriptors AND the reference's own objects (duck-typed on the attribute
    names of transformers' warpers / the reference's penalty class).  Anything else cannot be fused
    into the kernel and is rejected loudly.  Order must be penalty -> top-p -> top-k (core.py:649)."""
    plan = SamplingPlan()
    stage = 0
    for p in processors:
        if hasattr(p, "penalty") and hasattr(p, "past_window"):
            if infer_text:
                # the reference's processor receives [B, n, 1] histories in text mode (gpt.py:477-485) and its
                # one_hot(...).sum(1) then broadcasts [B,V] against [B,1,V]: it only works because refine-text
                # defaults to repetition_penalty = 1.0, which creates no processor (processors.py:52)
                raise NotImplementedError("refine-text mode supports repetition_penalty = 1.0 only (reference default)")
            if stage > 0 or p.past_window != 16 or p.max_input_ids != GPT.n_audio - 1:
                raise NotImplementedError("repetition penalty must come first with past_window=16, max_input_ids=625")
            plan.penalty = float(p.penalty)
            stage = 1
        elif hasattr(p, "top_p"):
            if stage > 1 or getattr(p, "min_tokens_to_keep", 3) != 3:
                raise NotImplementedError("top-p must precede top-k and use min_tokens_to_keep=3")
            plan.top_p = float(p.top_p)
            stage = 2
        elif hasattr(p, "top_k"):
            if getattr(p, "min_tokens_to_keep", 3) != 3:
                raise NotImplementedError("top-k must use min_tokens_to_keep=3")
            plan.top_k = int(p.top_k)
            stage = 3
        else:
            raise NotImplementedError(f"logits processor {type(p).__name__} cannot be fused into the HIP sampling kernel")
    return plan


@dataclass(repr=False, eq=False)
class GenerationOutputs:          # gpt.py:276-285
    ids: List[torch.Tensor]
    attentions: list
    hiddens: List[torch.Tensor]

    def destroy(self):
        self.ids.clear()
        self.attentions.clear()
        self.hiddens.clear()


class RowList(list):
    """The per-utterance rows of a result (what the reference hands around as a plain list) that are VIEWS of one zero-padded
    [B, Tmax, ...] tensor, `padded` -- the batch `Chat._decode_to_wavs` would rebuild from them row by row (core.py:525-533).
    `CodecEngine.decode_to_wavs` takes it as is; any list operation (slicing, copying) yields a plain list and the generic path."""
    padded: Optional[torch.Tensor] = None


class Context:                    # gpt.py:103-111
    def __init__(self):
        self._interrupt = False

    def set(self, v: bool):
        self._interrupt = v

    def get(self) -> bool:
        return self._interrupt


class _EventGroup:
    """several CUDA events waited on as one"""

    def __init__(self, evs):
        self.evs = evs

    def synchronize(self):
        for e in self.evs:
            wait_event(e)


def cu_masked_stream(lib, dev, first: int, n: int, stride: int, complement: bool) -> "torch.cuda.Stream":
    """a HIP stream confined to CUs first, first + stride, ... (n of them) -- or to every OTHER CU (complement): ctts_stream_create_cu_mask"""
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(lib.ctts_stream_create_cu_mask(first, n, stride, 1 if complement else 0, C.byref(h)), "ctts_stream_create_cu_mask")
    return torch.cuda.ExternalStream(h.value, device=dev)


def codec_cu_spec():
    """CTTS_CODEC_CUS="n[:stride[:first]]" -> (first, n, stride) or None"""
    spec = os.environ.get("CTTS_CODEC_CUS", "")
    if not spec:
        return None
    parts = [int(v) for v in spec.split(":")]
    return (parts[2] if len(parts) > 2 else 0), parts[0], (parts[1] if len(parts) > 1 else 1)


def left_pad_starts(attention_mask: torch.Tensor) -> torch.Tensor:
    """kv_start[b] = number of leading zeros; raises unless the mask is left padding (tokenizer.py:73-110)."""
    m = attention_mask.to(torch.bool).cpu()
    T = m.shape[1]
    n = m.sum(1)
    start = T - n
    ar = torch.arange(T)[None, :]
    if not torch.equal(m, ar >= start[:, None]):
        raise NotImplementedError("only left-padded attention masks (what Tokenizer.encode produces) are supported")
    if int(n.min()) <= 0:
        raise ValueError("empty prompt row")
    return start.to(torch.int32)


def rope_row_perm() -> torch.Tensor:
    """Row order of q_proj / k_proj inside wqkv in perf mode: within every head the 16-row tiles hold
    dims [8t..8t+7] followed by [32+8t..32+8t+7], so that the two halves of a rotate-half pair land in
    the same 16-column MFMA tile of the QKV kernel and RoPE + KV append run in its epilogue."""
    idx = []
    for h in range(GPT.n_heads):
        for t in range(4):
            idx += [h * 64 + 8 * t + i for i in range(8)] + [h * 64 + 32 + 8 * t + i for i in range(8)]
    return torch.tensor(idx, dtype=torch.long)


def pack_frag(w: torch.Tensor) -> torch.Tensor:
    """[R, C] (R % 16 == 0, C % 32 == 0) -> the fragment-packed order of csrc/decode.hip,
    [R/16][C/32][lane = (c%32)/8 * 16 + r%16][c%8]: every (16-row tile, 32-column chunk) becomes one contiguous KiB (bf16)
    in exactly the lane order v_mfma_f32_16x16x32_bf16 reads its operand, so a wave's fragment load is ONE coalesced KiB
    instead of 64 scattered 16-byte pieces."""
    R, Cc = w.shape
    assert R % 16 == 0 and Cc % 32 == 0
    return w.reshape(R // 16, 16, Cc // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


X3_LO_SCALE = 2048.0


def split_f16(w: torch.Tensor):
    """float32 -> (hi, lo') float16: the "f32x3" operand format of the GPT projections (csrc/common.hpp x3_split): hi = fp16(w),
    lo' = fp16((w - hi) * 2^11), w = hi + lo' / 2^11 to 22 significant bits; inputs saturated at the fp16 range."""
    w = w.to(torch.float32).clamp(-65504.0, 65504.0)
    hi = w.to(torch.float16)
    lo = ((w - hi.to(torch.float32)) * X3_LO_SCALE).to(torch.float16)
    return hi, lo


def pack_frag_x3(w: torch.Tensor) -> torch.Tensor:
    """float32 [R, C] -> the SPLIT-fp16 planes of csrc/decode32x.hip: [2][R/16][C/32][64][8] float16, plane 0 = hi = fp16(w), plane 1 =
    lo' = fp16((w - hi) * 2^11) (w = hi + lo' / 2^11 to 22 significant bits), each plane in pack_frag's fragment order.  Three fp16 MFMAs
    (hi*hi; lo'*hi + hi*lo' on a second accumulator, x 2^-11; f32 accumulation) then stand for one float32 product."""
    hi, lo = split_f16(w)
    return torch.stack([pack_frag(hi), pack_frag(lo)], 0).contiguous()


def unpack_frag_x3(p: torch.Tensor, R: int, Cc: int) -> torch.Tensor:
    """planes -> float32 hi + lo' / 2048 (tests)"""
    return unpack_frag(p[0].float(), R, Cc) + unpack_frag(p[1].float(), R, Cc) / X3_LO_SCALE


def pack_wo_heads(wo: torch.Tensor) -> torch.Tensor:
    """o_proj.weight [768 out, 768 in] (bf16) -> [12 heads][8 (k / 8)][768 out][8] : the slice of Wo one attention head multiplies,
    laid out so that a wave's 16-byte loads (one output column per lane) are one contiguous KiB (csrc/gpt.hip attention_k<OPJ>)"""
    assert tuple(wo.shape) == (GPT.hidden, GPT.hidden)
    return wo.view(GPT.hidden, GPT.n_heads, 8, 8).permute(1, 2, 0, 3).contiguous()


def pack_frag32(w: torch.Tensor) -> torch.Tensor:
    """float32 twin of pack_frag for the parity mode (csrc/decode32.hip): [R, C] (R % 16 == 0, C % 16 == 0) ->
    [R/16][C/16][lane = (c%16)/4 * 16 + r%16][c%4], one contiguous KiB per (16-row tile, 16-column chunk) in the lane order of
    four consecutive v_mfma_f32_16x16x4_f32 steps."""
    R, Cc = w.shape
    assert R % 16 == 0 and Cc % 16 == 0
    return w.reshape(R // 16, 16, Cc // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous()


def unpack_frag32(p: torch.Tensor, R: int, Cc: int) -> torch.Tensor:
    """inverse of pack_frag32 (tests / debugging)"""
    return p.reshape(R // 16, Cc // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(R, Cc).contiguous()


def unpack_frag(p: torch.Tensor, R: int, Cc: int) -> torch.Tensor:
    """inverse of pack_frag (tests / debugging)"""
    return p.reshape(R // 16, Cc // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(R, Cc).contiguous()


def rope_tables(max_pos: int, head_dim: int = GPT.head_dim, theta: float = GPT.rope_theta):
    """cos/sin [max_pos, head_dim/2] float32, evaluated with the same torch f32 ops HF's
    LlamaRotaryEmbedding uses (inv_freq = 1/theta^(arange(0,d,2)/d); freqs = pos * inv_freq)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(torch.float32) / head_dim))
    pos = torch.arange(max_pos, dtype=torch.float32)
    freqs = pos[:, None] * inv_freq[None, :]
    return freqs.cos().contiguous(), freqs.sin().contiguous()


# ---------------------------------------------------------------------------------------------
class GptEngine:
    """Device-resident, repacked GPT weights + the generate loop."""

    NQ_RING = 64   # unseeded sampling: ring of per-step Exp(1) draws uploaded ahead of the GPU
    POLL = 16      # decode steps enqueued between two looks at the device-side finish flags
    # Stated bound on what the split-fp16 projections ("f32x3") move a PRE-temperature logit by, against the exact f32 kernels
    # under the same token history, RELATIVE to the head's logit scale (rms over the vocabulary of |W_v| * rms(final norm gain): the
    # standard deviation a logit has for a unit-rms hidden state; 4.02 for the synthetic checkpoint).  Measured with tools/x3_logit_bound.py
    # on the bench workload (all 64 rows, every step, teacher-forced on the reference's stream; profiles/r6o_x3_logit_bound_fp16split.log):
    # max |dlogit| 1.42e-5 = 3.5e-6 of the scale over 13.4 M logits (rms 3.5e-7; the bf16 split of round 5: 2.1e-5 / 3.3e-6), stated here
    # with a 1.5x allowance; re-measure on a trained checkpoint.  The certificate compares 2 * REL_ERR_X3 * scale / min(temperature) with the smallest decision margin of the call
    # (ctts_gen_state.margin).  What the same measurement says about LONG calls: the margins of the workload's 85,752 draws have density
    # ~0.8 per tempered-logit unit near 0 (smallest 1.3e-5), so ~10 draws sit below the bound: a worst-case bound flags several 500-step
    # utterances per batch although not one of the 85,752 draws actually differs between the two arithmetics (empirical rate on random
    # inputs: 1.3e-6 per draw, every divergence flagged: profiles/r6o_x3_flip_rate_fp16split.log).
    REL_ERR_X3 = 5.3e-6

    def __init__(self, gpt_sd: dict, embed_sd: dict, device: torch.device, dtype: str = "bf16",
                 max_pos: int = GPT.max_pos, logger: logging.Logger = log, rms_eps: float = GPT.rms_eps,
                 rope_theta: float = GPT.rope_theta, certify: Optional[bool] = None, exact_fallback: bool = False):
        """`dtype` names the arithmetic, explicitly:
          "f32"   -- the parity mode on float32 arithmetic throughout (f32-input MFMA, csrc/decode32.hip / prefill32.hip);
          "f32x3" -- the parity mode with the Llama projections on SPLIT-fp16 operands (csrc/decode32x.hip, prefill32x.hip: 22 significant
                     bits per operand, exact products, f32 accumulation -- measured closer to a float64 evaluation of the model than the
                     f32 MFMA kernels, profiles/r6p_f64_distance.log; attention, heads and sampling stay float32).  Same token ids as "f32" whenever no
                     draw of the call was decided by less than the arithmetic's logit error: every call computes its smallest decision
                     margin on the device (`certify`, default on in this mode; `last_stats["min_margin"]`, `["certified"]`).  With
                     `exact_fallback=True` the utterances whose margin is below the stated bound are generated again on the exact kernels
                     (both weight copies are resident): the result is then the "f32" engine's by construction.  OFF by default: the bound
                     is a worst case, long utterances almost always hold a draw below it (see REL_ERR_X3), and regenerating them costs
                     more than running "f32" in the first place -- a caller that needs the guarantee on long calls loads "f32";
          "bf16"  -- the perf mode (bf16 weights / KV / activations).
        `rms_eps` / `rope_theta` / `max_pos`: the run-time fields of `asset/gpt/config.json` (weights.check_gpt_config;
        `LlamaModel.from_pretrained`, gpt.py:75); everything else in that file is the geometry the kernels are compiled for."""
        if dtype not in ("bf16", "f32", "f32x3"):
            raise ValueError("dtype must be 'bf16' (perf), 'f32' (parity, exact float32) or 'f32x3' (parity, split-fp16 projections)")
        self.lib = _lib.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.EngineError("GptEngine needs a ROCm GPU device (there is no CPU path)")
        self.logger = logger
        self.dtype = dtype
        self.wdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.code = _lib.BF16 if dtype == "bf16" else _lib.F32
        self.n_layers = gpt_layer_count(gpt_sd)
        self.max_pos = max_pos
        dev = self.device
        f = lambda t: t.to(torch.float32).contiguous().to(dev)
        wcast = lambda t: t.to(torch.float32).to(self.wdt).contiguous().to(dev)
        self.wqkv, self.wo, self.wgu, self.wd, self.ln1, self.ln2 = [], [], [], [], [], []
        # perf mode folds the RMSNorm gains into the following projection (W' = W * gain[None, :], rounded to bf16
        # once at load): the kernels then only need the per-row 1/rms, applied in the GEMM epilogue.
        fold = (lambda w, g: w.float() * g.float()[None, :]) if dtype == "bf16" else (lambda w, g: w)
        perm = rope_row_perm() if dtype == "bf16" else torch.arange(GPT.hidden)
        for i in range(self.n_layers):
            p = f"layers.{i}."
            ln1, ln2 = gpt_sd[p + "input_layernorm.weight"], gpt_sd[p + "post_attention_layernorm.weight"]
            self.wqkv.append(wcast(fold(torch.cat([gpt_sd[p + "self_attn.q_proj.weight"][perm], gpt_sd[p + "self_attn.k_proj.weight"][perm],
                                                   gpt_sd[p + "self_attn.v_proj.weight"]], 0), ln1)))
            self.wo.append(wcast(gpt_sd[p + "self_attn.o_proj.weight"]))
            self.wgu.append(wcast(fold(torch.cat([gpt_sd[p + "mlp.gate_proj.weight"], gpt_sd[p + "mlp.up_proj.weight"]], 0), ln2)))
            self.wd.append(wcast(gpt_sd[p + "mlp.down_proj.weight"]))
            self.ln1.append(f(gpt_sd[p + "input_layernorm.weight"]))
            self.ln2.append(f(gpt_sd[p + "post_attention_layernorm.weight"]))
        self.norm = f(gpt_sd["norm.weight"])
        self.emb_code = f(torch.stack([embed_sd[f"emb_code.{k}.weight"] for k in range(GPT.n_vq)], 0))
        self.emb_text = f(embed_sd["emb_text.weight"])
        self.heads = f(torch.cat([fold_weight_norm(embed_sd[f"head_code.{k}.parametrizations.weight.original0"].float(),
                                                   embed_sd[f"head_code.{k}.parametrizations.weight.original1"].float())
                                  for k in range(GPT.n_vq)], 0))
        self.head_text = f(fold_weight_norm(embed_sd["head_text.parametrizations.weight.original0"].float(),
                                            embed_sd["head_text.parametrizations.weight.original1"].float()))
        # logit scale of the two heads (see REL_ERR_X3): rms_v |W_v|_2 * rms(final norm gain)
        ng = float(self.norm.pow(2).mean().sqrt())
        self.logit_scale = {False: float(self.heads.pow(2).sum(1).mean().sqrt()) * ng, True: float(self.head_text.pow(2).sum(1).mean().sqrt()) * ng}
        cos, sin = rope_tables(max_pos, theta=rope_theta)
        self.rope_cos, self.rope_sin = cos.to(dev), sin.to(dev)
        self._arrs = [_lib.ptr_array(x) for x in (self.wqkv, self.wo, self.wgu, self.wd, self.ln1, self.ln2)]
        # a second copy of the four matrices in the fragment-packed order the DECODE kernels read (bf16: decode.hip, f32:
        # decode32.hip); the row-major copy stays for the prefill kernels (+0.38 GB / +0.75 GB of the 288 GB)
        # (CTTS_DEC_PACKED=0, the A/B switch back to the row-major decode kernels, skips building them)
        use_packed = os.environ.get("CTTS_DEC_PACKED", "1") != "0"
        self.certify = (dtype == "f32x3") if certify is None else bool(certify)
        self.exact_fallback = bool(exact_fallback) and dtype == "f32x3"
        pk = pack_frag if dtype == "bf16" else pack_frag32
        self.packed, self._pk_arrs = None, None
        rp = rope_row_perm().to(dev)
        qk_perm = torch.cat([rp, GPT.hidden + rp, 2 * GPT.hidden + torch.arange(GPT.hidden, device=dev)])
        # "f32x3" reads the packed f32 copies only on an exact call (the fallback of its certificate, generate(exact=True)): without
        # `exact_fallback` they are not built (0.75 GB, and the packing time at load) -- an exact call then runs the row-major f32
        # kernels, bit-identical results (test_packed_f32_decode_is_bit_identical_to_row_major)
        if use_packed and (dtype != "f32x3" or self.exact_fallback):
            self.packed = [[pk(t) for t in ws] for ws in (self.wqkv, self.wo, self.wgu, self.wd)]
            if dtype != "bf16":
                # the packed f32 QKV matrix carries the RoPE row permutation too (its decode kernel rotates in the epilogue); an
                # output column's dot product does not depend on where the column sits, so the parity arithmetic is untouched
                self.packed[0] = [pack_frag32(t[qk_perm]) for t in self.wqkv]
            self._pk_arrs = [_lib.ptr_array(x) for x in self.packed]
        # dtype "f32x3": decode step on split-fp16 operands (csrc/decode32x.hip): the four matrices once more as hi | lo' fp16 planes (the
        # float32 bytes again), the RMSNorm gains folded in before the split; the prompt pass splits the row-major f32 matrices in its
        # tile loader (csrc/prefill32x.hip)
        self.x3, self._x3_arrs = None, None
        if use_packed and dtype == "f32x3":
            gain = lambda w_, g_: w_.float() * g_.float()[None, :]
            self.x3 = [[pack_frag_x3(gain(t[qk_perm], g_)) for t, g_ in zip(self.wqkv, self.ln1)], [pack_frag_x3(t) for t in self.wo],
                       [pack_frag_x3(gain(t, g_)) for t, g_ in zip(self.wgu, self.ln2)], [pack_frag_x3(t) for t in self.wd]]
            self._x3_arrs = [_lib.ptr_array(x) for x in self.x3]
        # perf mode: o_proj once more, sliced per attention head -- the decode step folds o_proj + residual into the attention launch
        # a second, per-head copy of every o_proj (23.6 MB of bf16) only for the opt-in fused attention + o_proj launch (CTTS_ATT_OPROJ=1)
        self.wo_hd = [pack_wo_heads(t) for t in self.wo] if (use_packed and dtype == "bf16" and os.environ.get("CTTS_ATT_OPROJ") == "1") else None
        self._wo_hd_arr = None if self.wo_hd is None else _lib.ptr_array(self.wo_hd)

        def pad16(t):      # zero rows up to a multiple of 16: the padded columns of the last logits tile are never stored
            r = (-t.shape[0]) % 16
            return t if r == 0 else torch.cat([t, torch.zeros((r, t.shape[1]), dtype=t.dtype, device=t.device)], 0)
        self.heads_pk = pack_frag32(pad16(self.heads)) if use_packed else None
        self.head_text_pk = pack_frag32(pad16(self.head_text)) if use_packed else None
        w = _lib.GptWeights()
        w.n_layers, w.weight_dtype, w.kv_dtype, w.max_pos = self.n_layers, self.code, self.code, max_pos
        w.wqkv, w.wo, w.wgu, w.wd, w.ln1, w.ln2 = [C.cast(a, _lib.PP) for a in self._arrs]
        w.norm, w.emb_code, w.heads = self.norm.data_ptr(), self.emb_code.data_ptr(), self.heads.data_ptr()
        w.rope_cos, w.rope_sin = self.rope_cos.data_ptr(), self.rope_sin.data_ptr()
        w.rms_eps = float(rms_eps)
        w.emb_text, w.head_text, w.n_text = self.emb_text.data_ptr(), self.head_text.data_ptr(), GPT.n_text
        if self._pk_arrs is not None:
            w.wqkv_pk, w.wo_pk, w.wgu_pk, w.wd_pk = [C.cast(a, _lib.PP) for a in self._pk_arrs]
        w.heads_pk, w.head_text_pk = _lib.ptr(self.heads_pk), _lib.ptr(self.head_text_pk)
        if self._wo_hd_arr is not None:
            w.wo_hd = C.cast(self._wo_hd_arr, _lib.PP)
        if self._x3_arrs is not None:
            w.wqkv_x3, w.wo_x3, w.wgu_x3, w.wd_x3 = [C.cast(a, _lib.PP) for a in self._x3_arrs]
        self._w = w
        h = C.c_void_p()
        _lib.check(self.lib.ctts_gpt_create(C.byref(h), C.byref(w)), "ctts_gpt_create")
        self.handle = h
        # CTTS_GPT_COMPLEMENT=1 (with CTTS_CODEC_CUS): the generator's stream runs on every CU EXCEPT the acoustic decoder's side-stream CUs
        spec = codec_cu_spec() if os.environ.get("CTTS_GPT_COMPLEMENT") == "1" else None
        self.stream = cu_masked_stream(self.lib, dev, *spec, True) if spec else torch.cuda.Stream(device=dev)
        self._lane_res = [(self.handle, self.stream)]
        self._lane_res_alt = []
        self._lane_res_text = []
        self.default_lanes = 1
        self.rng = "host"         # default source of the multinomial's Exp(1) draws: "host" (the reference's CPU stream) | "device"
        self.last_stats = {}
        self._session = None      # buffers + instantiated graph of the last generate() geometry (see generate)
        self._session_alt = None  # ... and of the last exact re-run of certificate-flagged utterances (kept apart: it must not evict the main one)
        self._session_text = None  # ... and of the last refine-text call: the default `Chat.infer` alternates text and code calls (core.py:341-360)
        self._draws_cache = None  # (key, ExpDraws) of the last seeded call: the constant Exp(1) tensor

    def __del__(self):
        try:
            for h, _ in [*getattr(self, "_lane_res", []), *getattr(self, "_lane_res_alt", []), *getattr(self, "_lane_res_text", [])]:
                self.lib.ctts_gpt_destroy(h)
            self._lane_res, self._lane_res_alt, self._lane_res_text = [], [], []
            self.handle = None
        except Exception:
            pass

    def weight_bytes_per_step(self) -> int:
        """HBM bytes of weights one decode step streams (190,698,240 params)."""
        es = 2 if self.dtype == "bf16" else 4
        per_layer = (3 * 768 * 768 + 768 * 768 + 2 * 3072 * 768 + 768 * 3072) * es
        return per_layer * self.n_layers + self.heads.numel() * 4

    # -- a2: Embed.forward (embed.py:52-79): gathers only, done with torch indexing on the device
    def embed_prompt(self, input_ids: torch.Tensor, text_mask: torch.Tensor) -> torch.Tensor:
        ids = input_ids.to(self.device)
        tm = text_mask.to(self.device).bool()
        et = self.emb_text[ids[..., 0].clamp(0, GPT.n_text - 1)]
        cid = ids.clamp(0, GPT.n_audio - 1)
        ec = self.emb_code[0][cid[..., 0]]
        for k in range(1, GPT.n_vq):
            ec = ec + self.emb_code[k][cid[..., k]]
        return torch.where(tm[..., None], et, ec).contiguous()

    # -- a3: GPT.generate
    def _lane_resources(self, n: int, pool: str = ""):
        """(handle, stream) pairs for n concurrent lanes; lane 0 of the main pool is the engine's own handle/stream.  `pool`: "" (code
        mode), "_alt" (the exact re-run of flagged utterances), "_text" (refine-text) -- a handle owns ONE captured decode graph, so every
        session slot decodes on handles of its own and none of them replaces another's graph."""
        pool = getattr(self, "_lane_res" + pool)
        while len(pool) < n:
            h = C.c_void_p()
            _lib.check(self.lib.ctts_gpt_create(C.byref(h), C.byref(self._w)), "ctts_gpt_create")
            pool.append((h, torch.cuda.Stream(device=self.device)))
        return pool[:n]

    def generate(self, emb: torch.Tensor, inputs_ids: torch.Tensor, temperature: torch.Tensor, eos_token: int = GPT.n_audio - 1,
                 attention_mask: Optional[torch.Tensor] = None, max_new_token: int = 2048, min_new_token: int = 0,
                 logits_processors: Sequence = (), infer_text: bool = False, return_attn: bool = False,
                 return_hidden: bool = False, stream: bool = False, show_tqdm: bool = False, ensure_non_empty: bool = True,
                 stream_batch: int = 24, manual_seed: Optional[int] = None, context: Optional[Context] = None,
                 *, use_graph: bool = True, stop_at: Optional[torch.Tensor] = None, row_offset: int = 0,
                 total_rows: Optional[int] = None, profile_tag: Optional[int] = None,
                 profile_stride: int = 1, lanes: Optional[int] = None,
                 teacher_ids: Optional[torch.Tensor] = None, prefill_chunk: Optional[int] = None,
                 return_sampled: bool = False, rng: Optional[str] = None, rng_seed: Optional[int] = None,
                 rng_nonce=None, row_ids: Optional[torch.Tensor] = None, exact: bool = False,
                 text_rng: Optional[str] = None) -> Iterator[GenerationOutputs]:
        """Drop-in for `GPT.generate` (gpt.py:316-337), code mode.  Extra keyword-only arguments:
        `use_graph` (hipGraph replay of the decode step), `stop_at` ([B] int32 forced output lengths,
        benchmark hook), `row_offset`/`total_rows` (this shard's position inside a data-parallel batch:
        keeps the CPU draw and the rows>=625 penalty quirk keyed on the global row index), `lanes`
        (the batch is cut into that many contiguous row groups, each decoding on its own HIP stream
        with its own captured graph; utterances never interact, so the result is identical, while the
        per-kernel launch / dependent-load latency of one lane overlaps the others' kernels), `teacher_ids`
        ([B, max_new_token, 4] int64: teacher forcing -- the token written at step i is teacher_ids[:, i] instead of
        the sampled one; evaluation hook used to bound the bf16 mode's drift on the reference's token stream),
        `prefill_chunk` (tokens: the prompt is prefilled in pieces of that many slots -- `ctts_gpt_prefill_chunk` -- which
        bounds the activation workspace of a long prompt such as an `spk_smp` audio-code prompt, core.py:435-453: the workspace is
        then sized for a piece, not for the whole prompt), `return_sampled` (evaluation hook, the companion of `teacher_ids`: after
        the call `self.last_sampled` holds, per utterance, the [T_b, 4] tokens the sampler itself drew at every step before teacher
        forcing replaced them -- the teacher-forced token agreement of a numeric mode), `rng` ("host" | "device", default
        `self.rng` = "host"): where the Exp(1) draws of the multinomial come from.  "host" is the parity contract -- the reference's
        CPU generator call, uploaded (rng.py).  "device" draws them inside the sampling kernel (Philox4x32-10, counter = token / global
        row / step; the reference on a GPU device draws from the device generator too, gpt.py:39): with `manual_seed=None` -- the
        reference's DEFAULT -- that removes the ~2 ms per-step host draw + upload; the key is `rng_seed` or, if None, one draw from
        torch's global CPU generator (so `torch.manual_seed` still makes a run repeatable).  Code mode only: a refine-text call
        (`infer_text=True`) keeps the host stream whatever `rng` / `self.rng` say, unless `text_rng="device"` opts THAT call in (one
        sampling row per utterance, a seeded call draws with step word 0 as in code mode; what a text-mode slot pool with the device
        generator draws, serving.SlotPool(infer_text=True)).  `rng_nonce` (device generator
        only; an int or one int per utterance): the fourth word of the generator's counter instead of its constant -- a slot pool gives
        every admission its own (serving.SlotPool), and passing a request's number here reproduces that request in isolation.
        `row_ids` ([B] ints, with `total_rows`): the GLOBAL utterance index of every row of this call when they are not the contiguous
        block `row_offset` describes (a length-balanced data-parallel shard, dist.infer_sharded; the exact re-run below): the Exp(1) draw
        of row b is the full-batch draw's row, and the rows >= 625 penalty quirk / device generator are keyed on it.  `exact` (dtype
        "f32x3" only): this call's decode steps on the exact f32 kernels.
        PARITY CERTIFICATE (`self.certify`, default in "f32x3"): after the call `last_stats["min_margin"]` is the smallest decision margin
        of any step of any utterance in tempered-logit units (include/chattts_amd.h, ctts_gen_state.margin), `last_stats["margin_bound"]` =
        2 * REL_ERR_X3 * logit_scale / min(temperature), `last_margins` the per-utterance minima.  Utterances below the bound: a warning, and
        (`self.exact_fallback`, non-streaming calls) they are generated again on the exact kernels and replace their rows of the result."""
        if return_attn:
            raise NotImplementedError("return_attn is not supported by the fused attention kernel")
        context = context or Context()
        plan = plan_from_processors(logits_processors, infer_text)
        lib, dev = self.lib, self.device
        B, T, nvq = inputs_ids.shape
        assert nvq == GPT.n_vq and emb.shape == (B, T, GPT.hidden)
        nrow = 1 if infer_text else nvq                   # sampling rows per utterance (gpt.py:459-464 vs :439-440)
        V = GPT.n_text if infer_text else GPT.n_audio
        max_new = int(max_new_token)
        if T + max_new > self.max_pos:
            raise ValueError(f"T + max_new_token = {T + max_new} exceeds max_position_embeddings {self.max_pos}")
        if attention_mask is None:
            attention_mask = torch.ones((B, T), dtype=torch.bool)
        kv_start_all = left_pad_starts(attention_mask)
        n_lanes = self.default_lanes if lanes is None else int(lanes)
        n_lanes = max(1, min(n_lanes, B))
        exact = bool(exact) and self.x3 is not None      # (the other modes have one arithmetic)
        certify = self.certify and teacher_ids is None
        rng_state0 = torch.get_rng_state() if (manual_seed is None and self.exact_fallback and not exact) else None
        rid = None
        if row_ids is not None:
            rid = torch.as_tensor(row_ids, dtype=torch.int64).reshape(-1).cpu()
            assert rid.numel() == B and total_rows is not None, "row_ids needs one global index per utterance and total_rows"
        if profile_tag is not None or not use_graph:
            n_lanes = 1
        from .dist import shard_bounds
        bounds = [shard_bounds(B, n_lanes, i) for i in range(n_lanes)]
        slot_sfx = "_alt" if exact else ("_text" if infer_text else "")
        res = self._lane_resources(n_lanes, slot_sfx)
        caller = torch.cuda.current_stream(dev)
        # seeded sampling re-seeds the CPU generator at every step (gpt.py:504-507): ONE constant tensor per (seed, batch
        # geometry).  Drawing it costs ~4 ms of host time per 256 rows (30 ms for the 2048 rows of an 8-GPU batch), so the
        # last one is kept across calls.
        rng_mode = rng or self.rng
        if rng_mode not in ("host", "device"):
            raise ValueError("rng must be 'host' or 'device'")
        if text_rng not in (None, "host", "device"):
            raise ValueError("text_rng must be 'host' or 'device'")
        # refine-text keeps the host stream unless the call opts in
        device_rng = (text_rng == "device") if infer_text else rng_mode == "device"
        dkey = (total_rows if total_rows is not None else B * nrow, V, manual_seed, row_offset, B * nrow, None if rid is None else tuple(rid.tolist()))
        if device_rng:
            draws = None
            seed_val = int(rng_seed) if rng_seed is not None else (int(manual_seed) if manual_seed is not None
                                                                    else int(torch.randint(0, 2 ** 62, (1,)).item()))
        elif manual_seed is not None and self._draws_cache is not None and self._draws_cache[0] == dkey:
            draws = self._draws_cache[1]
        else:
            srows = None if rid is None else (rid[:, None] * nrow + torch.arange(nrow)[None, :]).reshape(-1)
            draws = ExpDraws(dkey[0], V, manual_seed, row_begin=row_offset, row_end=row_offset + B * nrow, rows=srows)
            self._draws_cache = (dkey, draws) if draws.constant else None
        const_q = device_rng or draws.constant      # no per-step host draw / upload
        ptab = penalty_table(plan.penalty)
        nq = 1 if const_q else self.NQ_RING
        emb_all = emb.to(torch.float32).contiguous().to(dev)
        ids_all = inputs_ids.to(dev)
        temp_d = temperature.to(torch.float32).reshape(-1).to(dev)
        assert temp_d.numel() == nrow, "temperature must have one entry per sampling row of an utterance"
        ptab_d = None if ptab is None else ptab.to(dev)
        wait_stream(caller)  # inputs above were produced on the caller's stream

        class Lane:
            pass

        # ---- session reuse: a call with the same geometry and sampling constants as the previous one keeps that call's
        # device buffers AND its instantiated decode graph (every pointer and by-value field the captured kernels hold is
        # then unchanged); only buffer contents are re-initialised, stream-ordered on the lane's stream.  The first
        # replays of a freshly instantiated graph cost ~17 ms at B = 64 (tools/ttfs_probe.py), which a serving loop or a
        # second batch of the same shape should not pay again.  Results are handed out as copies (see outputs()).
        top_p_thr = float(np.float32(1.0 - plan.top_p)) if plan.top_p is not None else 0.0
        key = (tuple(bounds), T, max_new, nrow, V, nq, self.dtype, top_p_thr, plan.top_p is not None, int(plan.top_k or 0),
               plan.top_k is not None, int(min_new_token), int(eos_token), int(row_offset), bool(infer_text), stop_at is not None,
               ptab is not None, teacher_ids is not None, bool(return_sampled),
               None if prefill_chunk is None else int(prefill_chunk), device_rng, manual_seed is None, device_rng and rng_nonce is not None,
               exact, certify, rid is not None)
        # three slots: code mode, the exact re-run, refine-text -- an exact re-run keeps the main call's session (and graph) alive, and
        # the text / code calls the default `Chat.infer` alternates between each find theirs from the previous request
        slot = "_session" + slot_sfx
        sess = getattr(self, slot)
        sess = sess if (sess is not None and sess["key"] == key) else None
        if sess is None:
            setattr(self, slot, None)     # drop the previous session's buffers before allocating new ones
            sess = dict(key=key, lanes=[], graph=False, temp=torch.empty((nrow,), dtype=torch.float32, device=dev),
                        ptab=None if ptab is None else torch.empty_like(ptab, device=dev), q_sig=None,
                        seed=torch.zeros((1,), dtype=torch.int64, device=dev))
            for (lo, hi), (handle, st) in zip(bounds, res):
                ln = Lane()
                ln.lo, ln.hi, ln.handle, ln.st = lo, hi, handle, st
                Bl = hi - lo
                with torch.cuda.stream(st):
                    ln.ids_buf = torch.empty((Bl, T + max_new, nvq), dtype=torch.int64, device=dev)  # gpt.py:372-379
                    ln.len_d = torch.empty((Bl,), dtype=torch.int32, device=dev)
                    # finish flags and end_idx live in ONE padded device block (16-byte granules: [Bp] uint8 | [Bp] int32) so that a
                    # poll is one shader copy of it into pinned host memory (ctts_copy_bytes) -- see snapshot()
                    Bp = (Bl + 15) // 16 * 16
                    ln.state_blk = torch.zeros((5 * Bp,), dtype=torch.uint8, device=dev)
                    ln.finish = ln.state_blk[:Bl]                                             # gpt.py:346
                    ln.order = torch.empty((Bl,), dtype=torch.int32, device=dev)              # visiting order of the device-side compaction
                    ln.n_active = torch.empty((1,), dtype=torch.int32, device=dev)
                    ln.end_idx = ln.state_blk[Bp:].view(torch.int32)[:Bl]                     # gpt.py:343
                    ln.hiddens = torch.empty((Bl, max_new, GPT.hidden), dtype=torch.float32, device=dev)
                    kv_shape = (self.n_layers, Bl, GPT.n_heads, T + max_new, GPT.head_dim)
                    ln.kcache = torch.empty(kv_shape, dtype=self.wdt, device=dev)
                    ln.vcache = torch.empty(kv_shape, dtype=self.wdt, device=dev)
                    # the prefill carves for the rows it pushes through the layers at once (the whole prompt, or one chunk of it);
                    # the decode steps for one row per utterance
                    tc_ws = T if (prefill_chunk is None or int(prefill_chunk) >= T) else max(1, int(prefill_chunk))
                    ln.ws_bytes = max(lib.ctts_gpt_workspace_bytes(Bl, tc_ws), lib.ctts_gpt_workspace_bytes(Bl, 1))
                    ln.workspace = device_scratch(ln.ws_bytes, dev)
                    ln.kv_start = torch.empty((Bl,), dtype=kv_start_all.dtype, device=dev)
                    ln.stop_d = None if stop_at is None else torch.empty((Bl,), dtype=torch.int32, device=dev)
                    ln.q_d = torch.empty((1,) if device_rng else (nq, Bl * nrow, V), dtype=torch.float32, device=dev)
                    ln.teacher = None if teacher_ids is None else torch.empty((Bl, max_new, nvq), dtype=torch.int64, device=dev)
                    ln.sampled = torch.zeros((Bl, max_new, nvq), dtype=torch.int64, device=dev) if return_sampled else None
                    ln.nonce = torch.zeros((Bl,), dtype=torch.int32, device=dev) if (device_rng and rng_nonce is not None) else None
                    ln.margin = torch.empty((Bl,), dtype=torch.float32, device=dev) if certify else None
                    ln.row_base = torch.empty((Bl,), dtype=torch.int32, device=dev) if rid is not None else None
                s = _lib.GenState()
                s.B, s.T, s.max_new = Bl, T, max_new
                s.ids_buf, s.len, s.kv_start = ln.ids_buf.data_ptr(), ln.len_d.data_ptr(), ln.kv_start.data_ptr()
                s.finish, s.end_idx, s.hiddens = ln.finish.data_ptr(), ln.end_idx.data_ptr(), ln.hiddens.data_ptr()
                s.kcache, s.vcache, s.q, s.nq = ln.kcache.data_ptr(), ln.vcache.data_ptr(), ln.q_d.data_ptr(), nq
                s.temperature = sess["temp"].data_ptr()
                s.pow_table = _lib.ptr(sess["ptab"])
                s.top_p_thr = top_p_thr
                s.use_top_p = int(plan.top_p is not None)
                s.top_k = int(plan.top_k or 0)
                s.use_top_k = int(plan.top_k is not None)
                s.min_new, s.eos = int(min_new_token), int(eos_token)
                s.row_offset = int(row_offset + lo * nrow)
                s.infer_text = int(infer_text)
                s.stop_at = _lib.ptr(ln.stop_d)
                s.teacher_ids = _lib.ptr(ln.teacher)
                s.sampled_ids = _lib.ptr(ln.sampled)
                s.rng_device, s.rng_per_step, s.rng_seed = int(device_rng), int(manual_seed is None), sess["seed"].data_ptr()
                s.rng_nonce = _lib.ptr(ln.nonce)
                s.margin, s.row_base, s.proj_exact = _lib.ptr(ln.margin), _lib.ptr(ln.row_base), int(exact)
                s.prefill_valid_rows = 0      # set per call below (the session is keyed on geometry, not on the mask)
                # compaction order: utterances by descending context = ascending left padding (contexts of a batch differ only by
                # the static valid prompt length), so the attention grid starts its longest units first.  CTTS_ORDER=0: ascending slot
                s.order = ln.order.data_ptr() if os.environ.get("CTTS_ORDER", "1") != "0" else None
                s.workspace, s.workspace_bytes = ln.workspace.data_ptr(), ln.ws_bytes
                # no row_map: the library compacts on the device -- the first kernel of every decode step ranks the utterances
                # whose finish flag is 0 and writes n_active (include/chattts_amd.h), so finished utterances leave the step
                # at once and the host only ever READS finish / end_idx
                s.row_map, s.n_active = None, ln.n_active.data_ptr()
                ln.s = s
                sess["lanes"].append(ln)
            setattr(self, slot, sess)
        L = sess["lanes"]
        q_sig = dkey if (draws is not None and draws.constant) else None
        for ln in L:
            lo, hi = ln.lo, ln.hi
            Bl = hi - lo
            ln.done, ln.end_snap = False, None
            ln.live_ub = Bl      # upper bound of the lane's live utterances: what the last collected finish poll saw (flags only go up)
            with torch.cuda.stream(ln.st):
                if sess.get("out_ev") is not None:
                    ln.st.wait_event(sess["out_ev"])   # the previous call's result copies have read these buffers
                ln.ids_buf.zero_()
                ln.ids_buf[:, :T] = ids_all[lo:hi]
                ln.len_d.fill_(T)
                ln.finish.zero_()
                ln.order.copy_(torch.argsort(kv_start_all[lo:hi].to(torch.int64), stable=True).to(torch.int32))
                ln.n_active.fill_(Bl)
                ln.end_idx.zero_()
                ln.kv_start.copy_(kv_start_all[lo:hi])
                # "f32x3": the prompt pass runs over the valid prompt tokens only (ctts_gen_state.prefill_valid_rows; whole-prompt prefill only)
                ln.s.prefill_valid_rows = int((T - kv_start_all[lo:hi].to(torch.int64)).sum()) if self.x3 is not None else 0
                if ln.stop_d is not None:
                    ln.stop_d.copy_(stop_at[lo:hi].to(torch.int32))
                if ln.margin is not None:
                    ln.margin.fill_(float("inf"))
                if ln.row_base is not None:
                    ln.row_base.copy_((rid[lo:hi] * nrow).to(torch.int32))
                if getattr(ln, "nonce", None) is not None:
                    nz = torch.as_tensor(rng_nonce, dtype=torch.int64).reshape(-1)
                    nz = nz.expand(B) if nz.numel() == 1 else nz
                    ln.nonce.copy_(nz[lo:hi].to(torch.int32))
                if ln.teacher is not None:
                    assert tuple(teacher_ids.shape) == (B, max_new, nvq)
                    ln.teacher.copy_(teacher_ids[lo:hi].to(torch.int64))
                ln.emb = emb_all[lo:hi].contiguous()
                if draws is not None and draws.constant and sess["q_sig"] != q_sig:
                    ln.q_d[0].copy_(draws.step(0)[lo * nrow: hi * nrow])
                if ln is L[0]:
                    if device_rng:
                        sess["seed"].fill_(seed_val)
                    sess["temp"].copy_(temp_d)
                    if ptab is not None:
                        sess["ptab"].copy_(ptab)
        sess["q_sig"] = q_sig
        if n_lanes > 1:   # temp / ptab were written on lane 0's stream
            ev0 = torch.cuda.Event()
            ev0.record(L[0].st)
            for ln in L[1:]:
                ln.st.wait_event(ev0)

        # ---- Exp(1) draws of the unseeded mode: the reference draws one [rows, V] tensor per step from torch's global
        # CPU generator (gpt.py:498-500).  That stream is serial (~2 ms per step at B=64, more than a decode step), so
        # a worker thread draws 32-step blocks ahead into two pinned buffers while the GPU consumes the previous block;
        # uploads are stream-ordered behind the launches that still read the ring half they overwrite (no host sync).
        half = nq // 2
        feeder = None
        if not const_q:
            from concurrent.futures import ThreadPoolExecutor
            feeder = dict(pool=ThreadPoolExecutor(max_workers=1), bufs=[torch.empty((half, B * nrow, V), dtype=torch.float32).pin_memory()
                                                                           for _ in range(2)],
                          evs=[None, None], fut=None, next_block=0, states=[])

            def draw_block(blk):
                buf = feeder["bufs"][blk % 2]
                if feeder["evs"][blk % 2] is not None:
                    e_ = feeder["evs"][blk % 2]                 # the H2D copy that last read this buffer is done
                    e_.synchronize() if isinstance(e_, _EventGroup) else wait_event(e_)
                feeder["states"].append((blk, torch.get_rng_state()))
                nthr = torch.get_num_threads()
                torch.set_num_threads(1)   # exponential_ is a serial stream; a 100+-thread OpenMP wake-up costs ~10 ms per call
                try:
                    n = min(half, max_new - blk * half)
                    for j in range(max(n, 0)):
                        draws.step_into(blk * half + j, buf[j])
                finally:
                    torch.set_num_threads(nthr)
                return blk

            feeder["fut"] = feeder["pool"].submit(draw_block, 0)
        uploaded = 0  # steps whose Exp(1) draws are on the device (unseeded mode only)

        def ensure_q(upto: int):
            nonlocal uploaded
            if feeder is None:
                return
            while uploaded < upto:
                blk = feeder["fut"].result()
                n = min(half, max_new - uploaded)
                buf = feeder["bufs"][blk % 2]
                slab = uploaded % nq
                evs = []
                for ln in L:
                    with torch.cuda.stream(ln.st):
                        ln.q_d[slab: slab + n].copy_(buf[:n, ln.lo * nrow: ln.hi * nrow], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(ln.st)
                        evs.append(ev)
                feeder["evs"][blk % 2] = evs[-1] if len(evs) == 1 else _EventGroup(evs)
                uploaded += n
                if uploaded < max_new:
                    feeder["fut"] = feeder["pool"].submit(draw_block, blk + 1)
                else:
                    feeder["fut"] = None

        def finish_rng(steps_reference: int):
            """Leave torch's global CPU generator exactly where the reference would: it draws once per executed step
            (the loop of gpt.py:394 stops at the step where the last row hits EOS), while the feeder ran ahead."""
            if feeder is None:
                return
            if feeder["fut"] is not None:
                feeder["fut"].result()
            feeder["pool"].shutdown(wait=True)
            blk = min(steps_reference // half, len(feeder["states"]) - 1)
            torch.set_rng_state(feeder["states"][blk][1])
            tmp = torch.empty((draws.total_rows, V), dtype=torch.float32)
            for _ in range(steps_reference - blk * half):
                tmp.exponential_(1)

        def outputs() -> GenerationOutputs:
            """Snapshot of the result so far.  Uses each lane's `end_snap` (host copy of end_idx taken by the last
            poll) and makes the caller's stream wait for the poll-time event only, so a chunk that was already
            enqueued behind the poll keeps running while the consumer (e.g. the DVAE/Vocos decode of a streamed
            prefix) works on the caller's stream -- the two overlap on the GPU."""
            ids, hid = [], []
            # copies, on the caller's stream behind the poll-time event: the session's buffers are reused by the next
            # call of the same geometry, results must not alias them
            with torch.cuda.stream(caller):
                if len(L) == 1 and max(L[0].end_snap, default=0) > 0:
                    # one lane (the default): ONE strided copy per result instead of one clone per row (128 launches for a batch of 64,
                    # ~1.5 ms of host time between the last decode step and the acoustic decoder); rows are views of the copies, the
                    # hidden states come zero padded -- the batch the decoder needs (RowList.padded)
                    ln = L[0]
                    e, nb = ln.end_snap, ln.hi - ln.lo
                    Tm = max(e)
                    caller.wait_event(ln.ev)
                    ids_all = (ln.ids_buf[:nb, T: T + Tm, 0] if infer_text else ln.ids_buf[:nb, T: T + Tm]).clone()   # gpt.py:297-301
                    ids = [ids_all[b, : e[b]] for b in range(nb)]
                    hid = RowList()
                    if return_hidden:                                                                                 # gpt.py:303-307
                        e_d = torch.tensor(e, dtype=torch.int32).to(dev, non_blocking=True)
                        keep = torch.arange(Tm, device=dev, dtype=torch.int32)[None, :] < e_d[:, None]
                        hid.padded = torch.where(keep[..., None], ln.hiddens[:nb, :Tm], ln.hiddens.new_zeros(()))
                        hid.extend(hid.padded[b, : e[b]] for b in range(nb))
                    sess["out_ev"] = torch.cuda.Event()
                    sess["out_ev"].record(caller)
                    return GenerationOutputs(ids=ids, attentions=[], hiddens=hid)
                for ln in L:
                    e = ln.end_snap
                    caller.wait_event(ln.ev)
                    if infer_text:
                        ids += [ln.ids_buf[b, T: T + e[b], 0].clone() for b in range(ln.hi - ln.lo)]   # gpt.py:300-301
                    else:
                        ids += [ln.ids_buf[b, T: T + e[b]].clone() for b in range(ln.hi - ln.lo)]      # gpt.py:297-299
                    if return_hidden:
                        hid += [ln.hiddens[b, : e[b]].clone() for b in range(ln.hi - ln.lo)]           # gpt.py:303-307
                sess["out_ev"] = torch.cuda.Event()
                sess["out_ev"].record(caller)
            return GenerationOutputs(ids=ids, attentions=[], hiddens=hid)

        sync_poll = os.environ.get("CTTS_SYNC_POLL") == "1"   # profiling fallback: plain blocking D2H polls, no pinned buffers

        def snapshot(ln):
            """stream-ordered, ASYNCHRONOUS D2H of the lane's finish flags and end_idx into pinned host buffers, plus the event
            that marks the copy (and everything enqueued before it) done.  Two buffer sets: up to two chunks are in flight."""
            k = ln.snap_i = (getattr(ln, "snap_i", 0) + 1) % 2
            Bl_, Bp_ = ln.hi - ln.lo, ln.state_blk.numel() // 5
            if not hasattr(ln, "snap_buf"):
                ln.snap_buf = []
                for _ in range(2):
                    blk = torch.empty((5 * Bp_,), dtype=torch.uint8).pin_memory()
                    ln.snap_buf.append((blk[:Bl_], blk[Bp_:].view(torch.int32)[:Bl_], torch.cuda.Event(), blk))
            fin_h, end_h, ev, blk = ln.snap_buf[k]
            with torch.cuda.stream(ln.st):
                if sync_poll:
                    fin_h.copy_(ln.finish.cpu())
                    end_h.copy_(ln.end_idx.cpu())
                else:
                    # a SHADER copy into the pinned block (one packet of the stream; no copy-engine hand-off behind the step's kernels)
                    _lib.check(lib.ctts_copy_bytes(blk.data_ptr(), ln.state_blk.data_ptr(), blk.numel(), ln.st.cuda_stream), "ctts_copy_bytes")
                ev.record(ln.st)
            return k

        def collect(ln, k):
            """wait for snapshot k; the reference keeps stepping finished rows until the last one is done (gpt.py:512-518,592)
            but cuts their output at end_idx -- here they left the step on the device the moment they finished"""
            fin_h, end_h, ev, _ = ln.snap_buf[k]
            wait_event(ev)
            ln.ev = ev
            ln.end_snap = end_h.tolist()
            ln.done = bool(fin_h.all())
            ln.live_ub = (ln.hi - ln.lo) - int(fin_h.sum())
            return fin_h.clone()

        def poll(ln):
            return collect(ln, snapshot(ln))

        def enqueue(n):
            """n decode steps on every unfinished lane; unseeded mode: in pieces that stay inside one block of the Exp(1) ring,
            so a block is uploaded only after every step that still reads the half it overwrites has been enqueued"""
            nonlocal steps_enq
            while n > 0:
                k = n if feeder is None else min(n, half - (steps_enq % half))
                ensure_q(steps_enq + k)
                for ln in L:
                    if ln.done:
                        continue
                    if graph_ok:
                        # opt-in: the step captured for a BOUND on the live rows (16-row buckets below the batch; include/chattts_amd.h
                        # ctts_gpt_graph_build_rows): finished utterances then cost no workgroups at all.  The bound is what the last
                        # COLLECTED poll saw -- one or two chunks old, and finish flags only go up -- so it holds for every step enqueued
                        # here; the kernels read the exact live count themselves, the bits do not depend on the bound.
                        Bl_ = ln.hi - ln.lo
                        rows = (max(ln.live_ub, 1) + 15) // 16 * 16 if rows_graphs else Bl_
                        if rows < Bl_:
                            if rows not in sess.setdefault("rows_built", [set() for _ in L])[L.index(ln)]:
                                _lib.check(lib.ctts_gpt_graph_build_rows(ln.handle, C.byref(ln.s), rows, ln.st.cuda_stream), "ctts_gpt_graph_build_rows")
                                sess["rows_built"][L.index(ln)].add(rows)
                            _lib.check(lib.ctts_gpt_graph_launch_rows(ln.handle, k, rows, ln.st.cuda_stream), "ctts_gpt_graph_launch_rows")
                        else:
                            _lib.check(lib.ctts_gpt_graph_launch(ln.handle, k, ln.st.cuda_stream), "ctts_gpt_graph_launch")
                    else:
                        for _ in range(k):
                            _lib.check(lib.ctts_gpt_decode_step(ln.handle, C.byref(ln.s), ln.st.cuda_stream), "ctts_gpt_decode_step")
                steps_enq += k
                n -= k

        # ---- step 0: prefill ----
        ensure_q(1)
        for ln in L:
            if prefill_chunk is None or int(prefill_chunk) >= T:
                _lib.check(lib.ctts_gpt_prefill(ln.handle, C.byref(ln.s), ln.emb.data_ptr(), ln.st.cuda_stream), "ctts_gpt_prefill")
            else:
                tc = max(1, int(prefill_chunk))
                with torch.cuda.stream(ln.st):
                    for t0 in range(0, T, tc):
                        n = min(tc, T - t0)
                        piece = ln.emb[:, t0: t0 + n].contiguous()
                        _lib.check(lib.ctts_gpt_prefill_chunk(ln.handle, C.byref(ln.s), piece.data_ptr(), t0, n, int(t0 + n == T),
                                                              ln.st.cuda_stream), "ctts_gpt_prefill_chunk")
                        ln.keep_piece = piece   # stream-ordered use: stays alive until the next piece replaces it / the poll syncs
        steps_done = 1
        steps_enq = 1     # steps enqueued so far (>= steps_done: chunks run ahead of the host's finish polls)
        graph_ok = False
        for ln in L:
            ln.ev = torch.cuda.Event()
        fin0 = torch.cat([poll(ln) for ln in L])  # syncs: the step-0 rule needs it (gpt.py:527)
        if bool(fin0.any()):
            self.logger.warning("unexpected end at index %s", str(fin0.nonzero().flatten().tolist()))
            finish_rng(1)   # the reference drew exactly one tensor (step 0) before it got here
            if ensure_non_empty and manual_seed is None:
                self.logger.warning("regenerate in order to ensure non-empty")
                yield from self.generate(emb, inputs_ids, temperature, eos_token, attention_mask, max_new_token,
                                         min_new_token, logits_processors, infer_text, return_attn, return_hidden,
                                         stream, show_tqdm, ensure_non_empty, stream_batch, manual_seed, context,
                                         use_graph=use_graph, stop_at=stop_at, row_offset=row_offset, total_rows=total_rows,
                                         profile_tag=profile_tag, profile_stride=profile_stride, lanes=lanes,
                                         teacher_ids=teacher_ids, prefill_chunk=prefill_chunk, return_sampled=return_sampled,
                                         rng=rng, rng_seed=None, rng_nonce=rng_nonce, row_ids=row_ids, exact=exact, text_rng=text_rng)
            return  # gpt.py:570: the seeded case yields nothing

        graph_ok = use_graph and max_new > 1
        # OPT-IN (CTTS_GRAPH_ROWS=1): measured on the C3 bench it changes nothing -- 1399-1406 vs 1403-1413 audio-s/s, parity mode 1011-1031
        # vs 1021-1037 (profiles/r5o_ab_graph_rows.log): like the persistent attention grid, it removes workgroups that were not what the
        # step was waiting for.  Default: every chunk on the batch-sized graph.
        rows_graphs = os.environ.get("CTTS_GRAPH_ROWS", "0") == "1"
        if graph_ok and not sess["graph"]:
            for ln in L:
                _lib.check(lib.ctts_gpt_graph_build(ln.handle, C.byref(ln.s), ln.st.cuda_stream), "ctts_gpt_graph_build")
            sess["graph"] = True
            sess["rows_built"] = [set() for _ in L]     # (graph_build dropped whatever bounded graphs the handle had)
        if profile_tag is not None:
            _lib.check(lib.ctts_gpt_profile_begin(L[0].handle, int(profile_tag), 4096, int(profile_stride)), "profile_begin")

        chunk = stream_batch if stream else self.POLL
        all_done = all(ln.done for ln in L)
        interrupted = False
        # the reference yields when (i+1) % stream_batch == 0: keep chunk ends on those steps
        next_n = lambda done: min(chunk - (done % chunk), max_new - done)
        # Run-ahead: chunk k+1 is enqueued BEFORE the host looks at chunk k's finish flags (asynchronous snapshots), so the
        # GPU never idles on the host between chunks; a streamed chunk's consumer (DVAE/Vocos of the prefix) overlaps the
        # generation of the next one.  If everything turns out finished, the surplus chunk is ~100 empty launches per step.
        import time as _time
        t_dec0 = _time.perf_counter()
        inflight = []   # [(steps, [snapshot index per lane])], oldest first

        def launch_chunk():
            n = next_n(steps_enq)
            enqueue(n)
            inflight.append((n, [None if ln.done else snapshot(ln) for ln in L]))

        try:
            if steps_enq < max_new and not all_done:
                launch_chunk()
            while inflight:
                if len(inflight) < 2 and steps_enq < max_new and not context.get():
                    launch_chunk()
                n, snaps = inflight.pop(0)
                for ln, k in zip(L, snaps):
                    if k is not None and not ln.done:
                        collect(ln, k)
                steps_done += n
                all_done = all(ln.done for ln in L)
                if all_done:
                    inflight.clear()   # a surplus chunk computes nothing (no live rows); its launches drain in `finally`
                if stream:
                    emit = False
                    if not all_done and steps_done % stream_batch == 0:
                        emit = True                                      # gpt.py:579-589
                    elif all_done:
                        i_star = max(max(ln.end_snap) for ln in L)       # step at which the last row hit EOS
                        emit = i_star > 0 and i_star % stream_batch == 0  # the reference's duplicate yield (stream_iter quirk)
                    if emit:
                        yield outputs()
                # the reference tests the interrupt flag after the step's stream yield (gpt.py:579-592): a chunk that ends on a
                # yield boundary is still handed out.  Granularity here is one chunk (POLL / stream_batch steps), not one step.
                if context.get():
                    interrupted = True
                    # run-ahead: a chunk may already be enqueued behind the one just collected.  Its tokens WILL be in the buffers
                    # the final outputs() reads, so it is collected and counted too -- tokens, `steps` and the rewound position of
                    # the global CPU generator (unseeded mode) then describe the same number of steps.
                    while inflight:
                        n2, snaps2 = inflight.pop(0)
                        for ln, k in zip(L, snaps2):
                            if k is not None and not ln.done:
                                collect(ln, k)
                        steps_done += n2
                    all_done = all(ln.done for ln in L)
                    break
            if profile_tag is not None:
                n_s, tot = C.c_int32(0), C.c_double(0.0)
                buf = (C.c_float * 4096)()
                _lib.check(lib.ctts_gpt_profile_samples(L[0].handle, buf, 4096, C.byref(n_s)), "profile_samples")
                self.last_stats["profile_samples_ms"] = np.ctypeslib.as_array(buf)[: int(n_s.value)].copy()
                _lib.check(lib.ctts_gpt_profile_end(L[0].handle, C.byref(n_s), C.byref(tot)), "profile_end")
                self.last_stats["profile"] = (int(n_s.value), float(tot.value))
        finally:
            if feeder is not None:
                feeder["pool"].shutdown(wait=True)   # idempotent; the generator-state rewind happens in finish_rng
            for ln in L:
                wait_stream(ln.st)   # nothing of this call is still running when its buffers are handed to the next one
            self.last_stats["decode_ms"] = 1e3 * (_time.perf_counter() - t_dec0)   # host wall of the decode loop (streaming: incl. consumer time)
        if not all_done:
            if interrupted:
                self.logger.warning("generation is interrupted")
            else:
                self.logger.warning(f"incomplete result. hit max_new_token: {max_new_token}")   # gpt.py:601-607
        self.last_stats.update(steps=steps_done, B=B, T=T, lanes=n_lanes)
        for ln in L:
            if not ln.done or ln.end_snap is None:
                poll(ln)
        # steps the reference loop would have executed: up to and including the step at which the last row hit EOS
        steps_ref = (max(max(ln.end_snap) for ln in L) + 1) if all_done else min(steps_done, max_new)
        finish_rng(min(steps_ref, max_new))
        if return_sampled:
            self.last_sampled = [ln.sampled[b, : ln.end_snap[b]].clone() for ln in L for b in range(ln.hi - ln.lo)]
        final = outputs()
        if certify:
            # ---- parity certificate: the smallest decision margin of every utterance (tempered-logit units) against twice the stated
            # logit error of the split-fp16 projections.  The lanes are idle here (wait_stream above).
            marg = torch.cat([ln.margin for ln in L]).cpu().numpy()
            x3_run = self.x3 is not None and not exact
            bound = 2.0 * self.REL_ERR_X3 * self.logit_scale[bool(infer_text)] / max(float(temperature.min()), 1e-6) if x3_run else 0.0
            unsafe = np.nonzero(marg < bound)[0].tolist()
            self.last_margins = marg
            self.last_stats.update(min_margin=float(marg.min()) if marg.size else float("inf"), margin_bound=bound,
                                   certified=not unsafe, uncertified_rows=unsafe, exact_rerun_rows=[])
            if unsafe:
                (self.logger.warning if self.exact_fallback else self.logger.info)(
                                    "parity certificate: %d of %d utterances had a draw decided by less than %.2e tempered-logit units "
                                    "(smallest margin %.2e)%s", len(unsafe), B, bound, float(marg.min()),
                                    "; generating them again on the exact f32 kernels" if (self.exact_fallback and not stream and not interrupted)
                                    else "; the split-fp16 result stands as it is")
                if self.exact_fallback and not stream and not interrupted:
                    final = self._rerun_exact(final, unsafe, emb, inputs_ids, temperature, eos_token, attention_mask, max_new_token, min_new_token,
                                              logits_processors, infer_text, return_hidden, stream_batch, manual_seed, context, use_graph, stop_at,
                                              row_offset // nrow, (total_rows if total_rows is not None else B * nrow), prefill_chunk, rng,
                                              seed_val if device_rng else None, rng_nonce, rid, rng_state0, text_rng)
        yield final

    def _rerun_exact(self, final, rows, emb, inputs_ids, temperature, eos_token, attention_mask, max_new_token, min_new_token,
                     logits_processors, infer_text, return_hidden, stream_batch, manual_seed, context, use_graph, stop_at, first_row,
                     total_rows, prefill_chunk, rng, rng_seed, rng_nonce, rid, rng_state0, text_rng=None):
        """The exact fallback of the certificate: utterances `rows` of the call once more, as a sub-batch with the same padded prompt
        geometry, on the f32 MFMA decode kernels, with the draws of their own global rows -- what the "f32" engine gives for them (utterances
        never interact) -- spliced over their rows of `final`."""
        stats = dict(self.last_stats)
        sel = torch.tensor(rows, dtype=torch.long)
        gid = rid[sel] if rid is not None else sel + int(first_row)
        nz = None
        if rng_nonce is not None:
            nz = torch.as_tensor(rng_nonce, dtype=torch.int64).reshape(-1)
            nz = nz if nz.numel() == 1 else nz[sel]
        state_after = None
        if rng_state0 is not None:     # unseeded host draws: the same per-step tensors the main call consumed
            state_after = torch.get_rng_state()
            torch.set_rng_state(rng_state0)
        sub = None
        try:
            for sub in self.generate(emb[sel.to(emb.device)], inputs_ids[sel.to(inputs_ids.device)], temperature, eos_token,
                                     None if attention_mask is None else attention_mask[sel.to(attention_mask.device)], max_new_token, min_new_token,
                                     logits_processors, infer_text, False, return_hidden, False, False, False, stream_batch, manual_seed, context,
                                     use_graph=use_graph, stop_at=None if stop_at is None else stop_at[sel.to(stop_at.device)], total_rows=total_rows,
                                     lanes=1, prefill_chunk=prefill_chunk, rng=rng, rng_seed=rng_seed, rng_nonce=nz, row_ids=gid, exact=True, text_rng=text_rng):
                pass
        finally:
            # where the global generator is left: the reference draws once per step of its loop, which ends when the LAST utterance
            # finishes -- the run (main or re-run) that executed more steps decides; a re-run of every utterance IS the call
            if state_after is not None:
                keep_rerun = sub is not None and (len(rows) == len(final.ids) or self.last_stats.get("steps", 0) > stats.get("steps", 0))
                if not keep_rerun:
                    torch.set_rng_state(state_after)
        rerun_stats = self.last_stats
        self.last_stats = stats
        if sub is None:     # (an EOS at step 0 of the exact run: the seeded reference yields nothing, gpt.py:570)
            self.logger.warning("parity certificate: the exact re-run ended at step 0; the split-fp16 rows stand")
            return final
        same_len = all(int(sub.ids[j].shape[0]) == int(final.ids[b].shape[0]) for j, b in enumerate(rows))
        padded = getattr(final.hiddens, "padded", None)
        if return_hidden and not (same_len and padded is not None):
            final.hiddens = RowList(list(final.hiddens))      # plain rows: the decoder re-pads (core.py:525-533)
            padded = None
        for j, b in enumerate(rows):
            final.ids[b] = sub.ids[j]
            if return_hidden:
                if padded is not None:
                    padded[b, : sub.hiddens[j].shape[0]].copy_(sub.hiddens[j])     # (final.hiddens[b] is a view of it)
                else:
                    final.hiddens[b] = sub.hiddens[j]
        self.last_stats.update(exact_rerun_rows=list(rows), exact_rerun_steps=rerun_stats.get("steps"),
                               exact_rerun_min_margin=rerun_stats.get("min_margin"), certified=True)
        return final


def split_bf16(w: torch.Tensor) -> torch.Tensor:
    """[N, K] float32 -> [N, Kp/32, 2, 32] bfloat16, Kp = K rounded up to 32 and zero padded: for every row and every
    32-wide k block the hi values then the lo values, w = hi + lo up to 2^-17 |w| (the weight operand of the bf16x3
    GEMM tiles).  One k-step of one row is ONE 128-byte line (hi 64 B + lo 64 B), so a tile step never fetches a
    half-used cache line."""
    N, K = w.shape
    Kp = (K + 31) // 32 * 32
    wp = torch.zeros((N, Kp), dtype=torch.float32)
    wp[:, :K] = w
    hi = wp.to(torch.bfloat16)
    lo = (wp - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.stack([hi.view(N, Kp // 32, 32), lo.view(N, Kp // 32, 32)], 2).contiguous()


def pack_x3p(w: torch.Tensor) -> torch.Tensor:
    """[R, K] float32 (R % 32 == 0, K % 16 == 0) -> the PRE-SPLIT planes of csrc/codec_gemm.hip in MFMA fragment order,
    [R/32][K/16][hi | lo][lane = (k%16)/8*32 + r%32][k%8] bfloat16: w = hi + lo up to 2^-17 |w|, and every (32-row tile,
    16-wide k block, plane) is one contiguous KiB -- what `v_mfma_f32_32x32x16_bf16` takes as an operand, so a tile step is
    staged by plain LDS-DMA copies."""
    R, K = w.shape
    assert R % 32 == 0 and K % 16 == 0
    w = w.to(torch.float32)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    x = torch.stack([hi, lo], 0).reshape(2, R // 32, 32, K // 16, 2, 8)
    return x.permute(1, 3, 0, 4, 2, 5).contiguous()


def unpack_x3p(p: torch.Tensor, R: int, K: int) -> torch.Tensor:
    """inverse of pack_x3p: -> float32 [R, K] = hi + lo (tests)"""
    x = p.reshape(R // 32, K // 16, 2, 2, 32, 8).permute(2, 0, 4, 1, 3, 5).reshape(2, R, K).to(torch.float32)
    return x[0] + x[1]


def pack_h1p(w: torch.Tensor) -> torch.Tensor:
    """[R, K] float32 (R % 32 == 0, K % 16 == 0) -> ONE fp16 plane in MFMA fragment order (csrc/codec_gemm.hip: gemm_h1p_k),
    [R/32][K/16][lane = (k%16)/8*32 + r%32][k%8] float16, values saturated to the finite half range like the kernels' own
    activation rounding."""
    R, K = w.shape
    assert R % 32 == 0 and K % 16 == 0
    h = w.to(torch.float32).clamp(-65504.0, 65504.0).to(torch.float16)
    return h.reshape(R // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def unpack_h1p(p: torch.Tensor, R: int, K: int) -> torch.Tensor:
    """inverse of pack_h1p: -> float32 [R, K] (tests)"""
    return p.reshape(R // 32, K // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(R, K).to(torch.float32)


# ---------------------------------------------------------------------------------------------
class PendingWavs:
    """result of `CodecEngine.decode_to_wavs_async`: the float32 waveforms of one batch, in flight"""

    def __init__(self, codec, view, done, keep):
        self._codec, self._view, self._done, self._keep, self._out = codec, view, done, keep, None

    def done(self) -> bool:
        return self._out is not None or self._done.query()

    def result(self) -> np.ndarray:
        if self._out is None:
            wait_event(self._done)
            self._out = self._codec._copy_out(self._view) if self._view.numel() else np.zeros(tuple(self._view.shape), np.float32)
            self._keep = None
        return self._out


def ragged_offsets(lens):
    """packed-segment arithmetic of a ragged decode of rows with `lens` tokens: (token offsets int32, sample offsets int64 -- row i's
    256 (2 T_i - 1) samples at [off[i], off[i+1]) --, keep-mask byte offsets int64 -- row i's ceil(n_i / 8) bytes, byte aligned)"""
    lens = np.asarray(lens, dtype=np.int64)
    tok = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=tok[1:])
    off = VOCOS.hop * (2 * tok - np.arange(len(lens) + 1))
    return tok.astype(np.int32), off, keep_offsets(off)


def keep_offsets(off) -> np.ndarray:
    """byte offsets of the per-segment keep masks of samples packed at `off` (every segment starts on a byte boundary)"""
    off = np.asarray(off, dtype=np.int64)
    k = np.zeros(len(off), np.int64)
    np.cumsum((np.diff(off) + 7) // 8, out=k[1:])
    return k


def group_starts(off, grp) -> np.ndarray:
    """first output element of every group of `CodecEngine.float_to_int16_groups` (+ the total as the last entry): the running sum of the
    groups' unstripped lengths, each rounded up to 8 samples -- for a decode's offsets (multiples of 256) simply off[grp[g]]"""
    off, grp = np.asarray(off, dtype=np.int64), np.asarray(grp, dtype=np.int64)
    s = np.zeros(len(grp), np.int64)
    np.cumsum((np.diff(off[grp]) + 7) // 8 * 8, out=s[1:])
    return s


def ragged_views(flat, off) -> list:
    """the per-utterance pieces [off[i], off[i+1]) of a packed 1-D array or tensor (CodecEngine.decode_ragged): views, no copies"""
    return [flat[int(off[i]): int(off[i + 1])] for i in range(len(off) - 1)]


# receptive field of one output sample, in mel frames either side: ISTFT 4 overlapping frames; Vocos embed k7 + 8 ConvNeXt
# blocks k7 = 27; DVAE conv_in k3 + k3, 12 ConvNeXt blocks k7 dilation 2, out_conv k3 = 75 (dvae.py:145-161, config.py:83-121)
HALO_FRAMES = 27 + 75


def window_for_samples(Tn: int, s_lo: int, s_hi: int):
    """The token window that samples [s_lo, s_hi) of the decode of a `Tn`-token prefix depend on, and where they sit in its decode:
    (t_lo, t_hi, c_lo, c_hi) -- tokens [t_lo, t_hi) decoded alone give the samples at [c_lo, c_hi) of that decode (HALO_FRAMES mel
    frames + the 4 overlapping ISTFT frames either side; at the prefix's own ends the window's edge is the sequence's edge).  The range
    is clipped to the prefix's 256 (2 Tn - 1) samples; None when nothing is left.  Pure host arithmetic (`decode_window`,
    `decode_windows`)."""
    Tn = int(Tn)
    hop, nfft = VOCOS.hop, VOCOS.n_fft
    total = hop * (2 * Tn - 1)
    s_lo, s_hi = max(0, int(s_lo)), min(total, int(s_hi))
    if s_hi <= s_lo:
        return None
    f_a = (s_lo + nfft // 2) // hop - (nfft // hop - 1)          # first / last ISTFT frame that overlaps the samples
    f_b = min((s_hi - 1 + nfft // 2) // hop, 2 * Tn - 1)
    t_lo = max(0, (f_a - HALO_FRAMES) // 2)
    t_hi = min(Tn, (f_b + HALO_FRAMES) // 2 + 1)
    off = 2 * hop * t_lo                                          # sample index of the window's first sample
    return t_lo, t_hi, s_lo - off, s_hi - off


class CodecEngine:
    """DVAE decoder + Vocos on the device (channels-last)."""

    def __init__(self, decoder_sd: dict, vocos_sd: dict, device: torch.device, gemm: str = "bf16x3"):
        """gemm="bf16x3": dense layers run on split-bf16 MFMA tiles (x = hi + lo, 3 products; f32-class accuracy,
        measured wav RMS error vs the reference ~1e-6 against the 1e-4 bar); gemm="f32": f32-input MFMA tiles;
        gemm="f16" (the perf mode's decoder): as "bf16x3", but the ConvNeXt point-wise pairs of batches from 1024 frames take
        one fp16 MFMA per product with f32 accumulation -- waveform within 1e-5 RMS of "bf16x3" (stated and tested bound; the
        north-star bar is 1e-4), about half the decode time."""
        if gemm not in ("bf16x3", "f32", "f16"):
            raise ValueError("gemm must be 'bf16x3', 'f16' or 'f32'")
        self.gemm = gemm
        self.lib = _lib.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.EngineError("CodecEngine needs a ROCm GPU device (there is no CPU path)")
        dev = self.device
        f = lambda t: t.to(torch.float32).contiguous().to(dev)
        dww = lambda t: f(t[:, 0, :].t())                # [C,1,7] -> [7,C]

        def dense(t):
            """[N, K] float32 dense weight -> device tensor in the layout the selected GEMM tiles read"""
            t = t.to(torch.float32).reshape(t.shape[0], -1).contiguous()
            if gemm == "f32":
                return t.to(dev)
            return split_bf16(t).to(dev)

        convw = lambda t: dense(t.permute(0, 2, 1))      # [Cout,Cin,k] -> [Cout,k*Cin]
        self.keep = []
        k = self.keep.append
        w = _lib.CodecWeights()

        def P(t):
            k(t)
            return t.data_ptr()

        def PA(ts):
            k(ts)
            arr = _lib.ptr_array(ts)
            k(arr)
            return C.cast(arr, _lib.PP)

        d = decoder_sd
        w.conv_in0_w, w.conv_in0_b = P(convw(d["decoder.conv_in.0.weight"])), P(f(d["decoder.conv_in.0.bias"]))
        w.conv_in2_w, w.conv_in2_b = P(convw(d["decoder.conv_in.2.weight"])), P(f(d["decoder.conv_in.2.bias"]))
        nb = 0
        while f"decoder.decoder_block.{nb}.weight" in d:
            nb += 1
        w.n_dvae_blocks = nb
        blk = lambda i, n: d[f"decoder.decoder_block.{i}.{n}"]
        w.d_dw_w = PA([dww(blk(i, "dwconv.weight")) for i in range(nb)])
        w.d_dw_b = PA([f(blk(i, "dwconv.bias")) for i in range(nb)])
        w.d_ln_w = PA([f(blk(i, "norm.weight")) for i in range(nb)])
        w.d_ln_b = PA([f(blk(i, "norm.bias")) for i in range(nb)])
        w.d_pw1_w = PA([dense(blk(i, "pwconv1.weight")) for i in range(nb)])
        w.d_pw1_b = PA([f(blk(i, "pwconv1.bias")) for i in range(nb)])
        w.d_pw2_w = PA([dense(blk(i, "pwconv2.weight")) for i in range(nb)])
        w.d_pw2_b = PA([f(blk(i, "pwconv2.bias")) for i in range(nb)])
        w.d_gamma = PA([f(blk(i, "weight")) for i in range(nb)])
        w.conv_out_w = P(dense(d["decoder.conv_out.weight"][:, :, 0]))
        w.out_conv_w = P(convw(d["out_conv.weight"]))
        w.coef = P(f(d["coef"].reshape(-1)))
        v = vocos_sd
        w.v_embed_w, w.v_embed_b = P(convw(v["backbone.embed.weight"])), P(f(v["backbone.embed.bias"]))
        w.v_norm_w, w.v_norm_b = P(f(v["backbone.norm.weight"])), P(f(v["backbone.norm.bias"]))
        nv = 0
        while f"backbone.convnext.{nv}.gamma" in v:
            nv += 1
        w.n_vocos_blocks = nv
        vb = lambda i, n: v[f"backbone.convnext.{i}.{n}"]
        w.v_dw_w = PA([dww(vb(i, "dwconv.weight")) for i in range(nv)])
        w.v_dw_b = PA([f(vb(i, "dwconv.bias")) for i in range(nv)])
        w.v_ln_w = PA([f(vb(i, "norm.weight")) for i in range(nv)])
        w.v_ln_b = PA([f(vb(i, "norm.bias")) for i in range(nv)])
        w.v_pw1_w = PA([dense(vb(i, "pwconv1.weight")) for i in range(nv)])
        w.v_pw1_b = PA([f(vb(i, "pwconv1.bias")) for i in range(nv)])
        w.v_pw2_w = PA([dense(vb(i, "pwconv2.weight")) for i in range(nv)])
        w.v_pw2_b = PA([f(vb(i, "pwconv2.bias")) for i in range(nv)])
        w.v_gamma = PA([f(vb(i, "gamma")) for i in range(nv)])
        w.v_final_w, w.v_final_b = P(f(v["backbone.final_layer_norm.weight"])), P(f(v["backbone.final_layer_norm.bias"]))
        w.head_w, w.head_b = P(dense(v["head.out.weight"])), P(f(v["head.out.bias"]))
        w.window = P(f(v["head.istft.window"]))
        kk = torch.arange(VOCOS.n_fft // 2, dtype=torch.float64) * (2.0 * math.pi / VOCOS.n_fft)
        w.twiddle = P(f(torch.stack([kk.cos(), kk.sin()], 1)))
        w.gemm_mode = {"f32": 0, "bf16x3": 1, "f16": 2}[gemm]
        if gemm == "f16":
            h1p = lambda t: pack_h1p(t.to(torch.float32).reshape(t.shape[0], -1)).to(dev)
            w.d_pw1_x3p = PA([h1p(blk(i, "pwconv1.weight")) for i in range(nb)])
            w.d_pw2_x3p = PA([h1p(blk(i, "pwconv2.weight")) for i in range(nb)])
            w.v_pw1_x3p = PA([h1p(vb(i, "pwconv1.weight")) for i in range(nv)])
            w.v_pw2_x3p = PA([h1p(vb(i, "pwconv2.weight")) for i in range(nv)])
        if gemm == "bf16x3":
            # the ConvNeXt point-wise layers once more as pre-split fragment-order planes: from 12288 frames they run on the
            # LDS-DMA staged kernel of csrc/codec_gemm.hip (40 of the 45 GEMM launches of a decode)
            x3p = lambda t: pack_x3p(t.to(torch.float32).reshape(t.shape[0], -1)).to(dev)
            w.d_pw1_x3p = PA([x3p(blk(i, "pwconv1.weight")) for i in range(nb)])
            w.d_pw2_x3p = PA([x3p(blk(i, "pwconv2.weight")) for i in range(nb)])
            w.v_pw1_x3p = PA([x3p(vb(i, "pwconv1.weight")) for i in range(nv)])
            w.v_pw2_x3p = PA([x3p(vb(i, "pwconv2.weight")) for i in range(nv)])
        self._w = w
        h = C.c_void_p()
        _lib.check(self.lib.ctts_codec_create(C.byref(h), C.byref(w)), "ctts_codec_create")
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.ctts_codec_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _ws(self, B, F):
        """the codec workspace: ONE buffer per engine that only ever grows.  A streamed utterance asks for a different window size
        at every yield; going through the caching allocator each time meant a device allocation per yield whenever no cached block
        fitted (tens of milliseconds each on this pool's hosts, profiles/r3e_c5_sched_probe.log).  Kernels of consecutive calls
        are stream-ordered on the caller's stream, so sharing the buffer needs no extra synchronisation as long as ONE stream
        drives the engine at a time (the documented contract of a handle, include/chattts_amd.h)."""
        return self._ws_bytes(self.lib.ctts_codec_workspace_bytes(B, F))

    def _ws_bytes(self, n: int):
        cur = torch.cuda.current_stream(self.device)
        buf = getattr(self, "_ws_buf", None)
        if buf is None or buf.numel() < n or getattr(self, "_ws_stream", None) != cur.cuda_stream:
            if buf is not None:
                buf.record_stream(cur)
            with torch.cuda.stream(cur):
                self._ws_buf = buf = device_scratch(max(n, 0 if buf is None else buf.numel()), self.device)
            self._ws_stream = cur.cuda_stream
        return buf, buf.numel()

    def dvae_decode(self, hid: torch.Tensor) -> torch.Tensor:
        """hid [B,T,768] f32 (zero padded rows) -> mel [B,2T,100]   (dvae.py:276-297)."""
        B, T, H = hid.shape
        assert H == GPT.hidden
        hid = hid.to(torch.float32).contiguous().to(self.device)
        mel = torch.empty((B, 2 * T, DVAE.n_mels), dtype=torch.float32, device=self.device)
        ws, n = self._ws(B, 2 * T)
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.ctts_dvae_decode(self.handle, hid.data_ptr(), mel.data_ptr(), B, T, ws.data_ptr(), n, st), "ctts_dvae_decode")
        return mel

    def vocos_decode(self, mel: torch.Tensor) -> torch.Tensor:
        """mel [B,F,100] -> wav [B,256(F-1)]   (vocos.Vocos.decode, core.py:505-510)."""
        B, F, M = mel.shape
        assert M == VOCOS.n_mels and F >= 2
        mel = mel.to(torch.float32).contiguous().to(self.device)
        wav = torch.empty((B, VOCOS.hop * (F - 1)), dtype=torch.float32, device=self.device)
        ws, n = self._ws(B, F)
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.lib.ctts_vocos_decode(self.handle, mel.data_ptr(), wav.data_ptr(), B, F, ws.data_ptr(), n, st), "ctts_vocos_decode")
        return wav

    def float_to_int16(self, wav: torch.Tensor, per_row: bool = True, product: str = "f64", keep_thr: Optional[float] = None):
        """`float_to_int16` of the reference's back end (tools/audio/np.py:7-11) ON THE DEVICE, before the waveform crosses PCIe: wav
        [B, n] float32 (any row stride) -> (pcm [B, n] int16, keep) with am = 32767 * 32768 // (ceil(peak) * 32768) and truncation toward
        zero.  per_row: a peak per utterance (one call per utterance, examples/web/funcs.py:206-209) -- False: ONE peak over the block
        (the function applied to a [B, n] array, examples/cmd/stream.py:44).  product "f64": the reference's numba runtime (exact product),
        "f32": plain NumPy's reading of the same line.  keep_thr: also return the packed mask |x| > keep_thr ([B, ceil(n/8)] uint8,
        np.packbits order) -- the selector of Chat.infer's silence strip (core.py:262-265) -- else None.  Bit-exact against the reference
        function (tests/test_backend.py)."""
        assert wav.dim() == 2 and wav.dtype == torch.float32 and wav.is_cuda and (wav.shape[1] == 0 or wav.stride(1) == 1)
        B, n = int(wav.shape[0]), int(wav.shape[1])
        pcm = torch.empty((B, n), dtype=torch.int16, device=wav.device)
        keep = torch.empty((B, (n + 7) // 8), dtype=torch.uint8, device=wav.device) if keep_thr is not None else None
        if B == 0 or n == 0:
            return pcm, keep
        peak = torch.empty((B,), dtype=torch.int32, device=wav.device)
        st = torch.cuda.current_stream(wav.device).cuda_stream
        _lib.check(self.lib.ctts_float_to_int16(wav.data_ptr(), pcm.data_ptr(), _lib.ptr(keep), B, n, int(wav.stride(0)) if B > 1 else n,
                                                1 if per_row else 0, {"f64": 0, "f32": 1}[product], float(keep_thr or 0.0), peak.data_ptr(), st),
                   "ctts_float_to_int16")
        return pcm, keep

    # -- sample-rate conversion (csrc/resample.hip) ----------------------------------------------------------------------------------
    SAMPLE_RATE = 24000      # what the acoustic decoder produces and the DVAE encoder expects

    def _resample_taps(self, orig: int, new: int) -> torch.Tensor:
        """the float32 [L, K] polyphase table of a rate pair on the device, built once (resample.taps, float64 on the host)"""
        cache = self.__dict__.setdefault("_rs_taps", {})
        key = (int(orig), int(new))
        if key not in cache:
            cache[key] = torch.from_numpy(np.ascontiguousarray(RS.taps(*key), dtype=np.float32)).to(self.device)
        return cache[key]

    def _resample_launch(self, x: torch.Tensor, off: np.ndarray, y: torch.Tensor, off_out: np.ndarray, sel, orig: int, new: int) -> None:
        """ctts_resample_ragged over segments `sel` (None: all) of the pack x / off into y / off_out"""
        L, M = RS.ratio(orig, new)
        _, K = RS.geometry(L, M)
        taps = self._resample_taps(orig, new)
        n_seg = len(off) - 1
        sel_h = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        parts = [off.view(np.uint8), off_out.view(np.uint8)] + ([] if sel_h is None else [sel_h.view(np.uint8)])
        tabs = torch.from_numpy(np.concatenate(parts)).to(x.device)       # one upload: input offsets, output offsets, the selection
        st = torch.cuda.current_stream(x.device)
        base = tabs.data_ptr()
        _lib.check(self.lib.ctts_resample_ragged(
            x.data_ptr(), base, off.ctypes.data_as(C.c_void_p), y.data_ptr(), base + off.nbytes, off_out.ctypes.data_as(C.c_void_p), n_seg,
            None if sel_h is None else base + off.nbytes + off_out.nbytes, None if sel_h is None else sel_h.ctypes.data_as(C.c_void_p),
            0 if sel_h is None else len(sel_h), taps.data_ptr(), L, M, K, st.cuda_stream), "ctts_resample_ragged")
        tabs.record_stream(st)

    def resample(self, wav: torch.Tensor, orig: int, new: int, offsets=None):
        """Windowed-sinc polyphase conversion orig -> new Hz of a float32 device tensor (ctts_resample_ragged; the filter of
        resample.py): 1-D (one signal), [B, n] (rows, each alone -> [B, ceil(n L / M)]), or 1-D packed with `offsets` (n_seg + 1 sample
        offsets, the ragged decoder's layout; every segment as if alone) -> (tensor, new offsets).  `orig == new` returns the input
        untouched.  ValueError before any launch: an unsupported rate pair, an empty segment, non-ascending offsets, 2^31 samples out."""
        if int(orig) == int(new):
            return wav if offsets is None else (wav, offsets)
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("resample: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("resample: offsets go with a packed 1-D tensor")
        if wav.dim() == 2:
            B, n = int(wav.shape[0]), int(wav.shape[1])
            off = np.arange(B + 1, dtype=np.int64) * n
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int64) if offsets is not None else np.array([0, wav.numel()], dtype=np.int64)
        if len(off) < 2:
            raise ValueError("resample: nothing to convert")
        _, _, _, off_out = RS.plan(orig, new, off)
        if int(off[-1]) != wav.numel():
            raise ValueError("resample: the offsets do not cover the tensor")
        x = wav.contiguous()
        y = torch.empty((int(off_out[-1]),), dtype=torch.float32, device=wav.device)
        self._resample_launch(x.view(-1), off, y, off_out, None, int(orig), int(new))
        if wav.dim() == 2:
            return y.view(wav.shape[0], -1)
        return (y, off_out) if offsets is not None else y

    def resample_segments(self, wav: torch.Tensor, off, rates, orig: int = SAMPLE_RATE):
        """packed segments to ONE RATE EACH (`rates[i]` for segment i): requests that were decoded together and want different rates.
        One launch per distinct rate over that rate's segments, all into one packed output; segments that stay at `orig` are copied.
        -> (tensor, offsets).  A segment's samples are those of `resample` on it alone, bit for bit."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        rates = [int(r) for r in rates]
        if len(rates) != len(off) - 1:
            raise ValueError("resample_segments: one rate per segment")
        distinct = sorted(set(rates))
        if len(distinct) == 1:
            return self.resample(wav, orig, distinct[0], off)
        for r in distinct:
            if r != orig:
                RS.plan(orig, r, off)       # every refusal, before the first launch
        lens = [int(n) if r == orig else RS.out_len(int(n), *RS.ratio(orig, r)) for n, r in zip(np.diff(off), rates)]
        off_out = np.zeros(len(off), np.int64)
        np.cumsum(lens, out=off_out[1:])
        if int(off_out[-1]) >= 1 << 31:
            raise ValueError("resample: the output would hold 2^31 samples or more")
        if int(off[-1]) != wav.numel() or wav.dim() != 1:
            raise ValueError("resample_segments: a packed 1-D tensor covered by its offsets")
        x = wav.contiguous()
        y = torch.empty((int(off_out[-1]),), dtype=torch.float32, device=wav.device)
        for r in distinct:
            idx = [i for i, q in enumerate(rates) if q == r]
            if r == orig:
                for i in idx:
                    y[int(off_out[i]): int(off_out[i + 1])].copy_(x[int(off[i]): int(off[i + 1])])
            else:
                self._resample_launch(x, off, y, off_out, idx, orig, r)
        return y, off_out

    def resample_window(self, wav: torch.Tensor, origin: int, total: int, o_lo: int, o_hi: int, orig: int, new: int) -> torch.Tensor:
        """Outputs [o_lo, o_hi) of `resample(signal, orig, new)` from a WINDOW of the signal (ctts_resample_windows, resample_win_k):
        `wav`, 1-D or [B, n] float32 on the device, holds samples [origin, origin + n) of a signal of `total` samples (every row of its
        own signal, all at the same place) -> [.., o_hi - o_lo], bit for bit the slice of the whole signal's conversion.  The window
        must hold the inputs those outputs read (`resample.window_inputs`); samples outside the signal read as zero.  ValueError before
        any launch otherwise, and for what `resample` refuses."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("resample_window: a float32 device tensor, 1-D or [B, n]")
        L, M, K, _ = RS.plan(orig, new, [0, 1])
        origin, total, o_lo, o_hi = int(origin), int(total), int(o_lo), int(o_hi)
        B, n = (1, int(wav.shape[0])) if wav.dim() == 1 else (int(wav.shape[0]), int(wav.shape[1]))
        a, b = RS.window_inputs(L, M, K, o_lo, o_hi, total)
        if origin < 0 or n < 1 or origin + n > total or total >= 1 << 31:
            raise ValueError(f"resample_window: samples [{origin}, {origin + n}) are no window of a signal of {total}")
        if a < b and (origin > a or origin + n < b):
            raise ValueError(f"resample_window: outputs [{o_lo}, {o_hi}) read samples [{a}, {b}), the window holds [{origin}, {origin + n})")
        if not 1 <= B <= 1024:
            raise ValueError("resample_window: 1 to 1024 rows")
        m = o_hi - o_lo
        y = torch.empty((B, m), dtype=torch.float32, device=wav.device)
        if m > 0:
            x = wav.contiguous()
            tab = np.zeros(B, _lib.RS_WINDOW)
            tab["in_off"], tab["n_in"], tab["origin"], tab["total"] = np.arange(B, dtype=np.int64) * n, n, origin, total
            tab["o_lo"], tab["o_hi"], tab["out_off"] = o_lo, o_hi, np.arange(B, dtype=np.int64) * m
            tab_d = torch.from_numpy(tab.view(np.uint8)).to(wav.device)
            st = torch.cuda.current_stream(wav.device)
            _lib.check(self.lib.ctts_resample_windows(x.data_ptr(), x.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), B, y.data_ptr(),
                                                      y.numel(), None, None, 0, self._resample_taps(orig, new).data_ptr(), L, M, K,
                                                      st.cuda_stream), "ctts_resample_windows")
            tab_d.record_stream(st)
        return y[0] if wav.dim() == 1 else y

    # -- pitch-preserving time scaling (csrc/timescale.hip) ----------------------------------------------------------------------------
    def _time_scale_window(self) -> torch.Tensor:
        """the float32 [N] periodic Hann table on the device, built once (timescale.window, float64 on the host)"""
        w = self.__dict__.get("_ts_window")
        if w is None:
            w = self._ts_window = torch.from_numpy(np.ascontiguousarray(TS.window(), dtype=np.float32)).to(self.device)
        return w

    def _time_scale_launch(self, x: torch.Tensor, off: np.ndarray, y: torch.Tensor, path: torch.Tensor, off_out: np.ndarray,
                           path_off: np.ndarray, num: int, den: int) -> None:
        """ctts_time_scale_ragged over the pack x / off into y / off_out and path / path_off (views at a run of a larger pack allowed)"""
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), off_out.view(np.uint8), path_off.view(np.uint8)])).to(x.device)   # one upload
        st = torch.cuda.current_stream(x.device)
        base = tabs.data_ptr()
        _lib.check(self.lib.ctts_time_scale_ragged(
            x.data_ptr(), base, off.ctypes.data_as(C.c_void_p), y.data_ptr(), base + off.nbytes, off_out.ctypes.data_as(C.c_void_p),
            path.data_ptr(), base + off.nbytes + off_out.nbytes, path_off.ctypes.data_as(C.c_void_p), len(off) - 1,
            self._time_scale_window().data_ptr(), num, den, st.cuda_stream), "ctts_time_scale_ragged")
        tabs.record_stream(st)

    def time_scale(self, wav: torch.Tensor, speed: float, offsets=None, return_path: bool = False):
        """The same audio at the same pitch, `speed` times as fast: waveform-similarity overlap-add at 24 kHz (ctts_time_scale_ragged;
        the constants and formulas of timescale.py) of a float32 device tensor: 1-D (one signal), [B, n] (rows, each alone ->
        [B, ceil(n / speed)]), or 1-D packed with `offsets` (n_seg + 1 sample offsets, the ragged decoder's layout; every segment as if
        alone) -> (tensor, new offsets).  The speed is taken in hundredths; 1.0 returns the input untouched, with no launch.
        `return_path`: also the frame starts s_k the search chose -- an int32 device tensor ([B, F] for rows; packed, with its offsets,
        for a pack: (tensor, offsets, path, path offsets)).  ValueError before any launch: a speed outside 0.5 .. 2.0, an empty segment,
        non-ascending offsets, 2^31 samples."""
        num, den = TS.quantize(speed)
        if num == den:
            if return_path:
                raise ValueError("time_scale: speed 1 has no path")
            return wav if offsets is None else (wav, offsets)
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("time_scale: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("time_scale: offsets go with a packed 1-D tensor")
        if wav.dim() == 2:
            B, n = int(wav.shape[0]), int(wav.shape[1])
            off = np.arange(B + 1, dtype=np.int64) * n
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int64) if offsets is not None else np.array([0, wav.numel()], dtype=np.int64)
        if len(off) < 2:
            raise ValueError("time_scale: nothing to scale")
        _, _, off_out, path_off = TS.plan(speed, off)
        if int(off[-1]) != wav.numel():
            raise ValueError("time_scale: the offsets do not cover the tensor")
        x = wav.contiguous()
        y = torch.empty((int(off_out[-1]),), dtype=torch.float32, device=wav.device)
        path = torch.empty((int(path_off[-1]),), dtype=torch.int32, device=wav.device)
        self._time_scale_launch(x.view(-1), off, y, path, off_out, path_off, num, den)
        if wav.dim() == 2:
            return (y.view(wav.shape[0], -1), path.view(wav.shape[0], -1)) if return_path else y.view(wav.shape[0], -1)
        if offsets is not None:
            return (y, off_out, path, path_off) if return_path else (y, off_out)
        return (y, path) if return_path else y

    # -- time scaling of streams: per-stream device state (csrc/timescale.hip, timescale_stream_k) ---------------------------------------
    # Every streamed stage keeps its streams in a `statepool.StatePool` of its own, built on first use: label -> (the class attribute
    # with the pool's first size -- it doubles when every slot is taken --, the device buffers' {name: (tail, dtype)}; the library is
    # told the slot count and indexes them by slot).  The records are `statepool`'s: TimeScaleRec, ResampleRec, LimiterRec, PauseRec,
    # FlacRec, AdpcmRec, CompressRec.
    TS_STREAM_SLOTS = RS_STREAM_SLOTS = LM_STREAM_SLOTS = FLAC_STREAM_SLOTS = ADPCM_STREAM_SLOTS = CP_STREAM_SLOTS = 64
    PA_STREAM_SLOTS = 16
    ADPCM_CARRY = 2048        # int16 per slot: S - 1 = 2040 at 48 kHz
    CP_CARRY, CP_HIST = 1056, 544   # float32 per half of a slot: compressor.STREAM_CARRY / STREAM_HIST rounded up to 16 bytes (CTTS_CP_SCARRY / _SHIST)
    POOLS = {
        "time_scale": ("TS_STREAM_SLOTS", dict(carry=((2, TS.CARRY), torch.float32), state=((4,), torch.int32))),
        "resample": ("RS_STREAM_SLOTS", dict(carry=((2, RS.CARRY), torch.float32))),
        "limiter": ("LM_STREAM_SLOTS", dict(carry=((2, LM.CARRY), torch.float32), stats=((4,), torch.int32))),      # one limiter.STATS record per slot
        "pauses": ("PA_STREAM_SLOTS", dict(carry=((2, (PA.STREAM_FRAMES + 1) * 480), torch.float32), state=((PA.STATE,), torch.int32))),
        "flac": ("FLAC_STREAM_SLOTS", dict(carry=((FLAC.MIN_BLOCK,), torch.int16))),
        "adpcm": ("ADPCM_STREAM_SLOTS", dict(carry=((ADPCM_CARRY,), torch.int16))),
        "compress": ("CP_STREAM_SLOTS", dict(carry=((2, CP_CARRY), torch.float32), hist=((2, CP_HIST), torch.float32),
                                             stats=((4,), torch.int32))),                                           # one compressor.STATS record per slot
    }

    def _pool(self, label: str) -> SP.StatePool:
        pools = self.__dict__.setdefault("_pools", {})
        if label not in pools:
            slots, buffers = CodecEngine.POOLS[label]
            pools[label] = SP.StatePool(label, getattr(self, slots), buffers, self.device)
        return pools[label]

    def time_scale_stream_open(self, speed: float) -> int:
        """A stream of the time scaler at `speed` (0.5 .. 2.0, not 1): -> its handle, a slot of the engine's state pool.  The slot is
        fresh by construction -- the first step of a stream reads neither carry nor state -- so nothing is cleared.  ValueError for a
        speed the scaler does not take."""
        num, den = TS.quantize(speed)
        if num == den:
            raise ValueError("time_scale: the speed is 1, there is nothing to scale")
        return self._pool("time_scale").open(SP.TimeScaleRec(num, den, 0, 0, False))

    def time_scale_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._pool("time_scale").close(handle)

    def time_scale_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._pool("time_scale").in_use

    def time_scale_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`timescale.stream_plan` of the stream's next push: what a step with `n_in` more samples would run and emit"""
        rec = self._pool("time_scale").live(handle)
        return TS.stream_plan(rec.num / rec.den, rec.pushed, n_in, final)

    def _ts_descriptors(self, pushes):
        """pushes [(handle, in_off, n_in, final)], in the order given, a stream's pushes in ITS order -> (TS_STREAM table sorted into
        rounds with out_off / path_off unset, round_off, order: order[q] = the push behind row q, commit: handle -> its new host record).
        All in Python integers and before anything is launched; the records change only when the caller commits."""
        pool, commit, rows = self._pool("time_scale"), {}, []
        for h, in_off, n_in, final in pushes:
            h = int(h)
            rec = pool.live(h, commit)
            p = TS.stream_plan(rec.num / rec.den, rec.pushed, n_in, final)
            rows.append(((int(in_off), int(n_in), rec.pushed, p["total"], 0, 0, p["k_prev"], p["k_now"], h, rec.phase, rec.num, rec.den, p["n_out"], 0),
                         p["n_path"]))
            commit[h] = rec._replace(pushed=rec.pushed + int(n_in), phase=rec.phase ^ 1, done=bool(final))
        _, members = SP.rounds(int(p[0]) for p in pushes)
        order = [i for m in members for i in m]
        tab = np.zeros(len(order), _lib.TS_STREAM)
        for q, i in enumerate(order):
            tab[q] = rows[i][0]
        round_off = np.zeros(len(members) + 1, np.int32)
        np.cumsum([len(m) for m in members], out=round_off[1:])
        return tab, round_off, order, [rows[i][1] for i in order], commit

    def time_scale_stream_step(self, x: torch.Tensor, pushes, return_path: bool = False):
        """ONE step of many streams (ctts_time_scale_stream_step, one launch): `x`, a 1-D float32 device tensor, holds the new samples
        of every stream; `pushes` = [(handle, in_off, n_in, final)]: x[in_off, in_off + n_in) continue stream `handle` (n_in 0: nothing
        new), `final`: they are its last.  -> (y, off): stream i's chunk is y[off[i], off[i+1]) (possibly empty); the chunks of a
        stream, concatenated, are `time_scale` of its concatenated pushes, bit for bit, however they were cut.  `return_path`: also
        (path, path_off), the frame starts the step chose (s_0 comes with frame 1's).  A handle may appear once per call.  Every
        refusal (ValueError here, EngineError from the library) comes before the launch and leaves all streams as they were."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("time_scale: a contiguous 1-D float32 device tensor")
        SP.check_pushes("time_scale", pushes, x.numel(), most=None)           # more than 1024: the library refuses
        tab, _, order, n_path, commit = self._ts_descriptors(pushes)
        assert order == list(range(len(pushes)))
        off = np.zeros(len(pushes) + 1, np.int64)
        np.cumsum(tab["n_out"], out=off[1:])
        path_off = np.zeros(len(pushes) + 1, np.int64)
        np.cumsum(n_path, out=path_off[1:])
        tab["out_off"], tab["path_off"] = off[:-1], path_off[:-1]
        pool = self._pool("time_scale")
        y = torch.empty((int(off[-1]),), dtype=torch.float32, device=x.device)
        path = torch.empty((int(path_off[-1]),), dtype=torch.int32, device=x.device)
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(x.device)
        st = torch.cuda.current_stream(x.device)
        _lib.check(self.lib.ctts_time_scale_stream_step(
            x.data_ptr() if x.numel() else None, x.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(tab),
            y.data_ptr() if y.numel() else None, y.numel(), path.data_ptr() if path.numel() else None, path.numel(), pool.buf["carry"].data_ptr(),
            pool.buf["state"].data_ptr(), pool.slots, self._time_scale_window().data_ptr(), st.cuda_stream), "ctts_time_scale_stream_step")
        tab_d.record_stream(st)
        pool.commit(commit)
        return (y, off, path, path_off) if return_path else (y, off)

    # -- sample-rate conversion of streams: per-stream device state (csrc/resample.hip, resample_stream_k) --------------------------------
    def resample_stream_open(self, orig: int, new: int) -> int:
        """A stream of the resampler from `orig` to `new` Hz: -> its handle, a slot of the engine's state pool.  The slot is fresh by
        construction -- the first step of a stream reads no carry -- so nothing is cleared.  ValueError for a pair `resample` refuses,
        and for one whose filter (K taps per phase) would carry more than RS.CARRY samples."""
        L, M, K, _ = RS.plan(orig, new, [0, 1])
        if K - 1 > RS.CARRY:
            raise ValueError(f"resample: a stream {orig} -> {new} Hz would carry up to {K - 1} samples, a slot keeps {RS.CARRY}")
        return self._pool("resample").open(SP.ResampleRec(int(orig), int(new), 0, 0, 0, False))

    def resample_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._pool("resample").close(handle)

    def resample_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._pool("resample").in_use

    def resample_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`resample.stream_plan` of the stream's next push: what a step with `n_in` more samples would emit and keep"""
        rec = self._pool("resample").live(handle)
        L, M = RS.ratio(rec.orig, rec.new)
        return RS.stream_plan(L, M, RS.geometry(L, M)[1], rec.pushed, rec.emitted, n_in, final)

    def _rs_descriptors(self, pushes):
        """pushes [(handle, in_off, n_in, final)], a stream's pushes in ITS order -> (RS_STREAM table with out_off / pad unset, sorted
        into groups, groups: [round, (orig, new), first row, end row] -- a stream's r-th push of the call lies in round r, a round's rows
        at one rate pair make one launch --, order: order[q] = the push behind row q, commit: handle -> its new host record).  All in
        Python integers and before anything is launched; the records change only when the caller commits."""
        pool, commit, rows = self._pool("resample"), {}, []
        rnd, _ = SP.rounds(int(p[0]) for p in pushes)
        for i, (h, in_off, n_in, final) in enumerate(pushes):
            h = int(h)
            rec = pool.live(h, commit)
            L, M = RS.ratio(rec.orig, rec.new)
            p = RS.stream_plan(L, M, RS.geometry(L, M)[1], rec.pushed, rec.emitted, n_in, final)
            rows.append((rnd[i], (rec.orig, rec.new), i, (int(in_off), int(n_in), rec.pushed, p["total"], rec.emitted, p["n_out"], 0, h, rec.phase,
                                                          p["carry_in"], p["carry_out"], 0, 0)))
            commit[h] = rec._replace(pushed=rec.pushed + int(n_in), emitted=p["emitted"], phase=rec.phase ^ 1, done=bool(final))
        rows.sort(key=lambda e: e[:3])
        tab = np.zeros(len(rows), _lib.RS_STREAM)
        groups: list = []
        for q, (r, pair, _, row) in enumerate(rows):
            tab[q] = row
            if groups and groups[-1][:2] == [r, pair]:
                groups[-1][3] = q + 1
            else:
                groups.append([r, pair, q, q + 1])
        return tab, groups, [e[2] for e in rows], commit

    def resample_stream_step(self, x: torch.Tensor, pushes):
        """ONE step of many streams (ctts_resample_stream_step, one launch per distinct rate pair): `x`, a 1-D float32 device tensor,
        holds the new samples of every stream; `pushes` = [(handle, in_off, n_in, final)]: x[in_off, in_off + n_in) continue stream
        `handle` (n_in 0: nothing new), `final`: they are its last.  -> (y, off): stream i's chunk is y[off[i], off[i+1]) (possibly
        empty; `resample_stream_plan`'s n_out); the chunks of a stream, concatenated, are `resample` of its concatenated pushes, bit
        for bit, however they were cut.  A handle may appear once per call.  Every refusal (ValueError here, EngineError from the
        library) comes before the first launch and leaves all streams as they were."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("resample: a contiguous 1-D float32 device tensor")
        SP.check_pushes("resample", pushes, x.numel())
        tab, groups, order, commit = self._rs_descriptors(pushes)
        n_out = np.zeros(len(pushes), np.int64)
        n_out[order] = tab["n_out"]
        off = np.zeros(len(pushes) + 1, np.int64)
        np.cumsum(n_out, out=off[1:])
        if int(off[-1]) >= 1 << 31:
            raise ValueError("resample: the output would hold 2^31 samples or more")
        tab["out_off"] = off[:-1][order]
        pool = self._pool("resample")
        y = torch.empty((int(off[-1]),), dtype=torch.float32, device=x.device)
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(x.device)
        st = torch.cuda.current_stream(x.device)
        for _, (orig, new), lo, hi in groups:
            L, M = RS.ratio(orig, new)
            _lib.check(self.lib.ctts_resample_stream_step(
                x.data_ptr() if x.numel() else None, x.numel(), tab_d.data_ptr() + lo * tab.itemsize, tab[lo:hi].ctypes.data_as(C.c_void_p),
                hi - lo, y.data_ptr() if y.numel() else None, y.numel(), pool.buf["carry"].data_ptr(), pool.slots,
                self._resample_taps(orig, new).data_ptr(), L, M, RS.geometry(L, M)[1], st.cuda_stream), "ctts_resample_stream_step")
        tab_d.record_stream(st)
        pool.commit(commit)
        return y, off

    def time_scale_segments(self, wav: torch.Tensor, off, speeds):
        """packed segments at ONE SPEED EACH (`speeds[i]` for segment i): requests that were decoded together and want different speeds.
        One call per run of neighbouring segments at one speed, all into one packed output; segments at speed 1 are copied, not
        processed.  -> (tensor, offsets).  A segment's samples are those of `time_scale` on it alone, bit for bit."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        q = [TS.quantize(v) for v in speeds]
        if len(q) != len(off) - 1:
            raise ValueError("time_scale_segments: one speed per segment")
        if len(set(q)) == 1:
            return self.time_scale(wav, q[0][0] / q[0][1], off)
        if wav.dim() != 1 or int(off[-1]) != wav.numel() or off[0] != 0 or np.any(np.diff(off) <= 0):
            raise ValueError("time_scale_segments: a packed 1-D tensor covered by ascending offsets")
        runs = []                     # [first segment, one past the last, (num, den)]
        for i, v in enumerate(q):
            if runs and runs[-1][2] == v:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1, v])
        plans = [None if v[0] == v[1] else TS.plan(v[0] / v[1], off[a: b + 1] - off[a]) for a, b, v in runs]   # every refusal, before the first launch
        lens = np.diff(off).copy()
        for (a, b, _), p in zip(runs, plans):
            if p is not None:
                lens[a:b] = np.diff(p[2])
        off_out = np.zeros(len(off), np.int64)
        np.cumsum(lens, out=off_out[1:])
        if int(off_out[-1]) >= 1 << 31:
            raise ValueError("time_scale: the pack would hold 2^31 samples or more")
        x = wav.contiguous()
        y = torch.empty((int(off_out[-1]),), dtype=torch.float32, device=wav.device)
        for (a, b, v), p in zip(runs, plans):
            xi, yi = x[int(off[a]): int(off[b])], y[int(off_out[a]): int(off_out[b])]
            if p is None:
                yi.copy_(xi)
            else:
                path = torch.empty((int(p[3][-1]),), dtype=torch.int32, device=wav.device)
                self._time_scale_launch(xi, np.ascontiguousarray(off[a: b + 1] - off[a]), yi, path, p[2], p[3], v[0], v[1])
        return y, off_out

    # -- loudness normalisation (csrc/loudness.hip) -----------------------------------------------------------------------------------
    def _loudness_coef(self, rates):
        """the coefficient table of a call's distinct rates on the device, built once per set of rates -> (device, host, {rate: row})"""
        cache = self.__dict__.setdefault("_ln_coef", {})
        key = tuple(sorted(set(rates)))
        if key not in cache:
            host, index = LN.coef_table(key)
            cache[key] = (torch.from_numpy(host).to(self.device), host, index)
        return cache[key]

    def loudness_normalize(self, wav: torch.Tensor, target, offsets=None, groups=None, rates=None, return_stats: bool = False, out=None,
                           limiter=None):
        """ITU-R BS.1770-4 integrated loudness of a float32 device tensor and ONE gain per group that brings it to `target` LUFS
        (ctts_loudness_normalize_ragged; the definition, the +30 dB cap and the -1 dBFS ceiling of loudness.py): 1-D (one signal),
        [B, n] (rows, each alone), or 1-D packed with `offsets` (n_seg + 1 sample offsets, the ragged decoder's layout; every segment
        filtered as if alone).  `groups`: the table `float_to_int16_groups` takes -- segments groups[g] .. groups[g+1]-1 share one
        loudness, one peak and one gain; without it every segment is its own group.  `target`: one number of LUFS in -40 .. -5 or one
        per group; None leaves that group alone (bit for bit), and with every target None and no `return_stats` the input comes back
        untouched, with no launch.  `rates`: the segments' sample rates in Hz (one, or one per segment; default 24000), multiples of 10
        in 8000 .. 48000.  Returns a tensor of the input's shape (`out`, when given: a float32 device tensor of that shape, possibly
        `wav` itself), and with `return_stats` also the groups' records (a NumPy array of loudness.STATS: L, peak, g32, the block
        counts, the term that bound).  A group's record and samples do not depend on what it is packed with.  ValueError before any
        launch: a rate or target out of range, an empty segment, non-ascending offsets, a bad group table, 2^31 - 4096 samples.
        `limiter` (None: off; one bool, or one per group): a flagged group's gain is min(target term, +30 dB cap) -- the ceiling term
        is dropped, its record's bound is 0 or 1 -- and each of its segments goes through the look-ahead peak limiter alone at that
        gain (`peak_limit`, ctts_loudness_limited_ragged in front of it: no host round trip in between), also where the gain is 1
        (no target, a silent group).  With `return_stats` the limiter's records follow as a third element (limiter.STATS per
        segment; zeros for a segment outside a flagged group)."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("loudness_normalize: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("loudness_normalize: offsets go with a packed 1-D tensor")
        if wav.numel() == 0:
            raise ValueError("loudness_normalize: nothing to normalise")
        if wav.dim() == 2:
            offsets = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
        off, grp, rates, tg = LN.tables(wav.numel(), offsets, groups, rates, target)
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == wav.shape
                                    and out.is_contiguous()):
            raise ValueError("loudness_normalize: out is a contiguous float32 device tensor of the input's shape")
        lim = LM.per_row(limiter, len(grp) - 1, "loudness_normalize")
        if all(t is None for t in tg) and not return_stats:
            if lim is not None:                                   # nothing to measure: the limiter at unity gain
                return self._peak_limit_runs(wav, off, rates, np.repeat(lim, np.diff(grp)), None, out)[0]
            if out is None or out is wav:
                return wav
            out.copy_(wav)
            return out
        x = wav.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        y = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty_like(x)
        n_seg, n_grp = len(off) - 1, len(grp) - 1
        if lim is not None:
            return self._loudness_limited(wav, x, y, out, off, grp, rates, tg, lim, return_stats)
        coef_d, coef_h, index = self._loudness_coef(rates)
        ridx = np.array([index[r] for r in rates], dtype=np.int32)
        tgt = np.array([math.nan if t is None else t for t in tg], dtype=np.float64)
        off_p = off.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_loudness_normalize_ragged_scratch_bytes(off_p, n_seg))
        if sb == 0:
            _lib.check(-1, "ctts_loudness_normalize_ragged")      # the offsets were refused: the library's message says why
        dev = wav.device
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), tgt.view(np.uint8), ridx.view(np.uint8), grp.view(np.uint8)])).to(dev)   # one upload
        work = device_scratch(LN.STATS.itemsize * n_grp + sb, dev)                                       # the records, then the scratch
        st = torch.cuda.current_stream(dev)
        base = tabs.data_ptr()
        _lib.check(self.lib.ctts_loudness_normalize_ragged(
            x.data_ptr(), y.data_ptr(), base, off_p, n_seg, base + off.nbytes + tgt.nbytes, ridx.ctypes.data_as(C.c_void_p),
            coef_d.data_ptr(), coef_h.ctypes.data_as(C.c_void_p), int(coef_h.shape[0]),
            base + off.nbytes + tgt.nbytes + ridx.nbytes, grp.ctypes.data_as(C.c_void_p), n_grp, base + off.nbytes,
            tgt.ctypes.data_as(C.c_void_p), work.data_ptr(), work.data_ptr() + LN.STATS.itemsize * n_grp, sb, st.cuda_stream),
            "ctts_loudness_normalize_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        if out is not None and y is not out:
            out.copy_(y)
            y = out
        y = y.view(wav.shape)
        if return_stats:
            return y, work[: LN.STATS.itemsize * n_grp].cpu().numpy().view(LN.STATS)
        return y

    def _loudness_limited(self, wav, x, y, out, off, grp, rates, tg, lim, return_stats):
        """`loudness_normalize` with a limiter table: ctts_loudness_limited_ragged (the flagged groups' gains without the ceiling
        term, their segments left unscaled in y, every segment's gain in a device table), then the limiter over the flagged
        segments in place in y, reading that table"""
        n_seg, n_grp = len(off) - 1, len(grp) - 1
        coef_d, coef_h, index = self._loudness_coef(rates)
        ridx = np.array([index[r] for r in rates], dtype=np.int32)
        tgt = np.array([math.nan if t is None else t for t in tg], dtype=np.float64)
        lmt = np.array(lim, dtype=np.int32)
        off_p = off.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_loudness_normalize_ragged_scratch_bytes(off_p, n_seg))
        if sb == 0:
            _lib.check(-1, "ctts_loudness_limited_ragged")
        dev = wav.device
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), tgt.view(np.uint8), ridx.view(np.uint8), grp.view(np.uint8), lmt.view(np.uint8)])).to(dev)
        work = device_scratch(LN.STATS.itemsize * n_grp + sb, dev)                                       # the records, then the scratch
        gains = torch.empty((n_seg,), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev)
        base = tabs.data_ptr()
        p_tgt, p_ridx = base + off.nbytes, base + off.nbytes + tgt.nbytes
        p_grp = p_ridx + ridx.nbytes
        _lib.check(self.lib.ctts_loudness_limited_ragged(
            x.data_ptr(), y.data_ptr(), base, off_p, n_seg, p_ridx, ridx.ctypes.data_as(C.c_void_p),
            coef_d.data_ptr(), coef_h.ctypes.data_as(C.c_void_p), int(coef_h.shape[0]),
            p_grp, grp.ctypes.data_as(C.c_void_p), n_grp, p_tgt, tgt.ctypes.data_as(C.c_void_p),
            p_grp + grp.nbytes, lmt.ctypes.data_as(C.c_void_p), gains.data_ptr(),
            work.data_ptr(), work.data_ptr() + LN.STATS.itemsize * n_grp, sb, st.cuda_stream), "ctts_loudness_limited_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        yv = y.view(-1)
        lstats = self._peak_limit_runs(yv, off, rates, np.repeat(lim, np.diff(grp)), gains, yv, return_stats)[1]
        if out is not None and y is not out:
            out.copy_(y)
            y = out
        y = y.view(wav.shape)
        if return_stats:
            return y, work[: LN.STATS.itemsize * n_grp].cpu().numpy().view(LN.STATS), lstats
        return y

    # -- look-ahead peak limiter (csrc/limiter.hip) ------------------------------------------------------------------------------------
    def _peak_limit_runs(self, wav, off, rates, flags, gains, out, return_stats: bool = False):
        """the limiter over the flagged segments of a pack, run of neighbours by run (one call where every segment is flagged);
        `gains`: None (unity) or a float32 device tensor with one gain per segment -> (tensor of wav's shape, records or None)"""
        flat = wav.contiguous().view(-1)
        if out is wav:
            y = flat                                              # in place
        else:
            y = torch.empty_like(flat) if out is None else out.view(-1)
            y.copy_(flat)
        recs = np.zeros(len(off) - 1, dtype=LM.STATS) if return_stats else None
        a = 0
        while a < len(flags):
            if not flags[a]:
                a += 1
                continue
            b = a
            while b < len(flags) and flags[b]:
                b += 1
            sub = y[int(off[a]): int(off[b])]
            res = self.peak_limit(sub, offsets=off[a: b + 1] - off[a], rates=[int(r) for r in rates[a:b]],
                                  gains=None if gains is None else gains[a:b], return_stats=return_stats, out=sub)
            if return_stats:
                recs[a:b] = res[1]
            a = b
        return y.view(wav.shape), recs

    def peak_limit(self, wav: torch.Tensor, offsets=None, rates=None, gains=None, return_stats: bool = False, out=None):
        """The look-ahead peak limiter on a float32 device tensor (ctts_peak_limit_ragged; the definition of limiter.py): 1-D (one
        signal), [B, n] (rows, each alone), or 1-D packed with `offsets` (n_seg + 1 sample offsets, the ragged decoder's layout;
        every segment limited as if alone, its windows never reach a neighbour).  `gains`: the float32 pre-gain -- None (1), one
        number, one per segment, or a float32 device tensor with one per segment (the loudness stage's).  `rates`: the segments'
        sample rates in Hz (one, or one per segment; default 24000), multiples of 10 in 8000 .. 48000: the look-ahead and the
        smoothing are 10 ms each.  No sample of the result exceeds float32(10^(-1/20)) in magnitude, and a segment with no sample
        over the threshold comes back as gain * x bit for bit.  Returns a tensor of the input's shape (`out`, when given: a float32
        device tensor of that shape, possibly `wav` itself), and with `return_stats` also the segments' records (a NumPy array of
        limiter.STATS: the pre-gain, the smallest gain, the samples over the threshold, the samples touched).  A segment's samples
        and record do not depend on what it is packed with.  ValueError before any launch: a rate or gain out of range, an empty
        segment, non-ascending offsets, 2^31 - 4096 samples, more than 65535 segments."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("peak_limit: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("peak_limit: offsets go with a packed 1-D tensor")
        if wav.numel() == 0:
            raise ValueError("peak_limit: nothing to limit")
        if wav.dim() == 2:
            offsets = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
        on_dev = isinstance(gains, torch.Tensor)
        off, rt, g = LM.tables(wav.numel(), offsets, rates, None if on_dev else gains)
        n_seg = len(off) - 1
        if on_dev and not (gains.is_cuda and gains.dtype == torch.float32 and gains.dim() == 1 and gains.numel() == n_seg and gains.is_contiguous()):
            raise ValueError("peak_limit: gains on the device are a contiguous float32 tensor with one per segment")
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == wav.shape
                                    and out.is_contiguous()):
            raise ValueError("peak_limit: out is a contiguous float32 device tensor of the input's shape")
        x = wav.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        y = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty_like(x)
        off_p = off.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_peak_limit_ragged_scratch_bytes(off_p, n_seg))
        if sb == 0:
            _lib.check(-1, "ctts_peak_limit_ragged")              # the offsets were refused: the library's message says why
        dev = wav.device
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), rt.view(np.uint8), g.view(np.uint8)])).to(dev)   # one upload
        work = device_scratch(-(-LM.STATS.itemsize * n_seg // 16) * 16 + sb, dev)                                    # the records, then the scratch
        st = torch.cuda.current_stream(dev)
        base = tabs.data_ptr()
        _lib.check(self.lib.ctts_peak_limit_ragged(
            x.data_ptr(), y.data_ptr(), base, off_p, n_seg, base + off.nbytes, rt.ctypes.data_as(C.c_void_p),
            gains.data_ptr() if on_dev else base + off.nbytes + rt.nbytes, work.data_ptr(),
            work.data_ptr() + -(-LM.STATS.itemsize * n_seg // 16) * 16, sb, st.cuda_stream), "ctts_peak_limit_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        if on_dev:
            gains.record_stream(st)
        if out is not None and y is not out:
            out.copy_(y.view(out.shape))
            y = out
        y = y.view(wav.shape)
        if return_stats:
            return y, work[: LM.STATS.itemsize * n_seg].cpu().numpy().view(LM.STATS)
        return y

    # -- dynamic range compressor (csrc/compressor.hip) ---------------------------------------------------------------------------------
    def compress(self, wav: torch.Tensor, spec, offsets=None, rates=None, return_stats: bool = False, out=None):
        """The look-ahead compressor on a float32 device tensor (ctts_compress_ragged; the definition of compressor.py): 1-D (one
        signal), [B, n] (rows, each alone), or 1-D packed with `offsets` (n_seg + 1 sample offsets, the ragged decoder's layout;
        every segment compressed as if alone, its windows never reach a neighbour).  `spec`: True (the defaults) or a dict with any
        of threshold_db, ratio, knee_db, attack_ms, hold_ms -- one for all, or a list with one per segment; a segment whose spec is
        None or False is copied through.  `rates`: the segments' sample rates in Hz (one, or one per segment; default 24000),
        multiples of 10 in 8000 .. 48000: a block is 1 ms.  No sample is raised (g <= 1), and a segment whose block peaks all lie
        under the knee comes back bit for bit.  Returns a tensor of the input's shape (`out`, when given: a float32 device tensor of
        that shape, possibly `wav` itself), and with `return_stats` also the segments' records (a NumPy array of compressor.STATS:
        the smallest gain, the blocks under the curve, the samples touched, the largest block peak).  A segment's samples and record
        do not depend on what it is packed with.  ValueError before any launch: a bad spec, a rate out of range, an empty segment,
        non-ascending offsets, 2^31 - 4096 samples, more than 65535 segments, no segment that asks for the compressor."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("compress: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("compress: offsets go with a packed 1-D tensor")
        if wav.numel() == 0:
            raise ValueError("compress: nothing to compress")
        if wav.dim() == 2:
            offsets = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
        off, rt, par, tabs_h, _ = CP.tables(wav.numel(), spec, offsets, rates)
        n_seg = len(off) - 1
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == wav.shape
                                    and out.is_contiguous()):
            raise ValueError("compress: out is a contiguous float32 device tensor of the input's shape")
        x = wav.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        y = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty_like(x)
        off_p = off.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_compress_ragged_scratch_bytes(off_p, n_seg))
        if sb == 0:
            _lib.check(-1, "ctts_compress_ragged")                # the offsets were refused: the library's message says why
        dev = wav.device
        tabs_h = np.ascontiguousarray(tabs_h)
        host = [tabs_h.view(np.uint8).reshape(-1), off.view(np.uint8), rt.view(np.uint8), par.view(np.uint8).reshape(-1)]   # the gain tables first: 16-byte aligned
        tabs = torch.from_numpy(np.concatenate(host)).to(dev)                                                              # one upload
        rec_bytes = -(-CP.STATS.itemsize * n_seg // 16) * 16
        work = device_scratch(rec_bytes + sb, dev)                                                                         # the records, then the scratch
        st = torch.cuda.current_stream(dev)
        base = tabs.data_ptr()
        p_off = base + tabs_h.nbytes
        _lib.check(self.lib.ctts_compress_ragged(
            x.data_ptr(), y.data_ptr(), p_off, off_p, n_seg, p_off + off.nbytes, rt.ctypes.data_as(C.c_void_p),
            p_off + off.nbytes + rt.nbytes, par.ctypes.data_as(C.c_void_p), base, tabs_h.ctypes.data_as(C.c_void_p), int(tabs_h.shape[0]),
            work.data_ptr(), work.data_ptr() + rec_bytes, sb, st.cuda_stream), "ctts_compress_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        if out is not None and y is not out:
            out.copy_(y.view(out.shape))
            y = out
        y = y.view(wav.shape)
        if return_stats:
            return y, work[: CP.STATS.itemsize * n_seg].cpu().numpy().view(CP.STATS)
        return y

    # -- output equaliser (csrc/equalizer.hip) ------------------------------------------------------------------------------------------
    def equalize(self, wav: torch.Tensor, spec, offsets=None, rates=None, out=None):
        """The output equaliser on a float32 device tensor (ctts_equalize_ragged; the definition of equalizer.py): 1-D (one signal),
        [B, n] (rows, each alone), or 1-D packed with `offsets` (n_seg + 1 sample offsets, the ragged decoder's layout; every segment
        filtered as if alone, from zero state at its first sample).  `spec`: a preset name ("telephone", "rumble") or a dict with any
        of highpass_hz, lowshelf {hz, db}, highshelf {hz, db}, peaks [{hz, db, q}, ...], at most four sections -- one for all, or a
        list with one per segment; a segment whose spec is None, False or the identity is copied through bit for bit.  `rates`: the
        segments' sample rates in Hz (one, or one per segment; default 24000), multiples of 10 in 8000 .. 48000; a section's hz lies
        in 20 .. 0.45 of its segment's rate.  The result is the serial float64 cascade rounded once to float32, to within one float32
        ulp where a value sits on a rounding boundary.  Returns a tensor of the input's shape (`out`, when given: a float32 device
        tensor of that shape, possibly `wav` itself).  A segment's samples do not depend on what it is packed with.  ValueError
        before any launch: a bad spec, a rate out of range, an empty segment, non-ascending offsets, 2^31 - 4096 samples, more than
        65535 segments, no segment that asks for the equaliser."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("equalize: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("equalize: offsets go with a packed 1-D tensor")
        if wav.numel() == 0:
            raise ValueError("equalize: nothing to equalise")
        if wav.dim() == 2:
            offsets = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
        off, sel, coef_h, _ = EQ.tables(wav.numel(), spec, offsets, rates)
        n_seg = len(off) - 1
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == wav.shape
                                    and out.is_contiguous()):
            raise ValueError("equalize: out is a contiguous float32 device tensor of the input's shape")
        x = wav.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        y = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty_like(x)
        off_p = off.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_equalize_ragged_scratch_bytes(off_p, n_seg))
        if sb == 0:
            _lib.check(-1, "ctts_equalize_ragged")                # the offsets were refused: the library's message says why
        dev = wav.device
        host = [coef_h.view(np.uint8).reshape(-1), off.view(np.uint8), sel.view(np.uint8)]                  # the coefficient rows first: 16-byte aligned
        tabs = torch.from_numpy(np.concatenate(host)).to(dev)                                              # one upload
        work = device_scratch(sb, dev)
        st = torch.cuda.current_stream(dev)
        base = tabs.data_ptr()
        p_off = base + coef_h.nbytes
        _lib.check(self.lib.ctts_equalize_ragged(
            x.data_ptr(), y.data_ptr(), p_off, off_p, n_seg, p_off + off.nbytes, sel.ctypes.data_as(C.c_void_p),
            base, coef_h.ctypes.data_as(C.c_void_p), int(coef_h.shape[0]), work.data_ptr(), sb, st.cuda_stream), "ctts_equalize_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        if out is not None and y is not out:
            out.copy_(y.view(out.shape))
            y = out
        return y.view(wav.shape)

    # -- the compressor of streams: per-stream device state (csrc/compressor.hip, compress_stream_*_k) -----------------------------------
    def compress_stream_open(self, rate: int, spec=True) -> int:
        """A stream of the compressor at `rate` Hz with `spec` (True: the defaults, or a dict of `compress`'s fields): -> its handle, a
        slot of the engine's state pool.  The first step of a stream reads neither carry nor history, so those are not cleared; the
        slot's RECORD is set to (1, 0, 0, 0) here, by a device-side copy in stream order in front of the stream's first step -- the
        steps touch it by atomics only.  ValueError for a rate or spec `compress` refuses, and for a spec that is off."""
        rate = LN.check_rate(rate)
        spec = CP.check(spec, "compress_stream_open")
        if spec is None:
            raise ValueError("compress_stream_open: the spec is off, there is nothing to compress")
        pool = self._pool("compress")
        slot = pool.open(SP.CompressRec(rate, spec, 0, 0, 0, False))
        if "_cp_rec0" not in self.__dict__:
            self._cp_rec0 = torch.from_numpy(np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32).view(np.int32)).to(self.device)
        pool.buf["stats"][slot].copy_(self._cp_rec0)
        return slot

    def compress_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._pool("compress").close(handle)

    def compress_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._pool("compress").in_use

    def compress_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`compressor.stream_plan` of the stream's next push: what a step with `n_in` more samples would emit and keep"""
        rec = self._pool("compress").live(handle)
        A, H = CP.blocks(rec.spec)
        return CP.stream_plan(rec.rate // 1000, A, rec.pushed, rec.emitted, n_in, final, H)

    def compress_stream_stats(self, handle: int) -> np.ndarray:
        """the stream's compressor.STATS record so far (a device read: it waits for the steps so far): the blocks counted as their
        gains were computed, the samples as they were emitted; after the last push it is `compress`'s record of the whole signal."""
        pool = self._pool("compress")
        pool.get(handle)
        return pool.buf["stats"][int(handle)].cpu().numpy().view(CP.STATS)[0]

    def _cp_descriptors(self, pushes):
        """pushes [(handle, in_off, n_in, final)], one per stream -> (CP_STREAM table with out_off unset, in the pushes' order, the
        distinct specs' gain tables [n_tab, TABLE], commit: handle -> its new host record).  All in Python integers and before
        anything is launched; the records change only when the caller commits."""
        pool, commit, specs = self._pool("compress"), {}, {}
        tab = np.zeros(len(pushes), _lib.CP_STREAM)
        cb = 0
        for i, (h, in_off, n_in, final) in enumerate(pushes):
            h = int(h)
            if h in commit:
                raise ValueError("compress: a stream appears twice in one step")
            rec = pool.live(h)
            B = rec.rate // 1000
            A, H = CP.blocks(rec.spec)
            p = CP.stream_plan(B, A, rec.pushed, rec.emitted, n_in, final, H)
            nbc0, nbc1 = rec.pushed // B, -(-p["total"] // B) if final else p["total"] // B
            h_in = nbc0 - max(0, rec.emitted // B - A - H - 1)
            tab[i] = (int(in_off), int(n_in), rec.pushed, p["total"] if final else -1, rec.emitted, p["n_out"], 0, cb, h, rec.phase, rec.rate,
                      A, H, specs.setdefault(rec.spec, len(specs)), p["carry_in"], p["carry_out"], h_in, p["c_keep"])
            cb += nbc1 - nbc0
            commit[h] = rec._replace(pushed=p["total"], emitted=p["emitted"], phase=rec.phase ^ 1, done=bool(final))
        return tab, np.ascontiguousarray(np.stack([CP.table(s) for s in specs])), commit, cb

    def compress_stream_step(self, x: torch.Tensor, pushes, out: Optional[torch.Tensor] = None, out_off=None):
        """ONE step of many compressor streams (ctts_compress_stream_step, two launches whatever their number, rates and specs): `x`,
        a 1-D float32 device tensor, holds the new samples of every stream; `pushes` = [(handle, in_off, n_in, final)]: x[in_off,
        in_off + n_in) continue stream `handle` (n_in 0: nothing new), `final`: they are its last.  -> (y, off): stream i's chunk is
        y[off[i], off[i+1]) (possibly empty; `compress_stream_plan`'s n_out), a tensor of its own -- x is never written.  A stream
        lags by (A + 1) blocks of 1 ms and its open block, whatever its hold; the chunks of a stream, end to end, are `compress` of
        its concatenated pushes with the stream's spec, bit for bit, however they were cut, and after the last push
        `compress_stream_stats` is that call's record.  A handle may appear once per call.  `out` with `out_off`: a contiguous 1-D
        float32 device tensor of the caller's (not x) and one offset per push -- stream i's chunk is written to out[out_off[i] ..]
        instead, and (out, out_off) comes back.  Every refusal (ValueError here, EngineError from the library) comes before the
        first launch and leaves all streams as they were."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("compress: a contiguous 1-D float32 device tensor")
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 1
                                    and out.is_contiguous() and out_off is not None and len(out_off) == len(pushes)):
            raise ValueError("compress: out is a contiguous 1-D float32 device tensor, with one offset per push")
        SP.check_pushes("compress", pushes, x.numel(), once=False)            # a stream twice: `_cp_descriptors` refuses
        tab, tabs_h, commit, n_new = self._cp_descriptors(pushes)
        off = np.zeros(len(pushes) + 1, np.int64)
        np.cumsum(tab["n_out"], out=off[1:])
        if int(off[-1]) >= 1 << 31:
            raise ValueError("compress: the output would hold 2^31 samples or more")
        if out is None:
            tab["out_off"] = off[:-1]
            y = torch.empty((int(off[-1]),), dtype=torch.float32, device=x.device)
        else:
            off = np.array([int(v) for v in out_off], dtype=np.int64)
            if np.any(off < 0) or np.any(off + tab["n_out"] > out.numel()):
                raise ValueError("compress: a chunk lies outside `out`")
            tab["out_off"], y = off, out
        if x.data_ptr() % 16:
            x = x.clone()                                                     # the peak launch loads 16 bytes at a time
        pool = self._pool("compress")
        up = torch.from_numpy(np.concatenate([tabs_h.view(np.uint8).reshape(-1), tab.view(np.uint8)])).to(x.device)   # one upload, the gain tables first: 16-byte aligned
        sb = int(self.lib.ctts_compress_stream_scratch_bytes(n_new))
        if sb == 0:
            raise ValueError("compress: the step would complete 2^31 blocks or more")
        work = device_scratch(sb, x.device)
        st = torch.cuda.current_stream(x.device)
        _lib.check(self.lib.ctts_compress_stream_step(
            x.data_ptr() if x.numel() else None, x.numel(), up.data_ptr() + tabs_h.nbytes, tab.ctypes.data_as(C.c_void_p), len(tab),
            up.data_ptr(), tabs_h.ctypes.data_as(C.c_void_p), int(tabs_h.shape[0]), y.data_ptr() if y.numel() else None, y.numel(),
            pool.buf["carry"].data_ptr(), pool.buf["hist"].data_ptr(), pool.buf["stats"].data_ptr(), pool.slots, work.data_ptr(), sb,
            st.cuda_stream), "ctts_compress_stream_step")
        up.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        pool.commit(commit)
        return y, off

    # -- the limiter of streams: per-stream device state (csrc/limiter.hip, limiter_stream_k) ---------------------------------------------
    def peak_limit_stream_open(self, rate: int, gain=1.0) -> int:
        """A stream of the limiter at `rate` Hz with the float32 pre-gain `gain` (any positive finite float32): -> its handle, a slot
        of the engine's state pool.  The slot is fresh by construction -- the first step of a stream reads no carry, and the step
        that carries a stream's first push resets the slot's record on the device in front of its own atomics -- so nothing is
        cleared here.  ValueError for a rate or gain `peak_limit` refuses."""
        rate = LN.check_rate(rate)
        g = np.float32(gain)
        if not (np.isfinite(g) and g > 0):
            raise ValueError("limiter: a pre-gain is a positive finite number")
        return self._pool("limiter").open(SP.LimiterRec(rate, g, 0, 0, 0, False))

    def peak_limit_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._pool("limiter").close(handle)

    def peak_limit_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._pool("limiter").in_use

    def peak_limit_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`limiter.stream_plan` of the stream's next push: what a step with `n_in` more samples would emit and keep"""
        rec = self._pool("limiter").live(handle)
        return LM.stream_plan(rec.rate // 100, rec.pushed, rec.emitted, n_in, final)

    def peak_limit_stream_stats(self, handle: int) -> np.ndarray:
        """the stream's limiter.STATS record, counted over the samples emitted so far (a device read: it waits for the steps so far);
        after the last push it is `peak_limit`'s record of the whole signal.  Before the first push nothing has been counted."""
        pool = self._pool("limiter")
        rec = pool.get(handle)
        out = np.zeros((), dtype=LM.STATS)
        if rec.pushed == 0:                                       # the slot's record is reset by the step of the first push
            out["g32"], out["min_gain"] = rec.gain, 1.0
            return out
        return pool.buf["stats"][int(handle)].cpu().numpy().view(LM.STATS)[0]

    def _lm_descriptors(self, pushes):
        """pushes [(handle, in_off, n_in, final)], one per stream -> (LM_STREAM table with out_off unset, in the pushes' order,
        commit: handle -> its new host record).  All in Python integers and before anything is launched; the records change only
        when the caller commits."""
        pool, commit = self._pool("limiter"), {}
        tab = np.zeros(len(pushes), _lib.LM_STREAM)
        for i, (h, in_off, n_in, final) in enumerate(pushes):
            h = int(h)
            if h in commit:
                raise ValueError("limiter: a stream appears twice in one step")
            rec = pool.live(h)
            p = LM.stream_plan(rec.rate // 100, rec.pushed, rec.emitted, n_in, final)
            tab[i] = (int(in_off), int(n_in), rec.pushed, p["total"] if final else -1, rec.emitted, p["n_out"], 0, h, rec.phase, p["carry_in"],
                      p["carry_out"], rec.rate, rec.gain)
            commit[h] = rec._replace(pushed=p["total"], emitted=p["emitted"], phase=rec.phase ^ 1, done=bool(final))
        return tab, commit

    def peak_limit_stream_step(self, x: torch.Tensor, pushes, out: Optional[torch.Tensor] = None, out_off=None):
        """ONE step of many streams (ctts_peak_limit_stream_step, one launch whatever their rates and gains): `x`, a 1-D float32
        device tensor, holds the new samples of every stream; `pushes` = [(handle, in_off, n_in, final)]: x[in_off, in_off + n_in)
        continue stream `handle` (n_in 0: nothing new), `final`: they are its last.  -> (y, off): stream i's chunk is
        y[off[i], off[i+1]) (possibly empty; `peak_limit_stream_plan`'s n_out), a tensor of its own -- x is never written.  A stream
        lags by 2 W = rate // 50 samples; the chunks of a stream, concatenated, are `peak_limit` of its concatenated pushes with the
        stream's gain, bit for bit, however they were cut, and after the last push `peak_limit_stream_stats` is that call's record.
        A handle may appear once per call.  `out` with `out_off`: a contiguous 1-D float32 device tensor of the caller's (not x) and
        one offset per push -- stream i's chunk is written to out[out_off[i] ..] instead, and (out, out_off) comes back.  Every
        refusal (ValueError here, EngineError from the library) comes before the first launch and leaves all streams as they were."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("limiter: a contiguous 1-D float32 device tensor")
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 1
                                    and out.is_contiguous() and out_off is not None and len(out_off) == len(pushes)):
            raise ValueError("limiter: out is a contiguous 1-D float32 device tensor, with one offset per push")
        SP.check_pushes("limiter", pushes, x.numel(), once=False)             # a stream twice: `_lm_descriptors` refuses
        tab, commit = self._lm_descriptors(pushes)
        off = np.zeros(len(pushes) + 1, np.int64)
        np.cumsum(tab["n_out"], out=off[1:])
        if int(off[-1]) >= 1 << 31:
            raise ValueError("limiter: the output would hold 2^31 samples or more")
        if out is None:
            tab["out_off"] = off[:-1]
            y = torch.empty((int(off[-1]),), dtype=torch.float32, device=x.device)
        else:
            off = np.array([int(v) for v in out_off], dtype=np.int64)
            if np.any(off < 0) or np.any(off + tab["n_out"] > out.numel()):
                raise ValueError("limiter: a chunk lies outside `out`")
            tab["out_off"], y = off, out
        pool = self._pool("limiter")
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(x.device)
        st = torch.cuda.current_stream(x.device)
        _lib.check(self.lib.ctts_peak_limit_stream_step(
            x.data_ptr() if x.numel() else None, x.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(tab),
            y.data_ptr() if y.numel() else None, y.numel(), pool.buf["carry"].data_ptr(), pool.buf["stats"].data_ptr(), pool.slots,
            st.cuda_stream), "ctts_peak_limit_stream_step")
        tab_d.record_stream(st)
        pool.commit(commit)
        return y, off

    # -- pause control (csrc/pauses.hip) ------------------------------------------------------------------------------------------------
    def trim_pauses(self, wav: torch.Tensor, spec, offsets=None, rates=None, return_stats: bool = False):
        """Trims the silence at every segment's edges and caps its inner pauses (ctts_trim_pauses_ragged; the definition of
        pauses.py): 1-D (one signal) -> a tensor; [B, n] (rows, each alone) -> (packed, offsets); 1-D packed with `offsets` (n_seg + 1
        sample offsets, the ragged decoder's layout) -> (packed, offsets), `offsets` a host int64 array.  `spec`: None, True (the
        defaults), a `pauses.PauseSpec` or a dict of its fields -- one for all, or a list with one per segment; a segment whose spec is
        None is copied through bit for bit, and with every spec None and no `return_stats` the input comes back untouched, with no
        launch.  `rates`: the segments' sample rates in Hz (one, or one per segment; default 24000), 8000 .. 48000.  With
        `return_stats` the segments' records follow (int32 [n_seg, 8], `pauses.RECORD`).  The output's length depends on the samples:
        the call ends in ONE device-to-host copy of the new offsets and the records, its only synchronisation, however many segments
        there are.  A segment's samples and record do not depend on what it is packed with.  ValueError before any launch: a bad spec,
        a rate out of range, an empty segment, non-ascending offsets, 2^31 - 4096 samples, more than 65535 segments."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
            raise ValueError("trim_pauses: a float32 device tensor, 1-D or [B, n]")
        if offsets is not None and wav.dim() != 1:
            raise ValueError("trim_pauses: offsets go with a packed 1-D tensor")
        if wav.numel() == 0:
            raise ValueError("trim_pauses: nothing to trim")
        single = wav.dim() == 1 and offsets is None
        if wav.dim() == 2:
            offsets = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
        tb = PA.tables(np.array([0, wav.numel()], dtype=np.int64) if offsets is None else offsets, rates, spec)
        off, rows, fbase, fade = tb["off"], tb["rows"], tb["fbase"], tb["fade"]
        if int(off[-1]) != wav.numel():
            raise ValueError("trim_pauses: the offsets do not cover the tensor")
        n_seg = len(off) - 1
        if all(s is None for s in tb["specs"]) and not return_stats:
            flat = wav.reshape(-1)
            return flat if single else (flat, off)
        x = wav.contiguous().view(-1)
        if x.data_ptr() % 16:
            x = x.clone()
        dev = wav.device
        y = torch.empty_like(x)
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), fbase.view(np.uint8), rows.reshape(-1).view(np.uint8), fade.view(np.uint8)])).to(dev)   # one upload
        res_bytes = 8 * (n_seg + 1) + 4 * PA.REC * n_seg                                                  # off_out, then the records
        work = device_scratch(-(-res_bytes // 16) * 16 + tb["scratch"], dev)
        st = torch.cuda.current_stream(dev)
        base, wp = tabs.data_ptr(), work.data_ptr()
        _lib.check(self.lib.ctts_trim_pauses_ragged(
            x.data_ptr(), y.data_ptr(), base, off.ctypes.data_as(C.c_void_p), base + off.nbytes, fbase.ctypes.data_as(C.c_void_p),
            base + off.nbytes + fbase.nbytes, rows.ctypes.data_as(C.c_void_p), n_seg, base + off.nbytes + fbase.nbytes + rows.nbytes,
            int(fade.size), wp, wp + 8 * (n_seg + 1), wp + -(-res_bytes // 16) * 16, tb["scratch"], st.cuda_stream), "ctts_trim_pauses_ragged")
        tabs.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        res = work[:res_bytes].cpu().numpy()                                                              # the one copy, and the one wait
        off_out = res[: 8 * (n_seg + 1)].view(np.int64).copy()
        y = y[: int(off_out[-1])]
        out = (y,) if single else (y, off_out)
        if return_stats:
            out = (*out, res[8 * (n_seg + 1):].view(np.int32).reshape(n_seg, PA.REC).copy())
        return out[0] if len(out) == 1 else out

    # -- pause control of streams: per-stream device state (csrc/pauses.hip, pause_stream_walk_k) -----------------------------------------
    def trim_pauses_stream_open(self, rate: int, spec=True) -> int:
        """A pause stream at `rate` Hz with `spec` (True: the defaults, a `pauses.PauseSpec` or a dict of its fields): -> its handle, a
        slot of the engine's state pool.  The slot is fresh by construction -- the step that carries a stream's first sample reads
        neither state nor carry -- so nothing is cleared here.  ValueError: a bad rate or spec, no spec, a spec that makes a stream
        hold more than `pauses.STREAM_FRAMES` frames."""
        rate, spec = PA.check_stream(rate, spec)
        return self._pool("pauses").open(SP.PauseRec(rate, spec, 0, 0, False, 0, 0))

    def trim_pauses_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._pool("pauses").close(handle)

    def trim_pauses_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._pool("pauses").in_use

    def trim_pauses_stream_stats(self, handle: int) -> dict:
        """the stream so far: `record` (int32 [8], `pauses.RECORD`, a device read that waits for the steps so far; after the last push
        it is `trim_pauses`' record of the whole signal, all zero for a stream that ended empty), `pushed` and `emitted` samples,
        `held` frames that wait, `done`"""
        pool = self._pool("pauses")
        rec = pool.get(handle)
        record = np.zeros(PA.REC, dtype=np.int32) if rec.pushed == 0 else pool.buf["state"][int(handle), 3: 3 + PA.REC].cpu().numpy()
        return dict(record=record, pushed=rec.pushed, emitted=rec.emitted, held=rec.held, done=rec.done)

    def _pa_descriptors(self, pushes):
        """pushes [(handle, in_off, n_in, final)], one per stream -> (PA_STREAM table, the distinct frames' fade tables one behind the
        other, commit: handle -> its host record behind the step, `held` and `emitted` as they were: the step's copy brings those).
        All in Python integers and before anything is launched; the records change only when the caller commits.  A stream's chunk
        gets room for what may wait and what arrives."""
        pool = self._pool("pauses")
        tab = np.zeros(len(pushes), _lib.PA_STREAM)
        commit, fade_off, parts = {}, {}, []
        out = fr = ls = 0
        for i, (h, in_off, n_in, final) in enumerate(pushes):
            h, in_off, n_in = int(h), int(in_off), int(n_in)
            if h in commit:
                raise ValueError("pauses: a stream appears twice in one step")
            rec = pool.live(h)
            rate, spec, pushed, phase = rec.rate, rec.spec, rec.pushed, rec.phase
            if n_in < 0 or in_off < 0:
                raise ValueError("pauses: a push cannot be negative")
            if pushed + n_in >= 1 << 31:
                raise ValueError("pauses: the stream would hold 2^31 samples or more")
            F, pad, lead, tail, P, thr = PA.stream_row(rate, spec)
            if F not in fade_off:
                fade_off[F] = sum(len(p) for p in parts)
                parts.append(PA.fade_table(F))
            need, avail = PA.stream_need(spec), pushed % F + n_in
            nf = avail // F + (1 if final and avail % F else 0)
            n_list = 2 * need + nf + 1
            tab[i] = (in_off, n_in, pushed, out, fr, ls, h, phase, need, int(bool(final)), F, pad, lead, tail, P, thr, fade_off[F], n_list)
            out, fr, ls = out + need * F + avail, fr + nf, ls + n_list
            commit[h] = rec._replace(pushed=pushed + n_in, phase=phase ^ 1, done=bool(final))
        if out >= 1 << 31:
            raise ValueError("pauses: the output would hold 2^31 samples or more")
        return tab, np.ascontiguousarray(np.concatenate(parts)), commit

    def trim_pauses_stream_step(self, x: torch.Tensor, pushes):
        """ONE step of many pause streams (ctts_trim_pauses_stream_step: three launches whatever their number, rates and specs): `x`, a
        1-D float32 device tensor, holds the new samples of every stream; `pushes` = [(handle, in_off, n_in, final)]: x[in_off, in_off
        + n_in) continue stream `handle` (n_in 0: nothing new), `final`: they are its last.  -> (y, off): stream i's chunk is
        y[off[i], off[i+1]) (possibly empty), a tensor of its own -- x is never written.  The chunks of a stream, concatenated, are
        `trim_pauses` of its concatenated pushes bit for bit, however they were cut (`pauses.py`: what a push emits, and the lags).
        A chunk's length depends on the samples: the step ends in ONE device-to-host copy of the streams' counts, its only
        synchronisation.  A handle may appear once per call.  Every refusal (ValueError here, EngineError from the library) comes
        before the first launch and leaves all streams as they were."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()):
            raise ValueError("pauses: a contiguous 1-D float32 device tensor")
        SP.check_pushes("pauses", pushes, x.numel(), once=False)              # a stream twice: `_pa_descriptors` refuses
        tab, fade, commit = self._pa_descriptors(pushes)
        n, dev = len(tab), x.device
        room = int(tab["out_off"][-1]) + int(tab["need"][-1]) * int(tab["F"][-1]) + int(tab["pos"][-1]) % int(tab["F"][-1]) + int(tab["n_in"][-1])
        frames, entries = int(tab["fr_off"][-1]) + int(tab["n_list"][-1]) - 2 * int(tab["need"][-1]) - 1, int(tab["list_off"][-1]) + int(tab["n_list"][-1])
        y = torch.empty((room,), dtype=torch.float32, device=dev)
        up = torch.from_numpy(np.concatenate([tab.view(np.uint8), fade.view(np.uint8)])).to(dev)              # one upload
        scratch = int(self.lib.ctts_trim_pauses_stream_scratch_bytes(frames, entries))
        res_bytes = -(-4 * 4 * n // 16) * 16
        work = device_scratch(res_bytes + scratch, dev)
        pool = self._pool("pauses")
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_trim_pauses_stream_step(
            x.data_ptr() if x.numel() else None, x.numel(), up.data_ptr(), tab.ctypes.data_as(C.c_void_p), n, y.data_ptr() if room else None, room,
            pool.buf["carry"].data_ptr(), pool.buf["state"].data_ptr(), pool.slots, up.data_ptr() + tab.nbytes, int(fade.size),
            work.data_ptr(), work.data_ptr() + res_bytes, scratch, st.cuda_stream), "ctts_trim_pauses_stream_step")
        up.record_stream(st)
        work.record_stream(st)
        x.record_stream(st)
        res = work[: 16 * n].cpu().numpy().view(np.int32).reshape(n, 4)                                       # the one copy, and the one wait
        pool.commit({h: rec._replace(held=int(res[i, 1]), emitted=rec.emitted + int(res[i, 0])) for i, (h, rec) in enumerate(commit.items())})  # in push order
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(res[:, 0], out=off[1:])
        if n == 1:
            return y[: int(off[1])], off
        return torch.cat([y[int(tab["out_off"][i]): int(tab["out_off"][i]) + int(res[i, 0])] for i in range(n)]), off

    # -- ragged decode: packed utterances, each decoded as if alone ---------------------------------------------------------------
    def decode_ragged(self, rows: List[torch.Tensor], return_mel: bool = False, sample_rate=None, speed=None, loudness=None, pauses=None,
                      limiter=None, compress=None, eq=None):
        """Every [T_i, 768] hidden-state row (views allowed) through DVAE + Vocos EXACTLY AS IF DECODED ALONE, in one pass over the
        packed frames (ctts_dvae_decode_ragged / ctts_vocos_decode_ragged): each utterance gets zero padding at its own edges in every
        convolution, so its audio does not depend on what else is in the call -- unlike `decode_to_wavs`, whose zero-padded [B, Tmax]
        batch (the reference's semantics, core.py:525-533) lets the padding's bias-driven activations into a shorter row's last ~51 tokens.
        Returns (wav, off): ONE flat float32 device tensor with utterance i's 256 (2 T_i - 1) samples at [off[i], off[i+1]) (`off` a host
        int64 array of len(rows) + 1; `ragged_views(wav, off)` gives the per-utterance views), plus the packed mel [sum 2 T_i, 100] as a
        third element when `return_mel`.  With gemm "f32" or "bf16x3", every utterance's mel and waveform are bit-identical to its B = 1
        decode at any packed size.  With "f16", a pack of at least CTTS_X3P_MIN_ROWS (default 1024) frames runs the point-wise pairs
        on fp16 planes: an utterance of at least that many frames takes them alone too and is bit-identical, a shorter one takes
        split-bf16 tiles alone and is within 2e-5 RMS.
        `sample_rate` (None: 24000): the rate of the returned samples -- one value, or one per row (requests that finish together at
        different rates share the decode).  The waveform is resampled on the device directly behind the ISTFT (`resample_segments`),
        every row as if alone; `off` then holds the resampled rows' offsets.
        `speed` (None: 1.0): pitch-preserving time scaling -- one value, or one per row (`time_scale_segments`: rows at speed 1 are
        copied through).  It runs at 24 kHz, behind the ISTFT and in front of the resampler, every row as if alone.
        `loudness` (None: untouched): a target in LUFS -- one value, or one per row, None entries left alone.  The rows are
        normalised in place (`loudness_normalize`), each as a group of its own at its own rate: the last float32 stage, behind the
        time scaler and the resampler.
        `pauses` (None: untouched): a pause spec -- one, or a list with one per row, None entries copied through (`trim_pauses`, every
        row alone at its own rate).  It runs behind the time scaler and the resampler and in front of the loudness stage, so the
        milliseconds are those of what is heard and the gain is computed on what is delivered; `off` then holds the trimmed rows'
        offsets, read back from the device in the call's one extra copy.
        `limiter` (None: off; one bool, or one per row): a flagged row goes through the look-ahead peak limiter (`peak_limit`) behind
        the loudness stage's gain, which then drops its ceiling term (`loudness_normalize(limiter=)`); without `loudness` at unity
        gain.  The rows that do not ask for it are not touched by it.
        `compress` (None: off): a compressor spec (True or a dict, `compressor.check`) -- one, or a list with one per row, None entries
        copied through (`compress`, every row alone at its own rate, in place): behind `pauses` and in front of the loudness stage, so
        the target is reached on compressed samples and the limiter still holds the ceiling.
        `eq` (None: off): an equaliser spec (a preset name or a dict, `equalizer.check`) -- one, or a list with one per row, None
        entries copied through (`equalize`, every row alone at its own rate from zero state, in place): behind `pauses`, whose detector
        sees the signal it was tuned on, and in front of `compress`, so the compressor, the loudness stage and the limiter see what the
        listener will hear."""
        if len(rows) == 0:
            raise ValueError("decode_ragged needs at least one row")
        plan = OC.Plan.rows("decode_ragged", len(rows), sample_rate, speed, loudness, pauses, limiter, compress, eq)     # every refusal, before the decode
        if plan.on:
            out = self.decode_ragged(rows, return_mel)                # the plain decode, through the public method
            return (*OC.run(self, out[0], plan, offsets=out[1], in_place=True), *out[2:])
        lens = [int(r.size(0)) for r in rows]
        if min(lens) < 1:
            raise ValueError("decode_ragged: every row needs at least one token")
        for r in rows:
            if r.dim() != 2 or r.size(1) != GPT.hidden:
                raise ValueError("decode_ragged: rows must be [T, 768]")
        tok, off, _ = ragged_offsets(lens)
        T = int(tok[-1])
        hid = torch.cat([r.to(device=self.device, dtype=torch.float32) for r in rows]) if len(rows) > 1 else \
            rows[0].to(device=self.device, dtype=torch.float32).contiguous()
        tok_d = torch.from_numpy(tok).to(self.device, non_blocking=False)
        mel = torch.empty((2 * T, DVAE.n_mels), dtype=torch.float32, device=self.device)
        wav = torch.empty((int(off[-1]),), dtype=torch.float32, device=self.device)
        ws, n = self._ws_bytes(self.lib.ctts_codec_ragged_workspace_bytes(len(rows), T))
        st = torch.cuda.current_stream(self.device).cuda_stream
        tok_h = tok.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.ctts_dvae_decode_ragged(self.handle, hid.data_ptr(), tok_d.data_ptr(), tok_h, len(rows), mel.data_ptr(),
                                                    ws.data_ptr(), n, st), "ctts_dvae_decode_ragged")
        _lib.check(self.lib.ctts_vocos_decode_ragged(self.handle, mel.data_ptr(), tok_d.data_ptr(), tok_h, len(rows), wav.data_ptr(),
                                                     ws.data_ptr(), n, st), "ctts_vocos_decode_ragged")
        tok_d.record_stream(torch.cuda.current_stream(self.device))
        return (wav, off, mel) if return_mel else (wav, off)

    def float_to_int16_ragged(self, wav: torch.Tensor, off, product: str = "f64", keep_thr: Optional[float] = None, out=None):
        """`float_to_int16` per utterance of a packed waveform (`decode_ragged`'s output): one peak per segment [off[i], off[i+1]), on the
        device (ctts_float_to_int16_ragged).  Returns (pcm, keep, keep_off): pcm int16 in the waveform's layout; keep (keep_thr given) the
        packed masks |x| > keep_thr (np.packbits order), segment i's from byte keep_off[i] on -- every segment starts on a byte boundary
        -- else None.  `out`: optional (pcm, keep) device tensors to write into (e.g. views of one buffer, so that a single copy brings
        both to the host).  Bit-exact against `audio.float_to_int16` of each segment."""
        off = np.asarray(off, dtype=np.int64)
        assert wav.dim() == 1 and wav.dtype == torch.float32 and wav.is_cuda and wav.numel() == int(off[-1])
        n_seg = len(off) - 1
        keep_off = keep_offsets(off)
        if out is not None:
            pcm, keep = out
            assert pcm.dtype == torch.int16 and pcm.numel() == wav.numel() and (keep is None) == (keep_thr is None)
            assert keep is None or (keep.dtype == torch.uint8 and keep.numel() == int(keep_off[-1]))
        else:
            pcm = torch.empty((wav.numel(),), dtype=torch.int16, device=wav.device)
            keep = torch.empty((int(keep_off[-1]),), dtype=torch.uint8, device=wav.device) if keep_thr is not None else None
        peak = torch.empty((n_seg,), dtype=torch.int32, device=wav.device)
        off_d = torch.from_numpy(off).to(wav.device)
        st = torch.cuda.current_stream(wav.device)
        _lib.check(self.lib.ctts_float_to_int16_ragged(wav.data_ptr(), pcm.data_ptr(), _lib.ptr(keep), off_d.data_ptr(),
                                                       off.ctypes.data_as(C.c_void_p), n_seg, {"f64": 0, "f32": 1}[product],
                                                       float(keep_thr or 0.0), peak.data_ptr(), st.cuda_stream),
                   "ctts_float_to_int16_ragged")
        off_d.record_stream(st)
        return pcm, keep, keep_off

    def float_to_int16_groups(self, wav: torch.Tensor, off, grp, product: str = "f64", keep_thr: Optional[float] = 1e-5, encodings=None):
        """The last step of split_text requests on the device (ctts_float_to_int16_groups): segments grp[g] .. grp[g+1]-1 of a packed
        waveform (`decode_ragged`'s output) are request g's sentences.  ONE peak per group; the group's samples with |x| > keep_thr
        are converted and written contiguously, in order (keep_thr None: nothing is stripped, a plain concatenation under one peak).
        Returns (blob, starts): ONE uint8 device tensor -- a header of the groups' kept counts (int64 [n_grp], padded to 16 bytes), then
        the int16 samples, group g's from element starts[g] = sum_{h<g} ceil8(n_h) on (for a decode: off[grp[g]]) -- so that a single
        copy brings counts and bytes to the host; `unpack_groups(host_blob, starts)` cuts it.  Group g's result equals
        `audio.float_to_int16(np.concatenate([w[np.abs(w) > keep_thr] for w in its segments]))` bit for bit.
        `encodings` (None, or all None: the call above): one entry per group, None / "ulaw" / "alaw".  A companded group's slot
        [starts[g], starts[g+1]) is converted whole by ONE ctts_g711_encode_ranges launch behind the conversion (its kept count is
        known on the device only; the bytes behind it are never handed out).  The device buffer is then int16 samples | count header
        | companded bytes, and the blob returned is the part the host needs: header | bytes when every group is companded, the whole
        buffer otherwise -- one copy either way; `unpack_groups(host_blob, starts, encodings)` cuts it."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        grp = np.ascontiguousarray(grp, dtype=np.int32)
        if encodings is not None:
            if len(encodings) != len(grp) - 1:
                raise ValueError("float_to_int16_groups: one encoding per group")
            if all(G711.check_encoding(e) is None for e in encodings):
                encodings = None
        assert wav.dim() == 1 and wav.dtype == torch.float32 and wav.is_cuda and wav.is_contiguous() and wav.numel() == int(off[-1])
        n_seg, n_grp = len(off) - 1, len(grp) - 1
        off_p, grp_p = off.ctypes.data_as(C.c_void_p), grp.ctypes.data_as(C.c_void_p)
        sb = int(self.lib.ctts_float_to_int16_groups_scratch_bytes(off_p, n_seg, grp_p, n_grp))
        if sb == 0:
            _lib.check(-1, "ctts_float_to_int16_groups")      # the tables were refused: the library's message says why
        starts = group_starts(off, grp)
        hdr = (8 * n_grp + 15) // 16 * 16
        dev = wav.device
        E = int(starts[-1])                                                                              # a multiple of 8
        if encodings is None:
            blob = torch.empty((hdr + 2 * E,), dtype=torch.uint8, device=dev)
            cnt_p, pcm_p = blob.data_ptr(), blob.data_ptr() + hdr
        else:                                                                                           # samples | header | companded bytes
            blob = torch.empty((2 * E + hdr + (E + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
            cnt_p, pcm_p = blob.data_ptr() + 2 * E, blob.data_ptr()
        tabs = torch.from_numpy(np.concatenate([off.view(np.uint8), grp.view(np.uint8)])).to(dev)      # one upload: offsets, then groups
        work = device_scratch(4 * n_grp + sb, dev)                                                      # peaks, then the tile counts
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_float_to_int16_groups(wav.data_ptr(), pcm_p, cnt_p, tabs.data_ptr(), off_p, n_seg,
                                                       tabs.data_ptr() + off.nbytes, grp_p, n_grp, {"f64": 0, "f32": 1}[product],
                                                       -1.0 if keep_thr is None else float(keep_thr), work.data_ptr(),
                                                       work.data_ptr() + 4 * n_grp, sb, st.cuda_stream), "ctts_float_to_int16_groups")
        tabs.record_stream(st)
        work.record_stream(st)
        if encodings is not None:
            self.g711_encode(blob[: 2 * E].view(torch.int16), [(int(starts[g]), int(starts[g + 1] - starts[g]), encodings[g]) for g in range(n_grp)],
                             out=blob[2 * E + hdr:])
            if all(e is not None for e in encodings):
                return blob[2 * E:], starts
        return blob, starts

    def float_to_int16_groups_flac(self, wav: torch.Tensor, off, grp, rates, product: str = "f64", keep_thr: Optional[float] = 1e-5,
                                   encodings=None) -> list:
        """`float_to_int16_groups` with FLAC behind it: `rates`, one entry per group -- None: the group comes back as
        `unpack_groups` hands it out (int16 samples, or with `encodings` its G.711 codes); a rate in Hz: as the complete FLAC file (a
        uint8 array) of exactly its int16 samples.  The grouped slots and the count header on the device go straight into
        `flac_encode` (a group's stripped length is known on the device only); when every group is encoded the samples never cross
        the bus.  A group has a rate or an encoding, not both."""
        n_grp = len(grp) - 1
        if len(rates) != n_grp or (encodings is not None and len(encodings) != n_grp):
            raise ValueError("float_to_int16_groups_flac: one rate (or None) and one encoding (or None) per group")
        for g, r in enumerate(rates):
            if r is not None:
                FLAC.rate_code(r)
                if encodings is not None and encodings[g] is not None:
                    raise ValueError("float_to_int16_groups_flac: a group is FLAC or companded, not both")
        if encodings is not None and all(G711.check_encoding(e) is None for e in encodings):
            encodings = None
        blob, starts = self.float_to_int16_groups(wav, off, grp, product, keep_thr, encodings=encodings)
        if all(r is None for r in rates):
            return self.unpack_groups(self.to_host(blob), starts, encodings)
        hdr, E = (8 * n_grp + 15) // 16 * 16, int(starts[-1])
        pcm_at, cnt_at = (hdr, 0) if encodings is None else (0, 2 * E)           # header | samples, or samples | header | codes
        enc = self.flac_encode(blob[pcm_at: pcm_at + 2 * E].view(torch.int16),
                               [(int(starts[g]), int(starts[g + 1] - starts[g]), rates[g], g) for g in range(n_grp)],
                               counts=blob[cnt_at: cnt_at + 8 * n_grp].view(torch.int64), info=True)
        plain = self.unpack_groups(self.to_host(blob), starts, encodings) if any(r is None for r in rates) else None
        return [plain[g] if rates[g] is None else FLAC.file_bytes(enc[g][0], enc[g][1], enc[g][2], rates[g]) for g in range(n_grp)]

    @staticmethod
    def unpack_groups(host_blob: np.ndarray, starts, encodings=None) -> List[np.ndarray]:
        """`float_to_int16_groups`'s blob on the host -> one int16 array per group (views of the blob); with `encodings` (those of the
        call) a companded group's uint8 codes instead"""
        n_grp = len(starts) - 1
        hdr = (8 * n_grp + 15) // 16 * 16
        if encodings is not None and any(e is not None for e in encodings):
            E = int(starts[-1])
            base = 0 if all(e is not None for e in encodings) else 2 * E       # where the count header sits
            n_kept = host_blob[base: base + 8 * n_grp].view(np.int64)
            codes = host_blob[base + hdr:]
            pcm = host_blob[: 2 * E].view(np.int16) if base else None
            return [(pcm if e is None else codes)[int(starts[g]): int(starts[g]) + int(n_kept[g])] for g, e in enumerate(encodings)]
        n_kept = host_blob[: 8 * n_grp].view(np.int64)
        pcm = host_blob[hdr:].view(np.int16)
        return [pcm[int(starts[g]): int(starts[g]) + int(n_kept[g])] for g in range(n_grp)]

    HALO_FRAMES = HALO_FRAMES

    def decode_window(self, result_list: List[torch.Tensor], s_lo: int, s_hi: int, sample_rate: Optional[int] = None) -> torch.Tensor:
        """Samples [s_lo, s_hi) of `decode_to_wavs(result_list)` WITHOUT decoding the whole batch: the acoustic decoder is a
        stack of short symmetric convolutions, so those samples depend only on the tokens within HALO_FRAMES mel frames
        (+ the 4 overlapping ISTFT frames) of them.  Only that token window (zero padded like core.py:525-533) goes
        through DVAE + Vocos; at the true ends of the sequence the window is the sequence's own edge, so the result equals
        the full decode up to summation order.  This is what makes streaming O(n): the reference re-decodes the entire
        prefix at every yield (core.py:482-497) to hand out the next `stream_speed` samples of it.
        `sample_rate` (None or 24000: the path above, bit for bit): the same range of the decode RESAMPLED AS ONE SIGNAL -- outputs
        [ceil(s_lo L / M), ceil(s_hi L / M)) of `resample(decode_to_wavs(result_list))`, so consecutive ranges tile the resampled
        signal.  The window of `resample.window_inputs` is decoded as above and converted by `resample_window`: no filter state."""
        if sample_rate is not None and int(sample_rate) != self.SAMPLE_RATE:
            Tn = max(int(r.size(0)) for r in result_list)
            total = VOCOS.hop * (2 * Tn - 1)
            L, M, K, _ = RS.plan(self.SAMPLE_RATE, int(sample_rate), [0, 1])
            lo, hi = min(max(0, int(s_lo)), max(total, 0)), min(max(total, 0), int(s_hi))
            o_lo, o_hi = RS.out_len(lo, L, M), RS.out_len(max(lo, hi), L, M)
            if o_hi <= o_lo:
                return torch.empty((len(result_list), 0), dtype=torch.float32, device=self.device)
            a, b = RS.window_inputs(L, M, K, o_lo, o_hi, total)
            return self.resample_window(self.decode_window(result_list, a, b), a, total, o_lo, o_hi, self.SAMPLE_RATE, int(sample_rate))
        win = window_for_samples(max(int(r.size(0)) for r in result_list), s_lo, s_hi)
        if win is None:
            return torch.empty((len(result_list), 0), dtype=torch.float32, device=self.device)
        t_lo, t_hi, c_lo, c_hi = win
        batch = torch.zeros((len(result_list), t_hi - t_lo, GPT.hidden), dtype=torch.float32, device=self.device)
        for i, r in enumerate(result_list):
            n = min(int(r.size(0)), t_hi) - t_lo
            if n > 0:
                batch[i, :n] = r[t_lo: t_lo + n]
        wav = self.vocos_decode(self.dvae_decode(batch))
        return wav[:, c_lo: c_hi]

    def decode_windows(self, store: torch.Tensor, windows, pcm16: bool = True, keep_thr: Optional[float] = None, product: str = "f64",
                       sample_rates=None, encodings=None, speeds=None, ts_streams=None, rs_streams=None, flac=None, flac_streams=None,
                       limiter=None, lm_streams=None, pauses=None, pa_streams=None, adpcm=None, adpcm_streams=None, compress=None,
                       cp_streams=None):
        """The chunks of many streamed utterances in ONE ragged decoder pass, each at its own position (ctts_codec_decode_windows).
        `store`: a hidden-state store [slots, hid_cap, 768] float32 on the device (SlotPool.hiddens; read in place, nothing is sliced
        or copied per slot).  `windows`: a list of (slot, Tn, s_lo, s_hi) or (slot, Tn, s_lo, s_hi, tail): samples [s_lo, s_hi) (s_hi
        None: to the end) of the decode of the first Tn rows of that slot -- what `decode_window([store[slot, :Tn]], s_lo, s_hi)[0]`
        returns, bit for bit with gemm "f32" / "bf16x3" (the ragged decoder's bar; "f16": within its 2e-5 RMS).  Returns one numpy
        array per window: int16 through `float_to_int16`'s arithmetic with one peak per window over its own samples (`pcm16`), else
        float32.  With `keep_thr`, a window marked `tail` comes back with its samples |x| <= keep_thr removed -- the serial path's
        last chunk (core.py, `_infer`): the mask is taken from the float samples on the device, the conversion uses the peak over
        the whole crop (the removed samples are all below the threshold, so that is the peak of the kept ones whenever any is kept).
        One table upload, one pass, one device-to-host copy whatever the number of windows.
        `sample_rates` (None, or all 24000: the call above, argument for argument): one rate per window.  A window at rate r yields
        outputs [ceil(s_lo L / M), ceil(s_hi L / M)) of the resampled decode of its prefix -- `decode_window(.., sample_rate=r)` --
        with the peak, the conversion and a tail's strip taken on the resampled samples (ctts_codec_decode_windows_rate: the same
        pass, one resampler launch per distinct rate, one conversion launch).
        `encodings` (None, or all None: the call above, argument for argument; needs `pcm16`): one entry per window, None / "ulaw" /
        "alaw".  A companded window comes back as uint8, `g711.encode` of the int16 array it would come back as -- strictly behind the
        conversion, a tail's strip included (ONE ctts_g711_encode_ranges launch over the windows' own element offsets; the codes and
        the keep masks sit side by side in the output buffer, so one copy brings both; a call that mixes PCM16 and companded windows
        copies the PCM16 samples with them, still in one copy).
        `speeds` (None, or all 1.0: the call above, argument for argument): one speed per window, with `ts_streams`, one entry per
        window: the handle of the time scaler's stream (`time_scale_stream_open`) the window continues, None at speed 1.  A window
        at another speed PUSHES its 24 kHz crop into its stream and yields what that step emits (`time_scale_stream_step`: a
        multiple of 512 samples, possibly none; a window marked `tail` is the stream's last push and yields the rest) -- crop ->
        stream step -> conversion on the device (ctts_codec_decode_windows_speed), the peak, the conversion, a tail's strip and the
        companding taken on the scaled samples; still one decoder pass and one copy.  A window whose crop is empty still steps its
        stream.  Several windows of one stream are taken in the order given.  Windows at speed 1 return the bytes they return
        without `speeds`.  A speed together with a rate other than 24000 is refused (resampling the scaled stream needs its history
        and a look-ahead carried too) unless `rs_streams` carries them: one entry per window, the handle of the resampler's stream
        (`resample_stream_open(24000, rate)`) the window continues, None for a window at speed 1 or at 24000 Hz.  A window at
        another speed AND another rate pushes its crop into its time-scale stream and the chunk that step emits into its resampler
        stream, and yields what that second step emits (`resample_stream_step`; ctts_codec_decode_windows_speed_rate: behind the
        scaler's rounds one resampler launch per distinct rate per round, then the one conversion launch); the peak, the
        conversion, a tail's strip and the companding are taken on those samples.  A `tail` window is the last push of both
        streams; several windows of one stream go to successive rounds in both stages.  Windows at speed 1 and another rate keep
        the stateless window path of `sample_rates` and return its bytes; in a call that also holds windows at another speed they
        take a decoder pass of their own.
        `flac` (None, or all False: the call above, argument for argument; needs `pcm16`) with `flac_streams`: one flag and one entry
        per window, the handle of the FLAC stream (`flac_stream_open`, at the window's rate) a flagged window continues.  A flagged
        window PUSHES the int16 samples it would come back as into its stream and comes back as uint8, the frames that push completes
        (possibly none; `flac.StreamEncoder.push` byte for byte) -- strictly behind the conversion, on every path above; a window
        marked `tail` is the stream's last push, and with `keep_thr` it is stripped on the device by the conversion's keep mask.  ONE
        `flac_stream_step` for the whole call (four launches), one small copy of the frame offsets and one of the bytes used: a flagged
        window's samples never cross the bus (a call whose windows are all flagged copies no samples at all).  A flagged window whose
        crop is empty still steps its stream; several windows of one stream are taken in the order given, each in a step of its own
        round.  A flag together with an encoding is refused.
        `limiter` (None, or all False: the call above, argument for argument) with `lm_streams`: one flag and one entry per window,
        the handle of the limiter stream (`peak_limit_stream_open`, at the window's output rate) a flagged window continues.  A
        flagged window PUSHES the float32 samples it would otherwise convert -- behind the plain crop, the stateless rate path, the
        time-scale stream or the time-scale and resampler streams -- into its limiter stream and yields what that step emits
        (`peak_limit_stream_step`: the stream lags by rate // 50 samples; a window marked `tail` is the stream's last push and yields
        the rest): the peak, the 16-bit conversion, a tail's strip, the companding and a FLAC push all act on the limited samples,
        the non-streamed order.  The float chunks stay on the device: the flagged windows take a decoder pass of their own (two
        where some are at another speed and some are not), one limiter step per round -- several windows of one stream go to
        successive rounds, in the order given --, ONE ctts_float_to_int16_ragged launch, and the epilogue of every other path (one
        copy).  A flagged window whose crop is empty still steps its stream.  Unflagged windows return the bytes they return
        without `limiter`.
        `pauses` (None, or all None / False: the call above, argument for argument, with no extra copy) with `pa_streams`: one flag
        and one entry per window, the handle of the pause stream (`trim_pauses_stream_open`, at the window's output rate; the stream
        holds the spec) a flagged window continues.  A flagged window PUSHES its float32 samples -- behind the same float stages as
        the limiter's -- into its pause stream and goes on with what that step emits (`trim_pauses_stream_step`; a window marked
        `tail` is the stream's last push): in front of the limiter stream, the conversion (one peak per window over the samples that
        come out), a tail's strip (`keep_thr` acts on what the last push emits), G.711 and the FLAC push, the non-streamed order.
        One pause step per round, each with its one small copy of the counts; the chunks then start on multiples of 8 samples again,
        as the FLAC step needs them.
        `adpcm` (None, or all False: the call above, argument for argument; needs `pcm16`) with `adpcm_streams`: `flac` /
        `flac_streams` for IMA ADPCM -- one flag and one entry per window, the handle of the ADPCM stream (`adpcm_stream_open`, at the
        window's rate) a flagged window continues.  A flagged window PUSHES the int16 samples it would come back as into its stream and
        comes back as uint8, the blocks that push completes (possibly none; `adpcm.StreamEncoder.push` byte for byte), on every path
        and by the rules of a FLAC push: behind the conversion, a `tail` is the last push and is stripped by the keep mask on the
        device, an empty crop still steps its stream, several windows of one stream go to successive rounds.  ONE `adpcm_stream_step`
        for the flagged windows of the call (two launches; where no tail is stripped, one copy: the blocks).  A window takes FLAC or
        ADPCM, not both; neither goes with an encoding.
        `compress` (None, or all None / False: the call above, argument for argument) with `cp_streams`: one flag and one entry per
        window, the handle of the compressor stream (`compress_stream_open`, at the window's output rate; the stream holds the spec)
        a flagged window continues.  A flagged window PUSHES its float32 samples -- behind the same float stages as the limiter's, and
        behind its pause stream -- into its compressor stream and goes on with what that step emits (`compress_stream_step`: the
        stream lags by its attack and two blocks of 1 ms at the most; a window marked `tail` is the stream's last push): in front of
        the limiter stream, the conversion, a tail's strip, G.711, FLAC and ADPCM, the non-streamed order.  One compressor step per
        round (two launches), no copy of its own.  Unflagged windows return the bytes they return without `compress`."""
        ws, S, cap, free, held, laws = self._parse_windows(store, windows, pcm16, keep_thr, dict(
            sample_rates=sample_rates, encodings=encodings, speeds=speeds, ts_streams=ts_streams, rs_streams=rs_streams, flac=flac,
            flac_streams=flac_streams, limiter=limiter, lm_streams=lm_streams, pauses=pauses, pa_streams=pa_streams, adpcm=adpcm,
            adpcm_streams=adpcm_streams, compress=compress, cp_streams=cp_streams))
        out: list = [None] * len(ws)
        companded = laws and any(w.law >= 0 for _, p in free for w in p)
        for kind, p in free:            # the windows behind no float stage: every pass with the epilogue of its own
            self._windows_emit(p, self._pass(kind)(store, S, cap, p, pcm16, keep_thr, product, companded), pcm16, companded, out)
        if held:                        # the others: float chunks left on the device, the stages' rounds, one conversion, one epilogue
            self._windows_staged(store, S, cap, held, pcm16, keep_thr, product, laws, out)
        return out

    # -- what the passes of `decode_windows` share: the store, the parsing of the call into one record per window, the crops' places in the
    # packed decode, the output layout, the tail of the C call and the epilogue.  A further pass kind builds its own tables between them
    @staticmethod
    def _windows_store(store: torch.Tensor):
        assert store.dim() == 3 and store.dtype == torch.float32 and store.is_cuda and store.size(2) == GPT.hidden and store.stride(2) == 1
        return int(store.size(0)), int(store.size(1))

    def _pass(self, kind: str):
        """the method that runs a pass of `winchain.passes`' kind"""
        return {"plain": self._pass_plain, "rate": self._pass_rate, "speed": self._pass_speed}[kind]

    def _parse_windows(self, store, windows, pcm16: bool, keep_thr, given: dict):
        """`decode_windows`' arguments (`given`: its arguments by name), checked once -> (one `winchain.Window` per window, S, cap, the
        free passes, the held passes, whether the call compands).  Every refusal that reads the lists is raised here, before anything is
        launched: the stages' in the order of `winchain.CHECKED`, then the speeds', the encodings', the rates', each window's place in
        the store and the streams of its speed (a rate the resampler does not take and a push a stream does not take are refused by
        their planning, in front of their pass's launch).  Nothing below looks at the lists again"""
        n_w, SR = len(windows), self.SAMPLE_RATE
        sample_rates, encodings, speeds, ts_streams, rs_streams = (given[k] for k in ("sample_rates", "encodings", "speeds", "ts_streams", "rs_streams"))
        tails = [len(w) > 4 and bool(w[4]) for w in windows]
        hs = {s.name: self._window_streams(s, given[s.flag], given[s.streams], tails, sample_rates, pcm16, encodings) for s in WC.CHECKED}
        both = [v for s, v in zip(WC.CHECKED, hs.values()) if s.kind == "int16" and v is not None]
        if len(both) > 1 and any(f is not None and a is not None for f, a in zip(*both)):
            raise ValueError("decode_windows: a window takes FLAC or ADPCM, not both")
        rated = sample_rates is not None and any(int(r) != SR for r in sample_rates)
        q = None
        if speeds is not None:
            if len(speeds) != n_w:
                raise ValueError("decode_windows: one speed per window")
            q = [tuple(TS.quantize(v)) for v in speeds]
            if all(n == d for n, d in q):
                q = None
            elif rs_streams is None and rated:
                raise ValueError("decode_windows: a streamed speed goes with 24000 Hz only (resampling the scaled stream would need "
                                 "its history and a look-ahead carried too)")
            elif ts_streams is None or len(ts_streams) != n_w:
                raise ValueError("decode_windows: speeds need ts_streams, one entry per window")
        laws = None
        if encodings is not None:
            if len(encodings) != n_w:
                raise ValueError("decode_windows: one encoding per window")
            if any(G711.check_encoding(e) is not None for e in encodings):
                if not pcm16:
                    raise ValueError("decode_windows: G.711 companding comes behind the 16-bit conversion (pcm16=True)")
                laws = [-1 if e is None else G711.LAWS[e] for e in encodings]
        if q is not None and rated and (len(sample_rates) != n_w or len(rs_streams) != n_w):
            raise ValueError("decode_windows: one sample rate and one rs_streams entry per window")
        if q is None and sample_rates is not None and len(sample_rates) != n_w:
            raise ValueError("decode_windows: one sample rate per window")
        S, cap = self._windows_store(store)
        none, geo, hop = [None] * n_w, [], VOCOS.hop
        for i, w in enumerate(windows):
            slot, Tn, s_lo, s_hi = (int(w[0]), int(w[1]), int(w[2]), w[3])
            if not (0 <= slot < S and 0 <= Tn <= cap):
                raise ValueError(f"decode_windows: window {i} (slot {slot}, {Tn} tokens) lies outside the [{S}, {cap}] store")
            geo.append((i, slot, Tn, s_lo, hop * (2 * Tn - 1) if s_hi is None else int(s_hi)))
        # the records, column by column: the handles per stage in the table's order (a speed's streams as given: `_check_speed_streams`
        # checks them below, and only a scaled window's are read), which windows stand behind a float stage, the int16 stage of each
        cols = {"time_scale": ts_streams if q is not None else none, "resample": rs_streams if q is not None and rated else none, **hs}
        staged, codec = [False] * n_w, none
        for s in WC.CHECKED:
            if hs[s.name] is not None and s.kind == "float":
                staged = [a or h is not None for a, h in zip(staged, hs[s.name])]
            elif hs[s.name] is not None:
                codec = [c if h is None else (s.name, h) for c, h in zip(codec, hs[s.name])]
        qs = [(1, 1)] * n_w if q is None else q
        new = tuple.__new__                        # (a NamedTuple's own constructor is a Python call per window)
        ws = [new(WC.Window, (*g, *rest)) for g, *rest in zip(
            geo, tails, [int(r) for r in sample_rates] if rated else [SR] * n_w, qs, [a != b for a, b in qs], [-1] * n_w if laws is None else laws,
            zip(*(cols[s.name] or none for s in WC.STAGES)), staged, codec)]
        free, held = WC.passes(ws, q is not None, rated)
        if q is not None:
            for group in ([w for _, p in free for w in p], *(p for _, p in held)):
                self._check_speed_streams(sorted(group, key=lambda w: w.i), ts_streams, rs_streams)
        return ws, S, cap, free, held, laws is not None

    def _check_speed_streams(self, group, ts_streams, rs_streams) -> None:
        """a group that scales (`winchain.passes`): a scaled window names an open stream of its speed and, at another rate, an open
        resampler stream to that rate, no other window names either"""
        if not any(w.scaled for w in group):
            return
        SR, rated = self.SAMPLE_RATE, any(w.rate != self.SAMPLE_RATE for w in group)
        recs = self._pool("time_scale").records
        rs_recs = self._pool("resample").records if rated else {}
        for w in group:
            h, hr = ts_streams[w.i], rs_streams[w.i] if rated else None
            if w.scaled:
                rec = None if h is None else recs.get(int(h))
                if rec is None or (rec.num, rec.den) != w.q:
                    raise ValueError(f"decode_windows: window {w.i} at speed {w.q[0]}/{w.q[1]} needs an open stream of that speed")
            elif h is not None or hr is not None:
                raise ValueError(f"decode_windows: window {w.i} is at speed 1 but names a stream")
            if w.scaled and w.rate != SR:
                rec = None if hr is None else rs_recs.get(int(hr))
                if rec is None or (rec.orig, rec.new) != (SR, w.rate):
                    raise ValueError(f"decode_windows: window {w.i} at {w.rate} Hz needs an open resampler stream {SR} -> {w.rate}")
            elif hr is not None:
                raise ValueError(f"decode_windows: window {w.i} stays at {SR} Hz but names a resampler stream")

    def _window_streams(self, stage, flags, streams, tails, sample_rates, pcm16: bool, encodings):
        """The flags and streams of one streamed stage (a row of `winchain.STAGES`) of a `decode_windows` call, checked -> per window its
        stream's handle or None; None when no window is flagged.  A float stage refuses a stream that has had its last push, before
        the call or by a tail window earlier in it, by window; for an int16 stage the pool's `live` refuses, and the call must
        convert to 16 bits and give a flagged window no encoding."""
        arg, arg_streams, name, ends = stage.flag, stage.streams, stage.title, stage.kind == "float"
        an = lambda s: ("an " if s[0] in "aA" else "a ") + s
        if flags is None or not any((stage.any_flag or stage.flagged)(f) for f in flags):
            if streams is not None and any(h is not None for h in streams):
                raise ValueError(f"decode_windows: {arg_streams} without {an(arg)} flag")
            return None
        if len(flags) != len(tails) or streams is None or len(streams) != len(tails):
            raise ValueError(f"decode_windows: one {arg} flag and one {arg_streams} entry per window")
        if stage.kind == "int16":
            if not pcm16:
                raise ValueError(f"decode_windows: {name} comes behind the 16-bit conversion (pcm16=True)")
            if encodings is not None and any(f and e is not None for f, e in zip(flags, encodings)):
                raise ValueError(f"decode_windows: {arg} does not go with an encoding ({an(name)} stream holds the 16-bit samples)")
        pool, ended, out, flagged = self._pool(stage.name), set(), [], stage.flagged
        records, want = pool.records, self.SAMPLE_RATE
        for i, (f, h) in enumerate(zip(flags, streams)):
            if f is not True and not flagged(f):
                if h is not None:
                    raise ValueError(f"decode_windows: window {i} has no {arg} flag but names {an(name)} stream")
                out.append(None)
                continue
            if sample_rates is not None:
                want = int(sample_rates[i])
            rec = None if h is None else records.get(int(h)) if ends else pool.live(h)
            if rec is None or rec.rate != want:
                raise ValueError(f"decode_windows: window {i} needs an open {name} stream at {want} Hz")
            h = int(h)
            if ends:
                if rec.done or h in ended:
                    raise ValueError(f"decode_windows: window {i}: {name} stream {h} has had its last push")
                if tails[i]:
                    ended.add(h)
            out.append(h)
        return out

    @staticmethod
    def _packed_crops(tab: np.ndarray):
        """ctts_window rows -> (tok, start): the windows' token offsets [n + 1] in the packed decode, each crop's first sample in it"""
        tok = np.zeros(len(tab) + 1, np.int64)
        np.cumsum(tab[:, 2] - tab[:, 1], out=tok[1:])
        return tok, VOCOS.hop * (2 * tok[:-1] - np.arange(len(tab))) + tab[:, 3]

    def _windows_layout(self, n, keep, pcm16: bool, laws):
        """the output of one call from its chunks' lengths `n` and keep flags -> (off, n_out, n_g, n_keep, buf): every chunk starts on a
        multiple of 8 samples (`off`, in elements); `buf` = samples (n_out bytes) | companded bytes (n_g, with `laws`) | keep masks
        (n_keep, when any chunk is stripped), so ONE copy brings all of it; at least 16 bytes (a call whose chunks are all empty)"""
        off = np.zeros(len(n) + 1, np.int64)
        np.cumsum((n + 7) // 8 * 8, out=off[1:])
        n_out = int(off[-1]) * (2 if pcm16 else 4)
        n_keep = (int(off[-1]) // 8 + 15) // 16 * 16 if keep.any() else 0
        n_g = (int(off[-1]) + 15) // 16 * 16 if laws is not None else 0
        return off, n_out, n_g, n_keep, torch.empty((max(16, n_out + n_g + n_keep),), dtype=torch.uint8, device=self.device)

    def _windows_call_tail(self, lay, keep, pcm16: bool, product: str, keep_thr: Optional[float], ws_bytes: int):
        """the current stream and the arguments every window entry ends in: out_type, out, keep_bits, product, keep_thr, workspace, its
        size, stream"""
        _, n_out, n_g, _, buf = lay
        ws, nws = self._ws_bytes(ws_bytes)
        cur = torch.cuda.current_stream(self.device)
        return cur, (1 if pcm16 else 0, buf.data_ptr(), buf.data_ptr() + n_out + n_g if keep.any() else None, {"f64": 0, "f32": 1}[product],
                     float(keep_thr or 0.0), ws.data_ptr(), nws, cur.cuda_stream)

    def _windows_emit(self, ws, chunks, pcm16: bool, companded: bool, out: list) -> None:
        """the epilogue of one pass over the windows `ws`: its chunks (what a `_pass_*` hands back, or None: no window had a sample)
        to the host -- `_windows_to_host`, the FLAC / ADPCM pushes of these windows with it -- and into the call's `out`"""
        mine: list = [None] * len(ws)
        if chunks is None or len(chunks[3]) < len(ws):      # the windows without a chunk come back empty
            has = set() if chunks is None else set(chunks[3])
            mine = [None if k in has else np.zeros((0,), np.uint8 if companded and w.law >= 0 else np.int16 if pcm16 else np.float32) for k, w in enumerate(ws)]
        fl = ([w.codec for w in ws], [w.tail for w in ws]) if any(w.codec for w in ws) else None
        if chunks is None:              # no window has a sample: the flagged ones still step their streams (a tail brings what its stream held)
            idle = [k for k, w in enumerate(ws) if w.codec]
            if idle:
                mine = self._flac_rounds(torch.zeros((8,), dtype=torch.int16, device=self.device), None, idle, [(fl[0][k], 0, 0, fl[1][k]) for k in idle], mine)
        else:
            (off, n_out, n_g, n_keep, buf), n, keep, live = chunks
            mine = self._windows_to_host(buf[: n_out + n_g + n_keep], n_out, n_g, off, n, keep, live, [ws[k].law for k in live] if companded else None,
                                         np.int16 if pcm16 else np.float32, mine, fl)
        for w, a in zip(ws, mine):
            out[w.i] = a

    def _stage_rounds(self, stage, ws, x: torch.Tensor, src: dict) -> torch.Tensor:
        """the steps of one float stage over the held windows `ws`: the r-th push of a stream goes to round r, in the order given; what
        a step emits lies behind x, and `src` (window -> first sample, samples) then names it there"""
        at = WC.PLACE[stage.name]
        _, rounds = SP.rounds(w.h[at] for w in ws)
        if not rounds:
            return x
        parts, base = [x], x.numel()
        for rnd in rounds:
            y, o = getattr(self, stage.step)(x, [(ws[k].h[at], *src.get(ws[k].i, (0, 0)), ws[k].tail) for k in rnd])
            for j, k in enumerate(rnd):
                src[ws[k].i] = (base + int(o[j]), int(o[j + 1] - o[j]))
            parts.append(y)
            base += y.numel()
        return torch.cat(parts)

    def _windows_staged(self, store: torch.Tensor, S: int, cap: int, held, pcm16: bool, keep_thr: Optional[float], product: str, companded: bool,
                        out: list) -> None:
        """the windows behind a limiter stream, a pause stream or a compressor stream (`held`: their passes): the float chunks of the
        passes stay on the device, end to end; the stages of `winchain.ROUNDS` step round by round, then the limiter; one conversion"""
        ws = held[0][1] if len(held) == 1 else sorted((w for _, p in held for w in p), key=lambda w: w.i)      # in the call's order
        src, bufs, base = {}, [], 0                                # window -> (first sample, samples) in the passes' chunks, end to end
        for kind, p in held:
            got = self._pass(kind)(store, S, cap, p, False, None, product, False)
            if got is not None:                                    # None: no window of the pass had a sample
                (off, n_out, _, _, buf), n, _, live = got
                for k, j in enumerate(live):
                    src[p[j].i] = (base + int(off[k]), int(n[k]))
                bufs.append(buf[:n_out].view(torch.float32))
                base += bufs[-1].numel()
        x = torch.cat(bufs) if len(bufs) > 1 else bufs[0] if bufs else torch.zeros((8,), dtype=torch.float32, device=self.device)
        for stage in WC.ROUNDS:
            x = self._stage_rounds(stage, ws, x, src)
        # the limiter's steps: the r-th window of a stream in round r; the limited chunks start on multiples of 8 samples, zeros between
        lm = [w.h[WC.PLACE["limiter"]] for w in ws]
        tails = [w.tail for w in ws]
        recs, shadow = self._pool("limiter").records, {}
        _, rounds = SP.rounds(lm)
        n = np.zeros(len(ws), np.int64)
        for k, w in enumerate(ws):
            if lm[k] is None:                                      # paused or compressed only: the chunk goes on as it came out
                n[k] = src.get(w.i, (0, 0))[1]
                continue
            rec = shadow.get(lm[k], recs[lm[k]])
            p = LM.stream_plan(rec.rate // 100, rec.pushed, rec.emitted, src.get(w.i, (0, 0))[1], tails[k])
            n[k] = p["n_out"]
            shadow[lm[k]] = rec._replace(pushed=p["total"], emitted=p["emitted"])
        keep = np.array([t and keep_thr is not None for t in tails], dtype=bool)
        off = np.zeros(len(ws) + 1, np.int64)
        np.cumsum((n + 7) // 8 * 8, out=off[1:])
        lim = torch.zeros((max(8, int(off[-1])),), dtype=torch.float32, device=self.device)
        for rnd in rounds:
            self.peak_limit_stream_step(x, [(lm[k], *src.get(ws[k].i, (0, 0)), tails[k]) for k in rnd], out=lim, out_off=[int(off[k]) for k in rnd])
        for k, w in enumerate(ws):
            if lm[k] is None and n[k]:
                lim[int(off[k]): int(off[k]) + int(n[k])] = x[src[w.i][0]: src[w.i][0] + int(n[k])]
        live = [k for k in range(len(ws)) if n[k] > 0]
        if not pcm16:
            host = self.to_host(lim)
            for k, w in enumerate(ws):
                a = host[int(off[k]): int(off[k]) + int(n[k])]
                out[w.i] = a[np.abs(a) > keep_thr] if keep[k] and n[k] else a
            return
        chunks = None
        if live:
            # the conversion: every limited chunk with its zero pad is a segment of ctts_float_to_int16_ragged -- the pad changes no peak, and
            # the segments' samples, codes and keep masks then lie where `_windows_to_host` expects those of a window entry
            n_l, keep_l = n[live], keep[live]
            lay = o, n_out, n_g, _, buf = self._windows_layout(n_l, keep_l, True, [] if companded else None)
            masks = buf[n_out + n_g: n_out + n_g + int(o[-1]) // 8] if keep_l.any() else None
            self.float_to_int16_ragged(lim[: int(o[-1])], o, product, keep_thr if keep_l.any() else None, out=(buf[:n_out].view(torch.int16), masks))
            chunks = lay, n_l, keep_l, live
        self._windows_emit(ws, chunks, True, companded, out)

    def _flac_rounds(self, pcm: torch.Tensor, masks, idx, pushes, out: list) -> list:
        """pushes[j] is window idx[j]'s, its stream the (stage, handle) of the window's record: ONE `flac_stream_step` and ONE
        `adpcm_stream_step` (each for its own windows) when no stream is named twice, else the r-th push of a stream goes to step r,
        in the order given; -> `out` with the windows' chunks in place"""
        out = list(out)
        for members in SP.rounds(p[0] for p in pushes)[1]:
            rnd = [(idx[j], pushes[j]) for j in members]
            for arg, step in (("flac", self.flac_stream_step), ("adpcm", self.adpcm_stream_step)):
                mine = [(i, p) for i, p in rnd if p[0][0] == arg]
                if mine:
                    for (i, _), c in zip(mine, step(pcm, [(p[0][1], *p[1:]) for _, p in mine], None, masks)):
                        out[i] = c
        return out

    def _pass_plain(self, store: torch.Tensor, S: int, cap: int, ws, pcm16: bool, keep_thr: Optional[float], product: str, companded: bool):
        """One decoder pass over the windows `ws`, every one at speed 1 and 24 kHz (ctts_codec_decode_windows) -> the chunks where they
        lie on the device: (the output's layout `_windows_layout`, the chunks' lengths, their keep flags, live: the places in `ws` of
        the windows that have a chunk); None when no window has a sample.  `_pass_rate` and `_pass_speed` hand back the same"""
        rows, live = [], []
        for k, w in enumerate(ws):
            win = window_for_samples(w.Tn, w.s_lo, w.hi)
            if win is not None:
                rows.append((w.slot, *win, int(w.tail and keep_thr is not None), 0, 0))
                live.append(k)
        if not live:
            return None
        tab = np.ascontiguousarray(np.array(rows, dtype=np.int32))          # ctts_window[n]: slot, t_lo, t_hi, c_lo, c_hi, keep, 0, 0
        n = (tab[:, 4] - tab[:, 3]).astype(np.int64)
        lay = self._windows_layout(n, tab[:, 5], pcm16, [] if companded else None)
        tab_d = torch.from_numpy(tab).to(self.device)
        cur, tail_args = self._windows_call_tail(lay, tab[:, 5], pcm16, product, keep_thr,
                                                 self.lib.ctts_codec_windows_workspace_bytes(len(live), int((tab[:, 2] - tab[:, 1]).sum())))
        _lib.check(self.lib.ctts_codec_decode_windows(self.handle, store.data_ptr(), int(store.stride(0)), int(store.stride(1)), S, cap,
                                                      tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(live), *tail_args),
                   "ctts_codec_decode_windows")
        tab_d.record_stream(cur)
        return lay, n, tab[:, 5], live

    def _pass_speed(self, store: torch.Tensor, S: int, cap: int, ws, pcm16: bool, keep_thr: Optional[float], product: str, companded: bool):
        """`_pass_plain` for windows of which at least one is at another speed than 1: a scaled window pushes its crop into its
        time-scale stream and, at another rate, what that emits into its resampler stream (ctts_codec_decode_windows_speed /
        _speed_rate); an empty crop still steps its streams.  The windows at speed 1 are at 24 kHz"""
        rows, conv, pushes = [], [], []     # decode windows; (place in ws, decode row or None, push or None, keep); stream pushes
        push_rs = []                        # per push: the resampler stream its chunk goes on into, or None
        for j, w in enumerate(ws):
            win = window_for_samples(w.Tn, w.s_lo, w.hi)
            if win is None and not w.scaled:
                continue
            k = None
            if win is not None:
                k = len(rows)
                rows.append((w.slot, *win, 0, 0, 0))
            if w.scaled:
                pushes.append([int(w.h[WC.PLACE["time_scale"]]), k, 0, w.tail])
                push_rs.append(int(w.h[WC.PLACE["resample"]]) if w.rate != self.SAMPLE_RATE else None)
            conv.append((j, k, len(pushes) - 1 if w.scaled else None, int(w.tail and keep_thr is not None)))
        tab = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 8))       # ctts_window[n_win]: what is decoded
        tok, start = self._packed_crops(tab)
        width = (tab[:, 4] - tab[:, 3]).astype(np.int64)
        for p in pushes:
            p[1], p[2] = (0, 0) if p[1] is None else (int(start[p[1]]), int(width[p[1]]))
        ts, round_off, order, n_path, commit = self._ts_descriptors([tuple(p) for p in pushes])
        rank = {i: r for r, i in enumerate(order)}                                       # push -> its row of the descriptor table
        ctab = np.zeros((len(conv), 8), np.int32)                                        # ctts_window[n_conv]: only `keep` is read
        rtab = np.zeros(len(conv), _lib.RS_WINDOW)
        rtab["rate"] = -1
        chunk = paths = 0
        for e, (i, k, pi, keep) in enumerate(conv):
            ctab[e, 5] = keep
            if k is not None:
                rtab["in_off"][e], rtab["n_in"][e] = start[k], width[k]
            if pi is not None:
                r = rank[pi]
                m = int(ts["n_out"][r])
                ts["out_off"][r], ts["path_off"][r] = chunk, paths
                rtab["o_hi"][e], rtab["out_off"][e], rtab["rate"][e] = m, chunk, r
                chunk += (m + 7) // 8 * 8
                paths += n_path[r]
        # the resampler stage: every scaled chunk that leaves 24 kHz is the push of its resampler stream; the resampled chunks lie behind
        # all scaled ones, in chunk order, and the output entry then names the resampled chunk
        staged = [(e, pi) for e, (_, _, pi, _) in enumerate(conv) if pi is not None and push_rs[pi] is not None]
        rs = groups = rs_commit = None
        if staged:
            rs, groups, rs_order, rs_commit = self._rs_descriptors(
                [(push_rs[pi], int(ts["out_off"][rank[pi]]), int(ts["n_out"][rank[pi]]), pushes[pi][3]) for _, pi in staged])
            rs_rank = {k: r for r, k in enumerate(rs_order)}
            rs_of_ts = np.full(len(ts), -1, np.int32)
            for k, (e, pi) in enumerate(staged):
                r = rs_rank[k]
                m = int(rs["n_out"][r])
                rs["out_off"][r], rs["pad"][r] = chunk, -m % 8
                rtab["o_hi"][e], rtab["out_off"][e] = m, chunk
                rs_of_ts[rank[pi]] = r
                chunk += m + (-m % 8)
        n = np.where(rtab["rate"] >= 0, rtab["o_hi"], rtab["n_in"]).astype(np.int64)
        lay = self._windows_layout(n, ctab[:, 5], pcm16, [] if companded else None)
        parts = [tab.view(np.uint8).reshape(-1), ctab.view(np.uint8).reshape(-1), rtab.view(np.uint8), ts.view(np.uint8)]
        if staged:
            parts.append(rs.view(np.uint8))
        blob_d = torch.from_numpy(np.concatenate(parts)).to(self.device)                 # one upload: the tables
        p0 = blob_d.data_ptr()
        p1, p2 = p0 + parts[0].nbytes, p0 + parts[0].nbytes + parts[1].nbytes
        p3 = p2 + parts[2].nbytes
        pool = self._pool("time_scale")
        cur, tail_args = self._windows_call_tail(lay, ctab[:, 5], pcm16, product, keep_thr, self.lib.ctts_codec_windows_speed_workspace_bytes(
            len(rows), int(tok[-1]), chunk + (paths + 7) // 8 * 8))
        front = (self.handle, store.data_ptr(), int(store.stride(0)), int(store.stride(1)), S, cap, p0 if len(rows) else None,
                 tab.ctypes.data_as(C.c_void_p) if len(rows) else None, len(rows), p1, ctab.ctypes.data_as(C.c_void_p), p2,
                 rtab.ctypes.data_as(C.c_void_p), len(conv), p3, ts.ctypes.data_as(C.c_void_p), round_off.ctypes.data_as(C.c_void_p),
                 len(round_off) - 1, pool.buf["carry"].data_ptr(), pool.buf["state"].data_ptr(), pool.slots,
                 self._time_scale_window().data_ptr())
        if staged:
            pairs = sorted({g[1] for g in groups})
            rate_tab = (_lib.Rate * len(pairs))()
            for k, (orig, new) in enumerate(pairs):
                L, M = RS.ratio(orig, new)
                rate_tab[k].taps, rate_tab[k].L, rate_tab[k].M, rate_tab[k].K = self._resample_taps(orig, new).data_ptr(), L, M, RS.geometry(L, M)[1]
            grp_off = np.array([g[2] for g in groups] + [groups[-1][3]], dtype=np.int32)
            grp_rate = np.array([pairs.index(g[1]) for g in groups], dtype=np.int32)
            rs_pool = self._pool("resample")
            _lib.check(self.lib.ctts_codec_decode_windows_speed_rate(
                *front, p3 + parts[3].nbytes, rs.ctypes.data_as(C.c_void_p), rs_of_ts.ctypes.data_as(C.c_void_p),
                grp_off.ctypes.data_as(C.c_void_p), grp_rate.ctypes.data_as(C.c_void_p), len(groups), C.cast(rate_tab, C.c_void_p), len(pairs),
                rs_pool.buf["carry"].data_ptr(), rs_pool.slots, *tail_args), "ctts_codec_decode_windows_speed_rate")
        else:
            _lib.check(self.lib.ctts_codec_decode_windows_speed(*front, *tail_args), "ctts_codec_decode_windows_speed")
        blob_d.record_stream(cur)
        pool.commit(commit)
        if staged:
            rs_pool.commit(rs_commit)
        return lay, n, ctab[:, 5], [c[0] for c in conv]

    def _windows_to_host(self, buf: torch.Tensor, n_out: int, n_g: int, off, n, keep, live, laws, dt, out: list, fl=None) -> list:
        """the end of `decode_windows`: `buf` = samples (n_out bytes) | companded bytes (n_g, 0 without `laws`) | keep masks.  The
        companded windows (laws[k] >= 0) are converted by one launch over their own element offsets `off`; ONE copy to the host -- of
        the codes and the masks when every window is companded, of the whole buffer otherwise -- and live window k becomes out[live[k]].
        `fl` = (FLAC stream or None per window, tail flag per window): the flagged windows, live or not, are the pushes of ONE
        `flac_stream_step` over the int16 samples and the keep masks where they lie; their samples are not copied, and when every
        live window is flagged nothing of `buf` is"""
        chunks = {}
        if fl is not None:
            row = {i: k for k, i in enumerate(live)}
            idx = [i for i, h in enumerate(fl[0]) if h is not None]
            pushes = [(fl[0][i], int(off[row[i]]), int(n[row[i]]), fl[1][i], None, bool(keep[row[i]])) if i in row else (fl[0][i], 0, 0, fl[1][i])
                      for i in idx]
            masks = buf[n_out + n_g:] if any(len(p) > 4 and p[5] for p in pushes) else None
            done = self._flac_rounds(buf[:n_out].view(torch.int16), masks, idx, pushes, out)
            chunks = {i: done[i] for i in idx}
            if all(i in chunks for i in live):
                out[:] = done
                return out
        base = 0
        if laws is not None:
            self.g711_encode(buf[:n_out].view(torch.int16), [(int(off[k]), int(n[k]), laws[k]) for k in range(len(live))],
                             out=buf[n_out: n_out + n_g])
            if all(l >= 0 for l in laws):
                base = n_out
        host = self.to_host(buf[base:] if base else buf)
        vals = host[: n_out - base].view(dt) if base == 0 else None
        codes = host[n_out - base: n_out - base + n_g]
        for k, i in enumerate(live):
            if laws is not None and laws[k] >= 0:
                a = codes[int(off[k]): int(off[k]) + int(n[k])]
            else:
                a = vals[int(off[k]): int(off[k]) + int(n[k])]
            if keep[k]:
                kb = n_out - base + n_g + int(off[k]) // 8
                a = a[np.unpackbits(host[kb: kb + (int(n[k]) + 7) // 8])[: int(n[k])].astype(bool)]
            out[i] = a
        for i, c in chunks.items():
            out[i] = c
        return out

    def g711_encode(self, pcm: torch.Tensor, ranges, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """G.711 companding on the device (ctts_g711_encode_ranges, csrc/g711.hip): `pcm`, a contiguous int16 device tensor, taken as
        flat; `ranges`: up to 1024 (start, n, law) in ascending order -- elements [start, start + n) become BYTES [start, start + n)
        of the result under law 0 / "ulaw", 1 / "alaw"; -1 / None: the range is skipped.  Starts are multiples of 8.  Returns a flat
        uint8 device tensor of pcm.numel() bytes (rounded up to 16; `out`: write into this one instead); bytes outside the ranges
        and those of skipped ranges are left as they were.  One launch whatever the number of ranges; equal to `g711.encode` byte
        for byte.  The library refuses bad tables before anything is launched (EngineError)."""
        if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()):
            raise ValueError("g711_encode: a contiguous int16 device tensor")
        n_el = pcm.numel()
        if out is None:
            out = torch.empty(((n_el + 15) // 16 * 16,), dtype=torch.uint8, device=pcm.device)
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n_el):
            raise ValueError("g711_encode: `out` must be a contiguous uint8 device tensor of at least pcm.numel() bytes")
        tab = np.zeros(len(ranges), _lib.G711_RANGE)
        for k, (start, n, law) in enumerate(ranges):
            tab[k] = (int(start), int(n), -1 if law is None or law == -1 else G711.law_of(law), 0, 0)
        if len(tab) and int((tab["start"] + np.maximum(tab["n"], 0)).max()) > n_el:
            raise ValueError(f"g711_encode: a range ends beyond the {n_el} samples")
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(pcm.device)
        st = torch.cuda.current_stream(pcm.device)
        _lib.check(self.lib.ctts_g711_encode_ranges(pcm.data_ptr(), out.data_ptr(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), len(tab),
                                                    st.cuda_stream), "ctts_g711_encode_ranges")
        tab_d.record_stream(st)
        return out

    def flac_encode(self, pcm: torch.Tensor, ranges, counts: Optional[torch.Tensor] = None, info: bool = False) -> list:
        """FLAC on the device (ctts_flac_encode_ranges, csrc/flac.hip): `pcm`, a contiguous int16 device tensor, taken as flat;
        `ranges`: up to 1024 (start, n, rate) or (start, n, rate, count_idx) in ascending order -- elements [start, start + n) are one
        signal at `rate` Hz (None / 0: the range is skipped); with a count_idx the signal's length is min(counts[count_idx], n), read on
        the device (`counts`: an int64 device tensor, e.g. float_to_int16_groups' count header).  Starts are multiples of 8.  Returns
        one uint8 array per range, its frames back to back (`flac.frames` byte for byte; None for a skipped range); `info`: (frames,
        frame lengths, samples) instead -- what `flac.file_bytes` needs.  Three launches whatever the number of ranges, then one small
        copy (the frame offsets, the total and the sample counts) and one copy of exactly the bytes used: the compressed bytes are what
        cross the bus.  The library refuses bad tables before anything is launched (EngineError)."""
        if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()):
            raise ValueError("flac_encode: a contiguous int16 device tensor")
        if counts is not None and not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()):
            raise ValueError("flac_encode: `counts` must be a contiguous int64 device tensor")
        n_el, n_rng = pcm.numel(), len(ranges)
        tab = np.zeros(n_rng, _lib.FLAC_RANGE)
        slots = 0
        for k, r in enumerate(ranges):
            rate = int(r[2] or 0)
            ci = int(r[3]) if len(r) > 3 and r[3] is not None else -1
            if ci >= 0 and (counts is None or ci >= counts.numel()):
                raise ValueError(f"flac_encode: range {k} reads count {ci}, beyond `counts`")
            tab[k] = (int(r[0]), int(r[1]), rate, ci, slots)
            slots += (max(int(r[1]), 0) + FLAC.BLOCK - 1) // FLAC.BLOCK if rate else 0
        if n_rng and int((tab["start"] + np.maximum(tab["n"], 0)).max()) > n_el:
            raise ValueError(f"flac_encode: a range ends beyond the {n_el} samples")
        sizes = (C.c_int64 * 3)()
        _lib.check(self.lib.ctts_flac_encode_sizes(tab.ctypes.data_as(C.c_void_p), n_rng, sizes), "ctts_flac_encode_sizes")
        n_frames, out_bytes, work_bytes = (int(v) for v in sizes)
        empty = np.zeros((0,), np.uint8)
        if n_frames == 0:
            res = [(None if not tab["rate"][k] else empty) for k in range(n_rng)]
            return [None if b is None else (b, np.zeros((0,), np.int64), 0) for b in res] if info else res
        dev = pcm.device
        out = torch.empty(((out_bytes + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_flac_encode_ranges(pcm.data_ptr(), _lib.ptr(counts), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), n_rng,
                                                    out.data_ptr(), out.numel(), work.data_ptr(), work.numel(), st.cuda_stream),
                   "ctts_flac_encode_ranges")
        tab_d.record_stream(st)
        meta = self.to_host(work[: (8 * (n_frames + 1 + n_rng) + 15) // 16 * 16]).view(np.int64)     # offsets, total, sample counts
        total = int(meta[n_frames])
        blob = self.to_host(out[: (total + 15) // 16 * 16])[:total] if total else empty
        res = []
        for k in range(n_rng):
            if not tab["rate"][k]:
                res.append(None)
                continue
            f0 = int(tab["frame0"][k])
            offs = meta[f0: f0 + (int(tab["n"][k]) + FLAC.BLOCK - 1) // FLAC.BLOCK + 1]
            lens = np.diff(offs)
            frames = blob[int(offs[0]): int(offs[-1])]
            res.append((frames, lens[lens > 0], int(meta[n_frames + 1 + k])) if info else frames)
        return res

    def adpcm_encode(self, pcm: torch.Tensor, ranges, counts: Optional[torch.Tensor] = None, info: bool = False) -> list:
        """IMA ADPCM on the device (ctts_adpcm_encode_ranges, csrc/adpcm.hip): `pcm`, a contiguous int16 device tensor, taken as flat;
        `ranges`: up to 1024 (start, n, rate) or (start, n, rate, count_idx) in ascending order -- elements [start, start + n) are one
        signal at `rate` Hz (None / 0: the range is skipped); with a count_idx the signal's length is min(counts[count_idx], n), read on
        the device (`counts`: an int64 device tensor, e.g. float_to_int16_groups' count header).  Starts are multiples of 8.  Returns
        one uint8 array per range, its blocks back to back (`adpcm.encode_blocks` byte for byte; empty for a signal of no samples, None
        for a skipped range); `info`: (blocks, samples) instead -- what `adpcm.wav_bytes` needs.  One launch whatever the number of
        ranges, then one small copy (the sample counts) when a range leaves its length to the device, and one copy of the blocks: the
        4-bit codes are what cross the bus.  The library refuses bad tables before anything is launched (EngineError)."""
        if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous()):
            raise ValueError("adpcm_encode: a contiguous int16 device tensor")
        if counts is not None and not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()):
            raise ValueError("adpcm_encode: `counts` must be a contiguous int64 device tensor")
        n_el, n_rng = pcm.numel(), len(ranges)
        tab = np.zeros(n_rng, _lib.ADPCM_RANGE)
        blocks = nbytes = 0
        for k, r in enumerate(ranges):
            rate = int(r[2] or 0)
            ci = int(r[3]) if len(r) > 3 and r[3] is not None else -1
            if ci >= 0 and (counts is None or ci >= counts.numel()):
                raise ValueError(f"adpcm_encode: range {k} reads count {ci}, beyond `counts`")
            tab[k] = (int(r[0]), int(r[1]), blocks, nbytes, rate, ci, 0)
            if rate > 0:
                nb = ADPCM.n_blocks(int(r[1]), rate)
                blocks, nbytes = blocks + nb, nbytes + nb * ADPCM.align(rate)
        if n_rng and int((tab["start"] + np.maximum(tab["n"], 0)).max()) > n_el:
            raise ValueError(f"adpcm_encode: a range ends beyond the {n_el} samples")
        sizes = (C.c_int64 * 3)()
        _lib.check(self.lib.ctts_adpcm_encode_sizes(tab.ctypes.data_as(C.c_void_p), n_rng, sizes), "ctts_adpcm_encode_sizes")
        n_blocks, out_bytes, used_bytes = (int(v) for v in sizes)
        empty = np.zeros((0,), np.uint8)
        if n_blocks == 0:
            return [None if not tab["rate"][k] else ((empty, 0) if info else empty) for k in range(n_rng)]
        dev = pcm.device
        buf = torch.empty((used_bytes + out_bytes,), dtype=torch.uint8, device=dev)      # the sample counts, then the blocks: one copy brings both
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_adpcm_encode_ranges(pcm.data_ptr(), _lib.ptr(counts), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p), n_rng,
                                                     buf.data_ptr() + used_bytes, out_bytes, buf.data_ptr(), used_bytes, st.cuda_stream),
                   "ctts_adpcm_encode_ranges")
        tab_d.record_stream(st)
        host = self.to_host(buf)
        used, blob = host[: 8 * n_rng].view(np.int64), host[used_bytes:]
        res = []
        for k in range(n_rng):
            rate = int(tab["rate"][k])
            if not rate:
                res.append(None)
                continue
            m = int(used[k])                                                             # the blocks behind ceil(m / S) were not written
            b0 = int(tab["byte0"][k])
            blk = blob[b0: b0 + ADPCM.n_blocks(m, rate) * ADPCM.align(rate)]
            res.append((blk, m) if info else blk)
        return res

    def float_to_int16_groups_adpcm(self, wav: torch.Tensor, off, grp, rates, product: str = "f64", keep_thr: Optional[float] = 1e-5,
                                    encodings=None) -> list:
        """`float_to_int16_groups` with IMA ADPCM behind it, `float_to_int16_groups_flac`'s form: `rates`, one entry per group -- None:
        the group comes back as `unpack_groups` hands it out (int16 samples, or with `encodings` its G.711 codes); a rate in Hz: as
        the complete WAVE_FORMAT_IMA_ADPCM file (a uint8 array; `adpcm.encode` byte for byte) of exactly its int16 samples.  The
        grouped slots and the count header on the device go straight into `adpcm_encode`; when every group is encoded the samples
        never cross the bus.  A group has a rate or an encoding, not both.  A group of no samples comes back as the bare 60-byte header
        (`adpcm.behind_decode`), as FLAC hands out a bare `fLaC` header there."""
        n_grp = len(grp) - 1
        if len(rates) != n_grp or (encodings is not None and len(encodings) != n_grp):
            raise ValueError("float_to_int16_groups_adpcm: one rate (or None) and one encoding (or None) per group")
        for g, r in enumerate(rates):
            if r is not None:
                ADPCM.check_rate(r)
                if encodings is not None and encodings[g] is not None:
                    raise ValueError("float_to_int16_groups_adpcm: a group is ADPCM or companded, not both")
        if encodings is not None and all(G711.check_encoding(e) is None for e in encodings):
            encodings = None
        blob, starts = self.float_to_int16_groups(wav, off, grp, product, keep_thr, encodings=encodings)
        if all(r is None for r in rates):
            return self.unpack_groups(self.to_host(blob), starts, encodings)
        hdr, E = (8 * n_grp + 15) // 16 * 16, int(starts[-1])
        pcm_at, cnt_at = (hdr, 0) if encodings is None else (0, 2 * E)           # header | samples, or samples | header | codes
        enc = self.adpcm_encode(blob[pcm_at: pcm_at + 2 * E].view(torch.int16),
                                [(int(starts[g]), int(starts[g + 1] - starts[g]), rates[g], g) for g in range(n_grp)],
                                counts=blob[cnt_at: cnt_at + 8 * n_grp].view(torch.int64), info=True)
        plain = self.unpack_groups(self.to_host(blob), starts, encodings) if any(r is None for r in rates) else None
        return [plain[g] if rates[g] is None else ADPCM.behind_decode(enc[g][0], enc[g][1], rates[g]) for g in range(n_grp)]

    # -- FLAC for streams: per-stream device state (csrc/flac.hip, flac_stage_k) ---------------------------------------------------------
    # `_flac_pool` / `_flac_rec` (and ADPCM's pair below) are all of the pool seam that the stream methods of the two int16 formats use,
    # so that an object with no more than a library, a device and its `*_STREAM_SLOTS` can borrow them without the decoder's weights
    def _flac_pool(self) -> SP.StatePool:
        return CodecEngine._pool(self, "flac")

    def _flac_rec(self, handle: int):
        return self._flac_pool().live(handle)

    def flac_stream_open(self, rate: int, first_sample: int = 0) -> int:
        """A FLAC stream at `rate` Hz whose first sample has the number `first_sample`: -> its handle, a slot of the engine's state
        pool.  The slot is fresh by construction -- a stream that holds no samples reads none -- so nothing is cleared.  ValueError for
        a rate the format cannot code and a sample number beyond 36 bits."""
        FLAC.rate_code(rate)
        if not 0 <= int(first_sample) < FLAC.MAX_SAMPLES:
            raise ValueError(f"flac: sample number {first_sample} does not fit 36 bits")
        return self._flac_pool().open(SP.FlacRec(int(rate), int(first_sample), 0, False))

    def flac_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._flac_pool().close(handle)

    def flac_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._flac_pool().in_use

    def flac_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`flac.stream_plan` of the stream's next push: the blocks a step with `n_in` more samples would emit, the number of the first
        of them, the samples the stream would hold afterwards, and the most bytes the push can emit"""
        rec = self._flac_rec(handle)
        blocks, held = FLAC.stream_plan(rec.carry, n_in, final)
        return dict(rate=rec.rate, sample=rec.sample, blocks=blocks, carry=held, bound=FLAC.stream_bound(n_in))

    def flac_stream_step(self, pcm: torch.Tensor, pushes, counts: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None) -> list:
        """ONE step of many FLAC streams (ctts_flac_stream_step: four launches whatever their number): `pcm`, a contiguous int16 device
        tensor taken as flat, holds the new samples of every stream; `pushes` = [(handle, start, n, final)] or [(handle, start, n,
        final, count_idx, masked)]: pcm[start, start + n) continue stream `handle` (n 0: nothing new; starts are multiples of 8),
        `final`: they are its last.  A final push may leave its length to the device: with a count_idx only the first
        min(counts[count_idx], n) samples count (`counts`: an int64 device tensor), and `masked` keeps only the samples whose bit is
        set in `masks` (a uint8 device tensor, MSB first, the bit of element e of `pcm` in byte e / 8: `decode_windows`' keep masks).
        -> one uint8 array per push: the frames that push completes (possibly none), `flac.StreamEncoder.push` byte for byte; behind
        `flac.stream_header(rate)` a stream's chunks are a FLAC stream of its pushes, concatenated, however they were cut.  A handle may
        appear once per call.  One small copy (the frame offsets and the total) and one copy of exactly the bytes used come to the host;
        the samples stay on the device.  Every refusal (ValueError here, EngineError from the library) comes before the first launch
        and leaves all streams as they were."""
        pool = self._flac_pool()
        tab = np.zeros(len(pushes), _lib.FLAC_PUSH)
        stage = slots = 0
        commit = {}
        for k, (h, start, n, final, ci, masked, rec) in enumerate(SP.int16_pushes("flac", pcm, pushes, counts, masks, self._flac_rec)):
            rate, sample, carry = rec.rate, rec.sample, rec.carry
            if sample + carry + n >= FLAC.MAX_SAMPLES:
                raise ValueError(f"flac: push {k} would take the stream's sample number to 2^36")
            tab[k] = (start, n, sample, stage, slots, rate, h, carry, int(final) | 2 * int(masked), ci, 0)
            blocks, held = FLAC.stream_plan(carry, n, final)                     # a final push's own count only shortens its last blocks
            commit[h] = SP.FlacRec(rate, sample + sum(blocks), held, final)
            stage += (carry + n + 7) // 8 * 8
            slots += (carry + n + FLAC.BLOCK - 1) // FLAC.BLOCK
        n_el, n_push, n_slots = pcm.numel(), len(pushes), pool.slots
        sizes = (C.c_int64 * 4)()
        _lib.check(self.lib.ctts_flac_stream_sizes(tab.ctypes.data_as(C.c_void_p), n_push, n_slots, n_el, sizes), "ctts_flac_stream_sizes")
        n_frames, out_bytes, work_bytes, _ = (int(v) for v in sizes)
        empty = np.zeros((0,), np.uint8)
        if n_frames == 0:                                                        # no stream holds or gets a sample
            pool.commit(commit)
            return [empty for _ in pushes]
        dev = pcm.device
        out = torch.empty(((out_bytes + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_flac_stream_step(pcm.data_ptr(), n_el, _lib.ptr(masks), _lib.ptr(counts), tab_d.data_ptr(),
                                                  tab.ctypes.data_as(C.c_void_p), n_push, pool.buf["carry"].data_ptr(), n_slots, out.data_ptr(),
                                                  out.numel(), work.data_ptr(), work.numel(), st.cuda_stream), "ctts_flac_stream_step")
        tab_d.record_stream(st)
        pool.commit(commit)
        meta = self.to_host(work[: (8 * (n_frames + 1) + 15) // 16 * 16]).view(np.int64)              # the slots' offsets and the total
        total = int(meta[n_frames])
        blob = self.to_host(out[: (total + 15) // 16 * 16])[:total] if total else empty
        res = []
        for k in range(n_push):
            f0 = int(tab["frame0"][k])
            f1 = f0 + (int(tab["carry"][k]) + int(tab["n"][k]) + FLAC.BLOCK - 1) // FLAC.BLOCK
            res.append(blob[int(meta[f0]): int(meta[f1])])
        return res

    # -- IMA ADPCM for streams: per-stream device state (csrc/adpcm.hip, adpcm_stage_k) -------------------------------------------------
    def _adpcm_pool(self) -> SP.StatePool:
        return CodecEngine._pool(self, "adpcm")

    def _adpcm_rec(self, handle: int):
        return self._adpcm_pool().live(handle)

    def adpcm_stream_open(self, rate: int) -> int:
        """An IMA ADPCM stream at `rate` Hz: -> its handle, a slot of the engine's state pool.  The slot is fresh by construction -- a
        stream that holds no samples reads none -- so nothing is cleared.  ValueError for a rate that is no rate, or whose block
        (55125 Hz and above) does not fit a slot."""
        if ADPCM.samples_per_block(rate) - 1 > self.ADPCM_CARRY:
            raise ValueError(f"adpcm: a block at {rate} Hz holds {ADPCM.samples_per_block(rate)} samples, more than a stream's slot "
                             f"({self.ADPCM_CARRY}): streams run below 55125 Hz")
        return self._adpcm_pool().open(SP.AdpcmRec(int(rate), 0, False))

    def adpcm_stream_close(self, handle: int) -> None:
        """gives the stream's slot back (any time: finished, or abandoned half way)"""
        self._adpcm_pool().close(handle)

    def adpcm_streams_in_use(self) -> int:
        """the streams that are open: slots of the state pool not on its free list"""
        return self._adpcm_pool().in_use

    def adpcm_stream_plan(self, handle: int, n_in: int, final: bool) -> dict:
        """`adpcm.stream_plan` of the stream's next push: the blocks a step with `n_in` more samples would emit, the samples the stream
        would hold afterwards, and the most bytes the push can emit"""
        rec = self._adpcm_rec(handle)
        blocks, held = ADPCM.stream_plan(rec.carry, n_in, final, rec.rate)
        return dict(rate=rec.rate, blocks=blocks, carry=held, bound=ADPCM.stream_bound(n_in, rec.rate))

    def adpcm_stream_step(self, pcm: torch.Tensor, pushes, counts: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None) -> list:
        """ONE step of many IMA ADPCM streams (ctts_adpcm_stream_step: two launches whatever their number): `pcm`, a contiguous int16
        device tensor taken as flat, holds the new samples of every stream; `pushes` = [(handle, start, n, final)] or [(handle, start,
        n, final, count_idx, masked)]: pcm[start, start + n) continue stream `handle` (n 0: nothing new; starts are multiples of 8),
        `final`: they are its last.  A final push may leave its length to the device: with a count_idx only the first
        min(counts[count_idx], n) samples count (`counts`: an int64 device tensor), and `masked` keeps only the samples whose bit is
        set in `masks` (a uint8 device tensor, MSB first, the bit of element e of `pcm` in byte e / 8: `decode_windows`' keep masks).
        -> one uint8 array per push: the blocks that push completes (possibly none), `adpcm.StreamEncoder.push` byte for byte; behind
        `adpcm.stream_header(rate)` a stream's chunks are the blocks of `adpcm.encode_blocks` over its pushes, concatenated, however
        they were cut.  A handle may appear once per call.  When no push leaves its length to the device the chunk sizes are known
        here and ONE copy, of the blocks, comes to the host; otherwise one more small copy brings the samples each push encoded.  The
        samples stay on the device.  Every refusal (ValueError here, EngineError from the library) comes before the first launch and
        leaves all streams as they were."""
        pool = self._adpcm_pool()
        tab = np.zeros(len(pushes), _lib.ADPCM_PUSH)
        stage = blocks = nbytes = samples = 0
        commit, by_device = {}, False
        for k, (h, start, n, final, ci, masked, rec) in enumerate(SP.int16_pushes("adpcm", pcm, pushes, counts, masks, self._adpcm_rec)):
            rate, carry = rec.rate, rec.carry
            by_device = by_device or ci >= 0 or masked
            tab[k] = (start, n, stage, blocks, nbytes, rate, h, carry, int(final) | 2 * int(masked), ci, 0)
            nb, held = ADPCM.stream_plan(carry, n, final, rate)                  # a final push's own count only lowers its blocks
            commit[h] = SP.AdpcmRec(rate, held, final)
            stage += (carry + n + 7) // 8 * 8
            blocks, nbytes, samples = blocks + nb, nbytes + nb * ADPCM.align(rate), samples + carry + n
        n_el, n_push, n_slots = pcm.numel(), len(pushes), pool.slots
        sizes = (C.c_int64 * 4)()
        _lib.check(self.lib.ctts_adpcm_stream_sizes(tab.ctypes.data_as(C.c_void_p), n_push, n_slots, n_el, sizes), "ctts_adpcm_stream_sizes")
        n_blocks, out_bytes, work_bytes, _ = (int(v) for v in sizes)
        empty = np.zeros((0,), np.uint8)
        if samples == 0:                                                         # no stream holds or gets a sample
            pool.commit(commit)
            return [empty for _ in pushes]
        dev = pcm.device
        out = torch.empty((max(out_bytes, 16),), dtype=torch.uint8, device=dev)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device=dev)
        tab_d = torch.from_numpy(tab.view(np.uint8)).to(dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(self.lib.ctts_adpcm_stream_step(pcm.data_ptr(), n_el, _lib.ptr(masks), _lib.ptr(counts), tab_d.data_ptr(),
                                                   tab.ctypes.data_as(C.c_void_p), n_push, pool.buf["carry"].data_ptr(), n_slots, out.data_ptr(),
                                                   out.numel(), work.data_ptr(), work.numel(), st.cuda_stream), "ctts_adpcm_stream_step")
        tab_d.record_stream(st)
        pool.commit(commit)
        if n_blocks == 0:                                                        # samples went to the slots, and no block is complete
            return [empty for _ in pushes]
        used = self.to_host(work[: (8 * n_push + 15) // 16 * 16]).view(np.int64) if by_device else None
        blob = self.to_host(out[:out_bytes])
        res = []
        for k in range(n_push):
            rate, b0 = int(tab["rate"][k]), int(tab["byte0"][k])
            if used is None:
                size = ADPCM.stream_plan(int(tab["carry"][k]), int(tab["n"][k]), bool(tab["flags"][k] & 1), rate)[0] * ADPCM.align(rate)
            else:
                size = (ADPCM.n_blocks(int(used[k]), rate) if tab["flags"][k] & 1 else int(used[k]) // ADPCM.samples_per_block(rate)) * ADPCM.align(rate)
            res.append(blob[b0: b0 + size])
        return res

    def _pass_rate(self, store: torch.Tensor, S: int, cap: int, ws, pcm16: bool, keep_thr: Optional[float], product: str, companded: bool):
        """`_pass_plain` for windows at speed 1 of which at least one is at another rate than 24 kHz: the stateless window path
        (ctts_codec_decode_windows_rate)"""
        plans, pairs = {}, {}              # rate -> (L, M, K); rate -> (index, L, M, K) once a window at it has samples
        rows, res, live = [], [], []
        for k, w in enumerate(ws):
            r, hi, total = w.rate, w.hi, VOCOS.hop * (2 * w.Tn - 1)
            if r == self.SAMPLE_RATE:
                win, rs = window_for_samples(w.Tn, w.s_lo, hi), None
            else:
                if r not in plans:
                    plans[r] = RS.plan(self.SAMPLE_RATE, r, [0, 1])[:3]        # every refusal before the launch
                L, M, K = plans[r]
                lo, hi = max(0, w.s_lo), min(total, hi)
                o_lo, o_hi = (RS.out_len(lo, L, M), RS.out_len(hi, L, M)) if hi > lo else (0, 0)
                win = None
                if o_hi > o_lo:
                    a, b = RS.window_inputs(L, M, K, o_lo, o_hi, total)
                    q = pairs.setdefault(r, (len(pairs), L, M, K))[0]
                    win, rs = window_for_samples(w.Tn, a, b), (q, a, total, o_lo, o_hi)
            if win is None:
                continue
            rows.append((w.slot, *win, int(w.tail and keep_thr is not None), 0, 0))
            res.append(rs)
            live.append(k)
        if not live:
            return None
        tab = np.ascontiguousarray(np.array(rows, dtype=np.int32))          # ctts_window[n]
        tok, start = self._packed_crops(tab)
        rtab = np.zeros(len(live), _lib.RS_WINDOW)                           # ctts_rs_window[n]
        rtab["in_off"] = start
        rtab["n_in"] = tab[:, 4] - tab[:, 3]
        rtab["rate"] = -1
        chunk = 0
        for k, rs in enumerate(res):
            if rs is not None:
                q, a, total, o_lo, o_hi = rs
                m = o_hi - o_lo
                rtab[k] = (rtab["in_off"][k], rtab["n_in"][k], a, total, o_lo, o_hi, chunk, q, -m % 8)
                chunk += m + (-m % 8)
        sel = np.array([k for q in range(len(pairs)) for k, rs in enumerate(res) if rs is not None and rs[0] == q], dtype=np.int32)
        n = np.where(rtab["rate"] >= 0, rtab["o_hi"] - rtab["o_lo"], rtab["n_in"]).astype(np.int64)
        lay = self._windows_layout(n, tab[:, 5], pcm16, [] if companded else None)
        blob = np.concatenate([tab.view(np.uint8).reshape(-1), rtab.view(np.uint8), sel.view(np.uint8)])
        blob_d = torch.from_numpy(blob).to(self.device)                      # one upload: both tables and the selection
        by_q = sorted(pairs.items(), key=lambda kv: kv[1][0])
        rate_tab = (_lib.Rate * max(1, len(by_q)))()
        for r, (q, L, M, K) in by_q:
            rate_tab[q].taps, rate_tab[q].L, rate_tab[q].M, rate_tab[q].K = self._resample_taps(self.SAMPLE_RATE, r).data_ptr(), L, M, K
        cur, tail_args = self._windows_call_tail(lay, tab[:, 5], pcm16, product, keep_thr,
                                                 self.lib.ctts_codec_windows_rate_workspace_bytes(len(live), int(tok[-1]), chunk))
        base = blob_d.data_ptr()
        _lib.check(self.lib.ctts_codec_decode_windows_rate(
            self.handle, store.data_ptr(), int(store.stride(0)), int(store.stride(1)), S, cap, base, tab.ctypes.data_as(C.c_void_p),
            base + tab.nbytes, rtab.ctypes.data_as(C.c_void_p), base + tab.nbytes + rtab.nbytes, sel.ctypes.data_as(C.c_void_p), len(live),
            C.cast(rate_tab, C.c_void_p), len(by_q), *tail_args), "ctts_codec_decode_windows_rate")
        blob_d.record_stream(cur)
        return lay, n, tab[:, 5], live

    def to_host(self, t: torch.Tensor) -> np.ndarray:
        """device tensor -> numpy, the `.cpu().numpy()` that ends the reference path (core.py:508-510), through a cached PINNED
        staging buffer: a pageable `.cpu()` of the 67 MB of waveforms of a 64-utterance batch runs at a fraction of the PCIe rate.
        The returned array is a copy (the staging buffer is reused by the next call)."""
        t = t.contiguous()
        n = t.numel()
        if n == 0:
            return np.zeros(tuple(t.shape), dtype={torch.int16: np.int16, torch.uint8: np.uint8}.get(t.dtype, np.float32))
        pins = self.__dict__.setdefault("_pinned", {})     # one grow-only staging buffer per element type (float32 waveforms, int16 PCM, uint8 masks)
        buf = pins.get(t.dtype)
        if buf is None or buf.numel() < n:
            buf = pins[t.dtype] = torch.empty(((n + 15) // 16 * 16,), dtype=t.dtype).pin_memory()
        view = buf[:n].view(t.shape)
        nbytes = n * t.element_size()
        if nbytes >= (16 << 20) and nbytes % 64 == 0 and t.data_ptr() % 16 == 0 and os.environ.get("CTTS_D2H_PIPE", "1") != "0":
            # a batch's worth of waveforms: the copy over PCIe (1.2 ms for 67 MB) and the copy out of the staging buffer (2 ms on 4
            # threads) in 4 pieces, piece i leaving the staging buffer while piece i + 1 crosses the bus (tools/pass_timeline.py)
            return self._to_host_piped(t, view, nbytes)
        if nbytes % 16 == 0 and t.data_ptr() % 16 == 0 and os.environ.get("CTTS_D2H_SHADER", "1") != "0":
            # shader copy (plain stores over PCIe into the pinned buffer): the same rate as hipMemcpyAsync (67 MB in 1.2 ms,
            # profiles/r3j_d2h_probe.log) and just the next packet of the stream -- no copy-engine hand-off behind the decode kernels
            _lib.check(self.lib.ctts_copy_bytes(view.data_ptr(), t.data_ptr(), nbytes, torch.cuda.current_stream(self.device).cuda_stream),
                       "ctts_copy_bytes")
        else:
            view.copy_(t, non_blocking=True)
        wait_stream(torch.cuda.current_stream(self.device))
        # The result must not alias the staging buffer: copy it out with plain memcpy (numpy), NOT `view.clone()`: torch's intra-op
        # pool has one thread per hardware thread (128 here) and this pool's hosts run under a 16-CPU cgroup quota, so waking it up
        # intermittently costs 60-90 ms of CFS throttling (profiles/r3l_hostcopy_probe.log: clone max 92 ms vs numpy 0.1 ms for one
        # streamed chunk) -- that was what turned the streaming config C5 from 266 into 600 ms per batch.  Large results are cut into
        # 4 slices copied by 4 plain threads (memcpy releases the GIL).
        return self._copy_out(view)

    # -- software pipelining across batches ------------------------------------------------------------------------------------
    def decode_to_wavs_async(self, result_list: List[torch.Tensor]) -> "PendingWavs":
        """`decode_to_wavs` + the `.cpu().numpy()` of core.py:508-510, ASYNCHRONOUSLY on the engine's own side stream: the call
        returns at once (everything is enqueued), `PendingWavs.result()` hands out the numpy array.  A caller that works through a
        queue of batches starts the NEXT batch's generation before asking for the result, so the acoustic decode (MFMA-bound, big
        kernels) overlaps the next batch's decode steps (latency-bound, most SIMDs idle) on the same GPU -- the batch-level form of
        what BASELINE config 4 does per streamed chunk.  The input tensors must not be modified until `result()` returned
        (`GptEngine.generate` hands out copies, so its outputs qualify).  Results are bit-identical to the synchronous calls."""
        dev = self.device
        if not hasattr(self, "_side"):
            # CTTS_CODEC_CUS="n[:stride[:first]]": the side stream is confined to n compute units (ctts_stream_create_cu_mask), so the big
            # MFMA kernels of the decode of batch i do not take the CUs the latency-bound decode steps of batch i + 1 run on
            spec = codec_cu_spec()
            if spec:
                self._side = cu_masked_stream(self.lib, dev, *spec, False)
            else:
                self._side = torch.cuda.Stream(device=dev)
            self._side_pins = [None, None]     # two staging buffers: a result may still be in its buffer when the next decode is enqueued
            self._side_n = 0
        caller = torch.cuda.current_stream(dev)
        ready = torch.cuda.Event()
        ready.record(caller)                   # the hidden states were produced on the caller's stream
        k = self._side_n = (self._side_n + 1) % 2
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            wav = self.decode_to_wavs(result_list)
            n = wav.numel()
            pin = self._side_pins[k]
            if pin is None or pin.numel() < n:
                pin = self._side_pins[k] = torch.empty(((n + 3) // 4 * 4,), dtype=torch.float32).pin_memory()
            view = pin[:n].view(wav.shape)
            if n and (n * 4) % 16 == 0:
                _lib.check(self.lib.ctts_copy_bytes(view.data_ptr(), wav.data_ptr(), n * 4, self._side.cuda_stream), "ctts_copy_bytes")
            elif n:
                view.copy_(wav, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
            for r in result_list:
                r.record_stream(self._side)
            wav.record_stream(self._side)
        return PendingWavs(self, view, done, wav)

    def _to_host_piped(self, t: torch.Tensor, view: torch.Tensor, nbytes: int, pieces: int = 4) -> np.ndarray:
        st = torch.cuda.current_stream(self.device)
        per = (nbytes // pieces + 63) // 64 * 64
        cuts = [(o, min(per, nbytes - o)) for o in range(0, nbytes, per)]
        evs = []
        for off, ln in cuts:
            _lib.check(self.lib.ctts_copy_bytes(view.data_ptr() + off, t.data_ptr() + off, ln, st.cuda_stream), "ctts_copy_bytes")
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        src = view.numpy()
        out = np.empty(src.shape, dtype=src.dtype)
        fs, fo = src.reshape(-1).view(np.uint8), out.reshape(-1).view(np.uint8)
        pool = getattr(self, "_copy_pool", None)
        if pool is None:
            from concurrent.futures import ThreadPoolExecutor
            pool = self._copy_pool = ThreadPoolExecutor(max_workers=4)
        for (off, ln), ev in zip(cuts, evs):
            wait_event(ev)
            q = (ln // 4 + 63) // 64 * 64
            list(pool.map(lambda a: np.copyto(fo[off + a: off + min(a + q, ln)], fs[off + a: off + min(a + q, ln)]), range(0, ln, q)))
        return out

    def _copy_out(self, view: torch.Tensor) -> np.ndarray:
        """pinned staging view -> fresh numpy array by plain memcpy (see to_host)"""
        src = view.numpy()
        out = np.empty(src.shape, dtype=src.dtype)
        flat_s, flat_o = src.reshape(-1), out.reshape(-1)
        if flat_s.nbytes < (8 << 20):
            np.copyto(flat_o, flat_s)
        else:
            pool = getattr(self, "_copy_pool", None)
            if pool is None:
                from concurrent.futures import ThreadPoolExecutor
                pool = self._copy_pool = ThreadPoolExecutor(max_workers=4)
            step = (flat_s.size + 3) // 4
            list(pool.map(lambda i: np.copyto(flat_o[i * step: (i + 1) * step], flat_s[i * step: (i + 1) * step]), range(4)))
        return out

    def decode_to_wavs(self, result_list: List[torch.Tensor], pad_to: Optional[int] = None, sample_rate: Optional[int] = None,
                       speed: Optional[float] = None, loudness=None, pauses=None, limiter=None, compress=None, eq=None) -> torch.Tensor:
        """`Chat._decode_to_wavs` (core.py:513-539): zero-pad the per-row [T_b,768] hidden lists to the
        longest row, DVAE decode, Vocos decode -> [B, 256(2Tmax-1)] float32 on the device.  `pad_to`: pad to that many tokens instead
        (>= the longest row): a data-parallel shard decodes its rows as part of the GLOBAL batch (dist.infer_sharded) -- the reference
        decodes a shorter row's tail from zero hidden states and returns it.  `sample_rate` (None: 24000): the rows are resampled to
        that rate on the device, directly behind the ISTFT (`resample`) -> [B, ceil(n * new / 24000)].  `speed` (None: 1.0): the rows
        are time-scaled at 24 kHz (`time_scale`), each alone, behind the ISTFT and in front of the resampler.  `loudness` (None:
        untouched): a target in LUFS, one value or one per row (None entries left alone) -- every row, padding and all, is normalised
        alone (`loudness_normalize`) at the returned rate, the last float32 stage.  `pauses` (None: untouched): a pause spec, one or
        a list with one per row (None entries copied through) -- every row, padding and all, is trimmed alone (`trim_pauses`) at the
        returned rate, behind the resampler and in front of the loudness stage, and the result is then (packed, offsets) instead of
        [B, n]: the rows' lengths differ.  `limiter` (None: off; one bool, or one per row): a flagged row, padding and all, goes
        through the look-ahead peak limiter (`peak_limit`) behind the loudness stage's gain, which then drops its ceiling term
        (`loudness_normalize(limiter=)`); without `loudness` at unity gain.  `compress` (None: off): a compressor spec, one or a
        list with one per row (None entries copied through) -- every row, padding and all, is compressed alone (`compress`) at the
        returned rate, behind `pauses` and in front of the loudness stage.  `eq` (None: off): an equaliser spec, one or a list with
        one per row (None entries copied through) -- every row, padding and all, is filtered alone from zero state (`equalize`) at the
        returned rate, behind `pauses` and in front of `compress`."""
        if len(result_list) == 0:
            return torch.empty((0,), dtype=torch.float32)
        plan = OC.Plan.batch("decode_to_wavs", len(result_list), sample_rate, speed, loudness, pauses, limiter, compress, eq)   # every refusal, before the decode
        if plan.on:
            return OC.run(self, self.decode_to_wavs(result_list, pad_to), plan, in_place=True)   # the plain decode, through the public method
        longest = max(int(r.size(0)) for r in result_list)
        if pad_to is not None and int(pad_to) < longest:
            raise ValueError("pad_to is shorter than the longest row")
        pad = getattr(result_list, "padded", None)
        if (pad is not None and pad.dim() == 3 and pad.shape[0] == len(result_list) and pad.shape[2] == GPT.hidden and pad.device == self.device
                and pad.dtype == torch.float32 and pad.shape[1] == longest and (pad_to is None or int(pad_to) == longest)):
            return self.vocos_decode(self.dvae_decode(pad))      # GptEngine.generate's rows: views of exactly this batch (RowList)
        Tmax = longest if pad_to is None else int(pad_to)
        batch = torch.zeros((len(result_list), Tmax, GPT.hidden), dtype=torch.float32, device=self.device)
        for i, r in enumerate(result_list):
            batch[i, : r.size(0)] = r
        return self.vocos_decode(self.dvae_decode(batch))

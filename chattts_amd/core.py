"""`Chat`-level seam of the hot path: mirror of `Chat.infer` / `_infer` / `_infer_code` / `_refine_text` /
`_decode_to_wavs` (/root/reference/ChatTTS/core.py:208-270, 395-503, 513-751).

Two entry levels:
  * text level  -- `Chat.infer(text, ...)` with the reference's argument list.  Needs a tokenizer directory
    (`asset/tokenizer`, config.py:10) and, for speaker sampling, the `Config.spk_stat` string (config.py:132); the host
    front end lives in `chattts_amd.frontend`.
  * token level -- `infer_code` / `refine_text_ids` / `infer_ids` / `infer_ids_stream` / `infer_tokens` start where
    `_infer_code` has tensors: `input_ids [B,T,4]`, `attention_mask [B,T]`, `text_mask [B,T]` exactly as
    `Tokenizer.encode` returns them (tokenizer.py:36-126).  bench.py and the parity tests use this level (synthetic
    prompts; the trained tokenizer is not reachable offline).
INTEGRATION.md shows the ~10-line patch that routes the reference's own `Chat` through the engine instead.
"""
from __future__ import annotations

import logging
import os
import re
from dataclasses import dataclass
from typing import Iterator, List, Optional, Union

import numpy as np
import torch

from . import adpcm as ADPCM
from . import compressor as CP
from . import equalizer as EQ
from . import flac as FLAC
from . import g711 as G711
from . import limiter as LM
from . import loudness as LN
from . import outchain
from . import pauses as PA
from . import resample as RS
from . import weights as W
from . import winchain as WC
from .audio import float_to_int16
from .config import GPT
from .dvae import DvaeEngine
from .engine import CodecEngine, Context, GenerationOutputs, GptEngine, gen_logits, keep_offsets, ragged_views
from .frontend import Normalizer, Speaker, Tokenizer, apply_speaker
from .outchain import Plan


@dataclass(repr=False, eq=False)
class RefineTextParams:           # core.py:182-193
    prompt: str = ""
    top_P: float = 0.7
    top_K: int = 20
    temperature: float = 0.7
    repetition_penalty: float = 1.0
    max_new_token: int = 384
    min_new_token: int = 0
    show_tqdm: bool = True
    ensure_non_empty: bool = True
    manual_seed: Optional[int] = None


@dataclass(repr=False, eq=False)
class InferCodeParams:            # core.py:195-206 (+ the RefineTextParams fields it inherits, :182-193)
    prompt: str = "[speed_5]"
    top_P: float = 0.7
    top_K: int = 20
    temperature: float = 0.3
    repetition_penalty: float = 1.05
    max_new_token: int = 2048
    min_new_token: int = 0
    show_tqdm: bool = True
    ensure_non_empty: bool = True
    manual_seed: Optional[int] = None
    spk_emb: Optional[str] = None
    spk_smp: Optional[str] = None
    txt_smp: Optional[str] = None
    stream_batch: int = 24
    stream_speed: int = 12000
    pass_first_n_batches: int = 2


def split_sentences(text: str) -> List[str]:
    """how `Chat.infer(text: str, split_text=True)` cuts its input (core.py:225-233): at newlines when there are any, else after every CJK
    full stop and after every ". ".  `Chat.infer` and the batched server (serving.SpeechBatcher.submit(split_text=True)) both cut here."""
    if "\n" in text:
        return text.split("\n")
    return [t for t in re.split(r"(?<=\u3002)|(?<=\.\s)", text) if t]     # sentence ends: after a CJK full stop, or after ". "


class Chat:
    RefineTextParams = RefineTextParams      # the reference nests the two dataclasses in `Chat` (core.py:182-206)
    InferCodeParams = InferCodeParams

    def __init__(self, logger=logging.getLogger("chattts_amd"), homophones_map: Optional[str] = None):
        """`homophones_map`: path of the reference package's `res/homophones_map.json` (core.py:39-42); without it the
        normalizer skips homophone replacement."""
        self.logger = logger
        self.context = Context()
        self.gpt: Optional[GptEngine] = None
        self.codec: Optional[CodecEngine] = None
        self.dvae: Optional[DvaeEngine] = None
        self.tokenizer: Optional[Tokenizer] = None
        self.speaker: Optional[Speaker] = None
        self.normalizer = Normalizer(homophones_map, logger)
        self.incremental_stream = True   # stream=True decodes token windows with halos, not the whole prefix per yield

    def has_loaded(self, use_decoder: bool = True) -> bool:
        """core.py:50-66: the decoder path needs `Decoder.safetensors`, the `use_decoder=False` path the full DVAE"""
        return self.gpt is not None and self.codec is not None and (use_decoder or self.dvae is not None)

    def load(self, source: str = "local", force_redownload: bool = False, compile: bool = False, custom_path: Optional[str] = None,
             device: Optional[torch.device] = None, coef=None, use_flash_attn: bool = False, use_vllm: bool = False,
             experimental: bool = False, *, dtype: str = "bf16", state_dicts: Optional[dict] = None,
             tokenizer: Union[None, str, Tokenizer] = None, spk_stat: Optional[str] = None, codec_gemm: Optional[str] = None,
             warm=None) -> bool:
        """`Chat.load` with the reference's positional parameters and defaults (core.py:137-148), for `source="local"` /
        `"custom"` (assets already on disk; there is no network path here, `"huggingface"` returns False): the four
        hot-path safetensors files under `custom_path` (default: the working directory, like the reference's "local"
        source) and `asset/tokenizer`.  Keyword-only extras of this engine: `dtype` ("bf16" perf mode | "f32" parity mode on float32 arithmetic
        throughout | "f32x3" parity mode with split-fp16 Llama projections (float32-class, faster), every call reports its decision margins -- GptEngine),
        `state_dicts` short-circuits disk I/O (synthetic weights); `tokenizer` is a directory or a `Tokenizer`;
        `spk_stat` is the reference's `Config.spk_stat` string (needed by `sample_random_speaker` only); `codec_gemm` picks the
        acoustic decoder's dense-layer arithmetic (`CodecEngine`: "f16" | "bf16x3" | "f32"; default: "f16" in perf mode --
        waveform within 2e-5 RMS of the f32-class decoder for the same hidden states -- and "bf16x3" in parity mode).
        `warm=(B, T)` or `(B, T, InferCodeParams)`: pay the first request's cold start at load time instead (see `Chat.warm`).
        `compile`, `use_flash_attn`, `use_vllm`, `experimental` select between the reference's torch back ends and
        have no meaning for this engine (accepted, ignored).  `coef` is accepted and has no effect, as in the reference:
        `DVAE.__init__` installs it (dvae.py:219-226) and `load_pretrained` then overwrites the buffer with the
        checkpoint's `coef` tensor (dvae.py:254-259)."""
        if source not in ("custom", "local"):
            self.logger.error("chattts_amd loads local assets only (source=%s)", source)
            return False
        device = device or torch.device("cuda:0")
        root = custom_path if custom_path is not None else os.getcwd()
        try:
            sds = state_dicts if state_dicts is not None else W.load_assets(root)
        except W.AssetError as e:
            self.logger.error("%s", e)
            return False
        try:
            for name in W.ASSET_FILES:      # key set / shapes / dtypes against SURVEY App. B: a diff, not a KeyError in the repacking
                W.validate_state_dict(name, sds[name])
        except (W.AssetError, KeyError) as e:   # the reference's load logs and returns False (core.py:131-135,384)
            self.logger.error("%s", e)
            return False
        self.gpt = GptEngine(sds["gpt"], sds["embed"], device, dtype=dtype, logger=self.logger, **sds.get("gpt_config", {}))
        self.codec = CodecEngine(sds["decoder"], sds["vocos"], device, gemm=codec_gemm or ("f16" if dtype == "bf16" else "bf16x3"))
        self.dvae = DvaeEngine(sds["dvae"], device) if "dvae" in sds else None
        self.device = device
        if tokenizer is None and state_dicts is None and os.path.isdir(os.path.join(root, "asset", "tokenizer")):
            tokenizer = os.path.join(root, "asset", "tokenizer")
        if tokenizer is not None:
            self.tokenizer = tokenizer if isinstance(tokenizer, Tokenizer) else Tokenizer(tokenizer)
        if spk_stat is not None:
            self.speaker = Speaker(GPT.hidden, spk_stat, torch.device("cpu"))
        if warm is not None:
            self.warm(*warm)
        return True

    def warm(self, batch: int, prompt_len: int, params: Optional["Chat.InferCodeParams"] = None, stream: bool = True, **kw) -> float:
        """Pre-warm the engine for one geometry -- `batch` utterances, prompts padded to `prompt_len` tokens, the sampling constants
        and `max_new_token` of `params` (default: InferCodeParams()) -- so that the FIRST request of that shape finds what a second one
        would: the generation session (KV cache, token / hidden-state buffers: 2.3 GB at batch 64 x 2048 new tokens), the captured and
        instantiated decode graphs with their first replays behind them, the acoustic decoder's workspace and the pinned staging buffers
        (profiles/r4u_ttfs_probe.log: first audio of a fresh engine after 280 ms, 32-51 ms from the second call on).  Runs the real path
        on a synthetic prompt up to its first streamed chunk and interrupts it (core.py:272-273); a request of another shape still
        benefits from the allocator's cached blocks and the decoder's buffers (`kw`: the extra keywords the requests will pass to
        `infer_code`, e.g. a `stop_at` tensor -- the session is keyed on their presence).  The reference has no counterpart: its first call pays
        torch's lazy initialisation the same way (core.py:137-163 loads weights only).  Returns the seconds it took."""
        import time
        assert self.has_loaded()
        t0 = time.perf_counter()
        params = params or Chat.InferCodeParams(show_tqdm=False)
        ids = torch.ones((batch, prompt_len, GPT.n_vq), dtype=torch.int64)
        attn = torch.ones((batch, prompt_len), dtype=torch.bool)
        was = self.context.get()
        self.context.set(False)
        # an unseeded warm-up (manual_seed=None, the default) draws from torch's global CPU generator like any request: put the
        # generator back afterwards, so that a later unseeded request reproduces the reference's draws for a seed set before load().
        # stream=False: the generator is polled once per chunk of GptEngine.POLL steps, so the interrupt below stops it after the
        # first chunk, not after `max_new_token` steps.
        rng_state = torch.get_rng_state()
        try:
            n = 0
            for out in self.infer_code(ids, attn, torch.ones((batch, prompt_len), dtype=torch.bool), params, stream=stream, **kw):
                n += 1
                if out is not None and len(out.hiddens) and max(int(h.shape[0]) for h in out.hiddens) > 0 and self.codec is not None:
                    if stream:
                        self._stream_piece(out.hiddens, 0, params.stream_speed)      # window decode + staging buffers
                    else:
                        self.decode_to_wavs(out.hiddens)
                self.context.set(True)          # one chunk is enough: the generator stops at its next poll
        finally:
            self.context.set(was)
            torch.set_rng_state(rng_state)
        torch.cuda.synchronize(self.device)
        return time.perf_counter() - t0

    def unload(self):               # core.py:165-174
        self.gpt = None
        self.codec = None
        self.dvae = None
        self.tokenizer = None
        self.speaker = None

    # -- speakers (core.py:176-180) ---------------------------------------------------------------------------
    def sample_random_speaker(self) -> str:
        if self.speaker is None:
            raise RuntimeError("speaker statistics not loaded: pass spk_stat= to Chat.load")
        return self.speaker.sample_random()

    def sample_audio_speaker(self, wav, sample_rate: Optional[int] = None) -> str:
        """waveform -> `spk_smp` string: DVAE encode to [4,T] codes, packed like `Speaker.encode_prompt`.  `sample_rate`: the clip's rate;
        None or 24000: the clip is encoded as it is (the reference's callers resample with `load_audio(path, 24000)` first,
        examples/web/funcs.py:121-122); any other rate: the clip is uploaded and resampled to 24 kHz on the device
        (CodecEngine.resample) and goes to the encoder from there."""
        if self.dvae is None:
            raise RuntimeError("full DVAE not loaded (asset/DVAE.safetensors, or state_dicts['dvae'])")
        if sample_rate is not None and int(sample_rate) != CodecEngine.SAMPLE_RATE:
            if self.codec is None:
                raise RuntimeError("resampling a clip needs the acoustic decoder's engine (Chat.load)")
            if isinstance(wav, np.ndarray):
                wav = torch.from_numpy(np.ascontiguousarray(wav))
            wav = wav.reshape(-1).to(torch.float32).contiguous().to(self.codec.device)
            wav = self.codec.resample(wav, int(sample_rate), CodecEngine.SAMPLE_RATE)
        return Speaker.encode_prompt(self.dvae.sample_audio(wav))

    def refer_speaker(self, rows, use_decoder: bool = True, *, on_device: bool = False, release=None) -> str:
        """core.py:435-453: the refer sentence's result (its one row, decoded alone) -> the `spk_smp` prompt of the other sentences of a
        split_text call.  `release`: called once the rows have been decoded (`_infer` frees the generator's result there).
        `on_device` (the batched server's stage A, decoder path): the waveform goes from the decoder to the DVAE encoder without
        visiting the host -- the same samples, hence the same string."""
        if on_device:
            wavs = self.codec.decode_to_wavs(rows)
        else:
            wavs = self.decode_to_wavs(rows, use_decoder)
        if release is not None:
            release()
        return self.sample_audio_speaker(wavs[0])

    def interrupt(self):            # core.py:272-273
        self.context.set(True)

    def infer_code(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, text_mask: torch.Tensor,
                   params: InferCodeParams = InferCodeParams(), stream: bool = False, return_hidden: bool = True,
                   spk_emb_ids: Optional[int] = None, **shard_kw) -> Iterator[GenerationOutputs]:
        """`Chat._infer_code` from `gen_logits` on (core.py:580-658).  With `params.spk_emb` and `spk_emb_ids` (the
        tokenizer's id of `[spk_emb]`) the prompt embedding gets the speaker vector at those positions (:630-637)."""
        assert self.has_loaded()
        # core.py:558-561: a scalar temperature is replicated over the 4 codebooks, a list is used as is
        temperature = torch.tensor(params.temperature if isinstance(params.temperature, list) else [params.temperature] * GPT.n_vq)
        warpers, procs = gen_logits(GPT.n_audio - 1, params.top_P, params.top_K, params.repetition_penalty)
        emb = self.prompt_embedding(input_ids, text_mask, params, spk_emb_ids)
        return self.gpt.generate(
            emb, input_ids, temperature, GPT.n_audio - 1, attention_mask, params.max_new_token, params.min_new_token,
            (*procs, *warpers), False, False, return_hidden, stream, params.show_tqdm, params.ensure_non_empty,
            params.stream_batch, params.manual_seed, self.context, **shard_kw)

    def prompt_embedding(self, input_ids: torch.Tensor, text_mask: torch.Tensor, params: InferCodeParams,
                         spk_emb_ids: Optional[int] = None) -> torch.Tensor:
        """the prompt embedding of the code pass (core.py:616-637): Embed, then the speaker vector at the `[spk_emb]` positions"""
        emb = self.gpt.embed_prompt(input_ids, text_mask)
        if params.spk_emb is not None and spk_emb_ids is not None:
            apply_speaker(emb, params.spk_emb, input_ids, spk_emb_ids)
        return emb

    def code_prompt(self, text, params: InferCodeParams):
        """decorate (prompt, `txt_smp`, `spk_emb`) -> tokenise (+ audio-code prompt `spk_smp`) of ALREADY NORMALISED texts
        (core.py:589-606): (input_ids [B,T,4], attention_mask [B,T], text_mask [B,T]).  The code pass of `Chat.infer` and the batched
        server (serving.SpeechBatcher) both build their prompts here."""
        self._need_tokenizer()
        if not isinstance(text, list):
            text = [text]
        assert len(text), "text should not be empty"
        prompt = Speaker.decode_prompt(params.spk_smp) if params.spk_smp is not None else None
        return self.tokenizer.encode(Speaker.decorate_code_prompts(text, params.prompt, params.txt_smp, params.spk_emb), GPT.n_vq,
                                     prompt=prompt)

    def refine_text_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, text_mask: torch.Tensor, eos_token: int,
                        params: RefineTextParams = RefineTextParams(), num_code: int = GPT.n_text, **kw) -> GenerationOutputs:
        """`Chat._refine_text` from `gen_logits` on (core.py:682-751): the same generator in text mode
        (`infer_text=True`: text embedding, 21178-way text head, tokens replicated over the 4 slots); `eos_token`
        is `tokenizer.eos_token` ([Ebreak]).  Returns `GenerationOutputs` whose `ids[b]` is the 1-D refined token row."""
        assert self.has_loaded()
        warpers, procs = gen_logits(num_code, params.top_P, params.top_K, params.repetition_penalty)   # core.py:682-687: len(tokenizer)
        emb = self.gpt.embed_prompt(input_ids, text_mask)
        return next(self.gpt.generate(
            emb, input_ids, torch.tensor([params.temperature]), eos_token, attention_mask, params.max_new_token,
            params.min_new_token, (*procs, *warpers), True, False, False, False, params.show_tqdm, params.ensure_non_empty,
            24, params.manual_seed, self.context, **kw))

    def decode_to_wavs(self, result_list: List[torch.Tensor], use_decoder: bool = True, pad_to: Optional[int] = None, *,
                       ragged: bool = False, sample_rate=None, speed=None, loudness=None, pauses=None, limiter=None, compress=None,
                       eq=None):
        """`Chat._decode_to_wavs` (core.py:513-539) -> np.float32 [B, n]: per-row hidden states [T_b,768] through the
        decoder, or (use_decoder=False) per-row token ids [T_b,4] through the full DVAE's codebook; then Vocos.
        `pad_to`: decode as rows of a batch whose longest row has that many tokens (dist.infer_sharded).
        `ragged=True` (not the reference's batch semantics): every row decoded as if alone, in one pass (CodecEngine.decode_ragged)
        -> List[np.ndarray], row b's 256 (2 T_b - 1) samples; the decoder path only.
        `sample_rate` (None: 24000; with `ragged` also one per row): the waveforms are resampled on the device behind the ISTFT.
        `speed` (None: 1.0; with `ragged` also one per row): pitch-preserving time scaling on the device (CodecEngine.time_scale), at
        24 kHz, behind the ISTFT and in front of the resampler.
        `loudness` (None: untouched; a target in LUFS, -40 .. -5, also one per row, None entries left alone): every row is brought to
        that BS.1770 integrated loudness on the device (CodecEngine.loudness_normalize), under the +30 dB cap and the -1 dBFS ceiling:
        the last float32 stage, behind the time scaler and the resampler.
        `pauses` (None: untouched; True, a pauses.PauseSpec or a dict of its fields, also a list with one per row, None entries copied
        through): every row loses the silence at its edges and the middle of its long pauses on the device
        (CodecEngine.trim_pauses), behind the resampler and in front of the loudness stage.  The rows' lengths then differ: the
        result is a List[np.ndarray] also without `ragged`.
        `limiter` (None / False: off; True, also one flag per row): every flagged row goes through the look-ahead peak limiter on the
        device (CodecEngine.peak_limit; the definition of limiter.py) where the loudness stage is, behind its gain: that gain then
        drops the -1 dBFS ceiling term, and the limiter holds the ceiling sample by sample.  Without `loudness` it runs at unity
        gain.
        `compress` (None / False: off; True or a dict of compressor.RANGES' fields, also a list with one per row, None entries copied
        through): every row goes through the look-ahead compressor on the device (CodecEngine.compress; the definition of
        compressor.py), behind `pauses` and in front of the loudness stage.
        `eq` (None / False: off; an equaliser preset name or a dict of equalizer.FIELDS, also a list with one per row, None entries
        copied through): every row goes through the biquad cascade on the device (CodecEngine.equalize; the definition of
        equalizer.py) from zero state, behind `pauses` and in front of `compress`."""
        plan = Plan.given("decode_to_wavs", sample_rate, speed, loudness, pauses, limiter, one_rate=not ragged, compress=compress, eq=eq)
        if ragged and not use_decoder:
            raise NotImplementedError("ragged decoding covers the hidden-state decoder only (use_decoder=True)")
        assert self.has_loaded(use_decoder)
        if ragged and pad_to is not None:
            raise ValueError("ragged decoding decodes every row at its own length: pad_to does not apply")
        if len(result_list) == 0:
            return [] if ragged else np.array([], dtype=np.float32)
        wav, off = self._decode_float(result_list, use_decoder, ragged, pad_to, plan)
        host = self.codec.to_host(wav)
        return host if off is None else ragged_views(host, off)

    def _decode_float(self, result_list, use_decoder: bool, ragged: bool, pad_to, plan: Plan, own_chain: bool = False):
        """the front half of the decode calls: the rows through the acoustic decoder and the output chain of `plan` ("The
        output chain") -> (float32 device waveform, host offsets), offsets None for a [B, n] batch.  The engine's decode calls take
        the options and run the chain; Chat runs it (outchain.run) on the DVAE-codes path and, with `own_chain`, behind the plain
        zero-padded decode of decode_to_pcm16 (the last stage then writes a tensor of its own, not the decode's).  Rows that the
        pause stage trims leave either path as a pack."""
        codec = self.codec
        if ragged:
            return codec.decode_ragged(list(result_list), sample_rate=plan.sample_rate, **plan.kwargs())
        if use_decoder and (plan.pauses is not None or not own_chain):
            res = codec.decode_to_wavs(result_list, pad_to=pad_to, sample_rate=plan.sample_rate, **plan.kwargs())
        else:
            wav = codec.decode_to_wavs(result_list) if use_decoder else codec.vocos_decode(self.dvae.decode_codes(result_list, pad_to=pad_to))
            res = outchain.run(codec, wav, plan)
        return res if isinstance(res, tuple) else (res, None)

    def decode_to_pcm16(self, result_list: List[torch.Tensor], use_decoder: bool = True, strip: bool = True,
                        product: str = "f64", *, ragged: bool = False, sample_rate=None, encoding=None, speed=None,
                        flac=None, loudness=None, pauses=None, limiter=None, adpcm=None, compress=None, eq=None) -> List[np.ndarray]:
        """`_decode_to_wavs` followed by what the reference's callers do with every waveform -- the sample-level silence strip of
        core.py:262-265 and `float_to_int16` (tools/audio/np.py:7-11; examples/web/funcs.py:209, tools/audio/pcm.py:29), one peak per
        utterance -- with the conversion ON THE DEVICE: the batch crosses PCIe as int16 + one mask bit per sample instead of float32.
        Returns one int16 array per utterance, equal to `float_to_int16(wav[np.abs(wav) > 1e-5])` bit for bit (the strip only removes
        samples that are far below one count, so the peak -- hence the scale -- is that of the unstripped row).
        `sample_rate` (None: 24000; with `ragged` also one per row): `wav` above is the waveform resampled on the device directly
        behind the ISTFT; strip and conversion are the same kernels, fed the resampled samples.
        `encoding` (None: the call above; "ulaw" / "alaw"; with `ragged` also one per row): G.711 companding on the device, strictly
        behind the conversion (CodecEngine.g711_encode) -- row b comes back as uint8, `g711.encode` of the int16 array above.
        `speed` (None: 1.0; with `ragged` also one per row): `wav` above is the waveform time-scaled on the device
        (CodecEngine.time_scale) at 24 kHz, in front of the resampler; rows at speed 1 are not touched.
        `flac` (None / False: the call above; True; with `ragged` also one flag per row): a flagged row comes back as a uint8 array, the
        complete FLAC file (chattts_amd/flac.py) of exactly the int16 samples above at the row's rate, encoded on the device behind the
        conversion (CodecEngine.float_to_int16_groups_flac: the stripped length is known there only); not together with `encoding`.
        `loudness` (None: untouched; a target in LUFS, also one per row, None entries left alone): `wav` above is the waveform
        normalised on the device (CodecEngine.loudness_normalize) at the rate it is returned at -- behind the time scaler and the
        resampler, in front of the strip, the conversion, the companding and FLAC, so the -1 dBFS ceiling holds on exactly the samples
        that are converted.
        `pauses` (None: untouched; True, a pauses.PauseSpec or a dict of its fields, also a list with one per row, None entries copied
        through): `wav` above is the waveform with its edge silence trimmed and its long pauses capped on the device
        (CodecEngine.trim_pauses), every row alone -- behind the resampler, in front of the loudness stage and everything behind it.
        Without `ragged` the trimmed rows of the batch go on as a pack, through the ragged calls' conversion.
        `limiter` (None / False: off; True, also one flag per row): `wav` above is the waveform behind the look-ahead peak limiter
        (CodecEngine.peak_limit), which runs where the loudness stage is, at its gain without the ceiling term (unity without
        `loudness`): no sample that is converted exceeds -1 dBFS, and a peak above full scale is limited instead of clipped.
        `adpcm` (None / False: the call above; True; with `ragged` also one flag per row): a flagged row comes back as a uint8 array, the
        complete WAVE_FORMAT_IMA_ADPCM file (chattts_amd/adpcm.py: 4 bits per sample) of exactly the int16 samples above at the row's
        rate, encoded on the device behind the conversion (CodecEngine.float_to_int16_groups_adpcm); not together with `flac`, nor
        with an `encoding` on the same row.
        `compress` (None / False: off; True or a dict of compressor.RANGES' fields, also a list with one per row, None entries copied
        through): `wav` above is the waveform behind the look-ahead compressor (CodecEngine.compress), every row alone -- behind
        `pauses`, in front of the loudness stage and everything behind it.
        `eq` (None / False: off; an equaliser preset name or a dict of equalizer.FIELDS, also a list with one per row, None entries
        copied through): `wav` above is the waveform behind the equaliser (CodecEngine.equalize), every row alone from zero state --
        behind `pauses`, in front of `compress`, the loudness stage and everything behind it."""
        plan = Plan.given("decode_to_pcm16", sample_rate, speed, loudness, pauses, limiter, one_rate=not ragged, compress=compress, eq=eq)
        if ragged and not use_decoder:
            raise NotImplementedError("ragged decoding covers the hidden-state decoder only (use_decoder=True)")
        assert self.has_loaded(use_decoder)
        encs, flags = self._formats(encoding, flac, len(result_list), per_row=ragged, who="decode_to_pcm16")
        aflags = self._adpcm_flags(adpcm, len(result_list), encoding, flags, ragged, "decode_to_pcm16")
        if len(result_list) == 0:
            return []
        if aflags is not None:
            for r in plan.row_rates(len(result_list)):
                ADPCM.check_rate(r)
        wav, off = self._decode_float(result_list, use_decoder, ragged, None, plan, own_chain=True)
        if flags is not None or aflags is not None:
            return self._decode_to_flac(wav, off, plan.row_rates(len(result_list)), flags or aflags, strip, product, encs,
                                        **({} if aflags is None else {"adpcm": True}))
        if off is not None:
            return self._decode_to_pcm16_ragged(wav, off, strip, product, encs)
        encoding = None if encs is None else encs[0]
        pcm, keep = self.codec.float_to_int16(wav, per_row=True, product=product, keep_thr=1e-5 if strip else None)
        if encoding is not None:       # codes | keep masks in one buffer: one copy
            B, n = int(pcm.shape[0]), int(pcm.shape[1])
            nc, kb = (B * n + 15) // 16 * 16, (keep.numel() + 15) // 16 * 16 if strip else 0
            buf = torch.empty((nc + kb,), dtype=torch.uint8, device=pcm.device)
            self.codec.g711_encode(pcm.view(-1), [(0, B * n, encoding)], out=buf[:nc])
            if strip:
                buf[nc: nc + keep.numel()].copy_(keep.view(-1))
            host = self.codec.to_host(buf)
            codes = host[: B * n].reshape(B, n)
            if not strip:
                return [codes[b] for b in range(B)]
            keep_h = host[nc: nc + keep.numel()].reshape(B, -1)
            return [codes[b][np.unpackbits(keep_h[b])[:n].astype(bool)] for b in range(B)]
        pcm_h = self.codec.to_host(pcm)
        if not strip:
            return [pcm_h[b] for b in range(pcm_h.shape[0])]
        keep_h = self.codec.to_host(keep)
        n = pcm_h.shape[1]
        return [pcm_h[b][np.unpackbits(keep_h[b])[:n].astype(bool)] for b in range(pcm_h.shape[0])]

    @staticmethod
    def _flac_flags(flac, n: int, encoding, per_row: bool, who: str):
        """the `flac=` option of the decode calls -> one bool per row, or None when no row asks for it (today's call)"""
        if flac is None or flac is False:
            return None
        if isinstance(flac, (bool, np.bool_)):
            flags = [bool(flac)] * n
        else:
            if not per_row:
                raise ValueError(f"{who}: one flac flag for the whole call (one per row goes with ragged=True)")
            flags = [bool(f) for f in flac]
            if len(flags) != n:
                raise ValueError(f"{who}: one flac flag per row, or one for all")
        if not any(flags):
            return None
        encs = None if encoding is None else ([encoding] * n if isinstance(encoding, str) else list(encoding))
        if encs is not None and (len(encs) != n or any(f and e is not None for f, e in zip(flags, encs))):
            raise ValueError(f"{who}: flac does not go with an encoding (a FLAC file holds the 16-bit samples; one entry per row)")
        return flags

    @staticmethod
    def _adpcm_flags(adpcm, n: int, encoding, flac_flags, per_row: bool, who: str):
        """the `adpcm=` option of the decode calls -> one bool per row, or None when no row asks for it (today's call); `flac_flags`:
        what `_flac_flags` made of the same call's `flac=`"""
        if adpcm is None or adpcm is False:
            return None
        if isinstance(adpcm, (bool, np.bool_)):
            flags = [bool(adpcm)] * n
        else:
            if not per_row:
                raise ValueError(f"{who}: one adpcm flag for the whole call (one per row goes with ragged=True)")
            flags = [bool(f) for f in adpcm]
            if len(flags) != n:
                raise ValueError(f"{who}: one adpcm flag per row, or one for all")
        if not any(flags):
            return None
        if flac_flags is not None:
            raise ValueError(f"{who}: adpcm does not go with flac (a call hands out one kind of file)")
        encs = None if encoding is None else ([encoding] * n if isinstance(encoding, str) else list(encoding))
        if encs is not None and (len(encs) != n or any(f and e is not None for f, e in zip(flags, encs))):
            raise ValueError(f"{who}: adpcm does not go with an encoding (an ADPCM file is coded from the 16-bit samples; one entry per row)")
        return flags

    @staticmethod
    def _formats(encoding, flac, n: int, per_row: bool, who: str, unit: str = "row"):
        """the `encoding=` and `flac=` options of the 16-bit calls, once for every path and before the decode -> (encs, flags): one
        encoding per row, None unless a row is companded or some row is a FLAC file; one flac flag per row, None when none is set
        (`_flac_flags`, which also refuses a row that asks for both)"""
        flags = Chat._flac_flags(flac, n, encoding, per_row, who)
        if not per_row:
            G711.check_encoding(encoding)
        if encoding is None or n == 0:
            return None, flags
        encs = [encoding] * n if isinstance(encoding, str) else list(encoding)
        if flags is not None:
            return encs, flags
        if len(encs) != n:
            raise ValueError(f"{who}: one encoding per {unit}, or one for all")
        return (encs if any(G711.check_encoding(e) is not None for e in encs) else None), None

    def _decode_to_flac(self, wav, off, rates, flags, strip: bool, product: str, encs=None, grp=None, adpcm: bool = False) -> List[np.ndarray]:
        """a decoded waveform -- [B, n], or packed with `off` -- with at least one row (with `grp`: one request, its sentences) as a
        FLAC file at its entry of `rates`: the grouped conversion with one group per row (the same samples; slots that start on
        multiples of 8 and a count header on the device) and the encoder behind it.  `adpcm`: the flagged rows are IMA ADPCM WAV files
        instead (CodecEngine.float_to_int16_groups_adpcm, the same seam)"""
        if off is None:
            wav = wav.contiguous()
            off = np.arange(wav.shape[0] + 1, dtype=np.int64) * int(wav.shape[1])
            wav = wav.view(-1)
        grp = np.arange(len(flags) + 1, dtype=np.int32) if grp is None else grp
        convert = self.codec.float_to_int16_groups_adpcm if adpcm else self.codec.float_to_int16_groups_flac
        out = convert(wav, off, grp, [r if f else None for r, f in zip(rates, flags)], product=product, keep_thr=1e-5 if strip else None,
                      encodings=encs)
        return [p if p.dtype == np.uint8 else p.copy() for p in out]

    def _decode_to_pcm16_ragged(self, wav, off, strip: bool, product: str, encs=None) -> List[np.ndarray]:
        """the back half of decode_to_pcm16 for a pack (the ragged decode's rows, or the trimmed rows of a zero-padded batch): one
        peak per row, and the PCM + keep masks of the whole group cross PCIe in ONE copy (both live in one device buffer).  Row b's
        result equals `float_to_int16(w[np.abs(w) > 1e-5])` of its waveform w.  `encs` (one per row, None entries stay int16; None:
        no row is companded): the companded rows are converted by one launch behind the conversion, and the codes travel with the
        keep masks in the one copy (the PCM16 samples too when some row stays int16)."""
        codec = self.codec
        if encs is not None:
            return self._decode_to_g711_ragged(wav, off, strip, product, encs)
        n = wav.numel()
        kb = int(keep_offsets(off)[-1]) if strip else 0
        blob = torch.empty(((2 * n + kb + 15) // 16 * 16,), dtype=torch.uint8, device=wav.device)
        pcm_d = blob[: 2 * n].view(torch.int16)
        keep_d = blob[2 * n: 2 * n + kb] if strip else None
        _, _, keep_off = codec.float_to_int16_ragged(wav, off, product=product, keep_thr=1e-5 if strip else None, out=(pcm_d, keep_d))
        host = codec.to_host(blob)
        pcm_h = host[: 2 * n].view(np.int16)
        pieces = ragged_views(pcm_h, off)
        if not strip:
            return pieces
        keep_h = host[2 * n: 2 * n + kb]
        return [p[np.unpackbits(keep_h[keep_off[i]: keep_off[i + 1]])[: p.size].astype(bool)] for i, p in enumerate(pieces)]

    def _decode_to_g711_ragged(self, wav, off, strip: bool, product: str, encs) -> List[np.ndarray]:
        """`_decode_to_pcm16_ragged` with at least one companded row.  The device buffer is int16 samples | codes | keep masks; rows
        that share a law and follow each other make one range.  A range starts on a multiple of 8 elements: rows resampled to
        another rate sit at arbitrary offsets, so a call that mixes laws over such rows goes through the grouped conversion instead
        (one group per row: the same bytes, slots that start on multiples of 8)."""
        codec = self.codec
        runs = []                     # [first row, one past the last, encoding]
        for i, e in enumerate(encs):
            if runs and runs[-1][2] == e:
                runs[-1][1] = i + 1
            else:
                runs.append([i, i + 1, e])
        if any(int(off[a]) % 8 for a, _, e in runs if e is not None):
            grp = np.arange(len(encs) + 1, dtype=np.int32)
            blob, starts = codec.float_to_int16_groups(wav, off, grp, product=product, keep_thr=1e-5 if strip else None, encodings=encs)
            return [p.copy() for p in codec.unpack_groups(codec.to_host(blob), starts, encs)]
        n = wav.numel()
        kb = int(keep_offsets(off)[-1]) if strip else 0
        n2, nc = (2 * n + 15) // 16 * 16, (n + 15) // 16 * 16
        blob = torch.empty((n2 + nc + (kb + 15) // 16 * 16,), dtype=torch.uint8, device=wav.device)
        pcm_d = blob[: 2 * n].view(torch.int16)
        keep_d = blob[n2 + nc: n2 + nc + kb] if strip else None
        _, _, keep_off = codec.float_to_int16_ragged(wav, off, product=product, keep_thr=1e-5 if strip else None, out=(pcm_d, keep_d))
        codec.g711_encode(pcm_d, [(int(off[a]), int(off[b] - off[a]), e) for a, b, e in runs if e is not None], out=blob[n2: n2 + nc])
        base = n2 if all(e is not None for e in encs) else 0
        host = codec.to_host(blob[base:] if base else blob)
        codes = ragged_views(host[n2 - base: n2 - base + n], off)
        pieces = codes if base else [c if e is not None else p for c, p, e in zip(codes, ragged_views(host[: 2 * n].view(np.int16), off), encs)]
        if not strip:
            return pieces
        keep_h = host[n2 - base + nc: n2 - base + nc + kb]
        return [p[np.unpackbits(keep_h[keep_off[i]: keep_off[i + 1]])[: p.size].astype(bool)] for i, p in enumerate(pieces)]

    def decode_split_to_pcm16(self, groups, strip: bool = True, product: str = "f64", sample_rate=None, encoding=None,
                              speed=None, flac=None, loudness=None, pauses=None, limiter=None, adpcm=None, compress=None,
                              eq=None) -> List[np.ndarray]:
        """The end of `Chat.infer(..., split_text=True, pcm16=True)` for MANY requests at once: `groups[g]` = request g's per-sentence
        hidden states ([T, 768] each, in sentence order).  ONE ragged decode over all sentences of all requests (each as if alone), ONE
        grouped conversion (CodecEngine.float_to_int16_groups: one peak per request, silent samples dropped, the rest compacted on the
        device) and ONE device-to-host copy.  Request g's result equals
        `float_to_int16(np.concatenate([w[np.abs(w) > 1e-5] for w in its sentences' alone decodes]))` bit for bit.
        `sample_rate` (None: 24000; or one per request): every sentence is resampled alone, on the device, behind the ISTFT; the
        grouped conversion then works on offsets that are no multiples of 8.
        `encoding` (None: the call above; "ulaw" / "alaw"; or one per request, None entries stay int16): the companded requests come
        back as uint8, `g711.encode` of the int16 array above (CodecEngine.float_to_int16_groups(encodings=): one launch behind the
        grouped conversion, still one copy).
        `speed` (None: 1.0; or one per request): every sentence is time-scaled alone, on the device, at 24 kHz -- in front of the
        resampler, hence in front of the group's strip and concatenation.
        `flac` (None / False: the call above; True; or one flag per request): a flagged request comes back as a uint8 array, the
        complete FLAC file of exactly the int16 samples above at the request's rate, encoded on the device straight from the grouped
        slots and their count header (CodecEngine.float_to_int16_groups_flac); not together with `encoding`.
        `loudness` (None: untouched; a target in LUFS, or one per request, None entries left alone): a request gets ONE loudness and
        ONE gain over its sentences (CodecEngine.loudness_normalize with the group table of the conversion behind it): every sentence
        is filtered alone, the gates run over all of the request's blocks, the peak is the request's.
        `pauses` (None: untouched; a pause spec, or a list with one per request, None entries copied through): every SENTENCE is
        trimmed alone (CodecEngine.trim_pauses) behind the resampler, so the gap at a join is at most tail + lead; the request's one
        gain is then computed over its trimmed sentences.
        `limiter` (None / False: off; True, or one flag per request): a flagged request's ONE gain drops the ceiling term and the
        look-ahead peak limiter (CodecEngine.peak_limit) runs behind it over every sentence alone: its windows never span two
        sentences.  Without `loudness` it runs at unity gain.
        `adpcm` (None / False: the call above; True; or one flag per request): a flagged request comes back as a uint8 array, ONE
        WAVE_FORMAT_IMA_ADPCM file over its concatenated sentences at the request's rate (CodecEngine.float_to_int16_groups_adpcm);
        not together with `flac`, nor with an `encoding` on the same request.
        `compress` (None / False: off; a compressor spec, or a list with one per request, None entries copied through): every
        SENTENCE is compressed alone (CodecEngine.compress) behind `pauses`: no window spans a join; the request's one gain is then
        computed over its compressed sentences.
        `eq` (None / False: off; an equaliser spec, or a list with one per request, None entries copied through): every SENTENCE is
        filtered alone from zero state (CodecEngine.equalize) behind `pauses` and in front of `compress`: no filter state crosses a
        join."""
        assert self.has_loaded()
        groups = [list(g) for g in groups]
        if len(groups) == 0:
            return []
        if any(len(g) == 0 for g in groups):
            raise ValueError("decode_split_to_pcm16: every request needs at least one sentence")
        grp = np.zeros(len(groups) + 1, np.int32)
        np.cumsum([len(g) for g in groups], out=grp[1:])
        codec = self.codec
        encs, flags = self._formats(encoding, flac, len(groups), per_row=True, who="decode_split_to_pcm16", unit="request")
        aflags = self._adpcm_flags(adpcm, len(groups), encoding, flags, True, "decode_split_to_pcm16")
        plan = Plan.given("decode_split_to_pcm16", sample_rate, speed, loudness, pauses, limiter, compress=compress, eq=eq)
        rates = plan.row_rates(len(groups))
        if aflags is not None:
            for r in rates:
                ADPCM.check_rate(r)
        plan = plan.per_sentence(groups)
        rows = [h for g in groups for h in g]
        wav, off = codec.decode_ragged(rows, sample_rate=plan.sample_rate, **plan.kwargs("speed", "pauses", "compress", "eq"))
        if plan.levels:                                               # ONE gain per request: the stage runs here, over the group table
            wav = codec.loudness_normalize(wav, plan.loudness, offsets=off, groups=grp, out=wav, rates=plan.row_rates(len(rows)),
                                           **plan.kwargs("limiter"))
        if flags is not None or aflags is not None:
            return self._decode_to_flac(wav, off, rates, flags or aflags, strip, product, encs, grp=grp, **({} if aflags is None else {"adpcm": True}))
        blob, starts = codec.float_to_int16_groups(wav, off, grp, product=product, keep_thr=1e-5 if strip else None,
                                                   **({} if encs is None else {"encodings": encs}))
        return [p.copy() for p in codec.unpack_groups(codec.to_host(blob), starts, *(() if encs is None else (encs,)))]

    def decode_windows_pcm16(self, store: torch.Tensor, windows, sample_rates=None, encodings=None, speeds=None, ts_streams=None,
                             rs_streams=None, flac=None, flac_streams=None, limiter=None, lm_streams=None, pauses=None,
                             pa_streams=None, adpcm=None, adpcm_streams=None, compress=None, cp_streams=None) -> List[np.ndarray]:
        """the chunks of many pooled streams that are due together, as the serial streamed path (`_infer`, stream, pcm16) hands them
        out one by one: (slot, prefix tokens, s_lo, s_hi, is_tail) -> int16 pieces, a tail with its silent samples removed
        (CodecEngine.decode_windows; serving.SpeechBatcher.submit_stream).  `encodings`: one per window, None / "ulaw" / "alaw" -- a
        companded window's piece is uint8, `g711.encode` of the int16 piece.  `speeds` with `ts_streams` (one entry per window; a
        speed other than 1 with the handle of its stream of the time scaler): the window's samples are pushed into that stream and
        the piece is what the step emits, converted (CodecEngine.decode_windows(speeds=)); `rs_streams` (with `speeds` and
        `sample_rates`): the handle of the resampler's stream of a window at another speed AND rate, None otherwise.  `flac` with
        `flac_streams` (one flag and one entry per window; a flagged window with the handle of its FLAC stream): the window's int16
        samples are pushed into that stream and the piece is uint8, the frames the push completes
        (CodecEngine.decode_windows(flac=)); `limiter` with `lm_streams` (one flag and one entry per window; a flagged window with the
        handle of its limiter stream): the window's float samples are pushed into that stream and the piece is what the step emits,
        converted (CodecEngine.decode_windows(limiter=)); `adpcm` with `adpcm_streams`: as `flac` / `flac_streams`, with the handle of
        the window's IMA ADPCM stream -- the piece is the blocks the push completes (CodecEngine.decode_windows(adpcm=)); without
        them today's call, argument for argument"""
        given = dict(sample_rates=sample_rates, encodings=encodings, speeds=speeds, ts_streams=ts_streams, rs_streams=rs_streams, flac=flac,
                     flac_streams=flac_streams, limiter=limiter, lm_streams=lm_streams, pauses=pauses, pa_streams=pa_streams, adpcm=adpcm,
                     adpcm_streams=adpcm_streams, compress=compress, cp_streams=cp_streams)
        kw = {k: given[k] for k in ("sample_rates", "encodings", "speeds") if given[k] is not None}
        for st in WC.STAGES:            # a stage whose flag is given: its flag and its streams (the resampler's only when given too)
            if given[st.flag] is not None and not (st.optional and given[st.streams] is None):
                kw[st.flag], kw[st.streams] = given[st.flag], given[st.streams]
        return self.codec.decode_windows(store, windows, pcm16=True, keep_thr=1e-5, **kw)

    def infer_ids(self, input_ids, attention_mask, text_mask, params: InferCodeParams = InferCodeParams(), **kw) -> np.ndarray:
        """non-stream `Chat._infer` body for one batch (core.py:469-481, split_text=False, skip_refine_text=True),
        BEFORE the sample-level silence strip of core.py:258-270."""
        last = None
        for last in self.infer_code(input_ids, attention_mask, text_mask, params, stream=False, **kw):
            pass
        if last is None:
            return np.zeros((0,), np.float32)
        return self.decode_to_wavs(last.hiddens)

    def infer_ids_pipelined(self, batches, params: InferCodeParams = InferCodeParams(), **kw) -> Iterator[np.ndarray]:
        """`infer_ids` over a QUEUE of batches (an iterable of `(input_ids, attention_mask, text_mask)` or of
        `(input_ids, attention_mask, text_mask, kwargs)`), software-pipelined: the acoustic decode + host copy of batch i run on the
        codec engine's side stream while batch i+1 is being generated (`CodecEngine.decode_to_wavs_async`).  Yields one
        np.float32 [B_i, n_i] array per batch, in order, each identical to `infer_ids` of that batch; a batch's result is yielded
        once the NEXT batch's generation has been issued and finished, the last one at the end."""
        pending = []        # results not yet handed out, oldest first: a PendingWavs, or None for a batch that produced nothing
        for item in batches:
            a, extra = (item[:3], item[3]) if len(item) == 4 else (item, {})
            last = None
            for last in self.infer_code(*a, params, stream=False, **{**kw, **extra}):
                pass
            pending.append(None if last is None else self.codec.decode_to_wavs_async(last.hiddens))
            while len(pending) > 1:     # exactly ONE item per input batch, in order, also for batches that yielded no output
                p = pending.pop(0)
                yield np.zeros((0,), np.float32) if p is None else p.result()
        for p in pending:
            yield np.zeros((0,), np.float32) if p is None else p.result()

    def _stream_piece(self, hiddens, a: int, b: Optional[int], use_decoder: bool = True, pcm16: bool = False,
                      rate: Optional[int] = None, encoding=None, on_device: bool = False, lm_handles=None, final: bool = False) -> np.ndarray:
        """samples [a, b) (b=None: to the end) of the decode of the current prefix (core.py:482-497), from a token window with
        halos instead of the whole prefix (`CodecEngine.decode_window`); `incremental_stream=False` restores the reference's
        full re-decode per yield.  `rate` (None: 24 kHz): [a, b) stay 24 kHz samples and the piece is outputs
        [ceil(a L / M), ceil(b L / M)) of the prefix's decode resampled as one signal -- from the widened window
        (`decode_window(sample_rate=)`), or, `incremental_stream=False`, sliced out of the whole prefix resampled whole.
        `encoding` ("ulaw" / "alaw", with `pcm16`): the int16 piece companded -- on the device where the conversion ran there, by the
        host twin where it ran on the host.  `on_device` (with `pcm16`, without `encoding`): a piece that was converted on the device
        stays there, as an int16 tensor (a streamed FLAC pushes it on).  `lm_handles` (one limiter stream per row, at the piece's
        rate; the decoder path): the float samples are PUSHED into the rows' streams (CodecEngine.peak_limit_stream_step, all rows in
        one launch) and the piece is what the step emits -- the conversion and the companding act on the limited samples; `final`:
        the streams' last push, which comes back as float32 whatever `pcm16` says (the caller filters its columns first)."""
        if lm_handles:
            Tn = max(int(r.size(0)) for r in hiddens)
            total = max(0, 256 * (2 * Tn - 1))
            hi = total if b is None else min(b, total)
            rkw = {} if rate is None else {"sample_rate": rate}
            if hi > a and self.incremental_stream:
                x = self.codec.decode_window(hiddens, a, hi, **rkw).contiguous()
            elif hi > a:        # decoded whole on the host path: the piece goes back to the device for the limiter
                x = torch.from_numpy(np.ascontiguousarray(self._stream_piece(hiddens, a, b, True, False, **({} if rate is None else {"rate": rate})),
                                                          dtype=np.float32)).to(self.device)
            else:               # nothing new: the streams are stepped all the same (the last push brings what they held)
                x = torch.empty((len(hiddens), 0), dtype=torch.float32, device=self.device)
            m = int(x.shape[1])
            y, off = self.codec.peak_limit_stream_step(x.view(-1), [(h, i * m, m, final) for i, h in enumerate(lm_handles)])
            return self._finish_piece(y.view(len(hiddens), int(off[1])), final, pcm16, encoding, on_device)
        if encoding is not None:
            if not pcm16:
                raise ValueError("encoding needs pcm16=True")
            Tn = max(int(r.size(0)) for r in hiddens)
            hi = 256 * (2 * Tn - 1) if b is None else min(b, 256 * (2 * Tn - 1))
            if use_decoder and self.incremental_stream and hi > a:
                win = self.codec.decode_window(hiddens, a, hi) if rate is None else self.codec.decode_window(hiddens, a, hi, sample_rate=rate)
                if win.shape[1] > 0:
                    pcm = self.codec.float_to_int16(win, per_row=True)[0]
                    codes = self.codec.g711_encode(pcm.view(-1), [(0, pcm.numel(), encoding)])
                    return self.codec.to_host(codes)[: pcm.numel()].reshape(tuple(pcm.shape))
            piece = self._stream_piece(hiddens, a, b, use_decoder, pcm16, **({} if rate is None else {"rate": rate}))
            return G711.encode(piece, encoding) if piece.dtype == np.int16 else piece.astype(np.uint8)
        Tn = max(int(r.size(0)) for r in hiddens)
        total = 256 * (2 * Tn - 1) if use_decoder else None
        if not use_decoder or not self.incremental_stream:
            if rate is not None:
                n24 = max(0, 256 * (2 * Tn - 1))      # the decode's width at 24 kHz, on both decode paths
                L, M = RS.ratio(CodecEngine.SAMPLE_RATE, rate)
                o_lo, o_hi = (RS.out_len(min(v, n24), L, M) for v in (a, n24 if b is None else b))
                piece = self.decode_to_wavs(hiddens, use_decoder, sample_rate=rate)[:, o_lo: max(o_lo, o_hi)]
                return np.stack([float_to_int16(r) for r in piece]) if (pcm16 and piece.shape[1]) else piece
            wavs = self.decode_to_wavs(hiddens, use_decoder)
            piece = wavs[:, a: wavs.shape[1] if b is None else min(b, wavs.shape[1])]
            return np.stack([float_to_int16(r) for r in piece]) if (pcm16 and piece.shape[1]) else piece
        hi = total if b is None else min(b, total)
        if hi <= a:     # a window that starts past the end of this prefix (a later split batch, see `_infer`): nothing to decode
            return np.zeros((len(hiddens), 0), np.int16 if pcm16 else np.float32)
        win = self.codec.decode_window(hiddens, a, hi) if rate is None else self.codec.decode_window(hiddens, a, hi, sample_rate=rate)
        if pcm16 and win.shape[1] > 0:     # every row by its own peak -- float_to_int16(chunk[b]), examples/web/funcs.py:203-206 -- on the device
            pcm = self.codec.float_to_int16(win, per_row=True)[0]
            return pcm if on_device else self.codec.to_host(pcm)
        return self.codec.to_host(win)

    def _stream_piece_scaled(self, hiddens, a: int, b: Optional[int], handles, final: bool, pcm16: bool = False, encoding=None,
                             rs_handles=None, on_device: bool = False, lm_handles=None) -> np.ndarray:
        """`_stream_piece` at another speed: samples [a, b) of the decode of the current prefix are PUSHED into the rows' streams of the
        time scaler (`handles`, one per row; CodecEngine.time_scale_stream_step, all rows in one launch) and the piece is what the step
        emits -- [B, 512 k] samples, possibly none; every row has had the same number of samples, so the chunk stays rectangular.
        `final`: the last push (the stream's tail); it comes back as float32 whatever `pcm16` says: the caller filters its columns
        first.  Otherwise `pcm16` converts every row under its own peak on the device, `encoding` compands behind that.
        `rs_handles` (one resampler stream per row, 24000 -> the request's rate): what the scaler's step emits is pushed on into them
        (CodecEngine.resample_stream_step, all rows in one launch) and the piece is what THAT step emits.  `lm_handles` (one limiter
        stream per row, at the piece's rate): the last float stage's chunk is pushed on into them in the same way."""
        codec = self.codec
        Tn = max(int(r.size(0)) for r in hiddens)
        total = max(0, 256 * (2 * Tn - 1))
        hi = total if b is None else min(b, total)
        B, m = len(hiddens), max(0, hi - a)
        if m > 0 and self.incremental_stream:
            x = codec.decode_window(hiddens, a, hi).contiguous().view(-1)
        elif m > 0:
            x = torch.from_numpy(np.ascontiguousarray(self.decode_to_wavs(hiddens)[:, a: hi], dtype=np.float32)).to(self.device).view(-1)
        else:
            x = torch.empty((0,), dtype=torch.float32, device=self.device)
        y, off = codec.time_scale_stream_step(x, [(h, i * m, m, final) for i, h in enumerate(handles)])
        if rs_handles:
            y, off = codec.resample_stream_step(y, [(h, int(off[i]), int(off[i + 1] - off[i]), final) for i, h in enumerate(rs_handles)])
        if lm_handles:
            y, off = codec.peak_limit_stream_step(y, [(h, int(off[i]), int(off[i + 1] - off[i]), final) for i, h in enumerate(lm_handles)])
        return self._finish_piece(y.view(B, int(off[1])), final, pcm16, encoding, on_device)

    def _stream_rows_paused(self, hiddens, a: int, b: Optional[int], final: bool, pa_handles, rate: Optional[int] = None, ts_handles=None,
                            rs_handles=None, lm_handles=None, pcm16: bool = False, encoding=None, fs_handles=None, fs_step=None,
                            cp_handles=None) -> list:
        """One chunk of a PAUSED or COMPRESSED stream (Chat.infer's `stream_pauses`, `stream_compress`; `pa_handles` None: not paused;
        `cp_handles`: the rows' compressor streams, stepped behind the pause streams and in front of the limiter's,
        CodecEngine.compress_stream_step): samples [a, b) of the decode of the current prefix go through
        the rows' float stages as in `_stream_piece` / `_stream_piece_scaled` (the resampled window at `rate`, or the time scaler's
        streams `ts_handles` and behind them the resampler's `rs_handles`), then into the rows' pause streams `pa_handles`
        (CodecEngine.trim_pauses_stream_step, all rows in one step) -- the one-shot chain's order: behind the last float stage, in front
        of the limiter streams `lm_handles`, the 16-bit conversion (one peak per row over the samples that come out), G.711 and the
        FLAC streams `fs_handles` (`fs_step`: another format's step in place of `flac_stream_step`, the ADPCM streams').  The rows emit different numbers of samples, so the chunk is a list with one array per row,
        possibly empty.  `final`: the streams' last push; every row's own samples with |x| <= 1e-5 are removed (the reference's tail
        filter, core.py:500-503, read for one row) and the rest is converted on the host, as a limited stream's last chunk is."""
        codec, B = self.codec, len(hiddens)
        Tn = max(int(r.size(0)) for r in hiddens)
        total = max(0, 256 * (2 * Tn - 1))
        hi = total if b is None else min(b, total)
        m = max(0, hi - a)
        rkw = {} if rate is None or ts_handles is not None else {"sample_rate": rate}
        if m > 0 and self.incremental_stream:
            x = codec.decode_window(hiddens, a, hi, **rkw).contiguous()
        elif m > 0:            # decoded whole on the host path: the piece goes back to the device for the streams
            skw = {} if not rkw else {"rate": rate}
            x = torch.from_numpy(np.ascontiguousarray(self._stream_piece(hiddens, a, b, True, False, **skw), dtype=np.float32)).to(self.device)
        else:
            x = torch.empty((B, 0), dtype=torch.float32, device=self.device)
        w = int(x.shape[1])
        y, off = x.view(-1), np.arange(B + 1, dtype=np.int64) * w
        step = lambda fn, hs: fn(y, [(h, int(off[i]), int(off[i + 1] - off[i]), final) for i, h in enumerate(hs)])
        if ts_handles is not None:
            y, off = step(codec.time_scale_stream_step, ts_handles)
            if rs_handles:
                y, off = step(codec.resample_stream_step, rs_handles)
        if pa_handles:
            y, off = step(codec.trim_pauses_stream_step, pa_handles)
        if cp_handles:
            y, off = step(codec.compress_stream_step, cp_handles)
        if lm_handles:
            y, off = step(codec.peak_limit_stream_step, lm_handles)
        off = np.asarray(off, dtype=np.int64)
        n = np.diff(off)
        if final or not pcm16:
            host = codec.to_host(y.contiguous())
            rows = [host[off[i]: off[i + 1]] for i in range(B)]
            if not final:
                return rows
            rows = [r[np.abs(r) > 1e-5] for r in rows]
            if not pcm16:
                return rows
            rows = [float_to_int16(r) if r.size else r.astype(np.int16) for r in rows]
            if encoding is not None:
                return [G711.encode(r, encoding) for r in rows]
            if fs_handles is None:
                return rows
            pcm = torch.from_numpy(np.concatenate(rows) if int(sum(r.size for r in rows)) else np.zeros(0, np.int16)).to(self.device)
            n = np.array([r.size for r in rows], dtype=np.int64)
            off = np.concatenate([[0], np.cumsum(n)])
        elif int(off[-1]) == 0:
            pcm = torch.zeros((0,), dtype=torch.int16, device=self.device)
        else:                  # every row under its own peak, on the device; empty rows are no segments
            seg = np.concatenate([[0], off[1:][n > 0]])
            pcm = codec.float_to_int16_ragged(y.contiguous(), seg)[0]
        if fs_handles is not None:      # every row's push starts on a multiple of 8 samples
            start = np.concatenate([[0], np.cumsum((n + 7) // 8 * 8)])
            buf = torch.zeros((max(8, int(start[-1])),), dtype=torch.int16, device=self.device)
            for i in range(B):
                if n[i]:
                    buf[int(start[i]): int(start[i]) + int(n[i])] = pcm[int(off[i]): int(off[i + 1])]
            return (fs_step or codec.flac_stream_step)(buf, [(h, int(start[i]), int(n[i]), final) for i, h in enumerate(fs_handles)])
        host = codec.to_host(pcm)
        rows = [host[off[i]: off[i + 1]] for i in range(B)]
        return rows if encoding is None else [G711.encode(r, encoding) if r.size else r.astype(np.uint8) for r in rows]

    def _finish_piece(self, y: torch.Tensor, final: bool, pcm16: bool, encoding, on_device: bool):
        """what a stream step emitted, [B, n] float32 on the device -> the piece: float32 on the host (`final`, or not `pcm16`), else
        converted row by row under its own peak on the device, companded behind that"""
        codec, B = self.codec, int(y.shape[0])
        if final or not pcm16:
            return codec.to_host(y)
        if y.shape[1] == 0:
            return np.zeros((B, 0), np.int16 if encoding is None else np.uint8)
        pcm = codec.float_to_int16(y, per_row=True)[0]
        if encoding is None:
            return pcm if on_device else codec.to_host(pcm)          # (`on_device`: a streamed FLAC pushes the tensor on)
        codes = codec.g711_encode(pcm.view(-1), [(0, pcm.numel(), encoding)])
        return codec.to_host(codes)[: pcm.numel()].reshape(tuple(pcm.shape))

    def infer_ids_stream(self, input_ids, attention_mask, text_mask, params: InferCodeParams = InferCodeParams(), *,
                         sample_rate: Optional[int] = None, **kw):
        """stream=True body of `Chat._infer` for one batch (core.py:455-503): every `stream_batch` live steps the
        generator yields the cumulative result and the next `stream_speed` samples of the decode of that prefix are
        emitted; the first `pass_first_n_batches` yields are dropped (core.py:488-490); the tail is emitted with all-silent
        columns removed (core.py:500-503).  The reference decodes the WHOLE prefix at every yield (O(n^2), App. D-10);
        here only the token window those samples depend on is decoded (same samples, O(n) in total), on the caller's
        stream while the generator's own stream already runs the next chunk.
        `sample_rate` (None or 24000: as above): every piece is its range of the prefix's decode resampled as one signal
        (`_stream_piece`); the schedule -- `length` -- stays in 24 kHz samples."""
        rate = None if sample_rate is None or int(sample_rate) == CodecEngine.SAMPLE_RATE else int(sample_rate)
        length = 0
        pass_batch_count = 0
        result = None
        for result in self.infer_code(input_ids, attention_mask, text_mask, params, stream=True, **kw):
            pass_batch_count += 1
            if pass_batch_count <= params.pass_first_n_batches:
                continue
            if rate is None:
                piece = self._stream_piece(result.hiddens, length, length + params.stream_speed)
                length += piece.shape[1]
            else:      # the 24 kHz count of the range, not the resampled piece's length
                piece = self._stream_piece(result.hiddens, length, length + params.stream_speed, rate=rate)
                total = 256 * (2 * max(int(r.size(0)) for r in result.hiddens) - 1)
                length += max(0, min(length + params.stream_speed, total) - length)
            yield piece
        if result is not None:
            new_wavs = self._stream_piece(result.hiddens, length, None, **({} if rate is None else {"rate": rate}))
            keep_cols = np.sum(np.abs(new_wavs) > 1e-5, axis=0) > 0
            yield new_wavs[:, keep_cols]

    def infer_tokens(self, input_ids, attention_mask, text_mask, params: InferCodeParams = InferCodeParams(),
                     stream: bool = False, split_text: bool = False, max_split_batch: int = 4, **kw):
        """`Chat.infer(..., skip_refine_text=True)` from the point where text has become tokens
        (core.py:208-270 + `_infer` :455-503): batches of `max_split_batch` rows when `split_text` (else one
        batch), then the sample-level silence strip of :258-268 (`wav[|wav| > 1e-5]`, also mid-utterance) and,
        with `split_text`, one concatenated waveform.  `stream=True` returns the chunk generator instead.
        `interrupt()` state is cleared first, like core.py:223."""
        self.context.set(False)
        B = int(input_ids.shape[0])
        if B == 0:
            return []
        if stream:
            return self.infer_ids_stream(input_ids, attention_mask, text_mask, params, **kw)
        step = max_split_batch if split_text else B
        thr = np.float32(1e-5)
        stripped = []
        for lo in range(0, B, step):
            sl = slice(lo, min(lo + step, B))
            kw_b = dict(kw)
            if "stop_at" in kw_b and kw_b["stop_at"] is not None:
                kw_b["stop_at"] = kw_b["stop_at"][sl]
            wavs = self.infer_ids(input_ids[sl], attention_mask[sl], text_mask[sl], params, **kw_b)
            for wav in wavs:
                stripped.append(wav[np.abs(wav) > thr])
        if split_text:
            return [np.concatenate(stripped)]
        return stripped

    # ---------------------------------------------------------------------------------------------------------
    # text level: the reference's public call (core.py:208-270) and its private helpers
    # ---------------------------------------------------------------------------------------------------------
    def _need_tokenizer(self):
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer loaded: Chat.load(custom_path=<dir holding asset/tokenizer>) or tokenizer=<dir>")

    def _infer_code(self, text, stream: bool, device, return_hidden: bool, params: InferCodeParams) -> Iterator[GenerationOutputs]:
        """core.py:542-662: decorate -> tokenise (+ audio-code prompt `spk_smp`) -> embed -> speaker -> generate."""
        ids, attn, tmask = self.code_prompt(text, params)
        return self.infer_code(ids, attn, tmask, params, stream=stream, return_hidden=return_hidden,
                               spk_emb_ids=self.tokenizer.spk_emb_ids)

    def infer_sharded(self, text, params_infer_code: InferCodeParams = InferCodeParams(), lang=None, do_text_normalization: bool = True,
                      do_homophone_replacement: bool = True, policy: str = "snake", group=None, dst: int = 0, use_decoder: bool = True):
        """`Chat.infer(text, skip_refine_text=True, split_text=False, use_decoder=...)` (core.py:208-270) over the ranks of the `torch.distributed` process
        group: every rank calls this with the SAME texts and parameters; the batch is tokenised everywhere (host work, deterministic), dealt
        by prompt length, generated and decoded shard by shard (`dist.infer_sharded`: global row numbering for the CPU draws and the
        rows >= 625 quirk, decode padded to the global longest utterance) and rank `dst` returns the list of stripped waveforms in the
        caller's order -- what the single-process call returns; the other ranks return None.  The reference has no data-parallel mode."""
        from .dist import infer_sharded
        assert self.has_loaded(use_decoder=use_decoder)
        self._need_tokenizer()
        self.context.set(False)
        if not isinstance(text, list):
            text = [text]
        if len(text) == 0:
            return []
        text = [self.normalizer(t, do_text_normalization, do_homophone_replacement, lang) for t in text]
        params = params_infer_code
        prompt = Speaker.decode_prompt(params.spk_smp) if params.spk_smp is not None else None
        ids, attn, tmask = self.tokenizer.encode(
            Speaker.decorate_code_prompts(text, params.prompt, params.txt_smp, params.spk_emb), GPT.n_vq, prompt=prompt)
        wavs = infer_sharded(self, ids, attn, tmask, params, policy=policy, group=group, dst=dst, use_decoder=use_decoder,
                             spk_emb_ids=self.tokenizer.spk_emb_ids)
        if wavs is None:
            return None
        thr = np.float32(1e-5)
        return [wav[np.abs(wav) > thr] for wav in wavs]     # core.py:258-266: the sample-level strip

    def _refine_text(self, text, device, params: RefineTextParams) -> GenerationOutputs:
        """core.py:665-751"""
        ids, attn, tmask = self.refine_prompt(text, params)
        return self.refine_text_ids(ids, attn, tmask, self.tokenizer.eos_token, params, num_code=self.tokenizer.len)

    def refine_prompt(self, text, params: RefineTextParams):
        """decorate -> tokenise of ALREADY NORMALISED texts for the refine-text pass (the head of `_refine_text`): (input_ids [B,T,4], attention_mask
        [B,T], text_mask [B,T]).  `Chat.infer` and the batched server's refine stage (serving.SpeechBatcher) both build their prompts here."""
        self._need_tokenizer()
        if not isinstance(text, list):
            text = [text]
        return self.tokenizer.encode(Speaker.decorate_text_prompts(text, params.prompt), GPT.n_vq)

    def refined_text(self, rows) -> List[str]:
        """refined token rows -> the texts of the code pass (what `_infer` does with them): control tokens >= [break_0] dropped, then decoded.  Shared
        by `_infer` and the batched server's hand-off from the text pool to the code pool."""
        self._need_tokenizer()
        tokens = [row[row.less(self.tokenizer.break_0_ids)] for row in rows]
        return self.tokenizer.decode(tokens)

    def infer(self, text, stream=False, lang=None, skip_refine_text=False, refine_text_only=False, use_decoder=True,
              do_text_normalization=True, do_homophone_replacement=True, split_text=True, max_split_batch=4,
              params_refine_text: RefineTextParams = RefineTextParams(), params_infer_code: InferCodeParams = InferCodeParams(),
              *, pcm16: bool = False, ragged_decode: bool = False, sample_rate: int = 24000, stream_resample: bool = False,
              encoding: Optional[str] = None, speed: float = 1.0, stream_time_scale: bool = False, stream_scaled_resample: bool = False,
              flac: bool = False, loudness=None, stream_flac: bool = False, pauses=None, limiter=None,
              stream_limiter: bool = False, gain_db=None, stream_pauses: bool = False, adpcm: bool = False, stream_adpcm: bool = False,
              compress=None, stream_compress: bool = False, eq=None):
        """core.py:208-270: `List[np.ndarray]` (one stripped waveform per text, or ONE concatenated waveform when
        `split_text`), a generator of `np.ndarray [B, n]` chunks when `stream`, the refined text when `refine_text_only`.
        `pcm16=True` (keyword-only, not in the reference): the same results as 16-bit PCM -- what the reference's callers get from
        `float_to_int16` (tools/audio/np.py:7-11) on each returned waveform / on each row of each streamed chunk, computed on the
        device so that half the bytes cross PCIe: `infer(t, pcm16=True)[i] == float_to_int16(infer(t)[i])` bit for bit.
        `ragged_decode=True` (keyword-only, non-streamed only; NOT the reference's batch semantics): every utterance of a batch is
        decoded as if alone (CodecEngine.decode_ragged) instead of as a row of the reference's zero-padded batch, so a shorter
        utterance's last second no longer depends on the longer ones it was batched with.
        `sample_rate` (keyword-only, non-streamed only): the rate of the returned audio.  Every decoded waveform is resampled on the
        device directly behind the ISTFT (CodecEngine.resample); the silence strip, the 16-bit conversion and the concatenation of a
        split request work on the resampled samples.  The refer sentence's audio that becomes `spk_smp` of a split request stays at
        24 kHz.  A streamed call at another rate raises unless `stream_resample=True` (keyword-only): then every chunk is its range
        of the prefix's decode resampled as one signal -- the chunk the 24 kHz schedule defines as samples [s_lo, s_hi) becomes outputs
        [ceil(s_lo L / M), ceil(s_hi L / M)), so the chunks tile the resampled stream; the schedule itself (stream_speed,
        pass_first_n_batches, ...) stays in 24 kHz samples; each chunk's 16-bit peak and the tail's silence strip are taken on the
        resampled samples.  No filter state is carried: a chunk is converted from a token window widened by the filter's reach
        (CodecEngine.decode_window).  A `split_text` stream at another rate raises.
        `encoding` (keyword-only; None: 16-bit PCM, the call above): "ulaw" / "alaw" -- G.711, one byte per sample, what telephone
        bridges take (usually with sample_rate=8000).  Needs `pcm16=True` (ValueError otherwise).  Every result is `g711.encode` of the
        int16 array the same call returns without it, element for element: the companding comes strictly behind the 16-bit conversion
        and runs on the device wherever that does (CodecEngine.g711_encode).
        `speed` (keyword-only, non-streamed only; 0.5 .. 2.0, taken in hundredths): the same utterance at the same pitch, `speed` times
        as fast -- the generator samples exactly what it samples at 1.0, and every decoded waveform is time-scaled on the device at
        24 kHz (CodecEngine.time_scale: waveform-similarity overlap-add) directly behind the ISTFT, in front of the resampler, the
        silence strip, the 16-bit conversion and the companding; the sentences of a split request are scaled one by one.  The refer
        sentence's audio that becomes `spk_smp` of a split request stays at speed 1.  A streamed call at another speed raises: a
        chunk's frames depend on the path the search took through everything before it, which is not carried across chunks --
        unless `stream_time_scale=True` (keyword-only): then every row of the batch gets a stream of the time scaler
        (CodecEngine.time_scale_stream_step: the path's last entry and a short tail of samples are carried on the device), the
        24 kHz chunks of the unchanged schedule are pushed into it and each yield hands out what its push made final: the chunks,
        concatenated, are `time_scale` of the speed-1 stream with its tail not yet stripped; each chunk's 16-bit peak, the tail's
        column filter and the companding are taken on the scaled samples.  A chunk is a multiple of 512 samples and may be empty;
        the first one needs ~55-75 ms of audio beyond its frames.  Refused with a streamed speed: a `sample_rate` other than 24000
        (resampling the scaled stream would need its history and a look-ahead carried too), `split_text` (`length` pulls back
        between batches) and `use_decoder=False`.
        `stream_scaled_resample=True` (keyword-only; with `stream_time_scale` and `stream_resample`) carries that history and
        look-ahead: every row also gets a stream of the resampler (CodecEngine.resample_stream_step: at most K - 1 scaled samples are
        kept on the device), the scaler's chunks are pushed into it and each yield hands out the outputs whose inputs have all
        arrived: the chunks, concatenated, are `resample(time_scale(speed-1 stream), 24000, sample_rate)`; the 16-bit peak, the
        tail's column filter and the companding are taken on those samples.  The first output needs width + M scaled samples
        beyond its frame (22 at 8000 Hz: under 1 ms on top of the scaler's own).
        `flac=True` (keyword-only, non-streamed only; needs `pcm16=True`, not together with `encoding`: ValueError otherwise): every
        result is a uint8 array holding the complete FLAC file (chattts_amd/flac.py: mono, 16 bits, at `sample_rate`) of exactly the
        int16 samples the same call returns without it -- lossless, encoded on the device behind the conversion
        (CodecEngine.flac_encode), so that the compressed bytes are what cross PCIe.  A streamed call raises unless
        `stream_flac=True` (keyword-only): then every row of the batch gets a FLAC stream (variable-block-size frames that carry the
        number of their first sample; chattts_amd/flac.py, StreamEncoder) and every yield is a list with one uint8 array per row: the
        frames that chunk completes -- an empty array when it completes none (up to 15 samples wait for the next chunk; the last
        chunk brings them).  The frames of a row behind `flac.stream_header(sample_rate)` are a FLAC stream that decodes to exactly
        the int16 chunks the call yields without `flac`, concatenated.  The chunks are pushed on the device
        (CodecEngine.flac_stream_step; a chunk that was converted on the host, like the last one, is uploaded for its push); with
        `incremental_stream=False` or without the decoder every chunk is converted on the host and the host twin encodes the
        stream.  It combines with `sample_rate` / `stream_resample`, `speed` / `stream_time_scale` and `stream_scaled_resample`; not
        with `split_text` (every split batch would end the stream).  The streams' slots are given back when the generator ends or
        is dropped.  Without `stream_flac` a streamed FLAC is refused: it needs a variable-block-size
        stream and carried sample numbers: it raises.
        `loudness` (keyword-only, non-streamed only; None: untouched): a target in LUFS, -40 .. -5 -- one number, or one per text.
        Every utterance is brought to that ITU-R BS.1770-4 integrated loudness on the device (CodecEngine.loudness_normalize) by one
        gain, capped at +30 dB and at a -1 dBFS sample peak: the last float32 stage, behind the time scaler and the resampler and in
        front of the silence strip, the 16-bit conversion, the companding and FLAC.  A split request gets ONE gain over its sentences
        (one target only).  A streamed call with a target raises: an integrated loudness needs the whole utterance.
        `pauses` (keyword-only, non-streamed only; None: untouched): True (the defaults), a pauses.PauseSpec or a dict of its fields
        (max_pause_ms, lead_ms, tail_ms, threshold_db, pad_ms) -- one, or a list with one per text.  Every utterance loses the
        near-silence in front of and behind it down to lead_ms / tail_ms, and an inner pause longer than max_pause_ms keeps its two
        ends, crossfaded (CodecEngine.trim_pauses, on the device): behind the time scaler and the resampler, so the milliseconds are
        those of what is heard, and in front of the loudness stage, the silence strip, the 16-bit conversion, the companding and
        FLAC.  Every sentence of a split request is trimmed alone (one spec only), so the gap at a join is at most tail + lead; with
        `loudness` the request still gets ONE gain, over its trimmed sentences.  A streamed call with it raises: the run state would
        have to be carried across chunks.
        `limiter` (keyword-only, non-streamed only; None / False: off): True -- or one flag per text -- puts the look-ahead peak
        limiter (CodecEngine.peak_limit; the definition of limiter.py: 10 ms of look-ahead, 10 ms of smoothing, a -1 dBFS ceiling
        held sample by sample) behind the loudness stage's gain, which then drops its ceiling term: one loud plosive no longer
        decides the level of the whole utterance.  Without `loudness` it runs at unity gain, so a decoded peak above full scale is
        limited instead of clipped by the 16-bit conversion.  It sits where the loudness stage does: behind the time scaler, the
        resampler and `pauses`, in front of the silence strip, the 16-bit conversion, the companding and FLAC.  The sentences of a
        split request (one flag only) are limited one by one under the request's ONE gain.  A streamed call with it raises: the
        look-ahead is not carried across chunks -- unless
        `stream_limiter=True` (keyword-only): then every row of a streamed batch gets a limiter stream (CodecEngine.peak_limit_stream_*,
        opened at the first chunk, closed when the generator ends or is dropped) between the last float stage -- the crop, the
        resampled window, the time scaler's or the scaled resampler's stream -- and the 16-bit conversion, so every chunk is converted,
        companded and FLAC-encoded from limited samples.  The stream lags by 20 ms (rate // 50 samples: a sample's gain needs the 20 ms
        behind it); its chunks, end to end, are the limiter of the whole float stream bit for bit, and the last chunk brings the rest.
        One flag for the whole batch; refused with `split_text` and without the decoder.
        `stream_pauses=True` (keyword-only): then `pauses` goes with `stream=True` -- one spec for the whole batch; every row gets a pause
        stream (CodecEngine.trim_pauses_stream_*), opened at the first chunk and closed when the generator ends or is dropped, behind the
        last float stage and in front of the limiter stream and the conversion.  The rows emit different numbers of samples, so every
        yield is a list with one array per row, possibly empty, as a streamed FLAC yields; per row the chunks, end to end, are the
        one-shot `pauses` result of that row's stream.  Refused with `split_text`, without the decoder, and for a spec whose
        `pauses.stream_need` exceeds `pauses.STREAM_FRAMES`.  Without the switch the refusal above stays.
        `gain_db` (keyword-only; with `stream=True, limiter=True, stream_limiter=True` only): a fixed make-up gain in dB, -30 .. +30, one
        for the whole batch, applied in front of the limiter as its float32 pre-gain 10 ** (gain_db / 20).  A non-streamed call has
        `loudness` for its level and refuses it.
        `adpcm=True` (keyword-only, non-streamed only; needs `pcm16=True`, not together with `encoding` or `flac`: ValueError
        otherwise): every result is a uint8 array holding the complete WAVE_FORMAT_IMA_ADPCM file (chattts_amd/adpcm.py: mono, 4 bits
        per sample, blocks of 256 / 512 / 1024 bytes by `sample_rate`) of exactly the int16 samples the same call returns without it
        -- half of G.711's size, encoded on the device behind the conversion (CodecEngine.adpcm_encode), at whatever rate, speed,
        pauses, loudness and limiter the call has.  A split request is one file over its concatenated sentences.  A streamed call
        raises unless `stream_adpcm=True` (keyword-only): then every row of the batch gets an ADPCM stream at the output rate (opened at
        the first chunk, closed with the generator) and every yield is a list with one uint8 array per row: the whole blocks that
        chunk completes, possibly none -- a stream keeps up to S - 1 samples of an open block (chattts_amd/adpcm.py, StreamEncoder),
        and the last chunk brings them, padded as the file's last block is.  The chunks of a row, concatenated, are
        `adpcm.encode_blocks` of the int16 chunks the call yields without `adpcm`, concatenated; behind `adpcm.stream_header(rate)`
        they are an open-ended WAV file, whose reader cannot know the true length and decodes up to S - 1 padded samples behind the
        last real one.  The chunks are pushed on the device (CodecEngine.adpcm_stream_step; the placement and the host-twin
        fallback of a streamed FLAC), behind whatever `sample_rate` + `stream_resample`, `speed` + `stream_time_scale`, `limiter` +
        `stream_limiter` and `pauses` + `stream_pauses` make of the stream.  Not with `split_text`, nor with `use_decoder=False`.
        `compress` (keyword-only, non-streamed only; None / False: off): True (the defaults) or a dict with any of threshold_db, ratio,
        knee_db, attack_ms, hold_ms (chattts_amd/compressor.py) -- one, or a list with one per text.  Every utterance goes through the
        feed-forward look-ahead compressor on the device (CodecEngine.compress): levels above the threshold are brought down along a
        soft-knee curve, block by block of 1 ms, with the gain ramped down ahead of a loud block and held behind it; no sample is
        raised.  It is stage 3 1/2 of the output chain: behind the time scaler, the resampler and `pauses`, in front of the loudness
        stage -- so the target is reached on compressed samples -- the limiter, the silence strip, the 16-bit conversion, the
        companding and the file formats.  Every sentence of a split request is compressed alone (one spec only).  A streamed call
        with it raises: a compressed stream would need the block state carried across chunks -- unless
        `stream_compress=True` (keyword-only): then `compress` goes with `stream=True` -- one spec for the whole batch; every row gets a
        compressor stream (CodecEngine.compress_stream_*: the block gains of the hold and the few unemitted raw samples are carried on
        the device), behind the streamed rate, speed and pause stages and in front of the limiter stream, the conversion, the
        companding and the streamed file formats, the non-streamed order.  A row's chunks, end to end, are its uncompressed stream's
        samples compressed as one signal, bit for bit; the stream lags by the attack and at most two more milliseconds, and the last
        chunk brings the rest.  As with `stream_pauses` a chunk is a list with one array per row.  Not with `split_text`, nor with
        `use_decoder=False`.
        `eq` (keyword-only, non-streamed only; None / False: off): an equaliser preset name ("telephone": a 300 Hz high-pass; "rumble":
        an 80 Hz high-pass) or a dict with any of highpass_hz, lowshelf {hz, db}, highshelf {hz, db}, peaks [{hz, db, q}, ...], at most
        four second-order sections (chattts_amd/equalizer.py) -- one, or a list with one per text.  Every utterance goes through the
        biquad cascade on the device (CodecEngine.equalize), in float64 from zero state: stage 3 1/4 of the output chain, behind the
        time scaler, the resampler and `pauses` -- the pause detector sees the signal it was tuned on -- and in front of `compress`, the
        loudness stage and the limiter, which see what the listener will hear, the silence strip, the 16-bit conversion, the
        companding and the file formats.  Frequencies lie in 20 Hz .. 0.45 of the returned rate.  Every sentence of a split request
        is filtered alone from zero state (one spec only).  A streamed call with it raises: an equalised stream would need the
        filter state carried across chunks."""
        ekw = Plan.given("infer", eq=eq).kwargs()
        if ekw and stream:
            raise ValueError("eq applies to non-streamed inference only (an equalised stream would need the filter state carried across "
                             "chunks)")
        if ekw and split_text and isinstance(eq, list):
            raise ValueError("a split_text request is one waveform: it takes one equaliser spec")
        if ekw:
            for e in eq if isinstance(eq, list) else [eq]:
                EQ.check(e, "infer", LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate)))
        mkw = Plan.given("infer", limiter=limiter).kwargs()
        if gain_db is not None and np.ndim(gain_db) != 0:
            raise ValueError("gain_db is one make-up gain for the whole batch")
        g32 = LM.check_gain_db(gain_db)
        if g32 is not None and not mkw:
            raise ValueError("gain_db is the make-up gain in front of the limiter: it needs limiter=True")
        if g32 is not None and not stream:
            raise ValueError("gain_db applies to a limited stream only (a non-streamed call sets its level with loudness)")
        if mkw and stream and not stream_limiter:
            raise ValueError("limiter applies to non-streamed inference only (the look-ahead is not carried across chunks)")
        smkw = {}
        if mkw and stream:
            if np.ndim(limiter) != 0:
                raise ValueError("a limited stream takes one limiter flag for the whole batch")
            if split_text:
                raise ValueError("a limited stream does not go with split_text (every split batch would end the stream)")
            if not use_decoder:
                raise ValueError("a limited stream needs the hidden-state decoder (use_decoder=True)")
            LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
            smkw, mkw = {"lm_gain": np.float32(1.0) if g32 is None else g32}, {}
        if mkw and split_text and np.ndim(limiter) != 0:
            raise ValueError("a split_text request is one waveform: it takes one limiter flag")
        if mkw:
            LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
        pkw = Plan.given("infer", pauses=pauses).kwargs()
        if pkw and stream and not stream_pauses:
            raise ValueError("pauses applies to non-streamed inference only (a stream would need the run state carried across chunks)")
        spkw = {}
        if pkw and stream:
            if isinstance(pauses, (list, tuple)):
                raise ValueError("a paused stream takes one pause spec for the whole batch")
            if split_text:
                raise ValueError("a paused stream does not go with split_text (every split batch would end the stream)")
            if not use_decoder:
                raise ValueError("a paused stream needs the hidden-state decoder (use_decoder=True)")
            spkw = {"pa_spec": PA.check_stream(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate), pauses, "infer")[1]}
            pkw = {}
        if pkw and split_text and isinstance(pauses, (list, tuple)):
            raise ValueError("a split_text request is one waveform: it takes one pause spec")
        if pkw:
            PA.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
        ckw = Plan.given("infer", compress=compress).kwargs()
        if ckw and stream and not stream_compress:
            raise ValueError("compress applies to non-streamed inference only (a compressed stream would need the block state carried "
                             "across chunks)")
        sckw = {}
        if ckw and stream:
            if isinstance(compress, list):             # (a tuple is a checked spec, as the endpoint passes it on)
                raise ValueError("a compressed stream takes one compressor spec for the whole batch")
            if split_text:
                raise ValueError("a compressed stream does not go with split_text (every split batch would end the stream)")
            if not use_decoder:
                raise ValueError("a compressed stream needs the hidden-state decoder (use_decoder=True)")
            LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
            sckw, ckw = {"cp_spec": CP.check(compress, "infer")}, {}
        if ckw and split_text and isinstance(compress, list):
            raise ValueError("a split_text request is one waveform: it takes one compressor spec")
        if ckw:
            LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
        lkw = Plan.given("infer", loudness=loudness).kwargs()
        if lkw and stream:
            raise ValueError("loudness applies to non-streamed inference only (an integrated loudness needs the whole utterance; a "
                             "stream would need a running measure)")
        if lkw and split_text and np.ndim(loudness) != 0:
            raise ValueError("a split_text request is one waveform: it takes one loudness target")
        if lkw:
            LN.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
        if G711.check_encoding(encoding) is not None and not pcm16:
            raise ValueError("encoding applies to 16-bit output: pass pcm16=True")
        if flac:
            if not pcm16:
                raise ValueError("flac applies to 16-bit output: pass pcm16=True")
            if encoding is not None:
                raise ValueError("flac does not go with an encoding (a FLAC file holds the 16-bit samples)")
            if stream and not stream_flac:
                raise ValueError("flac applies to non-streamed inference only (a streamed FLAC needs a variable-block-size stream and "
                                 "carried sample numbers, which is not implemented)")
            if stream and split_text:
                raise ValueError("a streamed FLAC does not go with split_text (every split batch would end the stream)")
            FLAC.rate_code(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
        if adpcm:
            if not pcm16:
                raise ValueError("adpcm applies to 16-bit output: pass pcm16=True")
            if encoding is not None:
                raise ValueError("adpcm does not go with an encoding (an ADPCM file is coded from the 16-bit samples)")
            if flac:
                raise ValueError("adpcm does not go with flac (a call hands out one kind of file)")
            if stream and not stream_adpcm:
                raise ValueError("adpcm applies to non-streamed inference only (a streamed ADPCM file would carry up to a block's "
                                 "samples across chunks, which is not implemented)")
            if stream and split_text:
                raise ValueError("a streamed ADPCM file does not go with split_text (every split batch would end the stream)")
            if stream and not use_decoder:
                raise ValueError("a streamed ADPCM file needs the hidden-state decoder (use_decoder=True)")
            ADPCM.check_rate(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate))
            if stream and ADPCM.samples_per_block(CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate)) - 1 > CodecEngine.ADPCM_CARRY:
                raise ValueError(f"a streamed ADPCM file at {int(sample_rate)} Hz would carry more than a stream keeps ({CodecEngine.ADPCM_CARRY} "
                                 "samples): streams run below 55125 Hz")
        akw = {"adpcm": True} if adpcm else {}
        skw = Plan.given("infer", speed=speed).kwargs()
        if stream and skw and not stream_time_scale:
            raise ValueError("speed applies to non-streamed inference only (a chunk's frames depend on the path of everything before it; "
                             "pass stream_time_scale=True to carry the path across chunks)")
        sample_rate = CodecEngine.SAMPLE_RATE if sample_rate is None else int(sample_rate)
        if stream and skw:
            if sample_rate != CodecEngine.SAMPLE_RATE and not stream_scaled_resample:
                raise ValueError("a streamed speed is served at 24000 Hz only (resampling the scaled stream would need its history and a "
                                 "look-ahead carried too)")
            if split_text:
                raise ValueError("a streamed speed does not go with split_text (the schedule's length pulls back between batches)")
            if not use_decoder:
                raise ValueError("a streamed speed needs the hidden-state decoder (use_decoder=True)")
            if np.ndim(speed) != 0:
                raise ValueError("a streamed speed is one number for the whole batch")
        if stream and sample_rate != CodecEngine.SAMPLE_RATE:
            if not stream_resample:
                raise ValueError("sample_rate applies to non-streamed inference only (a stream's chunks would need the filter's state carried "
                                 "across them, which is not implemented)")
            if split_text:
                raise ValueError("a streamed split_text request is served at 24000 Hz only")
            K = RS.plan(CodecEngine.SAMPLE_RATE, sample_rate, [0, 1])[2]      # an unsupported pair is refused here, not at the first chunk
            if skw and K - 1 > RS.CARRY:
                raise ValueError(f"a streamed speed at {sample_rate} Hz would carry up to {K - 1} samples, a resampler stream keeps {RS.CARRY}")
        rate = None if sample_rate == CodecEngine.SAMPLE_RATE else sample_rate
        if ragged_decode and stream:
            raise ValueError("ragged_decode applies to non-streamed inference only")
        if ragged_decode and not use_decoder:
            raise NotImplementedError("ragged decoding covers the hidden-state decoder only (use_decoder=True)")
        self.context.set(False)
        if split_text and isinstance(text, str):
            text = split_sentences(text)
            self.logger.info("split text into %d parts", len(text))
        if len(text) == 0:
            return []
        # split_text + pcm16 + ragged_decode: the hidden states of every split batch are collected and the whole request is decoded,
        # stripped, converted under its one peak and compacted on the device (decode_split_to_pcm16) -- the bytes of the host lines below
        split_dev = bool(split_text and pcm16 and ragged_decode and not stream and not refine_text_only)
        lkw = {**lkw, **mkw}
        split_host = bool(lkw and split_text and not split_dev and not refine_text_only)      # one gain over the sentences: applied below
        res_gen = self._infer(text, stream, lang, skip_refine_text, refine_text_only, use_decoder, do_text_normalization,
                              do_homophone_replacement, split_text, max_split_batch, params_refine_text, params_infer_code,
                              pcm16=pcm16 and not refine_text_only and not (split_text and not stream), ragged=ragged_decode, raw=split_dev,
                              sample_rate=rate, **({} if encoding is None else {"encoding": encoding}), **skw, **({"flac": True} if flac else {}),
                              **({} if split_host else lkw), **pkw, **smkw, **spkw, **akw, **ckw, **sckw, **ekw)
        if stream:
            return res_gen
        if refine_text_only:
            return next(res_gen)
        if split_dev:
            rows = [h for hids in res_gen for h in hids]
            if rows:
                return self.decode_split_to_pcm16([rows], **({} if rate is None else {"sample_rate": rate}),
                                                  **({} if encoding is None else {"encoding": encoding}), **skw,
                                                  **({"flac": True} if flac else {}), **lkw, **pkw, **akw, **ckw, **ekw)
            res_gen = iter(())      # no batch produced anything: what the host lines below make of that
        if pcm16 and not split_text:
            return [w for wavs in res_gen for w in wavs]          # already stripped and converted, utterance by utterance, on the device
        thr = np.float32(1e-5)
        if split_host:
            res_gen = [self._normalize_request([w for wavs in res_gen for w in wavs], lkw.get("loudness"), sample_rate, **mkw)]
        stripped = [wav[np.abs(wav) > thr] for wavs in res_gen for wav in wavs]   # sample-level strip, also mid-utterance
        if pcm16:      # split_text: ONE concatenated waveform, hence one peak over all sentences -- converted on the host
            one = float_to_int16(np.concatenate(stripped))
            if flac:      # a split request concatenated on the host: encoded by the host twin, like the conversion in front of it
                return [np.frombuffer(FLAC.encode(one, sample_rate), np.uint8)]
            if adpcm:
                return [ADPCM.encode_result(one, sample_rate)]
            return [one if encoding is None else G711.encode(one, encoding)]
        return [np.concatenate(stripped)] if split_text else stripped

    def _normalize_request(self, wavs, target, rate: int, **lim) -> List[np.ndarray]:
        """the sentences of a split request that is concatenated on the host: ONE loudness and ONE gain over all of them, on the
        device (the waveforms go there and back as one pack; every sentence is filtered alone, and with `limiter` limited alone)"""
        if len(wavs) == 0:
            return []
        off = np.zeros(len(wavs) + 1, np.int64)
        np.cumsum([len(w) for w in wavs], out=off[1:])
        pack = torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float32) for w in wavs])).to(self.device)
        out = self.codec.loudness_normalize(pack, target, offsets=off, groups=np.array([0, len(wavs)], np.int32), rates=rate, out=pack, **lim)
        return ragged_views(self.codec.to_host(out), off)

    def _infer(self, text, stream, lang, skip_refine_text, refine_text_only, use_decoder, do_text_normalization,
               do_homophone_replacement, split_text, max_split_batch, params_refine_text, params_infer_code, pcm16: bool = False,
               ragged: bool = False, raw: bool = False, sample_rate: Optional[int] = None, encoding: Optional[str] = None,
               speed: Optional[float] = None, flac: bool = False, loudness=None, pauses=None, limiter=None, lm_gain=None, pa_spec=None,
               adpcm: bool = False, compress=None, cp_spec=None, eq=None):
        """core.py:395-503 (generator).  `cp_spec` with `stream`: the rows' compressor streams and their spec (Chat.infer's `stream_compress`).  `pa_spec` with `stream`: the rows' pause streams and their spec (Chat.infer's `stream_pauses`).  `lm_gain` with `stream`: the rows' limiter streams and their pre-gain (Chat.infer's `stream_limiter`).  `flac` with `stream`: the rows' FLAC streams (Chat.infer's `stream_flac`).  `raw` (non-streamed, decoder path): a batch's hidden-state rows are yielded undecoded."""
        assert self.has_loaded(use_decoder=use_decoder)
        if not isinstance(text, list):
            text = [text]
        text = [self.normalizer(t, do_text_normalization, do_homophone_replacement, lang) for t in text]
        if not skip_refine_text:
            refined = self._refine_text(text, self.device, params_refine_text)
            text = self.refined_text(refined.ids)     # control tokens >= [break_0] dropped, decoded
            refined.destroy()
            if refine_text_only:
                yield "\n".join(text) if (split_text and isinstance(text, list)) else text
                return
        if split_text and len(text) > 1 and params_infer_code.spk_smp is None:
            # core.py:435-453: the first sentence is synthesised alone and its audio becomes the speaker prompt of the rest
            refer_text = text[0]
            result = next(self._infer_code(refer_text, False, self.device, use_decoder, params_infer_code))
            params_infer_code.spk_smp = self.refer_speaker(result.hiddens if use_decoder else result.ids, use_decoder, release=result.destroy)
            params_infer_code.txt_smp = refer_text
        step = max_split_batch if split_text else len(text)
        sets = [] if stream else None      # a stream: one `winchain.StreamSet` per row, opened at the first chunk (`_infer_batches`)
        on = lambda v: stream and v is not None
        try:
            yield from self._infer_batches(text, step, stream, use_decoder, split_text, params_infer_code, pcm16, ragged, raw, sample_rate,
                                           encoding, speed, sets, **({"flac": True} if flac else {}),
                                           **({} if loudness is None else {"loudness": loudness}), **({} if pauses is None else {"pauses": pauses}),
                                           **({} if limiter is None else {"limiter": limiter}), **({"lm_gain": lm_gain} if on(lm_gain) else {}),
                                           **({"pa_spec": pa_spec} if on(pa_spec) else {}), **({"adpcm": True} if adpcm else {}),
                                           **({} if compress is None else {"compress": compress}), **({} if eq is None else {"eq": eq}),
                                           **({"cp_spec": cp_spec} if on(cp_spec) else {}))
        finally:
            for st in sets or ():              # also when the consumer drops the generator half way
                st.close(self.codec)

    def _infer_batches(self, text, step, stream, use_decoder, split_text, params_infer_code, pcm16, ragged, raw, sample_rate, encoding, speed,
                       sets=None, flac: bool = False, loudness=None, pauses=None, limiter=None, lm_gain=None, pa_spec=None, adpcm: bool = False,
                       compress=None, cp_spec=None, eq=None):
        """the batch loop of `_infer`.  `sets` (a stream): the rows' `winchain.StreamSet`s, opened here at the first chunk, closed by `_infer`"""
        scaled = stream and speed is not None
        filed = stream and (flac or adpcm) and pcm16           # the chunks are FLAC frames, or with `adpcm` IMA ADPCM blocks
        rowwise = stream and (pa_spec is not None or cp_spec is not None)      # the chunks are lists with one array per row
        # a filed stream's encoder streams are on the device, or host twins where every chunk is converted on the host: the same placement
        Twin, twins = ADPCM.StreamEncoder if adpcm else FLAC.StreamEncoder, []
        fs_step = lambda pcm, pushes: (self.codec.adpcm_stream_step if adpcm else self.codec.flac_stream_step)(pcm, pushes)

        def handles(rows):
            """the rows' stream sets, opened at the first chunk with what the options need -> stage name -> the rows' handles"""
            if not sets:
                dev = filed and (rowwise or (use_decoder and self.incremental_stream))
                sets.extend(WC.StreamSet.open(self.codec, rate=sample_rate, speed=speed, pauses=pa_spec, compress=cp_spec, limiter_gain=lm_gain,
                                              flac=dev and not adpcm, adpcm=dev and adpcm) for _ in rows)
            return {name: [st[name] for st in sets] for name in (sets[0] if sets else ())}

        def flac_chunks(piece, final, fs):
            """the rows of one streamed chunk (int16 [B, n]: a device tensor, or converted on the host) pushed into the rows' encoder
            streams `fs` (None: the host twins) -> one uint8 array per row"""
            B, n = int(piece.shape[0]), int(piece.shape[1])
            if fs is None:
                if not twins:
                    twins.extend(Twin(CodecEngine.SAMPLE_RATE if sample_rate is None else sample_rate) for _ in range(B))
                piece = np.asarray(piece).astype(np.int16, copy=False)
                return [np.frombuffer(e.push(np.ascontiguousarray(r), final), np.uint8) for e, r in zip(twins, piece)]
            if not isinstance(piece, torch.Tensor):
                piece = torch.from_numpy(np.ascontiguousarray(piece, dtype=np.int16)).to(self.device)
            if n == 0:
                piece = torch.zeros((B, 8), dtype=torch.int16, device=self.device)
            elif n % 8 and B > 1:  # every row starts on a multiple of 8 samples
                piece = torch.nn.functional.pad(piece, (0, -n % 8))
            row = int(piece.shape[1])
            piece = piece.contiguous()
            if piece.data_ptr() % 16:          # a view into the conversion's buffer: the encoder reads 16-byte units
                piece = piece.clone()
            return fs_step(piece.view(-1), [(h, i * row, n, final) for i, h in enumerate(fs)])

        def piece_of(rows, a, b, final):
            """one chunk of the stream through the rows' streams: `_stream_rows_paused` (a list, one array per row), `_stream_piece_scaled`
            or `_stream_piece`, each with the handle lists it takes -> (the chunk, the rows' encoder streams or None)"""
            h = handles(rows) if stream else {}
            fs = h.get("adpcm" if adpcm else "flac")
            lkw = {"lm_handles": h["limiter"]} if "limiter" in h else {}
            dkw = {"on_device": True} if filed else {}
            if rowwise:
                return self._stream_rows_paused(rows, a, b, final, h.get("pauses"), sample_rate, h.get("time_scale"), h.get("resample"),
                                                h.get("limiter"), pcm16, encoding if pcm16 else None, fs, **({"fs_step": fs_step} if adpcm else {}),
                                                **({"cp_handles": h["compress"]} if "compress" in h else {})), fs
            if scaled:
                rkw = {"rs_handles": h["resample"]} if "resample" in h else {}
                if final:
                    return self._stream_piece_scaled(rows, a, b, h["time_scale"], True, **rkw, **lkw), fs
                return self._stream_piece_scaled(rows, a, b, h["time_scale"], False, pcm16, encoding if pcm16 else None, **rkw, **dkw, **lkw), fs
            skw = {"rate": sample_rate} if sample_rate is not None else {}      # 24 kHz: today's call, argument for argument
            if final:
                return self._stream_piece(rows, a, b, use_decoder, **skw, **({**lkw, "final": True} if lkw else {})), fs
            if encoding is not None and pcm16:
                skw["encoding"] = encoding
            return self._stream_piece(rows, a, b, use_decoder, pcm16, **skw, **dkw, **lkw), fs
        length = 0
        pass_batch_count = 0
        for lo in range(0, len(text), step):
            batch = text[lo: lo + step]
            if split_text:
                self.logger.info("infer split %d~%d", lo, lo + len(batch))
            last = None
            for result in self._infer_code(batch, stream, self.device, use_decoder, params_infer_code):
                if not stream:
                    src = result.hiddens if use_decoder else result.ids
                    rkw = {} if sample_rate is None else {"sample_rate": sample_rate}      # 24 kHz: today's call, argument for argument
                    if encoding is not None and pcm16:
                        rkw["encoding"] = encoding
                    if speed is not None:
                        rkw["speed"] = speed
                    if flac and pcm16:
                        rkw["flac"] = True
                    if adpcm and pcm16:
                        rkw["adpcm"] = True
                    if loudness is not None and not raw:
                        rkw["loudness"] = loudness
                    if limiter is not None and not raw:
                        rkw["limiter"] = limiter
                    if pauses is not None and not raw:
                        rkw["pauses"] = pauses[lo: lo + step] if isinstance(pauses, list) else pauses
                    if compress is not None and not raw:
                        rkw["compress"] = compress[lo: lo + step] if isinstance(compress, list) else compress
                    if eq is not None and not raw:
                        rkw["eq"] = eq[lo: lo + step] if isinstance(eq, list) else eq
                    if raw:         # Chat.infer decodes the whole split request at once (decode_split_to_pcm16)
                        rows = [h.clone() for h in src]
                        result.destroy()
                        yield rows
                        continue
                    if ragged:      # every utterance as if alone (Chat.infer's ragged_decode)
                        wavs = self.decode_to_pcm16(src, ragged=True, **rkw) if pcm16 else self.decode_to_wavs(src, ragged=True, **rkw)
                    else:
                        wavs = self.decode_to_pcm16(src, use_decoder, **rkw) if pcm16 else self.decode_to_wavs(src, use_decoder, **rkw)
                    result.destroy()
                    yield wavs
                    continue
                if last is not None:
                    last.destroy()
                last = result
                pass_batch_count += 1
                if pass_batch_count <= params_infer_code.pass_first_n_batches:
                    continue     # the reference decodes these yields and drops the audio (core.py:482-490)
                src = result.hiddens if use_decoder else result.ids
                piece, fs = piece_of(src, length, length + params_infer_code.stream_speed, False)
                if filed and not rowwise:
                    piece = flac_chunks(piece, False, fs)
                # core.py:491-496: `b = a + stream_speed`, clamped to the width of THIS decode, becomes the new `length` -- also when
                # that is BELOW `a`: `length` and `pass_batch_count` are not reset between split batches, so the first yields of a
                # later batch (a short prefix again) are empty and pull `length` back (tests/test_host_flow.py, stream_split_batches)
                # (the decode width of a T-token prefix is 256 (2 T - 1) samples on both decode paths; never negative for an empty yield)
                length = min(length + params_infer_code.stream_speed, max(0, 256 * (2 * max(int(r.size(0)) for r in src) - 1)))
                yield piece
            if stream and last is not None and rowwise:      # rows of different lengths: filtered and converted row by row
                tail, _ = piece_of(last.hiddens, length, None, True)
                last.destroy()
                yield tail
                continue
            if stream and last is not None:
                new_wavs, fs = piece_of(last.hiddens if use_decoder or scaled else last.ids, length, None, True)
                last.destroy()
                keep_cols = np.sum(np.abs(new_wavs) > 1e-5, axis=0) > 0
                tail = new_wavs[:, keep_cols]
                # the last chunk is filtered by columns on the float samples first (core.py:500-503): converted on the host, row by row
                if pcm16:     # int16 like every other chunk of the stream, also when nothing survives the column filter
                    tail = np.stack([float_to_int16(r) for r in tail]) if tail.shape[1] else tail.astype(np.int16)
                    if encoding is not None:      # companded by the host twin, like the conversion in front of it
                        tail = G711.encode(tail, encoding)
                    if filed:                     # the streams' last push: what they held leaves with it
                        tail = flac_chunks(tail, True, fs)
                yield tail

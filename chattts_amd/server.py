"""OpenAI-compatible speech endpoint on top of `Chat` (the last open piece of the host back end): the behaviour of the
reference's `examples/api/openai_api.py` -- `POST /v1/audio/speech` with the OpenAI TTS request fields, `GET /health`, a lock around the
model, WAV streaming with an open-ended RIFF header -- re-stated for this engine (reference lines cited per function; nothing is imported
from it).  What differs, deliberately:
  * the 16-bit conversion (`float_to_int16`, tools/audio/np.py:7-11, called by tools/audio/pcm.py:8-33,92-93) runs ON THE DEVICE
    (`Chat.infer(..., pcm16=True)`, csrc/codec.hip pcm16_k): the waveform crosses PCIe as int16, the bytes are the reference's bit for bit;
  * generation runs in a worker thread (starlette's thread pool), so the event loop keeps serving `/health` and other requests queue on the
    lock instead of on a blocked loop; the lock is held until a streamed response has been fully produced (the reference releases it before
    the generator is consumed, openai_api.py:211-224,265-276);
  * `response_format`: "wav" and "pcm" (raw little-endian PCM16, the OpenAI API's own name for it) always; "mp3" / "ogg" go through PyAV in
    the reference (tools/audio/av.py) and are offered only where `av` imports -- elsewhere they are refused with a 400 that says so.

    from chattts_amd.core import Chat
    from chattts_amd.server import create_app
    chat = Chat(); chat.load(custom_path=..., dtype="bf16")
    app = create_app(chat, voices={"default": spk_emb_string})        # uvicorn.run(app, ...)

`create_app(..., batch_slots=N)` serves concurrent non-streamed requests in ONE batch: a worker thread owns a slot pool of N utterance
slots with per-request sampling parameters (serving.SpeechBatcher, serving.SlotPool(per_request=True)), so eight clients share the chip
instead of queueing for it.  Every response is what the serial endpoint returns for the same request (the same tokens; PCM within one
count).  Streamed requests keep the serial path (a threading lock keeps them and the worker from issuing GPU work at the same time) unless
`batch_streams=True`: then they are served from the same pool, their chunks decoded together (serving.SpeechBatcher.submit_stream).
"""
from __future__ import annotations

import asyncio
import io
import logging
import threading
import wave
from typing import Dict, Optional

import numpy as np

from .audio import g711_to_wav_bytes

try:        # the upload route's parameter type: annotations of this module are resolved against its globals
    from starlette.requests import Request
except ImportError:      # create_app raises on its own fastapi import
    Request = None

ALLOWED_PARAMS = {"model", "input", "voice", "response_format", "speed", "stream", "output_format"}    # openai_api.py:97-105
SAMPLE_RATE = 24000


def wav_stream_header(sample_rate: int = SAMPLE_RATE, bits_per_sample: int = 16, channels: int = 1) -> bytes:
    """openai_api.py:226-243: a RIFF/WAVE header whose two length fields are 0xFFFFFFFF (the length of a stream is not known)"""
    byte_rate = sample_rate * channels * bits_per_sample // 8
    block_align = channels * bits_per_sample // 8
    return (b"RIFF" + b"\xff\xff\xff\xff" + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little")
            + channels.to_bytes(2, "little") + sample_rate.to_bytes(4, "little") + byte_rate.to_bytes(4, "little")
            + block_align.to_bytes(2, "little") + bits_per_sample.to_bytes(2, "little") + b"data" + b"\xff\xff\xff\xff")


def g711_wav_stream_header(law, sample_rate: int = 8000) -> bytes:
    """`wav_stream_header` for a G.711 stream: WAVE_FORMAT_MULAW / WAVE_FORMAT_ALAW, mono, 8 bits, an 18-byte `fmt ` chunk and a `fact` chunk, with
    0xFFFFFFFF in the RIFF, `fact` and `data` lengths (audio.g711_wav_header)"""
    from .audio import g711_wav_header
    return g711_wav_header(law, sample_rate, None)


def pcm16_to_wav_bytes(pcm: np.ndarray, sample_rate: int = SAMPLE_RATE) -> bytes:
    """tools/audio/pcm.py:8-33 for samples that are already int16: mono 16-bit RIFF/WAVE"""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(sample_rate)
        wf.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())
    return buf.getvalue()


def _av_encode(pcm: np.ndarray, fmt: str, sample_rate: int = SAMPLE_RATE) -> bytes:
    """tools/audio/av.py: WAV bytes -> mp3 / ogg through PyAV (absent in the build container: only reached where `av` imports)"""
    import av
    src = av.open(io.BytesIO(pcm16_to_wav_bytes(pcm, sample_rate)), "r")
    out_buf = io.BytesIO()
    out = av.open(out_buf, "w", format=fmt)
    stream = out.add_stream({"mp3": "mp3", "ogg": "libvorbis"}[fmt], rate=sample_rate)
    for frame in src.decode(audio=0):
        for p in stream.encode(frame):
            out.mux(p)
    for p in stream.encode(None):
        out.mux(p)
    out.close()
    src.close()
    return out_buf.getvalue()


def _have_av() -> bool:
    import importlib.util
    return importlib.util.find_spec("av") is not None


def create_app(chat, voices: Optional[Dict[str, str]] = None, logger: Optional[logging.Logger] = None, infer_kwargs: Optional[dict] = None,
               batch_slots: Optional[int] = None, batcher=None, ragged_decode: bool = False, batch_streams: bool = False,
               batch_refine: bool = False, refine_params=None, batch_split: bool = False, sample_rates=None, voice_upload: bool = False,
               stream_sample_rates=None, g711: bool = False, speed: bool = False, stream_speed: bool = False,
               stream_speed_rates: bool = False, flac: bool = False, loudness: bool = False, stream_flac: bool = False,
               pauses: bool = False, limiter: bool = False, stream_limiter: bool = False, stream_pauses: bool = False,
               adpcm: bool = False, stream_adpcm: bool = False, compress: bool = False, stream_compress: bool = False,
               eq: bool = False):
    """FastAPI app serving `chat` (a loaded `chattts_amd.core.Chat`).  `voices`: OpenAI voice name -> `spk_emb` string
    (`Chat.sample_random_speaker()` / the reference's speaker files); an unknown voice falls back to "default" like openai_api.py:165.
    `infer_kwargs`: extra keywords for every serial `chat.infer` call (tests).  `batch_slots`: None = one request at a time (the
    reference's behaviour); N = non-streamed requests are batched in a pool of N slots (serving.SpeechBatcher; `batcher`: a ready one,
    tests).  `ragged_decode` (batching only): the requests that finish together are decoded in one ragged pass, each as if alone,
    instead of one decode per request (SpeechBatcher(ragged_decode=True)).  `batch_streams` (batching only; off: every path is as
    without it): a request with `"stream": true` joins the pool too (SpeechBatcher.submit_stream) instead of taking `model_lock` and
    running as a batch of one -- concurrent streams advance together, the chunks that are due at one poll come from one decoder pass,
    and a client that goes away cancels its request.  `batch_refine` (batching only; off: every path is as without it): a request body
    may carry `"refine_text": true` -- the reference's default two-stage call: its text goes through the batcher's text-mode pool first
    (SpeechBatcher(refine=True)), with `refine_params` (a `RefineTextParams`, or a callable returning one; default
    `RefineTextParams(show_tqdm=False, manual_seed=42)`, a fixed seed like the code stage's), and the refined text is what is
    synthesised.  It applies to the requests the pool serves (non-streamed ones, streamed ones with `batch_streams`); without
    `batch_refine` the key is ignored with the "unsupported parameters" warning, like any unknown key.  `batch_split` (batching only; off:
    every path is as without it): a non-streamed request body may carry `"split_text": true` -- the reference's default handling of a long
    input: the text is cut into sentences that run side by side in the pool under one voice (SpeechBatcher.submit(split_text=True));
    with `"stream": true` the key is ignored with a warning.  A `voices` value may also be a dict `{"spk_emb"?, "spk_smp"?, "txt_smp"?}`
    (a plain string means `spk_emb`): a cloned voice -- with it a split request needs no refer sentence.  `sample_rates` (default None:
    every path is as without it, a `"sample_rate"` key is ignored with the "unsupported parameters" warning): the rates a non-streamed
    request body may ask for with `"sample_rate"`, e.g. (8000, 16000, 24000, 44100, 48000) -- the audio is resampled on the device
    (Chat.infer(sample_rate=) / SpeechBatcher.submit(sample_rate=)) and the WAV header carries the rate; another rate, or a rate other
    than 24000 with `"stream": true`, gets a 400 -- unless `stream_sample_rates` (default None: every path is as without it) holds it: the
    rates a STREAMED request body may ask for.  Such a stream's chunks are their ranges of the resampled decode (Chat.infer(stream=True,
    sample_rate=, stream_resample=True); with `batch_streams` SpeechBatcher.submit_stream(sample_rate=), the chunks of streams at
    different rates still share one decoder pass) and the open-ended WAV header carries the rate.  `voice_upload=True` adds
    `POST /v1/audio/voices?name=NAME[&text=TRANSCRIPT]`, whose body is a WAV file (8/16/32-bit PCM, any rate, any channel count): the clip
    is resampled to 24 kHz on the device and encoded (Chat.sample_audio_speaker(wav, rate)) under the GPU lock, and NAME becomes a cloned
    voice of this app.  `g711=True` (default off: every response, status and warning is as without it): telephony output.
    `response_format` "ulaw" / "alaw" returns raw headerless G.711 bytes, one per sample, like "pcm" (media types audio/PCMU /
    audio/PCMA); "wav" with a body key `"encoding": "ulaw" | "alaw"` returns a WAVE_FORMAT_MULAW / WAVE_FORMAT_ALAW file (a stream: its
    open-ended form); another `"encoding"` value gets a 400.  The companding runs on the device behind the 16-bit conversion
    (Chat.infer(encoding=) / SpeechBatcher.submit(encoding=) / submit_stream(encoding=)); the rate is whatever `sample_rates` /
    `stream_sample_rates` allow -- 8000 is the telephone's.  With `voice_upload`, mu-law / A-law WAV clips are accepted too
    (audio.load_wav(g711=True)).  `speed=True` (default off: the body's `"speed"` is validated to lie in 0.5 .. 2.0 and then ignored, like
    the reference does): a non-streamed request is served at its `"speed"` -- the same utterance at the same pitch, time-scaled on the
    device behind the decode (Chat.infer(speed=) / SpeechBatcher.submit(speed=)); a speed other than 1.0 with `"stream": true` gets a 400
    -- unless `stream_speed=True` (with `speed`; default off): then a streamed request is served at its speed too, the time scaler's path
    carried across its chunks on the device -- from the pool with `batch_streams` (SpeechBatcher(stream_speeds=True).submit_stream(speed=)),
    serially otherwise (Chat.infer(stream=True, speed=, stream_time_scale=True)); a streamed speed at a rate other than 24000 gets a 400 -- unless
    `stream_speed_rates=True` (with `speed`, `stream_speed` and the rate in `stream_sample_rates`; default off): then such a request is
    served, the scaled stream resampled with the filter's history and look-ahead carried on the device -- from the pool when it can take
    it (SpeechBatcher(stream_speeds=True, stream_speed_rates=True).submit_stream(speed=, sample_rate=)), serially otherwise
    (Chat.infer(..., stream_time_scale=True, stream_resample=True, stream_scaled_resample=True)); with `g711`, companded too.
    `flac=True` (default off: every response, status, warning and /health list is as without it): `response_format` "flac" returns the
    request's 16-bit samples as a FLAC file (audio/flac; lossless: the samples of the "wav" response, bit for bit), encoded on the device
    behind the 16-bit conversion (Chat.infer(flac=True) / SpeechBatcher.submit(flac=True)), at whatever rate and speed `sample_rates` /
    `speed` allow.  `"stream": true` with it gets a 400 (a streamed FLAC needs a variable-block-size stream and carried sample numbers),
    an `"encoding"` key with it too -- unless `stream_flac=True` (with `flac`; default off): then a streamed request with
    `response_format` "flac" is served as audio/flac: `flac.stream_header(rate)` (STREAMINFO with blocks of 16 .. 4096 samples, the total
    unknown) in front of the first chunk, then every chunk's frames as they are completed -- variable-block-size frames that carry the
    number of their first sample, at most 15 samples behind the PCM stream of the same request, whose samples they decode to bit for
    bit; from the pool with `batch_streams` (SpeechBatcher(stream_flac=True).submit_stream(flac=True)), serially otherwise
    (Chat.infer(stream=True, flac=True, stream_flac=True)), at whatever streamed rate and speed the other options allow, and /health
    carries `"stream_flac": true`.  `loudness=True` (default off: every response, status and warning is as without it, a `"loudness"`
    key is ignored with the "unsupported parameters" warning): a non-streamed request body may carry `"loudness"`, a target in LUFS
    (-40 .. -5) -- the utterance is brought to that ITU-R BS.1770-4 integrated loudness on the device, under a +30 dB cap and a -1 dBFS
    ceiling, in front of the 16-bit conversion (Chat.infer(loudness=) / SpeechBatcher.submit(loudness=)), in whatever format, rate and
    speed the other options allow; a value that is no number or out of range gets a 400, `"stream": true` with it too (an integrated
    loudness needs the whole utterance), and /health carries `"loudness": true`.  `pauses=True` (default off: every response, status,
    warning and /health list is as without it, a `"pauses"` key is ignored with the "unsupported parameters" warning): a non-streamed
    request body may carry `"pauses"`: true (the defaults) or an object with any of `max_pause_ms`, `lead_ms`, `tail_ms`,
    `threshold_db`, `pad_ms` (chattts_amd/pauses.py) -- the silence in front of and behind the utterance is trimmed and its long pauses
    are capped on the device, in front of the loudness stage and the 16-bit conversion (Chat.infer(pauses=) /
    SpeechBatcher.submit(pauses=)), in whatever format, rate and speed the other options allow; false or null leaves the audio alone;
    a wrong type, an unknown field or a value out of range gets a 400, `"stream": true` with it too (the run state is not carried
    across chunks), and /health carries `"pauses": true`.  `limiter=True` (default off: every response, status, warning and /health
    body is as without it, a `"limiter"` key is ignored with the "unsupported parameters" warning): a non-streamed request body may
    carry `"limiter": true`, with or without `"loudness"` -- the look-ahead peak limiter (chattts_amd/limiter.py) runs on the device
    behind the loudness stage's gain, which then drops its ceiling term, or at unity gain (Chat.infer(limiter=) /
    SpeechBatcher.submit(limiter=)): no sample exceeds -1 dBFS and one loud peak no longer decides the level; false or null leaves
    the audio alone; a value that is no boolean gets a 400, `"stream": true` with it too (the look-ahead is not carried across
    chunks), and /health carries `"limiter": true` -- unless `stream_limiter=True` (with `limiter`; default off): then a body with
    `"stream": true, "limiter": true` is served, every chunk converted from samples that went through the request's limiter stream, 20 ms
    behind (chattts_amd/limiter.py, the stream) -- from the pool with `batch_streams` when it can take it
    (SpeechBatcher(stream_limiter=True).submit_stream(limiter=True)), serially otherwise (Chat.infer(stream=True, limiter=True,
    stream_limiter=True)), with whatever streamed rate, speed and format the other options allow; such a body may also carry
    `"gain_db"`, a fixed make-up gain of -30 .. +30 dB in front of the limiter (a bad value, or the key without `"stream": true` and
    `"limiter": true`, gets a 400), and /health carries `"stream_limiter": true`.  `stream_pauses=True` (with `pauses`; default off): a
    body with `"stream": true` and `"pauses"` is served too -- every stream gets a pause stream on the device that carries the run
    state across chunks (chattts_amd/pauses.py: the schedule and the lags), from the pool where the batcher was built with
    `stream_pauses=True`, serially otherwise (Chat.infer(stream=True, pauses=, stream_pauses=True)); a spec that would make a stream
    hold more frames than a slot has gets a 400, chunks that come out empty are not written, and /health carries
    `"stream_pauses": true`.  `adpcm=True` (default off: every response, status, warning and /health list is as without it):
    `response_format` "adpcm" returns the request's 16-bit samples as a WAVE_FORMAT_IMA_ADPCM file (audio/wav; 4 bits per sample, mono:
    half of G.711's size, chattts_amd/adpcm.py), encoded on the device behind the 16-bit conversion (Chat.infer(adpcm=True) /
    SpeechBatcher.submit(adpcm=True)), at whatever rate, speed, loudness, pauses and limiter the other options allow; `"stream": true`
    with it gets a 400 (a streamed file would carry up to a block's samples across chunks), an `"encoding"` key with it too.  With
    `voice_upload`, mono IMA ADPCM WAV clips are accepted too (audio.load_wav(adpcm=True)).  `stream_adpcm=True` (with
    `adpcm`; default off) lifts that 400: a streamed request with `response_format` "adpcm" is served as audio/wav: `adpcm.stream_header(rate)`
    (the file's header with 0xFFFFFFFF in the RIFF, `fact` and `data` lengths), then the whole blocks each chunk completes; empty
    chunks are not written.  The blocks are those of the non-streamed file over the same samples; a reader of the open-ended file
    cannot know the true length and decodes up to a block's worth of padded samples behind the last real one.  It is served from the
    pool with `batch_streams` (SpeechBatcher(stream_adpcm=True).submit_stream(adpcm_blocks=True)), serially otherwise
    (Chat.infer(stream=True, adpcm=True, stream_adpcm=True)), at the rates `stream_sample_rates` allows (below 55125 Hz), and
    /health carries `"stream_adpcm": true`.  `compress=True` (default off: every response, status, warning and /health list is as
    without it, a `"compress"` key is ignored with the "unsupported parameters" warning): a non-streamed request body may carry
    `"compress"`: true (the defaults) or an object with any of `threshold_db`, `ratio`, `knee_db`, `attack_ms`, `hold_ms`
    (chattts_amd/compressor.py) -- the utterance goes through the look-ahead compressor on the device, behind `pauses` and in front of
    the loudness stage, the limiter and the 16-bit conversion (Chat.infer(compress=) / SpeechBatcher.submit(compress=)), in whatever
    format, rate and speed the other options allow; false or null leaves the dynamics alone; a bad spec gets a 400 with the
    validator's message; `"stream": true` with it gets a 400 (a compressed stream would need the block state carried across chunks),
    and /health carries `"compress": true`.  `stream_compress=True` (with `compress`; default off): a body with `"stream": true` and
    `"compress"` is served -- the stream's chunks come out of a compressor stream that carries the hold's block gains and the few
    unemitted samples across chunks (CodecEngine.compress_stream_*), the attack and at most two milliseconds behind -- from the pool where
    `batch_streams` allows it and the batcher was built with `stream_compress=True`, serially otherwise (Chat.infer(stream=True,
    compress=, stream_compress=True)); /health carries `"stream_compress": true`.  `eq=True` (default off: every response, status,
    warning and /health list is as without it, an `"eq"` key is ignored with the "unsupported parameters" warning): a non-streamed
    request body may carry `"eq"`: a preset name ("telephone", "rumble") or an object with any of `highpass_hz`, `lowshelf` {hz, db},
    `highshelf` {hz, db}, `peaks` [{hz, db, q}, ...], at most four sections (chattts_amd/equalizer.py) -- the utterance goes through the
    biquad cascade on the device, behind `pauses` and in front of the compressor, the loudness stage, the limiter and the 16-bit
    conversion (Chat.infer(eq=) / SpeechBatcher.submit(eq=)), in whatever format, rate and speed the other options allow; false or
    null leaves the spectrum alone; a bad spec (a frequency above 0.45 of the request's rate too) gets a 400 with the validator's
    message; `"stream": true` with it gets a 400 (an equalised stream would need the filter state carried across chunks), and
    /health carries `"eq": true`."""
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import JSONResponse, Response, StreamingResponse
    from pydantic import BaseModel, Field, ValidationError
    from starlette.concurrency import iterate_in_threadpool, run_in_threadpool

    log = logger or logging.getLogger("chattts_amd.server")
    voices = dict(voices or {})
    extra = dict(infer_kwargs or {})
    app = FastAPI()
    app.state.chat = chat
    app.state.model_lock = asyncio.Lock()            # openai_api.py:66
    gpu_lock = threading.Lock()                      # batching: the worker's chunks / decodes vs the streamed path's chunks
    if batcher is None and batch_slots is not None:
        from .serving import SpeechBatcher
        batcher = SpeechBatcher(chat, int(batch_slots), gpu_lock, logger=log, ragged_decode=ragged_decode, streams=bool(batch_streams),
                                **({"refine": True} if batch_refine else {}), **({"stream_speeds": True} if speed and stream_speed else {}),
                                **({"stream_speed_rates": True} if speed and stream_speed and stream_speed_rates else {}),
                                **({"stream_flac": True} if flac and stream_flac else {}),
                                **({"stream_limiter": True} if limiter and stream_limiter else {}),
                                **({"stream_pauses": True} if pauses and stream_pauses else {}),
                                **({"stream_adpcm": True} if adpcm and stream_adpcm else {}),
                                **({"stream_compress": True} if compress and stream_compress else {}))
    if batcher is not None:
        gpu_lock = batcher.lock
    app.state.batcher = batcher
    pool_streams = bool(batch_streams) and batcher is not None and bool(getattr(batcher, "streams", False))
    pool_stream_speeds = pool_streams and bool(speed and stream_speed) and bool(getattr(batcher, "stream_speeds", False))
    speed_rates = bool(speed and stream_speed and stream_speed_rates)
    pool_stream_speed_rates = pool_stream_speeds and speed_rates and bool(getattr(batcher, "stream_speed_rates", False))
    flac_streams = bool(flac and stream_flac)
    pool_stream_flac = pool_streams and flac_streams and bool(getattr(batcher, "stream_flac", False))
    adpcm_streams = bool(adpcm and stream_adpcm)
    pool_stream_adpcm = pool_streams and adpcm_streams and bool(getattr(batcher, "stream_adpcm", False))
    limiter_streams = bool(limiter and stream_limiter)
    pool_stream_limiter = pool_streams and limiter_streams and bool(getattr(batcher, "stream_limiter", False))
    pause_streams = bool(pauses and stream_pauses)
    pool_stream_pauses = pool_streams and pause_streams and bool(getattr(batcher, "stream_pauses", False))
    compress_streams = bool(compress and stream_compress)
    pool_stream_compress = pool_streams and compress_streams and bool(getattr(batcher, "stream_compress", False))
    pool_refine = bool(batch_refine) and batcher is not None and bool(getattr(batcher, "refine", False))
    pool_split = bool(batch_split) and batcher is not None
    allowed = ALLOWED_PARAMS | ({"refine_text"} if pool_refine else set()) | ({"split_text"} if pool_split else set())
    rates_ok = None if sample_rates is None else {int(r) for r in sample_rates}
    stream_rates_ok = None if stream_sample_rates is None else {int(r) for r in stream_sample_rates}
    if rates_ok is not None or stream_rates_ok is not None:
        allowed = allowed | {"sample_rate"}

    def voice_token_room():
        """how many audio-prompt tokens of a cloned voice fit a pool slot beside a prompt: the pool admits a request when prompt +
        max_new_token + 1 + 2 POLL <= cap (SlotPool.submit); 64 tokens are left for a short text and its decoration.  None without a
        pool (the serial path has no slot)."""
        pool = getattr(batcher, "pool", None)
        cap = getattr(pool, "cap", None)
        if cap is None:
            return None
        return max(0, int(cap) - int(code_params(None).max_new_token) - 1 - 2 * int(getattr(pool, "POLL", 0)) - 64)

    def refine_of(request_data):         # the refine stage's parameters of a request that asks for it, or None
        if not (pool_refine and bool(request_data.get("refine_text", False))):
            return None
        if refine_params is None:
            return chat.RefineTextParams(show_tqdm=False, manual_seed=42)
        return refine_params() if callable(refine_params) else refine_params

    def locked_chunks(gen):
        """one chunk of a streamed response at a time under the GPU lock (batching on): the worker's chunks interleave with these"""
        while True:
            with gpu_lock:
                try:
                    chunk = next(gen)
                except StopIteration:
                    return
            yield chunk
    formats = {"wav", "pcm"} | ({"mp3", "ogg"} if _have_av() else set()) | ({"ulaw", "alaw"} if g711 else set())
    if g711:
        allowed = allowed | {"encoding"}
    if flac:
        from . import flac as FLAC
        formats = formats | {"flac"}
    if adpcm:
        from . import adpcm as ADPCM
        formats = formats | {"adpcm"}
    if loudness:
        from . import loudness as LN
        allowed = allowed | {"loudness"}
    if pauses:
        from . import pauses as PA
        allowed = allowed | {"pauses"}
    if limiter:
        from . import loudness as LN
        allowed = allowed | {"limiter"}
    if limiter_streams:
        from . import limiter as LM
        allowed = allowed | {"gain_db"}
    if compress:
        from . import compressor as CP
        from . import loudness as LN
        allowed = allowed | {"compress"}

    if eq:
        from . import equalizer as EQ
        allowed = allowed | {"eq"}

    class SpeechRequest(BaseModel):                  # openai_api.py:108-127
        model: str = "tts-1"
        input: str = Field(..., max_length=2048)
        voice: Optional[str] = "default"
        response_format: Optional[str] = "wav" if "mp3" not in formats else "mp3"
        speed: Optional[float] = Field(1.0, ge=0.5, le=2.0)
        stream: Optional[bool] = False
        output_format: Optional[str] = None

    @app.exception_handler(Exception)
    async def on_error(request, exc):                # openai_api.py:141-149: one error shape
        log.error("error: %s", exc)
        return JSONResponse(status_code=getattr(exc, "status_code", 500), content={"error": {"message": str(exc), "type": exc.__class__.__name__}})

    def code_params(voice: Optional[str]):           # openai_api.py:185-205, field for field
        v = voices.get(voice, voices.get("default"))
        v = v if isinstance(v, dict) else {"spk_emb": v}      # a plain string: the speaker embedding; a dict: a cloned voice's fields too
        return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                    min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42,
                                    spk_emb=v.get("spk_emb"), spk_smp=v.get("spk_smp"), txt_smp=v.get("txt_smp"), stream_batch=24,
                                    stream_speed=12000, pass_first_n_batches=2)

    def infer(req: "SpeechRequest", rate: int = SAMPLE_RATE, law: Optional[str] = None, spd: Optional[float] = None,
              as_flac: bool = False, lufs: Optional[float] = None, trim=None, lim: bool = False, gdb=None,
              as_adpcm: bool = False, comp=None, tone=None):                        # openai_api.py:168-183,207-222
        kw = dict(extra) if rate == SAMPLE_RATE else {**extra, "sample_rate": rate}
        if tone is not None:
            kw = {**kw, "eq": tone}
        if comp is not None:
            kw = {**kw, "compress": comp}
        if lim:
            kw = {**kw, "limiter": True}
        if trim is not None:
            kw = {**kw, "pauses": trim}
        if lufs is not None:
            kw = {**kw, "loudness": lufs}
        if as_flac:
            kw = {**kw, "flac": True}
        if as_adpcm:
            kw = {**kw, "adpcm": True}
        if spd is not None:
            kw = {**kw, "speed": spd}
        if law is not None:
            kw = {**kw, "encoding": law}
        if req.stream and rate != SAMPLE_RATE:       # one text: split_text changes nothing but is refused for a stream at another rate
            kw = {**kw, "stream_resample": True, "split_text": False}
        if req.stream and as_flac:                   # likewise for a streamed FLAC
            kw = {**kw, "stream_flac": True, "split_text": False}
        if req.stream and as_adpcm:                  # ... and for a streamed ADPCM file
            kw = {**kw, "stream_adpcm": True, "split_text": False}
        if req.stream and spd is not None:           # likewise for a stream at another speed
            kw = {**kw, "stream_time_scale": True, "split_text": False}
            if rate != SAMPLE_RATE:                  # ... and another rate: the resampler's history and look-ahead are carried
                kw = {**kw, "stream_scaled_resample": True}
        if req.stream and lim:                       # likewise for a limited stream
            kw = {**kw, "stream_limiter": True, "split_text": False, **({} if gdb is None else {"gain_db": gdb})}
        if req.stream and trim is not None:          # likewise for a paused stream
            kw = {**kw, "stream_pauses": True, "split_text": False}
        if req.stream and comp is not None:          # likewise for a compressed stream
            kw = {**kw, "stream_compress": True, "split_text": False}
        return chat.infer(text=[req.input], stream=bool(req.stream), lang=None, skip_refine_text=True, refine_text_only=False,
                          use_decoder=True, do_text_normalization=True, do_homophone_replacement=True,
                          params_infer_code=code_params(req.voice), pcm16=True, **kw)

    @app.post("/v1/audio/speech")
    async def speech(request_data: Dict):
        unknown = set(request_data) - allowed                                 # openai_api.py:130-138
        if unknown:
            log.warning("ignoring unsupported parameters: %s", sorted(unknown))
        data = {k: request_data[k] for k in ALLOWED_PARAMS if k in request_data}
        data["model"] = "tts-1"
        try:
            req = SpeechRequest(**data)
        except ValidationError as e:
            raise HTTPException(422, detail=str(e))
        fmt = req.response_format
        if fmt not in formats:
            hint = " (mp3 / ogg need PyAV, which is not installed here)" if fmt in ("mp3", "ogg") else ""
            raise HTTPException(400, detail=f"Unsupported audio format: {fmt}, supported formats: {', '.join(sorted(formats))}{hint}")
        rate = SAMPLE_RATE
        if (rates_ok is not None or stream_rates_ok is not None) and request_data.get("sample_rate") is not None:
            try:
                rate = int(request_data["sample_rate"])
            except (TypeError, ValueError):
                rate = -1
            if req.stream and stream_rates_ok is not None and rate in stream_rates_ok:
                pass                                 # a stream at this rate is served
            elif rates_ok is None and not req.stream:
                log.warning("ignoring unsupported parameters: ['sample_rate']")       # only streams were given rates: as without the key
                rate = SAMPLE_RATE
            elif rates_ok is not None and rate not in rates_ok:
                raise HTTPException(400, detail=f"Unsupported sample_rate: {request_data['sample_rate']}, supported: "
                                                f"{', '.join(str(r) for r in sorted(rates_ok))}")
            elif req.stream and rate != SAMPLE_RATE:
                raise HTTPException(400, detail=f"sample_rate {rate} is served for non-streamed requests only: a stream's chunks are "
                                                f"produced at {SAMPLE_RATE} Hz (the resampling filter's state is not carried across chunks)")
        spd = None                                   # the request's speed where it is honoured and is not 1.0
        if speed and req.speed is not None and int(round(100.0 * req.speed)) != 100:
            if req.stream and not stream_speed:
                raise HTTPException(400, detail=f"speed {req.speed} is served for non-streamed requests only: a stream's chunks are "
                                                f"produced at speed 1.0 (the time scaler's path is not carried across chunks)")
            if req.stream and rate != SAMPLE_RATE and not speed_rates:
                raise HTTPException(400, detail=f"a streamed speed is served at {SAMPLE_RATE} Hz only: speed {req.speed} with sample_rate {rate} "
                                                f"would need the scaled stream's history and a look-ahead carried into the resampler")
            spd = int(round(100.0 * req.speed)) / 100
        lufs = None                                  # the request's loudness target where it is honoured
        if loudness and request_data.get("loudness") is not None:
            try:
                lufs = LN.check_target(request_data["loudness"])
                LN.check_rate(rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
            if req.stream:
                raise HTTPException(400, detail=f"loudness {lufs} is served for non-streamed requests only: an integrated loudness needs "
                                                f"the whole utterance (a stream would need a running measure)")
        trim = None                                  # the request's pause spec where it is honoured
        if pauses and request_data.get("pauses") is not None and request_data["pauses"] is not False:
            spec = request_data["pauses"]
            if spec is not True and not isinstance(spec, dict):
                raise HTTPException(400, detail=f"pauses is true or an object with any of {', '.join(PA.RANGES)} (got {spec!r})")
            try:
                trim = PA.check(spec)
                PA.check_rate(rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
            if req.stream and not pause_streams:
                raise HTTPException(400, detail="pauses is served for non-streamed requests only: a stream would need the run state "
                                                "carried across chunks")
            if req.stream:
                try:
                    PA.check_stream(rate, trim)
                except ValueError as e:
                    raise HTTPException(400, detail=str(e))
        comp = None                                  # the request's compressor spec where it is honoured
        if compress and request_data.get("compress") is not None and request_data["compress"] is not False:
            try:
                comp = CP.check(request_data["compress"], "compress")
                LN.check_rate(rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
            if req.stream and not compress_streams:
                raise HTTPException(400, detail="compress is served for non-streamed requests only: a compressed stream would need the "
                                                "block state carried across chunks")
        tone = None                                  # the request's equaliser spec where it is honoured
        if eq and request_data.get("eq") is not None and request_data["eq"] is not False:
            try:
                tone = EQ.check(request_data["eq"], "eq", rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
            if tone is not None and req.stream:
                raise HTTPException(400, detail="eq is served for non-streamed requests only: an equalised stream would need the filter "
                                                "state carried across chunks")
        lim = False                                  # the request's limiter flag where it is honoured
        if limiter and request_data.get("limiter") is not None:
            if not isinstance(request_data["limiter"], bool):
                raise HTTPException(400, detail=f"limiter is true or false (got {request_data['limiter']!r})")
            lim = request_data["limiter"]
            if lim:
                try:
                    LN.check_rate(rate)
                except ValueError as e:
                    raise HTTPException(400, detail=str(e))
                if req.stream and not limiter_streams:
                    raise HTTPException(400, detail="limiter is served for non-streamed requests only: the look-ahead is not carried "
                                                    "across chunks")
        gdb = None                                   # the request's make-up gain in dB where it is honoured
        if limiter_streams and request_data.get("gain_db") is not None:
            if not (lim and req.stream):
                raise HTTPException(400, detail='gain_db is the make-up gain of a limited stream: it goes with "stream": true and "limiter": true')
            try:
                LM.check_gain_db(request_data["gain_db"])
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
            gdb = float(request_data["gain_db"])
        refine = refine_of(request_data)
        rkw = {} if refine is None else {"refine": refine}
        if refine is not None and req.stream and not pool_streams:
            log.warning("refine_text is served by the batched path only: ignored for a serially streamed request")
        if pool_split and bool(request_data.get("split_text", False)):
            if req.stream:
                log.warning("split_text is served for non-streamed requests only: ignored for a streamed request")
            else:
                rkw = {**rkw, "split_text": True}
        law = None                                   # G.711: the engine hands out uint8 codes
        if g711:
            law = fmt if fmt in ("ulaw", "alaw") else None
            enc = request_data.get("encoding")
            if enc is not None:
                if enc not in ("ulaw", "alaw") or (law is not None and enc != law):
                    raise HTTPException(400, detail=f"Unsupported encoding: {enc}, supported: alaw, ulaw")
                if fmt not in ("wav", "ulaw", "alaw"):
                    raise HTTPException(400, detail=f"encoding {enc} goes with response_format wav, ulaw or alaw, not {fmt}")
                law = enc
        as_flac = bool(flac) and fmt == "flac"       # the engine hands out the file
        if as_flac:
            if req.stream and not flac_streams:
                raise HTTPException(400, detail="flac is served for non-streamed requests only: a streamed FLAC needs a variable-block-size "
                                                "stream and carried sample numbers")
            if request_data.get("encoding") is not None:
                raise HTTPException(400, detail=f"encoding {request_data['encoding']} does not go with response_format flac (a FLAC file "
                                                f"holds the 16-bit samples)")
            try:
                FLAC.rate_code(rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
        as_adpcm = bool(adpcm) and fmt == "adpcm"    # likewise
        if as_adpcm:
            if req.stream and not adpcm_streams:
                raise HTTPException(400, detail="adpcm is served for non-streamed requests only: a streamed ADPCM file would carry up to "
                                                "a block's samples across chunks")
            if req.stream and rate >= 55125:
                raise HTTPException(400, detail=f"a streamed ADPCM file is served below 55125 Hz (a stream keeps up to 2048 samples of an "
                                                f"open block), not at {rate} Hz")
            if request_data.get("encoding") is not None:
                raise HTTPException(400, detail=f"encoding {request_data['encoding']} does not go with response_format adpcm (an ADPCM "
                                                f"file is coded from the 16-bit samples)")
            try:
                ADPCM.check_rate(rate)
            except ValueError as e:
                raise HTTPException(400, detail=str(e))
        akw = {"as_adpcm": True} if as_adpcm else {}
        media = {"wav": "audio/wav", "pcm": "audio/pcm", "mp3": "audio/mpeg", "ogg": "audio/ogg", "ulaw": "audio/PCMU", "alaw": "audio/PCMA",
                 "flac": "audio/flac", "adpcm": "audio/wav"}[fmt]
        ekw = {"adpcm": True} if as_adpcm else ({} if law is None else {"encoding": law}) if not as_flac else {"flac": True}
        stream_header = wav_stream_header if law is None else (lambda r: g711_wav_stream_header(law, r))

        def encode(pcm: np.ndarray, header: bool) -> bytes:
            if as_flac or as_adpcm:
                return np.ascontiguousarray(np.asarray(pcm).reshape(-1), dtype=np.uint8).tobytes()
            if law is not None:
                codes = np.ascontiguousarray(np.asarray(pcm).reshape(-1), dtype=np.uint8)
                return g711_to_wav_bytes(codes, law, rate) if (fmt == "wav" and header) else codes.tobytes()
            pcm = np.ascontiguousarray(np.asarray(pcm).reshape(-1), dtype="<i2")
            if fmt == "wav":
                return pcm16_to_wav_bytes(pcm, rate) if header else pcm.tobytes()        # pcm.py:84-93
            if fmt == "pcm":
                return pcm.tobytes()
            return _av_encode(pcm, fmt, rate)

        if req.stream and pool_streams and (spd is None or (pool_stream_speeds and (rate == SAMPLE_RATE or pool_stream_speed_rates))) \
                and (not as_flac or pool_stream_flac) and (not lim or pool_stream_limiter) and (trim is None or pool_stream_pauses) \
                and (not as_adpcm or pool_stream_adpcm) and (comp is None or pool_stream_compress):
            async def pooled_stream():       # the serial streamed branch's framing; the chunks come from the shared pool
                skw = rkw if rate == SAMPLE_RATE else {**rkw, "sample_rate": rate}
                if spd is not None:
                    skw = {**skw, "speed": spd}
                if lim:
                    skw = {**skw, "limiter": True, **({} if gdb is None else {"gain_db": gdb})}
                if trim is not None:
                    skw = {**skw, "pauses": trim}
                if comp is not None:
                    skw = {**skw, "compress": comp}
                chunks = batcher.submit_stream(req.input, code_params(req.voice), **skw, **({"adpcm_blocks": True} if as_adpcm else ekw))
                try:
                    first = True
                    async for chunk in iterate_in_threadpool(chunks):
                        if fmt == "wav" and first:
                            yield stream_header(rate)
                        if as_flac and first:
                            yield FLAC.stream_header(rate)
                        if as_adpcm and first:
                            yield ADPCM.stream_header(rate)
                        first = False
                        if np.asarray(chunk).size:
                            yield encode(chunk, header=False)
                except Exception as e:
                    log.error("speech synthesis failed mid-stream: %s", e)
                finally:
                    chunks.close()           # a client that went away: the request leaves the pool
            return StreamingResponse(pooled_stream(), media_type=media)

        if req.stream:
            async def audio_stream():                                                 # openai_api.py:259-274
                async with app.state.model_lock:
                    try:
                        first = True
                        gen = infer(req, rate, law, spd, as_flac, None, trim, lim, gdb, **akw, comp=comp) if comp is not None else \
                            infer(req, rate, law, spd, as_flac, None, trim, lim, gdb, **akw) if trim is not None else \
                            infer(req, rate, law, spd, as_flac, None, None, True, gdb, **akw) if lim else infer(req, rate, law, spd, True) if as_flac else \
                            infer(req, rate, None, spd, **akw) if as_adpcm else infer(req, rate, law, spd) if spd is not None else (infer(req, rate) if law is None else infer(req, rate, law))
                        async for chunk in iterate_in_threadpool(locked_chunks(gen) if batcher is not None else gen):
                            if fmt == "wav" and first:
                                yield stream_header(rate)
                            if as_flac and first:
                                yield FLAC.stream_header(rate)
                            if as_adpcm and first:
                                yield ADPCM.stream_header(rate)
                            first = False
                            if np.asarray(chunk).size:
                                yield encode(chunk, header=False)
                    except Exception as e:      # the status line is gone by now: end the body, log the cause
                        log.error("speech synthesis failed mid-stream: %s", e)
            return StreamingResponse(audio_stream(), media_type=media)

        if batcher is not None:
            try:
                if rate != SAMPLE_RATE:
                    rkw = {**rkw, "sample_rate": rate}
                if spd is not None:
                    rkw = {**rkw, "speed": spd}
                if lufs is not None:
                    rkw = {**rkw, "loudness": lufs}
                if trim is not None:
                    rkw = {**rkw, "pauses": trim}
                if lim:
                    rkw = {**rkw, "limiter": True}
                if comp is not None:
                    rkw = {**rkw, "compress": comp}
                if tone is not None:
                    rkw = {**rkw, "eq": tone}
                wavs = [await asyncio.wrap_future(batcher.submit(req.input, code_params(req.voice), **rkw, **ekw))]
            except Exception as e:
                raise HTTPException(500, detail=f"Speech synthesis failed: {e}")
        else:
            async with app.state.model_lock:
                try:
                    if tone is not None:
                        wavs = await run_in_threadpool(infer, req, rate, law, spd, as_flac, lufs, trim, lim, **akw,
                                                       **({} if comp is None else {"comp": comp}), tone=tone)
                    elif comp is not None:
                        wavs = await run_in_threadpool(infer, req, rate, law, spd, as_flac, lufs, trim, lim, **akw, comp=comp)
                    elif lim:
                        wavs = await run_in_threadpool(infer, req, rate, law, spd, as_flac, lufs, trim, True, **akw)
                    elif trim is not None:
                        wavs = await run_in_threadpool(infer, req, rate, law, spd, as_flac, lufs, trim, **akw)
                    elif lufs is not None:
                        wavs = await run_in_threadpool(infer, req, rate, law, spd, as_flac, lufs, **akw)
                    elif as_adpcm:
                        wavs = await run_in_threadpool(infer, req, rate, None, spd, **akw)
                    elif as_flac:
                        wavs = await run_in_threadpool(infer, req, rate, None, spd, True)
                    else:
                        wavs = await run_in_threadpool(infer, req, rate, *(() if law is None and spd is None else (law,)),
                                                       *(() if spd is None else (spd,)))
                except Exception as e:
                    raise HTTPException(500, detail=f"Speech synthesis failed: {e}")
        if len(wavs) == 0:
            raise HTTPException(500, detail="Speech synthesis failed: the engine returned no audio")
        body = encode(wavs[0], header=True)                                           # openai_api.py:277-288
        return Response(content=body, media_type=media, headers={"Content-Disposition": f"attachment; filename=output.{'wav' if as_adpcm else fmt}"})

    if voice_upload:
        from .audio import load_wav
        from .frontend import Speaker

        def clone(wav, clip_rate: int) -> str:
            with gpu_lock:
                return chat.sample_audio_speaker(wav, clip_rate)

        @app.post("/v1/audio/voices")
        async def add_voice(request: Request, name: str, text: Optional[str] = None):
            if not name or name == "default":
                raise HTTPException(400, detail='a voice needs a name other than "default"')
            try:
                wav, clip_rate = load_wav(await request.body(), **({"g711": True} if g711 else {}), **({"adpcm": True} if adpcm else {}))
            except ValueError as e:
                raise HTTPException(400, detail=f"bad WAV upload: {e}")
            async with app.state.model_lock:
                try:
                    smp = await run_in_threadpool(clone, wav, clip_rate)
                except ValueError as e:                # a rate pair the resampler refuses
                    raise HTTPException(400, detail=str(e))
            tokens = int(Speaker.decode_prompt(smp).shape[-1])
            if tokens == 0:
                raise HTTPException(400, detail="the clip is too short: it encodes to no audio token")
            room = voice_token_room()
            if room is not None and tokens > room:
                raise HTTPException(400, detail=f"the clip encodes to {tokens} audio tokens; a pool slot holds at most {room} beside a prompt")
            voices[name] = {"spk_smp": smp, **({"txt_smp": text} if text else {})}
            return {"name": name, "seconds": wav.shape[0] / clip_rate, "sample_rate": clip_rate, "tokens": tokens}

    @app.get("/health")
    async def health():                                                               # openai_api.py:291-294
        loaded = bool(getattr(chat, "has_loaded", lambda: True)())
        out = {"status": "healthy" if loaded else "loading", "model_loaded": loaded, "formats": sorted(formats)}
        if batcher is not None:
            out["pool"] = batcher.occupancy()
        if loudness:
            out["loudness"] = True
        if flac_streams:
            out["stream_flac"] = True
        if adpcm_streams:
            out["stream_adpcm"] = True
        if pauses:
            out["pauses"] = True
        if limiter:
            out["limiter"] = True
        if limiter_streams:
            out["stream_limiter"] = True
        if pause_streams:
            out["stream_pauses"] = True
        if compress:
            out["compress"] = True
        if compress_streams:
            out["stream_compress"] = True
        if eq:
            out["eq"] = True
        return out

    return app

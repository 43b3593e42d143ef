"""Load test of the speech endpoint: N concurrent non-streamed requests (several voices and texts) sent to the app in-process, once with
batching (`create_app(..., batch_slots=S)`) and once without, plus the sampling kernel's cost in a per-request pool vs a plain pool.
Prints one JSON line.  Not a bench.py leg.

    python tools/serve_load.py [--n 16] [--slots 8] [--max-new 256] [--dtype bf16] [--ragged-decode] [--stream [--repeat R] [--sample-rate HZ [--encoding ulaw|alaw]] [--speed V]]
    python tools/serve_load.py --refine [--refine-max-new 64] [--n 16] [--slots 8] [--max-new 256] [--dtype bf16]
    python tools/serve_load.py --split [--split-sentences 6] [--n 16] [--slots 8] [--max-new 256] [--dtype bf16]

--split: N concurrent MULTI-SENTENCE requests (the reference's default `split_text` handling of a long input), in one process: (a) through
`Chat.infer(text, split_text=True, ragged_decode=True, pcm16=True)` one by one under a lock, (b) through the batcher
(`SpeechBatcher.submit(text, params, split_text=True)`, ragged_decode on: a request's sentences side by side in the slots).  Audio-s/s,
p50 / p95 latency, acoustic-decoder calls (stage A's included) and the batcher's `split` occupancy.

--refine: the same N concurrent requests WITH the refine-text pass (the reference's default two-stage call), in one process: (a) through
`Chat.infer(skip_refine_text=False)` one at a time under a lock, (b) through the two-pool batcher (`SpeechBatcher(refine=True,
streams=True)`: a text-mode pool feeding the code pool).  Non-streamed: audio-s/s, p50 / p95 latency; then the same requests streamed:
additionally the time to the first audio chunk.

--stream: instead, N concurrent STREAMED requests against the batching app with `batch_streams` off (streams served one after the
other, each a batch of one) and on (streams share the slot pool, the chunks due at one poll come from one window decode): per request
the time to the first audio byte and the total time, p50 / p95, and audio-s/s; then one streamed request alone on both (--repeat runs
each, off and on alternating: the single-stream time to first byte and its run-to-run spread).  --ragged-decode composes.
--stream --sample-rate HZ: instead, the pooled streams (`batch_streams` on) at 24 kHz and asking for HZ (`stream_sample_rates`: every chunk
resampled on the device) in one process, the same figures, and one stream alone on both, alternating.
--stream --sample-rate HZ --encoding ulaw|alaw: instead, the pooled streams at HZ as 16-bit PCM and at HZ as G.711 (`g711=True`: every chunk
companded on the device behind the conversion) in one process, the same figures, and one stream alone on both legs, alternating: the
G.711 leg's first-byte p50 beside the PCM16 leg's, and the PCM16 leg's own run-to-run spread to judge the difference against.

--stream --speed V [--sample-rate HZ [--encoding ulaw|alaw]]: instead, the pooled streams (`batch_streams` on) at speed 1 and at V (`speed=True, stream_speed=True`: every chunk is what its
push into the request's stream of the time scaler made final), then one stream alone on both legs, alternating, --repeat times.
--ragged-decode: also the batched burst with `create_app(..., ragged_decode=True)` (the requests that finish in one poll decoded in one
ragged pass) -- an A/B against the default batched burst (one decode per request), with both runs' decode-call counts.

Synthetic weights (chattts_amd.weights) and the repository's test tokenizer: random weights do not stop on cue, so every request is capped
at --max-new tokens (the endpoint's own max_new_token is 2048).  audio_s_per_s = seconds of returned audio / wall seconds of the burst."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chattts_amd import _lib, server  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool  # noqa: E402
from chattts_amd.weights import synthetic_all  # noqa: E402

TEXTS = ["What is [uv_break]your favorite english food?", "Hello there, how are you today?", "The quick brown fox jumps over the lazy dog.",
         "Good morning, and welcome to the show.", "Numbers like 42 and 7 are read out loud.", "A longer sentence, with a pause, and an ending."]


def burst(chat, voices, n, batch_slots, ragged_decode=False, counts=False):
    from starlette.testclient import TestClient
    app = server.create_app(chat, voices, batch_slots=batch_slots, ragged_decode=ragged_decode)
    names = sorted(voices)
    lat, samples, codes = [0.0] * n, [0] * n, [0] * n
    with TestClient(app) as c:
        c.post("/v1/audio/speech", json={"input": "Warm up.", "response_format": "pcm"})       # first-call costs out of the burst

        def one(i):
            t0 = time.perf_counter()
            r = c.post("/v1/audio/speech", json={"input": TEXTS[i % len(TEXTS)], "voice": names[i % len(names)], "response_format": "pcm"})
            lat[i] = time.perf_counter() - t0
            codes[i] = r.status_code
            if r.status_code == 200:
                samples[i] = len(r.content) // 2
            else:
                print(f"request {i}: {r.status_code} {r.text[:300]}", file=sys.stderr)
        t0 = time.perf_counter()
        ths = [threading.Thread(target=one, args=(i,)) for i in range(n)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        wall = time.perf_counter() - t0
        health = c.get("/health").json()
    if app.state.batcher is not None:
        app.state.batcher.close()
    audio = sum(samples) / server.SAMPLE_RATE
    out = dict(failed=sum(c != 200 for c in codes), audio_s_per_s=round(audio / wall, 2), wall_s=round(wall, 3), audio_s=round(audio, 2),
               p50_s=round(float(np.percentile(lat, 50)), 3), p95_s=round(float(np.percentile(lat, 95)), 3),
               max_coresident=(health.get("pool") or {}).get("max_coresident", 1))
    if counts:       # the warm-up request is one of the decodes
        pool = health.get("pool") or {}
        out.update(decode_calls=pool.get("decode_calls"), max_decode_group=pool.get("max_decode_group"))
    return out


def stream_burst(chat, voices, n, slots, batch_streams, ragged_decode=False, app=None, rate=None, encoding=None, speed=None):
    """n concurrent streamed requests, driven through the ASGI interface on one event loop (a test client would hand the body over only
    once it is complete): the clock of a request stops at its first body message that carries audio, and at its last message.
    `rate`: the streams ask for that sample rate (`stream_sample_rates`; None: 24 kHz, the body carries no rate).  `encoding`: the streams
    ask for raw G.711 ("ulaw" / "alaw": `g711=True`, one byte per sample).  `speed`: the streams carry that speed (`speed=True,
    stream_speed=True`: the time scaler's path carried across their chunks; with `rate` also `stream_speed_rates=True`: the scaled stream
    resampled with the filter's history carried); the audio seconds counted are those of the scaled stream"""
    import asyncio
    own = app is None
    if own:
        app = server.create_app(chat, voices, batch_slots=slots, ragged_decode=ragged_decode, batch_streams=batch_streams,
                                **({} if rate is None else {"stream_sample_rates": (int(rate),)}), **({} if encoding is None else {"g711": True}),
                                **({} if speed is None else {"speed": True, "stream_speed": True}),
                                **({"stream_speed_rates": True} if speed is not None and rate is not None else {}))
    names = sorted(voices)
    more = {**({} if rate is None else {"sample_rate": int(rate)}), **({} if speed is None else {"speed": float(speed)})}

    async def one(i, text, out):
        body = json.dumps({"input": text, "voice": names[i % len(names)], "response_format": encoding or "pcm", "stream": True, **more}).encode()
        scope = dict(type="http", asgi={"version": "3.0"}, http_version="1.1", method="POST", path="/v1/audio/speech", raw_path=b"/v1/audio/speech",
                     query_string=b"", root_path="", scheme="http", server=("load", 80), client=("load", 1),
                     headers=[(b"content-type", b"application/json"), (b"content-length", str(len(body)).encode())])
        sent = [False]

        async def receive():
            if not sent[0]:
                sent[0] = True
                return {"type": "http.request", "body": body, "more_body": False}
            await asyncio.sleep(3600)
            return {"type": "http.disconnect"}
        t0 = time.perf_counter()

        async def send(msg):
            if msg["type"] == "http.response.start":
                out["status"] = msg["status"]
            elif msg["type"] == "http.response.body" and msg.get("body"):
                out.setdefault("first_s", time.perf_counter() - t0)
                out["bytes"] = out.get("bytes", 0) + len(msg["body"])
        await app(scope, receive, send)
        out["total_s"] = time.perf_counter() - t0

    async def run(texts):
        outs = [dict() for _ in texts]
        t0 = time.perf_counter()
        await asyncio.gather(*[one(i, t, outs[i]) for i, t in enumerate(texts)])
        return outs, time.perf_counter() - t0
    asyncio.run(run(["Warm up."]))                                 # first-call costs out of the burst
    outs, wall = asyncio.run(run([TEXTS[i % len(TEXTS)] for i in range(n)]))
    pool = app.state.batcher.occupancy() if app.state.batcher is not None else {}
    if own and app.state.batcher is not None:
        app.state.batcher.close()
    first = [o.get("first_s", float("nan")) for o in outs]
    total = [o["total_s"] for o in outs]
    audio = sum(o.get("bytes", 0) for o in outs) / (2 if encoding is None else 1) / (server.SAMPLE_RATE if rate is None else int(rate))
    pct = lambda v, q: round(float(np.percentile(v, q)), 4)
    out = dict(failed=sum(o.get("status") != 200 or "first_s" not in o for o in outs), audio_s_per_s=round(audio / wall, 2), wall_s=round(wall, 3),
               audio_s=round(audio, 2), first_byte_p50_s=pct(first, 50), first_byte_p95_s=pct(first, 95), total_p50_s=pct(total, 50),
               total_p95_s=pct(total, 95))
    for k in ("max_coresident", "stream_decode_calls", "stream_chunks", "max_stream_group", "decode_calls", "stream_resampled_chunks", "companded",
              "stream_scaled_chunks"):
        if k in pool:
            out[k] = pool[k]
    return out


def stream_rate_main(chat, voices, a):
    """--stream --sample-rate R: the pooled streams at 24 kHz and at R Hz in one process, then one stream alone on both, alternating"""
    base = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode)
    at = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode, rate=a.sample_rate)
    single = {"24000": [], str(a.sample_rate): []}
    for _ in range(a.repeat):
        for rate in (None, a.sample_rate):
            single[str(rate or 24000)].append(stream_burst(chat, voices, 1, a.slots, True, a.ragged_decode, rate=rate)["first_byte_p50_s"])
    print(json.dumps(dict(metric="serve_load_stream_rate", n=a.n, slots=a.slots, max_new=a.max_new, dtype=a.dtype, sample_rate=a.sample_rate,
                          at_24000=base, at_rate=at, first_byte_p50_delta_s=round(at["first_byte_p50_s"] - base["first_byte_p50_s"], 4),
                          single_stream_first_byte_s=single)))


def stream_speed_main(chat, voices, a):
    """--stream --speed V [--sample-rate R [--encoding E]]: the pooled streams at speed 1 and at V (both at R Hz, as E, when given) in one
    process, then one stream alone on both, alternating"""
    rate = None if a.sample_rate is None or int(a.sample_rate) == server.SAMPLE_RATE else int(a.sample_rate)
    fmt = dict(rate=rate, encoding=a.encoding)
    base = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode, **fmt)
    at = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode, speed=a.speed, **fmt)
    single = {"1.0": [], str(a.speed): []}
    for _ in range(a.repeat):
        for v in (None, a.speed):
            single[str(v or 1.0)].append(stream_burst(chat, voices, 1, a.slots, True, a.ragged_decode, speed=v, **fmt)["first_byte_p50_s"])
    p50 = {k: round(float(np.percentile(v, 50)), 4) for k, v in single.items()}
    print(json.dumps(dict(metric="serve_load_stream_speed", n=a.n, slots=a.slots, max_new=a.max_new, dtype=a.dtype, speed=a.speed, sample_rate=rate or 24000,
                          encoding=a.encoding, at_1=base,
                          at_speed=at, single_stream_first_byte_s=single, single_stream_first_byte_p50_s=p50,
                          single_stream_p50_delta_s=round(p50[str(a.speed)] - p50["1.0"], 4),
                          speed_1_spread_s=round(max(single["1.0"]) - min(single["1.0"]), 4))))


def stream_encoding_main(chat, voices, a):
    """--stream --sample-rate R --encoding E: the pooled streams at R Hz as PCM16 and as G.711 in one process, then one stream alone on both"""
    rate = None if a.sample_rate is None or int(a.sample_rate) == server.SAMPLE_RATE else int(a.sample_rate)
    base = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode, rate=rate)
    at = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode, rate=rate, encoding=a.encoding)
    single = {"pcm16": [], a.encoding: []}
    for _ in range(a.repeat):
        for enc in (None, a.encoding):
            single[enc or "pcm16"].append(stream_burst(chat, voices, 1, a.slots, True, a.ragged_decode, rate=rate, encoding=enc)["first_byte_p50_s"])
    p50 = {k: round(float(np.percentile(v, 50)), 4) for k, v in single.items()}
    print(json.dumps(dict(metric="serve_load_stream_encoding", n=a.n, slots=a.slots, max_new=a.max_new, dtype=a.dtype, sample_rate=rate or 24000,
                          encoding=a.encoding, pcm16=base, g711=at, single_stream_first_byte_s=single, single_stream_first_byte_p50_s=p50,
                          single_stream_p50_delta_s=round(p50[a.encoding] - p50["pcm16"], 4),
                          pcm16_spread_s=round(max(single["pcm16"]) - min(single["pcm16"]), 4))))


def stream_main(chat, voices, a):
    if a.speed is not None and int(round(100 * a.speed)) != 100:
        return stream_speed_main(chat, voices, a)
    if a.encoding is not None:
        return stream_encoding_main(chat, voices, a)
    if a.sample_rate is not None and int(a.sample_rate) != server.SAMPLE_RATE:
        return stream_rate_main(chat, voices, a)
    off = stream_burst(chat, voices, a.n, a.slots, False, a.ragged_decode)
    on = stream_burst(chat, voices, a.n, a.slots, True, a.ragged_decode)
    single = {"off": [], "on": []}
    for _ in range(a.repeat):                                      # one stream alone, the two legs alternating
        for name, flag in (("off", False), ("on", True)):
            single[name].append(stream_burst(chat, voices, 1, a.slots, flag, a.ragged_decode)["first_byte_p50_s"])
    print(json.dumps(dict(metric="serve_load_stream", n=a.n, slots=a.slots, max_new=a.max_new, dtype=a.dtype, ragged_decode=a.ragged_decode,
                          batch_streams_off=off, batch_streams_on=on,
                          first_byte_p50_ratio=round(off["first_byte_p50_s"] / on["first_byte_p50_s"], 2),
                          audio_rate_ratio=round(on["audio_s_per_s"] / off["audio_s_per_s"], 2),
                          single_stream_first_byte_s=single)))


def leg(call, n, stream=False):
    """n threads, `call(i)` -> the waveform, or an iterator of chunks"""
    lat, first, samples = [0.0] * n, [float("nan")] * n, [0] * n

    def one(i):
        t0 = time.perf_counter()
        try:
            got = call(i)
            for c in (got if stream else [got]):
                if np.asarray(c).size and first[i] != first[i]:
                    first[i] = time.perf_counter() - t0
                samples[i] += int(np.asarray(c).size)
        except Exception as e:
            print(f"request {i}: {e}", file=sys.stderr)
        lat[i] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ths = [threading.Thread(target=one, args=(i,)) for i in range(n)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    wall = time.perf_counter() - t0
    audio = sum(samples) / server.SAMPLE_RATE
    pct = lambda v, q: round(float(np.nanpercentile(v, q)), 4)
    out = dict(failed=sum(x == 0 for x in samples), audio_s_per_s=round(audio / wall, 2), wall_s=round(wall, 3), audio_s=round(audio, 2),
               p50_s=pct(lat, 50), p95_s=pct(lat, 95))
    if stream:
        out.update(first_chunk_p50_s=pct(first, 50), first_chunk_p95_s=pct(first, 95))
    return out


def refine_main(chat, voices, a):
    from chattts_amd.serving import SpeechBatcher
    names = sorted(voices)
    refine = chat.RefineTextParams(show_tqdm=False, manual_seed=42, max_new_token=a.refine_max_new)

    def code_params(i):
        return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                    show_tqdm=False, manual_seed=42, spk_emb=voices[names[i % len(names)]])

    lock = threading.Lock()
    res = {}
    for stream in (False, True):
        def serial(i):
            def call():
                return chat.infer([TEXTS[i % len(TEXTS)]], stream=stream, skip_refine_text=False, params_refine_text=refine,
                                  params_infer_code=code_params(i), pcm16=True)
            if not stream:
                with lock:
                    return call()[0]

            def chunks():          # the lock is held for the stream's whole life, like the serial endpoint's model_lock
                with lock:
                    yield from call()
            return chunks()
        leg(serial, 1, stream)                                           # first-call costs out of the burst
        res["serial_stream" if stream else "serial"] = leg(serial, a.n, stream)
        b = SpeechBatcher(chat, a.slots, threading.Lock(), refine=True, streams=True)
        try:
            def pooled(i):
                if stream:
                    return b.submit_stream(TEXTS[i % len(TEXTS)], code_params(i), refine=refine)
                return b.submit(TEXTS[i % len(TEXTS)], code_params(i), refine=refine).result()
            leg(pooled, 1, stream)
            res["pooled_stream" if stream else "pooled"] = {**leg(pooled, a.n, stream), "refine": b.occupancy()["refine"],
                                                             "max_coresident": b.occupancy()["max_coresident"]}
        finally:
            b.close()
    print(json.dumps(dict(metric="serve_load_refine", n=a.n, slots=a.slots, max_new=a.max_new, refine_max_new=a.refine_max_new, dtype=a.dtype,
                          **res, speedup=round(res["pooled"]["audio_s_per_s"] / res["serial"]["audio_s_per_s"], 2),
                          stream_speedup=round(res["pooled_stream"]["audio_s_per_s"] / res["serial_stream"]["audio_s_per_s"], 2))))


def split_main(chat, voices, a):
    """N concurrent multi-sentence requests: `Chat.infer(text, split_text=True, ragged_decode=True, pcm16=True)` one by one under a lock
    against `SpeechBatcher.submit(text, params, split_text=True)` (ragged_decode on), in one process"""
    from chattts_amd.serving import SpeechBatcher
    names = sorted(voices)
    texts = ["\n".join(TEXTS[(i + j) % len(TEXTS)] for j in range(a.split_sentences)) for i in range(a.n)]

    def code_params(i):
        return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                    show_tqdm=False, manual_seed=42, spk_emb=voices[names[i % len(names)]])
    lock = threading.Lock()
    decodes = [0]
    ragged, alone = chat.codec.decode_ragged, chat.codec.decode_to_wavs

    def counted(fn):
        def wrap(*args, **kw):
            decodes[0] += 1
            return fn(*args, **kw)
        return wrap

    def serial(i):
        with lock:
            return chat.infer(texts[i], skip_refine_text=True, split_text=True, ragged_decode=True, pcm16=True, params_infer_code=code_params(i))[0]
    leg(serial, 1)                                                       # first-call costs out of the burst
    chat.codec.decode_ragged, chat.codec.decode_to_wavs = counted(ragged), counted(alone)
    try:
        res = {"serial": {**leg(serial, a.n), "decode_calls": decodes[0]}}
        decodes[0] = 0
        b = SpeechBatcher(chat, a.slots, threading.Lock(), ragged_decode=True)
        try:
            def pooled(i):
                return b.submit(texts[i], code_params(i), split_text=True).result()
            leg(pooled, 1)
            decodes[0] = 0
            res["pooled"] = {**leg(pooled, a.n), "decode_calls": decodes[0], "split": b.occupancy()["split"],
                             "max_coresident": b.occupancy()["max_coresident"]}
        finally:
            b.close()
    finally:
        del chat.codec.decode_ragged, chat.codec.decode_to_wavs
    print(json.dumps(dict(metric="serve_load_split", n=a.n, slots=a.slots, max_new=a.max_new, sentences=a.split_sentences, dtype=a.dtype, **res,
                          speedup=round(res["pooled"]["audio_s_per_s"] / res["serial"]["audio_s_per_s"], 2))))


def sample_k_ms(eng, per_request, slots, steps=64):
    """mean sample_k time (profile tag 9) over `steps` eager decode steps of a full pool of identical requests"""
    pool = SlotPool(eng, slots=slots, cap=512, hid_cap=256, manual_seed=42, per_request=per_request)
    rs = np.random.RandomState(3)
    for i in range(slots):
        ids = np.repeat(rs.randint(1, 21178, size=(24, 1)), 4, axis=1).astype(np.int64)
        kw = dict(params=dict(manual_seed=42)) if per_request else {}
        pool.submit(i, ids, max_new_token=200, stop_at=200, **kw)
    pool._admit()
    lib = pool.lib
    _lib.check(lib.ctts_gpt_profile_begin(pool.handle, 9, 4096, 1), "profile_begin")
    for _ in range(steps):
        _lib.check(lib.ctts_gpt_decode_step(pool.handle, C.byref(pool.dec), pool.st.cuda_stream), "decode_step")
    pool.st.synchronize()
    n, tot = C.c_int32(0), C.c_double(0.0)
    _lib.check(lib.ctts_gpt_profile_end(pool.handle, C.byref(n), C.byref(tot)), "profile_end")
    pool.close()
    return tot.value / max(1, n.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--max-new", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--ragged-decode", action="store_true", help="A/B: also the batched burst with one ragged decode per poll")
    ap.add_argument("--stream", action="store_true", help="streamed requests: batch_streams off vs on")
    ap.add_argument("--sample-rate", type=int, default=None, help="--stream: the pooled streams at 24 kHz vs at this rate (resampled chunks)")
    ap.add_argument("--encoding", choices=("ulaw", "alaw"), default=None,
                    help="--stream: the pooled streams as 16-bit PCM vs as G.711 at --sample-rate (8000: the telephone's)")
    ap.add_argument("--speed", type=float, default=None, help="--stream: the pooled streams at speed 1 vs at this speed (the scaler's path carried across chunks)")
    ap.add_argument("--repeat", type=int, default=5, help="--stream: single-stream runs per leg (run-to-run spread)")
    ap.add_argument("--refine", action="store_true", help="two-stage requests: Chat.infer serially vs the two-pool batcher")
    ap.add_argument("--refine-max-new", type=int, default=64, help="--refine: max_new_token of the refine-text pass")
    ap.add_argument("--split", action="store_true", help="multi-sentence requests: Chat.infer(split_text=True) serially vs the batcher's split path")
    ap.add_argument("--split-sentences", type=int, default=6, help="--split: sentences per request")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    sds = synthetic_all()
    if a.split:       # the refer sentence's audio goes through the full DVAE's encoder
        from chattts_amd.weights import synthetic_dvae
        sds = {**sds, "dvae": synthetic_dvae()}
    assert chat.load(state_dicts=sds, device=dev, dtype=a.dtype, tokenizer=os.path.join(gold, "tokenizer"), spk_stat=spk_stat)
    torch.manual_seed(5)
    voices = {"default": chat.sample_random_speaker(), "alloy": chat.sample_random_speaker(), "echo": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": a.max_new})
    if a.split:
        return split_main(chat, voices, a)
    if a.refine:
        return refine_main(chat, voices, a)
    if a.stream:
        return stream_main(chat, voices, a)
    serial = burst(chat, voices, a.n, None)
    batched = burst(chat, voices, a.n, a.slots, counts=a.ragged_decode)
    extra = {}
    if a.ragged_decode:
        r = burst(chat, voices, a.n, a.slots, ragged_decode=True, counts=True)
        extra = dict(batched_ragged=r, ragged_speedup=round(r["audio_s_per_s"] / batched["audio_s_per_s"], 2))
    plain_ms = sample_k_ms(chat.gpt, False, a.slots)
    table_ms = sample_k_ms(chat.gpt, True, a.slots)
    print(json.dumps(dict(metric="serve_load", n=a.n, slots=a.slots, max_new=a.max_new, dtype=a.dtype, serial=serial, batched=batched,
                          speedup=round(batched["audio_s_per_s"] / serial["audio_s_per_s"], 2), **extra,
                          sample_k_us=dict(plain_pool=round(plain_ms * 1e3, 2), per_request_pool=round(table_ms * 1e3, 2)))))


if __name__ == "__main__":
    main()

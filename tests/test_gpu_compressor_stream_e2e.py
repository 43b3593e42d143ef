"""Compressed streams on the GPU, through every layer: `decode_windows(compress=, cp_streams=)` against `CodecEngine.compress` of the same
call's uncompressed float chunks, end to end (and the NumPy twin `compressor.StreamCompressor`, chunk by chunk) -- behind the plain crop,
the stateless rate path, the time-scale stream and the time-scale + resampler streams, behind a pause stream, in front of a limiter
stream, the conversion, G.711 and IMA ADPCM --, unflagged windows, the serial `Chat.infer` stream, a pooled stream against the serial
call, and the endpoint.  The spec's threshold is set from the uncompressed chunks' own peak, so the compressor engages whatever the
synthetic decode's level.  Synthetic weights.  `pytest -m gpu`."""
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import adpcm as ADPCM, compressor as CP, engine as E, g711 as G711, limiter as LM  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests.test_gpu_limiter_stream_e2e import LAWS, POLLS, STREAMS, _converted, _floats, _limited, _run  # noqa: E402
from tests.test_gpu_pauses_stream_e2e import _paused, _spec as _pause_spec  # noqa: E402
from tests.test_gpu_resample_stream_e2e import _close, _open  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _store  # noqa: E402

DEV = torch.device("cuda:0")
THR = np.float32(1e-5)
TEXT = ["One more short line."]


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def store():
    return _store()


def _idle(c):
    return (c.compress_streams_in_use(), c.trim_pauses_streams_in_use(), c.peak_limit_streams_in_use(), c.adpcm_streams_in_use(),
            c.time_scale_streams_in_use(), c.resample_streams_in_use()) == (0, 0, 0, 0, 0, 0)


@pytest.fixture(autouse=True)
def every_stream_given_back(codec):
    yield
    assert _idle(codec)


def _spec(chunks):
    """a spec whose threshold lies 18 dB under the stream's own peak (inside the validator's range), with a hold longer than a chunk's lag"""
    peak = max(float(np.abs(c).max()) for c in chunks if c.size)
    return {"threshold_db": float(np.clip(20 * np.log10(peak) - 18, -60, -6)), "ratio": 4, "knee_db": 6, "attack_ms": 5, "hold_ms": 120}


def _compressed(codec, chunks, rate, spec):
    """float chunks (the last one the stream's last push) -> (the twin's compressed chunks, its record); end to end they are
    `CodecEngine.compress` of the chunks end to end, bit for bit, and that call's record"""
    tw = CP.StreamCompressor(rate, spec)
    out = [tw.push(c, k == len(chunks) - 1) for k, c in enumerate(chunks)]
    whole = np.concatenate(chunks)
    if whole.size:
        y, rec = codec.compress(torch.from_numpy(whole).to(DEV), spec, rates=rate, return_stats=True)
        assert np.concatenate(out).tobytes() == y.cpu().numpy().tobytes() and tw.stats.tobytes() == rec[0].tobytes()
    return out, tw.stats


@pytest.fixture(scope="module")
def plain(codec, store):
    """per stream of the four float stages: today's float chunks, its spec, the compressed chunks and record -- once"""
    ts, rs = _open(codec, STREAMS.values())
    flt = _run(codec, store, POLLS, ts, rs, pcm16=False)
    _close(codec, ts, rs)
    out = {}
    for s, (v, r) in STREAMS.items():
        spec = _spec(flt[s])
        cmp, rec = _compressed(codec, flt[s], r, spec)
        assert rec["n_blocks"] > 0 and rec["n_touched"] > 0 and rec["min_gain"] < 1, (s, rec)
        assert sum(c.size for c in cmp) == sum(c.size for c in flt[s])
        out[s] = (flt[s], spec, cmp, rec)
    return out


def _windows(codec, store, plain, polls, pa=None, lm=None, ad=None, **kw):
    ts, rs = _open(codec, STREAMS.values())
    cp = {s: codec.compress_stream_open(r, plain[s][1]) for s, (_, r) in STREAMS.items()}
    try:
        got = {s: [] for s in STREAMS}
        for wins in polls:
            pkw = {} if pa is None else dict(pauses=[True] * len(wins), pa_streams=[pa[w[0]] for w in wins])
            lkw = {} if lm is None else dict(limiter=[True] * len(wins), lm_streams=[lm[w[0]] for w in wins])
            akw = {} if ad is None else dict(adpcm=[w[0] in ad for w in wins], adpcm_streams=[ad.get(w[0]) for w in wins])
            out = codec.decode_windows(store, wins, speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins],
                                       sample_rates=[STREAMS[w[0]][1] for w in wins], rs_streams=[rs[w[0]] for w in wins],
                                       compress=[plain[w[0]][1] for w in wins], cp_streams=[cp[w[0]] for w in wins], **pkw, **lkw, **akw, **kw)
            for w, a in zip(wins, out):
                got[w[0]].append(a)
        recs = {s: codec.compress_stream_stats(cp[s]) for s in STREAMS}
    finally:
        _close(codec, ts, rs)
        for h in cp.values():
            codec.compress_stream_close(h)
    return got, recs


# ---- 1. decode_windows(compress=, cp_streams=) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_call", [False, True])
def test_windows_behind_every_float_stage_equal_compress_of_the_uncompressed_chunks(codec, store, plain, one_call):
    polls = [[w for wins in POLLS for w in wins]] if one_call else POLLS          # one call: a stream's windows go to successive rounds
    flt, recs = _windows(codec, store, plain, polls, pcm16=False)
    for s in STREAMS:
        _, _, cmp, rec = plain[s]
        assert [a.size for a in flt[s]] == [c.size for c in cmp], (s, [a.size for a in flt[s]])
        assert all(a.dtype == np.float32 and a.tobytes() == c.tobytes() for a, c in zip(flt[s], cmp)), s
        assert recs[s].tobytes() == rec.tobytes(), (s, recs[s], rec)


def test_behind_a_pause_stream_and_in_front_of_a_limiter_stream(codec, store, plain):
    specs = {s: _pause_spec(plain[s][0], r) for s, (_, r) in STREAMS.items()}
    want = {}
    for s, (_, r) in STREAMS.items():
        cut, _ = _paused(plain[s][0], r, specs[s])
        cmp, rec = _compressed(codec, cut, r, plain[s][1])
        g = np.float32(1.6 / max(np.abs(c).max() for c in cmp if c.size))
        lim, lrec = _limited(cmp, r, g)
        assert rec["n_touched"] > 0 and lrec["n_over"] > 0 and sum(c.size for c in cut) < sum(c.size for c in plain[s][0]), s
        want[s] = (cmp, g, lim)
    pa = {s: codec.trim_pauses_stream_open(r, specs[s]) for s, (_, r) in STREAMS.items()}
    try:
        got, _ = _windows(codec, store, plain, POLLS, pa=pa, pcm16=False)
    finally:
        for h in pa.values():
            codec.trim_pauses_stream_close(h)
    for s in STREAMS:
        assert [a.tobytes() for a in got[s]] == [c.tobytes() for c in want[s][0]], s
    pa = {s: codec.trim_pauses_stream_open(r, specs[s]) for s, (_, r) in STREAMS.items()}
    lm = {s: codec.peak_limit_stream_open(r, want[s][1]) for s, (_, r) in STREAMS.items()}
    try:
        got, _ = _windows(codec, store, plain, POLLS, pa=pa, lm=lm, pcm16=False)
    finally:
        for h in pa.values():
            codec.trim_pauses_stream_close(h)
        for h in lm.values():
            codec.peak_limit_stream_close(h)
    for s in STREAMS:
        assert [a.tobytes() for a in got[s]] == [c.tobytes() for c in want[s][2]], s


def test_at_8_khz_the_conversion_g711_and_adpcm_act_on_the_compressed_samples(codec, store, plain):
    got, _ = _windows(codec, store, plain, POLLS, pcm16=True, keep_thr=1e-5, encodings=[LAWS[w[0]] for w in POLLS[0]])
    for s in STREAMS:                                                             # stream 1: mu-law at 8 kHz
        for k, (a, w) in enumerate(zip(got[s], _converted(plain[s][2], LAWS[s]))):
            assert a.dtype == w.dtype and a.tobytes() == w.tobytes(), (s, k, a.shape, w.shape)
    assert STREAMS[1][1] == 8000 and LAWS[1] == "ulaw" and got[1][0].dtype == np.uint8
    ad = {1: codec.adpcm_stream_open(8000)}
    try:
        got, _ = _windows(codec, store, plain, POLLS, ad=ad, pcm16=True, keep_thr=1e-5)
    finally:
        codec.adpcm_stream_close(ad[1])
    enc = ADPCM.StreamEncoder(8000)
    pcm = _converted(plain[1][2])
    blocks = [enc.push(np.ascontiguousarray(w), k == len(pcm) - 1) for k, w in enumerate(pcm)]
    assert [np.asarray(a).tobytes() for a in got[1]] == [bytes(b) for b in blocks] and sum(len(b) for b in blocks) > 0
    for s in (0, 2, 3):                                                           # the others: 16-bit samples of the compressed chunks
        assert [a.tobytes() for a in got[s]] == [w.tobytes() for w in _converted(plain[s][2])], s


def test_unflagged_windows_and_compress_none_return_todays_bytes(codec, store, plain):
    def call(flags, cp):
        ts, rs = _open(codec, STREAMS.values())
        try:
            wins = POLLS[0]
            kw = dict(speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins], sample_rates=[STREAMS[w[0]][1] for w in wins],
                      rs_streams=[rs[w[0]] for w in wins], encodings=[LAWS[w[0]] for w in wins])
            if flags is not None:
                kw.update(compress=flags, cp_streams=cp)
            return codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw)
        finally:
            _close(codec, ts, rs)
    today = call(None, None)
    for flags in ([False] * 4, [None] * 4, None):
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(call(flags, [None] * 4), today))
    a, b = codec.compress_stream_open(24000, plain[0][1]), codec.compress_stream_open(22050, plain[3][1])
    try:
        mixed = call([True, False, None, True], [a, None, None, b])
        assert mixed[1].tobytes() == today[1].tobytes() and mixed[2].tobytes() == today[2].tobytes()
        for s, k in ((0, 0), (3, 3)):
            assert mixed[k].tobytes() == _converted(plain[s][2][:1] + [np.zeros(0, np.float32)], LAWS[s])[0].tobytes(), s
        rec = codec._pool("compress").records[a]
        for kw in (dict(compress=[True], cp_streams=[None]), dict(compress=[True], cp_streams=[b]), dict(compress=[False], cp_streams=[a]),
                   dict(compress=[True, True], cp_streams=[a])):
            with pytest.raises(ValueError):                                       # refused before any launch: the stream is where it was
                codec.decode_windows(store, [POLLS[1][0]] * len(kw["compress"]), **kw)
        assert codec._pool("compress").records[a] == rec
    finally:
        codec.compress_stream_close(a)
        codec.compress_stream_close(b)


# ---- 2. the serial stream, the pooled stream and the endpoint ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chat(weights):
    return _chat(weights, "f32")


@pytest.fixture(scope="module")
def spoken(chat):
    """one streamed request's schedule: the hidden states and ranges of its chunks, recorded from today's float stream -- once"""
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    seen, orig = [], chat._stream_piece

    def recording(hiddens, a, b, *args, **kw):
        seen.append(([h.clone() for h in hiddens], a, b))
        return orig(hiddens, a, b, *args, **kw)
    chat._stream_piece = recording
    try:
        flt = [np.asarray(c) for c in chat.infer(TEXT, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk))]
    finally:
        del chat._stream_piece
    assert len(flt) == len(seen) == 4 and seen[-1][2] is None
    return spk, seen


def _pcm(chunks):
    return [float_to_int16(c) if c.size else c.astype(np.int16) for c in chunks]


@pytest.mark.parametrize("v,r", [(1.0, 24000), (1.0, 8000), (1.25, 8000)])
def test_the_serial_stream_is_compress_of_its_float_stream(chat, spoken, v, r):
    spk, seen = spoken
    on = {}
    if r != 24000:
        on.update(sample_rate=r, stream_resample=True)
    if v != 1.0:
        on.update(speed=v, stream_time_scale=True, **({"stream_scaled_resample": True} if r != 24000 else {}))
    pre = _floats(chat, seen, v, r)
    spec = _spec(pre)
    cmp, rec = _compressed(chat.codec, pre, r, spec)
    assert rec["n_touched"] > 0
    cmp[-1] = cmp[-1][np.abs(cmp[-1]) > THR]                                      # the tail's strip, on the compressed samples
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk))
    with pytest.raises(ValueError, match="block state carried across chunks"):
        chat.infer(TEXT, **kw, compress=spec, **on)

    def run(**more):
        out = list(chat.infer(TEXT, **kw, compress=spec, stream_compress=True, **on, **more))
        assert all(isinstance(c, list) and len(c) == 1 for c in out)             # one array per row
        return [np.asarray(c[0]) for c in out]
    flt = run()
    assert [c.size for c in flt] == [c.size for c in cmp] and all(c.dtype == np.float32 for c in flt)
    assert [c.tobytes() for c in flt] == [c.tobytes() for c in cmp]
    want = _pcm(cmp)
    pcm, law = run(pcm16=True), run(pcm16=True, encoding="ulaw")
    assert [p.tobytes() for p in pcm] == [w.tobytes() for w in want] and all(p.dtype == np.int16 for p in pcm)
    assert [u.tobytes() for u in law] == [G711.encode(w, "ulaw").tobytes() for w in want]
    if r == 8000 and v == 1.0:                                                    # the telephony path: ADPCM blocks of the compressed samples
        enc = ADPCM.StreamEncoder(r)
        blocks = [enc.push(np.ascontiguousarray(w), k == len(want) - 1) for k, w in enumerate(want)]
        got = run(pcm16=True, adpcm=True, stream_adpcm=True)
        assert [np.asarray(g).tobytes() for g in got] == [bytes(b) for b in blocks]
        g32 = LM.check_gain_db(12.0)                                              # ... and in front of a limiter stream
        cmp_full, _ = _compressed(chat.codec, pre, r, spec)
        lim, _ = _limited(cmp_full, r, g32)
        lim[-1] = lim[-1][np.abs(lim[-1]) > THR]
        got = run(limiter=True, stream_limiter=True, gain_db=12.0)
        assert [g.tobytes() for g in got] == [c.tobytes() for c in lim]
    gen = chat.infer(TEXT, **kw, compress=spec, stream_compress=True, pcm16=True, **on)
    next(gen)
    assert chat.codec.compress_streams_in_use() == 1
    gen.close()                                                                   # a consumer that goes away gives the stream back
    assert _idle(chat.codec)


def test_the_batcher_returns_the_serial_calls_bytes_and_gives_its_slots_back(chat, spoken):
    spk, seen = spoken
    text = TEXT[0]
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk))
    spec = _spec(_floats(chat, seen, 1.0, 8000))
    on = dict(sample_rate=8000, stream_resample=True, pcm16=True)
    want = [np.asarray(c[0]) for c in chat.infer([text], **kw, **on, compress=spec, stream_compress=True)]
    today = [np.asarray(c)[0] for c in chat.infer([text], **kw, **on)]
    assert b"".join(w.tobytes() for w in want) != b"".join(t.tobytes() for t in today)
    off = SpeechBatcher(chat, 2, threading.Lock(), streams=True)
    try:
        with pytest.raises(TypeError, match="block state carried across chunks"):
            off.submit_stream(text, _params(chat, spk), compress=spec)
        assert "stream_compressed_chunks" not in off.occupancy()
    finally:
        off.close()
    b = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_compress=True)
    try:
        got = list(b.submit_stream(text, _params(chat, spk), compress=spec, sample_rate=8000))
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want] and all(g.dtype == np.int16 for g in got)
        assert b.occupancy()["stream_compressed_chunks"] == len(want)
        assert [g.tobytes() for g in b.submit_stream(text, _params(chat, spk), sample_rate=8000)] == [t.tobytes() for t in today]
        s = b.submit_stream(text, _params(chat, spk), compress=spec)              # a cancelled one gives its slot back
        next(s)
        s.close()
        deadline = time.time() + 30
        while chat.codec.compress_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert _idle(chat.codec) and b.occupancy()["cancelled"] == 1
    finally:
        b.close()


def test_the_endpoint_serves_a_compressed_stream_when_switched_on(chat, spoken):
    from starlette.testclient import TestClient
    from chattts_amd import server
    spk, _ = spoken
    voices = {"default": spk}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 80, "min_new_token": 80})       # random weights do not stop on cue
    try:
        p = orig(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=80, min_new_token=80,
                 show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=spk, stream_batch=24, stream_speed=12000, pass_first_n_batches=2)
        kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=p, pcm16=True, encoding="ulaw", sample_rate=8000,
                  stream_resample=True)
        flt = [np.asarray(c)[0] for c in chat.infer(["A streamed sentence."], **{**kw, "pcm16": False, "encoding": None})]
        spec = _spec(flt)
        today = b"".join(np.asarray(c).tobytes() for c in chat.infer(["A streamed sentence."], **kw))
        want = b"".join(np.asarray(c[0]).tobytes() for c in chat.infer(["A streamed sentence."], **kw, compress=spec, stream_compress=True))
        body = {"input": "A streamed sentence.", "response_format": "ulaw", "stream": True, "sample_rate": 8000}
        on = dict(stream_sample_rates=(8000,), g711=True, compress=True)
        with TestClient(server.create_app(chat, voices, **on)) as c:           # off: today's refusal
            r = c.post("/v1/audio/speech", json={**body, "compress": spec})
            assert r.status_code == 400 and "block state carried across chunks" in r.text and "stream_compress" not in c.get("/health").json()
            assert c.post("/v1/audio/speech", json=body).content == today
        with TestClient(server.create_app(chat, voices, **on, stream_compress=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "compress": spec})
            assert r.status_code == 200 and r.content == want and want != today and len(want) > 0
            assert c.post("/v1/audio/speech", json={**body, "compress": {"hold_ms": 2000}}).status_code == 400
            assert c.post("/v1/audio/speech", json=body).content == today and c.get("/health").json()["stream_compress"] is True
        bat = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_compress=True)    # from the pool: the same bytes
        try:
            with TestClient(server.create_app(chat, voices, **on, stream_compress=True, batcher=bat, batch_streams=True)) as c:
                r = c.post("/v1/audio/speech", json={**body, "compress": spec})
                assert r.status_code == 200 and r.content == want and bat.occupancy()["stream_compressed_chunks"] > 0
        finally:
            bat.close()
    finally:
        chat.InferCodeParams = orig

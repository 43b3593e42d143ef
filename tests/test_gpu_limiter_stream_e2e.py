"""Limited streams on the GPU, through every layer: `decode_windows(limiter=, lm_streams=)` against the plain call's float chunks pushed
through the NumPy twin (`limiter.StreamLimiter`), then the host conversion, strip and companding -- behind the plain crop, the stateless
rate path, the time-scale stream and the time-scale + resampler streams --, rounds and an empty tail, the serial `Chat.infer` stream in
every format, pooled streams against the serial composition, the endpoint, and the streams given back wherever a request ends.  The gains
are chosen from the plain chunks' own peak (g = 1.6 / peak), so the limiter engages whatever the synthetic decode's level.  Synthetic
weights.  `pytest -m gpu`."""
import math
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, flac as FLAC, g711 as G711, limiter as LM  # noqa: E402
from chattts_amd.audio import float_to_int16, pcm_scale  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, SpeechBatcher, StreamEvents, StreamSpec  # noqa: E402
from tests.test_gpu_resample_stream_e2e import _close, _open, _resample_alone  # noqa: E402
from tests.test_gpu_stream_pool import _alone_stream, _engine  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _store  # noqa: E402
from tests.test_gpu_timescale_stream_e2e import _scale_alone  # noqa: E402

DEV = torch.device("cuda:0")
THR = np.float32(1e-5)
END1 = 256 * (2 * 30 - 1)

# four streams, (speed, rate): the plain crop, the stateless rate path, the time-scale stream, the time-scale and resampler streams; each
# as the windows of three polls -- stream 0's second chunk is clipped by its prefix's end and its tail has nothing left
STREAMS = {0: (1.0, 24000), 1: (1.0, 8000), 2: (1.25, 24000), 3: (0.77, 22050)}
POLLS = [[(0, 30, 0, 12000, False), (1, 24, 0, 6000, False), (2, 40, 0, 9000, False), (3, 30, 0, 3000, False)],
         [(0, 30, 12000, END1 + 500, False), (1, 48, 6000, 18000, False), (2, 64, 9000, 21000, False), (3, 56, 3000, 15000, False)],
         [(0, 30, END1, None, True), (1, 48, 18000, None, True), (2, 64, 21000, None, True), (3, 72, 15000, None, True)]]
LAWS = {0: None, 1: "ulaw", 2: "alaw", 3: None}


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def store():
    return _store()


@pytest.fixture(autouse=True)
def every_stream_given_back(codec):
    yield
    assert codec.peak_limit_streams_in_use() == 0 and codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0


def _run(codec, store, polls, ts, rs, lm=None, **kw):
    """the polls' windows through decode_windows, stream s on handles ts[s] / rs[s] (/ lm[s], where it has one) -> per stream its chunks"""
    got = {s: [] for s in STREAMS}
    for wins in polls:
        lkw = {} if lm is None else dict(limiter=[lm[w[0]] is not None for w in wins], lm_streams=[lm[w[0]] for w in wins])
        out = codec.decode_windows(store, wins, speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins],
                                   sample_rates=[STREAMS[w[0]][1] for w in wins], rs_streams=[rs[w[0]] for w in wins], **lkw, **kw)
        for w, a in zip(wins, out):
            got[w[0]].append(a)
    return got


def _limited(chunks, rate, g):
    """float chunks (the last one the stream's last push) through the twin -> (limited float chunks, the final record)"""
    tw = LM.StreamLimiter(rate, g)
    return [tw.push(c, k == len(chunks) - 1) for k, c in enumerate(chunks)], tw.stats


def _converted(lim, law=None, thr=THR):
    """the serial path's end on one stream's limited chunks: the tail stripped, every chunk converted under its own peak, companded"""
    out = []
    for k, f in enumerate(lim):
        f = f[np.abs(f) > thr] if k == len(lim) - 1 else f
        p = float_to_int16(f) if f.size else f.astype(np.int16)
        out.append(p if law is None else G711.encode(p, law))
    return out


@pytest.fixture(scope="module")
def plain(codec, store):
    """per stream: the float chunks of today's call (no limiter), the gain that puts their peak at 1.6, the twin's limited chunks and
    record -- computed once, left unchanged"""
    ts, rs = _open(codec, STREAMS.values())
    flt = _run(codec, store, POLLS, ts, rs, pcm16=False)
    _close(codec, ts, rs)
    out = {}
    for s, (v, r) in STREAMS.items():
        g = np.float32(1.6 / max(np.abs(c).max() for c in flt[s] if c.size))
        lim, rec = _limited(flt[s], r, g)
        assert rec["n_over"] > 0 and rec["n_touched"] > rec["n_over"] and max(np.abs(c).max() for c in lim if c.size) <= LM.C32, (s, rec)
        out[s] = (flt[s], g, lim, rec)
    assert out[0][0][2].size == 0 and out[0][2][2].size == 2 * 240            # a tail with nothing left still brings the 20 ms the stream held
    return out


# ---- 1. decode_windows(limiter=, lm_streams=) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_call", [False, True])
def test_windows_behind_every_float_stage_equal_the_twin_then_the_host_conversion(codec, store, plain, one_call):
    ts, rs = _open(codec, STREAMS.values())
    lm = {s: codec.peak_limit_stream_open(r, plain[s][1]) for s, (_, r) in STREAMS.items()}
    try:
        polls = [[w for wins in POLLS for w in wins]] if one_call else POLLS      # one call: a stream's windows go to successive rounds
        flt = _run(codec, store, polls, ts, rs, lm, pcm16=False)
        recs = {s: codec.peak_limit_stream_stats(lm[s]) for s in STREAMS}
    finally:
        _close(codec, ts, rs)
        for h in lm.values():
            codec.peak_limit_stream_close(h)
    for s in STREAMS:
        _, g, lim, rec = plain[s]
        assert [a.size for a in flt[s]] == [c.size for c in lim], (s, [a.size for a in flt[s]])
        assert all(a.dtype == np.float32 and a.tobytes() == c.tobytes() for a, c in zip(flt[s][:-1], lim[:-1])), s
        assert flt[s][-1].tobytes() == lim[-1].tobytes() and recs[s].tobytes() == rec.tobytes(), (s, recs[s], rec)


def test_the_conversion_the_strip_and_the_companding_act_on_the_limited_samples(codec, store, plain):
    thr_big = float(np.median(np.abs(plain[1][2][2])))
    for keep_thr in (1e-5, thr_big):
        ts, rs = _open(codec, STREAMS.values())
        lm = {s: codec.peak_limit_stream_open(r, plain[s][1]) for s, (_, r) in STREAMS.items()}
        try:
            got = {s: [] for s in STREAMS}
            for wins in POLLS:
                out = codec.decode_windows(store, wins, pcm16=True, keep_thr=keep_thr, speeds=[STREAMS[w[0]][0] for w in wins],
                                           ts_streams=[ts[w[0]] for w in wins], sample_rates=[STREAMS[w[0]][1] for w in wins],
                                           rs_streams=[rs[w[0]] for w in wins], encodings=[LAWS[w[0]] for w in wins],
                                           limiter=[True] * len(wins), lm_streams=[lm[w[0]] for w in wins])
                for w, a in zip(wins, out):
                    got[w[0]].append(a)
        finally:
            _close(codec, ts, rs)
            for h in lm.values():
                codec.peak_limit_stream_close(h)
        for s in STREAMS:
            want = _converted(plain[s][2], LAWS[s], np.float32(keep_thr))
            for k, (a, w) in enumerate(zip(got[s], want)):
                assert a.dtype == w.dtype and a.tobytes() == w.tobytes(), (keep_thr, s, k, a.shape, w.shape)
    kept = np.abs(plain[1][2][2]) > np.float32(thr_big)
    assert 0 < kept.sum() < kept.size                                         # the large threshold strips inside the limited tail
    # every 16-bit chunk was converted at scale 32767: the limited peak is under 1, the unlimited one (1.6) was not
    for s in (0, 3):
        for f, p in zip(plain[s][2][:2], _converted(plain[s][2])[:2]):
            if f.size:
                assert pcm_scale(np.abs(f).max()) == 32767 > pcm_scale(np.float32(1.6))
                assert int(np.abs(p.astype(np.int32)).max()) == int(float(np.abs(f).max()) * 32767.0)


def test_unflagged_windows_and_limiter_none_return_todays_bytes(codec, store, plain):
    def call(flags, lm):
        ts, rs = _open(codec, STREAMS.values())
        try:
            wins = POLLS[0]
            kw = dict(speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins], sample_rates=[STREAMS[w[0]][1] for w in wins],
                      rs_streams=[rs[w[0]] for w in wins], encodings=[LAWS[w[0]] for w in wins])
            if flags is not None:
                kw.update(limiter=flags, lm_streams=lm)
            return codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw)
        finally:
            _close(codec, ts, rs)
    today = call(None, None)
    for flags in ([False] * 4, None):
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(call(flags, [None] * 4), today))
    a, b = codec.peak_limit_stream_open(24000, plain[0][1]), codec.peak_limit_stream_open(22050, plain[3][1])
    try:
        mixed = call([True, False, False, True], [a, None, None, b])
        assert mixed[1].tobytes() == today[1].tobytes() and mixed[2].tobytes() == today[2].tobytes()
        for s, k in ((0, 0), (3, 3)):
            assert mixed[k].tobytes() == _converted(plain[s][2][:1] + [np.zeros(0, np.float32)], LAWS[s])[0].tobytes(), s
        rec = codec._pool("limiter").records[a]
        for kw in (dict(limiter=[True], lm_streams=[None]), dict(limiter=[True], lm_streams=[b]), dict(limiter=[False], lm_streams=[a]),
                   dict(limiter=[True, True], lm_streams=[a]), dict(limiter=[1], lm_streams=[a])):
            with pytest.raises(ValueError):                                   # refused before any launch: the stream is where it was
                codec.decode_windows(store, [POLLS[1][0]] * len(kw["limiter"]), **kw)
        assert codec._pool("limiter").records[a] == rec
    finally:
        codec.peak_limit_stream_close(a)
        codec.peak_limit_stream_close(b)


# ---- 2. the serial stream and the endpoint ----------------------------------------------------------------------------------------------
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
        flt = [np.asarray(c) for c in chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False,
                                                 params_infer_code=_params(chat, spk))]
    finally:
        del chat._stream_piece
    assert len(flt) == len(seen) == 4 and seen[-1][2] is None
    return spk, seen


def _floats(chat, seen, v, r):
    """the float chunks in front of the limiter of the recorded schedule at speed v and rate r, the last one the tail before its strip"""
    if v == 1.0:
        return [chat._stream_piece(hid, a, b, **({} if r == 24000 else {"rate": r}))[0] for hid, a, b in seen]
    out = _scale_alone(chat.codec, [chat._stream_piece(hid, a, b)[0] for hid, a, b in seen], v)
    return out if r == 24000 else _resample_alone(chat.codec, out, r)


@pytest.mark.parametrize("v,r", [(1.0, 24000), (1.0, 8000), (1.25, 24000), (1.25, 8000)])
def test_the_serial_stream_in_every_format_is_the_twin_over_its_float_stream(chat, spoken, v, r):
    spk, seen = spoken
    on = {}
    if r != 24000:
        on.update(sample_rate=r, stream_resample=True)
    if v != 1.0:
        on.update(speed=v, stream_time_scale=True, **({"stream_scaled_resample": True} if r != 24000 else {}))
    pre = _floats(chat, seen, v, r)
    gain_db = 20 * math.log10(1.6 / max(np.abs(c).max() for c in pre if c.size))
    assert -30 <= gain_db <= 30, gain_db       # the fixture text "One more short line." reaches the threshold within the public range
    lim, rec = _limited(pre, r, LM.check_gain_db(gain_db))
    assert rec["n_over"] > 0 and max(np.abs(c).max() for c in lim if c.size) <= LM.C32 < 1

    def run(**kw):
        return [np.asarray(c) for c in chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False,
                                                  params_infer_code=_params(chat, spk), limiter=True, stream_limiter=True, gain_db=gain_db, **on, **kw)]
    with pytest.raises(ValueError, match="look-ahead is not carried"):
        chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk),
                   limiter=True, **on)
    flt = run()
    assert [c.shape for c in flt[:-1]] == [(1, f.size) for f in lim[:-1]]
    assert all(c.dtype == np.float32 and c[0].tobytes() == f.tobytes() for c, f in zip(flt[:-1], lim[:-1]))
    assert flt[-1][0].tobytes() == lim[-1][np.abs(lim[-1]) > THR].tobytes()
    want = _converted(lim)                      # under scale 32767 throughout: every limited chunk's peak is below 1
    pcm, law = run(pcm16=True), run(pcm16=True, encoding="ulaw")
    for k, (p, u, w) in enumerate(zip(pcm, law, want)):
        assert p.dtype == np.int16 and p[0].tobytes() == w.tobytes(), k
        assert u.dtype == np.uint8 and u[0].tobytes() == G711.encode(w, "ulaw").tobytes(), k
    enc = FLAC.StreamEncoder(r)
    frames = [enc.push(np.ascontiguousarray(w), k == len(want) - 1) for k, w in enumerate(want)]
    got = run(pcm16=True, flac=True, stream_flac=True)
    assert [np.asarray(g[0]).tobytes() for g in got] == [bytes(f) for f in frames]
    gen = chat.infer(["One more short line."], stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk),
                     limiter=True, stream_limiter=True, pcm16=True, **on)
    next(gen)
    assert chat.codec.peak_limit_streams_in_use() == 1
    gen.close()                                 # a consumer that goes away gives the stream back
    assert chat.codec.peak_limit_streams_in_use() == 0 and chat.codec.flac_streams_in_use() == 0


def test_the_endpoint_serves_a_limited_stream_when_switched_on_and_a_cancelled_pooled_stream_gives_its_slot_back(chat, spoken):
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
        today = b"".join(np.asarray(c).tobytes() for c in chat.infer(["A streamed sentence."], **kw))
        want = b"".join(np.asarray(c).tobytes() for c in chat.infer(["A streamed sentence."], **kw, limiter=True, stream_limiter=True, gain_db=24.0))
        body = {"input": "A streamed sentence.", "response_format": "ulaw", "stream": True, "sample_rate": 8000}
        on = dict(stream_sample_rates=(8000,), g711=True, limiter=True)
        with TestClient(server.create_app(chat, voices, **on)) as c:           # off: today's refusal, and gain_db is an unknown key
            r = c.post("/v1/audio/speech", json={**body, "limiter": True})
            assert r.status_code == 400 and "look-ahead is not carried" in r.text
            assert c.post("/v1/audio/speech", json={**body, "gain_db": 24.0}).content == today and "stream_limiter" not in c.get("/health").json()
        with TestClient(server.create_app(chat, voices, **on, stream_limiter=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "limiter": True, "gain_db": 24.0})
            assert r.status_code == 200 and r.content == want and want != today and len(want) > 0
            assert c.post("/v1/audio/speech", json={**body, "limiter": True, "gain_db": 31}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "gain_db": 6}).status_code == 400
            assert c.post("/v1/audio/speech", json=body).content == today and c.get("/health").json()["stream_limiter"] is True
    finally:
        chat.InferCodeParams = orig
    b = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_limiter=True)
    try:
        s = b.submit_stream("One more short line.", _params(chat, spk), limiter=True, gain_db=12.0)
        assert next(s).dtype == np.int16 and chat.codec.peak_limit_streams_in_use() == 1
        s.close()
        deadline = time.time() + 30
        while chat.codec.peak_limit_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.peak_limit_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1 and b.occupancy()["stream_limited_chunks"] >= 1
        with pytest.raises(ValueError, match="needs limiter=True"):
            b.submit_stream("x", _params(chat, spk), gain_db=3.0)
    finally:
        b.close()


# ---- 3. the pooled streams ----------------------------------------------------------------------------------------------------------------
def _pre_limiter(chat, hid, counts, spec, v, r):
    """the `stream` branch of `Chat._infer` (one text) replayed over `hid` in float up to the limiter: the schedule's pieces at speed v
    and rate r, the last one the tail before its strip"""
    sched, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        sched.append(([hid[:n]], length, length + spec.stream_speed))
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
    sched.append(([hid], length, None))
    return _floats(chat, sched, v, r)


def test_pooled_streams_with_and_without_the_limiter_share_polls_and_equal_their_serial_calls(weights, plain):
    """four streams through an 8-slot pool, the chunks of a poll from ONE decode_windows call -- limited at 24 kHz, unlimited at 8 kHz,
    limited at 1.25 and 8 kHz, limited at 22050 Hz: every chunk == the serial composition replayed over the hidden states the pool
    returned, byte for byte"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec, chat.device, chat.incremental_stream = codec, DEV, True
    pool = SlotPool(eng, slots=8, cap=256, hid_cap=128, per_request=True)
    rng = np.random.RandomState(35)
    g = np.float32(4.0 * plain[0][1])          # the synthetic decode's level, from the windows above, with room to spare
    plan = [(72, -1, 3000, 0, 1.0, 24000, g), (96, 48, 12000, 1, 1.0, 8000, None), (60, -1, 12000, 0, 1.25, 8000, g), (50, -1, 5000, 1, 1.0, 22050, g)]
    reqs, ts, rs, lm = {}, {}, {}, {}
    for i, (max_new, stop, speed, passed, v, r, gain) in enumerate(plan):
        ids = torch.from_numpy(np.repeat(rng.randint(1, 21178, size=(int(rng.randint(4, 30)), 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(900 + 13 * i))
        reqs[i] = (ids, p, max_new, stop, StreamSpec(24, speed, passed), v, r, gain)
        (ts[i],), (rs[i],) = _open(codec, [(v, r)])
        lm[i] = None if gain is None else codec.peak_limit_stream_open(r, gain)
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=reqs[i][4])
    chunks, results, groups = {}, {}, []
    try:
        for got in pool.run(events=True):
            if isinstance(got, StreamEvents):
                groups.append(len(got.chunks))
                pcm = codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5,
                                           speeds=[reqs[c[0]][5] for c in got.chunks], ts_streams=[ts[c[0]] for c in got.chunks],
                                           sample_rates=[reqs[c[0]][6] for c in got.chunks], rs_streams=[rs[c[0]] for c in got.chunks],
                                           limiter=[lm[c[0]] is not None for c in got.chunks], lm_streams=[lm[c[0]] for c in got.chunks])
                for c, a in zip(got.chunks, pcm):
                    chunks.setdefault(c[0], []).append(a)
            else:
                results[got[0]] = (got[1].cpu().numpy(), got[2])
    finally:
        _close(codec, ts.values(), rs.values())
        for h in lm.values():
            if h is not None:
                codec.peak_limit_stream_close(h)
    assert sorted(results) == [0, 1, 2, 3] and sorted(chunks) == [0, 1, 2, 3] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec, v, r, gain) in reqs.items():
        ref, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        assert np.array_equal(results[i][0], ref.ids[0].cpu().numpy()), i
        pre = _pre_limiter(chat, results[i][1], counts, spec, v, r)
        if gain is not None:
            pre, rec = _limited(pre, r, gain)
            assert rec["n_over"] > 0, (i, rec)
        want = _converted(pre)
        got = chunks[i]
        assert [a.shape for a in got] == [w.shape for w in want], (i, v, r, [a.shape for a in got], [w.shape for w in want])
        for k, (a, w) in enumerate(zip(got, want)):
            assert a.dtype == np.int16 and a.tobytes() == w.tobytes(), (i, v, r, k)
    assert codec.peak_limit_streams_in_use() == 0 and codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0
    pool.close()

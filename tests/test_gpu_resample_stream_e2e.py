"""Streams at another speed AND another sample rate on the GPU, through every layer: `decode_windows(speeds=, ts_streams=, sample_rates=,
rs_streams=)` against the one-shot composition `resample(time_scale(speed-1 chunks))` bit for bit and the host conversion / companding
of its float chunks, mixed calls, rounds and empty tails, the serial stream, pooled streams against the serial composition, and the
endpoint.  Synthetic weights.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, g711 as G711, resample as RS, timescale as TS  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, StreamEvents, StreamSpec  # noqa: E402
from tests.test_gpu_stream_pool import _alone_stream, _engine  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _serial_chunks_rate, _store  # noqa: E402
from tests.test_gpu_timescale_stream_e2e import _scale_alone, _serial_chunks_speed  # noqa: E402

DEV = torch.device("cuda:0")
THR = np.float32(1e-5)
END1 = 256 * (2 * 30 - 1)

# four streams, (speed, rate), each as the windows of three polls: a first chunk, an interior chunk (stream 1's clipped by its prefix's
# end), a tail (stream 1's with nothing left); the prefixes grow as a pool's do
STREAMS = {0: (1.25, 8000), 1: (0.5, 16000), 2: (2.0, 44100), 3: (0.77, 22050)}
POLLS = [[(0, 24, 0, 6000, False), (1, 30, 0, 12000, False), (2, 40, 0, 9000, False), (3, 30, 0, 3000, False)],
         [(0, 48, 6000, 18000, False), (1, 30, 12000, END1 + 500, False), (2, 64, 9000, 21000, False), (3, 56, 3000, 15000, False)],
         [(0, 48, 18000, None, True), (1, 30, END1, None, True), (2, 64, 21000, None, True), (3, 72, 15000, None, True)]]


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def store():
    return _store()


@pytest.fixture(scope="module")
def whole(codec, store):
    """per stream: the speed-1 float chunks of its windows (today's call), and the one-shot composition of their concatenation --
    computed once, left unchanged"""
    out = {}
    for s, (v, r) in STREAMS.items():
        plain = codec.decode_windows(store, [p[s] for p in POLLS], pcm16=False)
        x = torch.from_numpy(np.concatenate(plain)).to(DEV)
        out[s] = (plain, codec.resample(codec.time_scale(x, v), 24000, r).cpu().numpy())
    return out


def _open(codec, pairs):
    ts = [None if TS.quantize(v)[0] == 100 else codec.time_scale_stream_open(v) for v, _ in pairs]
    rs = [None if TS.quantize(v)[0] == 100 or r == 24000 else codec.resample_stream_open(24000, r) for v, r in pairs]
    return ts, rs


def _close(codec, ts, rs):
    for h in ts:
        if h is not None:
            codec.time_scale_stream_close(h)
    for h in rs:
        if h is not None:
            codec.resample_stream_close(h)


def _resample_alone(codec, pieces, rate):
    """the float pieces of ONE stream (the last one its tail) through a fresh stream of the resampler, one step each -> float chunks"""
    h = codec.resample_stream_open(24000, rate)
    try:
        out = []
        for k, f in enumerate(pieces):
            x = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(DEV)
            y, _ = codec.resample_stream_step(x, [(h, 0, x.numel(), k == len(pieces) - 1)])
            out.append(y.cpu().numpy())
        return out
    finally:
        codec.resample_stream_close(h)


def _polls(codec, store, polls, ts, rs, **kw):
    """the polls' windows through decode_windows, stream s on handles ts[s] / rs[s] -> per stream its chunks in order"""
    got = {s: [] for s in STREAMS}
    for wins in polls:
        out = codec.decode_windows(store, wins, speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins],
                                   sample_rates=[STREAMS[w[0]][1] for w in wins], rs_streams=[rs[w[0]] for w in wins], **kw)
        for w, a in zip(wins, out):
            got[w[0]].append(a)
    return got


# ---- 1. decode_windows(speeds=, sample_rates=, rs_streams=) ------------------------------------------------------------------------------
def test_float_chunks_tile_the_one_shot_composition_bit_for_bit(codec, store, whole):
    ts, rs = _open(codec, STREAMS.values())
    got = _polls(codec, store, POLLS, ts, rs, pcm16=False)
    _close(codec, ts, rs)
    for s, (v, r) in STREAMS.items():
        plain, want = whole[s]
        assert all(g.dtype == np.float32 for g in got[s]) and want.size == RS.out_len(TS.out_len(sum(p.size for p in plain), TS.quantize(v)[0]), *RS.ratio(24000, r))
        assert np.concatenate(got[s]).tobytes() == want.tobytes(), (s, v, r, [g.size for g in got[s]])
        # the composition alone, stage by stage: the same chunk edges
        alone = _resample_alone(codec, _scale_alone(codec, plain, v), r)
        assert [g.size for g in got[s]] == [a.size for a in alone] and all(g.tobytes() == a.tobytes() for g, a in zip(got[s], alone))
    assert whole[1][0][2].size == 0 and got[1][2].size > 0            # a tail with nothing left still flushes both stages
    assert codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0


def test_all_polls_in_one_call_go_to_successive_rounds_in_both_stages(codec, store, whole):
    ts, rs = _open(codec, STREAMS.values())
    flat = [w for wins in POLLS for w in wins]
    got = _polls(codec, store, [flat], ts, rs, pcm16=False)
    _close(codec, ts, rs)
    ts, rs = _open(codec, STREAMS.values())
    first = _polls(codec, store, [POLLS[0]], ts, rs, pcm16=False)              # streams abandoned half way: closed all the same
    _close(codec, ts, rs)
    for s in STREAMS:
        assert len(got[s]) == 3 and np.concatenate(got[s]).tobytes() == whole[s][1].tobytes(), s
        assert first[s][0].tobytes() == got[s][0].tobytes()
    assert codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0


def test_pcm16_tails_and_companding_are_taken_on_the_resampled_samples(codec, store, whole):
    ts, rs = _open(codec, STREAMS.values())
    flt = _polls(codec, store, POLLS, ts, rs, pcm16=False)
    _close(codec, ts, rs)
    conv = lambda f: float_to_int16(f) if f.size else f.astype(np.int16)
    thr = float(np.median(np.abs(flt[0][2])))
    for keep_thr in (1e-5, thr):
        ts, rs = _open(codec, STREAMS.values())
        pcm = _polls(codec, store, POLLS, ts, rs, pcm16=True, keep_thr=keep_thr)
        _close(codec, ts, rs)
        for s in STREAMS:
            want = [conv(flt[s][0]), conv(flt[s][1]), conv(flt[s][2][np.abs(flt[s][2]) > np.float32(keep_thr)])]
            for k, (g, w) in enumerate(zip(pcm[s], want)):
                assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (keep_thr, s, k, g.shape, w.shape)
    kept = np.abs(flt[0][2]) > np.float32(thr)
    assert 0 < kept.sum() < kept.size                                  # the large threshold strips inside the tail, on 8 kHz samples
    ts, rs = _open(codec, STREAMS.values())
    law = {0: "ulaw", 1: "alaw", 2: None, 3: "ulaw"}
    got = {s: [] for s in STREAMS}
    for wins in POLLS:
        out = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins],
                                   sample_rates=[STREAMS[w[0]][1] for w in wins], rs_streams=[rs[w[0]] for w in wins], encodings=[law[w[0]] for w in wins])
        for w, a in zip(wins, out):
            got[w[0]].append(a)
    _close(codec, ts, rs)
    for s in STREAMS:
        want = [conv(flt[s][0]), conv(flt[s][1]), conv(flt[s][2][np.abs(flt[s][2]) > THR])]
        for k, (g, w) in enumerate(zip(got[s], want)):
            w = w if law[s] is None else G711.encode(w, law[s])
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (s, k, law[s])


def test_a_call_mixes_the_four_kinds_of_window_and_each_returns_what_it_returns_alone(codec, store):
    wins = [(0, 24, 0, 12000, False), (1, 80, 24000, 36000, False), (2, 64, 12000, 15000, False), (3, 30, 12000, None, True),
            (4, 72, 20000, None, True), (5, 48, 3000, 9000, False)]
    pairs = [(1.0, 24000), (1.25, 24000), (1.0, 8000), (1.5, 8000), (1.0, 16000), (0.75, 44100)]
    alone = []
    for w, (v, r) in zip(wins, pairs):
        ts, rs = _open(codec, [(v, r)])
        kw = {}
        if v != 1.0:
            kw.update(speeds=[v], ts_streams=ts)
        if r != 24000:
            kw.update(sample_rates=[r])
        if v != 1.0 and r != 24000:
            kw.update(rs_streams=rs)
        alone.append(codec.decode_windows(store, [w], pcm16=True, keep_thr=1e-5, **kw)[0])
        _close(codec, ts, rs)
    assert all(a.size > 0 for a in alone)
    ts, rs = _open(codec, pairs)
    got = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, speeds=[v for v, _ in pairs], ts_streams=ts,
                               sample_rates=[r for _, r in pairs], rs_streams=rs)
    for i, (g, a) in enumerate(zip(got, alone)):
        assert g.dtype == a.dtype == np.int16 and g.tobytes() == a.tobytes(), (i, pairs[i], g.shape, a.shape)
    # refusals come before any launch and leave both kinds of stream as they were
    rec_t, rec_r = codec._pool("time_scale").records[ts[3]], codec._pool("resample").records[rs[3]]
    for kw in (dict(speeds=[1.5], ts_streams=[ts[3]], sample_rates=[8000]),                              # no rs_streams: today's refusal
               dict(speeds=[1.5], ts_streams=[ts[3]], sample_rates=[8000], rs_streams=[None]),
               dict(speeds=[1.5], ts_streams=[ts[3]], sample_rates=[8000], rs_streams=[rs[5]]),           # a stream at another rate
               dict(speeds=[1.5, 1.0], ts_streams=[ts[3], None], sample_rates=[8000, 8000], rs_streams=[rs[3], rs[3]])):   # speed 1 names one
        with pytest.raises(ValueError):
            codec.decode_windows(store, wins[:len(kw["speeds"])], **kw)
    assert codec._pool("time_scale").records[ts[3]] == rec_t and codec._pool("resample").records[rs[3]] == rec_r
    _close(codec, ts, rs)
    assert codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0


# ---- 2. the serial stream and the endpoint ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chat(weights):
    return _chat(weights, "f32")


def test_serial_stream_at_1_25_and_8000_hz_is_the_composition(chat, monkeypatch):
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    text = ["One more short line."]
    seen = []
    orig = chat._stream_piece_scaled

    def recording(hiddens, a, b, handles, final, pcm16=False, encoding=None, rs_handles=None):
        seen.append(([h.clone() for h in hiddens], a, b, final))
        return orig(hiddens, a, b, handles, final, pcm16, encoding, rs_handles=rs_handles)
    monkeypatch.setattr(chat, "_stream_piece_scaled", recording)
    on = dict(speed=1.25, stream_time_scale=True, sample_rate=8000, stream_resample=True)

    def run(**kw):
        return [np.asarray(c) for c in chat.infer(text, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), **kw)]
    with pytest.raises(ValueError, match="24000 Hz only"):
        run(**on, pcm16=True)
    flt = run(**on, stream_scaled_resample=True)
    assert chat.codec.time_scale_streams_in_use() == 0 and chat.codec.resample_streams_in_use() == 0 and len(flt) == len(seen) == 4
    pieces = [chat._stream_piece(hid, a, b)[0] for hid, a, b, _ in seen]             # the schedule at speed 1 and 24 kHz, float
    total = sum(p.size for p in pieces)
    x = torch.from_numpy(np.concatenate(pieces)).to(DEV)
    want = chat.codec.resample(chat.codec.time_scale(x, 1.25), 24000, 8000).cpu().numpy()
    assert total == 256 * (2 * 80 - 1) and want.size == RS.out_len(TS.out_len(total, 125), 1, 3)
    head = np.concatenate([c[0] for c in flt[:-1]])
    assert all(c.dtype == np.float32 and c.shape[0] == 1 for c in flt) and head.tobytes() == want[: head.size].tobytes()
    tail = want[head.size:]
    assert flt[-1][0].tobytes() == tail[np.abs(tail) > THR].tobytes()
    # 16-bit and mu-law: the conversion of those floats under each chunk's own peak, the companding behind it
    n = len(seen)
    pcm = run(**on, stream_scaled_resample=True, pcm16=True)
    law = run(**on, stream_scaled_resample=True, pcm16=True, encoding="ulaw")
    for k, (p, u, f) in enumerate(zip(pcm, law, flt)):
        w = float_to_int16(f[0]) if f.size else f[0].astype(np.int16)
        assert p.dtype == np.int16 and p[0].tobytes() == w.tobytes(), k
        assert u.dtype == np.uint8 and u[0].tobytes() == G711.encode(w, "ulaw").tobytes(), k
    assert len(seen) == 3 * n
    # a consumer that goes away gives both streams back
    gen = chat.infer(text, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), **on, stream_scaled_resample=True)
    next(gen)
    assert chat.codec.time_scale_streams_in_use() == 1 and chat.codec.resample_streams_in_use() == 1
    gen.close()
    assert chat.codec.time_scale_streams_in_use() == 0 and chat.codec.resample_streams_in_use() == 0


def test_endpoint_streams_ulaw_at_8000_hz_and_1_25(chat):
    from starlette.testclient import TestClient
    from chattts_amd import server
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 80, "min_new_token": 80})       # random weights do not stop on cue
    try:
        p = orig(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=80, min_new_token=80,
                 show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=voices["default"], stream_batch=24, stream_speed=12000,
                 pass_first_n_batches=2)
        want = [np.asarray(c).reshape(-1) for c in chat.infer(["A streamed sentence."], stream=True, skip_refine_text=True, split_text=False,
                                                                params_infer_code=p, pcm16=True, encoding="ulaw", speed=1.25, stream_time_scale=True,
                                                                sample_rate=8000, stream_resample=True, stream_scaled_resample=True)]
        body = {"input": "A streamed sentence.", "response_format": "ulaw", "stream": True, "speed": 1.25, "sample_rate": 8000}
        on = dict(speed=True, stream_speed=True, stream_sample_rates=(8000,), g711=True)
        with TestClient(server.create_app(chat, voices, **on)) as c:
            assert c.post("/v1/audio/speech", json=body).status_code == 400
        with TestClient(server.create_app(chat, voices, **on, stream_speed_rates=True)) as c:
            r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and all(w.dtype == np.uint8 for w in want)
        assert r.content == b"".join(w.tobytes() for w in want)
        total = 256 * (2 * 80 - 1)
        assert 0 < len(r.content) <= RS.out_len(TS.out_len(total, 125), 1, 3)
        assert chat.codec.time_scale_streams_in_use() == 0 and chat.codec.resample_streams_in_use() == 0
    finally:
        chat.InferCodeParams = orig


# ---- 3. the pooled streams ----------------------------------------------------------------------------------------------------------------
def _serial_chunks_speed_rate(chat, hid, counts, spec, speed, rate):
    """the `stream` branch of `Chat._infer` (pcm16, one text) replayed over `hid` at speed 1 and 24 kHz in float, the pieces through a fresh
    stream of the scaler, its chunks through a fresh stream of the resampler, then the serial path's conversion and tail strip"""
    pieces, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        pieces.append(chat._stream_piece([hid[:n]], length, length + spec.stream_speed, True, False)[0])
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
    pieces.append(chat._stream_piece([hid], length, None, True)[0])
    out = _resample_alone(chat.codec, _scale_alone(chat.codec, pieces, speed), rate)
    out[-1] = out[-1][np.abs(out[-1]) > THR]
    return [float_to_int16(s) if s.size else s.astype(np.int16) for s in out]


def test_pooled_streams_at_four_speed_rate_pairs_equal_the_serial_composition(weights):
    """four streams -- speed and rate, rate only, speed only, speed and another rate -- through an 8-slot pool, the chunks of a poll from
    ONE decode_windows call: every chunk == the serial composition replayed over the hidden states the pool returned, byte for byte"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec = codec
    pool = SlotPool(eng, slots=8, cap=256, hid_cap=128, per_request=True)
    rng = np.random.RandomState(35)
    plan = [(72, -1, 3000, 0, 0.75, 8000), (96, 48, 12000, 1, 1.0, 8000), (60, -1, 12000, 0, 1.25, 24000), (50, -1, 5000, 1, 2.0, 16000)]
    reqs, ts, rs = {}, {}, {}
    for i, (max_new, stop, speed, passed, v, r) in enumerate(plan):
        ids = torch.from_numpy(np.repeat(rng.randint(1, 21178, size=(int(rng.randint(4, 30)), 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(900 + 13 * i))
        reqs[i] = (ids, p, max_new, stop, StreamSpec(24, speed, passed), v, r)
        (ts[i],), (rs[i],) = _open(codec, [(v, r)])
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=reqs[i][4])
    chunks, results, groups = {}, {}, []
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            groups.append(len(got.chunks))
            pcm = codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5,
                                       speeds=[reqs[c[0]][5] for c in got.chunks], ts_streams=[ts[c[0]] for c in got.chunks],
                                       sample_rates=[reqs[c[0]][6] for c in got.chunks], rs_streams=[rs[c[0]] for c in got.chunks])
            for c, a in zip(got.chunks, pcm):
                chunks.setdefault(c[0], []).append(a)
        else:
            results[got[0]] = (got[1].cpu().numpy(), got[2])
    _close(codec, ts.values(), rs.values())
    assert sorted(results) == [0, 1, 2, 3] and sorted(chunks) == [0, 1, 2, 3] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec, v, r) in reqs.items():
        ref, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        assert np.array_equal(results[i][0], ref.ids[0].cpu().numpy()), i
        if v == 1.0:
            want = _serial_chunks_rate(chat, results[i][1], counts, spec, r)
        elif r == 24000:
            want = _serial_chunks_speed(chat, results[i][1], counts, spec, v)
        else:
            want = _serial_chunks_speed_rate(chat, results[i][1], counts, spec, v, r)
        got = chunks[i]
        assert [g.shape for g in got] == [w.shape for w in want], (i, v, r, [g.shape for g in got], [w.shape for w in want])
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (i, v, r, k)
    assert codec.time_scale_streams_in_use() == 0 and codec.resample_streams_in_use() == 0
    pool.close()

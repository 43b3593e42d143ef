"""Streams at other speeds on the GPU, through every layer: `decode_windows(speeds=, ts_streams=)` against the stream step applied to
the plain call's float chunks and the host conversion of that, the serial stream against its speed-1 schedule replayed over the recorded
hidden states and put through the scaler, streams at four speeds through a real pool against that serial composition, and the endpoint.
Synthetic weights.  `pytest -m gpu`."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import engine as E, g711 as G711, timescale as TS  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, StreamEvents, StreamSpec  # noqa: E402
from tests.test_gpu_stream_pool import _alone_stream, _engine  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params, _serial_chunks_rate, _store  # noqa: E402

DEV = torch.device("cuda:0")
THR = np.float32(1e-5)

# (slot, prefix tokens, s_lo, s_hi, tail), speed: a first chunk at sample 0, interior chunks, a chunk clipped by its prefix's end, tails at
# a speed and at speed 1, a one-sample push (an empty chunk)
SWINDOWS = [((0, 24, 0, 12000, False), 1.25), ((1, 80, 24000, 36000, False), 0.5), ((2, 64, 12000, 15000, False), 1.0),
            ((3, 30, 12000, 24000, False), 2.0), ((4, 72, 20000, None, True), 0.77), ((5, 48, 3000, 6000, False), 1.5),
            ((6, 80, 36000, None, True), 1.0), ((7, 40, 9000, 9001, False), 1.01)]


def _scale_alone(codec, pieces, speed):
    """the float pieces of ONE stream (the last one its tail) through a fresh stream of the scaler, one step each -> float chunks"""
    h = codec.time_scale_stream_open(speed)
    try:
        out = []
        for k, f in enumerate(pieces):
            x = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(DEV)
            y, off = codec.time_scale_stream_step(x, [(h, 0, x.numel(), k == len(pieces) - 1)])
            out.append(y.cpu().numpy())
        return out
    finally:
        codec.time_scale_stream_close(h)


def _open(codec, speeds):
    return [None if TS.quantize(v)[0] == 100 else codec.time_scale_stream_open(v) for v in speeds]


def _close(codec, hs):
    for h in hs:
        if h is not None:
            codec.time_scale_stream_close(h)


# ---- 1. decode_windows(speeds=) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_decode_windows_at_speeds_equals_the_stream_step_of_the_plain_chunks(weights, gemm):
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    store = _store()
    wins, speeds = [w for w, _ in SWINDOWS], [v for _, v in SWINDOWS]
    plain = codec.decode_windows(store, wins, pcm16=False)                       # today's call: the 24 kHz float chunks, nothing stripped
    # every window here is the only push of a fresh stream, and its last one where it is a tail
    want = [f if v == 1.0 else _scale_alone(codec, [f] if w[4] else [f, np.zeros(0, np.float32)], v)[0] for (w, v), f in zip(SWINDOWS, plain)]
    assert want[7].size == 0 and want[0].size % 512 == 0 and want[4].size == TS.out_len(plain[4].size, 77)
    for k in range(1, len(wins) + 1):
        hs = _open(codec, speeds[:k])
        got = codec.decode_windows(store, wins[:k], pcm16=False, speeds=speeds[:k], ts_streams=hs)
        _close(codec, hs)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes(), (gemm, k, i, g.shape, w.shape)
    # PCM16 and stripped tails: the host conversion of those floats, byte for byte; mu-law: g711.encode of that
    thr = float(np.median(np.abs(want[4])))
    for keep_thr in (1e-5, thr):
        hs = _open(codec, speeds)
        pcm = codec.decode_windows(store, wins, pcm16=True, keep_thr=keep_thr, speeds=speeds, ts_streams=hs)
        _close(codec, hs)
        exp = [float_to_int16(f[np.abs(f) > np.float32(keep_thr)]) if w[4] else (float_to_int16(f) if f.size else f.astype(np.int16))
               for (w, _), f in zip(SWINDOWS, want)]
        for i, (p, e) in enumerate(zip(pcm, exp)):
            assert p.dtype == np.int16 and p.tobytes() == e.tobytes(), (gemm, keep_thr, i, p.shape, e.shape)
    kept = np.abs(want[4]) > np.float32(thr)
    assert 0 < kept.sum() < kept.size
    encs = ["ulaw", None, "ulaw", "alaw", "ulaw", None, None, "ulaw"]
    hs = _open(codec, speeds)
    got = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, speeds=speeds, ts_streams=hs, encodings=encs)
    _close(codec, hs)
    exp5 = [float_to_int16(f[np.abs(f) > THR]) if w[4] else (float_to_int16(f) if f.size else f.astype(np.int16)) for (w, _), f in zip(SWINDOWS, want)]
    for i, (g, e, law) in enumerate(zip(got, exp5, encs)):
        w = e if law is None else G711.encode(e, law)
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (gemm, i, law)
    # speed-1 windows in a mixed call return the plain call's bytes; all-1.0 speeds are today's call
    old = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5)
    assert exp5[2].tobytes() == old[2].tobytes() and exp5[6].tobytes() == old[6].tobytes()
    hs = _open(codec, speeds)
    new = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, speeds=speeds, ts_streams=hs)
    _close(codec, hs)
    assert new[2].tobytes() == old[2].tobytes() and new[6].tobytes() == old[6].tobytes()
    same = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, speeds=[1.0] * len(wins), ts_streams=[None] * len(wins))
    assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(old, same))
    assert codec.time_scale_streams_in_use() == 0


def test_several_windows_of_one_stream_in_one_call_and_a_tail_with_nothing_left(weights):
    """what a pool's last poll looks like: a stream's final yield and its tail fall due together, and the tail may hold no sample -- the
    stream must still be flushed.  The windows of one stream are stepped in the order given (one launch per round)"""
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")
    store = _store()
    end = 256 * (2 * 30 - 1)
    wins = [(0, 48, 0, 12000, False), (1, 30, 0, 12000, False), (0, 48, 12000, None, True), (2, 40, 0, 5000, False), (1, 30, end, None, True),
            (1, 30, 12000, end, False)]
    plain = codec.decode_windows(store, wins, pcm16=False)
    assert plain[4].size == 0
    a = _scale_alone(codec, [plain[0], plain[2]], 1.25)
    b = _scale_alone(codec, [plain[1], plain[5], plain[4]], 0.5)
    ha, hb = codec.time_scale_stream_open(1.25), codec.time_scale_stream_open(0.5)
    # stream b's windows in push order: 1, 5, 4 -- the call lists them that way
    order = [0, 1, 2, 3, 5, 4]
    got = codec.decode_windows(store, [wins[i] for i in order], pcm16=True, keep_thr=1e-5, speeds=[1.25, 0.5, 1.25, 1.0, 0.5, 0.5],
                               ts_streams=[ha, hb, ha, None, hb, hb])
    codec.time_scale_stream_close(ha)
    codec.time_scale_stream_close(hb)
    strip = lambda f: float_to_int16(f[np.abs(f) > THR]) if (np.abs(f) > THR).any() else f[:0].astype(np.int16)
    want = [float_to_int16(a[0]), float_to_int16(b[0]), strip(a[1]), float_to_int16(plain[3]), float_to_int16(b[1]), strip(b[2])]
    assert b[2].size > 0 and sum(x.size for x in b) == TS.out_len(end, 50) and sum(x.size for x in a) == TS.out_len(256 * 95, 125)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (i, g.shape, w.shape)
    # a poll that holds nothing but such a tail: no window is decoded, the stream is flushed
    h = codec.time_scale_stream_open(0.5)
    first = codec.decode_windows(store, [wins[1], wins[5]], pcm16=False, speeds=[0.5, 0.5], ts_streams=[h, h])
    last = codec.decode_windows(store, [wins[4]], pcm16=False, keep_thr=1e-5, speeds=[0.5], ts_streams=[h])
    codec.time_scale_stream_close(h)
    assert first[0].tobytes() == b[0].tobytes() and first[1].tobytes() == b[1].tobytes()
    assert last[0].tobytes() == b[2][np.abs(b[2]) > THR].tobytes()
    # refusals leave the streams as they were
    h = codec.time_scale_stream_open(1.25)
    for kw in (dict(speeds=[1.25], ts_streams=[None]), dict(speeds=[0.5], ts_streams=[h]), dict(speeds=[1.25], ts_streams=[h], sample_rates=[8000]),
               dict(speeds=[1.25])):
        with pytest.raises(ValueError):
            codec.decode_windows(store, [wins[0]], **kw)
    assert codec._pool("time_scale").records[h] == (125, 100, 0, 0, False)
    codec.time_scale_stream_close(h)


# ---- 2. the serial stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_serial_stream_at_1_25_is_the_speed_1_schedule_through_the_scaler(weights, dtype, monkeypatch):
    chat = _chat(weights, dtype)
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    text = ["One more short line."]
    seen = []
    orig = chat._stream_piece_scaled

    def recording(hiddens, a, b, handles, final, pcm16=False, encoding=None):
        seen.append(([h.clone() for h in hiddens], a, b, final))
        return orig(hiddens, a, b, handles, final, pcm16, encoding)
    monkeypatch.setattr(chat, "_stream_piece_scaled", recording)

    def run(**kw):
        return [np.asarray(c) for c in chat.infer(text, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), **kw)]
    with pytest.raises(ValueError, match="path"):
        run(speed=1.25, pcm16=True)
    base = run(pcm16=True)
    got = run(speed=1.25, stream_time_scale=True, pcm16=True)
    assert chat.codec.time_scale_streams_in_use() == 0 and len(got) == len(base) == len(seen) == 4
    # the same schedule at speed 1 over the recorded hidden states (today's `_stream_piece`, float), then the scaler, then the conversion
    pieces = [chat._stream_piece(hid, a, b) for hid, a, b, _ in seen]
    assert [p.shape[1] for p in pieces[:-1]] == [c.shape[1] for c in base[:-1]] == [3000, 3000, 3000]
    scaled = _scale_alone(chat.codec, [p[0] for p in pieces], 1.25)
    total = sum(p.shape[1] for p in pieces)
    assert total == 256 * (2 * 80 - 1) and sum(s.size for s in scaled) == TS.out_len(total, 125)
    for k, (g, s) in enumerate(zip(got, scaled)):
        if k == len(got) - 1:
            s = s[np.abs(s) > THR]
        want = float_to_int16(s) if s.size else s.astype(np.int16)
        assert g.shape == (1, want.size) and g.dtype == np.int16 and g[0].tobytes() == want.tobytes(), (dtype, k, g.shape, want.shape)
    # float chunks, mu-law chunks, and the whole-prefix decode per yield (`incremental_stream=False`): the same lengths
    flt = run(speed=1.25, stream_time_scale=True)
    assert [c.shape for c in flt[:-1]] == [c.shape for c in got[:-1]] and all(c.dtype == np.float32 for c in flt)
    assert [c.tobytes() for c in flt[:-1]] == [s.tobytes() for s in scaled[:-1]]
    law = run(speed=1.25, stream_time_scale=True, pcm16=True, encoding="ulaw")
    assert [c.tobytes() for c in law] == [G711.encode(c, "ulaw").tobytes() for c in got]
    if dtype == "f32":
        chat.incremental_stream = False
        ref = run(speed=1.25, stream_time_scale=True, pcm16=True)
        chat.incremental_stream = True
        assert [c.shape for c in ref[:-1]] == [c.shape for c in got[:-1]] and abs(ref[-1].shape[1] - got[-1].shape[1]) <= 8
    # a consumer that goes away gives the streams back
    gen = chat.infer(text, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), speed=0.8, stream_time_scale=True)
    next(gen)
    assert chat.codec.time_scale_streams_in_use() == 1
    gen.close()
    assert chat.codec.time_scale_streams_in_use() == 0


# ---- 3. the pooled stream ---------------------------------------------------------------------------------------------------------------
def _serial_chunks_speed(chat, hid, counts, spec, speed):
    """the `stream` branch of `Chat._infer` (pcm16, one text) replayed over `hid` at speed 1 in float, the pieces through a fresh stream of
    the scaler, then the serial path's conversion and tail strip"""
    pieces, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        pieces.append(chat._stream_piece([hid[:n]], length, length + spec.stream_speed, True, False)[0])
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
    pieces.append(chat._stream_piece([hid], length, None, True)[0])
    scaled = _scale_alone(chat.codec, pieces, speed)
    scaled[-1] = scaled[-1][np.abs(scaled[-1]) > THR]
    return [float_to_int16(s) if s.size else s.astype(np.int16) for s in scaled]


def test_pooled_streams_at_four_speeds_equal_the_serial_composition(weights):
    """four streams at 0.75, 1.0, 1.25 and 2.0 through an 8-slot pool, the chunks of a poll from ONE decode_windows call: every chunk ==
    the serial composition replayed over the hidden states the pool returned, byte for byte; ids == the request generated alone"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec = codec
    pool = SlotPool(eng, slots=8, cap=256, hid_cap=128, per_request=True)
    rs = np.random.RandomState(34)
    plan = [(72, -1, 3000, 0, 0.75), (96, 48, 12000, 1, 1.0), (60, -1, 12000, 0, 1.25), (50, -1, 5000, 1, 2.0)]
    reqs, hs = {}, {}
    for i, (max_new, stop, speed, passed, v) in enumerate(plan):
        ids = torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(int(rs.randint(4, 30)), 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(900 + 13 * i))
        reqs[i] = (ids, p, max_new, stop, StreamSpec(24, speed, passed), v)
        hs[i] = None if v == 1.0 else codec.time_scale_stream_open(v)
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=reqs[i][4])
    chunks, results, groups = {}, {}, []
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            groups.append(len(got.chunks))
            pcm = codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5,
                                       speeds=[reqs[c[0]][5] for c in got.chunks], ts_streams=[hs[c[0]] for c in got.chunks])
            for c, a in zip(got.chunks, pcm):
                chunks.setdefault(c[0], []).append(a)
        else:
            results[got[0]] = (got[1].cpu().numpy(), got[2])
    for h in hs.values():
        if h is not None:
            codec.time_scale_stream_close(h)
    assert sorted(results) == [0, 1, 2, 3] and sorted(chunks) == [0, 1, 2, 3] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec, v) in reqs.items():
        ref, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        assert np.array_equal(results[i][0], ref.ids[0].cpu().numpy()), i
        want = _serial_chunks_rate(chat, results[i][1], counts, spec, 24000) if v == 1.0 else _serial_chunks_speed(chat, results[i][1], counts, spec, v)
        got = chunks[i]
        assert [g.shape for g in got] == [w.shape for w in want], (i, v, [g.shape for g in got], [w.shape for w in want])
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (i, v, k)
        n = results[i][1].shape[0]
        assert 0 < sum(g.size for g in got) <= TS.out_len(256 * (2 * n - 1), TS.quantize(v)[0])      # the chunks tile the scaled stream; the tail is stripped
        if v != 1.0:
            assert all(g.size % 512 == 0 for g in got[:-1])
    assert codec.time_scale_streams_in_use() == 0
    pool.close()


# ---- 4. the endpoint --------------------------------------------------------------------------------------------------------------------
def test_endpoint_streams_at_1_25(weights):
    from starlette.testclient import TestClient
    from chattts_amd import server
    chat = _chat(weights, "f32")
    torch.manual_seed(11)
    voices = {"default": chat.sample_random_speaker()}
    orig = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig(**{**kw, "max_new_token": 80, "min_new_token": 80})       # random weights do not stop on cue
    try:
        p = orig(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=80, min_new_token=80,
                 show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=voices["default"], stream_batch=24, stream_speed=12000,
                 pass_first_n_batches=2)
        want = [np.asarray(c).reshape(-1) for c in chat.infer(["A streamed sentence."], stream=True, skip_refine_text=True, split_text=False,
                                                                params_infer_code=p, pcm16=True, speed=1.25, stream_time_scale=True)]
        body = {"input": "A streamed sentence.", "response_format": "wav", "stream": True, "speed": 1.25}
        with TestClient(server.create_app(chat, voices, speed=True)) as c:
            assert c.post("/v1/audio/speech", json=body).status_code == 400
        with TestClient(server.create_app(chat, voices, speed=True, stream_speed=True)) as c:
            r = c.post("/v1/audio/speech", json=body)
            r1 = c.post("/v1/audio/speech", json={**body, "speed": 1.0})
        assert r.status_code == 200 and r1.status_code == 200 and r.content[:44] == server.wav_stream_header()
        assert r.content[44:] == b"".join(w.astype("<i2").tobytes() for w in want)
        # the length is that of the scaled stream: every chunk but the tail a whole number of hops, the sum out_len(total) less what the
        # tail's silence strip removed
        total = 256 * (2 * 80 - 1)
        n = (len(r.content) - 44) // 2
        assert all(w.size % 512 == 0 for w in want[:-1]) and 0 < n <= TS.out_len(total, 125) and (len(r1.content) - 44) // 2 <= total
        assert sum(w.size for w in want[:-1]) == 512 * TS.frames_final(sum((12000, 12000)), 125)      # two yields of 12,000 samples reached the scaler
        assert chat.codec.time_scale_streams_in_use() == 0
    finally:
        chat.InferCodeParams = orig

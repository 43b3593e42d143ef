"""Pause streams end to end: `Chat.infer(stream=True, pauses=, stream_pauses=True)` and the endpoint against the float chunks of the
same request without the option pushed through the NumPy twin (`pauses.StreamPauses`), then the host conversion, `g711.encode`, the host
FLAC stream encoder and the limiter's twin -- all exact.  The spec's threshold is set from the un-paused stream's own frame peaks, so
that the synthetic decode has frames on both sides of it whatever its level.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import flac as FLAC, g711 as G711, limiter as LM, pauses as PA  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from tests.test_gpu_limiter_stream_e2e import _floats  # noqa: E402
from tests.test_gpu_stream_resample import _chat, _params  # noqa: E402

THR = np.float32(1e-5)
TEXT = ["One more short line."]


@pytest.fixture(scope="module")
def chat(weights):
    return _chat(weights, "f32")


@pytest.fixture(autouse=True)
def every_stream_given_back(chat):
    yield
    c = chat.codec
    assert (c.trim_pauses_streams_in_use(), c.peak_limit_streams_in_use(), c.flac_streams_in_use(), c.time_scale_streams_in_use(),
            c.resample_streams_in_use()) == (0, 0, 0, 0, 0)


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


def _spec(pre, rate):
    """a spec whose threshold is the median frame peak of the un-paused stream: frames on both sides, runs longer than P = 2 frames"""
    x = np.concatenate(pre)
    F = rate // 100
    peaks = np.abs(x[: len(x) // F * F]).reshape(-1, F).max(1)
    db = float(np.clip(20 * np.log10(max(float(np.median(peaks)), 1e-5)), -100, 0))
    return dict(max_pause_ms=20, lead_ms=10, tail_ms=20, pad_ms=0, threshold_db=db)


def _paused(pre, rate, spec):
    tw = PA.StreamPauses(rate, spec)
    out = [tw.push(c, k == len(pre) - 1) for k, c in enumerate(pre)]
    assert np.concatenate(out).tobytes() == PA.apply(np.concatenate(pre), rate, spec)[0].tobytes()
    return out, tw.record


def _pcm(chunks):
    return [float_to_int16(c) if c.size else c.astype(np.int16) for c in chunks]


@pytest.mark.parametrize("v,r", [(1.0, 24000), (1.0, 8000), (1.25, 8000)])
def test_the_serial_stream_in_every_format_is_the_twin_over_its_float_stream(chat, spoken, v, r):
    spk, seen = spoken
    on = {}
    if r != 24000:
        on.update(sample_rate=r, stream_resample=True)
    if v != 1.0:
        on.update(speed=v, stream_time_scale=True, **({"stream_scaled_resample": True} if r != 24000 else {}))
    pre = _floats(chat, seen, v, r)
    spec = _spec(pre, r)
    cut, rec = _paused(pre, r, spec)
    assert 0 < rec[7] < sum(c.size for c in pre) and rec[1] > 0          # something goes, something stays
    last = cut[-1][np.abs(cut[-1]) > THR]

    def run(**kw):
        out = list(chat.infer(TEXT, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), pauses=spec,
                              stream_pauses=True, **on, **kw))
        assert all(isinstance(c, list) and len(c) == 1 for c in out) and len(out) == len(pre)
        return [np.asarray(c[0]) for c in out]
    with pytest.raises(ValueError, match="run state carried across chunks"):
        chat.infer(TEXT, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), pauses=spec, **on)
    flt = run()
    assert [c.size for c in flt[:-1]] == [c.size for c in cut[:-1]]
    assert all(c.dtype == np.float32 and c.tobytes() == w.tobytes() for c, w in zip(flt[:-1], cut[:-1])) and flt[-1].tobytes() == last.tobytes()
    want = _pcm([*cut[:-1], last])
    pcm, law = run(pcm16=True), run(pcm16=True, encoding="ulaw")
    for k, (p, u, w) in enumerate(zip(pcm, law, want)):
        assert p.dtype == np.int16 and p.tobytes() == w.tobytes(), k
        assert u.dtype == np.uint8 and u.tobytes() == G711.encode(w, "ulaw").tobytes(), k
    enc = FLAC.StreamEncoder(r)
    frames = [enc.push(np.ascontiguousarray(w), k == len(want) - 1) for k, w in enumerate(want)]
    assert [g.tobytes() for g in run(pcm16=True, flac=True, stream_flac=True)] == [bytes(f) for f in frames]
    # in front of the limiter stream: the paused chunks are the limiter's pushes
    g32 = LM.check_gain_db(6.0)
    tw = LM.StreamLimiter(r, g32)
    lim = [tw.push(c, k == len(cut) - 1) for k, c in enumerate(cut)]
    want = _pcm([*lim[:-1], lim[-1][np.abs(lim[-1]) > THR]])
    got = run(pcm16=True, limiter=True, stream_limiter=True, gain_db=6.0)
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    gen = chat.infer(TEXT, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), pauses=spec,
                     stream_pauses=True, pcm16=True, flac=True, stream_flac=True, **on)
    next(gen)
    assert chat.codec.trim_pauses_streams_in_use() == 1
    gen.close()                                 # a consumer that goes away gives every stream back (the fixture checks all pools)


def test_two_rows_yield_per_row_lists_and_the_refusals_come_before_anything_is_generated(chat, spoken):
    spk, _ = spoken
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk))
    texts = ["One more short line.", "A second, rather longer line of text to speak."]
    seen, orig = [], chat._stream_piece

    def recording(hiddens, a, b, *args, **kw2):
        seen.append(([h.clone() for h in hiddens], a, b))
        return orig(hiddens, a, b, *args, **kw2)
    chat._stream_piece = recording
    try:
        n_plain = len(list(chat.infer(texts, **kw)))
    finally:
        del chat._stream_piece
    pre = [chat._stream_piece(hid, a, b) for hid, a, b in seen]          # the float chunks, the last one before its column filter
    spec = _spec([c[0] for c in pre], 24000)
    got = list(chat.infer(texts, **kw, pauses=spec, stream_pauses=True))
    assert len(got) == len(pre) == n_plain and all(isinstance(c, list) and len(c) == 2 for c in got)
    for row in range(2):
        cut, _ = _paused([c[row] for c in pre], 24000, spec)
        assert [c[row].tobytes() for c in got[:-1]] == [c.tobytes() for c in cut[:-1]], row
        assert got[-1][row].tobytes() == cut[-1][np.abs(cut[-1]) > THR].tobytes(), row
    for bad, why in [(dict(pauses=[spec, spec]), "one pause spec for the whole batch"), (dict(pauses=spec, split_text=True), "split_text"),
                     (dict(pauses=spec, use_decoder=False), "use_decoder=True"), (dict(pauses={"max_pause_ms": 2000}), "a slot holds 112"),
                     (dict(pauses={"max_pause": 1}), "unknown field")]:
        with pytest.raises(ValueError, match=why):
            chat.infer(texts, **{**kw, "stream_pauses": True, **bad})


def test_the_endpoint_serves_a_paused_stream_when_switched_on(chat, spoken):
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
        spec = _spec(flt, 8000)
        today = b"".join(np.asarray(c).tobytes() for c in chat.infer(["A streamed sentence."], **kw))
        want = b"".join(np.asarray(c[0]).tobytes() for c in chat.infer(["A streamed sentence."], **kw, pauses=spec, stream_pauses=True))
        body = {"input": "A streamed sentence.", "response_format": "ulaw", "stream": True, "sample_rate": 8000}
        on = dict(stream_sample_rates=(8000,), g711=True, pauses=True)
        with TestClient(server.create_app(chat, voices, **on)) as c:           # off: today's refusal
            r = c.post("/v1/audio/speech", json={**body, "pauses": spec})
            assert r.status_code == 400 and "run state" in r.text and "stream_pauses" not in c.get("/health").json()
        with TestClient(server.create_app(chat, voices, **on, stream_pauses=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "pauses": spec})
            assert r.status_code == 200 and r.content == want and 0 < len(want) < len(today)
            r = c.post("/v1/audio/speech", json={**body, "pauses": {"max_pause_ms": 2000}})
            assert r.status_code == 400 and "a slot holds 112" in r.text
            assert c.post("/v1/audio/speech", json={**body, "pauses": {"pause": 1}}).status_code == 400
            assert c.post("/v1/audio/speech", json=body).content == today and c.get("/health").json()["stream_pauses"] is True
        import threading
        from chattts_amd.serving import SpeechBatcher
        bat = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_pauses=True)      # from the pool: the same bytes
        try:
            with TestClient(server.create_app(chat, voices, **on, stream_pauses=True, batcher=bat, batch_streams=True)) as c:
                r = c.post("/v1/audio/speech", json={**body, "pauses": spec})
                assert r.status_code == 200 and r.content == want and bat.occupancy()["stream_paused_chunks"] > 0
                assert c.post("/v1/audio/speech", json={**body, "pauses": {"max_pause_ms": 2000}}).status_code == 400
        finally:
            bat.close()
    finally:
        chat.InferCodeParams = orig


# ---- decode_windows(pauses=, pa_streams=) ------------------------------------------------------------------------------------------------
import threading  # noqa: E402
import time  # noqa: E402

from chattts_amd import engine as E  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests.test_gpu_limiter_stream_e2e import LAWS, POLLS, STREAMS, _converted, _limited, _run  # noqa: E402
from tests.test_gpu_resample_stream_e2e import _close, _open  # noqa: E402
from tests.test_gpu_stream_resample import _store  # noqa: E402

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="f32")


@pytest.fixture(scope="module")
def store():
    return _store()


@pytest.fixture(scope="module")
def plain(codec, store):
    """per stream of the four float stages: today's float chunks, its spec, the twin's paused chunks and record -- once"""
    ts, rs = _open(codec, STREAMS.values())
    flt = _run(codec, store, POLLS, ts, rs, pcm16=False)
    _close(codec, ts, rs)
    out = {}
    for s, (v, r) in STREAMS.items():
        spec = _spec(flt[s], r)
        cut, rec = _paused(flt[s], r, spec)
        assert 0 < rec[7] < sum(c.size for c in flt[s]), (s, rec)
        out[s] = (flt[s], spec, cut, rec)
    return out


def _windows(codec, store, plain, polls, lm=None, fl=None, **kw):
    ts, rs = _open(codec, STREAMS.values())
    pa = {s: codec.trim_pauses_stream_open(r, plain[s][1]) for s, (_, r) in STREAMS.items()}
    try:
        got = {s: [] for s in STREAMS}
        for wins in polls:
            lkw = {} if lm is None else dict(limiter=[True] * len(wins), lm_streams=[lm[w[0]] for w in wins])
            fkw = {} if fl is None else dict(flac=[True] * len(wins), flac_streams=[fl[w[0]] for w in wins])
            out = codec.decode_windows(store, wins, speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins],
                                       sample_rates=[STREAMS[w[0]][1] for w in wins], rs_streams=[rs[w[0]] for w in wins],
                                       pauses=[plain[w[0]][1] for w in wins], pa_streams=[pa[w[0]] for w in wins], **lkw, **fkw, **kw)
            for w, a in zip(wins, out):
                got[w[0]].append(a)
        recs = {s: codec.trim_pauses_stream_stats(pa[s])["record"] for s in STREAMS}
    finally:
        _close(codec, ts, rs)
        for h in pa.values():
            codec.trim_pauses_stream_close(h)
    assert codec.trim_pauses_streams_in_use() == 0
    return got, recs


@pytest.mark.parametrize("one_call", [False, True])
def test_windows_behind_every_float_stage_equal_the_twin(codec, store, plain, one_call):
    polls = [[w for wins in POLLS for w in wins]] if one_call else POLLS          # one call: a stream's windows go to successive rounds
    flt, recs = _windows(codec, store, plain, polls, pcm16=False)
    for s in STREAMS:
        _, _, cut, rec = plain[s]
        assert [a.size for a in flt[s]] == [c.size for c in cut], s
        assert all(a.dtype == np.float32 and a.tobytes() == c.tobytes() for a, c in zip(flt[s], cut)) and list(recs[s]) == list(rec), s


def test_the_limiter_the_conversion_the_companding_and_flac_act_on_the_paused_samples(codec, store, plain):
    got, _ = _windows(codec, store, plain, POLLS, pcm16=True, keep_thr=1e-5, encodings=[LAWS[w[0]] for w in POLLS[0]])
    for s in STREAMS:                                                             # stream 1: mu-law at 8 kHz
        for k, (a, w) in enumerate(zip(got[s], _converted(plain[s][2], LAWS[s]))):
            assert a.dtype == w.dtype and a.tobytes() == w.tobytes(), (s, k)
    gains = {s: np.float32(1.6 / max(np.abs(c).max() for c in plain[s][2] if c.size)) for s in STREAMS}
    lm = {s: codec.peak_limit_stream_open(r, gains[s]) for s, (_, r) in STREAMS.items()}
    try:
        got, _ = _windows(codec, store, plain, POLLS, lm=lm, pcm16=True, keep_thr=1e-5)
    finally:
        for h in lm.values():
            codec.peak_limit_stream_close(h)
    for s, (_, r) in STREAMS.items():
        lim, rec = _limited(plain[s][2], r, gains[s])
        assert rec["n_over"] > 0
        assert [a.tobytes() for a in got[s]] == [w.tobytes() for w in _converted(lim)], s
    fl = {s: codec.flac_stream_open(r) for s, (_, r) in STREAMS.items()}
    try:
        got, _ = _windows(codec, store, plain, POLLS, fl=fl, pcm16=True, keep_thr=1e-5)
    finally:
        for h in fl.values():
            codec.flac_stream_close(h)
    for s, (_, r) in STREAMS.items():                                             # the host twin over the int16 chunks, frame for frame
        enc, want = FLAC.StreamEncoder(r), _converted(plain[s][2])
        frames = [enc.push(np.ascontiguousarray(w), k == len(want) - 1) for k, w in enumerate(want)]
        assert [a.tobytes() for a in got[s]] == [bytes(f) for f in frames], s


def test_flags_off_return_todays_bytes_and_bad_tables_are_refused(codec, store, plain):
    ts, rs = _open(codec, STREAMS.values())
    h = codec.trim_pauses_stream_open(24000, True)
    try:
        wins = POLLS[0]
        kw = dict(speeds=[STREAMS[w[0]][0] for w in wins], ts_streams=[ts[w[0]] for w in wins], sample_rates=[STREAMS[w[0]][1] for w in wins],
                  rs_streams=[rs[w[0]] for w in wins], encodings=[LAWS[w[0]] for w in wins])
        today = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw)
        _close(codec, ts, rs)
        for flags in ([None] * 4, [False] * 4):
            ts, rs = _open(codec, STREAMS.values())
            kw.update(ts_streams=[ts[w[0]] for w in wins], rs_streams=[rs[w[0]] for w in wins])
            off = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, **kw, pauses=flags, pa_streams=[None] * 4)
            _close(codec, ts, rs)
            assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(off, today))
        ts, rs = _open(codec, STREAMS.values())
        before = dict(codec.trim_pauses_stream_stats(h))
        for bad, why in [(dict(pauses=[True], pa_streams=[None]), "needs an open pause stream at 24000 Hz"), (dict(pauses=[True]), "one pauses flag"),
                         (dict(pauses=[True, None], pa_streams=[h, h]), "no pauses flag but names"), (dict(pa_streams=[h]), "pa_streams without a pauses flag"),
                         (dict(pauses=[True], pa_streams=[h], sample_rates=[8000]), "at 8000 Hz")]:
            with pytest.raises(ValueError, match=why):
                codec.decode_windows(store, [POLLS[0][0]] * len(bad.get("pauses", [0])), **bad)
        with pytest.raises(ValueError, match="has had its last push"):
            codec.decode_windows(store, [POLLS[2][0], POLLS[0][0]], pauses=[True, True], pa_streams=[h, h])
        after = codec.trim_pauses_stream_stats(h)
        assert (after["pushed"], after["done"]) == (before["pushed"], before["done"]) == (0, False)
    finally:
        _close(codec, ts, rs)
        codec.trim_pauses_stream_close(h)


# ---- the batcher -----------------------------------------------------------------------------------------------------
def test_the_batcher_returns_the_serial_calls_bytes_and_gives_its_slots_back(chat, spoken):
    spk, _ = spoken
    text = "One more short line."
    kw = dict(stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk))
    spec = _spec([np.asarray(c)[0] for c in chat.infer([text], **kw)], 24000)
    want = [np.asarray(c[0]) for c in chat.infer([text], **kw, pcm16=True, pauses=spec, stream_pauses=True)]
    off = SpeechBatcher(chat, 2, threading.Lock(), streams=True)
    try:
        with pytest.raises(ValueError, match="run state carried across chunks"):
            off.submit_stream(text, _params(chat, spk), pauses=spec)
        assert "stream_paused_chunks" not in off.occupancy()
    finally:
        off.close()
    b = SpeechBatcher(chat, 2, threading.Lock(), streams=True, stream_pauses=True)
    try:
        with pytest.raises(ValueError, match="submit_stream: this spec makes a stream hold"):
            b.submit_stream(text, _params(chat, spk), pauses={"max_pause_ms": 2000})
        got = list(b.submit_stream(text, _params(chat, spk), pauses=spec))
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want] and all(g.dtype == np.int16 for g in got)
        assert b.occupancy()["stream_paused_chunks"] == len(want)
        deadline = time.time() + 30
        while chat.codec.trim_pauses_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.trim_pauses_streams_in_use() == 0
        s = b.submit_stream(text, _params(chat, spk), pauses=spec)                # a cancelled one gives its slot back
        next(s)
        s.close()
        deadline = time.time() + 30
        while chat.codec.trim_pauses_streams_in_use() and time.time() < deadline:
            time.sleep(0.01)
        assert chat.codec.trim_pauses_streams_in_use() == 0 and b.occupancy()["cancelled"] == 1
    finally:
        b.close()

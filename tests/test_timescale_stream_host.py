"""Host side of the streamed time scaler: when a frame is final (`need`, `frames_final`), what a stream keeps (`base`, the carry
constant), `stream_plan` over random push schedules at every speed, the float64 oracle's reads against those bounds, the NumPy twin
sliced at the plan's chunk edges, the refusals in Python and in the library, and the default-off plumbing on fakes."""
import ctypes as C
import logging
import threading

import numpy as np
import pytest

from chattts_amd import _lib, timescale as TS
from tests.timescale_oracle import HOP, RAD, WIN, time_scale_f64

SPEEDS = [n / 100 for n in range(50, 201) if n != 100]
PUSHES = (0, 1, 7, 511, 512, 513, 3000, 12000)
TOTALS = (1, 511, 512, 513, 2000, 20000)


def _schedule(rng, total):
    """push sizes from PUSHES (the last one cut to fit) that add up to `total`; sometimes an empty last push"""
    sizes, left = [], total
    while left > 0:
        n = min(int(rng.choice(PUSHES)), left)
        sizes.append(n)
        left -= n
    if rng.integers(2):
        sizes.append(0)
    return sizes


def _walk(speed, sizes):
    """the plans of a stream pushed in `sizes`, the last push final"""
    pushed, plans = 0, []
    for i, n in enumerate(sizes):
        plans.append(TS.stream_plan(speed, pushed, n, i == len(sizes) - 1))
        pushed += n
    return plans


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def test_there_are_150_speeds_and_the_constants_are_the_stated_ones():
    assert len(SPEEDS) == 150 and (TS.N, TS.HS, TS.D) == (WIN, HOP, RAD)
    assert TS.CARRY == 2560 and _lib.TS_STREAM.itemsize == 80


def test_need_and_base_by_their_formulas():
    for num in (50, 77, 99, 101, 125, 200):
        a = lambda k: k * HOP * num // 100
        assert TS.need(0, num) == 0 and TS.base(0, num) == 0
        for k in (1, 2, 3, 10, 57):
            assert TS.a_of(k, num) == a(k)
            assert TS.need(k, num) == max(a(k - 1) + RAD + WIN - 1, a(k) - HOP + RAD + WIN - 1)
            assert TS.base(k, num) == max(0, a(k) - HOP - RAD)
        # the template's reach decides below speed 1, the span's end above it
        assert (TS.need(5, num) == a(4) + RAD + WIN - 1) == (num <= 100)


@pytest.mark.parametrize("num", [50, 51, 99, 101, 125, 199, 200])
def test_frames_final_is_the_largest_frame_whose_need_is_met(num):
    for n_avail in list(range(0, 4000, 37)) + [TS.need(k, num) + d for k in (1, 2, 7, 40) for d in (-1, 0, 1)]:
        K = TS.frames_final(n_avail, num)
        assert TS.need(K, num) <= n_avail < TS.need(K + 1, num), (num, n_avail, K)


def test_every_speed_random_schedules_tile_the_output_and_stay_under_the_carry():
    rng = np.random.default_rng(20240)
    worst = 0
    for speed in SPEEDS:
        num = int(round(100 * speed))
        for total in TOTALS:
            sizes = _schedule(rng, total)
            plans = _walk(speed, sizes)
            n_out = TS.out_len(total, num)
            F = TS.frames(n_out)
            emitted, k, paths = 0, 0, 0
            for p in plans:
                assert p["k_prev"] == k and p["k_now"] >= k, (speed, sizes)                        # K is monotone
                assert p["k_now"] <= F - 1, (speed, sizes)
                assert p["n_out"] >= 0 and p["carry_in"] <= TS.CARRY and p["carry_out"] <= TS.CARRY
                worst = max(worst, p["carry_in"], p["carry_out"])
                if p["total"] < 0:
                    assert p["n_out"] == HOP * (p["k_now"] - k) and emitted + p["n_out"] == HOP * p["k_now"]
                emitted += p["n_out"]
                paths += p["n_path"]
                k = p["k_now"]
            assert k == F - 1 and emitted == n_out and paths == F, (speed, sizes)                # the chunks tile [0, n_out)
            assert plans[-1]["total"] == total and all(p["total"] == -1 for p in plans[:-1])
    print("largest carry seen:", worst)
    assert worst < TS.CARRY


def test_the_carry_bound_holds_for_every_speed_and_every_frame_count():
    """after a step n_avail < need(K + 1): the carry is below need(K + 1) - base(K), whatever was pushed"""
    for num in range(50, 201):
        if num == 100:
            continue
        for K in range(0, 400):
            assert TS.need(K + 1, num) - 1 - TS.base(K, num) <= TS.CARRY - 1, (num, K)


def test_one_sample_pushes_tile_too():
    for speed in (0.5, 1.25, 2.0):
        plans = _walk(speed, [1] * 3000)
        assert sum(p["n_out"] for p in plans) == TS.out_len(3000, int(100 * speed)) and sum(p["n_path"] for p in plans) == TS.frames(sum(p["n_out"] for p in plans))
        assert max(p["carry_out"] for p in plans) < TS.CARRY


# ---- the oracle's reads, and the twin sliced at the chunk edges ---------------------------------------------------------------------
@pytest.mark.parametrize("speed", [0.5, 0.77, 0.99, 1.01, 1.25, 2.0])
def test_every_read_of_frame_k_lies_between_base_and_need(speed):
    num = int(round(100 * speed))
    x = np.random.default_rng(num).uniform(-1, 1, 9000).astype(np.float32)
    path = time_scale_f64(x, speed)["path"]
    for k in range(1, len(path)):
        a = k * HOP * num // 100
        # the template, the span, and the two halves of the overlap-add: every position frame k reads
        reads = [(int(path[k - 1]) + HOP, int(path[k - 1]) + HOP + WIN), (a - HOP - RAD, a - HOP + RAD + WIN - 1), (int(path[k]), int(path[k]) + HOP)]
        hi = max(b for _, b in reads)
        lo = min(a_ for a_, _ in reads)
        assert hi <= TS.need(k, num), (speed, k, hi, TS.need(k, num))
        assert max(lo, 0) >= TS.base(k - 1, num), (speed, k, lo, TS.base(k - 1, num))


@pytest.mark.parametrize("speed", [0.5, 0.77, 1.25, 2.0])
def test_apply_sliced_at_the_plans_chunk_edges_equals_the_unsliced_result(speed):
    rng = np.random.default_rng(int(100 * speed))
    x = rng.uniform(-1, 1, 20000).astype(np.float32)
    path = time_scale_f64(x, speed)["path"]
    whole = TS.apply(x, speed, path)
    sizes = _schedule(rng, len(x))
    lo = 0
    pushed = 0
    for i, (n, p) in enumerate(zip(sizes, _walk(speed, sizes))):
        pushed += n
        final = i == len(sizes) - 1
        # what the step may read: nothing at or beyond `pushed` unless the stream has ended; a copy cut there gives the same samples
        seen = x[:pushed]
        if not final:
            m = np.arange(lo, lo + p["n_out"])
            k1, j = m // HOP, m % HOP
            w = TS.window().astype(np.float32)

            def read(g):
                ok = (g >= 0) & (g < len(seen))
                return np.where(ok, seen[np.where(ok, g, 0)], np.float32(0.0)).astype(np.float32)

            got = w[j + HOP] * read(path[k1] + HOP + j) + w[j] * read(path[k1 + 1] + j)
        else:
            got = TS.apply(seen, speed, path)[lo:]
        assert got.astype(np.float32).tobytes() == whole[lo: lo + p["n_out"]].tobytes(), (speed, i)
        lo += p["n_out"]
    assert lo == len(whole)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_stream_plan_refusals():
    with pytest.raises(ValueError, match="nothing to scale"):
        TS.stream_plan(1.0, 0, 100, False)
    with pytest.raises(ValueError, match="0.5 .. 2.0"):
        TS.stream_plan(2.5, 0, 100, False)
    with pytest.raises(ValueError, match="negative"):
        TS.stream_plan(1.25, -1, 100, False)
    with pytest.raises(ValueError, match="negative"):
        TS.stream_plan(1.25, 0, -1, False)
    with pytest.raises(ValueError, match="empty stream"):
        TS.stream_plan(1.25, 0, 0, True)
    with pytest.raises(ValueError, match="2\\^31"):
        TS.stream_plan(1.25, (1 << 31) - TS.REACH - 10, 10, False)
    assert TS.stream_plan(1.25, 0, 0, False)["n_out"] == 0


def _desc(speed, pushed, n_in, final, slot=0, phase=0, **over):
    p = TS.stream_plan(speed, pushed, n_in, final)
    row = dict(in_off=0, n_in=n_in, pos=pushed, total=p["total"], out_off=0, path_off=0, k_prev=p["k_prev"], k_now=p["k_now"], slot=slot,
               phase=phase, num=p["num"], den=p["den"], n_out=p["n_out"], reserved=0)
    row.update(over)
    return row, p


def test_library_refuses_before_it_launches():
    """ctts_time_scale_stream_step checks the host mirror first: these calls fail on a machine without a GPU, with the reason"""
    lib = _lib.lib()
    fake = C.c_void_p(4096)          # never dereferenced: every call below is refused on its host arguments

    def call(rows, n_x=1 << 20, n_y=1 << 20, n_path=1 << 10, n_slots=4, null=()):
        tab = np.zeros(len(rows), _lib.TS_STREAM)
        for i, r in enumerate(rows):
            tab[i] = tuple(r[k] for k in _lib.TS_STREAM.names)
        p = {k: (None if k in null else fake) for k in ("x", "dev", "y", "path", "carry", "state", "window")}
        rc = lib.ctts_time_scale_stream_step(p["x"], n_x, p["dev"], tab.ctypes.data_as(C.c_void_p), len(rows), p["y"], n_y, p["path"], n_path,
                                             p["carry"], p["state"], n_slots, p["window"], None)
        return rc, lib.ctts_last_error().decode()

    good = lambda **o: {**_desc(1.25, 3000, 5000, False)[0], **o}
    kn = good()["k_now"]
    cases = [
        (dict(rows=[good()], null=("carry",)), "null"), (dict(rows=[good()], null=("state",)), "null"), (dict(rows=[good()], null=("window",)), "null"),
        (dict(rows=[good()], null=("dev",)), "null"), (dict(rows=[good()], null=("x",)), "null"), (dict(rows=[good()], null=("y",)), "null"),
        (dict(rows=[good()], null=("path",)), "null"),
        (dict(rows=[good(den=50)]), "num / 100"), (dict(rows=[good(num=49)]), "50 <= num <= 200"), (dict(rows=[good(num=201)]), "50 <= num <= 200"),
        (dict(rows=[good(num=100)]), "nothing to scale"),
        (dict(rows=[good(k_now=kn + 1)]), "final, got"), (dict(rows=[good(k_now=kn - 1)]), "final, got"), (dict(rows=[good(k_prev=0)]), "final, got"),
        (dict(rows=[good(total=8001)]), "last push"), (dict(rows=[good(total=7999)]), "last push"), (dict(rows=[good(total=-2)]), "last push"),
        (dict(rows=[{**_desc(1.25, 0, 0, False)[0], "total": 0}]), "last push"),
        (dict(rows=[good(n_out=good()["n_out"] + 1)]), "emits"), (dict(rows=[good(n_out=0)]), "emits"),
        (dict(rows=[good()], n_y=good()["n_out"] - 1), "outside the output"), (dict(rows=[good(out_off=5)], n_y=good()["n_out"] + 4), "outside the output"),
        (dict(rows=[good()], n_x=4999), "outside the input"), (dict(rows=[good(in_off=1)], n_x=5000), "outside the input"),
        (dict(rows=[good()], n_path=kn - good()["k_prev"] - 1), "outside the path"),
        (dict(rows=[good(slot=4)]), "outside the pool"), (dict(rows=[good(slot=-1)]), "outside the pool"),
        (dict(rows=[good(), good(slot=1), good()]), "twice"), (dict(rows=[good(phase=2)]), "phase"),
        (dict(rows=[good(n_in=-1)]), "negative"), (dict(rows=[good(pos=-1)]), "negative"), (dict(rows=[good(out_off=-8)]), "negative"),
        (dict(rows=[good(pos=(1 << 31) - 4096 - 5000)]), "2^31"), (dict(rows=[good(n_in=1 << 31)]), "2^31"),
        (dict(rows=[]), "n_streams"), (dict(rows=[good()], n_slots=0), "no slot"),
    ]
    for kw, why in cases:
        rc, msg = call(**kw)
        assert rc != 0 and "ctts_time_scale_stream_step" in msg and why in msg, (kw, msg)
    # "a carry above the capacity" cannot be reached past the frame-range check: K(pos) pins the carry below need(K + 1) - base(K)
    # (test_the_carry_bound_holds_for_every_speed_and_every_frame_count); the check stays in the library as a second line


# ---- the default-off plumbing, on fakes -------------------------------------------------------------------------------------------------
def test_chat_infer_keeps_the_refusal_without_the_flag_and_names_what_it_still_refuses():
    from chattts_amd.core import Chat
    chat = Chat.__new__(Chat)
    with pytest.raises(ValueError, match="path"):
        chat.infer(["hello"], stream=True, speed=1.25)
    with pytest.raises(ValueError, match="24000 Hz only"):
        chat.infer(["hello"], stream=True, speed=1.25, stream_time_scale=True, sample_rate=8000, stream_resample=True, split_text=False)
    with pytest.raises(ValueError, match="split_text"):
        chat.infer(["hello"], stream=True, speed=1.25, stream_time_scale=True)               # split_text is the default
    with pytest.raises(ValueError, match="use_decoder"):
        chat.infer(["hello"], stream=True, speed=1.25, stream_time_scale=True, split_text=False, use_decoder=False)
    with pytest.raises(ValueError, match="0.5 .. 2.0"):
        chat.infer(["hello"], stream=True, speed=2.5, stream_time_scale=True, split_text=False)


def test_the_engine_plans_a_polls_pushes_in_rounds_and_commits_nothing_on_its_own():
    """CodecEngine._ts_descriptors without a device: two windows of one stream in one call go to successive rounds, with the position
    and the carry phase of the second following the first; the host records change only when the caller commits"""
    from chattts_amd import statepool as SP
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    eng._pools = {"time_scale": SP.StatePool("time_scale", 4)}
    recs = eng._pools["time_scale"].records
    a, b = eng.time_scale_stream_open(1.25), eng.time_scale_stream_open(0.5)
    assert (a, b) == (0, 1) and eng.time_scale_streams_in_use() == 2
    tab, round_off, order, n_path, commit = eng._ts_descriptors([(a, 0, 3000, False), (b, 3000, 2000, False), (a, 5000, 0, True)])
    assert list(round_off) == [0, 2, 3] and order == [0, 1, 2]
    assert [int(v) for v in tab["slot"]] == [a, b, a] and [int(v) for v in tab["pos"]] == [0, 0, 3000] and [int(v) for v in tab["phase"]] == [0, 0, 1]
    assert int(tab["total"][2]) == 3000 and int(tab["total"][0]) == -1
    assert sum(int(tab["n_out"][i]) for i in (0, 2)) == TS.out_len(3000, 125) and n_path[0] + n_path[2] == TS.frames(TS.out_len(3000, 125))
    assert recs == {a: SP.TimeScaleRec(125, 100, 0, 0, False), b: SP.TimeScaleRec(50, 100, 0, 0, False)}        # nothing committed yet
    assert commit == {a: SP.TimeScaleRec(125, 100, 3000, 0, True), b: SP.TimeScaleRec(50, 100, 2000, 1, False)}
    with pytest.raises(ValueError, match="last push"):
        eng._ts_descriptors([(a, 0, 10, True), (a, 10, 10, False)])
    with pytest.raises(ValueError, match="not open"):
        eng._ts_descriptors([(7, 0, 10, False)])
    eng.time_scale_stream_close(a)
    with pytest.raises(ValueError, match="not open"):
        eng.time_scale_stream_close(a)
    assert eng.time_scale_stream_open(2.0) == a                      # the slot is handed out again, with a fresh record
    assert recs[a] == SP.TimeScaleRec(200, 100, 0, 0, False)
    with pytest.raises(ValueError, match="nothing to scale"):
        eng.time_scale_stream_open(1.0)


def test_decode_windows_refuses_a_speed_with_a_rate_and_a_speed_without_streams():
    from chattts_amd.engine import CodecEngine
    eng = CodecEngine.__new__(CodecEngine)
    wins = [(0, 40, 0, 12000), (1, 40, 0, 12000)]
    with pytest.raises(ValueError, match="24000 Hz only"):
        eng.decode_windows(None, wins, speeds=[1.25, 1.0], ts_streams=[0, None], sample_rates=[24000, 8000])
    with pytest.raises(ValueError, match="ts_streams"):
        eng.decode_windows(None, wins, speeds=[1.25, 1.0])
    with pytest.raises(ValueError, match="one speed per window"):
        eng.decode_windows(None, wins, speeds=[1.25])
    with pytest.raises(ValueError, match="0.5 .. 2.0"):
        eng.decode_windows(None, wins, speeds=[1.25, 3.0], ts_streams=[0, None])


class _TsCodec:
    """the part of CodecEngine a batcher touches for streamed speeds: open / close, recorded"""

    def __init__(self):
        self.opened, self.closed, self.free = [], [], [3, 2, 1, 0]

    def time_scale_stream_open(self, speed):
        self.opened.append((self.free[-1], speed))
        return self.free.pop()

    def time_scale_stream_close(self, h):
        self.closed.append(h)
        self.free.append(h)


def _speed_chat():
    from tests.test_stream_pool_host import _FakeChat, _piece

    class _SpeedStreamChat(_FakeChat):
        def __init__(self):
            super().__init__()
            self.codec, self.kw_calls = _TsCodec(), []

        def decode_windows_pcm16(self, store, windows, **kw):
            self.window_calls.append(list(windows))
            self.kw_calls.append(dict(kw))
            return [_piece(store[slot], prefix, a, b) for slot, prefix, a, b, tail in windows]
    return _SpeedStreamChat()


def _wait(cond, timeout=10.0):
    import time
    t0 = time.monotonic()
    while not cond():
        assert time.monotonic() - t0 < timeout, "the batcher did not get there"
        time.sleep(0.001)


def test_three_streams_at_three_speeds_due_at_one_poll_make_one_decode_call():
    from chattts_amd.serving import SpeechBatcher
    from tests.test_stream_pool_host import _FakePool, _Params
    lock, holder = threading.Lock(), {}
    chat = _speed_chat()
    b = SpeechBatcher(chat, 3, lock, make_pool=lambda: holder.setdefault("p", _FakePool(3, lock)), streams=True, stream_speeds=True)
    try:
        with pytest.raises(ValueError, match="24000 Hz only"):
            b.submit_stream("x", _Params(48), speed=1.25, sample_rate=8000)
        with pytest.raises(ValueError, match="0.5 .. 2.0"):
            b.submit_stream("x", _Params(48), speed=3.0)
        with lock:       # submitted together: admitted in one chunk, their chunks fall due at the same polls
            streams = [b.submit_stream(t, _Params(96), speed=v) for t, v in (("A", 0.75), ("B", 1.0), ("C", 1.25))]
        got = {}
        ths = [threading.Thread(target=lambda k, s: got.__setitem__(k, list(s)), args=(k, s)) for k, s in enumerate(streams)]
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=30)
        assert all(len(got[k]) > 0 for k in range(3))
        full = [(w, kw) for w, kw in zip(chat.window_calls, chat.kw_calls) if len(w) == 3]
        assert full and len(chat.window_calls) == b.occupancy()["stream_decode_calls"]          # one call per poll for the three streams
        slot_of = {}
        for w, kw in full:
            speeds = [{0: 0.75, 1: 1.0, 2: 1.25}[x[0]] for x in w]
            assert kw["speeds"] == speeds and set(kw) == {"speeds", "ts_streams"}, kw
            for x, v, h in zip(w, speeds, kw["ts_streams"]):
                assert (h is None) == (v == 1.0)
                assert slot_of.setdefault(x[0], h) == h                                           # a stream keeps its slot
        _wait(lambda: len(chat.codec.closed) == 2)
        assert sorted(chat.codec.closed) == sorted(h for h, _ in chat.codec.opened) and [v for _, v in chat.codec.opened] == [0.75, 1.25]
        occ = b.occupancy()
        assert occ["stream_scaled_chunks"] == 2 * occ["stream_chunks"] // 3 > 0
        # speed 1 alone (or none) passes no new argument: the call is today's
        n_calls = len(chat.kw_calls)
        assert len(list(b.submit_stream("D", _Params(48), speed=1.0))) > 0 and len(list(b.submit_stream("E", _Params(48)))) > 0
        assert len(chat.kw_calls) > n_calls and all(kw == {} for kw in chat.kw_calls[n_calls:]) and len(chat.codec.opened) == 2
    finally:
        b.close()
    assert not lock.locked()


def test_a_cancelled_stream_gives_its_slot_back_and_the_flag_is_off_by_default():
    from chattts_amd.serving import SpeechBatcher
    from tests.test_stream_pool_host import _FakePool, _Params
    lock, holder = threading.Lock(), {}
    chat = _speed_chat()
    b = SpeechBatcher(chat, 2, lock, make_pool=lambda: holder.setdefault("p", _FakePool(2, lock)), streams=True, stream_speeds=True)
    try:
        s = b.submit_stream("A", _Params(400), speed=1.5)
        first = next(s)
        assert len(first) > 0 and chat.codec.opened == [(0, 1.5)] and chat.codec.closed == []
        s.close()
        _wait(lambda: chat.codec.closed == [0])
        assert b.occupancy()["cancelled"] == 1
        assert len(list(b.submit_stream("B", _Params(48), speed=0.5))) > 0                      # the slot serves the next stream
        _wait(lambda: chat.codec.closed == [0, 0])
    finally:
        b.close()
    off = SpeechBatcher(_speed_chat(), 2, lock, make_pool=lambda: _FakePool(2, lock), streams=True)
    try:
        with pytest.raises(ValueError, match="non-streamed"):
            off.submit_stream("a", _Params(48), speed=1.25)
        assert "stream_scaled_chunks" in off.occupancy() and off.occupancy()["stream_scaled_chunks"] == 0
    finally:
        off.close()


def test_endpoint_matrix_of_streamed_speeds():
    from starlette.testclient import TestClient
    from chattts_amd import server
    from tests.test_split_pool_host import _EndpointChat
    from tests.test_stream_resample_host import _StreamBatcher
    body = {"input": "hello", "response_format": "wav", "stream": True}

    def app(chat, **kw):
        return TestClient(server.create_app(chat, {"default": "SPK-D"}, logger=logging.getLogger("test_timescale_stream_host"), **kw))

    chat = _EndpointChat()
    with app(chat, speed=True) as c:                                     # `speed` alone: the 400 stays, with its text
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
        assert r.status_code == 400 and "non-streamed" in r.text and "path" in r.text and not chat.calls
    chat = _EndpointChat()
    with app(chat, stream_speed=True) as c:                              # without `speed` the field is validated and ignored, as ever
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.25}).status_code == 200 and "speed" not in chat.calls[-1][2]
    chat = _EndpointChat()
    with app(chat, speed=True, stream_speed=True, stream_sample_rates=(8000,)) as c:
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25})
        text, stream, kw = chat.calls[-1]
        assert r.status_code == 200 and stream and (kw["speed"], kw["stream_time_scale"], kw["split_text"]) == (1.25, True, False)
        assert r.content[:44] == server.wav_stream_header()
        n = len(chat.calls)
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.25, "sample_rate": 8000})
        assert r.status_code == 400 and "24000 Hz only" in r.text and "look-ahead" in r.text and len(chat.calls) == n
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.0}).status_code == 200
        assert "speed" not in chat.calls[-1][2] and "stream_time_scale" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "sample_rate": 8000}).status_code == 200 and "speed" not in chat.calls[-1][2]
        assert c.post("/v1/audio/speech", json={**body, "speed": 2.5}).status_code == 422
        r = c.post("/v1/audio/speech", json={**body, "stream": False, "speed": 1.25})       # non-streamed: as before
        assert r.status_code == 200 and chat.calls[-1][2]["speed"] == 1.25 and "stream_time_scale" not in chat.calls[-1][2]
    chat, bat = _EndpointChat(), _StreamBatcher()
    bat.stream_speeds = True
    with app(chat, batcher=bat, batch_streams=True, speed=True, stream_speed=True) as c:     # through the pool
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.5})
        assert r.status_code == 200 and bat.calls[-1] == ("hello", {"speed": 1.5}) and not chat.calls
        assert c.post("/v1/audio/speech", json=body).status_code == 200 and bat.calls[-1] == ("hello", {})
    chat, bat = _EndpointChat(), _StreamBatcher()                        # a pool that was built without stream_speeds: served serially
    with app(chat, batcher=bat, batch_streams=True, speed=True, stream_speed=True) as c:
        r = c.post("/v1/audio/speech", json={**body, "speed": 1.5})
        assert r.status_code == 200 and not bat.calls and chat.calls[-1][2]["stream_time_scale"] is True
    chat, bat = _EndpointChat(), _StreamBatcher()
    bat.stream_speeds = True
    with app(chat, batcher=bat, batch_streams=True, speed=True) as c:    # the app's flag is off: the 400, whatever the pool could do
        assert c.post("/v1/audio/speech", json={**body, "speed": 1.5}).status_code == 400 and not bat.calls and not chat.calls

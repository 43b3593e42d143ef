"""Streams at other sample rates on the GPU: `resample_win_k` against the whole-signal resample bit for bit (and the float64 oracle
under the float32 bound), packed windows of mixed rates, `decode_windows(sample_rates=)` against `resample_window(decode_window(..))`
and the host conversion, the serial stream against its `incremental_stream=False` composition, streams at four rates through a real
pool against the serial schedule replayed over the pool's hidden states, and the endpoint.  `pytest -m gpu`."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import _lib, engine as E, resample as RS  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.core import Chat  # noqa: E402
from chattts_amd.serving import SlotPool, StreamEvents, StreamSpec  # noqa: E402
from tests.resample_oracle import PAIRS, oracle_taps, reduced, resample_f64  # noqa: E402
from tests.test_gpu_stream_pool import _alone_stream, _engine  # noqa: E402

DEV = torch.device("cuda:0")
TILE = RS.TILE
THR = np.float32(1e-5)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def codec(weights):
    return E.CodecEngine(weights["decoder"], weights["vocos"], DEV)


# ---- 1. the kernel against the whole-signal resample ------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_window_chunks_equal_slices_of_the_whole_resample(codec, orig, new):
    """chunks at every phase and tile position, from the tight window [a, b) and from one with 300 real samples more either side:
    == resample(x)[o_lo:o_hi] bit for bit, and within (K + 3) 2^-24 sum |h| |x| of the float64 oracle"""
    M, L = reduced(orig, new)
    h, width = oracle_taps(orig, new)
    K = h.shape[1]
    n = max(6000, 2 * TILE * M // L + K)             # the outputs span two tiles and a part of a third
    x = np.random.default_rng(3 * orig + new).uniform(-1, 1, n).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    whole = codec.resample(xd, orig, new).cpu().numpy()
    n_out = RS.out_len(n, L, M)
    assert whole.shape == (n_out,) and n_out > 2 * TILE
    want64, scale = resample_f64(x, orig, new, with_bound=True)
    bound = (K + 3) * 2.0 ** -24 * scale
    edge = (n_out - 1) // TILE * TILE                # the last tile's edge, in the whole signal's tiles
    starts = sorted({0, 1, L - 1, L, 2047, 2048, 2049, edge - 1, edge, edge + 1})
    done = 0
    for o_lo in starts:
        for m in sorted({0, 1, 7, 8, 9, 2047, 2048, 2049, n_out - o_lo}):
            o_hi = o_lo + m
            if o_hi > n_out:
                continue
            a, b = RS.window_inputs(L, M, K, o_lo, o_hi, n)
            for lo, hi in ((a, b), (max(0, a - 300), min(n, b + 300))):
                if hi == lo:                         # an empty chunk reads nothing: any window will do
                    lo, hi = 0, 1
                got = codec.resample_window(xd[lo:hi], lo, n, o_lo, o_hi, orig, new).cpu().numpy()
                assert got.shape == (m,) and got.tobytes() == whole[o_lo:o_hi].tobytes(), (o_lo, o_hi, lo, hi)
                assert np.all(np.abs(got.astype(np.float64) - want64[o_lo:o_hi]) <= bound[o_lo:o_hi]), (o_lo, o_hi)
                done += 1
    assert done > 100
    # rows: [B, n] windows of B signals at the same place
    a, b = RS.window_inputs(L, M, K, 2047, 2047 + 9, n)
    two = torch.stack([xd[a:b], -xd[a:b]])
    got = codec.resample_window(two, a, n, 2047, 2056, orig, new).cpu().numpy()
    assert got[0].tobytes() == whole[2047:2056].tobytes() and np.array_equal(got[1], -got[0])
    # a window that does not hold the inputs, outputs beyond the signal's: refused on the host
    for args in ((xd[a + 1:b], a + 1, n, 2047, 2056), (xd[a:b - 1], a, n, 2047, 2056), (xd[a:b], a, n, 2047, n_out + 1), (xd[a:b], a, n, 9, 8),
                 (xd, 1, n, 0, 8)):
        with pytest.raises(ValueError):
            codec.resample_window(*args, orig, new)


def _windows_call(codec, xd, tab, sel, orig, new, y, taps="table", n_win=None):
    L, M = RS.ratio(orig, new)
    _, K = RS.geometry(L, M)
    tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    sel_h = np.ascontiguousarray(sel, dtype=np.int32)
    sel_d = torch.from_numpy(sel_h).to(DEV)
    t = codec._resample_taps(orig, new).data_ptr() if taps == "table" else taps
    rc = codec.lib.ctts_resample_windows(xd.data_ptr(), xd.numel(), tab_d.data_ptr(), tab.ctypes.data_as(C.c_void_p),
                                         len(tab) if n_win is None else n_win, y.data_ptr(), y.numel(), sel_d.data_ptr(),
                                         sel_h.ctypes.data_as(C.c_void_p), len(sel_h), t, L, M, K, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_packed_windows_of_mixed_rates_equal_themselves_alone(codec):
    """eight windows of four signals, at four rates, in one pack (one call per rate through `sel`): each == `resample_window` on it
    alone, bit for bit; its zero pad is written, nothing else is; a refused call launches nothing"""
    rng = np.random.default_rng(11)
    n = 9000
    sigs = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(4)]
    plan = [(0, 8000, 0, 700), (1, 16000, 2047, 2049), (2, 48000, 4090, 8200), (3, 44100, 1, 4100), (0, 8000, 2999, 3000), (1, 48000, 17000, 18000),
            (2, 16000, 5999, 6000), (3, 8000, 100, 2900)]          # (signal, rate, o_lo, o_hi); 6000 / 3000: the signals' last outputs
    tab = np.zeros(len(plan), _lib.RS_WINDOW)
    xs, in_off, out_off = [], 0, 0
    for i, (s, rate, o_lo, o_hi) in enumerate(plan):
        L, M = RS.ratio(24000, rate)
        _, K = RS.geometry(L, M)
        a, b = RS.window_inputs(L, M, K, o_lo, o_hi, n)
        m = o_hi - o_lo
        tab[i] = (in_off, b - a, a, n, o_lo, o_hi, out_off, 0, -m % 8)
        xs.append(sigs[s][a:b])
        in_off += b - a
        out_off += m + (-m % 8)
    xd = torch.from_numpy(np.concatenate(xs)).to(DEV)
    y = torch.full((out_off + 64,), 7.0, dtype=torch.float32, device=DEV)
    for rate in sorted({p[1] for p in plan}):
        assert _windows_call(codec, xd, tab, [i for i, p in enumerate(plan) if p[1] == rate], 24000, rate, y) == 0, codec.lib.ctts_last_error()
    got = y.cpu().numpy()
    assert np.all(got[out_off:] == 7.0)
    for i, (s, rate, o_lo, o_hi) in enumerate(plan):
        w = tab[i]
        alone = codec.resample_window(xd[int(w["in_off"]): int(w["in_off"] + w["n_in"])], int(w["origin"]), n, o_lo, o_hi, 24000, rate).cpu().numpy()
        lo = int(w["out_off"])
        assert got[lo: lo + o_hi - o_lo].tobytes() == alone.tobytes(), i
        assert np.all(got[lo + o_hi - o_lo: lo + o_hi - o_lo + int(w["pad"])] == 0.0), i
        whole = codec.resample(torch.from_numpy(sigs[s]).to(DEV), 24000, rate).cpu().numpy()
        assert alone.tobytes() == whole[o_lo:o_hi].tobytes(), i
    # refusals reach no launch: the output keeps its fill
    y.fill_(7.0)
    bad = tab.copy()
    bad["n_in"][0] -= 1                              # one sample short of what its outputs read
    assert _windows_call(codec, xd, bad, [0, 4, 7], 24000, 8000, y) != 0
    bad = tab.copy()
    bad["o_hi"][4] = bad["o_lo"][4] - 1
    assert _windows_call(codec, xd, bad, [0, 4, 7], 24000, 8000, y) != 0
    assert _windows_call(codec, xd, tab, [0, 4, 7], 24000, 8000, y, taps=None) != 0
    assert _windows_call(codec, xd, tab, [0, 4, 9], 24000, 8000, y) != 0
    big = np.concatenate([tab] * 129)[:1025]
    assert _windows_call(codec, xd, big, [0], 24000, 8000, y) != 0
    assert bool((y == 7.0).all())


# ---- 2. decode_windows(sample_rates=) ------------------------------------------------------------------------------------------------
# (slot, prefix tokens, s_lo, s_hi, tail), rate: a first chunk at sample 0, interior chunks, a chunk clipped by its prefix's end, tails
RWINDOWS = [((0, 24, 0, 12000, False), 8000), ((1, 80, 24000, 36000, False), 16000), ((2, 64, 12000, 15000, False), 24000),
            ((3, 30, 12000, 24000, False), 48000), ((4, 72, 20000, None, True), 8000), ((5, 48, 3000, 6000, False), 44100),
            ((6, 80, 36000, None, True), 24000), ((7, 40, 9000, 9001, False), 16000)]


def _store(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((8, 80, 768), device=DEV, generator=g)


@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_decode_windows_at_rates_equals_resample_window_of_decode_window(weights, gemm):
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm=gemm)
    store = _store()
    wins, rates = [w for w, _ in RWINDOWS], [r for _, r in RWINDOWS]
    alone = []
    for (s, Tn, lo, hi, _), r in RWINDOWS:
        total = 256 * (2 * Tn - 1)
        hi = total if hi is None else min(hi, total)          # a chunk is clipped by its prefix's end
        if r == 24000:
            alone.append(codec.decode_window([store[s, :Tn]], lo, hi)[0].cpu().numpy())
            continue
        L, M = RS.ratio(24000, r)
        _, K = RS.geometry(L, M)
        o_lo, o_hi = RS.out_len(lo, L, M), RS.out_len(hi, L, M)
        a, b = RS.window_inputs(L, M, K, o_lo, o_hi, total)
        ext = codec.decode_window([store[s, :Tn]], a, b)                  # the extended range, decoded alone
        alone.append(codec.resample_window(ext, a, total, o_lo, o_hi, 24000, r)[0].cpu().numpy())
        assert alone[-1].shape == (o_hi - o_lo,)
        assert np.array_equal(alone[-1], codec.decode_window([store[s, :Tn]], lo, hi, sample_rate=r)[0].cpu().numpy())
    for k in range(1, len(wins) + 1):
        got = codec.decode_windows(store, [w[:4] for w in wins[:k]], pcm16=False, sample_rates=rates[:k])
        for i, (g, w) in enumerate(zip(got, alone)):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (gemm, k, i)
    # PCM16 and stripped tails: the host conversion of those floats, byte for byte
    thr = float(np.median(np.abs(alone[4])))
    for keep_thr in (1e-5, thr):
        pcm = codec.decode_windows(store, wins, pcm16=True, keep_thr=keep_thr, sample_rates=rates)
        for i, ((w, r), f, p) in enumerate(zip(RWINDOWS, alone, pcm)):
            want = float_to_int16(f[np.abs(f) > np.float32(keep_thr)]) if w[4] else float_to_int16(f)
            assert p.dtype == np.int16 and p.tobytes() == want.tobytes(), (gemm, keep_thr, i, p.shape, want.shape)
    kept = np.abs(alone[4]) > np.float32(thr)
    assert 0 < kept.sum() < kept.size
    flt = codec.decode_windows(store, wins, pcm16=False, keep_thr=thr, sample_rates=rates)
    assert np.array_equal(flt[4], alone[4][kept]) and np.array_equal(flt[0], alone[0])
    # all-24000 rates: today's call, today's bytes
    for pcm16 in (True, False):
        old = codec.decode_windows(store, wins, pcm16=pcm16, keep_thr=1e-5)
        new = codec.decode_windows(store, wins, pcm16=pcm16, keep_thr=1e-5, sample_rates=[24000] * len(wins))
        assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(old, new))
    # a 24 kHz window among resampled ones gets the bytes it gets alone; empty ranges come back empty
    old = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5)
    new = codec.decode_windows(store, wins, pcm16=True, keep_thr=1e-5, sample_rates=rates)
    assert new[2].tobytes() == old[2].tobytes() and new[6].tobytes() == old[6].tobytes()
    got = codec.decode_windows(store, [(0, 24, 12032, 24000), (1, 80, 0, 12000), (2, 0, 0, 100), (3, 30, 1, 2)], pcm16=False,
                               sample_rates=[8000, 16000, 8000, 8000])
    assert got[0].size == 0 and got[2].size == 0 and got[3].size == 0 and got[1].shape == (8000,)
    with pytest.raises(ValueError):
        codec.decode_windows(store, wins[:2], sample_rates=[8000])
    with pytest.raises(ValueError):
        codec.decode_windows(store, wins[:2], sample_rates=[8000, 24001])


# ---- 3. the serial stream ---------------------------------------------------------------------------------------------------------------
def _chat(weights, dtype):
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    chat = Chat()
    assert chat.load(state_dicts=weights, device=DEV, dtype=dtype, tokenizer=os.path.join(GOLD, "tokenizer"), spk_stat=spk_stat)
    return chat


def _params(chat, spk, **kw):
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=80,
                                min_new_token=80, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=spk, stream_batch=24,
                                stream_speed=3000, pass_first_n_batches=1, **kw)


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_serial_stream_at_8k_tiles_and_matches_the_whole_prefix_composition(weights, dtype):
    """Chat.infer(stream=True, sample_rate=8000, stream_resample=True): the chunk lengths are the 24 kHz schedule's ranges mapped through
    ceil(s L / M); every chunk is within the windowed-versus-full tolerance of the 24 kHz decode (test_gpu_e2e.py,
    test_decode_window_equals_slices_of_the_full_decode: 2e-6 RMS, 1e-4 max) times max_i sum_k |h[i][k]| of the slice of the whole
    prefix decoded and resampled whole (`incremental_stream=False`) -- an error e on every input moves an output by at most
    sum_k |h| e --; at 24000 with the flag on the bytes are those of the call without it"""
    chat = _chat(weights, dtype)
    torch.manual_seed(11)
    spk = chat.sample_random_speaker()
    text = ["One more short line."]

    def run(**kw):
        return [np.asarray(c) for c in chat.infer(text, stream=True, skip_refine_text=True, split_text=False, params_infer_code=_params(chat, spk), **kw)]
    base = run()
    flag = run(sample_rate=24000, stream_resample=True)
    assert len(base) == len(flag) >= 3 and all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(base, flag))
    with pytest.raises(ValueError, match="non-streamed inference only"):
        chat.infer(text, stream=True, skip_refine_text=True, split_text=False, sample_rate=8000)
    with pytest.raises(ValueError):
        chat.infer(text, stream=True, skip_refine_text=True, split_text=True, sample_rate=8000, stream_resample=True)
    got = run(sample_rate=8000, stream_resample=True)
    chat.incremental_stream = False
    ref = run(sample_rate=8000, stream_resample=True)
    chat.incremental_stream = True
    L, M = RS.ratio(24000, 8000)
    bounds = np.concatenate([[0], np.cumsum([c.shape[1] for c in base[:-1]])])       # the 24 kHz schedule: s_lo of every chunk
    want = [RS.out_len(int(bounds[i + 1]), L, M) - RS.out_len(int(bounds[i]), L, M) for i in range(len(base) - 1)]
    assert [c.shape[1] for c in got[:-1]] == want == [c.shape[1] for c in ref[:-1]] and len(got) == len(base) == len(ref)
    # min_new_token = max_new_token: exactly 80 tokens, yields at 24 (dropped), 48, 72 and the final result, then the tail -- what is
    # left of the tiling, less the columns the silence strip removes
    assert len(got) == 4 and bounds.tolist() == [0, 3000, 6000, 9000]
    assert 0 < got[-1].shape[1] <= RS.out_len(256 * (2 * 80 - 1), L, M) - RS.out_len(9000, L, M)
    s = float(np.abs(oracle_taps(24000, 8000)[0]).sum(axis=1).max())
    for k, (g, r) in enumerate(zip(got, ref)):
        if g.shape != r.shape:                       # the 1e-5 strip can flip on a borderline column of the tail
            assert k == len(got) - 1 and abs(g.shape[1] - r.shape[1]) <= 8
            continue
        d = g.astype(np.float64) - r
        rms, mx = float(np.sqrt(np.mean(d ** 2))) if d.size else 0.0, float(np.abs(d).max()) if d.size else 0.0
        print(f"serial stream[{dtype}] chunk {k}: {g.shape[1]} samples, rms {rms:.2e}, max {mx:.2e} (bars {2e-6 * s:.2e}, {1e-4 * s:.2e})")
        assert rms < 2e-6 * s and mx < 1e-4 * s, (k, rms, mx)


# ---- 4. the pooled stream ---------------------------------------------------------------------------------------------------------------
def _serial_chunks_rate(chat, hid, counts, spec, rate):
    """the `stream` branch of `Chat._infer` (pcm16, one text, `sample_rate=rate`) replayed over `hid`"""
    kw = {} if rate == 24000 else {"rate": rate}
    chunks, length, passed = [], 0, 0
    for n in counts:
        passed += 1
        if passed <= spec.pass_first_n_batches:
            continue
        chunks.append(chat._stream_piece([hid[:n]], length, length + spec.stream_speed, True, True, **kw)[0])
        length = min(length + spec.stream_speed, max(0, 256 * (2 * n - 1)))
    w = chat._stream_piece([hid], length, None, True, **kw)[0]
    w = w[np.abs(w) > 1e-5]
    chunks.append(float_to_int16(w) if w.size else w.astype(np.int16))
    return chunks


def test_pooled_streams_at_four_rates_equal_the_serial_composition(weights):
    """four streams at 8, 16, 24 and 48 kHz through a 4-slot pool, the chunks of a poll from ONE decode_windows call: every chunk ==
    the serial composition replayed over the hidden states the pool returned, byte for byte; ids == the request generated alone"""
    eng = _engine(weights, "f32")
    codec = E.CodecEngine(weights["decoder"], weights["vocos"], DEV, gemm="bf16x3")
    chat = Chat()
    chat.codec = codec
    pool = SlotPool(eng, slots=4, cap=256, hid_cap=128, per_request=True)
    rs = np.random.RandomState(33)
    plan = [(72, -1, 3000, 0, 8000), (96, 48, 12000, 1, 16000), (60, -1, 12000, 0, 24000), (50, -1, 5000, 1, 48000)]
    reqs = {}
    for i, (max_new, stop, speed, passed, rate) in enumerate(plan):
        ids = torch.from_numpy(np.repeat(rs.randint(1, 21178, size=(int(rs.randint(4, 30)), 1)), 4, axis=1).astype(np.int64))
        p = dict(temperature=0.3, top_P=0.7, top_K=20, repetition_penalty=1.05, min_new_token=0, manual_seed=int(700 + 13 * i))
        reqs[i] = (ids, p, max_new, stop, StreamSpec(24, speed, passed), rate)
        pool.submit(i, ids, max_new_token=max_new, stop_at=stop, params=p, stream=reqs[i][4])
    chunks, results, groups = {}, {}, []
    for got in pool.run(events=True):
        if isinstance(got, StreamEvents):
            groups.append(len(got.chunks))
            pcm = codec.decode_windows(pool.hiddens, [c[1:] for c in got.chunks], pcm16=True, keep_thr=1e-5,
                                       sample_rates=[reqs[c[0]][5] for c in got.chunks])
            for c, a in zip(got.chunks, pcm):
                chunks.setdefault(c[0], []).append(a)
        else:
            results[got[0]] = (got[1].cpu().numpy(), got[2])
    assert sorted(results) == [0, 1, 2, 3] and sorted(chunks) == [0, 1, 2, 3] and max(groups) >= 2
    for i, (ids, p, max_new, stop, spec, rate) in reqs.items():
        ref, counts = _alone_stream(eng, ids, p, max_new, stop, 24)
        assert np.array_equal(results[i][0], ref.ids[0].cpu().numpy()), i
        want = _serial_chunks_rate(chat, results[i][1], counts, spec, rate)
        got = chunks[i]
        assert [g.shape for g in got] == [w.shape for w in want], (i, rate, [g.shape for g in got], [w.shape for w in want])
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.int16 and g.tobytes() == w.tobytes(), (i, rate, k)
        L, M = RS.ratio(24000, rate) if rate != 24000 else (1, 1)
        n = results[i][1].shape[0]
        assert 0 < sum(g.size for g in got) <= RS.out_len(256 * (2 * n - 1), L, M)      # the chunks tile the resampled stream; the tail is stripped
    pool.close()


# ---- 5. the endpoint --------------------------------------------------------------------------------------------------------------------
def test_endpoint_streams_at_8k_with_the_rate_in_the_header(weights):
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
                                                                params_infer_code=p, pcm16=True, sample_rate=8000, stream_resample=True)]
        body = {"input": "A streamed sentence.", "response_format": "wav", "stream": True, "sample_rate": 8000}
        with TestClient(server.create_app(chat, voices, sample_rates=(8000, 24000))) as c:
            assert c.post("/v1/audio/speech", json=body).status_code == 400
        with TestClient(server.create_app(chat, voices, stream_sample_rates=(8000,))) as c:
            r = c.post("/v1/audio/speech", json=body)
        assert r.status_code == 200 and r.content[:44] == server.wav_stream_header(8000)
        assert struct.unpack("<I", r.content[24:28])[0] == 8000
        assert len(r.content) - 44 == 2 * sum(w.size for w in want) > 0
        assert r.content[44:] == b"".join(w.astype("<i2").tobytes() for w in want)
    finally:
        chat.InferCodeParams = orig

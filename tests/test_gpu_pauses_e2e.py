"""`pauses` end to end on the GPU: `Chat.infer(pauses=)` against the public CodecEngine calls composed in the chain's order (time scaler,
resampler, trim_pauses, loudness, conversion), with every output format, a split request trimmed sentence by sentence under one gain,
pooled requests with their own specs, and the endpoint.  Synthetic weights need not produce pauses, so the threshold is taken from the
measured decode: the median frame peak.  At most 32 tokens.  `pytest -m gpu`."""
import io
import os
import threading
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from chattts_amd import flac as FLAC  # noqa: E402
from chattts_amd import g711 as G711  # noqa: E402
from chattts_amd import weights as W  # noqa: E402
from chattts_amd.audio import float_to_int16  # noqa: E402
from chattts_amd.serving import SpeechBatcher  # noqa: E402
from tests import pauses_oracle as PO  # noqa: E402

DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = np.float32(1e-5)
TEXTS = ["Good morning!", "Numbers like 42 and 7.", "Hello there."]
SPLIT = "Hello there. How are you. Fine."
KW = dict(skip_refine_text=True, split_text=False)


@pytest.fixture(scope="module")
def chat(weights):
    from chattts_amd.core import Chat
    with open(os.path.join(GOLD, "spk_stat.txt"), encoding="utf-8") as f:
        spk_stat = f.read()
    c = Chat()
    assert c.load(state_dicts={**weights, "dvae": W.synthetic_dvae()}, device=DEV, dtype="f32", tokenizer=os.path.join(GOLD, "tokenizer"),
                  spk_stat=spk_stat)
    torch.manual_seed(11)
    c.test_voice = c.sample_random_speaker()
    return c


def _params(chat, i=0, max_new=None, **kw):
    return chat.InferCodeParams(top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=max_new or [24, 32, 16][i % 3], show_tqdm=False,
                                manual_seed=300 + 7 * i, spk_emb=chat.test_voice, **kw)


def _strip(w):
    return w[np.abs(w) > THR]


def _hiddens_of(chat, run):
    """the hidden states the serial call generates, batch by batch (recorded at `_infer_code`), and the call's result"""
    orig, calls = chat._infer_code, []

    def rec(text, stream, device, return_hidden, params):
        for out in orig(text, stream, device, return_hidden, params):
            calls.append([h.clone() for h in out.hiddens])
            yield out
    chat._infer_code = rec
    try:
        res = run()
    finally:
        del chat._infer_code
    return calls, res


def _median_db(x, F):
    """the median frame peak of the rows x [B, n] in dB, clipped to the spec's range"""
    n = x.shape[1] // F * F
    peaks = np.abs(x[:, :n]).reshape(x.shape[0], -1, F).max(2)
    with np.errstate(divide="ignore"):
        return float(np.clip(20.0 * np.log10(np.median(peaks)), -100.0, 0.0))


def _specs(db):
    return (dict(max_pause_ms=20, lead_ms=0, tail_ms=10, pad_ms=0, threshold_db=db), dict(max_pause_ms=50, lead_ms=10, tail_ms=0, pad_ms=10, threshold_db=db))


@pytest.fixture(scope="module")
def base(chat):
    """the plain call's hidden states and 24 kHz batch decode, once, and the specs whose threshold is the decode's median frame peak"""
    calls, _ = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), **KW))
    assert len(calls) == 1
    wav = chat.codec.decode_to_wavs(calls[0])
    x = chat.codec.to_host(wav)
    db = _median_db(x, 240)
    print(f"median frame peak of the decode: {db:.2f} dBFS")
    a, b = _specs(db)
    return {"hid": calls[0], "wav": wav, "x": x, "A": a, "B": b}


def _chain(chat, wav, spec, speed=None, rate=None, target=None):
    """the public CodecEngine calls in the chain's order on a [B, n] decode -> the rows on the host, and the trim's records"""
    codec = chat.codec
    if speed is not None:
        wav = codec.time_scale(wav, speed)
    if rate is not None:
        wav = codec.resample(wav, 24000, rate)
    fs = 24000 if rate is None else rate
    y, off, rec = codec.trim_pauses(wav, spec, rates=fs, return_stats=True)
    if target is not None:
        y = codec.loudness_normalize(y, target, offsets=off, rates=fs)
    y = codec.to_host(y)
    return [y[off[i]: off[i + 1]] for i in range(len(off) - 1)], rec, codec.to_host(wav)


def test_no_spec_is_todays_call_bit_for_bit(chat):
    for kw in (dict(), dict(pcm16=True), dict(pcm16=True, ragged_decode=True), dict(ragged_decode=True)):
        kw = dict(**KW, **kw)
        a = chat.infer(TEXTS[:2], params_infer_code=_params(chat), **kw)
        b = chat.infer(TEXTS[:2], params_infer_code=_params(chat), pauses=None, **kw)
        c = chat.infer(TEXTS[:2], params_infer_code=_params(chat), pauses=[None, None], **kw)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b] == [x.tobytes() for x in c] and a[0].dtype == b[0].dtype
    with pytest.raises(ValueError, match="non-streamed"):
        chat.infer(TEXTS[:1], stream=True, params_infer_code=_params(chat), pauses=True)


@pytest.mark.parametrize("speed,rate,target", [(None, None, None), (1.25, 8000, -16.0)])
def test_float_and_pcm16_output_are_the_chain_composed_from_the_public_calls(chat, base, speed, rate, target):
    opt = {**({} if speed is None else {"speed": speed}), **({} if rate is None else {"sample_rate": rate}),
           **({} if target is None else {"loudness": target})}
    fs = 24000 if rate is None else rate
    front = _chain(chat, base["wav"], None, speed, rate)[2]                       # what the trim is given: scaled, resampled
    db = _median_db(front, fs // 100)                                             # the threshold: the median frame peak of THAT signal
    A, B = _specs(db)
    want, rec, before = _chain(chat, base["wav"], A, speed, rate, target)
    print(f"speed {speed} rate {rate} target {target}: threshold {db:.2f} dB, records {rec.tolist()}")
    assert before.tobytes() == front.tobytes()
    for b in range(3):                                                            # the trim itself against the oracle, row by row
        yo, ro = PO.trim(before[b], fs, A)
        assert rec[b].tolist() == list(ro)
        if target is None:
            assert want[b].tobytes() == yo.tobytes()
    assert any(len(w) < before.shape[1] for w in want), "no row lost a sample: the threshold does not bite"
    assert all(r[1] > 0 for r in rec.tolist()), "a row without an active frame: the threshold cuts everything"
    base = {**base, "A": A, "B": B}
    calls, got = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat), pauses=base["A"], **opt, **KW))
    assert all(torch.equal(p, q) for p, q in zip(calls[0], base["hid"])), "the spec changed what was generated"
    assert len(got) == 3 and all(g.dtype == np.float32 and g.tobytes() == _strip(w).tobytes() for g, w in zip(got, want))
    assert [w.tobytes() for w in chat.decode_to_wavs(base["hid"], pauses=base["A"], **opt)] == [w.tobytes() for w in want]
    pcm = chat.infer(TEXTS, params_infer_code=_params(chat), pauses=base["A"], pcm16=True, **opt, **KW)
    for b in range(3):
        assert pcm[b].dtype == np.int16 and pcm[b].tobytes() == float_to_int16(_strip(want[b])).tobytes()
    # one spec per text, None entries copied through
    per = chat.infer(TEXTS, params_infer_code=_params(chat), pauses=[base["A"], None, base["B"]], pcm16=True, **opt, **KW)
    want_b, _, _ = _chain(chat, base["wav"], [None, None, base["B"]], speed, rate, target)
    assert per[0].tobytes() == pcm[0].tobytes() and per[1].tobytes() == float_to_int16(_strip(want_b[1])).tobytes()
    assert per[2].tobytes() == float_to_int16(_strip(want_b[2])).tobytes()


def test_every_output_format_is_the_host_composition_behind_the_trimmed_waveform(chat, base):
    want, _, _ = _chain(chat, base["wav"], base["A"])
    kw = dict(pcm16=True, pauses=base["A"], **KW)
    got = chat.infer(TEXTS, params_infer_code=_params(chat), encoding="ulaw", **kw)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.tobytes() == G711.encode(float_to_int16(_strip(w)), "ulaw").tobytes()
    got = chat.infer(TEXTS, params_infer_code=_params(chat), flac=True, **kw)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.tobytes() == FLAC.encode(float_to_int16(_strip(w)), 24000)
    # ragged rows: each decoded, scaled, resampled, trimmed and normalised alone, whatever it is packed with
    rows = [torch.randn(t, 768, device=DEV) * 0.1 for t in (9, 14, 5)]
    sp, tg, rates, encs = [base["A"], None, base["B"]], [-20.0, None, -30.0], [8000, 24000, 11025], ["ulaw", None, None]
    mixed = chat.decode_to_pcm16(rows, ragged=True, pauses=sp, sample_rate=rates, encoding=encs, speed=[1.0, 1.25, 0.8])
    for g, r, p, sr, e, s in zip(mixed, rows, sp, rates, encs, (1.0, 1.25, 0.8)):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, speed=s, **({} if p is None else {"pauses": p}),
                                     **({} if e is None else {"encoding": e}))[0]
        assert g.dtype == alone.dtype and g.tobytes() == alone.tobytes()
    today = chat.decode_to_pcm16(rows, ragged=True, sample_rate=rates, speed=[1.0, 1.25, 0.8])
    assert mixed[1].tobytes() == today[1].tobytes() and mixed[2].tobytes() != today[2].tobytes()
    both = chat.decode_to_pcm16(rows, ragged=True, pauses=sp, loudness=tg, sample_rate=[8000, 24000, 16000])
    for g, r, p, t, sr in zip(both, rows, sp, tg, [8000, 24000, 16000]):
        alone = chat.decode_to_pcm16([r], ragged=True, sample_rate=sr, **({} if p is None else {"pauses": p}), **({} if t is None else {"loudness": t}))[0]
        assert g.tobytes() == alone.tobytes()
    flacs = chat.decode_to_pcm16(rows, ragged=True, pauses=base["A"], flac=[True, False, True])
    plain = chat.decode_to_pcm16(rows, ragged=True, pauses=base["A"])
    assert flacs[1].tobytes() == plain[1].tobytes() and flacs[0].tobytes() == FLAC.encode(plain[0], 24000) and flacs[2].tobytes() == FLAC.encode(plain[2], 24000)


def test_a_split_request_is_trimmed_sentence_by_sentence_under_one_gain(chat, base):
    codec = chat.codec
    target = -20.0
    for ragged in (True, False):
        calls, got = _hiddens_of(chat, lambda: chat.infer(SPLIT, params_infer_code=_params(chat), pauses=base["A"], loudness=target,
                                                          ragged_decode=ragged, skip_refine_text=True, split_text=True, pcm16=True))
        if ragged:                        # calls[0]: the refer sentence
            ws = [codec.decode_to_wavs([h])[0] for c in calls[1:] for h in c]
        else:                             # the reference's padded batches: every row of a batch
            ws = [w for c in calls[1:] for w in codec.decode_to_wavs(c)]
        assert len(ws) == 3
        off = np.concatenate([[0], np.cumsum([w.numel() for w in ws])]).astype(np.int64)
        t, off_t, rec = codec.trim_pauses(torch.cat(ws), base["A"], offsets=off, return_stats=True)
        for i, w in enumerate(ws):        # every sentence alone: its record is the oracle's of that sentence
            assert rec[i].tolist() == list(PO.trim(codec.to_host(w), 24000, base["A"])[1]), i
        assert any(rec[i][7] < ws[i].numel() for i in range(3)), "no sentence lost a sample"
        y, st = codec.loudness_normalize(t, target, offsets=off_t, groups=[0, 3], return_stats=True)
        assert len(st) == 1                                                       # ONE gain over the trimmed sentences
        y = codec.to_host(y)
        want = float_to_int16(np.concatenate([_strip(y[off_t[i]: off_t[i + 1]]) for i in range(3)]))
        assert len(got) == 1 and got[0].tobytes() == want.tobytes(), ragged
    floats = chat.infer(SPLIT, params_infer_code=_params(chat), pauses=base["A"], loudness=target, skip_refine_text=True, split_text=True)
    assert len(floats) == 1 and float_to_int16(floats[0]).tobytes() == got[0].tobytes()


class _Recording(SpeechBatcher):
    def _handle(self, got):
        for it in ([got] if isinstance(got, tuple) else got if isinstance(got, list) else []):
            self.hids[it[0]] = it[2].clone()
        super()._handle(got)


def test_pooled_requests_with_their_specs_share_a_decode_and_equal_their_own_calls(chat, base):
    specs = [base["A"], base["B"], None]
    b = _Recording(chat, 4, threading.Lock(), ragged_decode=True)
    b.hids = {}
    seen, orig = [], chat.codec.trim_pauses
    chat.codec.trim_pauses = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        with b.lock:
            futs = [b.submit(TEXTS[0], _params(chat, 0, 24), pauses=p) for p in specs]      # the same text: they finish at one poll
        got = [f.result(timeout=300) for f in futs]
        decodes, trims, occ = b.decode_calls, len(seen), b.occupancy()
    finally:
        del chat.codec.trim_pauses
        b.close()
    assert decodes == 1 and trims == 1 and occ["trimmed"] == 2, "the three requests did not share one decode and one trim_pauses call"
    for i, (g, p) in enumerate(zip(got, specs)):
        alone = chat.decode_to_pcm16([b.hids[futs[i].rid]], ragged=True, **({} if p is None else {"pauses": p}))[0]
        assert g.dtype == np.int16 and g.tobytes() == alone.tobytes(), i
    assert got[0].tobytes() != got[2].tobytes()


def _server_params(chat):
    """the endpoint's fixed sampling parameters for the default voice (server.create_app: code_params), capped like the test's app"""
    return chat.InferCodeParams(prompt="[speed_5]", top_P=0.5, top_K=10, temperature=0.1, repetition_penalty=1.1, max_new_token=2048,
                                min_new_token=0, show_tqdm=False, ensure_non_empty=True, manual_seed=42, spk_emb=chat.test_voice,
                                stream_batch=24, stream_speed=12000, pass_first_n_batches=2)


def _frames(body):
    with wave.open(io.BytesIO(body), "rb") as wf:
        assert wf.getframerate() == 24000
        return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")


def test_endpoint_serves_the_spec_when_asked_to_and_ignores_it_by_default(chat, base):
    from starlette.testclient import TestClient
    from chattts_amd import server
    orig_params = chat.InferCodeParams
    chat.InferCodeParams = lambda **kw: orig_params(**{**kw, "max_new_token": 24})     # (random weights do not emit EOS on cue)
    try:
        body = {"input": TEXTS[0], "response_format": "wav"}
        p = _server_params(chat)
        today = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p)[0]
        dflt = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, pauses=True)[0]
        cut = chat.infer([TEXTS[0]], skip_refine_text=True, pcm16=True, params_infer_code=p, pauses=base["A"])[0]
        assert cut.dtype == np.int16 and cut.tobytes() != today.tobytes() and len(cut) < len(today)
        with TestClient(server.create_app(chat, {"default": chat.test_voice}, pauses=True)) as c:
            r = c.post("/v1/audio/speech", json={**body, "pauses": True})
            assert r.status_code == 200 and _frames(r.content).tobytes() == dflt.tobytes()
            r = c.post("/v1/audio/speech", json={**body, "pauses": base["A"]})
            assert r.status_code == 200 and _frames(r.content).tobytes() == cut.tobytes()
            assert _frames(c.post("/v1/audio/speech", json=body).content).tobytes() == today.tobytes()
            assert c.post("/v1/audio/speech", json={**body, "pauses": True, "stream": True}).status_code == 400
            assert c.post("/v1/audio/speech", json={**body, "pauses": {"max_pause_ms": 1}}).status_code == 400
            assert c.get("/health").json()["pauses"] is True
        with TestClient(server.create_app(chat, {"default": chat.test_voice})) as c:
            r = c.post("/v1/audio/speech", json={**body, "pauses": True})
            assert r.status_code == 200 and _frames(r.content).tobytes() == today.tobytes()
    finally:
        chat.InferCodeParams = orig_params

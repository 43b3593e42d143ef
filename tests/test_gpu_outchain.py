"""The output chain end to end on the GPU ("The output chain"): the decode calls with EVERY option on at once, each with its
own value in every row, against the public stage calls composed by hand from one option-free decode -- time_scale_segments,
resample_segments, trim_pauses, loudness_normalize(limiter=).  The same kernels run on the same inputs in the same order, so every
comparison is for equality, bit for bit.

The rows are the hidden states of test_gpu_pauses_e2e.py's texts, from its `chat` fixture and its sampling parameters.  Its own
`base` rows have at most 32 tokens, and the row at speed 2.0 needs 38 to hold one whole 400 ms gating block at 8 kHz behind the time
scaler (0.4 s * 2.0 * 24000 = 19200 samples = 256 (2 * 38 - 1)), so the texts are generated once more with room for 40 tokens and
every row is cut to the shortest length that leaves it one whole block at its own speed: 38, 20 and 16 tokens.  `pytest -m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from chattts_amd.audio import float_to_int16  # noqa: E402
from tests.test_gpu_pauses_e2e import KW, TEXTS, _hiddens_of, _median_db, _params, _specs, _strip, chat  # noqa: E402,F401

SPEEDS = [2.0, 1.0, 0.8]                      # 1.0: the row is copied through
RATES = [8000, 24000, 16000]                  # 24000: the row is copied through
TARGETS = [-20.0, -16.0, None]                # None: measured and left alone -- here: the limiter at unity gain
LIMITER = [True, False, True]
TOKENS = [38, 20, 16]                         # ceil((0.4 s * speed * 24000 / 256 + 1) / 2): one whole gating block behind the time scaler


@pytest.fixture(scope="module")
def rows(chat):  # noqa: F811
    """the three rows, their one option-free ragged decode and the pause specs (threshold: the decode's median frame peak; None for
    the second row)"""
    calls, _ = _hiddens_of(chat, lambda: chat.infer(TEXTS, params_infer_code=_params(chat, max_new=40), **KW))
    assert len(calls) == 1 and [int(h.shape[0]) >= t for h, t in zip(calls[0], TOKENS)] == [True] * 3
    hid = [h[:t].clone() for h, t in zip(calls[0], TOKENS)]
    wav, off = chat.codec.decode_ragged(hid)
    assert np.diff(off).tolist() == [256 * (2 * t - 1) for t in TOKENS]
    for n, s in zip(np.diff(off), SPEEDS):    # one whole 400 ms block behind the time scaler, and not with one token fewer
        assert -(-int(n) * 100 // round(100 * s)) >= 9600 > -(-(int(n) - 512) * 100 // round(100 * s))
    A, B = _specs(_median_db(chat.codec.to_host(wav)[None, : int(off[1])], 240))
    return {"hid": hid, "wav": wav, "off": off, "specs": [A, None, B]}


def _compose(codec, wav, off, speeds, rates, specs, targets, lims, groups=None):
    """the public stage calls in the chain's order on a pack -> the rows on the host"""
    w, o = codec.time_scale_segments(wav, off, speeds)
    w, o = codec.resample_segments(w, o, rates)
    w, o = codec.trim_pauses(w, specs, offsets=o, rates=rates)
    w = codec.loudness_normalize(w, targets, offsets=o, rates=rates, limiter=lims, **({} if groups is None else {"groups": groups}))
    w = codec.to_host(w)
    return [w[o[i]: o[i + 1]] for i in range(len(o) - 1)]


def test_the_ragged_calls_are_the_hand_composition_bit_for_bit(chat, rows):  # noqa: F811
    want = _compose(chat.codec, rows["wav"], rows["off"], SPEEDS, RATES, rows["specs"], TARGETS, LIMITER)
    plain = chat.codec.to_host(rows["wav"])
    assert want[1].tobytes() != plain[rows["off"][1]: rows["off"][2]].tobytes()      # the row that only gets a gain: it got one
    kw = dict(speed=SPEEDS, sample_rate=RATES, pauses=rows["specs"], loudness=TARGETS, limiter=LIMITER)
    got = chat.decode_to_wavs(rows["hid"], ragged=True, **kw)
    assert len(got) == 3 and [g.dtype for g in got] == [np.float32] * 3
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    pcm = chat.decode_to_pcm16(rows["hid"], ragged=True, **kw)
    assert [p.dtype for p in pcm] == [np.int16] * 3
    assert [p.tobytes() for p in pcm] == [float_to_int16(_strip(w)).tobytes() for w in want]


def test_the_split_call_is_the_grouped_composition_with_per_request_options(chat, rows):  # noqa: F811
    """one request of two sentences and one request of one: every sentence through the first three stages alone, ONE gain a request"""
    A = rows["specs"][0]
    speeds, rates, specs, targets, lims = [2.0, 1.0], [8000, 24000], [A, None], [None, -18.0], [True, False]
    per = lambda v: [v[0], v[0], v[1]]        # request -> sentences
    want = _compose(chat.codec, rows["wav"], rows["off"], per(speeds), per(rates), per(specs), targets, lims, groups=[0, 2, 3])
    want = [float_to_int16(np.concatenate([_strip(w) for w in want[:2]])), float_to_int16(_strip(want[2]))]
    got = chat.decode_split_to_pcm16([rows["hid"][:2], rows["hid"][2:]], speed=speeds, sample_rate=rates, pauses=specs, loudness=targets, limiter=lims)
    assert [g.dtype for g in got] == [np.int16] * 2 and [g.tobytes() for g in got] == [w.tobytes() for w in want]


def test_the_zero_padded_call_is_the_hand_composition_with_one_option_set_for_all(chat, rows):  # noqa: F811
    codec, A = chat.codec, rows["specs"][0]
    w = codec.resample(codec.time_scale(codec.decode_to_wavs(rows["hid"]), 1.25), 24000, 8000)
    w, o = codec.trim_pauses(w, A, rates=8000)
    w = codec.to_host(codec.loudness_normalize(w, -18.0, offsets=o, rates=8000, limiter=True))
    got = chat.decode_to_wavs(rows["hid"], speed=1.25, sample_rate=8000, pauses=A, loudness=-18.0, limiter=True)
    assert len(got) == 3 and [g.tobytes() for g in got] == [w[o[i]: o[i + 1]].tobytes() for i in range(3)]

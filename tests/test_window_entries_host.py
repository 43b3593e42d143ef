"""The three window-decode entries (ctts_codec_decode_windows, _rate, _speed) share one window-table check, one store-geometry check
and one out_type / product check: each fault below is refused by every entry, under the entry's own name and with the same phrase.
No GPU: the host mirrors are checked before anything is launched, the pointers are never dereferenced."""
import ctypes as C

import numpy as np
import pytest

from chattts_amd import _lib, timescale as TS

S, CAP, TN, CHUNK = 8, 64, 40, 12000          # one window of 40 tokens: 256 * (2 * 40 - 1) = 20224 samples, of which 12000 are cropped
FAKE = C.c_void_p(4096)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _plain(lib, win, strides, out_type, product, ws):
    tab = np.ascontiguousarray(np.array([[*win, 0, 0, 0]], dtype=np.int32))
    return lib.ctts_codec_decode_windows(FAKE, FAKE, strides[0], strides[1], S, CAP, FAKE, _ptr(tab), 1, out_type, FAKE, FAKE, product, 1e-5,
                                         FAKE, ws, None)


def _rate(lib, win, strides, out_type, product, ws):
    """the window stays at 24 kHz (rate -1): its chunk is its crop, no conversion is named"""
    tab = np.ascontiguousarray(np.array([[*win, 0, 0, 0]], dtype=np.int32))
    rtab = np.zeros(1, _lib.RS_WINDOW)
    rtab[0] = (win[3], win[4] - win[3], 0, 0, 0, 0, 0, -1, 0)
    sel = np.zeros(1, np.int32)
    return lib.ctts_codec_decode_windows_rate(FAKE, FAKE, strides[0], strides[1], S, CAP, FAKE, _ptr(tab), FAKE, _ptr(rtab), FAKE, _ptr(sel), 1,
                                              None, 0, out_type, FAKE, FAKE, product, 1e-5, FAKE, ws, None)


def _speed(lib, win, strides, out_type, product, ws):
    """the window's crop is the first push of a stream at 1.25: one chunk, one descriptor, one round"""
    tab = np.ascontiguousarray(np.array([[*win, 0, 0, 0]], dtype=np.int32))
    ctab = np.zeros((1, 8), np.int32)
    p = TS.stream_plan(1.25, 0, CHUNK, False)
    ts = np.zeros(1, _lib.TS_STREAM)
    row = dict(in_off=0, n_in=CHUNK, pos=0, total=p["total"], out_off=0, path_off=0, k_prev=p["k_prev"], k_now=p["k_now"], slot=0, phase=0,
               num=p["num"], den=p["den"], n_out=p["n_out"], reserved=0)
    ts[0] = tuple(row[k] for k in _lib.TS_STREAM.names)
    rtab = np.zeros(1, _lib.RS_WINDOW)
    rtab[0] = (0, CHUNK, 0, 0, 0, p["n_out"], 0, 0, 0)
    rounds = np.array([0, 1], np.int32)
    return lib.ctts_codec_decode_windows_speed(FAKE, FAKE, strides[0], strides[1], S, CAP, FAKE, _ptr(tab), 1, FAKE, _ptr(ctab), FAKE, _ptr(rtab), 1,
                                               FAKE, _ptr(ts), _ptr(rounds), 1, FAKE, FAKE, 4, FAKE, out_type, FAKE, FAKE, product, 1e-5, FAKE, ws,
                                               None)


ENTRIES = {"ctts_codec_decode_windows": _plain, "ctts_codec_decode_windows_rate": _rate, "ctts_codec_decode_windows_speed": _speed}
OK = (0, 0, TN, 0, CHUNK)                      # slot, t_lo, t_hi, c_lo, c_hi
GEOMETRY = b"the store must be [n_slots][hid_cap][768] floats with 16-byte aligned rows"
FAULTS = [
    (dict(win=(S, 0, TN, 0, CHUNK)), b"names slot"),
    (dict(win=(0, 7, 7, 0, CHUNK)), b"is empty"),
    (dict(win=(0, 0, CAP + 1, 0, CHUNK)), b"beyond the slot's capacity"),
    (dict(win=(0, 0, TN, 0, 256 * (2 * TN - 1) + 1)), b"outside its"),
    (dict(strides=(CAP * 768, 767)), GEOMETRY),
    (dict(strides=(CAP * 768 + 2, 768)), GEOMETRY),
    (dict(out_type=2), b"out_type and product must be 0 or 1"),
    (dict(product=2), b"out_type and product must be 0 or 1"),
]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_window_entry_refuses_the_same_faults_under_its_own_name(name):
    lib = _lib.lib()

    def call(win=OK, strides=(CAP * 768, 768), out_type=1, product=0, ws=1024):
        return ENTRIES[name](lib, win, strides, out_type, product, ws), lib.ctts_last_error()
    rc, msg = call()
    assert rc != 0 and b"workspace" in msg, msg           # the valid tables get as far as the workspace check
    for kw, phrase in FAULTS:
        rc, msg = call(**kw)
        assert rc != 0 and name.encode() + b":" in msg and phrase in msg, (kw, msg)

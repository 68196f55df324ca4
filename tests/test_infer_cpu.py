"""The inference forward's C entry points (fhvae_lstm_seq_infer, fhvae_lstm_infer_cs_elems) and eval_model.py's CLI, without a GPU:
argument errors come back from the host before anything is launched."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library()


def test_infer_symbols_exported_and_bound(lib):
    import hip_binding as hb

    for name in ("fhvae_lstm_seq_infer", "fhvae_lstm_infer_cs_elems"):
        assert name in hb.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype == hb.SIGNATURES[name][0] and list(fn.argtypes) == hb.SIGNATURES[name][1]


def _desc(hb, p):
    d = hb.LstmDesc()
    d.L, d.B, d.T, d.H, d.I, d.dtype = 1, 8, 2, 8, 8, hb.F32
    for k in ("x", "hs", "cs", "pre"):
        setattr(d, k, p.value)
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        getattr(d, k)[0] = p.value
    return d


def test_infer_argument_errors(lib):
    import hip_binding as hb

    assert lib.fhvae_lstm_seq_infer(None, None) == -1
    assert lib.fhvae_lstm_infer_cs_elems(None) == 0
    d = hb.LstmDesc()
    d.L = 9
    assert lib.fhvae_lstm_seq_infer(ctypes.byref(d), None) == -2
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _desc(hb, p)
    d.gates = p.value  # the inference forward saves nothing: a gate buffer is a caller error
    assert lib.fhvae_lstm_seq_infer(ctypes.byref(d), None) == -2
    d = _desc(hb, p)
    d.hs = None
    assert lib.fhvae_lstm_seq_infer(ctypes.byref(d), None) == -1
    # the per-step schedules' two-slot ring of c: 2 L B H floats, required
    d = _desc(hb, p)
    assert lib.fhvae_lstm_infer_cs_elems(ctypes.byref(d)) == 2 * 1 * 8 * 8
    d.cs = None
    assert lib.fhvae_lstm_seq_infer(ctypes.byref(d), None) == -1
    # the schedule queries do not look at gates / cs (the inference forward takes the training forward's schedule)
    assert lib.fhvae_lstm_layout_id(ctypes.byref(d)) == 0 and lib.fhvae_lstm_form(ctypes.byref(d)) == 0
    # shape rules of fhvae_lstm_seq_fwd apply as they stand: H = 6 is not a multiple of 4 in f32 mode
    d = _desc(hb, p)
    d.H = 6
    assert lib.fhvae_lstm_seq_infer(ctypes.byref(d), None) == -4


def test_eval_model_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pytorch-scalablefhvae_amd", "eval_model.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--checkpoint", "--out", "--feat-scp", "--len-scp", "--batch-size", "--convert-to", "--max-recon"):
        assert flag in r.stdout

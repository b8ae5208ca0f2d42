"""CPU: tmat_model_layers (include/tmat.h) -- which kernel every convolution of a weight blob runs on, without a GPU -- and the case table
of tests/test_gpu_conv_narrow.py on the CPU (the oracle inside the float64 reference's bound at 16, 48 and 80 channels too)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

from tmat_amd import _lib, synth  # noqa: E402

DEFAULT, FC32, FC16 = (64, 128, 256, 512), (32, 64, 128, 256), (16, 32, 64, 128)

# the launches launch_conv refuses, per model, as (ksize, stride, cin, cout) in launch order (ksize 2: the sub-pixel form)
NARROW = {
    FC32: [(1, 1, 32, 64), (1, 2, 32, 64), (2, 1, 64, 32), (1, 1, 64, 32), (3, 1, 32, 32)],
    FC16: [(1, 1, 16, 32), (1, 1, 32, 32), (1, 2, 16, 32), (1, 1, 32, 64), (1, 2, 32, 64),
           (2, 1, 64, 32), (1, 1, 64, 32), (3, 1, 32, 32), (2, 1, 32, 16), (1, 1, 32, 16), (3, 1, 16, 16)],
}


def layers(fc):
    return _lib.model_layers(synth.pack_weights(synth.synth_weights(0, filter_counts=fc)))


def main_kernel_takes(k, stride, cin, cout):
    """launch_conv's rule as include/tmat.h states it at tmat_conv2d / tmat_conv2d_roi"""
    return cout % 64 == 0 and (cin % 32 == 0 if k == 2 else cin % 64 == 0)


def test_default_model_never_runs_the_narrow_kernel():
    ls = layers(DEFAULT)
    assert len(ls) == 21 and (ls[:, 5] != 1).all()
    # three down blocks: the 160² and 80² levels fused (two separable launches and the residual 1x1), the 40² level unfused
    assert ls[:9, 5].tolist() == [2, 0, 2, 2, 0, 2, 0, 0, 0]
    assert ls[1].tolist() == [1, 1, 64, 128, 80, 0]          # the residual over the stem at its even pixels: unit stride
    assert ls[-1].tolist() == [3, 1, 64, 64, 160, 0]


@pytest.mark.parametrize("fc", [FC32, FC16], ids=["32", "16"])
def test_narrow_models(fc):
    ls = layers(fc)
    assert len(ls) == 21
    got = [tuple(r[:4]) for r in ls.tolist() if r[5] == 1]
    assert got == NARROW[fc], got
    for k, st, cin, cout, side, launcher in ls.tolist():
        if launcher == 2:
            continue
        assert (launcher == 0) == main_kernel_takes(k, st, cin, cout), (k, st, cin, cout, launcher)
        assert cin % 16 == 0 and cout % 16 == 0
    # (32, ...): level 0 unfused, level 1 fused, level 2 unfused; (16, ...): no fused level
    assert [int(r[5] == 2) for r in ls[:9].tolist()] == ([0, 0, 0, 1, 0, 1, 0, 0, 0] if fc == FC32 else [0] * 9)
    # output sides: the last up block ends at half the patch
    assert ls[-1].tolist()[:5] == [3, 1, fc[0], fc[0], 160]


@pytest.mark.parametrize("fc", [(8, 16, 32, 64), (24, 48, 96, 192), (64, 128, 256, 520)], ids=["8", "24", "520"])
def test_blobs_no_kernel_takes_are_refused(fc):
    blob = synth.pack_weights(synth.synth_weights(0, filter_counts=fc))
    with pytest.raises(_lib.TmatError) as e:
        _lib.model_layers(blob)
    assert "(-3)" in str(e.value)                              # TMAT_E_WEIGHTS
    assert _lib.lib().tmat_last_error().decode().startswith("weights: "), e.value
    assert "16" in str(e.value) or "power of two" in str(e.value)


def test_switches_are_read_as_tmat_create_reads_them(monkeypatch):
    monkeypatch.setenv("TMAT_FUSED_SEP", "0")
    ls = layers(DEFAULT)
    assert (ls[:, 5] == 0).all() and ls[2].tolist() == [1, 2, 64, 128, 80, 0]
    ls = layers(FC32)
    assert [tuple(r[:4]) for r in ls.tolist() if r[5] == 1] == NARROW[FC32]


def test_small_cap_reports_the_count():
    import ctypes as C
    blob = synth.pack_weights(synth.synth_weights(0, filter_counts=FC16))
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    out = np.zeros((4, 6), np.int32)
    n = C.c_int(0)
    rc = _lib.lib().tmat_model_layers(C.cast(buf, C.c_void_p), len(blob), 4, _lib.ptr(out), C.byref(n))
    assert rc == _lib.E_CAP and n.value == 21


def test_narrow_case_table_on_the_cpu():
    """the oracle lies inside the derived bound of the float64 reference on every shape the GPU test runs (tests/test_conv_ref.py does the same
    for the main kernel's table): a last K block of 16 channels, Cout 48 and 80, the sub-pixel form at Cin 16"""
    import conv_cases as cc
    import narrow_cases as nc
    worst = 0.0
    for c in nc.all_cases():
        o = cc.operands(c)
        v, bound = cc.reference(c, o)
        orc = cc.oracle(c, o)
        assert orc.shape == v.shape, c["id"]
        worst = max(worst, float((np.abs(orc.astype(np.float64) - v) / bound).max()))
    assert worst <= 1.0, worst

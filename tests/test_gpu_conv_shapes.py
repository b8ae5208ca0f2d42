"""GPU: conv_mfma_kernel (csrc/unet_kernels.hip) against CPU values at shapes OFF the networks' grid.

The other GPU files compare the kernel with something computed on a CPU only at the layer shapes of the UNet (320 / 160 / 80 / 40 / 20,
square) and of the ResNet at 64 and 256 (powers of two): Wo % 8 == 0 and M a whole number of tiles, every time.  The output shape picks
among the kernel's code paths -- flat / row-uniform / per-lane prologue, row-uniform / per-lane / row-split epilogue, the tail past M,
the fast divisions by Ho Wo and Wo, 64- and 128-wide column tiles -- so here the shapes are chosen by those paths (tests/helpers/conv_cases.py):
one row, widths 2 / 5 / 7, an odd width behind a stride, M = 2 / 127 / 129 / 255 / 257, non-square images, Cout 192 and 384 (three column
tiles), Cin 192, the sub-pixel form at Cin 32.

Every f32 case is asserted twice: bit for bit against the oracle (oracle/unet.py:_conv / _conv_subpixel, the same chain order), and
within the DERIVED bound of the independent float64 reference tests/helpers/conv_ref.py (gamma_(K + 2) mag, gamma_(K + 5) for the
sub-pixel form; tests/test_conv_ref.py holds the oracle to the same bound on the same cases, on the CPU).
  A  tmat_conv2d, prec 0, each shape bare and with scale + residual + both ReLUs;
  B  tmat_conv2d_roi without segments -- the full-frame launch tests/test_gpu_conv_roi.py takes as ITS reference -- in all seven forms;
  C  the region form straight against the oracle: inside the rectangles the oracle's bits, outside the caller's sentinel;
  D  prec 3 (f16 operands) and prec 4 (f16 activations) on the shapes of A, by the gate of tests/test_gpu_invdepth_f16.py;
  E  what launch_conv refuses, as include/tmat.h states it.
Not covered: M near 2^30 (the fast division at large m) -- such a case needs gigabytes of operands.
The process never imports torch."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import conv_cases as cc  # noqa: E402
import conv_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.678)
SENT_BITS = SENTINEL.view(np.uint32)


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


_refs = {}


def ref_of(c):
    """(operands, oracle, float64 reference, bound) of a case: computed once, shared, read-only"""
    if c["id"] not in _refs:
        o = cc.operands(c)
        v, bound = cc.reference(c, o)
        orc = cc.oracle(c, o)
        for a in list(o.values()) + [orc, v, bound]:
            if a is not None:
                a.setflags(write=False)
        _refs[c["id"]] = (o, orc, v, bound)
    return _refs[c["id"]]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_parity(got, orc, v, bound, what):
    """the two assertions of every f32 case"""
    assert got.shape == orc.shape == v.shape, what
    ratio = float((np.abs(got.astype(np.float64) - v) / bound).max())
    nbad = int((bits(got) != bits(orc)).sum())
    print(f"{what}: {nbad} of {got.size} words differ from the oracle; max |GPU - ref64| / bound = {ratio:.4f}", flush=True)
    assert nbad == 0, (what, "differs from the oracle", np.argwhere(bits(got) != bits(orc))[:8].tolist())
    assert ratio <= 1.0, (what, "outside the derived bound of the float64 reference", ratio)


def run_conv2d(h, c, o, prec=0):
    return h.conv2d(o["x"], o["w"], o["scale"], o["shift"], c["stride"], o["resid"], c["relu_in"], c["relu_out"], prec=prec)


def run_roi(h, c, o, segs):
    up = 2 if c["subpixel"] else 1
    shape = (c["n"], c["hh"] * up, c["ww"] * up, c["cout"])
    out = np.full(shape, SENTINEL, np.float32)
    out2 = np.full(shape, SENTINEL, np.float32) if c["copy"] else None
    h.conv2d_roi(o["x"], o["w"], o["scale"], o["shift"], segs, out, resid=o["resid"], rs=c["rs"], subpixel=c["subpixel"], relu_in=c["relu_in"],
                 relu_out=c["relu_out"], out_relu=out2)
    return out, out2


CASES_A, CASES_B, CASES_C = cc.cases_a(), cc.cases_b(), cc.cases_c()


# ---- A ----
@pytest.mark.parametrize("c", CASES_A, ids=[c["id"] for c in CASES_A])
def test_conv2d_f32(plain, c):
    o, orc, v, bound = ref_of(c)
    assert_parity(run_conv2d(plain, c, o), orc, v, bound, c["id"])


# ---- B ----
def test_forms_are_those_of_the_region_test():
    import test_gpu_conv_roi
    assert cc.FORMS == test_gpu_conv_roi.FORMS


@pytest.mark.parametrize("c", CASES_B, ids=[c["id"] for c in CASES_B])
def test_full_frame_launch_of_every_form(plain, c):
    o, orc, v, bound = ref_of(c)
    out, out2 = run_roi(plain, c, o, [])
    assert_parity(out, orc, v, bound, c["id"])
    if c["copy"]:
        assert np.array_equal(bits(out2), bits(np.maximum(out, 0) + 0.0)), (c["id"], "out_relu is not max(out, +0)")


# ---- C ----
@pytest.mark.parametrize("c,tables", CASES_C, ids=[c["id"] for c, _ in CASES_C])
def test_region_form_against_the_oracle(plain, c, tables):
    o, orc, v, bound = ref_of(c)
    up = 2 if c["subpixel"] else 1
    want = {"out": orc, "out_relu": np.maximum(orc, 0) + 0.0}
    for segs in tables:
        inside = np.zeros(orc.shape[:3], bool)
        for p0, npat, y0, x0, rh, rw in segs:
            assert 0 <= p0 and p0 + npat <= c["n"] and 0 <= y0 and y0 + rh <= c["hh"] and 0 <= x0 and x0 + rw <= c["ww"] and rw >= 2
            inside[p0:p0 + npat, y0 * up:(y0 + rh) * up, x0 * up:(x0 + rw) * up] = True
        out, out2 = run_roi(plain, c, o, segs)
        for what, g in (("out", out), ("out_relu", out2)):
            if g is None:
                continue
            bad_in = int((bits(g)[inside] != bits(want[what])[inside]).sum())
            bad_out = int((bits(g)[~inside] != SENT_BITS).sum())
            print(f"{c['id']}, {segs}, {what}: {bad_in} words differ from the oracle inside, {bad_out} words written outside", flush=True)
            assert bad_in == 0, (c["id"], segs, what, "differs from the oracle inside the rectangles")
            assert bad_out == 0, (c["id"], segs, what, "a word outside the rectangles was written")
        err = np.abs(out.astype(np.float64) - v)[inside]
        assert (err <= bound[inside]).all(), (c["id"], segs, "outside the derived bound of the float64 reference")


# ---- D ----
@pytest.mark.parametrize("c", CASES_A, ids=[c["id"] for c in CASES_A])
def test_f16_modes(plain, c):
    """The project's gate (tests/test_gpu_invdepth_f16.py): max|GPU(prec 3) - R_q| <= 4 max|O_q - R_q|, R_q = ref64 and O_q = the oracle on
    operands rounded to f16 (x, w and resid: f16-exact, so every mode multiplies the same numbers); prec 4 = round_f16(prec 3) bit for bit."""
    assert c["cin"] % 64 == 0 and c["n"] * (c["hh"] // c["stride"]) * (c["ww"] // c["stride"]) <= 1440
    o = cc.operands(c, f16_exact=True)
    rq, _ = cc.reference(c, o)
    oq = cc.oracle(c, o)
    g3 = run_conv2d(plain, c, o, prec=3)
    g4 = run_conv2d(plain, c, o, prec=4)
    e_gpu, e_orc = float(np.abs(g3.astype(np.float64) - rq).max()), float(np.abs(oq.astype(np.float64) - rq).max())
    ratio = e_gpu / e_orc if e_orc > 0 else float("inf") if e_gpu > 0 else 0.0
    print(f"{c['id']}: prec 3 |GPU-R| {e_gpu:.3e} |O-R| {e_orc:.3e} ratio {ratio:.2f}", flush=True)
    assert np.isfinite(g3).all() and e_gpu <= 4 * e_orc, (c["id"], e_gpu, e_orc)
    assert np.array_equal(bits(g4), bits(conv_ref.round_f16(g3))), (c["id"], "prec 4 is not round_f16(prec 3)")


# ---- E ----
def test_refusals(plain):
    """include/tmat.h: ksize 1 and 3 want cin % 64 == 0 (the sub-pixel form cin % 32 == 0), cout % 64 == 0, an output at least two pixels
    wide, even sizes at stride 2, ksize 3 at stride 1.  The checks of tmat_conv2d and launch_conv stand in front of the launch: a refused
    call returns TMAT_E_ARG with a message, the caller's output is not touched, and the handle goes on working."""
    from tmat_amd import _lib

    def conv2d(k, stride, cin, cout, hh, ww):
        x = np.zeros((1, hh, ww, cin), np.float32)
        return plain.conv2d(x, np.zeros((k, k, cin, cout), np.float32), None, np.zeros(cout, np.float32), stride)

    for what, args in [("ksize 1, Cin 32", (1, 1, 32, 64, 4, 4)), ("ksize 1, Cin 96", (1, 1, 96, 64, 4, 4)), ("ksize 3, Cin 96", (3, 1, 96, 64, 4, 4)),
                       ("Cout 32", (1, 1, 64, 32, 4, 4)), ("Cout 96", (3, 1, 64, 96, 4, 4)), ("ww = 1", (3, 1, 64, 64, 4, 1)),
                       ("stride 2, ww = 2", (1, 2, 64, 64, 4, 2)), ("stride 2, odd hh", (1, 2, 64, 64, 3, 4)), ("ksize 3, stride 2", (3, 2, 64, 64, 4, 4))]:
        with pytest.raises(_lib.TmatError) as e:
            conv2d(*args)
        print(f"{what}: {e.value}", flush=True)
        assert "launch_conv: unsupported shape" in str(e.value) or "tmat_conv2d: bad argument" in str(e.value), what
    # the same through the region entry point, whose output buffer is the caller's: it keeps every word
    for what, k, sub, cin, cout, ww in [("ksize 3, Cin 32", 3, False, 32, 64, 4), ("sub-pixel, Cin 48", 3, True, 48, 64, 4), ("Cout 96", 1, False, 64, 96, 4),
                                        ("ww = 1", 3, False, 64, 64, 1)]:
        up = 2 if sub else 1
        out = np.full((1, 4 * up, ww * up, cout), SENTINEL, np.float32)
        with pytest.raises(_lib.TmatError) as e:
            plain.conv2d_roi(np.zeros((1, 4, ww, cin), np.float32), np.zeros((k, k, cin, cout), np.float32), None, np.zeros(cout, np.float32), [], out, subpixel=sub)
        assert "launch_conv: unsupported shape" in str(e.value), what
        assert (bits(out) == SENT_BITS).all(), what
    c = CASES_A[0]
    o, orc, v, bound = ref_of(c)
    assert_parity(run_conv2d(plain, c, o), orc, v, bound, c["id"] + " after the refusals")

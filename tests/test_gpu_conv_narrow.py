"""GPU: conv_narrow_kernel (csrc/conv_narrow_kernels.hip), the convolution of the 16- and 32-channel layers, against CPU values.

In the manner of tests/test_gpu_conv_shapes.py (cases: tests/helpers/narrow_cases.py).  Every case is asserted twice: bit for bit against
the oracle (oracle/unet.py:_conv / _conv_subpixel, the same chain order) and within the DERIVED bound of the float64 reference
tests/helpers/conv_ref.py.
  A1  channels: every (Cin, Cout) the two narrow models launch, a short last K block (48, 80), a Cout that is no power of two, in the 1x1,
      3x3 and sub-pixel forms, bare and with scale + residual + both ReLUs + the activated copy;
  A2  pixels at 32 -> 32 and 16 -> 16: one row, widths 2 / 5 / 7, an odd width behind stride 2, non-square images, M around the 128-pixel
      tile and above twice it, n = 1 and 3;
  A3  on the shapes conv_mfma_kernel takes too, the two kernels give the same bits in all forms;
  B   the region form straight against the oracle: inside the rectangles the oracle's bits, outside the caller's sentinel;
  C   what launch_conv_narrow refuses, as include/tmat.h states it.
The process never imports torch."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import conv_cases as cc  # noqa: E402
import narrow_cases as nc  # noqa: E402

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
    assert got.shape == orc.shape == v.shape, what
    ratio = float((np.abs(got.astype(np.float64) - v) / bound).max())
    nbad = int((bits(got) != bits(orc)).sum())
    print(f"{what}: {nbad} of {got.size} words differ from the oracle; max |GPU - ref64| / bound = {ratio:.4f}", flush=True)
    assert nbad == 0, (what, "differs from the oracle", np.argwhere(bits(got) != bits(orc))[:8].tolist())
    assert ratio <= 1.0, (what, "outside the derived bound of the float64 reference", ratio)


def out_shape(c):
    up = 2 if c["subpixel"] else 1
    return (c["n"], c["hh"] * up // c["stride"], c["ww"] * up // c["stride"], c["cout"])


def run_narrow(h, c, o, segs):
    out = np.full(out_shape(c), SENTINEL, np.float32)
    out2 = np.full(out_shape(c), SENTINEL, np.float32) if c["copy"] else None
    h.conv2d_narrow(o["x"], o["w"], o["scale"], o["shift"], segs, out, stride=c["stride"], resid=o["resid"], rs=c["rs"], subpixel=c["subpixel"],
                    relu_in=c["relu_in"], relu_out=c["relu_out"], out_relu=out2)
    return out, out2


def check_full_frame(plain, c):
    o, orc, v, bound = ref_of(c)
    out, out2 = run_narrow(plain, c, o, [])
    assert_parity(out, orc, v, bound, c["id"])
    if c["copy"]:
        assert np.array_equal(bits(out2), bits(np.maximum(out, 0) + 0.0)), (c["id"], "out_relu is not max(out, +0)")


CASES_A1, CASES_A2, CASES_A3, CASES_B = nc.cases_a1(), nc.cases_a2(), nc.cases_a3(), nc.cases_b()


def test_case_tables():
    """what the tables promise: every narrow pair of the two models, the extra pairs, the pixel counts around the tile, the size limit"""
    pairs = {(c["cin"], c["cout"]) for c in CASES_A1}
    assert {(32, 64), (64, 32), (32, 32), (16, 32), (32, 16), (16, 16), (48, 48), (96, 32), (16, 80)} <= pairs
    ms = {c["n"] * (c["hh"] // c["stride"]) * (c["ww"] // c["stride"]) for c in CASES_A2 if not c["subpixel"]}
    assert {nc.TILE - 1, nc.TILE, nc.TILE + 1} <= ms and max(ms) > 2 * nc.TILE
    assert {c["n"] for c in CASES_A2} >= {1, 3} and {c["ww"] // c["stride"] for c in CASES_A2} >= {2, 3, 5, 7}
    for c in nc.all_cases():
        assert np.prod(out_shape(c)[:3]) < 20000, c["id"]
    assert len({c["id"] for c in nc.all_cases()}) == len(nc.all_cases())


# ---- A1, A2 ----
@pytest.mark.parametrize("c", CASES_A1, ids=[c["id"] for c in CASES_A1])
def test_channels(plain, c):
    check_full_frame(plain, c)


@pytest.mark.parametrize("c", CASES_A2, ids=[c["id"] for c in CASES_A2])
def test_pixels(plain, c):
    check_full_frame(plain, c)


# ---- A3 ----
@pytest.mark.parametrize("c,how", CASES_A3, ids=[c["id"] for c, _ in CASES_A3])
def test_same_bits_as_the_main_kernel(plain, c, how):
    o = cc.operands(c)
    out, out2 = run_narrow(plain, c, o, [])
    if how == "conv2d":
        main, main2 = plain.conv2d(o["x"], o["w"], o["scale"], o["shift"], c["stride"], o["resid"], c["relu_in"], c["relu_out"]), None
    else:
        main = np.full(out_shape(c), SENTINEL, np.float32)
        main2 = np.full(out_shape(c), SENTINEL, np.float32) if c["copy"] else None
        plain.conv2d_roi(o["x"], o["w"], o["scale"], o["shift"], [], main, resid=o["resid"], rs=c["rs"], subpixel=c["subpixel"], relu_in=c["relu_in"],
                         relu_out=c["relu_out"], out_relu=main2)
    nbad = int((bits(out) != bits(main)).sum())
    print(f"{c['id']}: {nbad} of {out.size} words differ between the kernels", flush=True)
    assert nbad == 0, c["id"]
    if c["copy"]:
        assert np.array_equal(bits(out2), bits(main2)), (c["id"], "out_relu")
    orc = cc.oracle(c, o)
    assert np.array_equal(bits(out), bits(orc)), (c["id"], "differs from the oracle")


# ---- B ----
@pytest.mark.parametrize("c,tables", CASES_B, ids=[c["id"] for c, _ in CASES_B])
def test_region_form_against_the_oracle(plain, c, tables):
    o, orc, v, bound = ref_of(c)
    up = 2 if c["subpixel"] else 1
    rh_max, rw_max = c["hh"] // c["stride"], c["ww"] // c["stride"]       # the rectangles enumerate output pixels (sub-pixel form: stored pixels)
    want = {"out": orc, "out_relu": np.maximum(orc, 0) + 0.0}
    for segs in tables:
        inside = np.zeros(orc.shape[:3], bool)
        for p0, npat, y0, x0, rh, rw in segs:
            assert 0 <= p0 and p0 + npat <= c["n"] and 0 <= y0 and y0 + rh <= rh_max and 0 <= x0 and x0 + rw <= rw_max and rw >= 2
            inside[p0:p0 + npat, y0 * up:(y0 + rh) * up, x0 * up:(x0 + rw) * up] = True
        out, out2 = run_narrow(plain, c, o, segs)
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


# ---- C ----
def test_refusals(plain):
    """include/tmat.h: cin and cout multiples of 16 (8 and 24 are refused), an output at least two pixels wide, ksize 3 at stride 1, no
    residual in the sub-pixel form.  A refused call returns TMAT_E_ARG with a message, the caller's output is not touched, and the
    handle goes on working."""
    from tmat_amd import _lib
    for what, k, st, sub, cin, cout, hh, ww, res in [("Cin 8", 1, 1, False, 8, 16, 4, 4, False), ("Cout 24", 3, 1, False, 16, 24, 4, 4, False),
                                                       ("ww = 1", 3, 1, False, 16, 16, 4, 1, False), ("ksize 3, stride 2", 3, 2, False, 16, 16, 4, 4, False),
                                                       ("sub-pixel with a residual", 3, 1, True, 32, 16, 4, 4, True)]:
        up = 2 if sub else 1
        shape = (1, hh * up // st, ww * up // st, cout)
        out = np.full(shape, SENTINEL, np.float32)
        resid = np.zeros((1, hh, ww, cout), np.float32) if res else None
        with pytest.raises(_lib.TmatError) as e:
            plain.conv2d_narrow(np.zeros((1, hh, ww, cin), np.float32), np.zeros((k, k, cin, cout), np.float32), None, np.zeros(cout, np.float32), [], out,
                                stride=st, subpixel=sub, resid=resid)
        print(f"{what}: {e.value}", flush=True)
        assert f"({_lib.E_ARG})" in str(e.value), what
        assert "launch_conv_narrow: unsupported shape" in str(e.value) or "tmat_conv2d_narrow: bad argument" in str(e.value), what
        assert (bits(out) == SENT_BITS).all(), what
    check_full_frame(plain, CASES_A1[0])

"""GPU: the region form of the MFMA convolution (conv_mfma_kernel<..., ROI>) on rectangles of any first column and width, through
tmat_conv2d_roi -- one launch with a segment table on host buffers.

The exact region plan (tests/test_roi_plan_exact.py) launches every layer's need itself, so odd first columns and odd widths are the
normal case.  A wave's group of 8 consecutive pixels (4 or 8 in the epilogue) may then break into the next row of the rectangle or into
the next patch: the prologue converts such pixels per lane, the row-split epilogue converts the group's first pixel on the scalar unit
and lets a lane choose between two row bases.  Checked here for every form the up path launches (3x3, 1x1, the sub-pixel form, the 3x3 with a same-resolution
and with a half-resolution residual, with the activated copy) at Cout 64 and 128 (8 and 4 pixels per epilogue group), on 20- and 24-pixel
patches: inside the rectangles the bits are those of the full-frame launch of the same convolution, outside every output word still
holds the sentinel the caller put there.  No tolerance: a computed pixel sees the same operands in the same order.
Reference: fl_tissue_model_tools/models.py:146-166 (the up path's convolutions)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.678)
N = 3
CIN = 64


def seg_sets(S):
    """(name, segments (p0, np, y0, x0, rh, rw)) for S x S patches"""
    return [
        # M = 130 in the first segment: a group straddles a row, a patch boundary and a tile, and M % 8 != 0; the second starts at column 0
        ("odd", [(0, 2, 1, 7, 5, 13), (2, 1, 0, 0, 7, 9)]),
        ("full rows", [(0, 3, 2, 0, 6, S)]),                # S = 20: no multiple of 8, rows follow each other without a gap
        ("rw 16", [(0, 3, 3, 4, 5, 16)]),                   # the row-uniform forms
        ("rw 16, odd column", [(0, 1, 3, 3, 5, 16), (1, 2, 0, 1, S, 16)]),     # row-uniform prologue, row-split epilogue (an odd column under the half-resolution residual)
        ("rw 5", [(0, 3, 2, 9, 6, 5)]),                     # below 8: the per-lane forms
        ("last columns", [(1, 2, S - 9, S - 11, 9, 11)]),   # patch 0 computes nothing; the rectangle ends in the patch's last pixel
    ]


FORMS = ["3x3", "1x1", "subpixel", "3x3 resid", "3x3 resid rs1", "3x3 resid copy", "3x3 resid rs1 copy"]


def rect_mask(segs, S, up):
    m = np.zeros((N, S * up, S * up), bool)
    for p0, npat, y0, x0, rh, rw in segs:
        m[p0:p0 + npat, y0 * up:(y0 + rh) * up, x0 * up:(x0 + rw) * up] = True
    return m


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("S", [20, 24])
def test_region_form_equals_full_frame_inside_and_keeps_the_rest(handle, S, cout, form):
    rs = np.random.RandomState(1000 * S + cout + len(form))
    k = 1 if form == "1x1" else 3
    sub = form == "subpixel"
    up = 2 if sub else 1
    x = rs.standard_normal((N, S, S, CIN)).astype(np.float32)
    w = (rs.standard_normal((k, k, CIN, cout)) / np.sqrt(k * k * CIN)).astype(np.float32)
    shift = rs.standard_normal(cout).astype(np.float32)
    scale = None if form == "1x1" else rs.uniform(0.5, 1.5, cout).astype(np.float32)
    r_shift = 1 if "rs1" in form else 0
    resid = rs.standard_normal((N, S >> r_shift, S >> r_shift, cout)).astype(np.float32) if "resid" in form else None
    copy = "copy" in form
    kw = dict(resid=resid, rs=r_shift, subpixel=sub, relu_in=form in ("3x3", "subpixel"), relu_out=sub)
    shape = (N, S * up, S * up, cout)

    def run(segs):
        out = np.full(shape, SENTINEL, np.float32)
        out2 = np.full(shape, SENTINEL, np.float32) if copy else None
        handle.conv2d_roi(x, w, scale, shift, segs, out, out_relu=out2, **kw)
        return out, out2

    ref, ref2 = run([])                                      # the full-frame launch (ROI = false) of the same convolution
    assert not (ref.view(np.uint32) == SENTINEL.view(np.uint32)).all(axis=-1).any(), "the full-frame launch writes every pixel"
    if copy:
        assert np.array_equal(ref2, np.maximum(ref, 0) + 0.0)
    for name, segs in seg_sets(S):
        got, got2 = run(segs)
        inside = rect_mask(segs, S, up)
        for what, g, r in (("out", got, ref), ("out_relu", got2, ref2)):
            if g is None:
                continue
            gu, ru = g.view(np.uint32), r.view(np.uint32)
            bad_in = int((gu[inside] != ru[inside]).sum())
            bad_out = int((gu[~inside] != SENTINEL.view(np.uint32)).sum())
            print(f"{S} x {S}, Cout {cout}, {form}, {name}, {what}: {bad_in} words differ inside, {bad_out} words written outside")
            assert bad_in == 0, (name, what, "differs from the full-frame launch inside the rectangles")
            assert bad_out == 0, (name, what, "a word outside the rectangles was written")


def test_bad_segment_tables_are_refused(handle):
    from tmat_amd import _lib
    x = np.zeros((N, 20, 20, CIN), np.float32)
    w = np.zeros((3, 3, CIN, 64), np.float32)
    out = np.zeros((N, 20, 20, 64), np.float32)
    for segs in ([(0, 2, 1, 7, 5, 14)], [(0, 4, 0, 0, 4, 8)], [(1, 1, 0, 0, 4, 8), (0, 1, 0, 0, 4, 8)], [(0, 1, 0, 0, 4, 1)]):
        with pytest.raises(_lib.TmatError):
            handle.conv2d_roi(x, w, None, np.zeros(64, np.float32), segs, out)

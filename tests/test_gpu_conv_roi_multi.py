"""GPU: the region form of the MFMA convolution (conv_mfma_kernel<..., ROI>) with SEVERAL disjoint rectangles on one patch range, through
tmat_conv2d_roi.

The shared-interior form of the down path's rectangle launches (tests/test_roi_plan_share_rect.py) gives a class up to four rectangles:
its segment table names the class's patch range once per rectangle.  Inside the kernel only the tile -> segment search sees the longer
table; every segment still owns its M tiles.  Checked here as tests/test_gpu_conv_roi.py does: inside the rectangles the bits are
those of the full-frame launch of the same convolution, outside every output word still holds the sentinel the caller put there.  No
tolerance: a computed pixel sees the same operands in the same order.  The stride-2 1x1 form (the down path's residual launch, through
tmat_conv2d_roi_s2) takes a 2 S x 2 S input, so that its output has the same S x S pixels and the same segment sets apply."""
import numpy as np
import pytest

from test_gpu_conv_roi import CIN, N, SENTINEL, rect_mask

pytestmark = pytest.mark.gpu


def seg_sets(S):
    """(name, segments (p0, np, y0, x0, rh, rw)) for S x S patches"""
    return [
        # two rectangles on one range; the first has 3 * 5 * 12 = 180 pixels, so with 128-pixel tiles the second M tile of the launch
        # holds the first segment's tail (52 pixels) and the next tile starts the second segment of the SAME patches
        ("two, a tile boundary between them", [(0, 3, 1, 0, 5, 12), (0, 3, 1, 16, 5, 4)]),
        # three: a far-side strip 4 wide that ends in the patch's last column
        ("three, last columns", [(0, 2, 0, 0, 7, 8), (0, 2, 0, S - 4, 7, 4), (0, 2, 10, 0, 6, 8), (2, 1, 2, 4, 9, 12)]),
        # four: the product of two row and two column intervals, then another range with one rectangle
        ("four", [(0, 2, 0, 0, 6, 12), (0, 2, 0, 16, 6, 4), (0, 2, 9, 0, S - 9, 12), (0, 2, 9, 16, S - 9, 4), (2, 1, 3, 8, 5, 8)]),
        # more than 16 segments: single rows, three column strips each, on two patch ranges
        ("eighteen", [(0, 2, y, x0, 1, 4) for y in (0, 3, 6) for x0 in (0, 8, 16)] + [(2, 1, y, x0, 2, 4) for y in (1, 5, 9) for x0 in (4, 12, S - 4)]),
    ]


FORMS = ["1x1", "1x1 stride 2", "3x3 resid rs1 copy"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("S", [20, 24])
def test_several_rectangles_per_patch_equal_the_full_frame_launch(handle, S, cout, form):
    rs = np.random.RandomState(2000 * S + cout + len(form))
    k = 1 if form.startswith("1x1") else 3
    s2 = form == "1x1 stride 2"
    x = rs.standard_normal((N, 2 * S, 2 * S, CIN) if s2 else (N, S, S, CIN)).astype(np.float32)
    w = (rs.standard_normal((k, k, CIN, cout)) / np.sqrt(k * k * CIN)).astype(np.float32)
    shift = rs.standard_normal(cout).astype(np.float32)
    scale = None if k == 1 else rs.uniform(0.5, 1.5, cout).astype(np.float32)
    r_shift = 1 if "rs1" in form else 0
    resid = rs.standard_normal((N, S >> r_shift, S >> r_shift, cout)).astype(np.float32) if "resid" in form else None
    copy = "copy" in form
    kw = dict(resid=resid, rs=r_shift)
    shape = (N, S, S, cout)

    def run(segs):
        out = np.full(shape, SENTINEL, np.float32)
        out2 = np.full(shape, SENTINEL, np.float32) if copy else None
        if s2:
            handle.conv2d_roi_s2(x, w, scale, shift, segs, out)
        else:
            handle.conv2d_roi(x, w, scale, shift, segs, out, out_relu=out2, **kw)
        return out, out2

    ref, ref2 = run([])
    assert not (ref.view(np.uint32) == SENTINEL.view(np.uint32)).all(axis=-1).any(), "the full-frame launch writes every pixel"
    for name, segs in seg_sets(S):
        if name == "eighteen":
            assert len(segs) > 16
        got, got2 = run(segs)
        inside = rect_mask(segs, S, 1)
        assert inside.sum() == sum(s[1] * s[4] * s[5] for s in segs), "the rectangles of a set are disjoint"
        for what, g, r in (("out", got, ref), ("out_relu", got2, ref2)):
            if g is None:
                continue
            gu, ru = g.view(np.uint32), r.view(np.uint32)
            bad_in = int((gu[inside] != ru[inside]).sum())
            bad_out = int((gu[~inside] != SENTINEL.view(np.uint32)).sum())
            print(f"{S} x {S}, Cout {cout}, {form}, {name}, {what}: {bad_in} words differ inside, {bad_out} words written outside")
            assert bad_in == 0, (name, what, "differs from the full-frame launch inside the rectangles")
            assert bad_out == 0, (name, what, "a word outside the rectangles was written")

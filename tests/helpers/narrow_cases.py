"""The case table of tests/test_gpu_conv_narrow.py: conv_narrow_kernel (csrc/conv_narrow_kernels.hip) against the oracle and the float64
reference.  A case is a dict of conv_cases' kind (its `operands`, `oracle` and `reference` evaluate these too).  numpy only."""
import conv_cases as cc

TILE = 128          # pixels per workgroup of the kernel (NW_BM): four waves of 32

# ---- A1: channels.  The pairs the two narrow models launch (the table of DESIGN 4.1.8), then a short last K block (48, 80, 96 = 32 + 32 + 32
# is whole), a Cout that is no power of two (48, 80: a half-empty last column tile), one and three column groups ----
PAIRS_A1 = [(32, 64), (64, 32), (32, 32), (16, 32), (32, 16), (16, 16), (16, 64), (64, 16), (48, 48), (96, 32), (16, 80), (80, 48)]
IMAGE_A1 = (2, 6, 11)                   # M = 132: a full tile and a tail of four pixels; an odd width

# ---- A2: pixels, at 32 -> 32 and 16 -> 16: (ksize, stride, subpixel, n, hh, ww, the point of the case) ----
SHAPES_A2 = [
    (1, 1, False, 1, 1, 2, "M = 2, the smallest accepted"),
    (3, 1, False, 1, 1, TILE - 1, "one row: upper and lower taps all outside; M one short of the tile"),
    (3, 1, False, 1, 8, TILE // 8, "M = the tile"),
    (3, 1, False, 1, 3, 43, "M = 129: one pixel in the second tile"),
    (3, 1, False, 1, 9, 2, "width 2: every pixel on a border"),
    (3, 1, False, 2, 4, 5, "width 5"),
    (3, 1, False, 2, 5, 7, "width 7, odd height, waves cross rows and images"),
    (1, 1, False, 3, 5, 17, "M = 255"),
    (1, 1, False, 1, 1, 2 * TILE + 1, "M above twice the tile"),
    (3, 1, False, 3, 7, 13, "M = 273, three images"),
    (1, 2, False, 2, 4, 6, "an odd width behind stride 2 (6 -> 3)"),
    (1, 2, False, 1, 14, 28, "stride 2, Wo = 14"),
    (1, 2, False, 3, 2, 4, "stride 2 down to one row of two"),
    (3, 1, False, 3, 20, 24, "non-square"),
    (3, 1, False, 2, 24, 20, "non-square, the other way"),
    (3, 1, True, 1, 3, 2, "sub-pixel form, width 2"),
    (3, 1, True, 2, 5, 7, "sub-pixel form, odd sizes"),
    (3, 1, True, 3, 6, 8, "sub-pixel form, M = 144"),
]

# ---- A3: the shapes conv_mfma_kernel takes too ----
PAIRS_A3 = [(64, 64), (64, 128), (128, 64)]
IMAGE_A3 = (2, 6, 10)

# ---- B: region form.  (image as (n, hh, ww) of the pixels the rectangles enumerate, [segment tables (p0, np, y0, x0, rh, rw)]) ----
REGIONS_B = cc.REGIONS_C + [
    ((3, 8, 12), [
        [(0, 3, 1, 1, 4, 9)],                                               # one rectangle, odd first column, 9 wide
        [(0, 2, 0, 0, 3, 2), (0, 2, 3, 3, 3, 5), (2, 1, 2, 5, 4, 5)],       # two disjoint rectangles on one patch range, 2 and 5 wide
        [(1, 1, 0, 1, 6, 2), (1, 1, 0, 4, 2, 5), (1, 1, 3, 3, 3, 7)],       # three on one range; patches 0 and 2 compute nothing
    ]),
]


def case(ksize, stride, cin, cout, n, hh, ww, subpixel, full, seed, rs=0, copy=None, tag=""):
    """`full`: scale + residual + both ReLUs + the activated copy (the sub-pixel form and stride 2 have no residual and the sub-pixel form no
    copy: the entry point's contract)"""
    resid = full and not subpixel and stride == 1
    copy = (full and not subpixel) if copy is None else copy
    return dict(ksize=ksize, stride=stride, cin=cin, cout=cout, n=n, hh=hh, ww=ww, subpixel=subpixel, scale=full, resid=resid, rs=rs if resid else 0,
                relu_in=full, relu_out=full, copy=copy, seed=seed,
                id=f"{tag}k{ksize} s{stride}{' sub' if subpixel else ''} {cin}->{cout} {n}x{hh}x{ww} {'full' if full else 'bare'}")


def cases_a1():
    out = []
    n, hh, ww = IMAGE_A1
    for i, (cin, cout) in enumerate(PAIRS_A1):
        for fi, (k, sub) in enumerate([(1, False), (3, False), (3, True)]):
            for full in (False, True):
                out.append(case(k, 1, cin, cout, n, hh, ww, sub, full, 11000 + 10 * i + 2 * fi + full))
    return out


def cases_a2():
    out = []
    for ci, c in enumerate((32, 16)):
        for i, (k, st, sub, n, hh, ww, _) in enumerate(SHAPES_A2):
            for full in (False, True):
                # the full form at even sizes takes its residual at half resolution on every other shape
                rs = 1 if (full and not (hh | ww) & 1 and i % 2 == 0) else 0
                out.append(case(k, st, c, c, n, hh, ww, sub, full, 12000 + 100 * ci + 2 * i + full, rs=rs))
    return out


def cases_a3():
    """(case, how the main kernel runs it: "roi" through conv2d_roi without segments, "conv2d" for stride 2)"""
    out = []
    n, hh, ww = IMAGE_A3
    for i, (cin, cout) in enumerate(PAIRS_A3):
        for fi, form in enumerate(cc.FORMS):
            c = cc.form_case(form, cin, cout, n, hh, ww, 13000 + 10 * i + fi)
            out.append((c, "roi"))
        out.append((case(1, 2, cin, cout, n, hh, ww, False, False, 13500 + i), "conv2d"))
    return out


def cases_b():
    """(case, segment tables): 32 -> 32 3x3 with the half-resolution residual and the activated copy, 64 -> 32 sub-pixel, 32 -> 64 1x1 at stride 2"""
    out = []
    for ii, ((n, hh, ww), tables) in enumerate(REGIONS_B):
        out.append((cc.form_case("3x3 resid rs1 copy", 32, 32, n, hh, ww, 14000 + ii), tables))
        out.append((cc.form_case("subpixel", 64, 32, n, hh, ww, 14100 + ii), tables))
        # the rectangles are output pixels: the input is twice the size
        out.append((case(1, 2, 32, 64, n, 2 * hh, 2 * ww, False, True, 14200 + ii), tables))
        out.append((cc.form_case("1x1", 16, 16, n, hh, ww, 14300 + ii), tables))
    return out


def all_cases():
    return cases_a1() + cases_a2() + [c for c, _ in cases_a3()] + [c for c, _ in cases_b()]

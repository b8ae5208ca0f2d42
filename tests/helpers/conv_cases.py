"""The case table of tests/test_conv_ref.py (CPU: oracle against the float64 reference) and tests/test_gpu_conv_shapes.py (GPU: kernel
against both): shapes OFF the networks' grid, chosen by the code paths of conv_mfma_kernel (csrc/unet_kernels.hip) that the output
shape selects.  numpy only.  A case is a dict; `operands` makes its arrays, `oracle` / `reference` evaluate it on the CPU."""
import numpy as np

import conv_ref

# ---- A: tmat_conv2d, prec 0.  (ksize, stride, cin, cout, n, hh, ww, the point of the case); each runs bare and full ----
SHAPES_A = [
    (1, 1, 64, 64, 1, 1, 2, "M = 2, the smallest accepted"),
    (3, 1, 64, 64, 1, 1, 127, "one row: upper and lower taps all outside; M one short of a tile"),
    (3, 1, 64, 128, 1, 3, 43, "M = 129"),
    (3, 1, 128, 64, 1, 9, 2, "every pixel on a border"),
    (3, 1, 64, 128, 2, 5, 7, "groups of 8 cross rows and images"),
    (1, 1, 64, 256, 3, 5, 17, "M = 255, flat form"),
    (1, 1, 128, 64, 1, 1, 257, "M = 257, flat form"),
    (1, 1, 64, 64, 1, 8, 16, "exactly one tile"),
    (1, 2, 64, 128, 2, 2, 4, "stride 2 down to one row of two"),
    (1, 2, 128, 192, 3, 6, 10, "odd Wo behind a stride; three 64-wide column tiles"),
    (1, 2, 64, 64, 1, 14, 28, "Wo = 14 behind a stride"),
    (3, 1, 192, 384, 1, 3, 33, "Cin 192; three 128-wide column tiles"),
    (3, 1, 64, 64, 3, 20, 24, "non-square, Wo % 8 == 0"),
    (3, 1, 64, 128, 2, 24, 20, "non-square, Wo % 8 != 0"),
    # weights above 3 MB with 2 / 4 / 8 column tiles: launch_conv_ks picks the N-stationary block mapping (XCD x keeps column tile x % nNt).
    # The networks reach it with the 512 -> 512 3x3 layers only (four tiles, whole 20 x 20 patches); these are two and eight tiles, M off the tiles
    (3, 1, 512, 256, 3, 7, 13, "N-stationary mapping, two column tiles, M = 273: three pixel tiles"),
    (1, 1, 1024, 1024, 1, 3, 5, "N-stationary mapping, eight column tiles, flat form, M = 15"),
]

# ---- B: tmat_conv2d_roi without segments: the forms of tests/test_gpu_conv_roi.py (that file's FORMS; the GPU test checks the two lists agree) ----
FORMS = ["3x3", "1x1", "subpixel", "3x3 resid", "3x3 resid rs1", "3x3 resid copy", "3x3 resid rs1 copy"]
IMAGES_B = [(3, 20, 20), (3, 24, 24), (2, 6, 10), (1, 2, 2)]
IMAGE_B_ODD = (2, 5, 7)             # odd sizes: the forms without the half-resolution residual

# ---- C: the region form straight against the oracle: (image, [segment tables (p0, np, y0, x0, rh, rw)]) ----
FORMS_C = ["3x3 resid rs1 copy", "subpixel", "1x1"]
REGIONS_C = [
    ((3, 6, 10), [
        # 9 wide from an odd column to the last one (>= 8, no multiple of 4 or 8); 7 wide from an odd column, ending in the last pixel of patch 2
        [(0, 1, 1, 1, 4, 9), (1, 2, 0, 3, 6, 7)],
        # whole rows of 10 (rows follow each other without a gap); 5 wide from an odd column, ending in the last pixel
        [(0, 2, 0, 0, 3, 10), (2, 1, 2, 5, 4, 5)],
    ]),
    ((3, 10, 14), [
        # 13 wide from column 1 ending in the last pixel; 3 wide over every row
        [(0, 2, 3, 1, 7, 13), (2, 1, 0, 5, 10, 3)],
        # 11 wide from an odd column; 12 wide (a multiple of 4, not of 8); one row of 7 ending in the last pixel
        [(0, 1, 0, 3, 5, 11), (1, 1, 2, 0, 8, 12), (2, 1, 9, 7, 1, 7)],
    ]),
]


def form_case(form, cin, cout, n, hh, ww, seed):
    k = 1 if form == "1x1" else 3
    sub = form == "subpixel"
    return dict(ksize=k, stride=1, cin=cin, cout=cout, n=n, hh=hh, ww=ww, subpixel=sub, scale=form != "1x1", resid="resid" in form,
                rs=1 if "rs1" in form else 0, relu_in=form in ("3x3", "subpixel"), relu_out=sub, copy="copy" in form, seed=seed,
                id=f"{form} {cin}->{cout} {n}x{hh}x{ww}")


def cases_a():
    out = []
    for i, (k, st, cin, cout, n, hh, ww, _) in enumerate(SHAPES_A):
        for full in (False, True):
            out.append(dict(ksize=k, stride=st, cin=cin, cout=cout, n=n, hh=hh, ww=ww, subpixel=False, scale=full, resid=full, rs=0,
                            relu_in=full, relu_out=full, copy=False, seed=7000 + 2 * i + full,
                            id=f"k{k} s{st} {cin}->{cout} {n}x{hh}x{ww} {'full' if full else 'bare'}"))
    return out


def cases_b():
    out = []
    for cout in (64, 128):
        for fi, form in enumerate(FORMS):
            imgs = IMAGES_B + ([IMAGE_B_ODD] if "rs1" not in form else [])
            for ii, (n, hh, ww) in enumerate(imgs):
                out.append(form_case(form, 64, cout, n, hh, ww, 8000 + 100 * fi + 10 * ii + cout // 64))
        out.append(form_case("subpixel", 32, cout, 1, 3, 2, 8900 + cout // 64))
    return out


def cases_c():
    """(case, segment tables)"""
    out = []
    for cout in (64, 128):
        for fi, form in enumerate(FORMS_C):
            for ii, ((n, hh, ww), tables) in enumerate(REGIONS_C):
                out.append((form_case(form, 64, cout, n, hh, ww, 9000 + 100 * fi + 10 * ii + cout // 64), tables))
    return out


def all_cases():
    return cases_a() + cases_b() + [c for c, _ in cases_c()]


def operands(c, f16_exact=False):
    """x standard normal, w normal / sqrt(taps cin), scale in (0.5, 1.5), shift and resid normal; `f16_exact`: x, w and resid rounded to f16"""
    rs = np.random.RandomState(c["seed"])
    k, cin, cout = c["ksize"], c["cin"], c["cout"]
    x = rs.standard_normal((c["n"], c["hh"], c["ww"], cin)).astype(np.float32)
    w = (rs.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, cout).astype(np.float32) if c["scale"] else None
    shift = rs.standard_normal(cout).astype(np.float32)
    up = 2 if c["subpixel"] else 1
    Ho, Wo = c["hh"] * up // c["stride"], c["ww"] * up // c["stride"]
    resid = rs.standard_normal((c["n"], Ho >> c["rs"], Wo >> c["rs"], cout)).astype(np.float32) if c["resid"] else None
    if f16_exact:
        x, w = conv_ref.round_f16(x), conv_ref.round_f16(w)
        resid = None if resid is None else conv_ref.round_f16(resid)
    return dict(x=x, w=w, scale=scale, shift=shift, resid=resid)


def oracle(c, o):
    """oracle/unet.py on the case: _conv, or _conv_subpixel (the pre-summed 4-tap form the kernel runs) for the sub-pixel form"""
    from oracle import unet as ou
    if c["subpixel"]:
        return ou._conv_subpixel(o["x"], o["w"], int(c["relu_in"]), o["scale"], o["shift"], int(c["relu_out"]))
    return ou._conv(o["x"], o["w"], c["ksize"], c["stride"], 0, int(c["relu_in"]), o["scale"], o["shift"], o["resid"], c["rs"], int(c["relu_out"]))


def reference(c, o, mutation=None):
    """(v, bound): conv_ref.ref64 on the case (the sub-pixel form as the 3x3 over the upsampled input) and the derived float32 bound"""
    v, mag = conv_ref.ref64(o["x"], o["w"], c["ksize"], c["stride"], int(c["subpixel"]), c["relu_in"], o["scale"], o["shift"], o["resid"], c["rs"],
                            c["relu_out"], mutation=mutation)
    return v, conv_ref.bound(mag, c["ksize"], c["cin"], c["subpixel"])

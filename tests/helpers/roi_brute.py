"""Brute force for the region-plan tests: what the smooth blend reads of every patch, and what of every up-path layer those reads
depend on, as boolean masks -- by enumerating blend_kernel's gathers and dilating masks, with no interval arithmetic and nothing taken
from csrc/roi_plan.cpp.
Reference: fl_tissue_model_tools/smooth_tiled_predictions.py:68-79, 136-217 (pad, tile, blend, crop), models.py:146-166 (up path)."""
import numpy as np


def geom(hh, ww, ws):
    """the tiling of an (hh, ww) image (blend_kernels.hip:make_geom): padded frame, windows per orientation, first tile per orientation"""
    step, aug = ws // 2, (ws + 1) // 2
    Hp, Wp = hh + 2 * aug, ww + 2 * aug
    cntH, cntW = (Hp - ws) // step + 1, (Wp - ws) // step + 1
    na, nb = (cntH, cntW), (cntW, cntH)
    off, o = [], 0
    for g in range(8):
        off.append(o)
        o += na[g & 1] * nb[g & 1]
    return dict(hh=hh, ww=ww, ws=ws, step=step, aug=aug, Hp=Hp, Wp=Wp, na=na, nb=nb, off=off, tiles=o)


def pad_to_frame(g, y, x, Hp, Wp):
    """blend_kernels.hip:pad_to_frame: padded-image pixel -> pixel of orientation g's frame"""
    k = g & 3
    xp = Wp - 1 - x if g & 4 else x
    if k == 0:
        return y, xp
    if k == 1:
        return Wp - 1 - xp, y
    if k == 2:
        return Hp - 1 - y, Wp - 1 - xp
    return xp, Hp - 1 - y


def blend_reads(gm):
    """[tiles][ws][ws] bool: the (patch, p, q) that blend_kernel gathers (its loop bounds restated)"""
    ws, step = gm["ws"], gm["step"]
    read = np.zeros((gm["tiles"], ws, ws), bool)
    yo, xo = np.mgrid[0:gm["hh"], 0:gm["ww"]]
    y, x = yo + gm["aug"], xo + gm["aug"]
    for g in range(8):
        u, v = pad_to_frame(g, y, x, gm["Hp"], gm["Wp"])
        na, nb = gm["na"][g & 1], gm["nb"][g & 1]
        a_hi = np.minimum(u // step, na - 1)
        a_lo = np.where(u - ws + step > 0, (u - ws + step) // step, 0)
        b_hi = np.minimum(v // step, nb - 1)
        b_lo = np.where(v - ws + step > 0, (v - ws + step) // step, 0)
        for a in range(na):
            p = u - a * step
            oka = (a >= a_lo) & (a <= a_hi) & (p < ws)
            for b in range(nb):
                q = v - b * step
                ok = oka & (b >= b_lo) & (b <= b_hi) & (q < ws)
                assert (p[ok] >= 0).all() and (q[ok] >= 0).all()
                read[gm["off"][g] + a * nb + b, p[ok], q[ok]] = True
    return read


def dil3(m):
    """3 x 3 binary dilation, clipped to the frame"""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def half_any(m):
    """a half-resolution pixel is needed when any of the 2 x 2 pixels on it is ((y >> 1, x >> 1))"""
    return m[0::2, 0::2] | m[0::2, 1::2] | m[1::2, 0::2] | m[1::2, 1::2]


def subpixel_sources(t1):
    """stored pixels a sub-pixel layer reads for the needed outputs t1: output (2i + py, 2j + px) sees stored
    (i + py - 1 + {0, 1}, j + px - 1 + {0, 1})"""
    R = t1.shape[0] // 2
    need = np.zeros((R, R), bool)
    for py in range(2):
        for px in range(2):
            i, j = np.nonzero(t1[py::2, px::2])
            for da in range(2):
                for db in range(2):
                    ii, jj = i + py - 1 + da, j + px - 1 + db
                    ok = (ii >= 0) & (ii < R) & (jj >= 0) & (jj < R)
                    need[ii[ok], jj[ok]] = True
    return need


def rect_mask(r, R, scale=1):
    """the rectangle (y0, x0, rows, columns) of an R x R layer as a mask, each pixel blown up to scale x scale"""
    m = np.zeros((R * scale, R * scale), bool)
    y0, x0, rh, rw = (int(v) for v in r)
    m[y0 * scale:(y0 + rh) * scale, x0 * scale:(x0 + rw) * scale] = True
    return m


def layer_res(layer, ws, n_up):
    """side of the square that layer 3 j + kind (or the final convolution, 3 n_up) enumerates"""
    if layer == 3 * n_up:
        return ws // 2
    j, kind = divmod(layer, 3)
    Hs = ws >> n_up if j == 0 else (ws >> n_up) << (j - 1)
    return Hs if kind < 2 or j == 0 else 2 * Hs


def layer_needs(out_need, n_up):
    """[3 n_up + 1] masks: the pixels every layer has to compute for the network outputs out_need (ws x ws) to be right.
    3 j: first convolution of up block j (sub-pixel form for j > 0: stored pixels), 3 j + 1: residual 1x1, 3 j + 2: second 3x3."""
    need = [None] * (3 * n_up + 1)
    need[3 * n_up] = half_any(out_need)                 # final convolution: stored pixels whose 2 x 2 outputs are read
    s_need = dil3(need[3 * n_up])                       # of the last block's output
    for j in range(n_up - 1, -1, -1):
        need[3 * j + 2] = s_need
        t1_need = dil3(s_need)
        need[3 * j + 1] = half_any(s_need) if j else s_need
        need[3 * j] = half_any(t1_need) if j else t1_need       # sub-pixel form: stored pixel i makes outputs 2i, 2i + 1
        if j:
            s_need = need[3 * j + 1] | subpixel_sources(t1_need)    # plain copy for the residual, activated copy for the first convolution
    return need

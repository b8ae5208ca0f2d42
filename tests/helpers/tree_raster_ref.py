"""numpy restatement of the tree overlay, barcode and branch colour specifications (DESIGN.md "Tree overlay and barcode pictures").
Written from the specification: float32 arithmetic, one operation per statement, vectorised over the pixels.  A pixel centre farther
than the capsule's reach from a segment has coverage 0 and C + 0 * (col - C) == C exactly, so each segment is only evaluated on its
bounding box grown by the reach and two pixels of slack."""
import math

import numpy as np

F = np.float32


def branch_color(i):
    """hue byte = floor(step i) mod 256; H = 2 hue mod 360, S = 220 / 255, V = 1; HSV -> RGB; floor(255 v + 0.5); (B, G, R) used as (R, G, B)"""
    step = 180 * 0.618033988749895
    hue = int(math.floor(step * i)) % 256
    H, S, V = float((2 * hue) % 360), 220.0 / 255.0, 1.0
    hh = H / 60.0
    k = int(hh)
    f = hh - k
    p, q, t = V * (1.0 - S), V * (1.0 - S * f), V * (1.0 - S * (1.0 - f))
    r, g, b = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)][k]
    return np.array([math.floor(255.0 * c + 0.5) for c in (b, g, r)], np.uint8)


def canvas_shape(bh, bw, vis_width):
    return int(round(vis_width * bh / bw)), int(vis_width)          # Python's round: half to even


def _sample_index(n_dst, n_src):
    p = np.arange(n_dst, dtype=F)
    u = ((p + F(0.5)) * F(n_src)) / F(n_dst) - F(0.5)
    return np.clip(np.floor(u + F(0.5)).astype(np.int64), 0, n_src - 1)


def _to_canvas(v, n_dst, n_src):
    v = np.asarray(v, np.float64).astype(F)
    return ((v + F(0.5)) * F(n_dst)) / F(n_src) - F(0.5)


def render_tree(background, segs, seg_branch, vis_width):
    """one (bh, bw) u16 / f32 background, segs (k, 4) f64 [x1, y1, x2, y2] in background pixels -> (vh, vw, 3) u8"""
    bg = np.asarray(background).astype(F)
    bh, bw = bg.shape
    vh, vw = canvas_shape(bh, bw, vis_width)
    mn, mx = bg.min(), bg.max()
    rng = mx - mn
    if rng > 0:
        grey = np.floor(((bg - mn) / rng) * F(255) + F(0.5))
    else:
        grey = np.zeros_like(bg)
    g = grey[_sample_index(vh, bh)][:, _sample_index(vw, bw)]
    C = np.repeat(g[:, :, None], 3, axis=2).astype(F)
    rp = F(0.75 * (200.0 / 72.0) * (vis_width / 2000.0)) + F(0.5)
    segs = np.asarray(segs, np.float64).reshape(-1, 4)
    for s, bi in zip(segs, np.asarray(seg_branch).reshape(-1)):
        if not np.all(np.isfinite(s)):
            continue
        x1, x2 = _to_canvas(s[[0, 2]], vw, bw)
        y1, y2 = _to_canvas(s[[1, 3]], vh, bh)
        if not np.all(np.isfinite([x1, y1, x2, y2])):
            continue
        col = branch_color(int(bi)).astype(F)
        m = float(rp) + 2.0
        xa, xb = int(max(0, math.floor(min(x1, x2) - m))), int(min(vw, math.ceil(max(x1, x2) + m) + 1))
        ya, yb = int(max(0, math.floor(min(y1, y2) - m))), int(min(vh, math.ceil(max(y1, y2) + m) + 1))
        if xa >= xb or ya >= yb:
            continue
        cx = np.arange(xa, xb, dtype=F)[None, :]
        cy = np.arange(ya, yb, dtype=F)[:, None]
        dx, dy = x2 - x1, y2 - y1
        len2 = dx * dx + dy * dy
        px, py = cx - x1, cy - y1
        if len2 > 0:
            t = (px * dx + py * dy) / len2
            t = np.minimum(np.maximum(t, F(0)), F(1))
        else:
            t = np.zeros((yb - ya, xb - xa), F)
        ex, ey = px - t * dx, py - t * dy
        d = np.sqrt(ex * ex + ey * ey)
        a = np.minimum(np.maximum(rp - d, F(0)), F(1))
        assert a.dtype == F and d.dtype == F
        for ch in range(3):
            C[ya:yb, xa:xb, ch] = C[ya:yb, xa:xb, ch] + a * (col[ch] - C[ya:yb, xa:xb, ch])
    return np.floor(C + F(0.5)).astype(np.uint8)


def render_barcode(bars, vis_width):
    bars = np.asarray(bars, np.float64).reshape(-1, 2)
    S = int(round(vis_width * 0.9))
    out = np.full((S, S, 3), 255, np.uint8)
    n = len(bars)
    if n == 0:
        return out
    lo, hi = bars[:, 0].min(), bars[:, 1].max()
    span = hi - lo
    if not (span > 0 and np.isfinite(span)):
        return out
    order = sorted(range(n), key=lambda i: -bars[i, 0])             # sorted() is stable: birth descending
    pitch = S / n

    def edge(v):
        return int(min(S, max(0.0, math.floor((v - lo) / span * S + 0.5))))

    for k, bi in enumerate(order):
        xa, xb = edge(bars[bi, 0]), edge(bars[bi, 1])
        ya, yb = int(math.floor((k + 0.1) * pitch + 0.5)), int(math.floor((k + 0.9) * pitch + 0.5))
        if yb > ya and xb > xa:
            out[S - yb: S - ya, xa:xb] = branch_color(bi)          # row 0 of the bar chart is the lowest picture row
    return out

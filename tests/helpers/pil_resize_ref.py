"""Pillow's resize of a mode-"F" image restated in Python (LANCZOS: the two-pass convolution resample; NEAREST: the affine scale whose
source coordinate accumulates), for the tests of tmat_resize_pil_f32 where Pillow itself is absent, and the cases of
tests/golden/pil_resize.npz (tools/make_goldens.py:gen_pil_resize).  sin is libm's (math.sin), not numpy's."""
import math

import numpy as np

SHAPES = [(37, 23), (75, 130), (64, 64)]
RATIOS = [0.625, 0.5, 0.3, 1.6]
FILTERS = ["lanczos", "nearest"]


def cases():
    """(key, input shape, output shape (rows, cols), filter): every shape at every ratio, the non-square ones also with the axes' targets
    swapped (what predict(auto_resample=True) asks for), and one with an axis unchanged"""
    out = []
    for shape in SHAPES:
        for r in RATIOS:
            for swap in ((False, True) if shape[0] != shape[1] else (False,)):
                tgt = tuple(int(v) for v in np.round(np.multiply(shape[::-1] if swap else shape, r)))
                for f in FILTERS:
                    out.append((f"{shape[0]}x{shape[1]}_r{r}_{'swap_' if swap else ''}{f}", shape, tgt, f))
    for f in FILTERS:
        out.append((f"64x64_cols_only_{f}", (64, 64), (64, 40), f))
        out.append((f"37x23_rows_only_{f}", (37, 23), (50, 23), f))
    return out


def case_input(shape):
    return np.random.RandomState(shape[0] * 1000 + shape[1]).uniform(-1, 2, shape).astype(np.float32)


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    return _sinc(t) * _sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


def _taps(n_in, n_out):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    rows = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - xmin
        k = [_lanczos((x + xmin - center + 0.5) / fs) for x in range(cnt)]
        ww = 0.0
        for w in k:
            ww += w
        rows.append((xmin, np.array([w / ww if ww != 0.0 else w for w in k], np.float64)))
    return rows


def _pass(img, n_out):
    """resample the LAST axis of a float32 image: f64 sums from 0.0 over ascending taps, stored as float32"""
    out = np.empty(img.shape[:-1] + (n_out,), np.float32)
    for xx, (xmin, k) in enumerate(_taps(img.shape[-1], n_out)):
        ss = np.zeros(img.shape[:-1], np.float64)
        for i, w in enumerate(k):
            ss = ss + img[..., xmin + i].astype(np.float64) * w
        out[..., xx] = ss.astype(np.float32)
    return out


def _nearest_index(n_in, n_out):
    a0 = n_in / n_out
    xo = 0.5 * a0
    idx = []
    for _ in range(n_out):
        idx.append(int(xo))
        xo += a0
    return np.array(idx)


def resize(x, out_shape, resample):
    """PIL.Image.fromarray(x float32).resize(out_shape[::-1], resample) as an array; out_shape (rows, cols)"""
    x = np.asarray(x, np.float32)
    oh, ow = out_shape
    if resample == "nearest":
        return x[_nearest_index(x.shape[0], oh)][:, _nearest_index(x.shape[1], ow)]
    if ow != x.shape[1]:
        x = _pass(x, ow)
    if oh != x.shape[0]:
        x = _pass(x.T, oh).T
    return np.ascontiguousarray(x)

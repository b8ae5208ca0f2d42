"""The convolution of include/tmat.h:tmat_conv2d / tmat_conv2d_roi as written, in float64 numpy -- the INDEPENDENT reference of
tests/test_conv_ref.py and tests/test_gpu_conv_shapes.py.  It shares no code and no summation order with oracle/unet_exact.c or the HIP
kernel: it restates the Keras layers of the reference's models.py:110-166 and build_ResNet50_TL in their fused inference form,

    out[n, y, x, o] = act_out( scale[o] * sum_{ky, kx, c} act_in(X)[n, y s + ky - p, x s + kx - p, c] * w[ky, kx, c, o] + shift[o]
                               + resid[n, y >> rs, x >> rs, o] ),

  * X = x, or UpSampling2D(2)(x) (nearest) for up = 1;
  * Conv2D(ksize, padding="same"): zero padding, p = 1 for ksize 3 and 0 for ksize 1 (stride 1: TF SAME pads (k - 1) / 2 on both sides);
  * Conv2D(1, strides=2, padding="same") on even sizes: TF SAME pads nothing, the output samples the EVEN indices;
  * scale / shift: the folded BatchNormalization and bias (scale None: plain bias);
  * resid: add([x, residual]); rs = 1 is the residual hoisted below the UpSampling2D(2): pixel (y, x) adds resid[y >> 1, x >> 1].

No torch, no oracle.  The sums run through numpy's float64 matmul: its own rounding (about K 2^-53 of `mag`) is nine orders of magnitude
below the float32 bound derived in `bound`.
"""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of IEEE binary32


def gamma(n, u=U32):
    """Higham's gamma_n = n u / (1 - n u): n successive roundings change a value by at most this much, relatively"""
    return n * u / (1.0 - n * u)


def ref64(x, w, ksize, stride, up, relu_in, scale, shift, resid, rs, relu_out, mutation=None):
    """-> (v, mag), both float64 (n, Ho, Wo, cout): the convolution above, and the same sum over absolute values,
    mag = |scale| sum |X| |w| + |shift| + |resid| -- what every rounding error of a float32 evaluation is relative to.
    x (n, h, w, cin); w (ksize, ksize, cin, cout); resid (n, Ho >> rs, Wo >> rs, cout) or None.

    `mutation` makes a deliberately WRONG reference (tests/test_conv_ref.py checks that the bound tells each from the right one):
    "right tap wraps": the right neighbour of a row's last pixel is the next row's first pixel (what a linear index x + 1 reads) instead
    of the zero padding; "resid shift": the residual is read at (y >> rs + 1, x >> rs + 1); "odd samples": the stride-2 convolution samples
    the odd indices."""
    assert ksize in (1, 3) and stride in (1, 2) and not (ksize == 3 and stride == 2) and mutation in (None, "right tap wraps", "resid shift", "odd samples")
    X = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    assert X.ndim == 4 and w.shape[:3] == (ksize, ksize, X.shape[-1])
    if relu_in:
        X = np.maximum(X, 0.0)
    if up:
        X = X.repeat(2, axis=1).repeat(2, axis=2)
    n, H, W, cin = X.shape
    cout = w.shape[-1]
    assert H % stride == 0 and W % stride == 0
    Ho, Wo = H // stride, W // stride
    p = (ksize - 1) // 2
    Xp = np.zeros((n, H + 2 * p, W + 2 * p, cin))
    Xp[:, p:p + H, p:p + W] = X
    if mutation == "right tap wraps" and p:
        Xp[:, p:p + H - 1, p + W] = X[:, 1:, 0]
        Xp[:, p + H - 1, p + W] = np.concatenate([X[1:, 0, 0], np.zeros((1, cin))])
    first = 1 if mutation == "odd samples" and stride == 2 else 0
    acc = np.zeros((n, Ho, Wo, cout))
    mag = np.zeros((n, Ho, Wo, cout))
    for ky in range(ksize):
        for kx in range(ksize):
            win = Xp[:, ky + first:ky + H:stride, kx + first:kx + W:stride]
            acc += win @ w[ky, kx]
            mag += np.abs(win) @ np.abs(w[ky, kx])
    sc = np.ones(cout) if scale is None else np.asarray(scale, np.float64)
    sh = np.asarray(shift, np.float64)
    v = acc * sc + sh
    mag = mag * np.abs(sc) + np.abs(sh)
    if resid is not None:
        r = np.asarray(resid, np.float64)
        assert r.shape == (n, Ho >> rs, Wo >> rs, cout)
        s = rs + 1 if mutation == "resid shift" else rs
        r = r[:, np.arange(Ho) >> s][:, :, np.arange(Wo) >> s]
        v = v + r
        mag = mag + np.abs(r)
    if relu_out:
        v = np.maximum(v, 0.0)      # 1-Lipschitz: the bound on v holds for max(v, 0)
    return v, mag


def bound(mag, ksize, cin, subpixel=False):
    """|float32 result - v| <= this, for ANY order of the K = ksize^2 cin fused multiply-adds: a chain of K single-rounding FMAs from +0
    is off by at most gamma_K sum |x| |w| (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 -- any order), and the epilogue's
    one FMA (scale, shift) and one add (residual) each round once more: gamma_(K + 2) mag.  The sub-pixel form multiplies weights that
    are float32 sums of up to four of the nine taps (three more roundings; its chain is the shorter 4 cin): gamma_(K + 5) mag against the
    3x3 convolution of the upsampled input as written."""
    K = ksize * ksize * cin
    return gamma(K + (5 if subpixel else 2)) * mag


def round_f16(a):
    """float32 array rounded to IEEE binary16 (nearest even) and widened again"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)

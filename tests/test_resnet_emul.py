"""CPU: tests/helpers/resnet_emul.py, the float64 evaluation of the invasion-depth classifier that the f16 GPU tests
(tests/test_gpu_invdepth_f16.py) measure against -- and the two facts about f16 operands that shape those tests:

  * f16 operands move the ensemble's probabilities less than bf16 operands do (the opt-in mode is f16, not bf16);
  * the f16 network is CHAOTIC in the accumulation order: two correct evaluations of the same f16-operand network that differ only
    in how they sum (exactly / in f32) differ at the trunk output by far more than the f32 path's own error, because a 1e-7
    difference in an accumulator flips the f16 rounding of a few next-layer operands by a whole f16 ulp.  So no CPU emulation pins a
    multi-layer f16 result tightly; the GPU tests pin ONE convolution tightly and compare deviation SIZES end to end.  Do not
    "tighten" the end-to-end GPU gate to an element-wise comparison with this helper: it would fail for every correct kernel.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

SMALL = "conv3_block1_out"      # stem, pool, stage 2, one strided block with its projection shortcut: every kernel kind of the model


def _small_inputs(n=3, seed=2):
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 255, (n, 64, 64, 1)) - np.array([103.939, 116.779, 123.68])).astype(np.float32)


def test_exact_mode_agrees_with_the_f32_oracle_at_f32_accumulation_level():
    import resnet_emul as em
    from oracle import resnet as orr
    from tmat_amd import inv_depth
    w = inv_depth.synth_resnet_weights(3, SMALL)
    x = _small_inputs()
    ref = orr.forward(w, x).astype(np.float64)
    got = em.forward(w, x, "exact")
    # f32 chains of K <= 1152 products of O(1) activations: relative error ~1e-6 per layer, a dozen layers, sigmoid slope <= 1/4
    assert np.abs(got - ref).max() < 2e-5, np.abs(got - ref).max()
    assert 0.01 < got.min() and got.max() < 0.99
    # and the single-convolution form against oracle.unet._conv (3x3 with residual and ReLU; 1x1 stride 2)
    from oracle import unet as ou
    rs = np.random.RandomState(0)
    for k, st, cin, cout in ((3, 1, 64, 64), (1, 2, 64, 128)):
        xx = rs.normal(0, 1, (2, 16, 16, cin)).astype(np.float32)
        ww = rs.normal(0, 1, (k, k, cin, cout)).astype(np.float32)
        sc, sh = rs.uniform(0.5, 1.5, cout).astype(np.float32), rs.normal(0, 1, cout).astype(np.float32)
        rr = rs.normal(0, 1, (2, 16 // st, 16 // st, cout)).astype(np.float32)
        o = ou._conv(xx, ww, k, st, 0, 0, sc, sh, rr, 0, 1).astype(np.float64)
        e = em.conv(xx, ww, k, st, sc, sh, rr, False, True, "exact")
        assert e.shape == o.shape
        assert np.abs(o - e).max() <= 64 * 2.0 ** -24 * np.abs(e).max(), (k, st, np.abs(o - e).max())


def test_f16_mode_on_f16_exact_operands_equals_exact_mode():
    import resnet_emul as em
    rs = np.random.RandomState(1)
    x = rs.normal(0, 1, (2, 8, 8, 32)).astype(np.float16).astype(np.float32)
    w = rs.normal(0, 1, (3, 3, 32, 64)).astype(np.float16).astype(np.float32)
    sc, sh = rs.uniform(0.5, 1.5, 64).astype(np.float32), rs.normal(0, 1, 64).astype(np.float32)
    a = em.conv(x, w, 3, 1, sc, sh, None, False, False, "exact")
    b = em.conv(x, w, 3, 1, sc, sh, None, False, False, "f16")
    assert np.array_equal(a, b)
    x2 = (x + np.float32(1e-4)).astype(np.float32)                     # no longer f16 values: now the two modes differ
    assert not np.array_equal(em.conv(x2, w, 3, 1, sc, sh, None, False, False, "exact"), em.conv(x2, w, 3, 1, sc, sh, None, False, False, "f16"))


def test_rounding_saturation_and_the_subnormal_switch():
    import resnet_emul as em
    v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 65504.0, 65519.0, 65520.0, 1e9, -1e9, np.float32(2.0 ** -14), 2.0 ** -15,
                  3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -26, -(2.0 ** -20)], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -9, 2048.0, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -15,
                     2.0 ** -23, 0.0, 0.0, -(2.0 ** -20)], np.float32)                      # ties to even; beyond the range: +-65504, never inf
    got = em.quant_np(v, "f16")
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(em.round_f16_np(v), want)                    # the torch-free form the GPU tests pre-round with
    r = np.random.RandomState(3).normal(0, 1, 100000).astype(np.float32) * np.float32(2.0) ** np.random.RandomState(4).randint(-30, 20, 100000).astype(np.float32)
    assert np.array_equal(em.round_f16_np(r), em.quant_np(r, "f16")) and np.array_equal(em.round_f16_np(r, True), em.quant_np(r, "f16", True))
    flushed = em.quant_np(v, "f16", flush_subnormals=True)
    sub = np.abs(want) < 2.0 ** -14
    assert np.array_equal(flushed[~sub], want[~sub]) and not flushed[sub].any() and sub.sum() == 5
    # through a convolution: one input channel, one weight; a subnormal-f16 weight contributes unless flushed; a huge input enters as 65504
    x = np.zeros((1, 2, 2, 32), np.float32)
    x[0, 0, 0, 0] = 1e9
    x[0, 1, 1, 0] = 1024.0
    w = np.zeros((1, 1, 32, 64), np.float32)
    w[0, 0, 0, 0] = 2.0 ** -16
    z = np.zeros(64, np.float32)
    keep = em.conv(x, w, 1, 1, None, z, None, False, False, "f16")
    flush = em.conv(x, w, 1, 1, None, z, None, False, False, "f16", flush_subnormals=True)
    assert keep[0, 0, 0, 0] == 65504.0 * 2.0 ** -16 and keep[0, 1, 1, 0] == 2.0 ** -6 and np.isfinite(keep).all()
    assert not flush.any()


@pytest.fixture(scope="module")
def reduced_sample():
    """two members of the configured model (conv4_block6_out, 256 x 256) on 4 slices: exact, f16 and bf16 operands (exact accumulation),
    and f32 accumulation of the exact and of the f16 operands, trunk outputs kept"""
    import resnet_emul as em
    from oracle import resnet as orr
    from tmat_amd import inv_depth, synth
    x = orr.prep_inv_depth_imgs(synth.synth_stack(20, 4, 300, 360, n_vessels=8), 256)
    out = []
    for seed in (0, 1):
        w = inv_depth.synth_resnet_weights(seed)
        out.append({k: em.forward(w, x, operands=o, acc=a, return_feat=True)
                    for k, (o, a) in {"exact": ("exact", "f64"), "f16": ("f16", "f64"), "bf16": ("bf16", "f64"), "exact32": ("exact", "f32"),
                                      "f16_32": ("f16", "f32")}.items()})
    return out


def test_f16_operands_move_the_probabilities_less_than_bf16(reduced_sample):
    p = {k: np.stack([m[k][0] for m in reduced_sample], axis=1) for k in ("exact", "f16", "bf16")}
    d16 = np.abs(p["f16"] - p["exact"])
    db = np.abs(p["bf16"] - p["exact"])
    print(f"member |dp|: f16 {d16.max():.2e}, bf16 {db.max():.2e}; mean |dp|: f16 {np.abs(p['f16'].mean(1) - p['exact'].mean(1)).max():.2e}, "
          f"bf16 {np.abs(p['bf16'].mean(1) - p['exact'].mean(1)).max():.2e}")
    # bf16 keeps 8 significant bits, f16 11: a factor of 8 in operand error; asserted loosely (2) on this small sample
    assert 2 * d16.max() < db.max()
    assert 2 * np.abs(p["f16"].mean(1) - p["exact"].mean(1)).max() < np.abs(p["bf16"].mean(1) - p["exact"].mean(1)).max()
    assert d16.max() < 1e-2          # and f16 stays a small perturbation of the probabilities (measured on 32 slices x 3 members: <= 1.6e-3)


def test_the_f16_network_is_chaotic_in_the_accumulation_order(reduced_sample):
    for m in reduced_sample:
        f = {k: v[1] for k, v in m.items()}
        d32 = np.abs(f["exact32"] - f["exact"]).max()                    # the f32 path's own error at the trunk output
        order = np.abs(f["f16_32"] - f["f16"])                           # two accumulation orders of ONE f16-operand network
        quant = np.abs(f["f16"] - f["exact"])
        frac = float((order > 4 * d32).mean())
        rms_o, rms_q = float(np.sqrt((order ** 2).mean())), float(np.sqrt((quant ** 2).mean()))
        print(f"trunk output: f32 error {d32:.2e}; f16 orders differ by > 4x that on {frac:.0%} of the elements, rms {rms_o:.2e} "
              f"(quantisation itself rms {rms_q:.2e})")
        assert frac > 0.25 and rms_o > 20 * d32 / 4          # measured: 76 %, rms 3.5e-3 against d32 ~ 1e-5
        assert rms_o > 0.2 * rms_q                           # the order effect is of the SIZE of the quantisation effect, not a correction to it
        # ... and it averages out at the output: the probabilities of the two orders are much closer than either is to the exact ones
        dp_order = np.abs(m["f16_32"][0] - m["f16"][0]).max()
        dp_quant = np.abs(m["f16"][0] - m["exact"][0]).max()
        assert dp_order < 0.5 * dp_quant, (dp_order, dp_quant)

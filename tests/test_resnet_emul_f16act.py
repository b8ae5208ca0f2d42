"""CPU: tests/helpers/resnet_emul_f16act.py, the float64 evaluation of the f16act contract (TMAT_RESNET_PRECISION_F16ACT, include/tmat.h)
that tests/test_gpu_invdepth_f16act.py measures the GPU's deviation size against.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

SMALL = "conv3_block1_out"      # stem, pool, stage 2, one strided block with its projection shortcut


def test_f16act_evaluation_on_the_small_trunk():
    import resnet_emul as em
    import resnet_emul_f16act as ea
    from tmat_amd import inv_depth
    w = inv_depth.synth_resnet_weights(3, SMALL)
    rs = np.random.RandomState(2)
    x = (rs.uniform(0, 255, (3, 64, 64, 1)) - np.array([103.939, 116.779, 123.68])).astype(np.float32)
    p16, a16 = ea.forward(w, x, store="f32", return_acts=True)
    pa, aa = ea.forward(w, x, store="f16", return_acts=True)
    # the restated forward with the f32 store IS resnet_emul's f16 evaluation
    assert np.array_equal(p16, em.forward(w, x, operands="f16"))
    # every stored activation is an f16 value
    assert set(aa) == set(a16) and len(aa) == 2 + (1 + 3 * 3) + 4      # stem, pool, stage 2 (c0 + 3 blocks of 3 convolutions), conv3_block1 (c0 + 3)
    for name, v in aa.items():
        assert np.array_equal(em.round_f16_np(v.astype(np.float32)).astype(np.float64), v), name
    # up to the first block's c2 output no residual is involved: the f16 mode rounds the same f32 values when it loads them, so the
    # f16act activation is the rounded f16-mode activation exactly ...
    for name in ("conv1", "pool1", "s2b1.c0", "s2b1.c1", "s2b1.c2"):
        assert np.array_equal(aa[name], em.round_f16_np(a16[name].astype(np.float32)).astype(np.float64)), name
    # ... and behind the first residual add (an f16 shortcut instead of an f32 one) it is not: the mode is a third set of numbers
    assert not np.array_equal(aa["s2b1.c3"], em.round_f16_np(a16["s2b1.c3"].astype(np.float32)).astype(np.float64))
    assert not np.array_equal(pa, p16)
    pe = em.forward(w, x, operands="exact")
    assert np.abs(pa - pe).max() < 1e-2 and np.abs(p16 - pe).max() < 1e-2


def test_f16act_moves_the_ensemble_as_much_as_f16():
    """the inputs of the GPU deviation test (stack seeds 20-23, z = 8, 300 x 360, members 0-2, size 256): the f16act evaluation's ensemble
    deviation from the exact one is of the f16 evaluation's size -- under twice it.  Measured: member deviations 3.88e-4, 1.64e-3,
    3.6e-10 and mean 4.19e-4 for f16act; no saturation (largest activation 46.6); nearest exact mean 9.7e-4 from the threshold, beyond
    the GPU test's exclusion radius 2 x 4.19e-4: no slice is excluded from its label check and no label flips.
    (96 float64 forwards of the whole trunk per mode, three modes, in one CPU-only child process: the long test of this file.)"""
    import resnet_emul_f16act as ea
    E = ea.in_child("ensemble_probs", seeds=[0, 1, 2], stack_seeds=[20, 21, 22, 23], z=8, H=300, W=360, size=256, n_vessels=8, modes=("exact", "f16", "f16act"))
    e64, e16, eact = E["exact"], E["f16"], E["f16act"]
    assert e64.shape == e16.shape == eact.shape == (32, 3)
    dev_act, dev_16 = np.abs(eact - e64).max(axis=0), np.abs(e16 - e64).max(axis=0)
    mean_act, mean_16 = np.abs(eact.mean(1) - e64.mean(1)).max(), np.abs(e16.mean(1) - e64.mean(1)).max()
    margin = np.abs(e64.mean(1) - 0.5).min()
    flips = int(((eact.mean(1) > 0.5) != (e64.mean(1) > 0.5)).sum())
    print(f"member max|E16act-E64| {dev_act} vs max|E16-E64| {dev_16}; mean {mean_act:.3e} vs {mean_16:.3e}; nearest exact mean to 0.5: {margin:.3e}; "
          f"label flips {flips}; largest activation {E['max_act']:.1f}", flush=True)
    assert np.abs(eact - e64).max() < 2 * np.abs(e16 - e64).max()
    assert mean_act < 2 * mean_16
    assert E["max_act"] < 65504 and flips == 0 and margin > 2 * mean_act

"""GPU: the opt-in f16 matrix-core mode of the invasion-depth classifier (tmat_resnet_set_precision, include/tmat.h).

The mode is NOT bit-exact with oracle/resnet.py, and a multi-layer f16 network is chaotic in its accumulation order
(tests/test_resnet_emul.py), so the checks are:
  1. ONE convolution (tmat_conv2d), tight, against the float64 evaluation of the contract on the same operands;
  2. determinism, and switching back to f32 restores the bit-exact path;
  3. end to end: the SIZE of the deviation from the exact evaluation, against the size the float64 evaluation of the contract shows;
  4. the CLI's --precision f16.
The float64 evaluations (tests/helpers/resnet_emul.py, torch) run in CPU-only child processes: this process never imports torch.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

pytestmark = pytest.mark.gpu

# Observed on an MI355X with the subnormal case of test 1 (f16-subnormal weights, |w| < 2^-14): v_mfma_f32_32x32x16_f16 multiplies
# subnormal f16 operands as they are (no flush); the float64 references below are evaluated accordingly.
FLUSH_SUBNORMALS = False

# every distinct (ksize, stride, Cin, Cout, spatial size) of ResNet50 up to conv4_block6_out at 256 x 256, the K = 192 im2col stem first
TRUNK_SHAPES = [(1, 1, 192, 64, 128),
                (1, 1, 64, 256, 64), (1, 1, 64, 64, 64), (3, 1, 64, 64, 64), (1, 1, 256, 64, 64),
                (1, 2, 256, 512, 64), (1, 2, 256, 128, 64), (3, 1, 128, 128, 32), (1, 1, 128, 512, 32), (1, 1, 512, 128, 32),
                (1, 2, 512, 1024, 32), (1, 2, 512, 256, 32), (3, 1, 256, 256, 16), (1, 1, 256, 1024, 16), (1, 1, 1024, 256, 16)]


def _specs():
    specs = []
    for i, (k, st, cin, cout, size) in enumerate(TRUNK_SHAPES):
        for full in (0, 1):             # without / with residual + ReLU
            specs.append(dict(ksize=k, stride=st, cin=cin, cout=cout, size=size, n=2 + (i + full) % 2, resid=bool(full), relu_in=False, relu_out=bool(full),
                              seed=100 + 2 * i + full, kind="plain"))
    specs.append(dict(ksize=3, stride=1, cin=64, cout=128, size=16, n=2, resid=False, relu_in=True, relu_out=False, seed=200, kind="plain"))      # the load-side ReLU form
    specs.append(dict(ksize=1, stride=1, cin=64, cout=64, size=16, n=2, resid=True, relu_in=True, relu_out=True, seed=201, kind="plain"))
    specs.append(dict(ksize=1, stride=1, cin=256, cout=128, size=16, n=2, resid=False, relu_in=False, relu_out=False, seed=202, kind="subnormal"))
    specs.append(dict(ksize=3, stride=1, cin=64, cout=64, size=16, n=2, resid=False, relu_in=False, relu_out=False, seed=203, kind="huge"))
    return specs


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def test_one_convolution_tight(plain, tmp_path):
    """R = float64 convolution of the f16-rounded operands + epilogue; O = oracle.unet._conv fed the PRE-ROUNDED operands (the same
    contract in another f32 summation order, on the CPU).  Gate: max|GPU(prec 3) - R| <= 4 max|O - R|.  Why 4: two f32 summation orders
    of the same exact products each lie about |O - R| from the exact sum (triangle bound 2), doubled because the matrix pipe's summation
    of one instruction's 16 products is not documented to be a sequential f32 chain.  The gate separates a correct kernel from one that
    truncates instead of rounding, leaves an operand unrounded or misplaces a plane (all of size Q = max|R - float64 convolution of the
    UNROUNDED operands|) when 4 max|O - R| <= Q / 4, which is asserted too.  prec = 0 of every case equals O-on-unrounded bit for bit
    (that proves the entry point).  Measured ratios max|GPU - R| / max|O - R|: printed, and in DESIGN 7c."""
    import resnet_emul as em
    from oracle import unet as ou
    specs = _specs()
    for i, spec in enumerate(specs):
        c = em.make_conv_case(spec)
        g3 = plain.conv2d(c["x"], c["w"], c["scale"], c["shift"], spec["stride"], c["resid"], spec["relu_in"], spec["relu_out"], prec=3)
        g3b = plain.conv2d(c["x"], c["w"], c["scale"], c["shift"], spec["stride"], c["resid"], spec["relu_in"], spec["relu_out"], prec=3)
        assert np.array_equal(g3.view(np.uint32), g3b.view(np.uint32)), ("f16 convolution differs call to call", spec)
        g0 = plain.conv2d(c["x"], c["w"], c["scale"], c["shift"], spec["stride"], c["resid"], spec["relu_in"], spec["relu_out"], prec=0)
        o0 = ou._conv(c["x"], c["w"], spec["ksize"], spec["stride"], 0, int(spec["relu_in"]), c["scale"], c["shift"], c["resid"], 0, int(spec["relu_out"]))
        assert np.array_equal(g0.view(np.uint32), o0.view(np.uint32)), ("tmat_conv2d(prec 0) differs from oracle.unet._conv", spec)
        xq, wq = em.prerounded(spec, FLUSH_SUBNORMALS)
        oq = ou._conv(xq, wq, spec["ksize"], spec["stride"], 0, 0, c["scale"], c["shift"], c["resid"], 0, int(spec["relu_out"]))
        np.save(tmp_path / f"gpu_{i}.npy", g3)
        np.save(tmp_path / f"orc_{i}.npy", oq)
    figs = em.in_child("conv_case_figures", specs=specs, outputs_dir=str(tmp_path), flush_subnormals=FLUSH_SUBNORMALS)
    lines, bad = [], []
    for spec, f in zip(specs, figs):
        ratio = f["gpu_err"] / f["orc_err"] if f["orc_err"] > 0 else float("inf") if f["gpu_err"] > 0 else 0.0
        line = (f"k{spec['ksize']} s{spec['stride']} {spec['cin']}->{spec['cout']} @{spec['size']} n{spec['n']} resid={int(spec['resid'])} relu={int(spec['relu_in'])}{int(spec['relu_out'])} "
                f"{spec['kind']}: |GPU-R| {f['gpu_err']:.3e} |O-R| {f['orc_err']:.3e} ratio {ratio:.2f} Q {f['Q']:.3e} Q/|O-R| {f['Q'] / max(f['orc_err'], 1e-300):.0f} max|R| {f['rmax']:.3g}")
        if spec["kind"] == "subnormal":
            line += f" | subnormal weights: |GPU-R(kept)| {f['gpu_err_keep']:.3e} |GPU-R(flushed)| {f['gpu_err_flush']:.3e} |R(kept)-R(flushed)| {f['keep_vs_flush']:.3e}"
        lines.append(line)
        print(line, flush=True)
        if not f["finite"] or not f["gpu_err"] <= 4 * f["orc_err"] or not 4 * f["orc_err"] <= f["Q"] / 4:
            bad.append(line)
    assert not bad, "\n".join(["cases outside the gate:"] + bad + ["all cases:"] + lines)


@pytest.fixture(scope="module")
def members():
    from tmat_amd import inv_depth
    return [inv_depth.synth_resnet_weights(s) for s in range(3)]


def test_determinism_and_switching(plain, members, handle):
    import ctypes as C
    import os
    import subprocess
    from oracle import resnet as orr
    from tmat_amd import _lib, inv_depth, synth
    ws = members[:2]
    stacks = [synth.synth_stack(30 + i, 2, 300, 360, n_vessels=8) for i in range(2)]
    ens = inv_depth.InvDepthEnsemble(plain, ws)
    f32_before = ens.predict_stacks(stacks)
    ens.set_precision("f16")
    try:
        a = ens.predict_stacks(stacks)
        b = ens.predict_stacks(stacks)
        single = [ens.predict_stack(s) for s in stacks]
        for x, y, z in zip(a, b, single):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "f16 results differ call to call"
            assert np.array_equal(x.view(np.uint32), z.view(np.uint32)), "predict_stack and predict_stacks differ in f16 mode"
        assert not np.array_equal(a[0], f32_before[0]), "f16 mode computed the f32 result: the switch did nothing"
        assert np.abs(np.concatenate(a) - np.concatenate(f32_before)).max() < 2e-2
        # a model loaded while the mode is on gets its f16 weights at load
        ens2 = inv_depth.InvDepthEnsemble(plain, ws[:1])
        assert np.array_equal(ens2.predict_stack(stacks[0])[:, 0].view(np.uint32), a[0][:, 0].view(np.uint32))
        # tmat_resnet_predict follows the mode as well
        ox = orr.prep_inv_depth_imgs(stacks[0], 256)
        assert np.array_equal(ens.predict(ox, 0).view(np.uint32), a[0][:, 0].view(np.uint32))
    finally:
        ens.set_precision("f32")
    back = ens.predict_stacks(stacks)
    fresh_h = _lib.Handle(None, 0)
    try:
        fresh = inv_depth.InvDepthEnsemble(fresh_h, ws).predict_stacks(stacks)
    finally:
        fresh_h.close()
    for s, x, y, z in zip(stacks, back, fresh, f32_before):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
        ox = orr.prep_inv_depth_imgs(s, 256)
        ref = np.stack([orr.forward(w, ox) for w in ws], axis=1)
        assert np.array_equal(x.view(np.uint32), ref.view(np.uint32)), "f16 -> f32 does not restore the bit-exact path"
    # bad modes are refused, with a message, and leave the mode alone
    assert _lib.lib().tmat_resnet_set_precision(plain.raw, 2) != 0 and b"tmat_resnet_set_precision" in _lib.lib().tmat_last_error()
    with pytest.raises(ValueError):
        ens.set_precision("bf16")
    # independent of tmat_set_precision, on a model handle: the UNet's mode is untouched, its output stays bit-exact
    from oracle import unet as ou
    from tmat_amd import synth as sy
    x = np.random.RandomState(0).uniform(0, 1, (1, 320, 320)).astype(np.float32)
    ref = ou.forward_exact(sy.synth_weights(0), x)
    handle.resnet_set_precision("f16")
    try:
        assert np.array_equal(handle.unet_predict(x).view(np.uint32), ref.view(np.uint32))
        handle.set_precision("bf16x3")
        handle.set_precision("f32")
        e3 = inv_depth.InvDepthEnsemble(handle, ws[:1])
        assert np.array_equal(e3.predict_stack(stacks[0])[:, 0].view(np.uint32), a[0][:, 0].view(np.uint32)), "tmat_set_precision changed the classifier's mode"
    finally:
        handle.resnet_set_precision("f32")
    # the environment variable: f16 selects the mode at creation, an unknown value fails creation (child processes: the variable is read at creation)
    repo = Path(__file__).resolve().parents[1]
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from tmat_amd import _lib\n"
            "try:\n"
            "    h = _lib.Handle(None, 0)\n"
            "except _lib.TmatError as e:\n"
            "    print('REFUSED', e); sys.exit(3)\n"
            "import numpy as np\n"
            "from tmat_amd import inv_depth, synth\n"
            "ens = inv_depth.InvDepthEnsemble(h, [inv_depth.synth_resnet_weights(0)])\n"
            "np.save(sys.argv[1], ens.predict_stack(synth.synth_stack(30, 2, 300, 360, n_vessels=8)))\n"
            "h.close()\n") % (str(repo), str(repo / "tissue-model-analysis-tools_amd"))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, "-c", code, f"{d}/p.npy"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TMAT_INV_DEPTH_PRECISION="f16"))
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(np.load(f"{d}/p.npy")[:, 0].view(np.uint32), a[0][:, 0].view(np.uint32)), "TMAT_INV_DEPTH_PRECISION=f16 did not select the mode"
        r = subprocess.run([sys.executable, "-c", code, f"{d}/q.npy"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TMAT_INV_DEPTH_PRECISION="bf16"))
        assert r.returncode == 3 and "TMAT_INV_DEPTH_PRECISION" in r.stdout, r.stdout + r.stderr


def test_end_to_end_deviation_sizes(plain, members):
    """32 slices x 3 members.  E64 / E16 = the float64 evaluation's probabilities (exact / f16 operands).  GPU and E16 are two
    accumulation orders of one chaotic process (tests/test_resnet_emul.py), so the claim is equal deviation SIZE from E64:
    per member max|GPU - E64| <= 2 max|E16 - E64|, the same for the ensemble mean (two such orders were measured 0.07-0.15 of that
    deviation apart, which puts the GPU's deviation at 0.85-1.15 of E16's; 2 is headroom against the small sample).  Labels equal
    those of E64 on every slice whose exact mean is farther from the threshold than 2 max|mean E16 - mean E64|; cap: NO slice excluded.
    max|GPU - E16| and the GPU-f16-vs-GPU-f32 figures are recorded (printed), not gated."""
    import resnet_emul as em
    from tmat_amd import inv_depth, synth
    stack_seeds = [20, 21, 22, 23]
    stacks = [synth.synth_stack(s, 8, 300, 360, n_vessels=8) for s in stack_seeds]
    ens = inv_depth.InvDepthEnsemble(plain, members)
    g32 = np.concatenate(ens.predict_stacks(stacks)).astype(np.float64)
    ens.set_precision("f16")
    try:
        g16_f32 = np.concatenate(ens.predict_stacks(stacks))
    finally:
        ens.set_precision("f32")
    g16 = g16_f32.astype(np.float64)
    E = em.in_child("ensemble_probs", seeds=[0, 1, 2], stack_seeds=stack_seeds, z=8, H=300, W=360, size=256, n_vessels=8, flush_subnormals=FLUSH_SUBNORMALS)
    e64, e16 = E["exact"], E["f16"]
    assert g16.shape == e64.shape == e16.shape == (32, 3)
    dev_gpu = np.abs(g16 - e64).max(axis=0)
    dev_e16 = np.abs(e16 - e64).max(axis=0)
    mean_gpu = np.abs(g16.mean(1) - e64.mean(1)).max()
    mean_e16 = np.abs(e16.mean(1) - e64.mean(1)).max()
    margin = np.abs(e64.mean(1) - 0.5)
    excluded = int((margin <= 2 * mean_e16).sum())
    lab_gpu = np.array([lab for _, lab in inv_depth.ensemble_predictions(g16_f32, 0.5)])
    lab_f32 = np.array([lab for _, lab in inv_depth.ensemble_predictions(g32.astype(np.float32), 0.5)])
    r16 = np.array([p for p, _ in inv_depth.ensemble_predictions(g16_f32, 0.5)], np.float64)
    r32 = np.array([p for p, _ in inv_depth.ensemble_predictions(g32.astype(np.float32), 0.5)], np.float64)
    lab_e64 = (e64.mean(1) > 0.5).astype(int)
    msg = (f"per member max|GPU-E64| {dev_gpu} vs max|E16-E64| {dev_e16} (ratio {dev_gpu / dev_e16}); mean: {mean_gpu:.3e} vs {mean_e16:.3e} (ratio {mean_gpu / mean_e16:.2f}); "
           f"max|GPU-E16| {np.abs(g16 - e16).max():.3e}; nearest exact mean to 0.5: {margin.min():.3e}, slices excluded from the label check: {excluded}; "
           f"GPU f16 vs GPU f32: member {np.abs(g16 - g32).max():.3e}, mean {np.abs(g16.mean(1) - g32.mean(1)).max():.3e}, rounded differ on {int((r16 != r32).sum())} of 32 "
           f"(by <= {np.abs(r16 - r32).max():.1e}), label flips {int((lab_gpu != lab_f32).sum())}; f32 GPU vs E64: {np.abs(g32 - e64).max():.3e}; labels: {int(lab_e64.sum())} ones")
    print(msg, flush=True)
    assert np.abs(g32 - e64).max() < 2e-5, msg                     # the exact evaluation and the bit-exact f32 path agree: E64 is the right yardstick
    assert (dev_gpu <= 2 * dev_e16).all(), msg
    assert mean_gpu <= 2 * mean_e16, msg
    assert excluded == 0, msg
    assert np.array_equal(lab_gpu, lab_e64), msg


def test_script_precision_f16(tmp_path):
    """compute_inv_depth.py --precision f16 on two small stacks: runs, same CSV format, and its probabilities deviate from the f32 run's
    by no more than the size the float64 evaluation of the f16 contract shows on the same slices and members (gate as in the end-to-end
    test, on the script's own numbers: |mean f16 - mean f32| <= 2 max|mean E16 - mean E64|, plus 1e-4 for the two 4-decimal roundings)"""
    import csv
    import os
    import subprocess
    import resnet_emul as em
    from PIL import Image
    from tmat_amd import inv_depth, synth
    repo = Path(__file__).resolve().parents[1]
    ind = tmp_path / "in"
    ind.mkdir()
    seeds = {"gelA": 11, "gelB": 12}
    for k, sd in seeds.items():
        for z, sl in enumerate(synth.synth_stack(sd, 3, 128, 160, n_vessels=6)):
            Image.fromarray(sl).save(ind / f"{k}_z{z}.tif")
    script = repo / "tissue-model-analysis-tools_amd" / "scripts" / "compute_inv_depth.py"
    res = {}
    for mode in ("f32", "f16"):
        outd = tmp_path / f"out_{mode}"
        r = subprocess.run([sys.executable, str(script), str(ind), str(outd), "--precision", mode], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1"))
        assert r.returncode == 0, r.stdout + r.stderr
        rows = list(csv.reader(open(outd / "invasion_depth_predictions.csv")))
        assert rows[0] == ["Z Slice ID", "Invasion Probability", "Invasion Prediction (0=no 1=yes)"]
        res[mode] = {r_[0]: (float(r_[1]), int(r_[2])) for r_ in rows[1:]}
    r = subprocess.run([sys.executable, str(script), str(ind), str(tmp_path / "o3"), "--precision", "bf16"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1"))
    assert r.returncode == 2 and "--precision" in r.stderr                      # argparse refuses other values
    default = tmp_path / "out_default"
    r = subprocess.run([sys.executable, str(script), str(ind), str(default)], capture_output=True, text=True, timeout=600, env=dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1"))
    assert r.returncode == 0 and open(default / "invasion_depth_predictions.csv").read() == open(tmp_path / "out_f32" / "invasion_depth_predictions.csv").read()
    order = inv_depth.best_model_indices(repo / "tissue-model-analysis-tools_amd" / "model_training" / "best_ensemble", 5, 3)
    keys = sorted(res["f32"])
    assert sorted(res["f16"]) == keys and len(keys) == 6
    e_mean = {}
    for k, sd in seeds.items():
        E = em.in_child("ensemble_probs", seeds=[int(i) for i in order], stack_seeds=[sd], z=3, H=128, W=160, size=256, n_vessels=6, flush_subnormals=FLUSH_SUBNORMALS)
        for z in range(3):
            e_mean[f"{k}_z{z}"] = (E["exact"][z].mean(), E["f16"][z].mean())
    bound = 2 * max(abs(b - a) for a, b in e_mean.values()) + 1e-4
    diff = {k: abs(res["f16"][k][0] - res["f32"][k][0]) for k in keys}
    msg = f"|p f16 - p f32| per slice {diff}; bound {bound:.3e}; f32 {res['f32']}; f16 {res['f16']}"
    print(msg, flush=True)
    assert max(diff.values()) <= bound, msg
    assert any(res["f16"][k][0] != res["f32"][k][0] for k in keys), "the f16 run printed the f32 probabilities: --precision did nothing\n" + msg
    for k in keys:
        if abs(e_mean[k][0] - 0.5) > bound:
            assert res["f16"][k][1] == res["f32"][k][1], msg

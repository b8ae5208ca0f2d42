"""GPU: the opt-in f16act mode of the invasion-depth classifier (TMAT_RESNET_PRECISION_F16ACT, include/tmat.h): the f16
matrix-core mode with every activation tensor stored as IEEE binary16.

The mode keeps the f16 mode's k-step geometry and accumulation order, so -- unlike the f16 mode against a CPU emulation -- it is EXACTLY
testable against the f16 mode on the same GPU: on f16-exact operands an f16act convolution is round_f16(the prec-3 convolution), bit for
bit, and a whole network replays layer by layer.
  1. ONE convolution (tmat_conv2d, prec 4) == round_f16(prec 3), bit for bit, on every layer shape and tile edge case;
  2. the whole network (tmat_resnet_predict in f16act mode) == a host replay of prec-3 convolutions with an f16 rounding per layer;
  3. end to end: the SIZE of the deviation from the exact float64 evaluation, gate and inputs of tests/test_gpu_invdepth_f16.py;
  4. determinism, switching between the three modes, the environment variable, the refused values;
  5. the CLI's --precision f16act.
The float64 evaluations (tests/helpers/resnet_emul_f16act.py, torch) run in CPU-only child processes: this process never imports torch.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

pytestmark = pytest.mark.gpu

# the 15 distinct (ksize, stride, Cin, Cout) of ResNet50 up to conv4_block6_out, the K = 192 im2col stem first (TRUNK_SHAPES of
# tests/test_gpu_invdepth_f16.py without the spatial sizes)
LAYERS = [(1, 1, 192, 64),
          (1, 1, 64, 256), (1, 1, 64, 64), (3, 1, 64, 64), (1, 1, 256, 64),
          (1, 2, 256, 512), (1, 2, 256, 128), (3, 1, 128, 128), (1, 1, 128, 512), (1, 1, 512, 128),
          (1, 2, 512, 1024), (1, 2, 512, 256), (3, 1, 256, 256), (1, 1, 256, 1024), (1, 1, 1024, 256)]


def _specs():
    specs = []
    for i, (k, st, cin, cout) in enumerate(LAYERS):
        for full in (0, 1):             # without / with residual + ReLU
            common = dict(ksize=k, stride=st, cin=cin, cout=cout, resid=bool(full), relu_in=False, relu_out=bool(full), kind="plain")
            specs.append(dict(common, size=16, n=2, seed=300 + 2 * i + full))                # 512 (stride 2: 128) pixels: whole tiles
            # output width 14, 196 pixels: the generic prologue (14 % 8 != 0), two 128-pixel tiles of which the last ends past M
            specs.append(dict(common, size=14 * st, n=1, seed=400 + 2 * i + full))
    specs.append(dict(ksize=3, stride=1, cin=64, cout=128, size=8, n=1, resid=True, relu_in=False, relu_out=True, seed=500, kind="plain"))   # 64 pixels: less than a tile
    specs.append(dict(ksize=1, stride=1, cin=64, cout=64, size=8, n=1, resid=False, relu_in=False, relu_out=False, seed=501, kind="plain"))
    specs.append(dict(ksize=3, stride=1, cin=64, cout=64, size=16, n=2, resid=False, relu_in=False, relu_out=False, seed=203, kind="huge"))  # the existing "huge" case
    return specs


@pytest.fixture(scope="module")
def plain():
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_one_convolution_exact(plain, tmp_path):
    """conv2d(prec 4) == round_f16(conv2d(prec 3)) bit for bit on operands rounded to f16 beforehand: the same instruction, operand
    values, positions and order give the same accumulator, the epilogue is the same f32 code, and prec 4 then rounds once.  Every case
    (they all differ from the existing f16 test's in their spatial size) also takes that test's gate on the prec-3 output of the RAW
    case, max|GPU - R| <= 4 max|O - R| (resnet_emul.conv_case_figures), so that a mismatch can be attributed to one of the two forms."""
    import resnet_emul as em
    from oracle import unet as ou
    specs = _specs()
    mismatches = []
    for i, spec in enumerate(specs):
        c = em.make_conv_case(spec)
        xq, wq = em.round_f16_np(c["x"]), em.round_f16_np(c["w"])
        rq = None if c["resid"] is None else em.round_f16_np(c["resid"])

        def run(prec, x=xq, w=wq, r=rq, scale=c["scale"], shift=c["shift"]):
            return plain.conv2d(x, w, scale, shift, spec["stride"], r, False, spec["relu_out"], prec=prec)
        g4, g4b, g3 = run(4), run(4), run(3)
        want = em.round_f16_np(g3)
        assert np.array_equal(_bits(g4), _bits(g4b)), ("f16act convolution differs call to call", spec)
        assert np.array_equal(_bits(em.round_f16_np(g4)), _bits(g4)) and np.isfinite(g4).all(), ("prec 4 returned values that are not f16", spec)
        if not np.array_equal(_bits(g4), _bits(want)):
            d = g4 != want
            mismatches.append(f"{spec}: {int(d.sum())} of {d.size} differ, max |diff| {np.abs(g4.astype(np.float64) - want).max():.3e}, first at {tuple(np.argwhere(d)[0])}")
        if spec["kind"] == "huge":
            # outputs beyond +-65504 store as +-65504, finite: the same case with the folded scale times 1000
            big = c["scale"] * np.float32(1000)
            h4, h3 = run(4, scale=big), run(3, scale=big)
            assert np.abs(h3).max() > 65504 and np.isfinite(h4).all() and np.abs(h4).max() == 65504.0
            assert np.array_equal(_bits(h4), _bits(em.round_f16_np(h3))), "saturating case differs"
        # the existing gate's inputs: prec 3 on the raw case, the f32 oracle on the pre-rounded operands
        np.save(tmp_path / f"gpu_{i}.npy", plain.conv2d(c["x"], c["w"], c["scale"], c["shift"], spec["stride"], c["resid"], False, spec["relu_out"], prec=3))
        np.save(tmp_path / f"orc_{i}.npy", ou._conv(xq, wq, spec["ksize"], spec["stride"], 0, 0, c["scale"], c["shift"], c["resid"], 0, int(spec["relu_out"])))
    # outputs below 2^-14: subnormal f16 values are kept (scale and shift 2^-20 of a plain case's: |outputs| up to about 3e-5 < 6.1e-5)
    spec = dict(ksize=1, stride=1, cin=256, cout=128, size=16, n=2, resid=False, relu_in=False, relu_out=False, seed=502, kind="plain")
    c = em.make_conv_case(spec)
    xq, wq = em.round_f16_np(c["x"]), em.round_f16_np(c["w"])
    sc, sh = c["scale"] * np.float32(2.0 ** -20), c["shift"] * np.float32(2.0 ** -20)
    s4 = plain.conv2d(xq, wq, sc, sh, 1, None, False, False, prec=4)
    s3 = plain.conv2d(xq, wq, sc, sh, 1, None, False, False, prec=3)
    sub = (np.abs(s4) < 2.0 ** -14) & (s4 != 0)
    print(f"subnormal-output case: {int(sub.sum())} of {s4.size} outputs are non-zero f16 subnormals, max |out| {np.abs(s4).max():.3e}", flush=True)
    assert sub.mean() > 0.9, "the case should produce f16-subnormal outputs"
    assert np.array_equal(_bits(s4), _bits(em.round_f16_np(s3))), "subnormal outputs are not kept as round_f16 keeps them"
    figs = em.in_child("conv_case_figures", specs=specs, outputs_dir=str(tmp_path), flush_subnormals=False)
    lines, bad = [], []
    for spec, f in zip(specs, figs):
        ratio = f["gpu_err"] / f["orc_err"] if f["orc_err"] > 0 else float("inf") if f["gpu_err"] > 0 else 0.0
        line = (f"k{spec['ksize']} s{spec['stride']} {spec['cin']}->{spec['cout']} @{spec['size']} n{spec['n']} resid={int(spec['resid'])} {spec['kind']}: "
                f"prec 3 |GPU-R| {f['gpu_err']:.3e} |O-R| {f['orc_err']:.3e} ratio {ratio:.2f}")
        lines.append(line)
        if not f["finite"] or not f["gpu_err"] <= 4 * f["orc_err"]:
            bad.append(line)
    print("\n".join(lines), flush=True)
    assert not bad, "prec 3 outside the existing gate (the f16 form itself is off on these shapes):\n" + "\n".join(bad)
    assert not mismatches, "prec 4 != round_f16(prec 3):\n" + "\n".join(mismatches)


SMALL = "conv3_block1_out"      # stem, pool, stage 2, one strided block with its projection shortcut


def _replay(plain, w, x):
    """the f16act network on the host: oracle.resnet's im2col / pool / head / fold_bn, one conv2d(prec 3) per layer on f16-exact
    arrays, round_f16 after im2col and after every layer"""
    import resnet_emul as em
    from oracle import resnet as orr
    r16 = em.round_f16_np

    def conv(name, inp, ksize, st, resid=None, relu=True):
        sc, sh = orr.fold_bn(w[name + ".bn"], w[name + ".b"])
        return r16(plain.conv2d(inp, w[name + ".w"].astype(np.float32), sc, sh, st, resid, False, relu, prec=3))
    wk = np.zeros((1, 1, orr.STEM_K, 64), np.float32)
    wk[0, 0, :orr.STEM_TAPS] = w["conv1.w"].astype(np.float32).reshape(orr.STEM_TAPS, 64)
    sc, sh = orr.fold_bn(w["conv1.bn"], w["conv1.b"])
    a = r16(plain.conv2d(r16(orr.stem_im2col(x)), wk, sc, sh, 1, None, False, True, prec=3))
    a = orr.pool(a)
    assert np.array_equal(r16(a), a)
    stage = 2
    while f"s{stage}b1.c1.w" in w:
        blk = 1
        while f"s{stage}b{blk}.c1.w" in w:
            p = f"s{stage}b{blk}"
            st = 2 if (blk == 1 and stage > 2) else 1
            shortcut = conv(p + ".c0", a, 1, st, None, False) if blk == 1 else a
            t = conv(p + ".c1", a, 1, st)
            t = conv(p + ".c2", t, 3, 1)
            a = conv(p + ".c3", t, 1, 1, shortcut, True)
            blk += 1
        stage += 1
    return orr.head(a, w["fc.w"].ravel(), float(w["fc.b"].ravel()[0]))


def test_whole_network_exact_by_replay(plain):
    """tmat_resnet_predict in f16act mode == the host replay's probabilities, bit for bit: pins the buffer rotation, the half-size reuse
    of the activation buffers and the f16 forms of im2col, pool and head.  Size 64: widths 32 / 16 / 8; size 96: 48 / 24 / 12, of
    which 12 takes the generic prologue."""
    from tmat_amd import inv_depth
    w = inv_depth.synth_resnet_weights(5, SMALL)
    ens = inv_depth.InvDepthEnsemble(plain, [w])
    rs = np.random.RandomState(6)
    try:
        ens.set_precision("f16act")
        for size in (64, 96):
            x = (rs.uniform(0, 255, (3, size, size, 1)) - np.array([103.939, 116.779, 123.68])).astype(np.float32)
            got = ens.predict(x, 0)
            ref = _replay(plain, w, x)
            assert 0.001 < ref.min() and ref.max() < 0.999, ref
            assert np.array_equal(_bits(got), _bits(ref)), (size, got, ref)
    finally:
        ens.set_precision("f32")


@pytest.fixture(scope="module")
def members():
    from tmat_amd import inv_depth
    return [inv_depth.synth_resnet_weights(s) for s in range(3)]


def test_end_to_end_deviation_sizes(plain, members):
    """Gate and inputs of tests/test_gpu_invdepth_f16.py::test_end_to_end_deviation_sizes (32 slices x 3 members), with E16act = the
    float64 evaluation of the f16act contract: per member max|GPU - E64| <= 2 max|E16act - E64|, the same for the ensemble mean, labels
    equal E64's, and NO slice excluded from the label check (a condition).  The float64 evaluation gave member deviations 3.88e-4,
    1.64e-3 and 3.6e-10, mean deviation 4.19e-4 (exclusion radius 8.4e-4), nearest exact mean 9.7e-4 from the threshold, largest
    activation 46.6 (no saturation).  max|GPU - E16act| and the f16act-vs-f16 / f16act-vs-f32 figures are printed, not gated."""
    import resnet_emul_f16act as ea
    from tmat_amd import inv_depth, synth
    stack_seeds = [20, 21, 22, 23]
    stacks = [synth.synth_stack(s, 8, 300, 360, n_vessels=8) for s in stack_seeds]
    ens = inv_depth.InvDepthEnsemble(plain, members)
    g32 = np.concatenate(ens.predict_stacks(stacks)).astype(np.float64)
    try:
        ens.set_precision("f16")
        g16 = np.concatenate(ens.predict_stacks(stacks)).astype(np.float64)
        ens.set_precision("f16act")
        ga_f32 = np.concatenate(ens.predict_stacks(stacks))
    finally:
        ens.set_precision("f32")
    ga = ga_f32.astype(np.float64)
    E = ea.in_child("ensemble_probs", seeds=[0, 1, 2], stack_seeds=stack_seeds, z=8, H=300, W=360, size=256, n_vessels=8)
    e64, ea16 = E["exact"], E["f16act"]
    assert ga.shape == e64.shape == ea16.shape == (32, 3)
    dev_gpu = np.abs(ga - e64).max(axis=0)
    dev_e = np.abs(ea16 - e64).max(axis=0)
    mean_gpu = np.abs(ga.mean(1) - e64.mean(1)).max()
    mean_e = np.abs(ea16.mean(1) - e64.mean(1)).max()
    margin = np.abs(e64.mean(1) - 0.5)
    excluded = int((margin <= 2 * mean_e).sum())
    lab_gpu = np.array([lab for _, lab in inv_depth.ensemble_predictions(ga_f32, 0.5)])
    lab_e64 = (e64.mean(1) > 0.5).astype(int)
    msg = (f"per member max|GPU-E64| {dev_gpu} vs max|E16act-E64| {dev_e} (ratio {dev_gpu / dev_e}); mean: {mean_gpu:.3e} vs {mean_e:.3e} (ratio {mean_gpu / mean_e:.2f}); "
           f"max|GPU-E16act| {np.abs(ga - ea16).max():.3e}; nearest exact mean to 0.5: {margin.min():.3e}, slices excluded from the label check: {excluded}; "
           f"largest activation of E16act {E['max_act']:.1f}; GPU f16act vs GPU f16: member {np.abs(ga - g16).max():.3e}, mean {np.abs(ga.mean(1) - g16.mean(1)).max():.3e}; "
           f"GPU f16act vs GPU f32: member {np.abs(ga - g32).max():.3e}, mean {np.abs(ga.mean(1) - g32.mean(1)).max():.3e}; f32 GPU vs E64: {np.abs(g32 - e64).max():.3e}")
    print(msg, flush=True)
    assert np.abs(g32 - e64).max() < 2e-5, msg                     # E64 is the right yardstick
    assert (dev_gpu <= 2 * dev_e).all(), msg
    assert mean_gpu <= 2 * mean_e, msg
    assert excluded == 0, msg
    assert np.array_equal(lab_gpu, lab_e64), msg


def test_determinism_and_switching(plain, members):
    import os
    import subprocess
    import tempfile
    from oracle import resnet as orr
    from tmat_amd import _lib, inv_depth, synth
    ws = members[:2]
    stacks = [synth.synth_stack(30 + i, 2, 300, 360, n_vessels=8) for i in range(2)]
    ens = inv_depth.InvDepthEnsemble(plain, ws)
    f32_before = ens.predict_stacks(stacks)
    ens.set_precision("f16")
    f16_before = ens.predict_stacks(stacks)
    ens.set_precision("f16act")
    try:
        a = ens.predict_stacks(stacks)
        b = ens.predict_stacks(stacks)
        single = [ens.predict_stack(s) for s in stacks]
        for x, y, z in zip(a, b, single):
            assert np.array_equal(_bits(x), _bits(y)), "f16act results differ call to call"
            assert np.array_equal(_bits(x), _bits(z)), "predict_stack and predict_stacks differ in f16act mode"
        assert not np.array_equal(a[0], f32_before[0]) and not np.array_equal(a[0], f16_before[0]), "f16act computed the result of another mode"
        assert np.abs(np.concatenate(a) - np.concatenate(f32_before)).max() < 2e-2
        # a model loaded while the mode is on works (its f16 weights are made at load)
        ens2 = inv_depth.InvDepthEnsemble(plain, ws[:1])
        assert np.array_equal(_bits(ens2.predict_stack(stacks[0])[:, 0]), _bits(a[0][:, 0]))
        # poisoned workspaces: nothing of an earlier call is read
        for pattern in (0xFF, 0x00, 0x7B):          # f16 NaN, zero, large finite values
            plain.debug_poison(pattern)
            for x, y in zip(a, ens.predict_stacks(stacks)):
                assert np.array_equal(_bits(x), _bits(y)), f"f16act results change after tmat_debug_poison({pattern:#x})"
        # f16act -> f16: no half-width data leaks through the reused buffers
        ens.set_precision("f16")
        for x, y in zip(f16_before, ens.predict_stacks(stacks)):
            assert np.array_equal(_bits(x), _bits(y)), "f16act -> f16 does not reproduce the f16 bits"
        ens.set_precision("f16act")
        for x, y in zip(a, ens.predict_stacks(stacks)):
            assert np.array_equal(_bits(x), _bits(y))
    finally:
        ens.set_precision("f32")
    for s, x, z in zip(stacks, ens.predict_stacks(stacks), f32_before):
        assert np.array_equal(_bits(x), _bits(z))
        ox = orr.prep_inv_depth_imgs(s, 256)
        ref = np.stack([orr.forward(w, ox) for w in ws], axis=1)
        assert np.array_equal(_bits(x), _bits(ref)), "f16act -> f32 does not restore the bit-exact path"
    # value 3 is accepted; 2 and 4 are refused, with a message, and leave the mode alone
    L = _lib.lib()
    assert L.tmat_resnet_set_precision(plain.raw, 3) == 0
    for bad in (2, 4):
        assert L.tmat_resnet_set_precision(plain.raw, bad) != 0 and b"tmat_resnet_set_precision" in L.tmat_last_error()
    assert np.array_equal(_bits(ens.predict_stack(stacks[0])), _bits(a[0])), "a refused value changed the mode"
    assert L.tmat_resnet_set_precision(plain.raw, 0) == 0
    with pytest.raises(ValueError):
        ens.set_precision("bf16")
    # the environment variable selects the mode at creation (a child process: the variable is read at creation)
    repo = Path(__file__).resolve().parents[1]
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from tmat_amd import _lib\n"
            "h = _lib.Handle(None, 0)\n"
            "import numpy as np\n"
            "from tmat_amd import inv_depth, synth\n"
            "ens = inv_depth.InvDepthEnsemble(h, [inv_depth.synth_resnet_weights(0)])\n"
            "np.save(sys.argv[1], ens.predict_stack(synth.synth_stack(30, 2, 300, 360, n_vessels=8)))\n"
            "h.close()\n") % (str(repo), str(repo / "tissue-model-analysis-tools_amd"))
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, "-c", code, f"{d}/p.npy"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TMAT_INV_DEPTH_PRECISION="f16act"))
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(_bits(np.load(f"{d}/p.npy")[:, 0]), _bits(a[0][:, 0])), "TMAT_INV_DEPTH_PRECISION=f16act did not select the mode"


def test_script_precision_f16act(tmp_path):
    """compute_inv_depth.py --precision f16act on the two small stacks of the f16 CLI test: runs, same CSV format, its probabilities differ
    from the f32 run's by at most 2 max|mean E16act - mean E64| + 1e-4 (the two 4-decimal roundings), and are not identical to them"""
    import csv
    import os
    import subprocess
    import resnet_emul_f16act as ea
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
    for mode in ("f32", "f16act"):
        outd = tmp_path / f"out_{mode}"
        r = subprocess.run([sys.executable, str(script), str(ind), str(outd), "--precision", mode], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1"))
        assert r.returncode == 0, r.stdout + r.stderr
        rows = list(csv.reader(open(outd / "invasion_depth_predictions.csv")))
        assert rows[0] == ["Z Slice ID", "Invasion Probability", "Invasion Prediction (0=no 1=yes)"]
        res[mode] = {r_[0]: (float(r_[1]), int(r_[2])) for r_ in rows[1:]}
    order = inv_depth.best_model_indices(repo / "tissue-model-analysis-tools_amd" / "model_training" / "best_ensemble", 5, 3)
    keys = sorted(res["f32"])
    assert sorted(res["f16act"]) == keys and len(keys) == 6
    devs = []
    for k, sd in seeds.items():
        E = ea.in_child("ensemble_probs", seeds=[int(i) for i in order], stack_seeds=[sd], z=3, H=128, W=160, size=256, n_vessels=6)
        devs.append(np.abs(E["f16act"].mean(1) - E["exact"].mean(1)).max())
    bound = 2 * max(devs) + 1e-4
    diff = {k: abs(res["f16act"][k][0] - res["f32"][k][0]) for k in keys}
    msg = f"|p f16act - p f32| per slice {diff}; bound {bound:.3e}; f32 {res['f32']}; f16act {res['f16act']}"
    print(msg, flush=True)
    assert max(diff.values()) <= bound, msg
    assert any(res["f16act"][k][0] != res["f32"][k][0] for k in keys), "the f16act run printed the f32 probabilities: --precision did nothing\n" + msg

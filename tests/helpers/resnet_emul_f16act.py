"""CPU evaluation of the invasion-depth classifier's f16act mode in torch float64 -- TEST INFRASTRUCTURE ONLY.

Extends tests/helpers/resnet_emul.py: `forward` restates resnet_emul.forward with the activations kept, and with the store of the
contract of TMAT_RESNET_PRECISION_F16ACT (include/tmat.h): the prepared input is rounded once to IEEE binary16 (nearest even,
magnitudes above 65504 saturating), every convolution multiplies f16 values (weights rounded once, activations as stored), accumulates
exactly (float64), runs the f32 epilogue of resnet_emul (`_finish(..., store_f32=True)`: fold, residual add, ReLU, each rounded to f32)
and rounds the result ONCE to f16; the pool takes maxima of f16 values; global average, dense unit and sigmoid in float64.
`store="f32"` keeps the activations f32 instead: resnet_emul.forward(operands="f16"), restated (tests/test_resnet_emul_f16act.py checks
that the two agree bit for bit).

`in_child(name, **kwargs)` is resnet_emul.in_child for the functions of THIS module (the child runs this file).
"""
from __future__ import annotations

import pickle
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resnet_emul as em  # noqa: E402

REPO = em.REPO


def forward(w: dict, x: np.ndarray, store="f16", return_acts=False):
    """x (N, S, S, 3) float32 (prepared input) -> probabilities (N,) float64 [, {name: stored activation (N, C, h, h) float64}]"""
    torch = em._torch()
    F = torch.nn.functional
    acts = {}

    def keep(name, t):
        t = em.quant(t, "f16") if store == "f16" else t
        acts[name] = t
        return t

    def cv(a, name, k, st, resid=None, relu=True, pad=None):
        W = torch.tensor(np.asarray(w[name + ".w"], np.float32).astype(np.float64)).permute(3, 2, 0, 1)
        sc, sh = em.fold(w[name + ".bn"], w[name + ".b"])
        if pad is not None:                         # the stem: ZeroPadding2D(3) + 7x7 stride 2 'valid'
            y = F.conv2d(em.quant(a, "f16"), em.quant(W, "f16"), stride=st, padding=pad)
            y = y * sc[None, :, None, None] + sh[None, :, None, None]
            return keep(name, em._finish(y, None, relu, True))
        y, r, ro = em._conv_t(a, W, k, st, sc, sh, resid, False, relu, "f16", False, "f64")
        return keep(name, em._finish(y, r, ro, True))

    a = torch.tensor(np.asarray(x, np.float32).astype(np.float64)).permute(0, 3, 1, 2)
    if store == "f16":
        a = em.quant(a, "f16")                      # im2col holds the one rounding of the input
    a = cv(a, "conv1", 7, 2, pad=3)
    a = keep("pool1", F.max_pool2d(F.pad(a, (1, 1, 1, 1)), 3, 2))
    stage = 2
    while f"s{stage}b1.c1.w" in w:
        blk = 1
        while f"s{stage}b{blk}.c1.w" in w:
            p = f"s{stage}b{blk}"
            st = 2 if (blk == 1 and stage > 2) else 1
            s_ = cv(a, p + ".c0", 1, st, relu=False) if blk == 1 else a
            t = cv(a, p + ".c1", 1, st)
            t = cv(t, p + ".c2", 3, 1)
            a = cv(t, p + ".c3", 1, 1, resid=s_)
            blk += 1
        stage += 1
    z = a.mean(dim=(2, 3)) @ torch.tensor(np.asarray(w["fc.w"], np.float64).ravel()) + float(np.asarray(w["fc.b"]).ravel()[0])
    prob = torch.sigmoid(z).numpy()
    return (prob, {k: v.numpy() for k, v in acts.items()}) if return_acts else prob


def ensemble_probs(seeds, stack_seeds, z, H, W, size, n_vessels=8, last_layer=None, modes=("exact", "f16act")):
    """resnet_emul.ensemble_probs with the mode "f16act" (this module's forward) next to "exact" and "f16"; also returns "max_act",
    the largest stored activation of the f16act evaluation (saturation starts at 65504)"""
    sys.path[:0] = [p for p in (str(REPO), str(REPO / "tissue-model-analysis-tools_amd")) if p not in sys.path]
    from oracle import resnet as orr
    from tmat_amd import inv_depth, synth
    x = np.concatenate([orr.prep_inv_depth_imgs(synth.synth_stack(s, z, H, W, n_vessels=n_vessels), size) for s in stack_seeds])
    ws = [inv_depth.synth_resnet_weights(s, last_layer) if last_layer else inv_depth.synth_resnet_weights(s) for s in seeds]
    out = {}
    for m in modes:
        if m == "f16act":
            res = [forward(w, x, return_acts=True) for w in ws]
            out[m] = np.stack([r[0] for r in res], axis=1)
            out["max_act"] = float(max(np.abs(v).max() for r in res for v in r[1].values()))
        else:
            out[m] = np.stack([em.forward(w, x, operands=m) for w in ws], axis=1)
    return out


def in_child(name: str, **kwargs):
    """run `name(**kwargs)` of THIS module in a CPU-only child process: resnet_emul.in_child's protocol, the child running this file"""
    import os
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(f"{d}/in.pkl", "wb") as f:
            pickle.dump((name, kwargs), f)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), d], capture_output=True, text=True, timeout=3000,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with open(f"{d}/out.pkl", "rb") as f:
            return pickle.load(f)


if __name__ == "__main__":
    sys.path[:0] = [str(REPO), str(REPO / "tissue-model-analysis-tools_amd")]
    with open(f"{sys.argv[1]}/in.pkl", "rb") as f:
        _name, _kw = pickle.load(f)
    _res = globals()[_name](**_kw)
    with open(f"{sys.argv[1]}/out.pkl", "wb") as f:
        pickle.dump(_res, f)

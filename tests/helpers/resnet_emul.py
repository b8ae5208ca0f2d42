"""CPU evaluation of the invasion-depth classifier in torch float64 -- TEST INFRASTRUCTURE ONLY.

`operands="exact"`: every convolution on its f32 operands as they are, accumulated in float64 (error ~1e-16: "exact" next to f32).
`operands="f16"`: the contract of TMAT_RESNET_PRECISION_F16 (include/tmat.h) with exact accumulation: in each convolution (stem
included) the input activation and the weight are each rounded once to IEEE binary16, round to nearest even, magnitudes above
65504 saturating to +-65504; `flush_subnormals=True` additionally replaces results below 2^-14 in magnitude by zero (what a matrix
unit that flushes f16 subnormals would see).  `operands="bf16"` (for comparison only): bfloat16 operands.
`acc="f32"` runs the same convolutions in torch float32 instead: ANOTHER f32 summation order of the same products -- not the
library's, not the oracle's -- used to show how far two f32 orders of the f16 network drift apart.
Everything behind the accumulator follows oracle/resnet.py: folded scale / shift rounded to f32 (fold_bn), v = acc * scale + shift,
residual add, ReLU, each stored as f32 (the activations live in f32 memory); pool, global average and dense unit in float64.

The GPU tests never import torch (tests/conftest.py:forward_torch_child says why): they call `in_child("name", **kwargs)`, which
runs `name(**kwargs)` of this module in a CPU-only child process and returns its (picklable) result.
"""
from __future__ import annotations

import os
import pickle
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14


def _torch():
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch


def quant(t, operands: str, flush_subnormals: bool = False):
    """float64 tensor -> float64 tensor holding the operand values the mode's matrix unit multiplies"""
    torch = _torch()
    if operands == "exact":
        return t
    if operands == "f16":
        q = t.to(torch.float32).clamp(-F16_MAX, F16_MAX).to(torch.float16).to(torch.float64)      # f32 -> f16 is one RNE rounding
        if flush_subnormals:
            q = torch.where(q.abs() < F16_MIN_NORMAL, torch.zeros_like(q), q)
        return q
    if operands == "bf16":
        return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    raise ValueError(operands)


def quant_np(a, operands="f16", flush_subnormals=False) -> np.ndarray:
    """numpy float32 in, float32 out (every f16 / bf16 value is an f32 value): the PRE-ROUNDED operands the tests feed the f32 oracle"""
    torch = _torch()
    return quant(torch.tensor(np.asarray(a, np.float32).astype(np.float64)), operands, flush_subnormals).numpy().astype(np.float32)


def round_f16_np(a, flush_subnormals=False) -> np.ndarray:
    """quant_np(a, "f16") without torch (numpy's f32 -> f16 cast rounds to nearest even): for test processes that must not import torch"""
    with np.errstate(over="ignore"):
        q = np.clip(np.asarray(a, np.float32), -F16_MAX, F16_MAX).astype(np.float16).astype(np.float32)
    return np.where(np.abs(q) < F16_MIN_NORMAL, np.float32(0), q).astype(np.float32) if flush_subnormals else q


def _conv_t(x, W, ksize, stride, scale, shift, resid, relu_in, relu_out, operands, flush_subnormals, acc):
    """x (N, C, H, W) float64 tensor, W (Cout, Cin, k, k) float64 tensor, scale / shift float64 tensors of f32 values"""
    torch = _torch()
    F = torch.nn.functional
    if relu_in:
        x = F.relu(x)
    if ksize == 1 and stride == 2:                  # TF SAME, 1x1 stride 2: the even indices
        x = x[:, :, ::2, ::2]
        stride = 1
    dt = torch.float32 if acc == "f32" else torch.float64
    y = F.conv2d(quant(x, operands, flush_subnormals).to(dt), quant(W, operands, flush_subnormals).to(dt), stride=stride, padding=ksize // 2).double()
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    return y, resid, relu_out


def _finish(y, resid, relu_out, store_f32):
    torch = _torch()
    if store_f32:
        y = y.float().double()
    if resid is not None:
        y = y + resid
        if store_f32:
            y = y.float().double()
    return torch.nn.functional.relu(y) if relu_out else y


def conv(x, w, ksize, stride, scale, shift, resid=None, relu_in=False, relu_out=False, operands="exact", flush_subnormals=False,
         acc="f64") -> np.ndarray:
    """single convolution, numpy NHWC in (x (N, H, W, Cin), w Keras (k, k, Cin, Cout), resid like the result), float64 NHWC out.
    The result is NOT rounded to f32: it is the reference the f32 implementations are measured against.  scale None: plain bias."""
    torch = _torch()
    xt = torch.tensor(np.asarray(x, np.float32).astype(np.float64)).permute(0, 3, 1, 2)
    Wt = torch.tensor(np.asarray(w, np.float32).astype(np.float64)).permute(3, 2, 0, 1)
    cout = Wt.shape[0]
    sc = torch.ones(cout, dtype=torch.float64) if scale is None else torch.tensor(np.asarray(scale, np.float32).astype(np.float64))
    sh = torch.tensor(np.asarray(shift, np.float32).astype(np.float64))
    rt = None if resid is None else torch.tensor(np.asarray(resid, np.float32).astype(np.float64)).permute(0, 3, 1, 2)
    y, rt, ro = _conv_t(xt, Wt, ksize, stride, sc, sh, rt, relu_in, relu_out, operands, flush_subnormals, acc)
    return _finish(y, rt, ro, store_f32=False).permute(0, 2, 3, 1).contiguous().numpy()


def fold(bn, bias):
    """oracle/resnet.py:fold_bn, as float64 tensors of the f32-rounded values"""
    torch = _torch()
    g, b, m, v = (np.asarray(bn[i], np.float64) for i in range(4))
    sd = g / np.sqrt(v + 1.001e-5)
    return (torch.tensor(sd.astype(np.float32).astype(np.float64)),
            torch.tensor((b + (np.asarray(bias, np.float64) - m) * sd).astype(np.float32).astype(np.float64)))


def forward(w: dict, x: np.ndarray, operands="exact", flush_subnormals=False, acc="f64", return_feat=False):
    """x (N, S, S, 3) float32 (prepared input) -> probabilities (N,) float64 [, trunk output (N, h, h, C) float64]"""
    torch = _torch()
    F = torch.nn.functional

    def cv(a, name, k, st, resid=None, relu=True, pad=None):
        W = torch.tensor(np.asarray(w[name + ".w"], np.float32).astype(np.float64)).permute(3, 2, 0, 1)
        sc, sh = fold(w[name + ".bn"], w[name + ".b"])
        if pad is not None:                         # the stem: ZeroPadding2D(3) + 7x7 stride 2 'valid'
            dt = torch.float32 if acc == "f32" else torch.float64
            y = F.conv2d(quant(a, operands, flush_subnormals).to(dt), quant(W, operands, flush_subnormals).to(dt), stride=st, padding=pad).double()
            y = y * sc[None, :, None, None] + sh[None, :, None, None]
            return _finish(y, None, relu, True)
        y, r, ro = _conv_t(a, W, k, st, sc, sh, resid, False, relu, operands, flush_subnormals, acc)
        return _finish(y, r, ro, True)

    a = cv(torch.tensor(np.asarray(x, np.float32).astype(np.float64)).permute(0, 3, 1, 2), "conv1", 7, 2, pad=3)
    a = F.max_pool2d(F.pad(a, (1, 1, 1, 1)), 3, 2)          # activations are >= 0 behind the ReLU: zero padding = ZeroPadding2D(1)
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
    return (prob, a.permute(0, 2, 3, 1).contiguous().numpy()) if return_feat else prob


# ---- cases of the single-convolution GPU test (tests/test_gpu_invdepth_f16.py), made identically in the parent and in the child -----
def make_conv_case(spec: dict) -> dict:
    """spec: ksize, stride, cin, cout, size, n, resid, relu_in, relu_out, seed, kind ("plain" | "subnormal" | "huge")"""
    rs = np.random.RandomState(spec["seed"])
    k, cin, cout, S, n = spec["ksize"], spec["cin"], spec["cout"], spec["size"], spec["n"]
    x = rs.normal(0, 1, (n, S, S, cin)).astype(np.float32)
    w = rs.normal(0, 1, (k, k, cin, cout)).astype(np.float32)
    kind = spec.get("kind", "plain")
    if kind == "subnormal":         # weights of magnitude 2^-24 .. 2^-14 (f16 subnormals) against inputs ~ 2^10: products O(1e-3 .. 1)
        w = (rs.uniform(1.0, 1000.0, w.shape) * 2.0 ** -24 * rs.choice([-1.0, 1.0], w.shape)).astype(np.float32)
        x = (x * 1024.0).astype(np.float32)
    elif kind == "huge":            # a tenth of the inputs beyond the f16 range: they enter the products as +-65504
        big = rs.uniform(0, 1, x.shape) < 0.1
        x = np.where(big, x * 1.0e6, x).astype(np.float32)
        w = (w * 1.0e-3).astype(np.float32)
    So = S // spec["stride"]
    return dict(x=x, w=w, scale=rs.uniform(0.5, 1.5, cout).astype(np.float32), shift=rs.normal(0, 0.5, cout).astype(np.float32),
                resid=rs.normal(0, 1, (n, So, So, cout)).astype(np.float32) if spec["resid"] else None)


def conv_case_figures(specs, outputs_dir: str, flush_subnormals=False):
    """for every spec i: R = float64 convolution of the f16-rounded operands + epilogue, U = the same on the unrounded operands; with
    G = gpu_{i}.npy (library, prec 3) and O = orc_{i}.npy (f32 oracle fed the pre-rounded operands) read from outputs_dir, returns
    per case dict(gpu_err = max|G - R|, orc_err = max|O - R|, Q = max|R - U|, finite = all(isfinite(G)), rmax = max|R|)
    (+ gpu_err_flush / gpu_err_keep for kind "subnormal": G against R with and without flushed f16 subnormals)"""
    out = []
    for i, spec in enumerate(specs):
        c = make_conv_case(spec)
        args = (c["x"], c["w"], spec["ksize"], spec["stride"], c["scale"], c["shift"], c["resid"], spec["relu_in"], spec["relu_out"])
        R = conv(*args, operands="f16", flush_subnormals=flush_subnormals)
        U = conv(*args, operands="exact")
        G = np.load(os.path.join(outputs_dir, f"gpu_{i}.npy")).astype(np.float64)
        O = np.load(os.path.join(outputs_dir, f"orc_{i}.npy")).astype(np.float64)
        fig = dict(gpu_err=float(np.abs(G - R).max()), orc_err=float(np.abs(O - R).max()), Q=float(np.abs(R - U).max()),
                   finite=bool(np.isfinite(G).all()), rmax=float(np.abs(R).max()))
        if spec.get("kind") == "subnormal":
            Rf = conv(*args, operands="f16", flush_subnormals=True)
            Rk = conv(*args, operands="f16", flush_subnormals=False)
            fig.update(gpu_err_flush=float(np.abs(G - Rf).max()), gpu_err_keep=float(np.abs(G - Rk).max()), keep_vs_flush=float(np.abs(Rk - Rf).max()))
        out.append(fig)
    return out


def prerounded(spec, flush_subnormals=False):
    """the case's x (after the load-side ReLU where the spec has one) and w rounded to f16, as f32 arrays"""
    c = make_conv_case(spec)
    x = np.maximum(c["x"], 0) if spec["relu_in"] else c["x"]
    return round_f16_np(x, flush_subnormals), round_f16_np(c["w"], flush_subnormals)


def ensemble_probs(seeds, stack_seeds, z, H, W, size, n_vessels=8, last_layer=None, modes=("exact", "f16"), flush_subnormals=False):
    """probabilities (slices, members) float64 per mode for synth_resnet_weights(seed) members on the prepared slices of
    synth_stack(stack_seed, z, H, W) stacks (oracle.resnet.prep_inv_depth_imgs)"""
    sys.path[:0] = [p for p in (str(REPO), str(REPO / "tissue-model-analysis-tools_amd")) if p not in sys.path]
    from oracle import resnet as orr
    from tmat_amd import inv_depth, synth
    x = np.concatenate([orr.prep_inv_depth_imgs(synth.synth_stack(s, z, H, W, n_vessels=n_vessels), size) for s in stack_seeds])
    ws = [inv_depth.synth_resnet_weights(s, last_layer) if last_layer else inv_depth.synth_resnet_weights(s) for s in seeds]
    return {m: np.stack([forward(w, x, operands=m, flush_subnormals=flush_subnormals and m == "f16") for w in ws], axis=1) for m in modes}


def in_child(name: str, **kwargs):
    """run `name(**kwargs)` of this module in a CPU-only child process (no GPU visible: torch's own ROCm runtime stays unused)"""
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

#!/usr/bin/env python3
"""Measurement of BASELINE config #5 on one MI355X: compute_cell_area and the compute_inv_depth ensemble on
synthetic images, host buffers in (PCIe inclusive).  Prints two JSON lines in bench.py's format:
  * cell area: images/s for 1024 x 1024 uint16 images -> 512 x 512 -> GMM threshold -> area (batches of 64);
  * invasion depth: Z slices/s for 32-slice 512 x 512 stacks through 3 ResNet50(conv4_block6_out) classifiers at 256 x 256.
cpu_baseline: the oracles (numpy / scikit-learn-equivalent EM; oracle/resnet.py through the C convolution) on a bounded sample.

    python tools/bench_config5.py [--images 256] [--stacks 8] [--steps 3] [--no-cpu] [--precision f32|f16|f16act|both|all] [--skip-cell-area]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512, help="BASELINE config #5: 512 images")
    ap.add_argument("--stacks", type=int, default=16, help="16 stacks x 32 slices = 512 images for the invasion-depth tool")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--precision", choices=("f32", "f16", "f16act", "both", "all"), default="f32",
                    help="invasion-depth line(s): f32 (bit-exact contract), f16 (opt-in f16 matrix-core mode), f16act (opt-in: f16 mode with f16 activations in memory), "
                         "both (f32 and f16) or all (the three); the f16 and f16act lines carry their ratio and parity against the f32 result of the same run")
    ap.add_argument("--skip-cell-area", action="store_true", help="only the invasion-depth line(s)")
    a = ap.parse_args()
    from tmat_amd import _lib, inv_depth, preprocessing, synth
    h = _lib.Handle(None, 0)
    if not a.skip_cell_area:
        cell_area_line(a, h)
    inv_depth_lines(a, h)


def cell_area_line(a, h):
    from tmat_amd import preprocessing, synth
    base = np.stack([synth.synth_image(i, 1024, n_vessels=40) for i in range(8)])
    imgs = base[np.arange(a.images) % 8]

    def cell_step():
        out = []
        for i0 in range(0, a.images, 64):
            out.append(preprocessing.cell_area_batch(h, imgs[i0:i0 + 64], 512, 0.0)[0])
        return np.concatenate(out)
    area = cell_step()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        area = cell_step()
    dt = (time.perf_counter() - t0) / a.steps
    line = {"metric": "images/sec through compute_cell_area (1024x1024 uint16 -> 512 -> GMM threshold -> area)", "value": a.images / dt, "unit": "images/s",
            "n_gpus": 1, "steps": a.steps, "warmup": 1, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64 (EM on the histogram) / u16", "data": "synthetic", "config": {"workload": f"{a.images} images, host buffers in, batches of 64", "sd_coef": 0.0}}
    # roofline of the tool as a whole: HBM-bound by construction -- algorithmic bytes per image = the 1024^2 u16 input (2 MB) read once
    # + the 512^2 u16 down-sampled image written and read twice (histogram, threshold: 1.5 MB) + the 512^2 u8 result (0.25 MB);
    # the host-pointer entry moves the same 2 MB over PCIe first, which is what bounds this measurement (63 GB/s spec)
    alg_bytes = 1024 * 1024 * 2 + 3 * 512 * 512 * 2 + 512 * 512
    line["roofline"] = {"bound": "hbm", "achieved": alg_bytes * a.images / dt / 1e9, "peak": 8000.0, "unit": "GB/s",
                        "frac": alg_bytes * a.images / dt / 1e9 / 8000.0, "traffic": None,
                        "note": "whole tool, PCIe inclusive (2 MB/image of H2D at <= 63 GB/s = at most 31 500 images/s); per kernel see profiles/r04_config5_kernel_stats.csv"}
    if not a.no_cpu:
        from oracle import cellarea as ca
        c0 = time.perf_counter()
        ref = [ca.cell_area(base[i], 512, 0.0)[0] for i in range(4)]
        c1 = time.perf_counter()
        line["cpu_baseline"] = {"value": 4 / (c1 - c0), "unit": "images/s", "cores": 1, "kind": "port", "sample": "4 images through oracle/cellarea.py"}
        line["parity"] = bool(np.array_equal(area[:4], ref))
    print(json.dumps(line), flush=True)

def inv_depth_lines(a, h):
    from tmat_amd import inv_depth, synth
    stacks = [synth.synth_stack(i, 32, 512, 512, n_vessels=16) for i in range(2)]
    ws = [inv_depth.synth_resnet_weights(s) for s in range(3)]
    ens = inv_depth.InvDepthEnsemble(h, ws)
    batch = [stacks[k % 2] for k in range(a.stacks)]
    nsl = a.stacks * 32
    flops = inv_depth.flops_per_slice(ws[0], 256) * 3 * nsl
    f32_line = f32_probs = None
    for mode in {"both": ("f32", "f16"), "all": ("f32", "f16", "f16act")}.get(a.precision, (a.precision,)):
        ens.set_precision(mode)
        ens.predict_stack(stacks[0])                         # warm-up (and, in f16 mode, the f16 copy of the weights)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            all_probs = ens.predict_stacks(batch)                # stacks of one shape ride together, 128 slices per call
        dt = (time.perf_counter() - t0) / a.steps
        probs = all_probs[a.stacks - 1]
        peak = 157.3 if mode == "f32" else 2516.6            # dense f32 / f16 matrix peak of one MI355X, TFLOP/s
        line = {"metric": "Z slices/sec through compute_inv_depth (3 x ResNet50 conv4_block6_out at 256x256)", "value": nsl / dt, "unit": "slices/s", "n_gpus": 1,
                "steps": a.steps, "warmup": 1, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": {"f32": "f32", "f16": "f16 operands, f32 accumulate", "f16act": "f16 operands and activations, f32 accumulate"}[mode],
                "data": "synthetic", "config": {"workload": f"{a.stacks} stacks of 32 x 512 x 512 u16, host buffers in, 4 stacks per call; 3 ensemble members, random-init weights",
                                                "precision": mode},
                "roofline": {"bound": "mfma", "achieved": flops / dt / 1e12, "peak": peak, "unit": "TFLOP/s", "frac": flops / dt / 1e12 / peak, "traffic": None,
                             "note": "convolution FLOPs of the three ResNet50(conv4_block6_out) members (2 MACs, stem included) over the whole call: upload, resize, "
                                     "preparation, stem, pooling and head are inside the time"}}
        if mode == "f32":
            f32_line, f32_probs = line, np.concatenate(all_probs)
            if not a.no_cpu:
                from oracle import resnet as orr
                c0 = time.perf_counter()
                ox = orr.prep_inv_depth_imgs(stacks[(a.stacks - 1) % 2][:4], 256)
                ref = np.stack([orr.forward(w, ox) for w in ws], axis=1)
                c1 = time.perf_counter()
                line["cpu_baseline"] = {"value": 4 / (c1 - c0), "unit": "slices/s", "cores": "all (OpenMP C convolution)", "kind": "port", "sample": "4 slices x 3 models through oracle/resnet.py"}
                line["parity"] = bool(np.array_equal(probs[:4].view(np.uint32), ref.view(np.uint32)))
        else:
            if mode == "f16act":
                line["roofline"]["note"] += "; against the dense f16 peak -- activations are f16 in HBM and in LDS (DESIGN 7c)"
            else:
                line["roofline"]["note"] += "; against the dense f16 peak -- the f32 activations (HBM traffic, A-tile DMA + LDS reads), not the matrix pipe, bound the f16 convolution (DESIGN 7c)"
            if f32_line is not None:                     # reported, pass or fail, as the UNet's "alt" block is: the mode is not bit-exact by contract
                p16, p32 = np.concatenate(all_probs).astype(np.float64), f32_probs.astype(np.float64)
                e16, e32 = inv_depth.ensemble_predictions(p16.astype(np.float32)), inv_depth.ensemble_predictions(f32_probs)
                line["vs_f32_same_run"] = line["value"] / f32_line["value"]
                line["parity"] = {"max_abs_dp_member": float(np.abs(p16 - p32).max()), "max_abs_dp_mean": float(np.abs(p16.mean(1) - p32.mean(1)).max()),
                                  "rounded_differ": int(sum(x[0] != y[0] for x, y in zip(e16, e32))), "label_flips": int(sum(x[1] != y[1] for x, y in zip(e16, e32))),
                                  "slices": int(len(p16))}
        print(json.dumps(line), flush=True)
    ens.set_precision("f32")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The narrow models -- filter_counts (32, 64, 128, 256) and (16, 32, 64, 128) -- beside the shipped (64, 128, 256, 512) (GPU box).

    python tools/bench_narrow.py [--images 64] [--side 1024] [--rounds 3] [--out profiles/narrow_bench.json]
        analyze_batch on synth_image(i, side) with synth_weights(0, fc), one handle per model, the models alternating for `rounds` rounds:
        median images/s; the stage split -- segment_batch (front end + network + blend) alone, and with TMAT_TRACE=1 in the environment the
        library's per-pass trace lines (waited for the GPU / for the host jobs of the previous pass).
    python tools/bench_narrow.py --forward 32|16|64 [--patches 200]
        two plain forwards of `patches` patches: what tools/gpu_narrow_prof.sh runs under rocprofv3 --kernel-trace
    python tools/bench_narrow.py --table <kernel_trace.csv> --forward 32|16 [--patches 200]
        the narrow launches of the LAST forward of that trace in launch order, beside tmat_model_layers: time, bound, fraction of the bound
        as CSV rows on stdout.  Bound: the larger of the matrix time at 157.3 TFLOP/s (f32 MFMA peak) and the launch's compulsory bytes
        (input, output, residual, activated copy) at 4.0 TB/s, the rate of the project's streaming kernels (3.9-4.4).
"""
import argparse
import csv
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd"))
from tmat_amd import _lib, branches, synth  # noqa: E402

MODELS = {"64": (64, 128, 256, 512), "32": (32, 64, 128, 256), "16": (16, 32, 64, 128)}
CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)
MFMA_F32_PEAK = 157.3e12
HBM_RATE = 4.0e12


class StderrCapture:
    """the C library's trace lines (fprintf to stderr) of the calls made inside the block"""

    def __init__(self, active):
        self.active, self.text = active, ""

    def __enter__(self):
        if self.active:
            sys.stderr.flush()
            self.tmp = tempfile.TemporaryFile(mode="w+b")
            self.saved = os.dup(2)
            os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        if self.active:
            os.dup2(self.saved, 2)
            os.close(self.saved)
            self.tmp.seek(0)
            self.text = self.tmp.read().decode(errors="replace")
            self.tmp.close()
        return False


def forward(key, patches):
    h = _lib.Handle(synth.pack_weights(synth.synth_weights(0, filter_counts=MODELS[key])), 0, patches)
    x = np.random.RandomState(0).uniform(0, 1, (patches, 320, 320)).astype(np.float32)
    for r in range(2):
        t = time.time(); h.unet_predict(x); dt = time.time() - t
        print(f"{MODELS[key]} forward {r}: {dt * 1e3:.1f} ms for {patches} patches, copies included", flush=True)
    h.close()


def table(key, trace, patches):
    fc = MODELS[key]
    layers = [r for r in _lib.model_layers(synth.pack_weights(synth.synth_weights(0, filter_counts=fc))).tolist() if r[5] == 1]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(trace)) if "conv_narrow_kernel" in r["Kernel_Name"])
    assert len(layers) and len(rows) >= len(layers) and len(rows) % len(layers) == 0, (len(rows), len(layers))
    rows = rows[-len(layers):]
    w = csv.writer(sys.stdout)
    last3 = max(i for i, l in enumerate(layers) if l[0] == 3)           # the last up block's second convolution writes no activated copy
    for i, ((k, st, cin, cout, side, _), (t0, t1)) in enumerate(zip(layers, rows)):
        px_out = patches * side * side                                  # output pixels
        px_in = px_out // 4 if k == 2 else px_out                       # stored pixels read (stride 2 reads one input pixel per output pixel)
        taps = 4 if k == 2 else k * k
        flop = 2.0 * px_out * taps * cin * cout
        second = k == 3                                                 # an up block's second convolution: half-resolution residual in, activated copy out
        byts = 4.0 * (px_in * cin + px_out * cout * (2 if second and i != last3 else 1) + (px_out // 4 * cout if second else 0))
        us, f_us, b_us = (t1 - t0) / 1e3, flop / MFMA_F32_PEAK * 1e6, byts / HBM_RATE * 1e6
        bound = max(f_us, b_us)
        w.writerow(["x".join(map(str, fc)), k, st, cin, cout, side, patches, f"{us:.1f}", f"{f_us:.1f}", f"{b_us:.1f}",
                    "matrix" if f_us >= b_us else "hbm", f"{bound / us:.3f}", f"{b_us / us:.3f}"])


def trace_split(text):
    gpu = [float(m) for m in re.findall(r"waited ([0-9.]+) ms for the GPU", text)]
    jobs = [float(m) for m in re.findall(r"GPU, ([0-9.]+) ms for host jobs", text)]
    if not gpu:
        return None
    return dict(passes=len(gpu), waited_for_gpu_ms_per_pass_median=float(np.median(gpu)), waited_for_host_jobs_ms_per_pass_median=float(np.median(jobs)))


def bench(args):
    imgs = np.stack([synth.synth_image(i, args.side) for i in range(args.images)])
    trace = os.environ.get("TMAT_TRACE", "0") not in ("", "0")
    handles = {k: _lib.Handle(synth.pack_weights(synth.synth_weights(0, filter_counts=fc)), 0, args.max_patches) for k, fc in MODELS.items()}
    hh = ww = int(round(args.side * 0.625))
    res = {k: dict(filter_counts=list(fc), gflop_per_patch=synth.mfma_flops_per_patch(fc) / 1e9,
                   images_per_s=[], segment_ms_per_image=[], trace=[]) for k, fc in MODELS.items()}
    rows = {}
    for k, h in handles.items():                                        # warm-up: buffers, region plans, tables
        rows[k] = branches.analyze_batch(h, imgs[:8], CFG, 1000.0)
    for r in range(args.rounds):
        for k, h in handles.items():
            with StderrCapture(trace) as cap:
                t = time.time(); out = branches.analyze_batch(h, imgs, CFG, 1000.0); dt = time.time() - t
            assert out[:8] == rows[k], "rows changed between calls"
            res[k]["images_per_s"].append(args.images / dt)
            if trace:
                res[k]["trace"].append(trace_split(cap.text))
            pred = np.empty((args.images, hh, ww), np.float64)
            t = time.time()
            _lib.check(_lib.lib().tmat_segment_batch(h.raw, _lib.ptr(imgs), args.images, args.side, args.side, 0.625, _lib.ptr(pred)), "segment")
            res[k]["segment_ms_per_image"].append((time.time() - t) * 1e3 / args.images)
    for k, h in handles.items():
        h.close()
        v = res[k]
        v["images_per_s_median"] = float(np.median(v["images_per_s"]))
        v["images_per_s_spread"] = float(max(v["images_per_s"]) - min(v["images_per_s"]))
        v["segment_ms_per_image_median"] = float(np.median(v["segment_ms_per_image"]))
        v["branches_first_8"] = [r[1] for r in rows[k]]
    base = res["64"]
    for k in ("32", "16"):
        slack = max(base["images_per_s_spread"], res[k]["images_per_s_spread"])
        res[k]["not_below_default"] = bool(res[k]["images_per_s_median"] >= base["images_per_s_median"] - slack)
    line = dict(bench="narrow", images=args.images, side=args.side, rounds=args.rounds, max_patches=args.max_patches, models=res)
    print(json.dumps(line))
    if args.out:
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")
    return 0 if all(res[k]["not_below_default"] for k in ("32", "16")) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-patches", type=int, default=1600)
    ap.add_argument("--out", default="")
    ap.add_argument("--forward", choices=sorted(MODELS), default=None)
    ap.add_argument("--patches", type=int, default=200)
    ap.add_argument("--table", default="")
    a = ap.parse_args()
    if a.table:
        table(a.forward, a.table, a.patches)
    elif a.forward:
        forward(a.forward, a.patches)
    else:
        sys.exit(bench(a))

#!/usr/bin/env python3
"""Cost of the tree overlay.  Prints one JSON line; a full run (no --quick) also writes profiles/overlay_bench.json.

* render: tmat_render_tree_timed on --n images, one warm-up call, --repeats timed calls; every phase (upload, min-max kernels, render
  kernels, copy back of the overlays) is a HIP-event interval on the call's stream, reported as median / min / max.  The render-kernel time
  is set against its HBM floor: (canvas bytes written + background bytes read) / 6.3 TB/s, the achievable HBM rate of an MI355X.
* --pipeline N: tmat_analyze_batch against tmat_analyze_batch_tree on N synthetic 1024 x 1024 images (the bench shape is N = 256), one
  warm-up call and --repeats timed calls each, alternating; wall clock around the synchronous host-pointer entries (they upload, run every
  pass and return finished rows and overlays, so there is nothing an outside event could bracket more tightly).
* one PIL PNG encode and one matplotlib render of the same tree (single-image figures) for scale.
* --merge-kernel-stats CSV: the kernel_stats table of a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_overlay.py
  --quick` run is read and its ovl_* rows are stored beside the event figures.
* --merge-bench FILE: a text file of bench.py JSON result lines, each prefixed "parent " or "branch ", taken in one session; stored with
  the verdict "branch median inside the parent's min-max spread".

    python tools/bench_overlay.py [--n 16] [--vis-width 2000] [--repeats 5] [--pipeline 256] [--quick]
"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

HBM_BYTES_PER_S = 6.3e12            # achievable HBM rate of an MI355X (float4 copy), the floor's denominator


def spread(v, scale=1.0):
    v = [float(x) * scale for x in v]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), repeats=len(v))


def kernel_stats(path):
    """the ovl_* rows of rocprofv3's kernel_stats CSV"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "ovl_" in r.get("Name", ""):
                rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r})
    return rows


def bench_series(path):
    """lines "parent {json}" / "branch {json}" of bench.py runs of one session -> both series and the issue's condition"""
    runs = {"parent": [], "branch": []}
    for line in Path(path).read_text().splitlines():
        who, _, js = line.partition(" ")
        if who in runs and js.lstrip().startswith("{"):
            res = json.loads(js)
            v = res.get("images_per_s", res.get("value"))
            if v is not None:
                runs[who].append(float(v))
    out = dict(parent_images_per_s=runs["parent"], branch_images_per_s=runs["branch"])
    if len(runs["parent"]) >= 3 and len(runs["branch"]) >= 3:
        med = float(np.median(runs["branch"]))
        out.update(branch_median=med, parent_min=min(runs["parent"]), parent_max=max(runs["parent"]), parent_median=float(np.median(runs["parent"])),
                   branch_median_inside_parent_spread=bool(min(runs["parent"]) <= med <= max(runs["parent"])),
                   branch_median_not_below_parent_min=bool(med >= min(runs["parent"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--vis-width", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pipeline", type=int, default=0, metavar="N")
    ap.add_argument("--quick", action="store_true", help="4 images, 2 repeats, no matplotlib figure, no file written")
    ap.add_argument("--merge-kernel-stats", type=str, default=None, metavar="CSV")
    ap.add_argument("--merge-bench", type=str, default=None, metavar="FILE")
    a = ap.parse_args()
    if a.quick:
        a.n, a.repeats = 4, 2
    from make_goldens import synth_field
    from tmat_amd import _lib
    from tmat_amd.topology import MorseGraph
    field = synth_field(33, (384, 384))                          # the width the analysis hands to MorseGraph
    g = MorseGraph(field, thresholds=(5, 10), min_branch_length=5, smoothing_window=5)
    segs, sb, bars = g.colored_tree(1.0)
    bgs = np.stack([(field * (200 + i)).astype(np.uint16) for i in range(a.n)])
    trees = [(segs, sb)] * a.n
    h = _lib.Handle(None, 0)
    try:
        out, _ = h.render_tree_timed(bgs, trees, a.vis_width)    # warm-up: workspaces, code objects
        phases, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out, ms = h.render_tree_timed(bgs, trees, a.vis_width)
            wall.append(time.perf_counter() - t0)
            phases.append(ms)
    finally:
        h.close()
    t0 = time.perf_counter()
    host = _lib.host_render_tree(bgs[:1], trees[:1], a.vis_width)
    t_host = time.perf_counter() - t0
    same = bool(np.array_equal(out[0], host[0]))
    floor_bytes = int(out.nbytes + bgs.nbytes)
    floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
    ev = {k: spread([p[k] for p in phases]) for k in ("upload", "minmax", "render", "copy_back")}
    res = dict(images=a.n, vis_width=a.vis_width, segments_per_image=int(len(segs)), branches=int(len(bars)), canvas=list(out.shape[1:3]),
               bytes_written_per_image=int(out[0].nbytes), device_equals_host_twin=same,
               hip_event_ms_per_call=ev, wall_ms_per_call=spread(wall, 1e3),
               render_kernel_ms_per_image=ev["render"]["median"] / a.n, copy_back_ms_per_image=ev["copy_back"]["median"] / a.n,
               copy_back_GB_per_s=out.nbytes / (ev["copy_back"]["median"] * 1e-3) / 1e9 if ev["copy_back"]["median"] > 0 else None,
               hbm_floor=dict(bytes=floor_bytes, rate_bytes_per_s=HBM_BYTES_PER_S, floor_ms=floor_ms,
                              fraction_of_floor=floor_ms / ev["render"]["median"] if ev["render"]["median"] > 0 else None),
               host_twin_ms_single_image=t_host * 1e3)
    if a.pipeline:
        import io
        from PIL import Image
        from tmat_amd import branches, synth
        cfg = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)
        imgs = np.stack([synth.synth_image(i, 1024) for i in range(a.pipeline)])
        hm = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 0)
        try:
            fns = (("analyze_batch", lambda: branches.analyze_batch(hm, imgs, cfg, 1000.0)),
                   ("analyze_batch_tree", lambda: branches.analyze_batch_tree(hm, imgs, cfg, 1000.0, vis_width=a.vis_width)))
            ts = {name: [] for name, _ in fns}
            for name, fn in fns:
                fn()
            for _ in range(a.repeats):
                for name, fn in fns:
                    t0 = time.perf_counter()
                    r = fn()
                    ts[name].append(time.perf_counter() - t0)
            rows_equal = r[0] == branches.analyze_batch(hm, imgs, cfg, 1000.0)
        finally:
            hm.close()
        t0 = time.perf_counter()
        Image.fromarray(r[1][0], "RGB").save(io.BytesIO(), format="PNG")
        pipe = {name + "_images_per_s": spread([a.pipeline / t for t in v]) for name, v in ts.items()}
        pipe.update(images=a.pipeline, rows_equal=bool(rows_equal), pil_png_encode_ms_single_image=(time.perf_counter() - t0) * 1e3,
                    extra_s_per_call_median=float(np.median(ts["analyze_batch_tree"]) - np.median(ts["analyze_batch"])),
                    note="host-pointer entries, wall clock, one warm-up call each, then alternating timed calls")
        res["pipeline"] = pipe
    if a.merge_kernel_stats:
        res["rocprofv3_kernel_stats"] = kernel_stats(a.merge_kernel_stats)
    if a.merge_bench:
        res["bench_py_default_path"] = bench_series(a.merge_bench)
    if not a.quick:
        import matplotlib
        matplotlib.use("Agg")
        import io
        import matplotlib.pyplot as plt
        t0 = time.perf_counter()
        fig, ax = plt.subplots(figsize=(10, 10), dpi=200)
        ax.imshow(bgs[0], cmap="gray")
        g.plot_colored_tree(1.0, ax=ax)
        fig.savefig(io.BytesIO(), format="png", dpi=200)
        plt.close(fig)
        res["matplotlib_ms_single_image"] = (time.perf_counter() - t0) * 1e3
        (REPO / "profiles" / "overlay_bench.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measurement of the Z-stack (Sato) branch (reference scripts/compute_branches.py:224-306): synthetic
Z x 1024 x 1024 uint16 stacks through tmat_analyze_stack (host buffer in, one result row out: upload, per-slice gaussian,
resize to 384 wide, Sato over the slice pairs, the mask stages, DMT front end on the device, graph sweeps on the host).
Prints one JSON line in bench.py's format: value = stacks/s; cpu_baseline = oracle/sato.py (scipy.ndimage on the host) on
the same stacks.

    python tools/bench_stack.py [--slices 24] [--size 1024] [--steps 5] [--warmup 1] [--hessian gaussian_derivatives] [--batch 8]

--batch N (default 8; 0 skips it) adds the comparison of the batch entry point (tmat_analyze_stack_batch) with the per-stack
loop on the same N synthetic stacks, in this process on this handle: old, new, old, new after one untimed round of each.  The JSON line
gains "batch": stacks/s of the four runs, the within-pair spreads, whether the rows are equal, the batch call's per-pass split (wall ms
of the device stages and of the host graph stage, tmat_debug_stack_trace) and the verdict of the project's bar -- the lower new value
must exceed the higher old value by at least five times the larger within-pair spread.  --batch-only prints that comparison alone.

--batch-only with --detect-well and / or --tree compares, for each flag given, the route compute_branches.py took for Z stacks before
the batch path knew the flag with the route it takes now, on the same N synthetic stacks with a bright well:
    --detect-well   old: sato.stack_well_masks stack by stack in front of one analyze_stack_batch call on host buffers
                    new: one upload, sato.stack_well_masks_batch on the resident chunk, one call on the resident chunk
    --tree          old: per stack stack_field, field_stats, field_tree and Handle.render_tree over the host's max projection
                    new: one upload, one analyze_stack_batch call with the tree request
Same process, same handle, old, new, old, new after one untimed round of each (--repeat runs of the route per window: one run of the
batch route is under 0.1 s, too short a window to time), wall time around calls that end in a synchronise; rows,
bars and overlays are checked for equality; the same bar.  --out FILE also writes the JSON line there.
"""
import argparse
import json
import sys
import time
from pathlib import Path


REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=24)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hessian", default="gaussian_derivatives", choices=["gaussian_derivatives", "gradient"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--batch", type=int, default=8, help="stacks of the batch-vs-loop comparison (0: skip it)")
    ap.add_argument("--batch-only", action="store_true", help="only the batch-vs-loop comparison")
    ap.add_argument("--batch-path", choices=["both", "old", "new"], default="both",
                    help="with --batch-only: old / new runs that path alone, twice, untimed (for a kernel trace of one path: tools/gpu_stack_batch_prof.sh)")
    ap.add_argument("--detect-well", action="store_true", help="with --batch-only: the --detect-well routes of compute_branches.py, old against new")
    ap.add_argument("--tree", action="store_true", help="with --batch-only: the --tree-visualizations routes, old against new")
    ap.add_argument("--vis-width", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5,
                    help="with --detect-well / --tree: times a route runs inside each of the four timed windows (one run of the batch route is under 0.1 s)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    from tmat_amd import _lib, branches, sato, synth
    h = _lib.Handle(None, 0)
    if a.batch_only and (a.detect_well or a.tree):
        line = json.dumps({"metric": "z_stacks_per_sec_batch_flags", "unit": "stacks/s", "higher_is_better": True, "data": "synthetic",
                           "config": {"slices": a.slices, "size": a.size, "hessian": a.hessian, "vis_width": a.vis_width, "stacks": a.batch,
                                      "runs_per_window": a.repeat},
                           "flags": flags_compare(h, a)})
        print(line)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + "\n")
        return
    if a.batch_only:
        print(json.dumps({"metric": "z_stacks_per_sec_batch", "unit": "stacks/s", "higher_is_better": True, "data": "synthetic",
                          "config": {"slices": a.slices, "size": a.size, "hessian": a.hessian}, "batch": batch_compare(h, a)}))
        return
    stacks = [synth.synth_stack(i, a.slices, a.size, a.size, n_vessels=30) for i in range(2)]
    cfg = {"graph_thresh_1": 5, "graph_thresh_2": 10, "graph_smoothing_window": 12, "min_branch_length": 12, "remove_isolated_branches": False}
    sw, mn, mx = branches.graph_px_params(cfg, 384, 1000.0)

    def step(i):
        return sato.analyze_stack(h, stacks[i % 2], 5, 10, sw, mn, mx, False, hessian=a.hessian)
    rows = [step(i) for i in range(max(a.warmup, 1))]
    t0 = time.perf_counter()
    for i in range(a.steps):
        rows.append(step(i))
    dt = time.perf_counter() - t0
    # stage split of one stack (each call uploads / downloads its own operands)
    t1 = time.perf_counter()
    vol = sato.stack_prepare(h, stacks[0], (384 * a.size // a.size, 384))
    t2 = time.perf_counter()
    field = sato.vessel_field(h, vol, a.hessian)
    t3 = time.perf_counter()
    sato.field_stats(h, field, 5, 10, sw, mn, mx, False)
    t4 = time.perf_counter()
    out = {"metric": "z_stacks_per_sec", "value": a.steps / dt, "unit": "stacks/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64 accumulate / f32 store",
           "data": "synthetic", "config": {"workload": f"Z-stack (Sato) branch: {a.slices} x {a.size} x {a.size} u16 -> 384-wide field -> row, host buffers in (PCIe inclusive)",
                                           "hessian": a.hessian},
           "stages_ms": {"stack_prepare": (t2 - t1) * 1e3, "vessel_field": (t3 - t2) * 1e3, "field_stats": (t4 - t3) * 1e3},
           "rows": [list(r) for r in rows[-2:]]}
    # roofline of the stage that holds the branch's arithmetic: scipy-exact separable correlations of the Sato Hessian, f64 accumulation
    # (two adds + one multiply per tap pair, no contraction): 10 passes per sigma, radius r(sigma) tap pairs per pixel and pass
    import math
    if a.hessian == "gaussian_derivatives":
        radii = [int((100.0 if sg <= 1 else 8.0) * sg / math.sqrt(2) + 0.5) for sg in sato.SATO_SIGMAS]
        pairs_px = 10 * sum(radii)
    else:
        pairs_px = 2 * sum(int(4.0 * sg + 0.5) for sg in sato.SATO_SIGMAS)        # gaussian smoothing only; the gradients are differences
    pairs = float(pairs_px) * field.shape[0] * field.shape[1] * (a.slices - 1)
    F64_PAIR_PEAK = 39.3e12 / 3.0        # MI355X f64 vector rate (lane-ops/s) over the 3 operations of a tap pair
    out["roofline"] = {"bound": "f64 vector ALU", "achieved": pairs / (t3 - t2) / 1e12, "peak": F64_PAIR_PEAK / 1e12, "unit": "10^12 tap pairs/s",
                       "frac": pairs / (t3 - t2) / F64_PAIR_PEAK, "traffic": None, "kernel": "tmat::corr1d_col_kernel / corr1d_row_kernel (Sato Hessian)",
                       "note": f"{pairs_px} tap pairs per pixel and slice pair over the WHOLE vessel_field call (upload of the prepared volume, unsharp, "
                               "canny, medial axis, region growing and mask filter inside the time); per kernel: profiles/*_stack_kernel_stats.csv"}
    if not a.no_cpu:
        from oracle import sato as osato
        c0 = time.perf_counter()
        orow = osato.analyze_stack(stacks[0], cfg, 1000.0, hessian=a.hessian)
        c1 = time.perf_counter()
        out["cpu_baseline"] = {"value": 1.0 / (c1 - c0), "unit": "stacks/s", "cores": 1, "kind": "port", "sample": "one stack through oracle/sato.py (scipy.ndimage, single thread)"}
        out["parity"] = list(orow) == list(rows[max(a.warmup, 1) - 1 if False else 0])
    if a.batch > 0:
        out["batch"] = batch_compare(h, a)
    print(json.dumps(out))


def batch_compare(h, a):
    """the per-stack loop (tmat_analyze_stack per stack: the code path of before the batch entry point) against ONE analyze_stack_batch
    call on the same a.batch stacks; both in this process on handle h, alternating after one untimed round of each"""
    import numpy as np
    from tmat_amd import branches, sato, synth
    cfg = {"graph_thresh_1": 5, "graph_thresh_2": 10, "graph_smoothing_window": 12, "min_branch_length": 12, "remove_isolated_branches": False}
    sw, mn, mx = branches.graph_px_params(cfg, 384, 1000.0)
    stacks = np.stack([synth.synth_stack(100 + i, a.slices, a.size, a.size, n_vessels=30) for i in range(a.batch)])

    def old():
        return [sato.analyze_stack(h, st, 5, 10, sw, mn, mx, False, hessian=a.hessian) for st in stacks]

    def new():
        return sato.analyze_stack_batch(h, stacks, [(5, 10)], sw, mn, mx, False, hessian=a.hessian)[0]

    def timed(fn):
        t0 = time.perf_counter()
        rows = fn()
        return a.batch / (time.perf_counter() - t0), rows

    if a.batch_path != "both":                      # one path alone under a profiler: two rounds, so launches per stack = calls / (2 stacks)
        fn = old if a.batch_path == "old" else new
        fn(), fn()
        return {"stacks": a.batch, "path": a.batch_path, "rounds": 2}
    old(), new()                                    # untimed: pool blocks, pinned slots, gaussian tables
    runs = {"old": [], "new": []}
    rows = {}
    traces = []
    for _ in range(2):
        for name, fn in (("old", old), ("new", new)):
            v, rows[name] = timed(fn)
            runs[name].append(v)
            if name == "new":
                traces.append([{"gpu_ms": g, "host_graph_ms": hm} for g, hm in sato.stack_trace(h)])
    spread = {k: abs(v[0] - v[1]) for k, v in runs.items()}
    gain = min(runs["new"]) - max(runs["old"])
    need = 5 * max(spread.values())
    return {"stacks": a.batch, "order": "old, new, old, new", "old_stacks_per_s": runs["old"], "new_stacks_per_s": runs["new"],
            "within_pair_spread": spread, "rows_equal": [tuple(r) for r in rows["old"]] == [tuple(r) for r in rows["new"]],
            "passes": traces, "stacks_per_pass": sato.stack_pass_plan(a.batch, a.slices, a.size, a.size)[0],
            "lower_new_minus_higher_old": gain, "five_times_larger_spread": need, "bar_met": bool(gain >= need and gain > 0),
            "ratio_of_means": (sum(runs["new"]) / 2) / (sum(runs["old"]) / 2)}


def well_stack(index, slices, size):
    """synth_stack inside a bright well (the vignette of tools/bench_well.py:well_image on every slice): round for even indices, a
    rounded square for odd ones"""
    import numpy as np
    from tmat_amd import synth
    st = synth.synth_stack(index, slices, size, size, n_vessels=30).astype(np.float64)
    yy, xx = np.mgrid[0:size, 0:size]
    u, v = (xx - size * 0.51) / (size * 0.45), (yy - size * 0.49) / (size * 0.45)
    inside = (u ** 2 + v ** 2 < 1) if index % 2 == 0 else (u ** 8 + v ** 8 < 1)
    return np.clip(np.where(inside[None], st + 12000.0, 0.0), 0, 65535).astype(np.uint16)


def flags_compare(h, a):
    """per flag: the route of before (see the module text) against the batch route, alternating after one untimed round of each"""
    import numpy as np
    from tmat_amd import _lib, branches, sato
    cfg = {"graph_thresh_1": 5, "graph_thresh_2": 10, "graph_smoothing_window": 12, "min_branch_length": 12, "remove_isolated_branches": False}
    width_um = 1000.0
    sw, mn, mx = branches.graph_px_params(cfg, 384, width_um)
    stacks = np.stack([well_stack(100 + i, a.slices, a.size) for i in range(a.batch)])
    out_hw = sato.dsamp_shape(stacks.shape, 384)
    quiet = lambda m: None      # noqa: E731
    fixed_pruning = sato.stack_well_masks_batch(h, stacks, out_hw, 0, warn=quiet)[1]

    def well_old():
        pruning = np.stack([sato.stack_well_masks(h, st, out_hw, 0)[1] for st in stacks])
        return sato.analyze_stack_batch(h, stacks, [(5, 10)], sw, mn, mx, False, hessian=a.hessian, pruning_masks=pruning)[0], pruning

    def well_new():
        with sato.upload_stacks(h, stacks) as dev:
            pruning = sato.stack_well_masks_batch(h, dev, out_hw, 0, warn=quiet)[1]
            return sato.analyze_stack_batch(h, dev, [(5, 10)], sw, mn, mx, False, hessian=a.hessian, pruning_masks=pruning)[0], pruning

    def tree_old():
        rows, bars, over = [], [], []
        for i, st in enumerate(stacks):
            field = sato.stack_field(h, st, 384, a.hessian)
            rows.append(sato.field_stats(h, field, 5, 10, sw, mn, mx, False, pruning_mask=fixed_pruning[i]))
            background = st.max(0)
            tree, b, _ = branches.field_tree(h, _lib.host_rescale255_f32(field), cfg, width_um, (5, 10), fixed_pruning[i], background.shape[1] / field.shape[1])
            bars.append(b)
            over.append(h.render_tree(background[None], [tree], a.vis_width)[0])
        return rows, bars, np.stack(over)

    def tree_new():
        with sato.upload_stacks(h, stacks) as dev:
            rows, extra = sato.analyze_stack_batch(h, dev, [(5, 10)], sw, mn, mx, False, hessian=a.hessian, pruning_masks=fixed_pruning, tree=True,
                                                   vis_width=a.vis_width)
        return rows[0], extra["bars"][0], extra["overlays"][0]

    def same(x, y):
        if isinstance(x, np.ndarray):
            return bool(np.array_equal(x, y))
        return len(x) == len(y) and all(same(p, q) if isinstance(p, (np.ndarray, list)) else tuple(p) == tuple(q) for p, q in zip(x, y))

    def compare(old, new, names):
        import contextlib
        import io
        res = {}
        with contextlib.redirect_stdout(io.StringIO()):         # the per-stack mask route prints its warnings
            old(), new()                                        # untimed: pool blocks, pinned slots, tables
            runs = {"old": [], "new": []}
            for _ in range(2):
                for name, fn in (("old", old), ("new", new)):
                    t0 = time.perf_counter()
                    for _ in range(max(a.repeat, 1)):
                        res[name] = fn()
                    runs[name].append(max(a.repeat, 1) * a.batch / (time.perf_counter() - t0))
        spread = {k: abs(v[0] - v[1]) for k, v in runs.items()}
        gain = min(runs["new"]) - max(runs["old"])
        need = 5 * max(spread.values())
        return {"order": "old, new, old, new", "old_stacks_per_s": runs["old"], "new_stacks_per_s": runs["new"], "within_pair_spread": spread,
                "equal": {nm: same(x, y) for nm, x, y in zip(names, res["old"], res["new"])},
                "lower_new_minus_higher_old": gain, "five_times_larger_spread": need, "bar_met": bool(gain >= need and gain > 0),
                "ratio_of_means": (sum(runs["new"]) / 2) / (sum(runs["old"]) / 2)}

    out = {}
    if a.detect_well:
        out["detect_well"] = compare(well_old, well_new, ("rows", "pruning_masks"))
        out["detect_well"]["pruning_pixels"] = [int(m.sum()) for m in fixed_pruning]
    if a.tree:
        out["tree"] = compare(tree_old, tree_new, ("rows", "bars", "overlays"))
    return out


if __name__ == "__main__":
    main()

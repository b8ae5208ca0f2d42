#!/usr/bin/env python3
"""Old route against new route of the cell-area tool's Z-stack and --detect-well forms on one MI355X.  One process, the
two routes alternated, `--rounds` timed rounds after `--warmup` untimed rounds of every shape; outputs of the two routes are asserted equal at the
timed sizes.  Prints JSON lines in the format of tools/bench_config5.py, one per case and route, plus one for the fused kernel alone:

  (a) 8 stacks of 16 x 2048^2 u16 -> 512       old: zstacks.proj_max per stack + cell_area_batch     new: cell_area_stacks
  (b) 64 images of 1024^2 u16 with -w          old: cell_area_batch_well                             new: cell_area_stacks(detect_well=True)
  (c) 512 plain 1024^2 images, batches of 64   old: cell_area_batch                                  new: cell_area_stacks
  (d) the stacks of (a) inside a well, -w      old: proj_max per stack + cell_area_batch_well        new: cell_area_stacks(detect_well=True)

Whole-call times are host clock around calls that end in a device synchronise and include the PCIe copies.  The kernel line is the
HIP-event time of cell_small_kernel alone on resident stacks (tmat_prof_enable), over the bytes the algorithm must read -- the source
rows the taps touch x W x 2 x Z x n, plus the output -- against the HBM peak.

    python tools/bench_cell_area.py [--rounds 3] [--stacks 8] [--well-images 64] [--images 512] [--out profiles/cell_area_batch_bench.json]
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
sys.path.insert(0, str(REPO / "tools"))

HBM_PEAK_GBS = 8000.0           # HBM3E spec peak of one MI355X; a float4 copy measures 6 290 GB/s


def touched_rows(H, oh):
    """source rows the vertical taps of cv2's bilinear resize (or the 2 x 2 mean) read"""
    if H == 2 * oh:
        return H
    rows = set()
    for d in range(oh):
        fx = np.float32((d + 0.5) * (H / oh) - 0.5)
        sx = int(np.floor(fx))
        sx = min(max(sx, 0), H - 1)
        rows.update((sx, min(sx + 1, H - 1)))
    return len(rows)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def compare(name, workload, units, unit_name, old, new, rounds, lines, warmup=2):
    """`warmup` untimed alternating rounds, then `rounds` timed ones; equal outputs asserted"""
    for _ in range(max(warmup, 1)):
        ref_old, ref_new = old(), new()
        assert same(ref_old, ref_new), f"case {name}: the two routes disagree"
    ms = {"old": [], "new": []}
    for _ in range(rounds):
        for key, fn in (("old", old), ("new", new)):
            t, out = timed(fn)
            assert same(out, ref_old), f"case {name}: route {key} changed its output"
            ms[key].append(t)
    med_old = float(np.median(ms["old"]))
    for key in ("old", "new"):
        med = float(np.median(ms[key]))
        lines.append({"metric": f"cell area case ({name}), {key} route: {workload[key]}", "value": units / (med / 1e3), "unit": f"{unit_name}/s", "n_gpus": 1,
                      "steps": rounds, "warmup": max(warmup, 1), "ms_per_step": med, "ms_rounds": ms[key], "ms_spread": max(ms[key]) - min(ms[key]),
                      "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64 (EM on the histogram) / u16", "data": "synthetic",
                      "config": {"case": name, "route": key, "workload": workload["what"], "timing": "host clock around synchronising calls, PCIe inclusive"},
                      "vs_old_same_run": med_old / med, "parity": True})
        print(json.dumps(lines[-1]), flush=True)
    # the routing rule of DESIGN 7c: the new route's median must beat the old one's by more than the spread of the old route's repeats
    spread_old = max(ms["old"]) - min(ms["old"])
    verdict = {"metric": f"cell area case ({name}): routing", "case": name, "old_ms_median": med_old, "old_ms_spread": spread_old,
               "new_ms_median": float(np.median(ms["new"])), "new_route_wins": bool(med_old - float(np.median(ms["new"])) > spread_old)}
    lines.append(verdict)
    print(json.dumps(verdict), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds of both routes in front of the timed ones (the first calls of a shape allocate "
                                                          "workspaces and fault in fresh host pages)")
    ap.add_argument("--stacks", type=int, default=8)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--well-images", type=int, default=64)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--cases", default="abcdk", help="a, b, c, d: the cases; k: the fused kernel alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench_well import well_image
    from tmat_amd import _lib, preprocessing, synth, zstacks
    h = _lib.Handle(None, 0)
    L = _lib.lib()
    lines = []

    Z, S = a.slices, a.size
    stacks = None
    if "a" in a.cases or "k" in a.cases:
        base = [synth.synth_stack(i, Z, S, S, n_vessels=16) for i in range(2)]
        stacks = np.stack([base[i % 2] for i in range(a.stacks)])
    if "a" in a.cases:
        def old_a():
            proj = np.stack([zstacks.proj_max(st, handle=h) for st in stacks])           # what the script did per stack
            return preprocessing.cell_area_batch(h, proj, 512, 0.0)
        compare("a", {"what": f"{a.stacks} stacks of {Z} x {S} x {S} u16 -> 512", "old": "proj_max per stack + cell_area_batch", "new": "cell_area_stacks"},
                a.stacks, "stacks", old_a, lambda: preprocessing.cell_area_stacks(h, stacks, 512, 0.0), a.rounds, lines, a.warmup)
    if "k" in a.cases:
        oh, ow = preprocessing.resized_shape((S, S), 512)
        n = a.stacks
        with preprocessing._DevBlock(h, stacks.nbytes) as src, preprocessing._DevBlock(h, n * oh * ow * 2) as small:
            _lib.check(L.tmat_dev_upload(h.raw, src.ptr, _lib.ptr(stacks), stacks.nbytes), "tmat_dev_upload")
            call = lambda: _lib.check(L.tmat_cell_small_dev(h.raw, src.ptr, n, Z, S, S, 16, oh, ow, small.ptr), "tmat_cell_small_dev")  # noqa: E731
            call()
            h.prof_enable(True)
            h.prof_read(reset=True)
            ms = []
            for _ in range(max(a.rounds, 5)):
                call()
                ms.append(h.prof_read(reset=True)[0])
            h.prof_enable(False)
        read = touched_rows(S, oh) * S * 2 * Z * n
        alg = read + n * oh * ow * 2
        med = float(np.median(ms))
        line = {"metric": f"cell_small_kernel alone: max projection + down-sampling of {n} resident stacks of {Z} x {S} x {S} u16 -> {oh} x {ow}",
                "value": med, "unit": "ms (HIP events around the kernel)", "n_gpus": 1, "steps": len(ms), "warmup": 1, "ms_per_step": med, "ms_rounds": ms,
                "ms_spread": max(ms) - min(ms), "higher_is_better": False, "data": "synthetic",
                "roofline": {"bound": "hbm", "bytes_must_read": read, "bytes_algorithm": alg, "source_rows_touched": touched_rows(S, oh), "source_rows": S,
                             "achieved": alg / (med / 1e3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / (med / 1e3) / 1e9 / HBM_PEAK_GBS,
                             "note": "kernel time only; bytes = rows the taps touch x W x 2 x Z x n + the output, computed from the shapes; peak = HBM3E spec"}}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if "d" in a.cases:
        # the combination the script also meets: Z stacks with -w.  The vignette of bench_well.well_image on every slice
        yy, xx = np.mgrid[0:S, 0:S]
        u, v = (xx - S * 0.51) / (S * 0.45), (yy - S * 0.49) / (S * 0.45)
        wst = []
        for i in range(2):
            st = synth.synth_stack(i, Z, S, S, n_vessels=16).astype(np.float32)
            inside = (u ** 2 + v ** 2 < 1) if i % 2 == 0 else (u ** 8 + v ** 8 < 1)
            wst.append(np.clip(np.where(inside[None], st + 12000.0, 0.0), 0, 65535).astype(np.uint16))
        wstacks = np.stack([wst[i % 2] for i in range(a.stacks)])

        def old_d():
            proj = np.stack([zstacks.proj_max(st, handle=h) for st in wstacks])
            return preprocessing.cell_area_batch_well(h, proj, 512, 0.0, 0)
        compare("d", {"what": f"{a.stacks} stacks of {Z} x {S} x {S} u16, --detect-well, -> 512", "old": "proj_max per stack + cell_area_batch_well",
                      "new": "cell_area_stacks(detect_well=True)"},
                a.stacks, "stacks", old_d, lambda: preprocessing.cell_area_stacks(h, wstacks, 512, 0.0, detect_well=True, well_seed=0), a.rounds, lines, a.warmup)
        wstacks = None
    stacks = None
    if "b" in a.cases:
        wimgs = np.stack([well_image(i) for i in range(8)])[np.arange(a.well_images) % 8]
        compare("b", {"what": f"{a.well_images} images of 1024^2 u16, --detect-well, -> 512", "old": "cell_area_batch_well", "new": "cell_area_stacks(detect_well=True)"},
                a.well_images, "images", lambda: preprocessing.cell_area_batch_well(h, wimgs, 512, 0.0, 0),
                lambda: preprocessing.cell_area_stacks(h, wimgs, 512, 0.0, detect_well=True, well_seed=0), a.rounds, lines, a.warmup)
    if "c" in a.cases:
        base = np.stack([synth.synth_image(i, 1024, n_vessels=40) for i in range(8)])
        imgs = base[np.arange(a.images) % 8]

        def batches(fn):
            res = [fn(imgs[i0:i0 + 64]) for i0 in range(0, a.images, 64)]
            return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
        compare("c", {"what": f"{a.images} plain images of 1024^2 u16 -> 512, batches of 64", "old": "cell_area_batch", "new": "cell_area_stacks"},
                a.images, "images", lambda: batches(lambda b: preprocessing.cell_area_batch(h, b, 512, 0.0)),
                lambda: batches(lambda b: preprocessing.cell_area_stacks(h, b, 512, 0.0)), a.rounds, lines, a.warmup)
    h.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(lines, indent=1) + "\n")


if __name__ == "__main__":
    main()

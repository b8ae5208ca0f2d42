#!/usr/bin/env python3
"""What the PNG encoder on the device buys.  Needs a GPU.  Prints one JSON line and, without --quick, writes
profiles/png_bench.json.

* per kind of picture -- the four stage pictures of 16 bench images (640 x 640 grey, out of analyze_batch_ex), 16 tree overlays at
  --vis-width (RGB) and one barcode: ms per picture of PIL's Image.save on one thread (how the files were made before), ms per picture
  on the device as HIP-event intervals on the handle's stream (upload, kernels, copy back: tmat_png_encode_batch_timed; one warm-up call,
  --repeats timed calls, medians), file size device / PIL, and bytes copied back / raw bytes.
* end to end on --n synthetic 1024 x 1024 images, --rounds alternating rounds, wall clock: (a) analyze_batch, (b) analyze_batch_ex with
  stage pictures saved through PIL, (c) the same saved through the device encoder, files written.  Reported: whether (c) beats (b) by
  more than (b)'s round-to-round spread, and whether encode + write per image in (c) is below (a)'s time per image.
* overlays: render_tree + PIL against render_tree_png + write, the same rounds.
* --merge-bench FILE: bench.py result lines of one session, each prefixed "parent " or "branch " (tools/bench_overlay.py:bench_series).
* --compact: the same report for the encoder's two modes (Handle.png_set_mode) side by side, written to profiles/png_compact_bench.json:
  per kind the two modes alternate call by call after one warm-up call each (medians of --repeats), every compact file is checked against
  the host twin's, and the end-to-end rounds run (c) once per mode -- (c) fast and (c) compact alternate in the same rounds.

    python tools/bench_png.py [--n 64] [--rounds 3] [--repeats 5] [--vis-width 2000] [--quick] [--compact]
"""
import argparse
import io
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd", REPO / "tools"):
    sys.path.insert(0, str(p))

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)


def pil_files(pics):
    from PIL import Image
    out, t0 = [], time.perf_counter()
    for p in pics:
        b = io.BytesIO()
        Image.fromarray(p).save(b, format="PNG")
        out.append(b.getvalue())
    return out, (time.perf_counter() - t0) * 1e3 / len(pics)


def kind_report(handle, pics, repeats, modes=("fast",)):
    """one kind of picture: PIL against the device, per picture.  One mode: the report itself; several: {mode: report}, the modes
    alternating call by call"""
    from PIL import Image
    from tmat_amd import _lib
    pil, pil_ms = pil_files(pics)
    files, runs = {}, {m: [] for m in modes}
    for m in modes:
        handle.png_set_mode(m)
        files[m], _ = handle.png_encode_timed(pics)                             # warm-up: pool blocks, code objects
    for _ in range(repeats):
        for m in modes:
            handle.png_set_mode(m)
            runs[m].append(handle.png_encode_timed(pics)[1])
    handle.png_set_mode("fast")
    n = len(pics)
    out = {}
    for m in modes:
        same = all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), p) for f, p in zip(files[m], pics))
        ms = {k: float(np.median([r[k] for r in runs[m]])) / n for k in ("upload", "kernels", "copy_back")}
        dev_bytes, pil_bytes = sum(map(len, files[m])), sum(map(len, pil))
        out[m] = dict(pictures=n, shape=list(pics.shape[1:]), pil_ms_per_picture=pil_ms, device_ms_per_picture=ms,
                      device_total_ms_per_picture=sum(ms.values()), file_size_device_over_pil=dev_bytes / pil_bytes,
                      bytes_copied_back_over_raw=dev_bytes / pics.nbytes, device_file_bytes_mean=dev_bytes / n, pil_file_bytes_mean=pil_bytes / n,
                      pillow_decodes_to_the_pictures=bool(same))
        if len(modes) > 1 and len(pics) <= 16:
            out[m]["equals_the_host_twin"] = bool(files[m] == _lib.host_png_encode(pics, mode=m))
            out[m]["pillow_decodes_to_the_pictures"] = bool(same and out[m]["equals_the_host_twin"])
    return out[modes[0]] if len(modes) == 1 else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--vis-width", type=int, default=2000)
    ap.add_argument("--quick", action="store_true", help="8 images, 2 repeats, overlays 600 wide, no file written")
    ap.add_argument("--merge-bench", type=str, default=None, metavar="FILE")
    ap.add_argument("--compact", action="store_true", help="fast and compact side by side; writes profiles/png_compact_bench.json")
    a = ap.parse_args()
    if a.quick:
        a.n, a.repeats, a.vis_width = 8, 2, 600
    from bench_overlay import bench_series
    from make_goldens import synth_field
    from tmat_amd import _lib, branches, synth
    from tmat_amd.topology import MorseGraph

    distinct = [synth.synth_image(i, 1024) for i in range(min(16, a.n))]
    imgs = np.stack([distinct[i % len(distinct)] for i in range(a.n)])
    field = synth_field(33, (384, 384))
    segs, sb, bars = MorseGraph(field, thresholds=(5, 10), min_branch_length=5, smoothing_window=5).colored_tree(1.0)
    n_ov = min(16, a.n)
    bgs = np.stack([(field * (200 + i)).astype(np.uint16) for i in range(n_ov)])
    trees = [(segs, sb)] * n_ov
    handle = _lib.Handle(synth.pack_weights(synth.synth_weights(0)), 0, 0)
    res = dict(stripe_bytes=_lib.png_stripe(), images=a.n, rounds=a.rounds, vis_width=a.vis_width)
    ok = True
    modes = ("fast", "compact") if a.compact else ("fast",)

    def all_decode(report):
        return all(r["pillow_decodes_to_the_pictures"] for r in (report.values() if a.compact else [report]))
    try:
        # ---- per kind of picture ----
        _, ex = branches.analyze_batch_ex(handle, imgs[:n_ov], CFG, 500.0, stage_pictures=True)
        stage = np.ascontiguousarray(ex["pictures"]).reshape((-1,) + ex["pictures"].shape[2:])
        overlays = handle.render_tree(bgs, trees, a.vis_width)
        kinds = dict(stage_pictures=kind_report(handle, stage, a.repeats, modes), overlays=kind_report(handle, overlays, a.repeats, modes),
                     barcode=kind_report(handle, _lib.host_render_barcode(bars, a.vis_width)[None], a.repeats, modes))
        for name, plane in zip(_lib.STAGE_PLANES, range(4)):
            kinds["stage_" + name] = kind_report(handle, np.ascontiguousarray(stage[plane::4]), a.repeats if a.compact else max(2, a.repeats // 2), modes)
        res["kinds"] = kinds
        ok = all(all_decode(k) for k in kinds.values())

        # ---- end to end ----
        enc_write = []

        def form_a(d):
            return branches.analyze_batch(handle, imgs, CFG, 500.0)

        def form_b(d):
            rows, e = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, stage_pictures=True)
            for i in range(a.n):
                branches.save_stage_pictures(e["pictures"][i], Path(d) / f"img_{i}")
            return rows

        file_bytes = {}

        def form_c(d, mode="fast"):
            handle.png_set_mode(mode)
            rows, e = branches.analyze_batch_ex(handle, imgs, CFG, 500.0, stage_pictures=True)
            t0 = time.perf_counter()
            items = []
            for i in range(a.n):
                items += branches.stage_picture_items(e["pictures"][i], Path(d) / f"img_{i}")
            branches.write_png_batch(items, handle.png_encode)
            if mode == "fast":
                enc_write.append(time.perf_counter() - t0)
            handle.png_set_mode("fast")
            file_bytes[mode] = sum(p.stat().st_size for p in Path(d).rglob("*.png"))
            return rows

        def form_c_compact(d):
            return form_c(d, "compact")

        def rounds_of(forms):
            times, rows = {k: [] for k, _ in forms}, {}
            with tempfile.TemporaryDirectory() as d:
                for k, f in forms:
                    f(Path(d) / f"warm_{k}")
                enc_write.clear()
                for r in range(a.rounds):
                    for k, f in forms:
                        t0 = time.perf_counter()
                        rows[k] = f(Path(d) / f"r{r}_{k}")
                        times[k].append(time.perf_counter() - t0)
                    print(f"[bench_png] round {r + 1}/{a.rounds}: " + ", ".join(f"({k}) {times[k][-1]:.3f} s" for k, _ in forms), file=sys.stderr, flush=True)
            return times, rows

        times, rows = rounds_of((("a", form_a), ("b", form_b), ("c", form_c)) + ((("c_compact", form_c_compact),) if a.compact else ()))
        med = {k: float(np.median(v)) for k, v in times.items()}
        b_spread = max(times["b"]) - min(times["b"])
        ew_ms = 1e3 * float(np.median(enc_write)) / a.n
        a_ms = 1e3 * med["a"] / a.n
        e2e = dict(a_s=times["a"], b_s=times["b"], c_s=times["c"], a_images_per_s=a.n / med["a"], b_images_per_s=a.n / med["b"],
                   c_images_per_s=a.n / med["c"], b_round_to_round_spread_s=b_spread, b_minus_c_median_s=med["b"] - med["c"],
                   c_faster_than_b_by_more_than_b_spread=bool(med["b"] - med["c"] > b_spread),
                   c_encode_and_write_ms_per_image=ew_ms, a_ms_per_image=a_ms, c_encode_and_write_below_a_per_image=bool(ew_ms < a_ms),
                   rows_equal=bool(rows["a"] == rows["b"] == rows["c"]))
        if ew_ms >= a_ms:
            k = kinds["stage_pictures"]
            parts = dict(k["device_ms_per_picture"], host_python_and_file_write=ew_ms / 4 - k["device_total_ms_per_picture"])
            e2e["largest_phase_of_the_rest"] = max(parts, key=parts.get)
        if a.compact:
            mc = float(np.median(times["c_compact"]))
            e2e.update(c_compact_s=times["c_compact"], c_compact_images_per_s=a.n / mc, b_minus_c_compact_median_s=med["b"] - mc,
                       c_compact_faster_than_b_by_more_than_b_spread=bool(med["b"] - mc > b_spread),
                       c_compact_minus_c_median_s=mc - med["c"], png_bytes_written=dict(file_bytes),
                       rows_equal=bool(e2e["rows_equal"] and rows["c_compact"] == rows["a"]))
        res["end_to_end"] = e2e
        ok = ok and e2e["rows_equal"]

        # ---- overlays ----
        def ov_pil(d):
            from PIL import Image
            d.mkdir(parents=True)
            for i, o in enumerate(handle.render_tree(bgs, trees, a.vis_width)):
                Image.fromarray(o, "RGB").save(d / f"morse_tree_{i}.png")

        def ov_dev(d, mode="fast"):
            d.mkdir(parents=True)
            handle.png_set_mode(mode)
            for i, f in enumerate(handle.render_tree_png(bgs, trees, a.vis_width)):
                (d / f"morse_tree_{i}.png").write_bytes(f)
            handle.png_set_mode("fast")

        def ov_dev_compact(d):
            ov_dev(d, "compact")

        t2, _ = rounds_of((("pil", ov_pil), ("device", ov_dev)) + ((("device_compact", ov_dev_compact),) if a.compact else ()))
        res["overlays_end_to_end"] = dict(overlays=n_ov, render_tree_plus_pil_s=t2["pil"], render_tree_png_plus_write_s=t2["device"],
                                          pil_ms_per_overlay=1e3 * float(np.median(t2["pil"])) / n_ov,
                                          device_ms_per_overlay=1e3 * float(np.median(t2["device"])) / n_ov)
        if a.compact:
            res["overlays_end_to_end"].update(render_tree_png_compact_plus_write_s=t2["device_compact"],
                                              device_compact_ms_per_overlay=1e3 * float(np.median(t2["device_compact"])) / n_ov)
    finally:
        handle.close()
    if a.merge_bench:
        res["bench_py_default_path"] = bench_series(a.merge_bench)
    if not a.quick:
        (REPO / "profiles" / ("png_compact_bench.json" if a.compact else "png_bench.json")).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

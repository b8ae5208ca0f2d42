#!/usr/bin/env python3
"""Smooth tiling around an identity predictor: the device session route (tmat_amd.smooth_tiled_predictions with handle=,
csrc/smooth_kernels.hip) against oracle/blend.py, the numpy restatement of the reference driver, on the same host.

    python tools/bench_smooth.py [--size 640] [--window 320] [--rounds 3] [--out profiles/smooth_bench.json]

Per subdivision count (2 and 4) the two routes alternate for `--rounds` rounds after one untimed round; wall times end after the
result is on the host (tmat_smooth_end synchronises).  Also reported: HIP-event times of the two kernels alone (the gather summed
over the session's launches, the blend's one launch) and the blend's fraction of its byte floor -- prediction bytes + 8 hh ww over
the measured HBM copy rate of the MI355X, 6.29 TB/s.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "tissue-model-analysis-tools_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_BYTES_PER_S = 6.29e12


def identity(batch, verbose=0):
    return np.asarray(batch)[..., None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--window", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import blend
    from tmat_amd import _lib, smooth_tiled_predictions as stp

    h = _lib.Handle(None, 0)
    img = np.random.RandomState(11).uniform(0, 1, (a.size, a.size)).astype(np.float32)
    res = {"image": [a.size, a.size], "window_size": a.window, "predictor": "identity", "rounds": a.rounds, "cases": []}
    try:
        for sub in (2, 4):
            n_tiles = _lib.smooth_plan(a.size, a.size, a.window, sub)[3]
            dev, host, tiles_ms, blend_ms = [], [], [], []
            same = None
            for r in range(a.rounds + 1):           # round 0 warms both routes up
                t0 = time.perf_counter()
                got = stp.predict_img_with_smooth_windowing(img, a.window, sub, identity, handle=h)
                t1 = time.perf_counter()
                ref = blend.predict_img_with_smooth_windowing(img, a.window, sub, identity)
                t2 = time.perf_counter()
                same = bool(np.array_equal(got.view(np.uint64), ref.view(np.uint64)))
                if r:
                    dev.append(t1 - t0); host.append(t2 - t1)
                    tm = h.smooth_times()
                    tiles_ms.append(tm[0]); blend_ms.append(tm[1])
            floor_s = (n_tiles * a.window * a.window * 4 + 8 * a.size * a.size) / HBM_BYTES_PER_S
            res["cases"].append({
                "subdivisions": sub, "n_tiles": n_tiles, "bit_equal_to_oracle_blend": same,
                "device_route_s": dev, "oracle_blend_s": host,
                "device_route_median_s": float(np.median(dev)), "oracle_blend_median_s": float(np.median(host)),
                "device_route_spread_s": max(dev) - min(dev), "oracle_blend_spread_s": max(host) - min(host),
                "speedup_of_medians": float(np.median(host) / np.median(dev)),
                "tiles_kernel_ms": tiles_ms, "blend_kernel_ms": blend_ms,
                "blend_byte_floor_ms": floor_s * 1e3,
                "blend_fraction_of_floor": float(floor_s * 1e3 / np.median(blend_ms)) if np.median(blend_ms) > 0 else None,
            })
    finally:
        h.close()
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()

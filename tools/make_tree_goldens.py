#!/usr/bin/env python3
"""Generate tests/golden/morse_tree.npz by IMPORTING the reference's MorseGraph (CPU only, generation time only): the segments,
per-segment branch indices and scaled bars that MorseGraph._MorseGraph__compute_colored_tree_and_barcode(scaling_factor) builds
(reference topology.py:358-389).  Only data is stored.

    /opt/conda/bin/python3.9 tools/make_tree_goldens.py      # numpy 1.26.4 = the reference's pin, as for the dmt / morse groups

Shims as in tools/make_goldens.py (numba.njit = identity, a cv2 stub).  __random_color is stubbed: without cv2 it cannot run, and under
numpy 2 its np.uint8([step * i, ...]) raises OverflowError from the fourth branch on; the colour is specified in include/tmat.h instead.
The numpy version is recorded in the file.  float32 vertices times a Python float stay float32 under numpy 1.x and numpy 2 alike, so
the segments do not depend on it; the barcode does (numpy 2 keeps its float32 scalars in float32, the pinned numpy 1.x promotes them to
float64, which is what tests/golden/morse.npz and tmat_morse_stats pin), so the fixture is generated under the pin.
"""
import sys

import numpy as np

import make_goldens as mg

# every case of the existing Morse goldens on these fields (pruning mask: cases 6, 7; remove_isolated: 4, 7) x two scaling factors
TREE_FIELDS = ["s96", "s_rect", "zero"]
TREE_SCALES = [("s640", 640 / 384), ("s1", 1.0)]


def tree_fields():
    f = {n: mg.synth_field(seed, shape) for n, seed, shape in mg.DMT_SYNTH if n in TREE_FIELDS}
    f["zero"] = np.zeros((24, 24), np.float32)
    return f


def main():
    mg._shims()
    from fl_tissue_model_tools.topology import MorseGraph
    MorseGraph._MorseGraph__random_color = staticmethod(lambda i: (0.0, 0.0, 0.0))
    out = {"numpy_version": np.array(np.__version__)}
    for name, f in tree_fields().items():
        for ci, (d1, d2, sw, mn, mx, iso, um) in enumerate(mg.MORSE_CASES):
            pm = mg.prune_mask(f.shape) if um else None
            for sname, sf in TREE_SCALES:
                g = MorseGraph(f, thresholds=(d1, d2), min_branch_length=mn, max_branch_length=mx, remove_isolated_branches=iso,
                               smoothing_window=sw, pruning_mask=pm)
                g._MorseGraph__compute_colored_tree_and_barcode(scaling_factor=sf)
                edges = [e for e, _ in g._edges_and_colors]
                segs = np.array([[*np.asarray(a, np.float64), *np.asarray(b, np.float64)] for a, b in edges], np.float64).reshape(-1, 4)
                # the branch of a segment: segments are appended branch by branch, len(branch) per branch (one per edge)
                sb = np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(g._branches)] + [np.zeros(0, np.int32)])
                assert len(sb) == len(segs)
                bars = np.array([b for b, _ in g._barcode_and_colors], np.float64).reshape(-1, 2)
                key = f"{name}_c{ci}_{sname}"
                out[key + "_segs"], out[key + "_branch"], out[key + "_bars"] = segs, sb, bars
                print(key, len(bars), len(segs), flush=True)
    np.savez_compressed(mg.GOLD / "morse_tree.npz", **out)
    print("morse_tree.npz", sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    sys.exit(main())

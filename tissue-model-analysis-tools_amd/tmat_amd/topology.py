"""Mirror of fl_tissue_model_tools.topology.MorseGraph (reference topology.py:15-144, 148-389).
The plotting methods draw the reference's matplotlib artists from the library's branch geometry (tmat_morse_tree); matplotlib is
imported inside them only."""
from __future__ import annotations

from numbers import Number
from typing import Optional, Tuple

import numpy as np

from . import _lib


class MorseGraph:
    """Morse skeleton of an image represented as a forest; exposes `.barcode`,
    `get_total_branch_length()`, `get_average_branch_length()`."""

    def __init__(self, img, thresholds: Tuple[Number, Number] = (1, 4), min_branch_length: int = 15,
                 max_branch_length: Optional[int] = None, remove_isolated_branches: bool = False,
                 smoothing_window: int = 15, pruning_mask=None, method=0, handle=None):
        """handle (optional, a _lib.Handle): run the DMT front end on its device (tmat_dmt_graph with a handle)"""
        img = np.asarray(img)
        self.thresholds = thresholds
        self.min_branch_length = min_branch_length
        self.max_branch_length = max_branch_length
        self.remove_isolated_branches = remove_isolated_branches
        self.smoothing_window = smoothing_window
        self.pruning_mask = pruning_mask
        self._shape = img.shape[:2]
        V, E = _lib.dmt_graph(img.astype(np.float32), thresholds[0], thresholds[1], handle=handle)
        self._dmt_vertices, self._dmt_edges = V, E
        bars, n, tot, avg = _lib.morse_stats(V, E, self._shape, smoothing_window, min_branch_length, max_branch_length,
                                             remove_isolated_branches, pruning_mask)
        self.barcode = [(float(b), float(d)) for b, d in bars]
        self._total, self._avg = tot, avg

    def get_total_branch_length(self) -> float:
        return self._total

    def get_average_branch_length(self) -> float:
        return self._avg

    def colored_tree(self, scaling_factor=1.0):
        """(segs (s, 4) f64 [x1, y1, x2, y2], seg_branch (s) i32, bars (k, 2) f64 scaled): topology.py:358-389 from tmat_morse_tree"""
        segs, sb, bars, _, _, _ = _lib.morse_tree(self._dmt_vertices, self._dmt_edges, self._shape, self.smoothing_window,
                                                  self.min_branch_length, self.max_branch_length, self.remove_isolated_branches,
                                                  self.pruning_mask, scaling_factor)
        return segs, sb, bars

    @staticmethod
    def _colors(idx):
        return [tuple(_lib.branch_color(int(i)) / 255) for i in idx]

    def plot_colored_barcode(self, scaling_factor=1.0, ax=None, **kwargs):
        """topology.py:67-107: ax.barh of the bars sorted by birth (descending), each in its branch's colour"""
        import matplotlib.pyplot as plt
        _, _, bars = self.colored_tree(scaling_factor)
        ax_provided = ax is not None
        ax = ax if ax_provided else plt.gca()
        order = sorted(range(len(bars)), key=lambda i: bars[i][0], reverse=True)
        heights = list(range(len(order)))
        widths = [bars[i][1] - bars[i][0] for i in order]
        births = [bars[i][0] for i in order]
        ax.barh(heights, widths, left=births, color=self._colors(order), **kwargs)
        ax.set_yticks([])
        ax.set_xlabel("Barcode")
        if not ax_provided:
            plt.show()

    def plot_colored_tree(self, scaling_factor=1.0, ax=None, **kwargs):
        """topology.py:109-144: a LineCollection of the smoothed branch segments, one colour per branch"""
        import matplotlib.pyplot as plt
        from matplotlib.collections import LineCollection
        segs, sb, _ = self.colored_tree(scaling_factor)
        ax_provided = ax is not None
        ax = ax if ax_provided else plt.gca()
        if len(segs):
            colors = [(*c, 1.0) for c in self._colors(sb)]
            ax.add_collection(LineCollection(segs.reshape(-1, 2, 2), colors=colors, **kwargs))
        ax.set_axis_off()
        ax.autoscale()
        if not ax_provided:
            plt.show()

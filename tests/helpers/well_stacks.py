"""Inputs of the Z-stack --detect-well / tree tests: small synthetic stacks whose vessels sit inside a bright well (the vignette of
tools/bench_well.py:well_image on every slice; even indices a round well, odd ones a rounded square).

With seed 0 and a width of 800 microns the oracle (oracle/wellmask.py on oracle/sato.py:resize_aa of the max projection) gives, for the
(3, 128, 160) stacks and their (307, 384) field:
    40     keeps a fitted mask (coverage 0.49, 70 568 pruning pixels); its rows differ with and without the mask
    41     ends all-true (the coverage rule, with its warning)
    42     keeps a fitted mask (coverage 0.64); its rows do not change
    blank  no hull: circle + disk(5) erosion, 8 802 pruning pixels
"""
import functools

import numpy as np

WIDTH_UM = 800.0
SEED = 0
CFG = {"graph_thresh_1": 5, "graph_thresh_2": 10, "graph_smoothing_window": 12, "min_branch_length": 12, "remove_isolated_branches": False}
PAIRS = [(5, 10), (2, 5)]


def well_stack(index, Z=3, H=128, W=160, n_vessels=8):
    from tmat_amd import synth
    st = synth.synth_stack(index, Z, H, W, n_vessels=n_vessels).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    u, v = (xx - W * 0.51) / (W * 0.45), (yy - H * 0.49) / (H * 0.45)
    inside = (u ** 2 + v ** 2 < 1) if index % 2 == 0 else (u ** 8 + v ** 8 < 1)
    return np.clip(np.where(inside[None], st + 12000.0, 0.0), 0, 65535).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def four_stacks():
    """[40, 41, 42, blank]: fit, rejection, fit without effect, fallback"""
    a = np.stack([well_stack(40), well_stack(41), well_stack(42), np.zeros((3, 128, 160), np.uint16)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def odd_stacks():
    """two (4, 150, 140) stacks: a (411, 384) field, no side a multiple of a tile"""
    a = np.stack([well_stack(50, 4, 150, 140), well_stack(51, 4, 150, 140)])
    a.setflags(write=False)
    return a


def px_params(width_um=WIDTH_UM):
    from tmat_amd import branches
    return branches.graph_px_params(CFG, 384, width_um)


@functools.lru_cache(maxsize=None)
def oracle_front(which):
    """per stack of four_stacks() / odd_stacks(): (resize_aa of the max projection, thresh_small, border_small, (well, shrunken))"""
    from oracle import sato as osato
    from oracle import wellmask as ow
    stacks = four_stacks() if which == "four" else odd_stacks()
    H, W = stacks.shape[2:]
    out_hw = tuple(int(v) for v in np.multiply((H, W), 384 / W).round().astype(int))
    res = []
    for st in stacks:
        aa = osato.resize_aa(st.max(0), out_hw)
        th = ow.auto_threshold_well(aa)
        ratio = min(1, 200 / np.max(th.shape))
        small = tuple(int(v) for v in np.round(np.asarray(th.shape) * ratio))
        ts = ow.resize_nearest(th, small)
        res.append((aa, ts, ow.border_of(ts), ow.make_well_mask(aa, seed=SEED)))
    return res

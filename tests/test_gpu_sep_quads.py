"""GPU: the quadrant form of the plain fused separable launches (sepconv_ws_kernel<..., QUAD>; TMAT_ROI_QUAD).

The kernel works in 8 x 8 quadrants: a producer wave owns one with its own halo, a consumer wave stores two rows of two of them.  In
quadrant form a launch visits ANY four quadrants as one packed tile (csrc/roi_plan.cpp:roi_sep_quad_table names them; the planner side is
tests/test_roi_sep_quads.py).  The per-pixel arithmetic is the tile form's, so a listed quadrant must equal the oracle's exact
depthwise -> pointwise chain (oracle/unet.py:_dw -> _conv, for the stem form behind orc_stem) bit for bit, and every word of a quadrant
that is not listed must keep what the caller put there.

Kernel-level cases go through tmat_debug_sepconv_quads with the caller's quadrant list: every quadrant in shuffled order (packed tiles
whose four slots are unrelated quadrants of different patches), a sparse list whose length is 1 mod 4 (the last group is padded with a
repeat), and the four border strips of every patch (every producer meets the zero padding on some side).  N = 3, 48 x 48 (6 x 6
quadrants a patch), 64 -> 128 and 256 channels (one and two channel tiles per packed tile), with and without ReLU on load, and the stem
form.  The pipeline-level cases run the whole network with the switch unset, 0 and 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
N, H, CIN = 3, 48, 64
QW = H // 8
QPP = QW * QW
FUSED_LAYERS = (1, 3, 7, 9)


def make_handle(weights, max_patches, roi, **env):
    """the switches are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_SHARE": None, "TMAT_ROI_CONST": None, "TMAT_ROI_DOWN": None, "TMAT_ROI_QUAD": None,
            "TMAT_ROI_SHARE_RECT": None, "TMAT_ROI_SHARE_FUSED_RECT": None, "TMAT_FUSED_SEP": None, "TMAT_FUSED_POOL": None,
            "TMAT_STEM_FUSED": None}
    want.update(env)
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return _lib.Handle(synth.pack_weights(weights), 0, max_patches)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def quad_lists():
    rs = np.random.RandomState(16)
    every = rs.permutation(N * QPP)
    # 13 = 1 mod 4; ordered by the position inside the patch, so that neighbours in the list (one group) come from different patches
    sparse = np.array(sorted(rs.choice(N * QPP, 13, replace=False), key=lambda q: (q % QPP, q)))
    groups = sparse[:12].reshape(3, 4) // QPP
    assert any(len(set(g)) > 1 for g in groups), "some group mixes patches"
    qy, qx = np.divmod(np.arange(QPP), QW)
    ring = np.flatnonzero((qy == 0) | (qy == QW - 1) | (qx == 0) | (qx == QW - 1))
    border = np.concatenate([n * QPP + ring for n in range(N)])
    return {"every": every, "sparse": sparse, "border": border}


LISTS = quad_lists()


@pytest.fixture(scope="module")
def handle(weights):
    h = make_handle(weights, 8, True)
    yield h
    h.close()


@pytest.fixture(scope="module")
def chains():
    """per (form, cout): the launch's operands and the oracle's result, computed once"""
    from oracle import unet as ou
    out = {}
    rs = np.random.RandomState(48)
    for form in ("plain", "relu_in", "stem"):
        for cout in (128, 256):
            dw9 = rs.normal(0, 0.4, (9, CIN)).astype(np.float32)
            pw = rs.normal(0, 0.2, (CIN, cout)).astype(np.float32)
            scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
            shift = rs.normal(0, 0.3, cout).astype(np.float32)
            if form == "stem":
                x = rs.uniform(0, 1, (N, 2 * H, 2 * H)).astype(np.float32)
                stem = (rs.normal(0, 0.5, (9, CIN)).astype(np.float32), rs.uniform(0.5, 1.5, CIN).astype(np.float32),
                        rs.normal(0, 0.3, CIN).astype(np.float32))
                a = np.empty((N, H, H, CIN), np.float32)
                ou.lib().orc_stem(ou._p(x), N, 2 * H, 2 * H, ou._p(stem[0]), CIN, ou._p(stem[1]), ou._p(stem[2]), ou._p(a))
            else:
                x = rs.normal(0, 1, (N, H, H, CIN)).astype(np.float32)
                stem, a = None, x
            relu_in = form == "relu_in"
            ref = ou._conv(ou._dw(a, dw9, int(relu_in)), pw, 1, 1, 0, 0, scale, shift, None, 0, 1)
            assert not np.isnan(ref).any() and (ref > 0).any()
            out[(form, cout)] = dict(x=x, dw9=dw9, pw=pw, scale=scale, shift=shift, stem=stem, relu_in=relu_in, ref=ref)
    return out


@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("cout", (128, 256))
@pytest.mark.parametrize("form", ("plain", "relu_in", "stem"))
def test_listed_quadrants_equal_the_oracle_and_the_rest_is_untouched(handle, chains, form, cout, which):
    c = chains[(form, cout)]
    quads = LISTS[which]
    listed = np.zeros(N * QPP, bool)
    listed[quads] = True
    # (n, qy, 8, qx, 8, cout) view: quadrant (n, qy, qx) is [n, qy, :, qx, :, :]
    mask = np.broadcast_to(listed.reshape(N, QW, 1, QW, 1, 1), (N, QW, 8, QW, 8, cout)).reshape(N, H, H, cout)
    ref = c["ref"].view(np.uint32)
    for pattern in (0xFF, 0x7F):
        handle.debug_poison(pattern)
        sentinel = np.uint32(pattern * 0x01010101)
        out = np.full((N, H, H, cout), sentinel, np.uint32).view(np.float32)
        handle.debug_sepconv_quads(c["x"], c["dw9"], c["pw"], c["scale"], c["shift"], quads, out, relu_in=c["relu_in"], relu_out=True,
                                   stem=c["stem"])
        got = out.view(np.uint32)
        nbad = int((got[mask] != ref[mask]).sum())
        ntouched = int((got[~mask] != sentinel).sum())
        print(f"{form}, cout {cout}, {which} ({len(quads)} quadrants), pattern {pattern:#x}: {nbad} listed words differ, {ntouched} other words written")
        assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {int(mask.sum())} words of the listed quadrants differ from the oracle"
        assert ntouched == 0, f"pattern {pattern:#x}: {ntouched} words outside the listed quadrants were written"


def test_launcher_refusals(handle, chains):
    from tmat_amd import _lib
    c = chains[("plain", 128)]
    out = np.zeros((N, H, H, 128), np.float32)
    for bad in ([N * QPP], [-1], [0, 1, 2, N * QPP + 5], []):
        with pytest.raises(_lib.TmatError):
            handle.debug_sepconv_quads(c["x"], c["dw9"], c["pw"], c["scale"], c["shift"], bad, out)
    assert not out.any(), "a refused call launches nothing"


def test_analyze_batch_quad_equals_full_frame(weights):
    """the 250 x 300 source of test_gpu_roi_sep.py through the whole pipeline: rows equal with the switch unset, 0 and 1; the pipeline
    runs the quadrant form unless the switch is 0, and then visits fewer packed tiles in the two plain launches"""
    from tmat_amd import branches, synth
    odd = synth.synth_image(40, 300, n_vessels=10, scale=1.0)[:250]
    imgs = np.stack([odd, odd[::-1]])
    h0 = make_handle(weights, 64, False)
    try:
        rows0 = branches.analyze_batch(h0, imgs, CFG, 300.0)
    finally:
        h0.close()
    visited = {}
    for setting in (None, "0", "1"):
        h1 = make_handle(weights, 64, True, TMAT_ROI_QUAD=setting)
        try:
            held = None
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, imgs, CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_QUAD={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            visited[setting] = h1.debug_sep_tiles()
        finally:
            h1.close()
    print("visited (planned, full) per fused launch:", visited)
    assert visited[None] == visited["1"]
    for i, (a, b) in enumerate(zip(visited[None], visited["0"])):
        assert a[1] == b[1]
        if FUSED_LAYERS[i] % 6 == 1:
            assert a[0] < b[0], "unset visits fewer packed tiles than TMAT_ROI_QUAD=0"
        else:
            assert a == b, "the pooled launches keep their tile tables"


def test_predict_smooth_quad_equals_full_frame(weights):
    """320 x 320, 3 images per pass, 4 images (the last pass holds one): bitwise the whole-patch prediction, and the launches of the last
    pass visit the quadrant tables (plain layers) and the share form's tile tables (pooled layers)"""
    from tmat_amd import _lib
    hh = ww = 320
    per_pass, n = 3, 4
    rs = np.random.RandomState(1016)
    x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
    h0 = make_handle(weights, 72 * per_pass, False)
    try:
        full = h0.predict_smooth(x)
    finally:
        h0.close()
    assert not np.isnan(full).any()
    # (predict_smooth runs the shared-interior form only with the constant-ring form switched on as well)
    h1 = make_handle(weights, 72 * per_pass, True, TMAT_ROI_SHARE="1", TMAT_ROI_CONST="1", TMAT_ROI_QUAD="1")
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint32) != full.view(np.uint32)).sum())
            print(f"TMAT_ROI_QUAD=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
        k_last = n % per_pass or per_pass
        want = []
        for layer in FUSED_LAYERS:
            if layer % 6 == 1:
                _, own, _, tfull = _lib.roi_sep_quads(hh, ww, layer, k_last)
                want.append(((own + 3) // 4, tfull))
            else:
                ids, tfull = _lib.roi_sep_tiles_share(hh, ww, layer, k_last)
                want.append((len(ids), tfull))
        got_tiles = h1.debug_sep_tiles()
        print("fused launches (planned, full):", got_tiles, "tile tables:", [len(_lib.roi_sep_tiles_share(hh, ww, l, k_last)[0]) for l in FUSED_LAYERS])
        assert got_tiles == want
    finally:
        h1.close()

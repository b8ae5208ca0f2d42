"""GPU: the quadrant form of the POOLED fused separable launches (sepconv_ws_kernel<.., POOL, .., QUAD>, pool_fix_add_quad_kernel;
TMAT_ROI_QUAD_POOL).

In quadrant form the pooled launch visits any four 8 x 8 quadrants as one packed tile (csrc/roi_plan.cpp:roi_sep_quad_pool_table names
them; the planner side is tests/test_roi_sep_quads_pool.py).  Its epilogue pools inside a quadrant, leaves the quadrant's last pooled
row and column as partial maxima and writes the quadrant's own strips; the fix-up launch completes the 7 boundary pixels per quadrant.
The arithmetic is the tile form's (the maxima in another grouping, the residual added once behind the last one), so a pooled pixel whose
window lies in listed quadrants, or beyond the patch where TF pads with -inf, must equal the oracle's exact chain -- oracle/unet.py:_dw ->
_conv, then orc_maxpool_add (MaxPooling2D(3, 2, "same") + residual) -- bit for bit.

Kernel-level cases go through tmat_debug_sepconv_pool_quads with the caller's quadrant list: every quadrant in shuffled order (the
whole pooled tensor then equals the oracle), a sparse list of 13 that mixes patches inside a packed group (the last group is padded with
a repeat), and the four border strips of every patch (no neighbour below the last row and right of the last column).  N = 3, 48 x 48
(3 x 3 tiles, 6 x 6 quadrants a patch), 128 -> 128 channels (one channel tile, four steps) and 256 -> 256 (two channel tiles, eight
steps), with and without ReLU on load.  The pipeline-level cases run the whole network with the switch unset, 0 and 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12,
           remove_isolated_branches=False)
N, H = 3, 48
QW = H // 8
QPP = QW * QW
HP = H // 2
FUSED_LAYERS = (1, 3, 7, 9)


def make_handle(weights, max_patches, roi, **env):
    """the switches are read at tmat_create"""
    from tmat_amd import synth, _lib
    want = {"TMAT_ROI": "1" if roi else "0", "TMAT_ROI_SHARE": None, "TMAT_ROI_CONST": None, "TMAT_ROI_DOWN": None, "TMAT_ROI_QUAD": None,
            "TMAT_ROI_QUAD_POOL": None, "TMAT_ROI_SHARE_RECT": None, "TMAT_ROI_SHARE_FUSED_RECT": None, "TMAT_FUSED_SEP": None,
            "TMAT_FUSED_POOL": None, "TMAT_STEM_FUSED": None}
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
    rs = np.random.RandomState(17)
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


def pixel_sets(quads):
    """per pooled pixel (N, HP, HP): its window lies in listed quadrants or beyond the patch; it is a non-boundary pixel of an unlisted quadrant"""
    listed = np.zeros((N, QW, QW), bool)
    listed.reshape(-1)[quads] = True
    p = np.arange(HP)
    # the quadrant rows (columns) under the window 2 p .. 2 p + 2 of pooled row (column) p, cut to the patch
    lo, hi = (2 * p) // 8, np.minimum(2 * p + 2, H - 1) // 8
    complete = np.ones((N, HP, HP), bool)
    for a in (lo, hi):
        for b in (lo, hi):
            complete &= listed[:, a[:, None], b[None, :]]
    own = listed[:, p[:, None] // 4, p[None, :] // 4]
    inner = ((p % 4) != 3)[:, None] & ((p % 4) != 3)[None, :]
    untouched = ~own & inner[None]
    return complete, untouched


@pytest.fixture(scope="module")
def handle(weights):
    h = make_handle(weights, 8, True)
    yield h
    h.close()


@pytest.fixture(scope="module")
def chains():
    """per (channels, relu_in): the launch's operands and the oracle's result, computed once"""
    from oracle import unet as ou
    out = {}
    rs = np.random.RandomState(49)
    for ch in (128, 256):
        for relu_in in (False, True):
            x = rs.normal(0, 1, (N, H, H, ch)).astype(np.float32)
            dw9 = rs.normal(0, 0.4, (9, ch)).astype(np.float32)
            pw = rs.normal(0, 0.1, (ch, ch)).astype(np.float32)
            scale = rs.uniform(0.5, 1.5, ch).astype(np.float32)
            shift = rs.normal(0, 0.3, ch).astype(np.float32)
            resid = rs.normal(0, 1, (N, HP, HP, ch)).astype(np.float32)
            p2 = ou._conv(ou._dw(x, dw9, int(relu_in)), pw, 1, 1, 0, 0, scale, shift, None, 0, 0)
            ref = np.empty((N, HP, HP, ch), np.float32)
            ou.lib().orc_maxpool_add(ou._p(p2), N, H, H, ch, ou._p(resid), ou._p(ref))
            assert not np.isnan(ref).any()
            out[(ch, relu_in)] = dict(x=x, dw9=dw9, pw=pw, scale=scale, shift=shift, resid=resid, relu_in=relu_in, ref=ref)
    return out


@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("relu_in", (False, True))
@pytest.mark.parametrize("ch", (128, 256))
def test_pooled_pixels_equal_the_oracle_and_the_rest_is_untouched(handle, chains, ch, relu_in, which):
    c = chains[(ch, relu_in)]
    quads = LISTS[which]
    complete, untouched = pixel_sets(quads)
    if which == "every":
        assert complete.all() and not untouched.any()
    else:
        assert complete.any() and untouched.any()
    ref = c["ref"].view(np.uint32)
    for pattern in (0xFF, 0x7F):
        handle.debug_poison(pattern)
        sentinel = np.uint32(pattern * 0x01010101)
        out = np.full((N, HP, HP, ch), sentinel, np.uint32).view(np.float32)
        handle.debug_sepconv_pool_quads(c["x"], c["dw9"], c["pw"], c["scale"], c["shift"], c["resid"], quads, out, relu_in=relu_in, relu_out=False)
        got = out.view(np.uint32)
        nbad = int((got[complete] != ref[complete]).sum())
        ntouched = int((got[untouched] != sentinel).sum())
        print(f"{ch} channels, relu_in {relu_in}, {which} ({len(quads)} quadrants), pattern {pattern:#x}: {nbad} words of "
              f"{int(complete.sum())} complete pixels differ, {ntouched} words of {int(untouched.sum())} untouched pixels written")
        assert nbad == 0, f"pattern {pattern:#x}: {nbad} words of the complete pooled pixels differ from the oracle"
        assert ntouched == 0, f"pattern {pattern:#x}: {ntouched} words of unlisted quadrants' inner pixels were written"


def test_launcher_refusals(handle, chains):
    from tmat_amd import _lib
    c = chains[(128, False)]
    out = np.zeros((N, HP, HP, 128), np.float32)
    for bad in ([N * QPP], [-1], [0, 1, 2, N * QPP + 5], []):
        with pytest.raises(_lib.TmatError):
            handle.debug_sepconv_pool_quads(c["x"], c["dw9"], c["pw"], c["scale"], c["shift"], c["resid"], bad, out)
    assert not out.any(), "a refused call launches nothing"


def test_switch_refusals(weights):
    from tmat_amd import _lib
    for bad in ("2", "-1", "x", ""):
        with pytest.raises(_lib.TmatError):
            make_handle(weights, 8, True, TMAT_ROI_QUAD_POOL=bad)


def test_analyze_batch_quad_pool_equals_full_frame(weights):
    """the 250 x 300 pair of test_gpu_sep_quads.py through the whole pipeline: rows equal with the switch unset, 0 and 1; the pipeline
    runs the pooled quadrant form unless the switch is 0, and then visits fewer packed tiles in the two pooled launches"""
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
        h1 = make_handle(weights, 64, True, TMAT_ROI_QUAD_POOL=setting)
        try:
            held = None
            for pattern in (0xFF, 0x7F):
                h1.debug_poison(pattern)
                rows1 = branches.analyze_batch(h1, imgs, CFG, 300.0)
                assert [r[1:] for r in rows1] == [r[1:] for r in rows0], f"TMAT_ROI_QUAD_POOL={setting}, pattern {pattern:#x}"
                if held is None:
                    held = h1.debug_held_bytes()
                else:
                    assert h1.debug_held_bytes() == held, "held bytes change between calls"
            visited[setting] = (h1.debug_sep_tiles(), held)
        finally:
            h1.close()
    print("visited (planned, full) per fused launch, held bytes:", visited)
    assert visited[None] == visited["1"]
    assert visited[None][1] == visited["0"][1], "the handle holds the same bytes under every setting"
    for i, (a, b) in enumerate(zip(visited[None][0], visited["0"][0])):
        assert a[1] == b[1]
        if FUSED_LAYERS[i] % 6 == 3:
            assert a[0] < b[0], "unset visits fewer packed tiles than TMAT_ROI_QUAD_POOL=0"
        else:
            assert a == b, "the plain launches do not depend on the switch"


def test_predict_smooth_quad_pool_equals_full_frame(weights):
    """320 x 320, 3 images per pass, 4 images (the last pass holds one): bitwise the whole-patch prediction, and the pooled launches of
    the last pass report the packed tiles of the pooled quadrant tables (the plain ones the share form's tile tables: TMAT_ROI_QUAD is
    unset, and predict_smooth runs no form whose switch is unset)"""
    from tmat_amd import _lib
    hh = ww = 320
    per_pass, n = 3, 4
    rs = np.random.RandomState(1017)
    x = np.stack([rs.uniform(0.1 * i, 1, (hh, ww)) for i in range(n)]).astype(np.float32)
    h0 = make_handle(weights, 72 * per_pass, False)
    try:
        full = h0.predict_smooth(x)
    finally:
        h0.close()
    assert not np.isnan(full).any()
    h1 = make_handle(weights, 72 * per_pass, True, TMAT_ROI_SHARE="1", TMAT_ROI_CONST="1", TMAT_ROI_QUAD_POOL="1")
    try:
        for pattern in (0xFF, 0x7F):
            h1.debug_poison(pattern)
            got = h1.predict_smooth(x)
            nbad = int((got.view(np.uint32) != full.view(np.uint32)).sum())
            print(f"TMAT_ROI_QUAD_POOL=1, pattern {pattern:#x}: {nbad} of {got.size} words differ from the full-frame run")
            assert not np.isnan(got).any(), f"pattern {pattern:#x}: NaN in the prediction"
            assert nbad == 0, f"pattern {pattern:#x}: {nbad} of {got.size} differ, max |d| = {np.abs(got - full).max()}"
        k_last = n % per_pass or per_pass
        want = []
        for layer in FUSED_LAYERS:
            if layer % 6 == 3:
                _, own, _, tfull = _lib.roi_sep_quads_pool(hh, ww, layer, k_last)
                want.append(((own + 3) // 4, tfull))
            else:
                ids, tfull = _lib.roi_sep_tiles_share(hh, ww, layer, k_last)
                want.append((len(ids), tfull))
        got_tiles = h1.debug_sep_tiles()
        print("fused launches (planned, full):", got_tiles, "tile tables:", [len(_lib.roi_sep_tiles_share(hh, ww, l, k_last)[0]) for l in FUSED_LAYERS])
        assert got_tiles == want
    finally:
        h1.close()

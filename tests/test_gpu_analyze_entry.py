"""GPU: the nine entry points of the 2-D batch analysis family (tmat_analyze_batch, _dev, _masked, _tree, _tree_dev, _ex, _ex_dev, _grid,
_grid_dev) share one argument check and one path: every entry refuses the same bad arguments before it allocates or writes anything,
and a host entry computes what its device twin computes."""
import ctypes as C

import numpy as np
import pytest

from tmat_amd import _lib, branches, synth

pytestmark = pytest.mark.gpu

CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12, remove_isolated_branches=False)
PAIR = (5.0, 10.0)
VIS = 100
GUARD = 0xA5
# name -> (kind, images on the device); the kind decides the argument list
ENTRIES = {
    "tmat_analyze_batch": ("plain", False), "tmat_analyze_batch_dev": ("plain", True), "tmat_analyze_batch_masked": ("masked", False),
    "tmat_analyze_batch_tree": ("tree", False), "tmat_analyze_batch_tree_dev": ("tree", True),
    "tmat_analyze_batch_ex": ("ex", False), "tmat_analyze_batch_ex_dev": ("ex", True),
    "tmat_analyze_batch_grid": ("grid", False), "tmat_analyze_batch_grid_dev": ("grid", True),
}
HOST_TWINS = ("tmat_analyze_batch", "tmat_analyze_batch_tree", "tmat_analyze_batch_ex")


@pytest.fixture(scope="module")
def model(weights):
    """one model handle for the module: 72 patches, two 256 x 256 images (32 patches each) in one pass"""
    h = _lib.Handle(synth.pack_weights(weights), 0, 72)
    yield h
    h.close()


@pytest.fixture(scope="module")
def images():
    return np.stack([synth.synth_image(200 + i, 256, n_vessels=3, scale=1.0) for i in range(2)])


class DevImages:
    """a copy of imgs in device memory (tmat_dev_alloc), freed on exit"""

    def __init__(self, handle, imgs):
        self.handle, self.imgs, self.ptr = handle, np.ascontiguousarray(imgs), C.c_void_p()

    def __enter__(self):
        L = _lib.lib()
        _lib.check(L.tmat_dev_alloc(self.handle.raw, self.imgs.nbytes, C.byref(self.ptr)), "tmat_dev_alloc")
        _lib.check(L.tmat_dev_upload(self.handle.raw, self.ptr, _lib.ptr(self.imgs), self.imgs.nbytes), "tmat_dev_upload")
        return self.ptr

    def __exit__(self, *exc):
        _lib.lib().tmat_dev_free(self.handle.raw, self.ptr)


def outputs(n, H, W, stage=True, cap_b=64):
    """every output buffer an entry can write for n (H, W) images at one pair, filled with a pattern"""
    (hh, ww), _ = branches._shapes(H, W, 0.625)
    vh, vw = _lib.tree_canvas_shape(hh, ww, VIS)
    out = {"rows": (_lib.Row * n)(), "rgb": np.full((n, vh, vw, 3), GUARD, np.uint8), "bars": np.full((n, cap_b, 2), -7.0),
           "n_bars": np.full(n, -7, np.int32)}
    if stage:
        out["pictures"] = np.full((n, 4, hh, ww), GUARD, np.uint8)
    for r in out["rows"]:
        r.index, r.count, r.total_px, r.avg_px = -7, -7, -7.0, -7.0
    return out


def row_tuples(out):
    return [(r.index, r.count, r.total_px, r.avg_px) for r in out["rows"]]


def untouched(out):
    return (all(r == (-7, -7, -7.0, -7.0) for r in row_tuples(out)) and bool((out["rgb"] == GUARD).all()) and bool((out["bars"] == -7.0).all())
            and bool((out["n_bars"] == -7).all()) and ("pictures" not in out or bool((out["pictures"] == GUARD).all())))


def call(name, handle, imgs_ptr, shape, out, **bad):
    """entry `name` with valid arguments for images of `shape` and the buffers of `out` (ex / grid: tree and, when out has them, stage
    pictures requested), except what `bad` overrides: imgs, rows, n, H, W, ds_width, vis_width, rgb_out, bars_out, cap_b, n_bars"""
    L = _lib.lib()
    kind = ENTRIES[name][0]
    sw_px, min_px, max_px = branches.graph_px_params(CFG, 384, 500.0)
    a = dict(imgs=imgs_ptr, rows=out["rows"], n=shape[0], H=shape[1], W=shape[2], ds_width=384, vis_width=VIS, rgb_out=_lib.ptr(out["rgb"]),
             bars_out=_lib.ptr(out["bars"]), cap_b=out["bars"].shape[1], n_bars=_lib.ptr(out["n_bars"]))
    a.update(bad)
    fn = getattr(L, name)
    if kind in ("plain", "masked", "tree"):
        args = [handle.raw, a["imgs"], a["n"], a["H"], a["W"], 0.625, a["ds_width"], PAIR[0], PAIR[1], int(sw_px), int(min_px), int(max_px or 0), 0, 0]
        args += [None, None] if kind == "masked" else []
        args += [a["rows"]]
        args += [a["vis_width"], a["rgb_out"], a["bars_out"], a["cap_b"], a["n_bars"]] if kind == "tree" else []
        return fn(*args)
    as_int = lambda p: None if p is None else C.cast(p, C.c_void_p).value       # noqa: E731
    o = _lib.AnalyzeOpts(size=C.sizeof(_lib.AnalyzeOpts), ds_ratio=0.625, ds_width=a["ds_width"], graph_thresh_1=PAIR[0], graph_thresh_2=PAIR[1],
                         smoothing_window_px=int(sw_px), min_branch_length_px=int(min_px), max_branch_length_px=int(max_px or 0), remove_isolated=0,
                         first_index=0, vis_width=a["vis_width"], rgb_out=as_int(a["rgb_out"]), bars_out=as_int(a["bars_out"]), cap_b=a["cap_b"],
                         n_bars=as_int(a["n_bars"]), stage_out=out["pictures"].ctypes.data if "pictures" in out else None)
    if kind == "ex":
        return fn(handle.raw, a["imgs"], a["n"], a["H"], a["W"], C.byref(o), a["rows"])
    thresh = np.array([PAIR], np.float32)
    g = _lib.GridOpts(size=C.sizeof(_lib.GridOpts), n_thresh=1, thresh=thresh.ctypes.data)
    return fn(handle.raw, a["imgs"], a["n"], a["H"], a["W"], C.byref(o), C.byref(g), a["rows"])


def test_every_entry_refuses_the_same_bad_arguments(model, images):
    L = _lib.lib()
    small = np.zeros((2, 64, 64), np.uint16)
    plain = _lib.Handle(None, 0)
    corruptions = [(k, "any") for k in (dict(imgs=None), dict(rows=None), dict(n=-1), dict(H=0), dict(H=-1), dict(W=0), dict(ds_width=0))]
    corruptions += [(k, "tree request") for k in (dict(vis_width=0), dict(bars_out=None), dict(cap_b=-1), dict(n_bars=None))]
    corruptions += [(dict(rgb_out=None), "tree"), (dict(handle=plain), "any")]
    try:
        with DevImages(model, small) as dptr:
            for name, (kind, dev) in ENTRIES.items():
                ptr = dptr if dev else _lib.ptr(small)
                for bad, where in corruptions:
                    if (where == "tree request" and kind not in ("tree", "ex", "grid")) or (where == "tree" and kind != "tree"):
                        continue
                    bad = dict(bad)
                    h = bad.pop("handle", model)
                    out = outputs(2, 64, 64)
                    held = h.debug_held_bytes()
                    rc = call(name, h, ptr, small.shape, out, **bad)
                    msg = L.tmat_last_error() or b""
                    assert rc == _lib.E_ARG, (name, bad, rc)
                    assert msg.startswith(name.encode() + b":"), (name, bad, msg)
                    assert untouched(out), (name, bad)
                    assert h.debug_held_bytes() == held, (name, bad, "refused after an allocation")
                # no image: nothing to do, nothing written
                out = outputs(2, 64, 64)
                held = model.debug_held_bytes()
                assert call(name, model, ptr, (0, 64, 64), out) == 0, name
                assert untouched(out) and model.debug_held_bytes() == held, name
            for name in HOST_TWINS:         # ... but no image does not excuse the other arguments
                out = outputs(2, 64, 64)
                assert call(name, model, _lib.ptr(small), (0, 64, 64), out, H=-1) == _lib.E_ARG, name
                assert (L.tmat_last_error() or b"").startswith(name.encode() + b":") and untouched(out), name
    finally:
        plain.close()
    # the handle still works
    _lib.check(L.tmat_set_input_depth(model.raw, 16), "tmat_set_input_depth")
    out = outputs(2, 256, 256)
    assert call("tmat_analyze_batch", model, _lib.ptr(images), images.shape, out) == 0, L.tmat_last_error()
    assert [r[0] for r in row_tuples(out)] == [0, 1] and all(r[1] >= 0 for r in row_tuples(out))


def test_host_and_device_twins_agree(model, images):
    L = _lib.lib()
    _lib.check(L.tmat_set_input_depth(model.raw, 16), "tmat_set_input_depth")
    got = {}
    with DevImages(model, images) as dptr:
        for name, (kind, dev) in ENTRIES.items():
            if kind == "masked":
                continue
            out = outputs(2, 256, 256, stage=kind in ("ex", "grid"))
            assert call(name, model, dptr if dev else _lib.ptr(images), images.shape, out) == 0, (name, L.tmat_last_error())
            got[name] = out
    rows = row_tuples(got["tmat_analyze_batch"])
    print("rows", rows)
    assert sum(r[1] for r in rows) > 0, "the images should contain a branch"
    assert (got["tmat_analyze_batch_tree"]["n_bars"] == [r[1] for r in rows]).all()

    def same(a, b, keys):
        assert row_tuples(got[a]) == row_tuples(got[b]), (a, b)
        for k in keys:
            assert np.array_equal(got[a][k], got[b][k]), (a, b, k)
    tree, full = ("rgb", "bars", "n_bars"), ("rgb", "bars", "n_bars", "pictures")
    same("tmat_analyze_batch", "tmat_analyze_batch_dev", ())
    same("tmat_analyze_batch_tree", "tmat_analyze_batch_tree_dev", tree)
    same("tmat_analyze_batch_ex", "tmat_analyze_batch_ex_dev", full)
    same("tmat_analyze_batch_grid", "tmat_analyze_batch_grid_dev", full)
    same("tmat_analyze_batch_grid", "tmat_analyze_batch_ex", full)
    # and across the forms: the tree form's rows are the plain form's, the ex form's tree the tree form's
    same("tmat_analyze_batch_tree", "tmat_analyze_batch", ())
    same("tmat_analyze_batch_ex", "tmat_analyze_batch_tree", tree)
    assert not (got["tmat_analyze_batch_ex"]["pictures"] == GUARD).all() and not (got["tmat_analyze_batch_tree"]["rgb"] == GUARD).all()

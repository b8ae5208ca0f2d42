"""GPU: the tree overlay rasteriser (tmat_render_tree, overlay_kernels.hip) equals its host twin and the numpy restatement byte for byte."""
import numpy as np
import pytest

from tmat_amd import _lib

from test_tree_pictures import ALL_CASES, FIELDS, GT, background, reference_picture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    h = _lib.Handle(None, 0)
    yield h
    h.close()


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_render_tree_equals_host_twin_and_restatement(plain, case):
    name, bg, segs, sb, vis = case
    got = plain.render_tree(bg, [(segs, sb)], vis)[0]
    host = _lib.host_render_tree(bg, [(segs, sb)], vis)[0]
    assert np.array_equal(got, host), int((got != host).sum())
    assert np.array_equal(got, reference_picture(case))


def test_render_tree_batch_of_16_with_very_different_segment_counts(plain):
    """16 images in one launch set: 0 segments, a handful, more than one 256-segment chunk, and the fixture's trees; twice for determinism"""
    rs = np.random.RandomState(5)
    bgs = np.stack([background(20 + i, 96, 96) for i in range(16)])
    keys = ["s96_c0_s1", "s96_c1_s1", "s96_c3_s1", "s96_c6_s1"]
    trees = []
    for i in range(16):
        if i == 3:
            trees.append((np.zeros((0, 4)), np.zeros(0, np.int32)))
        elif i % 4 == 0:
            k = keys[i // 4]
            trees.append((GT[k + "_segs"].astype(np.float64), GT[k + "_branch"]))
        else:
            n = [1, 7, 300, 700][i % 4]
            p = rs.uniform(-10, 106, (n, 2))
            trees.append((np.concatenate([p, p + rs.normal(0, 6, (n, 2))], axis=1), rs.randint(0, 400, n).astype(np.int32)))
    assert max(len(t[0]) for t in trees) > 512 and min(len(t[0]) for t in trees) == 0
    got = plain.render_tree(bgs, trees, 500)
    host = _lib.host_render_tree(bgs, trees, 500)
    assert got.shape == (16, 500, 500, 3)
    for i in range(16):
        assert np.array_equal(got[i], host[i]), (i, int((got[i] != host[i]).sum()))
    assert (got[3].max(axis=2) == got[3].min(axis=2)).all()                # no segments: grey only
    again = plain.render_tree(bgs, trees, 500)
    assert np.array_equal(got, again)


def test_render_tree_f32_background_and_default_width(plain):
    key = "s_rect_c0_s1"
    tree = (GT[key + "_segs"].astype(np.float64), GT[key + "_branch"])
    got = plain.render_tree(FIELDS["s_rect"], [tree])[0]
    assert got.shape == (1500, 2000, 3)
    assert np.array_equal(got, _lib.host_render_tree(FIELDS["s_rect"], [tree])[0])


# ---- pictures out of the batched pipeline (tmat_analyze_batch_tree) ----
CFG = dict(graph_thresh_1=5, graph_thresh_2=10, graph_smoothing_window=12, min_branch_length=12)


def staged_tree(handle, img, cfg, width_um, thresh=(5.0, 10.0), ds_ratio=0.625):
    """one image through the staged entry points: (down-sampled u16 background, (segs, seg_branch), scaled bars, unscaled tmat_morse_stats bars, sf)"""
    from tmat_amd import branches
    H, W = img.shape
    hh, ww = int(round(W * ds_ratio)), int(round(H * ds_ratio))
    L = _lib.lib()
    pred = np.empty((1, hh, ww), np.float64)
    _lib.check(L.tmat_segment_batch(handle.raw, _lib.ptr(np.ascontiguousarray(img[None])), 1, H, W, float(ds_ratio), _lib.ptr(pred)), "segment")
    filt, dist = handle.filter_edt(pred)
    skel, _ = handle.medial_axis(filt)
    fshape = branches.dsamp_shape((H, W))
    _, f255 = handle.finish(pred, dist, skel, fshape)
    sw, mn, mx = branches.graph_px_params(cfg, 384, width_um)
    V, E = _lib.dmt_graph(f255[0], *thresh)
    sf = ww / fshape[1]
    segs, sb, bars, n, tot, avg = _lib.morse_tree(V, E, fshape, sw, mn, mx, False, None, sf)
    bars0 = _lib.morse_stats(V, E, fshape, sw, mn, mx, False, None)[0]
    return _lib.host_lanczos4_u16(img, (hh, ww)), (segs, sb), bars, bars0, sf


def test_analyze_batch_tree_over_three_passes(handle):
    from tmat_amd import branches, synth
    imgs = np.stack([synth.synth_image(i, 512, n_vessels=12, scale=1.0) for i in range(7)])       # 72 patches each, 256 per pass: 3 + 3 + 1
    imgs[5] = 1000                                                                              # an image without branches
    rows0 = branches.analyze_batch(handle, imgs, CFG, 500.0)
    rows, rgb, bars = branches.analyze_batch_tree(handle, imgs, CFG, 500.0, vis_width=500)
    assert rows == rows0                                            # bit for bit: tuples of ints and floats
    assert rgb.shape == (7, 500, 500, 3) and sum(r[1] for r in rows) > 0 and rows[5][1] == 0 and len(bars[5]) == 0
    for i in range(7):
        bg, tree, b_scaled, b_plain, sf = staged_tree(handle, imgs[i], CFG, 500.0)
        assert len(bars[i]) == rows[i][1]
        assert np.array_equal(bars[i], b_plain * sf) and np.array_equal(bars[i], b_scaled)
        want = _lib.host_render_tree(bg, [tree], 500)[0]
        assert np.array_equal(rgb[i], want), (i, int((rgb[i] != want).sum()))
    rows2, rgb2, bars2 = branches.analyze_batch_tree(handle, imgs, CFG, 500.0, vis_width=500)
    assert rows2 == rows and np.array_equal(rgb2, rgb) and all(np.array_equal(a, b) for a, b in zip(bars, bars2))
    assert branches.analyze_batch(handle, imgs, CFG, 500.0) == rows0            # the plain entry is untouched by the tree call before it


def test_morse_graph_mirror_with_a_handle(plain):
    from tmat_amd.topology import MorseGraph
    f = FIELDS["s96"]
    a = MorseGraph(f, thresholds=(5, 10), min_branch_length=5, smoothing_window=5)
    b = MorseGraph(f, thresholds=(5, 10), min_branch_length=5, smoothing_window=5, handle=plain)
    assert a.barcode == b.barcode and len(a.barcode) > 0
    for x, y in zip(a.colored_tree(640 / 384), b.colored_tree(640 / 384)):
        assert np.array_equal(x, y)


def test_script_tree_visualizations(tmp_path):
    """--tree-visualizations adds exactly morse_tree.png and barcode.png per image; a 2 x 2 threshold grid writes four suffixed pairs; a second
    run into the same folder writes -2 names; --visualizations alone still writes its four files"""
    from tmat_amd import synth
    from test_gpu_script import run
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    np.save(ind / "t_0.npy", synth.synth_image(0, 512, n_vessels=12, scale=1.0))
    base = [str(ind), str(outd), "--image-width-microns", "500"]
    r = run(base + ["--tree-visualizations", "--vis-width", "400"])
    assert r.returncode == 0, r.stdout + r.stderr
    vdir = outd / "visualizations" / "t_0"
    assert sorted(p.name for p in vdir.iterdir()) == ["barcode.png", "morse_tree.png"]
    from PIL import Image
    im = np.asarray(Image.open(vdir / "morse_tree.png"))
    assert im.shape == (400, 400, 3) and (im.max(axis=2) != im.min(axis=2)).any()
    assert np.asarray(Image.open(vdir / "barcode.png")).shape == (360, 360, 3)
    r = run(base + ["--tree-visualizations", "--vis-width", "400"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in vdir.iterdir()) == ["barcode-2.png", "barcode.png", "morse_tree-2.png", "morse_tree.png"]
    assert np.array_equal(np.asarray(Image.open(vdir / "morse_tree-2.png")), im)
    outg = tmp_path / "grid"
    r = run([str(ind), str(outg), "--image-width-microns", "500", "--tree-visualizations", "--vis-width", "400", "--graph-thresh-1", "2", "5",
             "--graph-thresh-2", "4", "10"])
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(p.name for p in (outg / "visualizations" / "t_0").iterdir())
    assert len(names) == 8 and all("_CONFIG_thresh1_" in n and "_thresh2_" in n for n in names)
    assert sum(n.startswith("morse_tree") for n in names) == 4 and sum(n.startswith("barcode") for n in names) == 4
    outv = tmp_path / "vis"
    r = run([str(ind), str(outv), "--image-width-microns", "500", "--visualizations"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in (outv / "visualizations" / "t_0").iterdir()) == ["distance_transform.png", "original_image.png", "prediction.png",
                                                                                  "segmentation_mask.png"]


def test_script_tree_visualizations_with_detect_well(tmp_path, handle):
    """-w --tree-visualizations on 2-D images: the tree of the (pruned) graph over the image's own down-sampled picture, equal to the host
    twin fed through the staged entry points; the CSV rows are the well form's rows; an image without branches writes no picture.
    Image 3 keeps its branches (its mask covers too little and is dropped, compute_branches.py:132-139); image 5 has a real well and no
    branch survives the pruning (tests/test_gpu_wellmask.py pins both facts against the oracle)."""
    from PIL import Image
    from tmat_amd import branches
    from test_gpu_script import read_csv, run
    from test_gpu_wellmask import _well_image
    imgs = {"w_3": _well_image(3), "w_5": _well_image(5)}
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    for k, im in imgs.items():
        np.save(ind / f"{k}.npy", im)
    r = run([str(ind), str(outd), "--image-width-microns", "500", "-w", "--well-seed", "7", "--tree-visualizations", "--vis-width", "400"])
    assert r.returncode == 0, r.stdout + r.stderr
    fields, bgs = branches.well_fields(handle, np.stack([imgs["w_3"], imgs["w_5"]]), 0.625, 16, 7, warn=lambda m: None, return_backgrounds=True)
    want_rows = branches.well_rows(handle, fields, CFG, 500.0)
    csv_rows = read_csv(outd / "branching_analysis.csv")[1:]
    counts = []
    for i, k in enumerate(("w_3", "w_5")):
        f255, pruning, _ = fields[i]
        tree, bars, (cnt, tot, avg) = branches.field_tree(handle, f255, CFG, 500.0, (5.0, 10.0), pruning, bgs[i].shape[1] / f255.shape[1])
        assert (i, cnt, tot, avg) == want_rows[i] and len(bars) == cnt
        assert csv_rows[i][0] == k and int(csv_rows[i][1]) == cnt
        assert float(csv_rows[i][2]) == pytest.approx(branches.pixels_to_microns(tot, 384, 500.0), rel=1e-12)
        vdir = outd / "visualizations" / k
        counts.append(cnt)
        if cnt == 0:
            assert not vdir.exists() and f"No branches found for {k}." in r.stdout
            continue
        assert sorted(p.name for p in vdir.iterdir()) == ["barcode.png", "morse_tree.png"]
        assert np.array_equal(np.asarray(Image.open(vdir / "morse_tree.png")), _lib.host_render_tree(bgs[i], [tree], 400)[0])
        assert np.array_equal(np.asarray(Image.open(vdir / "barcode.png")), _lib.host_render_barcode(bars, 400))
    assert counts[0] > 0


def test_script_tree_visualizations_on_z_stacks(tmp_path, plain):
    """--tree-visualizations on a Z stack: the tree of the vesselness field over the full-resolution max projection, scaled by W / 384
    (compute_branches.py:437); one suffixed pair per threshold configuration; beside them nothing new"""
    from PIL import Image
    from tmat_amd import branches, sato, synth
    from test_gpu_script import read_csv, run
    st = synth.synth_stack(1, 4, 200, 256, n_vessels=8)
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    for z, sl in enumerate(st):
        Image.fromarray(sl).save(ind / f"wellA_z{z}.tif")
    r = run([str(ind), str(outd), "--image-width-microns", "800", "--tree-visualizations", "--vis-width", "300", "--graph-thresh-1", "2", "5"])
    assert r.returncode == 0, r.stdout + r.stderr
    vdir = outd / "visualizations" / "wellA"
    sfx = {2.0: "_CONFIG_thresh1_2.0", 5.0: "_CONFIG_thresh1_5.0"}
    assert sorted(p.name for p in vdir.iterdir()) == sorted(f"{k}{s}.png" for k in ("barcode", "morse_tree") for s in sfx.values())
    f255 = _lib.host_rescale255_f32(sato.stack_field(plain, st, 384))
    assert f255.shape == (300, 384)
    for t1, s in sfx.items():
        tree, bars, (cnt, tot, avg) = branches.field_tree(plain, f255, CFG, 800.0, (t1, 10.0), None, 256 / 384)
        row = read_csv(outd / f"branching_analysis{s}.csv")[1]
        assert row[0] == "wellA" and int(row[1]) == cnt and cnt > 0 and len(bars) == cnt
        assert float(row[2]) == pytest.approx(branches.pixels_to_microns(tot, 384, 800.0), rel=1e-12)
        got = np.asarray(Image.open(vdir / f"morse_tree{s}.png"))
        assert got.shape == (234, 300, 3)                           # round_half_even(300 * 200 / 256)
        assert np.array_equal(got, _lib.host_render_tree(st.max(0), [tree], 300)[0])
        assert np.array_equal(np.asarray(Image.open(vdir / f"barcode{s}.png")), _lib.host_render_barcode(bars, 300))


def test_render_tree_timed_gives_the_same_bytes_and_four_phase_times(plain):
    name, bg, segs, sb, vis = ALL_CASES[0]
    got, ms = plain.render_tree_timed(bg, [(segs, sb)], vis)
    assert np.array_equal(got, plain.render_tree(bg, [(segs, sb)], vis))
    assert sorted(ms) == ["copy_back", "minmax", "render", "upload"] and all(v >= 0 for v in ms.values()) and ms["render"] > 0


def test_analyze_batch_tree_retries_with_a_larger_bar_capacity(handle):
    from tmat_amd import branches, synth
    imgs = synth.synth_image(0, 512, n_vessels=12, scale=1.0)[None]
    rows, rgb, bars = branches.analyze_batch_tree(handle, imgs, CFG, 500.0, vis_width=200)
    assert rows[0][1] > 1
    rows1, rgb1, bars1 = branches.analyze_batch_tree(handle, imgs, CFG, 500.0, vis_width=200, cap_bars=1)
    assert rows1 == rows and np.array_equal(rgb1, rgb) and np.array_equal(bars1[0], bars[0])

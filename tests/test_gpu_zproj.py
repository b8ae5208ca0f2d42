"""GPU parity: Z projections (csrc/zproj_kernels.hip) through tmat_zproj_batch against oracle/zproj.py, bit-exact,
including image borders, odd sizes, ties, uint8 stacks, the full config-#3 stack size (through crops the oracle can
check in seconds and through size-independent properties), and the drop-in script end to end."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def plain():
    sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd"))
    from tmat_amd import _lib
    h = _lib.Handle(None, 0)
    yield h
    h.close()


@pytest.mark.parametrize("shape", [(5, 37, 50), (3, 64, 64), (4, 3, 2), (2, 1, 9), (7, 33, 129), (1, 40, 40)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_focus_stacking_matches_oracle(plain, shape, dtype):
    from oracle import zproj as oz
    rs = np.random.RandomState(sum(shape))
    stacks = rs.randint(0, np.iinfo(dtype).max + 1, (3,) + shape).astype(dtype)
    stacks[1, :, : shape[1] // 2] = stacks[1, :1, : shape[1] // 2]      # identical slices in a region: ties keep slice 0
    stacks[2] = 1234 % (np.iinfo(dtype).max + 1)                        # flat stack: zero focus everywhere
    got = plain.zproj(stacks, "fs")
    assert got.dtype == dtype and got.shape == (3,) + shape[1:]
    for i in range(3):
        assert np.array_equal(got[i], oz.proj_focus_stacking(stacks[i])), i


@pytest.mark.parametrize("method", ["min", "max", "avg", "med"])
@pytest.mark.parametrize("Z", [1, 2, 5, 16, 64, 65, 130])
def test_reductions_match_numpy(plain, method, Z):
    from oracle import zproj as oz
    rs = np.random.RandomState(Z)
    stacks = rs.randint(0, 65536, (2, Z, 45, 70)).astype(np.uint16)
    stacks[0, :, :8] = rs.randint(0, 3, (Z, 8, 70))          # heavy ties (the deep-stack median is a radix select: Z > 64)
    got = plain.zproj(stacks, method)
    want = np.stack([getattr(oz, "proj_" + method)(s) for s in stacks])
    assert got.dtype == want.dtype
    assert np.array_equal(got, want)


def _dma_tiles(H, W):
    """(tiles that satisfy zproj_focus_kernel's `fast` condition for an aligned stack below 2 GiB, all tiles): the 72 x 72 window of the
    tile at (x0, y0) lies inside the image and W is even"""
    inside = lambda n: sum(1 for o in range(0, n, 64) if o >= 4 and o + 68 <= n)
    return (inside(W) * inside(H) if W % 2 == 0 else 0), -(-W // 64) * -(-H // 64)


def _differing(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} pixels differ, first at {bad[:4].tolist()}"


# the sizes at the edge of the `fast` condition, with the number of tiles that take the LDS-DMA branch.  (133, 135) checks the result at
# an odd width with an interior tile, not the `(W & 1) == 0` clause itself: with that clause removed the DMA loads pixel pairs at 2-byte
# alignment, an MI355X returns the right bytes for them, and every case here still passes (the same holds for the address clause below)
DMA_EDGE_SHAPES = {(132, 132): 1,        # 64 + 68 == 132 both ways: exactly one DMA tile
                   (131, 132): 0,        # one row short
                   (132, 130): 0,        # two columns short
                   (133, 135): 0,        # large enough, but odd W: the gather must run everywhere
                   (196, 260): 6,        # x0 = 64, 128, 192 (192 + 68 == W) times y0 = 64, 128
                   (197, 262): 6}        # the same tiles with a border tile to their right and below


@pytest.mark.parametrize("Z", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("hw", list(DMA_EDGE_SHAPES))
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_focus_stacking_interior_tiles_at_the_edge_of_the_dma_condition(plain, dtype, hw, Z):
    """images just large enough (or just too small, or of odd width) for tiles whose window needs no reflection: those tiles stage their
    slices by LDS-DMA, double-buffered (odd Z leaves the last slice alone in the first buffer); three stacks per launch, each with
    its own buffer base; the whole image against the oracle"""
    from oracle import zproj as oz
    H, W = hw
    assert _dma_tiles(H, W)[0] == DMA_EDGE_SHAPES[hw]
    rs = np.random.RandomState(1000 * H + 10 * W + Z)
    stacks = rs.randint(0, np.iinfo(dtype).max + 1, (3, Z, H, W)).astype(dtype)
    got = plain.zproj(stacks, "fs")
    assert got.dtype == dtype and got.shape == (3, H, W)
    for i in range(3):
        want = oz.proj_focus_stacking(stacks[i])
        assert np.array_equal(got[i], want), (i, _differing(got[i], want))


def test_focus_stacking_adversarial_content_in_interior_tiles(plain):
    """(196, 260): DMA tiles at x0 = 64, 128, 192 and y0 = 64, 128.  One launch of seven different stacks: ties over a region that spans a
    DMA tile and its neighbours, a flat stack (slice 0), saturated blocks and checkerboards (the largest blurred values and focus
    magnitudes: the 16-bit packing of the blurred tile), slices that differ in one pixel of an interior tile, and two stacks whose slices
    tie in focus everywhere but differ in value, in opposite slice orders: only those show which slice wins a tie (the first)"""
    from oracle import zproj as oz
    Z, H, W = 5, 196, 260
    assert _dma_tiles(H, W) == (6, 20)
    rs = np.random.RandomState(42)
    rnd = lambda *shape: rs.randint(0, 65536, shape).astype(np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    ties = rnd(Z, H, W)
    ties[:, 50:150, 100:210] = ties[:1, 50:150, 100:210]          # covers the tile at (y0 64, x0 128) and reaches into five more
    flat = np.full((Z, H, W), 1234, np.uint16)
    sat = rnd(Z, H, W)
    sat[1] = 0
    sat[1, 70:130, 90:200] = 65535                                # a saturated block on black: the steepest edges
    sat[2] = np.where((yy + xx) & 1, 65535, 0)                    # checkerboard of single pixels
    sat[3] = np.where(((yy >> 2) + (xx >> 2)) & 1, 65535, 0)      # checkerboard of 4 x 4 blocks
    sat[4] = 65535
    sat[:, :40] = rnd(Z, 40, W)                                   # and an ordinary strip, so that the stack is not all extremes
    one = rnd(Z, H, W)
    one[1] = one[0]; one[1, 100, 150] ^= 0x8000                   # slice 1 = slice 0 but for one pixel inside the tile at (64, 128)
    one[2] = one[0]
    one[4] = one[3]; one[4, 160, 200] ^= 1                        # the smallest change, inside the tile at (128, 192)
    block = np.zeros((Z, H, W), np.uint16)
    block[:, 64:128, 64:128] = 65535                              # exactly one saturated DMA tile in every slice
    block[3, 96, 96] = 0
    # slice + constant, nothing saturating: the blur weights sum to 256, so the blurred slice shifts by exactly the constant, and the
    # Laplacian weights sum to 0, so the focus measure of all five slices is equal at every pixel while their values differ
    shifted = rs.randint(0, 60000, (1, H, W)).astype(np.uint16) + np.array([0, 1000, 7, 3000, 1], np.uint16)[:, None, None]
    stacks = np.stack([ties, flat, sat, one, block, shifted, shifted[::-1]])
    got = plain.zproj(stacks, "fs")
    for i, name in enumerate(("ties", "flat", "saturated", "one pixel", "block", "shifted", "shifted, reversed")):
        want = oz.proj_focus_stacking(stacks[i])
        assert np.array_equal(got[i], want), (name, _differing(got[i], want))
    assert np.array_equal(got[5], shifted[0]) and np.array_equal(got[6], shifted[4])          # the first slice of each order, whole image


def test_focus_stacking_race_screen(plain):
    """(644, 644): 121 tiles per stack, 81 of them DMA tiles; four stacks per launch, copies of two bases in an order that changes from
    launch to launch, three launches on one handle.  Every stack must equal the oracle every time: an LDS-DMA ordering bug or a stale
    input buffer shows up as rare wrong tiles, not as a crash"""
    from oracle import zproj as oz
    Z, H, W = 5, 644, 644
    assert _dma_tiles(H, W) == (81, 121)
    rs = np.random.RandomState(11)
    base = rs.randint(0, 65536, (2, Z, H, W)).astype(np.uint16)
    base[1, 2, 200:420] = base[1, 1, 200:420]                      # a band of equal slices in the second base
    want = [oz.proj_focus_stacking(b) for b in base]
    for rep, order in enumerate(((0, 1, 0, 1), (1, 0, 0, 1), (1, 1, 1, 0))):
        got = plain.zproj(np.stack([base[k] for k in order]), "fs")
        for i, k in enumerate(order):
            assert np.array_equal(got[i], want[k]), (rep, i, _differing(got[i], want[k]))


def test_focus_stacking_from_an_unaligned_device_address(plain):
    """tmat_zproj_dev on a stack at a 4-byte-aligned device address and on the same stack 2 bytes further on, where the pixel pairs are
    not 4-byte aligned and the kernel's alignment clause turns the DMA off; both results equal the oracle.  Equal results show that the
    shifted stack is projected correctly, not which branch did it: a kernel without the clause gives the same bytes on an MI355X"""
    import ctypes as C
    from oracle import zproj as oz
    from tmat_amd import _lib
    L = _lib.lib()
    n, Z, H, W = 2, 3, 196, 260
    stacks = np.random.RandomState(5).randint(0, 65536, (n, Z, H, W)).astype(np.uint16)
    want = np.stack([oz.proj_focus_stacking(s) for s in stacks])
    din, dout = C.c_void_p(), C.c_void_p()
    _lib.check(L.tmat_dev_alloc(plain.raw, stacks.nbytes + 4, C.byref(din)), "alloc")
    try:
        _lib.check(L.tmat_dev_alloc(plain.raw, want.nbytes, C.byref(dout)), "alloc")
        assert din.value % 4 == 0
        for shift in (0, 2):
            src = C.c_void_p(din.value + shift)
            got = np.zeros_like(want)
            _lib.check(L.tmat_dev_upload(plain.raw, dout, _lib.ptr(got), got.nbytes), "upload")          # no stale result
            _lib.check(L.tmat_dev_upload(plain.raw, src, _lib.ptr(stacks), stacks.nbytes), "upload")
            _lib.check(L.tmat_zproj_dev(plain.raw, src, n, Z, H, W, 0, dout), "zproj")
            _lib.check(L.tmat_dev_download(plain.raw, _lib.ptr(got), dout, got.nbytes), "download")
            assert np.array_equal(got, want), (shift, _differing(got, want))
    finally:
        _lib.check(L.tmat_dev_free(plain.raw, din), "free")
        if dout.value:
            _lib.check(L.tmat_dev_free(plain.raw, dout), "free")


@pytest.mark.parametrize("method", ["min", "max", "avg", "med"])
@pytest.mark.parametrize("Z", [3, 65])
def test_reductions_uint8_three_stacks(plain, method, Z):
    """uint8 stacks, three per launch, 37 x 53 pixels (no multiple of the 256-pixel block: the last block of every stack is partial)"""
    from oracle import zproj as oz
    rs = np.random.RandomState(100 + Z)
    stacks = rs.randint(0, 256, (3, Z, 37, 53)).astype(np.uint8)
    stacks[1, :, :6] = rs.randint(0, 2, (Z, 6, 53))               # heavy ties
    stacks[2, :, 30:] = 255
    got = plain.zproj(stacks, method)
    want = np.stack([getattr(oz, "proj_" + method)(s) for s in stacks])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)


def test_model_entry_points_refuse_a_plain_handle(plain):
    with pytest.raises(Exception, match="no model"):
        plain.unet_predict(np.zeros((1, 320, 320), np.float32))


def test_full_size_stack_crops_and_properties(plain):
    """config #3 size: 16 slices of 2048 x 2048.  The oracle checks crops (corners keep the true image border, the
    interior crops are compared away from their own artificial border); the whole image is checked by properties."""
    from oracle import zproj as oz
    rs = np.random.RandomState(7)
    Z, H, W = 16, 2048, 2048
    st = rs.randint(0, 65536, (Z, H, W)).astype(np.uint16)
    st[5, 512:1024] = st[4, 512:1024]                    # two equal slices in a band
    got = plain.zproj(st[None], "fs")[0]
    assert np.all((st == got[None]).any(axis=0))         # every pixel is one of its own stack's values
    C = 160
    for (y, x) in ((0, 0), (0, W - C), (H - C, 0), (H - C, W - C), (700, 900), (1500, 40)):
        crop = st[:, y:y + C, x:x + C]
        want = oz.proj_focus_stacking(crop)
        ys = slice(0 if y == 0 else 4, C if y + C == H else C - 4)
        xs = slice(0 if x == 0 else 4, C if x + C == W else C - 4)
        assert np.array_equal(got[y:y + C, x:x + C][ys, xs], want[ys, xs]), (y, x)
    assert np.array_equal(plain.zproj(st[None, :1], "fs")[0], st[0])          # single slice: identity
    assert np.array_equal(plain.zproj(st[None], "max")[0], st.max(axis=0))


def test_script_end_to_end(tmp_path, plain):
    from PIL import Image
    from oracle import zproj as oz
    sys.path.insert(0, str(REPO / "tissue-model-analysis-tools_amd" / "scripts"))
    import compute_zproj as cz
    rs = np.random.RandomState(3)
    in_root, out_root = tmp_path / "in", tmp_path / "out"
    in_root.mkdir()
    stacks = {}
    for well in ("A1", "B7"):
        st = rs.randint(0, 65536, (4, 96, 80)).astype(np.uint16)
        stacks[well] = st
        for z in range(4):
            Image.fromarray(st[z]).save(in_root / f"{well}_z{z}.tif")
    cz.main(cz.parse_zproj_args([str(in_root), str(out_root), "-m", "fs"]))
    for well, st in stacks.items():
        got = np.array(Image.open(out_root / f"{well}_fs.tif"))
        assert got.dtype == np.uint16 and np.array_equal(got, oz.proj_focus_stacking(st))
    cz.main(cz.parse_zproj_args([str(in_root), str(out_root), "-m", "fs"]))          # second run: unique names
    assert (out_root / "A1_fs-2.tif").is_file()
    cz.main(cz.parse_zproj_args([str(in_root), str(out_root)]))                       # default method: max
    assert np.array_equal(np.array(Image.open(out_root / "B7_max.tif")), stacks["B7"].max(axis=0))


def test_script_time_series_and_area(tmp_path, plain):
    """--time N selects the T plane of an ImageJ hyperstack (reference helper.load_image), and -a/--area runs the cell-area drop-in on
    the projections with OUT_ROOT as its input and output directory (compute_zproj.py:98-119)"""
    import csv
    import subprocess
    from PIL import Image, TiffImagePlugin
    from oracle import cellarea as ca
    from tmat_amd import synth
    script = REPO / "tissue-model-analysis-tools_amd" / "scripts" / "compute_zproj.py"
    in_root, out_root = tmp_path / "in", tmp_path / "out"
    in_root.mkdir()
    T, Z = 2, 3
    vol = np.stack([np.stack([synth.synth_image(50 + 10 * t + z, 256, n_vessels=10, scale=0.5) for z in range(Z)]) for t in range(T)])      # (T, Z, H, W)
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[270] = f"ImageJ=1.53\nimages={T * Z}\nslices={Z}\nframes={T}\nhyperstack=true\n"
    pages = [Image.fromarray(vol[t, z]) for t in range(T) for z in range(Z)]          # ImageJ order: Z runs faster than T
    pages[0].save(in_root / "plate.tif", save_all=True, append_images=pages[1:], tiffinfo=ifd)
    r = subprocess.run([sys.executable, str(script), str(in_root), str(out_root)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "time series image but no time index" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, str(script), str(in_root), str(out_root), "--time", "1", "-m", "max", "-a"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    proj = np.array(Image.open(out_root / "plate_max.tif"))
    assert np.array_equal(proj, vol[1].max(axis=0))
    rows = list(csv.reader(open(out_root / "calculations" / "cell_area.csv")))
    assert rows[0] == ["image_id", "area_pct"] and rows[1][0] == "plate_max"
    oa, ok = ca.cell_area(proj, 512, 0.0)
    assert float(rows[1][1]) == oa * 100
    assert np.array_equal(np.array(Image.open(out_root / "thresholded" / "plate_max_thresholded.png")), ok)

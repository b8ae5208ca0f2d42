"""Mirror of the image-loading part of fl_tissue_model_tools.helper (reference helper.py:23-139): `load_image` returns the
pixel array and the physical pixel sizes found in the file's metadata.  The reference reads files through aicsimageio;
this build reads TIFF / PNG with Pillow and parses the two metadata conventions aicsimageio's TIFF readers honour:

* OME-TIFF: `PhysicalSizeX/Y/Z` (+ `PhysicalSize?Unit`, default µm) of the first `Pixels` element of the OME-XML held in
  the ImageDescription tag;
* ImageJ TIFF: `unit=micron|um|µm` in the ImageDescription together with the X/YResolution tags (pixels per unit).

Anything else yields PhysicalPixelSizes(None, None, None), for which compute_branches.py asks for --image-width-microns
exactly as the reference does (compute_branches.py:184-212).
"""
from __future__ import annotations

import re
from collections import namedtuple
from typing import Optional

import numpy as np

PhysicalPixelSizes = namedtuple("PhysicalPixelSizes", ["Z", "Y", "X"])

_UNIT_TO_MICRON = {"µm": 1.0, "um": 1.0, "micron": 1.0, "microns": 1.0, "micrometer": 1.0, "nm": 1e-3, "mm": 1e3, "cm": 1e4,
                   "m": 1e6, "pm": 1e-6, "inch": 25400.0, "in": 25400.0}


def _ome_sizes(desc: str):
    m = re.search(r"<Pixels\b[^>]*>", desc)
    if not m:
        return None
    attrs = dict(re.findall(r'(\w+)="([^"]*)"', m.group(0)))
    out = []
    for ax in "ZYX":
        v = attrs.get("PhysicalSize" + ax)
        if v is None:
            out.append(None)
            continue
        unit = attrs.get(f"PhysicalSize{ax}Unit", "µm").replace("μ", "µ")
        scale = _UNIT_TO_MICRON.get(unit)
        out.append(float(v) * scale if scale is not None else None)
    return PhysicalPixelSizes(*out)


def _imagej_sizes(desc: str, tags):
    if "ImageJ=" not in desc:
        return None
    m = re.search(r"unit=(\S+)", desc)
    if not m:
        return None
    unit = m.group(1).strip().replace("\\u00B5", "µ").replace("μ", "µ")
    scale = _UNIT_TO_MICRON.get(unit)
    if scale is None:
        return None

    def res(tag):
        v = tags.get(tag)
        if v is None:
            return None
        v = v[0] if isinstance(v, tuple) and len(v) == 1 else v
        try:
            v = float(v[0]) / float(v[1]) if isinstance(v, tuple) else float(v)
        except (TypeError, ZeroDivisionError, ValueError):
            return None
        return scale / v if v > 0 else None
    sp = re.search(r"spacing=([0-9.eE+-]+)", desc)
    return PhysicalPixelSizes(float(sp.group(1)) * scale if sp else None, res(283), res(282))


def physical_pixel_sizes(path) -> PhysicalPixelSizes:
    """PhysicalPixelSizes(Z, Y, X) in microns per pixel, None where the file does not say"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            tags = dict(getattr(im, "tag_v2", {}) or {})
    except OSError:
        return PhysicalPixelSizes(None, None, None)
    desc = tags.get(270, "")
    if isinstance(desc, (tuple, list)):
        desc = desc[0] if desc else ""
    if isinstance(desc, bytes):
        desc = desc.decode("utf8", "replace")
    for parse in (lambda: _ome_sizes(desc), lambda: _imagej_sizes(desc, tags)):
        got = parse()
        if got is not None:
            return got
    return PhysicalPixelSizes(None, None, None)


def page_layout(desc: str, n_pages: int):
    """(size_t, size_z, size_c, order) of a multi-page TIFF from its ImageDescription, order = the page axes from the fastest
    to the slowest varying one (e.g. "ZCT").  OME-XML: SizeT / SizeZ / SizeC / DimensionOrder of the first Pixels element;
    ImageJ hyperstacks: frames= / slices= / channels=, always channel-fastest ("CZT").  Files without either convention are
    one Z stack, as aicsimageio's plain TIFF reader presents them."""
    m = re.search(r"<Pixels\b[^>]*>", desc or "")
    if m:
        attrs = dict(re.findall(r'(\w+)="([^"]*)"', m.group(0)))
        try:
            st, sz, sc = int(attrs.get("SizeT", 1)), int(attrs.get("SizeZ", 1)), int(attrs.get("SizeC", 1))
        except ValueError:
            st = sz = sc = 0
        order = attrs.get("DimensionOrder", "XYZCT")[2:]
        if st * sz * sc == n_pages and sorted(order) == ["C", "T", "Z"]:
            return st, sz, sc, order
    if "ImageJ=" in (desc or ""):
        def num(key):
            mm = re.search(key + r"=(\d+)", desc)
            return int(mm.group(1)) if mm else 1
        st, sz, sc = num("frames"), num("slices"), num("channels")
        if st * sz * sc == n_pages:
            return st, sz, sc, "CZT"
    return 1, n_pages, 1, "ZCT"


def load_image(file_path, T: Optional[int] = None, C: Optional[int] = None):
    """(ZYX or YX array, PhysicalPixelSizes): the reference's contract (helper.py:23-95) for single files and for lists of
    slice files, with its error messages: T / C must be given for time series / multi-channel files and lie in range.  The
    page layout of multi-page files (which page is which T, Z, C) comes from the OME-XML or ImageJ description."""
    if isinstance(file_path, (list, tuple)):
        imgs, sizes = zip(*[load_image(fp, T, C) for fp in file_path])
        return np.array(imgs), sizes[0]
    from PIL import Image
    with Image.open(file_path) as im:
        n_pages = getattr(im, "n_frames", 1)
        tags = dict(getattr(im, "tag_v2", {}) or {})
        desc = tags.get(270, "")
        if isinstance(desc, (tuple, list)):
            desc = desc[0] if desc else ""
        if isinstance(desc, bytes):
            desc = desc.decode("utf8", "replace")
        st, sz, sc, order = page_layout(desc, n_pages)
        im.seek(0)
        first = np.array(im)
        interleaved = first.ndim == 3              # RGB(A) pages: the channel axis is inside the page
        n_c = first.shape[-1] if interleaved else sc
        if T is None:
            if st > 1:
                raise ValueError(f"{file_path} is a time series image but no time index was specified.")
            T = 0
        elif T >= st or T < 0:
            raise ValueError(f"Time {T} is out of range for {file_path} with times: 0 - {st - 1}")
        if C is None:
            if n_c > 1:
                raise ValueError(f"{file_path} is a multi channel image but no color channel index was specified.")
            C = 0
        elif C >= n_c or C < 0:
            raise ValueError(f"Color channel {C} is out of range for {file_path} with color channels: 0 - {n_c - 1}")
        sizes = {"T": st, "Z": sz, "C": sc}
        stride, strides = 1, {}
        for ax in order:
            strides[ax] = stride
            stride *= sizes[ax]
        planes = []
        for z in range(sz):
            page = T * strides["T"] + z * strides["Z"] + (0 if interleaved else C) * strides["C"]
            im.seek(page)
            a = np.array(im)
            planes.append(a[..., C] if interleaved else a)
    arr = planes[0] if len(planes) == 1 else np.stack(planes)
    return arr, physical_pixel_sizes(file_path)


# ---- TIFF pixels decoded on the device (include/tmat.h: tmat_tiff_decode_batch_dev) ----

def tiff_probe(path_or_bytes):
    """tmat_tiff_probe on a file (a path, or its bytes): one dict per page -- width, height, bits, compression, predictor, big_endian,
    rows_per_strip, n_strips, status (_lib.TIFF_OK / TIFF_FALLBACK / TIFF_CORRUPT) and reason.  No GPU."""
    from . import _lib
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    return _lib.tiff_probe(bytes(data))


class PlaneSource:
    """What load_image(file_path, T, C) would return, not yet decoded: the files' bytes, the (file, page, channel inside the page or
    None) of every plane, and `shape` ((Z, H, W), or (H, W) for a single plane), `dtype` and `nbytes` of the array, so that code
    which groups images by shape and depth takes it in place of the array."""

    def __init__(self, paths, blobs, planes, plane_shape, dtype, supported):
        self.paths, self.blobs, self.planes, self.supported = paths, blobs, planes, supported
        self.dtype = np.dtype(dtype)
        self.shape = tuple(plane_shape) if len(planes) == 1 else (len(planes),) + tuple(plane_shape)
        self.ndim = len(self.shape)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize

    def pil_plane(self, k):
        """plane k through Pillow, as load_image reads it"""
        from PIL import Image
        fi, page, ch = self.planes[k]
        with Image.open(self.paths[fi]) as im:
            im.seek(page)
            a = np.array(im)
        return a if ch is None else a[..., ch]


def plan_planes(file_path, T: Optional[int] = None, C: Optional[int] = None) -> PlaneSource:
    """load_image's page selection without the decode: the same T / C / Z rules through page_layout and the same error messages.  The
    containers are opened with Pillow for their description and page count only, and probed with tmat_tiff_probe."""
    from PIL import Image
    from . import _lib
    paths = [str(p) for p in file_path] if isinstance(file_path, (list, tuple)) else [str(file_path)]
    blobs, planes, shapes, dtypes, supported = [], [], set(), set(), []
    for fi, path in enumerate(paths):
        with Image.open(path) as im:
            n_pages = getattr(im, "n_frames", 1)
            tags = dict(getattr(im, "tag_v2", {}) or {})
            desc = tags.get(270, "")
            if isinstance(desc, (tuple, list)):
                desc = desc[0] if desc else ""
            if isinstance(desc, bytes):
                desc = desc.decode("utf8", "replace")
            st, sz, sc, order = page_layout(desc, n_pages)
            im.seek(0)
            bands = len(im.getbands())
            interleaved = bands > 1                     # RGB(A) pages: the channel axis is inside the page
            size, mode = im.size, im.mode
        n_c = bands if interleaved else sc
        t, c = T, C
        if t is None:
            if st > 1:
                raise ValueError(f"{path} is a time series image but no time index was specified.")
            t = 0
        elif t >= st or t < 0:
            raise ValueError(f"Time {t} is out of range for {path} with times: 0 - {st - 1}")
        if c is None:
            if n_c > 1:
                raise ValueError(f"{path} is a multi channel image but no color channel index was specified.")
            c = 0
        elif c >= n_c or c < 0:
            raise ValueError(f"Color channel {c} is out of range for {path} with color channels: 0 - {n_c - 1}")
        sizes = {"T": st, "Z": sz, "C": sc}
        stride, strides = 1, {}
        for ax in order:
            strides[ax] = stride
            stride *= sizes[ax]
        blob = open(path, "rb").read()
        probed = _lib.tiff_probe(blob) if blob[:2] in (b"II", b"MM") else []
        blobs.append(blob)
        for z in range(sz):
            page = t * strides["T"] + z * strides["Z"] + (0 if interleaved else c) * strides["C"]
            ok = page < len(probed) and probed[page]["status"] == _lib.TIFF_OK
            if ok:
                shapes.add((probed[page]["height"], probed[page]["width"]))
                dtypes.add(np.dtype(np.uint8 if probed[page]["bits"] == 8 else np.uint16))
            else:                                       # what Pillow will make of it: page 0's size and mode stand for the file's pages
                shapes.add((size[1], size[0]))
                dtypes.add(np.dtype({"L": np.uint8, "P": np.uint8, "RGB": np.uint8, "RGBA": np.uint8, "1": np.bool_, "F": np.float32,
                                     "I": np.int32}.get(mode, np.uint16)))
            supported.append(ok)
            planes.append((fi, page, c if interleaved else None))
    if len(shapes) != 1 or len(dtypes) != 1:
        raise ValueError(f"{paths[0]}: the planes differ in shape or pixel type")
    return PlaneSource(paths, blobs, planes, shapes.pop(), dtypes.pop(), supported)


class DevPlanes:
    """planes resident in device memory: `ptr` (a tmat_dev_alloc block of n H W uint16), `shape` (n, H, W), `bits` (8 or 16: what the
    callers pass on as input_bits) and `counts` (planes per source, in order).  free() it, or use it as a context manager."""

    def __init__(self, handle, ptr_, shape, bits, counts):
        self.handle, self.ptr, self.shape, self.bits, self.counts = handle, ptr_, tuple(shape), int(bits), list(counts)

    def __len__(self):
        return self.shape[0]

    def host(self):
        """the pixels as an array, downloaded once and kept (the same object on every call)"""
        if getattr(self, "_host", None) is None:
            self._host = self.download()
        return self._host

    def part(self, i0, k):
        """(device pointer, shape) of the items [i0, i0 + k) along the first axis"""
        import ctypes as C_
        per = int(np.prod(self.shape[1:]))
        return C_.c_void_p(self.ptr.value + int(i0) * per * 2), (int(k),) + self.shape[1:]

    def download(self):
        from . import _lib
        out = np.empty(self.shape, np.uint16)
        _lib.check(_lib.lib().tmat_dev_download(self.handle.raw, _lib.ptr(out), self.ptr, out.nbytes), "tmat_dev_download")
        return out

    def free(self):
        from . import _lib
        if self.ptr is not None:
            _lib.check(_lib.lib().tmat_dev_free(self.handle.raw, self.ptr), "tmat_dev_free")
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def load_planes_dev(handle, sources) -> DevPlanes:
    """The planes of `sources` (PlaneSource objects of one plane shape and pixel type, or (file_path, T, C) requests for plan_planes)
    decoded into ONE resident block: only the files' bytes cross to the device (tmat_tiff_decode_batch_dev).  A plane the device path
    does not take (tiles, Deflate, BigTIFF, RGB pages, PNG files, ...) is decoded by Pillow exactly as load_image does and uploaded into
    its slice, so the block always holds complete pixels.  Physical pixel sizes still come from physical_pixel_sizes."""
    import ctypes as C_
    from . import _lib
    sources = [s if isinstance(s, PlaneSource) else plan_planes(*s) for s in sources]
    if not sources:
        raise ValueError("load_planes_dev: no source")
    hw, dtype = sources[0].shape[-2:], sources[0].dtype
    for s in sources:
        if s.shape[-2:] != hw or s.dtype != dtype:
            raise ValueError("load_planes_dev: the sources differ in plane shape or pixel type")
    if dtype not in (np.uint8, np.uint16):
        raise ValueError(f"expected uint8/uint16 pixels, got {dtype}")
    H, W = hw
    files, planes, owner = [], [], []
    for s in sources:
        base = len(files)
        files += s.blobs
        for k, (fi, page, _) in enumerate(s.planes):
            planes.append((base + fi, page))
            owner.append((s, k))
    n = len(planes)
    L = _lib.lib()
    d = C_.c_void_p()
    _lib.check(L.tmat_dev_alloc(handle.raw, n * H * W * 2, C_.byref(d)), "tmat_dev_alloc")
    dev = DevPlanes(handle, d, (n, H, W), 8 * dtype.itemsize, [len(s.planes) for s in sources])
    try:
        _, status = handle.tiff_decode_dev(files, planes, H, W, d)       # planes that are not TIFF_OK are left alone and reported
        todo = [i for i, st in enumerate(status) if st != _lib.TIFF_OK]     # unsupported kinds; a corrupt one fails in Pillow as before
        for i in todo:
            s, k = owner[i]
            a = np.ascontiguousarray(s.pil_plane(k))
            if a.shape != (H, W) or a.dtype != dtype:
                raise ValueError(f"{s.paths[s.planes[k][0]]}: expected a {H} x {W} {dtype} plane, got {a.shape} {a.dtype}")
            a = a.astype(np.uint16)
            _lib.check(L.tmat_dev_upload(handle.raw, C_.c_void_p(d.value + i * H * W * 2), _lib.ptr(a), a.nbytes), "tmat_dev_upload")
    except Exception:
        dev.free()
        raise
    return dev

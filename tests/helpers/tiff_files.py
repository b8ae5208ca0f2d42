"""TIFF fixtures for the decoder tests, written at test time in two ways.

Pillow route: what Pillow / libtiff write (raw, LZW, LZW + horizontal predictor, PackBits, Deflate; chosen rows per strip; multi-page).
Hand-written route: a small struct-based writer with its own LZW and PackBits encoders and either byte order, for what Pillow does not
write: big-endian files, a stream that runs with a full string table, unsupported layouts and corrupt files.  Every VALID file of the
hand-written route is decoded with Pillow by its caller (check_with_pillow) and must equal its source array: that guards this helper.
Pillow is also the reference decoder of every test: it is not the code under test."""
import io
import struct

import numpy as np
from PIL import Image

SHAPES = [(1, 1), (1, 300), (7, 5), (64, 80), (300, 257), (130, 1024)]
DTYPES = [np.uint8, np.uint16]
ROWS_PER_STRIP = [1, 7, "H", None]                      # None: Pillow's default
COMPRESSIONS = ["none", "lzw", "lzw_pred", "packbits"]
CONTENTS = ["smooth", "noise", "const", "zero", "checker", "ramp"]
PIL_COMPRESSION = {"none": "raw", "lzw": "tiff_lzw", "lzw_pred": "tiff_lzw", "packbits": "packbits", "deflate": "tiff_adobe_deflate"}


def content(kind, shape, dtype, seed=0):
    H, W = shape
    top = np.iinfo(dtype).max
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "smooth":          # a smooth field plus noise: microscopy-like
        a = 0.4 * top * (1 + np.sin(yy / 23.0) * np.cos(xx / 31.0)) / 2 + rng.randint(0, max(top // 64, 2), (H, W))
    elif kind == "noise":
        a = rng.randint(0, top + 1, (H, W))
    elif kind == "const":
        a = np.full((H, W), top * 3 // 5)
    elif kind == "zero":
        a = np.zeros((H, W))
    elif kind == "checker":
        a = np.where(((yy // 3) + (xx // 5)) % 2 == 0, top, 0)
    elif kind == "ramp":          # steps that wrap modulo 2^bits under the predictor
        a = (xx * (top // 3 + 1) + yy * 7) % (top + 1)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a).astype(dtype)


def pil_tiff(arrays, compression="none", rows_per_strip=None):
    """one file through Pillow; arrays: one (H, W) array or a list of them (pages)"""
    pages = [arrays] if isinstance(arrays, np.ndarray) else list(arrays)
    info = {}
    if rows_per_strip is not None:
        info[278] = int(rows_per_strip)
    if compression == "lzw_pred":
        info[317] = 2
    ims = [Image.fromarray(a) for a in pages]
    buf = io.BytesIO()
    kw = dict(format="TIFF", compression=PIL_COMPRESSION[compression], tiffinfo=info)
    if len(ims) > 1:
        kw.update(save_all=True, append_images=ims[1:])
    ims[0].save(buf, **kw)
    return buf.getvalue()


def pil_decode(data, page=0):
    with Image.open(io.BytesIO(data)) as im:
        im.seek(page)
        return np.array(im)


def pil_decode_all(data):
    with Image.open(io.BytesIO(data)) as im:
        pages = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            pages.append(np.array(im))
    return np.stack(pages)


SENTINEL = 0xA5C3


def guarded(n, H, W):
    """(whole buffer, the (n, H, W) middle the decoder may write): one guard plane on either side, everything set to SENTINEL"""
    buf = np.full((n + 2, H, W), SENTINEL, np.uint16)
    return buf, buf[1:-1]


def assert_guards(buf):
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), "the decoder wrote outside its planes"


def grid_rows_per_strip(H):
    """the distinct strip heights of ROWS_PER_STRIP for an image of H rows; 0 stands for Pillow's default"""
    return sorted({min(r, H) if isinstance(r, int) else (H if r == "H" else 0) for r in ROWS_PER_STRIP})


def grid_cases(shape, dtype):
    """every (compression, rows per strip, content) of one shape and depth -> [(name, file, array)] through Pillow"""
    out = []
    for comp in COMPRESSIONS:
        for rps in grid_rows_per_strip(shape[0]):
            for k, kind in enumerate(CONTENTS):
                arr = content(kind, shape, dtype, seed=k + shape[0])
                out.append((f"{comp}-rps{rps or 'default'}-{kind}", pil_tiff(arr, comp, rps or None), arr))
    return out


# ---- hand-written route ----

def lzw_encode(data, clear_when_full=True):
    """TIFF LZW (MSB first, early change) -> (bytes, number of codes, True if the stream ran with a full table).  clear_when_full=False
    never clears: once 4096 entries exist the stream goes on in 12-bit codes without adding any."""
    out, acc, nacc = bytearray(), 0, 0
    width, n_codes, ran_full = 9, 0, False

    def emit(code):
        nonlocal acc, nacc, n_codes
        acc = (acc << width) | code
        nacc += width
        n_codes += 1
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 0xff)
            nacc -= 8
        acc &= (1 << nacc) - 1

    table, nxt = {bytes([i]): i for i in range(256)}, 258
    emit(256)
    w = b""
    for b in bytes(data):
        wc = w + bytes([b])
        if wc in table:
            w = wc
            continue
        emit(table[w])
        if nxt < 4096:
            table[wc] = nxt
            nxt += 1
            if nxt == 4095 and clear_when_full:
                emit(256)
                table, nxt, width = {bytes([i]): i for i in range(256)}, 258, 9
            elif nxt > (1 << width) - 1 and width < 12:
                width += 1
        else:
            ran_full = True
        w = bytes([b])
    if w:
        emit(table[w])
    emit(257)
    if nacc:
        out.append((acc << (8 - nacc)) & 0xff)
    return bytes(out), n_codes, ran_full


def packbits_encode(data):
    data, out, i, n = bytes(data), bytearray(), 0, len(data)
    while i < n:
        run = 1
        while i + run < n and run < 128 and data[i + run] == data[i]:
            run += 1
        if run >= 3:
            out += bytes([(1 - run) & 0xff, data[i]])
            i += run
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([j - i - 1]) + data[i:j]
        i = j
    return bytes(out)


def raw_strips(arr, rows_per_strip, order="<", predictor=False):
    """the raw bytes of each strip: predictor 2 on the samples, then the file's byte order"""
    a = arr.astype(np.int64)
    if predictor:
        a = np.concatenate([a[:, :1], np.diff(a, axis=1)], axis=1) % (np.iinfo(arr.dtype).max + 1)
    a = a.astype(arr.dtype.newbyteorder(order) if arr.dtype.itemsize > 1 else arr.dtype)
    return [a[y:y + rows_per_strip].tobytes() for y in range(0, arr.shape[0], rows_per_strip)]


def write_tiff(pages, order="<", magic=42, next_ifd=None, entry_count=None):
    """pages: dicts with width, height, bits, compression, strips (list of bytes) and optionally predictor, photometric, spp, rps,
    sample_format, tile (True: tile tags instead of strip tags), strip_offsets / strip_counts (lists that replace the true ones).
    next_ifd: what the LAST IFD points to ("self": itself); entry_count: the entry count the last IFD claims."""
    out = bytearray((b"II" if order == "<" else b"MM") + struct.pack(order + "HI", magic, 0))
    ifd_ptr_at = 4
    for k, p in enumerate(pages):
        offs = []
        for s in p["strips"]:
            if len(out) % 2:
                out.append(0)
            offs.append(len(out))
            out += s
        offs = p.get("strip_offsets", offs)
        cnts = p.get("strip_counts", [len(s) for s in p["strips"]])
        tags = {256: [p["width"]], 257: [p["height"]], 258: [p["bits"]] * p.get("spp", 1), 259: [p["compression"]],
                262: [p.get("photometric", 1)], 277: [p.get("spp", 1)]}
        if p.get("tile"):
            tags.update({322: [p["width"]], 323: [p["height"]], 324: offs, 325: cnts})
        else:
            tags.update({273: offs, 278: [p.get("rps", p["height"])], 279: cnts})
        if p.get("predictor", 1) != 1:
            tags[317] = [p["predictor"]]
        if "sample_format" in p:
            tags[339] = [p["sample_format"]]
        entries, extra = [], bytearray()
        if len(out) % 2:
            out.append(0)
        ifd_at = len(out)
        extra_at = ifd_at + 2 + 12 * len(tags) + 4
        for tag in sorted(tags):
            vals = tags[tag]
            short = tag in (258, 259, 262, 277, 317, 339)
            fmt, typ, size = ("H", 3, 2) if short else ("I", 4, 4)
            payload = struct.pack(order + fmt * len(vals), *vals)
            if len(payload) <= 4:
                field = payload.ljust(4, b"\0")
            else:
                field = struct.pack(order + "I", extra_at + len(extra))
                extra += payload + (b"\0" if len(payload) % 2 else b"")
            entries.append(struct.pack(order + "HHI", tag, typ, len(vals)) + field)
        last = k == len(pages) - 1
        struct.pack_into(order + "I", out, ifd_ptr_at, ifd_at)
        count = entry_count if (last and entry_count is not None) else len(entries)
        out += struct.pack(order + "H", count) + b"".join(entries)
        ifd_ptr_at = len(out)
        nxt = 0
        if last and next_ifd is not None:
            nxt = ifd_at if next_ifd == "self" else next_ifd
        out += struct.pack(order + "I", nxt) + extra
    return bytes(out)


COMP_CODE = {"none": 1, "lzw": 5, "lzw_pred": 5, "packbits": 32773}


def hand_tiff(arr, compression="none", rows_per_strip=None, order="<", lzw_clear=True, **page_kw):
    """one valid single-page file of the hand-written route"""
    rps = rows_per_strip or arr.shape[0]
    raws = raw_strips(arr, rps, order, predictor=compression == "lzw_pred")
    enc = {"none": lambda b: b, "lzw": lambda b: lzw_encode(b, lzw_clear)[0], "lzw_pred": lambda b: lzw_encode(b, lzw_clear)[0],
           "packbits": packbits_encode}[compression]
    page = dict(width=arr.shape[1], height=arr.shape[0], bits=arr.dtype.itemsize * 8, compression=COMP_CODE[compression],
                predictor=2 if compression == "lzw_pred" else 1, rps=rps, strips=[enc(r) for r in raws])
    page.update(page_kw)
    return write_tiff([page], order)


def check_with_pillow(data, arr):
    got = pil_decode(data)
    assert got.shape == arr.shape and np.array_equal(got.astype(np.int64), arr.astype(np.int64)), "the hand-written file does not decode to its source with Pillow"
    return data


def full_table_file():
    """a uint8 noise image whose single LZW strip never clears: the table fills and a few hundred codes follow (libtiff tolerates
    about a thousand).  -> (file, array)"""
    W = 64
    for H in range(60, 200, 2):
        arr = content("noise", (H, W), np.uint8, seed=5)
        _, n_codes, full = lzw_encode(raw_strips(arr, H)[0], clear_when_full=False)
        if full and n_codes > 3838 + 200:
            assert n_codes < 3838 + 900
            return hand_tiff(arr, "lzw", lzw_clear=False), arr
    raise AssertionError("no height fills the table")


def codes_to_bytes(codes, width=9):
    acc = nacc = 0
    out = bytearray()
    for c in codes:
        acc, nacc = (acc << width) | c, nacc + width
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 0xff)
            nacc -= 8
        acc &= (1 << nacc) - 1
    if nacc:
        out.append((acc << (8 - nacc)) & 0xff)
    return bytes(out)


def unsupported_files():
    """name -> (file, the reason tmat_tiff_probe must give).  All are (7, 5) pages."""
    a8 = content("smooth", (7, 5), np.uint8, 1)
    page = dict(width=5, height=7, bits=8, compression=1, strips=[a8.tobytes()])
    rgb = np.stack([a8, a8 // 2, a8 // 3], -1)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="TIFF")
    i32 = io.BytesIO()
    Image.fromarray(a8.astype(np.int32)).save(i32, format="TIFF")
    f32 = io.BytesIO()
    Image.fromarray(a8.astype(np.float32)).save(f32, format="TIFF")
    return {
        "deflate": (pil_tiff(a8, "deflate"), "compression"),
        "tiled": (write_tiff([dict(page, tile=True)]), "tiles"),
        "bigtiff": (write_tiff([page], magic=43), "bigtiff"),
        "rgb": (buf.getvalue(), "samples"),
        "int32": (i32.getvalue(), "bits"),
        "float32": (f32.getvalue(), "bits"),
        "min_is_white": (write_tiff([dict(page, photometric=0)]), "photometric"),
        "predictor_on_raw": (write_tiff([dict(page, predictor=2)]), "predictor"),
    }


def corrupt_files():
    """name -> (file, page to ask for, True if tmat_tiff_probe already says corrupt (else only the decoder can)).  (7, 5) uint8 pages."""
    a8 = content("smooth", (7, 5), np.uint8, 2)
    lzw_page = dict(width=5, height=7, bits=8, compression=5)
    good_lzw = lzw_encode(a8.tobytes())[0]
    whole = pil_tiff(content("smooth", (64, 80), np.uint8, 3), "lzw")
    raw_page = dict(width=5, height=7, bits=8, compression=1, strips=[a8.tobytes()])
    return {
        "truncated_file": (whole[: len(whole) // 2], 0, True),
        "truncated_strip": (write_tiff([dict(lzw_page, strips=[good_lzw], strip_counts=[len(good_lzw) // 2])]), 0, False),
        "raw_strip_short": (write_tiff([dict(raw_page, strip_counts=[20])]), 0, True),
        "offset_past_end": (write_tiff([dict(raw_page, strip_offsets=[1 << 20])]), 0, True),
        "offset_plus_count_wraps": (write_tiff([dict(raw_page, strip_offsets=[0xfffffff0], strip_counts=[0x20])]), 0, True),
        "strip_count_mismatch": (write_tiff([dict(raw_page, rps=2)]), 0, True),
        "code_above_free": (write_tiff([dict(lzw_page, strips=[codes_to_bytes([256, 65, 300, 66, 257])])]), 0, False),
        "first_code_not_literal": (write_tiff([dict(lzw_page, strips=[codes_to_bytes([256, 258, 66, 257])])]), 0, False),
        "eoi_too_early": (write_tiff([dict(lzw_page, strips=[codes_to_bytes([256, 65, 66, 257])])]), 0, False),
        "packbits_run_past_output": (write_tiff([dict(lzw_page, compression=32773, strips=[bytes([0x81, 7])])]), 0, False),
        "packbits_literals_past_input": (write_tiff([dict(lzw_page, compression=32773, strips=[bytes([30, 1, 2, 3])])]), 0, False),
        "ifd_loop": (write_tiff([raw_page], next_ifd="self"), 1, True),
        "ifd_past_end": (write_tiff([raw_page], next_ifd=1 << 24), 1, True),
        "entry_count_overruns": (write_tiff([raw_page], entry_count=0xffff), 0, True),
        "not_a_tiff": (b"\x89PNG\r\n\x1a\n" + bytes(32), 0, True),
        "too_short": (b"II*", 0, True),
    }


def dump(directory):
    """write the fixtures and a manifest for tools/tiff_sanitize.cpp: name, page, H, W, expected status, reference pixels"""
    from pathlib import Path
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    lines = []

    def put(name, data, page, shape, expect, ref=None):
        (d / f"{name}.tif").write_bytes(data)
        pix = ""
        if ref is not None:
            pix = f"{name}.p{page}.u16"
            (d / pix).write_bytes(np.ascontiguousarray(ref, np.uint16).tobytes())
        lines.append(f"{name}.tif {page} {shape[0]} {shape[1]} {expect} {pix}".rstrip())

    for shape in SHAPES:
        for dtype in DTYPES:
            for comp in COMPRESSIONS:
                for rps in grid_rows_per_strip(shape[0]):
                    for k, kind in enumerate(CONTENTS):
                        data = pil_tiff(content(kind, shape, dtype, seed=k + shape[0]), comp, rps or None)
                        put(f"grid_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}_{comp}_{rps}_{kind}", data, 0, shape, 0, pil_decode(data))
    pages = [content(k, (64, 80), np.uint16, i) for i, k in enumerate(("smooth", "noise", "checker"))]
    multi = pil_tiff(pages, "lzw_pred", 7)
    for pg in (2, 0, 1):
        put("multipage", multi, pg, (64, 80), 0, pil_decode(multi, pg))
    put("multipage", multi, 3, (64, 80), 2)
    for dtype in DTYPES:
        for comp, rps in (("none", 3), ("lzw_pred", 3), ("lzw", None), ("packbits", 2)):
            arr = content("ramp", (7, 5), dtype, 4)
            put(f"mm_{np.dtype(dtype).name}_{comp}", check_with_pillow(hand_tiff(arr, comp, rps, order=">"), arr), 0, (7, 5), 0, arr)
    full, arr = full_table_file()
    put("full_table", full, 0, arr.shape, 0, arr)
    for name, (data, _) in unsupported_files().items():
        put(f"unsupported_{name}", data, 0, (7, 5), 1)
    for name, (data, page, _) in corrupt_files().items():
        put(f"corrupt_{name}", data, page, (7, 5), 2)
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    return len(lines)


if __name__ == "__main__":
    import sys
    print(dump(sys.argv[1]), "cases written to", sys.argv[1])

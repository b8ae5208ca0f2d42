"""check_png: a PNG file of the library's encoder against the picture it was made from, through two decoders that are not the code
under test -- a walk of the file with zlib + an un-filter in numpy, and Pillow.  Plus the shapes and contents the PNG tests share."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunks_of(data: bytes):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND"""
    assert data[:8] == SIGNATURE, data[:8]
    out, p = [], 8
    while p < len(data):
        assert p + 12 <= len(data), "truncated chunk header"
        n, = struct.unpack(">I", data[p: p + 4])
        typ = data[p + 4: p + 8]
        assert p + 12 + n <= len(data), f"chunk {typ} runs past the file"
        body = data[p + 8: p + 8 + n]
        crc, = struct.unpack(">I", data[p + 8 + n: p + 12 + n])
        assert crc == zlib.crc32(typ + body), f"CRC of chunk {typ} at {p}"
        out.append((typ, body))
        p += 12 + n
        if typ == b"IEND":
            break
    assert p == len(data), f"{len(data) - p} bytes after IEND"
    return out


def unfilter(stream: np.ndarray, H: int, rb: int, bpp: int) -> np.ndarray:
    """the PNG specification's reconstruction of H filtered rows (1 + rb bytes each) -> (H, rb) u8"""
    rows = stream.reshape(H, rb + 1)
    out = np.zeros((H, rb), np.uint8)
    zero = np.zeros(rb, np.int32)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else zero
        if f == 0:
            cur = line
        elif f == 2:
            cur = line + up
        elif f == 1:
            cur = line.copy()
            for c in range(bpp):        # a running sum per channel
                cur[c::bpp] = np.cumsum(line[c::bpp])
        else:
            cur = np.zeros(rb, np.int32)
            for x in range(rb):
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(up[x])
                c = int(up[x - bpp]) if x >= bpp else 0
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (int(line[x]) + pred) & 255
        out[y] = (cur & 255).astype(np.uint8)
    return out


def check_png(data: bytes, pic: np.ndarray):
    """data is a complete, minimal PNG file of pic ((H, W) grey or (H, W, 3) RGB u8).  Returns the filter bytes of its rows."""
    from PIL import Image
    pic = np.asarray(pic)
    H, W = pic.shape[:2]
    ch = 3 if pic.ndim == 3 else 1
    ck = chunks_of(data)
    types = [t for t, _ in ck]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and len(types) >= 3, types
    assert all(t == b"IDAT" for t in types[1:-1]), types
    assert ck[-1][1] == b""
    assert ck[0][1] == struct.pack(">IIBBBBB", W, H, 8, 0 if ch == 1 else 2, 0, 0, 0), ck[0][1]
    z = zlib.decompressobj()
    raw = z.decompress(b"".join(body for _, body in ck[1:-1]))
    assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b""
    rb = W * ch
    assert len(raw) == H * (rb + 1), (len(raw), H * (rb + 1))
    stream = np.frombuffer(raw, np.uint8)
    filters = stream.reshape(H, rb + 1)[:, 0]
    assert filters.max() <= 4, filters.max()
    assert np.array_equal(unfilter(stream, H, rb, ch).reshape(pic.shape), pic), "numpy un-filter differs from the picture"
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.mode == ("L" if ch == 1 else "RGB"), im.mode
        assert np.array_equal(np.asarray(im), pic), "Pillow's pixels differ from the picture"
    return filters


# ---- shapes and contents (smallest at which the encoder can still go wrong) ----

def grey_with_stream(nbytes: int):
    """(H, W) of a grey picture whose filtered stream H (W + 1) has exactly nbytes bytes, H > 1 where a factor allows"""
    for H in (7, 5, 3, 2, 11, 13):
        if nbytes % H == 0 and nbytes // H >= 2:
            return H, nbytes // H - 1
    return 1, nbytes - 1


def content(kind: str, shape, seed: int = 0) -> np.ndarray:
    """u8 picture of shape (H, W) or (H, W, 3)"""
    rng = np.random.RandomState(seed)
    H, W = shape[:2]
    yy, xx = np.mgrid[:H, :W]
    if kind == "constant":
        a = np.full((H, W), 200)
    elif kind == "hramp":
        a = xx * 3
    elif kind == "vramp":
        a = yy * 5
    elif kind == "noise":
        return rng.randint(0, 256, shape).astype(np.uint8)
    elif kind == "blob":
        a = (((yy - 0.45 * H) ** 2 / max(1.0, (0.3 * H) ** 2) + (xx - 0.55 * W) ** 2 / max(1.0, (0.25 * W) ** 2)) < 1.0) * 255
    elif kind == "smooth":
        a = 127 + 100 * np.sin(yy / 17.0) * np.cos(xx / 23.0)
    elif kind == "pattern":         # one 300-byte string repeated through the whole picture, rows and stripes regardless
        return np.resize(rng.randint(0, 256, 300).astype(np.uint8), shape)
    else:
        raise ValueError(kind)
    a = (np.asarray(a).astype(np.int64) & 255).astype(np.uint8)
    return a if len(shape) == 2 else np.ascontiguousarray(np.stack([a, a[::-1], a.T if H == W else 255 - a], -1))


CONTENTS = ("constant", "hramp", "vramp", "noise", "blob", "smooth", "pattern")


def shapes(S: int):
    """{name: shape}: the shapes of the issue for a stripe of S bytes"""
    out = {"1x1": (1, 1), "1x1rgb": (1, 1, 3), "1x7": (1, 7), "7x1": (7, 1), "33x31rgb": (33, 31, 3), "401x37": (401, 37)}
    for name, nb in (("S-1", S - 1), ("S", S), ("S+1", S + 1), ("2S+1", 2 * S + 1)):
        out[name] = grey_with_stream(nb)
    out["row70000"] = (1, 70000)
    out["640"] = (640, 640)
    return out


def synthetic_tree(bh=60, bw=80):
    """a background (bh, bw) u16 and a small tree (segs (k, 4) f64, seg_branch (k) i32) over it"""
    rng = np.random.RandomState(5)
    bg = (rng.randint(0, 4000, (bh, bw)) + np.mgrid[:bh, :bw][1] * 500).astype(np.uint16)
    segs = np.array([[5, 5, 40, 30], [40, 30, 70, 20], [40, 30, 45, 55], [10, 50, 30, 40]], np.float64)
    return bg, (segs, np.array([0, 0, 1, 2], np.int32))

"""A small OpenEXR scanline reader and writer (the file layout of openexr.com/en/latest/OpenEXRFileLayout.html) for the UV maps of
the synthetic renders: the reference reads and writes them with cv2.imread(path, -1) / cv2.imwrite (neural_renderer_dataset.py:245,
face_image_normalizer.py:122-126), which is not installed here.

Reader: single-part scanline files, HALF and FLOAT channels without subsampling, compression NONE, ZIPS (one scanline per block) and
ZIP (16); anything else raises with the name of what it met.  Writer: uncompressed FLOAT.  `imread` / `imwrite` give and take cv2's
view of a colour file: (h, w, 3) float32 with the channels in the order B, G, R."""
import struct
import zlib

import numpy as np

MAGIC = 20000630
COMPRESSIONS = ("NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB")
LINES_PER_BLOCK = {"NONE": 1, "ZIPS": 1, "ZIP": 16}
PIXEL_TYPES = {1: np.dtype("<f2"), 2: np.dtype("<f4")}        # 0 is UINT: not a UV map


def _cstring(buf, pos):
    end = buf.index(b"\0", pos)
    return buf[pos:end].decode("latin-1"), end + 1


def _read_header(buf):
    magic, version = struct.unpack_from("<iI", buf, 0)
    if magic != MAGIC:
        raise ValueError("not an OpenEXR file (magic %#x)" % magic)
    for bit, what in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")):
        if version & bit:
            raise NotImplementedError("OpenEXR: %s files are not supported (single-part scanline files only)" % what)
    pos, attrs = 8, {}
    while buf[pos] != 0:
        name, pos = _cstring(buf, pos)
        kind, pos = _cstring(buf, pos)
        size, = struct.unpack_from("<i", buf, pos)
        attrs[name] = (kind, buf[pos + 4:pos + 4 + size])
        pos += 4 + size
    return attrs, pos + 1


def _channels(raw):
    pos, out = 0, []
    while raw[pos] != 0:
        name, pos = _cstring(raw, pos)
        ptype, _, xs, ys = struct.unpack_from("<iIii", raw, pos)
        pos += 16
        if ptype not in PIXEL_TYPES:
            raise NotImplementedError("OpenEXR: channel %s has pixel type %d (HALF and FLOAT only)" % (name, ptype))
        if (xs, ys) != (1, 1):
            raise NotImplementedError("OpenEXR: channel %s is subsampled (%d, %d)" % (name, xs, ys))
        out.append((name, PIXEL_TYPES[ptype]))
    return out


def unzip_block(data):
    """The ZIP / ZIPS block coding undone: inflate, then the byte predictor d[i] += d[i - 1] - 128, then the two halves (the bytes
    at even and at odd positions) interleaved again."""
    d = np.frombuffer(zlib.decompress(data), np.uint8).copy()
    d[1:] -= 128                                                        # (uint8 arithmetic wraps: everything here is modulo 256)
    d = np.cumsum(d, dtype=np.uint8)
    half = (d.size + 1) // 2
    out = np.empty(d.size, np.uint8)
    out[0::2] = d[:half]
    out[1::2] = d[half:]
    return out.tobytes()


def read_exr(path):
    """-> {channel name: (h, w) array of the file's type}, in the file's (alphabetical) channel order."""
    with open(path, "rb") as fp:
        buf = fp.read()
    attrs, pos = _read_header(buf)
    code = attrs["compression"][1][0]
    compression = COMPRESSIONS[code] if code < len(COMPRESSIONS) else "unknown (%d)" % code
    if compression not in LINES_PER_BLOCK:
        raise NotImplementedError("OpenEXR: compression %s is not supported (NONE, ZIPS, ZIP)" % compression)
    channels = _channels(attrs["channels"][1])
    x_min, y_min, x_max, y_max = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x_max - x_min + 1, y_max - y_min + 1
    lines = LINES_PER_BLOCK[compression]
    n_blocks = (h + lines - 1) // lines
    offsets = struct.unpack_from("<%dQ" % n_blocks, buf, pos)
    line_bytes = sum(dt.itemsize for _, dt in channels) * w
    raw = np.empty((h, line_bytes), np.uint8)                           # the scanlines as the file lays them out
    step = 8 + line_bytes
    if compression == "NONE" and len(buf) >= offsets[0] + h * step and offsets == tuple(range(offsets[0], offsets[0] + h * step, step)):
        # uncompressed chunks back to back (what every writer makes): one strided view instead of a loop over the scanlines
        chunks = np.frombuffer(buf, np.uint8, h * step, offsets[0]).reshape(h, step)
        ys = chunks[:, :4].copy().view("<i4").ravel() - y_min
        sizes = chunks[:, 4:8].copy().view("<i4").ravel()
        if not (np.array_equal(np.sort(ys), np.arange(h)) and (sizes == line_bytes).all()):
            raise ValueError("OpenEXR: %s: scanline chunks do not cover the data window" % path)
        raw[ys] = chunks[:, 8:]
    else:
        for off in offsets:
            y, size = struct.unpack_from("<ii", buf, off)
            row0 = y - y_min
            if not 0 <= row0 < h:
                raise ValueError("OpenEXR: block at scanline %d outside the data window" % y)
            rows = min(lines, h - row0)
            data = buf[off + 8:off + 8 + size]
            if len(data) != size:
                raise ValueError("OpenEXR: truncated block at scanline %d" % y)
            if compression != "NONE" and size < rows * line_bytes:     # (a block that did not shrink is stored as it is)
                data = unzip_block(data)
            if len(data) != rows * line_bytes:
                raise ValueError("OpenEXR: block at scanline %d holds %d bytes, expected %d" % (y, len(data), rows * line_bytes))
            raw[row0:row0 + rows] = np.frombuffer(data, np.uint8).reshape(rows, line_bytes)
    planes, at = {}, 0
    for name, dt in channels:                                           # per scanline: every channel's row, one after the other
        planes[name] = np.ascontiguousarray(raw[:, at:at + dt.itemsize * w]).view(dt)
        at += dt.itemsize * w
    return planes


def _attr(name, kind, value):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def write_exr(path, planes):
    """planes: {channel name: (h, w) array}; written as uncompressed FLOAT scanlines, channels in alphabetical order."""
    names = sorted(planes)
    arrays = [np.ascontiguousarray(planes[k], "<f4") for k in names]
    h, w = arrays[0].shape
    assert all(a.shape == (h, w) for a in arrays)
    chlist = b"".join(k.encode() + b"\0" + struct.pack("<iIii", 2, 0, 1, 1) for k in names) + b"\0"
    window = struct.pack("<4i", 0, 0, w - 1, h - 1)
    header = struct.pack("<iI", MAGIC, 2)
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", b"\0")
    header += _attr("dataWindow", "box2i", window) + _attr("displayWindow", "box2i", window)
    header += _attr("lineOrder", "lineOrder", b"\0") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    header += _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    header += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    line_bytes = 4 * w * len(names)
    first = len(header) + 8 * h
    offsets = struct.pack("<%dQ" % h, *[first + y * (8 + line_bytes) for y in range(h)])
    chunks = np.empty((h, 8 + line_bytes), np.uint8)                    # per scanline: y, byte count, channel after channel
    chunks[:, :4] = np.arange(h, dtype="<i4").view(np.uint8).reshape(h, 4)
    chunks[:, 4:8] = np.frombuffer(struct.pack("<i", line_bytes), np.uint8)
    chunks[:, 8:] = np.stack(arrays, axis=1).reshape(h, -1).view(np.uint8)
    with open(path, "wb") as fp:
        fp.write(header + offsets)
        fp.write(chunks.tobytes())


def imread(path):
    """cv2.imread(path, -1) of a colour EXR: (h, w, 3) float32, channels B, G, R (HALF widened to float32)."""
    planes = read_exr(path)
    missing = [k for k in "BGR" if k not in planes]
    if missing:
        raise ValueError("OpenEXR: %s has the channels %s, B, G and R are needed" % (path, sorted(planes)))
    return np.stack([planes[k].astype(np.float32) for k in "BGR"], axis=-1)


def imwrite(path, image):
    """cv2.imwrite(path, image) of an (h, w, 3) float32 B, G, R image."""
    image = np.asarray(image, np.float32)
    assert image.ndim == 3 and image.shape[2] == 3
    write_exr(path, {k: image[:, :, i] for i, k in enumerate("BGR")})

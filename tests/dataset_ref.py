"""Reference arithmetic of the dataset-creation tests, written apart from confignet_amd/face_image_normalizer.py: plain Python
integers pixel by pixel (no numpy broadcasting shared with the package), and a float64 statement of the same resampling.

  tables      cv2's warpAffine keeps the inverted transform as int32 tables with 10 fractional bits: adelta[x] = rint(m0 x 1024),
              bdelta[x] = rint(m3 x 1024), X0[y] = rint((m1 y + m2) 1024) + delta, Y0[y] = rint((m4 y + m5) 1024) + delta
              (delta 16 bilinear, 512 nearest; rint = round half to even; saturated to int32)
  bilinear    X = (X0[y] + adelta[x]) >> 5, sx = X >> 5, ax = X & 31 (Y likewise); four taps, 0 outside; (sum w p + 16384) >> 15
  float64     the exact bilinear value at (X / 32, Y / 32), then floor(v + 0.5): every weight is a multiple of 1/1024 and every
              pixel an integer below 256, so float64 holds the sum exactly and the two statements must give the same byte
  nearest     sx = (X0[y] + adelta[x]) >> 10

Also: synthetic OpenFace output and renders for the end-to-end tests, and an InceptionV3 feature extractor on the float64 oracle
for machines without a GPU."""
import json
import math
import os
import struct
import zlib

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _sat(v):
    if math.isnan(v):
        return I32_MIN
    if math.isinf(v):
        return I32_MAX if v > 0 else I32_MIN
    return max(I32_MIN, min(I32_MAX, round(v)))          # Python's round: half to even, exact on floats


def inverse(M):
    (a, b, c), (d, e, f) = [[float(v) for v in row] for row in M]
    det = a * e - b * d
    det = 1.0 / det if det != 0 else 0.0
    ia, ib, id_, ie = e * det, -b * det, -d * det, a * det
    return [ia, ib, -ia * c - ib * f, id_, ie, -id_ * c - ie * f]


def tables(M, oh, ow, delta):
    m = inverse(M)
    adelta = [_sat(m[0] * x * 1024.0) for x in range(ow)]
    bdelta = [_sat(m[3] * x * 1024.0) for x in range(ow)]
    x0 = [max(I32_MIN, min(I32_MAX, _sat((m[1] * y + m[2]) * 1024.0) + delta)) for y in range(oh)]
    y0 = [max(I32_MIN, min(I32_MAX, _sat((m[4] * y + m[5]) * 1024.0) + delta)) for y in range(oh)]
    return x0, y0, adelta, bdelta


def stack_tables(per_image):
    """[(x0, y0, adelta, bdelta) per image] -> four int32 arrays (n, oh), (n, oh), (n, ow), (n, ow)"""
    return tuple(np.array([t[k] for t in per_image], dtype=np.int64).astype(np.int32) for k in range(4))


def _px(img, y, x):
    h, w = len(img), len(img[0])
    return img[y][x] if 0 <= y < h and 0 <= x < w else None


def warp_u8_int(img, tabs, oh, ow):
    """img (sh, sw, c) uint8, tabs = (x0, y0, adelta, bdelta) as sequences of Python ints -> (oh, ow, c) uint8"""
    x0, y0, adelta, bdelta = [[int(v) for v in t] for t in tabs]
    src = np.asarray(img).tolist()
    c = np.asarray(img).shape[2]
    out = np.zeros((oh, ow, c), np.uint8)
    for y in range(oh):
        for x in range(ow):
            X, Y = (x0[y] + adelta[x]) >> 5, (y0[y] + bdelta[x]) >> 5
            sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
            taps = ((sy, sx, 32 * (32 - ax) * (32 - ay)), (sy, sx + 1, 32 * ax * (32 - ay)),
                    (sy + 1, sx, 32 * (32 - ax) * ay), (sy + 1, sx + 1, 32 * ax * ay))
            assert sum(t[2] for t in taps) == 32768
            for k in range(c):
                acc = 0
                for ty, tx, wt in taps:
                    p = _px(src, ty, tx)
                    if p is not None:
                        acc += wt * p[k]
                out[y, x, k] = (acc + 16384) >> 15
    return out


def warp_u8_float64(img, tabs, oh, ow):
    x0, y0, adelta, bdelta = [[int(v) for v in t] for t in tabs]
    src = np.asarray(img).astype(np.float64)
    sh, sw, c = src.shape
    out = np.zeros((oh, ow, c), np.uint8)

    def at(yy, xx):
        return src[yy, xx] if 0 <= yy < sh and 0 <= xx < sw else np.zeros(c)

    for y in range(oh):
        for x in range(ow):
            fx, fy = ((x0[y] + adelta[x]) >> 5) / 32.0, ((y0[y] + bdelta[x]) >> 5) / 32.0
            ix, iy = math.floor(fx), math.floor(fy)
            tx, ty = fx - ix, fy - iy
            v = (1 - ty) * ((1 - tx) * at(iy, ix) + tx * at(iy, ix + 1)) + ty * ((1 - tx) * at(iy + 1, ix) + tx * at(iy + 1, ix + 1))
            out[y, x] = np.floor(v + 0.5)
    return out


def warp_nearest(img, tabs, oh, ow):
    x0, y0, adelta, bdelta = [[int(v) for v in t] for t in tabs]
    src = np.asarray(img)
    sh, sw, c = src.shape
    out = np.zeros((oh, ow, c), src.dtype)
    for y in range(oh):
        for x in range(ow):
            sx, sy = (x0[y] + adelta[x]) >> 10, (y0[y] + bdelta[x]) >> 10
            if 0 <= sx < sw and 0 <= sy < sh:
                out[y, x] = src[sy, sx]
    return out


# the reference's EyeRegionSpec (neural_renderer_dataset.py:61-69), restated
EYE_L = (0.09, 0.16)
EYE_R = (0.84, 0.91)
EYE_Y = (0.07, 0.15)


def eye_mask(uv):
    """uv (..., c >= 2) float32: a float32 array compared with a Python float is compared with the float32 of that float"""
    u, v = np.asarray(uv, np.float32)[..., 0], np.asarray(uv, np.float32)[..., 1]
    f = np.float32
    in_y = (v < f(EYE_Y[1])) & (v > f(EYE_Y[0]))
    left = (u < f(EYE_L[1])) & (u > f(EYE_L[0]))
    right = (u < f(EYE_R[1])) & (u > f(EYE_R[0]))
    return ((left & in_y) | (right & in_y)).astype(np.uint8)


def threshold_uv():
    """A (3, 12, 3) UV map whose pixels sit on every float32 bound and one float32 step to either side of it (u with v inside its
    range, v with u inside the left and the right range), plus NaN and infinities."""
    f = np.float32
    around = lambda b: [np.nextafter(f(b), f(-1)), f(b), np.nextafter(f(b), f(2))]
    us = [x for b in EYE_L + EYE_R for x in around(b)]
    vs = [x for b in EYE_Y for x in around(b)]
    uv = np.zeros((3, 12, 3), np.float32)
    uv[0, :, 0], uv[0, :, 1] = us, f(0.1)
    uv[1, :6, 0], uv[1, :6, 1] = f(0.1), vs
    uv[1, 6:, 0], uv[1, 6:, 1] = f(0.9), vs
    uv[2, :, 0] = [np.nan, np.inf, -np.inf, 0.1, 0.9, 0.5, 0.1, 0.9, 0.0, 1.0, 0.125, 0.875]
    uv[2, :, 1] = [0.1, 0.1, 0.1, np.nan, np.inf, 0.1, 0.1, 0.1, 0.1, 0.1, 0.0, 0.2]
    uv[:, :, 2] = 7.0
    return uv


# ---- OpenEXR blocks built from the documented coding --------------------------------------------------------------------------
def zip_block(raw):
    """The ZIP / ZIPS coding of OpenEXR: bytes at even positions, then bytes at odd positions; then each byte replaced by its
    difference to its predecessor plus 128; then deflate."""
    b = np.frombuffer(raw, np.uint8)
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int64)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 255
    return zlib.compress(d.astype(np.uint8).tobytes())


def write_exr_compressed(path, planes, compression):
    """planes {name: (h, w) float16 / float32}; compression "ZIPS" (1 line per block) or "ZIP" (16)"""
    names = sorted(planes)
    h, w = planes[names[0]].shape
    code, lines = {"ZIPS": (2, 1), "ZIP": (3, 16)}[compression]

    def attr(name, kind, value):
        return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value

    chlist = b"".join(k.encode() + b"\0" + struct.pack("<iIii", 1 if planes[k].dtype == np.float16 else 2, 0, 1, 1) for k in names) + b"\0"
    win = struct.pack("<4i", 0, 0, w - 1, h - 1)
    head = struct.pack("<iI", 20000630, 2) + attr("channels", "chlist", chlist) + attr("compression", "compression", bytes([code]))
    head += attr("dataWindow", "box2i", win) + attr("displayWindow", "box2i", win) + attr("lineOrder", "lineOrder", b"\0")
    head += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0))
    head += attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    chunks = []
    for y in range(0, h, lines):
        raw = b"".join(planes[k][r].astype(planes[k].dtype.newbyteorder("<")).tobytes() for r in range(y, min(h, y + lines)) for k in names)
        packed = zip_block(raw)
        data = packed if len(packed) < len(raw) else raw                  # a block that does not shrink is stored raw
        chunks.append(struct.pack("<ii", y, len(data)) + data)
    at, offsets = len(head) + 8 * len(chunks), []
    for ch in chunks:
        offsets.append(at)
        at += len(ch)
    with open(path, "wb") as fp:
        fp.write(head + struct.pack("<%dQ" % len(offsets), *offsets) + b"".join(chunks))


# ---- synthetic OpenFace output and renders --------------------------------------------------------------------------------------
def face_landmarks_3d(scale=1.0):
    """68 head-frame 3-D points (mm): a deterministic cloud with the landmarks the normaliser reads placed like a face."""
    rng = np.random.default_rng(68)
    pts = rng.uniform(-40, 40, size=(68, 3)) * [1.0, 1.0, 0.2]
    pts[0], pts[16] = (-70, 0, 60), (70, 0, 60)                     # jaw ends: the head centre lies between them
    pts[36], pts[39], pts[42], pts[45] = (-45, -30, 0), (-15, -30, 0), (15, -30, 0), (45, -30, 0)
    pts[30], pts[48], pts[54], pts[51] = (0, 5, -15), (-25, 40, 0), (25, 40, 0), (0, 32, -5)
    return pts * scale


def project(points, K):
    p = points @ K.T
    return p[:, :2] / p[:, 2:]


def openface_csv_row(face_id, confidence, landmarks_2d, landmarks_3d, pose):
    return [face_id, confidence] + list(pose) + list(landmarks_2d[:, 0]) + list(landmarks_2d[:, 1]) + \
        list(landmarks_3d[:, 0]) + list(landmarks_3d[:, 1]) + list(landmarks_3d[:, 2])


def write_openface_files(processed_dir, name, rows, K):
    """`<name>.csv` with OpenFace's space-padded header and `<name>_of_details.txt` with the camera on its third line"""
    os.makedirs(processed_dir, exist_ok=True)
    cols = ["face", "confidence", "pose_Tx", "pose_Ty", "pose_Tz", "pose_Rx", "pose_Ry", "pose_Rz"]
    cols += ["x_%d" % i for i in range(68)] + ["y_%d" % i for i in range(68)]
    cols += ["%s_%d" % (a, i) for a in "XYZ" for i in range(68)]
    with open(os.path.join(processed_dir, name + ".csv"), "w") as fp:
        fp.write(", ".join(cols) + "\n")
        for row in rows:
            fp.write(", ".join(repr(float(v)) for v in row) + "\n")
    with open(os.path.join(processed_dir, name + "_of_details.txt"), "w") as fp:
        fp.write("Input:%s\nCamera:0\nCamera parameters:%r,%r,%r,%r\n" % (name, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])))


def write_render_tree(root, n=3, h=40, w=48, out_of_range=(2,), with_landmarks=True, seed=0):
    """n synthetic renders img_<i>.png (h x w) with uv_<i>.exr, meta_<i>.json, OpenFace files, the CelebA attribute list and the
    `landmarks_detected` marker.  Renders listed in out_of_range get a head pose outside the dataset's range.  -> (images in B, G, R, uv maps)"""
    from PIL import Image
    from confignet_amd import exr
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    K = np.array([[700.0, 0, w / 2], [0, 700.0, h / 2], [0, 0, 1]])
    imgs, uvs = [], []
    attr_lines = ["%d" % n, "Smiling Young"]
    for i in range(n):
        name = "img_%05d" % i
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        Image.fromarray(img[:, :, ::-1].copy()).save(os.path.join(root, name + ".png"))
        yy, xx = np.mgrid[0:h, 0:w]
        # u sweeps through the left and the right eye range along x, v through the eye band along y; channel 2 is unused
        uv = np.stack([(xx / (w - 1)).astype(np.float32), (yy / (h - 1) * 0.3).astype(np.float32), np.zeros((h, w), np.float32)], axis=-1)
        exr.imwrite(os.path.join(root, "uv_%05d.exr" % i), uv)
        head = [0.5, 0.0, 0.0] if i in out_of_range else [0.05 * i, 0.0, 0.1 * i]
        meta = {"bone_rotations": {"head": head, "left_eye": [0.0, 0.0, 0.01 * i], "jaw": [0.1 * i, 0.0, 0.0]},
                "hair_style": ["short", "long", None][i % 3], "beard_style": "none" if i % 2 else "full",
                "blendshape_values": {"smile": 0.1 * i, "brow_up": 0.2}, "texture_embedding": [0.1 * i, 0.2, 0.3]}
        with open(os.path.join(root, "meta_%05d.json" % i), "w") as fp:
            json.dump(meta, fp)
        pose = np.array([2.0 * i, -3.0, 400.0 + 10 * i, 0.0, 0.0, 0.0])
        l3 = face_landmarks_3d(0.12) + pose[:3]
        if with_landmarks:
            write_openface_files(os.path.join(root, "processed"), name, [openface_csv_row(0, 0.98, project(l3, K), l3, pose)], K)
        attr_lines.append("%s.jpg %s %s" % (name, "1" if i % 2 else "-1", "-1" if i % 3 else "1"))
        imgs.append(img)
        uvs.append(uv)
    with open(os.path.join(root, "list_attr_celeba.txt"), "w") as fp:
        fp.write("\n".join(attr_lines) + "\n")
    if with_landmarks:
        open(os.path.join(root, "landmarks_detected"), "w").close()
    return imgs, uvs


class OracleFeatureExtractor:
    """InceptionFeatureExtractor's interface on the float64 oracle (oracle/ref_metrics.py) with seeded He weights: the Inception
    side of the pipeline on a machine without a GPU."""

    def __init__(self, seed=0):
        import torch
        from oracle import ref_metrics as M
        rng = np.random.default_rng(seed)
        self.M, self.torch = M, torch
        self.weights, bn_slot = [], 0
        for shape in M.inception_weight_shapes():                   # kernel | beta, moving mean, moving variance
            if len(shape) == 4:
                self.weights.append(rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2])))
            else:
                self.weights.append(np.ones(shape) if bn_slot % 3 == 2 else np.zeros(shape))
                bn_slot += 1

    def get_features(self, images):
        t = self.torch
        x = t.tensor(np.asarray(images, np.float64) / 127.5 - 1.0)
        with t.no_grad():
            return self.M.inception_features([t.tensor(w) for w in self.weights], x).numpy().astype(np.float32)

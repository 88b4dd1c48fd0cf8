"""Face image normalisation (reference: confignet/face_image_normalizer.py): pre-normalisation on five 2-D landmark groups, then the
3-D head-centre normalisation, each a cv2.warpAffine of the picture (bilinear) and of its UV map (nearest).

cv2 is not installed here, so warpAffine is restated: cv2 does the coordinate arithmetic in double on the host and keeps it as int32
tables with 10 fractional bits; `affine_tables` builds those tables, and the resampling behind them is integer-only -- in numpy
(`device=None`) or by cn_warp_affine_u8 / cn_warp_nearest_f32 (csrc/dataset.hip), which give the same bytes.  DESIGN.md section 7
lists what of cv2 this cannot pin ([cv2 unpinned]).  Pictures are decoded with Pillow and held in cv2's B, G, R order."""
import glob
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import dataset_utils, exr

repo_root_dir_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
# (the reference points at its bundled Windows build; here: the user's own FaceLandmarkImg)
DEFAULT_OPENFACE_PATH = os.environ.get("OPENFACE_PATH") or os.path.join(repo_root_dir_path, "3rd_party", "OpenFace", "build", "bin",
                                                                         "FaceLandmarkImg")

AB_BITS = 10                    # cv2 imgwarp.cpp: fractional bits of the coordinate tables
INTER_BITS = 5                  # 32 x 32 bilinear positions per pixel
ROUND_DELTA_LINEAR = 1 << (AB_BITS - INTER_BITS - 1)        # 16
ROUND_DELTA_NEAREST = 1 << (AB_BITS - 1)                    # 512
MAX_THREADS = 16
CHUNK = 64                      # pictures decoded, warped and written at a time
DONE_FILE = "normalization_done"


def pick_device(name=None):
    """The device rule of the command lines: a torch device string as given, "none" for the numpy path, and without a choice the
    GPU when there is one."""
    if name is None:
        import torch
        return "cuda" if torch.cuda.is_available() else None
    return None if name.lower() == "none" else name


def _project(points, K):
    """pinhole projection of the rows of points (n, 3) with the camera matrix K -> (n, 2) pixels"""
    homogeneous = points @ K.T
    return homogeneous[:, :2] / homogeneous[:, 2:3]


# ---- files ----------------------------------------------------------------------------------------------------------------
def imread(path):
    """cv2.imread(path): (h, w, 3) uint8 in B, G, R order."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def imwrite(path, image):
    """cv2.imwrite(path, image) of an (h, w, 3) B, G, R (or (h, w) grey) uint8 image; JPEG at cv2's default quality 95."""
    from PIL import Image
    image = np.asarray(image, np.uint8)
    im = Image.fromarray(np.ascontiguousarray(image[:, :, ::-1]) if image.ndim == 3 else image)
    if os.path.splitext(path)[1].lower() in (".jpg", ".jpeg"):
        im.save(path, quality=95)
    else:
        im.save(path)


def thread_map(fn, items):
    items = list(items)
    if len(items) <= 1:
        return [fn(i) for i in items]
    with ThreadPoolExecutor(max_workers=min(MAX_THREADS, len(items))) as pool:
        return list(pool.map(fn, items))


# ---- transformations.euler_matrix(ai, aj, ak, axes="rxyz")[:3, :3] -----------------------------------------------------------
def euler_matrix_rxyz(ai, aj, ak):
    """The `transformations` package (Gohlke) is not installed; its euler_matrix restated for axes "rxyz", which its table codes as
    (firstaxis 2, parity 1, repetition 0, frame 1): i, j, k = 2, 1, 0, a rotating frame (the first and the last angle change
    places) and odd parity (all three change sign).  The result is Rx(ai) Ry(aj) Rz(ak), which scipy calls
    Rotation.from_euler("XYZ", (ai, aj, ak)) (intrinsic; tests/test_dataset_creation_cpu.py holds the comparison)."""
    i, j, k = 2, 1, 0
    ai, aj, ak = -ak, -aj, -ai
    si, sj, sk = np.sin(ai), np.sin(aj), np.sin(ak)
    ci, cj, ck = np.cos(ai), np.cos(aj), np.cos(ak)
    cc, cs = ci * ck, ci * sk
    sc, ss = si * ck, si * sk
    M = np.empty((3, 3))
    M[i, i], M[i, j], M[i, k] = cj * ck, sj * sc - cs, sj * cc + ss
    M[j, i], M[j, j], M[j, k] = cj * sk, sj * ss + cc, sj * cs - sc
    M[k, i], M[k, j], M[k, k] = -sj, cj * si, cj * ci
    return M


# ---- cv2.warpAffine: the host half ------------------------------------------------------------------------------------------
def invert_affine(M):
    """What cv2.warpAffine does to M (destination <- source) before it walks the destination (imgwarp.cpp, no WARP_INVERSE_MAP)."""
    m = np.array(M, dtype=np.float64).reshape(6)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _saturate_i32(v):
    """Round half to even and clamp to int32; NaN becomes INT32_MIN.  cv2's saturate_cast<int>(double) is cvRound, whose cvtsd2si
    gives INT32_MIN for EVERY value outside int32, a positive overflow included: there this clamps to INT32_MAX instead.  Either
    entry puts the pixel far outside any source (<= 32767 wide), so the picture is the same; the table is not."""
    v = np.rint(np.asarray(v, np.float64))
    v = np.where(np.isnan(v), -2.0 ** 31, v)
    return np.clip(v, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def affine_tables(M, oh, ow, round_delta):
    """cv2's coordinate tables of warpAffine(img, M, (ow, oh)): (x0 (oh), y0 (oh), adelta (ow), bdelta (ow)) int32."""
    m = invert_affine(M)
    x = np.arange(ow, dtype=np.float64)
    y = np.arange(oh, dtype=np.float64)
    scale = float(1 << AB_BITS)
    with np.errstate(all="ignore"):
        adelta = _saturate_i32(m[0] * x * scale)
        bdelta = _saturate_i32(m[3] * x * scale)
        x0 = np.clip(_saturate_i32((m[1] * y + m[2]) * scale) + round_delta, -2 ** 31, 2 ** 31 - 1)
        y0 = np.clip(_saturate_i32((m[4] * y + m[5]) * scale) + round_delta, -2 ** 31, 2 ** 31 - 1)
    return tuple(t.astype(np.int32) for t in (x0, y0, adelta, bdelta))


def batch_tables(Ms, oh, ow, round_delta):
    """One set of tables per transform, stacked: (n, oh), (n, oh), (n, ow), (n, ow)."""
    per = [affine_tables(M, oh, ow, round_delta) for M in Ms]
    return tuple(np.stack([p[k] for p in per]) for k in range(4))


# ---- the resampling half, numpy (csrc/dataset.hip is the same arithmetic) ---------------------------------------------------
def _tap(src, n_idx, sy, sx):
    """src[n, sy, sx] with 0 outside the source; sy, sx int64 of any size"""
    _, sh, sw, _ = src.shape
    inside = (sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)
    v = src[n_idx, np.where(inside, sy, 0), np.where(inside, sx, 0)]
    return np.where(inside[..., None], v, 0)


def warp_affine_u8_tables(src, tables):
    x0, y0, adelta, bdelta = [np.asarray(t).astype(np.int64) for t in tables]
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    X = (x0[:, :, None] + adelta[:, None, :]) >> (AB_BITS - INTER_BITS)
    Y = (y0[:, :, None] + bdelta[:, None, :]) >> (AB_BITS - INTER_BITS)
    sx, sy = X >> INTER_BITS, Y >> INTER_BITS
    ax, ay = (X & 31)[..., None], (Y & 31)[..., None]
    n_idx = np.arange(src.shape[0])[:, None, None]
    s64 = src.astype(np.int64)
    acc = 32 * (32 - ax) * (32 - ay) * _tap(s64, n_idx, sy, sx) + 32 * ax * (32 - ay) * _tap(s64, n_idx, sy, sx + 1) \
        + 32 * (32 - ax) * ay * _tap(s64, n_idx, sy + 1, sx) + 32 * ax * ay * _tap(s64, n_idx, sy + 1, sx + 1)
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_nearest_f32_tables(src, tables):
    x0, y0, adelta, bdelta = [np.asarray(t).astype(np.int64) for t in tables]
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 4
    sx = (x0[:, :, None] + adelta[:, None, :]) >> AB_BITS
    sy = (y0[:, :, None] + bdelta[:, None, :]) >> AB_BITS
    return _tap(src, np.arange(src.shape[0])[:, None, None], sy, sx).astype(np.float32)


def _on_device(fn, src, tables, oh, ow, device):
    import torch
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = fn(torch.from_numpy(np.ascontiguousarray(src)).to(dev), [torch.from_numpy(t).to(dev) for t in tables], oh, ow)
        return out.cpu().numpy()


def _one_by_one(fn, images, tables):
    """The numpy forms hold int64 copies of every tap: one picture per call, the calls spread over the thread pool."""
    return np.stack(thread_map(lambda i: fn(images[i:i + 1], [t[i:i + 1] for t in tables])[0], range(len(images))))


def warp_affine(images, Ms, dsize, device=None):
    """cv2.warpAffine(image, M, dsize) for a batch: images (n, sh, sw, c) uint8, Ms n transforms (2, 3), dsize = (width, height)."""
    ow, oh = int(dsize[0]), int(dsize[1])
    tables = batch_tables(Ms, oh, ow, ROUND_DELTA_LINEAR)
    if device is None:
        return _one_by_one(warp_affine_u8_tables, images, tables)
    from . import ops
    return _on_device(ops.warp_affine_u8, images, tables, oh, ow, device)


def warp_affine_nearest(images, Ms, dsize, device=None):
    """cv2.warpAffine(image, M, dsize, flags=cv2.INTER_NEAREST) for a batch of float32 images."""
    ow, oh = int(dsize[0]), int(dsize[1])
    tables = batch_tables(Ms, oh, ow, ROUND_DELTA_NEAREST)
    if device is None:
        return _one_by_one(warp_nearest_f32_tables, images, tables)
    from . import ops
    return _on_device(ops.warp_nearest_f32, images, tables, oh, ow, device)


def _warp_grouped(arrays, Ms, dsize, warp, device):
    """Arrays of equal shape go through one call of `warp`; results in the order of `arrays`."""
    groups = {}
    for i, a in enumerate(arrays):
        groups.setdefault(a.shape, []).append(i)
    out = [None] * len(arrays)
    for idxs in groups.values():
        res = warp(np.stack([arrays[i] for i in idxs]), [Ms[i] for i in idxs], dsize, device)
        for k, i in enumerate(idxs):
            out[i] = res[k]
    return out


class FaceImageNormalizer:
    """Brings face pictures into the framing ConfigNet was trained on (reference: confignet/face_image_normalizer.py; the constants,
    method names and file layout are the reference's, the bodies are restated).

    Two warps.  The pre-normalisation (real photos only; renders are centred already) maps five 2-D landmark groups onto fixed
    positions of a 1024 x 1024 picture, because the 3-D step is unreliable on off-centre faces.  The head-centre normalisation
    then projects the middle of the head from the 3-D landmarks and puts it at `ref_head_center_coords` of the output, scaled by
    the eye and eye-to-mouth distances of the head turned frontal and rotated so that the eyes are level.  OpenFace supplies the
    landmarks and runs once before each warp (dataset_utils.run_openface_on_dir)."""

    # pre-normalisation: landmark groups (a group is the mean of its landmarks) and where they go, as fractions of the picture;
    # pre_norm_face_scale shrinks the layout about the centre (1.0: the face fills most of the picture)
    ref_pre_norm_landmark_idxs = ((36, 39), (42, 45), (30,), (48,), (54,))
    ref_pre_norm_landmark_positions = np.array(((0.32, 0.45), (0.68, 0.45), (0.5, 0.6), (0.34, 0.82), (0.66, 0.82)))
    pre_norm_face_scale = 0.5
    pre_norm_image_size = 1024
    ref_pre_norm_landmark_positions = (ref_pre_norm_landmark_positions - 0.5) * pre_norm_face_scale + 0.5

    # head-centre normalisation
    ref_head_center_coords = (0.5, 0.42),           # (kept as the reference has it: a 1 x 2 tuple of tuples)
    eye_corner_idxs = (36, 45)
    mouth_top_idx = (51)
    head_center_idxs = (0, 16)                      # the head centre is taken midway between these two 3-D landmarks
    interocular_fraction = 0.45                     # outer eye corners: this share of the output width apart
    eye_to_mouth_fraction = 0.34                    # eye midpoint to upper lip: this share of the output height

    image_filename_patterns = ("*.jpg", "*.png", "*.bmp", "*.jpeg")

    @staticmethod
    def _mark_done(directory):
        open(os.path.join(directory, DONE_FILE), "w").close()

    @classmethod
    def normalize_dataset_dir(cls, input_dir, pre_normalize, output_image_shape, openface_path=DEFAULT_OPENFACE_PATH,
                              write_done_file=True, device=None):
        """input_dir/normalized (and input_dir/pre_normalized on the way) from the pictures of input_dir; a directory that holds
        its `normalization_done` marker is not made again.  A landmark pass that cannot run raises before the marker of the step
        that needs it is written, so a later call picks up where the user has supplied the landmark files."""
        normalized = os.path.join(input_dir, "normalized")
        if os.path.exists(os.path.join(normalized, DONE_FILE)):
            return
        dataset_utils.run_openface_on_dir(input_dir, openface_path)
        source = input_dir
        if pre_normalize:
            source = os.path.join(input_dir, "pre_normalized")
            if not os.path.exists(os.path.join(source, DONE_FILE)):
                side = cls.pre_norm_image_size
                cls._normalize_directory(input_dir, source, True, (side, side), device=device)
                dataset_utils.run_openface_on_dir(source, openface_path)
                if write_done_file:
                    cls._mark_done(source)
        cls._normalize_directory(source, normalized, False, output_image_shape, device=device)
        if write_done_file:
            cls._mark_done(normalized)

    @classmethod
    def normalize_individual_image(cls, image, output_image_shape, openface_path=DEFAULT_OPENFACE_PATH, device=None):
        """One B, G, R picture through both warps by way of a temporary directory; None when no face was found in it."""
        with tempfile.TemporaryDirectory() as work:
            imwrite(os.path.join(work, "temp_img.png"), image)
            cls.normalize_dataset_dir(work, True, output_image_shape, openface_path=openface_path, device=device)
            result = os.path.join(work, "normalized", "temp_img.png")
            return imread(result) if os.path.exists(result) else None

    @classmethod
    def _normalize_directory(cls, input_dir, output_dir, normalize_2D, output_image_shape, device=None):
        """Warps every picture of input_dir that has a confident face in input_dir/processed into output_dir (as PNG), and its
        UV map, if there is one, by the same transform.  normalize_2D: the pre-normalisation instead of the head-centre step."""
        os.makedirs(output_dir, exist_ok=True)
        processed = os.path.join(input_dir, "processed")
        pictures = [p for pattern in cls.image_filename_patterns for p in glob.glob(os.path.join(input_dir, pattern))]
        jobs = []                                   # (picture path, name without extension, M)
        for picture in pictures:
            name = os.path.splitext(os.path.basename(picture))[0]
            csv_path = os.path.join(processed, name + ".csv")
            if not os.path.exists(csv_path):        # no landmark file, or no confident face below: skipped without a word
                continue
            points_2d, points_3d, pose = dataset_utils.read_landmarks_and_pose_from_csv(csv_path)
            if points_2d is None:
                continue
            if normalize_2D:
                M = cls._get_normalizing_transform_2d(points_2d, output_image_shape)
            else:
                K = dataset_utils.read_estimated_intrinsics(os.path.join(processed, name + "_of_details.txt"))
                M = cls._get_normalizing_transform_3d(points_2d, points_3d, pose, K, output_image_shape)
            jobs.append((picture, name, M))

        dsize = tuple(output_image_shape[:2])       # (warpAffine reads it as (width, height): the reference passes it so)
        for begin in range(0, len(jobs), CHUNK):
            chunk = jobs[begin:begin + CHUNK]
            Ms = [j[2] for j in chunk]
            images = thread_map(imread, [j[0] for j in chunk])
            warped = _warp_grouped(images, Ms, dsize, warp_affine, device)
            thread_map(lambda a: imwrite(*a), [(os.path.join(output_dir, j[1] + ".png"), w) for j, w in zip(chunk, warped)])

            # the UV map of img<rest>.png is uv<rest>.exr; nearest neighbour, since values interpolated across a UV seam mean nothing
            uv_names = ["uv" + j[1][3:] + ".exr" for j in chunk]
            with_uv = [i for i, name in enumerate(uv_names) if os.path.exists(os.path.join(input_dir, name))]
            if with_uv:
                uv_images = thread_map(exr.imread, [os.path.join(input_dir, uv_names[i]) for i in with_uv])
                uv_warped = _warp_grouped(uv_images, [Ms[i] for i in with_uv], dsize, warp_affine_nearest, device)
                thread_map(lambda a: exr.imwrite(*a), [(os.path.join(output_dir, uv_names[i]), w) for i, w in zip(with_uv, uv_warped)])

    @classmethod
    def _get_normalizing_transform_3d(cls, landmarks_2d, landmarks_3d, pose, intrinsics, output_image_shape):
        """M (2, 3), picture -> output: scale from the head turned frontal, rotation from the eye line as seen, translation that
        puts the projected head centre at ref_head_center_coords.  pose = (tx, ty, tz, rx, ry, rz) of OpenFace."""
        height, width = output_image_shape[0], output_image_shape[1]
        left, right = cls.eye_corner_idxs
        # undo the head rotation about the head's own position: rows are points, so p R applies the inverse of R
        position = pose[:3]
        frontal = (landmarks_3d - position) @ euler_matrix_rxyz(pose[3], pose[4], pose[5]) + position
        px = _project(frontal, intrinsics)
        eye_span = np.linalg.norm(px[left] - px[right])
        eyes_to_mouth = np.linalg.norm(px[cls.mouth_top_idx] - (px[left] + px[right]) / 2)
        scale = (cls.interocular_fraction * width / eye_span + cls.eye_to_mouth_fraction * height / eyes_to_mouth) / 2
        # the in-plane angle comes from the picture as it is, not from the frontal head
        dx, dy = landmarks_2d[right] - landmarks_2d[left]
        angle = np.arctan2(dy, dx)
        A = scale * np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
        centre_3d = landmarks_3d[list(cls.head_center_idxs)].mean(axis=0)
        centre_px = _project(centre_3d[None, :], intrinsics)[0]
        target = (np.array(cls.ref_head_center_coords) * np.array(output_image_shape[:2])).reshape(2)
        return np.column_stack([A, target - A @ centre_px])

    @classmethod
    def _get_normalizing_transform_2d(cls, landmarks, output_image_shape):
        """M (2, 3): the least-squares similarity that takes the five landmark groups to their reference positions"""
        groups = np.stack([landmarks[list(idxs)].mean(axis=0) for idxs in cls.ref_pre_norm_landmark_idxs])
        targets = cls.ref_pre_norm_landmark_positions * np.asarray(output_image_shape[:2])
        A, t = dataset_utils.get_similarity_transform(targets, groups)
        return np.column_stack([A, t])

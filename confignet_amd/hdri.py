"""PCA model of 360-degree HDR environment maps (reference: hdri_encoding/hdri_pca_model.py): the 50-d `hdri_embedding` face-model
input of the datasets and the turntable embeddings of the demo's light sweep.

An image goes log2(x + 1) -> rotation about the vertical axis (a column roll) -> area resize to the model's shape -> PCA with
whitening.  The image side runs on the GPU in two kernels (csrc/hdri.hip): the vertical half of the resize does not depend on the
rotation, so it runs once per POOL image (cn_hdri_rows_v) and every (image, rotation) sample then reads only the vertically
reduced image (cn_hdri_rows_h); the projections go through ops.gemm.  The decomposition itself (fit) runs on the host in float64:
the matrix is (samples x oh ow 3) with samples in the hundreds, and scikit-learn -- which the reference calls -- does the same.

Neither cv2 nor scikit-learn is needed: Radiance .hdr files are read and written here, and HDRIModelPCA.load reads the reference's
pickles (a scikit-learn PCA inside an HDRIModelPCA) through a restricted unpickler."""
import glob
import io
import json
import os
import pickle

import numpy as np

FORMAT_TAG = "confignet_amd.hdri/1"
MAX_CHUNK_ROWS = 4096          # samples per cn_hdri_rows_h + projection launch


# ---------------------------------------------------------------------------------------------------------------------------------
# Radiance RGBE files
# ---------------------------------------------------------------------------------------------------------------------------------
def _decode_rgbe(rgbe):
    """(..., 4) uint8 -> (..., 3) float32 in B, G, R order: mantissa * 2^(e - 136), 0 where e == 0 (no +0.5 on the mantissa)."""
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return (rgbe[..., 2::-1].astype(np.float64) * scale[..., None]).astype(np.float32)


def read_hdr(path):
    """A Radiance picture as float32 (H, W, 3) in BGR order -- what cv2.imread(path, -1) returns.  Takes the standard top-down
    orientation (-Y h +X w) with new-style run-length encoded or flat scanlines; anything else raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"\n\n")
    if not data.startswith(b"#?") or end < 0:
        raise ValueError("%s: not a Radiance picture (no '#?' signature / no blank line after the header)" % path)
    header = data[:end].decode("latin-1").split("\n")
    fmt = [l.split("=", 1)[1].strip() for l in header if l.startswith("FORMAT=")]
    if fmt and fmt[0] != "32-bit_rle_rgbe":
        raise ValueError("%s: FORMAT=%s is not supported (32-bit_rle_rgbe only)" % (path, fmt[0]))
    eol = data.find(b"\n", end + 2)
    if eol < 0:
        raise ValueError("%s: no resolution line" % path)
    res = data[end + 2:eol].decode("latin-1").split()
    if len(res) != 4 or res[0] != "-Y" or res[2] != "+X" or not (res[1].isdigit() and res[3].isdigit()):
        raise ValueError("%s: resolution line %r is not '-Y h +X w'" % (path, " ".join(res)))
    h, w = int(res[1]), int(res[3])
    if h <= 0 or w <= 0:
        raise ValueError("%s: empty picture" % path)
    buf = np.frombuffer(data, np.uint8, offset=eol + 1)
    out = np.empty((h, w, 4), np.uint8)
    pos = 0
    for y in range(h):
        if pos + 4 > len(buf):
            raise ValueError("%s: truncated at scanline %d" % (path, y))
        if 8 <= w <= 32767 and buf[pos] == 2 and buf[pos + 1] == 2 and not buf[pos + 2] & 0x80:
            if (int(buf[pos + 2]) << 8 | int(buf[pos + 3])) != w:
                raise ValueError("%s: scanline %d is encoded for another width" % (path, y))
            pos += 4
            for plane in range(4):
                x = 0
                while x < w:
                    if pos >= len(buf):
                        raise ValueError("%s: truncated at scanline %d" % (path, y))
                    count = int(buf[pos])
                    pos += 1
                    if count > 128:                      # a run: one value, count - 128 times
                        count -= 128
                        if x + count > w or pos >= len(buf):
                            raise ValueError("%s: bad run in scanline %d" % (path, y))
                        out[y, x:x + count, plane] = buf[pos]
                        pos += 1
                    else:                                # count literal values
                        if count == 0 or x + count > w or pos + count > len(buf):
                            raise ValueError("%s: bad literal block in scanline %d" % (path, y))
                        out[y, x:x + count, plane] = buf[pos:pos + count]
                        pos += count
                    x += count
        else:
            if pos + 4 * w > len(buf):
                raise ValueError("%s: truncated at scanline %d" % (path, y))
            out[y] = buf[pos:pos + 4 * w].reshape(w, 4)
            pos += 4 * w
    return _decode_rgbe(out)


def write_hdr(path, img):
    """Writes a BGR float image (H, W, 3) as a Radiance picture with flat (not run-length encoded) RGBE pixels: per pixel the
    shared exponent of the largest channel, mantissas truncated.  Values that came out of an RGBE file re-encode exactly."""
    img = np.asarray(img, np.float64)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_hdr: (H, W, 3) image expected, got %s" % (img.shape,))
    rgb = np.maximum(img[..., ::-1], 0.0)
    top = rgb.max(axis=-1)
    frac, exp = np.frexp(top)                                # top = frac * 2^exp, frac in [0.5, 1)
    ok = (top >= 1e-32) & (exp + 128 <= 255)
    scale = np.where(ok, np.ldexp(1.0, 8 - np.where(ok, exp, 0)), 0.0)     # mantissa = value * 256 / 2^exp
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    out[..., :3] = np.minimum(np.floor(rgb * scale[..., None]), 255.0).astype(np.uint8)
    out[..., 3] = np.where(ok, exp + 128, 0).astype(np.uint8)
    out[~ok] = 0
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (img.shape[0], img.shape[1]))
        f.write(out.tobytes())


def load_hdris(hdri_dir):
    """Every *.hdr of a directory, stacked (N, H, W, 3), and their paths, in SORTED order.  The reference takes glob order (whatever
    the file system returns); sorted order is what reproduces its test fixture, and it makes seeded fits repeatable."""
    paths = sorted(glob.glob(os.path.join(hdri_dir, "*.hdr")))
    return np.array([read_hdr(p) for p in paths]), paths


# ---------------------------------------------------------------------------------------------------------------------------------
# rotation and area resize on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def rotation_shift(rotation_deg, n_cols):
    """Columns an image of n_cols columns is rolled by for a rotation in degrees (Python's round: half to even)."""
    return int(round(rotation_deg * n_cols / 360))


def rotate_hdri(hdri_image, rotation_deg):
    return np.roll(hdri_image, rotation_shift(rotation_deg, hdri_image.shape[1]), axis=1)


def apply_random_rotations(hdri_images, rotations_per_image):
    """rotations_per_image rolled copies of every image, image-major; one np.random.uniform(0, 360) per copy, in that order (the
    reference's random stream: a seeded run draws the same rotations)."""
    out = np.zeros((len(hdri_images) * rotations_per_image,) + tuple(hdri_images.shape[1:]), hdri_images.dtype)
    for k in range(len(out)):
        out[k] = rotate_hdri(hdri_images[k // rotations_per_image], np.random.uniform(0, 360))
    return out


def area_table(n_in, n_out):
    """Area (box) resampling n_in -> n_out cells along one axis, as cv2.resize INTER_AREA shrinks: output o averages the source
    interval [o s, (o + 1) s), s = n_in / n_out.  Returns (first (n_out) int32, weights (n_out, T) float32), T = ceil(s) + 1:
    weights[o][t] = overlap of source cell first[o] + t with the interval / s, computed in float64; cells past the interval
    (and past the image) have weight 0.  Enlarging is refused: INTER_AREA interpolates then."""
    n_in, n_out = int(n_in), int(n_out)
    if n_out <= 0 or n_in <= 0 or n_out > n_in:
        raise ValueError("area resize %d -> %d: only shrinking (or equal size) is supported" % (n_in, n_out))
    t_len = -(-n_in // n_out) + 1
    # in units of 1 / n_out of a source cell every bound is an integer: interval [o n_in, (o + 1) n_in), cell c = [c n_out, (c + 1) n_out)
    lo = np.arange(n_out, dtype=np.int64) * n_in
    first = lo // n_out
    cell = first[:, None] + np.arange(t_len)[None, :]
    overlap = np.minimum((lo + n_in)[:, None], (cell + 1) * n_out) - np.maximum(lo[:, None], cell * n_out)
    w = np.maximum(overlap, 0).astype(np.float64) / float(n_in)               # overlap / scale, one float64 rounding
    return first.astype(np.int32), w.astype(np.float32)


def _area_matrix(n_in, n_out):
    """The table of area_table as a dense (n_out, n_in) float64 matrix."""
    first, w = area_table(n_in, n_out)
    a = np.zeros((n_out, n_in))
    for t in range(w.shape[1]):
        cell = first + t
        ok = cell < n_in
        a[np.arange(n_out)[ok], cell[ok]] += w[ok, t]
    return a


def resize_hdris(hdri_images, output_shape):
    """Area resize of (N, H, W, 3) images to output_shape = (height, width) on the host (the --write_hdris outputs; the model's
    own rows come from the kernels)."""
    hdri_images = np.asarray(hdri_images)
    v = np.einsum("oy,nyxc->noxc", _area_matrix(hdri_images.shape[1], output_shape[0]), hdri_images.astype(np.float64))
    return np.einsum("px,noxc->nopc", _area_matrix(hdri_images.shape[2], output_shape[1]), v).astype(hdri_images.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# the decomposition
# ---------------------------------------------------------------------------------------------------------------------------------
class PCAResult:
    """What scikit-learn's PCA(svd_solver="full") keeps after fit, as float32 arrays."""
    FIELDS = ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "noise_variance_",
              "n_components_", "n_samples_", "n_features_")


def pca_from_rows(rows, n_components):
    """Full-SVD PCA of rows (n_samples, n_features) in float64, the way scikit-learn does it: centre, LAPACK SVD, flip every
    component so that the largest-magnitude entry of its column of U is positive, explained_variance = S^2 / (n - 1).
    n_components > 1: that many (int); in (0, 1): the fewest whose cumulative variance ratio exceeds it; more than
    min(n_samples, n_features) raises ValueError.  noise_variance_ = mean of the discarded variances (0 if none)."""
    x = np.asarray(rows, np.float64)
    n_samples, n_features = x.shape
    limit = min(n_samples, n_features)
    n_components = int(n_components) if n_components > 1 else n_components
    if not 0 < n_components <= limit:
        raise ValueError("n_components=%r must be in (0, 1) or an integer in [1, min(n_samples, n_features) = %d]" % (n_components, limit))
    mean = x.mean(axis=0)
    u, s, vt = np.linalg.svd(x - mean, full_matrices=False)
    signs = np.sign(u[np.abs(u).argmax(axis=0), np.arange(u.shape[1])])
    signs[signs == 0] = 1.0
    vt = vt * signs[:, None]
    var = s ** 2 / (n_samples - 1)
    ratio = var / var.sum()
    if n_components < 1:
        k = int(np.searchsorted(np.cumsum(ratio), n_components)) + 1
    else:
        k = int(n_components)
    res = PCAResult()
    res.mean_ = mean.astype(np.float32)
    res.components_ = vt[:k].astype(np.float32)
    res.explained_variance_ = var[:k].astype(np.float32)
    res.explained_variance_ratio_ = ratio[:k].astype(np.float32)
    res.singular_values_ = s[:k].astype(np.float32)
    res.noise_variance_ = np.float32(var[k:].mean() if k < limit else 0.0)
    res.n_components_, res.n_samples_, res.n_features_ = k, n_samples, n_features
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# reading the reference's pickles without scikit-learn
# ---------------------------------------------------------------------------------------------------------------------------------
class _Holder:
    """Plain attribute holder the restricted unpickler builds in place of the reference's classes."""


class _RestrictedUnpickler(pickle.Unpickler):
    _NUMPY = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
              ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar")}

    def find_class(self, module, name):
        if name == "HDRIModelPCA" and module in ("hdri_pca_model", "__main__"):
            return _Holder
        if name == "PCA" and (module == "sklearn.decomposition" or module.startswith("sklearn.decomposition.")):
            return _Holder
        if (module, name) in self._NUMPY:
            import importlib
            try:
                return getattr(importlib.import_module(module), name)
            except ImportError:                          # numpy.core <-> numpy._core across numpy versions
                other = module.replace("numpy.core", "numpy._core") if "numpy.core" in module else module.replace("numpy._core", "numpy.core")
                return getattr(importlib.import_module(other), name)
        raise pickle.UnpicklingError("HDRI model files may not reference %s.%s" % (module, name))


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
class HDRIModelPCA:
    def __init__(self, output_shape, n_rotations_per_image):
        self.n_rotations_per_image = int(n_rotations_per_image)
        self.output_shape = tuple(int(v) for v in output_shape)
        self.pca_model = None
        self._dev = None               # device copies of the projection matrices, made on first use

    # ---- device side -------------------------------------------------------------------------------------------------------
    @staticmethod
    def _device():
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("HDRIModelPCA: the image path runs on the GPU (cn_hdri_rows_v / cn_hdri_rows_h); there is no CPU fallback")
        return torch.device("cuda")

    def _tables(self, h, w):
        import torch
        dev = self._device()
        y0, wy = area_table(h, self.output_shape[0])
        x0, wx = area_table(w, self.output_shape[1])
        return [torch.as_tensor(a, device=dev) for a in (y0, wy, x0, wx)]

    def _check_pool(self, pool_images, image_idx, rotations):
        pool_images = np.asarray(pool_images, np.float32)
        if pool_images.ndim != 4 or pool_images.shape[3] != 3:
            raise ValueError("HDRI images must be (N, H, W, 3), got %s" % (pool_images.shape,))
        image_idx = np.asarray(image_idx, np.int64).reshape(-1)
        if rotations is None:
            rotations = np.zeros(len(image_idx))
        if len(rotations) != len(image_idx):
            raise ValueError("%d rotations for %d samples" % (len(rotations), len(image_idx)))
        if len(image_idx) and (image_idx.min() < 0 or image_idx.max() >= len(pool_images)):
            raise ValueError("image index out of range for a pool of %d images" % len(pool_images))
        w = pool_images.shape[2]
        # the shift is computed here, as rotate_hdri computes it, and reduced modulo the width: the kernel gets plain integers
        shifts = np.array([rotation_shift(float(r), w) % w for r in rotations], np.int32)
        return pool_images, image_idx.astype(np.int32), shifts

    def _device_rows(self, pool_images, image_idx, rotations, centred):
        """The one image path: uploads the pool, reduces it vertically once (cn_hdri_rows_v) and yields the samples' rows
        (chunk, oh * ow * 3) on the device, at most MAX_CHUNK_ROWS at a time (cn_hdri_rows_h), minus the model's mean when
        `centred`.  fit, transform and transform_indexed all draw their rows from here."""
        import torch
        from . import ops
        pool_images, image_idx, shifts = self._check_pool(pool_images, image_idx, rotations)
        if len(image_idx) == 0:
            return
        dev = self._device()
        mean = self._projection()["mean"] if centred else None
        y0, wy, x0, wx = self._tables(pool_images.shape[1], pool_images.shape[2])
        v = ops.hdri_rows_v(torch.as_tensor(pool_images, device=dev), y0, wy, self.output_shape[0])
        for s in range(0, len(image_idx), MAX_CHUNK_ROWS):
            idx = torch.as_tensor(image_idx[s:s + MAX_CHUNK_ROWS], device=dev)
            sh = torch.as_tensor(shifts[s:s + MAX_CHUNK_ROWS], device=dev)
            yield ops.hdri_rows_h(v, idx, sh, x0, wx, self.output_shape[1], mean).reshape(idx.numel(), -1)

    def rows_indexed(self, pool_images, image_idx, rotations=None, centred=False):
        """What the decomposition is fitted on (centred=False) and what transform projects (centred=True): rows
        (n, oh * ow * 3) float32 of samples (pool image image_idx[i], rotated rotations[i] degrees)."""
        chunks = [r.cpu().numpy() for r in self._device_rows(pool_images, image_idx, rotations, centred)]
        return np.concatenate(chunks) if chunks else np.zeros((0, self.output_shape[0] * self.output_shape[1] * 3), np.float32)

    def _projection(self):
        import torch
        if self.pca_model is None:
            raise RuntimeError("HDRIModelPCA: fit or load a model first")
        if self._dev is None:
            dev = self._device()
            p = self.pca_model
            sd = np.sqrt(np.asarray(p.explained_variance_, np.float64))
            comp = np.asarray(p.components_, np.float64)
            self._dev = {"mean": torch.as_tensor(np.asarray(p.mean_, np.float32), device=dev),
                         "whiten": torch.as_tensor((comp / sd[:, None]).astype(np.float32), device=dev),          # (k, F)
                         "colour": torch.as_tensor((comp * sd[:, None]).astype(np.float32), device=dev)}          # (k, F)
        return self._dev

    # ---- the reference's interface -----------------------------------------------------------------------------------------
    def fit(self, hdri_images, n_components=0.9):
        """n_components as in scikit-learn's PCA: a count, or in (0, 1) the fraction of variance to explain."""
        hdri_images = np.asarray(hdri_images, np.float32)
        n, per = len(hdri_images), self.n_rotations_per_image
        rotations = [np.random.uniform(0, 360) for _ in range(n * per)]        # image-major, as apply_random_rotations draws
        rows = self.rows_indexed(hdri_images, np.repeat(np.arange(n), per), rotations)
        self.pca_model = pca_from_rows(rows, n_components)
        self._dev = None
        kept = self.pca_model
        print("HDRI model: %d components hold %.2f %% of the variance of %d rotated pictures"
              % (kept.n_components_, 100 * float(np.sum(kept.explained_variance_ratio_)), kept.n_samples_))

    def transform_indexed(self, pool_images, image_idx, rotations=None):
        """Embeddings (n, k) float32 of samples (pool image image_idx[i] rotated by rotations[i] degrees).  The pool is uploaded
        once and reduced vertically once per image, whatever the number of samples that draw on it."""
        from . import ops
        proj = self._projection()
        out = [ops.gemm(rows, proj["whiten"], trans_b=True).cpu().numpy() for rows in self._device_rows(pool_images, image_idx, rotations, True)]
        return np.concatenate(out) if out else np.zeros((0, proj["whiten"].shape[0]), np.float32)

    def transform(self, hdri_images, rotations=None):
        return self.transform_indexed(hdri_images, np.arange(len(hdri_images)), rotations)

    def inverse_transform(self, X, log=False):
        """Embeddings (n, k) -> radiance images (n, oh, ow, 3) float32: X sqrt(ev) components + mean, then 2^y - 1.  log=True
        stops before the last step and returns y = log2(radiance + 1)."""
        import torch
        from . import ops
        proj = self._projection()
        X = np.asarray(X, np.float32).reshape(-1, proj["colour"].shape[0])
        out = []
        for s in range(0, len(X), MAX_CHUNK_ROWS):
            y = ops.gemm(torch.as_tensor(X[s:s + MAX_CHUNK_ROWS], device=proj["mean"].device), proj["colour"], bias=proj["mean"])
            out.append((y if log else ops.exp2m1(y)).cpu().numpy())
        images = np.concatenate(out) if out else np.zeros((0, proj["colour"].shape[1]), np.float32)
        return images.reshape((len(images),) + self.output_shape + (3,))

    def write_basis_images(self, output_dir):
        """Every component as an 8-bit picture, stretched to its own [min, max]."""
        from .confignet_utils import write_image
        os.makedirs(output_dir, exist_ok=True)
        for i, basis in enumerate(np.asarray(self.pca_model.components_)):
            img = basis.reshape(self.output_shape + (3,))
            img = 255 * (img - img.min()) / (img.max() - img.min())
            write_image(os.path.join(output_dir, str(i).zfill(3) + ".png"), img.astype(np.uint8))

    # ---- files -------------------------------------------------------------------------------------------------------------
    def save(self, output_path):
        """Our own file: a pickled plain dict of arrays and settings (FORMAT_TAG).  The reference cannot load it -- its loader
        unpickles its own classes around a scikit-learn object, which this project does not create."""
        state = {"format": FORMAT_TAG, "output_shape": tuple(self.output_shape), "n_rotations_per_image": self.n_rotations_per_image}
        for name in PCAResult.FIELDS:
            state[name] = getattr(self.pca_model, name)
        with open(output_path, "wb") as f:
            pickle.dump(state, f, protocol=4)          # (protocol 5 stores arrays through helpers load() does not admit)

    @staticmethod
    def load(input_path):
        """Reads a file written by save() or by the reference (hdri_pca_model.HDRIModelPCA around a scikit-learn PCA); scikit-learn
        is not imported, and a file may only reference those two classes and numpy's array reconstruction helpers."""
        with open(input_path, "rb") as f:
            obj = _RestrictedUnpickler(io.BytesIO(f.read())).load()
        pca = PCAResult()
        if isinstance(obj, dict):
            if obj.get("format") != FORMAT_TAG:
                raise ValueError("%s: unknown HDRI model format %r" % (input_path, obj.get("format")))
            model = HDRIModelPCA(obj["output_shape"], obj["n_rotations_per_image"])
            src = obj.get
        elif isinstance(obj, _Holder) and isinstance(getattr(obj, "pca_model", None), _Holder):
            model = HDRIModelPCA(obj.output_shape, obj.n_rotations_per_image)
            if not getattr(obj.pca_model, "whiten", True):
                raise ValueError("%s: a PCA without whitening is not an HDRI model" % input_path)
            src = lambda name: getattr(obj.pca_model, name, None)      # noqa: E731
        else:
            raise ValueError("%s: not an HDRI model file" % input_path)
        for name in PCAResult.FIELDS:
            setattr(pca, name, src(name))
        if pca.mean_ is None or pca.components_ is None or pca.explained_variance_ is None:
            raise ValueError("%s: the model holds no fitted PCA" % input_path)
        model.pca_model = pca
        return model


# ---------------------------------------------------------------------------------------------------------------------------------
# what the three command-line tools under hdri_encoding/ do (they only parse flags)
# ---------------------------------------------------------------------------------------------------------------------------------
def get_hdri_embeddings(hdri_model, hdris, hdri_names, metadata_dicts):
    """Embedding (n, k) of every render's environment map: image by illumination.HDRI_filename, rotation (degrees) =
    180 * illumination.HDRI_rotation[2] / pi -- all samples in ONE transform_indexed call over the pool of images."""
    position = {name: i for i, name in enumerate(hdri_names)}
    lights = [d["illumination"] for d in metadata_dicts]
    return hdri_model.transform_indexed(hdris, [position[l["HDRI_filename"]] for l in lights],
                                        [180 * l["HDRI_rotation"][2] / np.pi for l in lights])


def build_model(hdri_dir, output_dir, n_components, output_shape, n_rotations_per_image, seed, write_hdris=False):
    """Fits a model on the pictures of hdri_dir under np.random.seed(seed) and leaves in output_dir: hdri_model.pck, pca_basis/
    (one picture per component) and, with write_hdris, hdris/NNN_reconstructed.hdr (picture -> embedding -> picture) next to
    hdris/NNN_original.hdr (the picture at the model's shape)."""
    pictures, paths = load_hdris(hdri_dir)
    if len(paths) == 0:
        raise ValueError("no .hdr files in %s" % hdri_dir)
    print("read %d pictures of %d x %d from %s" % (len(paths), pictures.shape[1], pictures.shape[2], hdri_dir))
    np.random.seed(seed)
    model = HDRIModelPCA(tuple(output_shape), n_rotations_per_image)
    model.fit(pictures, n_components)
    os.makedirs(output_dir, exist_ok=True)
    model.save(os.path.join(output_dir, "hdri_model.pck"))
    model.write_basis_images(os.path.join(output_dir, "pca_basis"))
    if write_hdris:
        os.makedirs(os.path.join(output_dir, "hdris"), exist_ok=True)
        for kind, stack in (("reconstructed", model.inverse_transform(model.transform(pictures))),
                            ("original", resize_hdris(pictures, model.output_shape))):
            for i, picture in enumerate(stack):
                write_hdr(os.path.join(output_dir, "hdris", "%03d_%s.hdr" % (i, kind)), picture)
    return model


def write_turntable(hdri_file_path, hdri_model_path, output_file_path, n_rotations, hdri_output_dir=None):
    """One picture seen under n_rotations rotations from -180 to 180 degrees (both ends included): the (n_rotations, k) float32
    embeddings go to output_file_path as .npy -- what the demo's light sweep plays back.  The picture is uploaded and reduced
    vertically once.  With hdri_output_dir the embeddings are decoded again and written there as NNNN.hdr."""
    model = HDRIModelPCA.load(hdri_model_path)
    angles = np.linspace(-180, 180, n_rotations)
    embeddings = model.transform_indexed(read_hdr(hdri_file_path)[None], np.zeros(n_rotations, np.int64), angles)
    np.save(output_file_path, embeddings)
    if hdri_output_dir is not None:
        os.makedirs(hdri_output_dir, exist_ok=True)
        for i, picture in enumerate(model.inverse_transform(embeddings)):
            write_hdr(os.path.join(hdri_output_dir, "%04d.hdr" % i), picture)
    return embeddings


def embed_render_metadata(input_dir, render_asset_dir, model_path, hdri_output_dir=None):
    """Adds "hdri_embedding" (a list of k numbers) to every *.json of input_dir, in place.  A file names its environment map
    (a picture of <render_asset_dir>/HDRI) and its rotation; all files are embedded in one call over that pool.  With
    hdri_output_dir, each render's rotated map and what the model makes of it are written there as .hdr pictures."""
    model = HDRIModelPCA.load(model_path)
    files = sorted(glob.glob(os.path.join(input_dir, "*.json")))
    records = []
    for path in files:
        with open(path) as f:
            records.append(json.load(f))
    pool, pool_paths = load_hdris(os.path.join(render_asset_dir, "HDRI"))
    names = [os.path.basename(p) for p in pool_paths]
    embeddings = get_hdri_embeddings(model, pool, names, records)
    if hdri_output_dir is not None:
        os.makedirs(hdri_output_dir, exist_ok=True)
        for i, (record, decoded) in enumerate(zip(records, model.inverse_transform(embeddings))):
            light = record["illumination"]
            seen = rotate_hdri(pool[names.index(light["HDRI_filename"])], 180 * light["HDRI_rotation"][2] / np.pi)
            write_hdr(os.path.join(hdri_output_dir, "%04d_original.hdr" % i), seen)
            write_hdr(os.path.join(hdri_output_dir, "%04d_reconstructed.hdr" % i), decoded)
    for path, record, embedding in zip(files, records, embeddings):
        record["hdri_embedding"] = [float(v) for v in embedding]
        with open(path, "w") as f:
            json.dump(record, f, indent=4)
    return embeddings

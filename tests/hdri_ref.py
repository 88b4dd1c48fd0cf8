"""Float64 NumPy restatement of the HDRI environment-map encoding (reference: hdri_encoding/hdri_pca_model.py), written from its
behaviour as loops and einsums.  Imports nothing from the product: the tests compare confignet_amd.hdri and the HIP kernels
against this file.

    image (H, W, 3) radiance -> log2(x + 1) -> np.roll along the columns -> area resize to (oh, ow) -> row of oh * ow * 3 values
    PCA with whitening over such rows (full SVD, scikit-learn's sign convention)."""
import math
from fractions import Fraction

import numpy as np


def area_weights(n_in, n_out):
    """Exact area-resampling table n_in -> n_out: output cell o covers the source interval [o s, (o + 1) s), s = n_in / n_out.
    Returns (first (n_out) ints, weights (n_out, T) float64), T = ceil(s) + 1, weights[o][t] = |cell first[o] + t  n  interval| / s
    evaluated in rational arithmetic and rounded once to float64."""
    if not 0 < n_out <= n_in:
        raise ValueError("area resize only shrinks")
    s = Fraction(n_in, n_out)
    t_len = math.ceil(s) + 1
    first = np.zeros(n_out, np.int64)
    w = np.zeros((n_out, t_len), np.float64)
    for o in range(n_out):
        lo, hi = o * s, (o + 1) * s
        first[o] = math.floor(lo)
        for t in range(t_len):
            cell = int(first[o]) + t
            overlap = min(hi, Fraction(cell + 1)) - max(lo, Fraction(cell))
            if cell < n_in and overlap > 0:
                w[o, t] = float(overlap / s)
    return first, w


def area_matrix(n_in, n_out):
    """The same table as a dense (n_out, n_in) matrix."""
    first, w = area_weights(n_in, n_out)
    a = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        for t in range(w.shape[1]):
            if w[o, t] != 0.0:
                a[o, first[o] + t] = w[o, t]
    return a


def shift_of(rotation_deg, n_cols):
    return int(round(rotation_deg * n_cols / 360))


def log_image(image):
    return np.log2(np.asarray(image, np.float64) + 1.0)


def rows(pool, idx, shifts, out_shape, mean=None):
    """(n, oh, ow, 3) float64: sample i = pool[idx[i]] -> log2(x + 1) -> rolled by shifts[i] columns -> area resize."""
    pool = np.asarray(pool)
    ay = area_matrix(pool.shape[1], out_shape[0])
    ax = area_matrix(pool.shape[2], out_shape[1])
    out = np.zeros((len(idx), out_shape[0], out_shape[1], 3), np.float64)
    for i, (p, s) in enumerate(zip(idx, shifts)):
        rolled = np.roll(log_image(pool[p]), int(s), axis=1)
        out[i] = np.einsum("px,oxc->opc", ax, np.einsum("oy,yxc->oxc", ay, rolled))
    if mean is not None:
        out -= np.asarray(mean, np.float64).reshape(out.shape[1:])
    return out


def seeded_fit_rows(images, out_shape, rotations_per_image, seed):
    """The rows the reference's fit builds under np.random.seed(seed): rotations_per_image draws of uniform(0, 360) per image,
    image-major.  Returns (n, oh * ow * 3) float64."""
    np.random.seed(seed)
    idx, shifts = [], []
    for p in range(len(images)):
        for _ in range(rotations_per_image):
            idx.append(p)
            shifts.append(shift_of(np.random.uniform(0, 360), images.shape[2]))
    return rows(images, idx, shifts, out_shape).reshape(len(idx), -1)


def pca(x, k):
    """Full-SVD PCA keeping k components: (mean, components (k, F), explained_variance (k), ratio (all), noise_variance).
    Sign: the entry of largest magnitude in each column of U is made positive (scikit-learn's svd_flip, u-based)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0)
    u, s, vt = np.linalg.svd(x - mean, full_matrices=False)
    for j in range(len(s)):
        if u[np.argmax(np.abs(u[:, j])), j] < 0:
            vt[j] = -vt[j]
    var = s * s / (n - 1)
    noise = float(np.mean(var[k:])) if k < min(x.shape) else 0.0
    return mean, vt[:k], var[:k], var / var.sum(), noise


def transform(centred_rows, components, explained_variance):
    """Whitened coordinates of rows that already have the mean subtracted."""
    return np.einsum("nf,kf->nk", np.asarray(centred_rows, np.float64), np.asarray(components, np.float64)) \
        / np.sqrt(np.asarray(explained_variance, np.float64))[None, :]


def inverse_log(x, mean, components, explained_variance):
    """Embeddings -> log2(radiance + 1) rows."""
    scaled = np.asarray(x, np.float64) * np.sqrt(np.asarray(explained_variance, np.float64))[None, :]
    return np.einsum("nk,kf->nf", scaled, np.asarray(components, np.float64)) + np.asarray(mean, np.float64)[None, :]


def inverse(x, mean, components, explained_variance):
    return np.exp2(inverse_log(x, mean, components, explained_variance)) - 1.0

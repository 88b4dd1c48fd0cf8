"""Host side of the HDRI environment-map encoding (confignet_amd/hdri.py), no GPU: the Radiance reader / writer, the rotation rule,
the area tables, and the decomposition -- pinned on what the reference itself once computed.

tests/golden/reference_assets/hdri_encoding/ holds the reference's own test assets: three 64 x 128 Radiance pictures and
hdri_model.pck, the model its hdri_pca_model.py (--output_shape 10 20 --n_components 5, seed 0, 5 rotations per image) fitted on
them through cv2 and scikit-learn 0.20 in float32.  The float64 restatement tests/hdri_ref.py + pca_from_rows reproduces that
model at float32 rounding level; measured when this test was written:
    mean_ 1.4e-7 abs (largest entry 1.18), components_ <= 4.7e-7 abs per row (signs included), explained_variance_ 5.1e-7
    relative, noise_variance_ 0.92418416 vs 0.9241842 (4e-8).
The bars below are 4 x those distances: the distances are the reference's own float32 rounding, the margin covers another LAPACK
build.  With HDRI_ERRORS naming a path the observed values are written there (profiles/hdri_errors.txt: run this file, then
tests/test_hdri_gpu.py, in one pytest call)."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the package, as every test module here: the HIP library binds to the HIP runtime torch ships)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdri_ref as R  # noqa: E402
from confignet_amd import hdri as H  # noqa: E402

ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_assets", "hdri_encoding")
BAR_MEAN, BAR_COMPONENTS, BAR_VARIANCE_REL, BAR_NOISE = 4 * 1.4e-7, 4 * 4.7e-7, 4 * 5.1e-7, 4 * 4e-8


def pin_distances(fitted, ref):
    """Distances of a fitted PCAResult from the reference's model, all in float64: (mean abs, per-component abs, variance rel, noise abs)."""
    f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
    return (float(np.abs(f64(fitted.mean_) - f64(ref.mean_)).max()),
            np.abs(f64(fitted.components_) - f64(ref.components_)).max(axis=1),
            float(np.abs(f64(fitted.explained_variance_) / f64(ref.explained_variance_) - 1).max()),
            abs(float(fitted.noise_variance_) - float(ref.noise_variance_)))


def write_pin(title, d, mode):
    path = os.environ.get("HDRI_ERRORS")
    if not path:
        return
    with open(path, mode) as f:
        if mode == "w":
            f.write("HDRI encoding: observed errors of tests/test_hdri_cpu.py and tests/test_hdri_gpu.py (written when HDRI_ERRORS names a path).\n"
                    "Pins: distance of a fit on the reference's three test pictures (seed 0, 5 rotations, 10 x 20, 5 components) from the\n"
                    "reference's own hdri_model.pck; bars mean %.2e abs, components %.2e abs, variance %.2e rel, noise %.2e abs.\n\n"
                    % (BAR_MEAN, BAR_COMPONENTS, BAR_VARIANCE_REL, BAR_NOISE))
        f.write("%s\n    mean_ %.3e abs   components_ %s abs   explained_variance_ %.3e rel   noise_variance_ %.3e abs\n"
                % (title, d[0], " ".join("%.3e" % v for v in d[1]), d[2], d[3]))


@pytest.fixture(scope="module")
def images():
    imgs, paths = H.load_hdris(ASSETS)
    assert [os.path.basename(p) for p in paths] == ["000.hdr", "001.hdr", "002.hdr"]
    imgs.setflags(write=False)
    return imgs


@pytest.fixture(scope="module")
def fit_rows(images):
    rows = R.seeded_fit_rows(images, (10, 20), 5, 0)
    rows.setflags(write=False)
    return rows


@pytest.fixture(scope="module")
def reference_model():
    return H.HDRIModelPCA.load(os.path.join(ASSETS, "hdri_model.pck"))


def test_read_hdr_on_the_reference_pictures_and_exact_round_trip(images, tmp_path):
    assert images.shape == (3, 64, 128, 3) and images.dtype == np.float32
    assert images.min() == np.float32(0.008300781) and images.max() == np.float32(26.25)
    for i, img in enumerate(images):
        path = str(tmp_path / ("%d.hdr" % i))
        H.write_hdr(path, img)
        back = H.read_hdr(path)
        assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), img.view(np.uint32))


def test_read_hdr_is_bgr_and_decodes_runs(tmp_path):
    """One hand-written file: a run-length encoded scanline (a run and a literal block per plane) and the channel order."""
    w = 8
    planes = [bytes([128 + w, 128]),                      # R: a run of 8 x mantissa 128
              bytes([w]) + bytes(range(8, 16)),           # G: 8 literals
              bytes([128 + 3, 64, 5]) + bytes([1, 2, 3, 4, 5]),   # B: a run of 3, then 5 literals
              bytes([128 + w, 129])]                      # E: 129 -> 2^-7
    path = str(tmp_path / "rle.hdr")
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 8\n" + bytes([2, 2, 0, w]) + b"".join(planes))
    img = H.read_hdr(path)
    assert img.shape == (1, 8, 3)
    assert np.array_equal(img[0, :, 2], np.full(8, 1.0, np.float32))                                    # R = 128 * 2^-7
    assert np.array_equal(img[0, :, 1], np.arange(8, 16, dtype=np.float32) / 128)
    assert np.array_equal(img[0, :, 0], np.array([64, 64, 64, 1, 2, 3, 4, 5], np.float32) / 128)


@pytest.mark.parametrize("content", [
    b"P6\n1 1\n255\n\0\0\0",                                                                  # not a Radiance file
    b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n+Y 1 +X 1\n\1\1\1\200",                            # bottom-up
    b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n\1\1\1\200",                            # another pixel format
    b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 1\n\1\1\1\200",                            # truncated
    b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 8\n\2\2\0\10\211\1",                       # run past the end of the scanline
])
def test_read_hdr_refuses_what_it_does_not_decode(content, tmp_path):
    path = str(tmp_path / "bad.hdr")
    with open(path, "wb") as f:
        f.write(content)
    with pytest.raises(ValueError):
        H.read_hdr(path)


def test_reference_pin_of_the_decomposition(fit_rows, reference_model):
    """hdri_ref rows of the three pictures under seed 0 -> pca_from_rows(rows, 5) against the model the reference fitted: every
    quantity inside 4 x the measured float32 distance, component signs as they come (no flip in this test)."""
    assert fit_rows.shape == (15, 600)
    fitted = H.pca_from_rows(fit_rows, 5)
    ref = reference_model.pca_model
    assert fitted.components_.shape == np.asarray(ref.components_).shape == (5, 600)
    assert all(np.asarray(getattr(fitted, n)).dtype == np.float32 for n in ("mean_", "components_", "explained_variance_", "noise_variance_"))
    d = pin_distances(fitted, ref)
    print("pin (host decomposition of float64 rows):", d)
    write_pin("host: pca_from_rows on the float64 rows of tests/hdri_ref.py", d, "w")
    assert d[0] <= BAR_MEAN
    assert (d[1] <= BAR_COMPONENTS).all()
    assert d[2] <= BAR_VARIANCE_REL
    assert d[3] <= BAR_NOISE
    assert fitted.n_components_ == 5 and fitted.n_samples_ == 15 and fitted.n_features_ == 600
    # the restatement's own decomposition agrees with the product's
    mean, comps, var, _, noise = R.pca(fit_rows, 5)
    assert np.abs(fitted.components_ - comps).max() < 1e-6 and abs(float(fitted.noise_variance_) - noise) < 1e-6


def test_fraction_of_variance_selects_six_components(fit_rows):
    ratio = R.pca(fit_rows, 15)[3]
    assert abs(np.cumsum(ratio)[4] - 0.8726) < 1e-4 and abs(np.cumsum(ratio)[5] - 0.9018) < 1e-4
    fitted = H.pca_from_rows(fit_rows, 0.9)
    assert fitted.n_components_ == 6 and fitted.components_.shape == (6, 600)


def test_more_components_than_samples_raises(fit_rows):
    with pytest.raises(ValueError):
        H.pca_from_rows(fit_rows, 16)
    assert H.pca_from_rows(fit_rows, 15).noise_variance_ == 0          # nothing discarded


def test_load_reads_the_reference_pickle_without_scikit_learn(monkeypatch):
    monkeypatch.setitem(sys.modules, "sklearn", None)                  # `import sklearn` would now raise ImportError
    model = H.HDRIModelPCA.load(os.path.join(ASSETS, "hdri_model.pck"))
    assert model.output_shape == (10, 20) and model.n_rotations_per_image == 5
    assert np.asarray(model.pca_model.components_).shape == (5, 600) and np.asarray(model.pca_model.mean_).shape == (600,)


def test_save_and_load_round_trip_and_refused_classes(fit_rows, tmp_path):
    import pickle
    model = H.HDRIModelPCA((10, 20), 5)
    model.pca_model = H.pca_from_rows(fit_rows, 5)
    path = str(tmp_path / "model.pck")
    model.save(path)
    back = H.HDRIModelPCA.load(path)
    assert back.output_shape == (10, 20) and back.n_rotations_per_image == 5
    for name in H.PCAResult.FIELDS:
        assert np.array_equal(np.asarray(getattr(back.pca_model, name)), np.asarray(getattr(model.pca_model, name))), name
    with open(path, "wb") as f:
        pickle.dump(os.path.join, f)                                   # any global outside the allowed set
    with pytest.raises(pickle.UnpicklingError):
        H.HDRIModelPCA.load(path)


@pytest.mark.parametrize("deg, shift", [(-180, -64), (-0.7, 0), (0, 0), (1.40625, 0), (4.21875, 2), (359.9, 128), (720, 256)])
def test_rotate_hdri_is_a_roll_by_the_rounded_shift(deg, shift):
    img = np.arange(2 * 128 * 3, dtype=np.float32).reshape(2, 128, 3)
    assert H.rotation_shift(deg, 128) == shift == R.shift_of(deg, 128)
    assert np.array_equal(H.rotate_hdri(img, deg), np.roll(img, shift, axis=1))


def test_apply_random_rotations_follows_the_seeded_stream():
    imgs = np.arange(2 * 4 * 16 * 3, dtype=np.float32).reshape(2, 4, 16, 3)
    np.random.seed(3)
    got = H.apply_random_rotations(imgs, 3)
    np.random.seed(3)
    want = [np.roll(imgs[i], R.shift_of(np.random.uniform(0, 360), 16), axis=1) for i in range(2) for _ in range(3)]
    assert got.shape == (6, 4, 16, 3) and np.array_equal(got, np.array(want))


@pytest.mark.parametrize("n_in, n_out", [(64, 10), (128, 20), (64, 16), (37, 7), (53, 53)])
def test_area_tables(n_in, n_out):
    first, w = H.area_table(n_in, n_out)
    first_ref, w_ref = R.area_weights(n_in, n_out)
    assert first.dtype == np.int32 and w.dtype == np.float32 and w.shape == w_ref.shape == (n_out, -(-n_in // n_out) + 1)
    assert np.array_equal(first, first_ref)
    # the float32 rounding of the exact weight: half an ulp of a value <= 1
    assert np.abs(w.astype(np.float64) - w_ref).max() <= 2.0 ** -25
    assert np.array_equal(w == 0, w_ref == 0)
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1).max() <= 2.0 ** -22
    assert (first >= 0).all() and ((first[:, None] + np.arange(w.shape[1]) < n_in) | (w == 0)).all()


def test_area_resize_refuses_to_enlarge():
    with pytest.raises(ValueError):
        H.area_table(10, 11)
    with pytest.raises(ValueError):
        H.resize_hdris(np.zeros((1, 8, 8, 3), np.float32), (4, 9))


def test_resize_hdris_against_the_restatement(images):
    got = H.resize_hdris(images, (10, 20))
    want = np.einsum("oy,px,nyxc->nopc", R.area_matrix(64, 10), R.area_matrix(128, 20), images.astype(np.float64))
    assert got.shape == (3, 10, 20, 3) and got.dtype == np.float32
    assert np.abs(got - want).max() <= 2.0 ** -23 * want.max()

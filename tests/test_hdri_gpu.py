"""HDRI environment-map encoding on the GPU: cn_hdri_rows_v / cn_hdri_rows_h / cn_exp2m1 (csrc/hdri.hip) and HDRIModelPCA
(confignet_amd/hdri.py) against the float64 restatement tests/hdri_ref.py and against the model the reference itself fitted
(tests/golden/reference_assets/hdri_encoding/hdri_model.pck; see tests/test_hdri_cpu.py for the pin and its bars).

Every bound is derived from the arithmetic, not tuned:
  rows      |got - ref| <= (Ty + Tx + 6) 2^-24 max(1, max log2(x + 1)): weights are <= 1 and sum to 1, values are non-negative, one
            rounding per term of either sum (fused multiply-add) and one per weight (the float32 table), ~1 ulp of log2f, the
            rounding of x + 1, the subtraction of the mean.
  transform |got - ref|_k <= (600 + 12) 2^-24 sum_i |x_i - mean_i| |c_ki| / sqrt(ev_k): a dot product of 600 terms in float32 in any
            order, plus the row's own error (above, relative to values it is made of) and the rounding of c / sqrt(ev).
  inverse   the same form with the dot's 5 terms, (5 + 12) 2^-24 (sum_k |X_k| sqrt(ev_k) |c_ki| + |mean_i|), before the exp2; after it
            4 2^-24 max(2^y, |2^y - 1|) (exp2f errs in proportion to 2^y, the subtraction of 1 rounds in proportion to the result)
            plus what the bound b on y becomes, 2^y (2^b - 1) (= b ln 2 2^y to first order).
The largest error / bound of each is appended to the file HDRI_ERRORS names (profiles/hdri_errors.txt)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdri_ref as R  # noqa: E402
from test_hdri_cpu import ASSETS, BAR_COMPONENTS, BAR_MEAN, BAR_NOISE, BAR_VARIANCE_REL, pin_distances, write_pin  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 64
NAN_PATTERN = 0x7FC0BEEF


def note(line):
    print(line)
    path = os.environ.get("HDRI_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def H():
    from confignet_amd import hdri
    return hdri


@pytest.fixture(scope="module")
def images(H):
    return H.load_hdris(ASSETS)[0]


@pytest.fixture(scope="module")
def reference_model(H):
    return H.HDRIModelPCA.load(os.path.join(ASSETS, "hdri_model.pck"))


@pytest.fixture(scope="module")
def reference_rows(images):
    """float64 rows (3, 600) of the three pictures at 10 x 20, unrotated -- shared by the projection tests."""
    rows = R.rows(images, [0, 1, 2], [0, 0, 0], (10, 20)).reshape(3, -1)
    rows.setflags(write=False)
    return rows


def guarded(numel):
    """A float32 device buffer of `numel` floats between two guard bands filled with a NaN bit pattern: (whole, view of the middle)."""
    whole = torch.full((numel + 2 * GUARD,), NAN_PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[GUARD:GUARD + numel]


def guards_intact(whole):
    bits = whole.view(torch.int32)
    return bool((bits[:GUARD] == NAN_PATTERN).all()) and bool((bits[-GUARD:] == NAN_PATTERN).all())


IDX = [2, 0, 0, 1, 2, 1, 0]


@pytest.mark.parametrize("h, w, oh, ow", [(64, 128, 10, 20), (64, 128, 16, 32), (64, 128, 64, 128), (37, 53, 7, 11)])
@pytest.mark.parametrize("with_mean", [False, True])
def test_kernels_against_the_float64_restatement(H, images, h, w, oh, ow, with_mean):
    from confignet_amd import _lib
    from confignet_amd.ops import _stream
    if (h, w) == (64, 128):
        pool = np.array(images)
    else:                                            # W * 3 = 159 floats per row: no row is 16-byte aligned with the next
        pool = np.exp(np.random.default_rng(5).standard_normal((3, h, w, 3))).astype(np.float32)
    shifts = [0, 1, -1, w - 1, w, -3 * w - 5, 17]
    ref = R.rows(pool, IDX, shifts, (oh, ow))
    mean = None
    if with_mean:
        mean = ref.mean(axis=0).astype(np.float32)
        ref = ref - mean.astype(np.float64)
    v_ref = np.einsum("oy,nyxc->noxc", R.area_matrix(h, oh), R.log_image(pool))
    y0, wy = H.area_table(h, oh)
    x0, wx = H.area_table(w, ow)
    ty, tx = wy.shape[1], wx.shape[1]
    dev = lambda a: torch.as_tensor(a, device="cuda")      # noqa: E731
    d_pool, d_y0, d_wy, d_x0, d_wx = dev(pool), dev(y0), dev(wy), dev(x0), dev(wx)
    d_idx, d_shift = dev(np.array(IDX, np.int32)), dev(np.array(shifts, np.int32))
    d_mean = dev(mean) if with_mean else None
    v_whole, v = guarded(3 * oh * w * 3)
    out_whole, out = guarded(len(IDX) * oh * ow * 3)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    rc = _lib.lib.cn_hdri_rows_v(p(d_pool), p(v), p(d_y0), p(d_wy), 3, h, w, oh, ty, _stream())
    assert rc == 0, _lib.lib.cn_last_error_string()
    rc = _lib.lib.cn_hdri_rows_h(p(v), p(out), p(d_idx), p(d_shift), p(d_x0), p(d_wx), p(d_mean), len(IDX), 3, w, oh, ow, tx, _stream())
    assert rc == 0, _lib.lib.cn_last_error_string()
    torch.cuda.synchronize()
    assert guards_intact(v_whole) and guards_intact(out_whole)
    top = max(1.0, float(R.log_image(pool).max()))
    bound = (ty + tx + 6) * U * top
    err_v = float(np.abs(v.cpu().numpy().reshape(v_ref.shape).astype(np.float64) - v_ref).max())
    err = float(np.abs(out.cpu().numpy().reshape(ref.shape).astype(np.float64) - ref).max())
    note("rows %dx%d -> %dx%d mean=%d: rows_v error / bound %.3f, rows_h error / bound %.3f (bound %.3e)"
         % (h, w, oh, ow, with_mean, err_v / bound, err / bound, bound))
    assert err_v <= bound
    assert err <= bound
    if not with_mean:                                # the wrappers of ops.py launch the same thing
        from confignet_amd import ops
        got = ops.hdri_rows_h(ops.hdri_rows_v(d_pool, d_y0, d_wy, oh), d_idx, d_shift, d_x0, d_wx, ow)
        assert got.shape == (len(IDX), oh, ow, 3) and torch.equal(got.reshape(-1), out)


def test_bad_arguments_are_refused_without_a_launch():
    from confignet_amd import _lib
    lib = _lib.lib
    t = torch.zeros(64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = lambda a: ctypes.c_void_p(a.data_ptr())      # noqa: E731
    calls = ((lambda: lib.cn_hdri_rows_v(p(t), p(t), p(i), p(t), 1, 4, 4, 5, 2, None), b"enlarges"),
             (lambda: lib.cn_hdri_rows_v(None, p(t), p(i), p(t), 1, 4, 4, 2, 3, None), b"NULL"),
             (lambda: lib.cn_hdri_rows_v(p(t), p(t), p(i), p(t), 1, 4, 4, 2, 2, None), b"too few"),                       # scale 2 needs 3
             (lambda: lib.cn_hdri_rows_h(p(t), p(t), p(i), p(i), p(i), p(t), None, 1, 1, 4, 1, 5, 2, None), b"enlarges"),
             (lambda: lib.cn_hdri_rows_h(p(t), p(t), None, p(i), p(i), p(t), None, 1, 1, 4, 1, 2, 3, None), b"NULL"),
             (lambda: lib.cn_hdri_rows_h(p(t), p(t), p(i), p(i), p(i), p(t), None, 1, 1, 5, 1, 2, 3, None), b"too few"),  # 2.5 needs 4
             (lambda: lib.cn_exp2m1(None, p(t), 4, None), b"NULL"))
    for call, word in calls:
        rc = call()
        assert rc == -1 and word in lib.cn_last_error_string(), (rc, word, lib.cn_last_error_string())
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


def test_a_sample_whose_image_index_is_outside_the_pool_is_marked_not_read():
    """Straight through the C ABI (HDRIModelPCA refuses such an index on the host): the sample comes out as NaN, its neighbours
    are computed, nothing outside the output is written."""
    from confignet_amd import _lib, hdri
    h, w, oh, ow = 8, 16, 4, 8
    pool = np.random.default_rng(2).uniform(0.1, 4.0, (2, h, w, 3)).astype(np.float32)
    idx, shifts = [1, 2, 0, -1], [0, 0, 3, 0]
    (y0, wy), (x0, wx) = hdri.area_table(h, oh), hdri.area_table(w, ow)
    dev = lambda a: torch.as_tensor(a, device="cuda")      # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    v = torch.empty((2, oh, w, 3), device="cuda")
    whole, out = guarded(len(idx) * oh * ow * 3)
    d = [dev(a) for a in (pool, y0, wy, np.array(idx, np.int32), np.array(shifts, np.int32), x0, wx)]
    assert _lib.lib.cn_hdri_rows_v(p(d[0]), p(v), p(d[1]), p(d[2]), 2, h, w, oh, wy.shape[1], None) == 0
    assert _lib.lib.cn_hdri_rows_h(p(v), p(out), p(d[3]), p(d[4]), p(d[5]), p(d[6]), None, len(idx), 2, w, oh, ow, wx.shape[1], None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(idx), oh, ow, 3)
    assert guards_intact(whole) and np.isnan(got[1]).all() and np.isnan(got[3]).all()
    want = R.rows(pool, [1, 0], [0, 3], (oh, ow))
    assert np.abs(got[[0, 2]] - want).max() <= (wy.shape[1] + wx.shape[1] + 6) * U * max(1.0, float(R.log_image(pool).max()))


def test_rows_are_bit_identical_where_the_arithmetic_is(H, images, reference_model):
    from confignet_amd import ops
    dev = lambda a: torch.as_tensor(a, device="cuda")      # noqa: E731
    # factor 4 along the width: a shift by 8 source columns is a roll by 2 output columns, same weights on the same values
    y0, wy = H.area_table(64, 16)
    x0, wx = H.area_table(128, 32)
    v = ops.hdri_rows_v(dev(np.array(images)), dev(y0), dev(wy), 16)
    idx = dev(np.array([0, 1, 2, 0, 1, 2], np.int32))
    rows = ops.hdri_rows_h(v, idx, dev(np.array([0, 0, 0, 8, 8, 8], np.int32)), dev(x0), dev(wx), 32)
    assert torch.equal(rows[3:], torch.roll(rows[:3], 2, dims=2)) and not torch.equal(rows[3:], rows[:3])
    # the two ends of a turntable are the same picture: -180 and +180 degrees are shifts of -64 and +64 of 128 columns
    ends = reference_model.rows_indexed(images[1:2], [0, 0], [-180.0, 180.0])
    assert ends.shape == (2, 600) and np.array_equal(ends[0].view(np.uint32), ends[1].view(np.uint32))
    # samples drawn from a pool by index == the same pictures stacked sample by sample
    rot = [10.0, -75.5, 200.0, 359.0, 0.0, 90.0, -180.0]
    a = reference_model.rows_indexed(images, IDX, rot, centred=True)
    b = reference_model.rows_indexed(images[IDX], np.arange(len(IDX)), rot, centred=True)
    assert a.shape == (7, 600) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(reference_model.transform_indexed(images, IDX, rot).shape, (7, 5))
    with pytest.raises(ValueError):
        reference_model.transform_indexed(images, [3], [0.0])


def test_fit_on_the_device_path_reproduces_the_reference_model(H, images, reference_model):
    """The whole fit -- kernels for the rows (float32), host decomposition -- against the reference's pickle, on the bars of the
    CPU pin (tests/test_hdri_cpu.py)."""
    np.random.seed(0)
    model = H.HDRIModelPCA((10, 20), 5)
    model.fit(np.array(images), 5)
    d = pin_distances(model.pca_model, reference_model.pca_model)
    print("pin (device rows):", d)
    write_pin("device: HDRIModelPCA.fit (float32 rows from the kernels)", d, "a")
    assert model.pca_model.components_.shape == (5, 600)
    assert d[0] <= BAR_MEAN
    assert (d[1] <= BAR_COMPONENTS).all()
    assert d[2] <= BAR_VARIANCE_REL
    assert d[3] <= BAR_NOISE


def test_transform_and_inverse_against_the_restatement(images, reference_model, reference_rows):
    pca = reference_model.pca_model
    mean, comps, ev = (np.asarray(a, np.float64) for a in (pca.mean_, pca.components_, pca.explained_variance_))
    centred = reference_rows - mean
    want = R.transform(centred, comps, ev)
    got = reference_model.transform(np.array(images))
    assert got.shape == (3, 5) and got.dtype == np.float32
    bound = (600 + 12) * U * np.einsum("nf,kf->nk", np.abs(centred), np.abs(comps)) / np.sqrt(ev)
    ratio = float((np.abs(got - want) / bound).max())
    note("transform (3 pictures, reference model): error / bound %.3f (bounds %.2e .. %.2e)" % (ratio, bound.min(), bound.max()))
    assert ratio <= 1.0
    # inverse: before the exp2 ...
    x = want.astype(np.float32)
    y_want = R.inverse_log(x, mean, comps, ev)
    b = (5 + 12) * U * (np.einsum("nk,kf->nf", np.abs(x.astype(np.float64)) * np.sqrt(ev), np.abs(comps)) + np.abs(mean))
    y_got = reference_model.inverse_transform(x, log=True).reshape(3, -1)
    ratio_y = float((np.abs(y_got - y_want) / b).max())
    # ... and after it
    img_want = R.inverse(x, mean, comps, ev).reshape(3, 10, 20, 3)
    img_got = reference_model.inverse_transform(x)
    assert img_got.shape == (3, 10, 20, 3) and img_got.dtype == np.float32
    b_img = (4 * U * np.maximum(np.exp2(y_want), np.abs(np.exp2(y_want) - 1)) + np.exp2(y_want) * (np.exp2(b) - 1)).reshape(img_want.shape)
    ratio_img = float((np.abs(img_got - img_want) / b_img).max())
    note("inverse_transform: error / bound %.3f before the exp2, %.3f after it" % (ratio_y, ratio_img))
    assert ratio_y <= 1.0
    assert ratio_img <= 1.0


def test_exp2m1_elementwise():
    from confignet_amd import ops
    x = np.concatenate([np.linspace(-20, 20, 1001), [0.0, 1.0, -1.0, 126.0, -140.0]]).astype(np.float32)
    got = ops.exp2m1(torch.as_tensor(x, device="cuda")).cpu().numpy().astype(np.float64)
    want = np.exp2(x.astype(np.float64)) - 1
    # exp2f errs in proportion to 2^x, the subtraction rounds in proportion to |2^x - 1|
    assert (np.abs(got - want) <= 4 * U * np.maximum(np.exp2(x.astype(np.float64)), np.abs(want))).all()
    assert got[1001] == 0.0 and got[1002] == 1.0 and got[1003] == -0.5


def test_the_reference_round_trip_assertion(images, reference_model):
    """tests/hdri_encoding_test.py of the reference, test_hdri_transform, with its own tolerance."""
    emb_1 = reference_model.transform(np.array(images))
    img_1 = reference_model.inverse_transform(emb_1)
    emb_2 = reference_model.transform(img_1)
    img_2 = reference_model.inverse_transform(emb_2)
    note("round trip: second embeddings - first %.3e, second pictures - first %.3e" % (np.abs(emb_2 - emb_1).max(), np.abs(img_2 - img_1).max()))
    assert np.isclose(emb_2, emb_1, atol=1e-6).all()
    assert np.isclose(img_2, img_1, atol=1e-6).all()


class _StubNetworks:
    """Stands in for a trained ConfigNet + LatentGAN in front of DemoSession: records what the session splices in."""
    config = {"facemodel_inputs": {"hdri_embedding": (5, 4), "bone_rotations:left_eye": (3, 2)}}

    def __init__(self):
        self.spliced = []

    def generate_latents(self, n, truncation=1.0):
        return np.zeros((n, 6), np.float32)

    def generate_images(self, emb, rot):
        return np.zeros((len(emb), 8, 8, 3), np.uint8)

    def set_facemodel_param_in_latents(self, latents, name, value):
        self.spliced.append((name, np.array(value)))
        return latents


def test_turntable_script_feeds_the_demo(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "hdri_encoding"))
    import generate_hdri_turntable_inputs
    from confignet_amd.demo import DemoSession
    out = str(tmp_path / "turntable.npy")
    generate_hdri_turntable_inputs.parse_args(["--hdri_file_path", os.path.join(ASSETS, "001.hdr"), "--output_file_path", out,
                                               "--hdri_model_path", os.path.join(ASSETS, "hdri_model.pck")])
    emb = np.load(out)
    assert emb.shape == (90, 5) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert np.array_equal(emb[0], emb[-1]) and not np.array_equal(emb[0], emb[45])         # -180 == +180; 0 degrees differs
    nets = _StubNetworks()
    session = DemoSession(nets, nets, None, 1, 1, emb)
    session.key("n")                                                                       # start the light sweep
    for _ in range(91):
        session.frame()
    frames = [v for n, v in nets.spliced if n == "hdri_embedding"]
    assert len(frames) == 91 and all(np.array_equal(f, emb[i % 90]) for i, f in enumerate(frames))


def test_metadata_script_writes_the_embeddings_of_transform(images, reference_model, tmp_path):
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "hdri_encoding"))
    import process_hdri_metadata
    os.makedirs(str(tmp_path / "assets" / "HDRI"))
    os.makedirs(str(tmp_path / "meta"))
    for name in ("000.hdr", "001.hdr", "002.hdr"):
        shutil.copy(os.path.join(ASSETS, name), str(tmp_path / "assets" / "HDRI" / name))
    cases = [("002.hdr", 1.0), ("000.hdr", -2.5)]
    for i, (name, angle) in enumerate(cases):
        with open(str(tmp_path / "meta" / ("%04d.json" % i)), "w") as f:
            json.dump({"illumination": {"HDRI_filename": name, "HDRI_rotation": [0.0, 0.0, angle]}, "other": i}, f)
    process_hdri_metadata.parse_args(["--input_dir", str(tmp_path / "meta"), "--render_asset_dir", str(tmp_path / "assets"),
                                      "--model_path", os.path.join(ASSETS, "hdri_model.pck")])
    for i, (name, angle) in enumerate(cases):
        with open(str(tmp_path / "meta" / ("%04d.json" % i))) as f:
            d = json.load(f)
        want = reference_model.transform(np.array(images[[2, 0]]), [180 * a / np.pi for _, a in cases])[i]
        assert d["other"] == i and isinstance(d["hdri_embedding"], list) and len(d["hdri_embedding"]) == 5
        assert np.array_equal(np.array(d["hdri_embedding"], np.float32), want)


@pytest.mark.parametrize("n_components, k", [("5", 5), ("0.9", 6)])
def test_model_creation_script(H, n_components, k, tmp_path):
    """The reference's test_hdri_model_creation_script: its arguments, and what it leaves behind can be read back."""
    sys.path.insert(0, os.path.join(ROOT, "hdri_encoding"))
    import hdri_pca_model
    out = str(tmp_path / "out")
    hdri_pca_model.parse_args(["--hdri_dir", ASSETS, "--output_dir", out, "--write_hdris", "--output_shape", "10", "20",
                               "--n_components", n_components])
    model = H.HDRIModelPCA.load(os.path.join(out, "hdri_model.pck"))
    assert model.output_shape == (10, 20) and model.pca_model.components_.shape == (k, 600)
    basis = sorted(os.listdir(os.path.join(out, "pca_basis")))
    assert len(basis) == k and basis[0].startswith("000.")
    for i in range(3):
        for kind in ("reconstructed", "original"):
            img = H.read_hdr(os.path.join(out, "hdris", "%03d_%s.hdr" % (i, kind)))
            assert img.shape == (10, 20, 3) and np.isfinite(img).all() and img.max() > 0

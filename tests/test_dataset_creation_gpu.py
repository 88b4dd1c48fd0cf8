"""Dataset creation on the GPU: cn_warp_affine_u8 / cn_warp_nearest_f32 / cn_eye_mask (csrc/dataset.hip) against the plain-integer
statement of tests/dataset_ref.py, bit for bit, into outputs between guard bands; and the whole pipeline with device="cuda"
against the numpy path.  The kernels are integer arithmetic, a gather and comparisons: every check is equality.  Only the
Inception features are floating point; they are compared at the tolerance tests/test_metrics_gpu.py uses for features (the two
runs feed identical bytes to the same network, so what remains is the order of its atomic reductions)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_ref as R  # noqa: E402
from test_dataset_creation_cpu import GEOMETRIES, WARP_CASES, source  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                      # bytes / floats on either side of an output
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def guarded(numel, dtype):
    fill = 0xA5 if dtype == torch.uint8 else -777.0
    whole = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + numel], fill


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_u8(src, tabs, oh, ow):
    from confignet_amd import ops
    n, c = src.shape[0], src.shape[3]
    whole, mid, fill = guarded(n * oh * ow * c, torch.uint8)
    out = ops.warp_affine_u8(dev(src), [dev(t) for t in tabs], oh, ow, out=mid.view(n, oh, ow, c))
    torch.cuda.synchronize()
    assert guards_intact(whole, fill)
    return out.cpu().numpy()


@pytest.mark.parametrize("case,c", WARP_CASES)
def test_warp_affine_u8_equals_the_integer_statement(case, c):
    """n = 3 transforms in one launch (a rotation by 30 degrees, scales 0.5 and 2.0, fractional shifts), 5x7 -> 4x6 and 7x5 -> 9x3,
    transforms that leave the source, a 1x1 source, 64x64 -> 33x31 random bytes; 1, 3 and 4 channels"""
    shape, (oh, ow), Ms = GEOMETRIES[case]
    src = source(shape, c, len(Ms), seed=case)
    per = [R.tables(M, oh, ow, 16) for M in Ms]
    got = run_u8(src, R.stack_tables(per), oh, ow)
    for i in range(len(Ms)):
        assert np.array_equal(got[i], R.warp_u8_int(src[i], per[i], oh, ow))
    if case == 2:
        assert not got.any()


def hostile_tables(oh, ow):
    """per image (x0, y0, adelta, bdelta) fills: sums far outside any source in both directions, and sums that cancel"""
    fills = [(I32_MAX, I32_MAX, I32_MAX, I32_MAX), (I32_MIN, I32_MIN, I32_MIN, I32_MIN), (I32_MAX, I32_MIN, I32_MAX, I32_MIN),
             (I32_MAX, I32_MAX, I32_MIN, I32_MIN), (I32_MAX, 16, 0, 0), (16, I32_MIN, 0, 0)]
    per = [([f[0]] * oh, [f[1]] * oh, [f[2]] * ow, [f[3]] * ow) for f in fills]
    return per, [0, 1, 2, 4, 5]          # the images that must come out all zero (3: MAX + MIN = -1, next to source pixel (0, 0))


@pytest.mark.parametrize("c", [1, 3, 4])
def test_hostile_table_entries_read_nothing(c):
    oh, ow = 4, 6
    per, zero = hostile_tables(oh, ow)
    src = np.full((len(per), 5, 7, c), 255, np.uint8)
    got = run_u8(src, R.stack_tables(per), oh, ow)
    for i in range(len(per)):
        assert np.array_equal(got[i], R.warp_u8_int(src[i], per[i], oh, ow))
    assert not got[zero].any()
    from confignet_amd import ops
    fsrc = np.full((len(per), 5, 7, 3), 3.5, np.float32)
    whole, mid, fill = guarded(len(per) * oh * ow * 3, torch.float32)
    out = ops.warp_nearest_f32(dev(fsrc), [dev(t) for t in R.stack_tables(per)], oh, ow, out=mid.view(len(per), oh, ow, 3)).cpu().numpy()
    assert guards_intact(whole, fill)
    for i in range(len(per)):
        assert np.array_equal(out[i], R.warp_nearest(fsrc[i], per[i], oh, ow))
    assert not out[zero].any()


def test_bad_arguments_are_refused():
    from confignet_amd import ops
    from confignet_amd._lib import ConfigNetHipError
    src = dev(np.zeros((1, 4, 4, 5), np.uint8))
    tabs = [dev(np.zeros((1, 4), np.int32))] * 4
    with pytest.raises(ConfigNetHipError, match="channels"):
        ops.warp_affine_u8(src, tabs, 4, 4)
    with pytest.raises(AssertionError):
        ops.warp_affine_u8(src[..., :3], tabs, 4, 5)                     # tables shorter than the output rows


@pytest.mark.parametrize("case", range(4))
def test_warp_nearest_and_eye_mask_equal_the_reference_form(case):
    from confignet_amd import ops
    from confignet_amd.neural_renderer_dataset import EyeRegionSpec
    shape, (oh, ow), Ms = GEOMETRIES[case]
    n = len(Ms)
    rng = np.random.default_rng(case)
    # UV values on a coarse grid that holds every float32 bound and its neighbours, so masks flip inside the small pictures
    pool = R.threshold_uv()[:2].reshape(-1, 3)
    src = pool[rng.integers(0, len(pool), size=(n,) + shape)]
    src[0, 0, 0] = [np.nan, np.inf, -0.0]
    per = [R.tables(M, oh, ow, 512) for M in Ms]
    whole, mid, fill = guarded(n * oh * ow * 3, torch.float32)
    warped = ops.warp_nearest_f32(dev(src), [dev(t) for t in R.stack_tables(per)], oh, ow, out=mid.view(n, oh, ow, 3))
    mwhole, mmid, mfill = guarded(n * oh * ow, torch.uint8)
    mask = ops.eye_mask(warped, EyeRegionSpec.bounds(), out=mmid.view(n, oh, ow))
    torch.cuda.synchronize()
    assert guards_intact(whole, fill) and guards_intact(mwhole, mfill)
    warped, mask = warped.cpu().numpy(), mask.cpu().numpy()
    for i in range(n):
        ref = R.warp_nearest(src[i], per[i], oh, ow)
        assert np.array_equal(warped[i].view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(mask[i], R.eye_mask(ref))


def test_eye_mask_at_the_thresholds():
    from confignet_amd import ops
    from confignet_amd.neural_renderer_dataset import EyeRegionSpec, eye_mask_from_uv
    uv = R.threshold_uv()
    got = ops.eye_mask(dev(uv), EyeRegionSpec.bounds()).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, R.eye_mask(uv)) and got.sum() == 4 + 4 + 2
    assert np.array_equal(eye_mask_from_uv(uv, device="cuda"), eye_mask_from_uv(uv))
    two = np.ascontiguousarray(uv[..., :2])                               # two channels: the stride is the channel count
    assert np.array_equal(ops.eye_mask(dev(two), EyeRegionSpec.bounds()).cpu().numpy(), got)


def test_pipeline_on_the_gpu_equals_the_numpy_path(tmp_path):
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    sets = {}
    for device in (None, "cuda"):
        root = str(tmp_path / ("renders_%s" % device))
        R.write_render_tree(root)
        out = str(tmp_path / ("set_%s.pck" % device))
        ds = NeuralRendererDataset((96, 96, 3), True, device=device)
        ds.generate_face_dataset(root, out, attribute_label_file_path=os.path.join(root, "list_attr_celeba.txt"), pre_normalize=False)
        sets[device] = NeuralRendererDataset.load(out)
    a, b = sets[None], sets["cuda"]
    assert a.imgs.shape == (2, 96, 96, 3) and np.asarray(a.imgs).any() and 0 < a.eye_masks.sum() < a.eye_masks.size
    assert np.array_equal(a.imgs, b.imgs) and np.array_equal(a.eye_masks, b.eye_masks)
    assert a.attributes == b.attributes and a.render_metadata == b.render_metadata
    assert b.inception_features.shape == (2, 2048) and np.isfinite(b.inception_features).all() and np.abs(b.inception_features).max() > 0
    np.testing.assert_allclose(b.inception_features, a.inception_features, rtol=1e-4, atol=1e-5)
    # the pre-normalisation's 1024 x 1024 pictures too: several row blocks, more than one workgroup per row
    from confignet_amd import face_image_normalizer as F
    src = source((40, 48), 3, 2, seed=5)
    Ms = [np.array([[20.0, 3.0, 11.5], [-3.0, 20.0, 7.25]]), np.array([[0.0, 25.0, -3.0], [-25.0, 0.0, 1030.0]])]
    assert np.array_equal(F.warp_affine(src, Ms, (1024, 1024), device="cuda"), F.warp_affine(src, Ms, (1024, 1024)))
    uv = np.random.default_rng(6).random((2, 40, 48, 3)).astype(np.float32)
    assert np.array_equal(F.warp_affine_nearest(uv, Ms, (1024, 1024), device="cuda"), F.warp_affine_nearest(uv, Ms, (1024, 1024)))

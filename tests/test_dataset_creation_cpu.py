"""Dataset creation without a GPU: the numpy statement of cv2.warpAffine (confignet_amd/face_image_normalizer.py) against two
independent statements (tests/dataset_ref.py: plain integers, and float64), the normalising transforms, the OpenFace file
parsing, the OpenEXR reader and writer, the eye mask at its float32 bounds, and the whole pipeline on three synthetic renders.
Everything compared for equality is integer or exactly representable arithmetic; the 1e-9 of the transform tests is float64
rounding of landmark coordinates of the order of 1e3 through a handful of operations (~1e-13), with room."""
import glob
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def F():
    from confignet_amd import face_image_normalizer
    return face_image_normalizer


def rot(deg, scale=1.0, tx=0.0, ty=0.0):
    a = np.deg2rad(deg)
    return np.array([[scale * np.cos(a), scale * np.sin(a), tx], [-scale * np.sin(a), scale * np.cos(a), ty]])


# (source shape, (oh, ow), transforms) -- shared with tests/test_dataset_creation_gpu.py
GEOMETRIES = [
    ((5, 7), (4, 6), [rot(30, 1.0, 1.5, -0.5), rot(0, 0.5), rot(0, 2.0, -1.0, 0.5)]),
    ((7, 5), (9, 3), [rot(30, 1.0, 2.0, 3.0), rot(-75, 2.0, 4.0, 1.0), rot(0, 1.0, 0.3, 1.7)]),
    ((5, 7), (4, 6), [rot(0, 1.0, 100.0, 0.0), rot(0, 1.0, 0.0, -50.0), rot(0, 1.0, 1e12, 0.0)]),        # leaves the source
    ((1, 1), (3, 4), [rot(0, 1.0, 1.0, 1.0), rot(0, 1.0, 0.5, 0.5), rot(45, 3.0, 1.0, 1.0)]),
    ((64, 64), (33, 31), [rot(17, 0.45, 3.3, -2.2)]),
]


def source(shape, c, n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + tuple(shape) + (c,), dtype=np.uint8)


# every small geometry with 1, 3 and 4 channels; the larger random one once
WARP_CASES = [(case, c) for case in range(4) for c in (1, 3, 4)] + [(4, 3)]


@pytest.mark.parametrize("case,c", WARP_CASES)
def test_warp_equals_the_integer_and_the_float64_statement(F, case, c):
    shape, (oh, ow), Ms = GEOMETRIES[case]
    src = source(shape, c, len(Ms), seed=case)
    got = F.warp_affine(src, Ms, (ow, oh))
    assert got.shape == (len(Ms), oh, ow, c) and got.dtype == np.uint8
    tabs = [R.tables(M, oh, ow, 16) for M in Ms]
    ours = F.batch_tables(Ms, oh, ow, F.ROUND_DELTA_LINEAR)
    for a, b in zip(ours, R.stack_tables(tabs)):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    for i in range(len(Ms)):
        assert np.array_equal(got[i], R.warp_u8_int(src[i], tabs[i], oh, ow))
        assert np.array_equal(got[i], R.warp_u8_float64(src[i], tabs[i], oh, ow))
    if case == 2:
        assert not got.any()


def test_warp_known_answers(F):
    src = source((6, 9), 3, 1, seed=9)
    eye = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(F.warp_affine(src, [eye], (9, 6)), src)
    shifted = F.warp_affine(src, [np.array([[1.0, 0, 2], [0, 1.0, 1]])], (9, 6))[0]
    assert np.array_equal(shifted[1:, 2:], src[0, :-1, :-2]) and not shifted[0].any() and not shifted[:, :2].any()
    assert not F.warp_affine(src, [np.array([[1.0, 0, 1000], [0, 1.0, 0]])], (9, 6)).any()
    one = np.full((1, 1, 1, 3), 200, np.uint8)
    out = F.warp_affine(one, [eye], (3, 2))[0]
    assert np.array_equal(out[0, 0], [200, 200, 200]) and out.sum() == 600
    # half a pixel to the right: the single source pixel is shared by two output pixels
    half = F.warp_affine(one, [np.array([[1.0, 0, 0.5], [0, 1.0, 0]])], (3, 2))[0]
    assert half[0, :, 0].tolist() == [100, 100, 0]
    # a singular transform: cv2 takes 1 / 0 as 0, so every output pixel reads source (0, 0)
    sing = F.warp_affine(src, [np.zeros((2, 3))], (4, 4))
    assert (sing == src[0, 0, 0]).all()


def test_nearest_warp_equals_the_integer_statement_and_keeps_special_values(F):
    for case, (shape, (oh, ow), Ms) in enumerate(GEOMETRIES[:4]):
        rng = np.random.default_rng(case)
        src = rng.random((len(Ms),) + shape + (3,)).astype(np.float32)
        src[0, 0, 0] = [np.nan, np.inf, -0.0]
        got = F.warp_affine_nearest(src, Ms, (ow, oh))
        for i, M in enumerate(Ms):
            ref = R.warp_nearest(src[i], R.tables(M, oh, ow, 512), oh, ow)
            assert got.dtype == np.float32 and np.array_equal(got[i].view(np.uint32), ref.view(np.uint32))


def test_euler_convention_is_scipys_intrinsic_XYZ(F):
    from scipy.spatial.transform import Rotation
    for angles in [(0.3, -0.2, 0.5), (1.2, 0.7, -2.0), (0.0, 0.0, 0.4)]:
        got = F.euler_matrix_rxyz(*angles)
        assert np.abs(got - Rotation.from_euler("XYZ", angles).as_matrix()).max() < 1e-15
    assert np.abs(F.euler_matrix_rxyz(0.3, -0.2, 0.5) - Rotation.from_euler("xyz", (0.3, -0.2, 0.5)).as_matrix()).max() > 0.1


def test_2d_transform_maps_the_landmark_groups_onto_the_reference_positions(F):
    N = F.FaceImageNormalizer
    size = (1024, 1024)
    target = N.ref_pre_norm_landmark_positions * np.array(size)
    a = np.deg2rad(-23.0)
    S = 1.7 * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    t = np.array([310.0, -45.0])
    groups = (target - t) @ np.linalg.inv(S).T                           # an exact similarity of the reference positions
    rng = np.random.default_rng(1)
    landmarks = rng.uniform(0, 1000, size=(68, 2))
    for idxs, g in zip(N.ref_pre_norm_landmark_idxs, groups):
        if len(idxs) == 2:
            d = rng.uniform(-20, 20, size=2)
            landmarks[idxs[0]], landmarks[idxs[1]] = g - d, g + d        # the group is the mean of the two
        else:
            landmarks[idxs[0]] = g
    M = N._get_normalizing_transform_2d(landmarks, size)
    assert M.shape == (2, 3)
    assert np.abs(groups @ M[:, :2].T + M[:, 2] - target).max() < 1e-9
    assert np.abs(M[:, :2] - S).max() < 1e-9


def test_3d_transform_centres_the_head_and_takes_the_mean_scale(F):
    N = F.FaceImageNormalizer
    K = np.array([[900.0, 0, 320], [0, 900.0, 240], [0, 0, 1]])
    pose = np.array([12.0, -8.0, 600.0, 0.0, 0.0, 0.0])
    l3 = R.face_landmarks_3d() + pose[:3]
    l2 = R.project(l3, K)
    shape = (256, 256, 3)
    M = N._get_normalizing_transform_3d(l2, l3, pose, K, shape)
    assert M.shape == (2, 3)
    centre = R.project(l3[[0, 16]].mean(axis=0, keepdims=True), K)[0]
    assert np.abs(M[:, :2] @ centre + M[:, 2] - np.array([0.5, 0.42]) * 256).max() < 1e-9
    interocular = np.linalg.norm(l2[36] - l2[45])
    eye_to_mouth = np.linalg.norm(l2[51] - (l2[36] + l2[45]) / 2)
    scale = (0.45 * 256 / interocular + 0.34 * 256 / eye_to_mouth) / 2
    assert abs(np.sqrt(abs(np.linalg.det(M[:, :2]))) - scale) < 1e-9
    assert abs(M[0, 1]) < 1e-9                                           # the eyes are level: no rotation
    # a rotated head is turned back before the distances are taken: the scale does not change, the in-plane rotation does
    pose_r = pose.copy()
    pose_r[3:] = (0.2, -0.3, 0.25)
    Rm = F.euler_matrix_rxyz(*pose_r[3:])
    l3_r = (l3 - pose[:3]) @ Rm.T + pose[:3]
    M_r = N._get_normalizing_transform_3d(R.project(l3_r, K), l3_r, pose_r, K, shape)
    assert abs(np.sqrt(abs(np.linalg.det(M_r[:, :2]))) - scale) < 1e-9
    assert abs(M_r[0, 1]) > 1e-3


def test_openface_files(tmp_path):
    from confignet_amd import dataset_utils as D
    K = np.array([[500.0, 0, 64.5], [0, 510.0, 48.25], [0, 0, 1]])
    rng = np.random.default_rng(2)
    faces = [(rng.uniform(0, 100, (68, 2)), rng.uniform(-50, 50, (68, 3)), rng.uniform(-1, 1, 6)) for _ in range(3)]
    rows = [R.openface_csv_row(i, conf, *f) for i, (conf, f) in enumerate(zip((0.7, 0.93, 0.2), faces))]
    R.write_openface_files(str(tmp_path), "two", rows[:2], K)
    R.write_openface_files(str(tmp_path), "one", rows[1:2], K)
    R.write_openface_files(str(tmp_path), "low", rows[2:], K)
    assert open(tmp_path / "two.csv").readline().split(",")[1] == " confidence"          # the headers are padded
    for name in ("two", "one"):
        l2, l3, pose = D.read_landmarks_and_pose_from_csv(str(tmp_path / (name + ".csv")))
        assert np.array_equal(l2, faces[1][0]) and np.array_equal(l3, faces[1][1]) and np.array_equal(pose, faces[1][2])
    assert D.read_landmarks_and_pose_from_csv(str(tmp_path / "low.csv")) == (None, None, None)
    assert D.read_landmarks_and_pose_from_csv(str(tmp_path / "low.csv"), confidence_threshold=0.1)[0] is not None
    assert np.array_equal(D.read_estimated_intrinsics(str(tmp_path / "two_of_details.txt")), K)
    A, t = D.get_similarity_transform(faces[0][0] @ np.array([[0, -2.0], [2.0, 0]]).T + 3, faces[0][0])
    assert np.abs(A - [[0, -2.0], [2.0, 0]]).max() < 1e-12 and np.abs(t - 3).max() < 1e-9
    with open(tmp_path / "attr.txt", "w") as fp:
        fp.write("2\nSmiling Young\na.jpg 1 -1\nb.png  -1  1\n")
    assert D.parse_celeba_attribute_file(str(tmp_path / "attr.txt")) == {"a": {"Smiling": 1, "Young": 0}, "b": {"Smiling": 0, "Young": 1}}


def test_exr_round_trip_and_zip_blocks(tmp_path):
    from confignet_amd import exr
    rng = np.random.default_rng(3)
    img = rng.normal(size=(19, 13, 3)).astype(np.float32)
    img[0, 0] = [np.inf, -0.0, 1e-40]
    exr.imwrite(str(tmp_path / "plain.exr"), img)
    assert np.array_equal(exr.imread(str(tmp_path / "plain.exr")).view(np.uint32), img.view(np.uint32))
    smooth = np.linspace(0, 1, 35 * 21, dtype=np.float32).reshape(35, 21)              # compressible: the blocks really are deflated
    planes32 = {"B": smooth, "G": smooth[::-1].copy(), "R": rng.normal(size=(35, 21)).astype(np.float32)}
    planes16 = {k: v.astype(np.float16) for k, v in planes32.items()}
    for compression in ("ZIPS", "ZIP"):
        for planes in (planes32, planes16, {"B": planes16["B"], "G": planes32["G"], "R": planes16["R"]}):
            path = str(tmp_path / (compression + ".exr"))
            R.write_exr_compressed(path, planes, compression)
            back = exr.read_exr(path)
            assert list(back) == ["B", "G", "R"]
            for k in planes:
                assert back[k].dtype == planes[k].dtype and np.array_equal(back[k], planes[k])
            bgr = exr.imread(path)
            assert bgr.dtype == np.float32 and np.array_equal(bgr[..., 0], planes["B"].astype(np.float32))
    # what is not read says what it is
    data = bytearray(open(tmp_path / "plain.exr", "rb").read())
    at = data.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    data[at] = 4
    (tmp_path / "piz.exr").write_bytes(bytes(data))
    with pytest.raises(NotImplementedError, match="PIZ"):
        exr.imread(str(tmp_path / "piz.exr"))


def test_eye_mask_is_strict_at_the_float32_bounds():
    from confignet_amd.neural_renderer_dataset import EyeRegionSpec, eye_mask_from_uv
    uv = R.threshold_uv()
    got = eye_mask_from_uv(uv)
    assert got.dtype == np.uint8 and np.array_equal(got, R.eye_mask(uv))
    # per bound: below, on, above -> only the side inside the open interval is set
    assert got[0].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0]
    assert got[1].tolist() == [0, 0, 1, 1, 0, 0] * 2
    assert got[2].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    assert EyeRegionSpec.bounds() == tuple(np.float32(v) for v in R.EYE_L + R.EYE_R + R.EYE_Y)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
CONFIG = {"facemodel_inputs": {"hair_style": (None, 4), "blendshape_values": (None, 4), "texture_embedding": (None, 4)}}


def check_dataset(ds, tmp_path, name):
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    assert ds.imgs.shape == (2, 96, 96, 3) and ds.imgs.dtype == np.uint8 and np.asarray(ds.imgs).any()
    assert ds.eye_masks.shape == (2, 96, 96) and ds.eye_masks.dtype == np.uint8 and 0 < ds.eye_masks.sum() < ds.eye_masks.size
    assert ds.inception_features.shape == (2, 2048) and np.isfinite(ds.inception_features).all()
    assert len(ds.render_metadata) == 2 and all(abs(m["bone_rotations"]["head"][0]) < 0.2 for m in ds.render_metadata)
    assert len(ds.attributes) == 2 and all(set(a) == {"Smiling", "Young"} for a in ds.attributes)
    pck = open(tmp_path / "out" / (name + ".pck"), "rb").read()
    assert b"confignet.neural_renderer_dataset" in pck and b"NeuralRendererDataset" in pck and b"confignet_amd" not in pck
    assert os.path.getsize(tmp_path / "out" / (name + "_imgs.dat")) == 2 * 96 * 96 * 3 and len(pck) < 200000   # the images are not pickled
    back = NeuralRendererDataset.load(str(tmp_path / "out" / (name + ".pck")))
    assert np.array_equal(back.imgs, ds.imgs) and np.array_equal(back.eye_masks, ds.eye_masks)
    assert np.array_equal(back.inception_features, ds.inception_features)
    assert back.render_metadata == ds.render_metadata and back.attributes == ds.attributes and tuple(back.img_shape) == (96, 96, 3)
    # the normaliser wrote all three renders; the dataset dropped the one whose head pose is out of range
    names = sorted(os.listdir(tmp_path / "renders" / "normalized"))
    assert "img_00002.png" in names and "uv_00002.exr" in names and "normalization_done" in names
    return back


def test_generate_face_dataset_end_to_end(tmp_path, F):
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    root = str(tmp_path / "renders")
    tree_imgs, tree_uvs = R.write_render_tree(root)
    os.makedirs(tmp_path / "out")
    out = str(tmp_path / "out" / "synth.pck")
    ds = NeuralRendererDataset((96, 96, 3), True)
    extractor = R.OracleFeatureExtractor()
    ds.generate_face_dataset(root, out, attribute_label_file_path=os.path.join(root, "list_attr_celeba.txt"), pre_normalize=False,
                             feature_extractor=extractor)
    back = check_dataset(ds, tmp_path, "synth")
    # each stored picture is the warp of its render by the transform of its landmark file, in B, G, R; each mask that of its UV map
    from confignet_amd import dataset_utils as D
    kept = sorted(int(os.path.basename(p)[4:9]) for p in glob.glob(os.path.join(root, "normalized", "img_*.png")))
    assert kept == [0, 1, 2]                                             # the normaliser keeps all; the dataset drops the pose
    stored = {a["Smiling"]: k for k, a in enumerate(ds.attributes)}      # render 0: Smiling 0, render 1: Smiling 1
    for i in (0, 1):
        name = "img_%05d" % i
        l2, l3, pose = D.read_landmarks_and_pose_from_csv(os.path.join(root, "processed", name + ".csv"))
        K = D.read_estimated_intrinsics(os.path.join(root, "processed", name + "_of_details.txt"))
        M = F.FaceImageNormalizer._get_normalizing_transform_3d(l2, l3, pose, K, (96, 96, 3))
        tabs = R.tables(M, 96, 96, 16)
        assert np.array_equal(ds.imgs[stored[i]], R.warp_u8_int(tree_imgs[i], tabs, 96, 96))
        uv = R.warp_nearest(tree_uvs[i], R.tables(M, 96, 96, 512), 96, 96)
        assert np.array_equal(ds.eye_masks[stored[i]], R.eye_mask(uv))
    # a second run finds the done files and touches nothing
    stamp = {f: os.path.getmtime(os.path.join(root, "normalized", f)) for f in os.listdir(os.path.join(root, "normalized"))}
    F.FaceImageNormalizer.normalize_dataset_dir(root, False, (96, 96, 3))
    assert stamp == {f: os.path.getmtime(os.path.join(root, "normalized", f)) for f in os.listdir(os.path.join(root, "normalized"))}
    # training-time processing works on what was written
    config = {"facemodel_inputs": dict(CONFIG["facemodel_inputs"])}
    back.process_metadata(config, update_config=True)
    assert back.metadata_inputs["hair_style"].shape == (2, 2) and back.metadata_inputs["blendshape_values"].shape == (2, 3)
    assert back.metadata_inputs["rotations"].shape == (2, 3) and config["facemodel_inputs"]["texture_embedding"] == (3, 4)
    assert np.array_equal(back.get_attribute_values([0, 1], ["Young"]), [[ds.attributes[0]["Young"]], [ds.attributes[1]["Young"]]])
    back.write_images(str(tmp_path / "jpg"))
    back.write_images_by_attribute(str(tmp_path / "jpg"))
    assert sorted(os.listdir(tmp_path / "jpg")) == ["00000.jpg", "00001.jpg", "Smiling", "Young", "mean_img.jpg"]
    # the reference's own unpickler needs nothing of this package: the class path resolves to whatever module carries that name
    import types
    fake = types.ModuleType("confignet.neural_renderer_dataset")

    class NeuralRendererDataset_:                                         # noqa: N801
        pass
    NeuralRendererDataset_.__name__ = NeuralRendererDataset_.__qualname__ = "NeuralRendererDataset"
    fake.NeuralRendererDataset = NeuralRendererDataset_

    class U(pickle.Unpickler):
        def find_class(self, module, name):
            if module == "confignet.neural_renderer_dataset":
                return getattr(fake, name)
            return super().find_class(module, name)
    with open(out, "rb") as fp:
        plain = U(fp).load()
    assert plain.imgs is None and not hasattr(plain, "_device") and plain.imgs_memmap_filename == "synth_imgs.dat"


def test_generate_dataset_command_line(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import generate_dataset
    from confignet_amd import neural_renderer_dataset as nrd
    root = str(tmp_path / "renders")
    R.write_render_tree(root)
    monkeypatch.setattr(nrd.NeuralRendererDataset, "_compute_inception_features",
                        lambda self, feature_extractor=None: setattr(self, "inception_features", np.zeros((len(self.imgs), 2048), np.float32)))
    ds = generate_dataset.parse_args(["--dataset_dir", root, "--dataset_name", "cli", "--output_dir", str(tmp_path / "out"),
                                      "--img_size", "96", "--pre_normalize", "0", "--load_attributes", "--synthetic_data",
                                      "--img_output_dir", str(tmp_path / "jpg")])
    assert os.path.exists(tmp_path / "out" / "cli_res_96.pck") and os.path.exists(tmp_path / "out" / "cli_res_96_imgs.dat")
    assert ds.imgs.shape == (2, 96, 96, 3) and os.path.exists(tmp_path / "jpg" / "mean_img.jpg") and os.path.isdir(tmp_path / "jpg" / "Young")


def test_demo_image_path_takes_a_directory_a_file_and_an_npy(tmp_path, F):
    sys.path.insert(0, os.path.join(ROOT, "evaluation"))
    sys.path.insert(0, ROOT)
    import confignet_demo
    root = str(tmp_path / "photos")
    R.write_render_tree(root, n=2, out_of_range=())
    pre = os.path.join(root, "pre_normalized")
    with pytest.raises(ImportError, match="OpenFace not found"):
        confignet_demo.process_images(root, 96, openface_path=str(tmp_path / "no_such_binary"))
    assert not os.path.exists(os.path.join(pre, "normalization_done")) and not os.path.exists(os.path.join(root, "normalized"))
    assert sorted(f for f in os.listdir(pre) if f.endswith(".png")) == ["img_%05d.png" % i for i in range(2)]
    K = np.array([[2000.0, 0, 512], [0, 2000.0, 512], [0, 0, 1]])
    pose = np.array([0.0, 0.0, 900.0, 0.0, 0.0, 0.0])
    l3 = R.face_landmarks_3d() + pose[:3]
    for i in range(2):
        R.write_openface_files(os.path.join(pre, "processed"), "img_%05d" % i, [R.openface_csv_row(0, 0.9, R.project(l3, K), l3, pose)], K)
    open(os.path.join(pre, "landmarks_detected"), "w").close()
    imgs = confignet_demo.process_images(root, 96, openface_path=str(tmp_path / "no_such_binary"))
    assert len(imgs) == 2 and all(im.shape == (96, 96, 3) and im.dtype == np.uint8 for im in imgs)
    assert not os.path.exists(os.path.join(root, "normalized", "normalization_done"))        # the demo writes no done file
    np.save(str(tmp_path / "faces.npy"), np.stack(imgs))
    assert len(confignet_demo.process_images(str(tmp_path / "faces.npy"), 96)) == 2
    np.save(str(tmp_path / "face.npy"), imgs[0])
    assert len(confignet_demo.process_images(str(tmp_path / "face.npy"), 96)) == 1
    with pytest.raises(ImportError, match="OpenFace not found"):                               # a single picture needs the binary
        confignet_demo.process_images(os.path.join(root, "img_00000.png"), 96, openface_path=str(tmp_path / "no_such_binary"))
    with pytest.raises(ValueError):
        confignet_demo.process_images(str(tmp_path / "nothing_here"), 96)


def test_pre_normalisation_needs_the_second_landmark_pass(tmp_path, F):
    """pre_normalize=True without a binary: the first pass is there (marker file), pre_normalized/ is written, then the landmark
    run on it raises before any normalization_done file exists; once the user has filled pre_normalized/processed and set the
    marker, a second call runs through."""
    N = F.FaceImageNormalizer
    root = str(tmp_path / "photos")
    imgs, _ = R.write_render_tree(root, n=2, out_of_range=())
    missing = str(tmp_path / "FaceLandmarkImg")
    with pytest.raises(ImportError, match="OpenFace not found, please download it using the download_deps.py script."):
        N.normalize_dataset_dir(root, True, (96, 96, 3), openface_path=missing)
    pre = os.path.join(root, "pre_normalized")
    assert not os.path.exists(os.path.join(pre, "normalization_done")) and not os.path.exists(os.path.join(root, "normalized"))
    from PIL import Image
    first = np.asarray(Image.open(os.path.join(pre, "img_00000.png")))
    assert first.shape == (1024, 1024, 3)
    K = np.array([[2000.0, 0, 512], [0, 2000.0, 512], [0, 0, 1]])
    pose = np.array([0.0, 0.0, 900.0, 0.0, 0.0, 0.0])
    l3 = R.face_landmarks_3d() + pose[:3]
    for i in range(2):
        R.write_openface_files(os.path.join(pre, "processed"), "img_%05d" % i, [R.openface_csv_row(0, 0.9, R.project(l3, K), l3, pose)], K)
    open(os.path.join(pre, "landmarks_detected"), "w").close()
    N.normalize_dataset_dir(root, True, (96, 96, 3), openface_path=missing)
    assert os.path.exists(os.path.join(pre, "normalization_done")) and os.path.exists(os.path.join(root, "normalized", "normalization_done"))
    out = F.imread(os.path.join(root, "normalized", "img_00001.png"))
    assert out.shape == (96, 96, 3) and out.any()
    # the UV maps went through both warps
    assert os.path.exists(os.path.join(pre, "uv_00001.exr")) and os.path.exists(os.path.join(root, "normalized", "uv_00001.exr"))


def test_missing_landmarks_raise_the_references_import_error(tmp_path, F):
    root = str(tmp_path / "photos")
    R.write_render_tree(root, n=1, out_of_range=(), with_landmarks=False)
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    with pytest.raises(ImportError, match="OpenFace not found, please download it using the download_deps.py script."):
        NeuralRendererDataset((96, 96, 3), True).generate_face_dataset(root, str(tmp_path / "x.pck"), pre_normalize=False,
                                                                      openface_path=str(tmp_path / "FaceLandmarkImg"))
    assert not os.path.exists(tmp_path / "x.pck") and not os.path.exists(os.path.join(root, "landmarks_detected"))


def test_the_binary_is_called_with_the_references_arguments(tmp_path):
    from confignet_amd import dataset_utils as D
    fake = tmp_path / "FaceLandmarkImg"
    fake.write_text("#!/bin/sh\nprintf '%s\\n' \"$@\" > \"$(dirname \"$0\")/args.txt\"\n")
    fake.chmod(0o755)
    photos = tmp_path / "photos"
    photos.mkdir()
    D.run_openface_on_dir(str(photos), str(fake))
    out = str(photos / "processed")
    assert (tmp_path / "args.txt").read_text().split("\n")[:-1] == ["-fdir", str(photos), "-wild", "-out_dir", out, "-2Dfp", "-3Dfp", "-pose",
                                                                     "-multi_view 1"]
    assert os.path.exists(photos / "landmarks_detected")
    fake.unlink()
    D.run_openface_on_dir(str(photos), str(fake))                         # the marker is there: nothing runs, nothing raises


def test_public_names():
    import confignet
    import confignet_amd
    from confignet_amd.face_image_normalizer import FaceImageNormalizer
    assert confignet.FaceImageNormalizer is FaceImageNormalizer and confignet_amd.FaceImageNormalizer is FaceImageNormalizer
    assert FaceImageNormalizer.ref_head_center_coords == ((0.5, 0.42),) and FaceImageNormalizer.pre_norm_image_size == 1024
    assert confignet.face_image_normalizer.FaceImageNormalizer is FaceImageNormalizer and confignet.dataset_utils.run_openface_on_dir

"""The CelebA attribute classifier and the controllability metrics on the HIP path: the depthwise 3x3 kernel, the ReLU6 / sigmoid
epilogues on every route MobileNetV2 takes, the image preprocessing kernel and the whole classifier against the float64
statement (tests/mobilenet_ref.py), then ControllabilityMetrics and its wiring into a second-stage training run and the
evaluation command line."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mobilenet_ref as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reference_assets")
DATASET = os.path.join(ASSETS, "test_dataset_res_256.pck")
BEARD_MAP = os.path.join(ASSETS, "beard_style_to_pca_map.json")


def t64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _dw_ref(x, k, b, stride, act):
    """float64 depthwise 3x3 with the TF "same" / correct_pad pads written out"""
    import torch.nn.functional as F
    xc = x.permute(0, 3, 1, 2)

    def pads(e):
        return (1, 1) if stride == 1 else MR._pad_s2(e)
    ph, pw = pads(x.shape[1]), pads(x.shape[2])
    y = F.conv2d(F.pad(xc, (pw[0], pw[1], ph[0], ph[1])), k.permute(2, 3, 0, 1), stride=stride, groups=x.shape[3])
    y = y + b.view(1, -1, 1, 1)
    if act == "relu6":
        y = torch.clamp(y, 0, 6)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("hw", [(7, 9), (33, 17), (128, 128)])
def test_dwconv3x3_against_float64(hw):
    from confignet_amd import ops
    rng = np.random.default_rng(hw[0])
    for c in (3, 13, 32, 96, 144, 384, 960):
        if hw == (128, 128) and c in (96, 384):
            continue
        n = 1 if hw == (128, 128) else 2
        x = rng.normal(size=(n, hw[0], hw[1], c)).astype(np.float32)
        k = rng.normal(size=(3, 3, c, 1)).astype(np.float32)
        b = rng.normal(size=c).astype(np.float32)
        xd, kd, bd = (torch.tensor(a, device="cuda") for a in (x, k, b))
        for stride in (1, 2):
            for act, code in (("none", ops.ACT_NONE), ("relu6", ops.ACT_RELU6)):
                got = ops.dwconv3x3_fwd(xd, kd, bd, stride, code).cpu().double()
                ref = _dw_ref(t64(x), t64(k), t64(b), stride, act)
                assert got.shape == ref.shape == (n, -(-hw[0] // stride), -(-hw[1] // stride), c)
                err = float((got - ref).abs().max())
                assert err <= 1e-5 * float(ref.abs().max()), (hw, c, stride, act, err)
    # no bias
    x = torch.tensor(rng.normal(size=(1, 9, 7, 12)).astype(np.float32), device="cuda")
    k = torch.tensor(rng.normal(size=(3, 3, 12, 1)).astype(np.float32), device="cuda")
    ref = _dw_ref(t64(x), t64(k), torch.zeros(12, dtype=torch.float64), 2, "none")
    assert float((ops.dwconv3x3_fwd(x, k, None, 2).cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def _act64(v, code):
    from confignet_amd import ops
    if code == ops.ACT_RELU6:
        return torch.clamp(v, 0, 6)
    if code == ops.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def test_relu6_and_sigmoid_epilogues_on_the_mobilenet_conv_routes():
    import torch.nn.functional as F
    from confignet_amd import ops
    from confignet_amd.ops import ConvSpec
    rng = np.random.default_rng(7)
    # (name, x shape, k, stride, cout, residual): Conv1, 1x1 expand, 1x1 projection with the residual, Conv_1 at batch 32
    cases = [("conv1", (2, 64, 48, 3), 3, 2, 32, False), ("expand", (2, 32, 32, 24), 1, 1, 144, False),
             ("project_res", (2, 16, 16, 192), 1, 1, 32, True), ("conv_1", (32, 8, 8, 320), 1, 1, 1280, False),
             ("conv_1_small", (2, 1, 1, 320), 1, 1, 1280, False)]
    for name, xs, k, s, cout, res in cases:
        x = rng.normal(size=xs).astype(np.float32)
        w = (rng.normal(size=(k, k, xs[-1], cout)) / np.sqrt(k * k * xs[-1]) * 4).astype(np.float32)
        b = rng.normal(size=cout).astype(np.float32)
        xd, wd, bd = (torch.tensor(a, device="cuda") for a in (x, w, b))
        g = ConvSpec((k, k), stride=s).geom(xs, cout)
        xc = t64(x).permute(0, 3, 1, 2)
        if k == 3:
            ph, pw = MR._pad_s2(xs[1]), MR._pad_s2(xs[2])
            xc = F.pad(xc, (pw[0], pw[1], ph[0], ph[1]))
        pre = (F.conv2d(xc, t64(w).permute(3, 2, 0, 1), stride=s) + t64(b).view(1, -1, 1, 1)).permute(0, 2, 3, 1)
        if res:
            r = rng.normal(size=pre.shape).astype(np.float32)
            got = ops.conv_fwd_res(xd, wd, bd, torch.tensor(r, device="cuda"), g, ops.ACT_NONE).cpu().double()
            ref = pre + t64(r)
            assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), name
        for code in (ops.ACT_RELU6, ops.ACT_SIGMOID):
            got = ops.conv_fwd(xd, wd, bd, g, code).cpu().double()
            ref = _act64(pre, code)
            assert got.shape == ref.shape
            assert float((got - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), (name, code)
            assert 0.0 <= float(got.min()) and float(got.max()) <= 6.0
    # the head GEMM (32 x 1280) (1280 x 38) + bias, sigmoid / none
    a = rng.normal(size=(32, 1280)).astype(np.float32)
    bm = (rng.normal(size=(1280, 38)) / 20).astype(np.float32)
    c = rng.normal(size=38).astype(np.float32)
    pre = t64(a) @ t64(bm) + t64(c)
    for code in (ops.ACT_NONE, ops.ACT_SIGMOID, ops.ACT_RELU6):
        got = ops.gemm(torch.tensor(a, device="cuda"), torch.tensor(bm, device="cuda"), bias=torch.tensor(c, device="cuda"), act=code)
        ref = _act64(pre, code)
        assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), code


def test_image_preprocess_against_float64_bilinear():
    from confignet_amd import ops
    rng = np.random.default_rng(3)
    for src, dst in (((37, 29), (64, 64)), ((256, 256), (96, 80)), ((50, 40), (50, 40)), ((128, 128), (64, 64))):
        u8 = rng.integers(0, 256, size=(3,) + src + (3,), dtype=np.uint8)
        got = ops.image_preprocess(torch.tensor(u8, device="cuda"), dst).cpu().double()
        ref = MR.bilinear_half_pixel(t64(u8), *dst) / 127.5 - 1
        assert got.shape == (3,) + dst + (3,)
        assert float((got - ref).abs().max()) < 1e-5, (src, dst)
        if src == dst:
            assert torch.equal(got.float(), torch.tensor(u8.astype(np.float32) / 127.5 - 1))
        f = rng.uniform(-1, 1, size=(2,) + src + (3,)).astype(np.float32)
        got = ops.image_preprocess(torch.tensor(f, device="cuda"), dst, from_signed=True).cpu().double()
        ref = MR.bilinear_half_pixel((t64(f) + 1) * 127.5, *dst) / 127.5 - 1
        assert float((got - ref).abs().max()) < 1e-5, (src, dst)


def _randomized_classifier(input_shape, attrs=None, seed=0):
    from confignet_amd.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["input_shape"] = tuple(input_shape)
    cfg["predicted_attributes"] = attrs or ["Attr_%02d" % i for i in range(38)]
    c = CelebaAttributeClassifier(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    ws = c.classifier.get_weights()
    i = 0
    while i < len(ws) - 2:                        # non-trivial inference statistics of every BatchNormalization
        if ws[i].ndim == 1:                       # gamma, beta, moving_mean, moving_variance
            sh = ws[i].shape
            ws[i:i + 4] = [rng.uniform(0.8, 1.2, sh), rng.normal(size=sh) * 0.1, rng.normal(size=sh) * 0.1, rng.uniform(0.5, 1.5, sh)]
            ws[i:i + 4] = [w.astype(np.float32) for w in ws[i:i + 4]]
            i += 4
        else:
            i += 1
    ws[-1] = (rng.normal(size=ws[-1].shape) * 0.1).astype(np.float32)
    c.classifier.set_weights(ws)
    return c, ws


@pytest.mark.parametrize("hw", [(256, 256), (97, 75)])
def test_classifier_against_the_float64_statement(hw):
    from confignet_amd import ops
    c, ws = _randomized_classifier(hw + (3,))
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, size=(2,) + hw + (3,)).astype(np.float32)
    xd = torch.tensor(x, device="cuda")
    probs = c.classifier(xd).cpu().double()
    logits = c.classifier(xd, logits=True).cpu().double()
    rp, rl = MR.classifier_forward([t64(w) for w in ws], t64(x))
    assert probs.shape == (2, 38)
    assert float((probs - rp).norm() / rp.norm()) < 1e-4
    assert float((logits - rl).norm() / rl.norm()) < 1e-4
    assert float(rl.std()) > 0.05                                         # (the check is not on a constant)
    # predict_attributes: uint8 input resized to the network size, batches of 32 over a ragged count
    imgs = rng.integers(0, 256, size=(35, hw[0] + 6, hw[1] - 4, 3), dtype=np.uint8)
    got = c.predict_attributes(imgs)
    assert got.dtype == np.float32 and got.shape == (35, 38)
    for s, e in ((0, 3), (30, 35)):
        direct = c.classifier(ops.image_preprocess(torch.tensor(imgs[s:e], device="cuda"), hw)).cpu().numpy()
        np.testing.assert_allclose(got[s:e], direct, rtol=1e-5, atol=1e-6)
    # float32 input is taken as [-1, 1]
    fl = imgs[:4].astype(np.float32) / 127.5 - 1
    np.testing.assert_allclose(c.predict_attributes(fl), got[:4], rtol=1e-4, atol=1e-5)


def _fixture_attributes():
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    d = NeuralRendererDataset.load(DATASET)
    return sorted(a for a in d.attributes[0].keys() if a not in ("Wearing_Necklace", "Wearing_Necktie"))


def _blendshape_names():
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    d = NeuralRendererDataset.load(DATASET)
    d.process_metadata(copy.deepcopy(DEFAULT_CONFIG))
    return d.metadata_input_labels["blendshape_values"]


def _small_confignet(seed=0):
    from confignet_amd import ConfigNet, SyntheticFaceDataset
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    ds = SyntheticFaceDataset(24, 128, seed=1)
    ds.metadata_input_labels = {"blendshape_values": _blendshape_names()}
    cfg = merge_configs(DEFAULT_CONFIG, {"batch_size": 4, "output_shape": (128, 128, 3), "metrics_checkpoint_period": 2,
                                         "image_checkpoint_period": 2})
    ds.process_metadata(cfg, True)
    np.random.seed(seed)
    return ConfigNet(cfg, seed=seed), ds


def test_controllability_metrics_end_to_end_on_a_small_confignet(tmp_path):
    from confignet_amd.metrics import ControllabilityMetrics
    from confignet_amd.metrics.controllability import CONFIGS
    m, ds = _small_confignet()
    m.setup_training(None, ds, 4, real_training_set=ds)
    clf, _ = _randomized_classifier((64, 64, 3), _fixture_attributes())
    cm = ControllabilityMetrics(m, clf, blendshape_names=ds.metadata_input_labels["blendshape_values"], beard_style_map=BEARD_MAP)
    imgs = np.asarray(ds.imgs[:5])
    lat, rot = m.encode_images(imgs)
    for name, cfg in cm.configs.items():                      # the splice touches the config's slice only
        mod = cm._modified_latents(cfg, lat)
        idx = list(m.get_facemodel_param_idxs_in_latent(cfg.facemodel_param_name))
        rest = [i for i in range(lat.shape[1]) if i not in idx]
        assert np.array_equal(mod[:, rest], lat[:, rest])
        assert np.all(mod[:, idx] == mod[:1, idx]) and not np.array_equal(mod[:, idx], lat[:, idx])
    metrics = cm.get_metrics(imgs, img_output_dir=str(tmp_path / "imgs"))
    assert list(metrics) == sorted(CONFIGS) + ["contr_attribute_means", "controllability"]
    for key in CONFIGS:
        assert len(metrics[key]) == 4 and all(np.isfinite(metrics[key]))
    assert np.isfinite(metrics["controllability"]) and len(metrics["contr_attribute_means"]) == 4
    assert len(os.listdir(tmp_path / "imgs")) >= 5 * 18
    # the per-image fine-tuning path
    cm.per_image_tuning_iters = 1
    raw, with_a, without_a = cm.generate_images_for_metric(imgs[:2])
    assert raw.shape == (2, 128, 128, 3) and raw.dtype == np.uint8
    assert all(with_a[k].shape == (2, 128, 128, 3) and without_a[k].shape == (2, 128, 128, 3) for k in CONFIGS)
    tuned = cm.get_metrics_from_attribute_images(with_a, without_a)
    assert np.isfinite(tuned["controllability"])


def test_training_run_writes_controllability_metrics(tmp_path):
    clf, _ = _randomized_classifier((64, 64, 3), _fixture_attributes())
    clf.save(str(tmp_path), "classifier")
    path = str(tmp_path / "classifier.json")
    m, ds = _small_confignet()
    m.config["beard_style_map_path"] = BEARD_MAP
    out = str(tmp_path / "run")
    m.train(ds, ds, ds, path, out, os.path.join(out, "log"), n_steps=3, n_samples_for_metrics=6)
    with open(os.path.join(out, "controllability_metrics.json")) as fp:
        logged = json.load(fp)
    assert "controllability" in logged and "mustache_config" in logged
    assert all(len(v) == 2 for v in logged.values())
    assert len(m.metrics["controllability"]) == 2 and len(m.metrics["perceptual_loss"]) == 2
    # the same run without a classifier: no file, the metric keys of today
    m2, ds2 = _small_confignet()
    out2 = str(tmp_path / "run2")
    m2.train(ds2, ds2, ds2, "none", out2, os.path.join(out2, "log"), n_steps=3, n_samples_for_metrics=6)
    assert not os.path.exists(os.path.join(out2, "controllability_metrics.json"))
    assert m2.controllability_metrics is None
    assert set(m2.metrics) == {"training_step_number", "kid", "fid", "perceptual_loss"}


def test_evaluation_command_line_writes_json_and_csv(tmp_path):
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    m, ds = _small_confignet()
    m.setup_training(None, ds, 2, real_training_set=ds)
    m.save(str(tmp_path), "model")
    clf, _ = _randomized_classifier((64, 64, 3), _fixture_attributes())
    clf.save(str(tmp_path), "classifier")
    test_set = NeuralRendererDataset(img_shape=(128, 128, 3))
    imgs = np.asarray(ds.imgs[:3])
    imgs.tofile(str(tmp_path / "test_imgs.dat"))
    test_set.imgs_memmap_filename, test_set.imgs_memmap_shape, test_set.imgs_memmap_dtype = "test_imgs.dat", imgs.shape, "uint8"
    test_set.save(str(tmp_path / "test.pck"))
    out = str(tmp_path / "eval")
    cmd = [sys.executable, os.path.join(ROOT, "evaluation", "evaluate_confignet_controllability.py"),
           "--model_path", str(tmp_path / "model.json"), "--attribute_classifier_path", str(tmp_path / "classifier.json"),
           "--test_set_path", str(tmp_path / "test.pck"), "--output_dir", out, "--synth_data_path", DATASET, "--n_samples", "3"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    name = "contr_metrics_tuning_iters_0_model"
    with open(os.path.join(out, name + ".json")) as fp:
        metrics = json.load(fp)
    assert "controllability" in metrics and "mustache_config" not in metrics and len(metrics["evaluated_configs"]) == 7
    csv = np.loadtxt(os.path.join(out, name + ".csv"), delimiter=",")
    assert csv.shape == (4, 8) and np.isfinite(csv).all()                # the 7 configurations and their means, as the reference

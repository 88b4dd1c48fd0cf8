"""CPU checks of the controllability metrics and the CelebA attribute classifier (no device work): the Keras weight list, the
reference's save / load format, the metric arithmetic on hand-made probabilities, the configuration table resolved against
the fixture dataset and the beard-style map, and the command lines."""
import copy
import json
import os
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reference_assets")
DATASET = os.path.join(ASSETS, "test_dataset_res_256.pck")
BEARD_MAP = os.path.join(ASSETS, "beard_style_to_pca_map.json")


def _fixture_attributes():
    """what train_attribute_classifier.py chooses from the dataset: its CelebA names minus the two ignored ones, sorted"""
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    d = NeuralRendererDataset.load(DATASET)
    return sorted(a for a in d.attributes[0].keys() if a not in ("Wearing_Necklace", "Wearing_Necktie"))


def _classifier(attrs=None, seed=0):
    from confignet_amd.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["input_shape"] = (256, 256, 3)
    cfg["predicted_attributes"] = attrs or _fixture_attributes()
    return CelebaAttributeClassifier(cfg, seed=seed)


def _blendshape_names():
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.neural_renderer_dataset import NeuralRendererDataset
    d = NeuralRendererDataset.load(DATASET)
    d.process_metadata(copy.deepcopy(DEFAULT_CONFIG))
    return d.metadata_input_labels["blendshape_values"]


def test_keras_weight_list_of_the_classifier():
    from tests import mobilenet_ref as MR
    attrs = _fixture_attributes()
    assert len(attrs) == 38
    net = _classifier(attrs).classifier
    ws = net.get_weights()
    assert len(ws) == 260 + 6
    assert sum(w.size for w in ws[:260]) == 2257984                                   # MobileNetV2 (alpha 1, no top)
    assert [w.shape for w in ws[260:]] == [(1280,)] * 4 + [(1280, 38), (38,)]
    assert [w.shape for w in ws] == MR.weight_shapes(38)
    assert net.count_params() == 2257984 + 4 * 1280 + 1280 * 38 + 38


def test_save_load_round_trip_is_bit_exact(tmp_path):
    from confignet_amd.metrics import CelebaAttributeClassifier
    c = _classifier(seed=3)
    rng = np.random.default_rng(0)
    ws = [rng.normal(size=w.shape).astype(np.float32) for w in c.classifier.get_weights()]
    c.classifier.set_weights(ws)
    c.logs = {"loss": [0.5, 0.25]}
    c.save(str(tmp_path), "model")
    with open(tmp_path / "model.json") as fp:
        meta = json.load(fp)
    assert set(meta) == {"logs", "config"} and meta["logs"] == {"loss": [0.5, 0.25]}
    back = CelebaAttributeClassifier.load(str(tmp_path / "model.json"))
    assert back.config["predicted_attributes"] == c.config["predicted_attributes"] and back.logs == c.logs
    for a, b in zip(back.classifier.get_weights(), ws):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    # an object array the way the reference's np.save(path, model.get_weights()) leaves it (a list of ragged arrays)
    arr = np.empty(len(ws), dtype=object)
    for i, w in enumerate(ws[::-1]):
        arr[len(ws) - 1 - i] = w
    np.save(str(tmp_path / "ref.npy"), arr, allow_pickle=True)
    with open(tmp_path / "ref.json", "w") as fp:
        json.dump({"logs": {}, "config": dict(c.config, input_shape=list(c.config["input_shape"]))}, fp)
    back = CelebaAttributeClassifier.load(str(tmp_path / "ref.json"))
    assert all(np.array_equal(a, b) for a, b in zip(back.classifier.get_weights(), ws))


class _Cfg:
    def __init__(self, driven, ignored):
        self.driven_attribute, self.ignored_attributes = driven, ignored


def test_metric_arithmetic_on_hand_made_probabilities():
    from confignet_amd.metrics import ControllabilityMetrics
    from confignet_amd.metrics.controllability import CONFIGS
    attrs = ["A", "B", "C", "D", "E"]
    m = ControllabilityMetrics(None, _classifier(attrs), blendshape_names=_blendshape_names(), beard_style_map=BEARD_MAP)
    rng = np.random.default_rng(1)
    s, ns = rng.uniform(size=(7, 5)), rng.uniform(size=(7, 5))
    post, pre, mad, corr = m.get_metrics_for_attribute_pairs(s, ns, _Cfg("B", ["D"]))
    assert post == pytest.approx(s[:, 1].mean()) and pre == pytest.approx(ns[:, 1].mean())
    const = [0, 2, 4]
    assert mad == pytest.approx(np.abs(s[:, const] - ns[:, const]).mean())
    ref = np.corrcoef(np.concatenate([np.ones(7), np.zeros(7)]), np.concatenate([s[:, 1], ns[:, 1]]))[0, 1]
    assert corr == pytest.approx(ref)

    # the full metrics dict from "images": a stub classifier returns a different probability table per image batch
    names = _fixture_attributes()
    m = ControllabilityMetrics(None, _classifier(names), blendshape_names=_blendshape_names(), beard_style_map=BEARD_MAP)
    tables = {}

    def predict(imgs):
        return tables[int(imgs[0, 0, 0, 0])]
    m.attribute_classifier.predict_attributes = predict
    with_a, without_a = {}, {}
    for i, name in enumerate(CONFIGS):
        tables[2 * i], tables[2 * i + 1] = rng.uniform(size=(4, 38)), rng.uniform(size=(4, 38))
        with_a[name] = np.full((4, 8, 8, 3), 2 * i, np.uint8)
        without_a[name] = np.full((4, 8, 8, 3), 2 * i + 1, np.uint8)
    got = m.get_metrics_from_attribute_images(with_a, without_a)
    assert list(got) == sorted(CONFIGS) + ["contr_attribute_means", "controllability"]
    per = []
    for i, (name, cfg) in enumerate(CONFIGS.items()):
        d = names.index(cfg.driven_attribute)
        const = [j for j, n in enumerate(names) if n not in list(cfg.ignored_attributes) + [cfg.driven_attribute]]
        s, ns = tables[2 * i], tables[2 * i + 1]
        exp = (s[:, d].mean(), ns[:, d].mean(), np.abs(s[:, const] - ns[:, const]).mean(),
               np.corrcoef(np.concatenate([np.ones(4), np.zeros(4)]), np.concatenate([s[:, d], ns[:, d]]))[0, 1])
        assert got[name] == pytest.approx(exp)
        per.append(exp)
    means = np.mean(per, axis=0)
    assert got["contr_attribute_means"] == pytest.approx(tuple(means))
    assert got["controllability"] == pytest.approx(10 * means[2] + (1 - means[0]))


class _StubModel:
    def __init__(self):
        from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
        self.config = copy.deepcopy(DEFAULT_CONFIG)
        self.config["facemodel_inputs"]["blendshape_values"] = (62, 30)
        self.config["facemodel_inputs"]["beard_style_embedding"] = (9, 7)
        self.config["facemodel_inputs"]["head_hair_color"] = (3, 3)

    def sample_facemodel_params(self, n):
        return [np.full((n, d[0] or 4), 0.5) for d in self.config["facemodel_inputs"].values()]


def test_configurations_resolve_against_the_fixtures():
    from confignet_amd.metrics import ControllabilityMetrics
    names = _blendshape_names()
    assert len(names) == 62
    assert [names.index(k) for k in ("jaw_opening", "mouthSmileLeft", "mouthSmileRight", "EyeBLinkLeft", "EyeBLinkRight")] == [61, 53, 54, 10, 11]
    model = _StubModel()
    m = ControllabilityMetrics(model, _classifier(), blendshape_names=names, beard_style_map=BEARD_MAP)
    fm = list(model.config["facemodel_inputs"])
    bs = fm.index("blendshape_values")
    p = m.get_facemodel_params_for_config(m.configs["smile_config"], False)[bs]
    assert p[0, 53] == 1.0 and p[0, 54] == 1.0 and np.count_nonzero(p) == 2
    p = m.get_facemodel_params_for_config(m.configs["squint_config"], False)[bs]
    assert p[0, 10] == 0.7 and p[0, 11] == 0.7 and np.count_nonzero(p) == 2
    p = m.get_facemodel_params_for_config(m.configs["mouth_open_config"], True)[bs]
    assert p[0, 61] == -0.05 and np.count_nonzero(p) == 1
    p = m.get_facemodel_params_for_config(m.configs["gray_hair_config"], False)[fm.index("head_hair_color")]
    assert p.tolist() == [[0.7, 0.7, 0.0]]
    with open(BEARD_MAP) as fp:
        beard = json.load(fp)
    mu = m.configs["mustache_config"]
    assert list(mu.facemodel_param_value) == beard["beard_Wavy_f"] and len(mu.facemodel_param_value) == 9
    assert list(mu.facemodel_param_value_other) == beard["beard_None"]
    p = m.get_facemodel_params_for_config(mu, True)[fm.index("beard_style_embedding")]
    assert np.array_equal(p[0], np.array(beard["beard_None"]))

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        m2 = ControllabilityMetrics(model, _classifier(), blendshape_names=names)
    assert any("mustache_config" in str(w.message) for w in caught)
    assert "mustache_config" not in m2.configs and len(m2.configs) == 7
    with pytest.raises(ValueError):
        ControllabilityMetrics(model, _classifier(), beard_style_map=BEARD_MAP)      # blendshape configs need the names


def test_reference_style_imports_and_dataset_attributes():
    import confignet
    from confignet.metrics.celeba_attribute_prediction import DEFAULT_CONFIG, CelebaAttributeClassifier
    from confignet.metrics.controllability_metric_configs import ControllabilityMetricConfigs
    assert confignet.CelebaAttributeClassifier is CelebaAttributeClassifier and DEFAULT_CONFIG["batch_size"] == 32
    assert [n for n, _ in ControllabilityMetricConfigs.all_configs()] == sorted(n for n, _ in ControllabilityMetricConfigs.all_configs())
    assert confignet.ControllabilityMetrics.__name__ == "ControllabilityMetrics"
    d = confignet.NeuralRendererDataset.load(DATASET)
    v = d.get_attribute_values([1, 0, 1], ["Smiling", "Male"])
    assert v.shape == (3, 2) and v[0].tolist() == [d.attributes[1]["Smiling"], d.attributes[1]["Male"]]


def test_command_lines_parse():
    import sys
    import train_confignet
    sys.path.insert(0, os.path.join(ROOT, "evaluation"))
    import evaluate_confignet_controllability as E
    args = E.build_parser().parse_args(["--model_path", "m.json", "--test_set_path", "t.pck", "--output_dir", "o",
                                        "--attribute_classifier_path", "c.json", "--synth_data_path", "s.pck",
                                        "--beard_style_map_path", "b.json", "--n_fine_tuning_iters", "3", "--n_samples", "5",
                                        "--write_images"])
    assert (args.n_fine_tuning_iters, args.n_samples, args.write_images, args.beard_style_map_path) == (3, 5, True, "b.json")
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--model_path", "m.json", "--test_set_path", "t.pck", "--output_dir", "o"])
    import argparse
    ap = argparse.ArgumentParser()
    for flag, kw in train_confignet.FLAGS:
        ap.add_argument(flag, **kw)
    a = ap.parse_args(["--output_dir", "o", "--attribute_classifier_path", "c.json", "--beard_style_map_path", "b.json"])
    assert a.attribute_classifier_path == "c.json" and a.beard_style_map_path == "b.json"
    assert "ignored" not in train_confignet.__doc__

"""ControllabilityMetrics (reference: confignet/metrics/metrics.py:15-199 and controllability_metric_configs.py): how well a
ConfigNet drives one face attribute (hair colour, mouth, smile, squint, mustache) through its face-model inputs, measured by
the CelebA attribute classifier on images generated with the attribute set and with a contrasting value (ConfigNet paper,
Table 2).

Per configuration the result is the tuple (post, pre, MAD, corr): the classifier's mean probability of the driven attribute
with the value set / with the contrasting value, the mean absolute change of the attributes that should stay constant, and
the correlation coefficient between set / not set and the driven attribute's probability.  `contr_attribute_means` averages
the tuples over the configurations that ran; `controllability = 10 * means[2] + (1 - means[0])`.

The data behind the configurations is looked up at run time instead of being written into this module: the blendshape
names come from the synthetic dataset (`metadata_input_labels["blendshape_values"]`), the beard-style embeddings of the
mustache configuration from the beard-style -> PCA map of the synthetic data's assets (by key), the attribute names from the
classifier's config."""
import dataclasses
import json
import os
import warnings

import numpy as np

from .celeba_attribute_prediction import CelebaAttributeClassifier


@dataclasses.dataclass(frozen=True)
class ControllableAttributeConfig:
    driven_attribute: str                    # the classifier attribute that should follow the face-model input
    ignored_attributes: tuple                # attributes allowed to change with it
    facemodel_param_name: str
    facemodel_param_value: object            # tuple: the whole input; dict: blendshape name -> value; str: beard-style key
    facemodel_param_value_other: object      # the contrasting value, same kinds


# The eight configurations, keyed and iterated in name order (the order of the JSON keys).
CONFIGS = {
    "black_hair_config": ControllableAttributeConfig(
        "Black_Hair", ("Blond_Hair", "Brown_Hair", "Gray_Hair"), "head_hair_color", (0, 1, 0), (0, 0.1, 0.1)),
    "blond_hair_config": ControllableAttributeConfig(
        "Blond_Hair", ("Black_Hair", "Brown_Hair", "Gray_Hair"), "head_hair_color", (0, 0.1, 0.1), (0, 1, 0)),
    "brown_hair_config": ControllableAttributeConfig(
        "Brown_Hair", ("Blond_Hair", "Black_Hair", "Gray_Hair"), "head_hair_color", (0, 0.6, 0.5), (0, 0.1, 0.1)),
    "gray_hair_config": ControllableAttributeConfig(
        "Gray_Hair", ("Blond_Hair", "Brown_Hair", "Black_Hair"), "head_hair_color", (0.7, 0.7, 0), (0.0, 0.7, 0)),
    "mouth_open_config": ControllableAttributeConfig(
        "Mouth_Slightly_Open", ("Narrow_Eyes", "Smiling"), "blendshape_values", {"jaw_opening": 0.2}, {"jaw_opening": -0.05}),
    "mustache_config": ControllableAttributeConfig(
        "Mustache", ("No_Beard", "Goatee", "Sideburns"), "beard_style_embedding", "beard_Wavy_f", "beard_None"),
    "smile_config": ControllableAttributeConfig(
        "Smiling", ("Narrow_Eyes", "Mouth_Slightly_Open"), "blendshape_values", {"mouthSmileLeft": 1.0, "mouthSmileRight": 1.0},
        {"mouthFrownLeft": 1.0, "mouthFrownRight": 1.0}),
    "squint_config": ControllableAttributeConfig(
        "Narrow_Eyes", ("Smiling", "Mouth_Slightly_Open"), "blendshape_values", {"EyeBLinkLeft": 0.7, "EyeBLinkRight": 0.7},
        {"EyeWideLeft": 1.0, "EyeWideRight": 1.0}),
}
assert list(CONFIGS) == sorted(CONFIGS)


class ControllabilityMetricConfigs:
    """The reference's access point to the table: all_configs() -> [(name, config)] in name order."""

    @staticmethod
    def all_configs():
        return list(CONFIGS.items())


def load_beard_style_map(beard_style_map):
    """A beard-style -> PCA embedding map given as a dict or as the path of its JSON file."""
    if beard_style_map is None or isinstance(beard_style_map, dict):
        return beard_style_map
    with open(beard_style_map) as fp:
        return json.load(fp)


class ControllabilityMetrics:
    def __init__(self, confinet_model, attribute_classifier, per_image_tuning_iters=0, blendshape_names=None, beard_style_map=None):
        self.confinet_model = confinet_model
        if isinstance(attribute_classifier, CelebaAttributeClassifier):
            self.attribute_classifier = attribute_classifier
        else:
            self.attribute_classifier = CelebaAttributeClassifier.load(attribute_classifier)
        self.per_image_tuning_iters = per_image_tuning_iters
        self.blendshape_names = None if blendshape_names is None else list(blendshape_names)
        self.beard_style_map = load_beard_style_map(beard_style_map)
        if confinet_model is not None:
            self.facemodel_param_names = list(self.confinet_model.config["facemodel_inputs"].keys())
        self.configs = self._resolve_configs()

    def _resolve_configs(self):
        """CONFIGS with the beard-style keys replaced by their embeddings; without a beard-style map the mustache
        configuration is left out (with a warning).  Blendshape names are checked here, looked up per use."""
        out = {}
        for name, cfg in CONFIGS.items():
            if cfg.facemodel_param_name == "beard_style_embedding":
                if self.beard_style_map is None:
                    warnings.warn("ControllabilityMetrics: no beard_style_map given -- %s is skipped; the means and "
                                  "`controllability` are over the other configurations" % name)
                    continue
                cfg = dataclasses.replace(cfg, facemodel_param_value=self._beard_value(cfg.facemodel_param_value),
                                          facemodel_param_value_other=self._beard_value(cfg.facemodel_param_value_other))
            elif isinstance(cfg.facemodel_param_value, dict):
                if self.blendshape_names is None:
                    raise ValueError("ControllabilityMetrics: %s sets blendshapes by name; pass blendshape_names= (the synthetic "
                                     "dataset's metadata_input_labels['blendshape_values'])" % name)
                missing = [k for k in list(cfg.facemodel_param_value) + list(cfg.facemodel_param_value_other)
                           if k not in self.blendshape_names]
                if missing:
                    raise ValueError("ControllabilityMetrics: blendshapes %s of %s are not in blendshape_names" % (missing, name))
            out[name] = cfg
        return out

    def _beard_value(self, key):
        if key not in self.beard_style_map:
            raise ValueError("ControllabilityMetrics: beard style %r is not in the beard_style_map" % key)
        return tuple(float(v) for v in self.beard_style_map[key])

    def get_facemodel_params_for_config(self, attribute_config, other_param):
        facemodel_params = self.confinet_model.sample_facemodel_params(1)
        param_value = attribute_config.facemodel_param_value_other if other_param else attribute_config.facemodel_param_value
        param_idx = self.facemodel_param_names.index(attribute_config.facemodel_param_name)
        if isinstance(param_value, dict):
            if attribute_config.facemodel_param_name != "blendshape_values":
                raise NotImplementedError
            facemodel_params[param_idx][:] = 0
            for key, value in param_value.items():
                facemodel_params[param_idx][:, self.blendshape_names.index(key)] = value
        else:
            facemodel_params[param_idx][:] = param_value
        return facemodel_params

    def _modified_latents(self, attribute_config, latent_vectors, other_param=False):
        """latent_vectors with the slice of the config's face-model input replaced by the synthetic encoder's embedding of the
        set (other_param: the contrasting) value"""
        facemodel_params = self.get_facemodel_params_for_config(attribute_config, other_param)
        latent_with_attribute = self.confinet_model.synthetic_encoder.predict(facemodel_params)
        idxs = list(self.confinet_model.get_facemodel_param_idxs_in_latent(attribute_config.facemodel_param_name))
        modified = np.copy(latent_vectors)
        modified[:, idxs] = latent_with_attribute[0, idxs]
        return modified

    def get_images_for_controllable_attribute(self, attribute_config, latent_vectors, rotations, other_param=False):
        return self.confinet_model.generate_images(self._modified_latents(attribute_config, latent_vectors, other_param), rotations)

    def _generate_attribute_images(self, latent_vectors, rotations):
        """The 2 x len(configs) generator passes of one set of latents as ONE generate_images call: (with, without) dicts"""
        n = len(latent_vectors)
        latents, rots = [], []
        for name, cfg in self.configs.items():
            for other in (False, True):
                latents.append(self._modified_latents(cfg, latent_vectors, other))
                rots.append(rotations)
        imgs = self.confinet_model.generate_images(np.concatenate(latents), np.concatenate(rots))
        with_attr, without_attr = {}, {}
        for i, name in enumerate(self.configs):
            with_attr[name] = imgs[(2 * i) * n:(2 * i + 1) * n]
            without_attr[name] = imgs[(2 * i + 1) * n:(2 * i + 2) * n]
        return with_attr, without_attr

    def generate_images_for_metric(self, input_images):
        if self.per_image_tuning_iters > 0:
            raw_decoded_images = []
            images_with_attributes = {name: [] for name in self.configs}
            images_without_attributes = {name: [] for name in self.configs}
            for img in input_images:
                latent_vectors, rotations = self.confinet_model.fine_tune_on_img(img[np.newaxis], n_iters=self.per_image_tuning_iters)
                raw_decoded_images.append(self.confinet_model.generate_images(latent_vectors, rotations)[0])
                with_attr, without_attr = self._generate_attribute_images(latent_vectors, rotations)
                for name in self.configs:
                    images_with_attributes[name].append(with_attr[name][0])
                    images_without_attributes[name].append(without_attr[name][0])
            raw_decoded_images = np.array(raw_decoded_images)
            images_with_attributes = {k: np.array(v) for k, v in images_with_attributes.items()}
            images_without_attributes = {k: np.array(v) for k, v in images_without_attributes.items()}
        else:
            latent_vectors, rotations = self.confinet_model.encode_images(input_images)
            raw_decoded_images = self.confinet_model.generate_images(latent_vectors, rotations)
            images_with_attributes, images_without_attributes = self._generate_attribute_images(latent_vectors, rotations)
        return raw_decoded_images, images_with_attributes, images_without_attributes

    def get_metrics_for_attribute_pairs(self, set_attributes, not_set_attributes, attribute_config):
        """(post, pre, MAD of the constant attributes, corr coef) of one configuration (metrics.py:115-136)"""
        attribute_names = list(self.attribute_classifier.config["predicted_attributes"])
        driven_attribute_idx = attribute_names.index(attribute_config.driven_attribute)
        changing_attribute_names = list(attribute_config.ignored_attributes) + [attribute_config.driven_attribute]
        constant_attribute_idxs = [i for i, n in enumerate(attribute_names) if n not in changing_attribute_names]
        mean_after_setting = np.mean(set_attributes[:, driven_attribute_idx])
        mean_after_setting_other = np.mean(not_set_attributes[:, driven_attribute_idx])
        n_samples = len(set_attributes)
        assert n_samples == len(not_set_attributes)
        attribute_values = np.hstack((np.ones(n_samples), np.zeros(n_samples)))
        predicted_values = np.hstack((set_attributes[:, driven_attribute_idx], not_set_attributes[:, driven_attribute_idx]))
        corr_coef = np.corrcoef(np.vstack((attribute_values, predicted_values)))
        mad = np.mean(np.abs(set_attributes[:, constant_attribute_idxs] - not_set_attributes[:, constant_attribute_idxs]), axis=0)
        mad = np.mean(mad)
        return float(mean_after_setting), float(mean_after_setting_other), float(mad), float(corr_coef[0, 1])

    def get_metrics_for_attribute_config(self, attribute_config, images_with_attribute, images_without_attribute):
        set_attributes = self.attribute_classifier.predict_attributes(images_with_attribute)
        not_set_attributes = self.attribute_classifier.predict_attributes(images_without_attribute)
        return self.get_metrics_for_attribute_pairs(set_attributes, not_set_attributes, attribute_config)

    def get_metrics(self, input_images, img_output_dir=None):
        raw_decoded_images, images_with_attributes, images_without_attributes = self.generate_images_for_metric(input_images)
        if img_output_dir is not None:
            from .. import confignet_utils
            os.makedirs(img_output_dir, exist_ok=True)
            gt = np.asarray(input_images)
            if gt.dtype != np.uint8:
                gt = np.clip((gt + 1.0) * 127.5, 0, 255).astype(np.uint8)
            for i in range(len(input_images)):
                confignet_utils.write_image(os.path.join(img_output_dir, "gt_img_%04d.png" % i), gt[i])
                confignet_utils.write_image(os.path.join(img_output_dir, "raw_img_%04d.png" % i), raw_decoded_images[i])
                for name in self.configs:
                    confignet_utils.write_image(os.path.join(img_output_dir, "%s_img_%04d.png" % (name, i)), images_with_attributes[name][i])
                    confignet_utils.write_image(os.path.join(img_output_dir, "%s_img_not_set_%04d.png" % (name, i)),
                                                images_without_attributes[name][i])
        return self.get_metrics_from_attribute_images(images_with_attributes, images_without_attributes)

    def get_metrics_from_attribute_images(self, images_with_attributes, images_without_attributes):
        """{config name: tuple} in name order, then contr_attribute_means and controllability (metrics.py:168-179); when a
        configuration was left out, `evaluated_configs` lists the ones the means are over."""
        metrics = {}
        for name, cfg in self.configs.items():
            metrics[name] = self.get_metrics_for_attribute_config(cfg, images_with_attributes[name], images_without_attributes[name])
        metrics["contr_attribute_means"] = tuple(float(v) for v in np.mean(list(metrics.values()), axis=0))
        metrics["controllability"] = 10 * metrics["contr_attribute_means"][2] + (1 - metrics["contr_attribute_means"][0])
        if len(self.configs) != len(CONFIGS):
            metrics["evaluated_configs"] = list(self.configs)
        return metrics

    def update_and_log_metrics(self, images, metrics_dict, output_dir, aml_run=None, tb_log_writer=None):
        """metrics.py:181-199 without the TensorBoard sink: appends every value to metrics_dict[key] and rewrites
        <output_dir>/controllability_metrics.json with those keys."""
        os.makedirs(output_dir, exist_ok=True)
        new_metrics = self.get_metrics(images)
        for key, value in new_metrics.items():
            metrics_dict.setdefault(key, []).append(value)
        if aml_run is not None:
            for key, value in new_metrics.items():
                aml_run.log(key, value)
        contr_only = {key: metrics_dict[key] for key in new_metrics}
        with open(os.path.join(output_dir, "controllability_metrics.json"), "w") as fp:
            json.dump(contr_only, fp, indent=4)
        return new_metrics

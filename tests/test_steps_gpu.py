"""GPU parity of WHOLE step functions against the CPU oracle (round-2 additions):

* fine_tune_on_img (confignet_second_stage.py:321-403; BASELINE.json configs[3]) against the committed golden
  tests/golden/fine_tune_128.npz (made by scripts/make_golden.py from oracle/ref_steps.py:fine_tune_on_img), eager and
  HIP-graph dispatch, plus the reference fixture's weight-free fact: after ONE iteration exactly the
  blendshape slice of the returned embedding has moved, by lr = 1e-4, and the rest is the (stale) encoder output.
* one whole second-stage training iteration (confignet_second_stage.py:277-288) dispatched as replayed HIP graphs with
  the concurrent discriminator phase, against oracle/ref_steps.py:second_stage_iteration on the same batches: all four
  loss dicts, the shared optimizer counter (per-step lr_t), every network's post-update weights and the EMA copy.
* the LatentGAN discriminator / generator steps + EMA (latent_gan.py:117-174; configs[4]) against the oracle.
* set_facemodel_param_in_latents values (confignet_first_stage.py:217-239).
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_golden as MG   # noqa: E402

from oracle import ref_nets as R   # noqa: E402
from oracle import ref_ops as O   # noqa: E402
from oracle import ref_steps as S   # noqa: E402

GOLD_FT = np.load(os.path.join(ROOT, "tests", "golden", "fine_tune_128.npz"))


def t64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def w64(net):
    """Keras-ordered float64 copy of a network's weights; BatchNorm moving statistics stay non-trainable."""
    return [torch.tensor(a, dtype=torch.float64, requires_grad=bool(p.requires_grad))
            for a, p in zip(net.get_weights(), net.weights)]


def _fine_tune_model():
    from confignet_amd import ConfigNet
    W, vgg, vggface, inp = MG.build_fine_tune()
    cfg = {"output_shape": (MG.RES, MG.RES, 3), "batch_size": 2, "facemodel_inputs": dict(MG.FM)}
    m = ConfigNet(cfg, seed=0)
    m.config["image_loss_weight"] *= 10                                    # train_confignet.py:67
    assert m.config["image_loss_weight"] == MG.FT_CFG["image_loss_weight"]
    m.generator.set_weights(W["generator"]); m.generator_smoothed.set_weights(W["generator_smoothed"])
    m.discriminator.set_weights(W["discriminator"]); m.synth_discriminator.set_weights(W["synth_discriminator"])
    m.latent_discriminator.set_weights(W["latent_discriminator"]); m.latent_regressor.set_weights(W["latent_regressor"])
    m.synthetic_encoder.set_weights(W["synthetic_encoder"]); m.encoder.set_weights(W["real_encoder"])
    m.perceptual_loss._pretrained_dnn_activations.set_weights(vgg)
    m.perceptual_loss_face_reco._pretrained_dnn_activations.set_weights(vggface)
    assert tuple(m.get_facemodel_param_idxs_in_latent("blendshape_values"))[0] == MG.FT_EXPR[0]
    return m, W, inp


def _check_loss_trajectory(got_steps, ref_steps):
    """Step 0 (identical weights): every scalar within 1e-3 (north_star).  Later steps follow Adam updates of lr*sign(g) on
    8 M generator weights; entries whose gradient is at fp32 noise level may step the other way than in the float64 oracle,
    and these losses move by up to 30 % PER STEP (two runs of the device path differ from each other by as much as either differs
    from the oracle: fp32 atomics), so from step 1 on the allowance also carries 10 % of the oracle's own accumulated step-to-step
    change of that scalar.  The sharp checks of the later steps are the embedding / rotation trajectories (steps of 1e-4, compared at
    5e-5) and the per-tensor update norms of the generator copy."""
    path = {k: 0.0 for k in ref_steps[0]}
    for step, (got, ref) in enumerate(zip(got_steps, ref_steps)):
        assert list(got.keys()) == list(ref.keys())
        for k, v in ref.items():
            if step > 0:
                path[k] += abs(v - ref_steps[step - 1][k])
            # steps 0 and 1 are the sharp ones (forward parity, then one lr*sign(g) step); from the second update on the
            # trajectories of the ill-conditioned deep discriminator heads spread from run to run (atomics order decides signs
            # of noise-level gradient entries: 3 of 14 runs exceeded 0.1 of the path length at step 2, none 0.12)
            tol = 1e-3 * max(1.0, abs(v)) + (0.1 if step < 2 else 0.3) * path[k]
            assert abs(got[k] - v) <= tol, ("step %d" % step, k, got[k], v, tol)


@pytest.mark.parametrize("graphs", [False, True])
def test_fine_tune_on_img_matches_oracle_golden(graphs):
    m, W, inp = _fine_tune_model()
    m.use_graphs = graphs
    imgs = inp["ft_imgs"].astype(np.float32)
    m.fine_tune_loss_log = []
    emb, rot = m.fine_tune_on_img(imgs, n_iters=3)
    names = list(GOLD_FT["loss_names"])
    assert list(m.fine_tune_loss_log[0].keys()) == names
    _check_loss_trajectory(m.fine_tune_loss_log, [dict(zip(names, row)) for row in GOLD_FT["loss_values"]])
    # three Adam steps of ~1e-4 each: a wrong lr_t / moment / stale tile shifts EVERY entry at the 1e-4 level; a single entry whose
    # gradient changes sign near zero in a later step may take that one step the other way (<= 2e-4)
    err = np.abs(emb - GOLD_FT["emb"]).ravel()
    # (0.9-quantile: 2e-5 .. 3.5e-5 over runs of the default mode, 4.07e-5 -- every time -- in deterministic mode)
    assert np.quantile(err, 0.9) < 5e-5 and err.max() < 2.5e-4, (np.quantile(err, 0.9), err.max())
    assert np.abs(rot - GOLD_FT["rot"]).max() < 1e-4, (rot, GOLD_FT["rot"])
    # the fine-tuned generator copy moved like the oracle's (per-tensor update norms; sign flips of noise-level
    # gradients move single entries by 2 lr)
    got_norms = np.array([float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).norm())
                          for a, b in zip(m.generator_fine_tuned.get_weights(), W["generator_smoothed"])])
    ref = GOLD_FT["gen_delta_norms"]
    sel = ref > 0
    # (measured over 20 runs: typically 1-3 %, one run in ~10 above 5 % on a 64-entry bias -- the atomics' summation order decides
    # the sign of noise-level gradient entries, and a sign step moves such an entry by 2 lr; a wrong lr_t / moment moves every
    # norm by 100 %)
    assert np.all(np.abs(got_norms[sel] - ref[sel]) <= 0.10 * ref[sel] + 1e-6), (got_norms, ref)
    assert float(got_norms[0]) == 0.0 and ref[0] == 0.0             # learned_input kernel: zero gradient, never moves
    # generate_images now decodes with the fine-tuned copy (confignet_second_stage.py:310-319)
    out = m.generate_images(emb, rot)
    assert out.shape == (1, MG.RES, MG.RES, 3) and out.dtype == np.uint8


def test_fine_tune_one_iteration_moves_exactly_the_expression_slice():
    """The reference's confignet_finetune_ref_*.npz fact: after n_iters=1 only the 30 expression
    dims differ from the encoder's embedding, each by lr = 1e-4 (first Adam step = lr*sign(g)); pre/post are returned
    as tiled BEFORE the step (confignet_second_stage.py:363-364,402); the rotations move by 1e-4."""
    m, W, inp = _fine_tune_model()
    imgs = inp["ft_imgs"].astype(np.float32)
    emb0, rot0 = m.encode_images(imgs)
    emb, rot = m.fine_tune_on_img(imgs, n_iters=1)
    d = (emb.astype(np.float64) - emb0.astype(np.float64))[0]
    lo, hi = MG.FT_EXPR
    # (the encoder's global average pool sums with fp32 atomics: two runs of encode agree to the last bits, not bitwise)
    rest = np.r_[0:lo, hi:d.shape[0]]
    assert np.abs(d[rest]).max() < 1e-6, d[rest]
    assert np.all(np.abs(np.abs(d[lo:hi]) - 1e-4) < 2e-6), d[lo:hi]
    assert np.abs(emb - GOLD_FT["emb_1iter"]).max() < 1e-3 and np.abs(emb0 - GOLD_FT["emb_encoder"]).max() < 1e-3
    assert np.array_equal(np.sign(d[lo:hi]), np.sign((GOLD_FT["emb_1iter"] - GOLD_FT["emb_encoder"])[0, lo:hi]))
    dr = (rot.astype(np.float64) - rot0.astype(np.float64))[0]
    assert np.all(np.abs(np.abs(dr) - 1e-4) < 2e-6), dr
    assert np.abs(rot - GOLD_FT["rot_1iter"]).max() < 1e-4


def test_fine_tune_force_neutral_expression_keeps_the_expression_slice_fixed():
    """force_neutral_expression=True (confignet_second_stage.py:328-331,393-394): the expression latents are replaced by
    the synthetic encoder's output for all-zero blendshapes and left out of the trainable list."""
    m, W, inp = _fine_tune_model()
    imgs = inp["ft_imgs"].astype(np.float32)
    lo, hi = MG.FT_EXPR
    neutral = O.mlp_simple(torch.zeros(1, 62, dtype=torch.float64), [t64(w) for w in W["synthetic_encoder"][4:8]], 0.3)
    Wt = {k: [t64(w) for w in v] for k, v in W.items()}
    vgg = [t64(w) for w in m.perceptual_loss._pretrained_dnn_activations.get_weights()]
    vggface = [t64(w) for w in m.perceptual_loss_face_reco._pretrained_dnn_activations.get_weights()]
    emb_r, rot_r, hist, _ = S.fine_tune_on_img(Wt, MG.FT_CFG, t64(imgs), 2, vgg, vggface, MG.FT_EXPR,
                                               force_neutral_expression=True, neutral_expr_latents=neutral)
    m.fine_tune_loss_log = []
    emb, rot = m.fine_tune_on_img(imgs, n_iters=2, force_neutral_expression=True)
    assert np.abs(emb[:, lo:hi] - neutral.numpy()).max() < 1e-5           # untouched by the optimizer
    err = np.abs(emb - emb_r.numpy()).ravel()
    assert np.quantile(err, 0.9) < 4e-5 and err.max() < 2.5e-4 and np.abs(rot - rot_r.numpy()).max() < 1e-4
    _check_loss_trajectory(m.fine_tune_loss_log, hist)


def test_fine_tune_at_the_stated_size_runs_200_steps_and_starts_on_the_oracle(monkeypatch):
    """BASELINE.json configs[3] at its stated size (reference confignet_second_stage.py:321-403): one 256 x 256 image, 200 steps,
    replayed step graph.  The first step (identical weights) must agree with the float64 oracle at 256 x 256 in every loss scalar
    to 1e-3 and in the embedding / rotation after that step; the 200-step run must stay finite, keep moving exactly the
    trainable slices, and bring the objective down (the optimizer minimises loss_sum over the embedding, the rotation and the
    generator copy: a wrong sign / stale graph input / lr_t shows up as a flat or rising curve)."""
    monkeypatch.setattr(MG, "RES", 256)
    m, W, inp = _fine_tune_model()
    imgs = inp["ft_imgs"].astype(np.float32)
    assert imgs.shape == (1, 256, 256, 3)
    cfg = dict(MG.FT_CFG, output_shape=(256, 256, 3))
    Wt = {k: [t64(w) for w in v] for k, v in W.items()}
    vgg = [t64(w) for w in m.perceptual_loss._pretrained_dnn_activations.get_weights()]
    vggface = [t64(w) for w in m.perceptual_loss_face_reco._pretrained_dnn_activations.get_weights()]
    emb_r, rot_r, hist, _ = S.fine_tune_on_img(Wt, cfg, t64(imgs), 1, vgg, vggface, MG.FT_EXPR)
    m.use_graphs = True
    m.fine_tune_loss_log = []
    emb0, rot0 = m.encode_images(imgs)
    emb, rot = m.fine_tune_on_img(imgs, n_iters=200)
    log = m.fine_tune_loss_log
    assert len(log) == 200 and list(log[0].keys()) == list(hist[0].keys())
    for k, v in hist[0].items():
        assert abs(log[0][k] - v) <= 1e-3 * max(1.0, abs(v)), ("step 0", k, log[0][k], v)
    vals = np.array([[d[k] for k in log[0].keys()] for d in log])
    assert np.isfinite(vals).all() and np.isfinite(emb).all() and np.isfinite(rot).all()
    total = vals[:, list(log[0].keys()).index("loss_sum")]
    print("fine-tune 256^2: loss_sum first %.4f, mean of steps 0-9 %.4f, 95-104 %.4f, 190-199 %.4f" %
          (total[0], total[:10].mean(), total[95:105].mean(), total[190:].mean()))
    assert total[190:].mean() < total[:10].mean() and total[95:105].mean() < total[:10].mean()
    # every embedding entry and rotation is a variable of the loop (l.340-352): none can move further than 200 Adam steps of
    # lr = 1e-4 (|step| <= lr up to the bias correction), and the loop must have moved them
    d = np.abs(emb.astype(np.float64) - emb0.astype(np.float64))[0]
    assert 2e-4 < d.max() <= 200 * 1e-4 * 1.05, d.max()
    assert np.abs(rot - rot0).max() <= 200 * 1e-4 * 1.05
    # a second call of ONE step from the same state reproduces the oracle's first step
    emb1, rot1 = m.fine_tune_on_img(imgs, n_iters=1)
    err = np.abs(emb1 - emb_r.numpy()).ravel()
    assert np.quantile(err, 0.9) < 5e-5 and err.max() < 2.5e-4 and np.abs(rot1 - rot_r.numpy()).max() < 1e-4, (err.max(), rot1, rot_r)


# ------------------------------------------------------------------------------------------------------------
def _oracle_batch(m, real_set, synth_set, dtype=torch.float64, staged=None):
    """The batches of one iteration, rebuilt on the host from the indices / flags / parameters the step functions
    staged (confignet_amd/graphs.py:StaticBuffers) -- independent of the device gather kernel.  staged: key -> host array
    (one entry per key of StaticBuffers.log); default: what the device buffers hold now (the LAST iteration when the
    cross-iteration overlap is off)."""
    B = staged if staged is not None else {k: v.detach().cpu().numpy() for k, v in m._bufs.bufs.items()}
    names = list(m.config["facemodel_inputs"].keys())

    def imgs(ds, idx, flip=None):
        x = ds.imgs[idx].astype(np.float64) / 127.5 - 1.0
        if flip is not None:
            for i, f in enumerate(flip):
                if f:
                    x[i] = x[i, :, ::-1]
        return torch.tensor(x, dtype=dtype)

    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    return {
        "real_d": imgs(real_set, B["d/real_idx"], B["d/real_flip"]), "enc_in_d": imgs(real_set, B["d/enc_idx"]),
        "real_sd": imgs(synth_set, B["sd/real_idx"], B["sd/real_flip"]),
        "params_sd": [t(B["sd/p/" + n]) for n in names], "rot_sd": t(B["sd/rot"]),
        "real_ld": imgs(real_set, B["ld/real_idx"], B["ld/real_flip"]), "params_ld": [t(B["ld/p/" + n]) for n in names],
        "params_g": [t(B["g/p/" + n]) for n in names], "rot_g": t(B["g/rot"]),
        "synth_imgs_g": imgs(synth_set, B["g/synth_idx"]), "eye_masks_g": torch.as_tensor(synth_set.eye_masks[B["g/synth_idx"]]),
        "real_imgs_g": imgs(real_set, B["g/real_idx"], B["g/real_flip"]),
    }


NET_NAMES = ("generator", "latent_regressor", "synthetic_encoder", "real_encoder", "discriminator", "synth_discriminator",
             "latent_discriminator", "generator_smoothed")


def _nets_by_name(m):
    return dict(zip(NET_NAMES, (m.generator, m.latent_regressor, m.synthetic_encoder, m.encoder, m.discriminator,
                                m.synth_discriminator, m.latent_discriminator, m.generator_smoothed)))


@pytest.mark.parametrize("overlap,n_iters", [(False, 1), (True, 2)])
def test_whole_second_stage_iteration_under_graph_dispatch_matches_oracle(overlap, n_iters):
    """overlap=True, two iterations: THE DISPATCH bench.py AND train() USE (graphs + concurrent discriminator phase + early
    generator forward + the real half of iteration 2's discriminator steps pre-replayed under iteration 1's generator tail, on
    the weights after iteration 1's discriminator phase and the batches drawn at the end of iteration 1), every loss key of
    both iterations (incl. GAN_loss_fake_i of the split steps) and the post-update weights of every network against
    oracle/ref_steps.second_stage_iteration (reference: confignet_second_stage.py:277-288)."""
    from confignet_amd import ConfigNet, SyntheticFaceDataset, optim
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    res, batch = 128, 2
    real_set, synth_set = SyntheticFaceDataset(8, res, seed=5), SyntheticFaceDataset(8, res, seed=6)
    cfg = merge_configs(DEFAULT_CONFIG, {"batch_size": batch, "output_shape": (res, res, 3),
                                         "facemodel_inputs": {k: (None, v[1]) for k, v in MG.FM.items()}})
    cfg["facemodel_inputs"] = {k: v for k, v in cfg["facemodel_inputs"].items() if k in MG.FM}
    synth_set.process_metadata(cfg, True)
    cfg["image_loss_weight"] *= 10
    np.random.seed(3)
    m = ConfigNet(cfg, seed=4)
    assert m.config["latent_dim"] == MG.L
    rng = np.random.default_rng(17)
    for net in m.all_networks():                               # biases / gammas / betas away from their 0/1 init
        ws = net.get_weights()
        net.set_weights([(w + rng.normal(size=w.shape) * 0.05).astype(np.float32) if (w.ndim == 1 and p.requires_grad) else w
                         for w, p in zip(ws, net.weights)])
    gw = m.generator.get_weights()                             # a learned input that is not constant (see make_golden.build_fine_tune)
    gw[1] = (1.0 + 0.5 * rng.standard_normal(32768)).astype(np.float32)
    m.generator.set_weights(gw)
    m.generator_smoothed.copy_weights_from(m.generator)
    m.setup_training(None, synth_set, 0, real_training_set=real_set)
    m.use_graphs = True
    m.overlap_discriminators = overlap
    d_opt, g_opt = optim.Adam(**m.config["optimizer"]), optim.Adam(**m.config["optimizer"])
    nets = m.all_networks()
    by_name = _nets_by_name(m)
    start = [n.get_weights() for n in nets]
    for _ in range(4 if overlap else 3):                       # eager warm-ups, capture (+ first replay), first concurrent replay
        m.training_iteration(real_set, synth_set, d_opt, g_opt)
    torch.cuda.synchronize()
    assert len(m._graphs) == 4 and all(g.graph is not None for g in m._graphs.values())
    if overlap:                                                # the split graphs are in use and a real half is in flight
        assert all(g.early_cut > 0 for g in m._graphs.values() if g.name in ("d", "sd", "g"))
        assert all(g.prelaunched for g in m._graphs.values() if g.name in ("d", "sd"))
        assert m._targets_ahead is not None and "g" in m._prestaged        # ... and the generator step's ground-truth VGG passes
    # back to the initial state: weights, Adam moments and the shared step counters (the captured graphs stay; the real halves
    # pre-replayed by the last warm-up iteration are for other weights and are redone by iteration 1)
    for n, w0 in zip(nets, start):
        n.set_weights(w0)
    for o in (d_opt, g_opt):
        o.iterations = 0
        for mom, var in o._state.values():
            mom.zero_(); var.zero_()
    W = {k: w64(by_name[k]) for k in NET_NAMES}
    W["generator_smoothed"] = [w.detach() for w in W["generator_smoothed"]]
    vgg_w = [t64(w) for w in m.perceptual_loss._pretrained_dnn_activations.get_weights()]

    # ---- the device path: n_iters iterations back to back (weights are read between them; nothing is re-staged) ----
    m._bufs.log = {}
    got, after = [], []
    for it in range(n_iters):
        out = m.training_iteration(real_set, synth_set, d_opt, g_opt)
        if overlap:                                            # iteration it+1's real halves are in flight NOW, next to the tail
            assert all(g.prelaunched for g in m._graphs.values() if g.name in ("d", "sd"))
        got.append([{k: float(v) for k, v in d.items()} for d in out])
        after.append({k: by_name[k].get_weights() for k in NET_NAMES})
        assert d_opt.iterations == 3 * (it + 1) and g_opt.iterations == it + 1   # one shared counter for D, synth-D, latent-D (R10)
    log, m._bufs.log = m._bufs.log, None
    # with the overlap the image-discriminator steps staged once more at the end (the batch of iteration n_iters + 1)
    assert len(log["g/rot"]) == len(log["ld/rot"]) == len(log["d/real_idx"]) == n_iters + (1 if overlap else 0)

    okw = {k: v for k, v in m.config["optimizer"].items() if k != "amsgrad"}
    ro_d, ro_g = O.KerasAdam(**okw), O.KerasAdam(**okw)
    lr = m.config["optimizer"]["lr"]

    margins = []                                               # (observed / bound, which bound, network, iteration, tensor): printed at the end (-s)

    def check_updates(name, it, gl, before, step_len):
        """Post-update weights of iteration `it`.  Iteration 1 (beta_1 = 0, zero moments): |step| = lr*sqrt(1-0.9^t)/sqrt(0.1)
        whatever |g| is, i.e. 1.000 lr for the discriminator (t=1), 1.378 lr for the synthetic-domain discriminator (t=2), 1.646 lr
        for the latent discriminator (t=3) and 1.000 lr for the generator step -- a wrong lr_t slot in the concurrent phase shows
        up as a wrong step length.  Iteration 2: the step depends on both iterations' gradients through the second moment and is
        compared with the oracle's entry by entry.  The direction is compared where the oracle's gradient is significant
        (noise-level gradients may take the other sign in fp32)."""
        for i, (a, w_ref, w0, g) in enumerate(zip(after[it][name], W[name], before[name], gl)):
            step = torch.as_tensor(a).double() - w0
            step_ref = w_ref.detach() - w0
            if g is None:                                       # BatchNorm moving statistics: never trained
                assert float(step.abs().max()) == 0.0 and float(step_ref.abs().max()) == 0.0
                continue
            if float(g.abs().max()) == 0.0:                     # the learned_input kernel: exactly zero gradient
                assert float(step.abs().max()) == 0.0, (name, i)
                continue
            # fp32 LeakyReLU-branch flips against the float64 oracle move single gradient entries by up to ~30 % of the tensor's
            # largest one (tests/test_nets_gpu.py:close_grads): above that the step must agree entry by entry
            sig = g.abs() > 0.3 * g.abs().max()
            # iteration 2: the step is 1.38 lr * g2 / sqrt(0.9 g1^2 + g2^2) -- it inherits iteration 1's fp32-vs-float64 branch
            # decisions through g1 (single entries of g1 differ by ~10 %: measured up to 0.10 lr on the learned input over runs);
            # a wrong lr_t, a missing half of a split gradient or a stale moment moves EVERY significant entry by O(lr)
            tol = 0.02 if it == 0 else 0.25
            margins.append((float((step - step_ref)[sig].abs().max()) / lr / tol, "step", name, it, i))
            assert float((step - step_ref)[sig].abs().max()) < tol * lr, (name, it, i, float((step - step_ref)[sig].abs().max()) / lr)
            if step_len is not None:
                assert abs(float(step[sig].abs().mean()) - step_len * lr) < 0.01 * lr, (name, i, float(step[sig].abs().mean()) / lr, step_len)
            live = g.abs() > 1e-4 * g.abs().max()                # (entries with an exactly-zero true gradient step on fp32 noise)
            # ... and below it all but a few per cent do.  Counted in entries, with a floor of 3: the 64-entry BatchNorm vectors of
            # the encoder's first stage have 1.6 % per entry, and which noise-level entries take the other sign changes from run to
            # run with the order of the filter gradients' atomic adds (six runs: 0 - 1 such entries in those vectors; a second one
            # failed the former 3 % bound about once in a dozen runs of the whole suite)
            n_wrong = int(((step - step_ref)[live].abs() > 0.1 * lr * (1 if it == 0 else 3)).sum())
            allowed = max(3.0, (0.03 if it == 0 else 0.10) * int(live.sum()))
            margins.append((n_wrong / allowed, "wrong", name, it, i))
            assert n_wrong < allowed, (name, it, i, n_wrong, int(live.sum()))

    for it in range(n_iters):
        before = {k: [w.detach().clone() for w in v] for k, v in W.items()}
        grads = {}

        def after_d_phase(Wd, it=it, before=before, grads=grads):
            first = it == 0
            check_updates("discriminator", it, grads["discriminator"], before, 1.0 if first else None)
            check_updates("synth_discriminator", it, grads["synth_discriminator"], before, np.sqrt(1 - 0.9 ** 2) / np.sqrt(0.1) if first else None)
            check_updates("latent_discriminator", it, grads["latent_discriminator"], before, np.sqrt(1 - 0.9 ** 3) / np.sqrt(0.1) if first else None)
            with torch.no_grad():                               # the generator step continues from the device path's discriminators
                for name in ("discriminator", "synth_discriminator", "latent_discriminator"):
                    for w, a in zip(Wd[name], after[it][name]):
                        w.copy_(torch.as_tensor(a).double())

        staged = {k: v[it] for k, v in log.items()}
        ref = S.second_stage_iteration(W, m.config, _oracle_batch(m, real_set, synth_set, staged=staged), ro_d, ro_g, vgg_w,
                                       keep_grads=grads, after_discriminator_phase=after_d_phase)
        for g, r, what in zip(got[it], (ref["d"], ref["synth_d"], ref["latent_d"], ref["g"]), ("D", "synth-D", "latent-D", "G")):
            assert list(g.keys()) == list(r.keys()), what
            for k in g:
                rv = float(r[k].detach())
                assert abs(g[k] - rv) <= 1e-3 * max(1.0, abs(rv)), ("iteration %d" % (it + 1), what, k, g[k], rv)
        cur = 0
        for name in ("generator", "latent_regressor", "synthetic_encoder", "real_encoder"):
            n = len([w for w in W[name] if w.requires_grad])
            gi = iter(grads["g_step"][cur:cur + n])
            check_updates(name, it, [next(gi) if w.requires_grad else None for w in W[name]], before, 1.0 if it == 0 else None)
            cur += n
        # EMA copy of the generator (confignet_first_stage.py:393-400)
        for a, r in zip(after[it]["generator_smoothed"], W["generator_smoothed"]):
            assert float((torch.as_tensor(a).double() - r).abs().max()) < 2e-6
        # the next iteration starts from the device path's weights (lr*sign(g) steps of noise-level gradient entries differ
        # between fp32 and float64; the oracle's Adam moments stay its own)
        with torch.no_grad():
            for name in NET_NAMES:
                for w, a in zip(W[name], after[it][name]):
                    w.copy_(torch.as_tensor(a).double())
    # how close the statistical bounds of check_updates came (pytest -s): observed / bound, largest first
    print("update-check margins (observed / bound):", sorted(margins, reverse=True)[:4])
    loss_m = max(abs(g[k] - float(r[k].detach())) / max(1.0, abs(float(r[k].detach()))) / 1e-3
                 for g, r in zip(got[-1], (ref["d"], ref["synth_d"], ref["latent_d"], ref["g"])) for k in g)
    print("last iteration's loss scalars: largest error / bound = %.3f" % loss_m)


def test_full_size_iteration_in_the_benchmarked_dispatch_matches_cpu_oracle():
    """BASELINE.json configs[1] AT ITS OWN SIZE (256x256, batch 16) in the dispatch bench.py times -- replayed step graphs,
    concurrent discriminator phase, early generator forward, real halves pre-replayed under the previous generator tail --
    against oracle/ref_steps.second_stage_iteration run by oracle/cpu_baseline.py (torch-CPU fp32) on the SAME weights and
    batches: every scalar of the four loss dicts within 1e-3 (north_star).  The size-selected code paths (128x128 / 128x96
    tiles, split-K, XCD-ordered launches, the 256x256 Winograd layers, batched R1 at 24576 rows) are all inside.
    bench.py reports the same comparison as `loss_parity_vs_cpu`."""
    import json
    import subprocess
    sys.path.insert(0, ROOT)
    import bench
    model, real_set, synth_set, d_opt, g_opt, _ = bench.setup(16, 256, 64)
    model.use_graphs = True
    model.overlap_discriminators = True
    for _ in range(4):                                         # eager warm-ups, capture, first concurrent replay (+ prestage)
        model.training_iteration(real_set, synth_set, d_opt, g_opt)
    torch.cuda.synchronize()
    st = bench.dump_parity_state(model, real_set, synth_set, d_opt, g_opt)
    try:
        assert "pre-replayed" in st["dispatch"], st["dispatch"]
        p = subprocess.run([sys.executable, "-m", "oracle.cpu_baseline", "16", "256", st["path"], "--parity-only"],
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        ref = json.loads(p.stdout.strip().splitlines()[-1])["parity_losses"]
    finally:
        os.remove(st["path"])
    cmp = bench.compare_losses(st["losses"], ref, st["dispatch"])
    assert cmp["n_scalars"] == 19 + 19 + 4 + len(st["losses"][3]) and cmp["ok"], cmp


def test_pipelined_loop_at_benchmark_size_stays_finite():
    """60 iterations of the benchmarked dispatch at 256x256, batch 16: every loss scalar, every weight and every gradient finite
    after every iteration.  (Round 4: a filter-gradient kernel that was only wrong under LDS contention -- i.e. only inside this
    loop, where four lines share the chip -- put NaN into a generator filter gradient in about half of such runs, somewhere
    between iteration 3 and 40; the two-iteration oracle comparisons never saw it.  tests/test_ops_gpu.py has the kernel-level
    regression, tests/test_abi_cpu.py the static one.)"""
    sys.path.insert(0, ROOT)
    import bench
    model, real_set, synth_set, d_opt, g_opt, _ = bench.setup(16, 256, 64)
    model.use_graphs = True
    model.overlap_discriminators = True
    outs = []
    for it in range(60):
        outs.append(model.training_iteration(real_set, synth_set, d_opt, g_opt))
    torch.cuda.synchronize()
    for it, out in enumerate(outs):
        for step, d in zip(("d", "synth_d", "latent_d", "g"), out):
            for k, v in d.items():
                assert np.isfinite(float(v)), (it, step, k, float(v))
    for net in model.all_networks():
        assert bool(torch.isfinite(net.arena).all()) and bool(torch.isfinite(net.grad_arena).all())


# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,device_sampling", [(128, False), (4096, False), (4096, True)])
def test_latent_gan_steps_and_ema_match_oracle(bs, device_sampling):
    """bs = 4096: BASELINE.json configs[4] at its own batch size (the skinny-M dense kernels of bs = 128 give way to the MFMA
    tile and its split-K at 4096 rows).  device_sampling: the configuration's fast path (config["device_latent_sampling"]: latents
    from the device generator, embeddings resident on the device) -- the oracle replays the logged draws."""
    from confignet_amd import LatentGAN, optim
    L = 145
    gan = LatentGAN({"latent_dim": L, "batch_size": bs, "device_latent_sampling": device_sampling}, seed=1)
    rng = np.random.default_rng(2)
    for net in (gan.generator, gan.discriminator):
        net.set_weights([(w + rng.normal(size=w.shape) * 0.05).astype(np.float32) if w.ndim == 1 else w for w in net.get_weights()])
    gan.generator_smoothed.copy_weights_from(gan.generator)
    emb = rng.normal(size=(max(500, 2 * bs), L)).astype(np.float32)
    opt = optim.Adam(**gan.config["optimizer"])
    g_w, d_w = w64(gan.generator), w64(gan.discriminator)
    sm = [w.detach().clone() for w in w64(gan.generator_smoothed)]
    ropt = O.KerasAdam(lr=gan.config["optimizer"]["lr"], beta_1=0.0, beta_2=0.9)
    lr = gan.config["optimizer"]["lr"]
    for it in range(2):
        # the step functions draw their batches from np.random in the reference's order (latent_gan.py:119-123,152):
        # replay the same draws for the oracle
        state = np.random.get_state()
        gan.latent_log = [] if device_sampling else None
        d = gan.discriminator_training_step(torch.as_tensor(emb).cuda() if device_sampling else emb, opt)
        g = gan.generator_training_step(opt)
        gan.update_smoothed_weights()
        after = np.random.get_state()
        np.random.set_state(state)
        if device_sampling:
            (z_d, z_g), gan.latent_log = gan.latent_log, None
            assert z_d.shape == (bs, L) and abs(float(z_d.mean())) < 0.02 and abs(float(z_d.std()) - 1.0) < 0.02 and not np.array_equal(z_d, z_g)
        else:
            z_d = np.random.normal(0, 1, (bs, L))
        idx = np.random.randint(0, emb.shape[0], bs)
        if not device_sampling:
            z_g = np.random.normal(0, 1, (bs, L))
        np.random.set_state(after)
        g0, d0 = [w.detach().clone() for w in g_w], [w.detach().clone() for w in d_w]
        rd = S.latent_gan_discriminator_step(g_w, d_w, t64(emb[idx]), t64(z_d), ropt)
        rg = S.latent_gan_generator_step(g_w, d_w, t64(z_g), ropt)
        S.ema_update(sm, g_w)
        for got, ref, what in ((d, rd, "D"), (g, rg, "G")):
            assert list(got.keys()) == list(ref.keys()), what
            for k in got:
                assert abs(float(got[k]) - float(ref[k])) <= 1e-3 * max(1.0, abs(float(ref[k]))), (what, it, k, float(got[k]), float(ref[k]))
    assert opt.iterations == 4 and ropt.t == 4                     # ONE optimizer for both networks (latent_gan.py:237)
    for net, ref in ((gan.generator, g_w), (gan.discriminator, d_w)):
        for a, r in zip(net.get_weights(), ref):
            diff = (torch.as_tensor(a).double() - r.detach()).abs()
            # two Adam steps each; single entries whose gradient is at fp32 noise level may step the other way
            assert float(diff.mean()) < 0.05 * lr and float(diff.max()) <= 8 * lr, (float(diff.mean()) / lr, float(diff.max()) / lr)
    for a, r in zip(gan.generator_smoothed.get_weights(), sm):
        assert float((torch.as_tensor(a).double() - r).abs().max()) < 1e-6
    lat = gan.generate_latents(7)
    assert lat.shape == (7, L) and np.isfinite(lat).all()


def test_set_facemodel_param_in_latents_values():
    """confignet_first_stage.py:217-239: the named input's MLP output replaces its slice of every latent row; all other
    entries are copied."""
    from confignet_amd import ConfigNetFirstStage
    cfg = {"output_shape": (128, 128, 3), "batch_size": 2, "facemodel_inputs": dict(MG.FM)}
    m = ConfigNetFirstStage(cfg, seed=3)
    rng = np.random.default_rng(4)
    m.synthetic_encoder.set_weights([(w + rng.normal(size=w.shape) * 0.1).astype(np.float32) for w in m.synthetic_encoder.get_weights()])
    lat = rng.normal(size=(3, MG.L)).astype(np.float32)
    val = rng.normal(size=62).astype(np.float32)
    out = m.set_facemodel_param_in_latents(lat, "blendshape_values", val)
    ws = [t64(w) for w in m.synthetic_encoder.get_weights()]
    ref = O.mlp_simple(t64(val[None]), ws[4:8], 0.3).numpy()      # second input in sorted order: 4 tensors per input MLP
    idx = list(m.get_facemodel_param_idxs_in_latent("blendshape_values"))
    assert idx == list(range(7, 37))
    assert np.abs(out[:, idx] - ref).max() < 1e-4
    keep = [i for i in range(MG.L) if i not in idx]
    assert np.array_equal(out[:, keep], lat[:, keep]) and out is not lat and np.array_equal(lat, lat.copy())
    # one row per latent also works (the demo passes (n, dim) values, confignet_demo.py:158)
    out2 = m.set_facemodel_param_in_latents(lat, "eye_color", np.eye(8, dtype=np.float32)[:3])
    ref2 = O.mlp_simple(t64(np.eye(8)[:3]), ws[8:12], 0.3).numpy()
    assert np.abs(out2[:, 37:40] - ref2).max() < 1e-4


def test_fit_facemodel_expression_params_to_latent_follows_the_sgd_loop_of_the_reference():
    """confignet_first_stage.py:646-679: plain SGD (lr 0.05) on one (1, 62) variable through the blendshape MLP of the synthetic
    encoder towards a latent's expression slice, clipped to [0, 1] after every step, unused expressions zeroed -- 60 steps against
    the same loop in float64 on the oracle's MLP (every step of the product runs on the HIP kernels; a clip decision on an entry
    within rounding of 0 or 1 would show as a jump: none may)."""
    from confignet_amd import ConfigNetFirstStage
    cfg = {"output_shape": (128, 128, 3), "batch_size": 2, "facemodel_inputs": dict(MG.FM)}
    m = ConfigNetFirstStage(cfg, seed=5)
    rng = np.random.default_rng(6)
    m.synthetic_encoder.set_weights([(w + rng.normal(size=w.shape) * 0.1).astype(np.float32) for w in m.synthetic_encoder.get_weights()])
    lat = rng.normal(size=(2, MG.L)).astype(np.float32)
    unused = [3, 17, 40]
    got = m.fit_facemodel_expression_params_to_latent(lat, unused_expr_idxs=unused, n_iters=60, learning_rate=0.05)
    assert got.shape == (1, 62) and got.min() >= 0.0 and got.max() <= 1.0 and np.all(got[:, unused] == 0.0)
    ws = [t64(w) for w in m.synthetic_encoder.get_weights()][4:8]
    target = t64(lat[:, 7:37])
    v = torch.zeros((1, 62), dtype=torch.float64, requires_grad=True)
    for _ in range(60):
        loss = torch.mean(torch.square(target - O.mlp_simple(v, ws, 0.3)))
        (g,) = torch.autograd.grad(loss, [v])
        with torch.no_grad():
            v -= 0.05 * g
            v.clamp_(0.0, 1.0)
            v[:, unused] = 0.0
    assert float(np.abs(got - v.detach().numpy()).max()) < 1e-4
    assert float(got.max()) > 0.0                       # (the fit moved)


def test_train_scripts_run_on_the_reference_dataset_files(tmp_path):
    """The reference's own smoke tests (tests/training_test.py:13-31): train_confignet.py with the 2-image dataset, 1 + 1
    steps, batch 4; then train_latent_gan.py on the model it wrote."""
    import train_confignet
    import train_latent_gan
    asset = os.path.join(ROOT, "tests", "golden", "reference_assets", "test_dataset_res_256.pck")
    out = str(tmp_path / "run")
    model = train_confignet.parse_args(["--output_dir", out, "--real_training_set_path", asset, "--synth_training_set_path", asset,
                                        "--validation_set_path", asset, "--attribute_classifier_path", "none",
                                        "--batch_size", "4", "--stage_1_training_steps", "1", "--n_samples_for_metrics", "10"])
    assert model.config["latent_dim"] == 145 and tuple(model.config["output_shape"]) == (256, 256, 3)
    assert model.config["facemodel_inputs"]["blendshape_values"][0] == 62
    assert np.isfinite(model.g_losses["loss_sum"]).all() and len(model.g_losses["loss_sum"]) == 1
    for f in ("000000.npz", "000000.json", "000000_facemodel_distr.pck"):
        assert os.path.exists(os.path.join(out, "checkpoints", f)) and os.path.exists(os.path.join(out, "first_stage", "checkpoints", f))
    import confignet
    m2 = confignet.load_confignet(os.path.join(out, "checkpoints", "000000.json"))
    assert type(m2).__name__ == "ConfigNet" and set(m2.facemodel_param_distributions) == set(model.config["facemodel_inputs"])
    gan = train_latent_gan.parse_args(["--confignet_path", os.path.join(out, "checkpoints", "000000.json"), "--training_set_path", asset,
                                       "--output_dir", str(tmp_path / "lg"), "--n_training_steps", "1", "--batch_size", "8"])
    assert os.path.exists(str(tmp_path / "lg" / "checkpoints" / "000000.npz")) and gan.generate_latents(3).shape == (3, 145)


FM_DEMO = OrderedDict(sorted(dict(MG.FM, **{"bone_rotations:left_eye": (3, 2), "hdri_embedding": (50, 20)}).items()))
L_DEMO = sum(v[1] for v in FM_DEMO.values())


def _write_reference_checkpoint(tmp_path, res=128):
    """A checkpoint in the reference's on-disk format made WITHOUT this package's save(): model.npz = np.savez of one object
    array per network holding the Keras get_weights() list (confignet_first_stage.py:129-140,173-180, second stage :35-43),
    shapes from the oracle's Keras-ordered shape lists; model.json = the config dict; model_facemodel_distr.pck."""
    import json
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.neural_renderer_dataset import ExemplarDistribution, OneHotDistribution, dump_pickle
    L = L_DEMO
    lists = {
        "generator_weights": MG.seeded_weights(R.generator_weight_shapes(L, res), 21),
        "generator_smoothed_weights": MG.seeded_weights(R.generator_weight_shapes(L, res), 22),
        "discriminator_weights": MG.seeded_weights(R.discriminator_weight_shapes(res), 23),
        "latent_regressor_weights": MG.seeded_weights(R.latent_regressor_weight_shapes(L, res), 24),
        "synthetic_encoder_weights": MG.seeded_weights(R.synthetic_encoder_weight_shapes(list(FM_DEMO.values())), 25),
        "latent_discriminator_weights": MG.seeded_weights(R.mlp_weight_shapes(4, L, L, 1), 26),
        "synth_discriminator_weights": MG.seeded_weights(R.discriminator_weight_shapes(res), 27),
        "real_encoder_weights": MG.seeded_weights(R.real_encoder_weight_shapes(L), 28, he=True),
    }
    for i, role in enumerate(R.resnet50_weight_roles()):                   # sane BatchNorm statistics
        if role == "var":
            lists["real_encoder_weights"][i] = (1.0 + np.abs(lists["real_encoder_weights"][i])).astype(np.float32)
        elif role == "gamma":
            lists["real_encoder_weights"][i] = (0.5 + lists["real_encoder_weights"][i]).astype(np.float32)
    for k in ("real_encoder_weights",):
        lists[k][-4] *= 0.05
        lists[k][-2] *= 0.05
    arrays = {}
    for k, lst in lists.items():
        a = np.empty(len(lst), dtype=object)
        a[:] = lst
        arrays[k] = a
    np.savez(str(tmp_path / "model.npz"), **arrays)
    cfg = dict(DEFAULT_CONFIG, model_type="ConfigNet", output_shape=[res, res, 3], latent_dim=L,
               facemodel_inputs={k: list(v) for k, v in FM_DEMO.items()})
    with open(str(tmp_path / "model.json"), "w") as fp:
        json.dump(cfg, fp)
    rng = np.random.default_rng(3)
    distr = {}
    for k, (din, _) in FM_DEMO.items():
        distr[k] = OneHotDistribution() if k == "eye_color" else ExemplarDistribution()
        distr[k].fit(np.eye(din, dtype=np.float32) if k == "eye_color" else rng.standard_normal((5, din)).astype(np.float32))
    dump_pickle(distr, str(tmp_path / "model_facemodel_distr.pck"))
    lg = {}
    for k, seed, nout in (("generator_weights", 31, L), ("smoothed_generator_weights", 32, L), ("discriminator_weights", 33, 1)):
        lst = MG.seeded_weights(R.mlp_weight_shapes(3, L, int(L * 1.5), nout), seed)
        a = np.empty(len(lst), dtype=object)
        a[:] = lst
        lg[k] = a
    os.makedirs(str(tmp_path / "lg"))
    np.savez(str(tmp_path / "lg" / "model.npz"), **lg)
    with open(str(tmp_path / "lg" / "model.json"), "w") as fp:
        json.dump({"latent_dim": L, "optimizer": {"lr": 5e-5, "beta_1": 0.0, "beta_2": 0.9, "amsgrad": False}, "batch_size": 32,
                   "num_mlp_layers": 3, "latent_distribution_type": "normal", "hidden_layer_size_multiplier": 1.5,
                   "n_samples_for_metrics": 1000, "verbose_log_period": 500, "logging_img_square_size": 6}, fp)
    return lists, lg


def test_reference_format_checkpoint_loads_and_the_demo_loop_runs(tmp_path):
    """f1 + f3 of SURVEY.md section 8: a model.json / model.npz / _facemodel_distr.pck triple in the reference's layout loads
    through load_confignet (weights land in the right tensors: generate_images / encode_images match the oracle evaluated on
    the file's own Keras-ordered lists), LatentGAN.load likewise, and the headless demo loop (evaluation/confignet_demo.py
    --test_mode, the reference's tests/evaluation_test.py:30-48) runs in both of its modes on top of them."""
    import confignet
    from confignet_amd import ops
    sys.path.insert(0, os.path.join(ROOT, "evaluation"))
    import confignet_demo
    lists, lg = _write_reference_checkpoint(tmp_path)
    m = confignet.load_confignet(str(tmp_path / "model.json"))
    assert type(m).__name__ == "ConfigNet" and m.config["latent_dim"] == L_DEMO and set(m.facemodel_param_distributions) == set(FM_DEMO)
    for key, net in (("generator_weights", m.generator), ("generator_smoothed_weights", m.generator_smoothed),
                     ("real_encoder_weights", m.encoder), ("latent_regressor_weights", m.latent_regressor)):
        got = net.get_weights()
        assert len(got) == len(lists[key]) and all(np.array_equal(a, b) for a, b in zip(got, lists[key])), key
    rng = np.random.default_rng(9)
    z, rot = rng.standard_normal((3, L_DEMO)), rng.uniform(-0.3, 0.3, (3, 3))
    imgs = m.generate_images(z, rot)                                        # smoothed generator, replayed HIP graph
    ref = R.generator_forward([t64(w) for w in lists["generator_smoothed_weights"]], t64(z), t64(rot), 128)
    ref_u8 = ((ref.clamp(-1, 1) + 1) * 127.5).numpy()
    assert imgs.dtype == np.uint8 and np.abs(imgs.astype(np.float64) - ref_u8).max() <= 1.0 + 127.5e-3     # truncation + 1e-3
    m.use_inference_graphs = False
    assert np.abs(m.generate_images(z, rot).astype(int) - imgs.astype(int)).max() <= 1                     # eager dispatch
    m.use_inference_graphs = True
    assert np.abs(m.generate_images(z[:1], rot[:1]).astype(int) - imgs[:1].astype(int)).max() <= 1         # another batch size
    face = rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    emb, r = m.encode_images(face)
    emb_r, rot_r = R.real_encoder_forward([t64(w) for w in lists["real_encoder_weights"]], t64(face.astype(np.float64) / 127.5 - 1.0))
    assert np.abs(emb - emb_r.numpy()).max() <= 1e-3 * max(1.0, float(emb_r.abs().max())) and np.abs(r - rot_r.numpy()).max() < 1e-4
    gan = confignet.LatentGAN.load(str(tmp_path / "lg" / "model.json"))
    assert all(np.array_equal(a, b) for a, b in zip(gan.generator_smoothed.get_weights(), lg["smoothed_generator_weights"]))
    np.random.seed(0)
    lat = gan.generate_latents(1)
    np.random.seed(0)
    zz = np.random.normal(0, 1, (1, L_DEMO))
    assert np.abs(lat - O.mlp_simple(t64(zz), [t64(w) for w in lg["smoothed_generator_weights"]], 0.3).numpy()).max() < 1e-4
    # the demo: sampled from the LatentGAN (6 faces), and on one input image (incl. the one-shot fine-tune key)
    np.save(str(tmp_path / "face.npy"), face[0])
    frames = []
    s1 = confignet_demo.run(["--confignet_model_path", str(tmp_path / "model.json"), "--latent_gan_model_path", str(tmp_path / "lg" / "model.json"),
                             "--output_dir", str(tmp_path / "frames"), "--test_mode"])
    canvas = np.load(str(tmp_path / "frames" / "frame_0000.npy"))
    assert canvas.shape == (2 * 128, 3 * (2 * 128 + 20), 3) and canvas.dtype == np.uint8 and s1.exit
    s2 = confignet_demo.run(["--confignet_model_path", str(tmp_path / "model.json"), "--image_path", str(tmp_path / "face.npy"), "--test_mode"])
    assert s2.n_rows == s2.n_cols == 1 and s2.model.generator_fine_tuned is not None and s2.exit
    # a keyed session: head pose / gaze / attribute keys change the rendering, 'v' restores the embedding target
    s3 = confignet_demo.DemoSession(m, gan, None, 1, 2)
    a = s3.frame()
    for k in "ddwix":
        s3.key(k)
    b = s3.frame()
    assert a.shape == b.shape == (128, 2 * 276, 3) and np.abs(a.astype(int) - b.astype(int)).max() > 0
    assert abs(s3.rotation_offset[0, 0] - 0.1) < 1e-12 and abs(s3.eye_rotation_offset[0, 0] + 0.05) < 1e-12
    assert ops.ACT_DTYPE == torch.float32


def test_loss_dicts_survive_the_next_replay_and_keras_style_apply_gradients():
    """Boundary details of the step API: (1) in HIP-graph mode the returned loss scalars are copies taken
    right after the replay, so a caller may keep last iteration's dicts (the reference returns fresh tensors every step);
    (2) optimizer.apply_gradients(zip(gradients, variables)) -- the Keras call shape of confignet_first_stage.py:472-474 -- works
    on the weights of a network and equals the arena form."""
    from confignet_amd import ConfigNet, SyntheticFaceDataset, optim
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    from confignet_amd.dnn_models.building_blocks import MLPSimple
    ds = SyntheticFaceDataset(16, 128, seed=3)
    cfg = merge_configs(DEFAULT_CONFIG, {"batch_size": 4, "output_shape": (128, 128, 3)})
    ds.process_metadata(cfg, True)
    np.random.seed(1)
    m = ConfigNet(cfg, seed=0)
    m.setup_training(None, ds, 0, real_training_set=ds)
    m.use_graphs = True
    dopt, gopt = optim.Adam(**m.config["optimizer"]), optim.Adam(**m.config["optimizer"])
    for _ in range(3):
        m.training_iteration(ds, ds, dopt, gopt)
    kept = m.training_iteration(ds, ds, dopt, gopt)
    torch.cuda.synchronize()
    before = [{k: float(v) for k, v in d.items()} for d in kept]
    nxt = m.training_iteration(ds, ds, dopt, gopt)
    torch.cuda.synchronize()
    after = [{k: float(v) for k, v in d.items()} for d in kept]
    assert before == after                                                     # untouched by the following replay
    assert any(abs(float(a["loss_sum"]) - b["loss_sum"]) > 0 for a, b in zip(nxt, before))   # ... which produced new numbers
    # Keras-style call
    rng = np.random.default_rng(0)
    a, b = MLPSimple(3, 8, 12, 4, rng=np.random.default_rng(5)), MLPSimple(3, 8, 12, 4, rng=np.random.default_rng(5))
    grads = [torch.tensor(rng.standard_normal(tuple(w.shape)), dtype=torch.float32, device="cuda") for w in a.weights]
    o1, o2 = optim.Adam(lr=1e-3), optim.Adam(lr=1e-3)
    o1.apply_gradients(zip(grads, a.trainable_weights))
    for p, g in zip(b.weights, grads):
        p.grad.copy_(g)
    o2.apply_gradients(b)
    assert o1.iterations == o2.iterations == 1 and torch.equal(a.arena, b.arena)
    assert float((a.arena - MLPSimple(3, 8, 12, 4, rng=np.random.default_rng(5)).arena).abs().max()) > 5e-4


def test_cross_iteration_overlap_of_the_discriminator_steps():
    """overlap_discriminators (bench.py / train() switch it on): the real half of the next iteration's discriminator and
    synthetic-discriminator steps is replayed next to the generator tail.  Same np.random draws in the same order, same
    first iteration, and -- as far as the chaotic lr*sign(g) steps of a fresh GAN allow a comparison -- the same trajectory:
    the terms that depend only on the discriminator's own weights and the real batch (GAN_loss_real_i, gp_loss_i) stay
    together, the fake terms spread like two runs of the SAME configuration do (atomics order)."""
    from confignet_amd import ConfigNet, SyntheticFaceDataset, optim
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    runs = {}
    for flag in (False, True):
        np.random.seed(0)
        ds = SyntheticFaceDataset(64, 128, seed=1)
        cfg = merge_configs(DEFAULT_CONFIG, {"batch_size": 4, "output_shape": (128, 128, 3)})
        ds.process_metadata(cfg, True)
        m = ConfigNet(cfg, seed=0)
        m.setup_training(None, ds, 0, real_training_set=ds)
        m.use_graphs, m.overlap_discriminators = True, flag
        dopt, gopt = optim.Adam(**cfg["optimizer"]), optim.Adam(**cfg["optimizer"])
        draws, orig = [], m._stage_real

        def logged(key, dataset, n, orig=orig, draws=draws):
            st = np.random.get_state()
            draws.append((key, tuple(np.random.randint(0, dataset.imgs.shape[0], n).tolist())))
            np.random.set_state(st)
            return orig(key, dataset, n)
        m._stage_real = logged
        hist = []
        for _ in range(5):
            hist.append([{k: float(v) for k, v in d.items()} for d in m.training_iteration(ds, ds, dopt, gopt)])
        torch.cuda.synchronize()
        segs = {k[0]: (len(g.segments), g.early_cut) for k, g in m._graphs.items()}
        runs[flag] = (hist, draws, segs, m, ds, dopt, gopt)
    (h0, d0, s0, _, _, _, _), (h1, d1, s1, m, ds, dopt, gopt) = runs[False], runs[True]
    assert s0["d"] == (1, 0) and s1["d"] == (2, 1) and s1["sd"] == (2, 1) and s1["g"] == s0["g"]
    # the overlapped run has drawn the NEXT iteration's batches already (all four host halves, in the iteration's order: the
    # generator step's ground-truth VGG passes are replayed ahead with the discriminators' real halves), nothing else differs
    assert d1[:len(d0)] == d0 and [k for k, _ in d1[len(d0):]] == ["d", "sd", "ld", "g"]
    assert set(m._prestaged) == {"d", "sd", "ld", "g"} and m._targets_ahead is not None
    for a, b in zip(h0[0], h1[0]):                                   # first iteration: the split update against the single one
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-3 * max(1.0, abs(a[k])), (k, a[k], b[k])
    for it in range(1, 5):
        for step in (0, 1):                                          # discriminator, synthetic discriminator
            for k, v in h0[it][step].items():
                # (two runs of the SAME configuration are 1e-5 apart here at iteration 1 and percents apart by iteration 3)
                # (round 6: iteration 2 at 1e-1 -- one run in ~15 of the unchanged comparison left the 2e-2 band there, as two runs of
                # ONE configuration do; iteration 1 stays at 2e-2)
                if it <= 2 and (k.startswith("GAN_loss_real_") or k.startswith("gp_loss_")):
                    assert abs(v - h1[it][step][k]) <= (2e-2 if it == 1 else 1e-1) * max(1.0, abs(v)), (it, step, k, v, h1[it][step][k])
        assert all(np.isfinite(v) for d in h1[it] for v in d.values())
    # a step called on its own while its real half is in flight completes that iteration's step ...
    before = m.discriminator.get_weights()[2].copy()
    out = m.discriminator_training_step(ds, dopt)
    assert np.isfinite(float(out["loss_sum"])) and "d" not in m._prestaged
    assert np.abs(m.discriminator.get_weights()[2] - before).max() > 0
    # ... and one called with other arguments does not use the half that was prepared for these
    from confignet_amd import SyntheticFaceDataset as SFD
    other = SFD(32, 128, seed=7)
    other.process_metadata(m.config, True)
    m.training_iteration(ds, ds, dopt, gopt)
    assert "sd" in m._prestaged
    out = m.synth_discriminator_training_step(other, dopt)
    assert np.isfinite(float(out["loss_sum"])) and "sd" not in m._prestaged


# ------------------------------------------------------------------------------------------------------------
def _small_second_stage(res=128, batch=2):
    from confignet_amd import ConfigNet, SyntheticFaceDataset, optim
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    real_set, synth_set = SyntheticFaceDataset(8, res, seed=5), SyntheticFaceDataset(8, res, seed=6)
    cfg = merge_configs(DEFAULT_CONFIG, {"batch_size": batch, "output_shape": (res, res, 3)})
    synth_set.process_metadata(cfg, True)
    np.random.seed(11)
    m = ConfigNet(cfg, seed=12)
    m.setup_training(None, synth_set, 0, real_training_set=real_set)
    return m, real_set, synth_set, optim.Adam(**cfg["optimizer"]), optim.Adam(**cfg["optimizer"])


def test_eager_forwards_between_replays_and_after_ema_see_the_current_weights(monkeypatch):
    """Derived filter copies (parity-class filters of the upsample-folded layers, Winograd filters, tap-flipped copies) and the
    cached inference graphs are keyed on Net.epoch.  Raw-pointer updates -- the EMA kernel (confignet_first_stage.py:393-400)
    and the Adam launches that are NODES of a replayed step graph -- must move that epoch, or generate_images / encode_images
    between training iterations mix filters of the previous weights with current biases (ADVICE round 2, high + medium)."""
    from confignet_amd import ops
    m, real_set, synth_set, d_opt, g_opt = _small_second_stage()
    m.use_graphs = True
    rng = np.random.default_rng(0)
    z, rot = rng.standard_normal((2, m.config["latent_dim"])), rng.uniform(-0.3, 0.3, (2, 3))
    face = rng.integers(0, 256, (2, 128, 128, 3), dtype=np.uint8)
    for _ in range(3):                                       # eager, capture, replay
        m.training_iteration(real_set, synth_set, d_opt, g_opt)
    img0, (emb0, _) = m.generate_images(z, rot), m.encode_images(face)      # caches / inference graph of the current weights
    for _ in range(2):                                       # pure replays: Adam as graph nodes, then EMA
        m.training_iteration(real_set, synth_set, d_opt, g_opt)
    m.update_smoothed_weights(smoother_alpha=0.0)            # smoothed := trained generator (a visible change)
    img1, (emb1, _) = m.generate_images(z, rot), m.encode_images(face)
    # the same forwards with nothing derived and nothing cached
    monkeypatch.setattr(ops, "UPFOLD", False)
    monkeypatch.setattr(ops, "WINOGRAD", False)
    m.use_inference_graphs = False
    for net in (m.generator_smoothed, m.encoder):
        net.mark_updated()
    img_ref, (emb_ref, _) = m.generate_images(z, rot), m.encode_images(face)
    assert np.abs(img1.astype(int) - img_ref.astype(int)).max() <= 1, np.abs(img1.astype(int) - img_ref.astype(int)).max()
    assert np.abs(emb1 - emb_ref).max() <= 1e-4 * max(1.0, np.abs(emb_ref).max()), np.abs(emb1 - emb_ref).max()
    assert np.abs(img1.astype(int) - img0.astype(int)).max() > 1 and np.abs(emb1 - emb0).max() > 1e-4     # (the weights did move)


@pytest.mark.parametrize("graphs", [False, True])
def test_deterministic_mode_is_bitwise_reproducible(graphs):
    """cn_set_deterministic (CN_DETERMINISTIC=1): fixed-order reductions instead of fp32 atomics in the statistics passes,
    split-K, the filter gradients, the loss reductions and the rotation's scatter -- two runs of two whole training
    iterations from the same state end in BIT-IDENTICAL weights, Adam moments and loss scalars (the default mode does not:
    the order of its atomics decides last bits, and through lr*sign(g) steps whole entries)."""
    from confignet_amd import ops
    ops.set_deterministic(True)
    try:
        m, real_set, synth_set, d_opt, g_opt = _small_second_stage()
        assert not m.fork_generator_step
        m.use_graphs = graphs
        m.overlap_discriminators = graphs
        nets = m.all_networks()
        for _ in range(4 if graphs else 1):                   # (graphs: eager warm-ups, capture, first pipelined replay)
            m.training_iteration(real_set, synth_set, d_opt, g_opt)
        torch.cuda.synchronize()
        start = [n.get_weights() for n in nets]

        def run():
            for n, w0 in zip(nets, start):
                n.set_weights(w0)
            for o in (d_opt, g_opt):
                o.iterations = 0
                for mom, var in o._state.values():
                    mom.zero_(); var.zero_()
            np.random.seed(123)
            losses = []
            for _ in range(2):
                out = m.training_iteration(real_set, synth_set, d_opt, g_opt)
                losses.append([{k: float(v) for k, v in d.items()} for d in out])
            torch.cuda.synchronize()
            state = [n.arena.detach().cpu().clone() for n in nets]
            state += [t.detach().cpu().clone() for o in (d_opt, g_opt) for pair in o._state.values() for t in pair]
            return losses, state

        l1, s1 = run()
        l2, s2 = run()
        assert l1 == l2, [(a, b) for x, y in zip(l1, l2) for da, db in zip(x, y) for (_, a), (_, b) in zip(da.items(), db.items()) if a != b][:5]
        for i, (a, b) in enumerate(zip(s1, s2)):
            assert torch.equal(a, b), ("tensor %d differs" % i, float((a - b).abs().max()))
    finally:
        ops.set_deterministic(False)


def test_data_parallel_dispatch_with_overlap_matches_single_process(tmp_path):
    """The multi-rank code path -- step graphs that end after the backward pass, RCCL all-reduce of the gradient arenas and
    Adam issued eagerly after every replay (also for the split discriminator graphs of the cross-iteration overlap, whose real
    half is pre-replayed under the previous generator tail and ACCUMULATES into the arena), the generator step's two-part
    backward with the early all-reduce of the generator / regressor arenas, and the global batch statistics of the latent
    regression (DeferredGlobalStatsRegression: two graph cuts with a collective each) -- on a 1-rank RCCL group
    (CN_FORCE_DP=1), against the single-process dispatch of the same iterations.  Deterministic mode: without the statistics
    flag the two must agree BIT FOR BIT (a 1-rank mean is the identity; the Adam kernel is the same launch inside or after
    the graph)."""
    import subprocess
    helper = os.path.join(ROOT, "tests", "dp_run_helper.py")
    dp_env = {"CN_FORCE_DP": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29547", "RANK": "0", "WORLD_SIZE": "1"}
    outs = []
    for tag, extra, flag in (("single", {}, 0), ("dp", dp_env, 0), ("dp_stats", dict(dp_env, MASTER_PORT="29549"), 1)):     # (a port of its own per group)
        env = {k: v for k, v in os.environ.items() if k not in ("CN_FORCE_DP",)}
        env.update(extra)
        path = str(tmp_path / (tag + ".npz"))
        for attempt in (0, 1):
            r = subprocess.run([sys.executable, helper, path, str(flag)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
            # torch's RCCL watchdog THREAD polls the end events of collectives with hipEventQuery; next to a HIP-graph capture in the
            # same process that query has been seen to fail with hipErrorCapturedEvent and take the process down (rc -6, twice in ~8
            # runs of the whole suite, never in 38 runs of this helper alone: DESIGN.md section 5) -- a runtime race outside the
            # arithmetic this test compares; one retry with a fresh rendezvous port, anything else fails at once
            if r.returncode == 0 or attempt == 1 or "last recorded in a capturing stream" not in r.stderr:
                break
            env["MASTER_PORT"] = str(int(env.get("MASTER_PORT", "29547")) + 20)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append(np.load(path))
    a, b, c = outs
    assert not bool(a["dp"][0]) and bool(b["dp"][0]) and bool(b["split"].all()) and not bool(a["split"].any())
    assert np.array_equal(a["losses"], b["losses"]), np.abs(a["losses"] - b["losses"]).max()
    for k in a.files:
        if k[0] in "wmvf":
            assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))
    # global batch statistics (config["dp_global_batch_statistics"]): with ONE rank the global batch is the local one, so the
    # objective is the same; the statistics are computed by another formula (E[x^2] - mean^2 of the reduced sums), hence not
    # bit for bit: first-iteration loss scalars to 1e-4, first-iteration weight steps (lr*sign(g)) equal but for noise-level entries
    l_a, l_c = a["losses"][0], c["losses"][0]
    assert np.all(np.abs(l_a - l_c) <= 1e-4 * np.maximum(1.0, np.abs(l_a))), np.abs(l_a - l_c).max()
    lr = 4e-4
    for k in a.files:
        if k[0] == "f":
            wrong = float((np.abs(a[k] - c[k]) > 0.1 * lr).mean())
            assert wrong < 0.02, (k, wrong)


def _run_two_ranks(tmp_path, tag, global_stats, deterministic, port, dtype="f32"):
    """Two processes of tests/dp2_run_helper.py on the ONE device, a gloo group between them (RCCL refuses two ranks on one
    device; gloo moves the same arenas through the host).  Returns the two ranks' result files."""
    import subprocess
    helper = os.path.join(ROOT, "tests", "dp2_run_helper.py")
    procs, paths = [], []
    for r in range(2):
        env = {k: v for k, v in os.environ.items() if k not in ("CN_FORCE_DP",)}
        env.update({"CN_DP_BACKEND": "gloo", "CN_DP_SHARE_DEVICE": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                    "RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "2", "OMP_NUM_THREADS": "8"})
        path = str(tmp_path / ("%s_rank%d.npz" % (tag, r)))
        paths.append(path)
        log = open(str(tmp_path / ("%s_rank%d.log" % (tag, r))), "w")
        procs.append((subprocess.Popen([sys.executable, helper, path, "rank", "8", str(global_stats), str(deterministic), "--dtype=" + dtype],
                                       env=env, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT), log))
    try:
        for p, log in procs:
            rc = p.wait(timeout=1500)
            log.close()
            assert rc == 0, open(log.name).read()[-4000:]
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
    return paths


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _run_single(tmp_path, tag, batch, deterministic, replay, dtype="f32"):
    """One process of tests/dp2_run_helper.py re-running the batches that ranks of a two-rank run logged (concatenated)."""
    import subprocess
    helper = os.path.join(ROOT, "tests", "dp2_run_helper.py")
    env = {k: v for k, v in os.environ.items() if k not in ("CN_FORCE_DP", "CN_DP_BACKEND", "CN_DP_SHARE_DEVICE", "RANK", "WORLD_SIZE")}
    path = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, helper, path, "single", str(batch), "0", str(deterministic), "--dtype=" + dtype] + list(replay),
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = np.load(path)
    assert not bool(out["dp"][0]) and not bool(out["split"].any())
    return out


@pytest.mark.parametrize("deterministic", [0, 1])
def test_two_rank_data_parallel_run_of_the_benchmarked_dispatch(tmp_path, deterministic):
    """BASELINE.json configs[2] with N > 1 (reference confignet_second_stage.py:277-288 on every rank): TWO
    processes run the benchmark's own model at 256 x 256, batch 8 each, in the benchmark's dispatch -- step graphs that end after
    the backward pass, gradient all-reduce + Adam issued eagerly after every replay, split discriminator graphs whose real half
    is pre-replayed under the previous generator tail, the generator step's two-part backward with the early buckets, per-rank
    seeds -- for three iterations, once with the per-rank batch statistics and once with dp_global_batch_statistics.
    (a) the replicas stay BIT-IDENTICAL (weights and both Adam moments of every network on the two ranks, after 1 and 3 iterations);
    (b) the gradient Adam saw in iteration 1 (beta_1 = 0: its first moment IS the all-reduced gradient)
        * deterministic mode, discriminator-type networks: equals 0.5 * (g_0 + g_1) BIT FOR BIT, g_r = the gradient of a single
          process that runs rank r's logged batches at batch 8 (same kernels, same launch shapes: the exchange adds nothing but
          the mean);
        * equals the gradient of ONE process that runs the concatenated batch of 16, to what two fp32 runs with different launch
          shapes (batch 8 / 16 pick different tiles and row splits) can agree on: 2e-3 relative L2 for the discriminator-type
          networks (measured 8e-5 ... 5.5e-4; the latent discriminator, an MLP, 1.2e-7), 4e-2 for the generator step's networks
          with the global batch statistics (measured 2e-3 ... 1.5e-2: the chain generator -> VGG-19 -> ResNet-50 -> six heads
          differs by 1e-2 ... 1e-1 between ANY two summation orders through LeakyReLU / ReLU / max-pool decisions on near-zero
          inputs, DESIGN.md section 7 -- the exact statement of this identity is the float64 gloo test, tests/test_parallel_cpu.py);
        * the flag does what it says: with dp_global_batch_statistics the rank mean of the latent-regression loss equals the
          batch-16 value, with per-rank statistics (SURVEY.md section 8e option (ii)) it does not;
    (c) the ranks drew different batches."""
    runs = {}
    for gs in (0, 1):
        paths = _run_two_ranks(tmp_path, "gs%d" % gs, gs, deterministic, 29561 + gs + 2 * deterministic)
        runs[gs] = [np.load(p) for p in paths]
    single = _run_single(tmp_path, "single16", 16, deterministic, [str(tmp_path / ("gs1_rank%d.npz" % i)) for i in range(2)])
    for gs in (0, 1):
        r0, r1 = runs[gs]
        assert bool(r0["dp"][0]) and bool(r0["split"].all()) and int(r0["g_segments"][0]) >= 2       # early-bucket cut(s) present
        assert np.isfinite(r0["losses"]).all() and np.isfinite(r1["losses"]).all()
        # (a) replicas bit for bit
        n_checked = 0
        for k in r0.files:
            if k[0] == "w" or k.startswith(("first_", "last_")):
                assert np.array_equal(r0[k], r1[k]), (gs, k, float(np.abs(r0[k] - r1[k]).max()))
                n_checked += 1
        assert n_checked >= 8 + 2 * 2 * 7
        # (c) different batches per rank, and the two configurations drew the same ones
        assert not np.array_equal(r0["log/d/real_idx"], r1["log/d/real_idx"]) and not np.array_equal(r0["log/g/rot"], r1["log/g/rot"])
        assert np.array_equal(r0["log/g/synth_idx"], runs[1][0]["log/g/synth_idx"])
    keys = sorted(k for k in single.files if k.startswith("first_m"))
    assert len(keys) == 7                             # d_opt: discriminator, synth-D, latent-D; g_opt: the generator step's four
    # (b) deterministic mode: the exchanged gradient is exactly the mean of the two local ones
    if deterministic:
        local = [_run_single(tmp_path, "single8_r%d" % r, 8, 1, [str(tmp_path / ("gs0_rank%d.npz" % r))]) for r in range(2)]
        # (the three discriminator-type networks: their steps come first in the iteration, so every rank and the lone processes
        # differentiate at the same weights.  The generator step follows the discriminator updates -- made with the EXCHANGED
        # gradient in the two-rank run, with the local one in a lone process -- so its gradients are not comparable this way.)
        for k in keys[:3]:
            mean = (local[0][k] + local[1][k]) * np.float32(0.5)
            assert np.abs(mean).max() > 0
            assert np.array_equal(runs[0][0][k], mean), (k, _rel_l2(runs[0][0][k], mean))
        # ... and each rank computed what a lone process computes: every scalar of the three discriminator-type steps
        names0 = [str(n) for n in single["loss_names"]]
        n_dtype = [i for i, n in enumerate(names0) if n == "loss_sum"][2] + 1
        assert np.array_equal(local[0]["losses"][0][:n_dtype], runs[0][0]["losses"][0][:n_dtype])
    # (b) rank mean against the global batch
    worst = {}
    for gs in (0, 1):
        for k in keys:
            assert np.abs(single[k]).max() > 0
            worst[(gs, k)] = _rel_l2(runs[gs][0][k], single[k])
    print("rank-mean vs global-batch gradient, rel L2:", {("%d/%s" % k): "%.2e" % v for k, v in worst.items()})
    n_d = 3
    for (gs, k), e in worst.items():
        idx = int(k[len("first_m"):])
        if idx < n_d:
            assert e <= 2e-3, (gs, k, e)                  # (measured 4e-5 ... 5.5e-4 over a dozen runs)
        elif gs == 1:
            assert e <= 4e-2, (gs, k, e)
    # loss scalars, first iteration (same weights everywhere): per-sample means agree between the rank mean and the global batch;
    # the latent-regression term only with the global statistics
    names = [str(n) for n in single["loss_names"]]
    l_one = single["losses"][0]
    dev = {}
    for gs in (0, 1):
        l_dp = 0.5 * (runs[gs][0]["losses"][0] + runs[gs][1]["losses"][0])
        for i, n in enumerate(names):
            if n.startswith("GAN_loss") or n == "latent_GAN_loss":
                # (forward-only scalars; the deepest heads of the discriminators on GENERATED images sit behind generator + five
                # blocks and differ by up to ~1e-3 between two launch-shape sets: measured 5e-4 ... 6e-4 on GAN_loss_synth_5)
                assert abs(l_dp[i] - l_one[i]) <= 3e-3 * max(1.0, abs(l_one[i])), (gs, n, l_dp[i], l_one[i])
        i = [j for j, n in enumerate(names) if n == "latent_regression_loss"][-1]
        dev[gs] = abs(l_dp[i] - l_one[i]) / abs(l_one[i])
    print("latent-regression loss, |rank mean - global batch| / global:", dev)
    assert dev[1] <= 2e-4 and dev[0] > 20 * max(dev[1], 1e-6), dev


@pytest.mark.gpu
def test_two_rank_data_parallel_run_in_bf16(tmp_path):
    """BASELINE.json configs[2] as it is named -- bf16 compute AND N > 1 together (the fp32 test above and the one-rank bf16 DP test
    of tests/test_bf16_gpu.py cover the two halves separately): two processes run the benchmark's model at 256 x 256, batch 8 each,
    bf16 activations, in the benchmark's dispatch, global batch statistics, three iterations.
    (a) every scalar is finite; (b) the replicas stay BIT-IDENTICAL (fp32 master weights and both Adam moments of every network --
    the exchange is on the fp32 gradient arenas, so bf16 changes nothing about this identity); (c) the ranks drew different batches;
    (d) the exchanged gradient of iteration 1 against ONE bf16 process on the concatenated batch of 16 (different launch shapes:
    batch 8 and 16 pick different tiles and splits), measured beside the yardstick that says what bf16 can resolve at all: the same
    single process in fp32 on the same batches.  Discriminator-type networks: <= 5e-2 relative L2 (measured ~1e-2; fp32: 5e-4).
    Generator-step networks: the rank mean must be as close to the bf16 global-batch gradient as that gradient is to the fp32 one,
    within a factor 2 -- i.e. the exchange adds nothing to bf16's own error (both are printed; for the generator itself the bf16
    gradient of ONE iteration differs from fp32 by O(1) in relative L2: the bf16 run takes it at another forward point -- 2^-9 of
    storage rounding per tensor, amplified by the normalisation stacks of the networks the loss runs through; at equal forward
    state and equal branch decisions the same networks' bf16 gradients are within 1 - 3 % of the float64 oracle
    (tests/test_bf16_grads_gpu.py, tests/test_bf16_grad_yardstick_cpu.py) -- a property of configs[2]'s dtype, not of the exchange);
    (e) the per-sample loss means of the rank mean and of the global batch agree to 0.15 of max(1, |value|) (the deepest heads
    move by up to 8 % between the batch-8 and the batch-16 launch shapes in bf16; tests/test_bf16_gpu.py's whole-iteration bound
    against the oracle is 5 % + an R1-scaled allowance)."""
    paths = _run_two_ranks(tmp_path, "bf16", 1, 0, 29581, dtype="bf16")
    r0, r1 = [np.load(p) for p in paths]
    single = _run_single(tmp_path, "bf16_single16", 16, 0, paths, dtype="bf16")
    assert bool(r0["dp"][0]) and bool(r0["split"].all()) and int(r0["g_segments"][0]) >= 2
    assert np.isfinite(r0["losses"]).all() and np.isfinite(r1["losses"]).all() and np.isfinite(single["losses"]).all()
    n_checked = 0
    for k in r0.files:
        if k[0] == "w" or k.startswith(("first_", "last_")):
            assert np.isfinite(r0[k]).all(), k
            assert np.array_equal(r0[k], r1[k]), (k, float(np.abs(r0[k] - r1[k]).max()))
            n_checked += 1
    assert n_checked >= 8 + 2 * 2 * 7
    assert not np.array_equal(r0["log/d/real_idx"], r1["log/d/real_idx"]) and not np.array_equal(r0["log/g/rot"], r1["log/g/rot"])
    keys = sorted(k for k in single.files if k.startswith("first_m"))
    assert len(keys) == 7
    single32 = _run_single(tmp_path, "f32_single16", 16, 0, paths, dtype="f32")
    worst = {k: _rel_l2(r0[k], single[k]) for k in keys}
    yard = {k: _rel_l2(single[k], single32[k]) for k in keys}
    print("bf16: rank-mean vs global-batch gradient, rel L2:", {k: "%.2e" % v for k, v in worst.items()})
    print("bf16: global-batch gradient, bf16 vs fp32 run of the same batches, rel L2:", {k: "%.2e" % v for k, v in yard.items()})
    for k, e in worst.items():
        assert np.abs(single[k]).max() > 0
        if int(k[len("first_m"):]) < 3:
            assert e <= 5e-2, (k, e)
        else:
            assert e <= 2.0 * max(yard[k], 1e-2), (k, e, yard[k])
    names = [str(n) for n in single["loss_names"]]
    l_dp, l_one = 0.5 * (r0["losses"][0] + r1["losses"][0]), single["losses"][0]
    dev = {n: abs(a - b) / max(1.0, abs(b)) for n, a, b in zip(names, l_dp, l_one) if n.startswith("GAN_loss") or n in ("latent_GAN_loss", "latent_regression_loss")}
    print("bf16: loss scalars, |rank mean - global batch| / max(1, |global|), worst:", max(dev.items(), key=lambda kv: kv[1]))
    # (measured worst: 8.3e-2 on GAN_loss_real_5, the deepest head -- five bf16 blocks behind the image, at two launch-shape sets)
    assert max(dev.values()) <= 0.15, dev

"""The AdaIN MLP bank (F.mlp_bank on cn_gemm_rows_grouped_k) at 17..32 rows, where its backward products (k = 2c = 512 and more at
MT = 32) no longer fit the whole-block launch and take gemm_rows_grouped_ksteps_kernel; and the training steps at the default batch of
DEFAULT_CONFIG (24, the reference's own value).

Gradients: at these row counts the layerwise form (one F.linear per Dense layer) computes the same products on the 64 x 64 MFMA tile
kernel, so the two forms are not bit-equal.  Both are fp32 sums of the same K products in another order; each is compared with a
float64 statement of the same MLPs (torch CPU double), and the bank's relative L2 error may be at most 4 x the layerwise form's on the
same inputs -- the factor covers the order of the sums only.  The figures go to profiles/gemm_rows_ksteps_errors.txt when
GEMM_ROWS_KSTEPS_ERRORS names a path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_rows_ksteps_notes as NOTES

SLOPE = 0.2                  # TF_LRELU, the AdaIN MLPs' hidden activation


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _rel(a, ref):
    return float((a.detach().double().cpu() - ref).norm() / ref.norm())


def _mlp64(zs, sets, cots):
    """float64 gradients of sum_i <MLP_i(z_i), cot_i> (cot None: no term): d/dz per DISTINCT z tensor of `zs` (in order of first
    appearance) and d/d(w0, b0, w1, b1) per MLP (None where the MLP has no cotangent)"""
    uniq = []
    for z in zs:
        if all(z is not u for u in uniq):
            uniq.append(z)
    z64 = [u.detach().double().cpu().requires_grad_(True) for u in uniq]
    w64 = [[t.detach().double().cpu().requires_grad_(True) for t in st] for st in sets]
    loss = 0.0
    for z, w, c in zip(zs, w64, cots):
        if c is None:
            continue
        h = torch.nn.functional.leaky_relu(z64[[u is z for u in uniq].index(True)] @ w[0] + w[1], SLOPE)
        loss = loss + ((h @ w[2] + w[3]) * c.detach().double().cpu()).sum()
    live = [t for w, c in zip(w64, cots) if c is not None for t in w]
    g = torch.autograd.grad(loss, z64 + live)
    return list(g[:len(z64)]), list(g[len(z64):])


def _hold(tag, names, bank, layer, refs_bank, refs_layer):
    """the rule of the module docstring, per gradient; prints and records every pair of errors before it asserts"""
    over = []
    worst = (0.0, None)
    for name, b, l, rb, rl in zip(names, bank, layer, refs_bank, refs_layer):
        eb, el = _rel(b, rb), _rel(l, rl)
        print("%s %s: bank %.3e layerwise %.3e" % (tag, name, eb, el))
        if el > 0 and eb / el > worst[0]:
            worst = (eb / el, "%s: bank %.3e, layerwise %.3e" % (name, eb, el))
        if not eb <= 4.0 * el:
            over.append((name, eb, el))
    NOTES.note("bank and generator", tag, "%-44s largest bank / layerwise %.3f at %s" % (tag, worst[0], worst[1]))
    assert not over, over


# ---- (a) the bank against the layerwise chains --------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("n", [24, 17])
def test_mlp_bank_at_17_and_24_rows_equals_the_separate_dense_layers(n, deterministic):
    """tests/test_ops_gpu.py::test_mlp_bank_equals_the_separate_dense_layers at 24 and 17 rows, the first MLP 1024 wide: the backward
    products run k = 1024 and 512 (4 and 2 chunks at MT = 32) next to 256, 128 and 64 (one chunk).  Outputs bit for bit (forward k =
    145 and 128: one chunk, gemm_rows_kernel's arithmetic); gradients by the float64 rule; one output left without a cotangent."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    rng = np.random.default_rng(31 + n)
    latent, hidden = 145, 128
    outs = [1024, 256, 512, 128, 64, 64]
    za, zb = dev(rng.normal(size=(n, latent))), dev(rng.normal(size=(n, latent)))
    sets = [[dev(rng.normal(size=(latent, hidden)) * 0.1), dev(rng.normal(size=hidden) * 0.1), dev(rng.normal(size=(hidden, o)) * 0.1),
             dev(rng.normal(size=o) * 0.1)] for o in outs]
    cot = [None if k == 3 else dev(rng.normal(size=(n, o))) for k, o in enumerate(outs)]          # MLP 3 gets no cotangent
    res = {}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(deterministic)
    try:
        for bank in (False, True):
            z1, z2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
            zs = [z1, z2, z1, z1, z2, z1]
            ws = [[t.clone().requires_grad_(True) for t in st] for st in sets]
            if bank:
                sb = F.mlp_bank(zs, ws, SLOPE)
            else:
                sb = [F.linear(F.linear(z, w[0], w[1], ops.ACT_LRELU, SLOPE), w[2], w[3]) for z, w in zip(zs, ws)]
            loss = sum((o * c).sum() for o, c in zip(sb, cot) if c is not None)
            leaves = [z1, z2] + [t for k, st in enumerate(ws) if k != 3 for t in st]
            res[bank] = ([o.detach() for o in sb], torch.autograd.grad(loss, leaves))
    finally:
        ops.set_deterministic(prev)
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    gz, gw = _mlp64([za, zb, za, za, zb, za], sets, cot)
    refs = gz + gw
    names = ["z1", "z2"] + ["mlp%d/%s" % (k, s) for k in range(6) if k != 3 for s in ("w0", "b0", "w1", "b1")]
    _hold("bank n %d det %d" % (n, deterministic), names, res[True][1], res[False][1], refs, refs)


# ---- (b) the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("n", [24, 17])
def test_generator_forward_and_backward_at_17_and_24_samples(n, deterministic, monkeypatch):
    """HologanGenerator at 128 x 128, forward and backward with a random cotangent, mlp_bank True against False (the yardstick).  In
    deterministic mode the images are bit-equal, and so are the gradients of every weight outside the AdaIN MLPs (the same launches
    on the same bits).  The latent only feeds the MLPs, so its gradient and the MLP weights' are functions of the latent, the MLP
    weights and the cotangents that reach the five MLP outputs: those are recorded in each run (a hook on AdaIN's second input), the
    float64 MLPs are run backward from them, and each run's gradients are held to its own float64 statement by the rule above."""
    from confignet_amd import functional as F
    from confignet_amd import ops
    from confignet_amd.dnn_models.hologan_generator import HologanGenerator
    rng = np.random.default_rng(7 + n)
    g = HologanGenerator(145, (128, 128), 128, 2, "tanh", rng=rng)
    z0, rot = dev(rng.normal(size=(n, 145))), dev(rng.uniform(-0.3, 0.3, size=(n, 3)))
    cot = dev(rng.normal(size=(n, 128, 128, 3)))
    adain, seen = F.adain, []

    def recording_adain(x, sb, *a, **kw):
        slot = [None]
        seen.append(slot)
        if sb.requires_grad:
            sb.register_hook(lambda gr, slot=slot: slot.__setitem__(0, gr.detach().clone()))
        return adain(x, sb, *a, **kw)
    monkeypatch.setattr(F, "adain", recording_adain)
    weights = [w for w in g.weights if w.requires_grad]
    mlp_sets = [g.weights[4:8], g.weights[10:14]] + [g.weights[22 + 6 * j:26 + 6 * j] for j in range(3)]
    assert all(tuple(s[0].shape) == (145, 128) and s[2].shape[0] == 128 for s in mlp_sets)
    mlp_ids = {id(t) for s in mlp_sets for t in s}
    res = {}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(deterministic)
    try:
        for bank in (False, True):
            g.mlp_bank = bank
            del seen[:]
            z = z0.clone().requires_grad_(True)
            img = g((z, rot))
            grads = torch.autograd.grad(img, [z] + weights, grad_outputs=cot, allow_unused=True)
            torch.cuda.synchronize()
            assert len(seen) == 5 and all(s[0] is not None for s in seen)
            res[bank] = (img.detach(), grads, [s[0] for s in seen])
    finally:
        ops.set_deterministic(prev)
    assert img.shape == (n, 128, 128, 3)
    if deterministic:
        assert torch.equal(res[False][0], res[True][0])
    assert bool(torch.isfinite(res[True][0]).all())
    refs = {}
    for bank in (False, True):
        gz, gw = _mlp64([z0] * 5, mlp_sets, res[bank][2])
        refs[bank] = gz + gw
    pick = lambda gs: [gs[0]] + [gr for w, gr in zip(weights, gs[1:]) if id(w) in mlp_ids]
    names = ["latent"] + ["%s/%s" % (m, s) for m in ("map_3d_0", "map_3d_1", "map_2d_0", "map_2d_1", "map_2d_2") for s in ("w0", "b0", "w1", "b1")]
    assert len(pick(res[True][1])) == 21
    if deterministic:
        for w, a, b in zip(weights, res[False][1][1:], res[True][1][1:]):
            if id(w) not in mlp_ids and a is not None:
                assert torch.equal(a, b), tuple(w.shape)
    _hold("generator n %d det %d" % (n, deterministic), names, pick(res[True][1]), pick(res[False][1]), refs[True], refs[False])


# ---- (c), (d) the training steps at the default batch ---------------------------------------------------------------------------
def _default_config():
    from confignet_amd.confignet_first_stage import DEFAULT_CONFIG
    from confignet_amd.confignet_utils import merge_configs
    cfg = merge_configs(DEFAULT_CONFIG, {"output_shape": (128, 128, 3)})
    assert cfg["batch_size"] == DEFAULT_CONFIG["batch_size"] == 24
    return cfg


def test_one_first_stage_step_at_the_default_batch_with_and_without_the_bank():
    """one discriminator_training_step (24 generated images, forward only) and one generator_training_step (the batch splits into 12
    synthetic and 12 sampled latents) of ConfigNetFirstStage at DEFAULT_CONFIG's batch size, 128 x 128, in deterministic mode so that
    the comparison is about the bank: every loss finite, and bank on / off agree to 1e-3 (the loss-parity tolerance of the project)"""
    from confignet_amd import ConfigNetFirstStage, SyntheticFaceDataset, ops, optim
    cfg = _default_config()
    runs = {}
    prev = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        for bank in (True, False):
            np.random.seed(3)
            ds = SyntheticFaceDataset(32, 128, seed=2)
            ds.process_metadata(cfg, True)
            m = ConfigNetFirstStage(cfg, seed=0)
            m.setup_training(None, ds, 0, real_training_set=ds)
            m.generator.mlp_bank = bank
            dopt, gopt = optim.Adam(**cfg["optimizer"]), optim.Adam(**cfg["optimizer"])
            d = m.discriminator_training_step(ds, dopt)
            gl = m.generator_training_step(ds, ds, gopt)
            torch.cuda.synchronize()
            runs[bank] = {"d/" + k: float(v) for k, v in d.items()}
            runs[bank].update({"g/" + k: float(v) for k, v in gl.items()})
    finally:
        ops.set_deterministic(prev)
    assert m.get_batch_size() == 24 and len(runs[True]) >= 10
    for k, v in runs[True].items():
        print("%s: bank %.6f layerwise %.6f" % (k, v, runs[False][k]))
    for k, v in runs[True].items():
        assert np.isfinite(v) and np.isfinite(runs[False][k]), k
        assert abs(v - runs[False][k]) <= 1e-3 * max(1.0, abs(v)), (k, v, runs[False][k])


@pytest.mark.parametrize("merged", [False, True], ids=["two_passes", "stacked_pass"])
def test_one_second_stage_iteration_at_the_default_batch(merged):
    """one training_iteration of ConfigNet at DEFAULT_CONFIG's batch size, 128 x 128: every loss finite.  two_passes is the default
    form (the generator runs the synthetic and the real half as two batches of 12); stacked_pass (merge_generator_passes) runs all 24
    samples through the generator as one batch, whose backward pass is the one that needs the chunked launch"""
    from confignet_amd import ConfigNet, SyntheticFaceDataset, optim
    cfg = _default_config()
    np.random.seed(5)
    ds = SyntheticFaceDataset(32, 128, seed=6)
    ds.process_metadata(cfg, True)
    m = ConfigNet(cfg, seed=1)
    m.setup_training(None, ds, 0, real_training_set=ds)
    m.merge_generator_passes = merged
    assert m.generator.mlp_bank and m.get_batch_size() == 24
    out = m.training_iteration(ds, ds, optim.Adam(**cfg["optimizer"]), optim.Adam(**cfg["optimizer"]))
    torch.cuda.synchronize()
    assert len(out) == 4
    for d in out:
        for k, v in d.items():
            assert np.isfinite(float(v)), k

"""bf16 storage mode: the gradients of whole networks, held to about 1 % at the product's OWN forward state.

tests/test_bf16_gpu.py holds these gradients at rel-L2 0.3 against the fp32 oracle -- it cannot do better: the distance is the
gradient being taken at another forward point (tests/test_bf16_grad_yardstick_cpu.py, profiles/bf16_grad_attribution.txt).  Here the
oracle runs inside O.bf16_storage() with every stored activation REPLAYED from the product's run (ops.stored_log ->
O.StoredReplay) and every LeakyReLU decision forced from it (ops.branch_log -> O.BranchControl), so both gradients belong to one
forward state.  Per parameter tensor k the bound is 4 * b_k + 5e-3, b_k being what bf16 storage of the gradients costs in the
oracle itself (measured in the same test, 2e-3 - 7e-3); the conditions that keep the replay from hiding a wrong forward kernel are
asserted per storage point.  Account, constants and reasons: tests/bf16_grad_yardstick.py.

Cases (the smallest shapes each network takes; the float64 passes run on the CPU):
  generator       HologanGenerator 128 x 128, n = 2, loss (img * cot).sum(), ops.UPFOLD off: the bf16 kernels on per-tap filters
  generator_fold  the same with the upsample-folded layers collapsed (the default product); the oracle restates the pre-summed
                  class filters (O.bf16_storage(class_filters=True))
  discr_r1        compute_discriminator_loss at 64 x 64, n = 2: R1 through the stacked tangent pass
  discr_r1_heads  the same with losses.BATCHED_TANGENT off (head-by-head tangent passes)
  regressor       HologanLatentRegressor at 64 x 64, n = 2, random cotangent
Every 3x3 / 3x3x3 / 4x4 filter of every case must FAIL the comparison when its product gradient is scaled by 1.05.

Measured table: profiles/bf16_grad_errors.txt (written when BF16_GRAD_ERRORS names a path)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_nets as R
from oracle import ref_ops as O
from oracle import ref_steps as S
from tests import bf16_grad_yardstick as Y

CASES = ("generator", "generator_fold", "discr_r1", "discr_r1_heads", "regressor")
GEN_FOLDED_CALLS = (1, 3, 11, 13)      # `stored` calls of R.generator_forward directly behind an UpSampling + Conv layer
_results = {}
_tables = {}


@pytest.fixture(autouse=True)
def _bf16_mode():
    from confignet_amd import ops
    ops.set_activation_dtype("bf16")
    yield
    ops.set_activation_dtype("f32")


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda().contiguous()


def _perturb(net, rng, scale=0.1):
    """Biases, gammas and betas are zero / one initialised: move them so that their gradients matter."""
    ws = net.get_weights()
    net.set_weights([(w + scale * rng.normal(size=w.shape)).astype(np.float32) if w.ndim == 1 else w for w in ws])


def _product_generator(rng, fold):
    from confignet_amd import ops
    from confignet_amd.dnn_models.hologan_generator import HologanGenerator
    g = HologanGenerator(43, (128, 128), 128, 2, "tanh", rng=rng)
    ws = g.get_weights()
    ws[1] = (1 + 0.5 * rng.standard_normal(32768)).astype(np.float32)
    g.set_weights(ws)
    z = rng.normal(size=(2, 43))
    rot = rng.uniform(-0.4, 0.4, size=(2, 3)).astype(np.float32)
    cot = rng.normal(size=(2, 128, 128, 3))
    upfold, ops.UPFOLD = ops.UPFOLD, fold
    try:
        g.zero_grad()
        with ops.stored_log() as slog, ops.branch_log() as blog:
            img = g((z, rot))
            torch.autograd.backward((img * dev(cot)).sum(), inputs=g.trainable_weights)
    finally:
        ops.UPFOLD = upfold
    wr = [t64(w).requires_grad_(True) for w in g.get_weights()]
    return g, wr, (lambda: (R.generator_forward(wr, t64(z), t64(rot), 128) * t64(cot)).sum()), slog, blog


def _product_discriminator(rng, batched_tangent):
    from confignet_amd import losses as L
    from confignet_amd import ops
    from confignet_amd.dnn_models.hologan_discriminator import HologanDiscriminator
    d = HologanDiscriminator((64, 64), 5, 512, 3, 48, True, rng=rng)
    _perturb(d, rng)
    real, fake = rng.uniform(-1, 1, size=(2, 64, 64, 3)), rng.uniform(-1, 1, size=(2, 64, 64, 3))
    prev, L.BATCHED_TANGENT = L.BATCHED_TANGENT, batched_tangent
    try:
        d.zero_grad()
        with ops.stored_log() as slog, ops.branch_log() as blog:
            loss = L.compute_discriminator_loss(d, d.to_device(real), d.to_device(fake))["loss_sum"]
            torch.autograd.backward(loss, inputs=d.trainable_weights)
    finally:
        L.BATCHED_TANGENT = prev
    wr = [t64(w).requires_grad_(True) for w in d.get_weights()]
    return d, wr, (lambda: S.discriminator_loss(wr, t64(real), t64(fake))["loss_sum"]), slog, blog


def _product_regressor(rng):
    from confignet_amd import ops
    from confignet_amd.dnn_models.hologan_discriminator import HologanLatentRegressor
    net = HologanLatentRegressor(43, (64, 64), 5, 512, 3, 48, True, rng=rng)
    _perturb(net, rng)
    img = rng.uniform(-1, 1, size=(2, 64, 64, 3))
    cot = rng.normal(size=(2, 46))
    net.zero_grad()
    with ops.stored_log() as slog, ops.branch_log() as blog:
        out = net(net.to_device(img))
        torch.autograd.backward((out * dev(cot)).sum(), inputs=net.trainable_weights)
    wr = [t64(w).requires_grad_(True) for w in net.get_weights()]
    return net, wr, (lambda: (R.latent_regressor_forward(wr, t64(img)) * t64(cot)).sum()), slog, blog


def _run(case):
    """Product pass (logged), the oracle at its forward state, the oracle's yardstick pass: computed once per case."""
    if case in _results:
        if isinstance(_results[case], Exception):
            raise _results[case]
        return _results[case]
    rng = np.random.default_rng(1 + CASES.index(case.replace("_fold", "").replace("_heads", "")))
    try:
        if case.startswith("generator"):
            net, wr, loss, slog, blog = _product_generator(rng, case.endswith("_fold"))
        elif case.startswith("discr"):
            net, wr, loss, slog, blog = _product_discriminator(rng, not case.endswith("_heads"))
        else:
            net, wr, loss, slog, blog = _product_regressor(rng)
        got = [torch.zeros(tuple(p.shape), dtype=torch.float64) if p.grad is None else p.grad.detach().cpu().double() for p in net.weights]
    except Exception as e:                 # one product pass per case, whatever it did: the other tests of the case do not repeat it
        _results[case] = e
        raise
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in net.weights)
    # (the collapsed product rounds PRE-SUMMED class filters: its pre-activations behind a folded layer differ from those of the
    # per-tap filters by ~2^-9 of their scale, more than the margin a forced decision may have -- the oracle restates the class
    # filters, O.up_conv_same, or four activations would go unforced and every tensor below them would miss its bound by 2x)
    folded = GEN_FOLDED_CALLS if case == "generator_fold" else ()
    kw = {"class_filters": True} if folded else {}
    ref, rep, frep = Y.oracle_grads(loss, wr, stored=slog, branch=blog, **kw)
    ref_rg, rep_rg, frep_rg = Y.oracle_grads(loss, wr, stored=slog, branch=blog, round_grads=True, **kw)
    names = ["[%d] %s %s" % (i, e[0], tuple(p.shape)) for i, (e, p) in enumerate(zip(net._entries, net.weights))]
    rows = Y.grad_rows(names, got, ref, ref_rg)
    header = Y.replay_header(rep, folded) + "; decisions: %d calls forced, %d differ from the oracle's own (margin %.2e), %d unmatched" % (
        frep["forced_calls"], frep["forced_decisions"], frep["max_margin"], len(frep["unmatched"]))
    _tables[case] = Y.table(case, header, rows)
    print(_tables[case])
    path = os.environ.get("BF16_GRAD_ERRORS")
    if path:
        with open(path, "w") as f:
            f.write("# bf16 storage mode, network gradients against the float64 oracle at the product's own forward state (tests/test_bf16_grads_gpu.py)\n"
                    "# b_k: cost of bf16 storage of the gradients in the oracle itself; bound = 4 b_k + 5e-3; cosine bound 1 - bound^2 / 2\n"
                    + "\n".join(_tables[c] for c in CASES if c in _tables) + "\n")
    _results[case] = {"names": names, "got": got, "ref": ref, "ref_rg": ref_rg, "rows": rows, "rep": rep, "rep_rg": rep_rg,
                      "frep": frep, "frep_rg": frep_rg, "folded": folded, "shapes": [tuple(p.shape) for p in net.weights]}
    return _results[case]


@pytest.mark.parametrize("case", CASES)
def test_the_replay_does_not_hide_a_wrong_forward_kernel(case):
    """Per storage point: matched, <= 1 % of the elements off the oracle's own rounding, rel-L2 <= 1e-3 (behind a folded layer:
    rel-L2 <= 2^-8); every decision forced within BranchControl.force_margin = 2e-3."""
    r = _run(case)
    assert O.BranchControl.force_margin == 2e-3
    for rep, frep in ((r["rep"], r["frep"]), (r["rep_rg"], r["frep_rg"])):
        bad = Y.replay_problems(rep, r["folded"])
        assert not bad, "%s: %s" % (case, bad)
        assert not frep["unmatched"] and frep["forced_calls"] > 0, (case, frep["unmatched"][:4])
    n_points = {"generator": 15, "generator_fold": 15, "discr_r1": 20, "discr_r1_heads": 20, "regressor": 10}[case]
    assert len(r["rep"]["calls"]) == n_points


@pytest.mark.parametrize("case", CASES)
def test_bf16_network_gradients_at_the_products_forward_state(case):
    """Measured on an MI355X: profiles/bf16_grad_errors.txt."""
    r = _run(case)
    assert len(r["rows"]) >= 6
    bad = [row for row in r["rows"] if not row["ok"]]
    assert not bad, "%s: %s" % (case, ["%s: rel-L2 %.3e cos %.6f, bound %.3e (b_k %.3e)" % (b["name"], b["rel"], b["cos"], b["bound"], b["b"]) for b in bad])


@pytest.mark.parametrize("case", CASES)
def test_the_bound_is_sharp_a_filter_gradient_scaled_by_1_05_fails(case):
    r = _run(case)
    filters = [k for k, s in enumerate(r["shapes"]) if len(s) >= 4 and s[0] in (3, 4)]
    assert len(filters) == {"generator": 8, "generator_fold": 8, "discr_r1": 5, "discr_r1_heads": 5, "regressor": 5}[case]
    passed = []
    for k in filters:
        got = list(r["got"])
        got[k] = got[k] * 1.05
        row = next(row for row in Y.grad_rows(r["names"], got, r["ref"], r["ref_rg"]) if row["name"] == r["names"][k])
        if row["ok"]:
            passed.append("%s: rel-L2 %.3e within %.3e" % (row["name"], row["rel"], row["bound"]))
    assert not passed, passed

"""The instruments and the account behind tests/test_bf16_grads_gpu.py, on the oracle alone (no GPU, no product code):

* O.StoredReplay: replaying the bf16-storage oracle's own stored tensors reproduces its gradients exactly and reports share 0;
  a tampered, a missing and a surplus entry are each reported; a real / fake pair logged as one stacked tensor is matched, and so
  is a stacked oracle call whose halves were logged apart;
* the account (tests/bf16_grad_yardstick.py): on the 64 x 64 discriminator loss with R1 the bf16 gradient's distance from the fp32
  one is sensitivity to FORWARD storage -- at equal LeakyReLU decisions it is >= 8 x what bf16 storage of the gradients costs (b_k) --
  and the decisions that differ between the two oracles are under 1 % of all;
* the per-storage-point attribution of that distance (profiles/bf16_grad_attribution.txt, written when BF16_GRAD_ATTRIBUTION names
  a path)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_nets as R
from oracle import ref_ops as O
from oracle import ref_steps as S
from tests import bf16_grad_yardstick as Y

RES, N = 64, 2
FILTERS = (2, 6, 10, 14, 18)          # the five 3x3 filters in discriminator_weight_shapes order


def _trunk_weights(rng, shapes, n_blocks=5):
    """Glorot kernels; biases, gammas and betas perturbed by 0.1 as tests/test_nets_gpu.py randomize() does."""
    ws = []
    for i, s in enumerate(shapes):
        if len(s) > 1:
            w = O.glorot_uniform(rng, s)
        else:
            gamma = 2 <= i < 2 + 4 * n_blocks and (i - 2) % 4 == 2
            w = (1.0 if gamma else 0.0) + 0.1 * rng.normal(size=s)
        ws.append(torch.tensor(np.asarray(w, np.float32), dtype=torch.float64, requires_grad=True))
    return ws


@pytest.fixture(scope="module")
def dcase():
    rng = np.random.default_rng(64)
    w = _trunk_weights(rng, R.discriminator_weight_shapes(RES))
    real = torch.tensor(rng.uniform(-1, 1, size=(N, RES, RES, 3)))
    fake = torch.tensor(rng.uniform(-1, 1, size=(N, RES, RES, 3)))
    loss = lambda: S.discriminator_loss(w, real, fake)["loss_sum"]
    stored, masks = [], []
    base, _, _ = Y.oracle_grads(loss, w, recording=stored, mask_log=masks)
    return {"w": w, "loss": loss, "stored": stored, "masks": masks, "base": base}


def test_replaying_the_oracles_own_stored_tensors_reproduces_its_gradients_exactly(dcase):
    assert len(dcase["stored"]) == 20 and len(dcase["masks"]) == 10        # (conv output, block output) x 5 blocks x (real, fake)
    got, rep, frep = Y.oracle_grads(dcase["loss"], dcase["w"], stored=dcase["stored"], branch=dcase["masks"])
    assert Y.replay_problems(rep) == [] and not frep["unmatched"] and frep["forced_decisions"] == 0
    assert len(rep["calls"]) == 20 and all(c["share"] == 0.0 and c["rel"] == 0.0 for c in rep["calls"])
    for g, b in zip(got, dcase["base"]):
        assert float((g - b).abs().max()) == 0.0
    # the yardstick run (gradients rounded at every storage point) at the same state: small, and not zero
    rg, rep2, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=dcase["stored"], branch=dcase["masks"], round_grads=True)
    assert Y.replay_problems(rep2) == []
    for k in FILTERS:
        b = float((rg[k] - got[k]).norm() / got[k].norm())
        assert 2e-4 <= b <= 2e-2, (k, b)


def _bf16_step(t):
    """t (bf16-representable float64) moved to the next bf16 value away from zero."""
    bits = t.to(torch.bfloat16).view(torch.int16) + 1
    return bits.view(torch.bfloat16).to(torch.float64)


def test_a_tampered_a_missing_and_a_surplus_entry_are_each_reported(dcase):
    stored = dcase["stored"]
    # 2 % of one tensor's elements moved by one bf16 step
    j = 6
    t = stored[j].clone().reshape(-1)
    idx = torch.arange(0, t.numel(), 50)
    t[idx] = _bf16_step(t[idx])
    tampered = stored[:j] + [t.reshape(stored[j].shape)] + stored[j + 1:]
    _, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=tampered, branch=dcase["masks"])
    bad = Y.replay_problems(rep)
    assert len(bad) >= 1 and all("stored call" in b for b in bad), bad
    hit = rep["calls"][j]
    assert hit["call"] == j and hit["shape"] == tuple(stored[j].shape) and 0.019 <= hit["share"] <= 0.021 and hit["share"] > Y.SHARE_MAX and hit["rel"] > 0.0
    assert all(c["share"] == 0.0 for c in rep["calls"][:j])       # (the points behind it see another input than the logged pass did)
    assert any("differ from the oracle's own rounding" in b for b in bad)
    # a missing entry: the last call of that shape goes without one, and a gradient reaches it
    _, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=stored[:j] + stored[j + 1:], branch=dcase["masks"])
    assert len(rep["unmatched"]) == 1 and rep["unmatched"][0]["shape"] == tuple(stored[j].shape)
    assert any("found no logged tensor" in b for b in Y.replay_problems(rep))
    # a surplus entry
    _, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=stored + [stored[3].clone()], branch=dcase["masks"])
    assert not rep["unmatched"] and len(rep["leftover"]) == 1 and rep["leftover"][0]["shape"] == tuple(stored[3].shape)
    assert any("left over" in b for b in Y.replay_problems(rep))
    # nothing logged at all
    _, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=[], branch=dcase["masks"])
    assert len(rep["unmatched"]) == 20 and Y.replay_problems(rep)


def test_a_real_fake_pair_logged_as_one_stacked_tensor_is_matched_and_the_other_way_round(dcase):
    stored = dcase["stored"]
    stacked = [torch.cat([stored[j], stored[10 + j]], dim=0) for j in range(10)]
    got, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=stacked, branch=dcase["masks"])
    assert Y.replay_problems(rep) == [] and len(rep["calls"]) == 20 and all(c["share"] == 0.0 for c in rep["calls"])
    for g, b in zip(got, dcase["base"]):
        assert float((g - b).abs().max()) == 0.0
    # swapped halves are NOT matched silently: the values of the fake pass arrive at the real pass's calls
    swapped = [torch.cat([stored[10 + j], stored[j]], dim=0) for j in range(10)]
    _, rep, _ = Y.oracle_grads(dcase["loss"], dcase["w"], stored=swapped, branch=dcase["masks"])
    assert Y.replay_problems(rep)
    # the other way round: one stacked oracle call, its sample blocks logged by two separate passes (instance statistics are per
    # sample, so the halves' values are the stack's)
    rng = np.random.default_rng(5)
    w = _trunk_weights(rng, R.latent_regressor_weight_shapes(13, RES))
    img = torch.tensor(rng.uniform(-1, 1, size=(2 * N, RES, RES, 3)))
    cot = torch.tensor(rng.normal(size=(2 * N, 16)))
    halves, whole = [], []
    for h in range(2):
        Y.oracle_grads(lambda: (R.latent_regressor_forward(w, img[h * N:(h + 1) * N]) * cot[h * N:(h + 1) * N]).sum(), w, recording=halves)
    loss = lambda: (R.latent_regressor_forward(w, img) * cot).sum()
    base, _, _ = Y.oracle_grads(loss, w, recording=whole)
    assert len(halves) == 20 and len(whole) == 10
    got, rep, _ = Y.oracle_grads(loss, w, stored=halves)
    assert Y.replay_problems(rep) == [] and len(rep["calls"]) == 10 and max(c["share"] for c in rep["calls"]) <= 1e-4
    for g, b in zip(got, base):
        assert float((g - b).norm()) <= 1e-3 * float(b.norm())


@pytest.mark.parametrize("xs,ws", [((2, 5, 6, 16), (4, 4, 16, 8)), ((1, 3, 4, 5, 8), (3, 3, 3, 8, 16)), ((1, 4, 4, 8), (3, 3, 8, 8)), ((1, 4, 5, 8), (2, 2, 8, 8))])
def test_class_filter_form_of_upsample_plus_convolution_is_an_identity(xs, ws):
    """O.up_conv_classes (what the oracle evaluates for the collapsed product) against conv_same(upsample2(x)): values and both
    gradients to float64 rounding; with rounded class filters it stays within bf16 filter rounding of it, and differs from the
    per-tap rounding (else the restatement would be idle)."""
    g = torch.Generator().manual_seed(sum(ws))
    x = torch.randn(xs, dtype=torch.float64, generator=g).requires_grad_(True)
    w = torch.randn(ws, dtype=torch.float64, generator=g).requires_grad_(True)
    b = torch.randn(ws[-1], dtype=torch.float64, generator=g)
    a, c = O.conv_same(O.upsample2(x), w, b), O.up_conv_classes(x, w, b)
    assert float((a - c).detach().abs().max()) <= 1e-12 * float(a.detach().abs().max())
    cot = torch.randn(a.shape, dtype=torch.float64, generator=g)
    ga = torch.autograd.grad((a * cot).sum(), [x, w], retain_graph=True)
    for p, q in zip(ga, torch.autograd.grad((c * cot).sum(), [x, w])):
        assert float((p - q).abs().max()) <= 1e-12 * float(p.abs().max())
    assert torch.equal(O.up_conv_same(x, w, b), a)
    with O.bf16_storage(class_filters=True):
        d = O.up_conv_same(x, w, b)
        gd = torch.autograd.grad((d * cot).sum(), w)[0]
    with O.bf16_storage():
        e = O.up_conv_same(x, w, b)
    rel = lambda u, v: float((u - v).detach().norm() / v.detach().norm())
    assert 1e-4 < rel(d, a) <= 2.0 ** -8 and 1e-4 < rel(d, e) <= 2.0 ** -7
    assert rel(gd, ga[1]) <= 1e-12                   # (straight-through: the derivative w.r.t. the taps is the exact sum's)


def _decisions(masks):
    return torch.cat([m[1].reshape(-1) for m in masks])


def test_the_account_forward_storage_dominates_and_decisions_are_a_minor_part(dcase):
    """Measured (this file's case): plain against bf16-storage oracle at equal decisions 0.070 - 0.074 over the five filters (0.073 -
    0.090 with the decisions free), b_k 2.1e-3 - 5.3e-3: ratio 13 - 33; 212 of 376 832 decisions differ (0.056 %)."""
    w, loss, masks = dcase["w"], dcase["loss"], dcase["masks"]
    own = []
    Y.oracle_grads(loss, w, storage=False, mask_log=own)
    a, b = _decisions(own), _decisions(masks)
    assert a.numel() == b.numel() == 2 * N * sum(c * (RES >> (i + 1)) ** 2 for i, c in enumerate(R.discr_channels()))
    differ = float((a != b).double().mean())
    # the bf16-storage oracle's decisions forced into both (a decision of the plain pass may move wherever storage rounding moved
    # the input across zero: far beyond the fp32 margin the GPU comparisons allow)
    margin, O.BranchControl.force_margin = O.BranchControl.force_margin, 1.0
    try:
        plain, _, frep = Y.oracle_grads(loss, w, storage=False, branch=masks)
    finally:
        O.BranchControl.force_margin = margin
    assert not frep["unmatched"] and frep["forced_calls"] == 10 and frep["forced_decisions"] > 0
    free, _, _ = Y.oracle_grads(loss, w, storage=False)
    rg, _, _ = Y.oracle_grads(loss, w, branch=masks, round_grads=True)
    base = dcase["base"]
    print("decisions that differ between the plain and the bf16-storage oracle: %d of %d (%.3e)" % (int((a != b).sum()), a.numel(), differ))
    for k in FILTERS:
        fwd = float((base[k] - plain[k]).norm() / plain[k].norm())
        fwd_free = float((base[k] - free[k]).norm() / free[k].norm())
        bk = float((rg[k] - base[k]).norm() / base[k].norm())
        print("filter %2d %-18s forward storage at equal decisions %.3e, decisions free %.3e, b_k %.3e, ratio %.1f" % (k, tuple(w[k].shape), fwd, fwd_free, bk, fwd / bk))
        assert fwd >= 8.0 * bk, (k, fwd, bk)
    assert differ < 1e-2


def test_per_storage_point_attribution_of_the_bf16_gradient_distance(dcase):
    """Column j: the change of each filter's gradient with storage point j alone rounded (exact filters, the plain oracle's
    decisions forced); `filters`: the bf16 filters alone; their root sum of squares beside the all-points figure.  The parts do
    NOT add up: single points of the fourth block (4 x 4 extent, 16 values per instance statistic) move the gradients by more than
    all points together (0.14 against 0.12), the root sum of squares is twice the whole -- the response to a perturbation of 2^-9
    is already past its linear range there.  The table is a reading aid for where the sensitivity sits; what is asserted is that
    the parts explain at least the whole and that the real pass (the one under the R1 term) carries it."""
    w, loss = dcase["w"], dcase["loss"]
    own = []
    plain, _, _ = Y.oracle_grads(loss, w, storage=False, mask_log=own)
    margin, O.BranchControl.force_margin = O.BranchControl.force_margin, 1.0
    try:
        whole, _, _ = Y.oracle_grads(loss, w, branch=own)
        cols = [Y.oracle_grads(loss, w, branch=own, only_point=j, filters=False)[0] for j in range(20)]
        cols.append(Y.oracle_grads(loss, w, branch=own, only_point=-1)[0])
    finally:
        O.BranchControl.force_margin = margin
    names = ["%s b%d %s" % ("real" if j < 10 else "fake", (j % 10) // 2, "conv" if j % 2 == 0 else "norm") for j in range(20)] + ["filters"]
    rel = lambda g, k: float((g[k] - plain[k]).norm() / plain[k].norm())
    lines = ["# bf16-storage oracle against the plain float64 oracle, 64 x 64 discriminator loss with R1, n = 2, the plain oracle's LeakyReLU",
             "# decisions forced: relative L2 change of each 3x3 filter's gradient with ONE storage point rounded (tests/test_bf16_grad_yardstick_cpu.py)",
             "# %-16s" % "storage point" + "".join(" %11s" % ("block%d" % i) for i in range(5))]
    for name, g in zip(names, cols):
        lines.append("  %-16s" % name + "".join(" %11.3e" % rel(g, k) for k in FILTERS))
    rss = [float(np.sqrt(sum(rel(g, k) ** 2 for g in cols))) for k in FILTERS]
    allp = [rel(whole, k) for k in FILTERS]
    lines.append("  %-16s" % "root sum of sq." + "".join(" %11.3e" % v for v in rss))
    lines.append("  %-16s" % "all points" + "".join(" %11.3e" % v for v in allp))
    text = "\n".join(lines)
    print(text)
    path = os.environ.get("BF16_GRAD_ATTRIBUTION")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
    for r, a in zip(rss, allp):
        assert np.isfinite(r) and r >= 0.5 * a, (r, a)
    # the fake pass carries no R1 term: each of its storage points moves the gradients by 1e-4 at the most, the real pass's by 1e-1
    for k in FILTERS:
        assert 100.0 * max(rel(cols[j], k) for j in range(10, 20)) < max(rel(cols[j], k) for j in range(10))

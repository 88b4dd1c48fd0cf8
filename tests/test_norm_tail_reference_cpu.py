"""Pins the float64 reference of the R1 tangent tail (tests/norm_tail_ref.py) on the CPU: its Jacobian-vector product and the
three gradients of L = <h, ty> + <u, tstyle> against central finite differences of the LAYER (tail) itself.  The GPU tests
(tests/test_norm_tails_gpu.py) hold the HIP kernels to this reference, so it must not share a mistake with them."""
import numpy as np
import torch

from tests import norm_tail_ref as NR

SHAPE = (2, 5, 7, 6)
STEP = 1e-6
BOUND = 1e-6          # relative to each quantity's maximum


def _inputs(seed=7):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    n, c = SHAPE[0], SHAPE[-1]
    x, tx, h = f(*SHAPE) * 1.5 + 0.2, f(*SHAPE), f(*SHAPE)
    u = f(n, 2 * c)
    gamma, beta = (1.0 + 0.5 * f(c)), 0.1 * f(c)
    return x, tx, gamma, beta, h, u


def _jvp_fd(x, tx, gamma, beta):
    """(tail(x + e tx) - tail(x - e tx)) / 2e in float64.  No element of x is within e |tx| of the LeakyReLU kink (asserted)."""
    x64, tx64, g64, b64 = (NR.tt(t) for t in (x, tx, gamma, beta))
    assert float((x64.abs() - 10 * STEP * tx64.abs()).min()) > 0
    yp, sp = NR.tail(x64 + STEP * tx64, g64, b64)
    ym, sm = NR.tail(x64 - STEP * tx64, g64, b64)
    return (yp - ym) / (2 * STEP), (sp - sm) / (2 * STEP)


def test_tangent_tail_jvp_matches_central_differences_of_the_layer():
    x, tx, gamma, beta, h, u = _inputs()
    ref = NR.tangent_tail_grads(x, tx, gamma, beta, h, u)
    ty_fd, ts_fd = _jvp_fd(x, tx, gamma, beta)
    assert NR.rel_err(ty_fd, ref["ty"]) <= BOUND
    assert NR.rel_err(ts_fd, ref["tstyle"]) <= BOUND


def _loss(x, tx, gamma, beta, h, u):
    """L = <h, ty> + <u, tstyle> as a plain float64 number, from the autograd JVP (pinned above)."""
    with torch.enable_grad():
        ty, ts = NR.tangent_tail(NR.tt(x), NR.tt(tx), NR.tt(gamma), NR.tt(beta))
    return float((ty.detach() * NR.tt(h)).sum() + (ts.detach() * NR.tt(u)).sum())


def _fd_grad(args, which):
    """Central differences of L w.r.t. every element of args[which] (float64 perturbations of the float32-drawn inputs)."""
    base = [np.asarray(a, np.float64) for a in args]
    g = np.zeros_like(base[which])
    flat = g.reshape(-1)
    for i in range(flat.size):
        p = [a.copy() for a in base]
        m = [a.copy() for a in base]
        p[which].reshape(-1)[i] += STEP
        m[which].reshape(-1)[i] -= STEP
        flat[i] = (_loss(*p) - _loss(*m)) / (2 * STEP)
    return NR.tt(g)


def test_tangent_tail_gradients_match_central_differences():
    x, tx, gamma, beta, h, u = _inputs()
    assert float(np.abs(x).min()) > 10 * STEP            # no perturbation crosses the LeakyReLU kink
    ref = NR.tangent_tail_grads(x, tx, gamma, beta, h, u)
    args = (x, tx, gamma, beta, h, u)
    for name, which in (("g_x", 0), ("g_tx", 1), ("g_gamma", 2)):
        err = NR.rel_err(_fd_grad(args, which), ref[name])
        assert err <= BOUND, "%s: finite differences differ by %.3e of its maximum" % (name, err)
    assert float(ref["g_x"].abs().max()) > 0.1          # the second-order term is not a small quantity here


def test_batched_reference_is_the_sum_of_its_heads_and_one_head_alone_reduces_to_the_single_statement():
    x, tx, gamma, beta, h, u = _inputs()
    rng = np.random.default_rng(8)
    n = SHAPE[0]
    txs = np.concatenate([tx] + [rng.normal(size=SHAPE).astype(np.float32) for _ in range(2)])
    hs = np.concatenate([h, rng.normal(size=SHAPE).astype(np.float32)])
    ref = NR.tangent_tail_batched_grads(x, txs, gamma, beta, hs, u)
    assert ref["ty"].shape[0] == 2 * n and ref["g_tx"].shape[0] == 3 * n and ref["tstyle"].shape == (n, 2 * SHAPE[-1])
    r0 = NR.tangent_tail_grads(x, txs[:n], gamma, beta, None, u)
    r1 = NR.tangent_tail_grads(x, txs[n:2 * n], gamma, beta, hs[:n], None)
    r2 = NR.tangent_tail_grads(x, txs[2 * n:], gamma, beta, hs[n:], None)
    assert torch.equal(ref["g_x"], r0["g_x"] + r1["g_x"] + r2["g_x"])
    assert torch.equal(ref["g_gamma"], r1["g_gamma"] + r2["g_gamma"])
    assert torch.equal(ref["g_tx"], torch.cat([r0["g_tx"], r1["g_tx"], r2["g_tx"]]))
    assert float(r0["g_gamma"].abs().max()) == 0.0       # the style statistics do not see gamma


def test_float32_yardstick_is_small_and_not_zero():
    x, tx, gamma, beta, h, u = _inputs()
    _, yard = NR.yardstick(lambda dt: NR.tangent_tail_grads(x, tx, gamma, beta, h, u, dtype=dt))
    for k, v in yard.items():
        assert 1e-9 < v < 1e-5, (k, v)

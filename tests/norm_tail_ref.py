"""float64 torch-CPU statements of the normalisation tails, written from the LAYERS' definitions (never from the kernels'
coefficient algebra), with every derivative taken by autograd:

  * tail(x): the tail of DiscrBlock.call (building_blocks.py:100-106): style = [mean_s x | sqrt(var_s x + 1e-6)],
    l = LeakyReLU(x), y = (l - mean l) / (std l + 1e-3) gamma + beta;
  * tangent_tail(...): (ty, tstyle) = the Jacobian-vector product of tail at x in direction tx, L = <h, ty> + <u, tstyle>, and
    dL/dtx, dL/dx, dL/dgamma -- what DualTailFn / DualTailBatchedFn and their backward passes compute for the R1 penalty;
  * adain(x, sb): AdaIn.call (building_blocks.py:135-149);
  * channel_affine_act: BatchNormalization (inference) folded to a per-channel affine, optional residual and ReLU.

Every function takes a `dtype`: torch.float64 is the reference, torch.float32 is the YARDSTICK -- the same statement evaluated
by torch on the CPU in the kernels' number format.  Its distance from the float64 run says what fp32 arithmetic costs for this
operation on these inputs; the kernels are held to a fixed multiple of it (tests/test_norm_tails_gpu.py).

Inputs are expected to be float32-representable (drawn in float32): the LeakyReLU / ReLU decisions of the float64 run, the
float32 run and the product are then the same decisions."""
import numpy as np
import torch

from oracle import ref_ops as O

SLOPE = 0.3          # keras LeakyReLU() default, the DiscrBlock's


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def rel_err(got, ref):
    """max |got - ref| / max |ref|: relative to the quantity's OWN maximum, without a clamp to 1."""
    got = got.detach().cpu().double() if torch.is_tensor(got) else tt(got)
    ref = ref.detach().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    scale = float(ref.abs().max())
    return float((got - ref).abs().max()) / (scale if scale > 0.0 else 1.0)      # (an identically zero reference: the absolute error)


def tail(x, gamma, beta, slope=SLOPE):
    """(y, style (N, 2C)) of the DiscrBlock tail."""
    n, c = x.shape[0], x.shape[-1]
    mu, sd = O.layer_style(x)
    style = torch.cat([mu.reshape(n, c), sd.reshape(n, c)], dim=1)
    y = O.instance_norm(O.leaky_relu(x, slope), gamma, beta)
    return y, style


def tail_grads(x, gamma, beta, gy, gstyle, slope=SLOPE, dtype=torch.float64):
    """First-order tail: y, style and the gradients of <gy, y> + <gstyle, style> (either cotangent may be None)."""
    xr = tt(x, dtype).requires_grad_(True)
    gr, br = tt(gamma, dtype).requires_grad_(True), tt(beta, dtype).requires_grad_(True)
    y, style = tail(xr, gr, br, slope)
    loss = 0.0
    if gy is not None:
        loss = loss + (y * tt(gy, dtype)).sum()
    if gstyle is not None:
        loss = loss + (style * tt(gstyle, dtype)).sum()
    g = torch.autograd.grad(loss, (xr, gr, br), allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    return {"y": y.detach(), "style": style.detach(), "g_x": z(g[0], xr), "g_gamma": z(g[1], gr), "g_beta": z(g[2], br)}


def tangent_tail(x, tx, gamma, beta, slope=SLOPE):
    """(ty, tstyle) with the graph kept: the JVP of tail at x in direction tx."""
    fn = lambda x_: tail(x_, gamma, beta, slope)
    return torch.autograd.functional.jvp(fn, x, tx, create_graph=True)[1]


def tangent_tail_grads(x, tx, gamma, beta, h, u, slope=SLOPE, dtype=torch.float64):
    """One head: ty, tstyle and the gradients of L = <h, ty> + <u, tstyle> w.r.t. tx, x and gamma (h or u may be None; beta
    does not enter a tangent).  g_x consists of second-order terms only: it is zero if the statistics are held constant."""
    xr, txr = tt(x, dtype).requires_grad_(True), tt(tx, dtype).requires_grad_(True)
    gr, br = tt(gamma, dtype).requires_grad_(True), tt(beta, dtype)
    ty, tstyle = tangent_tail(xr, txr, gr, br, slope)
    out = {"ty": ty.detach(), "tstyle": tstyle.detach()}
    loss = 0.0
    if h is not None:
        loss = loss + (ty * tt(h, dtype)).sum()
    if u is not None:
        loss = loss + (tstyle * tt(u, dtype)).sum()
    if h is None and u is None:
        return out
    g = torch.autograd.grad(loss, (txr, xr, gr), allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    out.update(g_tx=z(g[0], txr), g_x=z(g[1], xr), g_gamma=z(g[2], gr))
    return out


def tangent_tail_batched_grads(x, tx, gamma, beta, h, u, slope=SLOPE, dtype=torch.float64):
    """The stacked tangent pass of DualTailBatchedFn as the SUM OVER HEADS of the single-head statement: tx holds
    (1 + k) N samples head-major; head 0 leaves through the style statistics (cotangent u (N, 2C)), heads 1..k go on through
    LeakyReLU + instance norm (cotangent h, k N samples).  Sample j of a head pairs with x[j]."""
    n = np.asarray(x).shape[0]
    tx, h = np.asarray(tx), (None if h is None else np.asarray(h))
    k = tx.shape[0] // n - 1
    r0 = tangent_tail_grads(x, tx[:n], gamma, beta, None, u, slope, dtype)
    out = {"tstyle": r0["tstyle"], "ty": [], "g_tx": [r0["g_tx"]] if u is not None else [torch.zeros_like(tt(tx[:n], dtype))]}
    g_x = r0["g_x"].clone() if u is not None else torch.zeros_like(tt(x, dtype))
    g_gamma = torch.zeros_like(tt(gamma, dtype))
    for j in range(1, k + 1):
        hj = None if h is None else h[(j - 1) * n:j * n]
        r = tangent_tail_grads(x, tx[j * n:(j + 1) * n], gamma, beta, hj, None, slope, dtype)
        out["ty"].append(r["ty"])
        if hj is not None:
            out["g_tx"].append(r["g_tx"])
            g_x += r["g_x"]
            g_gamma += r["g_gamma"]
        else:
            out["g_tx"].append(torch.zeros_like(r["ty"]))
    out["ty"] = torch.cat(out["ty"])
    out["g_tx"] = torch.cat(out["g_tx"])
    out["g_x"], out["g_gamma"] = g_x, g_gamma
    return out


def adain(x, sb, eps=1e-3):
    """AdaIn.call: layer normalisation over the spatial axes (eps inside the root, no affine), then x (s + 1) + b with
    sb (N, 2C) = [s | b]."""
    n, c = x.shape[0], x.shape[-1]
    axes = tuple(range(1, x.dim() - 1))
    bc = (n,) + (1,) * len(axes) + (c,)
    mu = x.mean(dim=axes, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=axes, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * (sb[:, :c].reshape(bc) + 1.0) + sb[:, c:].reshape(bc)


def adain_grads(x, sb, gy, dtype=torch.float64):
    xr, sbr = tt(x, dtype).requires_grad_(True), tt(sb, dtype).requires_grad_(True)
    y = adain(xr, sbr)
    g_x, g_sb = torch.autograd.grad((y * tt(gy, dtype)).sum(), (xr, sbr))
    return {"y": y.detach(), "g_x": g_x, "g_sb": g_sb}


def channel_affine_act_grads(x, a, b, res, relu, gy, dtype=torch.float64):
    """y = relu?(x a[c] + b[c] (+ res)) and the gradients of <gy, y>."""
    xr, ar, br = (tt(t, dtype).requires_grad_(True) for t in (x, a, b))
    rr = None if res is None else tt(res, dtype).requires_grad_(True)
    y = xr * ar + br
    if rr is not None:
        y = y + rr
    if relu:
        y = O.relu(y)
    ins = (xr, ar, br) + ((rr,) if rr is not None else ())
    g = torch.autograd.grad((y * tt(gy, dtype)).sum(), ins)
    out = {"y": y.detach(), "g_x": g[0], "g_a": g[1], "g_b": g[2]}
    if rr is not None:
        out["g_res"] = g[3]
    return out


def yardstick(fn, keys=None):
    """fn(dtype) -> dict of tensors.  Returns (ref64, {key: rel. error of the float32 run against the float64 run})."""
    r64, r32 = fn(torch.float64), fn(torch.float32)
    return r64, {k: rel_err(r32[k], r64[k]) for k in (keys or r64.keys())}

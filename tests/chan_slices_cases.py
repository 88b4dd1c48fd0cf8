"""What tests/test_chan_slices_plan_cpu.py, tests/test_dwconv_bwd_gpu.py and tests/test_bn_train_edges_gpu.py share: the slice rule
of the per-channel training reductions written out once more in Python, the shapes its recorded plans cover, and the guarded
output tensor of the two GPU files.

dw_wgrad_plan() and bn_bwd_plan() are TRANSCRIPTIONS of the two functions of those names that csrc/depthwise.hip and
csrc/bn_train.hip carried before csrc/chan_slices.h existed, statement by statement: tests/golden/chan_slices_plans.json was written
from them (python -m tests.chan_slices_cases), never from cn_chan_slices_plan, and its slice counts were checked against
cn_dwconv3x3_wgrad_slices / cn_bn_train_bwd_slices of the library built from those two files."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chan_slices_plans.json")
FIELDS = ["rows", "c", "min_rows", "TX", "TY", "cb", "slices", "per_slice"]
DW_MIN_ROWS, BN_MIN_ROWS = 64, 0                         # the floor each caller hands to chan_slices_plan

# the shapes of tests/test_dwconv_bwd_gpu.py (n, h, w, c; both strides) and the reduce shapes of tests/test_bn_train_edges_gpu.py (rows, c)
DW_EDGE_SHAPES = [(1, 1, 1, 4), (2, 5, 7, 8), (3, 8, 6, 6), (1, 9, 9, 32), (2, 4, 4, 960), (2, 33, 17, 8), (2, 33, 33, 8), (1, 5, 5, 70)]
BN_REDUCE_SHAPES = [(60, 8), (37, 6), (512, 96), (1000, 260), (16, 1280), (37, 70)]
# channel groups on both sides of every boundary of TX (a power of two up to 64) and of the channel blocks (64 groups each)
BOUNDARY_CGS = [1, 2, 63, 64, 65, 128, 129]


def cdiv(a, b):
    return (a + b - 1) // b


def cgs_of(c):
    """channel groups: 4 channels per lane where c % 4 == 0, else 1"""
    return c // 4 if c % 4 == 0 else c


def dw_wgrad_plan(pixels, cgs):
    """[TX, TY, channel blocks, slices, pixels per slice]: DwWgradPlan dw_wgrad_plan(long pixels, int cgs)"""
    tx = 1
    while tx < cgs and tx < 64:
        tx *= 2
    ty = 256 // tx
    cb = cdiv(cgs, tx)
    min_px = 4 * ty if 4 * ty > 64 else 64
    slices = (pixels + min_px - 1) // min_px
    cap = 1024 // cb if 1024 // cb > 1 else 1
    if slices > cap:
        slices = cap
    per_slice = (pixels + slices - 1) // slices
    return [tx, ty, cb, (pixels + per_slice - 1) // per_slice, per_slice]


def bn_bwd_plan(m, cgs):
    """[TX, TY, channel blocks, slices, rows per slice]: BnPlan bn_bwd_plan(long m, int cgs)"""
    tx = 1
    while tx < cgs and tx < 64:
        tx *= 2
    ty = 256 // tx
    cb = cdiv(cgs, tx)
    slices = (m + 4 * ty - 1) // (4 * ty)
    cap = 1024 // cb if 1024 // cb > 1 else 1
    if slices > cap:
        slices = cap
    per_slice = (m + slices - 1) // slices
    return [tx, ty, cb, (m + per_slice - 1) // per_slice, per_slice]


def transcribed_plan(rows, c, min_rows):
    """what the caller with this floor got before the rule was shared"""
    return {DW_MIN_ROWS: dw_wgrad_plan, BN_MIN_ROWS: bn_bwd_plan}[min_rows](rows, cgs_of(c))


def dw_pixels(n, h, w, c, stride):
    return n * cdiv(h, stride) * cdiv(w, stride)


def mobilenet_layers(size, batch):
    """([(n, h, w, c, stride)] of the depthwise layers, [(rows, c)] of the BatchNormalization layers) of MobileNetV2"""
    from confignet_amd.metrics.mobilenet_v2 import mobilenet_v2_graph
    shapes, dw, bn = {}, [], []
    for name, kind, ins, p in mobilenet_v2_graph():
        if kind == "input":
            shapes[name] = (batch, size, size, 3)
        elif kind in ("conv", "dw"):
            n, h, w, c = shapes[ins[0]]
            s = p["stride"]
            shapes[name] = (n, cdiv(h, s), cdiv(w, s), p["filters"] if kind == "conv" else c)
            if kind == "dw":
                dw.append((n, h, w, c, s))
        else:
            shapes[name] = shapes[ins[0]]
            if kind == "bn":
                n, h, w, c = shapes[name]
                bn.append((n * h * w, c))
    return dw, bn


def boundary_requests():
    """(rows, c, min_rows) on both sides of every boundary of the rule: the 4 TY rows per lane, the depthwise floor of 64, and the
    row count at which the cap of 1024 workgroups starts to bind -- for every BOUNDARY_CGS with c % 4 == 0 (c = 4 cgs) and, where
    such a c exists, with c % 4 != 0 (c = cgs: not for 64 and 128 groups)"""
    out = []
    for cgs in BOUNDARY_CGS:
        for c in [4 * cgs] + ([cgs] if cgs % 4 else []):
            tx, ty, cb = dw_wgrad_plan(1, cgs)[:3]
            cap = max(1024 // cb, 1)
            for min_rows in (DW_MIN_ROWS, BN_MIN_ROWS):
                floor = max(4 * ty, min_rows)
                for rows in (4 * ty - 1, 4 * ty, 4 * ty + 1, 63, 64, 65, cap * floor - 1, cap * floor, cap * floor + 1):
                    out.append((rows, c, min_rows))
    return out


def golden_requests(dw_layers, bn_layers):
    """every (rows, c, min_rows) the recorded plans hold, in order, without repeats"""
    reqs = [(dw_pixels(*s), s[3], DW_MIN_ROWS) for s in dw_layers] + [(m, c, BN_MIN_ROWS) for m, c in bn_layers] + boundary_requests()
    seen, out = set(), []
    for r in reqs:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


# ---- the guarded output of the two GPU files ------------------------------------------------------------------------------------
GUARD, GUARD_VALUE = 256, 12345.0
NAN = float("nan")


def to_device(a):
    """a NumPy array or a tensor as a contiguous fp32 tensor on the GPU"""
    import torch
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.float().cuda().contiguous()


class Guarded:
    """a contiguous fp32 tensor of `shape` inside a larger allocation with sentinels on both sides, holding `fill` (a number or a
    tensor of that shape; NaN: what a call must write)"""

    def __init__(self, shape, fill=NAN):
        import torch
        k = int(np.prod(shape))
        self.buf = torch.full((k + 2 * GUARD,), GUARD_VALUE, device="cuda", dtype=torch.float32)
        self.t = self.buf[GUARD:GUARD + k].view(shape)
        if isinstance(fill, float):
            self.t.fill_(fill)
        else:
            self.t.copy_(fill)

    def check(self, want, what):
        """the guards are untouched and the tensor equals `want` (float64, NumPy or torch) element for element"""
        import torch
        edge = torch.full((GUARD,), GUARD_VALUE, device="cuda")
        assert torch.equal(self.buf[:GUARD], edge) and torch.equal(self.buf[-GUARD:], edge), what + ": a guard was written"
        want = want if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
        got, want = self.t.double().cpu(), want.reshape(self.t.shape)
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i = tuple(bad[0].tolist())
            raise AssertionError("%s: %d of %d elements wrong, first at %s: got %r, want %r" % (what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


class GuardedBuf:
    """`numel` elements of `dtype` inside a larger allocation of sentinel floats (Guarded for fp32, bf16 and uint8 views,
    and for inputs), starting `off` elements past a vector boundary; holds `data` (an input, or an accumulator's preset) or `fill`"""

    def __init__(self, numel, dtype=None, off=0, data=None, fill=NAN):
        import torch
        dtype = dtype or torch.float32
        item = torch.empty((), dtype=dtype).element_size()
        self.numel, self.dtype, self.off = int(numel), dtype, off
        self.floats = ((self.numel + off + 8) * item + 3) // 4
        self.buf = torch.full((self.floats + 2 * GUARD,), GUARD_VALUE, device="cuda", dtype=torch.float32)
        self.t = self._payload(self.buf)
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dtype))
        else:
            self.t.fill_(fill)
        self.before = self.buf.clone()
        assert (self.t.data_ptr() - off * item) % 16 == 0

    def _payload(self, buf):
        return buf[GUARD:GUARD + self.floats].view(self.dtype)[self.off:self.off + self.numel]

    @property
    def ptr(self):
        return self.t.data_ptr()

    def unchanged(self):
        """bit for bit what it held before the call, sentinels included"""
        import torch
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))

    def intact(self):
        """everything around the tensor is what it was"""
        import torch
        cur = self.buf.clone()
        self._payload(cur).copy_(self._payload(self.before))
        return torch.equal(cur.view(torch.int32), self.before.view(torch.int32))

    def values(self):
        return self.t.double().cpu().numpy()

    def check(self, want, what):
        assert self.intact(), what + ": written outside the tensor"
        got, want = self.values(), np.asarray(want, np.float64).reshape(-1)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(~(got == want))
            raise AssertionError("%s: %d of %d elements wrong, first at %d: got %r, want %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


if __name__ == "__main__":
    dw_layers, bn_layers = [], []
    for batch in (32, 1):
        dw, bn = mobilenet_layers(256, batch)
        dw_layers += dw
        bn_layers += bn
    n_net = (len(dw_layers), len(bn_layers))
    dw_layers += [s + (stride,) for s in DW_EDGE_SHAPES for stride in (1, 2)]
    bn_layers += BN_REDUCE_SHAPES
    doc = {"about": "Slice plans of the per-channel training reductions (cn_dwconv3x3_wgrad, cn_bn_train_bwd_reduce), RECORDED from the two "
                    "functions dw_wgrad_plan (csrc/depthwise.hip) and bn_bwd_plan (csrc/bn_train.hip) as they stood before csrc/chan_slices.h, as "
                    "tests/chan_slices_cases.py transcribes them.  dw_layers (n, h, w, c, stride): the %d depthwise layers of MobileNetV2 at 256 x 256, "
                    "batch 32 and batch 1, then the shapes of tests/test_dwconv_bwd_gpu.py at both strides; bn_layers (rows, c): its %d "
                    "BatchNormalization layers, then the reduce shapes of tests/test_bn_train_edges_gpu.py; then both sides of every boundary of "
                    "the rule (tests/chan_slices_cases.py: boundary_requests)." % n_net,
           "fields": FIELDS,
           "dw_layers": [list(s) for s in dw_layers],
           "bn_layers": [list(s) for s in bn_layers],
           "plans": [list(r) + transcribed_plan(*r) for r in golden_requests(dw_layers, bn_layers)]}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v) if k != "plans" else "[\n  " + ",\n  ".join(json.dumps(p) for p in v) + "\n ]")
                                   for k, v in doc.items()) + "\n}\n")
    print("wrote %d plans" % len(doc["plans"]))

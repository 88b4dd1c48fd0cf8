"""Raw (non-differentiable) wrappers: torch CUDA tensors in, C-ABI call on the current HIP
stream, torch tensors out.  torch only allocates memory and provides the stream here."""
import contextlib
import ctypes
import math
import os
import threading

import torch

from ._lib import CN_BF16, CN_EUNSUPPORTED, CN_F32, CN_U8, CnConvGeom, CnDepthJob, CnGanJob, CnRowsJob, CnSumJob, check, lib

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH, ACT_RELU6, ACT_SIGMOID = 0, 1, 2, 3, 4, 5

# Storage type of ACTIVATION tensors (channels-last tensors with more than 4 channels).  fp32 is the reference's arithmetic
# (BASELINE.json configs[1]); bf16 is configs[2]: bf16 activations and bf16 filter copies on v_mfma_f32_32x32x16_bf16 with
# fp32 accumulation, while 3-channel images, (N, F) latent-sized tensors, statistics, coefficients, losses, master weights,
# their gradients and the optimizer state stay fp32.
ACT_DTYPE = torch.float32


def set_activation_dtype(dtype):
    """dtype: torch.float32 / torch.bfloat16 (or "f32" / "bf16").  Process-wide; switch only between steps."""
    global ACT_DTYPE
    if isinstance(dtype, str):
        dtype = {"f32": torch.float32, "fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16,
                 "bfloat16": torch.bfloat16}[dtype]
    assert dtype in (torch.float32, torch.bfloat16)
    ACT_DTYPE = dtype


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Deterministic mode (CN_DETERMINISTIC=1 or set_deterministic(True); include/confignet_hip.h: cn_set_deterministic): every
# reduction in a fixed order instead of fp32 atomics, in fp32 and in bf16 storage (set_activation_dtype: the bf16 filter gradient
# adds its row slices' slabs in slice order) -- two runs on the same inputs are bit-identical.  Also
# switches off what reorders ADDS between streams: the generator step's fork (both branches add into the generator's slots).
DETERMINISTIC = False


def set_deterministic(on=True):
    global DETERMINISTIC
    check(lib.cn_set_deterministic(int(bool(on))), "cn_set_deterministic")
    DETERMINISTIC = bool(on)


def _partial_rows(rows):
    """Partial rows of a per-channel reduction over `rows` rows: every workgroup ends in one atomic per channel, so a long
    reduction is spread over partial rows (as if they were samples) that are added afterwards."""
    if rows < 8192:
        return 1
    return next(r for r in (16, 8, 4, 2, 1) if rows % r == 0)


def _spread(x):
    """(rep, s, c): x (..., c) seen as `rep` partial rows (_partial_rows) of s rows each."""
    c = x.shape[-1]
    rows = x.numel() // c
    rep = _partial_rows(rows)
    return rep, rows // rep, c


def _readd(t, rep, dim):
    """The partial rows of _spread (axis `dim` of t, kept with extent 1) added again."""
    return t.sum(dim, keepdim=True) if rep > 1 else t


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype in (torch.float32, torch.bfloat16, torch.uint8, torch.int64, torch.int32, torch.int16) and t.is_contiguous(), \
        "confignet_amd ops need contiguous CUDA tensors (got %s %s contiguous=%s)" % (t.device, t.dtype, t.is_contiguous())
    return ctypes.c_void_p(t.data_ptr())


def _fptr(t):
    """Pointer of a tensor the ABI declares as float*."""
    assert t is None or t.dtype == torch.float32, "fp32 tensor expected, got %s" % (t.dtype,)
    return _ptr(t)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _dt(t):
    return CN_BF16 if t.dtype == torch.bfloat16 else CN_F32


def cast(x, dtype):
    """Storage-type conversion fp32 <-> bf16 (round to nearest even) by a HIP kernel."""
    if x.dtype == dtype:
        return x
    x = _c(x)
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    check(lib.cn_cast(_ptr(x), _dt(x), _ptr(out), _dt(out), x.numel(), _stream()), "cn_cast")
    return out


def f32(x):
    return x if x is None else cast(x, torch.float32)


def _unify(*ts):
    """Activation operands of one elementwise call share a storage type: bf16 as soon as one of them is (an fp32 gradient
    arriving from a dense layer meets a bf16 activation)."""
    dt = torch.bfloat16 if any(t is not None and t.dtype == torch.bfloat16 for t in ts) else torch.float32
    return [None if t is None else cast(t, dt) for t in ts]


def _act_out_dtype(channels):
    return ACT_DTYPE if channels > 4 else torch.float32


# ---------------------------------------------------------------------------------------------
# convolution geometry ([TF-2.1] SAME rule R2: total = max((ceil(e/s)-1)*s + k - e, 0), lo = total//2)
# ---------------------------------------------------------------------------------------------
class ConvSpec:
    """Static description of one conv layer call: spatial kernel, stride, folded x2 upsample,
    optional explicit symmetric padding (ZeroPadding2D + 'valid')."""

    def __init__(self, kernel, stride=1, up=0, explicit_pad=None):
        self.kernel = tuple(kernel)
        self.stride, self.up, self.explicit_pad = stride, up, explicit_pad

    def geom(self, x_shape, cout):
        nd = len(self.kernel)
        assert len(x_shape) == nd + 2
        n, cin = x_shape[0], x_shape[-1]
        sp = list(x_shape[1:-1])
        ins, outs, pads = [1, 1, 1], [1, 1, 1], [0, 0, 0]
        ks = [1, 1, 1]
        for i in range(nd):
            a = 3 - nd + i
            e = sp[i] << self.up
            k, s = self.kernel[i], self.stride
            if self.explicit_pad is None:
                o = -(-e // s)
                total = max((o - 1) * s + k - e, 0)
                lo = total // 2
            else:
                lo = self.explicit_pad
                o = (e + 2 * lo - k) // s + 1
            ins[a], outs[a], pads[a], ks[a] = sp[i], o, lo, k
        g = CnConvGeom()
        g.nd, g.n = nd, n
        g.in_d, g.in_h, g.in_w, g.cin = ins[0], ins[1], ins[2], cin
        g.out_d, g.out_h, g.out_w, g.cout = outs[0], outs[1], outs[2], cout
        g.k_d, g.k_h, g.k_w = ks
        s = self.stride
        g.s_d, g.s_h, g.s_w = (s if nd == 3 else 1), s, s
        g.dl_d = g.dl_h = g.dl_w = 1
        g.p_d, g.p_h, g.p_w = pads
        g.up = self.up
        return g


def geom_out_shape(g):
    return (g.n, g.out_d, g.out_h, g.out_w, g.cout) if g.nd == 3 else (g.n, g.out_h, g.out_w, g.cout)


def geom_in_shape(g, upsampled=False):
    u = g.up if upsampled else 0
    if g.nd == 3:
        return (g.n, g.in_d << u, g.in_h << u, g.in_w << u, g.cin)
    return (g.n, g.in_h << u, g.in_w << u, g.cin)


_keepalive = None        # a list while an InferenceGraph is captured: every derived filter copy the capture references


def _weight_cache(w, slot, make):
    val = _weight_cache_lookup(w, slot, make)
    if _keepalive is not None:
        _keepalive.append(val)
    return val


def _weight_cache_lookup(w, slot, make):
    """Derived forms of a filter (tap-flipped fp32 copy, bf16 operand copies), cached on the tensor.  A weight of a network
    (nn.Net tags its tensors with their owner) is re-derived when THAT network's epoch moves; other tensors (the cotangent
    "filters" of double-backward calls) when torch's version counter does.  The key also holds the stream (a forked step
    derives on each branch instead of sharing a tensor across streams) and the global generation, which a HIP-graph capture
    bumps so that copies used inside a graph are made inside it -- except for FROZEN networks (no trainable weight: the VGG
    stacks), whose copies are made once, outside any capture, and then referenced by every graph."""
    from .nn import WEIGHTS_EPOCH
    owner = getattr(w, "_cn_owner", None)
    frozen = owner is not None and getattr(owner, "n_trainable", 1) == 0
    if frozen:
        key = (owner.epoch, w.data_ptr())
        c = getattr(w, slot, None)
        if c is not None and c[0] == key:
            return c[1]
        if not w.is_cuda or not torch.cuda.is_current_stream_capturing():   # (a host tensor knows no stream: nothing to ask the runtime)
            val = make(w.detach())
            if w.is_cuda:
                torch.cuda.current_stream().synchronize()   # once per frozen filter: any stream may read the copy from now on
            setattr(w, slot, (key, val))
            return val
        return make(w.detach())                    # first use happens inside a capture: a graph-private copy
    stream = torch.cuda.current_stream().cuda_stream if w.is_cuda else 0
    key = (WEIGHTS_EPOCH[0], owner.epoch if owner is not None else -1, w._version, w.data_ptr(), stream)
    c = getattr(w, slot, None)
    # one entry PER STREAM (a dict): the two branches of a forked step use the same generator / regressor filters alternately --
    # forward on one stream, forward on the other, then the two backward passes -- and a single entry made each of them derive its
    # copy again (the key holds the stream, so the other branch's entry never matched and was replaced)
    if isinstance(c, dict):
        e = c.get(stream)
        if e is not None and e[0] == key:
            return e[1]
    val = make(w.detach())
    try:
        if not isinstance(c, dict) or any(e[0][:4] != key[:4] for e in c.values()):
            c = {}                                   # another epoch / version / storage: drop every stream's stale copy
        c[stream] = (key, val)
        setattr(w, slot, c)
    except Exception:
        pass
    return val


def weight_prep_bf16(w):
    """(wf [t][co][ci], wd [t][ci][co]) bf16 operand copies of the fp32 filter w [..taps.., cin, cout]."""
    def make(wd_):
        taps, cin, cout = int(math.prod(wd_.shape[:-2])), wd_.shape[-2], wd_.shape[-1]
        both = torch.empty((2, taps * cin * cout), device=wd_.device, dtype=torch.bfloat16)
        check(lib.cn_conv_weight_prep_bf16(_fptr(_c(wd_)), _ptr(both[0]), _ptr(both[1]), taps, cin, cout, _stream()),
              "cn_conv_weight_prep_bf16")
        return both[0], both[1]
    return _weight_cache(w, "_cn_wbf16", make)


def _bf16_conv_ok(g):
    return ACT_DTYPE == torch.bfloat16 and g.cin % 8 == 0 and g.cout % 8 == 0


# ---------------------------------------------------------------------------------------------
# x2-upsample-folded convolutions collapsed per output-parity class (include/confignet_hip.h: cn_upfold_*)
# ---------------------------------------------------------------------------------------------
UPFOLD = True
UPFOLD_MAX_CLASS_TAPS = 64     # the implicit-GEMM loops keep the live taps of a tile in one 64-bit mask (csrc/conv_geom.h: par_tap_mask)


def upfold_class_taps(g):
    """Taps of the class filters of a folded layer: per used axis k + 1 (3 for k = 2), see cn_upfold_weights."""
    ks = (g.k_d, g.k_h, g.k_w) if g.nd == 3 else (g.k_h, g.k_w)
    return math.prod(k + 1 if k >= 3 else 3 for k in ks)


def upfold_ok(g):
    """Generator layers UpSampling + Conv(k2 .. k4, SAME, stride 1) with wide channels (map_final keeps its own kernel).  3-D extents
    whose class filters pass 64 taps -- (2,4,4), (3,3,4), (3,4,4), (4,4,4) and their permutations -- stay on the unfolded path."""
    return (UPFOLD and g.up == 1 and g.cin > 4 and g.cout > 4 and g.s_d * g.s_h * g.s_w == 1 and g.dl_d * g.dl_h * g.dl_w == 1
            and all(2 <= k <= 4 for k in ((g.k_d, g.k_h, g.k_w) if g.nd == 3 else (g.k_h, g.k_w)))
            and upfold_class_taps(g) <= UPFOLD_MAX_CLASS_TAPS
            and g.out_h == 2 * g.in_h and g.out_w == 2 * g.in_w and (g.nd == 2 or g.out_d == 2 * g.in_d))


def _copy_geom(g, **kw):
    out = CnConvGeom()
    for name, _ in CnConvGeom._fields_:
        setattr(out, name, getattr(g, name))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def upfold_prepare(w, g):
    """(wf, wd, gd, g2): class filters (fp32, cached on the filter per weight epoch) and the two geometries they are used
    with (rebuilt per call: batch and extents belong to the call, not to the filter)."""
    def make(wd_):
        k3 = (ctypes.c_int * 3)(g.k_d, g.k_h, g.k_w)
        p3 = (ctypes.c_int * 3)(g.p_d, g.p_h, g.p_w)
        k2, p2 = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
        wd_ = _c(wd_)
        ks = [g.k_d, g.k_h, g.k_w]
        sizes = [1 if (g.nd == 2 and i == 0) else (ks[i] + 1 if ks[i] >= 3 else 3) for i in range(3)]   # k2 per axis
        t2 = sizes[0] * sizes[1] * sizes[2]
        both = torch.empty((2, t2 * g.cin * g.cout), device=wd_.device, dtype=torch.float32)
        check(lib.cn_upfold_weights(_fptr(wd_), _ptr(both[0]), _ptr(both[1]), g.nd, k3, p3, g.cin, g.cout, k2, p2, _stream()),
              "cn_upfold_weights")
        assert list(k2) == sizes, (list(k2), sizes)
        return both[0], both[1], tuple(k2), tuple(p2)
    wf, wd, (kd, kh, kw), (pd, ph, pw) = _weight_cache(w, "_cn_upfold_%d_%d%d%d_%d%d%d" % (g.nd, g.k_d, g.k_h, g.k_w, g.p_d, g.p_h, g.p_w), make)
    # forward: zero-stuffed (dl = 2) convolution on the stored grid, parity-ordered rows, dead taps skipped
    gd = _copy_geom(g, k_d=kd, k_h=kh, k_w=kw, dl_d=(2 if g.nd == 3 else 1), dl_h=2, dl_w=2,
                    p_d=kd - 1 - pd, p_h=kh - 1 - ph, p_w=kw - 1 - pw, up=0)
    # conv2: from the output grid (cout channels) to the stored grid (cin channels), stride 2
    g2 = _copy_geom(g, in_d=g.out_d, in_h=g.out_h, in_w=g.out_w, cin=g.cout, out_d=g.in_d, out_h=g.in_h, out_w=g.in_w,
                    cout=g.cin, k_d=kd, k_h=kh, k_w=kw, s_d=(2 if g.nd == 3 else 1), s_h=2, s_w=2, p_d=pd, p_h=ph, p_w=pw, up=0)
    taps = (kd, kh, kw) if g.nd == 3 else (kh, kw)
    return wf.view(taps + (g.cin, g.cout)), wd.view(taps + (g.cout, g.cin)), gd, g2


def upfold_wgrad(gw2, g, w_shape, out=None, single_writer=False):
    """gw[kk][ci][co] from the conv2 filter gradient gw2[a][co][ci]; out: add to this tensor instead (atomically, unless the
    caller is the only one adding to it right now)."""
    gw = out if out is not None else torch.empty(w_shape, device=gw2.device, dtype=torch.float32)
    k3 = (ctypes.c_int * 3)(g.k_d, g.k_h, g.k_w)
    p3 = (ctypes.c_int * 3)(g.p_d, g.p_h, g.p_w)
    mode = 0 if out is None else (2 if single_writer else 1)
    check(lib.cn_upfold_wgrad(_fptr(_c(gw2)), _ptr(gw), g.nd, k3, p3, g.cin, g.cout, mode, _stream()), "cn_upfold_wgrad")
    return gw


# ---------------------------------------------------------------------------------------------
# Winograd F(2x2, 3x3) for the wide 2-D 3x3 stride-1 SAME layers (fp32 mode): include/confignet_hip.h: cn_conv_fwd_wino
# ---------------------------------------------------------------------------------------------
WINOGRAD = True
WINO_MIN_WGS = 32           # (round 6, alternating pipelined runs: 128 -> 64 -> 32 = 409.6 / 411.3 / 411.5 images/s; what counts next to other lines is the work issued, not the isolated latency)
WINO_MIN_FILL = 0.7         # fraction of the 8 x 8-tile blocks that must lie inside the image


def _wino_ok(g, cin, cout):
    """cin / cout: reduction / output channels of the convolution actually run (swapped for a data gradient)."""
    if not (WINOGRAD and g.nd == 2 and g.k_h == 3 and g.k_w == 3 and g.s_h == 1 and g.s_w == 1 and g.dl_h == 1 and g.dl_w == 1
            and g.up == 0 and g.p_h == 1 and g.p_w == 1 and g.out_h == g.in_h and g.out_w == g.in_w):
        return False
    if cin % 16 or cout % 64:
        return False
    # workgroup = 8 x 8 tiles (16 x 16 output pixels) x 64 channels: most of the block must be image, and there must be
    # enough workgroups to fill the chip (below that the direct kernel with split-K wins)
    th, tw = (g.in_h + 1) // 2, (g.in_w + 1) // 2
    bh, bw = (th + 7) // 8, (tw + 7) // 8
    if th * tw < WINO_MIN_FILL * (bh * bw * 64):
        return False
    return g.n * bh * bw * (cout // 64) >= WINO_MIN_WGS


WINO4 = True
WINO4_MIN_WGS = 128


def _wino4_ok(g, cin, cout):
    """Winograd F(4x4, 3x3) (csrc/winograd4.hip) takes the 3x3 stride-1 SAME layers whose image divides into its 16 x 32-pixel
    blocks and that fill the chip with them (VGG-19 conv1_2 .. conv3_4 at the benchmark's size); cin / cout as in _wino_ok."""
    if not (WINO4 and WINOGRAD and g.nd == 2 and g.k_h == 3 and g.k_w == 3 and g.s_h == 1 and g.s_w == 1 and g.dl_h == 1 and g.dl_w == 1
            and g.up == 0 and g.p_h == 1 and g.p_w == 1 and g.out_h == g.in_h and g.out_w == g.in_w):
        return False
    if g.in_h % 16 or g.in_w % 32 or cin % 16 or cout % 64:
        return False
    return g.n * (g.in_h // 16) * (g.in_w // 32) * (cout // 64) >= WINO4_MIN_WGS


def _wino4_filter(w, dgrad):
    def make(wd_):
        wd_ = _c(wd_)
        cin, cout = wd_.shape[-2], wd_.shape[-1]
        u = torch.empty((36, cout, cin) if dgrad else (36, cin, cout), device=wd_.device, dtype=torch.float32)
        check(lib.cn_conv_wino4_filter(_fptr(wd_), _ptr(u), cin, cout, int(dgrad), _stream()), "cn_conv_wino4_filter")
        return u
    return _weight_cache(w, "_cn_wino4_d" if dgrad else "_cn_wino4_f", make)


def wino4_saved_flops(g):
    """Direct-convolution multiply-adds (border taps counted) minus the 36 per 4x4 tile that F(4x4, 3x3) issues."""
    tiles = g.n * (g.in_h // 4) * (g.in_w // 4)
    return 2.0 * g.cin * g.cout * (9.0 * g.n * g.in_h * g.in_w - 36.0 * tiles)


def _wino_filter(w, dgrad):
    def make(wd_):
        wd_ = _c(wd_)
        cin, cout = wd_.shape[-2], wd_.shape[-1]
        u = torch.empty((16, cout, cin) if dgrad else (16, cin, cout), device=wd_.device, dtype=torch.float32)
        check(lib.cn_conv_wino_filter(_fptr(wd_), _ptr(u), cin, cout, int(dgrad), _stream()), "cn_conv_wino_filter")
        return u
    return _weight_cache(w, "_cn_wino_d" if dgrad else "_cn_wino_f", make)


# Statistics of a convolution's output taken in its epilogue (cn_conv_fwd_stats) for the normalisation layer that follows:
# `with request_stats(kind[, slope])` around the convolution, `take_stats(y, kind)` in the consumer.  kind "act": (sum a, sum a^2) of
# the stored, activated output (AdaIn); kind "pre4": (sum v, sum v^2, sum l, sum l^2), l = leaky_relu(v, slope), of a convolution
# without activation (DiscrBlock tail).  Only launches that can carry them do (fp32, the unsplit LDS-DMA loop, tiles inside one
# sample, a zero pool active, not the deterministic mode); everything else leaves no entry and the consumer runs its own pass.
class _StatsSlot(threading.local):        # per host thread: a request / a result never crosses to a convolution issued by another thread
    request = None
    ready = None                          # (data_ptr, shape, kind, tensors) of the most recent fused launch


_stats = _StatsSlot()
STATS_FUSION = True


class request_stats:
    def __init__(self, kind, slope=0.0):
        self.req = (kind, float(slope))

    def __enter__(self):
        self.prev, _stats.request = _stats.request, (self.req if STATS_FUSION and not DETERMINISTIC else None)

    def __exit__(self, *exc):
        _stats.request = self.prev


def take_stats(y, kind):
    """The statistics the producing convolution left for tensor y, or None."""
    ent, _stats.ready = _stats.ready, None
    if ent is not None and ent[0] == y.data_ptr() and ent[1] == tuple(y.shape) and ent[2] == kind:
        return ent[3]
    return None


def conv_fwd(x, w, bias, g, act=ACT_NONE, slope=0.0):
    req, _stats.request = _stats.request, None           # (a request applies to the next convolution only)
    _stats.ready = None
    out_dtype = _act_out_dtype(g.cout)
    if ACT_DTYPE == torch.float32 and x.dtype == torch.float32 and _wino4_ok(g, g.cin, g.cout):
        y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.float32)
        check(lib.cn_conv_fwd_wino4(g.n, g.in_h, g.in_w, g.cin, g.cout, _ptr(_c(x)), _ptr(_wino4_filter(w, False)), _fptr(bias), _ptr(y),
                                    act, slope, _stream()), "cn_conv_fwd_wino4")
        prof_note_saved(wino4_saved_flops(g))
        return y
    if ACT_DTYPE == torch.float32 and x.dtype == torch.float32 and _wino_ok(g, g.cin, g.cout):
        y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.float32)
        check(lib.cn_conv_fwd_wino(g.n, g.in_h, g.in_w, g.cin, g.cout, _ptr(x), _ptr(_wino_filter(w, False)), _fptr(bias), _ptr(y),
                                   act, slope, _stream()), "cn_conv_fwd_wino")
        prof_note_saved(wino_saved_flops(g))
        return y
    if _bf16_conv_ok(g):
        x = cast(x, torch.bfloat16)
        y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.bfloat16)
        wf, _ = weight_prep_bf16(w)
        check(lib.cn_conv_fwd_bf16(ctypes.byref(g), _ptr(x), _ptr(wf), _fptr(bias), _ptr(y), act, slope, _stream()), "cn_conv_fwd_bf16")
        return y
    x = f32(x)                                  # 3-channel image layers (and everything in fp32 mode): fp32 MFMA family
    if out_dtype == torch.bfloat16 and MIXED_FIRST_LAYERS and g.cin == 3:
        # first layer of the bf16 path: fp32 image in, bf16 out of the same kernel (no conversion pass over the wide tensor)
        y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.bfloat16)
        rc = lib.cn_conv_fwd_dt(ctypes.byref(g), _ptr(x), CN_F32, _fptr(w), _fptr(bias), _ptr(y), CN_BF16, act, slope, _stream())
        if rc == 0:
            return y
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_fwd_dt")
    y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.float32)
    if req is not None and out_dtype == torch.float32 and g.cout % 4 == 0 and (req[0] == "act" or act == ACT_NONE):
        nk = 2 if req[0] == "act" else 4
        mark = _active_pool.cur if _active_pool is not None else None
        st = zero_pool_alloc((nk, g.n, g.cout), x.device)
        if st is not None:
            rc = lib.cn_conv_fwd_stats(ctypes.byref(g), _ptr(_c(x)), _fptr(w), _fptr(bias), _ptr(y), act, slope, _ptr(st), 1 if nk == 2 else 2,
                                       req[1], _stream())
            if rc == 0:
                _stats.ready = (y.data_ptr(), tuple(y.shape), req[0], tuple(st[k] for k in range(nk)))
                return y
            if rc != CN_EUNSUPPORTED:
                check(rc, "cn_conv_fwd_stats")
            _active_pool.cur = mark                   # nothing was launched: hand the (untouched, still zero) slab back to the pool
    check(lib.cn_conv_fwd(ctypes.byref(g), _ptr(x), _fptr(w), _fptr(bias), _ptr(y), act, slope, _stream()), "cn_conv_fwd")
    return cast(y, out_dtype)


W4_EP_POOL, W4_EP_POOL_ONLY, W4_EP_MASK = 1, 2, 3        # epilogue modes of cn_conv_fwd_wino4_ep (include/confignet_hip.h)


def conv_fwd_pool(x, w, bias, g, act=ACT_NONE, slope=0.0, keep_full=True):
    """(y or None, maxpool 2x2/2 of y) for y = act(conv(x, w) + bias), the pool taken in the F(4x4) launch's epilogue
    (cn_conv_fwd_wino4_ep); keep_full=False: y is neither stored nor returned.  None where the layer is not an fp32 F(4x4)
    launch: the caller then runs conv_fwd and maxpool_fwd."""
    if not (ACT_DTYPE == torch.float32 and x.dtype == torch.float32 and _wino4_ok(g, g.cin, g.cout)):
        return None
    _stats.request = _stats.ready = None                 # (as conv_fwd: a request applies to the next convolution only)
    y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.float32) if keep_full else None
    pooled = torch.empty((g.n, g.in_h // 2, g.in_w // 2, g.cout), device=x.device, dtype=torch.float32)
    check(lib.cn_conv_fwd_wino4_ep(g.n, g.in_h, g.in_w, g.cin, g.cout, _ptr(_c(x)), _ptr(_wino4_filter(w, False)), _fptr(bias), _ptr(y),
                                   act, slope, W4_EP_POOL if keep_full else W4_EP_POOL_ONLY, _ptr(pooled), None, None, None, 1, 0.0,
                                   _stream()), "cn_conv_fwd_wino4_ep")
    prof_note_saved(wino4_saved_flops(g))
    return y, pooled


def conv_dgrad_masked(gy, w, g, y, target=None, s=None, k=0.0):
    """(conv_dgrad(gy, w, g) [+ (y - target) s[sample] k]) relu'(y): the data gradient of the convolution described by g with the
    elementwise backward step of the layer in front (act_bwd, or tap_bwd at a tapped layer; y = that layer's ReLU output, the
    shape of g's input) in the F(4x4) launch's epilogue.  s: 1 or n scales.  None where the data gradient is not an fp32 F(4x4)
    launch: the caller then runs the two passes."""
    if not (ACT_DTYPE == torch.float32 and gy.dtype == torch.float32 and y.dtype == torch.float32 and _wino4_ok(g, g.cout, g.cin)):
        return None
    if target is not None and (target.dtype != torch.float32 or s is None or s.numel() not in (1, g.n)):
        return None
    _log_mask(y, ACT_RELU)
    gu = torch.empty(geom_in_shape(g, upsampled=True), device=gy.device, dtype=torch.float32)
    check(lib.cn_conv_fwd_wino4_ep(g.n, g.in_h, g.in_w, g.cout, g.cin, _ptr(_c(gy)), _ptr(_wino4_filter(w, True)), None, _ptr(gu),
                                   ACT_NONE, 0.0, W4_EP_MASK, None, _ptr(_c(y)), None if target is None else _ptr(_c(target)),
                                   None if target is None else _fptr(s), 1 if target is None else s.numel(), k, _stream()),
          "cn_conv_fwd_wino4_ep")
    prof_note_saved(wino4_saved_flops(g))
    return gu


def conv_fwd_res(x, w, bias, res, g, act=ACT_NONE, slope=0.0):
    """act(conv(x, w) + bias + res): the residual add of a ResNet block in the convolution's epilogue where the launch carries it
    (cn_conv_fwd_res: unsplit implicit-GEMM launches), else convolution + one nc_lin2 pass."""
    assert act in (ACT_NONE, ACT_RELU)
    if ACT_DTYPE == torch.float32 and x.dtype == torch.float32 and res.dtype == torch.float32 and not _wino_ok(g, g.cin, g.cout):
        x, res = _c(x), _c(res)
        y = torch.empty(geom_out_shape(g), device=x.device, dtype=torch.float32)
        rc = lib.cn_conv_fwd_res(ctypes.byref(g), _ptr(x), _fptr(w), _fptr(bias), _ptr(res), _ptr(y), act, slope, _stream())
        if rc == 0:
            return y
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_fwd_res")
    y = conv_fwd(x, w, bias, g)
    return nc_lin2(tuple(y.shape), y, None, res, None, None, flags=8 if act == ACT_RELU else 0)


def scale_columns_segments(src, seg, a, total):
    """Packed copy of the filters listed in `seg` (int32 (nseg, 5) on the device: see cn_scale_columns_segments), each scaled per
    output channel by its slice of `a`."""
    dst = torch.empty(total, device=src.device, dtype=torch.float32)
    check(lib.cn_scale_columns_segments(_fptr(src), _ptr(dst), _ptr(seg), _fptr(_c(a)), seg.shape[0], total, _stream()),
          "cn_scale_columns_segments")
    return dst


def weight_tflip(w):
    w = _c(w)
    taps = int(math.prod(w.shape[:-2]))
    wt = torch.empty(w.shape[:-2] + (w.shape[-1], w.shape[-2]), device=w.device, dtype=torch.float32)
    check(lib.cn_conv_weight_tflip(_fptr(w), _ptr(wt), taps, w.shape[-2], w.shape[-1], _stream()), "cn_conv_weight_tflip")
    return wt


def conv_dgrad(gy, w, g):
    """Gradient w.r.t. the (virtually upsampled) input of the conv described by g; w is the filter itself (the operand
    copies the kernels want are derived and cached here)."""
    shape = geom_in_shape(g, upsampled=True)
    if _bf16_conv_ok(g):
        gy = cast(gy, torch.bfloat16)
        gu = torch.empty(shape, device=gy.device, dtype=torch.bfloat16)
        _, wd = weight_prep_bf16(w)
        check(lib.cn_conv_dgrad_bf16(ctypes.byref(g), _ptr(gy), _ptr(wd), _ptr(gu), _stream()), "cn_conv_dgrad_bf16")
        return gu
    if gy.dtype == torch.bfloat16 and MIXED_FIRST_LAYERS and g.cin == 3:
        # data gradient into the fp32 image straight from the bf16 output gradient
        gu = torch.empty(shape, device=gy.device, dtype=torch.float32)
        wt = _weight_cache(w, "_cn_tflip", weight_tflip)
        rc = lib.cn_conv_dgrad_dt(ctypes.byref(g), _ptr(_c(gy)), CN_BF16, _fptr(wt), _ptr(gu), CN_F32, _stream())
        if rc == 0:
            return cast(gu, _act_out_dtype(g.cin))
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_dgrad_dt")
    gy = f32(gy)
    gu = torch.empty(shape, device=gy.device, dtype=torch.float32)
    if ACT_DTYPE == torch.float32 and _wino4_ok(g, g.cout, g.cin):
        check(lib.cn_conv_fwd_wino4(g.n, g.in_h, g.in_w, g.cout, g.cin, _ptr(_c(gy)), _ptr(_wino4_filter(w, True)), None, _ptr(gu),
                                    ACT_NONE, 0.0, _stream()), "cn_conv_fwd_wino4")
        prof_note_saved(wino4_saved_flops(g))
        return gu
    if ACT_DTYPE == torch.float32 and _wino_ok(g, g.cout, g.cin):
        check(lib.cn_conv_fwd_wino(g.n, g.in_h, g.in_w, g.cout, g.cin, _ptr(gy), _ptr(_wino_filter(w, True)), None, _ptr(gu),
                                   ACT_NONE, 0.0, _stream()), "cn_conv_fwd_wino")
        prof_note_saved(wino_saved_flops(g))
        return gu
    if DGRAD_FROM_W:
        # the kernel transposes the filter tile on its way into LDS: no tap-flipped copy per trainable filter per step
        rc = lib.cn_conv_dgrad_w(ctypes.byref(g), _ptr(gy), _fptr(_c(w)), _ptr(gu), _stream())
        if rc == 0:
            return cast(gu, _act_out_dtype(g.cin))
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_dgrad_w")
    wt = _weight_cache(w, "_cn_tflip", weight_tflip)
    check(lib.cn_conv_dgrad(ctypes.byref(g), _ptr(gy), _fptr(wt), _ptr(gu), _stream()), "cn_conv_dgrad")
    return cast(gu, _act_out_dtype(g.cin))


def conv_dgrad_res(gy, w, g, res):
    """conv_dgrad(gy, w, g) + res: the gradient of a tensor that feeds this convolution and a skip connection, the add in the
    data-gradient launch's epilogue where the launch carries it (cn_conv_dgrad_w_res: fp32, stride 1, unsplit implicit-GEMM
    launches), else data gradient + one nc_lin2 pass."""
    if (ACT_DTYPE == torch.float32 and gy.dtype == torch.float32 and res.dtype == torch.float32 and DGRAD_FROM_W and not g.up
            and not _wino4_ok(g, g.cout, g.cin) and not _wino_ok(g, g.cout, g.cin)):
        gu = torch.empty(geom_in_shape(g, upsampled=True), device=gy.device, dtype=torch.float32)
        rc = lib.cn_conv_dgrad_w_res(ctypes.byref(g), _ptr(_c(gy)), _fptr(_c(w)), _ptr(_c(res)), _ptr(gu), _stream())
        if rc == 0:
            return gu
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_dgrad_w_res")
    gu = conv_dgrad(gy, w, g)
    return nc_lin2(tuple(gu.shape), gu, None, res, None, None)


MASK_EPILOGUE = True           # conv_dgrad_mask: False = always the data gradient and the pass
MASK_LOG = None                # a list (tests, A/B): conv_dgrad_mask appends "fwd2" / "wino" / "pass" per call


def conv_dgrad_mask(gy, w, g, mask, res=None, sums=(), defer=True):
    """act_bwd(conv_dgrad(gy, w, g) [+ res], mask, ACT_RELU) and, for every slice in `sums` (at most two), slice[c] += the channel
    sums of the result: the ReLU backward of the layer in front and its shift sums in the data-gradient launch's epilogue where
    the launch carries them -- Winograd F(2x2) where conv_dgrad takes it and there is no residual (cn_conv_fwd_wino_ep), else the
    unsplit LDS-DMA launches (cn_conv_dgrad_w_mask) -- with the same bits in the gradient.  Everything else (a K split, bf16 storage,
    the deterministic mode, F(4x4), and a residual on a layer conv_dgrad routes to F(2x2): conv_dgrad_res keeps that layer on
    Winograd with an add pass, so cn_conv_dgrad_w_mask is not asked there either -- the ResNet trunk has no such layer, its
    residuals ride on 1x1 launches) runs the data gradient and the pass: conv_dgrad / conv_dgrad_res, then act_bwd or
    act_bwd_partials + sum_rows_into(defer=defer)."""
    assert len(sums) <= 2
    fused = None
    if (MASK_EPILOGUE and not DETERMINISTIC and ACT_DTYPE == torch.float32 and gy.dtype == torch.float32 and mask.dtype == torch.float32
            and (res is None or res.dtype == torch.float32) and DGRAD_FROM_W and not g.up and not _bf16_conv_ok(g)
            and not _wino4_ok(g, g.cout, g.cin)):
        gu = torch.empty(geom_in_shape(g, upsampled=True), device=gy.device, dtype=torch.float32)
        assert tuple(gu.shape) == tuple(mask.shape), "conv_dgrad_mask: the mask has the shape of the data gradient"
        s0 = _fptr(sums[0]) if len(sums) > 0 else None
        s1 = _fptr(sums[1]) if len(sums) > 1 else None
        if _wino_ok(g, g.cout, g.cin):
            if res is None:
                rc = lib.cn_conv_fwd_wino_ep(g.n, g.in_h, g.in_w, g.cout, g.cin, _ptr(_c(gy)), _ptr(_wino_filter(w, True)), _ptr(gu),
                                             _ptr(_c(mask)), s0, s1, _stream())
                fused = "wino"
            else:
                rc = CN_EUNSUPPORTED
        else:
            rc = lib.cn_conv_dgrad_w_mask(ctypes.byref(g), _ptr(_c(gy)), _fptr(_c(w)), None if res is None else _ptr(_c(res)),
                                          _ptr(_c(mask)), _ptr(gu), s0, s1, _stream())
            fused = "fwd2"
        if rc == 0:
            _log_mask(mask, ACT_RELU)
            if sums and _SINK is not None:
                _SINK.note_stream()                  # (the sums are added on this stream: the join orders itself behind it)
            if fused == "wino":
                prof_note_saved(wino_saved_flops(g))
            if MASK_LOG is not None:
                MASK_LOG.append(fused)
            return gu
        if rc != CN_EUNSUPPORTED:
            check(rc, "cn_conv_fwd_wino_ep" if fused == "wino" else "cn_conv_dgrad_w_mask")
        del gu
    if MASK_LOG is not None:
        MASK_LOG.append("pass")
    gu = conv_dgrad(gy, w, g) if res is None else conv_dgrad_res(gy, w, g, res)
    if not sums:
        return act_bwd(gu, mask, ACT_RELU)
    gu, part = act_bwd_partials(gu, mask, ACT_RELU)
    for dst in sums:
        sum_rows_into(part, dst, defer=defer)
    return gu


DGRAD_FROM_W = True
MIXED_FIRST_LAYERS = True      # bf16 path: first-layer kernels that read / write both storage types
WGRAD_WRITE, WGRAD_ADD, WGRAD_ZEROED = 0, 1, 2      # include/confignet_hip.h: CN_WGRAD_*


def conv_wgrad(x, gy, g, w_shape, out=None, accumulate=True, defer=True, ws=None):
    """out: ADD the filter gradient to this tensor (a slot of a gradient arena, see grad_sink) instead of returning a new one;
    out with accumulate=False: WRITE it there (an uninitialised scratch the caller owns: the folded ResNet-50's packed gradients).
    defer=False: complete in `out` when this returns, also inside a grad_sink (no slab reduction left to its join).
    ws: the caller's own fp32 workspace (at least what cn_conv_wgrad_dt_workspace_bytes reports) instead of a fresh one.
    Which kernel runs is the library's decision (csrc/conv_dispatch.hip: plan_conv_wgrad); here only the storage types are chosen."""
    gw, mode = out, WGRAD_ADD if accumulate else WGRAD_WRITE
    if out is None:
        gw, mode = zero_pool_alloc(w_shape, x.device), WGRAD_ZEROED
        if gw is None:
            gw, mode = torch.empty(w_shape, device=x.device, dtype=torch.float32), WGRAD_WRITE
    # x in bf16 where the bf16 kernels take the layer, else fp32; gy as it is stored where a kernel reads that next to x (the K = 27
    # first layers read a bf16 gy next to the fp32 image), else in x's type
    x = _c(cast(x, torch.bfloat16 if _bf16_conv_ok(g) else torch.float32))
    nbytes = ctypes.c_size_t(0)
    rc = lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), _dt(x), _dt(gy), ctypes.byref(nbytes))
    if rc == CN_EUNSUPPORTED and gy.dtype != x.dtype:
        gy = cast(gy, x.dtype)
        rc = lib.cn_conv_wgrad_dt_workspace_bytes(ctypes.byref(g), _dt(x), _dt(gy), ctypes.byref(nbytes))
    check(rc, "cn_conv_wgrad_dt_workspace_bytes")
    gy, nbytes = _c(gy), nbytes.value
    # caller-owned workspace: the slabs of the row slices or the partial filters of the first / last layers' kernels (0 bytes: none)
    if ws is None:
        ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32) if nbytes else None
    else:
        assert ws.dtype == torch.float32 and ws.numel() * 4 >= nbytes, "conv_wgrad: workspace of %d bytes, %d needed" % (ws.numel() * 4, nbytes)
    # inside a backward pass (grad_sink): the row slices' slabs stay in `ws` and the pass adds the slabs of ALL its filter
    # gradients with one grouped launch at its join (grad_sink.join) instead of one reduction launch per layer on the chain
    parts = ctypes.c_int(0) if nbytes and out is not None and _SINK is not None and defer else None
    check(lib.cn_conv_wgrad_dt(ctypes.byref(g), _ptr(x), _dt(x), _ptr(gy), _dt(gy), _fptr(gw), mode, _ptr(ws), nbytes,
                               None if parts is None else ctypes.byref(parts), _stream()), "cn_conv_wgrad_dt")
    if parts is not None and parts.value:
        _SINK.slabs.append((ws, gw, parts.value, gw.numel(), int(mode != WGRAD_WRITE)))
    return gw


WGRAD_GROUPED = True      # (False: the deferred filter gradients one launch per layer, as conv_wgrad issues them -- cross-check)


def wgrad_groupable(x, gy, g):
    """True where a filter gradient may be deferred to conv_wgrad_grouped: fp32 operands on a geometry the LDS-DMA kernel takes, not
    in bf16 mode and not in deterministic mode (whose bits are those of the per-layer slice plans)."""
    if not WGRAD_GROUPED or DETERMINISTIC or ACT_DTYPE != torch.float32 or x.dtype != torch.float32 or gy.dtype != torch.float32:
        return False
    out = (ctypes.c_longlong * 12)()
    return lib.cn_conv_wgrad_plan(ctypes.byref(g), CN_F32, CN_F32, 1, 0xffffffff, -1, out) == 0 and out[0] == 3


def conv_wgrad_grouped_plan(geoms, solo=False):
    """(per job: tile, stages, slices, rows per slice, tiles x / y, first workgroup, workgroups, launch, workspace floats;
    launches, jobs a launch holds, bytes of a launch's arguments, bytes an argument block holds) -- cn_conv_wgrad_grouped_plan."""
    n = len(geoms)
    arr = (CnConvGeom * n)(*geoms)
    out, info = (ctypes.c_longlong * (10 * n))(), (ctypes.c_longlong * 4)()
    check(lib.cn_conv_wgrad_grouped_plan(n, arr, int(solo), out, info), "cn_conv_wgrad_grouped_plan")
    return [tuple(out[10 * j:10 * j + 10]) for j in range(n)], tuple(info)


def conv_wgrad_grouped(jobs, solo=False):
    """jobs: [(x, gy, geometry, out, accumulate)], every one wgrad_groupable.  The filter gradients of all of them in a few launches
    that fill the chip together (cn_conv_wgrad_grouped); out is written, or added to where accumulate.  Returns the slab sums that
    remain -- [(slabs, out, parts, count, accumulate)], the jobs of _sum_slabs_grouped -- for the jobs the plan cut into row slices;
    the others are complete."""
    if not jobs:
        return []
    n = len(jobs)
    xs, gys = [_c(j[0]) for j in jobs], [_c(j[1]) for j in jobs]
    plan, _ = conv_wgrad_grouped_plan([j[2] for j in jobs], solo)
    total = sum(p[9] for p in plan)
    ws_all = torch.empty(total, device=xs[0].device, dtype=torch.float32) if total else None
    ws, o = [], 0
    for p in plan:
        ws.append(ws_all[o:o + p[9]] if p[9] else None)
        o += p[9]
    vp = ctypes.c_void_p * n
    parts = (ctypes.c_int * n)()
    check(lib.cn_conv_wgrad_grouped(n, (CnConvGeom * n)(*[j[2] for j in jobs]), vp(*[_fptr(t).value for t in xs]),
                                    vp(*[_fptr(t).value for t in gys]), vp(*[_fptr(j[3]).value for j in jobs]),
                                    vp(*[None if w is None else w.data_ptr() for w in ws]),
                                    (ctypes.c_size_t * n)(*[4 * p[9] for p in plan]), (ctypes.c_int * n)(*[int(bool(j[4])) for j in jobs]),
                                    int(solo), parts, _stream()), "cn_conv_wgrad_grouped")
    return [(ws[k], jobs[k][3], parts[k], jobs[k][3].numel(), int(bool(jobs[k][4]))) for k in range(n) if parts[k]]


# ---------------------------------------------------------------------------------------------
# gradient sink: while nn.backward_into_arenas runs a backward pass, the filter / dense-weight / bias gradients are ADDED by
# their kernels straight into the weights' slots of the networks' gradient arenas (tf.GradientTape sums the contributions of
# every use of a variable: here the wgrad kernels' own accumulate mode does, not autograd's add kernels and not a copy pass
# afterwards).  Every sink launch runs on the stream that calls it; the pass' small reductions are queued and launched
# grouped at its join.  GRAD_SINK = False: gradients through autograd as before.
# Forking the filter gradients off the backward chain (a fifth stream, or the other branch's stream) was measured and
# rejected: DESIGN.md section 3.
# ---------------------------------------------------------------------------------------------
GRAD_SINK = True
_SINK = None              # the _Sink of the backward pass in flight (grad_sink), else None


def sink_rounds(jobs, key):
    """`jobs` split into rounds (lists, each in the original order): jobs with the same key(job) go into successive rounds,
    every other job into the first."""
    rounds, seen = [], {}
    for job in jobs:
        k = key(job)
        r = seen.get(k, 0)
        seen[k] = r + 1
        if r == len(rounds):
            rounds.append([])
        rounds[r].append(job)
    return rounds


class _Sink:
    """What one backward pass holds: the arena slots of its weights and the work queued for its join."""

    def __init__(self, params):
        self.slots = {p.data_ptr(): p.grad for p in params if p.grad is not None}
        self.touched = []       # every stream a sink launch was issued on (a forked step has two)
        self.wgrads = []        # (x, gy, geometry, dst, accumulate): filter gradients left to the join -> cn_conv_wgrad_grouped
        self.slabs = []         # (src, dst, parts, count, accumulate): ordered slab sums -> cn_sum_parts_grouped
        self.depth = []         # (a, b, slot): dense weight gradients a^T b -> cn_gemm_depth_grouped
        self.upfold = {}        # slot pointer -> (class-filter gradient scratch, geometry, filter shape, slot)
        self.post = []          # functions run once everything above has been issued
        self.post_keep = []     # the tensors they read

    def note_stream(self):
        cur = torch.cuda.current_stream()
        if all(cur != s_ for s_ in self.touched):
            self.touched.append(cur)


def _sum_slabs_grouped(slabs):
    # every filter gradient of the pass that split its rows: (slabs, destination, parts, count, accumulate) -> ONE launch
    # per 80 of them, each reduced in slice order exactly as cn_conv_wgrad_ws would have (same bits)
    # (a weight used more than once in the pass -- the generator runs twice in the generator step -- has several jobs
    # with ONE destination: they go into successive launches, in the order of their filter gradients, so that the adds
    # into one element keep a fixed order; typically two or three launches for ~70 reductions)
    for batch in sink_rounds(slabs, lambda job: job[1].data_ptr()):
        jobs = (CnSumJob * len(batch))()
        for q, (ws, dst, parts, count, acc) in zip(jobs, batch):
            q.src, q.dst, q.count, q.parts, q.accumulate = ws.data_ptr(), dst.data_ptr(), count, parts, acc
        check(lib.cn_sum_parts_grouped(jobs, len(batch), _stream()), "cn_sum_parts_grouped")


def _gemm_depth_grouped(depth):
    for batch in sink_rounds(depth, lambda job: job[2].data_ptr()):     # (same-destination jobs in successive launches, as above)
        jobs = (CnDepthJob * len(batch))()
        for q, (a, b, slot) in zip(jobs, batch):
            q.a, q.b, q.c = a.data_ptr(), b.data_ptr(), slot.data_ptr()
            q.m, q.n, q.k, q.lda, q.ldb, q.ldc = a.shape[1], b.shape[1], a.shape[0], a.shape[1], b.shape[1], b.shape[1]
        check(lib.cn_gemm_depth_grouped(jobs, len(batch), _stream()), "cn_gemm_depth_grouped")


def _release_operands(cur, others, operands):
    """After launches on `cur` that read tensors produced on the streams `others`."""
    if not torch.cuda.is_current_stream_capturing():      # (eager dispatch: the operands were allocated on the stream of
        for t in operands:                                # their producer, not on this one)
            t.record_stream(cur)
    for s_ in others:                         # a stream that produced operands must not run ahead of these launches: a block
        s_.wait_stream(cur)                   # the allocator hands out again after the join would be overwritten under them


class grad_sink:
    def __init__(self, params):
        self.params = params

    def __enter__(self):
        global _SINK
        assert _SINK is None, "nested gradient sinks"
        if GRAD_SINK and self.params:
            _SINK = _Sink(self.params)
        return self

    def join(self):
        """Order the calling stream after everything the sinks launched and issue, on it, what the pass queued for its end."""
        st = _SINK
        if st is None:
            return
        cur = torch.cuda.current_stream()
        others = [s_ for s_ in st.touched if s_ != cur]
        for s_ in others:                             # every stream a sink launched on (a forked step has two) before anything
            cur.wait_stream(s_)                       # below reads or adds to the arenas on the calling stream
        wgrads, slabs, depth, upfold, post, post_keep = st.wgrads, st.slabs, st.depth, st.upfold, st.post, st.post_keep
        st.touched, st.wgrads, st.slabs, st.depth, st.upfold, st.post, st.post_keep = [], [], [], [], {}, [], []
        # the order of the join: 1. the filter gradients left to it, in grouped launches (their slabs join the list); 2. the slab
        # sums and the dense weight gradients; 3. the upsample-folded scatters; 4. the post functions, which read what 1. - 3. completed
        slabs = slabs + conv_wgrad_grouped(wgrads)
        _sum_slabs_grouped(slabs)
        _gemm_depth_grouped(depth)
        if wgrads or slabs or depth:
            _release_operands(cur, others, [t for j in wgrads for t in j[:2]] + [j[0] for j in slabs] + [t for j in depth for t in j[:2]])
        for gw2, g, w_shape, slot in upfold.values():
            upfold_wgrad(gw2, g, w_shape, out=slot, single_writer=True)
        for fn in post:                               # launches that read what the grouped reductions above have just completed
            fn()                                      # (the folded ResNet-50's parameter gradients: cn_bn_fold_bwd)
        if post:
            _release_operands(cur, others, post_keep)
        if st.wgrads or st.slabs or st.depth or st.upfold or st.post:             # nothing runs after this point: work queued by a post function would be lost
            raise RuntimeError("a sink_post function queued work on the gradient sink after its join")

    def __exit__(self, exc_type, exc, tb):
        global _SINK
        try:
            if exc_type is None:                    # (the pass raised: no scatter work on half-written scratch, just let go)
                self.join()
        finally:
            _SINK = None                            # a failed pass must not leave every later one dying on "nested gradient sinks"


def sink_for(w):
    """The gradient-arena slot of weight w if a sink is active for it (else None)."""
    if _SINK is None or w is None:
        return None
    return _SINK.slots.get(w.data_ptr())


def sink_conv_wgrad(x, gy, g, w_shape, slot):
    if _SINK is not None:
        _SINK.note_stream()
    conv_wgrad(x, gy, g, w_shape, out=slot)


def sink_conv_wgrad_to(x, gy, g, w_shape, dst, defer=True):
    """The filter gradient WRITTEN (not added) into the caller's scratch `dst`, launched like a sink (a leaf of the pass)."""
    if _SINK is not None:
        _SINK.note_stream()
    conv_wgrad(x, gy, g, w_shape, out=dst, accumulate=False, defer=defer)


def sink_conv_wgrad_group(jobs):
    """Filter gradients that nothing in the pass waits for -- [(x, gy, geometry, dst, accumulate)], every one wgrad_groupable --
    left to the join of the active gradient sink, which issues them grouped (and keeps their operands alive until then); issued
    grouped here and now, slab sums included, without one."""
    st = _SINK
    if st is None:
        _sum_slabs_grouped(conv_wgrad_grouped(jobs))
        return
    st.note_stream()
    st.wgrads.extend(jobs)


def sink_post(fn, keep=()):
    """Run fn() once every sink launch of the pass -- the deferred grouped reductions included -- has been issued: at the join of
    the active gradient sink, on the stream that joins; immediately without one.  fn must not queue work on the sink."""
    st = _SINK
    if st is None:
        fn()
        return
    st.note_stream()
    st.post_keep.extend(t for t in keep if t is not None)
    st.post.append(fn)


def bn_fold_bwd(seg9, blocks, gwf, gshift, arena, a, rs, bm, gout, chunked=True):
    """cn_bn_fold_bwd: gout (laid out like `arena`) += the kernel / bias / gamma / beta gradients of every folded conv + BN pair.
    chunked: the rows of every filter cut over the grid (a scratch of chunks x columns floats, two launches); else, and in
    deterministic mode, the one-launch walk."""
    scratch = None
    if chunked and not DETERMINISTIC:
        scratch = torch.empty(lib.cn_bn_fold_bwd_chunks() * a.numel(), device=a.device, dtype=torch.float32)
    check(lib.cn_bn_fold_bwd(_ptr(seg9), seg9.shape[0], blocks, _fptr(gwf), _fptr(gshift), _fptr(arena), _fptr(a), _fptr(rs), _fptr(bm),
                             _fptr(gout), _fptr(scratch), a.numel(), _stream()), "cn_bn_fold_bwd")


def sink_upfold_wgrad(gy, x, g2, wd_shape, g, w_shape, slot):
    """Upsample-folded layer: the class-filter gradient of EVERY use of the weight in this backward pass (the generator runs twice
    in the generator step) is accumulated into one scratch by the filter-gradient kernel (atomics: any stream), and scattered
    back to the k taps ONCE, at the join of the pass, by a single writer (10 atomic scatters of up to 172 us -> 5 plain ones)."""
    st = _SINK
    ent = st.upfold.get(slot.data_ptr())
    if ent is None:
        gw2 = zero_pool_alloc(wd_shape, x.device)
        if gw2 is None:
            gw2 = torch.zeros(wd_shape, device=x.device, dtype=torch.float32)
        ent = st.upfold[slot.data_ptr()] = (gw2, g, w_shape, slot)
    st.note_stream()
    conv_wgrad(gy, x, g2, wd_shape, out=ent[0])


def sink_gemm(a, b, slot, trans_a=False, trans_b=False):
    st = _SINK
    if st is not None:
        st.note_stream()
        if (trans_a and not trans_b and a.shape[0] <= 32 and a.dtype == torch.float32 and b.dtype == torch.float32
                and a.is_contiguous() and b.is_contiguous() and slot.is_contiguous()):
            # a dense layer's weight gradient x^T gy over a batch of <= 32 rows: a leaf of the pass -- queued for ONE grouped launch at
            # the pass' join (grad_sink.join -> cn_gemm_depth_grouped) instead of a launch of its own on the backward chain
            st.depth.append((a, b, slot))
            return
    gemm_acc(a, b, slot, trans_a, trans_b)


# ---------------------------------------------------------------------------------------------
# per-step zero pool: accumulate-into outputs (statistics sums, filter gradients) are carved from a buffer that
# is cleared by ONE launch at the start of a training step instead of one clearing launch per call
# ---------------------------------------------------------------------------------------------
class _ZeroPool:
    def __init__(self, device, numel):
        self.buf = torch.zeros(numel, device=device, dtype=torch.float32)
        self.cur = 0
        self.dirty = 0          # high-water mark of the previous use


_pools = {}
_active_pool = None
ZERO_POOL_FLOATS = 96 * 1024 * 1024


def zero_pool_begin(name, device):
    """Activate pool `name` (created on first use) and clear what its previous use dirtied."""
    global _active_pool
    p = _pools.get((name, device))
    if p is None:
        p = _pools[(name, device)] = _ZeroPool(device, ZERO_POOL_FLOATS)
    if p.dirty:
        p.buf[:p.dirty].zero_()
    p.cur = 0
    _active_pool = p


def zero_pool_end():
    global _active_pool
    if _active_pool is not None:
        _active_pool.dirty = max(_active_pool.dirty, _active_pool.cur)
    _active_pool = None


def zero_pool_alloc(shape, device):
    p = _active_pool
    if p is None or p.buf.device != device:
        return None
    n = int(math.prod(shape))
    n4 = (n + 3) // 4 * 4
    if p.cur + n4 > p.buf.numel():
        return None
    out = p.buf[p.cur:p.cur + n].view(shape)
    p.cur += n4
    return out


def _sums(shape, device):
    """(fp32 sums of a reduction, flag): carved from the step's zero pool (16: already clear) or fresh (0: the call clears them
    where its kernel adds with atomics)."""
    t = zero_pool_alloc(shape, device)
    if t is not None:
        return t, 16
    return torch.empty(shape, device=device, dtype=torch.float32), 0


def zero_(t):
    """Clear a contiguous fp32 tensor with the library's own kernel (a graph node that re-executes on replay)."""
    check(lib.cn_zero(_fptr(t), t.numel() * 4, _stream()), "cn_zero")
    return t


def sumpool2(gu):
    nd = gu.dim() - 2
    sp = [s // 2 for s in gu.shape[1:-1]]
    gx = torch.empty((gu.shape[0], *sp, gu.shape[-1]), device=gu.device, dtype=gu.dtype)
    d, h, w = ([1] + sp) if nd == 2 else sp
    check(lib.cn_sumpool2(_ptr(gu), _ptr(gx), nd, gu.shape[0], d, h, w, gu.shape[-1], _dt(gu), _stream()), "cn_sumpool2")
    return gx


# ---------------------------------------------------------------------------------------------
def gemm(a, b, trans_a=False, trans_b=False, bias=None, act=ACT_NONE, slope=0.0):
    """C = act(op(a) @ op(b) + bias); a, b 2-D row-major."""
    m = a.shape[1] if trans_a else a.shape[0]
    k = a.shape[0] if trans_a else a.shape[1]
    n = b.shape[0] if trans_b else b.shape[1]
    kb = b.shape[1] if trans_b else b.shape[0]
    assert k == kb, "gemm inner dims %d vs %d" % (k, kb)
    a, b = f32(a), f32(b)                      # dense layers compute in fp32 (a flattened bf16 feature map is converted)
    c = torch.empty((m, n), device=a.device, dtype=torch.float32)
    check(lib.cn_gemm(int(trans_a), int(trans_b), m, n, k, _ptr(a), a.shape[1], _ptr(b), b.shape[1], _ptr(c), n,
                      _ptr(bias), act, slope, _stream()), "cn_gemm")
    return c


def gemm_acc(a, b, out, trans_a=False, trans_b=False):
    """out += op(a) @ op(b) (cn_gemm_acc)."""
    m = a.shape[1] if trans_a else a.shape[0]
    k = a.shape[0] if trans_a else a.shape[1]
    n = b.shape[0] if trans_b else b.shape[1]
    a, b = f32(a), f32(b)
    assert tuple(out.shape) == (m, n) and out.is_contiguous()
    check(lib.cn_gemm_acc(int(trans_a), int(trans_b), m, n, k, _ptr(a), a.shape[1], _ptr(b), b.shape[1], _fptr(out), n, _stream()),
          "cn_gemm_acc")
    return out


def _nsc(x):
    n, c = x.shape[0], x.shape[-1]
    return n, x.numel() // (n * c), c


def nc_reduce(x1, x2=None, want_sum=True, want_dot=True, flags=0, slope=0.0, per_channel=False, x2_period=0):
    """(sum_s f1(x1), sum_s f1(x1)*f2(x2 or x1)) per (n, c); per_channel folds n into s.
    x2_period: x2 holds only that many samples and sample n of x1 pairs with x2[n % x2_period]."""
    x1, x2 = _unify(x1, x2)
    n, s, c = _nsc(x1)
    assert not (x2_period and per_channel)
    flags |= x2_period << 8
    rep = 1
    if per_channel:
        # every workgroup ends in one atomic per channel: spread a long reduction over `rep` partial rows (as if
        # they were samples) so that no address takes more than ~128 of them, then add the partials
        rep, s, c = _spread(x1)
        n = rep
    # (both sums: adjacent outputs, cleared by one launch or by the step's zero pool)
    sums, flag = _sums((int(want_sum) + int(want_dot), n, c), x1.device)
    s1, s2 = (sums[0] if want_sum else None), (sums[-1] if want_dot else None)
    check(lib.cn_nc_reduce(_ptr(x1), _ptr(x2), _ptr(s1), _ptr(s2), n, s, c, flags | flag, slope, _dt(x1), _stream()), "cn_nc_reduce")
    sums = _readd(sums, rep, 1)
    return (sums[0] if want_sum else None), (sums[-1] if want_dot else None)


def nc_reduce4(x, slope):
    """(sum x, sum x^2, sum l, sum l^2) per (n, c) with l = leaky_relu(x, slope): cn_nc_reduce4 (one pass instead of two)."""
    n, s, c = _nsc(x)
    out, flags = _sums((4, n, c), x.device)
    check(lib.cn_nc_reduce4(_ptr(x), _ptr(out), n, s, c, slope, flags, _dt(x), _stream()), "cn_nc_reduce4")
    return out[0], out[1], out[2], out[3]


def nc_lin2(shape, x1=None, a1=None, x2=None, a2=None, b=None, flags=0, slope=0.0, per_channel=False, a3=None, b3=None,
            x2_period=0, out=None):
    """y = a1*f1(x1) + a2*f2(x2) + b with (n,c) [or (c,)] coefficients broadcast over space.
    x2_period: as in nc_reduce.  out: write into this (contiguous) tensor instead of a new one."""
    n, c = shape[0], shape[-1]
    s = int(math.prod(shape)) // (n * c)
    x1, x2 = _unify(x1, x2)
    if flags & 4:
        _log_mask(x2)                              # the result is multiplied by lrelu'(x2)
    ref = x1 if x1 is not None else (x2 if x2 is not None else b)
    dtype = ref.dtype if (x1 is not None or x2 is not None) else _act_out_dtype(c)
    if out is not None:
        assert out.is_contiguous() and out.numel() == int(math.prod(shape))
        if out.dtype != dtype:                     # the caller's buffer decides the storage type
            x1, x2 = (None if x1 is None else cast(x1, out.dtype)), (None if x2 is None else cast(x2, out.dtype))
        y = out
    else:
        y = torch.empty(shape, device=ref.device, dtype=dtype)
    flags |= x2_period << 8
    check(lib.cn_nc_lin2(_ptr(x1), _fptr(a1), _ptr(x2), _fptr(a2), _fptr(b), _fptr(a3), _fptr(b3), _ptr(y), n, s, c,
                         0 if per_channel else c, flags, slope, _dt(y), _stream()), "cn_nc_lin2")
    return y


NORM_ADAIN, NORM_INSTANCE, NORM_STYLE = 0, 1, 2


def norm_coef_fwd(mode, s1, s2, p1, p2, spatial, eps, x=None):
    """x (NORM_ADAIN): the normalised tensor, read by channels whose one-pass variance cannot be trusted (cn_norm_coef_fwd)."""
    n, c = s1.shape
    A = torch.empty((n, 2 * c) if mode == NORM_STYLE else (n, c), device=s1.device, dtype=torch.float32)
    B = torch.empty((n, c), device=s1.device, dtype=torch.float32) if mode != NORM_STYLE else None
    mean = torch.empty((n, c), device=s1.device, dtype=torch.float32)
    r = torch.empty((n, c), device=s1.device, dtype=torch.float32)
    check(lib.cn_norm_coef_fwd(mode, _ptr(s1), _ptr(s2), _ptr(p1), _ptr(p2), _ptr(A), _ptr(B), _ptr(mean), _ptr(r),
                               n, c, spatial, eps, _ptr(x), CN_F32 if x is None else _dt(x), _stream()), "cn_norm_coef_fwd")
    return A, B, mean, r


def norm_coef_bwd(mode, t1, t2, mean, r, p1, spatial, eps):
    n, c = mean.shape
    dev = mean.device
    c1 = torch.empty((n, c), device=dev, dtype=torch.float32) if mode != NORM_STYLE else None
    c2 = torch.empty((n, c), device=dev, dtype=torch.float32)
    c0 = torch.empty((n, c), device=dev, dtype=torch.float32)
    gp1 = gp2 = None
    if mode == NORM_ADAIN:
        gp1 = torch.empty((n, 2 * c), device=dev, dtype=torch.float32)
    elif mode == NORM_INSTANCE:
        gp1 = torch.empty((c,), device=dev, dtype=torch.float32)
        gp2 = torch.empty((c,), device=dev, dtype=torch.float32)
    check(lib.cn_norm_coef_bwd(mode, _ptr(t1), _ptr(t2), _ptr(mean), _ptr(r), _ptr(p1), _ptr(c1), _ptr(c2), _ptr(c0),
                               _ptr(gp1), _ptr(gp2), n, c, spatial, eps, _stream()), "cn_norm_coef_bwd")
    return c1, c2, c0, gp1, gp2


# AdaIn / instance norm: the coefficient algebra inline in the apply / backward pass (cn_norm_apply) where it fits.  -110 launches per
# iteration; on the iteration's time it is neutral for fp32 storage (425.8 against 426.1 images/s, alternating runs) and was -0.3 %
# for bf16 storage (762.4 against 764.8: every workgroup of the short bf16 pass starts with the dependent loads of the statistics),
# so bf16 tensors keep the separate coefficient launch.
NORM_APPLY = True


def norm_apply_fwd(mode, x, s1, s2, p1, p2, eps, flags=0, slope=0.0):
    """(y, mean, r) = the apply pass of AdaIn / instance norm with its coefficients computed inline (cn_norm_apply, dir 0), or None
    where the launch does not fit (the caller then runs norm_coef_fwd + nc_lin2)."""
    if not NORM_APPLY or x.shape[-1] % 4 or x.dtype != torch.float32:
        return None
    n, s, c = _nsc(x)
    y = torch.empty_like(x)
    mean = torch.empty((n, c), device=x.device, dtype=torch.float32)
    r = torch.empty_like(mean)
    rc = lib.cn_norm_apply(mode, 0, _ptr(x), None, _fptr(s1), _fptr(s2), _fptr(_c(p1)), _fptr(None if p2 is None else _c(p2)), _ptr(mean), _ptr(r),
                           None, None, None, None, _ptr(y), n, s, c, eps, flags, slope, _dt(x), _stream())
    if rc == CN_EUNSUPPORTED:
        return None
    check(rc, "cn_norm_apply")
    return y, mean, r


def norm_apply_bwd(mode, gy, x, t1, t2, mean, r, p1, eps, flags=0, slope=0.0, a3=None, b3=None):
    """(gx, gp1, gp2) = the input gradient of AdaIn / instance norm with the coefficients inline (cn_norm_apply, dir 1) and the
    parameter gradients (mode 0: gp1 = d[s|b] (n, 2c); mode 1: d gamma, d beta), or None where the launch does not fit."""
    if not NORM_APPLY or x.shape[-1] % 4 or x.dtype != torch.float32 or gy.dtype != torch.float32:
        return None
    gy, x = _unify(gy, x)
    n, s, c = _nsc(x)
    if flags & 4:
        _log_mask(x)
    gx = torch.empty_like(x)
    if mode == NORM_ADAIN:
        gp1, gp2 = torch.empty((n, 2 * c), device=x.device, dtype=torch.float32), None
    else:
        gp1 = torch.empty((c,), device=x.device, dtype=torch.float32)
        gp2 = torch.empty_like(gp1)
    rc = lib.cn_norm_apply(mode, 1, _ptr(gy), _ptr(x), _fptr(t1), _fptr(t2), _fptr(_c(p1)), None, _ptr(mean), _ptr(r), _ptr(gp1), _ptr(gp2),
                           _fptr(a3), _fptr(b3), _ptr(gx), n, s, c, eps, flags, slope, _dt(x), _stream())
    if rc == CN_EUNSUPPORTED:
        return None
    check(rc, "cn_norm_apply")
    return gx, gp1, gp2


def dual_tail_coef_fwd(T, U, mean, q, sm, ssd, gamma, spatial, eps=1e-3):
    """T = (T1, T2) or None (no ty wanted); U = (U1, U2) or None (no tstyle wanted).  One head at a time: the rows of T / U
    are the samples of the primal statistics.  Batched (both given): U holds the N samples of the head that leaves through the
    style statistics, T the (heads - 1) * N samples that go on, against N samples of primal statistics."""
    ref = mean if mean is not None else sm
    period, c = ref.shape
    mk = lambda *sh: torch.empty(sh, device=ref.device, dtype=torch.float32)
    C1 = C2 = C0 = ts = None
    n_inst = n_style = 0
    if T is not None:
        n_inst = T[0].shape[0]
        C1, C2, C0 = mk(n_inst, c), mk(n_inst, c), mk(n_inst, c)
    if U is not None:
        n_style = U[0].shape[0]
        ts = mk(n_style, 2 * c)
    T1, T2 = T if T is not None else (None, None)
    U1, U2 = U if U is not None else (None, None)
    check(lib.cn_dual_tail_coef_fwd(_ptr(T1), _ptr(T2), _ptr(U1), _ptr(U2), _ptr(mean), _ptr(q), _ptr(sm), _ptr(ssd),
                                    _ptr(gamma), _ptr(C1), _ptr(C2), _ptr(C0), _ptr(ts), n_inst + n_style, c, spatial, eps,
                                    n_style, period, _stream()),
          "cn_dual_tail_coef_fwd")
    return C1, C2, C0, ts


def dual_tail_coef_bwd(H, E, u, T, U, mean, q, sm, ssd, gamma, spatial, eps=1e-3):
    """Returns dict of coefficient tensors (see include/confignet_hip.h).  Row counts as in dual_tail_coef_fwd: the
    instance-norm group follows H (sum h ...), the style group follows u."""
    ref = mean if mean is not None else sm
    period, c = ref.shape
    names = ["K1", "K2", "K0", "D2", "D0", "kh", "kt", "ka", "kc", "et", "ex", "e0", "ggamma", "ggamma_rows"]
    out = {k: None for k in names}
    mk = lambda *sh: torch.empty(sh, device=ref.device, dtype=torch.float32)
    n_inst = n_style = 0
    if H is not None:
        n_inst = H[0].shape[0]
        for k in ("K1", "K2", "K0", "kh", "kt", "ka", "kc", "ggamma_rows"):
            out[k] = mk(n_inst, c)
        out["ggamma"] = mk(c)
    if u is not None:
        n_style = u.shape[0]
        for k in ("D2", "D0", "et", "ex", "e0"):
            out[k] = mk(n_style, c)
    arr = (ctypes.c_void_p * 14)(*[(out[k].data_ptr() if out[k] is not None else None) for k in names])
    H1, H2p = H if H is not None else (None, None)
    T1, T2 = T if T is not None else (None, None)
    U1, U2 = U if U is not None else (None, None)
    check(lib.cn_dual_tail_coef_bwd(_ptr(H1), _ptr(H2p), _ptr(E), _ptr(u), _ptr(T1), _ptr(T2), _ptr(U1), _ptr(U2),
                                    _ptr(mean), _ptr(q), _ptr(sm), _ptr(ssd), _ptr(gamma), arr, n_inst + n_style, c, spatial, eps,
                                    n_style, period, _stream()),
          "cn_dual_tail_coef_bwd")
    return out


def dual_tail_gx(h, ta, tx, x, co, slope):
    """h / ta may hold a multiple of x's samples (batched tangent pass: the heads that share this activation, summed here)."""
    h, ta, tx, x = _unify(h, ta, tx, x)
    _log_mask(x)
    n, s, c = _nsc(x)
    nrep = 1 if h is None else h.shape[0] // n
    assert h is None or (h.shape[0] == nrep * n and ta.shape[0] == nrep * n)
    out = torch.empty_like(x)
    check(lib.cn_dual_tail_gx(_ptr(h), _ptr(ta), _ptr(tx), _ptr(x), _ptr(co["kh"]), _ptr(co["kt"]), _ptr(co["ka"]),
                              _ptr(co["kc"]), _ptr(co["et"]), _ptr(co["ex"]), _ptr(co["e0"]), _ptr(out), n, s, c, slope,
                              nrep, _dt(x), _stream()), "cn_dual_tail_gx")
    return out


def dual_tail_gx_tx(h, ta, tx, x, co, slope, ta_is_tx=False):
    """(g_x, g_tx): dual_tail_gx and, from the same pass, the gradient w.r.t. the stacked tangent input tx (its first N samples
    the style head's D2 x + D0, then per head lrelu'(x) (K1 h + K2 lrelu(x) + K0)): cn_dual_tail_gx_tx."""
    h, ta, tx, x = _unify(h, ta, tx, x)
    _log_mask(x)
    n, s, c = _nsc(x)
    nrep = h.shape[0] // n
    assert h.shape[0] == nrep * n and ta.shape[0] == nrep * n and tx.shape[0] == (nrep + 1) * n
    out = torch.empty_like(x)
    out_tx = torch.empty_like(tx)
    check(lib.cn_dual_tail_gx_tx(_ptr(h), _ptr(ta), _ptr(tx), _ptr(x), _ptr(co["kh"]), _ptr(co["kt"]), _ptr(co["ka"]), _ptr(co["kc"]),
                                 _ptr(co["et"]), _ptr(co["ex"]), _ptr(co["e0"]), _ptr(co["K1"]), _ptr(co["K2"]), _ptr(co["K0"]),
                                 _ptr(co["D2"]), _ptr(co["D0"]), _ptr(out), _ptr(out_tx), n, s, c, slope, nrep, int(ta_is_tx), _dt(x), _stream()),
          "cn_dual_tail_gx_tx")
    return out, out_tx


def nc_reduce_hxt(h, x, ta, slope, ta_is_tx=False):
    """(sum h, sum h lrelu(x), sum h ta) per (n, c) of h in ONE pass (cn_nc_reduce_hxt); x holds h.shape[0] / k samples.
    ta_is_tx: `ta` is the tangent input tx, ta = lrelu'(x) tx is formed in the pass."""
    h, x, ta = _unify(h, x, ta)
    n, s, c = _nsc(h)
    out, flags = _sums((3, n, c), h.device)
    check(lib.cn_nc_reduce_hxt(_ptr(h), _ptr(x), _ptr(ta), _ptr(out), n, s, c, slope, x.shape[0], flags | (32 if ta_is_tx else 0), _dt(h),
                               _stream()), "cn_nc_reduce_hxt")
    return out[0], out[1], out[2]


def bn_act_bwd(gy, y, x, a, act, want_g):
    """(gx, g | None, sum_c g, sum_c g*x): cn_bn_act_bwd -- activation backward, BatchNorm(inference) input gradient and the two
    per-channel parameter sums in one pass over gy / y / x."""
    gy, y, x = _unify(gy, y, x)
    _log_mask(y, act)
    rep, s, c = _spread(gy)
    gx = torch.empty_like(gy)
    g = torch.empty_like(gy) if want_g else None
    s12, flags = _sums((2, rep, c), gy.device)
    check(lib.cn_bn_act_bwd(_ptr(gy), _ptr(y), _ptr(x), _fptr(_c(a)), _ptr(g), _ptr(gx), _ptr(s12[0]), _ptr(s12[1]), rep, s, c,
                            act, flags, _dt(gy), _stream()), "cn_bn_act_bwd")
    s12 = _readd(s12, rep, 1).reshape(2, c)
    return gx, g, s12[0], s12[1]


def nc_reduce_dact(x1, x2, act, slope, x2_period=0, flags=0, want_dot=True, want_a=True):
    """(a, sum_s a, sum_s a * f2(x2)) with a = x1 * act'(x2): cn_nc_reduce_dact (one pass instead of act_bwd + nc_reduce).
    want_a = False: the sums only (a is not stored: None)."""
    x1, x2 = _unify(x1, x2)
    _log_mask(x2, act)
    n, s, c = _nsc(x1)
    a = torch.empty_like(x1) if want_a else None
    s12, flag = _sums((2, n, c), x1.device)
    check(lib.cn_nc_reduce_dact(_ptr(x1), _ptr(x2), _ptr(s12[0]), _ptr(s12[1]) if want_dot else None, _ptr(a), n, s, c,
                                flags | flag | x2_period << 8, slope, act, _dt(x1), _stream()), "cn_nc_reduce_dact")
    return a, s12[0], (s12[1] if want_dot else None)


# ---------------------------------------------------------------------------------------------
# Test instrument (tests/test_nets_gpu.py: whole-step gradient parity): with `branch_log()` active every backward-pass site that
# evaluates a piecewise-linear derivative -- LeakyReLU / ReLU masks, max-pool arg-max -- appends the tensor its decisions are
# taken from (as a host-side boolean mask `t > 0`, or the pool's fp32 input) to the list.  The float64 oracle then FORCES the
# same decisions (oracle.ref_ops.BranchControl(forced=...)), so product and oracle gradients differ by summation error only.
# Off (None) in the product path: one `is not None` test per call.
# ---------------------------------------------------------------------------------------------
BRANCH_LOG = None


class branch_log:
    def __enter__(self):
        global BRANCH_LOG
        BRANCH_LOG = self.log = []
        return self.log

    def __exit__(self, *exc):
        global BRANCH_LOG
        BRANCH_LOG = None


def _log_mask(t, act=None):
    if BRANCH_LOG is not None and (act is None or act in (ACT_LRELU, ACT_RELU)):
        BRANCH_LOG.append(("act", (t.detach().float() > 0).reshape(-1).cpu()))


# ---------------------------------------------------------------------------------------------
# Test instrument (tests/test_bf16_grads_gpu.py: bf16 network gradients at the product's own forward state): with `stored_log()`
# active the generator, the discriminator / latent regressor and their blocks append every activation tensor they hand from one
# kernel to the next -- the points oracle.ref_nets marks with `O.stored(...)`, in forward order -- as a host copy of the value as
# it is STORED (a tensor that is still fp32 at its site and converted by the consuming convolution, the generator's learned
# constant, is logged in the activation type).  The oracle then REPLAYS these values (oracle.ref_ops.StoredReplay), so both
# gradients are taken at one forward state.  Off (None) in the product path: one `is not None` test per site.
# ---------------------------------------------------------------------------------------------
STORED_LOG = None


class stored_log:
    def __enter__(self):
        global STORED_LOG
        STORED_LOG = self.log = []
        return self.log

    def __exit__(self, *exc):
        global STORED_LOG
        STORED_LOG = None


def _log_stored(t):
    if STORED_LOG is not None:
        STORED_LOG.append(t.detach().to(_act_out_dtype(t.shape[-1])).float().cpu())


def act_fwd(x, act, slope=0.0):
    y = torch.empty_like(x)
    check(lib.cn_act_fwd(_ptr(x), _ptr(y), x.numel(), act, slope, _dt(x), _stream()), "cn_act_fwd")
    return y


def act_bwd(gy, y, act, slope=0.0):
    gy, y = _unify(gy, y)
    _log_mask(y, act)
    gx = torch.empty_like(gy)
    check(lib.cn_act_bwd(_ptr(gy), _ptr(y), _ptr(gx), gy.numel(), act, slope, _dt(gy), _stream()), "cn_act_bwd")
    return gx


def act_bwd_partials(gy, y, act, slope=0.0):
    """(gx, partial (rep, c)): act_bwd and the per-channel sums of its result over `rep` row slices, in one pass
    (cn_act_bwd_bias); the caller adds the slices (sum_rows_into)."""
    gy, y = _unify(gy, y)
    _log_mask(y, act)
    rep, s, c = _spread(gy)                          # as nc_reduce(per_channel=True)
    gx = torch.empty_like(gy)
    gb, flags = _sums((rep, c), gy.device)
    check(lib.cn_act_bwd_bias(_ptr(gy), _ptr(y), _ptr(gx), _ptr(gb), rep, s, c, act, slope, flags, _dt(gy), _stream()),
          "cn_act_bwd_bias")
    return gx, gb


def act_bwd_bias(gy, y, act, slope=0.0, sink=None):
    """(gx, gb): act_bwd fused with the per-channel sum of its result (the bias gradient) -- one pass instead of two.
    sink: the bias's slot of a gradient arena (grad_sink) -- the sum is ADDED there and gb is returned as None."""
    gx, gb = act_bwd_partials(gy, y, act, slope)
    if sink is not None:
        sum_rows_into(gb, sink)
        return gx, None
    return gx, _readd(gb, gb.shape[0], 0).reshape(-1)


def sum_rows_into(partial, dst, accumulate=True, defer=True):
    """dst[c] (+)= sum_r partial[r][c] (cn_sum_rows_into), on the calling stream; under a grad_sink the sum joins the pass' grouped
    reduction launch unless defer=False."""
    rows, c = partial.shape
    st = _SINK
    if st is not None:
        st.note_stream()
        if defer and accumulate and partial.dtype == torch.float32 and partial.is_contiguous():
            # a leaf of the backward pass: joins the pass' grouped reduction launch (grad_sink.join) -- dst[c] += sum_r partial[r][c] is
            # the ordered slab sum of `rows` parts of c floats; flag 2 keeps the serial order of cn_sum_rows_into for any row count
            st.slabs.append((partial, dst, rows, c, 1 | 2))
            return
    check(lib.cn_sum_rows_into(_fptr(partial), _fptr(dst), rows, c, int(accumulate), _stream()), "cn_sum_rows_into")


def bias_grad(gy, sink=None):
    """sum over every axis but the last of gy (the bias gradient of a linear / convolution layer without fused activation)."""
    gy = _c(gy)
    if sink is None:
        return nc_reduce(gy, None, want_dot=False, per_channel=True)[0].reshape(-1)
    rep, s, c = _spread(gy)
    if rep * s <= 64 and gy.dtype == torch.float32 and _SINK is not None:
        # a dense layer's bias gradient over a batch of a few rows: the rows ARE the slabs of the pass' grouped reduction
        # (grad_sink.join) -- no launch of its own
        sum_rows_into(gy.reshape(s, c), sink)
        return None
    part, flags = _sums((rep, c), gy.device)
    check(lib.cn_nc_reduce(_ptr(gy), None, _ptr(part), None, rep, s, c, flags, 0.0, _dt(gy), _stream()), "cn_nc_reduce")
    sum_rows_into(part, sink)
    return None


def axpby(x, y, a, b):
    x, y = _unify(x, y)
    out = torch.empty_like(x)
    check(lib.cn_axpby(_ptr(x), _ptr(y), _ptr(out), x.numel(), a, b, _dt(x), _stream()), "cn_axpby")
    return out


def mul(x, y):
    x, y = _unify(x, y)
    out = torch.empty_like(x)
    check(lib.cn_mul(_ptr(x), _ptr(y), _ptr(out), x.numel(), _dt(x), _stream()), "cn_mul")
    return out


def sqdiff_sum(a, b, scale):
    a, b = _unify(a, b)
    out = torch.zeros((1,), device=a.device, dtype=torch.float32)
    check(lib.cn_sqdiff_sum(_ptr(a), _ptr(b), _ptr(out), a.numel(), scale, _dt(a), _stream()), "cn_sqdiff_sum")
    return out


def row_sumsq(x):
    x = f32(x)
    n = x.shape[0]
    out = torch.empty((n,), device=x.device, dtype=torch.float32)
    check(lib.cn_row_sumsq(_ptr(x), _ptr(out), n, x.numel() // n, _stream()), "cn_row_sumsq")
    return out


def row_scale(x, s, k):
    out = torch.empty_like(x)
    check(lib.cn_row_scale(_ptr(x), _fptr(s), _ptr(out), x.shape[0], x.numel() // x.shape[0], k, _dt(x), _stream()), "cn_row_scale")
    return out


def row_scale_diff(a, b, s, k):
    """(a - b) * s[row] * k in one pass (the backward of sqdiff_sum: s = the incoming scalar gradient, one row)."""
    a, b = _unify(a, b)
    out = torch.empty_like(a)
    check(lib.cn_row_scale_diff(_ptr(a), _ptr(b), _fptr(s), _ptr(out), s.numel(), a.numel() // s.numel(), k, _dt(a), _stream()), "cn_row_scale_diff")
    return out


def maxpool2_bwd_relu(x, gy, target=None, s=None, k=0.0):
    """Backward of ReLU -> MaxPooling2D(2, 2) in one pass (cn_maxpool2_bwd_act): (routed gy [+ (x - target) s k]) relu'(x) for the ReLU
    output x that was pooled; None where the kernel does not take the shape (the caller then runs the two passes)."""
    n, h, w, c = x.shape
    if target is None:
        x, gy = _unify(x, gy)
    else:
        x, gy, target = _unify(x, gy, target)
    if s is not None and s.numel() not in (1, n):
        return None
    gx = torch.empty_like(x)
    rc = lib.cn_maxpool2_bwd_act(_ptr(x), _ptr(_c(gy)), _ptr(target), _fptr(s), k, _ptr(gx), n, h, w, c, 1 if s is None else s.numel(), _dt(x),
                                 _stream())
    if rc == CN_EUNSUPPORTED:
        return None
    check(rc, "cn_maxpool2_bwd_act")
    if BRANCH_LOG is not None:                     # (test instrument: the pool's arg-max decisions and the ReLU mask, as the two passes log them)
        BRANCH_LOG.append(("pool", x.detach().float().cpu(), (2, 2, 0)))
    _log_mask(x, ACT_RELU)
    return gx


def tap_bwd(y, target, g, s, k, act, slope=0.0):
    """(g + (y - target) s[row] k) act'(y) in one pass (cn_tap_bwd); g may be None; s: one scale per row (s.numel() rows)."""
    if g is None:
        y, target = _unify(y, target)
    else:
        y, target, g = _unify(y, target, _c(g))
    _log_mask(y, act)
    out = torch.empty_like(y)
    check(lib.cn_tap_bwd(_ptr(y), _ptr(target), _ptr(g), _fptr(s), _ptr(out), s.numel(), y.numel() // s.numel(), k, act, slope, _dt(y),
                         _stream()), "cn_tap_bwd")
    return out


def masked_diff(a, b, mask):
    a, b = f32(a), f32(b)
    out = torch.empty_like(a)
    check(lib.cn_masked_diff(_ptr(a), _ptr(b), _ptr(mask), _ptr(out), mask.numel(), a.shape[-1], _stream()), "cn_masked_diff")
    return out


def maxpool_fwd(x, k, s, pad):
    n, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    y = torch.empty((n, oh, ow, c), device=x.device, dtype=x.dtype)
    check(lib.cn_maxpool_fwd(_ptr(x), _ptr(y), n, h, w, c, k, s, pad, _dt(x), _stream()), "cn_maxpool_fwd")
    return y


def avgpool3_same(x):
    """AveragePooling2D((3, 3), strides 1, padding "same"); padding cells are not counted."""
    n, h, w, c = x.shape
    x = _c(x)
    y = torch.empty_like(x)
    check(lib.cn_avgpool3_same(_ptr(x), _ptr(y), n, h, w, c, _dt(x), _stream()), "cn_avgpool3_same")
    return y


def dwconv3x3_fwd(x, w, bias, stride, act=ACT_NONE, slope=0.0):
    """keras DepthwiseConv2D(3, strides=stride, depth_multiplier=1) on an NHWC fp32 tensor, TF "same" padding (the
    ZeroPadding2D(correct_pad) + VALID pair of MobileNetV2's stride-2 layers pads the same), + per-channel bias, + activation:
    (n, h, w, c) -> (n, ceil(h / stride), ceil(w / stride), c).  w: the Keras kernel (3, 3, c, 1)."""
    x = _c(f32(x))
    n, h, wd, c = x.shape
    assert tuple(w.shape) in ((3, 3, c, 1), (3, 3, c)), "depthwise kernel (3, 3, %d, 1) expected, got %s" % (c, tuple(w.shape))
    assert bias is None or tuple(bias.shape) == (c,)
    y = torch.empty((n, -(-h // stride), -(-wd // stride), c), device=x.device, dtype=torch.float32)
    check(lib.cn_dwconv3x3_fwd(_ptr(x), _fptr(_c(w)), _fptr(None if bias is None else _c(bias)), _ptr(y), n, h, wd, c, stride, act, slope,
                               _stream()), "cn_dwconv3x3_fwd")
    return y


def dwconv3x3_dgrad(gy, w, in_shape, stride, out=None):
    """Input gradient of dwconv3x3_fwd (no bias, no activation): gy (n, ceil(h / stride), ceil(w / stride), c) -> gx
    in_shape = (n, h, w, c) (cn_dwconv3x3_dgrad, a gather).  out: write into this contiguous tensor."""
    gy = _c(f32(gy))
    n, h, wd, c = (int(v) for v in in_shape)
    assert tuple(gy.shape) == (n, -(-h // stride), -(-wd // stride), c), (tuple(gy.shape), tuple(in_shape), stride)
    assert tuple(w.shape) in ((3, 3, c, 1), (3, 3, c))
    gx = out if out is not None else torch.empty((n, h, wd, c), device=gy.device, dtype=torch.float32)
    assert gx.is_contiguous() and gx.numel() == n * h * wd * c
    check(lib.cn_dwconv3x3_dgrad(_ptr(gy), _fptr(_c(w)), _fptr(gx), n, h, wd, c, stride, _stream()), "cn_dwconv3x3_dgrad")
    return gx


def _slice_partials(query, dims, cols, device, name, launch):
    """The per-slice partials (slices, cols) of a per-channel training reduction: slices = query(*dims), the library's own count;
    launch(part pointer, slices) is the checked call `name` that fills them."""
    slices = query(*dims)
    if slices <= 0:
        check(slices, query.__name__)
    part = torch.empty((slices, cols), device=device, dtype=torch.float32)
    check(launch(_fptr(part), slices), name)
    return part


def dwconv3x3_wgrad(x, gy, stride, out=None, accumulate=True, defer=True):
    """Filter gradient (3, 3, c, 1) of dwconv3x3_fwd.  cn_dwconv3x3_wgrad leaves one partial filter per slice of output pixels
    (the library's plan: cn_dwconv3x3_wgrad_slices) and sum_rows_into adds the slices in slice order -- as every per-channel
    reduction with partial rows here, with no atomics, so the default and the deterministic mode give the same bits.
    out: ADD the gradient to this tensor (a slot of a gradient arena); out with accumulate=False: WRITE it there.  Inside a
    grad_sink an accumulating sum joins the pass' grouped reduction unless defer=False (as conv_wgrad)."""
    x, gy = _c(f32(x)), _c(f32(gy))
    n, h, wd, c = x.shape
    assert tuple(gy.shape) == (n, -(-h // stride), -(-wd // stride), c), (tuple(gy.shape), tuple(x.shape), stride)
    part = _slice_partials(lib.cn_dwconv3x3_wgrad_slices, (n, h, wd, c, stride), 9 * c, x.device, "cn_dwconv3x3_wgrad",
                           lambda p, slices: lib.cn_dwconv3x3_wgrad(_ptr(x), _ptr(gy), p, slices, n, h, wd, c, stride, _stream()))
    if out is None:
        out, accumulate = torch.empty((3, 3, c, 1), device=x.device, dtype=torch.float32), False
    assert out.is_contiguous() and out.numel() == 9 * c and out.dtype == torch.float32
    sum_rows_into(part, out.view(-1), accumulate=accumulate, defer=defer)
    return out


def sink_dwconv3x3_wgrad(x, gy, stride, slot):
    """The depthwise filter gradient ADDED into its gradient-arena slot (a leaf of the backward pass, as sink_conv_wgrad)."""
    dwconv3x3_wgrad(x, gy, stride, out=slot)


BN_MOMENTUM = 0.99


def bn_train_fwd(x, gamma, beta, moving_mean=None, moving_var=None, act=ACT_NONE, eps=1e-3, momentum=BN_MOMENTUM, bessel=True):
    """Training-mode BatchNormalization over every axis but the last, then `act` (ACT_NONE / ACT_RELU6): one reduce pass
    (nc_reduce per channel), the coefficients (cn_bn_train_coef: a = gamma rsqrt(var + eps), b = beta - mean a; it also
    updates the moving statistics IN PLACE, the variance Bessel-corrected if `bessel`), one apply pass y = act(a x + b).
    Returns (y, saved) with saved = (mean, var, r, a) per channel for bn_train_bwd (var: the biased batch variance)."""
    x = _c(f32(x))
    c = x.shape[-1]
    m = x.numel() // c
    s1, s2 = nc_reduce(x, None, per_channel=True)
    co = torch.empty((5, c), device=x.device, dtype=torch.float32)                 # mean | var | r | a | b
    check(lib.cn_bn_train_coef(_fptr(_c(s1)), _fptr(_c(s2)), _fptr(_c(gamma)), _fptr(_c(beta)), _fptr(x), _fptr(co[0]), _fptr(co[1]),
                               _fptr(co[2]), _fptr(co[3]), _fptr(co[4]), _fptr(moving_mean), _fptr(moving_var), m, c, eps, momentum,
                               int(bool(bessel)), _stream()), "cn_bn_train_coef")
    y = torch.empty_like(x)
    check(lib.cn_bn_train_apply(_fptr(x), _fptr(co[3]), _fptr(co[4]), _fptr(y), m, c, act, _stream()), "cn_bn_train_apply")
    return y, (co[0], co[1], co[2], co[3])


def bn_train_bwd(gy, y, x, saved, act=ACT_NONE):
    """(gx, dgamma, dbeta) of bn_train_fwd: g = gy 1[0 < y < 6] (ACT_RELU6; y may be None for ACT_NONE), dbeta = sum g,
    dgamma = sum g xh in one reduce pass (cn_bn_train_bwd_reduce, per-slice partials added in slice order), then
    gx = a (g - (dbeta + xh dgamma) / m) in one apply pass (cn_bn_train_bwd_apply)."""
    mean, _, r, a = saved
    gy, x = _c(f32(gy)), _c(f32(x))
    c = x.shape[-1]
    m = x.numel() // c
    if BRANCH_LOG is not None and act == ACT_RELU6:
        BRANCH_LOG.append(("relu6", ((y.detach() > 0) & (y.detach() < 6)).reshape(-1).cpu()))
    yp = _fptr(y) if act == ACT_RELU6 else None
    part = _slice_partials(lib.cn_bn_train_bwd_slices, (m, c), 2 * c, x.device, "cn_bn_train_bwd_reduce",
                           lambda p, slices: lib.cn_bn_train_bwd_reduce(_fptr(gy), yp, _fptr(x), _fptr(mean), _fptr(r), p, slices, m, c, act, _stream()))
    sums = torch.empty(2 * c, device=x.device, dtype=torch.float32)
    # not sum_rows_into(..., accumulate=False, defer=False): the same one call, but under a grad_sink it also books this stream as one the
    # sink launched on -- with frozen kernels (only gamma / beta trained) no sink launch is on it, and the join would newly wait on it
    check(lib.cn_sum_rows_into(_fptr(part), _fptr(sums), part.shape[0], 2 * c, 0, _stream()), "cn_sum_rows_into")
    gx = torch.empty_like(x)
    check(lib.cn_bn_train_bwd_apply(_fptr(gy), yp, _fptr(x), _fptr(mean), _fptr(r), _fptr(a), _fptr(sums), _fptr(gx), m, c, act,
                                    _stream()), "cn_bn_train_bwd_apply")
    return gx, sums[c:], sums[:c]


def image_preprocess(imgs, out_hw, from_signed=False):
    """A batch of images (n, h, w, c), uint8 or float32 in pixel units [0, 255], -> the MobileNetV2 input (n, out_h, out_w, c)
    fp32 in one launch: bilinear resampling with half-pixel centres and edge clamping (cv2.resize INTER_LINEAR) when the size
    differs, then keras mobilenet_v2.preprocess_input (x / 127.5 - 1).  from_signed: float input in [-1, 1], mapped
    (x + 1) * 127.5 first.  uint8 input is interpolated in float: cv2's 11-bit fixed-point uint8 path is not reproduced, so
    results can differ from a cv2.resize of the same uint8 image by about one grey level before the scaling."""
    imgs = _c(imgs)
    assert imgs.dtype in (torch.uint8, torch.float32), imgs.dtype
    n, h, wd, c = imgs.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    y = torch.empty((n, oh, ow, c), device=imgs.device, dtype=torch.float32)
    mul, add = (127.5, 127.5) if from_signed else (1.0, 0.0)
    check(lib.cn_image_preprocess(_ptr(imgs), CN_U8 if imgs.dtype == torch.uint8 else CN_F32, _ptr(y), n, h, wd, c, oh, ow, mul, add,
                                  _stream()), "cn_image_preprocess")
    return y


def maxpool_bwd(x, gy, k, s, pad):
    n, h, w, c = x.shape
    x, gy = _unify(x, gy)
    if BRANCH_LOG is not None:                     # the kernel's decision: first maximum of a window in row-major order
        BRANCH_LOG.append(("pool", x.detach().float().cpu(), (k, s, pad)))
    gx = torch.empty_like(x)
    check(lib.cn_maxpool_bwd(_ptr(x), _ptr(gy), _ptr(gx), n, h, w, c, k, s, pad, _dt(x), _stream()), "cn_maxpool_bwd")
    return gx


def chan_affine3_fwd(x, perm, scale, off):
    x = f32(x)
    y = torch.empty_like(x)
    check(lib.cn_chan_affine3_fwd(_ptr(x), _ptr(y), x.numel() // 3, (ctypes.c_int * 3)(*perm), scale,
                                  (ctypes.c_float * 3)(*off), _stream()), "cn_chan_affine3_fwd")
    return y


def chan_affine3_bwd(gy, perm, scale):
    gy = f32(gy)
    gx = torch.empty_like(gy)
    check(lib.cn_chan_affine3_bwd(_ptr(gy), _ptr(gx), gy.numel() // 3, (ctypes.c_int * 3)(*perm), scale, _stream()),
          "cn_chan_affine3_bwd")
    return gx


def gan_loss_fwd(s, label):
    out = torch.empty((1,), device=s.device, dtype=torch.float32)
    check(lib.cn_gan_loss_fwd(_ptr(s), _ptr(out), s.numel(), label, _stream()), "cn_gan_loss_fwd")
    return out


def gan_loss_bwd(s, gout, label):
    gs = torch.empty_like(s)
    check(lib.cn_gan_loss_bwd(_ptr(s), _ptr(gout), _ptr(gs), s.numel(), label, _stream()), "cn_gan_loss_bwd")
    return gs


def gemm_rows_grouped(jobs):
    """cn_gemm_rows_grouped_k: every job (a, b, c, bias | None, mask | None, trans_b, act, slope, accumulate) -- c = epi(a op(b) + bias),
    a (m <= 32, k) with any k, contiguous fp32 2-D tensors -- in ONE launch per 16 jobs.  The library decides per launch whether the
    a blocks sit in LDS whole or go through it in K chunks (cn_gemm_rows_grouped_plan reports which)."""
    arr = (CnRowsJob * len(jobs))()
    for q, (a, b, c, bias, mask, tb, act, slope, acc) in zip(arr, jobs):
        q.a, q.b, q.c = _fptr(a).value, _fptr(b).value, _fptr(c).value
        q.bias = None if bias is None else _fptr(bias).value
        q.mask = None if mask is None else _fptr(mask).value
        q.m, q.k = a.shape
        q.n = b.shape[0] if tb else b.shape[1]
        q.lda, q.ldb, q.ldc = a.shape[1], b.shape[1], c.shape[1]
        q.tb, q.act, q.accumulate, q.slope = int(tb), int(act), int(acc), float(slope)
    check(lib.cn_gemm_rows_grouped_k(arr, len(jobs), _stream()), "cn_gemm_rows_grouped_k")


def gan_loss_grouped(scores, labels, gouts=None, backward=False):
    """cn_gan_loss_grouped: the GAN losses of several heads (forward: one (H,) tensor of scalars) or their score gradients
    (backward: a list shaped like `scores`; gouts[j] = the cotangent scalar of head j or None) in ONE launch."""
    jobs = (CnGanJob * len(scores))()
    if backward:
        outs = [torch.empty_like(s_) for s_ in scores]
    else:
        res = torch.empty(len(scores), device=scores[0].device, dtype=torch.float32)
        outs = [res[j:j + 1] for j in range(len(scores))]
    for q, s_, o, lab, j in zip(jobs, scores, outs, labels, range(len(scores))):
        q.s, q.out, q.n, q.label = _fptr(s_).value, o.data_ptr(), s_.numel(), float(lab)
        q.gout = gouts[j].data_ptr() if (backward and gouts[j] is not None) else None
    check(lib.cn_gan_loss_grouped(jobs, len(scores), int(backward), _stream()), "cn_gan_loss_grouped")
    return outs if backward else res


def euler_matrix(angles):
    a = _c(f32(angles)).reshape(-1, 3)
    out = torch.empty((a.shape[0], 3, 3), device=a.device, dtype=torch.float32)
    check(lib.cn_euler_matrix(_ptr(a), _ptr(out), a.shape[0], _stream()), "cn_euler_matrix")
    return out


def euler_matrix_bwd(angles, grot):
    a, g = _c(f32(angles)).reshape(-1, 3), _c(f32(grot)).reshape(-1, 9)
    out = torch.empty_like(a)
    check(lib.cn_euler_matrix_bwd(_ptr(a), _ptr(g), _ptr(out), a.shape[0], _stream()), "cn_euler_matrix_bwd")
    return out


def rotate3d_fwd(grid, rot):
    keep = grid.dtype
    grid = f32(grid)                           # fp32 kernel; a bf16 grid is converted on the way in and out
    out = torch.empty_like(grid)
    n, g, c = grid.shape[0], grid.shape[1], grid.shape[-1]
    check(lib.cn_rotate3d_fwd(_ptr(grid), _fptr(rot), _ptr(out), n, g, c, _stream()), "cn_rotate3d_fwd")
    return cast(out, keep)


def rotate3d_bwd(grid, rot, gout, need_rot):
    n, g, c = grid.shape[0], grid.shape[1], grid.shape[-1]
    keep = grid.dtype
    grid, gout = f32(grid), f32(gout)
    ggrid = torch.empty_like(grid)
    grot = torch.empty((n, 3, 3), device=grid.device, dtype=torch.float32) if need_rot else None
    check(lib.cn_rotate3d_bwd(_ptr(grid), _fptr(rot), _ptr(gout), _ptr(ggrid), _ptr(grot), n, g, c, _stream()),
          "cn_rotate3d_bwd")
    return cast(ggrid, keep), grot


def adam_step(theta, grad, m, v, ema, lr_t, beta1, beta2, eps, ema_alpha=0.999):
    """lr_t: a 1-element float32 CUDA tensor (read by the kernel at execution time)."""
    check(lib.cn_adam_step(_ptr(theta), _ptr(grad), _ptr(m), _ptr(v), _ptr(ema), theta.numel(), _ptr(lr_t), beta1, beta2,
                           eps, ema_alpha, _stream()), "cn_adam_step")


def ema_step(ema, theta, alpha):
    check(lib.cn_ema_step(_ptr(ema), _ptr(theta), theta.numel(), alpha, _stream()), "cn_ema_step")


def gather_images_u8(pool, idx, flip):
    n = idx.numel()
    _, h, w, c = pool.shape
    out = torch.empty((n, h, w, c), device=pool.device, dtype=torch.float32)
    check(lib.cn_gather_images_u8(_ptr(pool), _ptr(idx), _ptr(flip), _ptr(out), n, h, w, c, _stream()),
          "cn_gather_images_u8")
    return out


def _i32ptr(t):
    assert t.dtype == torch.int32, "int32 tensor expected, got %s" % (t.dtype,)
    return _ptr(t)


def hdri_rows_v(pool, y0, wy, oh):
    """cn_hdri_rows_v: pool (P, H, W, 3) fp32 radiance -> (P, oh, W, 3): log2(x + 1), then the vertical half of the area resize
    (y0 (oh) int32 first source rows, wy (oh, T) fp32 weights: hdri.area_table)."""
    pool = _c(pool)
    p, h, w, c = pool.shape
    assert c == 3 and tuple(y0.shape) == (oh,) and wy.shape[0] == oh and wy.dim() == 2
    v = torch.empty((p, oh, w, 3), device=pool.device, dtype=torch.float32)
    check(lib.cn_hdri_rows_v(_fptr(pool), _ptr(v), _i32ptr(y0), _fptr(wy), p, h, w, oh, wy.shape[1], _stream()), "cn_hdri_rows_v")
    return v


def hdri_rows_h(v, idx, shift, x0, wx, ow, mean=None):
    """cn_hdri_rows_h: v (P, oh, W, 3) from hdri_rows_v -> (n, oh, ow, 3): sample i is image idx[i] rolled by shift[i] columns
    (np.roll along the width, any integer) and area-resized to ow columns, minus mean (oh, ow, 3) when given.  idx, shift: (n)
    int32; x0 (ow) int32, wx (ow, T) fp32: hdri.area_table."""
    v = _c(v)
    p, oh, w, c = v.shape
    n = idx.numel()
    assert c == 3 and shift.numel() == n and tuple(x0.shape) == (ow,) and wx.shape[0] == ow and wx.dim() == 2
    assert mean is None or mean.numel() == oh * ow * 3
    out = torch.empty((n, oh, ow, 3), device=v.device, dtype=torch.float32)
    check(lib.cn_hdri_rows_h(_fptr(v), _ptr(out), _i32ptr(idx), _i32ptr(shift), _i32ptr(x0), _fptr(wx),
                             _fptr(None if mean is None else _c(mean)), n, p, w, oh, ow, wx.shape[1], _stream()), "cn_hdri_rows_h")
    return out


def exp2m1(x):
    """2^x - 1 elementwise (cn_exp2m1)."""
    x = _c(x)
    y = torch.empty_like(x)
    check(lib.cn_exp2m1(_fptr(x), _ptr(y), x.numel(), _stream()), "cn_exp2m1")
    return y


def _warp_tables(tables, n, oh, ow):
    x0, y0, adelta, bdelta = tables
    assert tuple(x0.shape) == (n, oh) and tuple(y0.shape) == (n, oh), "x0, y0: one int32 per image and output row"
    assert tuple(adelta.shape) == (n, ow) and tuple(bdelta.shape) == (n, ow), "adelta, bdelta: one int32 per image and output column"
    return [_i32ptr(t) for t in tables]


def warp_affine_u8(src, tables, oh, ow, out=None):
    """cn_warp_affine_u8: cv2.warpAffine (bilinear, constant border 0) of src (n, sh, sw, c) uint8 into (n, oh, ow, c), one
    transform per image as int32 tables (x0 (n, oh), y0 (n, oh), adelta (n, ow), bdelta (n, ow):
    face_image_normalizer.affine_tables with delta 16)."""
    src = _c(src)
    n, sh, sw, c = src.shape
    assert src.dtype == torch.uint8
    ptrs = _warp_tables(tables, n, oh, ow)
    if out is None:
        out = torch.empty((n, oh, ow, c), device=src.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n, oh, ow, c)
    check(lib.cn_warp_affine_u8(_ptr(src), _ptr(out), *ptrs, n, sh, sw, c, oh, ow, _stream()), "cn_warp_affine_u8")
    return out


def warp_nearest_f32(src, tables, oh, ow, out=None):
    """cn_warp_nearest_f32: cv2.warpAffine(flags=INTER_NEAREST) of src (n, sh, sw, c) float32 (tables built with delta 512)."""
    src = _c(src)
    n, sh, sw, c = src.shape
    ptrs = _warp_tables(tables, n, oh, ow)
    if out is None:
        out = torch.empty((n, oh, ow, c), device=src.device, dtype=torch.float32)
    assert tuple(out.shape) == (n, oh, ow, c)
    check(lib.cn_warp_nearest_f32(_fptr(src), _fptr(out), *ptrs, n, sh, sw, c, oh, ow, _stream()), "cn_warp_nearest_f32")
    return out


def eye_mask(uv, bounds, out=None):
    """cn_eye_mask: uv (..., h, w, c >= 2) float32 -> (..., h, w) uint8, 1 where the first two channels lie strictly inside the left
    or the right eye rectangle; bounds = (l_min, l_max, r_min, r_max, y_min, y_max)."""
    uv = _c(uv)
    c = uv.shape[-1]
    if out is None:
        out = torch.empty(uv.shape[:-1], device=uv.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.numel() == uv.numel() // c and len(bounds) == 6
    check(lib.cn_eye_mask(_fptr(uv), _ptr(out), out.numel(), c, *[float(b) for b in bounds], _stream()), "cn_eye_mask")
    return out


def to_uint8(x):
    x = f32(x)
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    check(lib.cn_to_uint8(_ptr(x), _ptr(out), x.numel(), _stream()), "cn_to_uint8")
    return out


_PROF = {"on": False, "saved_flops": 0.0}


def prof_enable(on):
    _PROF["on"] = bool(on)
    check(lib.cn_prof_enable(int(on)), "cn_prof_enable")


def prof_reset():
    _PROF["saved_flops"] = 0.0
    check(lib.cn_prof_reset(), "cn_prof_reset")


def prof_note_saved(flops):
    """Multiply-adds a direct convolution would have issued and the algorithm in use does not (Winograd, parity-class
    collapse of upsample-folded layers): bench.py reports them next to the issued work, never inside `roofline.frac`."""
    if _PROF["on"]:
        _PROF["saved_flops"] += flops


def prof_saved_flops():
    return _PROF["saved_flops"]


def wino_saved_flops(g):
    """direct 3x3 count (border taps included: an upper bound) minus the 16 products per 2x2 tile issued"""
    tiles = g.n * ((g.in_h + 1) // 2) * ((g.in_w + 1) // 2)
    return 2.0 * g.cin * g.cout * (9.0 * g.n * g.in_h * g.in_w - 16.0 * tiles)


def upfold_saved_flops(g):
    """direct count of the conv on the x2-upsampled grid minus the parity-class form: (2/3)^nd of it for k3, (2.5/4)^nd for k4"""
    ks = [k for k in (g.k_d, g.k_h, g.k_w)][3 - g.nd:]
    ratio = 1.0
    for k in ks:
        ratio *= (2.0 / 3.0) if k == 3 else (2.5 / 4.0)
    direct = 2.0 * g.n * g.out_d * g.out_h * g.out_w * g.k_d * g.k_h * g.k_w * g.cin * g.cout
    return direct * (1.0 - ratio)


PROF_FAMILIES = ["igemm_fwd<128x128>", "igemm_fwd<128x64>", "igemm_fwd<64x64>", "igemm_fwd<128x32>", "igemm_fwd<128x96>",
                 "igemm_wgrad<128x128>", "igemm_wgrad<128x96>", "igemm_wgrad<64x64>", "igemm_wgrad<128x32>", "wino_fwd", "c3_fwd",
                 "s2_image_dgrad", "thin / up2k4_rgb", "c3_wgrad", "igemm_bf16", "igemm_bf16_wgrad", "igemm_wgrad<256x64>", "wgrad slab sums (grouped)"]


def prof_collect_by_family():
    """{family: {"launches", "ms", "gflop", "algorithmic_mb"}} of the launches recorded since prof_reset()."""
    n = (ctypes.c_int * 32)()
    ms, fl, by = (ctypes.c_double * 32)(), (ctypes.c_double * 32)(), (ctypes.c_double * 32)()
    check(lib.cn_prof_collect_by_family(n, ms, fl, by), "cn_prof_collect_by_family")
    out = {}
    for i in range(32):
        if n[i]:
            name = PROF_FAMILIES[i] if i < len(PROF_FAMILIES) else "other"
            out[name] = {"launches": int(n[i]), "ms": ms[i], "gflop": fl[i] / 1e9, "algorithmic_mb": by[i] / 1e6}
    return out


def prof_collect():
    n, ms, fl = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0)
    check(lib.cn_prof_collect(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), "cn_prof_collect")
    return n.value, ms.value, fl.value


if os.environ.get("CN_DETERMINISTIC") == "1":
    set_deterministic(True)

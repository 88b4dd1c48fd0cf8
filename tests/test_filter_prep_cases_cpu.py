"""What tests/test_filter_prep_gpu.py stands on, checked without a GPU (tests/filter_prep_cases.py):
  * the upsample-folded references: on every extent row the class filters, run as the scatter y[2 s + a - pad2] += wd[a] x[s] and as the
    gather over the zero-stuffed input with wf, give conv_same(upsample2(x), w); the scatter-back is the adjoint of w -> wd; k2 is
    what ops.upfold_prepare sizes its buffer with; the layer cases are ones ops.upfold_ok admits;
  * the Winograd references: with the standard B^T and A^T, A^T [(G g G^T) . (B^T d B)] A is the direct 3x3 convolution of a tile;
    the data-gradient operand is the filter of the adjoint convolution;
  * every exact case meets (sum of |terms|) 2^k < 2^24 and its expected values are representable in their storage type; the capped
    rows straddle their caps;
  * ops._weight_cache_lookup on CPU tensors (stream 0): which changes re-derive a copy, which do not, and that a stale key leaves the
    per-stream dictionary."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import filter_prep_cases as FP


# ---- the upsample-folded references ------------------------------------------------------------------------------------------------------
def _extent_rows():
    return [(nd, ks, tuple(FP.same_pad(k) for k in ks)) for nd, ks, _, _ in FP.UPFOLD_EXTENTS] + list(FP.UPFOLD_PADS)


def test_the_tables_hold_every_extent_the_issue_names():
    assert len(FP.UPFOLD_KS[2]) == 9 and len(FP.UPFOLD_KS[3]) == 27 and len(FP.UPFOLD_EXTENTS) == 36
    assert {p for _, _, pads in FP.UPFOLD_PADS for p in pads} == {0, 1, 2}
    assert [c[1] for c in FP.UPFOLD_EXTENT_CASES] == [(2, 2), (3, 4), (4, 3), (2, 4), (2, 2, 2), (2, 3, 4), (4, 4, 4), (3, 3, 4)]
    assert FP.CHANNEL_PAIRS == [(1, 1), (3, 5), (5, 3), (8, 8), (48, 20)] and FP.TAP_COUNTS == [1, 4, 9, 16, 27]
    assert sorted(t * ci * co for t, ci, co in FP.TOTALS) == [255, 256, 257]


@pytest.mark.parametrize("k,P,k2,pad2", [(2, 0, 3, 1), (3, 1, 4, 1), (4, 1, 5, 2)])
def test_one_axis_of_the_class_form(k, P, k2, pad2):
    tau, got_k2, got_pad2 = FP.upfold_axis(k, P)
    assert (got_k2, got_pad2) == (k2, pad2) and P == FP.same_pad(k)
    assert got_k2 == FP.hardcoded_k2(k)
    # every tap lands on both parities once, and a class tap has the parity of its tau
    M = FP.upfold_membership(k, P)
    assert M.sum() == 2 * k and (M.sum(0) == 2).all()
    for kk in range(k):
        assert tau[kk][0] % 2 == 0 and tau[kk][1] % 2 == 1


@pytest.mark.parametrize("nd,ks,pads", _extent_rows(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_class_filters_are_the_convolution_of_the_upsampled_input(nd, ks, pads):
    """scatter form (wd) and gather form (wf) against conv(upsample2(x), w) with low padding `pads` and the same output extent; the
    scatter-back is the adjoint of the class sums"""
    cin, cout = 3, 2
    sp = (3, 2) if nd == 2 else (2, 3, 2)
    seed = FP.flat_seed(*ks, *pads)
    x, w = FP.small_ints(sp + (cin,), seed), FP.small_ints(tuple(ks) + (cin, cout), seed + 1)
    wf, wd, k2, pad2 = FP.upfold_weights(w, pads)
    assert wd.shape == k2 + (cout, cin) and wf.shape == k2 + (cin, cout)
    want = FP.conv_same(FP.upsample2(x), w, pads)
    assert np.array_equal(FP.class_form_scatter(x, wd, pad2), want)
    assert np.array_equal(FP.class_form_gather(x, wf, pad2), want)
    # the layout of wf against wd, said once more without the slicing idiom
    for a in itertools.product(*[range(k) for k in k2]):
        rev = tuple(k2[ax] - 1 - a[ax] for ax in range(nd))
        assert np.array_equal(wf[rev], wd[a].T)
    g2 = FP.small_ints(wd.shape, seed + 2)
    gw = FP.upfold_wgrad(g2, ks, pads)
    assert gw.shape == w.shape
    assert float((wd * g2).sum()) == float((w * gw).sum())
    if all(p == FP.same_pad(k) for k, p in zip(ks, pads)):
        assert list(k2) == [FP.hardcoded_k2(k) for k in ks]


def test_the_layer_cases_are_admitted_and_sized_as_upfold_prepare_sizes_them():
    from confignet_amd import ops
    for xs, k, cout in FP.UPFOLD_EXTENT_CASES:
        g = ops.ConvSpec(k, up=1).geom(xs, cout)
        # (4,4,4) and (3,3,4): 125 and 80 class taps, past the 64 the tap mask of the implicit-GEMM gathers holds -- these two stay
        # on the unfolded path (tests/test_filter_prep_gpu.py runs them there); every other extent is admitted
        class_taps = int(np.prod([e + 1 if e >= 3 else 3 for e in k]))
        assert ops.upfold_class_taps(g) == class_taps
        assert ops.upfold_ok(g) == (class_taps <= 64), (xs, k)
        assert (class_taps > 64) == (k in ((4, 4, 4), (3, 3, 4)))
        assert all(e % 2 for e in xs[-3:-1]) and xs[-1] == 8 and cout == 8
        pads = (g.p_d, g.p_h, g.p_w)[3 - g.nd:]
        assert pads == tuple(FP.same_pad(e) for e in k)                 # ConvSpec's SAME rule on the doubled extent is (k - 1) // 2
        _, _, k2, _ = FP.upfold_weights(np.zeros(tuple(k) + (1, 1)), pads)
        assert list(k2) == [e + 1 if e >= 3 else 3 for e in k]          # the expression in ops.upfold_prepare


def test_upfold_ok_admits_every_extent_whose_class_filters_fit_the_tap_mask():
    from confignet_amd import ops
    refused = set()
    for nd, xs in ((2, (1, 3, 5, 8)), (3, (1, 2, 3, 3, 8))):
        for ks in FP.UPFOLD_KS[nd]:
            g = ops.ConvSpec(ks, up=1).geom(xs, 8)
            taps = int(np.prod([FP.upfold_axis(k, FP.same_pad(k))[1] for k in ks]))
            assert ops.upfold_class_taps(g) == taps
            assert ops.upfold_ok(g) == (taps <= ops.UPFOLD_MAX_CLASS_TAPS == 64), ks
            if not ops.upfold_ok(g):
                refused.add(tuple(sorted(ks)))
    assert refused == {(2, 4, 4), (3, 3, 4), (3, 4, 4), (4, 4, 4)}
    # an extent outside 2..4, a stride, thin channels: as before
    assert not ops.upfold_ok(ops.ConvSpec((5, 5), up=1).geom((1, 3, 5, 8), 8))
    assert not ops.upfold_ok(ops.ConvSpec((3, 3), up=1).geom((1, 3, 5, 4), 8))
    assert not ops.upfold_ok(ops.ConvSpec((3, 3), up=0).geom((1, 3, 5, 8), 8))


# ---- the Winograd references ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4])
def test_the_transform_matrices_give_the_direct_convolution_of_a_tile(m):
    G, BT, AT = FP.WINO[m]
    assert G.shape == (m + 2, 3) and BT.shape == (m + 2, m + 2) and AT.shape == (m, m + 2)
    rng = np.random.RandomState(m)
    # exactly, in rationals (the sixths of F(4x4) are no binary fractions): G as the nearest fractions with denominator 24
    Gq = np.array([[Fraction(int(round(v * 24)), 24) for v in row] for row in G], dtype=object)
    assert np.array_equal(Gq.astype(np.float64), G)
    gq, dq = rng.randint(-3, 4, (3, 3)).astype(object), rng.randint(-3, 4, (m + 2, m + 2)).astype(object)
    ATq, BTq = AT.astype(int).astype(object), BT.astype(int).astype(object)
    yq = ATq @ ((Gq @ gq @ Gq.T) * (BTq @ dq @ BTq.T)) @ ATq.T
    assert np.array_equal(yq.astype(np.float64), FP.direct_tile(gq.astype(np.float64), dq.astype(np.float64), m))
    assert all(v.denominator == 1 for v in yq.reshape(-1))
    g, d = rng.randn(3, 3), rng.randn(m + 2, m + 2)
    assert np.abs(FP.wino_tile(g, d, m) - FP.direct_tile(g, d, m)).max() < 1e-12
    # one perturbed entry of G is seen
    keep = G.copy()
    G[1, 1] *= 1.0 + 1e-6
    try:
        assert np.abs(FP.wino_tile(g, d, m) - FP.direct_tile(g, d, m)).max() > 1e-9
    finally:
        G[:] = keep
    assert np.array_equal(FP.G4[3], [1 / 24, 1 / 12, 1 / 6]) and np.array_equal(FP.G2[2], [0.5, -0.5, 0.5])


@pytest.mark.parametrize("m", [2, 4])
def test_the_transformed_filter_in_both_layouts(m):
    """forward: U[plane][ci][co] of w[., ., ci, co]; data gradient: of the adjoint convolution's filter -- the one whose direct
    convolution of gy gives d <y, gy> / dx -- as U[plane][co][ci]"""
    cin, cout = 3, 2
    rng = np.random.RandomState(10 + m)
    w = rng.randint(-3, 4, (3, 3, cin, cout)) * 576.0
    G = FP.WINO[m][0]
    u = FP.wino_filter(w, m, False)
    ud = FP.wino_filter(w, m, True)
    assert u.shape == ((m + 2) ** 2, cin, cout) and ud.shape == ((m + 2) ** 2, cout, cin)
    for ci in range(cin):
        for co in range(cout):
            assert np.allclose(u[:, ci, co].reshape(m + 2, m + 2), G @ w[:, :, ci, co] @ G.T, rtol=1e-13, atol=1e-9)
            assert np.allclose(ud[:, co, ci].reshape(m + 2, m + 2), G @ w[::-1, ::-1, ci, co] @ G.T, rtol=1e-13, atol=1e-9)
    # the adjoint through torch: y = conv_same(x, w); gx of <y, gy> is the SAME cross-correlation of gy with the flipped, swapped filter
    import torch.nn.functional as F
    x = torch.zeros(1, cin, 5, 6, dtype=torch.float64, requires_grad=True)
    wt = torch.from_numpy(w).permute(3, 2, 0, 1)                        # (co, ci, a, b)
    gy = torch.from_numpy(rng.randint(-3, 4, (1, cout, 5, 6)).astype(np.float64))
    (F.conv2d(x, wt, padding=1) * gy).sum().backward()
    adj = torch.from_numpy(FP.wino_operand(w, True).copy()).permute(3, 2, 0, 1)      # g[a][b][k = co][n = ci] -> (n, k, a, b)
    assert torch.equal(F.conv2d(gy, adj, padding=1), x.grad)
    assert np.all(FP.wino_bound(w, m, False) >= 0) and FP.WINO_ROUNDINGS == {2: 4, 4: 8}


def test_one_hot_filters_select_two_columns_of_G():
    for m in (2, 4):
        G = FP.WINO[m][0]
        for a, b in itertools.product(range(3), repeat=2):
            w = np.zeros((3, 3, 2, 3))
            w[a, b, 1, 2] = 1.0
            u = FP.wino_filter(w, m, False)
            assert np.array_equal(u[:, 1, 2].reshape(m + 2, m + 2), np.outer(G[:, a], G[:, b]))
            assert np.count_nonzero(u) == np.count_nonzero(u[:, 1, 2])
            ud = FP.wino_filter(w, m, True)
            assert np.array_equal(ud[:, 2, 1].reshape(m + 2, m + 2), np.outer(G[:, 2 - a], G[:, 2 - b]))


# ---- exactness and representability ---------------------------------------------------------------------------------------------------
def _f32_holds(a):
    return np.array_equal(np.asarray(a, np.float32).astype(np.float64), a)


def test_the_permutation_inputs_are_distinct_and_the_capped_rows_straddle_their_caps():
    for t, ci, co in FP.FLAT_CASES:
        w = FP.index_coded((t, ci, co))
        assert _f32_holds(w) and w.max() < 2 ** 24 and len(np.unique(w)) == w.size
        assert np.array_equal(FP.tflip(FP.tflip(w).reshape(t, co, ci)), w)            # (an involution)
    (a, b) = FP.CAP_4096_CASES
    assert np.prod(a) == FP.CAP_4096 and FP.CAP_4096 < np.prod(b) <= FP.CAP_4096 + 4 * FP.BLOCK
    ci, co = FP.WINO_CAP_PAIR
    assert ci * co > 1048576 == FP.CAP_4096 and (ci * co) % FP.BLOCK and ci != co
    for (lo, hi), taps in ((FP.UPFOLD_WGRAD_CAP, 4), (FP.UPFOLD_WEIGHTS_CAP, 9)):
        assert taps * lo[2] ** 2 <= FP.CAP_8192 < taps * hi[2] ** 2 and (taps * hi[2] ** 2) % FP.BLOCK
        assert lo[:2] == hi[:2] == (2, (2, 2))


def test_tflip_and_the_bf16_copies_by_element():
    t, ci, co = 4, 3, 5
    w = FP.index_coded((t, ci, co))
    wt = FP.tflip(w)
    u = FP.table_patterns(t, ci, co)
    wf, wd = FP.prep_bf16(u)
    for tt, i, o in itertools.product(range(t), range(ci), range(co)):
        assert wt[tt, o, i] == w[t - 1 - tt, i, o]
        assert wd[tt, i, o] == FP.bf16_bits(u[tt, i, o]) and wf[tt, o, i] == wd[tt, i, o]
    # the integer rounding is torch's on the patterns the table walks (NaN aside: torch's quiet bit is its own)
    big = FP.table_patterns(1, 1024, 1024)
    assert len(np.unique(big)) == 327680                                       # the whole cast table
    nan = (big & 0x7FFFFFFF) > 0x7F800000
    ours = FP.bf16_bits(big).reshape(big.shape)
    theirs = torch.from_numpy(big.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ours[~nan], theirs[~nan]) and nan.any()
    assert (((ours[nan] & 0x7FFF) > 0x7F80)).all()


def test_the_exact_cases_meet_the_margin_and_fit_their_storage():
    # F(2x2) on multiples of 4: two halvings of sums of three stay whole and small
    for ci, co in FP.WINO_PAIRS:
        w = FP.small_ints((3, 3, ci, co), FP.flat_seed(ci, co), step=4.0)
        for dgrad in (False, True):
            u = FP.wino_filter(w, 2, dgrad)
            assert np.array_equal(u, np.round(u)) and _f32_holds(u)
            assert FP.exact_margin([FP.wino_filter(w, 2, dgrad, absolute=True)]) < 2 ** 24
    # the class filters and their scatter-back: sums of at most 8 integers of [-3, 3]
    for nd, ks, ci, co in FP.UPFOLD_EXTENTS + FP.UPFOLD_CHANNELS:
        pads = tuple(FP.same_pad(k) for k in ks)
        w = FP.small_ints(tuple(ks) + (ci, co), FP.flat_seed(*ks, ci, co))
        wf, wd, k2, _ = FP.upfold_weights(w, pads)
        wa = FP.upfold_weights(np.abs(w), pads)[1]
        assert FP.exact_margin([wa]) < 2 ** 24 and _f32_holds(wd) and _f32_holds(wf)
        g2 = FP.small_ints(wd.shape, FP.flat_seed(*ks, ci, co) + 1)
        gw = FP.upfold_wgrad(g2, ks, pads)
        prior = FP.small_ints(gw.shape, 5, lim=5)
        assert FP.exact_margin([FP.upfold_wgrad(np.abs(g2), ks, pads), np.abs(prior)]) < 2 ** 24 and _f32_holds(gw + prior)
    # sumpool2: whole partial sums; the bf16 result is the one rounding of a value fp32 holds
    for row in FP.SUMPOOL:
        for dt in (FP.F32, FP.BF16):
            gu = FP.sumpool_input(row, dt)
            total = FP.sumpool2(np.abs(gu), FP.F32)
            assert FP.exact_margin([total]) < 2 ** 24
            want = FP.sumpool2(gu, dt)
            assert want.shape == (row[1],) + ((row[2],) if row[0] == 3 else ()) + (row[3], row[4], row[5])
            if dt == FP.BF16:
                assert np.array_equal(FP.bf16_round(gu), gu) and np.array_equal(FP.bf16_round(want), want)
            else:
                assert _f32_holds(want)
    assert any(not np.array_equal(FP.sumpool2(FP.sumpool_input(r, FP.BF16), FP.F32), FP.sumpool2(FP.sumpool_input(r, FP.BF16), FP.BF16))
               for r in FP.SUMPOOL)                                            # (the bf16 store does round somewhere)
    assert any(np.prod(r[1:5]) * (r[5] // 4) % FP.BLOCK for r in FP.SUMPOOL) and any(r[1:5] == (1, 1, 1, 1) for r in FP.SUMPOOL)
    assert all(r[5] % 4 == 0 for r in FP.SUMPOOL)


def test_sumpool2_is_the_adjoint_of_the_upsample():
    for nd, sp in ((2, (3, 5)), (3, (2, 3, 5))):
        x = FP.small_ints((2,) + sp + (4,), nd)
        xu = np.stack([FP.upsample2(x[i]) for i in range(2)])
        gu = FP.small_ints(xu.shape, nd + 1)
        assert float((xu * gu).sum()) == float((x * FP.sumpool2(gu, FP.F32)).sum())


# ---- the cache of derived copies, on CPU tensors ---------------------------------------------------------------------------------------
class _Owner:
    """what _weight_cache_lookup reads of a network"""

    def __init__(self, n_trainable):
        self.epoch, self.n_trainable = 0, n_trainable


class _Counting:
    def __init__(self):
        self.calls = 0

    def __call__(self, w):
        self.calls += 1
        return w.clone()


def _entry_keys(w, slot):
    c = getattr(w, slot)
    assert isinstance(c, dict)
    return [e[0] for e in c.values()]


def test_a_free_tensor_is_rederived_when_its_version_moves():
    from confignet_amd import ops
    w, make = torch.arange(6.0).reshape(1, 2, 3), _Counting()
    a = ops._weight_cache_lookup(w, "_cn_t", make)
    assert ops._weight_cache_lookup(w, "_cn_t", make) is a and make.calls == 1
    assert torch.equal(a, w)
    old = _entry_keys(w, "_cn_t")
    w.add_(1)
    b = ops._weight_cache_lookup(w, "_cn_t", make)
    assert make.calls == 2 and b is not a and torch.equal(b, w) and not torch.equal(a, w)
    assert ops._weight_cache_lookup(w, "_cn_t", make) is b and make.calls == 2
    keys = _entry_keys(w, "_cn_t")
    assert len(keys) == 1 and keys[0] not in old                          # the stale key left the per-stream dictionary
    assert keys[0][4] == 0                                                # a CPU tensor: stream 0
    # another slot of the same tensor is another entry
    other = _Counting()
    c = ops._weight_cache_lookup(w, "_cn_u", other)
    assert other.calls == 1 and c is not b and make.calls == 2
    assert ops._weight_cache_lookup(w, "_cn_t", make) is b and ops._weight_cache_lookup(w, "_cn_u", other) is c
    assert (make.calls, other.calls) == (2, 1)


def test_a_networks_filter_follows_its_own_epoch_and_the_global_one():
    from confignet_amd import ops
    from confignet_amd.nn import WEIGHTS_EPOCH
    mine, theirs = _Owner(6), _Owner(6)
    w, v = torch.arange(6.0).reshape(1, 2, 3), torch.ones(1, 2, 3)
    w._cn_owner, v._cn_owner = mine, theirs
    mw, mv = _Counting(), _Counting()
    a, av = ops._weight_cache_lookup(w, "_cn_t", mw), ops._weight_cache_lookup(v, "_cn_t", mv)
    assert ops._weight_cache_lookup(w, "_cn_t", mw) is a and (mw.calls, mv.calls) == (1, 1)
    # a raw-pointer update: the values move, torch's version does not; mark_updated() is what tells the cache
    version = w._version
    mine.epoch += 1
    assert w._version == version
    old = _entry_keys(w, "_cn_t")
    b = ops._weight_cache_lookup(w, "_cn_t", mw)
    assert mw.calls == 2 and b is not a
    assert old[0] not in _entry_keys(w, "_cn_t") and len(_entry_keys(w, "_cn_t")) == 1
    # ... and the other network's copies stay
    assert ops._weight_cache_lookup(v, "_cn_t", mv) is av and mv.calls == 1
    theirs.epoch += 1
    assert ops._weight_cache_lookup(w, "_cn_t", mw) is b and mw.calls == 2
    assert ops._weight_cache_lookup(v, "_cn_t", mv) is not av and mv.calls == 2
    # the global generation (a graph capture starts or ends) re-derives everything trainable
    before = WEIGHTS_EPOCH[0]
    try:
        WEIGHTS_EPOCH[0] += 1
        old = _entry_keys(w, "_cn_t")
        c = ops._weight_cache_lookup(w, "_cn_t", mw)
        assert mw.calls == 3 and c is not b and ops._weight_cache_lookup(w, "_cn_t", mw) is c
        assert old[0] not in _entry_keys(w, "_cn_t") and len(_entry_keys(w, "_cn_t")) == 1
    finally:
        WEIGHTS_EPOCH[0] = before
    # an in-place change through torch re-derives a network's filter as well
    with torch.no_grad():
        w.mul_(2)
    d = ops._weight_cache_lookup(w, "_cn_t", mw)
    assert mw.calls == 4 and torch.equal(d, w)


def test_a_frozen_networks_filter_is_derived_once_per_epoch_of_its_own():
    from confignet_amd import ops
    from confignet_amd.nn import WEIGHTS_EPOCH
    frozen = _Owner(0)
    w = torch.arange(6.0).reshape(1, 2, 3)
    w._cn_owner = frozen
    make = _Counting()
    a = ops._weight_cache_lookup(w, "_cn_t", make)
    assert ops._weight_cache_lookup(w, "_cn_t", make) is a and make.calls == 1
    before = WEIGHTS_EPOCH[0]
    try:
        WEIGHTS_EPOCH[0] += 1
        assert ops._weight_cache_lookup(w, "_cn_t", make) is a
    finally:
        WEIGHTS_EPOCH[0] = before
    w.add_(1)                                                             # (a frozen filter only changes with set_weights, which bumps the epoch)
    assert ops._weight_cache_lookup(w, "_cn_t", make) is a and make.calls == 1
    frozen.epoch += 1
    b = ops._weight_cache_lookup(w, "_cn_t", make)
    assert make.calls == 2 and b is not a and torch.equal(b, w)
    assert ops._weight_cache_lookup(w, "_cn_t", make) is b and make.calls == 2
    other = _Counting()
    assert ops._weight_cache_lookup(w, "_cn_u", other) is not b and other.calls == 1

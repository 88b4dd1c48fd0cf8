"""Which launch a dense product gets, checked without a GPU through cn_gemm_plan (csrc/gemm.hip: plan_gemm is the function cn_gemm
and cn_gemm_acc decide with).  tests/golden/gemm_plans.json holds RECORDED plans: what the routing chain written out in gemm_launch
before plan_gemm existed gives for each request, as tests/gemm_edge_cases.py transcribes it -- never generated from the function
it pins.  The requests are the two sides of every routing boundary (rows / depth / thin / tile, the K slices of the thin kernel, the
split-K of the tile kernel and its deterministic form), the split-K requests of tests/test_gemm_edges_gpu.py and the model's own
dense shapes."""
import ctypes
import json

import pytest

from confignet_amd._lib import lib
from tests import gemm_edge_cases as G

CN_EINVAL = -1


def plan(*req):
    out = (ctypes.c_int * 9)()
    assert lib.cn_gemm_plan(*req, ctypes.byref(out)) == 0, req
    return list(out)


@pytest.fixture(scope="module")
def doc():
    return json.load(open(G.GOLDEN))


def test_the_recorded_plans_are_what_the_library_plans(doc):
    assert doc["fields"] == G.REQUEST + G.PLAN
    assert len(doc["plans"]) >= 100
    for row in doc["plans"]:
        assert plan(*row[:10]) == row[10:], row[:10]


def test_the_recorded_plans_are_what_the_transcription_gives(doc):
    for row in doc["plans"]:
        assert G.transcribed_plan(*row[:10]) == row[10:], row[:10]
    assert [tuple(r[:10]) for r in doc["plans"]] == G.golden_requests()


def test_the_boundary_table_written_by_hand(doc):
    rec = {tuple(r[:10]): r[10:] for r in doc["plans"]}
    assert [tuple(r) for r in doc["boundaries"]] == [r for r, _ in G.BOUNDARIES]
    for req, (route, mt, grid, slices, kps, last, zero, parts, lds) in G.BOUNDARIES:
        p = rec[req]
        assert p == [route, mt, *grid, kps, zero, parts, lds], req
        assert G.slices_of(p, req[4]) == (slices, kps, last) and 0 < last <= kps, req
        assert plan(*req) == p, req


def test_every_route_every_row_count_and_both_sides_of_every_boundary_are_recorded(doc):
    rec = {tuple(r[:10]): r[10:] for r in doc["plans"]}
    assert {p[0] for p in rec.values()} == {G.ROWS, G.DEPTH, G.THIN, G.TILE}
    assert {p[1] for p in rec.values() if p[0] == G.ROWS} == {8, 16, 32} and {r[1] for r, p in rec.items() if p[0] == G.ROWS} == {0, 1}
    assert {p[1] for p in rec.values() if p[0] != G.ROWS} == {0}
    assert len(G.BOUNDARY_PAIRS) >= 11
    for a, b in G.BOUNDARY_PAIRS:
        pa, pb = rec[G.request(*a)], rec[G.request(*b)]
        assert pa != pb and (pa[0] != pb[0] or pa[2:5] != pb[2:5] or pa[5] != pb[5]), (a, b)
    # the thin kernel with 1, 2 and 3 slices; the tile kernel with one slice, atomics behind a zero pass, atomics onto a prior
    # value, and the ordered slabs of deterministic mode
    assert {p[3] for p in rec.values() if p[0] == G.THIN} >= {1, 2, 3}
    tile = [(r, p) for r, p in rec.items() if p[0] == G.TILE]
    assert any(p[4] == 1 for _, p in tile) and any(p[4] > 1 and p[6] for _, p in tile)
    assert any(p[4] > 1 and r[8] and not p[6] and not p[7] for r, p in tile)
    assert any(p[4] > 1 and p[7] == p[4] * r[2] * r[3] and not p[6] for r, p in tile)
    # the model's dense shapes and the split-K requests of the GPU file, deterministic off and on
    assert [tuple(s) for s in doc["workload"]] == G.WORKLOAD and len(G.WORKLOAD) == 9
    for s in G.WORKLOAD:
        for det in (0, 1):
            assert G.request(*s, has_bias=1, det=det) in rec and G.request(*s, accumulate=1, det=det) in rec, s
    assert [tuple(s) for s in doc["splitk"]] == list(G.SPLITK)
    for s, slices in G.SPLITK.items():
        for det in (0, 1):
            assert rec[G.request(*s, det=det)][4] == rec[G.request(*s, has_bias=1, det=det)][4] == slices, s
            assert rec[G.request(*s, det=det, ldc=s[3] + 5)][4] == (1 if det else slices), s
            assert rec[G.request(*s, accumulate=1, det=det)][4] == (1 if det else slices), s


def test_the_invariants_of_every_plan():
    """around every recorded shape: the slices cover K with a last one that is not empty, the zero pass comes exactly where atomics
    add into a C the call must write, the slabs exactly in deterministic mode"""
    shapes = sorted({(r[0][0], r[0][1], r[0][2] + dm, r[0][3] + dn, r[0][4] + dk) for r in G.BOUNDARIES for dm in (-1, 0, 1) for dn in (-1, 0, 1)
                     for dk in (-1, 0, 1) if r[0][2] + dm > 0 and r[0][3] + dn > 0 and r[0][4] + dk > 0})
    assert len(shapes) > 400
    for ta, tb, m, n, k in shapes:
        for has_bias, act, acc in ((0, 0, 0), (1, 0, 0), (1, G.LRELU, 0), (0, 0, 1)):
            for det in (0, 1):
                for ldc in (n, n + 5):
                    req = (ta, tb, m, n, k, ldc, has_bias, act, acc, det)
                    p = plan(*req)
                    assert p == G.transcribed_plan(*req), req
                    route, mt, gx, gy, gz, kps, zero, parts, lds = p
                    s, _, last = G.slices_of(p, k)
                    assert 0 < last <= kps and (s - 1) * kps < k <= s * kps, req
                    assert zero == int(s > 1 and not acc and not parts), req
                    assert parts == (s * m * n if det and s > 1 else 0) and parts <= G.DET_WS_FLOATS, req
                    assert not (s > 1 and act) and not (det and route == G.THIN and s > 1), req
                    if route == G.ROWS:
                        assert m <= mt and mt * k <= 8192 and lds == 4 * (mt * k + 3 * mt * 64) <= 65536 and (gx, gy, gz) == (G.cdiv(n, 64), 1, 1), req
                    else:
                        assert lds == 0 and mt == 0, req
                    if route == G.DEPTH:
                        assert k <= 32 and (gx, gy, gz) == (G.cdiv(m, 16), G.cdiv(n, 64), 1), req
                    if route == G.THIN:
                        assert n <= 4 and gx == m <= 256 and gz == 1, req
                    if route == G.TILE:
                        assert (gx, gy) == (G.cdiv(m, 64), G.cdiv(n, 64)) and kps % G.BK == 0, req


def test_the_deterministic_workspace_cap_never_binds():
    """Splitting needs tiles < 128, so m n <= 4096 tiles and the cap is at least 4096 / tiles slabs, while at most ceil(256 / tiles)
    slices are asked for: over a sweep of (m, n) with fewer than 128 tiles -- the corners of every tile count, the largest products
    and long K -- the split is the one of the rule without the cap, and the largest split / cap stays far below 1."""
    worst = 0.0
    count = 0
    sizes = sorted({v for t in range(1, 129) for v in (64 * t - 63, 64 * t - 1, 64 * t) if v > 0})
    for m in sizes:
        for n in sizes:
            if G.cdiv(m, 64) * G.cdiv(n, 64) >= 128:
                continue
            for k in (1024, 4609, 65536, 1 << 20):
                free = G.tile_split(m, n, k, det=1, capped=False)
                assert G.tile_split(m, n, k, det=1) == free, (m, n, k)
                worst = max(worst, free[0] / G.det_cap(m, n))
                count += 1
    assert count > 5000 and worst < 0.1, (count, worst)
    for m, n, k in ((8128, 64, 1 << 20), (64, 8128, 65536), (704, 704, 1 << 20), (257, 5, 1 << 20), (8128, 5, 1 << 16)):
        p = plan(0, 0, m, n, k, n, 0, 0, 0, 1)
        assert p[0] == G.TILE and (p[4], p[5]) == G.tile_split(m, n, k, det=1, capped=False) and p[7] == p[4] * m * n, (m, n, k)


def test_bad_plan_requests_are_argument_errors():
    out = (ctypes.c_int * 9)()
    for m, n, k, ldc in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 4, 1, 3)):
        assert lib.cn_gemm_plan(0, 0, m, n, k, ldc, 0, 0, 0, 0, ctypes.byref(out)) == CN_EINVAL, (m, n, k, ldc)
    assert lib.cn_gemm_plan(0, 0, 1, 1, 1, 1, 0, 0, 0, 0, None) == CN_EINVAL

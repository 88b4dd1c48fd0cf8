"""The dense GEMM family's launch rule written out once more in Python, and the edge requests of tests/test_gemm_plan_cpu.py and
tests/test_gemm_edges_gpu.py.

transcribed_plan() is a TRANSCRIPTION of the routing chain gemm_launch (csrc/gemm.hip) carried before plan_gemm existed, condition by
condition in its order: tests/golden/gemm_plans.json was written from it (python -m tests.gemm_edge_cases), never from cn_gemm_plan,
and tests/test_gemm_plan_cpu.py holds the library, the recorded plans and this transcription to each other.  BOUNDARIES is written
by hand: what each request next to a routing boundary must get."""
import json
import os

ROWS, DEPTH, THIN, TILE = 0, 1, 2, 3                     # the route codes of cn_gemm_plan
NONE, LRELU, RELU, TANH, RELU6 = 0, 1, 2, 3, 4           # CN_ACT_*
BK = 16                                                  # csrc/mma_tile.h: K depth of one LDS stage of the tile kernel
DET_WS_FLOATS = 16 << 20                                 # csrc/common.h: CN_DET_WS_FLOATS
REQUEST = ["ta", "tb", "m", "n", "k", "ldc", "has_bias", "act", "accumulate", "det"]
PLAN = ["route", "mt", "gx", "gy", "gz", "kps", "zero_first", "parts_floats", "lds_bytes"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.json")


def cdiv(a, b):
    return (a + b - 1) // b


def det_cap(m, n):
    """the most slabs of m x n floats the deterministic workspace of one stream holds"""
    return DET_WS_FLOATS // (m * n)


def tile_split(m, n, k, act=NONE, accumulate=0, ldc=None, det=0, capped=True):
    """(K slices, K per slice) of the tile route"""
    tiles = cdiv(m, 64) * cdiv(n, 64)
    splitk = 1
    if act == NONE and tiles < 128 and k >= 1024 and not (det and (accumulate or (ldc or n) != n)):
        splitk = cdiv(256, tiles)
        if splitk > k // 256:
            splitk = k // 256
        if splitk < 1:
            splitk = 1
    kps = cdiv(cdiv(k, splitk), BK) * BK
    splitk = cdiv(k, kps)
    if det and splitk > 1 and capped:
        cap = det_cap(m, n)
        if splitk > cap:
            splitk = max(cap, 1)
        kps = cdiv(cdiv(k, splitk), BK) * BK
        splitk = cdiv(k, kps)
    return splitk, kps


def transcribed_plan(ta, tb, m, n, k, ldc=None, has_bias=0, act=NONE, accumulate=0, det=0):
    """[route, MT, grid x, y, z, K per slice, zero pass first, deterministic partial floats, dynamic LDS bytes]"""
    ldc = n if ldc is None else ldc
    mt = 8 if m <= 8 else 16 if m <= 16 else 32
    if not accumulate and not ta and m <= 32 and n > 4 and mt * k <= 8192:
        return [ROWS, mt, cdiv(n, 64), 1, 1, k, 0, 0, 4 * (mt * k + 3 * mt * 64)]
    if ta and not tb and k <= 32 and not has_bias and act == NONE:
        return [DEPTH, 0, cdiv(m, 16), cdiv(n, 64), 1, k, 0, 0, 0]
    if not accumulate and not ta and not tb and n <= 4 and m <= 256 and k >= 128:
        slices = 1
        if act == NONE and k >= 8192 and not det:
            slices = k // 4096
        kps = cdiv(k, slices)
        slices = cdiv(k, kps)
        return [THIN, 0, m, slices, 1, kps, int(slices > 1), 0, 0]
    splitk, kps = tile_split(m, n, k, act, accumulate, ldc, det)
    parts = splitk * m * n if det and splitk > 1 else 0
    return [TILE, 0, cdiv(m, 64), cdiv(n, 64), splitk, kps, int(splitk > 1 and not accumulate and not parts), parts, 0]


def slices_of(plan, k):
    """(slices, K per slice, K of the last slice)"""
    s = plan[3] if plan[0] == THIN else plan[4]
    return s, plan[5], k - (s - 1) * plan[5]


def request(ta, tb, m, n, k, ldc=None, has_bias=0, act=NONE, accumulate=0, det=0):
    return (ta, tb, m, n, k, n if ldc is None else ldc, has_bias, act, accumulate, det)


def _b(ta, tb, m, n, k, want, **kw):
    return request(ta, tb, m, n, k, **kw), want


# request -> (route, MT, (grid x, y, z), slices, K per slice, K of the last slice, zero pass, partial floats, LDS bytes), by hand
BOUNDARIES = [
    # rows: mt * k <= 8192, and what lies one past it
    _b(0, 0, 8, 5, 1024, (ROWS, 8, (1, 1, 1), 1, 1024, 1024, 0, 0, 38912)),
    _b(0, 0, 8, 5, 1025, (TILE, 0, (1, 1, 4), 4, 272, 209, 1, 0, 0)),
    _b(0, 0, 16, 65, 512, (ROWS, 16, (2, 1, 1), 1, 512, 512, 0, 0, 45056)),
    _b(0, 0, 16, 65, 513, (TILE, 0, (1, 2, 1), 1, 528, 513, 0, 0, 0)),
    _b(0, 1, 32, 70, 256, (ROWS, 32, (2, 1, 1), 1, 256, 256, 0, 0, 57344)),
    _b(0, 1, 32, 70, 257, (TILE, 0, (1, 2, 1), 1, 272, 257, 0, 0, 0)),
    _b(0, 0, 9, 64, 3, (ROWS, 16, (1, 1, 1), 1, 3, 3, 0, 0, 12480)),              # K quarters of 1, 1, 1, 0
    _b(0, 0, 1, 5, 1, (ROWS, 8, (1, 1, 1), 1, 1, 1, 0, 0, 6176)),                 # three empty K quarters
    # depth: ta, !tb, k <= 32, no bias, no activation
    _b(1, 0, 17, 65, 32, (DEPTH, 0, (2, 2, 1), 1, 32, 32, 0, 0, 0)),
    _b(1, 0, 17, 65, 33, (TILE, 0, (1, 2, 1), 1, 48, 33, 0, 0, 0)),
    _b(1, 0, 17, 65, 32, (TILE, 0, (1, 2, 1), 1, 32, 32, 0, 0, 0), has_bias=1),
    _b(1, 0, 20, 70, 32, (DEPTH, 0, (2, 2, 1), 1, 32, 32, 0, 0, 0), accumulate=1),
    # thin: n <= 4, m <= 256, k >= 128
    _b(0, 0, 3, 4, 128, (THIN, 0, (3, 1, 1), 1, 128, 128, 0, 0, 0)),
    _b(0, 0, 3, 4, 127, (TILE, 0, (1, 1, 1), 1, 128, 127, 0, 0, 0)),
    _b(0, 0, 256, 1, 129, (THIN, 0, (256, 1, 1), 1, 129, 129, 0, 0, 0)),
    _b(0, 0, 257, 1, 129, (TILE, 0, (5, 1, 1), 1, 144, 129, 0, 0, 0)),
    _b(0, 0, 2, 3, 8191, (THIN, 0, (2, 1, 1), 1, 8191, 8191, 0, 0, 0)),
    _b(0, 0, 2, 3, 8192, (THIN, 0, (2, 2, 1), 2, 4096, 4096, 1, 0, 0)),
    _b(0, 0, 2, 3, 8193, (THIN, 0, (2, 2, 1), 2, 4097, 4096, 1, 0, 0)),
    _b(0, 0, 2, 2, 12287, (THIN, 0, (2, 2, 1), 2, 6144, 6143, 1, 0, 0)),
    _b(0, 0, 2, 2, 12289, (THIN, 0, (2, 3, 1), 3, 4097, 4095, 1, 0, 0)),
    _b(0, 0, 2, 3, 8192, (THIN, 0, (2, 1, 1), 1, 8192, 8192, 0, 0, 0), act=LRELU),
    _b(0, 0, 2, 3, 8192, (THIN, 0, (2, 1, 1), 1, 8192, 8192, 0, 0, 0), det=1),
    # tile: split-K from k = 1024, without activation
    _b(0, 0, 33, 5, 1023, (TILE, 0, (1, 1, 1), 1, 1024, 1023, 0, 0, 0)),
    _b(0, 0, 33, 5, 1024, (TILE, 0, (1, 1, 4), 4, 256, 256, 1, 0, 0)),
    _b(0, 0, 33, 5, 1025, (TILE, 0, (1, 1, 4), 4, 272, 209, 1, 0, 0)),
    _b(0, 0, 33, 5, 4609, (TILE, 0, (1, 1, 17), 17, 272, 257, 1, 0, 0)),          # 18 slices asked for, 17 after rounding to BK
    _b(0, 0, 33, 5, 1025, (TILE, 0, (1, 1, 1), 1, 1040, 1025, 0, 0, 0), act=LRELU),
    _b(0, 0, 33, 5, 1025, (TILE, 0, (1, 1, 4), 4, 272, 209, 0, 660, 0), det=1),
    _b(0, 0, 33, 5, 1025, (TILE, 0, (1, 1, 1), 1, 1040, 1025, 0, 0, 0), det=1, ldc=9),
    _b(0, 0, 33, 5, 1025, (TILE, 0, (1, 1, 1), 1, 1040, 1025, 0, 0, 0), det=1, accumulate=1),
    _b(0, 0, 8, 70, 1100, (TILE, 0, (1, 2, 4), 4, 288, 236, 0, 0, 0), accumulate=1),
    _b(1, 1, 65, 65, 1300, (TILE, 0, (2, 2, 5), 5, 272, 212, 1, 0, 0)),
    _b(1, 0, 70, 130, 2049, (TILE, 0, (2, 3, 8), 8, 272, 145, 1, 0, 0)),
]
# the two sides of every boundary, (ta, tb, m, n, k) each: both must be among BOUNDARIES (plain requests: no bias, not deterministic)
BOUNDARY_PAIRS = [((0, 0, 8, 5, 1024), (0, 0, 8, 5, 1025)), ((0, 0, 16, 65, 512), (0, 0, 16, 65, 513)), ((0, 1, 32, 70, 256), (0, 1, 32, 70, 257)),
                  ((1, 0, 17, 65, 32), (1, 0, 17, 65, 33)), ((0, 0, 3, 4, 128), (0, 0, 3, 4, 127)), ((0, 0, 256, 1, 129), (0, 0, 257, 1, 129)),
                  ((0, 0, 2, 3, 8191), (0, 0, 2, 3, 8192)), ((0, 0, 2, 3, 8192), (0, 0, 2, 3, 8193)), ((0, 0, 2, 2, 12287), (0, 0, 2, 2, 12289)),
                  ((0, 0, 33, 5, 1023), (0, 0, 33, 5, 1024)), ((0, 0, 33, 5, 1024), (0, 0, 33, 5, 1025))]

# the workload's own dense shapes (tests/test_ops_gpu.py: test_gemm), (ta, tb, m, n, k): plans only
WORKLOAD = [(0, 0, 16, 148, 32768), (0, 0, 16, 1, 32768), (0, 0, 16, 3, 2048), (0, 0, 8, 145, 145), (0, 0, 4096, 217, 145),
            (0, 1, 16, 32768, 148), (1, 0, 32768, 148, 16), (0, 0, 16, 128, 145), (0, 0, 8, 512, 128)]

# the split-K requests tests/test_gemm_edges_gpu.py runs on the tile kernel, (ta, tb, m, n, k) -> slices
SPLITK = {(0, 0, 33, 5, 1023): 1, (0, 0, 33, 5, 1024): 4, (0, 0, 33, 5, 1025): 4, (0, 0, 33, 5, 4609): 17, (1, 1, 65, 65, 1300): 5,
          (1, 0, 70, 130, 2049): 8}


def golden_requests():
    """every request the recorded plans hold, in order, without repeats"""
    reqs = [r for r, _ in BOUNDARIES]
    for s in WORKLOAD:
        for det in (0, 1):
            reqs.append(request(*s, has_bias=1, det=det))             # the Dense layer itself
            reqs.append(request(*s, accumulate=1, det=det))           # its weight-gradient form through cn_gemm_acc
    for s in SPLITK:
        for det in (0, 1):
            for bias in (0, 1):
                reqs.append(request(*s, has_bias=bias, det=det))
                reqs.append(request(*s, has_bias=bias, det=det, ldc=s[3] + 5))
            reqs.append(request(*s, accumulate=1, det=det))
    seen, out = set(), []
    for r in reqs:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


if __name__ == "__main__":
    doc = {"about": "Launch plans of cn_gemm / cn_gemm_acc, RECORDED from the routing chain gemm_launch carried before plan_gemm existed, as "
                    "tests/gemm_edge_cases.py: transcribed_plan writes it out (the deterministic workspace cap included: it binds on no request). "
                    "boundaries: the requests next to a routing boundary; workload: the dense shapes of the model (plans only); splitk: "
                    "the split-K requests of tests/test_gemm_edges_gpu.py.",
           "fields": REQUEST + PLAN,
           "boundaries": [list(r) for r, _ in BOUNDARIES],
           "workload": [list(s) for s in WORKLOAD],
           "splitk": [list(s) for s in SPLITK],
           "plans": [list(r) + transcribed_plan(*r) for r in golden_requests()]}
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v) if k != "plans" else "[\n  " + ",\n  ".join(json.dumps(p) for p in v) + "\n ]")
                                   for k, v in doc.items()) + "\n}\n")
    print("wrote %d plans" % len(doc["plans"]))

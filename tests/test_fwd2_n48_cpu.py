"""Which body a launch of the LDS-DMA loop gets (csrc/fwd2.hip), checked without a GPU: cn_fwd2_col_block is the function cn_fwd2
itself selects with.  The 64 x 48 body on 16-wide MFMA blocks takes exactly the gathered data gradients from the original filter
into 48 channels on the 64 x 64 tile with the default loop; the plan -- tile, grid, family -- is the one the 64 x 64 body had."""
import itertools
import json

import pytest

from confignet_amd._lib import lib
from tests import test_conv_plan_cpu as P

# the batch-16 256^2 iteration's data gradients into the 48-channel tensor of the first discriminator block, and the two GPU-test
# layers of the same form (tests/golden/conv_plans.json)
PINNED = ("round6_conv_shapes.txt:3", "round6_conv_shapes.txt:11", "round6_conv_shapes.txt:27", "round6_conv_shapes.txt:65",
          "round6_conv_shapes.txt:77", "FULL_SIZE_LAYERS[1]", "CONV_CASES[8]")


@pytest.fixture(autouse=True)
def _defaults():
    lib.cn_conv_tune(-1, 0, 0)
    lib.cn_conv_loop_select(-1, 0, 0, -1)
    yield
    lib.cn_conv_tune(-1, 0, 0)
    lib.cn_conv_loop_select(-1, 0, 0, -1)


def test_the_16_wide_body_is_selected_exactly_on_its_predicate():
    n16 = 0
    for cfg, bt, gathered, n, kb, np_ in itertools.product(range(-1, 6), (0, 1), (0, 1), (32, 48, 52, 64, 96), (16, 32), (0, 1, 2)):
        want = 16 if (cfg == 2 and bt == 1 and gathered == 1 and n == 48 and kb == 16 and np_ == 0) else 32
        assert lib.cn_fwd2_col_block(cfg, bt, gathered, n, kb, np_) == want, (cfg, bt, gathered, n, kb, np_)
        n16 += want == 16
    assert n16 == 1


def test_the_pinned_48_channel_data_gradients_keep_their_plan_and_take_the_16_wide_body():
    table = json.load(open(P.GOLDEN))
    layers = {e["name"]: e for e in table["layers"]}
    for name in PINNED:
        g = P.make_geom(layers[name]["g"])
        d = P.dgrad_geom(g)
        rc, p = P.plan_request(g, "dgrad_w")
        m = d.n * d.out_d * d.out_h * d.out_w
        assert rc == 0 and [rc] + p == layers[name]["plans"]["dgrad_w"], name
        assert p[0] == P.FWD2 and p[1] == 2 and p[2] == 1 and p[3] == 1 and p[5:] == [-(-m // 64), 1, 1], (name, p)
        assert d.cout == 48 and d.k_h * d.k_w == 9
        assert lib.cn_fwd2_col_block(p[1], 1, 1, d.cout, 16, 0) == 16, name

"""Deterministic mode in bf16 storage, at the level of whole training iterations: tests/test_steps_gpu.py's
test_deterministic_mode_is_bitwise_reproducible restated under ops.set_activation_dtype("bf16").  The one reduction of the bf16 path
whose order was left to the hardware -- the fp32 atomics of the bf16 filter gradient's row slices -- goes through slabs added in
slice order in this mode (csrc/igemm_bf16.hip, csrc/conv_dispatch.hip), so two runs from the same state end in the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_steps_gpu import _small_second_stage


@pytest.mark.parametrize("graphs", [False, True])
def test_deterministic_mode_is_bitwise_reproducible_in_bf16_storage(graphs):
    """Two runs of two whole second-stage iterations (128 x 128, batch 2) from the same weights, Adam moments and numpy seed, eager
    and under graph + overlap dispatch: equal loss scalars, bit-identical network arenas and Adam moments.  The first (eager)
    iteration is profiled to show that the run really is the bf16 one: it launches the bf16 filter gradient."""
    from confignet_amd import ops
    ops.set_deterministic(True)
    ops.set_activation_dtype("bf16")
    try:
        m, real_set, synth_set, d_opt, g_opt = _small_second_stage()
        assert not m.fork_generator_step
        m.use_graphs = graphs
        m.overlap_discriminators = graphs
        nets = m.all_networks()
        torch.cuda.synchronize()
        ops.prof_enable(True)
        try:
            ops.prof_reset()
            m.training_iteration(real_set, synth_set, d_opt, g_opt)
            torch.cuda.synchronize()
            assert "igemm_bf16_wgrad" in ops.prof_collect_by_family()
        finally:
            ops.prof_enable(False)
        for _ in range(3 if graphs else 0):                   # (graphs: one more eager warm-up, capture, first pipelined replay)
            m.training_iteration(real_set, synth_set, d_opt, g_opt)
        torch.cuda.synchronize()
        start = [n.get_weights() for n in nets]

        def run():
            for n, w0 in zip(nets, start):
                n.set_weights(w0)
            for o in (d_opt, g_opt):
                o.iterations = 0
                for mom, var in o._state.values():
                    mom.zero_(); var.zero_()
            np.random.seed(123)
            losses = []
            for _ in range(2):
                out = m.training_iteration(real_set, synth_set, d_opt, g_opt)
                losses.append([{k: float(v) for k, v in d.items()} for d in out])
            torch.cuda.synchronize()
            state = [n.arena.detach().cpu().clone() for n in nets]
            state += [t.detach().cpu().clone() for o in (d_opt, g_opt) for pair in o._state.values() for t in pair]
            return losses, state

        l1, s1 = run()
        l2, s2 = run()
        assert l1 == l2, [(a, b) for x, y in zip(l1, l2) for da, db in zip(x, y) for (_, a), (_, b) in zip(da.items(), db.items()) if a != b][:5]
        for i, (a, b) in enumerate(zip(s1, s2)):
            assert torch.equal(a, b), ("tensor %d differs" % i, float((a - b).abs().max()))
    finally:
        ops.set_activation_dtype("f32")
        ops.set_deterministic(False)

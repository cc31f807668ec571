"""The oracle's texture adjoint at the sizes and layouts of dr_texture_cases.py, pinned on the CPU before the GPU is held to it
(test_dr_textures_gpu.py): forward-mode duals against central finite differences of the replay, the one-channel path against the
four-channel one, and the reference's own summation-order noise."""
import numpy as np
import pytest

import dr_texture_cases as T
from dr_texture_cases import CASES

SPP = 3


def _oracle(case, data=None):
    from oracle.orc import OracleIntegrator
    sc = T.scene_of(case)
    cpu = OracleIntegrator(sc)
    T.register_cpu(cpu, case)
    d, ref = T.inputs(case, sc)
    return cpu, (d if data is None else data), ref


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_duals_match_finite_differences(case):
    """path_trace_dr against path_trace_dr_fd (the replay differentiated by central differences, the loss summed in double), with the
    tolerances of test_cpu.test_oracle_gradient_matches_finite_differences, on: the 12 largest elements, 12 seeded random non-zero ones,
    and every element of the first and last texel column and row (48 of them, drawn with a seed, on `sparse`)."""
    cpu, data, ref = _oracle(case)
    gens = cpu.random_gens().copy()
    loss, grad, _ = T.oracle_dr(cpu, SPP, ref, data)
    n = case.size()
    assert loss > 0 and np.all(grad[n:] == 0) and np.all(grad[T.alpha_elements(case)] == 0)
    g = grad[:n]
    rng = np.random.default_rng(2)
    nz = np.flatnonzero(g)
    border = T.border_elements(case)
    if case.name == "sparse":
        border = rng.choice(border, 48, replace=False)
    idx = np.unique(np.concatenate([np.argsort(-np.abs(g))[:12], rng.choice(nz, min(12, nz.size), replace=False), border]))
    cpu.set_random_gens(gens)
    fd = cpu.path_trace_dr_fd(SPP, ref, data, idx, h=2e-2)
    worst = float(np.max(np.abs(g[idx] - fd) / (5e-3 * np.abs(fd) + 1e-4)))
    print(f"{case.name}: {idx.size} elements compared, {np.count_nonzero(g[idx])} of them non-zero ({nz.size} of {n} in the buffer); worst error / bound = {worst:.3f}")
    assert 2 * np.count_nonzero(g[idx]) >= idx.size
    assert np.allclose(g[idx], fd, rtol=5e-3, atol=1e-4)


@pytest.mark.parametrize("name", ["mono_npot", "mono_pow2"])
def test_one_channel_equals_four_channels(name):
    """(W, H, 1) with data d against (W, H, 4) with data (d, d, d, 1): the same frame bit for bit, and the one-channel gradient is the sum of
    the rgb gradients (same sums, another order: rtol 1e-5, atol 1e-7 max|grad|)."""
    case = T.BY_NAME[name]
    cpu1, data, ref = _oracle(case)
    _, grad1, frame1 = T.oracle_dr(cpu1, SPP, ref, data)
    four, data4 = T.as_four_channels(case, data)
    cpu4, _, _ = _oracle(four, data4)
    _, grad4, frame4 = T.oracle_dr(cpu4, SPP, ref, data4)
    assert np.array_equal(frame1.view(np.uint32), frame4.view(np.uint32))
    assert np.array_equal(cpu1.random_gens(), cpu4.random_gens())
    g1, g4 = grad1[:case.size()], grad4[:four.size()].reshape(-1, 4)
    assert np.count_nonzero(g1) > case.size() // 2
    assert np.allclose(g1, g4[:, 0] + g4[:, 1] + g4[:, 2], rtol=1e-5, atol=1e-7 * np.abs(g1).max())
    assert np.all(g4[:, 3] == 0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_reorder_noise_of_the_reference(case):
    """e_ord: the oracle's gradient with 1 thread against 16. Printed; the GPU tests take their absolute floor from the largest."""
    e = T.reorder_noise(case)
    print(f"{case.name}: e_ord = {e:.3e}")
    assert np.isfinite(e) and e < 1e-5

"""The restatement of RayTraceDR (tests/raytrace_dr_reference.py) checked against itself on the CPU: its float64 gradient against central
finite differences of its float64 loss, the three places the reference leaves open (a miss, w > 0, alpha), and what the GPU tests rely on
(the share of elements with one term on the `sparse` case; the binding's ABI rows). No GPU."""
import functools

import numpy as np
import pytest

import dr_texture_cases as T
import raytrace_dr_reference as DR
from dr_texture_cases import CASES

STEP = 2.0 ** -10                                   # a power of two: data +- STEP is exact in float64 for data in [0.2, 0.9]


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle.orc import OracleIntegrator
    case = T.BY_NAME[name]
    sc = T.scene_of(case)
    cpu = OracleIntegrator(sc)
    data, ref = T.inputs(case, sc)
    f32 = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, ref)
    return case, sc, cpu, data, ref, f32


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_float64_gradient_matches_central_differences(case):
    """L is quadratic in every texel, so (L(x + h) - L(x - h)) / 2h is the derivative but for rounding. Each L is a sum of N pixel losses of
    about 32 float64 operations each, computed to (N + 32) 2^-53 L; the quotient divides that by h. The gradient element itself is a sum of n
    float64 terms of 4 roundings each: (n + 4) 2^-53 sum|term|. The bar is the sum of the two."""
    case, sc, cpu, data, ref, f32 = _case(case.name)
    regs = DR.registrations(case)
    t64 = DR.twin(sc, cpu, regs, data, ref, geom=f32["geom"])
    touched = np.flatnonzero(t64["n"] > 0)
    assert touched.size > 0 and np.array_equal(t64["n"] > 0, f32["n"] > 0)
    N, L = f32["loss_px"].size, float(t64["loss"])
    worst = 0.0
    for j in touched:
        d = data.astype(np.float64)
        d[j] += STEP
        lp = float(DR.twin(sc, cpu, regs, d, ref, geom=f32["geom"])["loss"])
        d[j] -= 2 * STEP
        lm = float(DR.twin(sc, cpu, regs, d, ref, geom=f32["geom"])["loss"])
        fd = (lp - lm) / (2 * STEP)
        bar = (N + 32) * 2.0 ** -53 * L / STEP + (t64["n"][j] + 4) * 2.0 ** -53 * t64["sum_abs"][j]
        err = abs(fd - t64["grad"][j])
        worst = max(worst, err / bar)
        assert err <= bar, f"{case.name}: element {j} = {T.where(case, j)}: finite difference {fd:.12g}, gradient {t64['grad'][j]:.12g}, bar {bar:.3g}"
    print(f"{case.name}: {touched.size} elements, worst error / bar = {worst:.3f}")
    assert np.all(t64["grad"][t64["n"] == 0] == 0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_two_twins_and_the_float32_gradient_agree(case):
    """The float32 gradient against the twin made of its own forward values: the bound of the GPU test, (n + 4) 2^-24 sum|term| (here the sum
    runs in tid order). The two twins differ by the float32 rounding of the forward values: 16 operations' worth of the terms."""
    case, sc, cpu, data, ref, f32 = _case(case.name)
    regs = DR.registrations(case)
    a = DR.twin(sc, cpu, regs, data, ref, forward="f32", f32=f32, geom=f32["geom"])
    b = DR.twin(sc, cpu, regs, data, ref, geom=f32["geom"])
    assert np.array_equal(a["n"], f32["n"]) and np.allclose(a["sum_abs"], f32["sum_abs"], rtol=1e-6, atol=0)   # |term| in float64 / in float32
    assert np.all(np.abs(f32["grad"].astype(np.float64) - a["grad"]) <= (a["n"] + 4) * 2.0 ** -24 * a["sum_abs"])
    scale = np.abs(f32["pieces"][0][3]).max() * 2.0                                   # |d term / d diff| <= 2 |base| w, w <= 1
    assert np.all(np.abs(a["grad"] - b["grad"]) <= a["n"] * 16 * 2.0 ** -24 * scale + 16 * 2.0 ** -24 * a["sum_abs"])


def test_a_miss_contributes_ref_squared_and_no_gradient():
    case, sc, cpu, data, ref, f32 = _case("npot")
    miss = ~f32["hit"]
    assert miss.any() and f32["hit"].any()
    xy = f32["xy"]
    y, x = (xy >> 16) & 0xFFFF, xy & 0xFFFF
    r = ref[sc.height - 1 - y, x, :3]
    want = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(np.float32)
    assert np.array_equal(f32["loss_px"][miss].view(np.uint32), want[miss].view(np.uint32))
    assert not f32["param"][miss].any() and not f32["color"][miss].any()
    sentinel = np.full((sc.height, sc.width, 4), 5.0, np.float32)
    again = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, ref, into=sentinel, geom=f32["geom"])
    assert np.all(again["frame"][y[miss], x[miss]] == 5.0) and np.all(again["frame"][y[~miss], x[~miss], 3] == 0.0)
    only_hits = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, np.zeros_like(ref), geom=f32["geom"])   # ref = 0: a miss has loss 0 and still no term
    assert not only_hits["loss_px"][miss].any()
    assert np.array_equal(only_hits["n"], f32["n"])


def test_a_material_with_positive_w_contributes_no_gradient():
    """The floor's base colour with w = 0.7: its pixels render clamp(w) splat and the parameter texture gets nothing at all."""
    import copy
    from oracle.orc import OracleIntegrator
    case, sc, _, data, ref, f32 = _case("npot")
    sc2 = copy.copy(sc)
    sc2.materials = [m.copy() for m in sc.materials]
    floor = next(i for i, m in enumerate(sc2.materials) if int(m["texid"][0]) == T.FLOOR_TEX)
    sc2.materials[floor]["colors"][0][3] = 0.7
    r = DR.ray_trace_dr(sc2, OracleIntegrator(sc2), DR.registrations(case), data, ref)
    assert f32["param"].any() and not r["param"].any() and not r["n"].any() and not r["grad"].any()
    was = f32["param"]
    assert np.all(r["color"][was] == np.float32(0.7))


@pytest.mark.parametrize("case", [c for c in CASES if T.alpha_elements(c).size], ids=repr)
def test_alpha_elements_are_exactly_zero(case):
    case, sc, cpu, data, ref, f32 = _case(case.name)
    a = T.alpha_elements(case)
    assert np.all(f32["grad"][a] == 0) and np.all(f32["n"][a] == 0)
    assert np.all(f32["grad"][case.size():] == 0)


def test_sparse_has_enough_elements_with_one_term():
    """What test_raytrace_dr_gpu's bit-for-bit gradient test needs: on `sparse` (64 x 24 texels under 260 pixels) at least a quarter of the
    touched elements receive exactly one term."""
    case, sc, cpu, data, ref, f32 = _case("sparse")
    touched, single = int((f32["n"] > 0).sum()), int((f32["n"] == 1).sum())
    print(f"sparse: {single} of {touched} touched elements have one term")
    assert touched > 0 and 4 * single >= touched


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_loss_accum_bounds_hold_for_every_order_of_the_wave_adds(case):
    """lossAccum on the GPU = the nine waves' partial sums (deterministic) added by float atomics in an order that is not fixed. All 9! orders
    are tried here at the GPU test's a_passNum, against the two bounds that test asserts:
      (6 + n_waves) 2^-24 S against the float64 sum S of loss / a_passNum: a lane's share passes through 6 tree adds and at most n_waves
      atomic adds, each rounding a partial sum of non-negative terms that is at most S (1 + small) - a rigorous bound;
      n_waves 2^-24 S against the SEQUENTIAL float32 sum, the host form's value: not rigorous, because that sum's own rounding (560 adds)
      enters the difference. It holds on these inputs for every order, so the GPU test cannot fail by the order of the atomics."""
    import itertools
    from test_raytrace_dr_gpu import PASSES
    case, sc, cpu, data, ref, _ = _case(case.name)
    f32 = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, ref, pass_num=PASSES)
    n_waves = (f32["loss_px"].size + 63) // 64
    assert n_waves == 9
    orders = np.array(list(itertools.permutations(range(n_waves))), np.int64)
    sums = DR.wave_sum(f32["loss_px"], PASSES, order=orders).astype(np.float64)
    S = float((f32["loss_px"].astype(np.float64) / PASSES).sum())
    to_exact, to_seq = np.abs(sums - S).max(), np.abs(sums - float(f32["loss"])).max()
    print(f"{case.name}: {orders.shape[0]} orders, worst distance to the float64 sum {to_exact:.3e} (bound {(6 + n_waves) * 2.0 ** -24 * S:.3e}), "
          f"to the sequential float32 sum {to_seq:.3e} (bound {n_waves * 2.0 ** -24 * S:.3e}); the sequential sum itself is {abs(float(f32['loss']) - S):.3e} from the float64 sum")
    assert to_exact <= (6 + n_waves) * 2.0 ** -24 * S
    assert to_seq <= n_waves * 2.0 ** -24 * S


def test_abi_table_has_the_new_symbols():
    from hydracore3_amd import api
    assert len(api.ABI["hpt_ray_trace_dr"][1]) == 10 and len(api.ABI["hpt_ray_trace_dr_dev"][1]) == 12
    lib = api.load_library()
    assert lib.hpt_ray_trace_dr.argtypes == api.ABI["hpt_ray_trace_dr"][1] and lib.hpt_ray_trace_dr_dev.restype is api.ABI["hpt_ray_trace_dr_dev"][0]
    assert hasattr(api.HipIntegrator, "RayTraceDR") and hasattr(api.HipIntegrator, "RayTraceDR_dev")

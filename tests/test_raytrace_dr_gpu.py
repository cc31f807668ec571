"""RayTraceDR on the GPU against the numpy restatement (tests/raytrace_dr_reference.py) on dr_texture_cases' floor-and-box scene at 33 x 17:
561 lanes = two full blocks and one of 49 lanes (eight full waves and a partial one). 296 pixels hit, 265 miss; 260 of the hits are on the
floor, whose texture is the parameter texture; the box's base colour has w = 1 (a splat, no gradient).

Colours and per-pixel losses: equal bits. The host form's loss: equal bits to the restatement's sequential float32 sum. Gradient elements:
|g - twin| <= (n + 4) 2^-24 sum|term| against the float64 twin made of the float32 pass's own forward values (the module text of the
restatement derives it), equal bits where an element has one term.

lossAccum (one float atomic per wave, in an order that is not fixed) is held to two bounds, S = the float64 sum of loss / a_passNum:
  (6 + n_waves) 2^-24 S against S itself: six tree adds and at most n_waves atomic adds per lane's share, each rounding a partial sum of
  non-negative terms - rigorous;
  n_waves 2^-24 S against the SEQUENTIAL float32 sum that the host form returns (the two loss outputs are meant to agree to the
  waves' rounding). This one is not rigorous: the sequential sum's own rounding over 560 adds (up to 2.1e-5 here, bounds 3.1e-5 .. 4.5e-5)
  enters the difference. test_raytrace_dr_cpu.test_loss_accum_bounds_hold_for_every_order_of_the_wave_adds tries all 9! orders of the wave
  adds on these inputs at this a_passNum: the worst is 0.89 of the bound (`mono_npot`), so the order of the atomics cannot make it fail. At
  a_passNum = 1 the same inputs exceed it on `clamp_u` and `clamp_uv` (1.5e-4 and 1.8e-4 against 1.1e-4), by the sequential sum's rounding alone.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import dr_texture_cases as T
import raytrace_dr_reference as DR
from conftest import ROOT, scene_path
from dr_texture_cases import CASES

pytestmark = pytest.mark.gpu

HPT_ERR_ARG, HPT_ERR_STATE = 1, 3
PASSES = 3                                          # a_passNum: loss / 3 rounds
SENTINEL = np.float32(-7.5)
LAYOUTS = {"two-level": 1, "flat": 2, "sweep": 3}   # hpt_set_accel_layout values the raytrace tests force, by accel_info's name


@functools.lru_cache(maxsize=None)
def _cpu(name, grad_mode=1):
    """The restatement and its float64 twin for a case, computed once."""
    from oracle.orc import OracleIntegrator
    case = T.BY_NAME[name]
    sc = T.scene_of(case)
    cpu = OracleIntegrator(sc)
    data, ref = T.inputs(case, sc)
    regs = DR.registrations(case)
    f32 = DR.ray_trace_dr(sc, cpu, regs, data, ref, pass_num=PASSES, grad_mode=grad_mode)
    tw = DR.twin(sc, cpu, regs, data, ref, forward="f32", f32=f32, geom=f32["geom"], pass_num=PASSES, grad_mode=grad_mode)
    return case, sc, data, ref, f32, tw


class Run:
    pass


@functools.lru_cache(maxsize=None)
def _gpu(name, layout="default", grad_mode=1):
    """One integrator per (case, layout): the host form, then the device form with every output, from sentinel-filled buffers."""
    from hydracore3_amd.api import HipIntegrator
    case, sc, data, ref, _, _ = _cpu(name)
    g = HipIntegrator(sc, accel_layout=LAYOUTS.get(layout, 0))
    if layout != "default":
        assert g.accel_info()["layout"] == layout, g.accel_info()
    T.register_gpu(g, case)
    if grad_mode != 1:
        g.set_option("dr_grad_mode", grad_mode)
    r = Run()
    r.g, r.xy = g, g.packed_xy()
    r.frame = np.full((sc.height, sc.width, 4), SENTINEL, np.float32)
    r.grad = np.full(data.size, -3.0, np.float32)
    r.loss = g.RayTraceDR(g.N, 4, r.frame, PASSES, ref, data, r.grad)
    r.slots = g.GetExecutionTime("RayTraceDR")
    pre = np.zeros(data.size, np.float32)
    pre[case.size():] = T.PAD_VALUE
    d_out, d_ref, d_data, d_grad = g.dev_array(np.full((sc.height, sc.width, 4), SENTINEL, np.float32)), g.dev_array(ref), g.dev_array(data), g.dev_array(pre)
    d_px, d_acc = g.dev_array(np.full(g.N, SENTINEL, np.float32)), g.dev_array(np.zeros(1, np.float32))
    g.RayTraceDR_dev(d_out, PASSES, d_ref, d_data, d_grad, d_px, d_acc)
    r.dev_frame, r.dev_grad, r.loss_px, r.loss_acc = d_out.download(), d_grad.download(), d_px.download(), float(d_acc.download()[0])
    g.RayTraceDR_dev(d_out, PASSES, d_ref, d_data, d_grad, d_px, d_acc)
    r.dev_grad_twice = d_grad.download()
    for a in (d_out, d_ref, d_data, d_grad, d_px, d_acc):
        a.free()
    return r


def _rows(xy):
    return (xy >> 16) & 0xFFFF, xy & 0xFFFF


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_gradient(case, got, tw, factor=1.0, what=""):
    """|got - factor * twin| <= factor (n + 4) 2^-24 sum|term| on every registered element; elements without a term exactly 0."""
    n = case.size()
    err = np.abs(got[:n].astype(np.float64) - factor * tw["grad"][:n])
    bound = factor * (tw["n"][:n] + 4) * 2.0 ** -24 * tw["sum_abs"][:n]
    touched = tw["n"][:n] > 0
    print(f"{what}{case.name}: {int(touched.sum())} of {n} elements touched, worst error / bound = {float((err[touched] / bound[touched]).max()):.3f}")
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, f"{what}{case.name}: {bad.size} elements out of bound, first {T.where(case, bad[0])}: gpu {got[bad[0]]:.9g} twin {factor * tw['grad'][bad[0]]:.12g} bound {bound[bad[0]]:.3g}"
    assert np.all(got[:n][~touched] == 0)


# ---- 1. colours and losses bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_colours_and_losses_equal_the_restatement(case, layout):
    case, sc, data, ref, f32, _ = _cpu(case.name)
    r = _gpu(case.name, layout)
    y, x = _rows(r.xy)
    hit = f32["hit"]
    assert hit.any() and (~hit).any() and f32["param"].any()
    for frame in (r.frame, r.dev_frame):
        assert np.array_equal(_bits(frame[y[hit], x[hit], :3]), _bits(f32["color"][hit])), "colours of hit pixels"
        assert np.all(frame[y[hit], x[hit], 3] == 0.0)
        assert np.all(frame[y[~hit], x[~hit]] == SENTINEL), "a missed pixel of out_color was written"
    assert np.array_equal(_bits(r.loss_px), _bits(f32["loss_px"])), "per-pixel losses"
    assert np.float32(r.loss).view(np.uint32) == np.float32(f32["loss"]).view(np.uint32), (r.loss, f32["loss"])
    assert r.slots[0] > 0.0 and all(v >= 0.0 for v in r.slots[:3])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_loss_accum_agrees_with_the_sequential_sum(case):
    """See the module text for the two bounds."""
    case, sc, data, ref, f32, _ = _cpu(case.name)
    r = _gpu(case.name)
    n_waves = (f32["loss_px"].size + 63) // 64
    exact = float((f32["loss_px"].astype(np.float64) / PASSES).sum())               # sum of what is summed: loss / a_passNum
    bound = n_waves * 2.0 ** -24 * exact
    print(f"{case.name}: lossAccum {r.loss_acc:.9g}, sequential sum {float(f32['loss']):.9g}, exact {exact:.9g}, difference {r.loss_acc - float(f32['loss']):.3e}, bound {bound:.3e}")
    assert abs(r.loss_acc - exact) <= (6 + n_waves) * 2.0 ** -24 * exact, "against the float64 sum: the tree's and the atomics' roundings"
    assert abs(r.loss_acc - float(f32["loss"])) <= bound


# ---- 2. / 3. the gradient -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_gradient_element_is_within_the_derived_bound(case):
    case, sc, data, ref, f32, tw = _cpu(case.name)
    r = _gpu(case.name)
    assert (tw["n"] > 0).any()
    _assert_gradient(case, r.dev_grad, tw, what="device form, ")
    _assert_gradient(case, r.grad, tw, what="host form, ")
    assert np.all(r.dev_grad[case.size():] == T.PAD_VALUE), "the device form wrote behind the registered textures"
    assert np.all(r.grad[case.size():] == 0.0)                                      # memset(a_dataGrad, 0, a_gradSize) (integrator_dr.cpp:399)
    assert np.all(r.grad[T.alpha_elements(case)] == 0)


def test_gradient_equals_the_restatement_where_an_element_has_one_term():
    case, sc, data, ref, f32, tw = _cpu("sparse")
    r = _gpu("sparse")
    touched, single = f32["n"] > 0, f32["n"] == 1
    print(f"sparse: {int(single.sum())} of {int(touched.sum())} touched elements have one term")
    assert 4 * int(single.sum()) >= int(touched.sum())
    for got in (r.grad, r.dev_grad):
        assert np.array_equal(_bits(got[single]), _bits(f32["grad"][single]))


# ---- 4. forward-only mode -----------------------------------------------------------------------------------------------------------------------------
def test_grad_mode_zero_renders_through_the_ordinary_sampler():
    from hydracore3_amd.api import HipIntegrator
    case, sc, data, ref, _, _ = _cpu("npot")
    _, _, _, _, plain, _ = _cpu("npot", 0)
    r = _gpu("npot", grad_mode=0)
    assert not r.grad.any() and np.array_equal(r.dev_grad[:case.size()], np.zeros(case.size(), np.float32))
    cast = np.zeros((sc.height, sc.width, 4), np.float32)
    r.g.CastSingleRayBlock(r.g.N, cast)
    y, x = _rows(r.xy)
    hit = plain["hit"]
    assert np.array_equal(_bits(r.frame[y[hit], x[hit]]), _bits(cast[y[hit], x[hit]]))
    assert np.array_equal(_bits(r.loss_px), _bits(plain["loss_px"])) and np.float32(r.loss).view(np.uint32) == np.float32(plain["loss"]).view(np.uint32)
    assert not np.array_equal(_bits(plain["loss_px"]), _bits(_cpu("npot")[4]["loss_px"])), "the two samplers must differ for this to test anything"
    outs = []
    for mode in (1, 0):                                                             # PathTraceDR does not read the option
        g = HipIntegrator(sc)
        T.register_gpu(g, case)
        g.set_option("dr_grad_mode", mode)
        frame, grad = np.zeros((sc.height, sc.width, 4), np.float32), np.zeros(data.size, np.float32)
        loss = g.PathTraceDR(g.N, 4, frame, 2, ref, data, grad)
        outs.append((frame, g.random_gens(), grad, loss))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2].any() and np.allclose(outs[0][2], outs[1][2], rtol=1e-4, atol=1e-7 * np.abs(outs[0][2]).max()) and abs(outs[0][3] - outs[1][3]) <= 1e-5 * abs(outs[0][3])


# ---- 5. host and device forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["npot", "mono_npot", "two"])
def test_host_and_device_forms_agree(name):
    case, sc, data, ref, f32, tw = _cpu(name)
    r = _gpu(name)
    assert r.frame.tobytes() == r.dev_frame.tobytes()
    assert not np.any(r.grad == -3.0), "the host form overwrites a_dataGrad"
    _assert_gradient(case, r.dev_grad_twice, tw, factor=2.0, what="two device calls, ")
    assert np.all(r.dev_grad_twice[case.size():] == T.PAD_VALUE)


# ---- 6. tid shorter than the window; a window inside a larger framebuffer -----------------------------------------------------------------------------
def test_tid_shorter_than_the_window():
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    case, sc, data, ref, full, _ = _cpu("npot")
    tid = 200                                                                       # three waves and 8 lanes
    cpu = OracleIntegrator(sc)
    f32 = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, ref, pass_num=PASSES, tid=tid)
    tw = DR.twin(sc, cpu, DR.registrations(case), data, ref, forward="f32", f32=f32, geom=f32["geom"], pass_num=PASSES, tid=tid)
    g = HipIntegrator(sc)
    T.register_gpu(g, case)
    frame, grad = np.full((sc.height, sc.width, 4), SENTINEL, np.float32), np.zeros(data.size, np.float32)
    loss = g.RayTraceDR(tid, 4, frame, PASSES, ref, data, grad)
    y, x = _rows(g.packed_xy())
    done = np.zeros(g.N, bool)
    done[:tid] = full["hit"][:tid]
    assert np.all(frame[y[~done], x[~done]] == SENTINEL), "pixels past tid (or missed) were written"
    assert np.array_equal(_bits(frame[y[done], x[done], :3]), _bits(full["color"][done]))
    assert np.float32(loss).view(np.uint32) == np.float32(f32["loss"]).view(np.uint32)
    _assert_gradient(case, grad, tw, what="tid 200, ")
    d_out, d_ref, d_px = g.dev_array(frame), g.dev_array(ref), g.dev_array(np.full(g.N, SENTINEL, np.float32))
    d_data, d_grad = g.dev_array(data), g.dev_array(np.zeros(data.size, np.float32))
    g.RayTraceDR_dev(d_out, PASSES, d_ref, d_data, d_grad, d_px, None, tid=tid)
    px = d_px.download()
    assert np.all(px[tid:] == SENTINEL) and not np.any(px[:tid] == SENTINEL)


def test_window_inside_a_larger_framebuffer():
    """A 20 x 9 window at (8, 5) of the 33 x 17 framebuffer: 180 pixels. Colours equal the crop of the full frame; losses and gradient equal the
    restatement under the same parameters (yRef counts from the WINDOW's height)."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    case, sc, data, _, full, _ = _cpu("npot")
    p = sc.params()
    p.winStartX, p.winStartY, p.winWidth, p.winHeight = 8, 5, 20, 9
    ref = np.random.default_rng(9).uniform(0.0, 0.5, (9, 20, 4)).astype(np.float32)
    cpu = OracleIntegrator(sc, p)
    f32 = DR.ray_trace_dr(sc, cpu, DR.registrations(case), data, ref, pass_num=PASSES, params=p)
    tw = DR.twin(sc, cpu, DR.registrations(case), data, ref, forward="f32", f32=f32, geom=f32["geom"], pass_num=PASSES, params=p)
    g = HipIntegrator(sc, p)
    assert (g.W, g.H, g.N) == (20, 9, 180) and np.array_equal(g.packed_xy(), cpu.packed_xy())
    T.register_gpu(g, case)
    frame, grad = np.full((9, 20, 4), SENTINEL, np.float32), np.zeros(data.size, np.float32)
    loss = g.RayTraceDR(g.N, 4, frame, PASSES, ref, data, grad)
    whole = _gpu("npot").frame
    assert f32["hit"].any() and (~f32["hit"]).any()
    assert frame.tobytes() == whole[5:14, 8:28].tobytes()
    assert np.float32(loss).view(np.uint32) == np.float32(f32["loss"]).view(np.uint32)
    _assert_gradient(case, grad, tw, what="window, ")


# ---- 7. isolation --------------------------------------------------------------------------------------------------------------------------------------
def test_the_pass_draws_no_random_numbers_and_changes_no_state():
    from hydracore3_amd.api import HipIntegrator
    case, sc, data, ref, _, _ = _cpu("npot")
    outs = []
    for with_rt in (False, True):
        g = HipIntegrator(sc)
        T.register_gpu(g, case)
        g0 = g.random_gens()
        if with_rt:
            g.RayTraceDR(g.N, 4, np.zeros((sc.height, sc.width, 4), np.float32), PASSES, ref, data, np.zeros(data.size, np.float32))
            assert np.array_equal(g.random_gens(), g0)
        frame, grad = np.zeros((sc.height, sc.width, 4), np.float32), np.zeros(data.size, np.float32)
        loss = g.PathTraceDR(g.N, 4, frame, 2, ref, data, grad)
        outs.append((frame, g.random_gens(), grad, loss))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.array_equal(outs[0][1], outs[1][1])
    assert np.allclose(outs[0][2], outs[1][2], rtol=1e-4, atol=1e-7 * np.abs(outs[0][2]).max()) and abs(outs[0][3] - outs[1][3]) <= 1e-5 * abs(outs[0][3])


def test_spectral_mode_gives_the_rgb_bytes():
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml
    ref = np.random.default_rng(3).uniform(0.0, 0.5, (48, 64, 3)).astype(np.float32)
    outs = []
    for spectral in (False, True):
        g = HipIntegrator(load_hydra_xml(scene_path("test_spectral"), 64, 48, spectral=spectral))
        frame = np.zeros((48, 64, 4), np.float32)
        outs.append((g.RayTraceDR(g.N, 3, frame, 1, ref, None, None), frame))
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and outs[0][0] == outs[1][0] and outs[0][1][..., :3].any()


# ---- 8. optimisation -----------------------------------------------------------------------------------------------------------------------------------
def test_twenty_adam_iterations_lower_the_loss():
    """drmain's loop with RayTraceDR: the reference frame is this pass's own render of the case's texture, the start a texture of ones. No ratio
    is asserted (profiles/raytrace_dr.md has the curve)."""
    from hydracore3_amd.api import HipIntegrator
    case, sc, data, _, _, _ = _cpu("npot")
    g = HipIntegrator(sc)
    T.register_gpu(g, case)
    n = case.size()
    target = np.zeros((sc.height, sc.width, 4), np.float32)
    g.RayTraceDR(g.N, 4, target, 1, np.zeros_like(target), data[:n], np.zeros(n, np.float32))
    ref = np.ascontiguousarray(target[::-1])                                        # the loss reads the reference bottom-up
    d_out, d_ref, d_data = g.dev_array(np.zeros_like(target)), g.dev_array(ref), g.dev_array(np.ones(n, np.float32))
    d_grad, d_mom, d_sq, d_loss = (g.dev_array(np.zeros(k, np.float32)) for k in (n, n, n, 1))
    losses = []
    for it in range(21):
        g._chk(g.L.hpt_device_memset(g.h, d_grad.ptr, 0, d_grad.nbytes))
        g._chk(g.L.hpt_device_memset(g.h, d_loss.ptr, 0, 4))
        g.RayTraceDR_dev(d_out, 1, d_ref, d_data, d_grad, None, d_loss)
        losses.append(float(d_loss.download()[0]))
        g.AdamStep_dev(d_data, d_grad, d_mom, d_sq, it)
    print("loss per iteration: " + " ".join(f"{v:.5g}" for v in losses))
    assert np.all(np.isfinite(losses)) and losses[20] < losses[0]


# ---- 9. errors and timing ------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_messages():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    case, sc, data, ref, _, _ = _cpu("npot")
    N = sc.width * sc.height
    frame, grad = np.zeros((sc.height, sc.width, 4), np.float32), np.zeros(data.size, np.float32)
    loss = C.c_float(5.0)

    def err(g):
        return g.L.hpt_last_error(g.h).decode()

    def calls(g, tid=N, channels=4, out=frame.ctypes.data, rf=ref.ctypes.data, size=data.size):
        return [lambda: g.L.hpt_ray_trace_dr(g.h, tid, channels, out, 1, rf, data.ctypes.data, grad.ctypes.data, size, C.byref(loss)),
                lambda: g.L.hpt_ray_trace_dr_dev(g.h, tid, channels, out, 1, rf, data.ctypes.data, grad.ctypes.data, size, None, None, None)]

    fresh = HipIntegrator()
    for call in calls(fresh, 1):
        assert call() == HPT_ERR_STATE and "CommitDeviceData" in err(fresh) and "RayTraceDR" in err(fresh)
    fresh.scene, fresh._desc = sc, sc.desc()
    fresh.CommitDeviceData()
    for call in calls(fresh, 1):                                                    # (the acceleration structure is committed with the upload)
        assert call() == HPT_ERR_STATE and "UpdateMembersPlainData" in err(fresh) and "RayTraceDR" in err(fresh)
    fresh.UpdateMembersPlainData(sc.params())
    for call in calls(fresh, 1):
        assert call() == HPT_ERR_STATE and "PackXYBlock" in err(fresh) and "RayTraceDR" in err(fresh)
    fresh.PackXYBlock(sc.width, sc.height)
    assert calls(fresh)[0]() == 0 and frame[..., :3].any()                          # no InitRandomGens needed

    g = HipIntegrator(sc)
    T.register_gpu(g, case)
    assert g.L.hpt_ray_trace_dr(None, N, 4, frame.ctypes.data, 1, ref.ctypes.data, data.ctypes.data, grad.ctypes.data, data.size, C.byref(loss)) == HPT_ERR_ARG
    for call in calls(g, out=None):
        assert call() == HPT_ERR_ARG and "out_color is null" in err(g)
    for call in calls(g, rf=None):
        assert call() == HPT_ERR_ARG and "a_refImg is null" in err(g)
    for call in calls(g, tid=N + 1):
        assert call() == HPT_ERR_ARG and "tid" in err(g) and "RayTraceDR" in err(g)
    for channels in (0, 1, 2, 5):
        for call in calls(g, channels=channels):
            assert call() == HPT_ERR_ARG and "channels" in err(g)
    for call in calls(g, size=case.size() - 1):
        assert call() == HPT_ERR_ARG and "a_gradSize" in err(g)
    for call in [lambda: g.L.hpt_ray_trace_dr(g.h, N, 4, frame.ctypes.data, 1, ref.ctypes.data, data.ctypes.data, None, data.size, C.byref(loss)),
                 lambda: g.L.hpt_ray_trace_dr_dev(g.h, N, 4, frame.ctypes.data, 1, ref.ctypes.data, data.ctypes.data, None, data.size, None, None, None)]:
        assert call() == HPT_ERR_ARG and "a_dataGrad is null" in err(g)
    with pytest.raises(HydraHipError, match="a_gradSize"):                          # a_data without a_dataGrad: a_gradSize 0 is below the registered size
        g.RayTraceDR(N, 4, frame, 1, ref, data, None)
    with pytest.raises(HydraHipError, match="channels"):
        g.RayTraceDR(N, 2, frame, 1, ref, data, grad)
    with pytest.raises(HydraHipError, match="dr_grad_mode"):
        g.set_option("dr_grad_mode", 2)
    grad[:] = 4.0
    before = frame.copy()
    assert calls(g, tid=0)[0]() == 0 and loss.value == 0.0 and not grad.any() and frame.tobytes() == before.tobytes()   # tid = 0: the gradient zeroed, loss 0
    g.L.hpt_set_accel_layout(g.h, 1)
    for call in calls(g, 1):
        assert call() == HPT_ERR_STATE and "CommitScene" in err(g)
    g.CommitScene()
    assert calls(g)[0]() == 0


def test_execution_time_slots():
    from hydracore3_amd.api import HipIntegrator
    case, sc, data, ref, _, _ = _cpu("npot")
    g = HipIntegrator(sc)
    T.register_gpu(g, case)
    assert g.GetExecutionTime("RayTraceDR") == [0.0, 0.0, 0.0, 0.0]
    g.RayTraceDR(g.N, 4, np.zeros((sc.height, sc.width, 4), np.float32), 1, ref, data, np.zeros(data.size, np.float32))
    slots = g.GetExecutionTime("RayTraceDR")
    assert slots[0] > 0.0 and all(v >= 0.0 for v in slots[:3]) and abs(g.last_kernel_ms() - slots[0]) < 1e-6
    assert g.GetExecutionTime("PathTraceDR")[0] == 0.0 and g.GetExecutionTime("CastSingleRayBlock")[0] == 0.0
    g.CastSingleRayBlock(g.N, np.zeros((sc.height, sc.width, 4), np.float32))
    assert g.GetExecutionTime("RayTraceDR") == slots


# ---- 10. the C++ demo ----------------------------------------------------------------------------------------------------------------------------------
def test_cpp_demo_prints_the_host_forms_loss():
    tool = os.path.join(ROOT, "hydracore3_amd", "raytrace_dr_demo")
    assert os.path.exists(tool), "build() compiles tests/cpp/raytrace_dr_demo.cpp"
    r = subprocess.run([tool], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"loss = ([0-9.eE+-]+) \(expected ([0-9.eE+-]+)\), gradient sum = ([0-9.eE+-]+) \(expected ([0-9.eE+-]+)\)", r.stdout)
    assert m, r.stdout
    loss, want_loss, gsum, want_gsum = (float(v) for v in m.groups())
    base = np.array([0.2, 0.5, 0.9], np.float32).astype(np.float64)
    d = 0.5 * base - 0.25
    assert abs(want_loss - 48 * 32 * float((d * d).sum()) / 2) <= 1e-6 * want_loss and abs(want_gsum - 48 * 32 * float((2 * d * base).sum())) <= 1e-6 * abs(want_gsum)
    assert abs(loss - want_loss) <= 1e-4 * want_loss and abs(gsum - want_gsum) <= 1e-4 * abs(want_gsum)

"""PathTraceVJP on the GPU (hpt_path_trace_vjp / _dev, hydracore3_amd.torch_dr): the same paths as PathTraceDR bit for bit, the gradient against
the device's own PathTraceDR adjoint and against the oracle (one sample per pixel directly, four by linearity: vjp_cases.py), zeros, windows,
refusals, and the PyTorch op. Scenes and bounds are dr_texture_cases.py's; every case under the three schedules."""
import functools

import numpy as np
import pytest

import dr_texture_cases as T
import vjp_cases as V
from conftest import scene_path
from dr_texture_cases import SCHEDULES
from vjp_cases import CASES, SPP

pytestmark = pytest.mark.gpu

HPT_ERR_ARG, HPT_ERR_UNSUPPORTED = 1, 4
FILL = -3.0                                     # what buffers the call must overwrite, or must not touch, are pre-filled with


def _gpu(case, schedule, sc=None):
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(T.scene_of(case) if sc is None else sc)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    T.register_gpu(gpu, case)
    return gpu


def _frame(gpu):
    return np.zeros((gpu.H, gpu.W, 4), np.float32)


def _vjp(case, schedule, adj, spp=SPP, tid_begin=0, tid_count=None, with_grad=True):
    """One host-form PathTraceVJP call on a fresh integrator into a zero frame and a gradient buffer pre-filled with FILL.
    Returns (frame, grad, generators)."""
    gpu = _gpu(case, schedule)
    data, _ = T.inputs(case, gpu.scene)
    frame, grad = _frame(gpu), np.full(data.size, FILL, np.float32)
    gpu.PathTraceVJP(gpu.N - tid_begin if tid_count is None else tid_count, 4, frame, spp, adj, data, grad if with_grad else None, tid_begin=tid_begin)
    assert gpu.last_schedule()[0] == schedule
    assert np.all(data[case.size():] == T.PAD_VALUE)                                  # a_data is only read
    return frame, grad, gpu.random_gens()


@functools.lru_cache(maxsize=None)
def dr_run(case, schedule, spp):
    """PathTraceDR from the same start with dr_texture_cases.inputs' reference frame: (frame, gradient, generators)."""
    gpu = _gpu(case, schedule)
    data, ref = T.inputs(case, gpu.scene)
    frame, grad = _frame(gpu), np.full(data.size, FILL, np.float32)
    gpu.PathTraceDR(gpu.N, 4, frame, spp, ref, data, grad)
    assert gpu.last_schedule()[0] == schedule
    return frame, grad, gpu.random_gens()


@functools.lru_cache(maxsize=None)
def linear_run(case, schedule):
    """The VJP of A = 2 (R2 - R1) at SPP samples per pixel, shared by the tests that look at it."""
    r1, d, _ = V.grid_frames(T.scene_of(case))
    return _vjp(case, schedule, V.adjoint_of(r1, r1 + d))


def _same_sums(a, b):
    """The project's floor for the same sums in another order (test_dr_textures_gpu.test_second_run_overwrites_the_gradient)."""
    return np.allclose(a, b, rtol=1e-4, atol=1e-7 * np.abs(b).max())


# ---- (a) same paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_same_paths_as_path_trace_dr(case, schedule):
    """Frame and m_randomGens after a VJP call - with an adjoint, and with none - equal PathTraceDR's bit for bit; without an adjoint a
    pre-filled gradient buffer stays as it was."""
    f_dr, _, gens_dr = dr_run(case, schedule, SPP)
    frame, grad, gens = linear_run(case, schedule)
    assert np.array_equal(frame.view(np.uint32), f_dr.view(np.uint32)) and np.array_equal(gens, gens_dr)
    assert np.count_nonzero(grad[:case.size()]) > 0
    frame0, grad0, gens0 = _vjp(case, schedule, None)
    assert np.array_equal(frame0.view(np.uint32), f_dr.view(np.uint32)) and np.array_equal(gens0, gens_dr)
    assert np.all(grad0 == FILL)
    frame1, _, gens1 = _vjp(case, schedule, None, with_grad=False)                    # a_dataGrad may be null then
    assert np.array_equal(frame1.view(np.uint32), f_dr.view(np.uint32)) and np.array_equal(gens1, gens_dr)


# ---- (b) one sample per pixel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_one_sample_equals_the_dr_adjoint_and_the_oracle(case, schedule):
    """At one sample per pixel PathTraceDR's seed 2 (colour - ref) can be formed from its frame: the VJP of that adjoint is PathTraceDR's
    gradient, the same products summed by the atomics in another order. And it meets the oracle's gradient as PathTraceDR's does."""
    n = case.size()
    c, g_dr, _ = dr_run(case, schedule, 1)
    _, ref = T.inputs(case, T.scene_of(case))
    adj = (np.float32(2.0) * (c - ref[::-1])).astype(np.float32)
    adj[..., 3] = FILL                                                                # the fourth float of an adjoint pixel is not read
    _, grad, _ = _vjp(case, schedule, adj, spp=1)
    print(f"{case.name}, schedule {schedule}: max |vjp - dr| / max|dr| = {np.abs(grad[:n] - g_dr[:n]).max() / np.abs(g_dr[:n]).max():.3e}")
    assert np.count_nonzero(g_dr[:n]) > 0
    assert _same_sums(grad[:n], g_dr[:n])
    gc = V.oracle_gradient(case, "ref", 1)
    T.assert_elements(case, grad[:n], gc, T.element_atol(gc), f"schedule {schedule}, 1 spp: ")


# ---- (c) four samples per pixel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_four_samples_against_the_oracle_by_linearity(case, schedule):
    """V(2 (R2 - R1)) = G(R1) - G(R2) with the oracle's PathTraceDR gradients G (vjp_cases.py; the oracle alone meets the bound with room:
    test_vjp_cpu.test_the_linearity_bound_is_met_by_the_oracle_alone)."""
    n = case.size()
    g1, g2 = V.oracle_gradient(case, "r1"), V.oracle_gradient(case, "r2")
    _, grad, _ = linear_run(case, schedule)
    want, bound = g1 - g2, V.linearity_bound(g1, g2)
    err = np.abs(grad[:n].astype(np.float64) - want)
    print(f"{case.name}, schedule {schedule}: worst error / bound = {(err / bound).max():.3e}, / max|V| = {err.max() / np.abs(want).max():.3e}, "
          f"non-zero elements {np.count_nonzero(want)} of {n}")
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, f"{bad.size} elements out of bound, first: {T.where(case, bad[0])} gpu {grad[bad[0]]:.9g} oracle {want[bad[0]]:.9g}"
    assert np.count_nonzero(want) > 0


# ---- (d) zeros -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_zeros(case, schedule):
    """A zero adjoint: no element of the gradient is non-zero (the host form zeroes all of a_gradSize, the tail behind the registered
    textures included, and nothing is scattered). With an adjoint: alpha elements are zero, and so is the tail - no tap lands outside the
    registered textures; a_data's tail is only read (checked in every call)."""
    n = case.size()
    _, grad, _ = _vjp(case, schedule, np.zeros((T.scene_of(case).height, T.scene_of(case).width, 4), np.float32))
    assert np.count_nonzero(grad) == 0
    _, grad, _ = linear_run(case, schedule)
    assert np.all(grad[T.alpha_elements(case)] == 0)
    assert grad.size == n + T.PAD and np.all(grad[n:] == 0)


# ---- (e) windows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_unaligned_windows_sum_to_the_whole_call(schedule):
    case = T.BY_NAME["npot"]
    n = case.size()
    r1, d, _ = V.grid_frames(T.scene_of(case))
    adj = V.adjoint_of(r1, r1 + d)
    f_whole, g_whole, gens_whole = linear_run(case, schedule)
    halves = [_vjp(case, schedule, adj, tid_begin=b, tid_count=cnt) for b, cnt in ((0, 200), (200, 361))]
    assert np.array_equal((halves[0][0] + halves[1][0]).view(np.uint32), f_whole.view(np.uint32))
    assert np.array_equal(np.where((np.arange(gens_whole.shape[0]) < 200)[:, None], halves[0][2], halves[1][2]), gens_whole)
    total = halves[0][1][:n] + halves[1][1][:n]
    assert np.count_nonzero(halves[0][1][:n]) > 0 and np.count_nonzero(halves[1][1][:n]) > 0
    assert np.allclose(total, g_whole[:n], rtol=1e-5, atol=1e-7 * np.abs(g_whole[:n]).max())


# ---- (f) errors ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    from hydracore3_amd.scene import load_hydra_xml
    case = T.BY_NAME["npot"]
    gpu = _gpu(case, 1)
    L, n = gpu.L, case.size()
    data, _ = T.inputs(case, gpu.scene)
    gens = gpu.random_gens()

    def buffers(channels=4):
        return (np.full((gpu.H, gpu.W, max(channels, 1)), FILL, np.float32), np.full((gpu.H, gpu.W, max(channels, 1)), 0.5, np.float32),
                np.full(data.size, FILL, np.float32))

    def host(ctx, channels, frame, adj, grad, grad_size):
        return L.hpt_path_trace_vjp(ctx, 0, gpu.N, channels, frame.ctypes.data, SPP, adj.ctypes.data, data.ctypes.data,
                                    None if grad is None else grad.ctypes.data, grad_size)

    def dev(ctx, channels, grad_ptr, grad_size, d):
        return L.hpt_path_trace_vjp_dev(ctx, 0, gpu.N, channels, d["frame"].ptr, SPP, d["adj"].ptr, d["data"].ptr, grad_ptr, grad_size, None)

    frame, adj, grad = buffers()
    d = {"frame": gpu.dev_array(frame), "adj": gpu.dev_array(adj), "data": gpu.dev_array(data), "grad": gpu.dev_array(grad)}
    calls = [("no context", lambda: host(None, 4, frame, adj, grad, data.size), lambda: dev(None, 4, d["grad"].ptr, data.size, d), None)]
    for ch in (1, 2, 5):
        f_ch, a_ch, _ = buffers(ch)
        calls.append((f"channels {ch}", lambda ch=ch, f_ch=f_ch, a_ch=a_ch: host(gpu.h, ch, f_ch, a_ch, grad, data.size),
                      lambda ch=ch: dev(gpu.h, ch, d["grad"].ptr, data.size, d), "channels must be 3 or 4"))
    calls.append(("short gradSize", lambda: host(gpu.h, 4, frame, adj, grad, n - 1), lambda: dev(gpu.h, 4, d["grad"].ptr, n - 1, d), "a_gradSize smaller"))
    calls.append(("adjoint without a gradient buffer", lambda: host(gpu.h, 4, frame, adj, None, data.size), lambda: dev(gpu.h, 4, None, data.size, d), "needs a_dataGrad"))
    for what, host_call, dev_call, message in calls:
        for call in (host_call, dev_call):
            assert call() == HPT_ERR_ARG, what
            if message is not None:
                assert message in L.hpt_last_error(gpu.h).decode(), (what, L.hpt_last_error(gpu.h).decode())
    assert np.all(frame == FILL) and np.all(grad == FILL)
    assert np.all(d["frame"].download() == FILL) and np.all(d["grad"].download() == FILL)
    assert np.array_equal(gpu.random_gens(), gens)

    # the environment-map fixture (test_gpu_dr.test_dr_refuses_environment_maps): HPT_ERR_UNSUPPORTED with the very message PathTraceDR gives for it
    env = HipIntegrator(load_hydra_xml(scene_path("env_map"), 32, 32))
    img, a4, p, g = np.full((32, 32, 4), FILL, np.float32), np.ones((32, 32, 4), np.float32), np.zeros(4, np.float32), np.full(4, FILL, np.float32)
    messages = []
    for fn in (env.PathTraceVJP, env.PathTraceDR):
        with pytest.raises(HydraHipError, match="not differentiated") as e:
            fn(env.N, 4, img, 1, a4, p, g)
        messages.append(str(e.value))
    assert messages[0] == messages[1] and messages[0].startswith(f"hydra_hip error {HPT_ERR_UNSUPPORTED}:")
    assert np.all(img == FILL) and np.all(g == FILL)
    # (that fixture has a lens stack too, which is refused first.) The case's own scene with a texture bound as its environment map:
    sc = T.scene_of(case)
    sc.env_tex_id = T.BOX_TEX
    env = _gpu(case, 1, sc)
    frame, grad = np.full((sc.height, sc.width, 4), FILL, np.float32), np.full(data.size, FILL, np.float32)
    with pytest.raises(HydraHipError, match=f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: environment maps"):
        env.PathTraceVJP(env.N, 4, frame, SPP, np.ones_like(frame), data, grad)
    assert np.all(frame == FILL) and np.all(grad == FILL)


# ---- device form -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_device_form_accumulates(schedule):
    """hpt_path_trace_vjp_dev adds to dataGradDev: two calls from the same generators leave twice the host form's gradient, and the tail behind
    the registered textures keeps what it held. GetExecutionTime("PathTraceVJP") answers with the host form's four slots."""
    case = T.BY_NAME["two"]
    n = case.size()
    gpu = _gpu(case, schedule)
    data, _ = T.inputs(case, gpu.scene)
    r1, dd, _ = V.grid_frames(gpu.scene)
    adj = V.adjoint_of(r1, r1 + dd)
    before = np.zeros(data.size, np.float32)
    before[n:] = FILL
    start = gpu.random_gens()
    d_frame, d_adj, d_data, d_grad = (gpu.dev_array(a) for a in (_frame(gpu), adj, data, before))
    gpu.PathTraceVJP_dev(d_frame, SPP, d_adj, d_data, d_grad)
    frame, once = d_frame.download(), d_grad.download()
    gpu.set_random_gens(start)
    gpu.PathTraceVJP_dev(d_frame, SPP, d_adj, d_data, d_grad)
    twice = d_grad.download()
    f_host, g_host, _ = linear_run(case, schedule)
    assert np.array_equal(frame.view(np.uint32), f_host.view(np.uint32))
    assert np.all(once[n:] == FILL) and np.all(twice[n:] == FILL)
    assert _same_sums(once[:n], g_host[:n]) and _same_sums(twice[:n], 2.0 * g_host[:n])
    slots = gpu.GetExecutionTime("PathTraceVJP")
    assert slots == [0.0, 0.0, 0.0, 0.0]                                               # (no host-form call on this integrator yet)
    gpu.PathTraceVJP(gpu.N, 4, _frame(gpu), 1, adj, data, np.zeros(data.size, np.float32))
    slots = gpu.GetExecutionTime("PathTraceVJP")
    assert slots[0] > 0 and slots[1] > 0 and slots[2] > 0


# ---- (g) torch -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def torch_results():
    """The PyTorch op's checks run in ONE child process (vjp_torch_child.py): torch brings a HIP runtime of its own, which has to come up
    before libhydra_hip.so's does and must not be loaded into this session at all (see test_cpu.test_no_gpu_means_loud_failure_not_fallback)."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vjp_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_torch_render_and_backward(schedule):
    """render() equals the null-adjoint frame bit for bit; for L = (img * Wt).sum() params.grad equals PathTraceVJP_dev of Wt to the floor of
    the same sums in another order; the generators after backward are those after forward; malformed params raise ValueError."""
    assert torch_results()[f"render_and_backward[{schedule}]"] == "ok"


def test_torch_adam_lowers_an_l1_loss():
    """Ten steps of torch.optim.Adam on an L1 loss to a frame rendered from other parameters end with a smaller loss than they started with."""
    assert torch_results()["adam"] == "ok"

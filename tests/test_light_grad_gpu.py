"""Light-colour gradients on the GPU (hpt_put_diff_lights): the forward frame bit for bit against a host-premultiplied scene,
the gradient of every light and channel against single-light frames under a derived worst-case bound, C_0 excluded, PathTraceDR's own loss,
textures and lights together, lights past the workgroups' bins, the device form, refusals and the PyTorch op. Scenes, gains and the bound are
light_grad_cases.py's; every case under the megakernel and the wavefront schedule, fixed seeds.

Worst observed |error| / bound: see profiles/light_grad.md."""
import functools

import numpy as np
import pytest

import light_grad_cases as G
from light_grad_cases import SCHEDULES

pytestmark = pytest.mark.gpu

HPT_ERR_ARG, HPT_ERR_UNSUPPORTED = 1, 4
FILL = -3.0
PAD = 8                                          # floats of a_data / a_dataGrad behind the registered ranges
N = G.WIDTH * G.HEIGHT
WINDOWS = {"whole": (0, N), "unaligned": (37, 300)}     # 300 threads from 37: no wave boundary at either end, a last wave of 44 lanes
SCENES = {"A": G.scene_a, "B": G.scene_b, "many": G.many_lights_scene}


def _gpu(sc, schedule, lights=None):
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(sc)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    if lights is not None:
        gpu.Update_m_lights(0, lights)
    return gpu


def _render(gpu, spp, window, data=None):
    """The frame of PathTraceVJP with a null adjoint; (frame, generators after)."""
    frame = np.zeros((gpu.H, gpu.W, 4), np.float32)
    gpu.PathTraceVJP(window[1], 4, frame, spp, None, np.zeros(4, np.float32) if data is None else data, None, tid_begin=window[0])
    return frame, gpu.random_gens()


@functools.lru_cache(maxsize=None)
def single_frames(scene, schedule, spp, window, which=None):
    """{l: F_l, None: F_0} through the existing kernels, lights unregistered: one integrator, the lights scaled with Update_m_lights and the
    generators put back before every frame. Also the packed pixel coordinates."""
    sc = SCENES[scene]()
    gpu = _gpu(sc, schedule)
    start, out = gpu.random_gens(), {}
    for l in [None] + list(range(len(sc.lights)) if which is None else which):
        gpu.Update_m_lights(0, G.only_light(sc, l))
        gpu.set_random_gens(start)
        out[l] = _render(gpu, spp, WINDOWS[window])[0]
        assert gpu.last_schedule()[0] == schedule
    return out, gpu.packed_xy()


def _data(n_lights, g, tex=None):
    """a_data: [the box texture], the gains, PAD floats of FILL; (data, offset of the gains)."""
    head = np.zeros(0, np.float32) if tex is None else tex.reshape(-1)
    return np.concatenate([head, np.asarray(g, np.float32).reshape(-1), np.full(PAD, FILL, np.float32)]).astype(np.float32), head.size


def _tex_values():
    t = np.random.default_rng(G.SEED + 7).uniform(0.2, 0.9, (G.TEX_H, G.TEX_W, 4)).astype(np.float32)
    t[..., 3] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def light_run(scene, schedule, spp, window, gains_kind, with_tex=False, adj_seed=G.SEED):
    """One host-form PathTraceVJP with every light of the scene registered: (frame, gradient, generators, offset of the gains, data)."""
    sc = SCENES[scene]()
    n = len(sc.lights)
    g = G.gains(n) if gains_kind == "random" else np.ones((n, 4), np.float32)
    gpu = _gpu(sc, schedule)
    tex = _tex_values() if with_tex else None
    if with_tex:
        assert tuple(gpu.PutDiffTex2D(G.BOX_TEX, G.TEX_W, G.TEX_H, 4)) == (0, G.TEX_W * G.TEX_H * 4)
    data, off = _data(n, g, tex)
    assert tuple(gpu.PutDiffLights(0, n)) == (off, 4 * n)
    frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
    w = WINDOWS[window]
    gpu.PathTraceVJP(w[1], 4, frame, spp, G.adjoint(adj_seed), data, grad, tid_begin=w[0])
    assert gpu.last_schedule()[0] == schedule
    return frame, grad, gpu.random_gens(), off, data


def _check_lights(scene, schedule, spp, window, grad, off, lights=None, what=""):
    """Case 2's bound for the given lights (all of them by default); returns the worst |error| / bound."""
    frames, xy = single_frames(scene, schedule, spp, window, None if lights is None else tuple(lights))
    w = WINDOWS[window]
    mask = G.pixel_mask(xy, w[0], w[1])
    n = w[1] * spp * (G.DEPTH + 1)
    a, worst = G.adjoint(), 0.0
    for l in sorted(k for k in frames if k is not None):
        want, bound = G.expected_and_bound(a, frames[l], frames[None], mask, n)
        got = grad[off + 4 * l: off + 4 * l + 3].astype(np.float64)
        ratio = np.abs(got - want) / bound
        print(f"{what}scene {scene}, schedule {schedule}, spp {spp}, {window}: light {l} grad {got} expected {want} |error| / bound {ratio}")
        assert np.all(bound > 0.0) and np.all(np.abs(want) > 0.0), f"light {l}: the check is vacuous"
        assert np.all(np.abs(got - want) <= bound), f"light {l}: gradient {got}, expected {want}, bound {bound}"
        worst = max(worst, float(ratio.max()))
    print(f"{what}scene {scene}, schedule {schedule}, spp {spp}, {window}: worst |error| / bound = {worst:.3e}")
    return worst


def _same_sums(a, b):
    """The same sums in another order (test_vjp_gpu._same_sums)."""
    return np.allclose(a, b, rtol=1e-4, atol=1e-7 * np.abs(b).max())


# ---- 1. forward, bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_forward_is_the_premultiplied_scene_bit_for_bit(schedule):
    sc = G.scene_a()
    n, spp, w = len(sc.lights), 4, WINDOWS["whole"]
    g = G.gains(n)
    assert np.any(g[:, :3] == 0.0) and np.all(g[n - 1, :3] == 1.0)
    plain, plain_gens = _render(_gpu(sc, schedule), spp, w)
    pre, pre_gens = _render(_gpu(sc, schedule, G.scaled_lights(sc, g)), spp, w)
    for gains, want, want_gens in ((g, pre, pre_gens), (np.ones((n, 4), np.float32), plain, plain_gens)):
        gpu = _gpu(sc, schedule)
        data, off = _data(n, gains)
        gpu.PutDiffLights(0, n)
        frame, gens = _render(gpu, spp, w, data)
        assert gpu.last_schedule()[0] == schedule
        assert np.array_equal(frame, want) and np.array_equal(frame.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(gens, want_gens)
    assert not np.array_equal(pre, plain)
    # ... and with an adjoint the frame and the generators are the same again
    frame, _, gens, _, _ = light_run("A", schedule, spp, "whole", "random")
    assert np.array_equal(frame, pre) and np.array_equal(gens, pre_gens)


# ---- 2. / 3. the gradient against single-light frames, whatever the gains ---------------------------------------------------------------------
@pytest.mark.parametrize("gains_kind", ["random", "ones"])
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_gradient_against_single_light_frames(schedule, spp, window, gains_kind):
    """|grad[l, c] - sum_p a[p, c] (F_l - F_0)[p, c]| <= 2 (n + 8) 2^-24 sum_p |a[p, c]| (F_l + F_0)[p, c], n = tid * spp * (traceDepth + 1), for
    every light and channel, at random gains (one channel exactly 0) and at gains of one: the derivative is per unit gain."""
    sc = G.scene_a()
    frames, _ = single_frames("A", schedule, 4, "whole")
    for l in range(len(sc.lights)):                                                  # the fixture is not vacuous
        assert G.lit_fraction(frames[l], frames[None]) > 0.05, f"light {l} lights {G.lit_fraction(frames[l], frames[None]):.3f} of the pixels"
    for l in G.AREA_LIGHTS:
        assert G.emitter_pixels(frames[l], sc.lights[l], 4) > 0, f"area light {l}: no pixel shows its mesh"
    _, grad, _, off, data = light_run("A", schedule, spp, window, gains_kind)
    _check_lights("A", schedule, spp, window, grad, off)
    n = len(sc.lights)
    assert np.all(grad[off + 3: off + 4 * n: 4] == 0.0)                               # the padding floats
    assert np.all(grad[off + 4 * n:] == 0.0)                                          # (the host form zeroes all of a_gradSize)
    if gains_kind == "random":
        assert data[off + 4 * 1 + 1] == 0.0 and grad[off + 4 * 1 + 1] != 0.0          # the gradient of the channel whose gain is 0


# ---- 4. C_0 is excluded -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_environment_and_unbound_emitters_carry_no_gradient(schedule):
    frames, _ = single_frames("B", schedule, 4, "whole")
    assert frames[None][..., :3].max() > 0.0                                         # F_0 != 0 on scene B
    _, grad, _, off, _ = light_run("B", schedule, 4, "whole", "random")
    _check_lights("B", schedule, 4, "whole", grad, off)


@pytest.mark.parametrize("scene", ["A", "many"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_homogeneity(scene, schedule):
    """Without an environment and unbound emitters C is homogeneous of degree one in the gains: sum_l g_l . grad_l = <a, F(g)>, channel by
    channel, within sum_l g_l bound_l = 2 (n + 8) 2^-24 sum_p |a| F(g)."""
    spp = 4
    frame, grad, _, off, data = light_run(scene, schedule, spp, "whole", "random")
    nl = len(SCENES[scene]().lights)
    g = data[off: off + 4 * nl].reshape(nl, 4)[:, :3].astype(np.float64)
    got = (g * grad[off: off + 4 * nl].reshape(nl, 4)[:, :3].astype(np.float64)).sum(axis=0)
    a = G.adjoint()[..., :3].astype(np.float64)
    want = (a * frame[..., :3]).sum(axis=(0, 1))
    bound = 2.0 * (N * spp * (G.DEPTH + 1) + 8) * 2.0 ** -24 * (np.abs(a) * frame[..., :3]).sum(axis=(0, 1))
    print(f"scene {scene}, schedule {schedule}: sum g grad {got}, <a, F(g)> {want}, |error| / bound {np.abs(got - want) / bound}")
    assert np.all(np.abs(want) > 0.0) and np.all(np.abs(got - want) <= bound)


# ---- 5. PathTraceDR's own loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_path_trace_dr_equals_the_vjp_of_its_own_adjoint(schedule):
    """At one sample per pixel PathTraceDR's seed 2 (colour - ref) can be formed from its frame (a_refImg is bottom-up)."""
    sc = G.scene_a()
    n = len(sc.lights)
    data, off = _data(n, G.gains(n))
    ref = np.random.default_rng(G.SEED + 3).uniform(0.0, 0.5, (G.HEIGHT, G.WIDTH, 4)).astype(np.float32)
    grads = []
    for adj in (None, "from the frame"):
        gpu = _gpu(sc, schedule)
        gpu.PutDiffLights(0, n)
        frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
        if adj is None:
            gpu.PathTraceDR(gpu.N, 4, frame, 1, ref, data, grad)
            colour = frame
        else:
            a = (np.float32(2.0) * (colour - ref[::-1])).astype(np.float32)
            gpu.PathTraceVJP(gpu.N, 4, frame, 1, a, data, grad)
            assert np.array_equal(frame, colour)
        assert gpu.last_schedule()[0] == schedule
        grads.append(grad[off: off + 4 * n])
    print(f"schedule {schedule}: max |vjp - dr| / max |dr| = {np.abs(grads[1] - grads[0]).max() / np.abs(grads[0]).max():.3e}")
    assert np.count_nonzero(grads[0]) == 3 * n and _same_sums(grads[1], grads[0])


# ---- 6. textures and lights together ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_textures_and_lights_together(schedule):
    sc = G.scene_a()
    n, nt, spp = len(sc.lights), G.TEX_W * G.TEX_H * 4, 4
    _, grad, _, off, data = light_run("A", schedule, spp, "whole", "random", True)
    assert off == nt
    # the texture part: the premultiplied scene with the texture alone registered
    gpu = _gpu(sc, schedule, G.scaled_lights(sc, G.gains(n)))
    gpu.PutDiffTex2D(G.BOX_TEX, G.TEX_W, G.TEX_H, 4)
    tex_data = np.concatenate([data[:nt], np.full(PAD, FILL, np.float32)])
    tex_grad = np.full(tex_data.size, FILL, np.float32)
    gpu.PathTraceVJP(gpu.N, 4, np.zeros((gpu.H, gpu.W, 4), np.float32), spp, G.adjoint(), tex_data, tex_grad)
    assert np.count_nonzero(tex_grad[:nt]) > 0 and _same_sums(grad[:nt], tex_grad[:nt])
    # the light part: the bound of case 2, against frames rendered with the same box texture bound (the fixture's own image differs from a_data's)
    frames = {}
    ref = _gpu(sc, schedule)
    ref.PutDiffTex2D(G.BOX_TEX, G.TEX_W, G.TEX_H, 4)
    start = ref.random_gens()
    for l in [None] + list(range(n)):
        ref.Update_m_lights(0, G.only_light(sc, l))
        ref.set_random_gens(start)
        frames[l] = _render(ref, spp, WINDOWS["whole"], tex_data)[0]
    a, mask = G.adjoint(), np.ones((G.HEIGHT, G.WIDTH), bool)
    for l in range(n):
        want, bound = G.expected_and_bound(a, frames[l], frames[None], mask, N * spp * (G.DEPTH + 1))
        got = grad[off + 4 * l: off + 4 * l + 3].astype(np.float64)
        assert np.all(np.abs(want) > 0.0) and np.all(np.abs(got - want) <= bound), (l, got, want, bound)
    assert np.all(grad[off + 3: off + 4 * n: 4] == 0.0) and np.all(grad[off + 4 * n:] == 0.0)


# ---- 7. past the bin capacity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_lights_past_the_bins(schedule):
    """BINS + 5 point lights: the first light, the last one inside the bins, the first one past them and the last one meet case 2's bound
    (the homogeneity identity over all of them: test_homogeneity["many"])."""
    assert len(G.many_lights_scene().lights) == G.BINS + 5
    _, grad, _, off, _ = light_run("many", schedule, 4, "whole", "random")
    _check_lights("many", schedule, 4, "whole", grad, off, lights=(0, G.BINS - 1, G.BINS, G.BINS + 4))


# ---- 8. device form and ABI edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_device_form_accumulates_and_touches_nothing_else(schedule):
    sc = G.scene_a()
    n, spp = len(sc.lights), 4
    gpu = _gpu(sc, schedule)
    data, off = _data(n, G.gains(n))
    gpu.PutDiffLights(0, n)
    before = np.full(data.size, FILL, np.float32)
    before[off: off + 4 * n] = 0.5
    d_frame, d_adj, d_data, d_grad = (gpu.dev_array(x) for x in (np.zeros((gpu.H, gpu.W, 4), np.float32), G.adjoint(), data, before))
    gpu.PathTraceVJP_dev(d_frame, spp, d_adj, d_data, d_grad)
    got = d_grad.download()
    _, host, _, _, _ = light_run("A", schedule, spp, "whole", "random")
    sel = np.zeros(data.size, bool)
    sel[off: off + 4 * n] = True
    sel[off + 3: off + 4 * n: 4] = False
    assert _same_sums(got[sel] - np.float32(0.5), host[sel])
    assert np.all(got[off + 3: off + 4 * n: 4] == 0.5) and np.all(got[off + 4 * n:] == FILL)   # padding and tail: as they were
    assert np.array_equal(d_data.download(), data)


def test_registration_refusals_change_nothing():
    sc = G.scene_a()
    n = len(sc.lights)
    gpu = _gpu(sc, 1)
    L = gpu.L
    import ctypes as C
    off, size = C.c_uint64(123), C.c_uint64(456)

    def put(first, count, o=off, s=size):
        return L.hpt_put_diff_lights(gpu.h, first, count, None if o is None else C.byref(o), None if s is None else C.byref(s))

    for what, call, message in (("count 0", lambda: put(0, 0), "count is 0"), ("past the lights", lambda: put(2, n - 1), "reach past"),
                                ("past the lights", lambda: put(n, 1), "reach past"), ("null offset", lambda: put(0, n, None, size), "null out-pointer"),
                                ("null size", lambda: put(0, n, off, None), "null out-pointer")):
        assert call() == HPT_ERR_ARG, what
        assert message in L.hpt_last_error(gpu.h).decode(), (what, L.hpt_last_error(gpu.h).decode())
    assert (off.value, size.value) == (123, 456)
    assert L.hpt_put_diff_lights(None, 0, n, C.byref(off), C.byref(size)) == HPT_ERR_ARG
    # a misaligned offset: a one-channel texture of three floats first
    assert tuple(gpu.PutDiffTex2D(G.BOX_TEX, 3, 1, 1)) == (0, 3)
    assert put(0, n) == HPT_ERR_ARG and "multiple of 4" in L.hpt_last_error(gpu.h).decode()
    assert tuple(gpu.PutDiffTex2D(G.BOX_TEX, 1, 1, 1)) == (3, 1)                      # nothing was appended by the refused calls
    assert tuple(gpu.PutDiffLights(1, 2)) == (4, 8)
    assert put(3, 1) == HPT_ERR_ARG and "already registered" in L.hpt_last_error(gpu.h).decode()
    assert gpu.grad_size == 12
    assert L.hpt_reset_diff_tex(gpu.h) == 0
    assert tuple(gpu.PutDiffLights(0, n)) == (0, 4 * n)                               # the reset cleared textures and lights


def test_block_local_request_is_refused_and_writes_nothing():
    from hydracore3_amd.api import HydraHipError
    sc = G.scene_a()
    n = len(sc.lights)
    gpu = _gpu(sc, 3)
    data, off = _data(n, G.gains(n))
    frame, grad, gens = np.full((gpu.H, gpu.W, 4), FILL, np.float32), np.full(data.size, FILL, np.float32), gpu.random_gens()
    gpu.PathTraceVJP(gpu.N, 4, np.zeros_like(frame), 1, G.adjoint(), np.zeros(4, np.float32), np.zeros(4, np.float32))   # unregistered: served as before
    gpu.set_random_gens(gens)
    gpu.PutDiffLights(0, n)
    ref = np.zeros_like(frame)
    for fn, args in ((gpu.PathTraceVJP, (gpu.N, 4, frame, 1, G.adjoint(), data, grad)), (gpu.PathTraceDR, (gpu.N, 4, frame, 1, ref, data, grad))):
        with pytest.raises(HydraHipError, match=f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: the block-local schedule"):
            fn(*args)
    assert np.all(frame == FILL) and np.all(grad == FILL) and np.array_equal(gpu.random_gens(), gens)
    d = {k: gpu.dev_array(v) for k, v in (("frame", frame), ("adj", G.adjoint()), ("data", data), ("grad", grad))}
    with pytest.raises(HydraHipError, match="block-local"):
        gpu.PathTraceVJP_dev(d["frame"], 1, d["adj"], d["data"], d["grad"])
    assert np.all(d["frame"].download() == FILL) and np.all(d["grad"].download() == FILL) and np.array_equal(gpu.random_gens(), gens)
    # the automatic choice does not pick it with lights registered, whatever the scene's tree
    gpu.set_schedule(0)
    gpu.PathTraceVJP(gpu.N, 4, np.zeros_like(frame), 1, G.adjoint(), data, grad)
    assert gpu.last_schedule()[0] in (1, 2)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_registration_survives_update_lights_and_is_cleared_by_reset(schedule):
    sc = G.scene_a()
    n, spp, w = len(sc.lights), 4, WINDOWS["whole"]
    g = G.gains(n)
    gpu = _gpu(sc, schedule)
    data, off = _data(n, g)
    gpu.PutDiffLights(0, n)
    start = gpu.random_gens()
    gpu.Update_m_lights(0, np.array(sc.lights))
    frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
    gpu.PathTraceVJP(gpu.N, 4, frame, spp, G.adjoint(), data, grad)
    want_frame, want_grad, _, _, _ = light_run("A", schedule, spp, "whole", "random")
    assert np.array_equal(frame, want_frame) and _same_sums(grad[off: off + 4 * n], want_grad[off: off + 4 * n])
    # RayTraceDR ignores the registration
    rt, rt_grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
    gpu.RayTraceDR(gpu.N, 4, rt, 1, np.zeros((gpu.H, gpu.W, 4), np.float32), data, rt_grad)
    assert np.all(rt_grad == 0.0)
    assert gpu.L.hpt_reset_diff_tex(gpu.h) == 0
    gpu.grad_size = 0
    gpu.set_random_gens(start)
    frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
    gpu.PathTraceVJP(gpu.N, 4, frame, spp, G.adjoint(), data, grad)
    plain, _ = _render(_gpu(sc, schedule), spp, w)
    assert np.array_equal(frame, plain) and np.all(grad == 0.0)                        # the gains are no longer read, nothing is differentiated


# ---- 9. torch -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def torch_results():
    """The PyTorch op's checks run in ONE child process (light_grad_torch_child.py), as test_vjp_gpu.torch_results' do."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "light_grad_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_torch_backward_fills_the_gain_slice(schedule):
    """torch_dr.render(...).backward() leaves case 2's values in the gain slice of params.grad."""
    got = np.asarray(torch_results()[f"backward[{schedule}]"], np.float32)
    n = len(G.scene_a().lights)
    grad = np.zeros(4 * n + PAD, np.float32)
    grad[:4 * n] = got
    _check_lights("A", schedule, 4, "whole", grad, 0, what="torch: ")
    assert np.all(got[3::4] == 0.0)


def test_torch_adam_on_the_gains_lowers_the_loss():
    """Thirty Adam steps on the gains alone, towards a frame rendered with other gains, end with a lower loss than they began with."""
    assert torch_results()["adam"] == "ok"

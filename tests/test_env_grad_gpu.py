"""Environment maps in the differentiable integrators (hpt_set_option "dr_environment") on the GPU: off by default and the
refusals, the forward frame against the oracle's forward integrator, scenes without a map untouched, the two schedules against each other,
the texel gradient against basis frames under the light-gradient bound, occlusion, the base-colour gradient under env light, PathTraceDR's
own loss, textures and the map together, the device form and the PyTorch op. Scenes, maps and adjoints are env_grad_cases.py's; every case
under the megakernel and the wavefront schedule, 32 x 32 pixels, fixed seeds.

Worst observed |error| / bound of the texel gradient: see profiles/env_grad.md."""
import functools

import numpy as np
import pytest

import env_grad_cases as E
from env_grad_cases import SCHEDULES, WINDOWS
from light_grad_cases import expected_and_bound, pixel_mask

pytestmark = pytest.mark.gpu

HPT_ERR_ARG, HPT_ERR_UNSUPPORTED = 1, 4
FILL = -3.0
PAD = 8                                          # floats of a_data / a_dataGrad behind the registered ranges
SCENES = {"P": E.plane_scene, "B": E.box_scene}
DEPTH = {"P": 1, "B": E.BOX_DEPTH}


def _gpu(sc, schedule, option=True, params=None):
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(sc, params)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    if option:
        gpu.set_option("dr_environment", 1)
    return gpu


def _render(gpu, spp, window, data):
    """The frame of PathTraceVJP with a null adjoint; (frame, generators after)."""
    frame = np.zeros((gpu.H, gpu.W, 4), np.float32)
    gpu.PathTraceVJP(window[1], 4, frame, spp, None, data, None, tid_begin=window[0])
    return frame, gpu.random_gens()


def _data(*parts):
    return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts] + [np.full(PAD, FILL, np.float32)]).astype(np.float32)


def _same_sums(a, b):
    """The same sums in another order (test_vjp_gpu._same_sums)."""
    return np.allclose(a, b, rtol=1e-4, atol=1e-7 * np.abs(b).max())


@functools.lru_cache(maxsize=None)
def env_run(scene, schedule, spp, window, base, size="4x2", sample=True):
    """One host-form PathTraceVJP with the map alone registered, at the random map or at the black one:
    (frame, gradient, generators after, the integrator's packed pixels)."""
    gpu = _gpu(SCENES[scene](size, sample), schedule)
    w, h = E.MAPS[size]
    assert tuple(gpu.PutDiffTex2D(E.ENV_TEX, w, h, 4)) == (0, w * h * 4)
    data = _data(E.env_image(size) if base == "random" else E.basis_image(size))
    frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
    win = WINDOWS[window]
    gpu.PathTraceVJP(win[1], 4, frame, spp, E.adjoint(), data, grad, tid_begin=win[0])
    assert gpu.last_schedule()[0] == schedule
    return frame, grad, gpu.random_gens(), gpu.packed_xy()


@functools.lru_cache(maxsize=None)
def basis_frames(scene, schedule, spp, window, size="4x2", sample=True):
    """{(k, c): F_k, None: F_0} from the same kernels with a null adjoint, the map registered and the generators put back before every frame."""
    gpu = _gpu(SCENES[scene](size, sample), schedule)
    w, h = E.MAPS[size]
    gpu.PutDiffTex2D(E.ENV_TEX, w, h, 4)
    start, out = gpu.random_gens(), {}
    for key in [None] + [(k, c) for k in range(w * h) for c in range(3)]:
        gpu.set_random_gens(start)
        out[key] = _render(gpu, spp, WINDOWS[window], _data(E.basis_image(size) if key is None else E.basis_image(size, *key)))[0]
        assert gpu.last_schedule()[0] == schedule
    return out


# ---- 1. off by default; the refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_off_by_default_and_the_refusals_write_nothing(schedule):
    from hydracore3_amd.api import HydraHipError
    from hydracore3_amd import scene as S
    data = _data(E.env_image("4x2"))

    def refused(gpu, match, data=data):
        frame, grad, gens = np.full((gpu.H, gpu.W, 4), FILL, np.float32), np.full(data.size, FILL, np.float32), gpu.random_gens()
        ref = np.zeros_like(frame)
        for fn, args in ((gpu.PathTraceVJP, (gpu.N, 4, frame, 1, E.adjoint(), data, grad)), (gpu.PathTraceDR, (gpu.N, 4, frame, 1, ref, data, grad))):
            with pytest.raises(HydraHipError, match=match):
                fn(*args)
        assert np.all(frame == FILL) and np.all(grad == FILL) and np.array_equal(gpu.random_gens(), gens)
        d = {k: gpu.dev_array(v) for k, v in (("frame", frame), ("adj", E.adjoint()), ("data", data), ("grad", grad))}
        with pytest.raises(HydraHipError, match=match):
            gpu.PathTraceVJP_dev(d["frame"], 1, d["adj"], d["data"], d["grad"])
        assert np.all(d["frame"].download() == FILL) and np.all(d["grad"].download() == FILL) and np.array_equal(gpu.random_gens(), gens)

    for sample in (True, False):
        refused(_gpu(E.box_scene("4x2", sample), schedule, option=False), f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: environment maps")
    gpu = _gpu(E.box_scene(), schedule)                                    # with the option the same call is served
    gpu.PathTraceVJP(gpu.N, 4, np.zeros((gpu.H, gpu.W, 4), np.float32), 1, E.adjoint(), data, np.zeros(data.size, np.float32))
    assert gpu.last_schedule()[0] == schedule
    # a camera back plate
    sc = E.box_scene()
    sc.env_cam_back_id = E.TEX
    refused(_gpu(sc, schedule), f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: a camera back plate")
    # lights registered on the same context
    gpu = _gpu(E.box_scene(), schedule)
    gpu.PutDiffLights(0, 1)
    refused(gpu, f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: the light-gradient variant has no environment-map form")
    # the block-local schedule; the automatic choice avoids it
    gpu = _gpu(E.box_scene(), 3)
    refused(gpu, f"error {HPT_ERR_UNSUPPORTED}: PathTraceDR: the block-local schedule has no environment-map variant")
    gpu.set_schedule(0)
    gpu.PathTraceVJP(gpu.N, 4, np.zeros((gpu.H, gpu.W, 4), np.float32), 1, E.adjoint(), data, np.zeros(data.size, np.float32))
    assert gpu.last_schedule()[0] in (1, 2)
    # a one-channel registration of the map
    gpu = _gpu(E.box_scene(), schedule)
    import ctypes as C
    off, size = C.c_uint64(123), C.c_uint64(456)
    assert gpu.L.hpt_put_diff_tex2d(gpu.h, E.ENV_TEX, 4, 2, 1, C.byref(off), C.byref(size)) == HPT_ERR_ARG
    assert "environment map takes 4 channels" in gpu.L.hpt_last_error(gpu.h).decode() and (off.value, size.value) == (123, 456)
    assert tuple(gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 4)) == (0, 32)          # nothing was appended by the refused call
    # ... also when it was made before the option was set
    gpu = _gpu(E.box_scene(), schedule, option=False)
    assert tuple(gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 1)) == (0, 8)
    gpu.set_option("dr_environment", 1)
    refused(gpu, f"error {HPT_ERR_ARG}: PathTraceDR: the environment map is registered with one channel")
    # ... and when the env light reads another texture than m_envTexId along the shadow ray, and that one has one channel
    sc = E.box_scene()
    gpu = _gpu(sc, schedule)
    assert tuple(gpu.PutDiffTex2D(E.TEX, E.BOX_TEX_W, E.BOX_TEX_H, 1)) == (0, E.BOX_TEX_W * E.BOX_TEX_H)
    lights = np.array(sc.lights).copy()
    lights[sc.env_light_id]["texId"] = E.TEX
    gpu.Update_m_lights(0, lights)
    refused(gpu, f"error {HPT_ERR_ARG}: PathTraceDR: the environment map is registered with one channel", _data(np.zeros(E.BOX_TEX_W * E.BOX_TEX_H)))


# ---- 2. the forward pinned independently ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mis_sampled", "mis_unsampled", "shadow_sampled"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_forward_is_the_oracles_forward_integrator(schedule, mode):
    """On (P) every path is camera -> plane -> sky, so PathTraceDR's frame at trace depth 1 is the forward integrator's at depth 2
    (camRespoceRGB 1, exposure 1, one sample per call): the device's null-adjoint frame against the oracle's PathTraceBlock."""
    from conftest import assert_pixel_parity
    from hydracore3_amd import scene as S
    from oracle.orc import OracleIntegrator
    integ = S.INTEGRATOR_SHADOW_PT if mode == "shadow_sampled" else S.INTEGRATOR_MIS_PT
    sc = E.plane_scene("4x2", mode != "mis_unsampled")
    sc.cam_respoce_rgb, sc.exposure_mult = (1.0, 1.0, 1.0, 1.0), 1.0
    cpu = OracleIntegrator(sc, sc.params(integ, 0, 2))
    want = cpu.render(1)
    gpu = _gpu(sc, schedule, params=sc.params(integ, 0, 1))
    got, _ = _render(gpu, 1, WINDOWS["whole"], np.zeros(4, np.float32))
    assert gpu.last_schedule()[0] == schedule
    assert want[..., :3].max() > 0.0
    assert_pixel_parity(got, want, 1, gpu, cpu, what=f"schedule {schedule}, {mode}: ")


# ---- 3. a scene without a map is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["one wave", "whole"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_a_scene_without_a_map_runs_the_old_kernels(schedule, window):
    """Option off, off again, on: frame and generators bit for bit. The gradient is a sum of float atomics. With 64 threads - one wave, so one
    order of the atomics - it is bit for bit too. With the whole frame the waves' atomics interleave as they arrive and two runs of one kernel
    differ in the last bits (the count is printed; profiles/env_grad.md has one run's): there the gradient is held as the same sums."""
    res = []
    tex = E._albedo(E.BOX_TEX_W, E.BOX_TEX_H, E.SEED + 9)
    win = (0, 64) if window == "one wave" else WINDOWS["whole"]
    for option in (False, False, True):
        gpu = _gpu(E.box_scene(with_env=False), schedule, option)
        gpu.PutDiffTex2D(E.TEX, E.BOX_TEX_W, E.BOX_TEX_H, 4)
        data = _data(tex)
        frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
        gpu.PathTraceVJP(win[1], 4, frame, 2, E.adjoint(), data, grad, tid_begin=win[0])
        assert gpu.last_schedule()[0] == schedule
        res.append((frame, gpu.random_gens(), grad))
    off, again, on = res
    assert np.count_nonzero(off[2][:tex.size]) > 0
    for k in (0, 1):                                                        # frame and generators: bit for bit
        assert np.array_equal(off[k].view(np.uint32), on[k].view(np.uint32)) and np.array_equal(off[k].view(np.uint32), again[k].view(np.uint32))
    repeats = off[2].view(np.uint32) == again[2].view(np.uint32)
    print(f"schedule {schedule}, {window}: {int(np.sum(~repeats))} of {repeats.size} gradient floats differ between two runs with the option off, "
          f"{int(np.sum(off[2].view(np.uint32) != on[2].view(np.uint32)))} between off and on")
    if window == "one wave":
        assert np.all(repeats) and np.array_equal(off[2].view(np.uint32), on[2].view(np.uint32))
    else:
        assert _same_sums(on[2], off[2]) and np.array_equal(on[2] == 0.0, off[2] == 0.0)


# ---- 4. the schedules agree ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["P", "B"])
def test_schedules_agree(scene):
    mega, wave = (env_run(scene, s, 4, "whole", "random") for s in SCHEDULES)
    assert np.array_equal(mega[0].view(np.uint32), wave[0].view(np.uint32)) and np.array_equal(mega[2], wave[2])
    assert np.count_nonzero(mega[1][:32]) > 0 and _same_sums(mega[1][:32], wave[1][:32])


# ---- 5. the texel gradient against basis frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["random", "black"])
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("scene", ["P", "B"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_texel_gradient_against_basis_frames(schedule, scene, spp, window, base):
    """|grad[k, c] - sum_p a (F_k - F_0)| <= 2 (n + 8) 2^-24 sum_p |a| (F_k + F_0), n = tids * spp * (depth + 1) * 4 (four taps), for every
    texel and channel of the 4 x 2 map, at a random map and at the black one: the derivative is per unit texel and never divides by one."""
    frame, grad, _, xy = env_run(scene, schedule, spp, window, base)
    frames = basis_frames(scene, schedule, spp, window)
    win = WINDOWS[window]
    mask = pixel_mask(xy, win[0], win[1], (E.HEIGHT, E.WIDTH))
    n = win[1] * spp * (DEPTH[scene] + 1) * 4
    a, worst = E.adjoint(), 0.0
    if base == "black":
        assert np.array_equal(frame, frames[None])
    for k in range(8):
        want, bound, got = np.zeros(3), np.zeros(3), grad[4 * k: 4 * k + 3].astype(np.float64)
        for c in range(3):
            w3, b3 = expected_and_bound(a, frames[(k, c)], frames[None], mask, n)
            want[c], bound[c] = w3[c], b3[c]
        ratio = np.abs(got - want) / bound
        print(f"scene {scene}, schedule {schedule}, spp {spp}, {window}, {base} map: texel {k} grad {got} expected {want} |error| / bound {ratio}")
        assert np.all(bound > 0.0) and np.all(np.abs(want) > 0.0), f"texel {k}: the check is vacuous"
        assert np.all(np.abs(got - want) <= bound), f"texel {k}: gradient {got}, expected {want}, bound {bound}"
        worst = max(worst, float(ratio.max()))
    print(f"scene {scene}, schedule {schedule}, spp {spp}, {window}, {base} map: worst |error| / bound = {worst:.3e}")
    assert np.all(grad[3:32:4] == 0.0)                                    # alpha is never read by the environment
    assert np.all(grad[32:] == 0.0)                                       # the padding floats (the host form zeroes all of a_gradSize)


# ---- 6. occlusion --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_a_texel_below_every_horizon_has_no_gradient(schedule):
    _, grad, _, _ = env_run("B", schedule, 4, "whole", "random", "8x4")
    assert np.count_nonzero(grad[:128]) > 0
    for k in E.below_horizon_texels("8x4"):
        assert np.all(grad[4 * k: 4 * k + 4] == 0.0), (k, grad[4 * k: 4 * k + 4])


# ---- 7. the base-colour gradient under env light --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [True, False])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_base_colour_gradient_under_env_light(schedule, sample):
    """(P) at depth 1 is affine in each texel of the plane's albedo (the plane is visited once): the texture gradient against the central
    difference of the device's own frames at h = 2^-3, within 2^-24 (n + 8) sum |a| (F+ + F-) / (2 h)."""
    spp, h, nt = 2, 0.125, E.PLANE_TEX_W * E.PLANE_TEX_H * 4
    gpu = _gpu(E.plane_scene("4x2", sample), schedule)
    assert tuple(gpu.PutDiffTex2D(E.TEX, E.PLANE_TEX_W, E.PLANE_TEX_H, 4)) == (0, nt)
    tex = E._albedo(E.PLANE_TEX_W, E.PLANE_TEX_H, E.SEED + 5).reshape(-1)
    start, a = gpu.random_gens(), E.adjoint()
    frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(nt + PAD, FILL, np.float32)
    gpu.PathTraceVJP(gpu.N, 4, frame, spp, a, _data(tex), grad)
    n = E.N * spp * 2 * 4
    a64, worst = a[..., :3].astype(np.float64), 0.0
    for i in [j for j in range(nt) if j % 4 != 3]:
        f = []
        for sign in (1.0, -1.0):
            t = tex.copy()
            t[i] += np.float32(sign * h)
            gpu.set_random_gens(start)
            f.append(_render(gpu, spp, WINDOWS["whole"], _data(t))[0][..., :3].astype(np.float64))
        want = float((a64 * (f[0] - f[1])).sum() / (2 * h))
        bound = 2.0 ** -24 * (n + 8) * float((np.abs(a64) * (f[0] + f[1])).sum()) / (2 * h)
        assert bound > 0.0 and abs(want) > 0.0 and abs(float(grad[i]) - want) <= bound, (i, float(grad[i]), want, bound)
        worst = max(worst, abs(float(grad[i]) - want) / bound)
    print(f"schedule {schedule}, sampling {sample}: base-colour gradient, worst |error| / bound = {worst:.3e}")
    assert np.all(grad[3:nt:4] == 0.0)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_skip_nonfinite_drops_the_env_terms_of_a_nonfinite_seed(schedule):
    """dr_skip_nonfinite treats the env terms as the texture terms: a term whose product with the seed is not finite is dropped. With an
    infinite adjoint at some pixels the map's gradient equals the one with those adjoints at 0 (the same sums); without the option it is not finite."""
    a = E.adjoint()
    bad = np.zeros((E.HEIGHT, E.WIDTH), bool)
    bad[5:9, 7:20] = True
    a_inf, a_zero = a.copy(), a.copy()
    a_inf[bad, :3], a_zero[bad, :3] = np.inf, 0.0
    data, grads = _data(E.env_image("4x2")), {}
    for key, adj, skip in (("inf, skipped", a_inf, 1), ("zeroed", a_zero, 1), ("inf", a_inf, 0)):
        gpu = _gpu(E.box_scene(), schedule)
        gpu.set_option("dr_skip_nonfinite", skip)
        gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 4)
        grad = np.full(data.size, FILL, np.float32)
        gpu.PathTraceVJP(gpu.N, 4, np.zeros((gpu.H, gpu.W, 4), np.float32), 4, adj, data, grad)
        grads[key] = grad[:32]
    assert not np.all(np.isfinite(grads["inf"]))
    assert np.all(np.isfinite(grads["inf, skipped"])) and np.count_nonzero(grads["zeroed"]) == 24
    assert _same_sums(grads["inf, skipped"], grads["zeroed"])


# ---- 8. PathTraceDR's own loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_path_trace_dr_equals_the_vjp_of_its_own_adjoint(schedule):
    """At one sample per pixel PathTraceDR's seed 2 (colour - ref) can be formed from its frame (a_refImg is bottom-up)."""
    data = _data(E.env_image("4x2"))
    ref = np.random.default_rng(E.SEED + 3).uniform(0.0, 0.5, (E.HEIGHT, E.WIDTH, 4)).astype(np.float32)
    grads = []
    for adj in (None, "from the frame"):
        gpu = _gpu(E.box_scene(), schedule)
        gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 4)
        frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
        if adj is None:
            gpu.PathTraceDR(gpu.N, 4, frame, 1, ref, data, grad)
            colour = frame
        else:
            gpu.PathTraceVJP(gpu.N, 4, frame, 1, (np.float32(2.0) * (colour - ref[::-1])).astype(np.float32), data, grad)
            assert np.array_equal(frame, colour)
        assert gpu.last_schedule()[0] == schedule
        grads.append(grad[:32])
    print(f"schedule {schedule}: max |vjp - dr| / max |dr| = {np.abs(grads[1] - grads[0]).max() / np.abs(grads[0]).max():.3e}")
    assert np.count_nonzero(grads[0]) == 24 and _same_sums(grads[1], grads[0])


# ---- 9. textures and the map together --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["texture first", "map first"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_textures_and_the_map_together(schedule, order):
    spp, nt, ne = 4, E.BOX_TEX_W * E.BOX_TEX_H * 4, 32
    tex, env = E._albedo(E.BOX_TEX_W, E.BOX_TEX_H, E.SEED + 9), E.env_image("4x2")
    reg = [(E.TEX, E.BOX_TEX_W, E.BOX_TEX_H, tex, nt), (E.ENV_TEX, 4, 2, env, ne)]

    def run(items):
        gpu = _gpu(E.box_scene(), schedule)
        offs = [gpu.PutDiffTex2D(t, w, h, 4)[0] for t, w, h, _, _ in items]
        data = _data(*[v for _, _, _, v, _ in items])
        frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
        gpu.PathTraceVJP(gpu.N, 4, frame, spp, E.adjoint(), data, grad)
        assert gpu.last_schedule()[0] == schedule
        return frame, [grad[o: o + it[4]] for o, it in zip(offs, items)], grad[sum(it[4] for it in items):]

    both = run(reg if order == "texture first" else reg[::-1])
    slices = both[1] if order == "texture first" else both[1][::-1]
    assert np.all(both[2] == 0.0)
    # each slice against its single registration; the other texture then comes from the scene, so render that run with the same values bound
    for i, item in enumerate(reg):
        sc = E.box_scene()
        if i == 0:
            E.with_map(sc, env)                                            # (the fixture's own map: the values a_data holds)
        else:
            from hydracore3_amd import scene as S
            sc.textures[E.TEX] = S.Texture(tex, S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_WRAP, S.FILTER_LINEAR)
        gpu = _gpu(sc, schedule)
        gpu.PutDiffTex2D(*item[:3], 4)
        data = _data(item[3])
        frame, grad = np.zeros((gpu.H, gpu.W, 4), np.float32), np.full(data.size, FILL, np.float32)
        gpu.PathTraceVJP(gpu.N, 4, frame, spp, E.adjoint(), data, grad)
        assert np.allclose(frame, both[0], rtol=1e-4, atol=1e-6)             # (a registered texture is fetched by texFetchAD, the scene's by the sampler)
        assert np.count_nonzero(grad[:item[4]]) > 0 and _same_sums(slices[i], grad[:item[4]])


# ---- 10. device form, torch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_device_form_accumulates_and_touches_nothing_else(schedule):
    spp = 4
    gpu = _gpu(E.box_scene(), schedule)
    gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 4)
    data = _data(E.env_image("4x2"))
    before = np.full(data.size, FILL, np.float32)
    before[:32] = 0.5
    d_frame, d_adj, d_data, d_grad = (gpu.dev_array(x) for x in (np.zeros((gpu.H, gpu.W, 4), np.float32), E.adjoint(), data, before))
    gpu.PathTraceVJP_dev(d_frame, spp, d_adj, d_data, d_grad)
    got = d_grad.download()
    _, host, _, _ = env_run("B", schedule, spp, "whole", "random")
    rgb = np.arange(32) % 4 != 3
    assert _same_sums(got[:32][rgb] - np.float32(0.5), host[:32][rgb])
    assert np.all(got[:32][~rgb] == 0.5) and np.all(got[32:] == FILL)      # alpha and everything past a_gradSize: as they were
    assert np.array_equal(d_data.download(), data)


@functools.lru_cache(maxsize=None)
def torch_results():
    """The PyTorch op's checks run in ONE child process (env_grad_torch_child.py), as test_vjp_gpu.torch_results' do."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "env_grad_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_torch_backward_fills_the_env_slice(schedule):
    """torch_dr.render(...).backward() leaves the host form's values in the map's slice of params.grad."""
    got = np.asarray(torch_results()[f"backward[{schedule}]"], np.float32)
    _, host, _, _ = env_run("B", schedule, 4, "whole", "random")
    assert got.size == 32 and np.count_nonzero(got) == 24 and _same_sums(got, host[:32])


def test_torch_adam_on_the_map_lowers_the_loss():
    """Ten Adam steps on the map alone, from a grey start towards a frame rendered with a coloured map, end with a lower L2 loss."""
    assert torch_results()["adam"] == "ok"

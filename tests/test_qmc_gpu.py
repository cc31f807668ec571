"""PathTraceBlockQMC on the GPU (hpt_qmc.hip): the sampler on the device, exact occupancy, exact per-sample colours against the CPU oracle,
the atomic frame against its own records, the generator contract, arguments.

What is compared with what:
 * pixel indices: tests/qmc_reference.py (numpy, table from the recorded fixture);
 * per-sample colours: the QMC camera rays formed in numpy float32 (qmc_reference.camera_rays) and fed to the oracle's
   PathTraceFromInputRaysBlock, on scenes where a sample's colour depends on its primary ray only (emitters, no lights, traceDepth 1);
 * the frame: the float64 scatter-sum of the same call's records, every pixel held to n * 2^-24 * sum|x_i| (n float32 additions in any order,
   each rounding a partial sum no larger than sum|x_i| by at most half an ulp = 2^-24 relative).
"""
import ctypes as C

import numpy as np
import pytest

import qmc_reference as Q
from conftest import scene_path
from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.scene import load_hydra_xml

HPT_ERR_ARG, HPT_ERR_STATE, HPT_ERR_UNSUPPORTED = 1, 3, 4
ENV = (0.5, 0.25, 2.0)                                                    # small powers of two: integer multiples add exactly in any order


def _sky_scene(w, h, dof=False, motion=False):
    """A constant environment colour and no geometry in view: the camera stands above the plane of synth.furnace_plane and looks straight up."""
    sc = synth.furnace_plane(w, h, env=ENV)
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 5.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 1.0)
    if dof:
        sc.cam_lens_radius = 0.05
    if motion:
        sc.inst_motion[0] = np.asarray(sc.inst_matrices[0], np.float64).reshape(4, 4) @ S.translate(0.25, 0.0, 0.0)
    return sc


def _checker(n=16):
    t = np.zeros((n, n, 4), np.float32)
    yy, xx = np.mgrid[0:n, 0:n]
    t[..., 0] = 0.25 + 0.75 * ((xx + yy) & 1)
    t[..., 1] = 0.125 + xx / (2.0 * n)
    t[..., 2] = 1.0 - yy / (2.0 * n)
    t[..., 3] = 1.0
    return t


def _emissive_cornell(w=64, h=64, dof=False, motion=False, textured=True):
    """test_035's geometry with every material turned into an emitter (every other one textured, linear float texels), no lights, traceDepth 1:
    a sample's colour is the emission its primary ray meets, or the environment colour."""
    sc = load_hydra_xml(scene_path("test_035"), w, h)
    tex = sc.add_texture(S.Texture(_checker(), S.TEX_RGBA32F, False))
    cols = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.7, 0.7, 0.6), (0.3, 0.4, 1.2), (1.5, 1.25, 0.5)]
    sc.materials = [S.material_emissive(cols[i % len(cols)], mult=1.0 + 0.25 * (i % 3), tex_id=(tex if textured and i % 2 == 0 else 0)) for i in range(len(sc.materials))]
    sc.lights = []
    sc.remap_inst = [(int(r[0]), -1) for r in np.asarray(sc.remap_inst).reshape(-1, 2)]
    sc.trace_depth = 1
    sc.env_color = (0.125, 0.25, 0.5, 0.0)
    sc.exposure_mult = 1.5
    sc.cam_respoce_rgb = (0.9, 1.1, 0.8, 1.0)
    if dof:
        sc.cam_lens_radius = 0.08
    if motion:
        last = len(sc.inst_matrices) - 1
        sc.inst_motion[last] = np.asarray(sc.inst_matrices[last], np.float64).reshape(4, 4) @ S.translate(0.4, 0.0, 0.1)
    return sc


def _table():
    return Q.load_fixture()[0]


# ---- 1. the sampler on the device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dof,motion", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("w,h,spp", [(64, 64, 4), (48, 20, 3)])
def test_sample_pixels_equal_the_restatement(dof, motion, w, h, spp):
    """All feature combinations that are not refused (the four without m_spectral_mode), a power-of-two and another window."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_sky_scene(w, h, dof, motion))
    _, col, pix = g.render_qmc(spp, frame=False, records=True)
    _, _, want = Q.sample_pixels(_table(), w * h * spp, w, h)
    assert pix.shape == want.shape and np.array_equal(pix, want), np.flatnonzero(pix != want)[:8]
    assert np.all(col[:, :3] == np.asarray(ENV, np.float32)) and np.all(col[:, 3] == 0.0)


# ---- 2. exact occupancy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp,channels", [(64, 64, 4, 4), (128, 64, 8, 3), (32, 32, 16, 4)])
def test_constant_scene_gives_spp_times_the_colour_bit_for_bit(w, h, spp, channels):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_sky_scene(w, h))
    img = np.zeros((h, w, channels), np.float32)
    g.PathTraceBlockQMC(w * h, channels, img, spp)
    want = np.zeros((h, w, channels), np.float32)
    want[..., :3] = np.asarray(ENV, np.float32) * np.float32(spp)
    assert img.tobytes() == want.tobytes(), np.argwhere(img != want)[:8]
    t = g.GetExecutionTime("PathTraceBlockQMC")
    assert t[0] > 0.0 and all(v >= 0.0 for v in t[1:3])
    # the call adds to what the frame held
    g.PathTraceBlockQMC(w * h, channels, img, spp)
    assert img.tobytes() == (want * np.float32(2)).tobytes()


@pytest.mark.gpu
def test_one_channel_frame_gets_the_luma():
    from hydracore3_amd.api import HipIntegrator
    w, h, spp = 32, 32, 4
    g = HipIntegrator(_sky_scene(w, h))
    img, col, pix = g.render_qmc(spp, channels=1, records=True)
    e = np.asarray(ENV, np.float32)
    mono = np.float32(np.float32(np.float32(np.float32(0.2126) * e[0]) + np.float32(np.float32(0.7152) * e[1])) + np.float32(np.float32(0.0722) * e[2]))
    assert np.all(col[:, 0] == mono) and np.all(col[:, 1:] == 0.0)
    ref = np.zeros(w * h, np.float64)
    np.add.at(ref, pix, col[:, 0].astype(np.float64))
    assert np.all(np.abs(img.reshape(-1) - ref) <= spp * 2.0 ** -24 * ref)


# ---- 3. exact per-sample colours against the CPU oracle -----------------------------------------------------------------------------------------
def _oracle_colours(sc, params, dof, motion_dim, samples):
    """The QMC camera rays of samples 0 .. samples - 1 through the oracle's PathTraceFromInputRaysBlock (4 channels, raw accumColor), then
    camRespoceRGB and exposure in float32 as IntegratorQMC::kernel_ContributeToImage applies them."""
    from oracle.orc import OracleIntegrator
    cpu = OracleIntegrator(sc, params)
    pos, dr = Q.camera_rays(_table(), params, samples, dof, motion_dim)
    raw = np.zeros((samples, 4), np.float32)
    for a in range(0, samples, cpu.N):                                   # the oracle holds one generator per pixel: batches of at most N rays
        b = min(samples, a + cpu.N)
        out = np.zeros((b - a, 4), np.float32)
        cpu.path_trace_from_input_rays_block(np.ascontiguousarray(pos[a:b]), np.ascontiguousarray(dr[a:b]), out, 1, channels=4)
        raw[a:b] = out
    cam = np.asarray(list(params.camRespoceRGB), np.float32)
    c = (raw[:, :3] * cam[:3]).astype(np.float32)
    return (np.float32(params.exposureMult) * c).astype(np.float32), raw


@pytest.mark.gpu
@pytest.mark.parametrize("name,dof,motion,layout", [("emissive textured walls", False, False, 0), ("the same, two-level", False, False, 1),
                                                    ("thin-lens camera", True, False, 0), ("moving instance", False, True, 0),
                                                    ("moving instance, single-level", False, True, 2)])
def test_per_sample_colours_equal_the_oracle(name, dof, motion, layout):
    """The thin-lens case runs on UNTEXTURED emitters. The lens point goes through sinf / cosf (MapSamplesToDisc), which no host routine is
    bound to reproduce bit for bit. Measured on the MI355X with TEXTURED walls (64 x 64 x 4 samples): against the restatement with numpy's
    float32 sin / cos 14 of 16384 samples differ from the oracle (at most 60 ulp of a colour component), against the one with correctly
    rounded sin / cos (qmc_reference: rounded=True) 20 differ (at most 76 ulp); 12 samples are in both sets, and there the two host variants
    give the same lens point - so neither host routine is the device's. The pinhole and moving-instance cases on the same textured walls
    have 0 of 16384. With a constant emission per wall the colour is piecewise constant in the ray, which the restatement CAN produce
    (0 of 16384 differ); the lens dimensions still decide which wall a sample near an edge sees. What this case cannot see is an error of
    an ulp or so in the device's lens arithmetic away from the edges."""
    from hydracore3_amd import api
    w, h, spp = 64, 64, 4
    sc = _emissive_cornell(w, h, dof, motion, textured=not dof)
    params = sc.params()
    g = api.HipIntegrator(sc, params, accel_layout=layout)
    _, col, pix = g.render_qmc(spp, frame=False, records=True)
    lay = api.qmc_layout(dof, False, motion)
    want, raw = _oracle_colours(sc, params, dof, lay["motion"] if motion else 0, w * h * spp)
    _, _, wpix = Q.sample_pixels(_table(), w * h * spp, w, h)
    assert np.array_equal(pix, wpix)
    hits = int(np.sum(np.any(raw[:, :3] != np.asarray(sc.env_color[:3], np.float32), axis=1)))
    assert hits > (w * h * spp) // 4, f"{name}: only {hits} samples see the emitters"
    diff = np.flatnonzero(np.any(col[:, :3].view(np.uint32) != want.view(np.uint32), axis=1))
    print(f"{name}: {w * h * spp} samples, {hits} on emitters, {len(np.unique(col[:, :3], axis=0))} distinct colours, {diff.size} differ")
    assert diff.size == 0, (name, diff[:8], col[diff[:4]], want[diff[:4]])
    assert np.all(col[:, 3] == 0.0)


# ---- 4. the atomic frame against its own records ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,w,h,spp", [("test_035", 64, 64, 16), ("test_228", 48, 32, 8)])
def test_frame_equals_the_scatter_sum_of_the_records(scene_name, w, h, spp):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(load_hydra_xml(scene_path(scene_name), w, h))
    img, col, pix = g.render_qmc(spp, channels=4, records=True)
    assert np.isfinite(col).all() and col[:, :3].max() > 0.0
    ref, mag = np.zeros((w * h, 3), np.float64), np.zeros((w * h, 3), np.float64)
    np.add.at(ref, pix, col[:, :3].astype(np.float64))
    np.add.at(mag, pix, np.abs(col[:, :3].astype(np.float64)))
    n = np.bincount(pix, minlength=w * h).astype(np.float64)[:, None]
    err = np.abs(img.reshape(-1, 4)[:, :3].astype(np.float64) - ref)
    bound = n * 2.0 ** -24 * mag
    print(f"{scene_name}: worst error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, samples per pixel {int(n.min())} .. {int(n.max())}")
    assert np.all(err <= bound), np.argwhere(err > bound)[:8]
    assert np.all(img[..., 3] == 0.0)


# ---- 5. the generator contract ------------------------------------------------------------------------------------------------------------------
def _rng_steps(gens, steps):
    """`steps` generator steps (rndFloat4_Pseudo and rndFloat1_Pseudo advance the state alike: include/crandom.h) on uint32 [n, 2] states."""
    sx, sy = gens[:, 0].astype(np.uint32).copy(), gens[:, 1].astype(np.uint32).copy()
    steps = np.broadcast_to(np.asarray(steps), sx.shape)
    with np.errstate(over="ignore"):
        for k in range(int(steps.max())):
            m = steps > k
            x = (sx * np.uint32(17) + sy * np.uint32(13123)).astype(np.uint32)
            sx = np.where(m, ((x << np.uint32(13)) ^ x).astype(np.uint32), sx)
            sy = np.where(m, (sy ^ (x << np.uint32(7))).astype(np.uint32), sy)
    return np.stack([sx, sy], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", [False, True])
def test_generators_advance_by_the_draws_of_their_samples(motion):
    """The constant-colour scene: the camera takes one float4 (the time comes from the motion dimension, without a pseudo draw), Contribute one
    float4; slot g runs samples g, g + N, ... in order. Fewer generators than pixels: the slots' chains have different lengths. A second call
    restarts the sample index, as the reference's does: two calls of p passes repeat the same samples on the generators as the first left them."""
    from hydracore3_amd.api import HipIntegrator
    w, h, spp = 32, 32, 3
    g = HipIntegrator(_sky_scene(w, h, motion=motion))
    n_gens = 1000                                                       # does not divide S = 3072: slots 0 .. 71 run 4 samples, the others 3
    g.InitRandomGens(n_gens)
    before = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, before.ctypes.data, n_gens))
    _, col, pix = g.render_qmc(spp, frame=False, records=True)
    after = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, after.ctypes.data, n_gens))
    S_ = w * h * spp
    per_slot = (S_ - np.arange(n_gens) + n_gens - 1) // n_gens
    assert per_slot.sum() == S_ and per_slot.min() == 3 and per_slot.max() == 4
    assert np.array_equal(after, _rng_steps(before, 2 * per_slot))
    _, col2, pix2 = g.render_qmc(spp, frame=False, records=True)
    after2 = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, after2.ctypes.data, n_gens))
    assert np.array_equal(pix2, pix) and np.array_equal(after2, _rng_steps(after, 2 * per_slot))


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_codes():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    sc = _sky_scene(32, 32)
    buf = np.zeros((32, 32, 4), np.float32)
    N = 32 * 32

    def err(g):
        return g.L.hpt_last_error(g.h).decode()

    g = HipIntegrator(sc)
    assert g.L.hpt_path_trace_qmc_block(None, N, 4, buf.ctypes.data, 1) == HPT_ERR_ARG
    assert g.L.hpt_path_trace_qmc_block_dev(None, N, 4, buf.ctypes.data, 1, None, None, None) == HPT_ERR_ARG
    assert g.L.hpt_path_trace_qmc_block(g.h, N, 4, None, 1) == HPT_ERR_ARG and "PathTraceBlockQMC" in err(g)
    assert g.L.hpt_path_trace_qmc_block_dev(g.h, N, 4, None, 1, None, None, None) == HPT_ERR_ARG and "no frame" in err(g)
    assert g.L.hpt_path_trace_qmc_block_dev(g.h, N, 4, None, 1, buf.ctypes.data, None, None) == HPT_ERR_ARG and "pair" in err(g)
    for channels in (5, 8, 2):
        assert g.L.hpt_path_trace_qmc_block(g.h, N, channels, buf.ctypes.data, 1) == HPT_ERR_UNSUPPORTED and "channels" in err(g)
    with pytest.raises(HydraHipError, match="channels"):
        g.PathTraceBlockQMC(N, 5, buf, 1)
    assert not buf.any()
    assert g.L.hpt_path_trace_qmc_block(g.h, N, 4, buf.ctypes.data, 0) == 0 and not buf.any()      # no samples: nothing to do

    fresh = HipIntegrator()
    assert fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1) == HPT_ERR_STATE and "CommitDeviceData" in err(fresh)
    fresh.scene, fresh._desc = sc, sc.desc()
    fresh.CommitDeviceData()
    fresh.UpdateMembersPlainData(sc.params())
    assert fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1) == HPT_ERR_STATE and "PackXYBlock" in err(fresh)
    fresh.PackXYBlock(32, 32)
    assert fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1) == HPT_ERR_ARG and "InitRandomGens" in err(fresh)
    fresh.InitRandomGens(N)
    assert fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1) == 0 and buf[..., :3].all()

    spec = load_hydra_xml(scene_path("test_spectral"), 32, 32, spectral=True)
    assert spec.spectral_mode == 1
    gs = HipIntegrator(spec)
    out = np.zeros((32, 32, 4), np.float32)
    assert gs.L.hpt_path_trace_qmc_block(gs.h, N, 4, out.ctypes.data, 1) == HPT_ERR_UNSUPPORTED and "spectral" in err(gs)
    assert not out.any()
    # the cap of the sample count is the host's computation; nothing of that size is launched here
    assert g.L.hpt_qmc_sample_count(1 << 16, 1 << 16) == 2 ** 32 - 1 and g.L.hpt_qmc_sample_count(N, 4) == 4 * N


# ---- 7. the light and material numbers of a lit vertex ------------------------------------------------------------------------------------------
def _two_light_floor(w, h, fov=90.0):
    """synth.plane_under_rect_light seen through a wide lens (part of the frame misses the floor), lit by a pure red and a pure blue square light:
    with traceDepth 1 a sample's colour is the one light sample of its first vertex, so its hue tells which light was selected."""
    sc = synth.plane_under_rect_light(w, h)
    sc.fov = fov
    sc.lights = [S.light_rect(S.translate(-1.5, 2.0, 0.0), 0.5, 0.5, (1, 0, 0), 10.0), S.light_rect(S.translate(1.5, 2.0, 0.0), 0.5, 0.5, (0, 0, 1), 10.0)]
    return sc


def _floor_hits(sc, params, samples):
    """Which samples' primary rays meet the floor: the restated camera rays through the oracle's closest-hit query."""
    from oracle.orc import OracleIntegrator
    pos, dr = Q.camera_rays(_table(), params, samples, False)
    wpos, wdir = Q.world_rays(params, pos, dr)
    return OracleIntegrator(sc, params).ray_nearest(wpos, wdir)["instId"] != 0xFFFFFFFF


@pytest.mark.gpu
def test_first_bounce_light_selection_comes_from_dimension_lgt_plus_2():
    """GetRandomNumbersLgts at bounce 0: the selection number is dimension lgt + 2 (= 6 in the plain layout), lightId = floor(u * 2). Every sample
    that meets the floor is lit by exactly one of the two lights (nothing stands in the way, both face the floor): red means light 0."""
    from hydracore3_amd import api
    w, h, spp = 64, 32, 4
    sc = _two_light_floor(w, h)
    params = sc.params()
    g = api.HipIntegrator(sc, params)
    _, col, _ = g.render_qmc(spp, frame=False, records=True)
    S_ = w * h * spp
    hit = _floor_hits(sc, params, S_)
    lay = api.qmc_layout(False, False, False)
    assert lay["lgt"] == 4
    u = Q.rnd_float(_table(), np.arange(S_, dtype=np.uint32), lay["lgt"] + 2)
    light = np.minimum(np.floor(u * np.float32(2.0)).astype(np.int64), 1)
    red, blue = col[:, 0] > 0.0, col[:, 2] > 0.0
    assert 0.2 * S_ < hit.sum() < 0.9 * S_, int(hit.sum())
    assert np.all(col[~hit, :3] == 0.0) and np.all(col[:, 1] == 0.0)
    assert np.all(red[hit] != blue[hit]), "a lit sample shows exactly one of the two lights"
    assert np.array_equal(blue[hit], light[hit] == 1), np.flatnonzero(hit & (blue != (light == 1)))[:8]
    # the other two light dimensions would give another answer on this scene (so the assert above can fail)
    for other in (lay["lgt"], lay["lgt"] + 1):
        v = np.minimum(np.floor(Q.rnd_float(_table(), np.arange(S_, dtype=np.uint32), other) * np.float32(2.0)).astype(np.int64), 1)
        assert not np.array_equal(blue[hit], v[hit] == 1)


@pytest.mark.gpu
def test_generators_advance_by_the_draws_of_a_lit_vertex():
    """The same floor, traceDepth 1. A sample that misses draws the camera's float4 and Contribute's float4: 2 generator steps. One that meets the
    floor also draws GetRandomNumbersLgts (a float4 and a float: 2 steps, made although bounce 0 overwrites three of the numbers) and
    GetRandomNumbersMats (1 step): 5 steps. Slot g runs samples g, g + N, ... of a generator count that does not divide S."""
    from hydracore3_amd.api import HipIntegrator
    w, h, spp = 64, 32, 3
    sc = _two_light_floor(w, h)
    params = sc.params()
    g = HipIntegrator(sc, params)
    n_gens = 1000
    g.InitRandomGens(n_gens)
    before = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, before.ctypes.data, n_gens))
    g.render_qmc(spp, frame=False, records=True)
    after = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, after.ctypes.data, n_gens))
    S_ = w * h * spp
    hit = _floor_hits(sc, params, S_)
    assert 0.2 * S_ < hit.sum() < 0.9 * S_
    steps = np.bincount(np.arange(S_) % n_gens, weights=np.where(hit, 5, 2), minlength=n_gens).astype(np.int64)
    assert np.array_equal(after, _rng_steps(before, steps)), np.flatnonzero(np.any(after != _rng_steps(before, steps), axis=1))[:8]


# ---- 8. convergence: the reference's own acceptance practice ------------------------------------------------------------------------------------
def _ldr(img, spp):
    """What the reference's testing/run_tests.py compares with cv2.PSNR: the 8-bit image its CLI saves (mean over spp, clamped, gamma 2.2)."""
    x = np.clip(np.asarray(img)[..., :3].astype(np.float64) / spp, 0.0, 1.0) ** (1.0 / 2.2)
    return np.floor(x * 255.0 + 0.5)


def _psnr(a, b):
    mse = float(np.mean((a - b) ** 2))
    return 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0.0 else 361.2     # cv2.PSNR's value for identical images


def _conv_scene(name):
    if name == "test_035 thin lens":
        sc = load_hydra_xml(scene_path("test_035"), 64, 64)
        sc.cam_lens_radius = 0.08
        return sc
    return load_hydra_xml(scene_path(name), 64, 64) if name == "test_035" else load_hydra_xml(scene_path(name), 48, 32)


# scene -> (spp, two-seed PSNR of the oracle's PathTraceBlock at that spp, max / min of the RMSE against a 16 x spp oracle frame over eight seeds);
# measured with the oracle on the CPU at these sizes (seed k: the generators of InitRandomGens rolled by 977 k pixels)
CONVERGENCE = {
    "test_035": (256, 38.04, 1.446),
    "test_228": (256, 42.72, 1.518),
    "test_035 thin lens": (256, 38.09, 1.570),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONVERGENCE))
def test_qmc_converges_to_the_path_tracer_s_image(name):
    """testing/run_tests.py: PSNR < 30 dB fails, >= 35 dB passes. The QMC frame / spp against the PathTraceBlock frame at the same spp must reach
    35 dB. The spp is the test's: the oracle's PathTraceBlock against ITSELF under two generator seeds measured, on the CPU, 38.04 dB
    (test_035, 64 x 64, 256 spp), 42.72 dB (test_228, 48 x 32, 256 spp) and 38.09 dB (test_035 with a thin lens, 64 x 64, 256 spp) - room to spare above
    the bar for an estimator that is no noisier than the path tracer.
    Second: QMC's RMSE against a 16 x spp PathTraceBlock frame is no worse than PathTraceBlock's own at equal spp, times the spread that RMSE
    shows over eight seeds (max / min, the oracle on the CPU: 1.446, 1.518, 1.570)."""
    from hydracore3_amd.api import HipIntegrator
    spp, _, margin = CONVERGENCE[name]
    sc = _conv_scene(name)
    g = HipIntegrator(sc)
    qmc, _, _ = g.render_qmc(spp)
    pt = HipIntegrator(sc).render(spp)
    ref_gpu = HipIntegrator(sc)
    ref_gpu.InitRandomGens(ref_gpu.N, first_seed=ref_gpu.N)             # other generators than the frame it is compared with
    ref = ref_gpu.render(16 * spp)
    psnr = _psnr(_ldr(qmc, spp), _ldr(pt, spp))

    def rmse(img, n):
        return float(np.sqrt(np.mean((img[..., :3].astype(np.float64) / n - ref[..., :3].astype(np.float64) / (16 * spp)) ** 2)))
    r_qmc, r_pt = rmse(qmc, spp), rmse(pt, spp)
    print(f"{name}: {spp} spp, PSNR(QMC, PathTraceBlock) = {psnr:.2f} dB; RMSE vs {16 * spp} spp: QMC {r_qmc:.5f}, PathTraceBlock {r_pt:.5f}, ratio {r_qmc / r_pt:.3f} (margin {margin})")
    assert psnr >= 35.0
    assert r_qmc <= r_pt * margin

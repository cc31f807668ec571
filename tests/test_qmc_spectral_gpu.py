"""PathTraceBlockQMC under m_spectral_mode on the GPU (hpt_spectral.hip: pathTraceQmcSpectralKernel; opt-in through
hpt_set_option("qmc_spectral", 1)): the switch, the wavelength dimension, exact per-sample colours on a sky with a spectrum, the atomic frame and
the atomic wavelength layers against the call's own records, the generator contract, the dispersive flag, arguments.

What is compared with what:
 * wavelengths and pixel indices: tests/qmc_reference.py and tests/qmc_spectral_reference.py (numpy float32, table from the recorded fixture);
 * per-sample colours: the restated SpectralCamRespoceToRGB of the restated radiance, bit for bit;
 * frames and layers: the float64 scatter-sum of the same call's records, every cell held to n * 2^-24 * sum|x_i| (n float32 additions in any
   order, each rounding a partial sum no larger than sum|x_i| by at most half an ulp: the bound derived in test_qmc_gpu.py).
"""
import numpy as np
import pytest

import qmc_reference as Q
import qmc_spectral_reference as QS
from conftest import scene_path
from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.scene import load_hydra_xml

HPT_ERR_ARG, HPT_ERR_STATE, HPT_ERR_UNSUPPORTED = 1, 3, 4
EXPOSURE = 1.5


def _table():
    return Q.load_fixture()[0]


def _spectrum(k):
    """A smooth positive spectrum at 1 nm from LAMBDA_MIN, 471 values, different for every k."""
    lam = np.arange(471, dtype=np.float64)
    return (0.75 + 0.5 * np.sin(lam / (23.0 + 9.0 * k) + k) + 0.001 * lam * (k % 3)).astype(np.float32)


def _sky_scene(w, h, dof=False, motion=False, response=None):
    """synth.furnace_plane seen from above, looking up: every path leaves the scene at once and picks up the environment's spectrum (id 0).
    response: None (the CIE observer) or (ids, type) for m_camResponseSpectrumId / m_camResponseType."""
    sc = synth.furnace_plane(w, h, env=(0.5, 0.25, 2.0))
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 5.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 1.0)
    sc.spectral_mode = 1
    sc.spec_values = np.concatenate([_spectrum(k) for k in range(4)])
    sc.spec_offset_sz = [(471 * k, 471) for k in range(4)]
    sc.env_spec_id, sc.env_spec_mult = 0, 2.5
    sc.exposure_mult = EXPOSURE
    if response is not None:
        sc.cam_response_spectrum_id, sc.cam_response_type = response
    if dof:
        sc.cam_lens_radius = 0.05
    if motion:
        sc.inst_motion[0] = np.asarray(sc.inst_matrices[0], np.float64).reshape(4, 4) @ S.translate(0.25, 0.0, 0.0)
    return sc


def _gpu(sc, on=True, **kw):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, **kw)
    if on:
        g.set_option("qmc_spectral", 1)
    return g


def _err(g):
    return g.L.hpt_last_error(g.h).decode()


def _restated_waves(samples, dof, motion):
    spd = Q.LAYOUTS[(dof, True, motion)][1]
    return QS.sample_wavelengths(QS.wave_samples(_table(), samples, spd)), spd


# ---- 1. off by default ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spectral_qmc_is_off_until_the_option_is_set():
    w = h = 32
    g = _gpu(_sky_scene(w, h), on=False)
    out = np.zeros((h, w, 4), np.float32)
    assert g.L.hpt_path_trace_qmc_block(g.h, w * h, 4, out.ctypes.data, 1) == HPT_ERR_UNSUPPORTED and "spectral" in _err(g)
    layers = np.zeros((8, h, w), np.float32)
    assert g.L.hpt_path_trace_qmc_block(g.h, w * h, 8, layers.ctypes.data, 1) == HPT_ERR_UNSUPPORTED
    assert not out.any() and not layers.any()
    g.set_option("qmc_spectral", 1)
    assert g.L.hpt_path_trace_qmc_block(g.h, w * h, 4, out.ctypes.data, 1) == 0, _err(g)
    assert np.isfinite(out).all() and out[..., :3].any() and not out[..., 3].any()
    g.set_option("qmc_spectral", 0)
    assert g.L.hpt_path_trace_qmc_block(g.h, w * h, 4, out.ctypes.data, 1) == HPT_ERR_UNSUPPORTED
    # the option leaves an RGB context alone: the same frame with and without it
    rgb = synth.furnace_plane(w, h, env=(0.5, 0.25, 2.0))
    a, _, _ = _gpu(rgb, on=False).render_qmc(2)
    b, _, _ = _gpu(rgb, on=True).render_qmc(2)
    assert a.tobytes() == b.tobytes()


# ---- 2. the wavelength dimension ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dof,motion", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("w,h,spp", [(64, 64, 4), (48, 20, 3)])
def test_sample_wavelengths_equal_the_restatement(dof, motion, w, h, spp):
    g = _gpu(_sky_scene(w, h, dof, motion))
    _, col, pix, wav = g.render_qmc(spp, frame=False, waves=True)
    want, spd = _restated_waves(w * h * spp, dof, motion)
    if (dof, motion) == (False, True):
        assert spd == 3                                                   # spectral + motion: the one layout whose wavelength dimension is not 4
    else:
        assert spd == 4
    from hydracore3_amd import api
    assert api.qmc_layout(dof, True, motion)["spd"] == spd
    assert wav.shape == want.shape and np.array_equal(wav.view(np.uint32), want.view(np.uint32)), np.flatnonzero(np.any(wav != want, axis=1))[:8]
    assert wav.min() >= QS.LAMBDA_MIN and wav.max() <= QS.LAMBDA_MAX
    _, _, wpix = Q.sample_pixels(_table(), w * h * spp, w, h)
    assert np.array_equal(pix, wpix)


# ---- 3. constant sky: exact per-sample colours --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("response", [None, ((1, 2, 3), 0), ((1, -1, 3), 1)], ids=["cie", "response-xyz", "response-rgb"])
@pytest.mark.parametrize("channels", [4, 1])
def test_sky_colours_equal_the_restated_conversion(response, channels):
    w, h, spp = 48, 20, 3
    sc = _sky_scene(w, h, response=response)
    g = _gpu(sc)
    _, col, pix, wav = g.render_qmc(spp, channels=channels, frame=False, waves=True)
    waves, _ = _restated_waves(w * h * spp, False, False)
    assert np.array_equal(wav.view(np.uint32), waves.view(np.uint32))
    radiance = QS.env_spectrum(sc, waves)
    want = QS.contribution(QS.spectral_cam_response_to_rgb(radiance, waves, sc), EXPOSURE, channels)
    diff = np.flatnonzero(np.any(col.view(np.uint32) != want.view(np.uint32), axis=1))
    print(f"{w * h * spp} samples, {len(np.unique(col, axis=0))} distinct colours, {diff.size} differ")
    assert len(np.unique(col, axis=0)) > 100
    assert diff.size == 0, (diff[:8], col[diff[:4]], want[diff[:4]])


# ---- 4. emitters with spectra: exact per-sample colours against the CPU oracle ---------------------------------------------------------------------
def _emitter_scene(w, h, dof=False, motion=False):
    """test_035's geometry, every material an emitter, traceDepth 1. An emitter's spectrum is its light record's (LightIntensity reads
    lights[remapInst[inst].y].specId): every instance is given a record of its own - a sphere light, whose emission has no facing test - with its
    own spectrum and multiplier. The records are never sampled: a light sample is only evaluated at a surface that is not an emitter. A ray that
    misses picks up the environment's spectrum. dof: constant spectra, for the sinf / cosf reason documented in
    test_qmc_gpu.test_per_sample_colours_equal_the_oracle."""
    sc = load_hydra_xml(scene_path("test_035"), w, h, spectral=True)
    remap = np.asarray(sc.remap_inst).reshape(-1, 2)
    n_inst = len(sc.inst_matrices)
    assert remap.shape[0] == n_inst
    lam = np.arange(471, dtype=np.float64)
    specs = [_spectrum(0)]
    for i in range(n_inst):
        level = 1.5 + 0.25 * (i % 5)
        specs.append(np.full(471, level, np.float32) if dof else (level + 0.4 * np.sin(lam / (17.0 + 5.0 * i) + i)).astype(np.float32))
    sc.spec_values = np.concatenate(specs)
    sc.spec_offset_sz = [(471 * k, 471) for k in range(len(specs))]
    sc.spec_tex_offset_sz = [(S.UINT_MAX, 0)] * len(specs)
    sc.materials = [S.material_emissive((1.0, 1.0, 1.0)) for _ in sc.materials]
    sc.lights = []
    for i in range(n_inst):
        lt = S.light_sphere(np.eye(4), 1.0, (1.0, 1.0, 1.0), 1.0 + 0.25 * (i % 3))
        lt["specId"] = i + 1
        sc.lights.append(lt)
    sc.remap_inst = [(int(r[0]), i) for i, r in enumerate(remap)]
    sc.trace_depth = 1
    sc.env_spec_id, sc.env_spec_mult = 0, 2.5
    sc.exposure_mult = EXPOSURE
    if dof:
        sc.cam_lens_radius = 0.08
    if motion:
        last = n_inst - 1
        sc.inst_motion[last] = np.asarray(sc.inst_matrices[last], np.float64).reshape(4, 4) @ S.translate(0.4, 0.0, 0.1)
    return sc


def _oracle_accum(sc, params, dof, motion_dim, waves):
    """Component i of a path's accumColor: the restated QMC camera rays through the oracle's PathTraceFromInputRaysBlock with wavelength
    lambda_i splatted over the four slots (kernel_InitEyeRayFromInput); its .x is what the hero path carries in slot i."""
    from oracle.orc import OracleIntegrator
    cpu = OracleIntegrator(sc, params)
    samples = waves.shape[0]
    pos, dr = Q.camera_rays(_table(), params, samples, dof, motion_dim)
    acc = np.zeros((samples, 4), np.float32)
    for i in range(4):
        pos[:, 3] = waves[:, i]
        for a in range(0, samples, cpu.N):
            b = min(samples, a + cpu.N)
            out = np.zeros((b - a, 4), np.float32)
            cpu.path_trace_from_input_rays_block(np.ascontiguousarray(pos[a:b]), np.ascontiguousarray(dr[a:b]), out, 1, channels=4)
            acc[a:b, i] = out[:, 0]
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("name,dof,motion,layout", [("pinhole, single-level", False, False, 0), ("two-level", False, False, 1),
                                                    ("moving instance", False, True, 0), ("thin lens, constant spectra", True, False, 0)])
def test_per_sample_colours_on_emitters_equal_the_oracle(name, dof, motion, layout):
    """The surface path of the kernel against an independent reference: cameraRayAt on the QMC numbers (lens dimensions 2 and 3, the time of
    the motion dimension), the traversal, shadeVertexSpec<.., QmcRands> at an emitter, the accumulator - then the restated conversion. The
    generators afterwards: a sample that meets an emitter draws the lens float4, GetRandomNumbersLgts (a float4 and a float: two steps, made
    although bounce 0 overwrites three of the numbers) and Contribute's float4 - 4 steps; one that misses draws 2. No step for the wave sample
    or the time."""
    from hydracore3_amd import api
    w, h, spp = 64, 64, 4
    S_ = w * h * spp
    sc = _emitter_scene(w, h, dof, motion)
    params = sc.params()
    g = _gpu(sc, params=params, accel_layout=layout)
    before = np.zeros((g.N, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, before.ctypes.data, g.N))
    _, col, pix, wav = g.render_qmc(spp, frame=False, waves=True)
    after = np.zeros((g.N, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, after.ctypes.data, g.N))
    lay = api.qmc_layout(dof, True, motion)
    waves, spd = _restated_waves(S_, dof, motion)
    assert lay["spd"] == spd and np.array_equal(wav.view(np.uint32), waves.view(np.uint32))
    _, _, wpix = Q.sample_pixels(_table(), S_, w, h)
    assert np.array_equal(pix, wpix)
    acc = _oracle_accum(sc, params, dof, lay["motion"] if motion else 0, waves)
    hit = np.any(acc != QS.env_spectrum(sc, waves), axis=1)
    assert hit.sum() > S_ // 4, f"{name}: only {int(hit.sum())} samples see the emitters"
    want = QS.contribution(QS.spectral_cam_response_to_rgb(acc, waves, sc), EXPOSURE, 4)
    diff = np.flatnonzero(np.any(col.view(np.uint32) != want.view(np.uint32), axis=1))
    print(f"{name}: {S_} samples, {int(hit.sum())} on emitters, {len(np.unique(col, axis=0))} distinct colours, {diff.size} differ")
    assert diff.size == 0, (name, diff[:8], col[diff[:4]], want[diff[:4]])
    steps = np.bincount(np.arange(S_) % g.N, weights=np.where(hit, 4, 2), minlength=g.N).astype(np.int64)
    assert np.array_equal(after, _rng_steps(before, steps)), np.flatnonzero(np.any(after != _rng_steps(before, steps), axis=1))[:8]


# ---- 5. the atomic frame against its own records ------------------------------------------------------------------------------------------------------
def _held(frame, ref, mag, n):
    err = np.abs(frame.astype(np.float64) - ref)
    bound = n * 2.0 ** -24 * mag
    print(f"worst error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, additions per cell up to {int(n.max())}")
    return np.all(err <= bound), np.argwhere(err > bound)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [4, 1])
def test_frame_equals_the_scatter_sum_of_the_records(channels):
    w, h, spp = 48, 32, 8
    g = _gpu(load_hydra_xml(scene_path("test_spectral"), w, h, spectral=True))
    img, col, pix = g.render_qmc(spp, channels=channels, records=True)
    k = 3 if channels == 4 else 1
    assert np.isfinite(col).all() and col[:, :k].max() > 0.0 and np.all(col[:, k:] == 0.0)
    ref, mag = np.zeros((w * h, k), np.float64), np.zeros((w * h, k), np.float64)
    np.add.at(ref, pix, col[:, :k].astype(np.float64))
    np.add.at(mag, pix, np.abs(col[:, :k].astype(np.float64)))
    n = np.bincount(pix, minlength=w * h).astype(np.float64)[:, None]
    ok, where = _held(img.reshape(w * h, channels)[:, :k], ref, mag, n)
    assert ok, where
    if channels == 4:
        assert np.all(img[..., 3] == 0.0)


# ---- 6. the wavelength layers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sky", "test_spectral"])
def test_layers_equal_the_scatter_sum_of_the_records(name):
    w, h, spp, layers = 48, 32, 8, 8
    sc = _sky_scene(w, h) if name == "sky" else load_hydra_xml(scene_path("test_spectral"), w, h, spectral=True)
    g = _gpu(sc)
    img, col, pix, wav = g.render_qmc(spp, channels=layers, waves=True)
    assert img.shape == (layers, h, w) and np.isfinite(col).all() and col.max() > 0.0
    lid = QS.layer_index(wav, layers)
    assert lid.min() >= 0 and lid.max() == layers - 1 and len(np.unique(lid)) == layers
    cell = (lid * (w * h) + pix[:, None].astype(np.int64)).reshape(-1)
    x = col.astype(np.float64).reshape(-1)
    ref, mag = np.zeros(layers * w * h, np.float64), np.zeros(layers * w * h, np.float64)
    np.add.at(ref, cell, x)
    np.add.at(mag, cell, np.abs(x))
    n = np.bincount(cell, minlength=layers * w * h).astype(np.float64)
    ok, where = _held(img.reshape(-1), ref, mag, n)
    assert ok, where
    # the layers of a pixel together hold the four components of its samples
    total, tmag = np.zeros(w * h, np.float64), np.zeros(w * h, np.float64)
    np.add.at(total, pix, col.astype(np.float64).sum(axis=1))
    np.add.at(tmag, pix, np.abs(col.astype(np.float64)).sum(axis=1))
    bound = (n * 2.0 ** -24 * mag).reshape(layers, w * h).sum(axis=0)          # the cells' bounds, added up
    assert np.all(np.abs(img.astype(np.float64).reshape(layers, w * h).sum(axis=0) - total) <= bound + 2.0 ** -50 * tmag)
    if name == "sky":
        # the record of a layered call is exposure * accumColor[i]: the restated environment spectrum at the restated wavelengths
        waves, _ = _restated_waves(w * h * spp, False, False)
        want = (QS.env_spectrum(sc, waves) * np.float32(EXPOSURE)).astype(np.float32)
        assert np.array_equal(col.view(np.uint32), want.view(np.uint32))


# ---- 7. the generator contract ------------------------------------------------------------------------------------------------------------------------
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
    """The sky: the camera takes one float4, Contribute one float4; the wavelength sample comes from its dimension (4, or 3 with motion) and the
    time from its own, neither with a pseudo draw: two steps per sample. Slot g runs samples g, g + N, ... of a generator count that does not
    divide S."""
    w, h, spp = 32, 32, 3
    g = _gpu(_sky_scene(w, h, motion=motion))
    n_gens = 1000
    g.InitRandomGens(n_gens)
    before = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, before.ctypes.data, n_gens))
    g.render_qmc(spp, frame=False, waves=True)
    after = np.zeros((n_gens, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, after.ctypes.data, n_gens))
    S_ = w * h * spp
    per_slot = (S_ - np.arange(n_gens) + n_gens - 1) // n_gens
    assert per_slot.sum() == S_ and per_slot.min() == 3 and per_slot.max() == 4
    assert np.array_equal(after, _rng_steps(before, 2 * per_slot))
    assert not np.array_equal(after, _rng_steps(before, 3 * per_slot))   # what a pseudo draw for the wavelength would leave


# ---- 8. a dispersive path -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_diverged_paths_keep_their_first_wavelength():
    """The spectral Cornell box with a flint-like glass sphere (tests/golden/scenes/spectral_glass: a dielectric whose interior IOR is a spectrum,
    under the box's emitter), traceDepth 3. A layered call (channels = 8) records the raw four components exposure * accumColor[i] (exposure 1
    here), the same call with 4 channels the colour. A sample whose path crossed the sphere carries RAY_FLAG_WAVES_DIVERGED: its colour is the
    restated conversion with terminate_waves = True of its own components; every other sample's the conversion without.
    What this does and does not show: a sample is CLASSIFIED by which of the two conversions of the device's own components equals its colour
    (no flag is recorded). So it shows that every colour is one of the two conversions and that both occur in numbers; which paths crossed the
    glass is checked against geometry only as far as this: the restated primary rays through the oracle's closest-hit query say which samples
    meet the sphere FIRST, and such a sample, if it is not black, must be diverged (its first vertex is the dispersive dielectric). Samples that
    reach the glass after a bounce are not checked against geometry."""
    w, h, spp = 32, 32, 4
    sc = load_hydra_xml(scene_path("spectral_glass"), w, h, spectral=True)
    sc.trace_depth = 3
    sc.exposure_mult = 1.0
    _, raw, pix8, wav8 = _gpu(sc).render_qmc(spp, channels=8, frame=False, waves=True)
    _, col, pix, wav = _gpu(sc).render_qmc(spp, channels=4, frame=False, waves=True)
    assert np.array_equal(pix, pix8) and np.array_equal(wav.view(np.uint32), wav8.view(np.uint32))
    plain = QS.contribution(QS.spectral_cam_response_to_rgb(raw, wav, sc, False), 1.0, 4)
    term = QS.contribution(QS.spectral_cam_response_to_rgb(raw, wav, sc, True), 1.0, 4)
    is_plain = np.all(col.view(np.uint32) == plain.view(np.uint32), axis=1)
    is_term = np.all(col.view(np.uint32) == term.view(np.uint32), axis=1)
    diverged = is_term & ~is_plain
    print(f"{col.shape[0]} samples: {int(diverged.sum())} diverged, {int((is_plain & ~is_term).sum())} not, {int((is_plain & is_term).sum())} either (black), "
          f"{int((~is_plain & ~is_term).sum())} neither")
    assert np.all(is_plain | is_term), np.flatnonzero(~(is_plain | is_term))[:8]
    assert diverged.sum() >= 0.05 * col.shape[0]
    assert (is_plain & ~is_term).sum() >= 0.05 * col.shape[0]
    # geometry: the instance the primary ray meets first, from the oracle; the sphere's is the one whose material is the dielectric
    from oracle.orc import OracleIntegrator
    params = sc.params()
    pos, dr = Q.camera_rays(_table(), params, col.shape[0], False)
    wpos, wdir = Q.world_rays(params, pos, dr)
    first = OracleIntegrator(sc, params).ray_nearest(wpos, wdir)
    glass_mats = {i for i, m in enumerate(sc.materials) if int(m["mtype"]) == S.MAT_TYPE_DIELECTRIC}
    assert glass_mats
    inst, prim = first["instId"].astype(np.int64), first["primId"].astype(np.int64)
    mvo = np.asarray(sc.mat_vert_offset, np.int64).reshape(-1, 2)
    geom = np.asarray(sc.inst_geom, np.int64)
    on_glass = np.zeros(col.shape[0], bool)
    ok = first["instId"] != 0xFFFFFFFF
    mat = np.asarray(sc.mat_id_by_prim, np.int64)[mvo[geom[inst[ok]], 0] + prim[ok]] & 0x00FFFFFF
    # the instance's remap list (pairs from -> to in all_remap_lists, the lists' offsets behind them), as RemapMaterialId applies it
    lists = np.asarray(sc.all_remap_lists, np.int64)
    flat, offs = lists[:sc.all_remap_lists_size], lists[sc.all_remap_lists_size:]
    rid = np.asarray(sc.remap_inst, np.int64).reshape(-1, 2)[inst[ok], 0]
    for r in np.unique(rid[rid >= 0]):
        for k in range(int(offs[r]), int(offs[r + 1]), 2):
            mat = np.where((rid == r) & (mat == flat[k]), flat[k + 1], mat)
    on_glass[ok] = np.isin(mat, list(glass_mats))
    lit = np.any(col[:, :3] != 0.0, axis=1)
    print(f"{int(on_glass.sum())} samples meet the glass first, {int((on_glass & lit).sum())} of them not black")
    assert (on_glass & lit).sum() >= 0.02 * col.shape[0]
    assert np.all(diverged[on_glass & lit]), np.flatnonzero(on_glass & lit & ~diverged)[:8]
    assert not np.any(diverged & ~on_glass & (first["instId"] == 0xFFFFFFFF))


# ---- 9. convergence ---------------------------------------------------------------------------------------------------------------------------------------
def _ldr(img, spp):
    """What the reference's testing/run_tests.py compares with cv2.PSNR: the 8-bit image its CLI saves (mean over spp, clamped, gamma 2.2)."""
    x = np.clip(np.asarray(img)[..., :3].astype(np.float64) / spp, 0.0, 1.0) ** (1.0 / 2.2)
    return np.floor(x * 255.0 + 0.5)


def _psnr(a, b):
    mse = float(np.mean((a - b) ** 2))
    return 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0.0 else 361.2


# the reference's test_spectral fixture at 48 x 32, 1024 spp, measured with the oracle on the CPU (seed k: the generators of InitRandomGens rolled
# by 977 k pixels): PSNR of the oracle's spectral PathTraceBlock under seed 0 against seed 1, and max - min of seed 0 against seeds 1 .. 7
CONV_SPP, CONV_TWO_SEED_PSNR, CONV_SEED_SPREAD = 1024, 37.09, 1.50


@pytest.mark.gpu
def test_spectral_qmc_converges_to_the_oracle_s_spectral_image():
    """The QMC spectral frame / spp against the oracle's spectral PathTraceBlock frame / spp (seed 0) on the reference's test_spectral fixture,
    48 x 32 at 1024 spp, as 8-bit images the way testing/run_tests.py compares them. The bar is the oracle's: PathTraceBlock against ITSELF
    under two generator seeds measured 37.09 dB on the CPU (seed 0 against seed 1); seed 0 against seeds 1 .. 7 gave 37.09, 38.37, 38.57,
    38.53, 37.75, 37.07, 38.24 dB, a seed-to-seed spread of 1.50 dB (the RGB test's scenes had 3 dB). An estimator that is no noisier than
    the path tracer does no worse than 37.09 - 1.50 = 35.59 dB. (At 256 spp the same measurement gave 30.1 .. 33.6 dB, a spread of 3.5 dB:
    too wide to say anything, hence 1024 spp; the oracle's frame takes about a second.) Measured on the MI355X: 38.87 dB."""
    from oracle.orc import OracleIntegrator
    w, h, spp = 48, 32, CONV_SPP
    sc = load_hydra_xml(scene_path("test_spectral"), w, h, spectral=True)
    qmc, _, _ = _gpu(sc).render_qmc(spp)
    ref = OracleIntegrator(sc).render(spp)
    psnr = _psnr(_ldr(qmc, spp), _ldr(ref, spp))
    bar = CONV_TWO_SEED_PSNR - CONV_SEED_SPREAD
    print(f"test_spectral {w} x {h}, {spp} spp: PSNR(QMC spectral, oracle PathTraceBlock) = {psnr:.2f} dB, bar {bar:.2f} dB "
          f"(oracle against itself {CONV_TWO_SEED_PSNR} dB, spread {CONV_SEED_SPREAD} dB)")
    assert np.isfinite(qmc).all()
    assert psnr >= bar


# ---- 10. arguments --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_codes():
    from hydracore3_amd.api import HydraHipError
    w = h = 32
    N = w * h
    g = _gpu(_sky_scene(w, h))
    buf = np.zeros((8, h, w), np.float32)
    assert g.L.hpt_path_trace_qmc_block(g.h, N, 2, buf.ctypes.data, 1) == HPT_ERR_UNSUPPORTED and "channels" in _err(g)
    assert g.L.hpt_path_trace_qmc_block_dev2(g.h, N, 4, None, 1, None, None, buf.ctypes.data, None) == HPT_ERR_ARG and "wavelength" in _err(g)
    assert g.L.hpt_path_trace_qmc_block_dev2(None, N, 4, None, 1, None, None, None, None) == HPT_ERR_ARG
    assert g.L.hpt_path_trace_qmc_block_dev2(g.h, N, 4, None, 1, None, None, None, None) == HPT_ERR_ARG and "no frame" in _err(g)
    assert g.L.hpt_set_option(g.h, b"qmc_spectral", 2) == HPT_ERR_ARG and "qmc_spectral" in _err(g)
    assert g.L.hpt_set_option(g.h, b"qmc_spectral", -1) == HPT_ERR_ARG
    assert not buf.any()
    g.PathTraceBlockQMC(N, 8, buf, 1)                                      # the option survived the refused values
    assert buf.any()
    t = g.GetExecutionTime("PathTraceBlockQMC")
    assert t[0] > 0.0 and all(v >= 0.0 for v in t[1:3])
    # films whose tables were precomputed for RGB rendering, as PathTraceBlock refuses them
    film = load_hydra_xml(scene_path("thin_film"), w, h, spectral=False)
    film.spectral_mode = 1
    gf = _gpu(film)
    out = np.zeros((h, w, 4), np.float32)
    with pytest.raises(HydraHipError, match="thin film"):
        gf.PathTraceBlockQMC(N, 4, out, 1)
    with pytest.raises(HydraHipError, match="thin film"):
        gf.render(1)
    assert not out.any()

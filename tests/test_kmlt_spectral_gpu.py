"""PathTraceBlockKMLT and the primary-sample-space pass under m_spectral_mode on the GPU (hpt_spectral.hip: pssEvalSpec, pathTracePssSpectralKernel,
kmltChainSpectralKernel; opt-in through hpt_set_option("kmlt_spectral", 1)).

What is compared with what:
 * wavelengths: SampleWavelengths of slot 4 restated in numpy (tests/qmc_spectral_reference.py), bit for bit;
 * colours on a sky with a spectrum: the restated SpectralCamRespoceToRGB of the restated radiance, bit for bit - no device path tracer involved;
 * F(x) for the vectors the pseudo generator would have drawn (tests/kmlt_spectral_reference.py): one spectral PathTraceBlock pass of the same
   context (device code, itself held to the oracle by test_gpu_spectral.py), bit for bit;
 * diverged paths: every colour is one of the two restated conversions of the pass's own raw components;
 * the chains: replayed from the device's own records against tests/kmlt_reference.py exactly as test_kmlt_gpu.py replays the RGB chains - the
   chain works on the RGB colour PathTraceF returns, so nothing of the bookkeeping is new; what is new is that F of a recorded vector is the
   spectral pass, and that slot 4 is mutated with the others.
"""
import numpy as np
import pytest

import kmlt_reference as K
import kmlt_spectral_reference as KS
import qmc_spectral_reference as QS
from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml
from test_qmc_spectral_gpu import EXPOSURE, _emitter_scene, _sky_scene

F32 = np.float32
HPT_ERR_ARG, HPT_ERR_UNSUPPORTED = 1, 4
EPS = 2.0 ** -24


def _gpu(sc, on=True, layout=0):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, accel_layout=layout)
    if on:
        g.set_option("kmlt_spectral", 1)
    return g


def _err(g):
    return g.L.hpt_last_error(g.h).decode()


def _vectors(g):
    return KS.base_vectors(g.random_gens(), g.packed_xy(), g.params, bool(g.scene.inst_motion))[0]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- 1. the switch -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spectral_mlt_is_off_until_the_option_is_set():
    import ctypes as C
    from hydracore3_amd.api import HydraHipError
    g = _gpu(load_hydra_xml(scene_path("test_spectral"), 16, 16, spectral=True), on=False)
    n = K.state_size(g.params.traceDepth)
    img = np.zeros((16, 16, 4), F32)
    x = _vectors(g)
    d = C.c_void_p()
    g._chk(g.L.hpt_device_malloc(g.h, 65536, C.byref(d)))

    def refused():
        assert g.L.hpt_path_trace_kmlt_block(g.h, g.N, 4, img.ctypes.data, 1) == HPT_ERR_UNSUPPORTED and "spectral" in _err(g) and "kmlt_spectral" in _err(g)
        assert g.L.hpt_path_trace_pss_dev(g.h, d, 1, n, d, d, None) == HPT_ERR_UNSUPPORTED and "spectral" in _err(g)
        assert g.L.hpt_path_trace_kmlt_block_dev(g.h, g.N, 4, d, 1, 1, None, None, None) == HPT_ERR_UNSUPPORTED and "spectral" in _err(g)
        assert not img.any()
    try:
        refused()
        g.set_option("kmlt_spectral", 1)
        g.set_option("kmlt_chains", 64)
        assert g.L.hpt_path_trace_kmlt_block(g.h, g.N, 4, img.ctypes.data, 2) == 0, _err(g)
        assert np.isfinite(img).all() and img[..., :3].any() and not img[..., 3].any()
        col, pix, wav, raw = g.path_trace_pss(x, waves=True, accum=True)
        assert np.isfinite(col).all() and col[:, :3].any() and wav.min() >= QS.LAMBDA_MIN and wav.max() <= QS.LAMBDA_MAX and raw.any()
        assert g.kmlt_chain_count(2) == (64, 8)
        img[:] = 0.0
        g.set_option("kmlt_spectral", 0)
        refused()
        # refused values leave the option as it is
        g.set_option("kmlt_spectral", 1)
        assert g.L.hpt_set_option(g.h, b"kmlt_spectral", 2) == HPT_ERR_ARG and "kmlt_spectral" in _err(g)
        assert g.L.hpt_set_option(g.h, b"kmlt_spectral", -1) == HPT_ERR_ARG
        assert g.L.hpt_path_trace_pss_dev(g.h, d, 1, n, d, d, None) == 0, _err(g)
        # channels stays 4: no wavelength layers in MLT
        assert g.L.hpt_path_trace_kmlt_block_dev(g.h, g.N, 8, d, 1, 1, None, None, None) == HPT_ERR_ARG and "channels" in _err(g)
    finally:
        g.L.hpt_device_free(g.h, d)
    # films whose tables were precomputed for RGB rendering, as PathTraceBlock and spectral QMC refuse them
    film = load_hydra_xml(scene_path("thin_film"), 16, 16, spectral=False)
    film.spectral_mode = 1
    gf = _gpu(film)
    with pytest.raises(HydraHipError, match="thin film"):
        gf.PathTraceBlockKMLT(gf.N, 4, img, 1)
    with pytest.raises(HydraHipError, match="thin film"):
        gf.path_trace_pss(np.zeros((4, K.state_size(gf.params.traceDepth)), F32))
    assert not img.any()
    # an RGB context: the option changes nothing, and there are no wavelengths to record
    from hydracore3_amd import synth
    rgb = synth.furnace_plane(16, 16, env=(0.5, 0.25, 2.0))
    a, b = _gpu(rgb, on=False), _gpu(rgb, on=True)
    xr = np.random.default_rng(3).random((64, K.state_size(a.params.traceDepth)), dtype=F32)
    assert a.path_trace_pss(xr)[0].tobytes() == b.path_trace_pss(xr)[0].tobytes()
    ra, rb = a.render_kmlt(2, chains=32, records=True), b.render_kmlt(2, chains=32, records=True)
    assert ra["color"].tobytes() == rb["color"].tobytes() and ra["accepted"].tobytes() == rb["accepted"].tobytes()
    with pytest.raises(HydraHipError, match="wavelength"):
        b.path_trace_pss(xr, waves=True)
    with pytest.raises(HydraHipError, match="wavelength"):
        b.path_trace_pss(xr, accum=True)


# ---- 2. the wavelengths ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wavelengths_are_sample_wavelengths_of_slot_4():
    w, h = 48, 20
    g = _gpu(_sky_scene(w, h))
    x = _vectors(g)
    hand = np.asarray([0.0, 0.25, 0.999999, 1.0], F32)                   # the lower end, a wrap-around onto LAMBDA_MAX, just below and at the upper end
    x[:hand.size, KS.WAVE_SLOT] = hand
    col, pix, wav = g.path_trace_pss(x, waves=True)
    want = QS.sample_wavelengths(x[:, KS.WAVE_SLOT])
    assert wav.shape == want.shape and np.array_equal(_bits(wav), _bits(want)), np.flatnonzero(np.any(wav != want, axis=1))[:8]
    assert wav[0].tolist() == [360.0, 477.5, 595.0, 712.5] and wav[1].tolist() == [477.5, 595.0, 712.5, 830.0] and wav[3].tolist() == [830.0, 477.5, 595.0, 712.5]
    assert wav.min() >= QS.LAMBDA_MIN and wav.max() <= QS.LAMBDA_MAX and len(np.unique(wav[:, 0])) > w * h // 2
    px = np.minimum((x[:, 0] * F32(w)).astype(np.uint32), w - 1)
    py = np.minimum((x[:, 1] * F32(h)).astype(np.uint32), h - 1)
    assert np.array_equal(pix, py * np.uint32(w) + px)


# ---- 3. a sky with a spectrum: the known answer -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("response", [None, ((1, 2, 3), 0), ((1, -1, 3), 1)], ids=["cie", "response-xyz", "response-rgb"])
def test_sky_colours_equal_the_restated_conversion(response):
    w, h = 48, 20
    sc = _sky_scene(w, h, response=response)
    g = _gpu(sc)
    x = _vectors(g)
    col, pix, wav, raw = g.path_trace_pss(x, waves=True, accum=True)
    waves = QS.sample_wavelengths(x[:, KS.WAVE_SLOT])
    assert np.array_equal(_bits(wav), _bits(waves))
    radiance = QS.env_spectrum(sc, waves)
    want = QS.contribution(QS.spectral_cam_response_to_rgb(radiance, waves, sc), EXPOSURE, 4)
    diff = np.flatnonzero(np.any(_bits(col) != _bits(want), axis=1))
    print(f"{w * h} paths, {len(np.unique(col, axis=0))} distinct colours, {diff.size} differ")
    assert len(np.unique(col, axis=0)) > 100
    assert diff.size == 0, (diff[:8], col[diff[:4]], want[diff[:4]])
    assert np.array_equal(_bits(raw), _bits((radiance * F32(EXPOSURE)).astype(F32)))


# ---- 4. F(x) == one spectral PathTraceBlock pass ------------------------------------------------------------------------------------------------------
def _pss_equals_one_spectral_pass(g):
    x = _vectors(g)
    xy = g.packed_xy()
    gens = g.random_gens().copy()
    col, pix, wav = g.path_trace_pss(x, waves=True)
    assert np.array_equal(g.random_gens(), gens)                         # the PSS pass touches no generator
    assert np.array_equal(_bits(wav), _bits(QS.sample_wavelengths(x[:, KS.WAVE_SLOT])))
    img = g.render(1)
    want = img[xy >> 16, xy & 0xFFFF]
    bad = np.flatnonzero(np.any(_bits(col[:, :3]) != _bits(want[:, :3]), axis=1))
    print(f"spectral PSS vs one PathTraceBlock pass: {bad.size} of {g.N} pixels differ; mean colour {float(want[:, :3].mean()):.4f}")
    assert bad.size == 0, (bad[:8], col[bad[:4]], want[bad[:4]])
    assert np.all(col[:, 3] == 0.0) and float(want[:, :3].max()) > 0.0
    px = np.minimum((x[:, 0] * F32(g.W)).astype(np.uint32), g.W - 1)
    py = np.minimum((x[:, 1] * F32(g.H)).astype(np.uint32), g.H - 1)
    assert np.array_equal(pix, py * np.uint32(g.W) + px)
    return x, col


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 64), (48, 20)])
def test_pss_equals_path_trace_block_on_test_spectral(w, h):
    _pss_equals_one_spectral_pass(_gpu(load_hydra_xml(scene_path("test_spectral"), w, h, spectral=True)))


@pytest.mark.gpu
def test_pss_equals_path_trace_block_on_spectral_glass():
    sc = load_hydra_xml(scene_path("spectral_glass"), 64, 64, spectral=True)
    sc.trace_depth = 3
    _pss_equals_one_spectral_pass(_gpu(sc))


@pytest.mark.gpu
def test_pss_equals_path_trace_block_on_thin_films():
    _pss_equals_one_spectral_pass(_gpu(load_hydra_xml(scene_path("thin_film"), 48, 32, spectral=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_pss_equals_path_trace_block_with_a_moving_instance(layout):
    x, _ = _pss_equals_one_spectral_pass(_gpu(_emitter_scene(48, 32, motion=True), layout=layout))
    assert np.any(x[:, KS.TIME_SLOT] != 0.0)


@pytest.mark.gpu
def test_pss_equals_path_trace_block_with_a_thin_lens():
    x, _ = _pss_equals_one_spectral_pass(_gpu(_emitter_scene(48, 32, dof=True)))
    assert np.any(x[:, 2] != 0.0)


# ---- 5. diverged paths ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_diverged_paths_keep_their_first_wavelength():
    """spectral_glass at 64 x 64, depth 3, exposure 1, the vectors of test 4. A path that crossed the dispersive sphere carries
    RAY_FLAG_WAVES_DIVERGED: its colour is the conversion with terminate_waves of its own raw components, every other path's the plain one. A path
    is classified by which of the two equals its colour (no flag is recorded); both classes must hold 2 % of the paths. The CPU oracle's
    spectral pass on this scene, camera and generators, classified the same way from its wavelength layers: 20.7 % diverged, 61.8 % not,
    17.5 % black, none neither."""
    sc = load_hydra_xml(scene_path("spectral_glass"), 64, 64, spectral=True)
    sc.trace_depth = 3
    sc.exposure_mult = 1.0
    g = _gpu(sc)
    col, pix, wav, raw = g.path_trace_pss(_vectors(g), waves=True, accum=True)
    plain, term = KS.colour_from_raw(raw, wav, sc, False), KS.colour_from_raw(raw, wav, sc, True)
    is_plain, is_term = np.all(_bits(col) == _bits(plain), axis=1), np.all(_bits(col) == _bits(term), axis=1)
    diverged, straight = is_term & ~is_plain, is_plain & ~is_term
    n = col.shape[0]
    print(f"{n} paths: {int(diverged.sum())} diverged, {int(straight.sum())} not, {int((is_plain & is_term).sum())} either (black), {int((~is_plain & ~is_term).sum())} neither")
    assert n == 4096 and np.all(is_plain | is_term), np.flatnonzero(~(is_plain | is_term))[:8]
    assert diverged.sum() >= 0.02 * n and straight.sum() >= 0.02 * n


# ---- 6. the chains, replayed from their records -------------------------------------------------------------------------------------------------------
CHAINS, STEPS, NSTATE = 64, 32, 48


@pytest.fixture(scope="module")
def chain_run():
    """One recorded run on test_spectral at 32 x 32, depth 3: 64 chains x 32 steps (2 passes), proposals kept, raw and normalised frame of the same run."""
    sc = load_hydra_xml(scene_path("test_spectral"), 32, 32, spectral=True)
    sc.trace_depth = 3
    g = _gpu(sc)
    gens = g.random_gens().copy()
    r = g.render_kmlt(2, chains=CHAINS, normalize=True, records=True, proposals=True, unnormalised=True)
    assert (r["chains"], r["steps"]) == (CHAINS, STEPS) and r["proposals"].shape == (CHAINS, STEPS, NSTATE)
    assert np.array_equal(g.random_gens(), gens)                         # m_randomGens is left untouched
    ref = K.run_chains(CHAINS, STEPS, NSTATE, (32, 32), recorded=r)
    return g, r, ref


@pytest.mark.gpu
def test_proposals_equal_the_restatement_and_slot_4_is_mutated(chain_run):
    _, r, ref = chain_run
    large = ref["isLarge"]
    assert large.any() and (~large).any()
    assert np.array_equal(_bits(r["proposals"][large]), _bits(ref["proposals"][large]))
    d = K.circular_distance(r["proposals"][~large], ref["proposals"][~large])
    print(f"small-step proposals: max circular distance {d.max():.3e} = {d.max() / EPS:.2f} x 2^-24 over {d.size} numbers")
    assert d.max() <= 8 * EPS
    # the wavelength sample moves with every small step: the state a proposal was made from is the last accepted proposal (or the initial state)
    cur = ref["init"].copy()
    moved = np.zeros((CHAINS, STEPS), bool)
    for i in range(STEPS):
        moved[:, i] = r["proposals"][:, i, KS.WAVE_SLOT] != cur[:, KS.WAVE_SLOT]
        cur = np.where(r["accepted"][:, i].astype(bool)[:, None], r["proposals"][:, i], cur)
    assert np.all(moved[~large]), np.argwhere(~moved & ~large)[:8]


@pytest.mark.gpu
def test_recorded_colours_are_spectral_f_of_the_recorded_proposals(chain_run):
    g, r, ref = chain_run
    col, pix = g.path_trace_pss(r["proposals"].reshape(-1, NSTATE))
    assert np.array_equal(_bits(col), _bits(r["color"].reshape(-1, 4)))
    assert np.array_equal(pix, r["pixel"].reshape(-1))
    col0, pix0 = g.path_trace_pss(ref["init"])                           # the initial state: stateSize rndFloat1 draws of gen2
    assert np.array_equal(_bits(col0), _bits(r["initColor"])) and np.array_equal(pix0, r["initPixel"])
    assert len(np.unique(col[:, :3], axis=0)) > 100


@pytest.mark.gpu
def test_bookkeeping_equals_the_restatement(chain_run):
    _, r, ref = chain_run
    assert np.array_equal(r["isLarge"].astype(bool), ref["isLarge"])
    assert np.array_equal(_bits(r["a"]), _bits(ref["a"]))
    assert np.array_equal(r["accepted"].astype(bool), ref["accepted"])
    assert np.array_equal(r["oldPixel"], ref["oldPixel"])
    for k, add in (("contribAtX", "addX"), ("contribAtY", "addY")):      # both contributions as formed, and whether the step added them
        assert np.array_equal(_bits(r[k][..., :3]), _bits(ref[k])), k
        assert np.array_equal(r[k][..., 3] == 1.0, ref[add]) and np.all((r[k][..., 3] == 0.0) | (r[k][..., 3] == 1.0))
    assert ref["addX"].any() and ref["addY"].any()
    assert 0 < ref["accepted"].sum() < ref["accepted"].size
    raw = r["frame_unnormalised"].reshape(-1, 4)
    err = np.abs(raw[:, :3].astype(np.float64) - ref["frame"])
    bound = ref["count"][:, None] * EPS * ref["mag"]
    print(f"raw frame vs float64 scatter sum: worst error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}; up to {ref['count'].max()} additions per pixel")
    assert np.all(err <= bound) and np.all(raw[:, 3] == 0.0) and ref["count"].max() > 2


@pytest.mark.gpu
def test_normalisation_equals_the_restatement(chain_run):
    g, r, ref = chain_run
    # the per-chain sums, restated from the records in step order (one double addition per large step), equal the chain restatement's ...
    accum, large = KS.chain_sums(r["isLarge"], r["color"])
    assert np.array_equal(accum, ref["accumBrightness"]) and np.array_equal(large, ref["largeSteps"]) and (large == 0).sum() < CHAINS
    assert np.array_equal(r["accepted"].astype(np.int64).sum(axis=1), ref["accept"])
    # ... and the four statistics formed from them in kmltStatsKernel's own summation order equal the device's doubles exactly. (The device does
    # not export the per-chain sums; avgBrightness is the only thing made of them, and it is compared with ==.)
    want = KS.stats_kernel(accum, large, ref["accept"], r["frame_unnormalised"], g.N, 2)
    got = r["stats"]
    print(f"stats {got.tolist()} restatement {want.tolist()}")
    for k, name in enumerate(("avgBrightness", "actualBrightness", "acceptance rate", "normConst")):
        assert got[k] == want[k], (name, float(got[k]).hex(), float(want[k]).hex())
    assert got[3] == float(F32(got[3])) and got[3] != 1.0
    assert r["frame"].tobytes() == (r["frame_unnormalised"] * F32(got[3])).astype(F32).tobytes()
    # the normalised frame against the float64 scatter sum: the sum's rounding bound times normConst, plus half an ulp of the value for the
    # scaling multiply's own rounding (test_kmlt_gpu.test_constant_sky_known_answer derives it)
    norm = got[3]
    want64 = ref["frame"] * norm
    tol = norm * ref["count"][:, None] * EPS * ref["mag"] + EPS * np.abs(want64)
    frame = r["frame"].reshape(-1, 4)[:, :3].astype(np.float64)
    print(f"normalised frame: worst error / tolerance {np.max(np.abs(frame - want64)[tol > 0] / tol[tol > 0]):.3f}")
    assert np.all(np.abs(frame - want64) <= tol)


# ---- 7. the estimator -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_step_mean_estimates_the_spectral_image_brightness():
    """As test_kmlt_gpu.test_large_step_mean_estimates_the_image_brightness: a large step is an independent uniform vector, so stats[0] is the mean
    of contribFunc(F) over n_large such vectors; the oracle's 64-pass spectral frame gives the same mean from 64 x 1024 samples; both have the
    one-sample deviation sigma, taken from the oracle's one-pass frame. Bound: 5 sigma of the difference.
    How much this shows: the scene has fireflies, sigma measured 4.64 against a mean of 0.316, so with about 8100 large steps the bound is
    0.273 - the test would still pass a large-step mean that is wrong by 85 %. It catches a wrong scale (a missing exposure, a factor 4 from
    the wavelength count, an unconverted spectrum), not a small bias; the exact checks are the tests above."""
    from oracle.orc import OracleIntegrator
    sc = load_hydra_xml(scene_path("test_spectral"), 32, 32, spectral=True)
    one = OracleIntegrator(sc).render(1).reshape(-1, 4)
    sigma = float(np.std(K.contrib_func(one[:, :3]).astype(np.float64), ddof=1))
    mean64 = float(np.mean(K.contrib_func((OracleIntegrator(sc).render(64) / F32(64)).reshape(-1, 4)[:, :3]).astype(np.float64)))
    g = _gpu(sc)
    r = g.render_kmlt(32, chains=512, normalize=False, records=True)
    assert r["steps"] == 64
    n_large = int(r["isLarge"].sum())
    bound = 5.0 * sigma * np.sqrt(1.0 / n_large + 1.0 / (64 * 1024))
    print(f"large-step mean {r['stats'][0]:.5f} vs oracle 64-pass mean brightness {mean64:.5f}: difference {abs(r['stats'][0] - mean64):.5f}, bound {bound:.5f} "
          f"(sigma {sigma:.4f}, {n_large} large steps)")
    assert abs(r["stats"][0] - mean64) <= bound


# ---- 8. deep stacks and layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_spectral_pss_and_kmlt_on_deep_trees(layout):
    """nested_sheets under m_spectral_mode (trees 18 / 16 levels deep: tests/test_deep_stacks.py): the spectral PSS pass == one spectral PathTraceBlock
    pass bit for bit, one short chain run replayed from its records, each with the witness that the HBM part of the stacks was written."""
    from test_deep_stacks import _witness
    from traversal_scenes import nested_sheets
    sc = nested_sheets(width=32, height=32, spectral=True)
    sc.trace_depth = 3
    g = _gpu(sc, layout=layout)
    g.set_option("dbg_stack_witness", 1)
    g.path_trace_pss(_vectors(g))
    _witness(g, f"spectral primary-sample-space pass, layout {layout}")
    _pss_equals_one_spectral_pass(g)
    g = _gpu(sc, layout=layout)
    g.set_option("dbg_stack_witness", 1)
    r = g.render_kmlt(2, chains=CHAINS, normalize=True, records=True, proposals=True)
    _witness(g, f"spectral PathTraceBlockKMLT, layout {layout}")
    assert (r["chains"], r["steps"]) == (CHAINS, STEPS) and r["proposals"].shape == (CHAINS, STEPS, NSTATE)
    ref = K.run_chains(CHAINS, STEPS, NSTATE, (32, 32), recorded=r)
    col, pix = g.path_trace_pss(r["proposals"].reshape(-1, NSTATE))
    assert np.array_equal(_bits(col), _bits(r["color"].reshape(-1, 4))) and np.array_equal(pix, r["pixel"].reshape(-1))
    col0, pix0 = g.path_trace_pss(ref["init"])
    assert np.array_equal(_bits(col0), _bits(r["initColor"])) and np.array_equal(pix0, r["initPixel"])
    assert np.array_equal(r["isLarge"].astype(bool), ref["isLarge"]) and np.array_equal(_bits(r["a"]), _bits(ref["a"]))
    assert np.array_equal(r["accepted"].astype(bool), ref["accepted"]) and np.array_equal(r["oldPixel"], ref["oldPixel"])
    assert 0 < ref["accepted"].sum() < ref["accepted"].size

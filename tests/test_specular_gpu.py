"""The device's smooth interfaces held to the float64 Fresnel, Snell and Airy values of tests/specular_reference.py: the smooth conductor, the smooth
dielectric, the legacy glass and the smooth thin film, through PathTraceFromInputRaysBlock (every sample's ray fixed by the test) and through the
pinhole frames of the kernels input rays cannot reach. Neither the oracle nor another device run is the reference. Figures: profiles/specular.md.

A deterministic case's outputs lie within passes * EPS * value of passes * value. A two-valued case passes two checks: every ray's output is
k * value for an integer k (within passes * EPS * value), and over the n = 4099 copies x 64 passes = 262336 trials of one angle the count K of
reflected samples lies within 5 sqrt(n R (1 - R)) + 1 of n R (exactly n where R = 1). The ray counts are no multiples of 64: a wave tail runs."""
import numpy as np
import pytest

import specular_reference as SR
from hydracore3_amd import scene as S

pytestmark = pytest.mark.gpu

COPIES, PASSES = 4099, 64                    # two-valued cases: n = 262336 >= 2^18 trials per angle; an odd count, so that a wave tail runs
DET_COPIES, DET_PASSES = 70, 3               # deterministic cases
RGB = [c.name for c in SR.CASES if not c.spectral]
SPECTRAL = [c.name for c in SR.CASES if c.spectral]
SNELL = [c.name for c in SR.CASES if c.kind == "dielectric"]
W, H, N = SR.WIDTH, SR.HEIGHT, SR.WIDTH * SR.HEIGHT
FRAME_PASSES = 4


def _gpu(sc, integrator=S.INTEGRATOR_MIS_PT, layout=0, schedule=0):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, sc.params(integrator=integrator), accel_layout=layout)
    if schedule:
        g.set_schedule(schedule)
    return g


def _label(case):
    return [f"{wl:.2f} nm, {th:.3f} deg" for wl, th in SR.groups(case)]


def _input_rays(name, channels):
    case = SR.CASE[name]
    sc = SR.goniometer(case)
    copies, passes = (DET_COPIES, DET_PASSES) if case.opaque else (COPIES, PASSES)
    pos, dr, grp = SR.goniometer_rays(sc, case, copies)
    assert pos.shape[0] <= sc.width * sc.height
    p, value = SR.expected(sc, case, pos, dr)
    out = np.zeros((pos.shape[0], channels), np.float32)
    _gpu(sc).PathTraceFromInputRaysBlock(pos.shape[0], channels, pos, dr, out, passes)
    c = min(channels, SR.channels(case))
    what = f"{name}, {channels} channel(s)"
    if case.opaque:
        SR.check_deterministic(out[:, :c], value, passes, SR.EPS, what)
    else:
        SR.check_two_valued(out[:, :c], p, value, grp, _label(case), passes, SR.EPS, what)


# ---- input rays -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("name", RGB)
def test_input_rays_rgb(name, channels):
    _input_rays(name, channels)


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("name", SPECTRAL)
def test_input_rays_spectral(name, channels):
    """The wavelength travels in the ray position's fourth float; the outputs are the raw samples."""
    _input_rays(name, channels)


# ---- the Snell target ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SNELL)
def test_snell_target(name):
    """Every refracted sample of a ray aimed at the strip's centre line is the refracted weight times the emission, every sample of the same ray moved
    3 w sideways is exactly 0: a refraction angle wrong by 1e-4 rad moves the landing point by a strip's half-width or more."""
    case = SR.CASE[name]
    sc = SR.snell_target(case)
    g = _gpu(sc)
    names = [f"{wl:.2f} nm, {th:.3f} deg" for wl, th in SR.snell_groups(case)]
    rep = 587                                                              # 7 distinct rays per angle, 587 copies of each: 4109 rays, 262976 trials
    for shift in (0.0, 3 * SR.STRIP_W, -3 * SR.STRIP_W):
        pos, dr, grp = SR.snell_rays(sc, case, 7, shift)
        p, value = SR.snell_expected(sc, case, pos, dr)
        pos, dr, grp, p, value = (np.ascontiguousarray(np.repeat(a, rep, axis=0)) for a in (pos, dr, grp, p, value))
        assert pos.shape[0] <= sc.width * sc.height
        out = np.zeros((pos.shape[0], 4), np.float32)
        g.PathTraceFromInputRaysBlock(pos.shape[0], 4, pos, dr, out, PASSES)
        if shift == 0.0:
            SR.check_two_valued(out[:, :SR.channels(case)], 1.0 - p, value, grp, names, PASSES, SR.EPS, name + ", on target")
        else:
            assert not out.any(), f"{name}: {int(out.any(1).sum())} rays {shift / SR.STRIP_W:+.0f} w beside the target are lit"


# ---- pinhole frames of G ------------------------------------------------------------------------------------------------------------------------------
def _frame(name, schedule=0, layout=0, naive=False, channels=4, moving=False, passes=FRAME_PASSES):
    sc = SR.goniometer(SR.CASE[name], W, H, depth=SR.pinhole_depth(naive), pinhole=True, moving=moving)
    g = _gpu(sc, S.INTEGRATOR_STUPID_PT if naive else S.INTEGRATOR_MIS_PT, layout, schedule)
    img = np.zeros((H, W, channels), np.float32)
    (g.NaivePathTraceBlock if naive else g.PathTraceBlock)(g.N, channels, img, passes)
    return g, img


@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_frame_under_every_schedule(name):
    """The automatic schedule and schedules 1-4 on the flat layout (the automatic layout of G's 4 triangles is the sweep, which only the megakernel
    walks): the interval check on each, and every served schedule's frame and generators equal schedule 1's bit for bit (a pixel is held by one
    lane or slot that adds its passes in order)."""
    g1, img1 = _frame(name, schedule=1, layout=2)
    assert g1.last_launch()["schedule"] == 1
    SR.check_pinhole_frame(img1, name, FRAME_PASSES, f"{name}, schedule 1")
    # automatic: the megakernel (a tree this small); 3: the block-local pools, which have no film kernel; 4: the one-launch wavefront is for lean
    # gltf scenes and hands G to the megakernel (set_schedule)
    want = {0: 1, 2: 2, 3: 1 if SR.CASE[name].kind == "film" else 3, 4: 1}
    for schedule in (0, 2, 3, 4):
        g, img = _frame(name, schedule=schedule, layout=2)
        served = g.last_launch()["schedule"]
        print(f"{name}: schedule {schedule} served by {served}")
        assert served == want[schedule], f"schedule {schedule} was served by {served}"
        SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, schedule {schedule} (served by {served})")
        assert np.array_equal(img, img1), f"{name}: schedule {schedule}'s frame differs from schedule 1's in {int((img != img1).any(-1).sum())} pixels"
        assert np.array_equal(g.random_gens(), g1.random_gens())


@pytest.mark.parametrize("layout", [1, 2, 3])
@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_frame_under_every_accel_layout(name, layout):
    g, img = _frame(name, layout=layout)
    assert g.accel_info()["layout"] == ("two-level", "flat", "sweep")[layout - 1]
    SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, accel layout {layout}")


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_frame_of_naive_path_trace(name, channels):
    g, img = _frame(name, naive=True, channels=channels)
    SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, NaivePathTraceBlock, {channels} channel(s)")


@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_frame_of_a_moving_instance_with_equal_keys(name):
    """The plane as a moving instance whose two key matrices are equal: the MOTION kernels on the same values."""
    g, img = _frame(name, moving=True)
    SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, moving instance")


@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_frame_through_the_camera_plugin_loop(name):
    from hydracore3_amd.api import CAM_PINHOLE, CamRays
    sc = SR.goniometer(SR.CASE[name], W, H, pinhole=True)
    g = _gpu(sc)
    cam = CamRays(g, CAM_PINHOLE)
    cam.SetParameters(W, H, np.asarray(list(g.params.projInv), np.float32), 0)
    cam.SetBatchSize(700)                                                  # three tiles, the last of 520 rays
    img = cam.render(FRAME_PASSES)
    SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, hpt_cam_render_dev with the pinhole")


@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
def test_qmc_records(name):
    """PathTraceBlockQMC's per-sample records: a sample that falls on a pixel wholly on an opaque quad lies in that pixel's interval; on the dielectric
    it is exactly 0 or the environment within EPS, and the number of lit samples lies within five standard deviations of [sum min R, sum max R] over the
    samples' pixels (the bound of check_pinhole_frame, per sample)."""
    import math
    sc = SR.goniometer(SR.CASE[name], W, H, pinhole=True)
    _, col, pix = _gpu(sc).render_qmc(FRAME_PASSES, frame=False, records=True)
    cls, lo, hi, p_lo, p_hi = SR.pinhole_footprints(name)
    cls, lo, hi, p_lo, p_hi = cls.reshape(-1), lo.reshape(-1, 4), hi.reshape(-1, 4), p_lo.reshape(-1), p_hi.reshape(-1)
    assert np.isfinite(col).all() and pix.max() < N
    env = np.asarray(SR.ENV[:3], np.float32)
    on = cls[pix] == SR.INSIDE
    assert on.sum() > 0.25 * on.size
    if SR.CASE[name].opaque:
        v, l, h = col[on, :3].astype(np.float64), lo[pix[on], :3], hi[pix[on], :3]
        exc = np.maximum(np.maximum((l - v) / l, (v - h) / h), 0.0)
        print(f"{name}, QMC records: {int(on.sum())} of {on.size} samples on the quad, worst excursion {exc.max():.3e}")
        assert exc.max() <= SR.EPS
    else:
        v = col[on, :3].astype(np.float64)                                  # (the reflected weight is cos * (R / cos) / R: 1 to the last bit or two)
        lit = np.all(np.abs(v - env) <= SR.EPS * env, axis=1)
        dark = np.all(v == 0.0, axis=1)
        assert np.all(lit | dark), f"{name}: {int((~(lit | dark)).sum())} records are neither 0 nor the environment"
        pl, ph = p_lo[pix[on]], p_hi[pix[on]]
        var = np.maximum(pl * (1 - pl), ph * (1 - ph))
        var[(pl < 0.5) & (ph > 0.5)] = 0.25
        slack = 5.0 * math.sqrt(var.sum()) + 1.0
        K = int(lit.sum())
        print(f"{name}, QMC records: {int(on.sum())} samples on the quad, K = {K}, allowed [{pl.sum() - slack:.1f}, {ph.sum() + slack:.1f}]")
        assert pl.sum() - slack <= K <= ph.sum() + slack
    off = cls[pix] == SR.OUTSIDE
    assert np.all(col[off, :3] == env)


def _spectral_frame(name, schedule):
    sc = SR.goniometer(SR.CASE[name], W, H, pinhole=True)
    sc.spectral_mode = 1
    sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    g = _gpu(sc, layout=2, schedule=schedule)                              # (the flat layout: see test_frame_under_every_schedule)
    img = np.zeros((H, W, 1), np.float32)
    g.PathTraceBlock(g.N, 1, img, FRAME_PASSES)
    return g, img


@pytest.mark.parametrize("schedule", [1, 3, 2], ids=["plain", "block_local", "wavefront"])
def test_frame_in_spectral_mode(schedule):
    """m_spectral_mode = 1 with one channel (the first wavelength's raw sample): the conductor's constant eta and k give the RGB case's F whatever
    wavelength a sample draws, so the RGB frame's intervals hold for the red channel. The three schedules that serve spectral mode; the frame and
    the generators of 3 and 2 equal schedule 1's bit for bit."""
    name = "conductor_0.2_3.9"
    g, img = _spectral_frame(name, schedule)
    assert g.last_launch()["schedule"] == schedule
    SR.check_pinhole_frame(img, name, FRAME_PASSES, f"{name}, spectral, schedule {schedule}")
    if schedule != 1:
        g1, img1 = _spectral_frame(name, 1)
        assert g1.last_launch()["schedule"] == 1
        assert np.array_equal(img, img1), f"spectral: schedule {schedule}'s frame differs from schedule 1's in {int((img != img1).any(-1).sum())} pixels"
        assert np.array_equal(g.random_gens(), g1.random_gens())


# ---- the device beside the oracle -------------------------------------------------------------------------------------------------------------------------
def test_device_excursions_beside_the_oracles():
    """Prints the device's worst excursion per deterministic case (4 channels) beside the oracle's on the same rays; asserts nothing the tests above
    do not."""
    from oracle.orc import OracleIntegrator
    for case in SR.CASES:
        if not case.opaque:
            continue
        sc = SR.goniometer(case)
        pos, dr, grp = SR.goniometer_rays(sc, case, DET_COPIES)
        p, value = SR.expected(sc, case, pos, dr)
        og, oc = np.zeros((pos.shape[0], 4), np.float32), np.zeros((pos.shape[0], 4), np.float32)
        _gpu(sc).PathTraceFromInputRaysBlock(pos.shape[0], 4, pos, dr, og, DET_PASSES)
        OracleIntegrator(sc, sc.params()).path_trace_from_input_rays_block(pos, dr, oc, DET_PASSES, 4)
        c = SR.channels(case)
        d, o = SR.excursion(og[:, :c], value, DET_PASSES), SR.excursion(oc[:, :c], value, DET_PASSES)
        print(f"{case.name}: worst excursion from float64 - device {d:.3e}, oracle {o:.3e} (EPS {SR.EPS:.3e})")
        assert d <= SR.EPS

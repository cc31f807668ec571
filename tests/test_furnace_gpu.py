"""Every film-writing path-tracing entry point of the device held to the closed-form radiance of two furnaces (tests/furnace_reference.py): the
integrating sphere S, where every sample of depth D is rho / pi * I * sum_{k < D} rho^k / |x_k|^2, and the cavity C under a constant sky, where
every sample is 0 or env * rho^k. Neither the oracle nor another device run is the reference here. Figures: profiles/furnace.md.

S: every pixel's sum / its passes lies in [V_lo (1 - EPS), V_hi (1 + EPS)]; pixels outside are counted against CAP of the run's samples (a pixel
outside holds at least one sample outside). C: every sample of a one-pass frame classifies; a four-pass frame is the sum of four one-pass frames
from the same generators, bit for bit: under every schedule a pixel is held by one lane (megakernel, block-local pools: PIX += per pass, stored once)
or one slot (wavefront: outColor[pixel] += per pass) that adds its passes in order. The one family that does not add in order is QMC, whose
samples reach the film by float atomics from any lane; it is held to the frame mean on S only.

Spectral mode (one channel, grey walls), the PathTraceDR / PathTraceVJP frames and KMLT's frame mean run on S as well."""
import numpy as np
import pytest

import furnace_reference as FR
from hydracore3_amd import scene as S

pytestmark = pytest.mark.gpu

PASSES = 4                                   # S never runs with fewer: CAP of 1920 x 4 samples is 7 pixels, the scene's own leaks are 1.5 per such run
W, H, N = FR.WIDTH, FR.HEIGHT, FR.WIDTH * FR.HEIGHT


def _gpu(sc, integrator=S.INTEGRATOR_MIS_PT, layout=0, schedule=0):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, sc.params(integrator=integrator), accel_layout=layout)
    if schedule:
        g.set_schedule(schedule)
    return g


def _pix(g):
    """tid -> index of its pixel in a [H * W] frame."""
    xy = g.packed_xy()
    return (xy >> 16).astype(np.int64) * g.W + (xy & 0xFFFF)


def _assert_sphere(values, passes, depth, what, albedo=FR.ALBEDO, sc=None):
    """values [m, c] sums of `passes` (scalar or [m]) samples each, c = 1 (the red channel), 3 or 4."""
    lo, hi = FR.sphere_interval(sc if sc is not None else FR.sphere_scene(depth), depth, albedo)
    v = np.asarray(values, np.float64).reshape(-1, values.shape[-1])
    p = np.broadcast_to(np.asarray(passes, np.float64).reshape(-1, 1), (v.shape[0], 1))
    out = FR.outside_interval(v[:, :3] / p, lo, hi)
    samples = float(p.sum())
    print(f"{what}: {int(out.sum())} of {v.shape[0]} pixels ({samples:.0f} samples) outside the interval; worst excursion "
          f"{float(FR.interval_excursion(v[:, :3] / p, lo, hi).max()):.3e}")
    assert out.sum() <= FR.CAP * samples, f"{what}: {int(out.sum())} pixels outside [{lo}, {hi}], first {np.nonzero(out)[0][:5]}: {(v[:, :3] / p)[out][:5]}"


def _assert_cavity(frame, kmax, what):
    """frame [..., c] of single samples, c = 1 (the red channel), 3 or 4."""
    f = np.asarray(frame)
    if f.shape[-1] == 1:
        k, ok = FR.classify_red_frame(f[..., 0], kmax)
    else:
        k, ok = FR.classify_frame(f, kmax)
    print(f"{what}: {int((~ok).sum())} of {ok.size} samples are no env * rho^k; powers seen {sorted(set(np.unique(k).astype(int).tolist()))}")
    assert (~ok).sum() <= FR.CAP * ok.size, f"{what}: {int((~ok).sum())} samples are no env * rho^k, first {f[~ok][:5]}"
    if ok.size == N:                                                      # a full frame: primary misses and every power up to k_max occur
        assert set(range(kmax + 1)) <= set(np.unique(k).tolist()), f"{what}: powers seen {np.unique(k)}"
    else:
        assert len(np.unique(k)) >= kmax, what
    return ok


def _sphere_frame(depth, passes=PASSES, channels=4, integrator=S.INTEGRATOR_MIS_PT, layout=0, schedule=0, setup=None):
    sc = FR.sphere_scene(depth)
    g = _gpu(sc, integrator, layout, schedule)
    if setup:
        setup(g)
    img = np.zeros((H, W, channels), np.float32)
    g.PathTraceBlock(g.N, channels, img, passes)
    return g, img


def _cavity_frames(channels=4, naive=False, layout=0, schedule=0, begin=0, count=N):
    """(four one-pass frames, the four-pass frame from the same generators, served schedule)."""
    sc = FR.cavity_scene()
    integ = S.INTEGRATOR_STUPID_PT if naive else S.INTEGRATOR_MIS_PT
    run = lambda g, img, n: (g.NaivePathTraceBlock if naive else g.PathTraceBlock)(count, channels, img, n, tid_begin=begin)
    g = _gpu(sc, integ, layout, schedule)
    ones = []
    for _ in range(4):
        img = np.zeros((H, W, channels), np.float32)
        run(g, img, 1)
        ones.append(img)
    served = g.last_launch()["schedule"]
    g4 = _gpu(sc, integ, layout, schedule)
    four = np.zeros((H, W, channels), np.float32)
    run(g4, four, 4)
    assert np.array_equal(g.random_gens(), g4.random_gens())
    return ones, four, served


def _assert_cavity_run(ones, four, served, kmax, what):
    oks = [_assert_cavity(f, kmax, f"{what}, one-pass frame {i}") for i, f in enumerate(ones)]
    total = ((ones[0] + ones[1]) + ones[2]) + ones[3]                     # float32, in pass order
    exact = np.array_equal(total, four)
    print(f"{what}: served by schedule {served}; the four-pass frame is {'bit for bit' if exact else 'NOT bit for bit'} the in-order sum")
    assert exact, f"{what}: the four-pass frame is not the in-order sum of its passes ({int((total != four).any(-1).sum())} pixels differ)"


# ---- depths and integrator types --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", [S.INTEGRATOR_MIS_PT, S.INTEGRATOR_SHADOW_PT], ids=["mis", "shadow"])
@pytest.mark.parametrize("depth", FR.DEPTHS)
def test_sphere_at_every_depth(depth, integ):
    g, img = _sphere_frame(depth, integrator=integ)
    _assert_sphere(img.reshape(-1, 4), PASSES, depth, f"S depth {depth}, integrator {integ}, schedule {g.last_launch()['schedule']}")


# ---- schedules ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("depth", [3, 6])
def test_sphere_under_every_schedule(schedule, depth):
    g, img = _sphere_frame(depth, schedule=schedule)
    served = g.last_launch()["schedule"]
    assert served == (schedule or 3), f"schedule {schedule} was served by {served}"   # (automatic: the block-local pools, by the tree's SAH estimate)
    _assert_sphere(img.reshape(-1, 4), PASSES, depth, f"S depth {depth}, schedule {schedule} (served by {served})")


@pytest.mark.parametrize("schedule", [0, 1, 2, 3, 4])
def test_cavity_under_every_schedule(schedule):
    ones, four, served = _cavity_frames(schedule=schedule)
    # schedule 4 (the one-launch wavefront) is for heavy gltf / emissive scenes and hands the 90 triangles of C to the megakernel (set_schedule)
    assert served == {0: 3, 1: 1, 2: 2, 3: 3, 4: 1}[schedule], f"schedule {schedule} was served by {served}"
    _assert_cavity_run(ones, four, served, FR.k_max(), f"C, schedule {schedule}")


# ---- accel layouts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [1, 2, 3])
def test_sphere_under_every_accel_layout(layout):
    g, img = _sphere_frame(2, layout=layout)
    assert g.accel_info()["layout"] == ("two-level", "flat", "sweep")[layout - 1]
    _assert_sphere(img.reshape(-1, 4), PASSES, 2, f"S depth 2, accel layout {layout}")


@pytest.mark.parametrize("layout", [1, 2, 3])
def test_cavity_under_every_accel_layout(layout):
    ones, four, served = _cavity_frames(layout=layout)
    _assert_cavity_run(ones, four, served, FR.k_max(), f"C, accel layout {layout}")


# ---- tid windows ----------------------------------------------------------------------------------------------------------------------------
BEGIN, COUNT = 37, 1000                      # starts in the first wave, ends 13 lanes into the seventeenth


def test_sphere_tid_window_inside_waves():
    sc = FR.sphere_scene(3)
    g = _gpu(sc)
    img = np.zeros((H, W, 4), np.float32)
    g.PathTraceBlock(COUNT, 4, img, PASSES, tid_begin=BEGIN)
    pix = _pix(g)
    flat = img.reshape(-1, 4)
    inside = np.zeros(N, bool); inside[pix[BEGIN:BEGIN + COUNT]] = True
    assert inside.sum() == COUNT and not flat[~inside].any()
    _assert_sphere(flat[inside], PASSES, 3, "S depth 3, tid window")


def test_cavity_tid_window_inside_waves():
    ones, four, served = _cavity_frames(begin=BEGIN, count=COUNT)
    g = _gpu(FR.cavity_scene())
    inside = np.zeros(N, bool); inside[_pix(g)[BEGIN:BEGIN + COUNT]] = True
    for f in ones + [four]:
        assert not f.reshape(-1, 4)[~inside].any()
    sel = lambda f: f.reshape(-1, 4)[inside]
    _assert_cavity_run([sel(f) for f in ones], sel(four), served, FR.k_max(), "C, tid window")


# ---- channels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_sphere_channels(channels):
    g, img = _sphere_frame(3, channels=channels)
    _assert_sphere(img.reshape(-1, channels), PASSES, 3, f"S depth 3, {channels} channel(s)")


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_cavity_channels(channels):
    ones, four, served = _cavity_frames(channels=channels)
    for i, f in enumerate(ones):
        _assert_cavity(f, FR.k_max(), f"C, {channels} channel(s), frame {i}")
    assert np.array_equal(((ones[0] + ones[1]) + ones[2]) + ones[3], four)


# ---- NaivePathTraceBlock ----------------------------------------------------------------------------------------------------------------------
def test_naive_sphere_is_exactly_black():
    sc = FR.sphere_scene(3)
    g = _gpu(sc, S.INTEGRATOR_STUPID_PT)
    img = np.zeros((H, W, 4), np.float32)
    g.NaivePathTraceBlock(g.N, 4, img, PASSES)
    assert not img.any()


def test_naive_cavity_reaches_one_bounce_further():
    ones, four, served = _cavity_frames(naive=True)
    kmax = FR.k_max(naive=True)
    _assert_cavity_run(ones, four, served, kmax, "C, NaivePathTraceBlock")
    assert max(int(FR.classify_frame(f, kmax)[0].max()) for f in ones) == kmax == FR.k_max() + 1


# ---- PathTraceFromInputRaysBlock ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [4, 1])
def test_sphere_from_input_rays(channels):
    sc = FR.sphere_scene(3)
    g = _gpu(sc)
    pos, dr = FR.sphere_input_rays(N - 77)                                # not a multiple of the wave
    out = np.zeros((pos.shape[0], channels), np.float32)
    g.PathTraceFromInputRaysBlock(pos.shape[0], channels, pos, dr, out, PASSES)
    _assert_sphere(out, PASSES, 3, f"S depth 3, input rays, {channels} channel(s)")


# ---- pass slices and the mailbox hand-over --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_", [1, 3, 5])
def test_sphere_in_pass_slices(slice_):
    """8 passes in slices of 1, 3 and 5 (a short last slice) on 1920 pixels, far fewer than lanes: every slice after a pixel's first takes the pixel
    from the mailbox. A dropped or doubled pass moves a pixel by 12 % or more."""
    def setup(g):
        g.set_schedule(1)
        g.set_option("pass_slice", slice_)
    g, img = _sphere_frame(6, passes=8, setup=setup)
    ll = g.last_launch()
    assert ll["schedule"] == 1 and ll["pass_slice"] == slice_, ll
    _assert_sphere(img.reshape(-1, 4), 8, 6, f"S depth 6, 8 passes in slices of {slice_}")


# ---- adaptive counts ----------------------------------------------------------------------------------------------------------------------------
def test_sphere_with_per_pixel_counts():
    from hydracore3_amd.api import MOMENTS_DTYPE
    sc = FR.sphere_scene(3)
    g = _gpu(sc)
    tid = np.arange(N)
    counts = np.array([0, 1, 3, 8], np.uint32)[(tid // 3 + tid // 50) % 4]  # runs of three lanes: every wave holds all four counts
    pix = _pix(g)
    img = np.zeros((H, W, 4), np.float32)
    flat = img.reshape(-1, 4)
    flat[pix[counts == 0]] = 7.0
    mom = np.zeros(N, MOMENTS_DTYPE)
    want = counts.copy()
    g.PathTraceBlockCounts(N, 4, img, 5, counts, mom)
    assert np.array_equal(mom["passes"], want)
    assert np.all(flat[pix[want == 0]] == 7.0) and not mom["sumY"][want == 0].any()
    lit = want > 0
    _assert_sphere(flat[pix[lit]], want[lit], 3, "S depth 3, counts 0 / 1 / 3 / 8")
    lo, hi = FR.sphere_interval(sc)
    y = mom["sumY"][lit].astype(np.float64) / want[lit]
    out = (y < FR.luminance(lo) * (1 - FR.EPS)) | (y > FR.luminance(hi) * (1 + FR.EPS))
    assert out.sum() <= FR.CAP * want.sum(), f"{int(out.sum())} moments records outside the interval's luminance"


# ---- QMC ----------------------------------------------------------------------------------------------------------------------------------------
def test_sphere_qmc_frame_mean():
    """Samples scatter over the frame: the sum over all pixels / the sample count lies in the interval; no pixel is negative or non-finite."""
    from hydracore3_amd.api import qmc_sample_count
    sc = FR.sphere_scene(3)
    g = _gpu(sc)
    img, _, _ = g.render_qmc(PASSES)
    assert np.isfinite(img).all() and (img >= 0).all()
    mean = img[..., :3].astype(np.float64).sum((0, 1)) / qmc_sample_count(N, PASSES)
    lo, hi = FR.sphere_interval(sc)
    print("S depth 3, QMC: frame mean", mean, "interval", lo, hi)
    assert not FR.outside_interval(mean[None, :], lo, hi)[0], (mean, lo, hi)


# ---- the camera plug-in loop ----------------------------------------------------------------------------------------------------------------------
def test_sphere_through_the_camera_plugin_loop():
    from hydracore3_amd.api import CAM_PINHOLE, CamRays
    sc = FR.sphere_scene(3)
    g = _gpu(sc)
    cam = CamRays(g, CAM_PINHOLE)
    cam.SetParameters(W, H, np.asarray(list(g.params.projInv), np.float32), 0)
    cam.SetBatchSize(700)                                                  # three tiles, the last of 520 rays
    img = cam.render(PASSES)
    _assert_sphere(img.reshape(-1, 4), PASSES, 3, "S depth 3, hpt_cam_render_dev with the pinhole")


# ---- spectral mode --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 3, 2], ids=["plain", "block_local", "wavefront"])
def test_sphere_in_spectral_mode(schedule):
    """m_spectral_mode = 1 with one channel (the first wavelength's sample): grey walls and a white light, so that whatever reading of an RGB colour
    the spectral path takes gives rho = 0.5 and I."""
    sc = FR.sphere_scene(3, albedo=FR.GREY)
    sc.spectral_mode = 1
    sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    g = _gpu(sc, schedule=schedule)
    img = np.zeros((H, W, 1), np.float32)
    g.PathTraceBlock(g.N, 1, img, PASSES)
    assert g.last_launch()["schedule"] == schedule
    _assert_sphere(img.reshape(-1, 1), PASSES, 3, f"S depth 3, spectral, schedule {schedule}", albedo=FR.GREY, sc=sc)


# ---- the frames of PathTraceDR and PathTraceVJP ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dr", "vjp"])
def test_sphere_frame_of_the_differentiable_calls(which):
    """One constant 4 x 4 texture registered on the wall's material, its texel the albedo (the material's own colour is 1)."""
    sc = FR.sphere_scene(3, albedo=(1.0, 1.0, 1.0))
    tex = np.zeros((4, 4, 4), np.float32)
    tex[..., :3], tex[..., 3] = FR.ALBEDO, 1.0
    tid = sc.add_texture(S.Texture(tex, S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_WRAP, S.FILTER_LINEAR))
    sc.materials[0]["texid"][0] = tid
    g = _gpu(sc)
    off, size = g.PutDiffTex2D(tid, 4, 4, 4)
    assert size == tex.size
    data = np.zeros(off + size, np.float32)
    data[off:off + size] = tex.reshape(-1)
    img = np.zeros((H, W, 4), np.float32)
    if which == "dr":
        g.PathTraceDR(g.N, 4, img, PASSES, np.zeros_like(img), data, np.zeros_like(data))
    else:
        g.PathTraceVJP(g.N, 4, img, PASSES, None, data, None)
    _assert_sphere(img.reshape(-1, 4), PASSES, 3, f"S depth 3, the frame of {which}")


# ---- KMLT ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [4, 64])
def test_sphere_kmlt_frame_mean(spp):
    """The contribution function is constant up to the interval's width, so the normalisation must return V: the frame's mean / spp lies in the
    interval. No margin is added: the oracle has no KMLT entry point to measure one on (profiles/furnace.md)."""
    sc = FR.sphere_scene(3)
    r = _gpu(sc).render_kmlt(spp)
    f = r["frame"][..., :3].astype(np.float64)
    assert np.isfinite(f).all() and (f >= 0).all()
    mean = f.mean((0, 1)) / spp
    lo, hi = FR.sphere_interval(sc)
    print(f"S depth 3, KMLT at {spp} spp ({r['chains']} chains x {r['steps']} steps): frame mean / spp", mean, "interval", lo, hi)
    assert not FR.outside_interval(mean[None, :], lo, hi)[0], (mean, lo, hi)

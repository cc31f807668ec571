"""Adaptive sampling under m_spectral_mode (hpt_set_option "adaptive_spectral"; DESIGN.md 2.13, "Spectral form").

A pixel's generator is its own (m_randomGens[tid]) and the spectral kernels keep one pixel on one lane or pool slot for all its passes, so a pixel given
k passes must hold, bit for bit, what a uniform k-pass spectral PathTraceBlock leaves there - frame and generator: the feature is held to kernels that
exist without it. The records are held to the numpy restatement (tests/adaptive_reference.py) over samples replayed by uniform one-pass calls, the
wavefront form to the megakernel form, the loop to its rounds driven by hand, and the chain behind it to tests/denoise_var_reference.py. Every
comparison is on uint32 views.

Not covered: the refusal of input rays. No entry point hands input rays to an adaptive call (the counts entries take none), so that branch of the
host's one check cannot be reached through the ABI."""
import ctypes as C

import numpy as np
import pytest

import adaptive_reference as R
import denoise_var_reference as V
from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

W, H = 40, 24                                        # 960 tids: three full blocks and one of 192 lanes; the tile swizzle has a seam
NAN_PAYLOAD = np.uint32(0x7FC12345)
LIMIT = 0xFFFFFF                                     # passes a pool slot's status word holds
ZERO_WAVE = 2                                        # tids 128 .. 191 of the frame: a whole wave without a pass


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counts(n, seed=7):
    """Counts in 0 .. 9 from a fixed seed: they vary inside every wave, at least one pixel in eight has none, and one whole wave has none."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 10, n).astype(np.uint32)
    c[rng.random(n) < 0.12] = 0
    c[64 * ZERO_WAVE:64 * (ZERO_WAVE + 1)] = 0
    c[[10, 77]] = 9
    assert (c == 0).mean() >= 1.0 / 8.0 and c.max() == 9
    for w in range(n // 64):
        assert len(np.unique(c[64 * w:64 * (w + 1)])) >= (1 if w == ZERO_WAVE else 6), w
    return c


def _prefill(h, w, channels, seed=3):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    flat = _bits(img).reshape(-1, channels)
    flat[::5, 0] = NAN_PAYLOAD                                            # a NaN with a payload and a negative zero, on pixels of every count
    flat[1::7, channels - 1] = np.uint32(0x80000000)
    return img


def _prefilled_moments(n):
    from hydracore3_amd.api import MOMENTS_DTYPE
    mom = np.zeros(n, MOMENTS_DTYPE)
    mom["sumY"], mom["sumY2"], mom["passes"] = 1.5, 2.5, 3
    return mom


def _scene(name, w=W, h=H):
    """The scenes of tests/test_kmlt_spectral_gpu.py under m_spectral_mode: the reference's spectral fixture, a dispersive sphere at depth 3, thin
    films, a moving instance; and a deep tree for the HBM half of the stacks."""
    if name == "moving":
        from test_qmc_spectral_gpu import _emitter_scene
        return _emitter_scene(w, h, motion=True)
    if name == "nested_sheets":
        from traversal_scenes import nested_sheets
        return nested_sheets(width=w, height=h, spectral=True)
    sc = load_hydra_xml(scene_path(name), w, h, spectral=True)
    if name == "spectral_glass":
        sc.trace_depth = 3
    return sc


def _gpu(name, layout=0, on=True, w=W, h=H):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene(name, w, h), accel_layout=layout)
    assert g.scene.spectral_mode
    if on:
        g.set_option("adaptive_spectral", 1)
    return g


def _uniform_refs(g, gens0, prefill, channels, begin, count, ks):
    """{k: (frame, gens)} of the uniform spectral PathTraceBlock with k passes over the window, each from the same generators into the same frame."""
    refs = {}
    for k in sorted(set(int(k) for k in ks)):
        g.set_random_gens(gens0)
        img = prefill.copy()
        if k:
            g.PathTraceBlock(count, channels, img, k, tid_begin=begin)
        refs[k] = (img, g.random_gens())
    return refs


def _assert_counts_equal_uniform(g, got_img, got_gens, counts, refs, gens0, prefill, begin, count, channels, what):
    xy = g.packed_xy()
    pix = (xy >> 16) * np.uint32(g.W) + (xy & 0xFFFF)
    gb = _bits(got_img).reshape(-1, channels)
    want = _bits(prefill).reshape(-1, channels).copy()
    want_gens = gens0.copy()
    for k, (img, gens) in refs.items():
        sel = np.arange(begin, begin + count)[counts[begin:begin + count] == k]
        want[pix[sel]] = _bits(img).reshape(-1, channels)[pix[sel]]
        want_gens[sel] = gens[sel]
    bad = np.nonzero((gb != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} pixels differ from the uniform calls, first {bad[:5]}"
    badg = np.nonzero((got_gens != want_gens).any(axis=1))[0]
    assert badg.size == 0, f"{what}: {badg.size} generators differ from the uniform calls, first {badg[:5]}"


def _counts_case(name, channels, layout=0, begin=0, count=W * H):
    g = _gpu(name, layout)
    gens0 = g.random_gens()
    counts = _counts(g.N)
    prefill = _prefill(H, W, channels)
    refs = _uniform_refs(g, gens0, prefill, channels, begin, count, np.unique(counts[begin:begin + count]))
    g.set_random_gens(gens0)
    img, mom = prefill.copy(), _prefilled_moments(g.N)
    g.PathTraceBlockCounts(count, channels, img, 5, counts, mom, tid_begin=begin)     # (passNum is not read when counts are given)
    ll = g.last_launch()
    assert ll["schedule"] == 1 and ll["pass_slice"] == 0, ll
    _assert_counts_equal_uniform(g, img, g.random_gens(), counts, refs, gens0, prefill, begin, count, channels, f"{name}, {channels} ch, layout {layout}")
    inside = np.zeros(g.N, bool); inside[begin:begin + count] = True
    before = _prefilled_moments(g.N)
    assert np.array_equal(mom["passes"], before["passes"] + np.where(inside, counts, 0))
    untouched = ~inside | (counts == 0)
    assert mom[untouched].tobytes() == before[untouched].tobytes(), "a pixel without a pass lost its record"
    assert (mom["sumY"][~untouched] != np.float32(1.5)).any()
    return g, ll


# ---- 1. a pixel with k passes is a uniform k-pass pixel --------------------------------------------------------------------------------------
CASES = [("test_spectral", 4, 0), ("test_spectral", 3, 0), ("test_spectral", 1, 0), ("test_spectral", 4, 1), ("test_spectral", 4, 2), ("test_spectral", 4, 3),
         ("spectral_glass", 4, 0), ("thin_film", 4, 0), ("moving", 4, 0), ("nested_sheets", 4, 0), ("typed_materials", 4, 0), ("env_map", 4, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels,layout", CASES, ids=[f"{n}-{c}ch-layout{l}" for n, c, l in CASES])
def test_pixel_with_k_passes_is_a_uniform_k_pass_pixel(name, channels, layout):
    """The references are uniform spectral PathTraceBlock calls in whatever schedule the context chooses for them (the three spectral forms render the
    same bits: tests/test_gpu_spectral.py); the counts call is asserted to run the one-thread-per-pixel kernel. Which ADAPT instantiation a case
    runs follows from the host's rule (launch_path_trace): test_spectral the narrowest scope on the automatic, two-level, single-level and sweep
    layouts, spectral_glass a dispersive dielectric (paths that keep one wavelength), thin_film the film branches, `moving` the MOTION
    instantiation (asserted on the scene), nested_sheets DEEP (asserted). The scope is not observable through the ABI and is stated, not asserted:
    by the host's rule the scenes above take scopes 0 and 1, typed_materials (glass, blends, plastic: more than three material types) scope 2,
    built for 3 waves per SIMD, and env_map (an environment map over few material types) scope 2 at 4 waves - units adaptive_spectral_wide and
    _wide4. The layout a case asks for is asserted. Pixels with count 0 keep a prefilled frame, their generator and a prefilled record (asserted
    in _counts_case)."""
    g, ll = _counts_case(name, channels, layout)
    if layout:
        assert g.accel_info()["layout"] == ("two-level", "flat", "sweep")[layout - 1], g.accel_info()
    if name == "nested_sheets":
        assert ll["deep_stack"], ll
    if name == "moving":
        assert g.scene.inst_motion


@pytest.mark.gpu
def test_window_that_neither_starts_nor_ends_on_a_wave():
    _counts_case("test_spectral", 4, begin=5, count=300)


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------------------------
def _per_sample(g, gens0, channels, passes):
    """The samples of every pixel, pass by pass: chained uniform one-pass spectral calls into zeroed frames -> [passes, N (tid order), channels]."""
    xy = g.packed_xy()
    pix = (xy >> 16) * np.uint32(g.W) + (xy & 0xFFFF)
    g.set_random_gens(gens0)
    out = []
    for _ in range(passes):
        img = np.zeros((g.H, g.W, channels), np.float32)
        g.PathTraceBlock(g.N, channels, img, 1)
        out.append(img.reshape(-1, channels)[pix])
    return np.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels", [("test_spectral", 4), ("test_spectral", 1), ("test_spectral", 3), ("spectral_glass", 4), ("thin_film", 4)])
def test_moments_are_the_luminance_sums_of_the_samples(name, channels):
    """A sample's three frame values are exposure * rgb after the camera response (its one value with channels == 1): a one-pass call into a zeroed
    frame shows them, 0 + v being v. The record must be their Rec. 709 luminance summed in f32 in pass order."""
    from hydracore3_amd.api import MOMENTS_DTYPE
    g = _gpu(name)
    gens0 = g.random_gens()
    first, second = _counts(g.N), _counts(g.N, seed=11)[::-1].copy()
    samples = _per_sample(g, gens0, channels, 18)
    ys = samples[..., 0] if channels == 1 else R.luminance(samples[..., :3])
    # from zeroed records ...
    want = R.accumulate(np.zeros(g.N, R.MOMENTS_DTYPE), [(ys[p], first > p) for p in range(9)])
    g.set_random_gens(gens0)
    frame, mom = np.zeros((H, W, channels), np.float32), np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, channels, frame, 0, first, mom)
    assert mom.tobytes() == want.tobytes(), np.nonzero(mom != want.view(MOMENTS_DTYPE))[0][:8]
    assert mom["sumY"].sum() > 0 and np.array_equal(mom["passes"], first)
    # ... and on from them: the second call's q-th sample of a pixel is the pixel's (first + q)-th
    idx = np.minimum(first[None, :].astype(np.int64) + np.arange(9)[:, None], 17)
    ys2 = np.take_along_axis(ys, idx, axis=0)
    want = R.accumulate(want, [(ys2[q], second > q) for q in range(9)])
    g.PathTraceBlockCounts(g.N, channels, frame, 0, second, mom)
    assert mom.tobytes() == want.tobytes(), np.nonzero(mom != want.view(MOMENTS_DTYPE))[0][:8]
    # from prefilled records
    want = R.accumulate(_prefilled_moments(g.N).view(R.MOMENTS_DTYPE), [(ys[p], first > p) for p in range(9)])
    g.set_random_gens(gens0)
    mom = _prefilled_moments(g.N)
    g.PathTraceBlockCounts(g.N, channels, np.zeros((H, W, channels), np.float32), 0, first, mom)
    assert mom.tobytes() == want.tobytes(), np.nonzero(mom != want.view(MOMENTS_DTYPE))[0][:8]
    # 3 passes then 5 on the same records = one 8-pass call = the restatement over 8 samples
    g.set_random_gens(gens0)
    a, fa = np.zeros(g.N, MOMENTS_DTYPE), np.zeros((H, W, channels), np.float32)
    g.PathTraceBlockCounts(g.N, channels, fa, 3, None, a)
    g.PathTraceBlockCounts(g.N, channels, fa, 5, None, a)
    g.set_random_gens(gens0)
    b, fb = np.zeros(g.N, MOMENTS_DTYPE), np.zeros((H, W, channels), np.float32)
    g.PathTraceBlockCounts(g.N, channels, fb, 8, None, b)
    want8 = R.accumulate(np.zeros(g.N, R.MOMENTS_DTYPE), [(ys[p], np.ones(g.N, bool)) for p in range(8)])
    assert a.tobytes() == b.tobytes() == want8.tobytes()
    assert np.array_equal(_bits(fa), _bits(fb))


@pytest.mark.gpu
def test_null_moments_and_null_counts():
    from hydracore3_amd.api import MOMENTS_DTYPE
    g = _gpu("test_spectral")
    gens0, counts = g.random_gens(), _counts(g.N)
    with_mom, mom = _prefill(H, W, 4), np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, 4, with_mom, 5, counts, mom)
    gens_with = g.random_gens()
    g.set_random_gens(gens0)
    without = _prefill(H, W, 4)
    g.PathTraceBlockCounts(g.N, 4, without, 5, counts, None)               # no records: the same frame and generators
    assert np.array_equal(_bits(without), _bits(with_mom)) and np.array_equal(g.random_gens(), gens_with)
    g.set_random_gens(gens0)
    u = _prefill(H, W, 4); g.PathTraceBlock(g.N, 4, u, 6); gens_u = g.random_gens()
    g.set_random_gens(gens0)
    v, mom6 = _prefill(H, W, 4), np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, 4, v, 6, None, mom6)                       # no counts: 6 passes everywhere = the uniform call
    assert g.last_launch()["schedule"] == 1
    assert np.array_equal(_bits(u), _bits(v)) and np.array_equal(g.random_gens(), gens_u) and (mom6["passes"] == 6).all()
    g.set_random_gens(gens0)
    x = _prefill(H, W, 4); g.PathTraceBlockCounts(g.N, 4, x, 6)            # neither
    assert np.array_equal(_bits(u), _bits(x)) and np.array_equal(g.random_gens(), gens_u)
    nothing, kept = _prefill(H, W, 4), _prefilled_moments(g.N)
    g.PathTraceBlockCounts(g.N, 4, nothing, 0, None, kept)                 # neither, and no passes: nothing runs
    assert np.array_equal(_bits(nothing), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens_u) and kept.tobytes() == _prefilled_moments(g.N).tobytes()


# ---- 3. wavefront form --------------------------------------------------------------------------------------------------------------------------
def _both_forms(name, channels, layout, counts_of):
    """The same two counts calls into the same records under hpt_set_schedule(2), "adaptive_wavefront" off and on. At 40 x 24 pixels a round queues far
    fewer rays than the trace grid has lanes, so no ray is suspended here: test_suspended_rays_keep_the_spectral_adaptive_call_exact covers that."""
    g = _gpu(name, layout)                                                  # (an explicit layout: the automatic one may pick the sweep, which the wavefront schedule does not walk)
    gens0, prefill = g.random_gens(), _prefill(H, W, channels)
    first, second = counts_of(g.N)
    out = []
    for on in (False, True):
        g.set_schedule(2, 56, 1, 1); g.set_option("wf_grace", 1)
        g.set_option("adaptive_wavefront", int(on))
        g.set_random_gens(gens0)
        img, mom = prefill.copy(), _prefilled_moments(g.N)
        g.PathTraceBlockCounts(g.N, channels, img, 5, first, mom)
        assert g.last_launch()["schedule"] == (2 if on else 1), g.last_launch()
        if on:
            assert g.last_schedule()[1] > 0
        mid = mom.copy()
        g.PathTraceBlockCounts(g.N, channels, img, 5, second, mom)
        assert g.last_launch()["schedule"] == (2 if on else 1), g.last_launch()
        out.append((img, g.random_gens(), mid, mom))
    return g, out, first, second


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels,layout", [("test_spectral", 4, 2), ("test_spectral", 1, 1), ("test_spectral", 3, 2), ("spectral_glass", 4, 2), ("spectral_glass", 4, 1),
                                                  ("typed_materials", 4, 2), ("env_map", 4, 2)])
def test_wavefront_form_equals_the_megakernel_form(name, channels, layout):
    """test_spectral and spectral_glass run wfShadeSpecKernel<1, ADAPT> (the wavefront schedule has no scope-0 shade kernel), typed_materials by the
    host's rule <2, ADAPT> and env_map <3, ADAPT> (stated, not observable: see test_pixel_with_k_passes_is_a_uniform_k_pass_pixel)."""
    g, (mega, wave), first, second = _both_forms(name, channels, layout, lambda n: (_counts(n), _counts(n, seed=11)[::-1].copy()))
    assert np.array_equal(_bits(wave[0]), _bits(mega[0])), "frames"
    assert np.array_equal(wave[1], mega[1]), "generators"
    assert wave[2].tobytes() == mega[2].tobytes() and wave[3].tobytes() == mega[3].tobytes(), "moments"
    assert np.array_equal(wave[3]["passes"], 3 + first + second)
    zero = (first == 0) & (second == 0)
    assert zero.any() and wave[3][zero].tobytes() == _prefilled_moments(g.N)[zero].tobytes()


def _interior(spectral):
    """The scene of test_adaptive_wavefront_gpu.test_suspended_rays_keep_the_adaptive_call_exact; under m_spectral_mode as the benchmark's interior is:
    gltf colours carried as four samples, a uniform spectrum in the table."""
    from hydracore3_amd import synth
    sc = synth.interior_scene(384, 320, objects=24, subdiv=2, tex_size=64)
    if spectral:
        sc.spectral_mode = 1
        sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    return sc


@pytest.mark.gpu
def test_suspended_rays_keep_the_spectral_adaptive_call_exact():
    """384 x 320 pixels under hpt_set_schedule(2, 56, 1, 1) and grace 1: one trace block per CU, so a round queues more than twice as many rays as the
    trace grid has lanes, the trace waves suspend rays when their queue runs dry, the rays are resumed in a later round and pixels with a ray in
    flight sit rounds out in wfShadeSpecKernel<.., ADAPT>. Frame, generators and records must equal the megakernel form's. Adaptive calls refuse the
    instrumented probe and so does the spectral wavefront schedule, so the witness that rays are suspended in this configuration is a uniform
    instrumented one-pass call on an RGB context of the same scene, whose rays the same trace kernel walks: a condition of the test."""
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_interior(True), accel_layout=2)
    g.set_option("adaptive_spectral", 1)
    gens0 = g.random_gens()
    counts = np.random.default_rng(5).choice(np.array([0, 1, 3], np.uint32), g.N).astype(np.uint32)
    res = []
    for on in (False, True):
        g.set_schedule(2, 56, 1, 1); g.set_option("wf_grace", 1)
        g.set_option("adaptive_wavefront", int(on))
        g.set_random_gens(gens0)
        img, mom = np.zeros((320, 384, 4), np.float32), np.zeros(g.N, MOMENTS_DTYPE)
        g.PathTraceBlockCounts(g.N, 4, img, 0, counts, mom)
        assert g.last_launch()["schedule"] == (2 if on else 1)
        res.append((img, g.random_gens(), mom))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(res[0][1], res[1][1]) and res[0][2].tobytes() == res[1][2].tobytes()
    assert np.array_equal(res[1][2]["passes"], counts) and res[1][2]["sumY"].sum() > 0
    w = HipIntegrator(_interior(False), accel_layout=2); w.set_schedule(2, 56, 1, 1); w.set_option("wf_grace", 1)
    w.set_instrumentation(True)
    w.render(1)
    suspended = list(w.counters().values())[12]
    assert suspended > 0, suspended


@pytest.mark.gpu
def test_loop_limit_holds_only_where_the_wavefront_form_is_reachable():
    """A moving instance has no spectral wavefront kernel, so every round of its loop runs the megakernel and a step past the status word is no error."""
    m = _gpu("moving", 1); m.set_schedule(2); m.set_option("adaptive_wavefront", 1)
    info = m.PathTraceBlockAdaptive(m.N, 4, np.zeros((H, W, 4), np.float32), 1, None, **dict(LOOP, step=LIMIT + 1, max_passes=LIMIT + 1))
    assert m.last_launch()["schedule"] == 1 and info["rounds"] >= 1


@pytest.mark.gpu
def test_wavefront_form_needs_both_options_and_a_schedule_that_allows_it():
    from hydracore3_amd.api import MOMENTS_DTYPE
    g = _gpu("test_spectral", 2)
    counts = _counts(g.N)
    for schedule, wave_opt, want in ((2, 0, 1), (2, 1, 2), (1, 1, 1), (3, 1, 1), (0, 1, 1)):     # (0: the automatic rule keeps this light scene on the megakernel)
        g.set_schedule(schedule); g.set_option("adaptive_wavefront", wave_opt)
        g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 0, counts, np.zeros(g.N, MOMENTS_DTYPE))
        assert g.last_launch()["schedule"] == want, (schedule, wave_opt, g.last_launch())
    # a moving instance has no spectral wavefront kernel: the call keeps the megakernel under either option
    m = _gpu("moving", 1); m.set_schedule(2); m.set_option("adaptive_wavefront", 1)
    m.PathTraceBlockCounts(m.N, 4, np.zeros((H, W, 4), np.float32), 0, counts, None)
    assert m.last_launch()["schedule"] == 1


@pytest.mark.gpu
def test_count_above_the_status_word_is_refused_and_nothing_is_written():
    from hydracore3_amd.api import HydraHipError
    g = _gpu("test_spectral", 2)
    gens0 = g.random_gens()
    g.set_schedule(2); g.set_option("adaptive_wavefront", 1)
    counts = _counts(g.N)
    counts[300] = LIMIT + 1
    frame, mom = _prefill(H, W, 4), _prefilled_moments(g.N)
    with pytest.raises(HydraHipError, match="hydra_hip error 1: adaptive sampling.*0xFFFFFF"):
        g.PathTraceBlockCounts(g.N, 4, frame, 0, counts, mom)
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()
    d_frame, d_cnt, d_mom = g.dev_array(frame), g.dev_array(counts.view(np.float32)), g.dev_array(mom.view(np.float32).reshape(-1, 4))
    try:                                                                    # the device form: the caller's own arrays
        with pytest.raises(HydraHipError, match="hydra_hip error 1: adaptive sampling.*0xFFFFFF"):
            g.PathTraceBlockCounts_dev(d_frame.ptr, 0, d_cnt.ptr, d_mom.ptr)
        assert np.array_equal(_bits(d_frame.download()), _bits(frame)) and d_mom.download().tobytes() == mom.tobytes() and np.array_equal(g.random_gens(), gens0)
    finally:
        d_frame.free(); d_cnt.free(); d_mom.free()
    with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockAdaptive.*0xFFFFFF"):
        g.PathTraceBlockAdaptive(g.N, 4, frame, 2, mom, **dict(LOOP, step=LIMIT + 1, max_passes=LIMIT + 1))
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()


@pytest.mark.gpu
def test_all_zero_counts_launch_no_round():
    g = _gpu("test_spectral", 2)
    g.set_schedule(2); g.set_option("adaptive_wavefront", 1)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 0, _counts(g.N), None)
    assert g.last_launch()["schedule"] == 2 and g.last_schedule()[1] > 0
    gens0 = g.random_gens()
    frame, mom = _prefill(H, W, 4), _prefilled_moments(g.N)
    g.PathTraceBlockCounts(g.N, 4, frame, 5, np.zeros(g.N, np.uint32), mom)
    assert g.last_launch()["schedule"] == 2
    assert g.last_schedule()[1] == 0
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()


# ---- 4. the loop --------------------------------------------------------------------------------------------------------------------------------
LOOP = dict(tol=0.05, lum_floor=0.05, min_passes=2, max_passes=24, step=4, dilate=1)


def _replay(g, gens0, channels, max_rounds, prm):
    """The loop by hand through the low-level entries: zeroed records, min_passes, then plan and counts calls until the plan is empty."""
    from hydracore3_amd.api import MOMENTS_DTYPE
    g.set_random_gens(gens0)
    img = _prefill(g.H, g.W, channels)
    mom = np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, channels, img, prm["min_passes"], None, mom)
    rounds, spent, rnd = 1, prm["min_passes"] * g.N, 0
    while True:
        counts, info = g.AdaptivePlan(mom, **prm)
        if info["passes"] == 0 or rnd >= max_rounds:
            break
        g.PathTraceBlockCounts(g.N, channels, img, 0, counts, mom)
        rounds += 1; spent += info["passes"]; rnd += 1
    return img, g.random_gens(), mom, dict(passes=spent, pixels=info["pixels"], maxPasses=info["maxPasses"], nonfinite=info["nonfinite"], rounds=rounds)


def _loop(g, gens0, channels, max_rounds):
    from hydracore3_amd.api import MOMENTS_DTYPE
    g.set_random_gens(gens0)
    img, mom = _prefill(g.H, g.W, channels), np.ones(g.N, MOMENTS_DTYPE)   # (stale records: the loop zeroes the window)
    info = g.PathTraceBlockAdaptive(g.N, channels, img, max_rounds, mom, **LOOP)
    info.pop("deviceMs")
    return img, g.random_gens(), mom, info


@pytest.mark.gpu
def test_loop_equals_its_rounds_replayed_by_hand_in_both_forms():
    g = _gpu("test_spectral", 2)
    gens0 = g.random_gens()
    for max_rounds in (8, 1):
        want = _replay(g, gens0, 4, max_rounds, LOOP)
        got = _loop(g, gens0, 4, max_rounds)
        assert g.last_launch()["schedule"] == 1
        print("adaptive spectral loop:", got[3])
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
        assert got[3] == want[3], (got[3], want[3])
        assert (got[2]["passes"] >= LOOP["min_passes"]).all() and (got[2]["passes"] <= LOOP["max_passes"]).all()
        assert got[3]["passes"] == int(got[2]["passes"].astype(np.uint64).sum())
        if max_rounds == 8:
            assert got[3]["rounds"] >= 2, "no planned round ran: the test compares nothing beyond a uniform call"
            assert len(np.unique(got[2]["passes"])) > 1
        g.set_schedule(2); g.set_option("adaptive_wavefront", 1)
        wave = _loop(g, gens0, 4, max_rounds)
        assert g.last_launch()["schedule"] == 2
        g.set_schedule(0); g.set_option("adaptive_wavefront", 0)
        assert np.array_equal(_bits(wave[0]), _bits(got[0])) and np.array_equal(wave[1], got[1]) and wave[2].tobytes() == got[2].tobytes()
        assert wave[3] == got[3], (wave[3], got[3])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
REFUSED = "hydra_hip error 4: adaptive sampling.*not served for"


def _assert_dev_loop_refused_untouched(g, match, channels=4):
    """The device form of the loop with the caller's own records: a refusal is made before the records are zeroed."""
    from hydracore3_amd.api import HydraHipError
    gens0 = g.random_gens()
    frame = _prefill(g.H, g.W, channels)
    mom = _prefilled_moments(g.N)
    d_frame, d_mom = g.dev_array(frame), g.dev_array(mom.view(np.float32).reshape(-1, 4))
    try:
        with pytest.raises(HydraHipError, match=match):
            g.PathTraceBlockAdaptive_dev(d_frame.ptr, 2, d_mom.ptr, channels=channels, **LOOP)
        assert np.array_equal(_bits(d_frame.download()), _bits(frame)), "a refused loop wrote the frame"
        assert d_mom.download().tobytes() == mom.tobytes(), "a refused loop touched the caller's records"
        assert np.array_equal(g.random_gens(), gens0)
    finally:
        d_frame.free(); d_mom.free()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["layers", "naive", "instrumented", "rgb_thin_film"])
def test_what_has_no_kernel_is_refused_with_the_option_set(what):
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    if what == "rgb_thin_film":
        g = HipIntegrator(load_hydra_xml(scene_path("thin_film"), W, H, spectral=False))
        g.set_option("adaptive_spectral", 1)
    else:
        g = _gpu("test_spectral")
    if what == "instrumented":
        g.set_instrumentation(True)
    channels = 5 if what == "layers" else 4
    gens0 = g.random_gens()
    frame, mom = _prefill(H, W, channels), _prefilled_moments(g.N)
    before = frame.copy()
    with pytest.raises(HydraHipError, match=REFUSED + (".*wavelength layers" if what == "layers" else "")):
        if what == "naive":
            d = g.dev_array(frame)
            try:
                g.PathTraceBlockCounts_dev(d.ptr, 2, naive=True)
            finally:
                frame = d.download(); d.free()
        else:
            g.PathTraceBlockCounts(g.N, channels, frame, 2, _counts(g.N), mom)
    assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()
    if what != "naive":                                                     # (the loop has no naive form)
        with pytest.raises(HydraHipError, match=REFUSED):
            g.PathTraceBlockAdaptive(g.N, channels, frame, 2, mom, **LOOP)
        assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()
        _assert_dev_loop_refused_untouched(g, REFUSED, channels)


@pytest.mark.gpu
def test_option_takes_0_or_1_and_0_refuses_again():
    from hydracore3_amd.api import HydraHipError
    g = _gpu("test_spectral", on=False)
    for bad in (2, -1):
        with pytest.raises(HydraHipError, match="hydra_hip error 1"):
            g.set_option("adaptive_spectral", bad)
    gens0 = g.random_gens()
    frame, mom = _prefill(H, W, 4), _prefilled_moments(g.N)
    with pytest.raises(HydraHipError, match=REFUSED + " m_spectral_mode"):   # the refused values left the default
        g.PathTraceBlockCounts(g.N, 4, frame, 2, None, mom)
    g.set_option("adaptive_spectral", 1)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 2)
    assert g.last_launch()["schedule"] == 1
    g.set_option("adaptive_spectral", 0)
    g.set_random_gens(gens0)
    with pytest.raises(HydraHipError, match=REFUSED + " m_spectral_mode"):
        g.PathTraceBlockCounts(g.N, 4, frame, 2, _counts(g.N), mom)
    with pytest.raises(HydraHipError, match=REFUSED + " m_spectral_mode"):
        g.PathTraceBlockAdaptive(g.N, 4, frame, 2, mom, **LOOP)
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()
    _assert_dev_loop_refused_untouched(g, REFUSED + " m_spectral_mode")


# ---- 6. down the chain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spectral_adaptive_frame_goes_down_the_chain_on_the_device():
    """The adaptive loop on a spectral context, then AdaptiveResolve, AdaptiveVariance, EvalGBuffer and DenoiseFrameVar, every array resident on the
    device: the filter's output equals tests/denoise_var_reference.py run on the downloaded inputs, so nothing behind the sampler needs to know
    that the frame was rendered with four wavelengths per path."""
    from hydracore3_amd.api import GBUFFER_DTYPE, MOMENTS_DTYPE
    from test_denoise_var_gpu import var_params_of
    g = _gpu("test_spectral")
    n, vp = g.N, C.c_void_p
    sizes = dict(frame=n * 16, mom=n * 16, var=n * 4, gb=n * 60, out=n * 16, out_var=n * 4)
    d = {k: vp() for k in sizes}
    for k, nbytes in sizes.items():
        g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(d[k])))
    try:
        g._chk(g.L.hpt_device_memset(g.h, d["frame"], 0, n * 16))
        info = g.PathTraceBlockAdaptive_dev(d["frame"], 2, d["mom"], tol=0.25, lum_floor=0.05, min_passes=2, max_passes=8, step=16, dilate=1)
        g.AdaptiveResolve_dev(d["frame"], d["mom"], d["frame"])
        g.AdaptiveVariance_dev(d["mom"], d["var"])
        g._chk(g.L.hpt_eval_gbuffer_dev(g.h, n, d["gb"], None, None))
        g.denoise_var_dev(d["frame"], d["gb"], d["var"], d["out"], d["out_var"])
        frame, out = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        var, out_var = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        gb, mom = np.zeros((H, W), GBUFFER_DTYPE), np.zeros(n, MOMENTS_DTYPE)
        for host, key in ((frame, "frame"), (out, "out"), (var, "var"), (out_var, "out_var"), (gb, "gb"), (mom, "mom")):
            g._chk(g.L.hpt_device_copy(g.h, host.ctypes.data, d[key], host.nbytes, 2))       # synchronous copies on the null stream: after the kernels
    finally:
        for p in d.values():
            g.L.hpt_device_free(g.h, p)
    print("adaptive spectral loop:", info, "passes", np.unique(mom["passes"]))
    assert mom["passes"].min() >= 2 and mom["passes"].max() <= 8 and len(np.unique(mom["passes"])) > 1, "the pass counts do not differ between pixels"
    assert np.isfinite(var).all() and len(np.unique(var)) > 16 and np.isfinite(frame).all() and frame[..., :3].mean() > 0
    assert np.array_equal(_bits(var), _bits(V.variance_of_mean(mom, g.packed_xy(), 0, n, W, H).reshape(H, W))), "variance plane vs restatement"
    assert np.array_equal(_bits(g.AdaptiveVariance(mom)), _bits(var)), "host-pointer AdaptiveVariance vs device form"
    host, host_v = g.denoise_var(frame, var, gb, return_variance=True)
    assert np.array_equal(_bits(host), _bits(out)) and np.array_equal(_bits(host_v), _bits(out_var)), "host-pointer form vs device-pointer form"
    want, want_v = V.denoise_var(frame, gb, var, **var_params_of({}))
    assert np.array_equal(_bits(out), _bits(want)), "device vs restatement"
    assert np.array_equal(_bits(out_var), _bits(want_v)), "device vs restatement: outVar"

"""Adaptive sampling on the device: per-pixel pass counts, luminance moments, the planner, the resolve and the loop.

The generator stream of a pixel is its own (m_randomGens[tid]), so a pixel given k passes must hold, bit for bit, what a uniform k-pass
PathTraceBlock call leaves there - frame and generator: the feature is held to the existing kernels, and the planner / resolve to the numpy
restatement in tests/adaptive_reference.py, everything bit for bit."""
import numpy as np
import pytest

import adaptive_reference as R
from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

W, H = 33, 17                                        # 561 pixels: eight full waves and one of 49 lanes; tile size 1
KS = (0, 1, 2, 3, 7, 64)
NAN_PAYLOAD = np.uint32(0x7FC12345)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counts(n, seed=7):
    """Counts from KS with a fixed seed; one pixel at 64 among neighbours (in tid order) at 0."""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array(KS[:-1], np.uint32), n).astype(np.uint32)
    c[n // 2 - 3:n // 2 + 4] = 0
    c[n // 2] = 64
    c[[10, 77]] = 64
    return c


def _prefill(h, w, channels, seed=3):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 2.0, (h, w, channels)).astype(np.float32)
    flat = _bits(img).reshape(-1, channels)
    flat[::5, 0] = NAN_PAYLOAD                                            # a NaN with a payload and a negative zero, on pixels of every count
    flat[1::7, channels - 1] = np.uint32(0x80000000)
    return img


def _scene(name, w=W, h=H):
    if name == "material_zoo":
        from hydracore3_amd import synth
        return synth.material_zoo(w, h)
    if name == "nested_sheets":
        from traversal_scenes import nested_sheets
        return nested_sheets(width=w, height=h)
    return load_hydra_xml(scene_path(name), w, h)


def _uniform_refs(g, gens0, prefill, channels, begin, count, ks):
    """{k: (frame, gens)} of PathTraceBlock with k passes over the window, each from the same generators into the same pre-filled frame."""
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


def _counts_case(name, channels, layout=0, begin=0, count=W * H, moments=False, setup=None):
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    sc = _scene(name)
    g = HipIntegrator(sc, accel_layout=layout)
    if setup:
        setup(g)
    gens0 = g.random_gens()
    counts = _counts(g.N)
    prefill = _prefill(H, W, channels)
    refs = _uniform_refs(g, gens0, prefill, channels, begin, count, np.unique(counts[begin:begin + count]))
    g.set_random_gens(gens0)
    img = prefill.copy()
    mom = np.zeros(g.N, MOMENTS_DTYPE) if moments else None
    g.PathTraceBlockCounts(count, channels, img, 5, counts, mom, tid_begin=begin)     # (passNum is not read when counts are given)
    ll = g.last_launch()
    assert ll["schedule"] == 1 and ll["pass_slice"] == 0, ll
    _assert_counts_equal_uniform(g, img, g.random_gens(), counts, refs, gens0, prefill, begin, count, channels, f"{name}, {channels} ch, layout {layout}")
    if moments:
        inside = np.zeros(g.N, bool); inside[begin:begin + count] = True
        assert np.array_equal(mom["passes"], np.where(inside, counts, 0))
    return g, ll


# ---- 1. a pixel with k passes is a uniform k-pass pixel --------------------------------------------------------------------------------------
def _force_full(g):
    g.set_option("force_full_materials", 1)


CASES = [("test_035", 4, 0, None), ("test_035", 1, 0, None), ("test_035", 3, 0, None), ("test_035", 4, 0, _force_full), ("test_228", 4, 1, None), ("test_228", 4, 2, None),
         ("material_zoo", 4, 1, None), ("material_zoo", 4, 2, None), ("typed_materials", 4, 0, None), ("env_map", 4, 0, None), ("legacy_materials", 4, 0, None),
         ("nested_sheets", 4, 0, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels,layout,setup", CASES, ids=[f"{n}-{c}ch-layout{l}{'-full' if s else ''}" for n, c, l, s in CASES])
def test_pixel_with_k_passes_is_a_uniform_k_pass_pixel(name, channels, layout, setup):
    """Which ADAPT instantiation a case runs follows from the host's rule (launch_path_trace); hpt_get_last_launch shows the layout's side of it
    (shading records = lean kernel on the single-level layout; the HBM part of the stacks = DEEP) and that is asserted; the MODE is not observable
    through the ABI and is stated here, not asserted:
      test_035            the lean kernel (MODE 3), sweep; with force_full_materials the kernel with every BSDF branch, sweep
      test_228            the lean kernel on the forced two-level and single-level layouts (asserted: shading records on the single-level one only)
      material_zoo        every BSDF branch (asserted: no shading records on the single-level layout, i.e. not the lean kernel), both layouts
      typed_materials,    every BSDF branch at 3 or at 4 waves per SIMD, whichever the scene's material-type count selects (MODE 0 / MODE 7:
      env_map             the rule sends scenes with at most three material types to MODE 7) - between them both groups are meant to run
      legacy_materials    a moving instance (asserted on the scene): the MOTION instantiation
      nested_sheets       DEEP (asserted)
    Not reached by any case: the moving-instance kernels with DEEP or on the single-level layout, and DEEP together with every BSDF branch."""
    g, ll = _counts_case(name, channels, layout, setup=setup)
    if name == "nested_sheets":
        assert ll["deep_stack"], ll
    if name == "legacy_materials":
        assert g.scene.inst_motion
    if name == "test_228":
        assert ll["shade_records"] == (layout == 2), ll
    if name == "material_zoo":
        assert not ll["shade_records"], ll


@pytest.mark.gpu
def test_window_that_does_not_start_on_a_wave():
    _counts_case("test_035", 4, begin=5, count=300)


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------------------------
def _per_sample(g, gens0, channels, passes):
    """The samples of every pixel, pass by pass: chained one-pass PathTraceBlock calls into zeroed frames -> [passes, N (tid order), channels]."""
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
@pytest.mark.parametrize("name,channels", [("test_035", 4), ("test_035", 1), ("typed_materials", 3)])
def test_moments_are_the_luminance_sums_of_the_samples(name, channels):
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_scene(name))
    gens0 = g.random_gens()
    counts = np.minimum(_counts(g.N), 7).astype(np.uint32)
    samples = _per_sample(g, gens0, channels, 8)
    ys = samples[..., 0] if channels == 1 else R.luminance(samples[..., :3])
    want = R.accumulate(np.zeros(g.N, R.MOMENTS_DTYPE), [(ys[p], counts > p) for p in range(7)])
    g.set_random_gens(gens0)
    mom = np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, channels, np.zeros((H, W, channels), np.float32), 0, counts, mom)
    assert mom.tobytes() == want.tobytes(), np.nonzero(mom != want.view(MOMENTS_DTYPE))[0][:8]
    assert mom["sumY"].sum() > 0
    # 3 passes then 5 passes on the same records = one 8-pass call = the restatement over 8 samples
    g.set_random_gens(gens0)
    a = np.zeros(g.N, MOMENTS_DTYPE); fa = np.zeros((H, W, channels), np.float32)
    g.PathTraceBlockCounts(g.N, channels, fa, 3, None, a)
    g.PathTraceBlockCounts(g.N, channels, fa, 5, None, a)
    g.set_random_gens(gens0)
    b = np.zeros(g.N, MOMENTS_DTYPE); fb = np.zeros((H, W, channels), np.float32)
    g.PathTraceBlockCounts(g.N, channels, fb, 8, None, b)
    want8 = R.accumulate(np.zeros(g.N, R.MOMENTS_DTYPE), [(ys[p], np.ones(g.N, bool)) for p in range(8)])
    assert a.tobytes() == b.tobytes() == want8.tobytes()
    assert np.array_equal(_bits(fa), _bits(fb))


@pytest.mark.gpu
def test_null_moments_and_uniform_counts_leave_frame_and_generators_alone():
    _counts_case("test_035", 4, moments=True)
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_035"))
    gens0 = g.random_gens()
    a = np.zeros((H, W, 4), np.float32); g.PathTraceBlock(g.N, 4, a, 6); ga = g.random_gens()
    g.set_random_gens(gens0)
    b = np.zeros((H, W, 4), np.float32); g.PathTraceBlockCounts(g.N, 4, b, 6)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(ga, g.random_gens())


# ---- 3. planner and resolve against the restatement --------------------------------------------------------------------------------------------
PLAN = dict(tol=0.05, lum_floor=0.01, min_passes=4, max_passes=40, step=16)


def _crafted(n):
    m = np.zeros(n, R.MOMENTS_DTYPE)
    c = R.crafted_records()
    m[:len(c)] = c
    m[200:200 + len(c)] = c
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("window", [(0, W * H), (37, 401)])
def test_planner_equals_the_restatement(dilate, window):
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_scene("test_035"))
    xy = g.packed_xy()
    rendered = np.zeros(g.N, MOMENTS_DTYPE)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 0, np.minimum(_counts(g.N), 7).astype(np.uint32), rendered)
    for what, mom in (("crafted", _crafted(g.N).view(MOMENTS_DTYPE)), ("rendered", rendered)):
        counts, info = g.AdaptivePlan(mom, tid=window[1], tid_begin=window[0], dilate=dilate, **PLAN)
        wc, wi = R.plan(mom, xy, window[0], window[1], W, H, PLAN["tol"], PLAN["lum_floor"], PLAN["min_passes"], PLAN["max_passes"], PLAN["step"], dilate)
        assert np.array_equal(counts, wc), (what, np.nonzero(counts != wc)[0][:8])
        assert {k: info[k] for k in wi} == wi, (what, info, wi)
        assert info["rounds"] == 0 and info["passes"] > 0
    if dilate:                                                             # the need image's effect: dilation only ever raises a count's source
        c0, _ = g.AdaptivePlan(rendered, tid=window[1], tid_begin=window[0], dilate=0, **dict(PLAN, step=1 << 30, max_passes=1 << 30))
        c1, _ = g.AdaptivePlan(rendered, tid=window[1], tid_begin=window[0], dilate=1, **dict(PLAN, step=1 << 30, max_passes=1 << 30))
        assert (c1 >= c0).all() and (c1 > c0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_resolve_equals_the_restatement_in_and_out_of_place(channels):
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_scene("test_035"))
    xy = g.packed_xy()
    mom = np.zeros(g.N, MOMENTS_DTYPE)
    mom["passes"] = _counts(g.N)                                           # (with pixels at 0)
    frame = _prefill(H, W, channels, seed=11)
    for begin, count in ((0, g.N), (37, 401)):
        out0 = _prefill(H, W, channels, seed=12)
        want = R.resolve(frame.reshape(-1), mom, xy, begin, count, W, channels, out=out0.copy().reshape(-1))
        got = g.AdaptiveResolve(frame.copy(), mom, out=out0.copy(), tid=count, tid_begin=begin)
        assert np.array_equal(_bits(got).reshape(-1), _bits(want))
        want_in = R.resolve(frame.reshape(-1), mom, xy, begin, count, W, channels)
        got_in = g.AdaptiveResolve(frame.copy(), mom, tid=count, tid_begin=begin)
        assert np.array_equal(_bits(got_in).reshape(-1), _bits(want_in))


# ---- 4. the loop --------------------------------------------------------------------------------------------------------------------------------
LOOP = dict(tol=0.25, lum_floor=0.05, min_passes=4, max_passes=48, step=16, dilate=1)


def _replay(g, gens0, channels, max_rounds, prm):
    """The loop by hand through the low-level entries."""
    from hydracore3_amd.api import MOMENTS_DTYPE
    g.set_random_gens(gens0)
    img = np.zeros((g.H, g.W, channels), np.float32)
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


@pytest.mark.gpu
def test_loop_equals_its_rounds_replayed_by_hand():
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(load_hydra_xml(scene_path("test_035"), 64, 64))
    gens0 = g.random_gens()
    for max_rounds in (8, 1):
        want = _replay(g, gens0, 4, max_rounds, LOOP)
        g.set_random_gens(gens0)
        img, mom = np.zeros((64, 64, 4), np.float32), np.ones(g.N, MOMENTS_DTYPE)      # (stale records: the loop zeroes the window)
        info = g.PathTraceBlockAdaptive(g.N, 4, img, max_rounds, mom, **LOOP)
        print("adaptive loop:", info)
        assert np.array_equal(_bits(img), _bits(want[0])) and np.array_equal(g.random_gens(), want[1]) and mom.tobytes() == want[2].tobytes()
        assert {k: info[k] for k in want[3]} == want[3], (info, want[3])
        assert (mom["passes"] >= LOOP["min_passes"]).all() and (mom["passes"] <= LOOP["max_passes"]).all()
        assert info["passes"] == int(mom["passes"].astype(np.uint64).sum())
        assert g.last_launch()["schedule"] == 1
    assert info["rounds"] == 2 and mom["passes"].max() > LOOP["min_passes"]
    # the same without a caller's array: the records live with the context
    g.set_random_gens(gens0)
    img2 = np.zeros((64, 64, 4), np.float32)
    info2 = g.PathTraceBlockAdaptive(g.N, 4, img2, 1, None, **LOOP)
    assert np.array_equal(_bits(img2), _bits(img)) and info2["passes"] == info["passes"]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["huge_tol", "no_rounds"])
def test_loop_that_asks_for_nothing_is_a_uniform_call(how):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(load_hydra_xml(scene_path("test_035"), 64, 64))
    gens0 = g.random_gens()
    ref = np.zeros((64, 64, 4), np.float32); g.PathTraceBlock(g.N, 4, ref, LOOP["min_passes"]); gref = g.random_gens()
    g.set_random_gens(gens0)
    img = np.zeros((64, 64, 4), np.float32)
    prm = dict(LOOP, tol=1e18) if how == "huge_tol" else LOOP
    info = g.PathTraceBlockAdaptive(g.N, 4, img, 8 if how == "huge_tol" else 0, None, **prm)
    assert np.array_equal(_bits(img), _bits(ref)) and np.array_equal(g.random_gens(), gref)
    assert info["rounds"] == 1 and info["passes"] == LOOP["min_passes"] * g.N
    assert info["pixels"] == 0 if how == "huge_tol" else info["pixels"] > 0


# ---- 5. options do not leak in ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("option", ["pass_slice", "schedule 2", "schedule 3", "schedule 4"])
def test_pass_slice_and_schedules_do_not_reach_the_adaptive_call(option):
    def setup(g):
        if option == "pass_slice":
            g.set_option("pass_slice", 2)
        else:
            g.set_schedule(int(option.split()[1]))
    _counts_case("test_035", 4, setup=setup)           # (asserts schedule 1 and whole pixels; the uniform references run under the option)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["spectral", "thin_film", "naive"])
def test_unsupported_calls_are_refused_and_leave_the_frame(what):
    from hydracore3_amd.api import HipIntegrator, HydraHipError, MOMENTS_DTYPE
    name = {"spectral": "test_spectral", "thin_film": "thin_film", "naive": "test_035"}[what]
    g = HipIntegrator(load_hydra_xml(scene_path(name), W, H, spectral=(what == "spectral")))
    gens0 = g.random_gens()
    frame = _prefill(H, W, 4)
    before = frame.copy()
    mom = np.zeros(g.N, MOMENTS_DTYPE)
    with pytest.raises(HydraHipError, match="hydra_hip error 4: adaptive sampling.*not served for"):
        if what == "naive":
            d = g.dev_array(frame)
            try:
                g.PathTraceBlockCounts_dev(d.ptr, 2, naive=True)
            finally:
                frame = d.download(); d.free()
        else:
            g.PathTraceBlockCounts(g.N, 4, frame, 2, None, mom)
    assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0) and not mom["passes"].any()
    if what != "naive":
        with pytest.raises(HydraHipError, match="hydra_hip error 4"):
            g.PathTraceBlockAdaptive(g.N, 4, frame, 2, None, **LOOP)
        assert np.array_equal(_bits(frame), _bits(before))
        _assert_dev_loop_refused_untouched(g, "hydra_hip error 4: adaptive sampling.*not served for")


def _assert_dev_loop_refused_untouched(g, match):
    """The device form of the loop with the caller's own records: a refusal is made before the records are zeroed."""
    from hydracore3_amd.api import HydraHipError, MOMENTS_DTYPE
    gens0 = g.random_gens()
    frame = _prefill(g.H, g.W, 4)
    mom = np.zeros(g.N, MOMENTS_DTYPE)
    mom["sumY"], mom["sumY2"], mom["passes"] = 1.5, 2.5, 3
    d_frame, d_mom = g.dev_array(frame), g.dev_array(mom.view(np.float32).reshape(-1, 4))
    try:
        with pytest.raises(HydraHipError, match=match):
            g.PathTraceBlockAdaptive_dev(d_frame.ptr, 2, d_mom.ptr, **LOOP)
        assert np.array_equal(_bits(d_frame.download()), _bits(frame)), "a refused loop wrote the frame"
        assert d_mom.download().tobytes() == mom.tobytes(), "a refused loop touched the caller's records"
        assert np.array_equal(g.random_gens(), gens0)
    finally:
        d_frame.free(); d_mom.free()


@pytest.mark.gpu
def test_loop_is_refused_under_a_tid_interleave():
    """hpt_set_tid_interleave with stride > 1 makes a render visit every stride-th chunk, far outside the contiguous window the loop zeroes, plans and
    counts: both loop entries and the host counts form refuse it, and nothing is written. Stride 1 restores them."""
    from hydracore3_amd.api import HipIntegrator, HydraHipError, MOMENTS_DTYPE
    g = HipIntegrator(load_hydra_xml(scene_path("test_035"), 64, 64))
    gens0 = g.random_gens()
    g.set_tid_interleave(1024, 2)
    frame = _prefill(64, 64, 4)
    before = frame.copy()
    mom = np.ones(g.N, MOMENTS_DTYPE)
    with pytest.raises(HydraHipError, match="hydra_hip error 4: PathTraceBlockAdaptive.*contiguous"):
        g.PathTraceBlockAdaptive(1024, 4, frame, 2, mom, **LOOP)
    with pytest.raises(HydraHipError, match="hydra_hip error 4: PathTraceBlockCounts"):
        g.PathTraceBlockCounts(1024, 4, frame, 2, None, mom)
    assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == np.ones(g.N, MOMENTS_DTYPE).tobytes()
    _assert_dev_loop_refused_untouched(g, "hydra_hip error 4: PathTraceBlockAdaptive.*contiguous")
    g.set_tid_interleave(0, 1)
    info = g.PathTraceBlockAdaptive(g.N, 4, np.zeros((64, 64, 4), np.float32), 1, None, **LOOP)
    assert info["rounds"] >= 1 and info["passes"] >= LOOP["min_passes"] * g.N


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [dict(tol=0.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(lum_floor=-1.0), dict(lum_floor=float("inf")), dict(min_passes=0),
                                 dict(min_passes=9, max_passes=8), dict(step=0), dict(dilate=2)])
def test_bad_parameters_are_argument_errors(bad):
    from hydracore3_amd.api import HipIntegrator, HydraHipError, MOMENTS_DTYPE
    g = HipIntegrator(_scene("test_035"))
    frame = np.zeros((H, W, 4), np.float32)
    with pytest.raises(HydraHipError, match="hydra_hip error 1"):
        g.AdaptivePlan(np.zeros(g.N, MOMENTS_DTYPE), **dict(LOOP, **bad))
    with pytest.raises(HydraHipError, match="hydra_hip error 1"):
        g.PathTraceBlockAdaptive(g.N, 4, frame, 2, None, **dict(LOOP, **bad))
    assert not frame.any()

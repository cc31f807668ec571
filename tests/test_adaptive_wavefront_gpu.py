"""Adaptive sampling on the wavefront schedule (hpt_set_option "adaptive_wavefront"; DESIGN.md 2.13, "Wavefront form").

The arithmetic per path is the same function in both schedules and a pool slot owns its pixel's generator for all its passes, so the new form is
held bit for bit to kernels that exist without it: a pixel given k passes to a uniform k-pass PathTraceBlock under the megakernel, moments, the
suspended-ray path and the loop to the same calls with the option off (the megakernel's ADAPT kernels). Every comparison is on uint32 views."""
import numpy as np
import pytest

from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

W, H = 33, 17                                        # 561 pixels: eight full waves and one of 49 lanes, one group
KS = (0, 1, 2, 3, 7, 64)
NAN_PAYLOAD = np.uint32(0x7FC12345)
LIMIT = 0xFFFFFF                                     # passes a pool slot's status word holds


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counts(n, seed=7):
    """Counts from KS with a fixed seed; one pixel at 64 among neighbours (in tid order) at 0 (tests/test_adaptive_gpu.py: _counts)."""
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


def _prefilled_moments(n):
    from hydracore3_amd.api import MOMENTS_DTYPE
    mom = np.zeros(n, MOMENTS_DTYPE)
    mom["sumY"], mom["sumY2"], mom["passes"] = 1.5, 2.5, 3
    return mom


def _scene(name, w=W, h=H):
    if name == "material_zoo":
        from hydracore3_amd import synth
        return synth.material_zoo(w, h)
    if name == "nested_sheets":
        from traversal_scenes import nested_sheets
        return nested_sheets(width=w, height=h)
    return load_hydra_xml(scene_path(name), w, h)


def _wavefront(g, *schedule):
    g.set_schedule(*(schedule or (2,)))
    g.set_option("adaptive_wavefront", 1)


def _uniform_refs(g, gens0, prefill, channels, begin, count, ks):
    """{k: (frame, gens)} of PathTraceBlock with k passes over the window under the megakernel, each from the same generators into the same frame."""
    g.set_schedule(1)
    refs = {}
    for k in sorted(set(int(k) for k in ks)):
        g.set_random_gens(gens0)
        img = prefill.copy()
        if k:
            g.PathTraceBlock(count, channels, img, k, tid_begin=begin)
            assert g.last_launch()["schedule"] == 1
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
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene(name), accel_layout=layout)
    gens0 = g.random_gens()
    counts = _counts(g.N)
    prefill = _prefill(H, W, channels)
    refs = _uniform_refs(g, gens0, prefill, channels, begin, count, np.unique(counts[begin:begin + count]))
    _wavefront(g)
    g.set_random_gens(gens0)
    img = prefill.copy()
    g.PathTraceBlockCounts(count, channels, img, 5, counts, None, tid_begin=begin)     # (passNum is not read when counts are given)
    ll = g.last_launch()
    assert ll["schedule"] == 2 and ll["pass_slice"] == 0, ll
    assert g.last_schedule()[1] > 0
    _assert_counts_equal_uniform(g, img, g.random_gens(), counts, refs, gens0, prefill, begin, count, channels, f"{name}, {channels} ch, layout {layout}")
    return g, ll


# ---- 1. a pixel with k passes is a uniform k-pass pixel --------------------------------------------------------------------------------------
CASES = [("test_228", 4, 1), ("test_228", 4, 2), ("test_228", 3, 0), ("test_228", 1, 0), ("material_zoo", 4, 1), ("material_zoo", 4, 2), ("env_map", 4, 0),
         ("legacy_materials", 4, 0), ("nested_sheets", 4, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels,layout", CASES, ids=[f"{n}-{c}ch-layout{l}" for n, c, l in CASES])
def test_pixel_with_k_passes_is_a_uniform_k_pass_pixel(name, channels, layout):
    """The references are uniform PathTraceBlock calls under the megakernel, an independent kernel. Which ADAPT shade kernel a case runs follows from
    the host's rule (launch_wavefront): test_228 the lean one (asserted through the shading records of the single-level layout), material_zoo and
    env_map every BSDF branch, legacy_materials the moving-instance one (asserted on the scene), nested_sheets the HBM part of the stacks."""
    g, ll = _counts_case(name, channels, layout)
    if name == "nested_sheets":
        assert ll["deep_stack"], ll
    if name == "legacy_materials":
        assert g.scene.inst_motion
    if name == "test_228" and layout:
        assert ll["shade_records"] == (layout == 2), ll


@pytest.mark.gpu
def test_window_that_does_not_start_on_a_wave():
    _counts_case("test_228", 4, begin=5, count=300)


def _counts_dev(g, gens0, prefill, counts, mom, begin, count):
    """The bare counts entry on device arrays: (frame, generators, moments) after the call."""
    g.set_random_gens(gens0)
    d_img, d_cnt, d_mom = g.dev_array(prefill), g.dev_array(counts.view(np.float32)), g.dev_array(mom.view(np.float32).reshape(-1, 4))
    try:
        g.PathTraceBlockCounts_dev(d_img.ptr, 5, d_cnt.ptr, d_mom.ptr, tid_begin=begin, tid_count=count)
        return d_img.download(), g.random_gens(), d_mom.download().view(mom.dtype).reshape(-1)
    finally:
        d_img.free(); d_cnt.free(); d_mom.free()


@pytest.mark.gpu
def test_counts_entry_serves_interleaved_tids_under_either_schedule():
    """hpt_set_tid_interleave(64, 2): item k renders tid (k / 64) * 128 + k % 64, so 320 items reach past the 561 tids of the frame and the last are
    dropped - by the init kernel, the summary and the shade kernel alike."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_228"))
    gens0, counts, prefill, mom0 = g.random_gens(), _counts(g.N), _prefill(H, W, 4), _prefilled_moments(g.N)
    g.set_tid_interleave(64, 2)
    want = _counts_dev(g, gens0, prefill, counts, mom0, 0, 320)
    assert g.last_launch()["schedule"] == 1
    _wavefront(g)
    got = _counts_dev(g, gens0, prefill, counts, mom0, 0, 320)
    assert g.last_launch()["schedule"] == 2
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
    tids = np.arange(g.N)
    visited = ((tids // 64) % 2 == 0) & (tids < 2 * 320)
    assert np.array_equal(got[2]["passes"], mom0["passes"] + np.where(visited, counts, 0))
    assert (got[1] != gens0).any(axis=1).sum() == np.count_nonzero(visited & (counts > 0))


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------------------------
def _moments_pair(name, channels, begin=0, count=W * H):
    """The same two counts calls into the same records, option off (the megakernel's ADAPT kernels) and on: [(frame, gens, moments)] * 2, counts."""
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_scene(name))
    gens0, counts, prefill = g.random_gens(), _counts(g.N), _prefill(H, W, channels)
    second = _counts(g.N, seed=11)[::-1].copy()
    out = []
    for on in (False, True):
        g.set_schedule(2)
        g.set_option("adaptive_wavefront", int(on))
        g.set_random_gens(gens0)
        img, mom = prefill.copy(), np.zeros(g.N, MOMENTS_DTYPE)
        g.PathTraceBlockCounts(count, channels, img, 5, counts, mom, tid_begin=begin)
        assert g.last_launch()["schedule"] == (2 if on else 1)
        first = mom.copy()
        g.PathTraceBlockCounts(count, channels, img, 5, second, mom, tid_begin=begin)
        assert g.last_launch()["schedule"] == (2 if on else 1)
        out.append((img, g.random_gens(), first, mom))
    return out, counts, second


@pytest.mark.gpu
@pytest.mark.parametrize("name,channels,begin,count", [("test_228", 4, 0, W * H), ("test_228", 1, 0, W * H), ("material_zoo", 3, 5, 300), ("legacy_materials", 4, 0, W * H)])
def test_moments_equal_the_megakernels(name, channels, begin, count):
    (off, on), counts, second = _moments_pair(name, channels, begin, count)
    inside = np.zeros(counts.size, bool); inside[begin:begin + count] = True
    assert np.array_equal(on[2]["passes"], np.where(inside, counts, 0))
    assert np.array_equal(on[3]["passes"], np.where(inside, counts + second, 0))
    assert on[2].tobytes() == off[2].tobytes(), np.nonzero(on[2] != off[2])[0][:8]
    assert on[3].tobytes() == off[3].tobytes(), np.nonzero(on[3] != off[3])[0][:8]
    assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(on[1], off[1])
    assert on[3]["sumY"].sum() > 0


@pytest.mark.gpu
def test_null_moments_and_null_counts_behave_as_under_the_megakernel():
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    g = HipIntegrator(_scene("test_228"))
    gens0, counts = g.random_gens(), _counts(g.N)
    res = {}
    for on in (False, True):
        g.set_schedule(2)
        g.set_option("adaptive_wavefront", int(on))
        g.set_random_gens(gens0)
        a = _prefill(H, W, 4); g.PathTraceBlockCounts(g.N, 4, a, 5, counts, None)                       # no records
        assert g.last_launch()["schedule"] == (2 if on else 1)
        ga = g.random_gens()
        b, mom = _prefill(H, W, 4), np.zeros(g.N, MOMENTS_DTYPE); g.PathTraceBlockCounts(g.N, 4, b, 6, None, mom)   # no counts: 6 passes everywhere
        assert g.last_launch()["schedule"] == (2 if on else 1)
        c = _prefill(H, W, 4); g.PathTraceBlockCounts(g.N, 4, c, 0, None, mom.copy())                    # neither, and no passes: nothing runs
        res[on] = (a, ga, b, g.random_gens(), mom, c)
    for i, (x, y) in enumerate(zip(res[False], res[True])):
        assert x.tobytes() == y.tobytes(), i
    assert (res[True][4]["passes"] == 6).all()
    assert np.array_equal(_bits(res[True][5]), _bits(_prefill(H, W, 4)))
    # ... and the uniform call of the counts entry is the uniform PathTraceBlock of the megakernel
    g.set_schedule(1); g.set_random_gens(gens0)
    u = _prefill(H, W, 4); g.PathTraceBlock(g.N, 4, u, 5); g.PathTraceBlock(g.N, 4, u, 6)
    _wavefront(g); g.set_random_gens(gens0)
    v = _prefill(H, W, 4); g.PathTraceBlockCounts(g.N, 4, v, 5); g.PathTraceBlockCounts(g.N, 4, v, 6)
    assert g.last_launch()["schedule"] == 2
    assert np.array_equal(_bits(u), _bits(v))


# ---- 3. suspended rays --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_suspended_rays_keep_the_adaptive_call_exact():
    """The configuration of test_wavefront_ray_suspension_is_exact: a small trace grid and grace 1 send rays through suspension and resumption, and
    pixels with a ray in flight sit rounds out. Adaptive calls refuse the instrumented probe, so the witness that rays are suspended here is a
    uniform instrumented one-pass call in the same configuration on a second context: a condition of the test, not a measurement."""
    from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE
    from hydracore3_amd import synth
    sc = synth.interior_scene(384, 320, objects=24, subdiv=2, tex_size=64)
    g = HipIntegrator(sc, accel_layout=2)
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
    assert np.array_equal(res[1][2]["passes"], counts)
    w = HipIntegrator(sc, accel_layout=2); w.set_schedule(2, 56, 1, 1); w.set_option("wf_grace", 1)
    w.set_instrumentation(True)
    w.render(1)
    suspended = list(w.counters().values())[12]
    assert suspended > 0, suspended


# ---- 4. the loop --------------------------------------------------------------------------------------------------------------------------------
LOOP = dict(tol=0.05, lum_floor=0.05, min_passes=2, max_passes=24, step=4, dilate=1)


def _loop(g, gens0, schedule, on):
    from hydracore3_amd.api import MOMENTS_DTYPE
    g.set_schedule(schedule)
    g.set_option("adaptive_wavefront", int(on))
    g.set_random_gens(gens0)
    img, mom = _prefill(g.H, g.W, 4), np.ones(g.N, MOMENTS_DTYPE)          # (stale records: the loop zeroes the window)
    info = g.PathTraceBlockAdaptive(g.N, 4, img, 8, mom, **LOOP)
    info.pop("deviceMs")
    return img, g.random_gens(), mom, info, g.last_launch()["schedule"]


@pytest.mark.gpu
def test_loop_is_the_megakernels_loop():
    """Every round decides for itself: the rule is useWavefront on the round's active-pixel count (the window in round 0, the plan's pixels above 0
    later). Under hpt_set_schedule(2) that is the wavefront form in every round; under (0) on this small scene it is the megakernel in every round.
    The switch between the two within one loop needs 2^19 active pixels and is left to profiles/adaptive_wavefront.md."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(load_hydra_xml(scene_path("test_228"), W, H))
    gens0 = g.random_gens()
    want = _loop(g, gens0, 2, False)
    assert want[4] == 1
    assert want[3]["rounds"] >= 3, want[3]                                 # round 0 and at least two planned rounds
    got = _loop(g, gens0, 2, True)
    assert got[4] == 2
    auto = _loop(g, gens0, 0, True)
    assert auto[4] == 1
    for r in (got, auto):
        assert np.array_equal(_bits(r[0]), _bits(want[0])) and np.array_equal(r[1], want[1]) and r[2].tobytes() == want[2].tobytes()
        assert r[3] == want[3], (r[3], want[3])


# ---- 5. the limit -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_count_above_the_status_word_is_refused_and_nothing_is_written():
    from hydracore3_amd.api import HipIntegrator, HydraHipError, MOMENTS_DTYPE
    g = HipIntegrator(_scene("test_228"))
    gens0 = g.random_gens()
    _wavefront(g)
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
    # the loop: refused where it makes its other refusals, before the caller's records are zeroed
    prm = dict(LOOP, step=LIMIT + 1, max_passes=LIMIT + 1)
    with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockAdaptive.*0xFFFFFF"):
        g.PathTraceBlockAdaptive(g.N, 4, frame, 2, mom, **prm)
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()
    d_frame, d_mom = g.dev_array(frame), g.dev_array(mom.view(np.float32).reshape(-1, 4))
    try:
        with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockAdaptive.*0xFFFFFF"):
            g.PathTraceBlockAdaptive_dev(d_frame.ptr, 2, d_mom.ptr, **prm)
        assert np.array_equal(_bits(d_frame.download()), _bits(frame)), "a refused loop wrote the frame"
        assert d_mom.download().tobytes() == mom.tobytes(), "a refused loop touched the caller's records"
    finally:
        d_frame.free(); d_mom.free()
    with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockAdaptive.*0xFFFFFF"):
        g.PathTraceBlockAdaptive(g.N, 4, frame, 2, mom, **dict(LOOP, min_passes=LIMIT + 1, max_passes=LIMIT + 2))
    assert np.array_equal(g.random_gens(), gens0)
    # where the schedule setting cannot choose the wavefront form, nothing is looked at and nothing refused here
    g.set_schedule(1)
    g.PathTraceBlockCounts(g.N, 4, frame, 0, np.zeros(g.N, np.uint32), mom)
    assert g.last_launch()["schedule"] == 1


# ---- 6. nothing to do ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_zero_counts_launch_no_round():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_228"))
    _wavefront(g)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 0, _counts(g.N), None)
    assert g.last_launch()["schedule"] == 2 and g.last_schedule()[1] > 0
    gens0 = g.random_gens()
    frame, mom = _prefill(H, W, 4), _prefilled_moments(g.N)
    g.PathTraceBlockCounts(g.N, 4, frame, 5, np.zeros(g.N, np.uint32), mom)
    assert g.last_launch()["schedule"] == 2
    assert g.last_schedule()[1] == 0
    assert np.array_equal(_bits(frame), _bits(_prefill(H, W, 4))) and np.array_equal(g.random_gens(), gens0) and mom.tobytes() == _prefilled_moments(g.N).tobytes()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["spectral", "thin_film", "naive", "instrumented"])
def test_unsupported_calls_are_refused_as_without_the_option(what):
    from hydracore3_amd.api import HipIntegrator, HydraHipError, MOMENTS_DTYPE
    name = {"spectral": "test_spectral", "thin_film": "thin_film", "naive": "test_228", "instrumented": "test_228"}[what]
    g = HipIntegrator(load_hydra_xml(scene_path(name), W, H, spectral=(what == "spectral")))
    _wavefront(g)
    if what == "instrumented":
        g.set_instrumentation(True)
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
            g.PathTraceBlockCounts(g.N, 4, frame, 2, _counts(g.N), mom)
    assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0) and not mom["passes"].any()
    if what != "naive":
        with pytest.raises(HydraHipError, match="hydra_hip error 4: adaptive sampling.*not served for"):
            g.PathTraceBlockAdaptive(g.N, 4, frame, 2, None, **LOOP)
        assert np.array_equal(_bits(frame), _bits(before)) and np.array_equal(g.random_gens(), gens0)


@pytest.mark.gpu
def test_option_takes_0_or_1():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    g = HipIntegrator(_scene("test_228"))
    with pytest.raises(HydraHipError, match="hydra_hip error 1: adaptive_wavefront"):
        g.set_option("adaptive_wavefront", 2)
    g.set_schedule(2)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 2)     # the refused value left the default: the megakernel
    assert g.last_launch()["schedule"] == 1
    g.set_option("adaptive_wavefront", 1); g.set_option("adaptive_wavefront", 0)
    g.PathTraceBlockCounts(g.N, 4, np.zeros((H, W, 4), np.float32), 2)
    assert g.last_launch()["schedule"] == 1

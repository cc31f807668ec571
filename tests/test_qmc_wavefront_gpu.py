"""PathTraceBlockQMC on the wavefront schedule (hpt_set_option "qmc_wavefront"; DESIGN.md 2.8, "Wavefront form").

A pool slot is a generator slot and runs its samples g, g + N, ... in order on the one generator, with the functions the megakernel inlines, so
the per-sample records (colour and pixel index at index s) and the generators are held bit for bit to the same call with the option at 0, from
the same generators: the existing pathTraceQmcKernel. The frame is an atomic sum under either schedule and is compared bit for bit only where the
sum is exact (colours that are small powers of two), otherwise against the float64 scatter sum of its own records. Comparisons are on uint32 views.

The frame is 33 x 17 = 561 slots (eight full waves and one of 49 lanes) everywhere but in the suspension case: a trace pass suspends nothing unless
its round holds more rays than twice its grid's lanes (wfTraceKernel), which 561 slots cannot supply, so that case runs 384 x 320 slots."""
import numpy as np
import pytest

from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

W, H = 33, 17
NAN_PAYLOAD = np.uint32(0x7FC12345)
LIMIT = 0xFFFFFF                                     # samples a pool slot's status word holds
HPT_ERR_ARG = 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(name, w=W, h=H):
    from hydracore3_amd import scene as S
    from hydracore3_amd import synth
    import test_qmc_gpu as T
    if name == "material_zoo":
        return synth.material_zoo(w, h)
    if name == "nested_sheets":
        from traversal_scenes import nested_sheets
        return nested_sheets(width=w, height=h)
    if name == "emissive_cornell":
        return T._emissive_cornell(w, h)
    if name == "sky":
        return T._sky_scene(w, h)
    if name == "lens":                                                     # a lit Cornell box through a thin lens: the dof dimensions
        sc = load_hydra_xml(scene_path("test_035"), w, h)
        sc.cam_lens_radius = 0.08
        return sc
    if name == "moving":                                                   # ... with a moving instance: the motion dimension, the MOTION kernels
        sc = load_hydra_xml(scene_path("test_035"), w, h)
        last = len(sc.inst_matrices) - 1
        sc.inst_motion[last] = np.asarray(sc.inst_matrices[last], np.float64).reshape(4, 4) @ S.translate(0.4, 0.0, 0.1)
        return sc
    return load_hydra_xml(scene_path(name), w, h)


def _gens(g, n):
    out = np.zeros((n, 2), np.uint32)
    g._chk(g.L.hpt_get_random_gens(g.h, out.ctypes.data, n))
    return out


def _call(g, on, spp, schedule=(2,), channels=4, pixels_num=None, n_gens=None, frame=True):
    """One render_qmc from freshly initialised generators: (frame, colours, pixels, generators after, last_launch, rounds)."""
    n_gens = g.N if n_gens is None else n_gens
    g.set_schedule(*schedule)
    g.set_option("qmc_wavefront", int(on))
    g.InitRandomGens(n_gens)
    img, col, pix = g.render_qmc(spp, channels=channels, frame=frame, records=True, pixels_num=pixels_num)
    return img, col, pix, _gens(g, n_gens), g.last_launch(), g.last_schedule()[1]


def _assert_same_records(on, off, what):
    bad = np.nonzero((_bits(on[1]) != _bits(off[1])).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(on[1])} sample colours differ from the megakernel's, first {bad[:5]}"
    assert np.array_equal(on[2], off[2]), f"{what}: pixel indices differ"
    badg = np.nonzero((on[3] != off[3]).any(axis=1))[0]
    assert badg.size == 0, f"{what}: {badg.size} generators differ from the megakernel's, first {badg[:5]}"


def _pair(g, spp, what, expect_on=2, **kw):
    off = _call(g, False, spp, **kw)
    assert off[4]["schedule"] == 1, off[4]
    on = _call(g, True, spp, **kw)
    assert on[4]["schedule"] == expect_on, on[4]
    if expect_on == 2:
        assert on[5] > 0 and not on[4]["shade_records"], (on[4], on[5])
    _assert_same_records(on, off, what)
    return on, off


# ---- 1. records and generators, bit for bit ---------------------------------------------------------------------------------------------------------
CASES = [("test_228", 0), ("material_zoo", 0), ("emissive_cornell", 1), ("emissive_cornell", 2), ("lens", 2), ("moving", 1), ("moving", 2), ("env_map", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("name,layout", CASES, ids=[f"{n}-layout{l}" for n, l in CASES])
def test_records_and_generators_equal_the_megakernels(name, layout, channels):
    """test_035's own layout is the triangle sweep, which keeps the megakernel: the Cornell cases force layouts 1 and 2."""
    from hydracore3_amd.api import HipIntegrator
    sc = _scene(name)
    g = HipIntegrator(sc, accel_layout=layout)
    if name == "lens":
        assert sc.cam_lens_radius > 0.0
    if name == "moving":
        assert sc.inst_motion
    if name == "env_map":
        assert sc.env_cam_back_id != 0xFFFFFFFF and sc.env_enable_sam == 1
    on, off = _pair(g, 3, f"{name}, layout {layout}, {channels} ch", channels=channels)
    assert on[1][:, 0].max() > 0.0 and len(np.unique(on[1][:, 0])) > 8       # the scene is lit and not constant
    if channels == 1:
        assert not on[1][:, 1:].any()


# ---- 2. the slot arithmetic -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_gens,pixels_num,spp", [(561, None, 3), (200, None, 3), (561, 100, 1), (1, 64, 1)],
                         ids=["N=561,S=1683", "N=200,S=1683 (uneven tail)", "N=561,S=100 (S<N)", "N=1,S=64 (one chain)"])
def test_slot_arithmetic(n_gens, pixels_num, spp):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_228"))
    assert g.N == 561
    S_ = (g.N if pixels_num is None else pixels_num) * spp
    per_slot = (S_ - np.arange(n_gens) + n_gens - 1) // n_gens
    per_slot[np.arange(n_gens) >= S_] = 0
    assert per_slot.sum() == S_
    if n_gens == 200:
        assert (per_slot[:83] == 9).all() and (per_slot[83:] == 8).all()
    g.InitRandomGens(n_gens)
    gens0 = _gens(g, n_gens)
    on, off = _pair(g, spp, f"N = {n_gens}, S = {S_}", pixels_num=pixels_num, n_gens=n_gens)
    assert len(on[1]) == S_
    idle = per_slot == 0
    assert np.array_equal(on[3][idle], gens0[idle]), "a generator without a sample was written"
    assert (on[3][~idle] != gens0[~idle]).any(axis=1).all()
    if n_gens == 561 and pixels_num == 100:
        assert idle.sum() == 461 and np.array_equal(on[3][100:], gens0[100:])


# ---- 3. the frame -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("channels", [4, 3, 1])
def test_frame_of_the_constant_scene_equals_the_megakernels_bit_for_bit(channels):
    """The sky scene of test_qmc_gpu.py: every sample adds the same small powers of two, so the atomic sums are exact in any order."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("sky"), accel_layout=2)                          # (its own layout is the triangle sweep, which keeps the megakernel)
    on, off = _pair(g, 4, f"sky, {channels} ch", channels=channels)
    assert on[0].any() and np.array_equal(_bits(on[0]), _bits(off[0]))
    if channels != 1:
        n = np.bincount(on[2], minlength=W * H).astype(np.float32)
        import test_qmc_gpu as T
        want = np.zeros((W * H, channels), np.float32)
        want[:, :3] = n[:, None] * np.asarray(T.ENV, np.float32)
        assert np.array_equal(_bits(on[0]).reshape(-1, channels), _bits(want))


@pytest.mark.gpu
def test_frame_equals_the_scatter_sum_of_its_records():
    """The bound of test_qmc_gpu.py's test_frame_equals_the_scatter_sum_of_the_records: n float32 additions in any order, each rounding a partial
    sum no larger than sum|x_i| by at most 2^-24 relative."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_228"))
    img, col, pix, _, ll, _ = _call(g, True, 8)
    assert ll["schedule"] == 2
    assert np.isfinite(col).all() and col[:, :3].max() > 0.0
    ref, mag = np.zeros((W * H, 3), np.float64), np.zeros((W * H, 3), np.float64)
    np.add.at(ref, pix, col[:, :3].astype(np.float64))
    np.add.at(mag, pix, np.abs(col[:, :3].astype(np.float64)))
    n = np.bincount(pix, minlength=W * H).astype(np.float64)[:, None]
    err = np.abs(img.reshape(-1, 4)[:, :3].astype(np.float64) - ref)
    bound = n * 2.0 ** -24 * mag
    print(f"test_228, wavefront: worst error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}, samples per pixel {int(n.min())} .. {int(n.max())}")
    assert np.all(err <= bound), np.argwhere(err > bound)[:8]
    assert np.all(img[..., 3] == 0.0)


# ---- 4. suspended rays ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_suspended_rays_keep_the_qmc_call_exact():
    """The settings of test_suspended_rays_keep_the_adaptive_call_exact (one trace block per CU, refill below 56, one group, wf_grace 1) on the nested
    sheets under layout 2, at 384 x 320 slots (the module's docstring says why). An instrumented context keeps the megakernel for QMC, so the
    witness that rays are suspended in this configuration is an instrumented uniform three-pass call on a second context: a condition of the test."""
    from hydracore3_amd.api import HipIntegrator
    sc = _scene("nested_sheets", 384, 320)
    g = HipIntegrator(sc, accel_layout=2)
    g.set_option("wf_grace", 1)
    on, off = _pair(g, 3, "nested sheets, suspension", schedule=(2, 56, 1, 1), frame=False)
    assert on[4]["deep_stack"], on[4]
    print(f"[qmc wavefront] suspension: {on[5]} rounds")
    w = HipIntegrator(sc, accel_layout=2); w.set_schedule(2, 56, 1, 1); w.set_option("wf_grace", 1)
    w.set_instrumentation(True)
    w.render(3)                                                              # (test_wavefront_suspension_carries_long_stacks: its call)
    suspended = list(w.counters().values())[12]
    assert suspended > 0, suspended


# ---- 5. deep stacks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deep_stacks_reach_the_hbm_part():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("nested_sheets"))
    g.set_option("dbg_stack_witness", 1)
    on, off = _pair(g, 3, "nested sheets")
    assert on[4]["deep_stack"], on[4]
    words, filled = g.stack_witness()                                      # (of the last call: the wavefront form's)
    assert filled > 0 and words > 0, (words, filled)


# ---- 6. the rule ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_schedule_setting_decides_as_for_path_trace_block():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_scene("test_228"))
    for schedule in (1, 3, 0, 4):                                           # never, never, the automatic rule on a small scene (twice)
        _pair(g, 2, f"schedule {schedule}", expect_on=1, schedule=(schedule,))
    _pair(g, 2, "schedule 2", expect_on=2)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["sweep", "thin_film", "spectral", "instrumented", "depth0"])
def test_unserved_calls_keep_the_megakernel_with_the_same_results(what):
    from hydracore3_amd.api import HipIntegrator
    if what == "sweep":
        g = HipIntegrator(_scene("test_228"), accel_layout=3)
        assert g.accel_info()["layout"] == "sweep"
    elif what == "thin_film":
        g = HipIntegrator(_scene("thin_film"))
    elif what == "spectral":
        g = HipIntegrator(load_hydra_xml(scene_path("test_spectral"), W, H, spectral=True))
        g.set_option("qmc_spectral", 1)
    elif what == "depth0":
        sc = _scene("test_228")
        sc.trace_depth = 0
        g = HipIntegrator(sc)
    else:
        g = HipIntegrator(_scene("test_228"))
        g.set_instrumentation(True)
    on, off = _pair(g, 2, what, expect_on=1)
    assert np.isfinite(on[1]).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slot_with_more_samples_than_the_status_word_holds_is_refused_and_nothing_is_written():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    g = HipIntegrator(_scene("test_228"))
    g.set_schedule(2); g.set_option("qmc_wavefront", 1)
    g.InitRandomGens(1)
    gens0 = _gens(g, 1)
    rng = np.random.default_rng(3)
    frame = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    fb = _bits(frame).reshape(-1, 4)
    fb[::5, 0] = NAN_PAYLOAD                                                # a NaN with a payload and a negative zero
    fb[1::7, 3] = np.uint32(0x80000000)
    col = rng.uniform(0.0, 1.0, (64, 4)).astype(np.float32)
    pix = rng.integers(0, 1 << 31, 64).astype(np.uint32)
    d_frame, d_col, d_pix = g.dev_array(frame), g.dev_array(col), g.dev_array(pix.view(np.float32))
    try:
        for pixels_num, spp in ((0x1000000, 1), (4096, 4096), (0xFFFFFFFF, 0xFFFFFFFF)):        # S = 2^24, 2^24, 2^32 - 1 on one generator
            with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockQMC.*0xFFFFFF"):
                g.path_trace_qmc_block_dev(d_frame.ptr, spp, pixels_num, 4, d_col.ptr, d_pix.ptr)
            assert np.array_equal(_bits(d_frame.download()), _bits(frame)), "a refused call wrote the frame"
            assert np.array_equal(_bits(d_col.download()), _bits(col)) and np.array_equal(d_pix.download().view(np.uint32), pix), "a refused call wrote the records"
            assert np.array_equal(_gens(g, 1), gens0), "a refused call wrote the generator"
        host = frame.copy()                                                 # the host-pointer form
        with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockQMC.*0xFFFFFF"):
            g.PathTraceBlockQMC(0x1000000, 4, host, 1)
        assert np.array_equal(_bits(host), _bits(frame)) and np.array_equal(_gens(g, 1), gens0)
        # one sample fewer fits the word: the decision alone, on a call that has nothing to run (the rule is looked at only where there are samples,
        # so the tiny calls below stand for it) - and under schedule 1 the rule does not apply at all
        assert g.L.hpt_path_trace_qmc_block_dev(g.h, 0x1000000, 4, d_frame.ptr, 0, None, None, None) == 0
        g.path_trace_qmc_block_dev(d_frame.ptr, 1, 64, 4, d_col.ptr, d_pix.ptr)
        assert g.last_launch()["schedule"] == 2 and not np.array_equal(_gens(g, 1), gens0)
        g.set_schedule(1)
        g.path_trace_qmc_block_dev(d_frame.ptr, 1, 64, 4, d_col.ptr, d_pix.ptr)
        assert g.last_launch()["schedule"] == 1
    finally:
        d_frame.free(); d_col.free(); d_pix.free()
    # two generators halve slot 0's samples: 2^24 samples are then served by the rule (not run here), 2^25 are refused
    g.set_schedule(2)
    g.InitRandomGens(2)
    with pytest.raises(HydraHipError, match="hydra_hip error 1: PathTraceBlockQMC.*0xFFFFFF"):
        g.render_qmc(2, frame=True, records=False, pixels_num=0x1000000)


@pytest.mark.gpu
def test_refusals_of_the_entry_are_the_same_on_and_off():
    """Every refusal of qmc_check, in its order, with the option on and off: the same code and the same text."""
    from hydracore3_amd.api import HipIntegrator
    sc = _scene("test_228")
    buf = np.zeros((H, W, 4), np.float32)
    N = W * H
    seen = {}
    for on in (0, 1):
        out = []

        def note(g, rc):
            out.append((rc, g.L.hpt_last_error(g.h).decode()))

        g = HipIntegrator(sc)
        g.set_schedule(2); g.set_option("qmc_wavefront", on)
        note(g, g.L.hpt_path_trace_qmc_block(g.h, N, 4, None, 1))
        note(g, g.L.hpt_path_trace_qmc_block_dev(g.h, N, 4, None, 1, None, None, None))
        note(g, g.L.hpt_path_trace_qmc_block_dev(g.h, N, 4, None, 1, buf.ctypes.data, None, None))
        note(g, g.L.hpt_path_trace_qmc_block_dev2(g.h, N, 4, None, 1, None, None, buf.ctypes.data, None))
        for channels in (5, 8, 2, 0):
            note(g, g.L.hpt_path_trace_qmc_block(g.h, N, channels, buf.ctypes.data, 1))
        fresh = HipIntegrator()
        fresh.set_schedule(2); fresh.set_option("qmc_wavefront", on)
        note(fresh, fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1))
        fresh.scene, fresh._desc = sc, sc.desc()
        fresh.CommitDeviceData()
        fresh.UpdateMembersPlainData(sc.params())
        note(fresh, fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1))
        fresh.PackXYBlock(W, H)
        note(fresh, fresh.L.hpt_path_trace_qmc_block(fresh.h, N, 4, buf.ctypes.data, 1))
        spec = HipIntegrator(load_hydra_xml(scene_path("test_spectral"), W, H, spectral=True))
        spec.set_schedule(2); spec.set_option("qmc_wavefront", on)
        note(spec, spec.L.hpt_path_trace_qmc_block(spec.h, N, 4, buf.ctypes.data, 1))
        assert not buf.any()
        seen[on] = out
    assert all(rc != 0 for rc, _ in seen[0]), seen[0]
    assert seen[0] == seen[1]
    assert sorted({rc for rc, _ in seen[0]}) == [1, 3, 4]


@pytest.mark.gpu
def test_option_takes_0_or_1():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    g = HipIntegrator(_scene("test_228"))
    g.set_schedule(2)
    for v in (2, -1, 255):
        with pytest.raises(HydraHipError, match="hydra_hip error 1: qmc_wavefront"):
            g.set_option("qmc_wavefront", v)
    g.render_qmc(1)                                                          # the refused values left the default: the megakernel
    assert g.last_launch()["schedule"] == 1
    g.set_option("qmc_wavefront", 1); g.render_qmc(1)
    assert g.last_launch()["schedule"] == 2
    g.set_option("qmc_wavefront", 0); g.render_qmc(1)
    assert g.last_launch()["schedule"] == 1


# ---- 8. PathTraceBlockKMLT with FB_DIRECT -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kmlt_direct_layer_reaches_the_wavefront_form():
    from hydracore3_amd.api import HipIntegrator
    sc = _scene("sky")
    g = HipIntegrator(sc, sc.params(render_layer=1), accel_layout=2)         # FB_DIRECT; not the scene's own sweep layout
    res = []
    for on in (0, 1):
        g.set_schedule(2); g.set_option("qmc_wavefront", on)
        g.InitRandomGens(g.N)
        img = np.zeros((H, W, 4), np.float32)
        g.PathTraceBlockKMLT(g.N, 4, img, 4)
        assert g.last_launch()["schedule"] == (2 if on else 1)
        t = g.GetExecutionTime("PathTraceBlockQMC")
        assert t[0] > 0.0
        res.append((img, g.random_gens()))
    assert res[1][0].any()
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(res[0][1], res[1][1])

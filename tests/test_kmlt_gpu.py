"""PathTraceBlockKMLT on the GPU (hpt_kmlt.hip): the primary-sample-space pass against PathTraceBlock bit for bit, then the Markov chains
against the numpy restatement (tests/kmlt_reference.py) replayed from the device's own records.

What is compared with what:
 * F(x) for the vectors the pseudo generator would have drawn: one PathTraceBlock pass of the same context (device code, itself held to the
   oracle by test_gpu_parity.py), bit for bit;
 * proposals: the restatement's gen2 stream (large steps bit for bit, small steps to 8 * 2^-24 in circular distance: MutateKelemen's step is
   1 / p2 times a difference of two expf values <= 1, three ulp each, and the final add rounds once - under 2 * 2^-24, times four);
 * F of every recorded proposal: the PSS pass on the recorded vector, bit for bit;
 * acceptance, compared pixel, contributions, statistics: the restatement fed with the recorded colours, bit for bit; the frame: the float64
   scatter sum of the contributions, every pixel held to n * 2^-24 * sum|x_i| (n float32 atomic additions in any order).
"""
import numpy as np
import pytest

import kmlt_reference as K
from conftest import scene_path
from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.scene import load_hydra_xml

F32 = np.float32
HPT_ERR_ARG, HPT_ERR_STATE, HPT_ERR_UNSUPPORTED = 1, 3, 4
ENV = (0.5, 0.25, 2.0)
EPS = 2.0 ** -24


def _integ(sc, params=None, layout=0):
    from hydracore3_amd.api import HipIntegrator
    return HipIntegrator(sc, params, accel_layout=layout)


def _sky_scene(w, h):
    """A constant environment colour and no geometry in view (the camera of synth.furnace_plane looks straight up)."""
    sc = synth.furnace_plane(w, h, env=ENV)
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 5.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 1.0)
    return sc


def _emissive_cornell(w, h, motion=True):
    """test_035's geometry with emitters for materials and no lights, its last instance moving; traceDepth 2 so that gltf-free paths still end."""
    sc = load_hydra_xml(scene_path("test_035"), w, h)
    cols = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.7, 0.7, 0.6), (0.3, 0.4, 1.2), (1.5, 1.25, 0.5)]
    sc.materials = [S.material_emissive(cols[i % len(cols)], mult=1.0 + 0.25 * (i % 3)) for i in range(len(sc.materials))]
    sc.lights = []
    sc.remap_inst = [(int(r[0]), -1) for r in np.asarray(sc.remap_inst).reshape(-1, 2)]
    sc.trace_depth = 2
    sc.env_color = (0.125, 0.25, 0.5, 0.0)
    sc.exposure_mult = 1.5
    if motion:
        last = len(sc.inst_matrices) - 1
        sc.inst_motion[last] = np.asarray(sc.inst_matrices[last], np.float64).reshape(4, 4) @ S.translate(0.4, 0.0, 0.1)
    return sc


def _blend_scene(w, h):
    """A sphere of M = blend(id1 = B, id2 = red gltf, 0.5), B = blend(conductor, Oren-Nayar, 0.3) under a rect light and a constant sky, depth 2:
    a vertex on it draws one blend number (< 0.5: the gltf leaf) or two."""
    sc = S.SceneData()
    sc.width, sc.height = w, h
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    sc.fov, sc.trace_depth = 40.0, 2
    sc.env_color = (0.3, 0.35, 0.4, 0.0)
    M = sc.materials
    M.append(S.material_gltf((0.8, 0.2, 0.2, 1.0), 0.0, 0.6, 1.0, 1.5))             # 0
    M.append(S.material_conductor(0.2, 3.9, 0.15, 0.15))                            # 1
    M.append(S.material_diffuse((0.2, 0.3, 0.8), 0.5))                              # 2
    M.append(S.material_blend(1, 2, 0.3))                                           # 3 = B
    M.append(S.material_blend(3, 0, 0.5))                                           # 4 = M
    sp = synth._sphere_mesh(3)
    sc.add_instance(sc.add_mesh(sp[0], sp[1], sp[2], sp[3], sp[4], np.full(sp[4].size // 3, 4, np.uint32)), np.eye(4))
    sc.lights.append(S.light_rect(S.translate(0.0, 4.0, 1.5), 1.0, 1.0, (1, 1, 1), 14.0))
    return sc


def _base_vectors(g, blend_weight=None):
    """The vectors x whose F equals what PathTraceBlock's next pass computes, per tid: the numbers the base class draws from m_randomGens[tid]
    (the lens float4, the time when instances move, per bounce the selection float, the light float4, [the blend numbers,]
    the material float4), laid out in IntegratorKMLT's slots; x[0], x[1]: the film point the base camera forms from pixel and jitter.
    blend_weight: every surface is the two-level blend of _blend_scene - bounce 0 draws a second blend number when the first is >= it."""
    p = g.params
    n = K.state_size(p.traceDepth)
    G = K.Gens.from_states(g.random_gens())
    xy = g.packed_xy()
    lens = G.float4()
    x = np.zeros((g.N, n), F32)
    fx = (xy & 0xFFFF).astype(F32) + lens[:, 0]
    fy = (xy >> 16).astype(F32) + lens[:, 1]
    x[:, 0] = (fx + F32(p.winStartX)) / F32(p.fbWidth)
    x[:, 1] = (fy + F32(p.winStartY)) / F32(p.fbHeight)
    x[:, 2:4] = lens[:, 2:4]
    if g.scene.inst_motion:
        x[:, 5] = G.float1()
    for b in range(p.traceDepth):
        o = K.BOUNCE_START + K.PER_BOUNCE * b
        x[:, o + 3] = G.float1()
        x[:, o:o + 3] = G.float4()[:, :3]
        if blend_weight is not None and b == 0:
            s0 = G.float1()
            two = s0 >= F32(blend_weight)
            s1 = G.float1(two)
            x[:, o + K.BLND_ID], x[:, o + K.BLND_ID + 1] = s0, np.where(two, s1, F32(0.0))
        x[:, o + K.MATS_ID:o + K.MATS_ID + 4] = G.float4()
    return x, xy


def _numpy_pixels(x, w, h):
    px = np.minimum((x[:, 0] * F32(w)).astype(np.uint32), w - 1)
    py = np.minimum((x[:, 1] * F32(h)).astype(np.uint32), h - 1)
    return py * np.uint32(w) + px


def _pss_equals_one_pass(g, blend_weight=None):
    x, xy = _base_vectors(g, blend_weight)
    gens = g.random_gens().copy()
    col, pix = g.path_trace_pss(x)
    assert np.array_equal(g.random_gens(), gens)                         # the PSS pass touches no generator
    img = g.render(1)
    want = img[xy >> 16, xy & 0xFFFF]
    bad = np.flatnonzero(np.any(col[:, :3].view(np.uint32) != want[:, :3].view(np.uint32), axis=1))
    print(f"PSS vs one PathTraceBlock pass: {bad.size} of {g.N} pixels differ; mean colour {float(want[:, :3].mean()):.4f}")
    assert bad.size == 0, (bad[:8], col[bad[:4]], want[bad[:4]])
    assert np.all(col[:, 3] == 0.0) and float(want[:, :3].max()) > 0.0
    assert np.array_equal(pix, _numpy_pixels(x, g.W, g.H))
    return x, col, pix


# ---- 1. the PSS pass against PathTraceBlock ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 64), (48, 20)])
def test_pss_equals_path_trace_block_on_the_cornell_box(w, h):
    sc = load_hydra_xml(scene_path("test_035"), w, h)
    sc.cam_respoce_rgb = (1.0, 1.0, 1.0, 1.0)
    _pss_equals_one_pass(_integ(sc))


@pytest.mark.gpu
def test_pss_equals_path_trace_block_on_legacy_materials():
    sc = load_hydra_xml(scene_path("legacy_materials"), 64, 48)
    sc.cam_respoce_rgb = (1.0, 1.0, 1.0, 1.0)
    _pss_equals_one_pass(_integ(sc))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_pss_equals_path_trace_block_with_a_moving_instance(layout):
    _pss_equals_one_pass(_integ(_emissive_cornell(48, 32), layout=layout))


@pytest.mark.gpu
def test_pss_equals_path_trace_block_with_a_thin_lens():
    sc = load_hydra_xml(scene_path("test_035"), 48, 32)
    sc.cam_respoce_rgb = (1.0, 1.0, 1.0, 1.0)
    sc.cam_lens_radius = 0.08
    x, _, _ = _pss_equals_one_pass(_integ(sc))
    assert np.any(x[:, 2] != 0.0)


@pytest.mark.gpu
def test_blend_numbers_are_read_from_slots_8_and_9():
    g = _integ(_blend_scene(48, 48))
    x, col, _ = _pss_equals_one_pass(g, blend_weight=0.5)
    # the slots matter: with the two numbers swapped for 1 - s the leaves change and so do colours
    y = x.copy()
    y[:, K.BOUNCE_START + K.BLND_ID] = F32(1.0) - x[:, K.BOUNCE_START + K.BLND_ID]
    col2, _ = g.path_trace_pss(y)
    assert np.any(col2 != col)
    # a vector longer than the state size is read up to the state size only; a shorter stride is refused
    wide = np.concatenate([x, np.full((x.shape[0], 5), 0.75, F32)], axis=1)
    assert np.array_equal(g.path_trace_pss(wide)[0], col)
    from hydracore3_amd.api import HydraHipError
    with pytest.raises(HydraHipError, match="strideFloats"):
        g.path_trace_pss(x[:, :-1])


# ---- 2 - 5. the chains, replayed from their records ---------------------------------------------------------------------------------------------
CHAINS, STEPS = 64, 32


@pytest.fixture(scope="module")
def chain_run():
    """One recorded run on test_035 at 32 x 32, depth 3: 64 chains x 32 steps (2 passes), proposals kept, raw and normalised frame of the same run."""
    sc = load_hydra_xml(scene_path("test_035"), 32, 32)
    sc.trace_depth = 3
    g = _integ(sc)
    gens = g.random_gens().copy()
    r = g.render_kmlt(2, chains=CHAINS, normalize=True, records=True, proposals=True, unnormalised=True)
    assert (r["chains"], r["steps"]) == (CHAINS, STEPS) and r["proposals"].shape == (CHAINS, STEPS, 48)
    assert np.array_equal(g.random_gens(), gens)                         # m_randomGens is left untouched
    ref = K.run_chains(CHAINS, STEPS, 48, (32, 32), recorded=r)
    return g, r, ref


@pytest.mark.gpu
def test_proposals_equal_the_restatement(chain_run):
    _, r, ref = chain_run
    large = ref["isLarge"]
    assert large.any() and (~large).any()
    assert np.array_equal(r["proposals"][large].view(np.uint32), ref["proposals"][large].view(np.uint32))
    d = K.circular_distance(r["proposals"][~large], ref["proposals"][~large])
    print(f"small-step proposals: max circular distance {d.max():.3e} = {d.max() / EPS:.2f} x 2^-24 over {d.size} numbers")
    assert d.max() <= 8 * EPS


@pytest.mark.gpu
def test_recorded_colours_are_f_of_the_recorded_proposals(chain_run):
    g, r, ref = chain_run
    col, pix = g.path_trace_pss(r["proposals"].reshape(-1, 48))
    assert np.array_equal(col.view(np.uint32), r["color"].reshape(-1, 4).view(np.uint32))
    assert np.array_equal(pix, r["pixel"].reshape(-1))
    col0, pix0 = g.path_trace_pss(ref["init"])                           # the initial state: stateSize rndFloat1 draws of gen2
    assert np.array_equal(col0.view(np.uint32), r["initColor"].view(np.uint32)) and np.array_equal(pix0, r["initPixel"])


@pytest.mark.gpu
def test_bookkeeping_equals_the_restatement(chain_run):
    _, r, ref = chain_run
    assert np.array_equal(r["isLarge"].astype(bool), ref["isLarge"])
    assert np.array_equal(r["a"].view(np.uint32), ref["a"].view(np.uint32))
    assert np.array_equal(r["accepted"].astype(bool), ref["accepted"])
    assert np.array_equal(r["oldPixel"], ref["oldPixel"])
    for k, add in (("contribAtX", "addX"), ("contribAtY", "addY")):      # both contributions as formed, and whether the step added them
        assert np.array_equal(r[k][..., :3].view(np.uint32), ref[k].view(np.uint32)), k
        assert np.array_equal(r[k][..., 3] == 1.0, ref[add]) and np.all((r[k][..., 3] == 0.0) | (r[k][..., 3] == 1.0))
    assert ref["addX"].any() and (~ref["addX"]).any() and ref["addY"].any()
    assert 0 < ref["accepted"].sum() < ref["accepted"].size
    raw = r["frame_unnormalised"].reshape(-1, 4)
    err = np.abs(raw[:, :3].astype(np.float64) - ref["frame"])
    bound = ref["count"][:, None] * EPS * ref["mag"]
    print(f"raw frame vs float64 scatter sum: worst error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}; up to {ref['count'].max()} additions per pixel")
    assert np.all(err <= bound) and np.all(raw[:, 3] == 0.0) and ref["count"].max() > 2


@pytest.mark.gpu
def test_normalisation_equals_the_restatement(chain_run):
    g, r, ref = chain_run
    want = K.normalisation(ref["accumBrightness"], ref["largeSteps"], ref["accept"], r["frame_unnormalised"], g.N, 2)
    got = r["stats"]
    print(f"stats {got.tolist()} restatement {want.tolist()}")
    assert abs(got[0] - want[0]) <= 1e-12 * want[0] and abs(got[1] - want[1]) <= 1e-12 * want[1]
    assert got[2] == want[2]
    assert abs(F32(got[3]) - F32(want[3])) <= np.spacing(F32(want[3])) and got[3] == float(F32(got[3])) and got[3] != 1.0
    assert r["frame"].tobytes() == (r["frame_unnormalised"] * F32(got[3])).astype(F32).tobytes()
    img = np.zeros((g.H, g.W, 4), F32)
    g.PathTraceBlockKMLT(g.N, 4, img, 2)                                 # the host-pointer form: the same chains, normalised
    t = g.GetExecutionTime("PathTraceBlockKMLT")
    assert t[0] > 0.0 and all(v >= 0.0 for v in t[1:3])
    assert np.allclose(img, r["frame"], rtol=1e-4, atol=1e-6)


# ---- 6. known answer -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_constant_sky_known_answer():
    w, h, spp, chains = 32, 16, 4, 128
    g = _integ(_sky_scene(w, h))
    r = g.render_kmlt(spp, chains=chains, records=True, unnormalised=True)
    steps = r["steps"]
    assert steps == w * h * spp // chains
    assert np.all(r["a"] == 1.0) and np.all(r["accepted"] == 1)
    env = np.asarray(ENV, F32)
    assert np.all(r["color"][..., :3] == env) and np.all(r["initColor"][:, :3] == env)
    # nothing is added at the old state: the raw frame is count_p * ENV / y, every step's own pixel once
    y = K.contrib_func(env)
    unit = (env * (F32(1.0) / y)).astype(F32)
    count = np.bincount(r["pixel"].reshape(-1), minlength=w * h).astype(np.float64)
    raw = r["frame_unnormalised"].reshape(-1, 4)[:, :3].astype(np.float64)
    assert np.all(np.abs(raw - count[:, None] * unit) <= count[:, None] * EPS * (count[:, None] * unit))
    # avgBrightness = y exactly; every step is accepted
    assert r["stats"][0] == float(y) and r["stats"][2] == chains * steps / (w * h * spp)
    norm = r["stats"][3]
    got = r["frame"].reshape(-1, 4)[:, :3].astype(np.float64)
    # (a) the frame through the float32 steps the device takes: (count_p * unit, summed by atomics) * normConst. The tolerance is the rounding
    # bound of the sum (test 4's) times normConst, plus half an ulp of the value for the scaling multiply's own rounding, which that bound
    # does not contain (a pixel with count 1 has a sum bound of half an ulp of unit and is then rounded once more).
    want32 = count[:, None] * unit.astype(np.float64) * norm
    tol = norm * count[:, None] * EPS * (count[:, None] * unit) + EPS * want32
    print(f"sky: normConst {norm:.6f}, worst error / tolerance {np.max(np.abs(got - want32)[want32 > 0] / tol[want32 > 0]):.3f}")
    assert np.all(np.abs(got - want32) <= tol)
    # (b) the closed form count_p * ENV * pixels * passNum / (C * steps): it differs from (a) only by normConst * unit against ENV * pixels *
    # passNum / (C * steps), a relation of two float32 quantities. Roundings between them, each at most 2^-24 relative: 1 / y and env * (1 / y)
    # in unit (2); the sums contribFunc(frame pixel) in actualBrightness see the atomic sums' rounding (at most max count) and contribFunc's own
    # two additions and one product (3); float(avg / actual) and float(passNum) * that (2); the comparison's own product (1): 8 + max count.
    closed = env.astype(np.float64) * (w * h) * spp / (chains * steps)
    rel = np.abs(norm * unit.astype(np.float64) - closed) / closed
    print(f"sky: normConst * unit against the closed form: {rel.max() / EPS:.2f} x 2^-24 relative (allowed {8 + count.max():.0f})")
    assert np.all(rel <= (8 + count.max()) * EPS)


# ---- 7. the estimator ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_large_step_mean_estimates_the_image_brightness():
    from oracle.orc import OracleIntegrator
    sc = load_hydra_xml(scene_path("test_035"), 32, 32)
    sc.cam_respoce_rgb = (1.0, 1.0, 1.0, 1.0)
    cpu = OracleIntegrator(sc)
    one = cpu.render(1).reshape(-1, 4)
    sigma = float(np.std(K.contrib_func(one[:, :3]).astype(np.float64), ddof=1))
    cpu = OracleIntegrator(sc)
    mean64 = float(np.mean(K.contrib_func((cpu.render(64) / F32(64)).reshape(-1, 4)[:, :3]).astype(np.float64)))
    g = _integ(sc)
    r = g.render_kmlt(32, chains=512, normalize=False, records=True)
    assert r["steps"] == 64
    n_large = int(r["isLarge"].sum())
    bound = 5.0 * sigma * np.sqrt(1.0 / n_large + 1.0 / (64 * 1024))
    print(f"large-step mean {r['stats'][0]:.5f} vs oracle 64-pass mean brightness {mean64:.5f}: difference {abs(r['stats'][0] - mean64):.5f}, bound {bound:.5f} "
          f"(sigma {sigma:.4f}, {n_large} large steps)")
    assert abs(r["stats"][0] - mean64) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp,blocks_per_cu", [(16, 16, 2, 0), (64, 64, 64, 0), (64, 64, 64, 2)])
def test_default_chain_count_sizes_the_records(w, h, spp, blocks_per_cu):
    """chains=None: the library's default, one chain per lane of the resident grid (CUs x blocks per CU x 256; 3 blocks unless the launch
    configuration says otherwise), at most pixels x passes; render_kmlt sizes its record arrays by the library's answer."""
    g = _integ(_sky_scene(w, h))
    if blocks_per_cu:
        g.set_launch_config(blocks_per_cu)
    total = w * h * spp
    want = min(g.device_info()["cus"] * (blocks_per_cu or 3) * 256, total)
    assert g.kmlt_chain_count(spp) == (want, total // want)
    r = g.render_kmlt(spp, records=True)
    assert (r["chains"], r["steps"]) == (want, total // want)
    assert r["a"].shape == (want, total // want) and r["initPixel"].shape == (want,) and r["contribAtY"].shape == (want, total // want, 4)
    assert np.all(r["accepted"] == 1) and r["accepted"].size == round(r["stats"][2] * total)   # every step on the sky is accepted: C * steps of them
    assert np.all(r["color"][..., :3] == np.asarray(ENV, F32)) and np.all(r["pixel"] < w * h)
    # the public option reaches the same place: the next call runs, and is sized for, what set_option says
    g.set_option("kmlt_chains", 96)
    r = g.render_kmlt(spp, records=True)
    assert (r["chains"], r["steps"]) == (96, total // 96) and r["pixel"].shape == (96, total // 96) and np.all(r["accepted"] == 1)


# ---- 8. arguments ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_arguments_and_refusals():
    import ctypes as C
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    g = _integ(_sky_scene(16, 16))
    n = K.state_size(g.params.traceDepth)
    img = np.zeros((16, 16, 4), F32)
    gens = g.random_gens().copy()

    def rc_msg(rc):
        return rc, g.L.hpt_last_error(g.h).decode()
    d = C.c_void_p()
    g._chk(g.L.hpt_device_malloc(g.h, 16 * 16 * 16 * 4, C.byref(d)))
    try:
        rc, msg = rc_msg(g.L.hpt_path_trace_pss_dev(g.h, None, 4, n, d, d, None))
        assert rc == HPT_ERR_ARG and "null" in msg
        rc, msg = rc_msg(g.L.hpt_path_trace_pss_dev(g.h, d, 4, n - 1, d, d, None))
        assert rc == HPT_ERR_ARG and "strideFloats" in msg
        for ch in (1, 3, 5):
            rc, msg = rc_msg(g.L.hpt_path_trace_kmlt_block_dev(g.h, g.N, ch, d, 1, 1, None, None, None))
            assert rc == HPT_ERR_ARG and "channels" in msg
        rc, msg = rc_msg(g.L.hpt_path_trace_kmlt_block_dev(g.h, g.N, 4, None, 1, 1, None, None, None))
        assert rc == HPT_ERR_ARG and "null" in msg
        rc, msg = rc_msg(g.L.hpt_set_option(g.h, b"kmlt_chains", 0))
        assert rc == HPT_ERR_ARG and "kmlt_chains" in msg
        g.set_option("kmlt_chains", g.N * 2 + 1)
        rc, msg = rc_msg(g.L.hpt_path_trace_kmlt_block(g.h, g.N, 4, img.ctypes.data, 2))
        assert rc == HPT_ERR_ARG and "kmlt_chains" in msg and not img.any()
        # a_passNum = 0: nothing is touched
        g.set_option("kmlt_chains", 8)
        g.PathTraceBlockKMLT(g.N, 4, img, 0)
        assert not img.any()
        # the remainder of (pixelsNum * a_passNum) / C is dropped
        g.set_option("kmlt_chains", 100)
        r = g.render_kmlt(1, records=True)
        assert (r["chains"], r["steps"]) == (100, 2) and r["stats"][2] == 200 / 256
        assert np.array_equal(g.random_gens(), gens)
    finally:
        g.L.hpt_device_free(g.h, d)
    # before PackXYBlock / CommitDeviceData
    bare = HipIntegrator()
    err = lambda: bare.L.hpt_last_error(bare.h).decode()
    db = C.c_void_p()
    bare._chk(bare.L.hpt_device_malloc(bare.h, 16 * 16 * 16 * 4, C.byref(db)))
    try:
        for stage in ("CommitDeviceData", "PackXYBlock"):
            assert bare.L.hpt_path_trace_kmlt_block(bare.h, 256, 4, img.ctypes.data, 1) == HPT_ERR_STATE and stage in err() and "PathTraceBlockKMLT" in err()
            assert bare.L.hpt_path_trace_kmlt_block_dev(bare.h, 256, 4, db, 1, 1, None, None, None) == HPT_ERR_STATE and stage in err()
            assert bare.L.hpt_path_trace_pss_dev(bare.h, db, 4, 64, db, db, None) == HPT_ERR_STATE and stage in err() and "PathTracePSS" in err()
            assert not img.any()
            if stage == "CommitDeviceData":
                sc = _sky_scene(16, 16)
                bare.scene, bare._desc = sc, sc.desc()
                bare.CommitDeviceData()
                bare.UpdateMembersPlainData(sc.params())
        bare.PackXYBlock(16, 16, 1)                                       # no InitRandomGens: neither entry needs m_randomGens
        assert bare.L.hpt_path_trace_kmlt_block(bare.h, 256, 4, img.ctypes.data, 1) == 0 and img[..., :3].any()
        img[:] = 0.0
    finally:
        bare.L.hpt_device_free(bare.h, db)
    # m_spectral_mode
    gs = HipIntegrator(load_hydra_xml(scene_path("test_spectral"), 16, 16, spectral=True))
    ns = K.state_size(gs.params.traceDepth)
    rc = gs.L.hpt_path_trace_kmlt_block(gs.h, gs.N, 4, img.ctypes.data, 1)
    assert rc == HPT_ERR_UNSUPPORTED and "spectral" in gs.L.hpt_last_error(gs.h).decode() and not img.any()
    dd = C.c_void_p()
    gs._chk(gs.L.hpt_device_malloc(gs.h, 4096, C.byref(dd)))
    rc = gs.L.hpt_path_trace_pss_dev(gs.h, dd, 1, ns, dd, dd, None)
    gs.L.hpt_device_free(gs.h, dd)
    assert rc == HPT_ERR_UNSUPPORTED and "spectral" in gs.L.hpt_last_error(gs.h).decode()


@pytest.mark.gpu
def test_direct_layer_forwards_to_the_qmc_path():
    sc = load_hydra_xml(scene_path("test_035"), 32, 32)
    prm = sc.params(render_layer=1)                                      # FB_DIRECT
    g = _integ(sc, prm)
    gens = g.random_gens().copy()
    _, col, pix = g.render_qmc(2, frame=False, records=True)
    after = g.random_gens().copy()
    g.set_random_gens(gens)
    img = np.zeros((32, 32, 4), F32)
    g.PathTraceBlockKMLT(g.N, 4, img, 2)
    assert np.array_equal(g.random_gens(), after)                        # the QMC path's generator contract, not KMLT's
    ref, mag = np.zeros((g.N, 3)), np.zeros((g.N, 3))
    np.add.at(ref, pix, col[:, :3].astype(np.float64))
    np.add.at(mag, pix, np.abs(col[:, :3]).astype(np.float64))
    cnt = np.bincount(pix, minlength=g.N)[:, None]
    assert np.all(np.abs(img.reshape(-1, 4)[:, :3] - ref) <= cnt * EPS * mag) and ref.max() > 0

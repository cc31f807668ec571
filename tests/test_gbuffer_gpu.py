"""EvalGBuffer on the GPU against the numpy float32 restatement (tests/gbuffer_reference.py): every field of every sample record and of
every reduced record, compared as uint32 views - equality is the bar. The reduced frame is also compared with the restatement's reduction
of the GPU's OWN samples, which tells a sampling fault from a reduction fault.

One field is held to 2 ulp instead, and only where the cause applies: r, g, b of samples whose material reads an sRGB texture (and of the
pixels such a sample is averaged into). The decode is x^2.2 after filtering. The pass rounds that power correctly (in double, rounded once);
the host's powf, which the restatement goes through, is correctly rounded for all but a few arguments in 10^4 (profiles/gbuffer.md has
the demonstration), so a few samples per 10^4 differ in the last bit. Everything else of those records - depth, normal, texture
coordinates, alpha, coverage, the ids and with them the winner - and all of every other record is compared for equality; the reduction
itself is compared for equality everywhere through the GPU's own samples."""
import numpy as np
import pytest

import gbuffer_reference as R
from conftest import scene_path
from hydracore3_amd import synth
from hydracore3_amd.api import GBUFFER_DTYPE
from hydracore3_amd.scene import load_hydra_xml
from traversal_scenes import forced_sweep_scene, sweep_scene

HPT_ERR_ARG, HPT_ERR_STATE = 1, 3


def _open_interior():
    """A miniature synth.interior_scene without its room: 24 instanced meshes (a tree, not the sweep) in front of the background."""
    sc = synth.interior_scene(64, 48, objects=24, subdiv=1, tex_size=16)
    sc.inst_geom.pop(0); sc.inst_matrices.pop(0); sc.remap_inst.pop(0)    # instance 0 is the closed room
    return sc


def _motion_scene():
    seed = next(s for s in range(100) if synth.random_scene(s).inst_motion)
    return synth.random_scene(seed)


def _cornell():
    return load_hydra_xml(scene_path("test_035"), 64, 64)


# name -> (scene key, scene builder, HipIntegrator keyword arguments, options set before a re-commit, layout expected or None)
CASES = {
    "test_035": ("test_035", _cornell, {}, {}, "sweep"),
    "test_035 layout 1": ("test_035", _cornell, {"accel_layout": 1}, {}, "two-level"),
    "test_035 layout 2": ("test_035", _cornell, {"accel_layout": 2}, {}, "flat"),
    "test_035 layout 3": ("test_035", _cornell, {"accel_layout": 3}, {}, "sweep"),
    "test_035 device_build 0": ("test_035", _cornell, {"accel_layout": 2}, {"device_build": 0}, "flat"),
    "test_035 device_build 1": ("test_035", _cornell, {"accel_layout": 2}, {"device_build": 1}, "flat"),
    "sweep_scene 11": ("sweep 11", lambda: sweep_scene(11), {}, {}, "sweep"),
    "sweep_scene 12": ("sweep 12", lambda: sweep_scene(12), {}, {}, "sweep"),
    "sweep_scene 13": ("sweep 13", lambda: sweep_scene(13), {}, {}, "sweep"),
    "forced_sweep_scene 21": ("forced 21", lambda: forced_sweep_scene(21), {"accel_layout": 3}, {}, "sweep"),
    "forced_sweep_scene 21 automatic": ("forced 21", lambda: forced_sweep_scene(21), {}, {}, None),
    "material_zoo": ("material_zoo", lambda: synth.material_zoo(96, 64), {}, {}, None),
    "png_textures": ("png_textures", lambda: load_hydra_xml(scene_path("png_textures"), 64, 48), {}, {}, None),
    "jpg_textures": ("jpg_textures", lambda: load_hydra_xml(scene_path("jpg_textures"), 64, 48), {}, {}, None),
    "interior": ("interior", _open_interior, {}, {}, None),
    "interior two-level": ("interior", _open_interior, {"accel_layout": 1}, {}, "two-level"),
    "motion": ("motion", _motion_scene, {}, {}, None),
    "motion single-level": ("motion", _motion_scene, {"accel_layout": 2}, {}, "flat"),
}

_scenes, _refs = {}, {}


def _reference(name):
    """(scene, oracle, reference frame, reference samples), computed once per scene."""
    key, build = CASES[name][:2]
    if key not in _scenes:
        from oracle.orc import OracleIntegrator
        sc = build()
        _scenes[key] = (sc, OracleIntegrator(sc))
    sc, cpu = _scenes[key]
    if key not in _refs:
        _refs[key] = R.eval_gbuffer(sc, cpu)
    return sc, cpu, _refs[key][0], _refs[key][1]


def _gpu(name, sc):
    from hydracore3_amd.api import HipIntegrator
    _, _, kw, opts, layout = CASES[name]
    g = HipIntegrator(sc, **kw)
    if opts:
        for k, v in opts.items():
            g.set_option(k, v)
        g.CommitScene()
        if "device_build" in opts:
            assert bool(g.commit_time()["device_built"]) == bool(opts["device_build"])
    if layout is not None:
        assert g.accel_info()["layout"] == layout, g.accel_info()
    return g


def _assert_scene_is_exercised(name, sc, raw):
    hit = raw["instId"] >= 0
    assert hit.any(), name
    if name in ("test_035", "material_zoo", "interior"):
        assert (~hit).any(), f"{name}: no sample misses"
    if name == "material_zoo":
        mt = np.array(sc.materials, dtype=sc.materials[0].dtype)["mtype"][raw["matId"][hit]]
        assert (mt == 0xEFFFFFFF).any() and np.unique(mt).size >= 4, "material_zoo: a light source and several material types in view"
    if name == "interior":
        assert np.unique(raw["instId"][hit]).size >= 10
    if name.startswith("motion"):
        assert any(int(i) in sc.inst_motion for i in np.unique(raw["instId"][hit])), "no sample hits the moving instance"


# ---- 1. raw samples, bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_raw_samples_equal_the_restatement(name):
    sc, cpu, _, ref_raw = _reference(name)
    g = _gpu(name, sc)
    _, raw = g.EvalGBuffer(samples=True)
    assert raw.shape == (sc.width * sc.height, 16)
    _assert_scene_is_exercised(name, sc, ref_raw)
    R.assert_records_equal(raw, ref_raw, f"{name}: raw samples", rgb_2ulp=R.srgb_textured(sc, ref_raw))
    assert g.last_kernel_ms() > 0.0


# ---- 2. reduced frame, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_reduced_frame_equals_the_restatement(name):
    """Exact: the frame against the restatement's reduction of the GPU's own samples, the host-pointer form against the device-pointer form,
    and against the restatement every field but r, g, b of pixels that average an sRGB-textured sample. Those three are held to 2 ulp, the
    bound for a field that cannot be made bit-equal. Measured on an MI355X: material_zoo 10 of 6144 pixels differ, png_textures 1 of 3072,
    both by at most 2 ulp; no pixel differs in the other 16 cases."""
    sc, cpu, ref_frame, ref_raw = _reference(name)
    g = _gpu(name, sc)
    frame, raw = g.EvalGBuffer(samples=True)
    assert frame.shape == (sc.height, sc.width)
    own, _ = R.reduce_samples(raw, sc.width, sc.height)                  # the restatement's reduction of the GPU's own samples
    R.assert_records_equal(frame, R.scatter(own, g.packed_xy(), sc.width, sc.height), f"{name}: frame vs reduction of the GPU's samples")
    R.assert_records_equal(g.EvalGBuffer(), frame, f"{name}: host-pointer form vs device-pointer form")
    exact = frame.copy()
    exact["rgba"][..., :3] = ref_frame["rgba"][..., :3]
    R.assert_records_equal(exact, ref_frame, f"{name}: frame vs restatement, every field but r, g, b")
    loose = R.scatter(R.srgb_textured(sc, ref_raw).any(axis=1), cpu.packed_xy(), sc.width, sc.height, np.zeros((sc.height, sc.width), bool))
    R.assert_records_equal(frame, ref_frame, f"{name}: frame vs restatement", rgb_2ulp=loose)


# ---- 3. window --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_inside_a_larger_framebuffer_and_tail_rows():
    """A 20 x 10 window at (8, 6) of a 48 x 32 framebuffer: 200 pixels = 12 full blocks of 16 pixels and a tail of 8 (3200 lanes = 12.5 blocks of
    256), a width that is no multiple of 16. The frame equals the crop of the FULL frame's raw samples, reduced with the window's size
    (projectedPixelSize takes winWidth / winHeight), and the restatement under the same parameters."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = sweep_scene(12)
    full = HipIntegrator(sc)
    _, full_raw = full.EvalGBuffer(samples=True)
    fxy = full.packed_xy()
    by_pixel = np.zeros((sc.height, sc.width, 16), GBUFFER_DTYPE)
    by_pixel[(fxy >> 16) & 0xFFFF, fxy & 0xFFFF] = full_raw
    p = sc.params()
    p.winStartX, p.winStartY, p.winWidth, p.winHeight, p.tileSize = 8, 6, 20, 10, 2
    win = HipIntegrator(sc, p)
    assert (win.W, win.H, win.N) == (20, 10, 200) and win.N % 16 != 0
    frame, raw = win.EvalGBuffer(samples=True)
    assert frame.shape == (10, 20) and raw.shape == (200, 16)
    wxy = win.packed_xy()
    crop = by_pixel[((wxy >> 16) & 0xFFFF) + 6, (wxy & 0xFFFF) + 8]
    R.assert_records_equal(raw, crop, "window: raw samples vs the full frame's")
    red, _ = R.reduce_samples(crop, 20, 10)
    R.assert_records_equal(frame, R.scatter(red, wxy, 20, 10), "window: frame vs the crop reduced")
    cpu = OracleIntegrator(sc, p)
    assert np.array_equal(cpu.packed_xy(), wxy)
    ref_frame, ref_raw = R.eval_gbuffer(sc, cpu, p)
    R.assert_records_equal(raw, ref_raw, "window: raw samples vs restatement", rgb_2ulp=R.srgb_textured(sc, ref_raw))
    loose = R.scatter(R.srgb_textured(sc, ref_raw).any(axis=1), wxy, 20, 10, np.zeros((10, 20), bool))
    R.assert_records_equal(frame, ref_frame, "window: frame vs restatement", rgb_2ulp=loose)


# ---- 4. partial blockNum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block_num", [1, 15, 16, 17, 1000, 64 * 64 - 1])
def test_partial_block_num_leaves_the_other_records_untouched(block_num):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_cornell())
    full, full_raw = g.EvalGBuffer(samples=True)
    xy = g.packed_xy()
    for samples in (False, True):
        out = np.zeros((64, 64), GBUFFER_DTYPE)
        out.view(np.uint32)[...] = 0xDEADBEEF
        res = g.EvalGBuffer(block_num, samples=samples, out=out)
        part = res[0] if samples else res
        done = np.zeros((64, 64), bool)
        done[(xy[:block_num] >> 16) & 0xFFFF, xy[:block_num] & 0xFFFF] = True
        assert np.all(part.view(np.uint32).reshape(64, 64, 15)[~done] == 0xDEADBEEF), "records past blockNum were written"
        R.assert_records_equal(part[done], full[done], f"blockNum {block_num}: the records written")
        if samples:
            assert res[1].shape == (block_num, 16)
            R.assert_records_equal(res[1], full_raw[:block_num], f"blockNum {block_num}: raw samples")


# ---- 5. determinism and isolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_calls_give_identical_bytes():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(synth.material_zoo(96, 64))
    a, ar = g.EvalGBuffer(samples=True)
    b, br = g.EvalGBuffer(samples=True)
    assert a.tobytes() == b.tobytes() and ar.tobytes() == br.tobytes()
    assert g.EvalGBuffer().tobytes() == a.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["test_035", "material_zoo"])
def test_the_pass_draws_no_random_numbers_and_changes_no_state(scene_name):
    """A PathTraceBlock frame and the generator states rendered after EvalGBuffer equal those rendered without it."""
    from hydracore3_amd.api import HipIntegrator
    sc = _cornell() if scene_name == "test_035" else synth.material_zoo(96, 64)
    plain, withgb = HipIntegrator(sc), HipIntegrator(sc)
    g0 = withgb.random_gens()
    withgb.EvalGBuffer(samples=True)
    withgb.EvalGBuffer()
    assert np.array_equal(withgb.random_gens(), g0)
    a, b = plain.render(3), withgb.render(3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(plain.random_gens(), withgb.random_gens())
    withgb.EvalGBuffer()
    assert np.array_equal(plain.random_gens(), withgb.random_gens())
    assert np.array_equal(plain.render(2).view(np.uint32), withgb.render(2).view(np.uint32))


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_codes_and_messages():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    sc = _cornell()
    buf = np.zeros((64, 64), GBUFFER_DTYPE)

    def err(g):
        return g.L.hpt_last_error(g.h).decode()

    fresh = HipIntegrator()                                              # no scene yet
    assert fresh.L.hpt_eval_gbuffer(fresh.h, 1, buf.ctypes.data) == HPT_ERR_STATE and "CommitDeviceData" in err(fresh)
    assert fresh.L.hpt_eval_gbuffer_dev(fresh.h, 1, buf.ctypes.data, None, None) == HPT_ERR_STATE and "CommitDeviceData" in err(fresh)
    fresh.scene, fresh._desc = sc, sc.desc()
    fresh.CommitDeviceData()
    fresh.UpdateMembersPlainData(sc.params())
    assert fresh.L.hpt_eval_gbuffer(fresh.h, 1, buf.ctypes.data) == HPT_ERR_STATE and "PackXYBlock" in err(fresh)
    fresh.PackXYBlock(64, 64)
    assert fresh.L.hpt_eval_gbuffer(fresh.h, 64 * 64, buf.ctypes.data) == 0                   # no InitRandomGens needed
    assert buf["coverage"].max() == 1.0

    g = HipIntegrator(sc)
    assert g.L.hpt_eval_gbuffer(g.h, 64 * 64, None) == HPT_ERR_ARG and "null" in err(g)
    assert g.L.hpt_eval_gbuffer_dev(g.h, 64 * 64, None, None, None) == HPT_ERR_ARG and "null" in err(g)
    assert g.L.hpt_eval_gbuffer(None, 1, buf.ctypes.data) == HPT_ERR_ARG
    assert g.L.hpt_eval_gbuffer(g.h, 64 * 64 + 1, buf.ctypes.data) == HPT_ERR_ARG and "blockNum" in err(g)
    with pytest.raises(HydraHipError, match="blockNum"):
        g.EvalGBuffer(64 * 64 + 1)
    assert g.L.hpt_eval_gbuffer(g.h, 0, buf.ctypes.data) == 0
    g.L.hpt_set_accel_layout(g.h, 1)                                     # the committed tree is dropped until the next CommitScene
    assert g.L.hpt_eval_gbuffer(g.h, 1, buf.ctypes.data) == HPT_ERR_STATE and "CommitScene" in err(g)
    g.CommitScene()
    assert g.L.hpt_eval_gbuffer(g.h, 1, buf.ctypes.data) == 0


# ---- 7. spectral mode -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_spectral_mode_gives_the_same_records():
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    rgb = load_hydra_xml(scene_path("test_spectral"), 64, 48)
    spec = load_hydra_xml(scene_path("test_spectral"), 64, 48, spectral=True)
    assert spec.spectral_mode == 1 and rgb.spectral_mode == 0
    a, ar = HipIntegrator(rgb).EvalGBuffer(samples=True)
    b, br = HipIntegrator(spec).EvalGBuffer(samples=True)
    R.assert_records_equal(br, ar, "spectral vs RGB: raw samples")
    R.assert_records_equal(b, a, "spectral vs RGB: frame")
    ref_frame, ref_raw = R.eval_gbuffer(spec, OracleIntegrator(spec))
    R.assert_records_equal(br, ref_raw, "spectral: raw samples vs restatement", rgb_2ulp=R.srgb_textured(spec, ref_raw))
    loose = R.scatter(R.srgb_textured(spec, ref_raw).any(axis=1), HipIntegrator(spec).packed_xy(), 64, 48, np.zeros((48, 64), bool))
    R.assert_records_equal(b, ref_frame, "spectral: frame vs restatement", rgb_2ulp=loose)

"""CastSingleRayBlock and RayTraceBlock on the GPU against the numpy float32 restatement (tests/raytrace_reference.py), full frames compared as
uint32 views. The bar is equality. One exception, taken from the G-buffer tests: colours that passed through an sRGB texture decode. The
restatement decodes with the host's powf, which is off by one bit for a few arguments in 10^4 (profiles/gbuffer.md); the kernels round the
power correctly. The restatement says per pixel whether any term of its sum read a decoded texel:

* pixels without the flag, and the fourth / untouched channel of every pixel: equal, no exception;
* flagged pixels of CastSingleRayBlock: 3 ulp - the 2 ulp the G-buffer tests hold a decoded texel to, plus one for the one product
  (base colour x texel) that follows it;
* flagged pixels of RayTraceBlock: per pixel and channel, the distance between two CPU frames - the restatement as it is, and the restatement
  with the decode done as float32(float64(x) ** float64(float32(2.2))) on the filtered linear texel - plus one ulp of the pixel value per float32
  operation that follows the texel on the longest path. The count: base * texel (1), INV_PI * colour (2), intensity * that (3), * cosine (4),
  / distance^2 (5), shade += for each of the L light entries (5 + L), throughput * shade (6 + L), accum += (7 + L), one more accum += for
  each of the other depth - 1 vertices (6 + L + depth), out_color += (7 + L + depth). The emitter term is shorter (base * texel, throughput *,
  * atten, accum +=). So K = 7 + L + depth with L = the scene's light entries and depth = traceDepth.

The sweep, forced-sweep, interior and motion cases have NO flagged pixel (their textures are flagged linear in the test's copy of the scene where
needed, and the test asserts the count is 0), so a traversal fault cannot hide behind the exception.

Every test prints, per case, how many pixels were flagged, how many differed and the largest distance (profiles/whitted.md has the measured values).
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import raytrace_reference as RT
from conftest import ROOT, scene_path
from hydracore3_amd import synth
from hydracore3_amd.scene import load_hydra_xml
from traversal_scenes import forced_sweep_scene, sweep_scene

HPT_ERR_ARG, HPT_ERR_STATE = 1, 3
PATTERN = 0xDEADBEEF


def _linear(sc):
    """The scene with every texture flagged linear: no pixel of it can fall under the sRGB exception."""
    for t in sc.textures:
        t.srgb = False
    return sc


def _open_interior():
    """A miniature synth.interior_scene without its room: 24 instanced meshes (a tree, not the sweep) in front of the background."""
    sc = synth.interior_scene(64, 48, objects=24, subdiv=1, tex_size=16)
    sc.inst_geom.pop(0); sc.inst_matrices.pop(0); sc.remap_inst.pop(0)    # instance 0 is the closed room
    return _linear(sc)


def _motion_scene():
    seed = next(s for s in range(100) if synth.random_scene(s).inst_motion)
    return _linear(synth.random_scene(seed))


def _cornell():
    return load_hydra_xml(scene_path("test_035"), 64, 64)


# name -> (scene key, scene builder, HipIntegrator keyword arguments, options set before a re-commit, layout expected or None, may have flagged pixels)
CASES = {
    "test_035": ("test_035", _cornell, {}, {}, "sweep", True),
    "test_035 layout 1": ("test_035", _cornell, {"accel_layout": 1}, {}, "two-level", True),
    "test_035 layout 2": ("test_035", _cornell, {"accel_layout": 2}, {}, "flat", True),
    "test_035 layout 3": ("test_035", _cornell, {"accel_layout": 3}, {}, "sweep", True),
    "test_035 device_build 0": ("test_035", _cornell, {"accel_layout": 2}, {"device_build": 0}, "flat", True),
    "test_035 device_build 1": ("test_035", _cornell, {"accel_layout": 2}, {"device_build": 1}, "flat", True),
    "sweep_scene 11": ("sweep 11", lambda: _linear(sweep_scene(11)), {}, {}, "sweep", False),
    "sweep_scene 12": ("sweep 12", lambda: _linear(sweep_scene(12)), {}, {}, "sweep", False),
    "sweep_scene 13": ("sweep 13", lambda: _linear(sweep_scene(13)), {}, {}, "sweep", False),
    "forced_sweep_scene 21": ("forced 21", lambda: _linear(forced_sweep_scene(21)), {"accel_layout": 3}, {}, "sweep", False),
    "forced_sweep_scene 21 automatic": ("forced 21", lambda: _linear(forced_sweep_scene(21)), {}, {}, None, False),
    "material_zoo": ("material_zoo", lambda: synth.material_zoo(96, 64), {}, {}, None, True),
    "png_textures": ("png_textures", lambda: load_hydra_xml(scene_path("png_textures"), 64, 48), {}, {}, None, True),
    "jpg_textures": ("jpg_textures", lambda: load_hydra_xml(scene_path("jpg_textures"), 64, 48), {}, {}, None, True),
    "interior": ("interior", _open_interior, {}, {}, None, False),
    "interior two-level": ("interior", _open_interior, {"accel_layout": 1}, {}, "two-level", False),
    "motion": ("motion", _motion_scene, {}, {}, None, False),
    "motion single-level": ("motion", _motion_scene, {"accel_layout": 2}, {}, "flat", False),
}

# Every case has lit AND shadowed pixels in view, asserted on the restatement's own arrays - but for this one scene of the table, where
# nothing stands between the surfaces in view and the light: its 42 hit pixels are all lit (checked on the CPU; the other two sweep scenes
# have 17 and 37 shadowed pixels). It stays in the table for its traversal; scene key -> its number of hit pixels.
NOTHING_IN_THE_WAY = {"sweep 13": 42}

_scenes, _cast, _whitted = {}, {}, {}


def _scene(name):
    """(scene, oracle, oracle over the copy with linear textures), built once per scene."""
    key, build = CASES[name][:2]
    if key not in _scenes:
        from oracle.orc import OracleIntegrator
        sc = build()
        lin = RT.linear_copy(sc)
        _scenes[key] = (sc, OracleIntegrator(sc), OracleIntegrator(lin), lin)
    return _scenes[key][:3]


def _cast_reference(name):
    key = CASES[name][0]
    if key not in _cast:
        sc, cpu, cpu_lin = _scene(name)
        _cast[key] = RT.cast_single_ray(sc, cpu)
    return _cast[key]


def _whitted_reference(name, depth):
    """(restatement, restatement with the correctly rounded decode) at this trace depth, 4 channels."""
    key = (CASES[name][0], depth)
    if key not in _whitted:
        sc, cpu, cpu_lin = _scene(name)
        p = sc.params(trace_depth=depth)
        a = RT.ray_trace(sc, cpu, params=p)
        b = RT.ray_trace(sc, cpu, params=p, cpu_linear=cpu_lin) if a["srgb"].any() else a
        _whitted[key] = (a, b)
    return _whitted[key]


def _gpu(name, sc, params=None):
    from hydracore3_amd.api import HipIntegrator
    _, _, kw, opts, layout, _ = CASES[name]
    g = HipIntegrator(sc, params, **kw)
    if opts:
        for k, v in opts.items():
            g.set_option(k, v)
        g.CommitScene()
        if "device_build" in opts:
            assert bool(g.commit_time()["device_built"]) == bool(opts["device_build"])
    if layout is not None:
        assert g.accel_info()["layout"] == layout, g.accel_info()
    return g


def _to_frame(per_pixel, xy, h, w):
    out = np.zeros((h, w) + per_pixel.shape[1:], per_pixel.dtype)
    out[(xy >> 16) & 0xFFFF, xy & 0xFFFF] = per_pixel
    return out


def _compare(what, got, want, flagged, allowed):
    """got / want [h, w, c] float32; flagged [h, w] bool; allowed: ulp distance per flagged pixel and channel (scalar or [h, w, 3]). Channels
    past the third and every unflagged pixel: equal bits."""
    assert got.shape == want.shape and got.dtype == np.float32
    ug, uw = got.view(np.uint32), want.view(np.uint32)
    ne = ug != uw
    dist = RT.ulp_distance(got[..., :3], want[..., :3])
    n_diff = int(np.any(ne[..., :3], axis=-1).sum())
    n_diff_plain = int((np.any(ne[..., :3], axis=-1) & ~flagged).sum())
    print(f"{what}: {int(flagged.sum())} of {flagged.size} pixels flagged, {n_diff} differ ({n_diff_plain} of them unflagged), largest distance {int(dist.max())} ulp")
    assert not ne[..., 3:].any(), f"{what}: the untouched channel differs"
    assert not ne[..., :3][~flagged].any(), f"{what}: {n_diff_plain} unflagged pixels differ, largest distance {int(dist[~flagged].max())} ulp"
    over = flagged[..., None] & (dist > allowed)
    assert not over.any(), f"{what}: {int(np.any(over, axis=-1).sum())} flagged pixels differ by more than allowed; largest excess {int((dist - allowed)[over].max())} ulp"


# ---- 3. full frames against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_cast_single_ray_equals_the_restatement(name):
    sc, cpu, _ = _scene(name)
    ref = _cast_reference(name)
    key = CASES[name][0]
    assert ref["hit"].any(), name
    if key in ("test_035", "material_zoo", "interior"):
        assert (~ref["hit"]).any(), f"{name}: no pixel misses"
    if not CASES[name][5]:
        assert not ref["srgb"].any(), f"{name}: this case must have no pixel under the sRGB exception"
    g = _gpu(name, sc)
    xy = g.packed_xy()
    assert np.array_equal(xy, cpu.packed_xy())
    out = np.zeros((sc.height, sc.width, 4), np.uint32)
    out[...] = PATTERN
    out = out.view(np.float32)
    g.CastSingleRayBlock(g.N, out)
    _compare(f"{name}: CastSingleRayBlock", out, ref["frame"], _to_frame(ref["srgb"], xy, sc.height, sc.width), 3)
    assert g.last_kernel_ms() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_ray_trace_equals_the_restatement(name):
    """traceDepth 1 and the scene's own, channels 3 and 4, full frame (accumulation over a pre-filled frame is test_ray_trace_accumulates_and_pass_num_is_unused). Measured on an MI355X: see profiles/whitted.md."""
    sc, cpu, _ = _scene(name)
    key = CASES[name][0]
    rng = np.random.RandomState(5)
    for depth in sorted({1, int(sc.trace_depth)}):
        a, b = _whitted_reference(name, depth)
        assert a["hit"].any(), name
        if key in ("test_035", "material_zoo", "interior"):
            assert (~a["hit"]).any(), f"{name}: no pixel misses"
        if not CASES[name][5]:
            assert not a["srgb"].any(), f"{name}: this case must have no pixel under the sRGB exception"
        if depth > 1:                                                        # the case is exercised: lit and shadowed pixels, and light carried over a bounce
            assert sc.lights and a["lit"].any(), f"{name}: no lit pixel"
            if key in NOTHING_IN_THE_WAY:
                assert not a["shadowed"].any() and int(a["hit"].sum()) == NOTHING_IN_THE_WAY[key], f"{name}: the scene changed - hold it to a shadowed pixel like the others"
            else:
                assert a["shadowed"].any(), f"{name}: no shadowed pixel"
            if key == "material_zoo":
                assert any(v.any() for v in a["vertex"][1:]), "material_zoo: no pixel with a non-zero contribution after the first bounce"
        p = sc.params(trace_depth=depth)
        g = _gpu(name, sc, p)
        xy = g.packed_xy()
        flagged = _to_frame(a["srgb"], xy, sc.height, sc.width)
        K = 7 + len(sc.lights) + depth
        allowed = RT.ulp_distance(_to_frame(a["accum"], xy, sc.height, sc.width), _to_frame(b["accum"], xy, sc.height, sc.width)) + K
        for channels in (3, 4):                                              # colour channels start at 0 (0 + x = x exactly); the fourth holds a pattern
            out = np.zeros((sc.height, sc.width, channels), np.float32)
            if channels == 4:
                out[..., 3] = rng.rand(sc.height, sc.width).astype(np.float32)
            want = out.copy()
            want[..., :3] = (out[..., :3] + _to_frame(a["accum"], xy, sc.height, sc.width)).astype(np.float32)
            g.RayTraceBlock(g.N, channels, out)
            _compare(f"{name}: RayTraceBlock depth {depth}, {channels} channels", out, want, flagged, allowed)
        assert g.GetExecutionTime("RayTraceBlock")[0] > 0.0


# ---- 4. semantics -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tid", [1, 63, 64, 65, 1000, 64 * 64 - 1])
def test_cast_single_ray_assigns_and_leaves_pixels_past_tid(tid):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_cornell())
    full = np.zeros((64, 64, 4), np.float32)
    g.CastSingleRayBlock(g.N, full)
    assert np.all(full[..., 3] == 0.0) and full[..., :3].any()
    out = np.zeros((64, 64, 4), np.uint32)
    out[...] = PATTERN
    g.CastSingleRayBlock(tid, out.view(np.float32), 7)
    xy = g.packed_xy()
    done = np.zeros((64, 64), bool)
    done[(xy[:tid] >> 16) & 0xFFFF, xy[:tid] & 0xFFFF] = True
    assert np.all(out[~done] == PATTERN), "pixels past tid were written"
    assert np.array_equal(out[done], full.view(np.uint32)[done]), "assigned, w = 0, whatever the buffer held"


@pytest.mark.gpu
def test_ray_trace_accumulates_and_pass_num_is_unused():
    from hydracore3_amd.api import HipIntegrator
    sc = synth.material_zoo(96, 64)
    g = HipIntegrator(sc)
    a = np.zeros((64, 96, 4), np.float32)
    g.RayTraceBlock(g.N, 4, a, 1)
    assert a[..., :3].any() and not a[..., 3].any()
    twice = a.copy()
    g.RayTraceBlock(g.N, 4, twice, 7)
    assert np.array_equal(twice.view(np.uint32), (a + a).astype(np.float32).view(np.uint32)), "two calls = a + a; a_passNum changes nothing"
    pre = np.random.RandomState(1).rand(64, 96, 4).astype(np.float32)
    out = pre.copy()
    g.RayTraceBlock(g.N, 4, out)
    assert np.array_equal(out[..., 3], pre[..., 3]), "channel 3 of a 4-channel buffer is untouched"
    assert np.array_equal(out[..., :3].view(np.uint32), (pre[..., :3] + a[..., :3]).astype(np.float32).view(np.uint32))
    three = np.zeros((64, 96, 3), np.float32)
    g.RayTraceBlock(g.N, 3, three)
    assert np.array_equal(three.view(np.uint32), np.ascontiguousarray(a[..., :3]).view(np.uint32))
    part = np.zeros((64, 96, 4), np.float32)
    g.RayTraceBlock(1000, 4, part)
    xy = g.packed_xy()
    done = np.zeros((64, 96), bool)
    done[(xy[:1000] >> 16) & 0xFFFF, xy[:1000] & 0xFFFF] = True
    assert not part[~done].any() and np.array_equal(part[done], a[done])
    b = np.zeros((64, 96, 4), np.float32)
    g.RayTraceBlock(g.N, 4, b)
    assert a.tobytes() == b.tobytes(), "two calls give identical bytes"
    c1, c2 = np.zeros((64, 96, 4), np.float32), np.zeros((64, 96, 4), np.float32)
    g.CastSingleRayBlock(g.N, c1, 1); g.CastSingleRayBlock(g.N, c2, 7)
    assert c1.tobytes() == c2.tobytes()


@pytest.mark.gpu
def test_host_pointer_and_device_pointer_forms_give_the_same_bytes():
    import ctypes as C
    from hydracore3_amd.api import HipIntegrator
    sc = synth.material_zoo(96, 64)
    g = HipIntegrator(sc)
    pre = np.random.RandomState(2).rand(64, 96, 4).astype(np.float32)
    for which in ("cast", "rt"):
        host = pre.copy()
        if which == "cast":
            g.CastSingleRayBlock(g.N, host)
        else:
            g.RayTraceBlock(g.N, 4, host)
        dev = C.c_void_p()
        g._chk(g.L.hpt_device_malloc(g.h, pre.nbytes, C.byref(dev)))
        try:
            g._chk(g.L.hpt_device_copy(g.h, dev, pre.ctypes.data, pre.nbytes, 1))
            if which == "cast":
                g.cast_single_ray_block_dev(dev)
            else:
                g.ray_trace_block_dev(dev, channels=4)
            back = np.zeros_like(pre)
            g._chk(g.L.hpt_device_copy(g.h, back.ctypes.data, dev, pre.nbytes, 2))      # synchronous copy on the null stream: after the kernel
        finally:
            g.L.hpt_device_free(g.h, dev)
        assert back.tobytes() == host.tobytes(), which
        assert g.last_kernel_ms() > 0.0


@pytest.mark.gpu
def test_window_inside_a_larger_framebuffer():
    """A 20 x 10 window at (8, 6) of a 48 x 32 framebuffer, tileSize 2: 200 pixels (no multiple of 64 or 256, width no multiple of 16). Both
    passes equal the crop of the full frame and the restatement under the same parameters."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = _linear(sweep_scene(12))
    full = HipIntegrator(sc)
    fc, fr = np.zeros((sc.height, sc.width, 4), np.float32), np.zeros((sc.height, sc.width, 4), np.float32)
    full.CastSingleRayBlock(full.N, fc); full.RayTraceBlock(full.N, 4, fr)
    p = sc.params()
    p.winStartX, p.winStartY, p.winWidth, p.winHeight, p.tileSize = 8, 6, 20, 10, 2
    win = HipIntegrator(sc, p)
    assert (win.W, win.H, win.N) == (20, 10, 200)
    wc, wr = np.zeros((10, 20, 4), np.float32), np.zeros((10, 20, 4), np.float32)
    win.CastSingleRayBlock(win.N, wc); win.RayTraceBlock(win.N, 4, wr)
    assert np.array_equal(wc.view(np.uint32), fc[6:16, 8:28].view(np.uint32))
    assert np.array_equal(wr.view(np.uint32), fr[6:16, 8:28].view(np.uint32))
    cpu = OracleIntegrator(sc, p)
    assert np.array_equal(cpu.packed_xy(), win.packed_xy())
    rc, rr = RT.cast_single_ray(sc, cpu, p), RT.ray_trace(sc, cpu, p)
    assert not rc["srgb"].any() and not rr["srgb"].any()
    assert np.array_equal(wc.view(np.uint32), rc["frame"].view(np.uint32))
    assert np.array_equal(wr.view(np.uint32), rr["frame"].view(np.uint32))
    assert wr[..., :3].any() and wc[..., :3].any()


# ---- 5. isolation -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["test_035", "material_zoo"])
def test_the_passes_draw_no_random_numbers_and_change_no_state(scene_name):
    """A PathTraceBlock frame and the generator states rendered after the two passes equal those rendered without them."""
    from hydracore3_amd.api import HipIntegrator
    sc = _cornell() if scene_name == "test_035" else synth.material_zoo(96, 64)
    plain, withrt = HipIntegrator(sc), HipIntegrator(sc)
    g0 = withrt.random_gens()
    buf = np.zeros((sc.height, sc.width, 4), np.float32)
    withrt.CastSingleRayBlock(withrt.N, buf); withrt.RayTraceBlock(withrt.N, 4, buf)
    assert np.array_equal(withrt.random_gens(), g0)
    a, b = plain.render(3), withrt.render(3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(plain.random_gens(), withrt.random_gens())
    withrt.RayTraceBlock(withrt.N, 4, buf); withrt.CastSingleRayBlock(withrt.N, buf)
    assert np.array_equal(plain.random_gens(), withrt.random_gens())
    assert np.array_equal(plain.render(2).view(np.uint32), withrt.render(2).view(np.uint32))


@pytest.mark.gpu
def test_spectral_mode_gives_the_rgb_bytes():
    from hydracore3_amd.api import HipIntegrator
    rgb = load_hydra_xml(scene_path("test_spectral"), 64, 48)
    spec = load_hydra_xml(scene_path("test_spectral"), 64, 48, spectral=True)
    assert spec.spectral_mode == 1 and rgb.spectral_mode == 0
    frames = []
    for sc in (rgb, spec):
        g = HipIntegrator(sc)
        c, r = np.zeros((48, 64, 4), np.float32), np.zeros((48, 64, 4), np.float32)
        g.CastSingleRayBlock(g.N, c); g.RayTraceBlock(g.N, 4, r)
        frames.append((c, r))
    assert frames[0][0].tobytes() == frames[1][0].tobytes() and frames[0][1].tobytes() == frames[1][1].tobytes()
    assert frames[0][0][..., :3].any()


# ---- 6. errors and timing ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_error_codes_and_messages():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    sc = _cornell()
    buf = np.zeros((64, 64, 4), np.float32)
    N = 64 * 64

    def err(g):
        return g.L.hpt_last_error(g.h).decode()

    def calls(g, tid, ptr):
        return [("CastSingleRayBlock", lambda: g.L.hpt_cast_single_ray_block(g.h, tid, ptr, 1)),
                ("CastSingleRayBlock", lambda: g.L.hpt_cast_single_ray_block_dev(g.h, tid, ptr, 1, None)),
                ("RayTraceBlock", lambda: g.L.hpt_ray_trace_block(g.h, tid, 4, ptr, 1)),
                ("RayTraceBlock", lambda: g.L.hpt_ray_trace_block_dev(g.h, tid, 4, ptr, 1, None))]

    fresh = HipIntegrator()                                              # no scene yet
    for what, call in calls(fresh, 1, buf.ctypes.data):
        assert call() == HPT_ERR_STATE and "CommitDeviceData" in err(fresh) and what in err(fresh)
    fresh.scene, fresh._desc = sc, sc.desc()
    fresh.CommitDeviceData()
    fresh.UpdateMembersPlainData(sc.params())
    for what, call in calls(fresh, 1, buf.ctypes.data)[::2]:
        assert call() == HPT_ERR_STATE and "PackXYBlock" in err(fresh) and what in err(fresh)
    fresh.PackXYBlock(64, 64)
    assert fresh.L.hpt_cast_single_ray_block(fresh.h, N, buf.ctypes.data, 1) == 0      # no InitRandomGens needed
    assert buf[..., :3].any()
    assert fresh.L.hpt_ray_trace_block(fresh.h, N, 4, buf.ctypes.data, 1) == 0

    g = HipIntegrator(sc)
    for what, call in calls(g, N, None):
        assert call() == HPT_ERR_ARG and "null" in err(g) and what in err(g)
    assert g.L.hpt_cast_single_ray_block(None, 1, buf.ctypes.data, 1) == HPT_ERR_ARG
    assert g.L.hpt_ray_trace_block(None, 1, 4, buf.ctypes.data, 1) == HPT_ERR_ARG
    for what, call in calls(g, N + 1, buf.ctypes.data)[::2]:
        assert call() == HPT_ERR_ARG and "tid" in err(g) and what in err(g)
    with pytest.raises(HydraHipError, match="tid"):
        g.RayTraceBlock(N + 1, 4, buf)
    with pytest.raises(HydraHipError, match="tid"):
        g.CastSingleRayBlock(N + 1, buf)
    before = buf.copy()
    for what, call in calls(g, 0, buf.ctypes.data)[::2]:                # tid = 0 is a no-op
        assert call() == 0
    assert buf.tobytes() == before.tobytes()
    for channels in (1, 2):                                              # refused: the reference writes outside the pixel there
        assert g.L.hpt_ray_trace_block(g.h, N, channels, buf.ctypes.data, 1) == HPT_ERR_ARG and "channels" in err(g)
        assert g.L.hpt_ray_trace_block_dev(g.h, N, channels, buf.ctypes.data, 1, None) == HPT_ERR_ARG and "channels" in err(g)
        with pytest.raises(HydraHipError, match="channels"):
            g.RayTraceBlock(N, channels, buf)
    assert buf.tobytes() == before.tobytes()
    five = np.zeros((64, 64, 5), np.uint32)
    five[...] = PATTERN
    assert g.L.hpt_ray_trace_block(g.h, N, 5, five.ctypes.data, 1) == 0   # above 4 nothing is written, as in the reference
    assert np.all(five == PATTERN)
    g.L.hpt_set_accel_layout(g.h, 1)                                     # the committed tree is dropped until the next CommitScene
    for what, call in calls(g, 1, buf.ctypes.data)[::2]:
        assert call() == HPT_ERR_STATE and "CommitScene" in err(g) and what in err(g)
    g.CommitScene()
    for what, call in calls(g, 1, buf.ctypes.data)[::2]:
        assert call() == 0


@pytest.mark.gpu
def test_execution_time_slots():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(_cornell())
    buf = np.zeros((64, 64, 4), np.float32)
    assert g.GetExecutionTime("RayTraceBlock")[0] == 0.0 and g.GetExecutionTime("CastSingleRayBlock")[0] == 0.0
    g.CastSingleRayBlock(g.N, buf)
    cast = g.GetExecutionTime("CastSingleRayBlock")
    assert cast[0] > 0.0 and g.GetExecutionTime("RayTraceBlock")[0] == 0.0
    assert abs(g.last_kernel_ms() - cast[0]) < 1e-6
    g.RayTraceBlock(g.N, 4, buf)
    rt = g.GetExecutionTime("RayTraceBlock")
    assert rt[0] > 0.0 and all(v >= 0.0 for v in rt[:3])
    assert g.GetExecutionTime("CastSingleRayBlock") == cast
    g.render(2)                                                          # a PathTraceBlock call does not move them
    assert g.GetExecutionTime("RayTraceBlock") == rt and g.GetExecutionTime("CastSingleRayBlock") == cast
    assert g.GetExecutionTime("PathTraceBlock")[0] > 0.0


# ---- 7. the HR2 driver in its preview mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hr2_driver_preview_mode_returns_cast_single_ray_block():
    from hydracore3_amd.api import HipIntegrator
    tool = os.path.join(ROOT, "hydracore3_amd", "hydra_hip_hr2_preview")
    assert os.path.exists(tool), "build() compiles tests/cpp/hydra_hip_hr2_preview.cpp"
    xml = scene_path("test_035")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "preview.bin")
        r = subprocess.run([tool, xml, "64", "64", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        frame = np.fromfile(out, np.float32).reshape(64, 64, 4)
    g = HipIntegrator(load_hydra_xml(xml, 64, 64))
    want = np.zeros((64, 64, 4), np.float32)
    g.CastSingleRayBlock(g.N, want)
    assert want[..., :3].any()
    assert frame.tobytes() == want.tobytes()

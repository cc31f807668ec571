"""CastSingleRayBlock / RayTraceBlock without a GPU: the ABI surface of the four entry points, and the numpy restatement
(tests/raytrace_reference.py) against hand-built scenes with closed-form answers. The closed forms take the pixel's ray from the restatement's
eye_rays (the camera model has its own tests) and do everything after it in float64."""
import os
import re

import numpy as np

import raytrace_reference as RT
from conftest import ROOT
from hydracore3_amd import scene as S
from hydracore3_amd import synth

SYMBOLS = ["hpt_cast_single_ray_block", "hpt_cast_single_ray_block_dev", "hpt_ray_trace_block", "hpt_ray_trace_block_dev"]
# relative bound for a closed form evaluated in float64 against the float32 restatement: the ray direction, the hit distance and the hit point
# each carry a few 2^-24, the formula a dozen more operations; 64 * 2^-24 = 3.8e-6 as in test_gbuffer_cpu.py
REL = 64 * 2.0 ** -24


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_four_symbols_and_the_front_end_binds_them():
    from hydracore3_amd import api
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/hydra_hip.h"
        assert name in api.ABI, f"{name} is not in api.ABI"
        restype, argtypes = api.ABI[name]
        assert len(argtypes) == len(m.group(1).split(",")), (name, m.group(1))
    assert [a.split()[-1].lstrip("*") for a in re.search(r"hpt_ray_trace_block\s*\(([^)]*)\)", hdr).group(1).split(",")] == ["ctx", "tid", "channels", "out_color", "passNum"]
    for meth in ("CastSingleRayBlock", "RayTraceBlock", "cast_single_ray_block_dev", "ray_trace_block_dev"):
        assert hasattr(api.HipIntegrator, meth)
    assert '("raytrace", "hpt_raytrace.hip"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "hydracore3_amd", "csrc", "hpt_raytrace.hip"))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def _down_camera(sc, width, height, d):
    sc.width, sc.height = width, height
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, d, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)
    sc.fov = 40.0


def _checker(n=4):
    rng = np.random.RandomState(7)
    return (rng.randint(1, 255, size=(n, n, 4)) / 256.0).astype(np.float32)


def _textured_quad(base=(0.5, 0.25, 0.75, 0.0), half=4.0, width=40, height=24):
    """A quad in y = 0 of half-size `half` seen from (0, 2, 0) straight down, with a 4 x 4 float texture, nearest filter, not sRGB."""
    sc = S.SceneData()
    _down_camera(sc, width, height, 2.0)
    sc.trace_depth = 1
    tex = sc.add_texture(S.Texture(_checker(), S.TEX_RGBA32F, False, filt=S.FILTER_NEAREST))
    m = S.material_lambert(base[:3], tex_id=tex)
    m["colors"][S.GLTF_COLOR_BASE][3] = base[3]
    sc.materials.append(m)
    p, n, t, uv, idx = synth._quad((-half, 0, half), (2 * half, 0, 0), (0, 0, -2 * half))
    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
    return sc


def _rays(cpu):
    xy = cpu.packed_xy()
    pos, dr = RT.eye_rays(cpu.params, xy)
    return xy, pos[:, :3].astype(np.float64), dr[:, :3].astype(np.float64)


def _by_packed(frame, xy):
    return frame[(xy >> 16) & 0xFFFF, xy & 0xFFFF]


# ---- 2. CastSingleRay -----------------------------------------------------------------------------------------------------------------------------
def test_cast_single_ray_is_base_times_the_texel_at_the_pixel_centre():
    from oracle.orc import OracleIntegrator
    base = (0.5, 0.25, 0.75, 0.0)
    h = 1.25                                                             # the view spans |x| < 1.22, |z| < 0.73 at the quad: it fills the view, 4 x 3 texels in sight
    sc = _textured_quad(base, half=h)
    cpu = OracleIntegrator(sc)
    res = RT.cast_single_ray(sc, cpu)
    assert res["hit"].all() and not res["srgb"].any()
    xy, o, d = _rays(cpu)
    t = -o[:, 1] / d[:, 1]
    P = o + t[:, None] * d
    s, tt = (P[:, 0] + h) / (2 * h), (h - P[:, 2]) / (2 * h)                # the quad's parametrisation (synth._quad)
    away = (np.abs(s * 4 - np.round(s * 4)) > 1e-3) & (np.abs(tt * 4 - np.round(tt * 4)) > 1e-3)   # pixels whose centre is not on a texel border
    assert away.sum() > 0.9 * away.size
    texels = _checker()[np.floor(tt * 4).astype(int), np.floor(s * 4).astype(int)]
    want = (np.asarray(base[:3], np.float32)[None, :] * texels[:, :3]).astype(np.float32)      # one float32 product
    got = _by_packed(res["frame"], xy)
    assert np.array_equal(got[away, :3], want[away])
    assert np.all(got[:, 3] == 0.0)
    assert np.unique(want[away], axis=0).shape[0] >= 8                    # several texels are in view


def test_cast_single_ray_base_alpha_gives_the_clamped_splat():
    from oracle.orc import OracleIntegrator
    for w, want in ((0.7, np.float32(0.7)), (1.5, np.float32(1.0))):
        sc = _textured_quad((0.5, 0.25, 0.75, w))
        res = RT.cast_single_ray(sc, OracleIntegrator(sc))
        assert np.all(res["frame"][..., :3] == want) and np.all(res["frame"][..., 3] == 0.0)


def test_cast_single_ray_miss_gives_four_zeros_at_its_own_pixel_and_nowhere_else():
    from oracle.orc import OracleIntegrator
    sc = _textured_quad(half=0.4)                                         # the quad covers the middle of the view only
    cpu = OracleIntegrator(sc)
    n = sc.width * sc.height
    tid = n - 37
    pattern = np.full((sc.height, sc.width, 4), 0, np.uint32)
    pattern[...] = 0xDEADBEEF
    res = RT.cast_single_ray(sc, cpu, tid=tid, into=pattern.view(np.float32))
    xy = cpu.packed_xy()
    got = _by_packed(res["frame"], xy).view(np.uint32)
    hit = res["hit"]
    assert hit.any() and (~hit).any() and hit.shape == (tid,)
    assert np.all(got[:tid][~hit] == 0), "a miss assigns 0 to the four floats of its own pixel"
    assert np.all(got[tid:] == 0xDEADBEEF), "pixels past tid keep their contents"
    assert np.all(got[:tid][hit][:, 3] == 0) and np.all(got[:tid][hit][:, :3] != 0xDEADBEEF) and np.all(_by_packed(res["frame"], xy)[:tid][hit][:, :3] > 0)


# ---- 3. Whitted -----------------------------------------------------------------------------------------------------------------------------------
def _lit_plane(occluder=False, light_up=False, albedo=0.5, intensity=(10.0, 7.0, 3.0)):
    sc = synth.plane_under_rect_light(48, 32, albedo=albedo)
    sc.lights[0]["intensity"] = (*intensity, 0.0)
    if light_up:
        sc.lights[0]["norm"] = (0.0, 1.0, 0.0, 0.0)
    if occluder:                                                          # a square of half-size 0.25 at y = 1, under the light at (0, 2, 0): its shadow on the floor is |x|, |z| < 0.5
        p, n, t, uv, idx = synth._quad((-0.25, 1.0, 0.25), (0.5, 0, 0), (0, 0, -0.5))
        sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
    return sc


def test_whitted_lambert_plane_under_one_light_is_the_point_light_formula():
    """pixel = I * albedo / pi * cos / d^2 with the light taken as a point at lights[0].pos, whatever its type (here a rect light)."""
    from oracle.orc import OracleIntegrator
    sc = _lit_plane()
    cpu = OracleIntegrator(sc)
    res = RT.ray_trace(sc, cpu)
    assert res["hit"].all() and res["lit"].all() and not res["shadowed"].any()
    xy, o, d = _rays(cpu)
    P = o + ((-o[:, 1] / d[:, 1]) * (1.0 - 1e-6))[:, None] * d              # kernel_RayTrace2 places the vertex at t * (1 - 1e-6): 1e-6 of the ray above the floor
    L = np.array([0.0, 2.0, 0.0])
    dist = np.linalg.norm(L - P, axis=1)
    cos = (L - P)[:, 1] / dist
    want = np.array([10.0, 7.0, 3.0])[None, :] * (0.5 / np.pi) * (cos / dist ** 2)[:, None]
    got = _by_packed(res["frame"], xy).astype(np.float64)
    rel = np.abs(got[:, :3] - want) / want
    print("lambert plane: worst relative error", rel.max())
    assert rel.max() < REL
    assert np.all(got[:, 3] == 0.0)                                       # the fourth channel is never touched
    # accumulation: a second call over the first frame gives a + a
    twice = RT.ray_trace(sc, cpu, into=res["frame"])["frame"]
    assert np.array_equal(twice[..., :3], (res["frame"][..., :3] + res["frame"][..., :3]).astype(np.float32))
    # three channels: the same numbers at a stride of three
    assert np.array_equal(RT.ray_trace(sc, cpu, channels=3)["frame"], res["frame"][..., :3])
    # above four channels nothing is written
    assert not RT.ray_trace(sc, cpu, channels=5)["frame"].any()


def test_whitted_is_zero_behind_an_occluder_and_where_the_light_faces_away():
    from oracle.orc import OracleIntegrator
    sc = _lit_plane(occluder=True)
    cpu = OracleIntegrator(sc)
    res = RT.ray_trace(sc, cpu)
    xy, o, d = _rays(cpu)
    got = _by_packed(res["frame"], xy)
    t_occ = (1.0 - o[:, 1]) / d[:, 1]                                    # pixels that see the occluder itself: its top faces the light, unoccluded
    Pq = o + t_occ[:, None] * d
    sees_occ = (np.abs(Pq[:, 0]) < 0.25) & (np.abs(Pq[:, 2]) < 0.25)
    P = o + (-o[:, 1] / d[:, 1])[:, None] * d
    in_shadow = ~sees_occ & (np.abs(P[:, 0]) < 0.49) & (np.abs(P[:, 2]) < 0.49)
    clear = ~sees_occ & ((np.abs(P[:, 0]) > 0.51) | (np.abs(P[:, 2]) > 0.51)) & ~((np.abs(Pq[:, 0]) < 0.26) & (np.abs(Pq[:, 2]) < 0.26))
    assert in_shadow.sum() >= 4 and clear.sum() > 100
    assert np.all(got[in_shadow] == 0.0) and res["shadowed"][in_shadow].all()
    assert np.all(got[clear][:, :3] > 0.0) and res["lit"][clear].all()
    up = _lit_plane(light_up=True)
    res_up = RT.ray_trace(up, OracleIntegrator(up))
    assert res_up["hit"].all() and not res_up["frame"].any() and not res_up["lit"].any()


def _mirror_under_emitter(c=(0.9, 0.6, 0.3), emission=(4.0, 2.0, 1.0), depth=2):
    sc = S.SceneData()
    sc.width, sc.height = 48, 32
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    sc.fov, sc.trace_depth = 35.0, depth
    m = S.material_gltf((0.8, 0.8, 0.8), metalness=1.0)
    m["colors"][S.GLTF_COLOR_METAL] = (*c, 0.0)
    sc.materials.append(m)
    sc.materials.append(S.material_emissive(emission))
    p, n, t, uv, idx = synth._quad((-50, 0, 50), (100, 0, 0), (0, 0, -100))
    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
    p, n, t, uv, idx = synth._quad((-1000, 5, -1000), (2000, 0, 0), (0, 0, 2000))
    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [1]), np.eye(4))
    return sc


def test_whitted_mirror_facing_an_emitter_is_colour_times_cosine_times_emission():
    from oracle.orc import OracleIntegrator
    c, e = (0.9, 0.6, 0.3), (4.0, 2.0, 1.0)
    sc = _mirror_under_emitter(c, e)
    cpu = OracleIntegrator(sc)
    res = RT.ray_trace(sc, cpu)
    xy, o, d = _rays(cpu)
    assert np.all(d[:, 1] < 0) and res["hit"].all()
    want = np.array(c)[None, :] * (-d[:, 1])[:, None] * np.array(e)[None, :]
    got = _by_packed(res["frame"], xy).astype(np.float64)[:, :3]
    rel = np.abs(got - want) / want
    print("mirror: worst relative error", rel.max())
    assert rel.max() < REL
    assert not res["vertex"][0].any() and np.array_equal(res["vertex"][1], res["accum"])     # everything arrives at the second vertex
    # one bounce only: the path ends on the mirror, which has no light entry to gather from
    one = RT.ray_trace(sc, cpu, params=sc.params(trace_depth=1))
    assert not one["frame"].any()


def test_whitted_trace_depth_zero_adds_nothing():
    from oracle.orc import OracleIntegrator
    sc = _lit_plane()
    cpu = OracleIntegrator(sc)
    into = np.random.RandomState(3).rand(sc.height, sc.width, 4).astype(np.float32)
    res = RT.ray_trace(sc, cpu, params=sc.params(trace_depth=0), into=into)
    assert np.array_equal(res["frame"][..., 3], into[..., 3])
    assert np.array_equal(res["frame"][..., :3], (into[..., :3] + np.float32(0.0)).astype(np.float32)) and not res["accum"].any()


def test_whitted_emitter_with_a_light_id_is_seen_from_below_only():
    """lightDirectionAtten: with a lightId the emitter counts where dot(rayDir, (0, -1, 0)) < 0, i.e. for rays that travel upwards."""
    from oracle.orc import OracleIntegrator
    e = (4.0, 2.0, 1.0)
    for cam_y, light_id, want in ((-3.0, 0, e), (3.0, 0, (0.0, 0.0, 0.0)), (3.0, S.UINT_MAX, e), (-3.0, S.UINT_MAX, e)):
        sc = S.SceneData()
        _down_camera(sc, 16, 12, cam_y)
        sc.trace_depth = 2
        sc.materials.append(S.material_emissive(e, light_id=light_id))
        sc.lights.append(S.light_rect(S.translate(0, 0, 0), 5.0, 5.0, (1, 1, 1), 1.0))
        p, n, t, uv, idx = synth._quad((-50, 0, 50), (100, 0, 0), (0, 0, -100))
        sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
        res = RT.ray_trace(sc, OracleIntegrator(sc))
        assert res["hit"].all()
        assert np.all(res["frame"][..., :3] == np.asarray(want, np.float32)), (cam_y, light_id)

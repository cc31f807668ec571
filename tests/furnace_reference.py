"""Two furnaces for the multi-bounce estimator: scenes in which every single sample has a value known in advance, in float64. Not a test.

Written from the definitions and from the reference's text, cited by line; nothing here is taken from the device code or from the oracle,
and nothing here calls either. What the closed forms rest on (integrator_pt.cpp):

  * PathTrace (:735-752) runs m_traceDepth iterations of  trace - light sample - next bounce;  NaivePathTrace (:696) runs m_traceDepth + 1
    iterations of  trace - next bounce;  neither has Russian roulette.
  * kernel_NextBounce (:524-530): the light sample is added with the throughput as it was BEFORE the bounce, then the throughput is multiplied
    by cosTheta * val / max(pdf, 1e-20) (:510-511). For the Lambert lobe (val = rho / pi, cosine sampling, pdf = cos / pi) that factor is rho, up
    to rounding.
  * a hit on a MAT_TYPE_LIGHT_SOURCE material ends the path (:461-506): an emitting wall reflects nothing, so a closed box of emitting and
    reflecting walls does not exist here. The furnaces use a delta light and a constant environment instead.
  * kernel_SampleLightSource (:384-420): shade = intensity * bsdf / lgtPdfW * max(dot(shadowRayDir, hit.norm), 0). hit.norm is the INTERPOLATED
    vertex normal (kernel_RayTrace2, :270-298), not the triangle's: the cosine in S below is taken against the radial normal and is 1.
    For an omni light LightEvalPDF gives pdfA r^2 / cos' with pdfA = 1 and cos' = 1 (the `point` case of tests/light_integrals_reference.py,
    pinned on the device), a point light gets MIS weight 1 (:410-411), one light is picked with probability 1.
  * a ray that leaves the scene: kernel_RayTrace2 (:343-347) sets RAY_FLAG_OUT_OF_SCENE, at bounce 0 also RAY_FLAG_PRIME_RAY_MISS; kernel_HitEnvironment
    (:550-594) then adds throughput * environment colour. `exitZero` (:564) only switches the MIS weight of a SAMPLED map off and selects the camera
    back texture when there is one (:579); with a constant colour and no back texture a primary miss is the environment colour itself, k = 0 below.

Scene S, the integrating sphere: an icosphere of radius R around an omni light of intensity I at its centre, vertex normals radial and inward,
Lambert albedo rho, no environment. At a wall point x the light sample is  rho / pi * I / |x|^2  (cosine 1, nothing occludes inside a convex
wall), every continuation meets the wall again, so under INTEGRATOR_SHADOW_PT and INTEGRATOR_MIS_PT a sample is, per channel,

      V = rho / pi * I * sum_{k < D} rho^k / |x_k|^2,      D = trace depth.

|x_k| lies between r_in, the smallest distance of any triangle to the centre (computed here from the float32 vertices the scene uploads), and
R: V_lo has every |x_k| = R, V_hi every |x_k| = r_in. At subdivision 5 the interval is 0.057 % wide (0.23 % at 4). NaivePathTrace gives exactly 0: a delta light
cannot be hit.

Scene C, the cavity: an open-topped cube of Lambert walls under a constant sky, no lights. A sample is 0 (every trace of the loop hit a wall)
or  env_c * rho_c^k  with one integer k for the three channels: k = 0 a primary miss, 1 <= k <= k_max a path that left after k bounces;
k_max = D - 1 for PathTrace (the D-th trace is the last, a miss there has seen D - 1 bounces), D for NaivePathTrace.

EPS: the rounding allowance of both, measured on the oracle (tests/test_furnace_cpu.py asserts the measurement, profiles/furnace.md has the figures).
CAP: the share of samples (C) or pixels (S) of one run that may miss - an edge leak between two triangles, a continuation that passes under a
flat triangle whose shading normal is radial, a pdf guard at grazing incidence. A condition of the scenes, not a tolerance of the kernels.
"""
import functools
import math

import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.synth import _merge, _quad

ALBEDO = (0.25, 0.5, 0.75)
GREY = (0.5, 0.5, 0.5)
WIDTH, HEIGHT = 48, 40                      # 1920 pixels: no multiple of 256 or 64, the block and wave tails run

# ---- S ------------------------------------------------------------------------------------------------------------------------------------
RADIUS = 2.0
INTENSITY = 10.0
SUBDIV = 5                                  # 20480 triangles; at 4 (5120) the oracle's leak rate is 9.8e-4 of the samples, over CAP_ORACLE: profiles/furnace.md
S_CAM_POS, S_CAM_LOOK_AT, S_CAM_UP, S_FOV = (0.6, 0.2, -0.4), (-0.3, 0.1, 1.5), (0.0, 1.0, 0.0), 100.0
DEPTHS = (1, 2, 3, 6)

# ---- C ------------------------------------------------------------------------------------------------------------------------------------
ENV = (1.0, 2.0, 0.5)
C_DEPTH = 6
C_CAM_POS, C_CAM_LOOK_AT, C_CAM_UP, C_FOV = (0.4, 4.5, 0.7), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 50.0
DARK = -1                                   # classify(): a sample that is exactly 0 in every channel

# ---- the allowances -----------------------------------------------------------------------------------------------------------------------
# four times the oracle's worst relative excursion beyond the analytic interval on S (depths 1, 2, 3, 6, 4 passes, both integrator types) and beyond
# the exact power on C (8 one-pass frames, PathTrace and NaivePathTrace): S 0 (no pixel mean leaves the interval by rounding), C 6.279e-7
# (profiles/furnace.md); tests/test_furnace_cpu.py measures both again and asserts 4 x worst <= EPS < 1e-4
EPS = 2.52e-6
CAP = 1e-3                                  # of the samples / pixels of any one run
CAP_ORACLE = 5e-4


@functools.lru_cache(maxsize=None)
def sphere_mesh(subdiv=SUBDIV, radius=RADIUS):
    """The wall of S: (pos4, norm4, tang4, uv, idx) with the normals radial and INWARD."""
    v, f = synth.icosphere(subdiv)
    nv = v.shape[0]
    pos4 = np.concatenate([v * radius, np.ones((nv, 1))], 1).astype(np.float32)
    norm4 = np.concatenate([-v, np.zeros((nv, 1))], 1).astype(np.float32)
    tang = np.stack([-v[:, 2], np.zeros(nv), v[:, 0]], 1)
    ln = np.linalg.norm(tang, axis=1, keepdims=True)
    tang = np.where(ln > 1e-6, tang / np.maximum(ln, 1e-6), np.array([[1.0, 0.0, 0.0]]))
    tang4 = np.concatenate([tang, np.zeros((nv, 1))], 1).astype(np.float32)
    uv = np.zeros((nv, 2), np.float32)
    return pos4, norm4, tang4, uv, f.reshape(-1)


def sphere_scene(depth, albedo=ALBEDO, subdiv=SUBDIV, tex_id=0, width=WIDTH, height=HEIGHT) -> S.SceneData:
    sc = S.SceneData()
    sc.width, sc.height = width, height
    sc.cam_pos, sc.cam_look_at, sc.cam_up = S_CAM_POS, S_CAM_LOOK_AT, S_CAM_UP
    sc.fov, sc.trace_depth = S_FOV, depth
    sc.materials.append(S.material_lambert(tuple(albedo), tex_id))
    p, n, t, uv, idx = sphere_mesh(subdiv)
    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
    sc.lights.append(S.light_point(np.eye(4), (1.0, 1.0, 1.0), INTENSITY, "omni"))
    return sc


def cavity_scene(depth=C_DEPTH, width=WIDTH, height=HEIGHT) -> S.SceneData:
    sc = S.SceneData()
    sc.width, sc.height = width, height
    sc.cam_pos, sc.cam_look_at, sc.cam_up = C_CAM_POS, C_CAM_LOOK_AT, C_CAM_UP
    sc.fov, sc.trace_depth = C_FOV, depth
    sc.env_color = (*ENV, 0.0)
    sc.materials.append(S.material_lambert(ALBEDO))
    X, Y, Z = 1.0, 2.0, 1.0
    parts = [(*_quad((-X, 0, Z), (2 * X, 0, 0), (0, 0, -2 * Z), 3, 3), 0),       # floor (+y)
             (*_quad((-X, 0, -Z), (2 * X, 0, 0), (0, Y, 0), 3, 3), 0),           # back wall (+z)
             (*_quad((X, 0, Z), (-2 * X, 0, 0), (0, Y, 0), 3, 3), 0),            # front wall (-z)
             (*_quad((-X, 0, Z), (0, 0, -2 * Z), (0, Y, 0), 3, 3), 0),           # left wall (+x)
             (*_quad((X, 0, -Z), (0, 0, 2 * Z), (0, Y, 0), 3, 3), 0)]            # right wall (-x)
    sc.add_instance(sc.add_mesh(*_merge(parts)), np.eye(4))
    return sc


# ---- S: the closed form -------------------------------------------------------------------------------------------------------------------
def _closest_to_origin(a, b, c):
    """Distance of the origin to each triangle (a, b, c [m, 3]): the foot of the plane when it lies inside, else the nearest edge point."""
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    foot = n * np.sum(a * n, 1, keepdims=True)
    inside = np.ones(a.shape[0], bool)
    for p, q in ((a, b), (b, c), (c, a)):
        inside &= np.sum(np.cross(q - p, foot - p) * n, 1) >= 0.0
    d = np.full(a.shape[0], np.inf)
    for p, q in ((a, b), (b, c), (c, a)):
        e = q - p
        t = np.clip(-np.sum(p * e, 1) / np.sum(e * e, 1), 0.0, 1.0)
        d = np.minimum(d, np.linalg.norm(p + t[:, None] * e, axis=1))
    return np.where(inside, np.linalg.norm(foot, axis=1), d)


def sphere_radii(sc: S.SceneData):
    """(r_in, r_out) of the mesh the scene uploads, in float64 from its float32 vertices: the smallest distance of any triangle to the centre and
    the largest distance of any vertex."""
    v = sc.vpos[:, :3].astype(np.float64)
    tri = sc.tri_indices.reshape(-1, 3)
    return float(_closest_to_origin(v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]).min()), float(np.linalg.norm(v, axis=1).max())


def sphere_interval(sc: S.SceneData, depth=None, albedo=ALBEDO):
    """(V_lo [3], V_hi [3]) of one sample of S under PathTrace."""
    depth = sc.trace_depth if depth is None else depth
    r_in, r_out = sphere_radii(sc)
    rho = np.asarray(albedo, np.float64)
    series = sum(rho ** k for k in range(depth))
    v = rho / math.pi * INTENSITY * series
    return v / (r_out * r_out), v / (r_in * r_in)


def luminance(rgb):
    """The moments record's luminance (Rec. 709 weights)."""
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def outside_interval(values, lo, hi, eps=EPS):
    """values [..., c] (means of samples) -> bool [...]: some channel outside [lo (1 - eps), hi (1 + eps)], or not finite."""
    v = np.asarray(values, np.float64)
    lo, hi = np.asarray(lo)[:v.shape[-1]], np.asarray(hi)[:v.shape[-1]]
    return ~np.all(np.isfinite(v) & (v >= lo * (1 - eps)) & (v <= hi * (1 + eps)), axis=-1)


def interval_excursion(values, lo, hi):
    """The relative excursion beyond [lo, hi] per element [...], 0 inside (the largest over the channels)."""
    v = np.asarray(values, np.float64)
    lo, hi = np.asarray(lo)[:v.shape[-1]], np.asarray(hi)[:v.shape[-1]]
    return np.maximum(np.maximum((lo - v) / lo, (v - hi) / hi), 0.0).max(-1)


def _check_depths():
    """An off-by-one in depth must stand clear of the interval: for every depth of DEPTHS and both neighbours, the gap exceeds four interval
    widths in at least one channel. A depth that fails is dropped (none does)."""
    sc = sphere_scene(1)
    keep = []
    for d in DEPTHS:
        lo, hi = sphere_interval(sc, d)
        width = hi - lo
        ok = True
        for other in (d - 1, d + 1):
            lo2, hi2 = sphere_interval(sc, other) if other > 0 else (np.zeros(3), np.zeros(3))
            gap = np.maximum(lo - hi2, lo2 - hi)
            ok &= bool(np.any(gap > 4 * np.maximum(width, hi2 - lo2)))
        if ok:
            keep.append(d)
    return tuple(keep)


DEPTHS = _check_depths()
assert DEPTHS == (1, 2, 3, 6), DEPTHS


# ---- C: the closed form -------------------------------------------------------------------------------------------------------------------
def k_max(depth=C_DEPTH, naive=False):
    return depth if naive else depth - 1


def cavity_value(k, albedo=ALBEDO, env=ENV):
    return np.asarray(env, np.float64) * np.asarray(albedo, np.float64) ** k


def classify_frame(frame, kmax, eps=EPS, albedo=ALBEDO, env=ENV):
    """frame [..., >= 3] of single samples -> (k int [...], ok bool [...]): k = DARK where the sample is exactly 0, else the power read off the
    green channel (adjacent powers are a factor 0.5 apart); ok where it is DARK or 0 <= k <= kmax and every channel is env_c rho_c^k (1 +- eps)."""
    v = np.asarray(frame, np.float64)[..., :3]
    rho, e = np.asarray(albedo, np.float64), np.asarray(env, np.float64)
    dark = np.all(v == 0.0, axis=-1)
    g = np.where(np.isfinite(v[..., 1]) & (v[..., 1] > 0), v[..., 1], 1.0)
    k = np.rint(np.log(g / e[1]) / math.log(rho[1])).astype(np.int64)
    want = e * rho ** np.clip(k, 0, 64)[..., None]
    ok = np.all(np.isfinite(v), axis=-1) & (k >= 0) & (k <= kmax) & np.all(np.abs(v - want) <= eps * want, axis=-1)
    return np.where(dark, DARK, k), ok | dark


def classify_red_frame(frame, kmax, eps=EPS, albedo=ALBEDO, env=ENV):
    """classify_frame for a one-channel frame [...], which holds the red channel alone (kernel_ContributeToImage, :631-635): env_r rho_r^k, adjacent
    powers a factor 0.25 apart. Returns (k, ok) alike."""
    v = np.asarray(frame, np.float64)
    rho, e = float(albedo[0]), float(env[0])
    dark = v == 0.0
    g = np.where(np.isfinite(v) & (v > 0), v, 1.0)
    k = np.rint(np.log(g / e) / math.log(rho)).astype(np.int64)
    want = e * rho ** np.clip(k, 0, 64)
    ok = np.isfinite(v) & (k >= 0) & (k <= kmax) & (np.abs(v - want) <= eps * want)
    return np.where(dark, DARK, k), ok | dark


def classify(sample, kmax, eps=EPS):
    """One sample (three floats) -> k, DARK, or None when it is no value a sample of C can take."""
    k, ok = classify_frame(np.asarray(sample, np.float64)[None, :], kmax, eps)
    return int(k[0]) if ok[0] else None


def power_excursion(frame, kmax):
    """The worst relative distance of the frame's lit samples from the nearest exact power (those within 1e-3 of one: the others are no
    rounding, they are counted by the cap)."""
    v = np.asarray(frame, np.float64)[..., :3]
    k, ok = classify_frame(v, kmax, 1e-3)
    lit = ok & (k >= 0)
    if not lit.any():
        return 0.0
    want = cavity_value(k[lit][:, None])
    return float(np.max(np.abs(v[lit] - want) / want))


# ---- rays inside S for PathTraceFromInputRaysBlock -------------------------------------------------------------------------------------------
def sphere_input_rays(n, seed=7):
    """n camera-space rays (float32 [n, 4] positions and directions) whose float64 origins lie within 0.6 R of the centre, directions uniform."""
    r = np.random.RandomState(seed)
    o = r.normal(size=(n, 3))
    o *= (0.6 * RADIUS * r.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(o, axis=1, keepdims=True)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    wv = S.look_at(S_CAM_POS, S_CAM_LOOK_AT, S_CAM_UP)
    pos, dr = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = o @ wv[:3, :3].T + wv[:3, 3]
    dr[:, :3] = d @ wv[:3, :3].T
    return pos, dr

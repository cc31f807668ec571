"""float64 statement of first-bounce direct lighting on a Lambert floor, and the case table of the light-integral tests. Not a test.

Written from the radiometric definitions and from the reference's conventions, cited by line; nothing here is taken from the device code
or from the oracle, and nothing here calls either. For a floor point P (normal n = +y, albedo rho) the module gives, per colour channel,

  I      the expected radiance leaving P: the integral of  rho/pi * Le * cos * cos' / r^2  over the emitter (or its delta-light form);
  sigma  the standard deviation of the renderer's ONE-SAMPLE light-sampling estimator F around I, sqrt(E[F^2] - I^2), by the same
         quadrature, under the sampling density the reference defines:
           rect / disc  uniform over the emitter's area       (areaLightSampleRev, clight.h:67-84; MapSamplesToDisc is area preserving)
           sphere       uniform over the WHOLE sphere         (sphereLightSampleRev, clight.h:86-103; pdfA = 1 / (4 pi r^2))
           environment  piecewise constant per texel          (SampleMap2D, integrator_pt_lgt.cpp:217-239; table: integrator_pt_scene_lgt.cpp:219-270)
           a light picked uniformly among K                   (LightPdfSelectRev, integrator_pt_lgt.cpp:60-63; kernel_SampleLightSource,
                                                               integrator_pt.cpp:375): F = K F_k with probability 1/K, E[F^2] = K sum E[F_k^2]
         and exactly 0 for a single delta light.

Conventions taken from the reference (the only places this module depends on it):
  * a light's direction is matrix * (0, -1, 0), normalised; a rect / disc lies in its local xz plane, sizes are half sizes, the matrix may
    scale (integrator_pt_scene_lgt.cpp:69-91). The area element here is |M ex x M ez|, from the matrix itself, not from the stored pdfA;
  * one-sided emitters: only dot(dir to light, light normal) < 0 is lit, except omni lights and lights with an IES profile
    (integrator_pt.cpp:391);
  * LightEvalPDF (integrator_pt_lgt.cpp:71-107) with pdfA = 1 for point lights: omni and spot get cos' = 1, the Lambert point light
    max(cos', 0); PdfAtoW = pdfA r^2 / cos' (cglobals.h:265-268); a directional light has pdf 1 and no falloff (integrator_pt.cpp:405-409);
  * spot: smoothstep((cos - cos2) / (cos1 - cos2)) (integrator_pt_lgt.cpp:145-151, clight.h:220-225);
  * IES: the profile at sphereMapTo2DTexCoord(-(iesMatrix * dir)) (integrator_pt_lgt.cpp:129-139; cglobals.h:335-358: x = phi / 2 pi,
    y = theta / pi, theta measured from -y, phi = atan2(dir.x, dir.z));
  * slide projector: the slide at ndc.xy * 0.5 + 0.5 of iesMatrix * (P, 1) (integrator_pt_lgt.cpp:153-161);
  * environment: L(omega) = colour * mult * map(sphereMapTo2DTexCoord(omega)) (integrator_pt_lgt.cpp:163-170); d omega = 2 pi^2 sin(theta) du dv
    (integrator_pt_lgt.cpp:46); under INTEGRATOR_SHADOW_PT with a sampled map an escaping ray adds nothing (integrator_pt.cpp:573-576);
  * the bilinear fetch and its address rules: Tex2DFetchAD / bilinearOffsets (diff_render/integrator_dr.cpp:60-93, 106-127): ff = uv * size - 0.5,
    CLAMP sets a negative ff to 0 (the lower edge only), the second tap is one texel towards the sign of ff, both taps wrap by modulo;
  * the Lambert BSDF is rho / pi with pdf cos / pi; MIS uses the balance heuristic (misWeightHeuristic, cglobals.h:277-282).

The sphere case: the floor is flat, so every floor point has the horizon y = 0, and a sphere that crosses it is seen at grazing incidence by
every point that keeps the table's distance. The sphere of that case dips 0.05 below the floor, which cuts its visible cap for every point
(most for the nearest one, by 0.4 % of I); the closed form rho * Le * (R / d)^2 * cos(theta) of a wholly visible sphere is checked on a
raised copy of the same sphere by the module's CPU test.
"""
import math

import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd.synth import _quad

ALBEDO = np.array([0.5, 0.7, 0.9])
RAY_ORIGIN = np.array([-3.0, 2.0, 2.5])                    # every ray starts here, 2 units above the floor
CAM_POS, CAM_LOOK_AT, CAM_UP = (0.5, 3.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
TRACE_DEPTH = 2                                            # the cosine-sampled ray of the MIS run has to reach the emitter
POINTS = 16
FLOOR_HALF = 8.0                                           # the floor is the square |x|, |z| <= 8
Y = np.array([0.0, 1.0, 0.0])


def _gl(n, a=0.0, b=1.0):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _polar(foot, pairs):
    """Floor points at (distance, azimuth in degrees from +x towards +z) around foot = (x, z)."""
    return np.array([[foot[0] + r * math.cos(math.radians(a)), 0.0, foot[1] + r * math.sin(math.radians(a))] for r, a in pairs])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the bilinear fetch (diff_render/integrator_dr.cpp:60-93, 106-127), in float64
# ---------------------------------------------------------------------------------------------------------------------------------------
def fetch_bilinear(data, uv, addr=(S.ADDR_WRAP, S.ADDR_WRAP)):
    """data [h, w] or [h, w, c]; uv [..., 2] -> [...] or [..., c]."""
    data = np.asarray(data, np.float64)
    uv = np.asarray(uv, np.float64)
    h, w = data.shape[:2]
    ffx, ffy = uv[..., 0] * w - 0.5, uv[..., 1] * h - 0.5
    if addr[0] == S.ADDR_CLAMP:
        ffx = np.where(ffx < 0, 0.0, ffx)
    if addr[1] == S.ADDR_CLAMP:
        ffy = np.where(ffy < 0, 0.0, ffy)
    px, py = np.trunc(ffx).astype(np.int64), np.trunc(ffy).astype(np.int64)
    fx, fy = np.abs(ffx - px), np.abs(ffy - py)
    sx, sy = np.where(ffx > 0, 1, -1), np.where(ffy > 0, 1, -1)
    x0, x1, y0, y1 = np.mod(px, w), np.mod(px + sx, w), np.mod(py, h), np.mod(py + sy, h)
    e = (lambda a: a[..., None]) if data.ndim == 3 else (lambda a: a)
    return (data[y0, x0] * e((1 - fx) * (1 - fy)) + data[y0, x1] * e(fx * (1 - fy))) + data[y1, x0] * e((1 - fx) * fy) + data[y1, x1] * e(fx * fy)


def sphere_map_to_tex(d):
    """sphereMapTo2DTexCoord (cglobals.h:335-358): phi = atan2(d.x, d.z) in [0, 2 pi), theta = acos(-d.y)."""
    d = np.asarray(d, np.float64)
    phi = np.arctan2(d[..., 0], d[..., 2])
    phi = np.where(phi < 0, phi + 2 * math.pi, phi)
    theta = np.arccos(np.clip(-d[..., 1], -1.0, 1.0))
    return np.stack([np.clip(phi / (2 * math.pi), 0, 1), np.clip(theta / math.pi, 0, 1)], -1)


def tex_to_sphere_map(u, v):
    """texCoord2DToSphereMap (cglobals.h:360-373): its inverse; returns (direction [..., 3], sin(theta))."""
    phi, theta = u * 2 * math.pi, v * math.pi
    st = np.sin(theta)
    return np.stack([st * np.sin(phi), -np.cos(theta), st * np.cos(phi)], -1), st


# ---------------------------------------------------------------------------------------------------------------------------------------
# lights: plain descriptions (float64) that both the scene builder and the integrals read
# ---------------------------------------------------------------------------------------------------------------------------------------
def _m3(light):
    return np.asarray(light["matrix"], np.float64)[:3, :3]


def _pos(light):
    return np.asarray(light["matrix"], np.float64)[:3, 3]


def _dirn(light):
    return _unit(_m3(light) @ np.array([0.0, -1.0, 0.0]))


def _le(light):
    return np.asarray(light["color"], np.float64) * light["mult"]


def _area_moments(light, P, x, n_l, dA, area):
    """I and E[F^2] of an emitter given quadrature points x [m, 3] with normals n_l [m, 3] (or one normal) and area weights dA [m];
    the sampling density is 1 / area."""
    v = x - P
    r2 = np.sum(v * v, -1)
    r = np.sqrt(r2)
    cos_p = np.maximum(v[:, 1] / r, 0.0)
    cos_l = np.maximum(-np.sum(v * n_l, -1) / r, 0.0)
    g = cos_p * cos_l / r2 / math.pi                          # per unit albedo and radiance
    k = ALBEDO * _le(light)
    return k * np.sum(g * dA), k * k * (np.sum(g * g * dA) * area)


def rect_moments(light, P, n=96):
    u, wu = _gl(n, -1.0, 1.0)
    m = _m3(light)
    ex, ez = m @ np.array([light["half"][0], 0.0, 0.0]), m @ np.array([0.0, 0.0, light["half"][1]])
    jac = np.linalg.norm(np.cross(ex, ez))
    uu, vv = np.meshgrid(u, u, indexing="ij")
    x = _pos(light) + uu.reshape(-1, 1) * ex + vv.reshape(-1, 1) * ez
    return _area_moments(light, P, x, _dirn(light), np.outer(wu, wu).reshape(-1) * jac, 4.0 * jac)


def disc_moments(light, P, nr=64, nphi=256):
    t, wt = _gl(nr)
    phi = (np.arange(nphi) + 0.5) * (2 * math.pi / nphi)
    m = _m3(light)
    ex, ez = m @ np.array([light["radius"], 0.0, 0.0]), m @ np.array([0.0, 0.0, light["radius"]])
    jac = np.linalg.norm(np.cross(ex, ez))
    tt, pp = np.meshgrid(t, phi, indexing="ij")
    x = _pos(light) + (tt * np.cos(pp)).reshape(-1, 1) * ex + (tt * np.sin(pp)).reshape(-1, 1) * ez
    dA = (np.outer(wt * t, np.full(nphi, 2 * math.pi / nphi))).reshape(-1) * jac
    return _area_moments(light, P, x, _dirn(light), dA, math.pi * jac)


def sphere_radius(light):
    return light["radius"] * np.linalg.norm(_m3(light)[:, 0])       # integrator_pt_scene_lgt.cpp: the matrix scales the radius


def sphere_moments(light, P, na=400, nb=64):
    """Over the cap that P sees: alpha from the axis centre -> P up to the terminator acos(R / d), beta around it, cut where the sphere
    is below the floor's horizon y = 0."""
    c, R = _pos(light), sphere_radius(light)
    d = np.linalg.norm(P - c)
    w = (P - c) / d
    s = math.hypot(w[0], w[2])
    b = np.array([-w[2], 0.0, w[0]]) / s if s > 1e-12 else np.array([1.0, 0.0, 0.0])
    a = np.cross(b, w)                                               # a.y = s >= 0: beta = 0 is the cap's highest meridian
    al, wa = _gl(na, 0.0, math.acos(R / d))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -(c[1] + R * np.cos(al) * w[1]) / (R * np.sin(al) * s) if s > 1e-12 else np.where(c[1] + R * np.cos(al) * w[1] > 0, -2.0, 2.0)
    bm = np.where(t <= -1, math.pi, np.where(t >= 1, 0.0, np.arccos(np.clip(t, -1, 1))))
    x01, w01 = _gl(nb)
    be = bm[:, None] * x01[None, :]
    wb = 2.0 * bm[:, None] * w01[None, :]                            # the integrand is even in beta
    nrm = (np.cos(al)[:, None, None] * w + np.sin(al)[:, None, None] * (np.cos(be)[..., None] * a + np.sin(be)[..., None] * b)).reshape(-1, 3)
    dA = ((wa * np.sin(al))[:, None] * wb).reshape(-1) * R * R
    return _area_moments(light, P, c + R * nrm, nrm, dA, 4 * math.pi * R * R)


def sphere_closed_form(light, P):
    """A sphere wholly above P's horizon: rho * Le * (R / d)^2 * cos(theta)."""
    c, R = _pos(light), sphere_radius(light)
    v = c - P
    d = np.linalg.norm(v)
    return ALBEDO * _le(light) * (R / d) ** 2 * (v[1] / d)


def _smoothstep(e0, e1, x):
    t = min(max((x - e0) / (e1 - e0), 0.0), 1.0)
    return t * t * (3.0 - 2.0 * t)


def _blocked(P, target, occluder):
    """Does the segment P -> target cross the horizontal rectangle (x0, x1, z0, z1, height)?"""
    if occluder is None:
        return False
    x0, x1, z0, z1, h = occluder
    d = target - P
    if d[1] <= 0 or not (P[1] < h < target[1]):
        return False
    q = P + d * ((h - P[1]) / d[1])
    return x0 <= q[0] <= x1 and z0 <= q[2] <= z1


def delta_radiance(light, P, occluder=None):
    """Point and directional lights: the one value the deterministic estimator takes."""
    n_l = _dirn(light)
    if light["kind"] == "directional":
        if _blocked(P, P - n_l * 1e5, occluder):
            return np.zeros(3)
        return ALBEDO / math.pi * _le(light) * max(-n_l[1], 0.0)
    v = _pos(light) - P
    r = np.linalg.norm(v)
    wdir = v / r
    cos_l = -float(np.dot(wdir, n_l))
    dist = light["dist"]
    lit = cos_l > 0 or dist == "omni" or dist == "ies"               # integrator_pt.cpp:391
    if not lit or _blocked(P, _pos(light), occluder):
        return np.zeros(3)
    val = ALBEDO / math.pi * _le(light) * max(wdir[1], 0.0) / (r * r)
    if dist == "lambert":
        val = val * max(cos_l, 0.0)
    if dist == "ies":
        dt = np.asarray(light["ies_matrix"], np.float64)[:3, :3] @ wdir
        val = val * fetch_bilinear(light["ies_data"], sphere_map_to_tex(-dt), (S.ADDR_CLAMP, S.ADDR_CLAMP))
    if dist == "spot":
        val = val * _smoothstep(light["cos2"], light["cos1"], max(cos_l, 0.0))
        if "slide" in light:
            clip = projective_matrix(light) @ np.array([*P, 1.0])
            uv = clip[:2] / clip[3] * 0.5 + 0.5
            val = val * fetch_bilinear(light["slide"], uv)[:3]
    return val


def projective_matrix(light):
    """integrator_pt_scene_lgt.cpp:136-159: perspective(fov, 1, near, far) * lookAt(pos, M * (0, -1, 0), rot(M) * (0, 0, 1))."""
    m = np.asarray(light["matrix"], np.float64)
    rot = m.copy(); rot[:, 3] = (0, 0, 0, 1)
    fov, z_near, z_far = light["projective"]
    pos, at, up = _pos(light), (m @ np.array([0, -1.0, 0, 1.0]))[:3], (rot @ np.array([0, 0, 1.0, 1.0]))[:3]
    return S.perspective_matrix(fov, 1.0, z_near, z_far) @ S.look_at(pos, at, up)


def env_table_pdf(env):
    """The density over texture coordinates that the table defines (integrator_pt_scene_lgt.cpp:219-270; SampleMap2D): per texel, the
    largest colour component floored at a tenth of the mean, normalised so that the density integrates to 1 over the unit square."""
    lum = np.asarray(env["map"], np.float64)[..., :3].max(-1)
    lum = np.maximum(lum, 0.1 * lum.mean())
    return lum / lum.sum() * lum.size


def env_moments(env, per=8):
    """rho/pi * integral of L(omega) cos d omega over the upper hemisphere (v in [0.5, 1]), as a composite Gauss-Legendre rule with `per`
    nodes per half texel and axis: both the bilinear fetch (kinks at texel centres) and the table (steps at texel edges) are smooth per panel."""
    img = np.asarray(env["map"], np.float64)
    h, w = img.shape[:2]
    def nodes(lo, hi, n):
        edges = np.arange(round(lo * 2 * n), round(hi * 2 * n) + 1) / (2.0 * n)
        xs, ws = zip(*[_gl(per, a, b) for a, b in zip(edges[:-1], edges[1:])])
        return np.concatenate(xs), np.concatenate(ws)
    u, wu = nodes(0.0, 1.0, w)
    v, wv = nodes(0.5, 1.0, h)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    d, st = tex_to_sphere_map(uu, vv)
    L = fetch_bilinear(img, np.stack([uu, vv], -1))[..., :3] * (np.asarray(env["color"], np.float64) * env["mult"])
    f = L * ALBEDO / math.pi * (np.maximum(d[..., 1], 0.0) * 2 * math.pi * math.pi * st)[..., None]      # per unit of du dv
    p = env_table_pdf(env)[np.minimum((vv * h).astype(int), h - 1), np.minimum((uu * w).astype(int), w - 1)]
    ww = np.outer(wu, wv)[..., None]
    return np.sum(f * ww, (0, 1)), np.sum(f * f / p[..., None] * ww, (0, 1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
RECT = {"kind": "rect", "matrix": S.translate(0.2, 0.9, -0.1) @ S.rotate_y(30) @ S.rotate_x(-25) @ S.scale(1.5, 1.0, 1.0),
        "half": (0.5, 0.2), "color": (1.0, 0.8, 0.6), "mult": 8.0}
SPOT = {"kind": "point", "dist": "spot", "matrix": S.translate(-0.4, 1.5, 0.3) @ S.rotate_y(-40) @ S.rotate_x(15),
        "cos1": math.cos(math.radians(20)), "cos2": math.cos(math.radians(35)), "color": (0.9, 1.0, 0.7), "mult": 12.0}
IES_DATA = (np.arange(32, dtype=np.float64).reshape(4, 8) * 0.0625 + 0.25) * np.where(np.arange(32).reshape(4, 8) % 3 == 0, 1.5, 1.0)
SLIDE = np.stack([(np.arange(16).reshape(4, 4) * k % 17 + 2) / 16.0 for k in (3, 5, 7, 11)], -1)
ENV_MAP = np.stack([np.full((8, 16), c) for c in (0.5, 0.75, 1.0, 1.0)], -1) * (1.0 + (np.arange(128).reshape(8, 16) % 5)[..., None] * 0.125)
ENV_MAP[5, 3, :3] *= 50.0                                           # one texel of the upper hemisphere 50 x the rest


def _spot_axis_foot(light):
    p, n = _pos(light), _dirn(light)
    return p + n * (p[1] / -n[1])


def _spot_points():
    """Inside the inner cone (20 deg), in the penumbra (20..35 deg) and outside (exactly 0), around the foot of the tilted axis."""
    p, n = _pos(SPOT), _dirn(SPOT)
    e1 = _unit(np.cross(n, Y)); e2 = np.cross(n, e1)
    pts = []
    for off_deg, az in ((0, 0), (8, 30), (15, 200), (19, 110), (21, 300), (24, 45), (27, 160), (29, 250), (31, 20), (33, 95), (34, 330),
                        (37, 60), (45, 180), (50, 270), (55, 10), (12, 280)):
        a, b = math.radians(off_deg), math.radians(az)
        d = math.cos(a) * n + math.sin(a) * (math.cos(b) * e1 + math.sin(b) * e2)
        pts.append(p + d * (p[1] / -d[1]))
    pts = np.array(pts); pts[:, 1] = 0.0
    return pts


class Case:
    """One scene, its 16 floor points, and the samples per point: R consecutive rays per point, pass_num samples per ray."""

    def __init__(self, name, lights, points, R, pass_num, integrator=S.INTEGRATOR_SHADOW_PT, env=None, occluder=None, bind_quad=False):
        self.name, self.lights, self.points, self.R, self.pass_num = name, lights, np.asarray(points, np.float64), R, pass_num
        self.integrator, self.env, self.occluder, self.bind_quad = integrator, env, occluder, bind_quad
        assert self.points.shape == (POINTS, 3) and np.all(self.points[:, 1] == 0.0) and np.abs(self.points).max() < FLOOR_HALF - 1.0
        self._moments = None

    @property
    def deterministic(self):
        return self.env is None and len(self.lights) == 1 and self.lights[0]["kind"] in ("point", "directional")

    @property
    def samples(self):
        return self.R * self.pass_num

    # -- float64 side ---------------------------------------------------------------------------------------------------------------
    def light_moments(self, light, P):
        k = light["kind"]
        if k == "rect":
            return rect_moments(light, P)
        if k == "disc":
            return disc_moments(light, P)
        if k == "sphere":
            return sphere_moments(light, P)
        v = delta_radiance(light, P, self.occluder)
        return v, v * v

    def moments(self):
        """(I [16, 3], sigma [16, 3]) of the one-sample light-sampling estimator; computed once."""
        if self._moments is None:
            I, E2 = np.zeros((POINTS, 3)), np.zeros((POINTS, 3))
            K = len(self.lights) + (1 if self.env is not None else 0)
            env = env_moments(self.env) if self.env is not None else None
            for i, P in enumerate(self.points):
                parts = [self.light_moments(l, P) for l in self.lights] + ([env] if env is not None else [])
                I[i] = sum(p[0] for p in parts)
                E2[i] = K * sum(p[1] for p in parts)
            var = E2 - I * I
            sigma = np.sqrt(np.maximum(var, 0.0))
            if self.deterministic:
                assert np.all(var == 0.0)
            self._moments = (I, sigma)
        return self._moments

    def sigma(self):
        """The deviation the assertion uses. The MIS run: the larger of the light-sampling estimator's and the cosine-sampling estimator's
        own deviation; the latter takes rho * Le with probability I / (rho * Le) and 0 otherwise, so E[F^2] = rho * Le * I."""
        I, sig = self.moments()
        if self.integrator != S.INTEGRATOR_MIS_PT:
            return sig
        k = ALBEDO * _le(self.lights[0])
        return np.maximum(sig, np.sqrt(np.maximum(k * I - I * I, 0.0)))

    def bound(self):
        """5 sigma / sqrt(N) per point and channel."""
        return 5.0 * self.sigma() / math.sqrt(self.samples)

    # -- the scene and the rays -----------------------------------------------------------------------------------------------------
    def scene(self):
        sc = S.SceneData()
        sc.width, sc.height = POINTS, self.R                          # one generator per ray: InitRandomGens(16 R)
        sc.cam_pos, sc.cam_look_at, sc.cam_up = CAM_POS, CAM_LOOK_AT, CAM_UP
        sc.fov, sc.trace_depth = 45.0, TRACE_DEPTH
        sc.materials.append(S.material_lambert(tuple(ALBEDO)))
        p, n, t, uv, idx = _quad((-FLOOR_HALF, 0, FLOOR_HALF), (2 * FLOOR_HALF, 0, 0), (0, 0, -2 * FLOOR_HALF))
        sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
        if self.occluder is not None:                                  # a black Lambert rectangle: it shadows, and reflects nothing
            x0, x1, z0, z1, h = self.occluder
            sc.materials.append(S.material_lambert((0.0, 0.0, 0.0)))
            p, n, t, uv, idx = _quad((x0, h, z1), (x1 - x0, 0, 0), (0, 0, z0 - z1))
            sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [len(sc.materials) - 1]), np.eye(4))
        for l in self.lights:
            k = l["kind"]
            if k == "rect":
                sc.lights.append(S.light_rect(l["matrix"], l["half"][0], l["half"][1], l["color"], l["mult"]))
                if self.bind_quad:                                     # as tests/dr_texture_cases._add_rect_light binds its emitter
                    light_id, emis = len(sc.lights) - 1, len(sc.materials)
                    sc.materials.append(S.material_emissive(l["color"], l["mult"], light_id))
                    sc.lights[light_id]["matId"] = emis
                    hx, hz = l["half"]
                    p, n, t, uv, idx = _quad((-hx, 0, -hz), (2 * hx, 0, 0), (0, 0, 2 * hz))           # normal -y
                    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [emis]), l["matrix"], -1, light_id)
            elif k == "disc":
                sc.lights.append(S.light_rect(l["matrix"], l["radius"], l["radius"], l["color"], l["mult"], disk_radius=l["radius"]))
            elif k == "sphere":
                sc.lights.append(S.light_sphere(l["matrix"], l["radius"], l["color"], l["mult"]))
            elif k == "directional":
                sc.lights.append(S.light_directional(l["matrix"], l["color"], l["mult"]))
            else:
                lt = S.light_point(l["matrix"], l["color"], l["mult"], l["dist"], l.get("cos1", 0.0), l.get("cos2", 0.0))
                if l["dist"] == "ies":
                    lt["iesId"] = sc.add_texture(S.Texture(l["ies_data"], S.TEX_R32F, False, S.ADDR_CLAMP, S.ADDR_CLAMP, S.FILTER_LINEAR))
                    lt["iesMatrix"] = S.colmajor(l["ies_matrix"])
                if "slide" in l:
                    tex = sc.add_texture(S.Texture(l["slide"], S.TEX_RGBA32F, False))
                    S.set_projective(lt, l["matrix"], *l["projective"], tex_id=tex)
                sc.lights.append(lt)
        if self.env is not None:
            tex = sc.add_texture(S.Texture(self.env["map"], S.TEX_RGBA32F, False))
            sc.set_environment(self.env["color"], tex, self.env["mult"], sample=True)
        return sc

    def params(self, sc):
        return sc.params(integrator=self.integrator)

    def rays(self):
        """Camera-space rays (float32 [16 R, 4] positions and directions): point i is rays i R .. i R + R - 1."""
        wv = S.look_at(CAM_POS, CAM_LOOK_AT, CAM_UP)
        d = self.points - RAY_ORIGIN
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pos, dr = np.zeros((POINTS * self.R, 4), np.float32), np.zeros((POINTS * self.R, 4), np.float32)
        pos[:, :3] = (wv @ np.array([*RAY_ORIGIN, 1.0]))[:3]
        dr[:, :3] = np.repeat(d @ wv[:3, :3].T, self.R, axis=0)
        return pos, dr

    def point_means(self, out):
        """out [16 R, c] as the integrators leave it (sums over pass_num) -> float64 means per point [16, c]."""
        return out.astype(np.float64).reshape(POINTS, self.R, -1).sum(1) / self.samples

    # -- geometry checks of the table itself -----------------------------------------------------------------------------------------
    def primary_rays_reach_the_floor(self):
        """No ray from RAY_ORIGIN meets the occluder or a bound emitter before its floor point."""
        for P in self.points:
            if _blocked(P, RAY_ORIGIN, self.occluder):
                return False
            for l in self.lights:
                if l["kind"] == "rect" and self.bind_quad:
                    m, c, n_l = _m3(l), _pos(l), _dirn(l)
                    d = RAY_ORIGIN - P
                    den = float(np.dot(d, n_l))
                    if abs(den) > 1e-12:
                        t = float(np.dot(c - P, n_l)) / den
                        if 0 < t < 1:
                            loc = np.linalg.solve(m, P + t * d - c)
                            if abs(loc[0]) <= l["half"][0] and abs(loc[2]) <= l["half"][1]:
                                return False
        return True

    def emitter_distance(self):
        """The smallest distance of a point to an area emitter over the emitter's larger half size (>= 1 by the table's rule)."""
        worst = math.inf
        g = np.linspace(-1, 1, 41)
        for l in self.lights:
            m, c = _m3(l), _pos(l)
            if l["kind"] == "rect":
                loc = np.array([[a * l["half"][0], 0.0, b * l["half"][1]] for a in g for b in g])
                half = max(np.linalg.norm(m @ [l["half"][0], 0, 0]), np.linalg.norm(m @ [0, 0, l["half"][1]]))
            elif l["kind"] == "disc":
                loc = np.array([[a * l["radius"], 0.0, b * l["radius"]] for a in g for b in g if a * a + b * b <= 1.0])
                half = max(np.linalg.norm(m @ [l["radius"], 0, 0]), np.linalg.norm(m @ [0, 0, l["radius"]]))
            elif l["kind"] == "sphere":
                half = sphere_radius(l)
                worst = min(worst, min(np.linalg.norm(P - c) - half for P in self.points) / half)
                continue
            else:
                continue
            x = c + loc @ m.T
            worst = min(worst, min(np.min(np.linalg.norm(x - P, axis=1)) for P in self.points) / half)
        return worst


def _occluder_over(P, target, height=0.3, half=0.1):
    """A small rectangle at `height` centred on the segment P -> target."""
    d = target - P
    q = P + d * (height / d[1])
    return (q[0] - half, q[0] + half, q[2] - half, q[2] + half, height)


def _cases():
    rect_pts = _polar((0.2, -0.1), [(0.0, 0), (0.9 * math.tan(math.radians(60)), 60), (0.9 * math.tan(math.radians(61)), 50),
                                    (0.9 * math.tan(math.radians(62)), 70), (0.5, 0), (0.5, 135), (0.9, 200), (1.0, 300), (0.7, 60),
                                    (1.2, 100), (1.3, 20), (1.0, 150), (0.6, 240), (1.1, 350), (3.0, 240), (3.5, 220)])
    disc = {"kind": "disc", "matrix": S.translate(-0.3, 1.15, 0.2) @ S.rotate_y(-20) @ S.rotate_x(20) @ S.scale(1.0, 1.0, 1.6),
            "radius": 0.5, "color": (0.7, 1.0, 0.9), "mult": 6.0}
    disc_pts = _polar((-0.3, 0.2), [(0.0, 0), (1.15 * math.tan(math.radians(60)), 250), (1.15 * math.tan(math.radians(70)), 270),
                                    (1.15 * math.tan(math.radians(80)), 230), (0.4, 30), (0.6, 140), (0.8, 260), (1.0, 330), (1.2, 200),
                                    (0.9, 90), (1.4, 290), (0.5, 210), (1.6, 250), (0.7, 0), (4.5, 70), (6.0, 90)])
    sphere = {"kind": "sphere", "matrix": S.translate(0.1, 0.25, -0.2), "radius": 0.3, "color": (1.0, 0.9, 0.5), "mult": 10.0}
    sphere_pts = _polar((0.1, -0.2), [(0.6, 45), (0.7, 130), (0.8, 220), (0.9, 310), (1.0, 10), (1.2, 80), (1.4, 170), (1.6, 260), (2.0, 350),
                                      (0.25 * math.tan(math.radians(80)), 30), (0.25 * math.tan(math.radians(75)), 150), (2.5, 200),
                                      (0.65, 280), (1.1, 240), (3.0, 100), (0.75, 0)])
    omni = {"kind": "point", "dist": "omni", "matrix": S.translate(0.3, 1.2, -0.2) @ S.rotate_x(10), "color": (1.0, 0.6, 0.8), "mult": 9.0}
    lamb = dict(omni, dist="lambert", matrix=S.translate(0.3, 1.2, -0.2) @ S.rotate_y(25) @ S.rotate_x(-50))
    point_pts = _polar((0.3, -0.2), [(0.0, 0), (1.2 * math.tan(math.radians(60)), 20), (1.2 * math.tan(math.radians(70)), 140),
                                     (1.2 * math.tan(math.radians(80)), 260), (0.3, 90), (0.6, 180), (0.9, 270), (1.2, 0), (1.5, 45), (1.8, 135),
                                     (2.4, 225), (3.0, 315), (0.45, 300), (1.0, 200), (4.0, 70), (5.0, 110)])
    omni_occ = _occluder_over(point_pts[9], _pos(omni))
    direct = {"kind": "directional", "matrix": S.rotate_y(35) @ S.rotate_x(-40), "color": (1.0, 0.95, 0.8), "mult": 3.0}
    dir_occ = _occluder_over(point_pts[9], point_pts[9] - _dirn(direct) * 10.0)
    ies = dict(omni, dist="ies", ies_data=IES_DATA, ies_matrix=S.rotate_y(50) @ S.rotate_x(30))
    proj = dict(SPOT, slide=SLIDE, projective=(80.0, 0.1, 20.0))
    env = {"map": ENV_MAP, "color": (1.0, 0.9, 0.8), "mult": 1.5}
    env_pts = _polar((0.0, 0.0), [(0.25 * i, 37 * i) for i in range(POINTS)])
    spot_pts = _spot_points()
    two_pts = np.concatenate([rect_pts[[0, 1, 2, 3, 4, 5, 6, 14]], spot_pts[[0, 1, 3, 5, 7, 9, 11, 12]]])
    return [
        Case("rect", [RECT], rect_pts, 128, 1536),
        Case("disc", [disc], disc_pts, 128, 2048),
        Case("sphere", [sphere], sphere_pts, 256, 8192),
        Case("omni", [omni], point_pts, 4, 2, occluder=omni_occ),
        Case("lambert_point", [lamb], point_pts, 4, 2),
        Case("spot", [SPOT], spot_pts, 4, 2),
        Case("directional", [direct], point_pts, 4, 2, occluder=dir_occ),
        Case("ies", [ies], point_pts, 4, 2, occluder=omni_occ),
        Case("projector", [proj], spot_pts, 4, 2),
        Case("env", [], env_pts, 256, 6144, env=env),
        Case("two_lights", [RECT, SPOT], two_pts, 128, 4096),
        Case("rect_mis", [RECT], rect_pts, 1024, 14336, integrator=S.INTEGRATOR_MIS_PT, bind_quad=True),
        Case("rect_mis_shadow", [RECT], rect_pts, 128, 1536, bind_quad=True),
    ]


CASES = {c.name: c for c in _cases()}
DETERMINISTIC = [n for n, c in CASES.items() if c.deterministic]
STOCHASTIC = [n for n, c in CASES.items() if not c.deterministic]

# ---------------------------------------------------------------------------------------------------------------------------------------
# the assertions, shared by the oracle's test (CPU) and the device's (GPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
# profiles/light_integrals.md: the oracle's worst relative error against I over every point and channel of the deterministic cases, and the
# bound of the device, four times that (the device's sinf / acosf / atan2f / powf differ from glibc's in the last bits: VERDICT.md weak 2).
# The worst point lies in the spot's outer penumbra (33 degrees off an axis whose smoothstep ends at 35), where I changes by 9e-5 I per
# 1e-5 of the point's height: the estimator looks at the light from the shadow ray's origin, which the reference lifts off the surface
# (integrator_pt.cpp:388), and a lift of 1.1e-5 in the float64 form reproduces the oracle there. Everywhere else the error is below 2e-5.
ORACLE_WORST_DELTA_ERROR = 1.07e-4
DELTA_BOUND = 4.0 * ORACLE_WORST_DELTA_ERROR


def delta_errors(case, out):
    """Relative errors |value - I| / I of a deterministic case, over every ray (not the mean), where I > 0: [n] float64."""
    I, _ = case.moments()
    raw = out.astype(np.float64).reshape(POINTS, case.R, -1)[:, :, :3] / case.pass_num
    lit = np.broadcast_to((I > 0)[:, None, :], raw.shape)
    return (np.abs(raw - I[:, None, :]) / np.where(I > 0, I, 1.0)[:, None, :])[lit]


def check_against_integral(case, out, what):
    """out: float32 [16 R, 4] as PathTraceFromInputRaysBlock left it on a zeroed array after case.pass_num passes. Every point and channel."""
    I, _ = case.moments()
    assert out.shape == (POINTS * case.R, 4) and np.all(out[:, 3] == 0.0), f"{what}: the fourth channel is not written"
    raw = out.reshape(POINTS, case.R, 4)[:, :, :3]
    dark = np.broadcast_to((I == 0)[:, None, :], raw.shape)
    assert np.all(raw[dark] == 0.0), f"{what} {case.name}: a value that must be exactly 0 is {np.abs(raw[dark]).max()}"
    lit = I > 0
    mean = case.point_means(out)[:, :3]
    if case.deterministic:
        err = delta_errors(case, out)
        print(f"{what} {case.name}: worst relative error {err.max():.3e} (bound {DELTA_BOUND:.1e})")
        assert err.max() <= DELTA_BOUND, f"{what} {case.name}: {err.max():.3e} > {DELTA_BOUND:.1e}"
        return float(err.max())
    b = case.bound()
    ratio = np.abs(mean - I)[lit] / b[lit]
    print(f"{what} {case.name}: N = {case.samples}, worst |mean - I| / (5 sigma / sqrt N) = {ratio.max():.3f}, worst |mean - I| / I = "
          f"{(np.abs(mean - I)[lit] / I[lit]).max():.3e}, worst bound / I = {(b[lit] / I[lit]).max():.3e}")
    assert np.all(np.abs(mean - I)[lit] <= b[lit]), f"{what} {case.name}: point, channel {np.argwhere(np.abs(mean - I) > b).tolist()} off by up to {ratio.max():.2f} bounds"
    return float(ratio.max())

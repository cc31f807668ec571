"""The smooth interfaces in float64: Fresnel, Snell and Airy values for the smooth conductor, the smooth dielectric, the legacy glass and the smooth
thin film, and three scenes in which every sample of such a surface has a value known in advance. Not a test.

Written from the physical definitions; nothing here calls or copies the device code or the oracle. Where the reference sets a convention its text is
cited by line (include/cmat_*.h, integrator_pt.cpp, integrator_pt_mat.cpp):

  * a sample's weight is  cosTheta * val / max(pdf, 1e-20)  (integrator_pt.cpp:510-530); every smooth lobe pre-divides val by that cosine
    (cmat_conductor.h:21, cmat_dielectric.h:55, cmat_glass.h:275, cmat_film.h:180), so the weight is val' / pdf with val' the undivided value.
  * conductor (cmat_conductor.h:7-28): val' = F(cos, eta + i k) * colors[0], pdf 1, the incident medium has index 1.
  * dielectric (cmat_dielectric.h:28-53): reflection with probability R, val' = R, pdf = R: weight 1; refraction with val' = eta_ti^2 T, pdf = T:
    weight eta_ti^2 = (n_incident / n_transmitted)^2, the radiance compression of the solid angle.
  * legacy glass (cmat_glass.h:247-277): reflection with probability R(ior / misPrev.ior), weight colors[0]; else weight colors[1]. misPrev.ior
    is 1 on an input ray, hence: from outside only.
  * thin film (cmat_film.h:145-180): opaque (substrate k > 1e-3, or transparent = 0): val' = R, pdf 1. Transparent: reflection with probability
    sR / (sR + sT), s the sum over the channels, val' = R: weight R (sR + sT) / sR; refraction: weight T (sR + sT) / sT, with no eta_ti^2 (:172).
    The refracted direction uses the substrate's index over the outside medium's (:38, :167-171); in RGB mode the substrate is read at 525 nm
    (integrator_pt_mat.cpp:208-213; the films here have constant indices, so this decides nothing). In RGB mode R and T are always read from the
    scene's table (:79-142), in spectral mode from the table when the loader made one (:43-61), else from the Airy sum per sample (:63-77).
    Table axis: theta = acos(cos) * 2 / pi * (FILM_ANGLE_RES - 1), w = (lambda - 360) / 470 * (FILM_LENGTH_RES - 1) (:45-53, :81-82); rows
    [0, RES) reflectance, [RES, 2 RES) transmittance, [2 RES, 4 RES) the same seen from the substrate ("reversed", :21-31).
  * a ray that leaves the scene adds throughput * environment colour (integrator_pt.cpp:550-594); a hit on an emissive material without a
    light entry adds throughput * colors[0] and ends the path (:461-506); PathTraceFromInputRays (:761-798) takes the wavelength from the
    ray's fourth float and adds the four raw accumulated values to the ray's output (kernel_CopyColorToOutput, :659-676).
  * after a refraction the next ray starts at the hit, taken at t (1 - 1e-6) (:240), moved on by 2e-6 t along the ray and by epsilonOfPos =
    1e-5 * max|coordinate| along the normal (:534-539, cglobals.h:233-247). Scene T's strip is 2e-4 h wide and a refracted ray at 82 deg is
    moved by several such widths, so the landing point is computed from that start.

Inputs are the float32 rays and the float32 scene data as uploaded (vertices, matrices, material records, spectra, film tables); everything after
that is float64.

The angles stay out of the reference's guards: the conductor's  cosThetaOut <= 1e-6  (cmat_conductor.h:21), the film's clamp of the cosine to
[1e-4, 1] (cmat_film.h:37) and the Airy sum's  |denominator|^2 < 1e-6  (airy_reflectance.h:86): the largest angle is 89.5 deg, cos = 8.7e-3.

EPS: the rounding allowance of the deterministic values, four times the oracle's worst relative excursion (tests/test_specular_cpu.py measures it
again on every run; profiles/specular.md has the figures).
"""
import dataclasses
import functools
import math

import numpy as np

from hydracore3_amd import scene as S

LAMBDA_MIN, LAMBDA_MAX = 360.0, 830.0                                    # cglobals.h:22-23
FILM_ANGLE_RES, FILM_LENGTH_RES = 180, 94                                # cglobals.h:19-20

ENV = (1.0, 2.0, 0.5, 0.25)                                              # three different channel values (and a fourth for the raw spectral samples)
EMIT = (3.0, 1.5, 0.75)
WIDTH, HEIGHT = 48, 40                                                   # the pinhole frames: 1920 pixels, block and wave tails run

# four times the oracle's worst relative excursion from the float64 value over every deterministic case: 1.8203e-6, set by the RGB-mode film over a
# conductor at 0 deg, where acos turns the last bit of a cosine next to 1 into 3.5e-4 rad of table axis (profiles/specular.md); asserted by
# tests/test_specular_cpu.py (4 x worst <= EPS < 1e-4). No case needs an allowance of its own: 89.5 deg stays below 1e-6.
EPS = 7.29e-6

# ---- the angle set ----------------------------------------------------------------------------------------------------------------------------
ANGLES = tuple(float(a) for a in range(0, 90, 10)) + (85.0, 88.0, 89.5)   # degrees from the normal; none reaches a guard (see above)
WAVELENGTHS = (380.0, 525.0, 700.0, 451.37)                              # the last lies between the nodes of every table (1 nm spectra, 5.05 nm films)


def critical_angle(n_in, n_out):
    return math.degrees(math.asin(n_out / n_in))


def node_angles(nodes=(0, 1, 57, 100, 177)):
    """Exact table-node angles and the midpoints to the next node, in degrees (node j sits at j * 90 / 179; 178 and 179 would pass 89.5 deg)."""
    step = 90.0 / (FILM_ANGLE_RES - 1)
    return tuple(j * step for j in nodes) + tuple((j + 0.5) * step for j in nodes)


# ---- the physics --------------------------------------------------------------------------------------------------------------------------------
def fresnel_dielectric(cos_i, n_i, n_t):
    """Unpolarised reflectance of the interface between real indices n_i (incident side) and n_t; exactly 1 beyond the critical angle."""
    c = np.asarray(cos_i, np.float64)
    s2 = (n_i / n_t) ** 2 * (1.0 - c * c)
    tir = s2 >= 1.0
    ct = np.sqrt(np.where(tir, 0.0, 1.0 - s2))
    rs = (n_i * c - n_t * ct) / (n_i * c + n_t * ct)
    rp = (n_t * c - n_i * ct) / (n_t * c + n_i * ct)
    return np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp))


def fresnel_conductor(cos_i, eta, k):
    """Unpolarised reflectance of a medium of complex index eta + i k seen from index 1."""
    c = np.asarray(cos_i, np.float64)
    n = np.asarray(eta, np.float64) + 1j * np.asarray(k, np.float64)
    ct = np.sqrt(1.0 - (1.0 - c * c) / (n * n))
    rs = (c - n * ct) / (c + n * ct)
    rp = (n * c - ct) / (n * c + ct)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


def refract(d, n, n_i, n_t):
    """Snell's law in vector form: d the unit direction of travel [.., 3], n the unit normal on the incident side. None beyond the critical angle."""
    d, n = np.asarray(d, np.float64), np.asarray(n, np.float64)
    c = -np.sum(d * n, -1, keepdims=True)
    r = n_i / n_t
    k = 1.0 - r * r * (1.0 - c * c)
    if np.any(k < 0.0):
        return None
    return r * d + (r * c - np.sqrt(k)) * n


def airy(cos_i, n_i, n_f, n_t, thickness, lam):
    """(R, T) of one film of complex index n_f and the given thickness (in the unit of lam) between the real index n_i and the complex index n_t,
    unpolarised: the Airy summation r = (r01 + r12 e^{i delta}) / (1 + r01 r12 e^{i delta}), delta = 4 pi n_f d cos(theta_f) / lambda, and
    T = |t|^2 Re(n_t cos theta_t) / (n_i cos theta_i)."""
    c0 = np.asarray(cos_i, np.float64) + 0j
    n0, n1, n2 = complex(n_i), complex(n_f), complex(n_t)
    s2 = (n0 * n0) * (1.0 - c0 * c0)                                       # (n sin theta)^2, the same in every medium
    c1, c2 = np.sqrt(1.0 - s2 / (n1 * n1)), np.sqrt(1.0 - s2 / (n2 * n2))  # principal root: the decaying wave
    ph = np.exp(1j * 4.0 * math.pi * n1 * c1 * thickness / lam)
    R = T = 0.0
    for pol in "sp":
        if pol == "s":
            r01, r12 = (n0 * c0 - n1 * c1) / (n0 * c0 + n1 * c1), (n1 * c1 - n2 * c2) / (n1 * c1 + n2 * c2)
            t01, t12 = 2 * n0 * c0 / (n0 * c0 + n1 * c1), 2 * n1 * c1 / (n1 * c1 + n2 * c2)
        else:
            r01, r12 = (n1 * c0 - n0 * c1) / (n1 * c0 + n0 * c1), (n2 * c1 - n1 * c2) / (n2 * c1 + n1 * c2)
            t01, t12 = 2 * n0 * c0 / (n1 * c0 + n0 * c1), 2 * n1 * c1 / (n2 * c1 + n1 * c2)
        den = 1.0 + r01 * r12 * ph
        R = R + 0.5 * np.abs((r01 + r12 * ph) / den) ** 2
        T = T + 0.5 * np.abs(t01 * t12 * np.sqrt(ph) / den) ** 2
    return R, T * np.maximum((n2 * c2).real, 0.0) / (n0 * c0).real


def spectrum_at(sc, spec_id, lam):
    """The scene's uploaded 1 nm spectrum read at lam: linear between the float32 samples at floor(lam) and floor(lam) + 1 (spectrum.h:106-126)."""
    off, size = sc.spec_offset_sz[spec_id]
    v = np.asarray(sc.spec_values, np.float32).astype(np.float64)[off:off + size]
    n = int(LAMBDA_MAX - LAMBDA_MIN)
    i = int(min(max(lam - LAMBDA_MIN, 0.0), n - 1))
    j = min(i + 1, n - 1)
    return v[i] + (lam - (LAMBDA_MIN + i)) * (v[j] - v[i])


def _as_uint(x):
    return int(np.float32(x).view(np.uint32))


def film_table_rgb(sc, mat, cos_i, reversed_):
    """(R [3], T [3]) read from the scene's uploaded table of an RGB-mode film without a thickness map, float64, linear in the angle axis."""
    tab = np.asarray(sc.precomp_thin_films, np.float32).astype(np.float64)
    off = _as_uint(mat["data"][S.FILM_PRECOMP_OFFSET])
    t = min(max(math.acos(min(max(cos_i, 1e-4), 1.0)) * 2.0 / math.pi, 0.0), 1.0) * (FILM_ANGLE_RES - 1)
    i = min(int(t), FILM_ANGLE_RES - 2)
    a = t - i
    row_r, row_t = (2 * FILM_ANGLE_RES, 3 * FILM_ANGLE_RES) if reversed_ else (0, FILM_ANGLE_RES)
    rd = lambda row: np.array([(1 - a) * tab[off + (row + i) * 3 + ch] + a * tab[off + (row + i + 1) * 3 + ch] for ch in range(3)])
    return rd(row_r), rd(row_t)


def film_table_spectral(sc, mat, cos_i, lam, reversed_):
    """(R, T) read from the scene's uploaded table of a spectral-mode film, float64, bilinear in (wavelength, angle)."""
    tab = np.asarray(sc.precomp_thin_films, np.float32).astype(np.float64)
    off = _as_uint(mat["data"][S.FILM_PRECOMP_OFFSET])
    w = min(max((lam - LAMBDA_MIN) / (LAMBDA_MAX - LAMBDA_MIN), 0.0), 1.0) * (FILM_LENGTH_RES - 1)
    t = min(max(math.acos(min(max(cos_i, 1e-4), 1.0)) * 2.0 / math.pi, 0.0), 1.0) * (FILM_ANGLE_RES - 1)
    i1, i2 = min(int(w), FILM_LENGTH_RES - 2), min(int(t), FILM_ANGLE_RES - 2)
    a, b = w - i1, t - i2
    row_r, row_t = (2 * FILM_ANGLE_RES, 3 * FILM_ANGLE_RES) if reversed_ else (0, FILM_ANGLE_RES)

    def rd(row):
        at = lambda p, q: tab[off + row * FILM_LENGTH_RES + p * FILM_ANGLE_RES + q]
        v0 = (1 - a) * at(i1, i2) + a * at(i1 + 1, i2)
        v1 = (1 - a) * at(i1, i2 + 1) + a * at(i1 + 1, i2 + 1)
        return (1 - b) * v0 + b * v1
    return rd(row_r), rd(row_t)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str                                   # conductor, dielectric, glass, film
    spectral: bool = False
    inside: bool = False                        # the rays come from the substrate's side
    eta: float = 1.5                            # conductor: eta; dielectric / glass: the inner index
    k: float = 0.0
    ext: float = 1.00028
    color: tuple = (1.0, 1.0, 1.0, 1.0)         # conductor: reflectance; glass: reflect colour
    color2: tuple = (1.0, 1.0, 1.0)             # glass: transparent colour
    dispersive: bool = False                    # spectral: eta (and k) come from spectra
    layers: tuple = ()                          # film: ((eta, k, thickness nm), ...), outermost first
    substrate: tuple = (1.5, 0.0)               # film: (eta, k)
    transparent: int = 0
    per_sample: bool = False                    # film, spectral: a thickness map, so that the loader makes no table and the device sums per sample
    table_angles: bool = False

    @property
    def opaque(self):
        return self.kind == "conductor" or (self.kind == "film" and (self.substrate[1] > 1e-3 or not self.transparent))

    def angles(self):
        a = ANGLES
        if self.inside:
            n_in = self.substrate[0] if self.kind == "film" else self.eta
            if not self.dispersive:
                crit = critical_angle(n_in, float(np.float32(self.ext)))
                above = crit + 0.1
                if self.kind == "film":
                    # the film's R and T come from a table with nodes 0.503 deg apart: 0.1 deg beyond the critical angle lies in the cell that
                    # straddles it, where the interpolated T is above 0 although nothing is refracted, and the reference then sends the refracted
                    # sample along the tangent plane (cos_theta_t = safe_sqrt(negative) = 0, cmaterial.h:658-660; val / max(|cos|, 1e-6),
                    # cmat_film.h:180) - a guard. The angle beyond is the middle of the first cell that lies beyond the critical angle altogether.
                    step = 90.0 / (FILM_ANGLE_RES - 1)
                    above = (math.ceil(crit / step) + 0.5) * step
                a = a + (crit - 0.1, above)
        if self.table_angles:
            a = a + node_angles()
        return tuple(sorted(set(a)))

    def wavelengths(self):
        return WAVELENGTHS if self.spectral else (0.0,)


GOLD = (0.2, 3.9)
CASES = (
    Case("conductor_0.2_3.9", "conductor", eta=0.2, k=3.9),
    Case("conductor_1.5_0", "conductor", eta=1.5, k=0.0),
    Case("conductor_coloured", "conductor", eta=0.2, k=3.9, color=(0.9, 0.6, 0.3, 1.0)),
    Case("dielectric_out", "dielectric"),
    Case("dielectric_in", "dielectric", inside=True),
    Case("dielectric_matched_out", "dielectric", eta=1.01, ext=1.0),
    Case("dielectric_matched_in", "dielectric", eta=1.01, ext=1.0, inside=True),
    Case("glass", "glass", eta=1.5, color=(0.8, 0.5, 0.9), color2=(0.3, 0.7, 0.2)),
    Case("film_rgb_conductor", "film", layers=((1.8, 0.05, 300.0),), substrate=GOLD, table_angles=True),
    Case("film_rgb_transparent_out", "film", layers=((2.0, 0.0, 250.0),), substrate=(1.5, 0.0), transparent=1, table_angles=True),
    Case("film_rgb_transparent_in", "film", layers=((2.0, 0.0, 250.0),), substrate=(1.5, 0.0), transparent=1, inside=True, table_angles=True),
    Case("spectral_conductor", "conductor", spectral=True, dispersive=True, color=(1.0, 0.8, 0.6, 0.4)),
    Case("spectral_dielectric_out", "dielectric", spectral=True, dispersive=True),
    Case("spectral_dielectric_in", "dielectric", spectral=True, dispersive=True, inside=True),
    Case("spectral_film_per_sample", "film", spectral=True, layers=((1.8, 0.05, 300.0),), substrate=GOLD, per_sample=True),
    Case("spectral_film_two_layers", "film", spectral=True, layers=((1.4, 0.0, 120.0), (2.1, 0.02, 200.0)), substrate=GOLD, table_angles=True),
    Case("spectral_film_transparent_out", "film", spectral=True, layers=((2.0, 0.0, 250.0),), substrate=(1.5, 0.0), transparent=1, table_angles=True),
    Case("spectral_film_transparent_in", "film", spectral=True, layers=((2.0, 0.0, 250.0),), substrate=(1.5, 0.0), transparent=1, inside=True,
         table_angles=True),
)
CASE = {c.name: c for c in CASES}


def channels(case):
    """How many of a ray's four output floats are compared: the three colour channels in RGB mode, the four raw samples in spectral mode."""
    return 4 if case.spectral else 3


def cauchy(lam, a, b):
    return a + b / (lam * lam)


def _add_spectrum(sc, values):
    off = int(np.asarray(sc.spec_values).size)
    sc.spec_values = np.concatenate([np.asarray(sc.spec_values, np.float32), np.asarray(values, np.float32)])
    sc.spec_offset_sz = list(sc.spec_offset_sz) + [(off, len(values))]
    return len(sc.spec_offset_sz) - 1


def _material(sc, case):
    """Appends the case's material (for a film: after another film, so that every offset of the one under test is above 0); returns its id."""
    lam = LAMBDA_MIN + np.arange(int(LAMBDA_MAX - LAMBDA_MIN) + 1)
    if case.spectral:
        sc.spectral_mode = 1
        _add_spectrum(sc, np.ones(lam.size))                              # spectrum 0: a flat one, so that the ids under test are above 0
    if case.kind == "conductor":
        m = S.material_conductor(case.eta, case.k, reflectance=case.color)
        if case.dispersive:
            m["spdid"][0] = _add_spectrum(sc, cauchy(lam, 0.15, 2.0e4))    # eta 0.30 ... 0.18
            m["spdid"][1] = _add_spectrum(sc, 1.5 + (lam - 360.0) * 6e-3)  # k 1.5 ... 4.3
    elif case.kind == "dielectric":
        m = S.material_dielectric(case.eta, case.ext)
        if case.dispersive:
            m["spdid"][0] = _add_spectrum(sc, cauchy(lam, 1.45, 1.5e4))    # 1.566 at 360 nm, 1.472 at 830 nm
    elif case.kind == "glass":
        m = S.material_glass(case.color, case.color2, case.eta)
    else:
        first = S.SceneData.material_thin_film(sc, [dict(eta=1.3, k=0.0, thickness=90.0)], dict(eta=1.6, k=0.0), transparent=1)
        sc.materials.append(first)
        layers = [dict(eta=e, k=k, thickness=t) for e, k, t in case.layers]
        tmap = (0.0, case.layers[0][2], 0, (1, 0, 0, 0), (0, 1, 0, 0)) if case.per_sample else None   # texture 0 is white: the thickness is the map's maximum
        m = sc.material_thin_film(layers, dict(eta=case.substrate[0], k=case.substrate[1]), ext_ior=case.ext, transparent=case.transparent,
                                  thickness_map=tmap)
        assert bool(_as_uint(m["data"][S.FILM_PRECOMP_FLAG])) != case.per_sample
    sc.materials.append(m)
    return len(sc.materials) - 1


def indices(sc, case, lam):
    """The indices the case's material has at lam (0: RGB mode), from the scene's float32 records: dict(ext, eta, k)."""
    m = sc.materials[case_material_id(sc, case)]
    f = lambda x: float(np.float32(x))
    if case.kind == "conductor":
        eta, k = f(m["data"][2]), f(m["data"][3])
        if case.dispersive:
            eta, k = spectrum_at(sc, int(m["spdid"][0]), lam), spectrum_at(sc, int(m["spdid"][1]), lam)
        return dict(ext=1.0, eta=eta, k=k)
    if case.kind == "dielectric":
        eta = spectrum_at(sc, int(m["spdid"][0]), lam) if case.dispersive else f(m["data"][1])
        return dict(ext=f(m["data"][0]), eta=eta, k=0.0)
    if case.kind == "glass":
        return dict(ext=1.0, eta=f(m["data"][2]), k=0.0)
    return dict(ext=f(m["data"][S.FILM_ETA_EXT]), eta=f(np.float32(case.substrate[0])), k=f(np.float32(case.substrate[1])))


def case_material_id(sc, case):
    return 1 if case.kind == "film" else 0


def sample_values(sc, case, cos_i, lam):
    """What one sample of a ray that meets the case's surface at cos_i can be, before the environment or the emission multiplies it:
    (p_reflect, w_reflect [4], w_refract [4]) - the probability of the reflected branch and the two branches' weights. An opaque surface has
    p_reflect = 1."""
    ix = indices(sc, case, lam)
    one = np.ones(4)
    m = sc.materials[case_material_id(sc, case)]
    if case.kind == "conductor":
        F = float(fresnel_conductor(cos_i, ix["eta"], ix["k"]))
        return 1.0, F * np.asarray(m["colors"][0], np.float32).astype(np.float64), np.zeros(4)
    if case.kind == "dielectric":
        n_i, n_t = (ix["eta"], ix["ext"]) if case.inside else (ix["ext"], ix["eta"])
        return float(fresnel_dielectric(cos_i, n_i, n_t)), one, one * (n_i / n_t) ** 2
    if case.kind == "glass":
        return float(fresnel_dielectric(cos_i, 1.0, ix["eta"])), np.asarray(m["colors"][0], np.float32).astype(np.float64), \
            np.asarray(m["colors"][1], np.float32).astype(np.float64)
    f32 = lambda x: float(np.float32(x))
    if not case.spectral:
        R3, T3 = film_table_rgb(sc, m, cos_i, case.inside)
        R, T = np.append(R3, 0.0), np.append(T3, 0.0)
    elif case.per_sample:
        (e, k, t), = case.layers
        assert not case.inside                                            # (an absorbing substrate has no inside to come from)
        r, t_ = airy(cos_i, ix["ext"], complex(f32(e), f32(k)), complex(ix["eta"], ix["k"]), f32(t), lam)
        R, T = np.array([float(r), 0, 0, 0]), np.array([float(t_), 0, 0, 0])
    else:
        r, t_ = film_table_spectral(sc, m, cos_i, lam, case.inside)
        R, T = np.array([r, 0, 0, 0]), np.array([t_, 0, 0, 0])
    if case.opaque:
        return 1.0, R, np.zeros(4)
    sR, sT = R.sum(), T.sum()
    return sR / (sR + sT), R * (sR + sT) / sR, (T * (sR + sT) / sT if sT > 0 else np.zeros(4))


def _quad(p0, ex, ey):
    """The parallelogram p0 + s ex + t ey, s, t in [0, 1], as two triangles (0, 1, 3), (0, 3, 2): (pos4, norm4, tang4, uv, idx), normal ex x ey, tangent ex."""
    p0, ex, ey = (np.asarray(v, np.float64) for v in (p0, ex, ey))
    n = np.cross(ex, ey)
    n /= np.linalg.norm(n)
    pos = np.stack([p0, p0 + ex, p0 + ey, p0 + ex + ey])
    pos4 = np.concatenate([pos, np.ones((4, 1))], 1).astype(np.float32)
    norm4 = np.tile(np.append(n, 0.0), (4, 1)).astype(np.float32)
    tang4 = np.tile(np.append(ex / np.linalg.norm(ex), 0.0), (4, 1)).astype(np.float32)
    uv = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    return pos4, norm4, tang4, uv, np.array([0, 1, 3, 0, 3, 2], np.uint32)


def _merge(parts):
    """(pos4, norm4, tang4, uv, idx, material id) pieces -> one mesh with a material id per triangle."""
    pos, nrm, tng, uv, idx, mat, base = [], [], [], [], [], [], 0
    for p, n, t, u, i, m in parts:
        pos.append(p); nrm.append(n); tng.append(t); uv.append(u)
        idx.append(i + base); mat.append(np.full(i.size // 3, m, np.uint32))
        base += p.shape[0]
    return (np.concatenate(pos), np.concatenate(nrm), np.concatenate(tng), np.concatenate(uv), np.concatenate(idx).astype(np.uint32), np.concatenate(mat))


# ---- the geometry all three scenes share --------------------------------------------------------------------------------------------------------
HALF = 2.0                                      # the quad is 4 x 4 in its own frame, normal +y, tangent +x
GAP = 0.01                                      # h: the distance of the black quads (G) and of the floors (T) from the plane
AXIS, TURN = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0), math.radians(40.0)
SHIFT = np.array([0.3, -0.2, -0.6])
P_OUT, P_IN = np.array([-1.0, 0.0, 0.4]), np.array([1.0, 0.0, 0.2])   # where the rays from outside / from inside meet the plane (both 0.42 / 0.85 off the diagonal x = -z)
JITTER = 0.05
CAM_LOCAL, FOV = np.array([0.9, 1.6, 3.4]), 62.0


def instance_matrix():
    """A rotation by 40 deg about (1, 2, 3) and a shift: no axis of the quad's frame stays an axis of the world."""
    x, y, z = AXIS
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(TURN) * K + (1 - math.cos(TURN)) * (K @ K)
    M[:3, 3] = SHIFT
    return M


def _to_world(p):
    M = instance_matrix()
    return np.asarray(p, np.float64) @ M[:3, :3].T + M[:3, 3]


def _base_scene(width, height, depth):
    sc = S.SceneData()
    sc.width, sc.height = width, height
    M = instance_matrix()
    sc.cam_pos = tuple(_to_world(CAM_LOCAL))
    sc.cam_look_at = tuple(_to_world((0.0, 0.0, 0.0)))
    sc.cam_up = tuple(M[:3, :3] @ np.array([0.0, 1.0, 0.0]))
    sc.fov, sc.trace_depth = FOV, depth
    return sc


def goniometer(case, width=1024, height=512, depth=2, pinhole=False, moving=False):
    """Scene G. Materials: the case's (id 0, or 1 behind the other film), then black Lambert. The quad carries the case's material; black quads lie
    at -h under the landing zone of the rays from outside and at +h over that of the rays from inside, so that a refracted ray ends black and a
    reflected one leaves (the rays from outside travel towards -x, those from inside towards +x, away from the other zone's quad). pinhole: one
    black quad under the whole plane instead (the camera is above it). moving: the instance has two equal key matrices (see below)."""
    sc = _base_scene(width, height, depth)
    sc.env_color = ENV
    mid = _material(sc, case)
    assert mid == case_material_id(sc, case)
    sc.materials.append(S.material_lambert((0.0, 0.0, 0.0)))
    black = len(sc.materials) - 1
    parts = [(*_quad((-HALF, 0, HALF), (2 * HALF, 0, 0), (0, 0, -2 * HALF)), mid)]
    if pinhole:
        parts.append((*_quad((-HALF, -GAP, HALF), (2 * HALF, 0, 0), (0, 0, -2 * HALF)), black))
    else:
        parts.append((*_quad((-1.9, -GAP, 1.6), (1.7, 0, 0), (0, 0, -2.4)), black))      # x in [-1.9, -0.2], z in [-0.8, 1.6]
        parts.append((*_quad((0.2, GAP, 1.4), (1.7, 0, 0), (0, 0, -2.4)), black))        # x in [0.2, 1.9], z in [-1.0, 1.4]
    M = instance_matrix()
    pos4, norm4, tang4, uv, idx, mat = _merge(parts)
    if moving:
        # kernel_RayTrace2 gives a moving instance's normal as lerp(N1 n, N2 (N1 n), time) (integrator_pt.cpp:285-291): the end key's normal matrix
        # is applied to the already transformed normal, so two equal keys leave the normal alone only when they do not rotate. The rotation goes
        # into the vertices here and the two equal keys are the shift: the same world-space scene, the same values.
        R = M[:3, :3]
        pos4 = np.concatenate([pos4[:, :3].astype(np.float64) @ R.T, np.ones((pos4.shape[0], 1))], 1).astype(np.float32)
        norm4 = np.concatenate([norm4[:, :3].astype(np.float64) @ R.T, np.zeros((pos4.shape[0], 1))], 1).astype(np.float32)
        tang4 = np.concatenate([tang4[:, :3].astype(np.float64) @ R.T, np.zeros((pos4.shape[0], 1))], 1).astype(np.float32)
        T = np.eye(4); T[:3, 3] = M[:3, 3]
        sc.add_instance(sc.add_mesh(pos4, norm4, tang4, uv, idx, mat), T, motion_matrix=T.copy())
    else:
        sc.add_instance(sc.add_mesh(pos4, norm4, tang4, uv, idx, mat), M)
    return sc


T_GAP = 0.25                                    # T: the floors' distance from the plane
STRIP_X = 1.0                                   # the lower strip's centre line is x = +1, the upper one's x = -1, both along z
STRIP_W = 1e-4 * T_GAP                          # half-width
T_REACH = 1.8                                   # a refracted ray may travel this far sideways before the floor (the quad is 4 wide); steeper angles are left out


def snell_target(case):
    """Scene T: the dielectric quad under a black environment, black floors at -h and +h, each with one emissive strip of half-width 1e-4 h along z
    (the lower at x = +1 for the rays from outside, which travel towards +x; the upper at x = -1 for those from inside, which travel towards -x)."""
    assert case.kind == "dielectric"
    sc = _base_scene(512, 512, 2)
    mid = _material(sc, case)
    sc.materials.append(S.material_lambert((0.0, 0.0, 0.0)))
    sc.materials.append(S.material_emissive(EMIT))
    black, emit = mid + 1, mid + 2
    parts = [(*_quad((-HALF, 0, HALF), (2 * HALF, 0, 0), (0, 0, -2 * HALF)), mid)]
    for y, xs in ((-T_GAP, STRIP_X), (T_GAP, -STRIP_X)):
        parts.append((*_quad((-HALF, y, HALF), (xs - STRIP_W + HALF, 0, 0), (0, 0, -2 * HALF)), black))
        parts.append((*_quad((xs - STRIP_W, y, HALF), (2 * STRIP_W, 0, 0), (0, 0, -2 * HALF)), emit))
        parts.append((*_quad((xs + STRIP_W, y, HALF), (HALF - xs - STRIP_W, 0, 0), (0, 0, -2 * HALF)), black))
    sc.add_instance(sc.add_mesh(*_merge(parts)), instance_matrix())
    return sc


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------------
def _camera_rays(sc, origin_w, dir_w, lam):
    """World-space float64 rays -> the float32 camera-space arrays PathTraceFromInputRaysBlock takes (wavelength in the position's fourth float)."""
    wv = S.look_at(sc.cam_pos, sc.cam_look_at, sc.cam_up)
    n = origin_w.shape[0]
    pos, dr = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = origin_w @ wv[:3, :3].T + wv[:3, 3]
    pos[:, 3] = lam
    dr[:, :3] = dir_w @ wv[:3, :3].T
    return pos, dr


def _azimuth(i, inside):
    """The direction of travel within the plane: within 50 deg of -x for the rays from outside, of +x for those from inside; it changes with the angle's
    number, so that the tangent frame meets the ray under many azimuths."""
    return math.radians((0.0 if inside else 180.0) - 50.0 + 100.0 * ((i * 0.6180339887) % 1.0))


def _local_ray(theta_deg, phi, inside, hit, height):
    """A ray that meets the plane y = 0 at `hit` under theta, travelling along phi, started at |y| = height on its side; (origin, direction), local."""
    th = math.radians(theta_deg)
    side = -1.0 if inside else 1.0
    d = np.array([math.sin(th) * math.cos(phi), -side * math.cos(th), math.sin(th) * math.sin(phi)])
    return hit - d * (height / math.cos(th)), d


def goniometer_rays(sc, case, copies, seed=11):
    """(pos, dir, group): `copies` rays per (wavelength, angle), group = the index of that pair; all of a group share the direction, their meeting
    points are scattered within JITTER of P_OUT / P_IN."""
    r = np.random.RandomState(seed)
    M = instance_matrix()
    o, d, lam, grp = [], [], [], []
    g = 0
    for wl in case.wavelengths():
        for i, th in enumerate(case.angles()):
            hit = (P_IN if case.inside else P_OUT) + np.stack([r.uniform(-JITTER, JITTER, copies), np.zeros(copies), r.uniform(-JITTER, JITTER, copies)], 1)
            _, ld = _local_ray(th, _azimuth(i, case.inside), case.inside, np.zeros(3), 0.5 * GAP)
            o.append(hit - ld * (0.5 * GAP / math.cos(math.radians(th)))); d.append(np.tile(ld, (copies, 1)))
            lam.append(np.full(copies, wl)); grp.append(np.full(copies, g))
            g += 1
    o, d = np.concatenate(o) @ M[:3, :3].T + M[:3, 3], np.concatenate(d) @ M[:3, :3].T
    pos, dr = _camera_rays(sc, o, d, np.concatenate(lam).astype(np.float32))
    return pos, dr, np.concatenate(grp)


def groups(case):
    """[(wavelength, angle in degrees)] in the order of goniometer_rays' group numbers."""
    return [(wl, th) for wl in case.wavelengths() for th in case.angles()]


def world_rays(sc, pos, dr):
    """The float32 camera-space rays through the scene's float32 worldViewInv, in float64: (origin [n, 3], unit direction [n, 3])."""
    m = np.asarray(list(sc.params().worldViewInv), np.float32).astype(np.float64).reshape(4, 4).T      # column-major storage
    o = pos[:, :3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    d = dr[:, :3].astype(np.float64) @ m[:3, :3].T
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


def plane(sc):
    """The quad as uploaded: (point [3], unit normal [3] from the float32 normal matrix, local frame as a function world -> local [.., 3])."""
    M = np.asarray(sc.inst_matrices[0], np.float64)
    M32 = S.colmajor(M).astype(np.float64).reshape(4, 4).T
    nm = S.colmajor(np.linalg.inv(M).T).astype(np.float64).reshape(4, 4).T
    n = nm[:3, :3] @ sc.vdata[0, 0:3].astype(np.float64)
    n /= np.linalg.norm(n)
    p0 = M32[:3, :3] @ np.zeros(3) + M32[:3, 3]
    inv = np.linalg.inv(M32)
    return p0, n, (lambda w: np.asarray(w, np.float64) @ inv[:3, :3].T + inv[:3, 3])


def meet(sc, o, d):
    """Where the rays meet the quad's plane: (cos of the incidence angle [n] (positive: from the normal's side), local hit points [n, 3], t [n])."""
    p0, n, to_local = plane(sc)
    dn = d @ n
    t = ((p0 - o) @ n) / dn
    return -dn, to_local(o + t[:, None] * d), t


def inside_margin(local):
    """How far the local points lie inside one triangle of the quad: the smallest of the distances to the rim and to the diagonal x = -z."""
    x, z = local[:, 0], local[:, 2]
    rim = np.minimum(HALF - np.abs(x), HALF - np.abs(z))
    return np.minimum(rim, np.abs(x + z) / math.sqrt(2.0))


def _per_ray(sc, case, c, lam):
    """sample_values for every ray, evaluated once per distinct (cosine, wavelength)."""
    keys, inv = np.unique(np.stack([c, lam], 1), axis=0, return_inverse=True)
    vals = [sample_values(sc, case, k[0], k[1]) for k in keys]
    inv = inv.reshape(-1)
    return (np.array([v[0] for v in vals])[inv], np.array([v[1] for v in vals])[inv], np.array([v[2] for v in vals])[inv])


def expected(sc, case, pos, dr, scale=ENV):
    """Per ray: (p_reflect [n], value of a reflected sample [n, 4]) in G, where a refracted sample ends black and is 0."""
    o, d = world_rays(sc, pos, dr)
    c = np.abs(meet(sc, o, d)[0])
    p, w, _ = _per_ray(sc, case, c, pos[:, 3].astype(np.float64))
    return p, w * np.asarray(scale, np.float64)


# ---- scene T ----------------------------------------------------------------------------------------------------------------------------------------
def snell_angles(case):
    """The case's angles whose refracted ray reaches the floor within T_REACH (for the dispersive one: at its largest index)."""
    n_in = cauchy(LAMBDA_MIN, 1.45, 1.5e4) if case.dispersive else case.eta
    n_i, n_t = (n_in, case.ext) if case.inside else (case.ext, n_in)
    keep = []
    for th in case.angles():
        s = math.sin(math.radians(th)) * n_i / n_t
        if s < 1.0 and T_GAP * s / math.sqrt(1.0 - s * s) <= T_REACH:
            keep.append(th)
    return tuple(keep)


def snell_groups(case):
    return [(wl, th) for wl in case.wavelengths() for th in snell_angles(case)]


def _landing(sc, case, o, d, lam):
    """Where the refracted continuation of the world-space rays (o, d) lands on the far floor, as the local x minus the far strip's centre line. The
    continuation starts where the reference's text puts it: the hit taken at t (1 - 1e-6) (integrator_pt.cpp:240), moved on by 2e-6 t along the ray
    (:536) and by 1e-5 max|coordinate| along the normal to the far side (:539, cglobals.h:233-247)."""
    p0, n, to_local = plane(sc)
    c, local, t = meet(sc, o, d)
    rot = lambda v: to_local(v) - to_local(np.zeros(3))
    land = np.zeros(c.size)
    for i in range(c.size):
        ix = indices(sc, case, lam[i])
        n_i, n_t = (ix["eta"], ix["ext"]) if case.inside else (ix["ext"], ix["eta"])
        nn = n if c[i] > 0 else -n
        hit = o[i] + t[i] * (1.0 - 1e-6) * d[i]
        start = to_local(hit + 2e-6 * t[i] * d[i] - 1e-5 * max(np.abs(hit).max(), 2e-5) * nn)
        tr = rot(refract(d[i], nn, n_i, n_t))
        far_y, far_x = (T_GAP, -STRIP_X) if case.inside else (-T_GAP, STRIP_X)
        land[i] = start[0] + tr[0] * ((far_y - start[1]) / tr[1]) - far_x
    return land, local


def snell_rays(sc, case, copies, shift=0.0, seed=13, tol=0.1):
    """Rays whose float64 refracted continuation lands on the centre line of the strip on the other side (shift = 0), or `shift` beside it. The rays
    are float32: of the candidates (one z per draw) those are kept whose landing point, computed from the float32 ray, is within tol * w of where
    it should be. Returns (pos, dir, group) as goniometer_rays does."""
    r = np.random.RandomState(seed)
    M = instance_matrix()
    pos_l, dir_l, grp = [], [], []
    g = 0
    for wl in case.wavelengths():
        ix = indices(sc, case, wl)
        n_i, n_t = (ix["eta"], ix["ext"]) if case.inside else (ix["ext"], ix["eta"])
        for th in snell_angles(case):
            phi = math.pi if case.inside else 0.0                         # across the strip
            side = -1.0 if case.inside else 1.0
            _, ld = _local_ray(th, phi, case.inside, np.zeros(3), 0.5 * GAP)
            tr = refract(ld, np.array([0.0, side, 0.0]), n_i, n_t)
            reach = tr[0] * (T_GAP / abs(tr[1]))
            have = 0
            while have < copies:
                m = 4 * copies
                z = r.uniform(1.2, 1.7, m) * side
                x = np.full(m, (-STRIP_X if case.inside else STRIP_X) + shift - reach)
                for _ in range(3):                                       # aim, look where the modelled start puts the landing point, aim again
                    hit = np.stack([x, np.zeros(m), z], 1)
                    lo = hit - ld * (0.5 * GAP / math.cos(math.radians(th)))
                    o, d = lo @ M[:3, :3].T + M[:3, 3], np.tile(ld @ M[:3, :3].T, (m, 1))
                    pos, dr = _camera_rays(sc, o, d, np.full(m, wl, np.float32))
                    land, _ = _landing(sc, case, *world_rays(sc, pos, dr), pos[:, 3].astype(np.float64))
                    x = x - (land - shift)
                good = np.nonzero(np.abs(land - shift) <= tol * STRIP_W)[0][:copies - have]
                pos_l.append(pos[good]); dir_l.append(dr[good]); grp += [g] * good.size
                have += good.size
            g += 1
    return np.ascontiguousarray(np.concatenate(pos_l)), np.ascontiguousarray(np.concatenate(dir_l)), np.asarray(grp)


def snell_landing(sc, case, pos, dr):
    """(landing point of the float64 refracted continuation minus the far strip's centre line [n], local hit points on the quad [n, 3])."""
    return _landing(sc, case, *world_rays(sc, pos, dr), pos[:, 3].astype(np.float64))


def snell_expected(sc, case, pos, dr):
    """Per ray of T: (p_reflect [n], value of a refracted sample that lands on the strip [n, 4]); a reflected sample is 0."""
    o, d = world_rays(sc, pos, dr)
    c = np.abs(meet(sc, o, d)[0])
    p, _, wt = _per_ray(sc, case, c, pos[:, 3].astype(np.float64))
    return p, wt * np.append(np.asarray(EMIT, np.float64), 0.0)


# ---- the two checks of a two-valued case ------------------------------------------------------------------------------------------------------------
def counts(out, value, passes, eps):
    """out [n, c] sums of `passes` samples, each 0 or value [n, c]: (k int [n], ok bool [n]) - the number of non-zero samples per ray, read off the
    channel where the value is largest, and whether every channel is within passes * eps * value of k * value with 0 <= k <= passes."""
    out, value = np.asarray(out, np.float64), np.asarray(value, np.float64)[:, :out.shape[1]]
    j = np.argmax(value, axis=1)
    rows = np.arange(out.shape[0])
    k = np.rint(out[rows, j] / value[rows, j]).astype(np.int64)
    ok = np.all(np.isfinite(out), 1) & (k >= 0) & (k <= passes) & np.all(np.abs(out - k[:, None] * value) <= passes * eps * value, axis=1)
    return k, ok


def count_bound(n, p):
    """|K - n p| <= 5 sqrt(n p (1 - p)) + 1: five standard deviations of the binomial count (two-sided tail about 6e-7) plus one for the rounding
    of n p; where p is exactly 0 or 1 the count must be exact."""
    return 0.0 if p in (0.0, 1.0) else 5.0 * math.sqrt(n * p * (1.0 - p)) + 1.0


def excursion(out, value, passes):
    """The worst relative distance of a deterministic case's outputs from passes * value, over the channels where the value is not 0."""
    out, value = np.asarray(out, np.float64), np.asarray(value, np.float64)[:, :out.shape[1]]
    nz = value > 0
    assert np.all(out[~nz] == 0.0)
    return float(np.max(np.abs(out[nz] - passes * value[nz]) / (passes * value[nz])))


# ---- G through the pinhole camera ---------------------------------------------------------------------------------------------------------------------
RIM_MARGIN = 0.1                                # a footprint within this of the quad's rim counts as crossing it (the refracted rays' landing zone)
INSIDE, RIM, OUTSIDE = 0, 1, 2


@functools.lru_cache(maxsize=None)
def pinhole_footprints(case_name, grid=9):
    """Per pixel of the 48 x 40 frame of goniometer(case, pinhole=True): (class [H, W], lo [H, W, 4], hi [H, W, 4], p_lo [H, W], p_hi [H, W]) - the
    smallest and the largest value of a reflected sample (w_reflect * ENV) and of the reflection probability over a 9 x 9 grid of the pixel's
    footprint, borders included (pixel (x, y) takes its rays from [x, x + 1] x [y, y + 1], integrator_pt.cpp:57-66)."""
    case = CASE[case_name]
    sc = goniometer(case, WIDTH, HEIGHT, pinhole=True)
    prm = sc.params()
    pi = np.asarray(list(prm.projInv), np.float32).astype(np.float64).reshape(4, 4).T
    u = np.linspace(0.0, 1.0, grid)
    xs = (np.arange(WIDTH)[:, None] + u[None, :]).reshape(-1) / WIDTH
    ys = (np.arange(HEIGHT)[:, None] + u[None, :]).reshape(-1) / HEIGHT
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    clip = np.stack([2 * X - 1, 2 * Y - 1, np.zeros_like(X), np.ones_like(X)], -1) @ pi.T               # EyeRayDirNormalized (cglobals.h:49-55)
    d = clip[..., :3] / clip[..., 3:4]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o, dw = world_rays_f64(sc, d.reshape(-1, 3))
    c, local, t = meet(sc, o, dw)
    hit = (t > 0) & (c > 0)
    edge = np.minimum(HALF - np.abs(local[:, 0]), HALF - np.abs(local[:, 2]))
    inside = (hit & (edge > RIM_MARGIN)).reshape(HEIGHT, grid, WIDTH, grid)
    outside = (~hit | (edge < -RIM_MARGIN)).reshape(HEIGHT, grid, WIDTH, grid)
    cls = np.full((HEIGHT, WIDTH), RIM)
    cls[inside.all((1, 3))] = INSIDE
    cls[outside.all((1, 3))] = OUTSIDE
    cg = np.abs(c).reshape(HEIGHT, grid, WIDTH, grid)
    lo, hi = np.zeros((HEIGHT, WIDTH, 4)), np.zeros((HEIGHT, WIDTH, 4))
    p_lo, p_hi = np.zeros((HEIGHT, WIDTH)), np.zeros((HEIGHT, WIDTH))
    env = np.asarray(ENV, np.float64)
    for y, x in zip(*np.nonzero(cls == INSIDE)):
        vals = [sample_values(sc, case, cc, 0.0) for cc in cg[y, :, x, :].reshape(-1)]
        w = np.array([v[1] for v in vals]) * env
        p = np.array([v[0] for v in vals])
        lo[y, x], hi[y, x], p_lo[y, x], p_hi[y, x] = w.min(0), w.max(0), p.min(), p.max()
    for a in (cls, lo, hi, p_lo, p_hi):
        a.setflags(write=False)
    return cls, lo, hi, p_lo, p_hi


def world_rays_f64(sc, d_cam):
    """Camera-space unit directions from the eye [n, 3] through the scene's float32 worldViewInv: (origin [n, 3], unit direction [n, 3])."""
    m = np.asarray(list(sc.params().worldViewInv), np.float32).astype(np.float64).reshape(4, 4).T
    d = d_cam @ m[:3, :3].T
    return np.broadcast_to(m[:3, 3], d.shape).copy(), d / np.linalg.norm(d, axis=1, keepdims=True)


PINHOLE_CASES = ("conductor_0.2_3.9", "film_rgb_conductor", "dielectric_out")
PINHOLE_COUNTS = (622, 318, 980)                           # (inside, rim, outside) pixels of the 48 x 40 frame: a geometric fact of the scene, the same for every case


# ---- the checks, shared by the oracle's and the device's tests ------------------------------------------------------------------------------------------
def check_deterministic(out, value, passes, eps, what):
    """Every output within passes * eps * value of passes * value; returns the worst relative excursion."""
    worst = excursion(out, value, passes)
    print(f"{what}: worst relative excursion {worst:.3e} (allowed {eps:.3e})")
    assert np.isfinite(out).all() and worst <= eps, f"{what}: worst relative excursion {worst:.3e} above {eps:.3e}"
    return worst


def check_two_valued(out, p, value, grp, names, passes, eps, what):
    """The value check per ray and the count check per group (one wavelength and angle)."""
    k, ok = counts(out, value, passes, eps)
    assert ok.all(), f"{what}: {int((~ok).sum())} rays are no k * value, first {np.nonzero(~ok)[0][:3]}: {out[~ok][:3]} against value {value[~ok][:3]}"
    for g in np.unique(grp):
        sel = grp == g
        n, pg = int(sel.sum()) * passes, float(p[sel].mean())
        assert np.ptp(p[sel]) <= 1e-9, (what, names[g])                   # the copies of one ray share the angle
        K, bound = int(k[sel].sum()), count_bound(n, pg)
        print(f"{what}, {names[g]}: K = {K} of n = {n}, n p = {n * pg:.1f}, allowed +- {bound:.1f}")
        assert abs(K - n * pg) <= bound, f"{what}, {names[g]}: K = {K} of n = {n}, n p = {n * pg:.1f}, allowed +- {bound:.1f}"


def pinhole_depth(naive):
    """One bounce, then the environment: PathTrace traces m_traceDepth times, NaivePathTrace once more (integrator_pt.cpp:696, :735) - the k_max rule of
    tests/furnace_reference.py with k_max = 1."""
    return 1 if naive else 2


def check_pinhole_frame(img, case_name, passes, what, eps=None):
    """img [H, W, c] sums of `passes` samples per pixel, c = 1 (the red channel), 3 or 4. Pixels off the quad hold the environment exactly; a pixel
    on an opaque quad has its mean within [min, max] of the value over its footprint, widened by eps; a pixel on the dielectric holds k * ENV with
    an integer k, and the frame's total K lies within five standard deviations of [sum passes * min R, sum passes * max R]. Rim pixels are not
    compared. Returns the worst excursion beyond the interval (opaque) or from k * ENV (dielectric)."""
    eps = EPS if eps is None else eps
    case = CASE[case_name]
    cls, lo, hi, p_lo, p_hi = pinhole_footprints(case_name)
    img = np.asarray(img)
    c = min(img.shape[-1], 3)
    v = img[..., :c].astype(np.float64)
    env = np.asarray(ENV, np.float64)[:c]
    assert np.isfinite(img).all() and (img >= 0).all(), what
    off = cls == OUTSIDE
    assert np.all(v[off] == passes * env), f"{what}: {int(np.any(v[off] != passes * env, -1).sum())} pixels off the quad do not hold the environment"
    on = cls == INSIDE
    if case.opaque:
        mean = v[on] / passes
        l, h = lo[on][:, :c], hi[on][:, :c]
        exc = np.maximum(np.maximum((l - mean) / l, (mean - h) / h), 0.0)
        print(f"{what}: {int(on.sum())} pixels on the quad, worst excursion beyond the footprint's interval {exc.max():.3e}")
        assert exc.max() <= eps, f"{what}: {int((exc > eps).any(-1).sum())} pixels outside their footprint's interval, worst {exc.max():.3e}"
        return float(exc.max())
    value = np.broadcast_to(np.asarray(ENV, np.float64), (int(on.sum()), 4))
    k, ok = counts(v[on], value, passes, eps)
    assert ok.all(), f"{what}: {int((~ok).sum())} pixels are no k * environment, first {v[on][~ok][:3]}"
    pl, ph = p_lo[on], p_hi[on]
    var = np.maximum(pl * (1 - pl), ph * (1 - ph))
    var[(pl < 0.5) & (ph > 0.5)] = 0.25
    slack = 5.0 * math.sqrt(passes * var.sum()) + 1.0
    K = int(k.sum())
    print(f"{what}: K = {K}, allowed [{passes * pl.sum() - slack:.1f}, {passes * ph.sum() + slack:.1f}]")
    assert passes * pl.sum() - slack <= K <= passes * ph.sum() + slack, f"{what}: K = {K} outside [{passes * pl.sum() - slack:.1f}, {passes * ph.sum() + slack:.1f}]"
    return float(np.max(np.abs(v[on] - k[:, None] * env) / env))

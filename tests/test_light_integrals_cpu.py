"""Every light type against a float64 irradiance integral: the reference module against itself, then the CPU oracle through
PathTraceFromInputRaysBlock on every case of tests/light_integrals_reference.py, under the assertions the device is held to in
tests/test_light_integrals_gpu.py. Figures: profiles/light_integrals.md."""
import math

import numpy as np
import pytest

import light_integrals_reference as LR
from hydracore3_amd import scene as S
from hydracore3_amd import synth


# ---- the reference against itself ----------------------------------------------------------------------------------------------------
def test_sphere_quadrature_matches_the_closed_form():
    """A sphere wholly above the horizon: rho * Le * (R / d)^2 * cos(theta), to 1e-9. The sphere of the case, raised clear of the floor."""
    light = dict(LR.CASES["sphere"].lights[0], matrix=S.translate(0.1, 0.85, -0.2) @ S.scale(1.3, 1.3, 1.3))
    for P in LR.CASES["sphere"].points:
        I, _ = LR.sphere_moments(light, P)
        ref = LR.sphere_closed_form(light, P)
        assert np.all(np.abs(I - ref) <= 1e-9 * ref), (P, I, ref)
    # ... and the case's own sphere dips below the floor: the closed form counts the hidden part with its negative cosine, the visible
    # cap alone gives more, most at the nearest point
    case = LR.CASES["sphere"]
    frac = np.array([LR.sphere_moments(case.lights[0], P)[0][0] / max(LR.sphere_closed_form(case.lights[0], P)[0], 1e-300) for P in case.points])
    assert np.all(frac > 1.003) and np.all(frac < 1.01) and frac.argmax() == 0


def test_rect_quadrature_matches_the_form_factor_of_plane_under_rect_light():
    """The set-up of synth.plane_under_rect_light (a 1 x 1 light of radiance 10 at y = 2 over a floor of albedo 0.5), whose form factor
    tests/test_cpu.py::test_direct_lighting_matches_form_factor sums on a 64 x 64 midpoint grid: the two quadratures agree to the
    midpoint rule's error."""
    sc = synth.plane_under_rect_light()
    lt = sc.lights[0]
    assert lt["geomType"] == S.LIGHT_GEOM_RECT and tuple(lt["size"]) == (0.5, 0.5) and lt["mult"] == 10.0
    light = {"kind": "rect", "matrix": S.translate(0, 2.0, 0), "half": (0.5, 0.5), "color": (1, 1, 1), "mult": 10.0}
    g = (np.arange(64) + 0.5) / 64 - 0.5
    lx, lz = np.meshgrid(g, g)
    Lp = np.stack([lx, np.full_like(lx, 2.0), lz], -1).reshape(-1, 3)
    for P in ([0.0, 0.0, 0.0], [0.7, 0.0, -0.4], [2.0, 0.0, 1.5]):
        v = Lp - np.asarray(P)
        r2 = np.sum(v * v, -1)
        expect = 0.5 / np.pi * 10.0 * np.mean((v[:, 1] / np.sqrt(r2)) ** 2 / r2)
        I, _ = LR.rect_moments(light, np.asarray(P, np.float64))
        assert abs(I[0] / LR.ALBEDO[0] * 0.5 - expect) <= 2e-4 * expect


def test_disc_quadrature_converges_and_matches_the_far_field():
    light = LR.CASES["disc"].lights[0]
    P = LR.CASES["disc"].points[0]
    a, b = LR.disc_moments(light, P), LR.disc_moments(light, P, nr=96, nphi=384)
    assert np.allclose(a[0], b[0], rtol=1e-12) and np.allclose(a[1], b[1], rtol=1e-12)
    far = LR._pos(light) + 40.0 * LR._dirn(light)                      # on the axis, 50 emitter sizes away: a small source of area pi r^2 * 1.6
    area = math.pi * light["radius"] ** 2 * 1.6
    point_like = LR.ALBEDO / math.pi * LR._le(light) * area * -LR._dirn(light)[1] / 40.0 ** 2
    assert np.allclose(LR.disc_moments(light, far)[0], point_like, rtol=2e-3)


def test_env_quadrature_of_a_constant_map_is_the_furnace_value():
    env = {"map": np.ones((8, 16, 4)), "color": (1.0, 2.0, 0.5), "mult": 1.0}
    I, E2 = LR.env_moments(env)
    assert np.allclose(I, LR.ALBEDO * np.array([1.0, 2.0, 0.5]), rtol=1e-9)
    # the case's map: refining the rule does not move it
    env = LR.CASES["env"].env
    a, b = LR.env_moments(env, per=8), LR.env_moments(env, per=16)
    assert np.allclose(a[0], b[0], rtol=1e-9) and np.allclose(a[1], b[1], rtol=1e-9)
    assert abs(LR.env_table_pdf(env).mean() - 1.0) < 1e-12


def test_bilinear_fetch_rules():
    tex = np.arange(32, dtype=np.float64).reshape(4, 8)
    uv = np.array([[(1 + 0.5) / 8, (2 + 0.5) / 4], [0.5, 0.5], [0.01, 0.01], [0.999, 0.3]])
    r = LR.fetch_bilinear(tex, uv, (S.ADDR_CLAMP, S.ADDR_CLAMP))
    assert r[0] == tex[2, 1] and r[1] == tex[1:3, 3:5].mean() and r[2] == tex[0, 0]
    ffx, ffy = 0.999 * 8 - 0.5, 0.3 * 4 - 0.5                         # the upper edge wraps to texel 0, CLAMP or not
    fx, fy = ffx - 7, ffy - 0
    assert np.isclose(r[3], (tex[0, 7] * (1 - fx) + tex[0, 0] * fx) * (1 - fy) + (tex[1, 7] * (1 - fx) + tex[1, 0] * fx) * fy)


def test_delta_lights_have_no_variance_and_sums_add():
    for name in LR.DETERMINISTIC:
        I, sigma = LR.CASES[name].moments()
        assert np.all(sigma == 0.0), name
    assert set(LR.DETERMINISTIC) == {"omni", "lambert_point", "spot", "directional", "ies", "projector"}
    two, rect, spot = LR.CASES["two_lights"], LR.CASES["rect"], LR.CASES["spot"]
    for i, P in enumerate(two.points):
        assert np.array_equal(two.moments()[0][i], rect.light_moments(LR.RECT, P)[0] + spot.light_moments(LR.SPOT, P)[0])
    assert np.all(two.moments()[1][two.moments()[0] > 0] > 0)          # picking one of two lights is never deterministic where either shines


# ---- the case table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LR.CASES))
def test_case_table_keeps_its_own_rules(name):
    case = LR.CASES[name]
    I, _ = case.moments()
    assert case.primary_rays_reach_the_floor()
    assert case.emitter_distance() >= 1.0                              # no point closer to an area emitter than its larger half size
    assert np.all((I == 0).all(1) | (I > 0).all(1))
    if name not in ("env", "sphere"):                                  # (the sky and a sphere light every point of an open floor)
        assert (I == 0).all(1).any(), "a point where the answer is exactly 0"
    cos_inc = []
    for l in case.lights:
        if l["kind"] != "directional":
            v = LR._pos(l) - case.points
            cos_inc.append(v[:, 1] / np.linalg.norm(v, axis=1))
    if cos_inc and name not in ("spot", "projector", "two_lights"):
        c = np.array(cos_inc[0])
        assert np.isclose(c, 1.0).any() or name == "sphere", "a point under the light"
        assert ((c <= math.cos(math.radians(59.9))) & (c >= math.cos(math.radians(80.1))) & (I[:, 0] > 0)).sum() >= 2, "points at 60-80 degrees"
    if name in ("spot", "projector"):
        ang = np.degrees(np.arccos([-(LR._unit(LR._pos(LR.SPOT) - P) @ LR._dirn(LR.SPOT)) for P in case.points]))
        assert (ang < 20).sum() >= 3 and ((ang > 20) & (ang < 35)).sum() >= 3 and (ang > 35).sum() >= 3
        assert np.all((I[:, 0] == 0) == (ang > 35))
    if not case.deterministic:
        lit = I > 0
        assert np.all(case.bound()[lit] <= 0.01 * I[lit]), (case.bound()[lit] / I[lit]).max()
        assert np.all(case.sigma()[lit] > 0)


# ---- the oracle against the integrals --------------------------------------------------------------------------------------------------
def _oracle(case):
    from oracle.orc import OracleIntegrator
    sc = case.scene()
    o = OracleIntegrator(sc, case.params(sc))
    pos, dr = case.rays()
    out = np.zeros((pos.shape[0], 4), np.float32)
    o.path_trace_from_input_rays_block(pos, dr, out, case.pass_num, 4)
    return out


@pytest.mark.parametrize("name", list(LR.CASES))
def test_oracle_matches_the_integral(name):
    """|value - I| <= DELTA_BOUND * I for the delta lights, |mean - I| <= 5 sigma / sqrt(N) for the others, exactly 0 where I is 0: every
    point, every channel."""
    case = LR.CASES[name]
    LR.check_against_integral(case, _oracle(case), "oracle")


def test_oracle_worst_deterministic_error_is_the_recorded_one():
    """DELTA_BOUND is four times the oracle's worst error over the deterministic cases (profiles/light_integrals.md): the recorded figure
    covers what the oracle gives and is not slack by more than a tenth of it."""
    worst = max(LR.delta_errors(LR.CASES[n], _oracle(LR.CASES[n])).max() for n in LR.DETERMINISTIC)
    print(f"oracle: worst deterministic relative error {worst:.3e}")
    assert 0.9 * LR.ORACLE_WORST_DELTA_ERROR <= worst <= LR.ORACLE_WORST_DELTA_ERROR
    assert LR.DELTA_BOUND == 4.0 * LR.ORACLE_WORST_DELTA_ERROR

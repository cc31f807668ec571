"""The float64 statement of the smooth interfaces (tests/specular_reference.py) checked against itself and pinned on the oracle: the conditions the GPU
tests rest on - EPS, that every ray meets the quad inside one triangle, that the Snell target's off-target rays are black, the pinhole frame's rim
count - hold here before a device kernel sees the scenes. Figures: profiles/specular.md.

Trials per angle of a two-valued case: n = 256 copies x 16 passes = 4096 here, 4096 copies x 64 passes = 2^18 on the device (test_specular_gpu.py)."""
import math

import numpy as np
import pytest

import specular_reference as SR
from hydracore3_amd import scene as S

COPIES, PASSES = 256, 16                     # two-valued cases
DET_COPIES, DET_PASSES = 5, 3                # deterministic cases
NAMES = [c.name for c in SR.CASES]
TWO_VALUED = [c.name for c in SR.CASES if not c.opaque]
DETERMINISTIC = [c.name for c in SR.CASES if c.opaque]
SNELL = [c.name for c in SR.CASES if c.kind == "dielectric"]


def _oracle(sc, integrator=S.INTEGRATOR_MIS_PT):
    from oracle.orc import OracleIntegrator
    return OracleIntegrator(sc, sc.params(integrator=integrator))


def _label(case):
    return [f"{wl:.2f} nm, {th:.3f} deg" for wl, th in SR.groups(case)]


@pytest.fixture(scope="module")
def runs():
    """{case name: (scene, pos, dir, group, p_reflect, value, output)} of G on the oracle, traced once per case."""
    cache = {}

    def get(name):
        if name not in cache:
            case = SR.CASE[name]
            sc = SR.goniometer(case)
            copies, passes = (DET_COPIES, DET_PASSES) if case.opaque else (COPIES, PASSES)
            pos, dr, grp = SR.goniometer_rays(sc, case, copies)
            assert pos.shape[0] <= sc.width * sc.height
            p, value = SR.expected(sc, case, pos, dr)
            out = np.zeros((pos.shape[0], 4), np.float32)
            _oracle(sc).path_trace_from_input_rays_block(pos, dr, out, passes, 4)
            for a in (pos, dr, grp, p, value, out):
                a.setflags(write=False)
            cache[name] = (sc, pos, dr, grp, p, value, out)
        return cache[name]
    return get


# ---- the statement against itself -------------------------------------------------------------------------------------------------------------------
def test_fresnel_at_normal_incidence_brewster_and_grazing():
    for n in (1.5, 1.01, 2.4):
        assert SR.fresnel_dielectric(1.0, 1.0, n) == pytest.approx(((n - 1) / (n + 1)) ** 2, rel=1e-14)
        assert SR.fresnel_dielectric(1.0, n, 1.0) == pytest.approx(((n - 1) / (n + 1)) ** 2, rel=1e-14)
        b = math.atan(n)                                                   # Brewster: the p term vanishes, what is left is half the s term
        rs = math.cos(2 * b) ** 2                                          # r_s at Brewster's angle = -cos(2 theta_B)
        assert SR.fresnel_dielectric(math.cos(b), 1.0, n) == pytest.approx(0.5 * rs, rel=1e-12)
        assert SR.fresnel_dielectric(1e-9, 1.0, n) == pytest.approx(1.0, abs=1e-7)
        crit = math.asin(1.0 / n)
        assert SR.fresnel_dielectric(math.cos(crit + 1e-6), n, 1.0) == 1.0 and SR.fresnel_dielectric(math.cos(crit - 1e-3), n, 1.0) < 1.0
    assert SR.fresnel_dielectric(0.3, 1.3, 1.3) < 1e-30


def test_reciprocity_of_the_dielectric_interface():
    """R from outside under theta equals R from inside under the refracted angle (Stokes)."""
    for th in (5.0, 40.0, 75.0, 89.0):
        c = math.cos(math.radians(th))
        ct = math.sqrt(1 - (1 - c * c) / 1.5 ** 2)
        assert SR.fresnel_dielectric(c, 1.0, 1.5) == pytest.approx(float(SR.fresnel_dielectric(ct, 1.5, 1.0)), rel=1e-12)


def test_conductor_without_absorption_is_the_dielectric_and_normal_incidence():
    c = np.cos(np.radians(np.array(SR.ANGLES)))
    assert np.allclose(SR.fresnel_conductor(c, 1.5, 0.0), SR.fresnel_dielectric(c, 1.0, 1.5), rtol=1e-13)
    n, k = 0.2, 3.9
    assert SR.fresnel_conductor(1.0, n, k) == pytest.approx(((n - 1) ** 2 + k * k) / ((n + 1) ** 2 + k * k), rel=1e-13)
    assert np.allclose(SR.fresnel_conductor(c, n, k), SR.fresnel_conductor(c, n, -k), rtol=1e-13)     # |r|^2 does not see the sign of k


def test_snell_in_vector_form():
    n = np.array([0.0, 1.0, 0.0])
    for th in (0.0, 30.0, 89.5):
        s, c = math.sin(math.radians(th)), math.cos(math.radians(th))
        t = SR.refract(np.array([s, -c, 0.0]), n, 1.0, 1.5)
        assert np.linalg.norm(t) == pytest.approx(1.0, rel=1e-14) and t[1] < 0
        assert 1.5 * t[0] == pytest.approx(s, rel=1e-13, abs=1e-15)        # n sin(theta) is kept
    assert SR.refract(np.array([math.sin(1.0), -math.cos(1.0), 0.0]), n, 1.5, 1.0) is None


def test_airy_limits_and_energy():
    c = np.cos(np.radians(np.array(SR.ANGLES)))
    R, T = SR.airy(c, 1.0, 2.0, 1.5, 250.0, 525.0)
    assert np.allclose(R + T, 1.0, rtol=1e-12)                             # no absorption: nothing is lost
    R0, T0 = SR.airy(c, 1.0, 2.0, 1.5, 0.0, 525.0)                         # no film: the bare interface
    assert np.allclose(R0, SR.fresnel_dielectric(c, 1.0, 1.5), rtol=1e-12)
    Rm, _ = SR.airy(c, 1.0, 1.5, 1.5, 300.0, 525.0)                        # a film of the substrate's index: the bare interface
    assert np.allclose(Rm, SR.fresnel_dielectric(c, 1.0, 1.5), rtol=1e-12)
    Rq, _ = SR.airy(1.0, 1.0, math.sqrt(1.5), 1.5, 525.0 / (4 * math.sqrt(1.5)), 525.0)   # the quarter-wave coating of index sqrt(n): no reflection
    assert Rq < 1e-28
    Ra, Ta = SR.airy(c, 1.0, complex(1.8, 0.05), complex(0.2, 3.9), 300.0, 525.0)
    assert np.all(Ra < 1.0) and np.all(Ra > 0.0)
    Rt, Tt = SR.airy(math.cos(math.radians(60.0)), 1.5, 2.0, 1.0, 250.0, 525.0)   # beyond the critical angle of substrate -> air: all comes back
    assert Rt == pytest.approx(1.0, rel=1e-12) and Tt == 0.0
    Rf, Tf = SR.airy(c, 1.0, 2.0, 1.5, 250.0, 525.0)
    ct = np.sqrt(1 - (1 - c * c) / 1.5 ** 2)
    Rb, Tb = SR.airy(ct, 1.5, 2.0, 1.0, 250.0, 525.0)
    assert np.allclose(Tf, Tb, rtol=1e-12)                                 # transmittance is the same both ways


def test_tables_of_the_scenes_agree_with_the_airy_sum_at_their_nodes():
    """What the table reads rest on: the scene's own spectral tables hold the Airy values at their nodes (host data, tested in test_cpu.py; here
    only that the float64 reader takes the node it means), forward and reversed."""
    for name in ("spectral_film_transparent_out", "spectral_film_transparent_in"):
        case = SR.CASE[name]
        sc = SR.goniometer(case)
        m = sc.materials[1]
        for j in (0, 57, 100, 177):
            th = j * (math.pi / 2) / (SR.FILM_ANGLE_RES - 1)
            lam = SR.LAMBDA_MIN + 30 * (SR.LAMBDA_MAX - SR.LAMBDA_MIN) / (SR.FILM_LENGTH_RES - 1)
            r, t = SR.film_table_spectral(sc, m, math.cos(th), lam, case.inside)
            n_i, n_t = (1.5, float(np.float32(case.ext))) if case.inside else (float(np.float32(case.ext)), 1.5)
            node = SR.LAMBDA_MIN + 30 * (SR.LAMBDA_MAX - SR.LAMBDA_MIN - 1) / (SR.FILM_LENGTH_RES - 1)   # the loader's nodes run to 829 nm (integrator_pt_scene_mat.cpp:791-890)
            ra, ta = SR.airy(max(math.cos(th), 1e-3), n_i, 2.0, n_t, 250.0, node)
            assert r == pytest.approx(float(ra), rel=2e-4, abs=2e-6) and t == pytest.approx(float(ta), rel=2e-4, abs=2e-6), (name, j)


def test_count_bound_and_value_check_reject_what_they_should():
    v = np.tile(np.array([[1.0, 2.0, 0.5, 0.25]]), (4, 1))
    out = np.array([3 * v[0], 3 * v[0] * (1 + 3 * SR.EPS), 17 * v[0], 2.5 * v[0]])
    k, ok = SR.counts(out, v, 16, SR.EPS)
    assert list(k[:3]) == [3, 3, 17] and list(ok) == [True, True, False, False]
    out[1] = 3 * v[0] * (1 + 17 * SR.EPS / 3)
    assert not SR.counts(out, v, 16, SR.EPS)[1][1]
    assert SR.count_bound(1000, 1.0) == 0.0 and SR.count_bound(1000, 0.0) == 0.0
    assert SR.count_bound(2 ** 18, 0.04) == pytest.approx(5 * math.sqrt(2 ** 18 * 0.04 * 0.96) + 1)


# ---- the conditions of the scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_ray_meets_the_quad_well_inside_one_triangle(name):
    case = SR.CASE[name]
    sc = SR.goniometer(case)
    pos, dr, grp = SR.goniometer_rays(sc, case, 16)
    o, d = SR.world_rays(sc, pos, dr)
    c, local, t = SR.meet(sc, o, d)
    assert np.all(t > 0) and np.all((c < 0) if case.inside else (c > 0))
    assert SR.inside_margin(local).min() > 1e-3 * 2 * SR.HALF             # off the rim and off the shared diagonal; no ray is left out
    want = np.cos(np.radians([th for _, th in SR.groups(case)]))[grp]
    assert np.allclose(np.abs(c), want, atol=2e-7)                         # the float32 rays still have the angles they were made for
    assert np.abs(c).min() > 5e-3                                          # far from the guards at 1e-6 and 1e-4
    # a refracted continuation ends on the black quad of its side, a reflected one passes the other black quad
    ix = SR.indices(sc, case, 525.0)
    if not case.opaque:
        n_in = ix["eta"]
        n_i, n_t = (n_in, ix["ext"]) if case.inside else (ix["ext"], n_in)
        s = np.sqrt(1 - c * c) * n_i / n_t
        reach = SR.GAP * s[s < 1] / np.sqrt(1 - s[s < 1] ** 2)
        assert reach.max() < 0.6, reach.max()                               # the black quads reach 0.8 beyond the meeting points along x, 1.2 along z


@pytest.mark.parametrize("name", SNELL)
def test_snell_target_rays_land_where_they_should(name):
    case = SR.CASE[name]
    sc = SR.snell_target(case)
    assert len(SR.snell_angles(case)) >= 4
    for shift in (0.0, 3 * SR.STRIP_W, -3 * SR.STRIP_W):
        pos, dr, grp = SR.snell_rays(sc, case, 4, shift)
        assert np.array_equal(np.bincount(grp), np.full(len(SR.snell_groups(case)), 4))
        land, local = SR.snell_landing(sc, case, pos, dr)
        print(f"{name}, shift {shift / SR.STRIP_W:+.0f} w: the float32 rays land within {np.abs(land - shift).max() / SR.STRIP_W:.3f} w of it")
        assert np.abs(land - shift).max() <= 0.1 * SR.STRIP_W             # on target: well inside the strip; off target: 2.9 w or more from its centre
        assert SR.inside_margin(local).min() > 1e-3 * 2 * SR.HALF
        # the reflected continuation travels on in the rays' direction and meets the near floor away from that floor's strip, which lies behind the ray
        assert np.all(local[:, 0] < SR.STRIP_X - 0.1) if case.inside else np.all(local[:, 0] > -SR.STRIP_X + 0.1)


def test_pinhole_frame_classes():
    cls = SR.pinhole_footprints(SR.PINHOLE_CASES[0])[0]
    got = tuple(int((cls == k).sum()) for k in (SR.INSIDE, SR.RIM, SR.OUTSIDE))
    print("pinhole frame: inside, rim, outside =", got)
    assert got == SR.PINHOLE_COUNTS and sum(got) == SR.WIDTH * SR.HEIGHT
    for name in SR.PINHOLE_CASES[1:]:
        assert np.array_equal(SR.pinhole_footprints(name)[0], cls)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DETERMINISTIC)
def test_oracle_holds_the_deterministic_values(runs, name):
    sc, pos, dr, grp, p, value, out = runs(name)
    assert np.all(p == 1.0)
    SR.check_deterministic(out[:, :SR.channels(SR.CASE[name])], value, DET_PASSES, SR.EPS, name)


@pytest.mark.parametrize("name", TWO_VALUED)
def test_oracle_holds_the_two_valued_cases(runs, name):
    sc, pos, dr, grp, p, value, out = runs(name)
    SR.check_two_valued(out[:, :SR.channels(SR.CASE[name])], p, value, grp, _label(SR.CASE[name]), PASSES, SR.EPS, name)
    if SR.CASE[name].inside:
        assert (p == 1.0).any() and (p < 1.0).any()                        # both sides of the critical angle occur


def test_eps_is_four_times_the_oracles_worst_excursion(runs):
    worst = {}
    for name in DETERMINISTIC:
        sc, pos, dr, grp, p, value, out = runs(name)
        c = SR.channels(SR.CASE[name])
        o, value = out.astype(np.float64)[:, :c], value[:, :c]
        rel = np.abs(o - DET_PASSES * value) / np.where(value > 0, DET_PASSES * value, 1.0)
        rel[~(value > 0)] = 0.0
        i = int(np.argmax(rel.max(1)))
        wl, th = SR.groups(SR.CASE[name])[grp[i]]
        worst[name] = (float(rel.max()), wl, th)
        print(f"{name}: worst excursion {rel.max():.3e} at {th:.3f} deg, {wl:.2f} nm")
    top = max(worst, key=lambda k: worst[k][0])
    print(f"EPS {SR.EPS:.3e}; the worst case is {top}: {worst[top]}")
    assert 4.0 * worst[top][0] <= SR.EPS < 1e-4
    assert SR.EPS <= 8.0 * worst[top][0]                                    # ... and the constant is not left wider than its measurement by a later edit


@pytest.mark.parametrize("name", SNELL)
def test_oracle_hits_the_snell_target(name):
    case = SR.CASE[name]
    sc = SR.snell_target(case)
    o = _oracle(sc)
    names = [f"{wl:.2f} nm, {th:.3f} deg" for wl, th in SR.snell_groups(case)]
    pos, dr, grp = SR.snell_rays(sc, case, COPIES)
    p, value = SR.snell_expected(sc, case, pos, dr)
    out = np.zeros((pos.shape[0], 4), np.float32)
    o.path_trace_from_input_rays_block(pos, dr, out, PASSES, 4)
    SR.check_two_valued(out[:, :SR.channels(case)], 1.0 - p, value, grp, names, PASSES, SR.EPS, name + ", on target")
    for shift in (3 * SR.STRIP_W, -3 * SR.STRIP_W):
        pos, dr, grp = SR.snell_rays(sc, case, COPIES, shift)
        out = np.zeros((pos.shape[0], 4), np.float32)
        o.path_trace_from_input_rays_block(pos, dr, out, PASSES, 4)
        assert not out.any(), f"{name}: {int(out.any(1).sum())} rays {shift / SR.STRIP_W:+.0f} w beside the target are lit"


@pytest.mark.parametrize("name", SR.PINHOLE_CASES)
@pytest.mark.parametrize("naive", [False, True], ids=["path_trace", "naive"])
def test_oracle_holds_the_pinhole_frame(name, naive):
    case = SR.CASE[name]
    sc = SR.goniometer(case, SR.WIDTH, SR.HEIGHT, depth=SR.pinhole_depth(naive), pinhole=True)
    img = _oracle(sc, S.INTEGRATOR_STUPID_PT if naive else S.INTEGRATOR_MIS_PT).render(4, naive=naive)
    SR.check_pinhole_frame(img, name, 4, f"{name}, {'NaivePathTrace' if naive else 'PathTrace'} on the oracle")

"""The two furnaces of tests/furnace_reference.py on the oracle, and the module's own checks: the conditions the GPU tests rest on (EPS, the cap,
the depth gaps) are pinned here before any device kernel sees the scenes. Figures: profiles/furnace.md."""
import numpy as np
import pytest

import furnace_reference as FR
from hydracore3_amd import scene as S

PASSES = 4
SEEDS = 8


def _oracle(sc, integrator=S.INTEGRATOR_MIS_PT):
    from oracle.orc import OracleIntegrator
    return OracleIntegrator(sc, sc.params(integrator=integrator))


@pytest.fixture(scope="module")
def sphere_runs():
    """{(integrator, depth): (pixel means, lo, hi)} of 4 passes of S on the oracle, rendered once."""
    runs = {}
    for integ in (S.INTEGRATOR_MIS_PT, S.INTEGRATOR_SHADOW_PT):
        for d in FR.DEPTHS:
            sc = FR.sphere_scene(d)
            mean = _oracle(sc, integ).render(PASSES)[..., :3].astype(np.float64) / PASSES
            mean.setflags(write=False)
            runs[(integ, d)] = (mean, *FR.sphere_interval(sc))
    return runs


@pytest.fixture(scope="module")
def cavity_runs():
    """{naive: [8 one-pass frames]} of C on the oracle, each from the generators the one before left."""
    runs = {}
    for naive in (False, True):
        sc = FR.cavity_scene()
        o = _oracle(sc, S.INTEGRATOR_STUPID_PT if naive else S.INTEGRATOR_MIS_PT)
        frames = []
        for _ in range(SEEDS):
            img = np.zeros((sc.height, sc.width, 4), np.float32)
            o.path_trace_block(img, 1, naive=naive)
            img.setflags(write=False)
            frames.append(img)
        runs[naive] = frames
    return runs


@pytest.mark.parametrize("integ", [S.INTEGRATOR_MIS_PT, S.INTEGRATOR_SHADOW_PT], ids=["mis", "shadow"])
@pytest.mark.parametrize("depth", FR.DEPTHS)
def test_oracle_holds_the_sphere(sphere_runs, integ, depth):
    mean, lo, hi = sphere_runs[(integ, depth)]
    out = FR.outside_interval(mean, lo, hi)
    print(f"S depth {depth} integrator {integ}: {int(out.sum())} of {out.size} pixels outside [{lo}, {hi}]")
    assert out.sum() <= FR.CAP_ORACLE * out.size * PASSES               # a pixel outside holds at least one sample outside
    assert not out.all() and mean.min() > 0


def test_oracle_naive_sphere_is_black():
    sc = FR.sphere_scene(3)
    img = _oracle(sc, S.INTEGRATOR_STUPID_PT).render(2, naive=True)
    assert not img.any()


@pytest.mark.parametrize("naive", [False, True], ids=["path_trace", "naive"])
def test_oracle_holds_the_cavity(cavity_runs, naive):
    kmax = FR.k_max(naive=naive)
    seen = set()
    for i, img in enumerate(cavity_runs[naive]):
        k, ok = FR.classify_frame(img, kmax)
        bad = np.argwhere(~ok)
        assert bad.shape[0] <= FR.CAP_ORACLE * ok.size, f"frame {i}: {bad.shape[0]} samples are no env * rho^k, first {bad[:3]}: {img[~ok][:3]}"
        seen |= set(np.unique(k).tolist())
        assert not img[..., 3].any()
    assert seen == set(range(-1, kmax + 1)), seen                        # dark pixels, primary misses and every power up to k_max occur


def test_eps_is_four_times_the_oracles_worst_excursion(sphere_runs, cavity_runs):
    """The measurement behind FR.EPS. S: the excursion of the pixel means that leave the interval by less than 1e-3 (the others are leaks, which the
    cap counts); C: the distance of every lit sample from its exact power."""
    s_worst = 0.0
    for mean, lo, hi in sphere_runs.values():
        e = FR.interval_excursion(mean, lo, hi)
        e = e[e < 1e-3]
        s_worst = max(s_worst, float(e.max()))
    c_worst = max(FR.power_excursion(img, FR.k_max(naive=naive)) for naive, frames in cavity_runs.items() for img in frames)
    print(f"worst excursion: S {s_worst:.3e}, C {c_worst:.3e}; EPS {FR.EPS:.3e}")
    assert 4.0 * max(s_worst, c_worst) <= FR.EPS < 1e-4
    assert FR.EPS <= 8.0 * max(s_worst, c_worst)                         # ... and the constant is not left wider than its measurement by a later edit


def test_interval_shrinks_with_the_subdivision():
    widths = []
    for subdiv in (2, 3, 4, 5):
        sc = FR.sphere_scene(3, subdiv=subdiv)
        r_in, r_out = FR.sphere_radii(sc)
        assert abs(r_out - FR.RADIUS) < 1e-6 and r_in < r_out
        lo, hi = FR.sphere_interval(sc)
        widths.append(float(((hi - lo) / lo).max()))
    assert all(a > 3.5 * b for a, b in zip(widths, widths[1:])), widths   # the sagitta goes with the edge length squared
    assert widths[-1] < 1e-3


def test_r_in_is_a_distance_to_the_triangles_not_to_the_vertices():
    sc = FR.sphere_scene(1, subdiv=1)
    v = sc.vpos[:, :3].astype(np.float64)
    tri = sc.tri_indices.reshape(-1, 3)
    r = np.random.RandomState(3)
    b = r.dirichlet((1, 1, 1), (200, tri.shape[0]))
    pts = np.einsum("stk,tkc->stc", b, v[tri])
    r_in, _ = FR.sphere_radii(sc)
    d = np.linalg.norm(pts, axis=-1)
    assert r_in <= d.min() and d.min() - r_in < 0.02 * FR.RADIUS


def test_depths_stand_clear_of_each_other():
    sc = FR.sphere_scene(1)
    for d in FR.DEPTHS:
        lo, hi = FR.sphere_interval(sc, d)
        lo2, hi2 = FR.sphere_interval(sc, d + 1)
        assert np.any(lo2 - hi > 4 * (hi2 - lo2)), d
        assert np.any((lo2 - hi) / hi > 0.015), d                         # an off-by-one moves a channel by 1.5 % or more


def test_classify_rejects_what_no_sample_can_be():
    kmax = FR.k_max()
    for k in range(kmax + 1):
        v = FR.cavity_value(k)
        assert FR.classify(v, kmax) == k
        assert FR.classify(v.astype(np.float32), kmax) == k
        assert FR.classify(v[[0, 2, 1]], kmax) is None                   # green and blue swapped
        assert FR.classify(v[[1, 0, 2]], kmax) is None
        assert FR.classify(v * (1 + 3 * FR.EPS), kmax) is None
        assert FR.classify(v * np.array([1.0, 1.0, 1 + 3 * FR.EPS]), kmax) is None
    assert FR.classify(FR.cavity_value(kmax + 1), kmax) is None
    assert FR.classify(FR.cavity_value(kmax + 1), FR.k_max(naive=True)) == kmax + 1
    assert FR.classify(np.zeros(3), kmax) == FR.DARK
    assert FR.classify(np.array([0.0, 0.0, 1e-9]), kmax) is None
    assert FR.classify(np.array([np.nan, 1.0, 1.0]), kmax) is None and FR.classify(np.array([1.0, np.inf, 1.0]), kmax) is None
    assert FR.classify(-FR.cavity_value(1), kmax) is None
    two = FR.cavity_value(1) + FR.cavity_value(2)                        # a doubled sample is no power either
    assert FR.classify(two, kmax) is None


def test_one_channel_classifier_rejects_what_no_sample_can_be():
    kmax = FR.k_max()
    red = np.array([FR.cavity_value(k)[0] for k in range(kmax + 2)])
    k, ok = FR.classify_red_frame(red.astype(np.float32), kmax)
    assert np.array_equal(k, np.arange(kmax + 2)) and ok[:kmax + 1].all() and not ok[kmax + 1]
    assert FR.classify_red_frame(red, FR.k_max(naive=True))[1].all()
    bad = np.array([red[1] * (1 + 3 * FR.EPS), red[2] * (1 - 3 * FR.EPS), -red[1], np.nan, np.inf, red[1] + red[2], 1e-9])
    assert not FR.classify_red_frame(bad, kmax)[1].any()
    k, ok = FR.classify_red_frame(np.zeros(3), kmax)
    assert ok.all() and (k == FR.DARK).all()


def test_input_rays_start_inside_the_sphere():
    pos, dr = FR.sphere_input_rays(300)
    wv = S.look_at(FR.S_CAM_POS, FR.S_CAM_LOOK_AT, FR.S_CAM_UP)
    world = (pos[:, :3].astype(np.float64) - wv[:3, 3]) @ wv[:3, :3]
    assert np.linalg.norm(world, axis=1).max() < 0.61 * FR.RADIUS
    assert np.allclose(np.linalg.norm(dr[:, :3], axis=1), 1.0, atol=1e-6)

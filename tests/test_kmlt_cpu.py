"""IntegratorKMLT's host side without a GPU: the generator restatement against the oracle's, the vector layout's size, MutateKelemen's
properties and the chain bookkeeping of tests/kmlt_reference.py on steps computed by hand."""
import numpy as np
import pytest

import kmlt_reference as K

F32 = np.float32


@pytest.mark.parametrize("seed", [0, 1, 7, 12345])
def test_generator_restatement_equals_the_oracle(seed):
    from oracle.orc import rng_kat
    st, vals = rng_kat(seed, 8)
    g = K.Gens.init([seed])
    assert [int(g.sx[0]), int(g.sy[0])] == [int(st[0]), int(st[1])]
    mine = np.stack([g.float4()[0] for _ in range(8)])
    assert mine.view(np.uint32).tolist() == vals.view(np.uint32).tolist()
    assert [int(g.sx[0]), int(g.sy[0])] == [int(st[2]), int(st[3])]
    # rndFloat1 is the first component's polynomial of the same state step
    a, b = K.Gens.init([seed]), K.Gens.init([seed])
    assert a.float1()[0] == b.float4()[0, 0] and np.array_equal(a.states(), b.states())
    # a masked draw leaves the other generators where they were
    two = K.Gens.init([seed, seed])
    two.float4(np.array([True, False]))
    assert np.array_equal(two.states()[1], K.Gens.init([seed]).states()[0]) and not np.array_equal(two.states()[0], two.states()[1])


def test_state_size_equals_the_restatement():
    from hydracore3_amd import api
    depths = list(range(1, 9)) + [32]
    got = [api.kmlt_state_size(d) for d in depths]
    assert got == [K.state_size(d) for d in depths]
    assert got == [16, 32, 48, 48, 64, 80, 80, 96, 336]
    assert all(g % 16 == 0 and g >= 10 * d + 6 and g - (10 * d + 6) < 16 for g, d in zip(got, depths))


@pytest.mark.parametrize("p2", [K.MUTATE_COEFF_SCREEN, K.MUTATE_COEFF_BSDF])
def test_mutate_kelemen_properties(p2):
    rng = np.random.default_rng(5)
    n = 20000
    v = rng.random(n, dtype=np.float32)
    rx, ry = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    out = K.mutate_kelemen(v, rx, ry, p2)
    assert out.dtype == F32 and np.all((out >= 0.0) & (out <= 1.0))
    step = K.circular_distance(out, v)
    assert np.all(step <= 1.0 / p2 + 2.0 ** -24)                        # the step is at most 1 / p2 (one rounding of the sum)
    assert np.all(step[rx < 0.5] >= step.min()) and step.max() > 0.5 / p2 * 0.5
    # rands.x = 1: exp(power) - exp(power) = 0
    assert np.array_equal(K.mutate_kelemen(v, np.ones(n, F32), ry, p2), v)
    # wrap-around at both ends: a step up from just under 1 lands just above 0 and the reverse
    big = F32(0.0)                                                      # rands.x = 0 gives the largest step, (1 - p2 / 1024) / p2
    dv = float(K.circular_distance(K.mutate_kelemen(F32(0.5), big, F32(0.25), p2), 0.5))
    assert abs(dv - (1.0 - p2 / 1024.0) / p2) < 1e-6
    hi = K.mutate_kelemen(F32(1.0 - dv / 4), big, F32(0.25), p2)
    lo = K.mutate_kelemen(F32(dv / 4), big, F32(0.75), p2)
    assert abs(float(hi) - 0.75 * dv) < 1e-6 and abs(float(lo) - (1.0 - 0.75 * dv)) < 1e-6


def test_chain_seeding_and_proposals():
    g1, g2 = K.chain_gens(20)
    for c in (0, 1, 16, 17, 19):
        a, b = K.Gens.init([7 * c + 1]), K.Gens.init([c])
        for _ in range(10 + c % 17):
            a.next_state()
            b.next_state()
        assert np.array_equal(g1.states()[c], a.states()[0]) and np.array_equal(g2.states()[c], b.states()[0])
    # a large step is n / 4 float4 draws of gen2 in slot order; a small one takes n / 2 states and moves every slot by at most 1 / p2
    n = 16
    x = np.full((2, n), 0.5, F32)
    g = K.Gens.init([3, 3])
    new = K.propose(x, np.array([True, False]), g)
    ref = K.Gens.init([3])
    assert np.array_equal(new[0], np.concatenate([ref.float4()[0] for _ in range(n // 4)])) and np.array_equal(g.states()[0], ref.states()[0])
    ref = K.Gens.init([3])
    for _ in range(n // 2):
        ref.next_state()
    assert np.array_equal(g.states()[1], ref.states()[0])
    d = K.circular_distance(new[1], 0.5)
    assert np.all(d[:2] <= 1.0 / 128 + 1e-7) and np.all(d[2:] <= 1.0 / 64 + 1e-7) and np.all(d > 0)


def test_chain_bookkeeping_on_hand_computed_steps():
    """One chain, three steps, F prescribed per step: black -> bright (yOld == 0: a = 1, nothing is added at the old state), bright -> a quarter
    as bright with a below the chain's draw (a reject: both states get their share), then bright again (a = 1)."""
    w, h, n = 4, 2, 16
    g1, _ = K.chain_gens(1)
    draws = [float(g1.float1()[0]) for _ in range(6)]                   # per step: the large-step draw, then the acceptance draw
    p2 = draws[3]
    assert p2 > 0.3                                                     # (a = 0.25 below is then a reject)
    bright, dim = (3.0, 1.5, 1.5), (0.75, 0.375, 0.375)
    rec = {"initColor": np.zeros((1, 4), F32), "initPixel": np.array([5]),
           "color": np.array([[bright + (0,), dim + (0,), bright + (0,)]], F32), "pixel": np.array([[1, 2, 3]])}
    r = K.run_chains(1, 3, n, (w, h), recorded=rec)
    assert r["isLarge"][0].tolist() == [draws[0] < 0.25, draws[2] < 0.25, draws[4] < 0.25]
    yb = F32(0.333334) * F32(6.0)
    yd = F32(0.333334) * F32(1.5)
    assert r["a"][0].tolist() == [1.0, float(F32(yd / yb)), 1.0] and abs(r["a"][0, 1] - 0.25) < 1e-6
    assert r["accepted"][0].tolist() == [True, False, True]
    assert r["oldPixel"][0].tolist() == [5, 1, 1]                       # the rejected proposal leaves the chain at pixel 1
    # step 0: the old state is black, its contribution (0) fails the 1e-12 test; the new state gets colour / y
    assert not r["addX"][0, 0] and r["addY"][0, 0]
    ky, kd = F32(1.0) / yb, F32(1.0) / yd
    assert np.array_equal(r["contribAtY"][0, 0], np.asarray(bright, F32) * ky * F32(1.0))
    # step 1: a at the proposal, 1 - a at the state that stays
    a1 = r["a"][0, 1]
    assert np.array_equal(r["contribAtY"][0, 1], (np.asarray(dim, F32) * kd).astype(F32) * a1)
    assert np.array_equal(r["contribAtX"][0, 1], (np.asarray(bright, F32) * ky).astype(F32) * (F32(1.0) - a1))
    # step 2: a = 1 again, 1 - a = 0 at the old state
    assert not r["addX"][0, 2] and r["addY"][0, 2]
    frame = np.zeros((w * h, 3))
    frame[1] = r["contribAtY"][0, 0].astype(np.float64) + r["contribAtX"][0, 1]
    frame[2] = r["contribAtY"][0, 1]
    frame[3] = r["contribAtY"][0, 2]
    assert np.array_equal(r["frame"], frame) and r["count"].tolist() == [0, 2, 1, 1, 0, 0, 0, 0]
    assert r["accept"][0] == 2
    want_large = sum(y for y, l in zip((float(yb), float(yd), float(yb)), r["isLarge"][0]) if l)
    assert r["largeSteps"][0] == int(np.sum(r["isLarge"][0])) and r["accumBrightness"][0] == want_large
    # the proposals: the initial vector is n rndFloat1 draws of gen2, proposals stay in [0, 1]
    _, g2 = K.chain_gens(1)
    assert np.array_equal(r["init"][0], np.array([g2.float1()[0] for _ in range(n)], F32))
    assert np.all((r["proposals"] >= 0.0) & (r["proposals"] <= 1.0))


def test_normalisation_restatement():
    frame = np.zeros((2, 2, 4), F32)
    frame[0, 0, :3] = (3.0, 1.5, 1.5)
    frame[1, 1, :3] = (0.75, 0.375, 0.375)
    s = K.normalisation(np.array([4.0, 0.0, 3.0]), np.array([2, 0, 3]), np.array([3, 1, 2]), frame, 4, 2)
    actual = (float(F32(0.333334) * F32(6.0)) + float(F32(0.333334) * F32(1.5))) / 4
    assert s[0] == 1.5 and s[1] == actual and s[2] == 6 / 8 and s[3] == float(F32(2) * F32(1.5 / actual))
    assert K.normalisation(np.array([0.0]), np.array([0]), np.array([0]), frame, 4, 2)[3] == 1.0
    assert K.normalisation(np.array([1.0]), np.array([1]), np.array([0]), np.zeros_like(frame), 4, 2)[3] == 1.0

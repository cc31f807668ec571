"""Treelet restructuring of device-built trees: hpt_set_option("device_build_quality", passes) runs passes of the Karras-Aila treelet optimiser
(hpt_lbvh.hip: lbvhTreeletKernel) over the linear BVH before it is emitted. Hits never depend on the tree, so queries and frames must stay bit
for bit what every other tree gives; the tree itself is read back (read_accel) and held to the float64 reader (tests/accel_reference.py) and to
the numpy restatement of the optimiser (tests/treelet_reference.py); build_info says what the passes did."""
import re

import numpy as np
import pytest

import accel_reference as AR
import treelet_reference as TR
from test_device_refit_gpu import SAH_REL, _apply, _check_boxes, _move_four, _scene, _tables, _tiny, random_rays
from traversal_scenes import assert_hits_equal, make_rays, nested_sheets, reference_hits, sweep_scene, with_tfar, world_triangles

NO_INFO = {"passes": 0, "examined": 0, "rewritten": 0, "ms": 0.0}


def _build(sc, passes, layout=0, refit=0, **opts):
    """A context whose single-level tree was built on the device with the given number of treelet passes."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, accel_layout=layout)
    g.set_option("device_build", 1); g.set_option("device_refit", refit); g.set_option("device_build_quality", passes)
    for k, v in opts.items():
        g.set_option(k, v)
    g.CommitScene(1)
    assert g.commit_time()["device_built"] and g.accel_info()["layout"] == "flat"
    return g


def _reachable_bytes(g):
    """(ids of the nodes the root reaches in walk order, their records' bytes, the records' bytes of the triangles, root)."""
    nodes, tris, root = g.read_accel()
    order = AR.reachable(nodes, root)
    return order, nodes[np.asarray(order, np.int64)].tobytes(), tris.tobytes(), root


def _cluster_scene(positions, length=10.0, w=6.0, eps=1e-3):
    """Clusters of two nearly coincident triangles (the second 1e-3 further along x) in planes x = p * length: equal centroids in y and z, so the
    Morton order is the order along x, the two triangles of a cluster are neighbours in it and the Karras tree folds each cluster into one leaf."""
    v, idx = [], []
    for p in positions:
        for x in (p * length, p * length + eps):
            idx.append([len(v), len(v) + 1, len(v) + 2])
            v += [[x, -w / 2, -w / 2], [x, w / 2, -w / 2], [x, 0.0, w / 2]]
    return _tiny([((np.array(v, float), np.array(idx)), [np.eye(4)])])


# ---- 1. one full treelet with a known optimum -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seven_clusters_reach_the_enumerated_optimum():
    """Seven clusters along a line, two of them astride the top Morton cell boundary (0.49 | 0.51): the Morton tree separates them at the root
    and pays for it; one pass over the root's treelet, which holds all seven leaves, must leave the optimal topology."""
    # (spacings chosen unequal: with 0.30 / 0.70 / 0.85 three topologies tie at the optimum, 0.15 = 0.15 and 0.30 + 0.21 = 0.51)
    sc = _cluster_scene([0.0, 0.27, 0.49, 0.51, 0.68, 0.86, 1.0])
    plain = _build(sc, 0, layout=2)
    nodes, tris, root = plain.read_accel()
    boxes = TR.tree_leaf_boxes(nodes, root, AR)
    assert len(AR.reachable(nodes, root)) == 6 and boxes.shape[0] == 7 and tris.shape[0] == 14
    assert plain.build_info() == NO_INFO
    area, cost, _ = TR.optimize(boxes)
    opt = float(cost[127])
    was = TR.tree_half_area_sum(nodes, root, AR)
    print(f"seven clusters: Morton tree {was:.3f}, enumerated optimum {opt:.3f} ({was / opt - 1:+.1%})")
    assert was > 1.05 * opt, "the scene must leave the optimiser more than 5 % to gain"
    costs = np.unique(TR.enumerated_costs(area, 7))
    assert costs[0] == cost[127] and (float(costs[1]) - opt) / opt > 1e-3, "the optimum must stand clear of the runner-up by far more than the 1e-4 it is held to"
    q = _build(sc, 1, layout=2)
    nodes, tris, root = _check_boxes(q, sc, "seven clusters, one pass")
    assert len(AR.reachable(nodes, root)) == 6
    got = TR.tree_half_area_sum(nodes, root, AR)
    # the read-back boxes are padded by 1e-5 relative (padBox), the leaves' before the union and the nodes' after it: 1e-4 covers both
    print(f"seven clusters: after one pass {got:.3f} (rel {abs(got - opt) / opt:.2e}), {q.build_info()}")
    assert abs(got - opt) <= 1e-4 * opt
    info = q.build_info()
    assert info["passes"] == 1 and info["rewritten"] == 1 and info["examined"] >= 1 and info["ms"] > 0.0
    assert q.accel_info()["sah_node_visits"] < plain.accel_info()["sah_node_visits"]


# ---- 2. a treelet with an inner subtree among its leaves ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eight_clusters_stay_sound_and_get_cheaper():
    sc = _cluster_scene([0.0, 0.12, 0.27, 0.49, 0.51, 0.68, 0.86, 1.0])
    plain = _build(sc, 0, layout=2)
    pn, _, pr = plain.read_accel()
    assert len(AR.reachable(pn, pr)) == 7 and TR.tree_leaf_boxes(pn, pr, AR).shape[0] == 8
    q = _build(sc, 1, layout=2)
    nodes, tris, root = _check_boxes(q, sc, "eight clusters")                # every record reached exactly once, every box contains what lies below it
    assert len(AR.reachable(nodes, root)) == 7 and tris.shape[0] == 16
    a, b = TR.tree_half_area_sum(nodes, root, AR), TR.tree_half_area_sum(pn, pr, AR)
    print(f"eight clusters: {b:.3f} -> {a:.3f}, {q.build_info()}")
    assert a < b * (1.0 - 1e-3) and q.accel_info()["sah_node_visits"] < plain.accel_info()["sah_node_visits"]
    assert q.build_info()["rewritten"] >= 1


# ---- 3. soundness at size -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_cost():
    return {kind: AR.sah_estimate(*_build(_scene(kind), 0).read_accel()[::2]) for kind in ("small", "17K")}


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("kind", ["small", "17K"])
def test_restructured_trees_are_sound_and_cheaper(kind, passes, plain_cost, monkeypatch, capfd):
    sc = _scene(kind)
    monkeypatch.setenv("HPT_DEBUG_ACCEL", "1")
    capfd.readouterr()
    q = _build(sc, passes)
    log = capfd.readouterr().err
    m = re.findall(r"device-built single-level BVH: \d+ triangles, depth (\d+),.*treelet passes (\d+) \((\d+) of (\d+) treelets rewritten", log)
    assert m, log
    depth, ran, rewritten, examined = (int(x) for x in m[-1])
    nodes, tris, root = _check_boxes(q, sc, f"{kind}, {passes} passes")      # record_counts == 1 everywhere, no containment violation in float64
    info = q.build_info()
    assert (info["passes"], info["rewritten"], info["examined"]) == (ran, rewritten, examined) and ran == passes
    assert info["rewritten"] > 0 and info["examined"] >= info["rewritten"]
    assert AR.height(nodes, root) + 1 <= depth + 1                            # (depth + 1: the stack the context sizes for this tree)
    want = AR.sah_estimate(nodes, root)
    got = q.accel_info()["sah_node_visits"]
    print(f"{kind}, {passes} passes: estimate {plain_cost[kind]:.4f} -> {want:.4f} (reported {got:.4f}, rel {abs(got - want) / want:.2e}), depth {depth}, {info}")
    assert want < plain_cost[kind]
    # SAH_REL covers the division and a float64 sum. Two things it does not cover, both of the plain device build too (which no test held to the reader):
    # (1) the build sums its float terms in float: six additions in each wave's reduction, then one float atomic per wave of the emitter's grid (a
    #     lane per triangle), every addition of positive terms within 2^-24 relative;
    # (2) the build divides by the half-area of the root's UNPADDED box, the reader by that of the union of the two padded boxes stored in the root.
    #     padBox moves every face out by p = 1e-5 * max(longest extent, largest |coordinate|) + 1e-30, taken here from the padded box (no smaller), so
    #     the padded half-area exceeds the unpadded by 4 p (dx + dy + dz) - 12 p^2 <= 4 p (dx + dy + dz) with the padded extents: (estimate - 1) moves
    #     by at most that share of it
    r = nodes["q"][int(root)].astype(np.float64)
    lo, hi = np.minimum(r[0:6:2], r[6:12:2]), np.maximum(r[1:6:2], r[7:12:2])
    d = hi - lo
    a0 = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    grow = 4.0 * (1e-5 * max(d.max(), np.abs(lo).max(), np.abs(hi).max()) + 1e-30) * d.sum()
    adds = 6 + tris.shape[0] // 64 + 1
    assert abs(got - want) <= (SAH_REL + adds * 2.0 ** -24) * want + (want - 1.0) * grow / (a0 - grow)
    again = _build(sc, passes)
    assert _reachable_bytes(again) == _reachable_bytes(q)
    assert again.build_info()["rewritten"] == info["rewritten"]


# ---- 4. hits and frames unchanged -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ray_queries_equal_brute_force_bit_for_bit():
    from oracle.orc import OracleIntegrator
    sc = sweep_scene(12)
    cpu = OracleIntegrator(sc)
    tris, ids = world_triangles(sc)
    pos, dr, _ = make_rays(tris, 12000, 19)
    h = cpu.ray_nearest(pos, dr, brute=True)
    dr = with_tfar(pos, dr, np.where(h["instId"] != 0xFFFFFFFF, h["t"], np.inf), 20)
    hb, ab = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=True)
    hit, _, inst, prim, robust = reference_hits(tris, ids, sc.inst_matrices, pos, dr)
    for passes in (1, 3):
        for wide in (1, 0):
            g = _build(sc, passes, layout=2, wide_nodes=wide)
            got = g.RayQuery_NearestHit(pos, dr)
            assert_hits_equal(got, hb, f"quality {passes}, wide_nodes {wide}")
            assert np.array_equal(g.RayQuery_AnyHit(pos, dr), ab)
            r = np.flatnonzero(robust & hit)
            assert r.size > 50 and np.array_equal(got["instId"][r].astype(np.int64), inst[r]) and np.array_equal(got["primId"][r].astype(np.int64), prim[r])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,schedule", [("small", 1), ("17K", 2)])
def test_frames_equal_the_host_built_trees(kind, schedule):
    from hydracore3_amd.api import HipIntegrator
    sc = _scene(kind)
    host = HipIntegrator(sc)
    assert not host.commit_time()["device_built"] and host.build_info() == NO_INFO
    q = _build(sc, 2)
    assert q.build_info()["rewritten"] > 0
    for g in (host, q):
        g.set_schedule(schedule)
    assert np.array_equal(q.render(3), host.render(3))
    assert np.array_equal(q.random_gens(), host.random_gens())
    assert q.last_schedule()[0] == schedule
    if kind == "17K":
        assert q.last_launch()["wide_nodes"]                                  # the 4-wide collapse of the restructured tree was walked


# ---- 5. refit composes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refit_of_a_restructured_tree():
    from hydracore3_amd.api import HipIntegrator
    sc, moved = _scene("small"), _scene("small")
    g = _build(sc, 2, refit=1)
    assert g.build_info()["rewritten"] > 0 and g.refit_info()["levels"] > 0
    _apply(g, _move_four(moved))
    assert g.commit_time()["refitted"] and not g.commit_time()["device_built"]
    assert g.build_info() == NO_INFO                                          # (a refit is no build)
    nodes, _, root = _check_boxes(g, moved, "refit of a restructured tree")
    want = AR.sah_estimate(nodes, root)
    assert abs(g.refit_info()["after"] - want) <= SAH_REL * want
    assert g.refit_info()["levels"] == AR.height(nodes, root) + 1
    _tables(g, moved)
    fresh = HipIntegrator(moved)
    pos, dr = random_rays(20000, 31)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert (hf["geomId"] != 0xFFFFFFFF).mean() > 0.5
    assert np.array_equal(g.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    dr2 = dr.copy(); dr2[:, 3] = np.random.default_rng(6).uniform(0.3, 9.0, dr.shape[0]).astype(np.float32)
    assert np.array_equal(g.RayQuery_AnyHit(pos, dr2), fresh.RayQuery_AnyHit(pos, dr2))
    # the rebuild of a device-built tree on update without device_refit runs the passes too
    again = _build(sc, 2)
    _apply(again, _move_four(_scene("small")))
    assert again.commit_time()["device_built"] and again.build_info()["passes"] == 2 and again.build_info()["rewritten"] > 0
    assert np.array_equal(again.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_trees_with_nothing_to_restructure():
    """1, 2 and 3 triangles: no treelet of three leaves; 64 coincident triangles: every half-area is 0, nothing is strictly lower. The trees are
    the plain build's byte for byte and build_info says what happened."""
    from hydracore3_amd import scene as S
    tri = lambda x: [[x, 0.0, 0.0], [x + 1.0, 0.0, 0.2], [x, 1.0, 0.1]]
    for count in (1, 2, 3):
        mesh = (np.array(sum((tri(3.0 * k - 3.0) for k in range(count)), [])), np.arange(3 * count).reshape(count, 3))
        sc = _tiny([(mesh, [np.eye(4)])])
        plain, q = _build(sc, 0, layout=2), _build(sc, 3, layout=2)
        assert _reachable_bytes(q) == _reachable_bytes(plain)
        assert q.build_info() == NO_INFO, count                               # (three triangles: one node over two leaves, so no pass runs)
    one = (np.array(tri(0.0)), np.arange(3).reshape(1, 3))
    sc = _tiny([(one, [S.translate(0.3, 0.2, 0.1)] * 64)])
    plain, q = _build(sc, 0, layout=2), _build(sc, 2, layout=2)
    assert _reachable_bytes(q) == _reachable_bytes(plain)
    info = q.build_info()
    assert info["passes"] == 2 and info["rewritten"] == 0 and info["examined"] == 2 * 15    # 31 nodes, the 16 lowest over leaves only
    _check_boxes(q, sc, "64 coincident triangles")


@pytest.mark.gpu
def test_deep_tree_is_restructured_or_handed_to_the_host():
    """nested_sheets x 8 (a Karras tree some 40 levels deep): either the restructured tree is sound and the frame bit-identical to the host-built
    tree's, or the build declined (deeper than the traversal stack) and the host's tree took over cleanly. The test prints which."""
    from hydracore3_amd.api import HipIntegrator
    sc = nested_sheets(4000, 1.003, instances=8)
    g = HipIntegrator(sc, accel_layout=2)
    g.set_option("device_build", 1); g.set_option("device_build_quality", 2); g.CommitScene(1)
    host = HipIntegrator(sc, accel_layout=2)
    if g.commit_time()["device_built"]:
        nodes, _, root = _check_boxes(g, sc, "nested sheets x 8, two passes")
        print(f"nested sheets x 8: restructured on the device, height {AR.height(nodes, root)}, {g.build_info()}")
        assert g.build_info()["passes"] in (0, 1, 2)
    else:
        print("nested sheets x 8: the device build declined; host-built tree")
        assert g.build_info() == NO_INFO
    assert np.array_equal(g.render(2), host.render(2)) and np.array_equal(g.random_gens(), host.random_gens())


# ---- 7. option 0 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quality_back_to_zero_gives_the_plain_tree():
    from hydracore3_amd.api import HydraHipError
    sc = _scene("small")
    g = _build(sc, 2)
    assert g.build_info()["rewritten"] > 0
    restructured = _reachable_bytes(g)
    g.set_option("device_build_quality", 0); g.CommitScene(1)
    assert g.commit_time()["device_built"] and g.build_info() == NO_INFO
    plain = _reachable_bytes(_build(sc, 0))
    assert _reachable_bytes(g) == plain and restructured != plain
    for bad in (5, 100):
        with pytest.raises(HydraHipError):
            g.set_option("device_build_quality", bad)
    g.set_option("device_build_quality", 4)

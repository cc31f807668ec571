"""Dynamic scenes on the device path: a tree built by hpt_lbvh.hip is refitted (hpt_set_option("device_refit", 1)) after UpdateInstance /
UpdateGeom_Triangles3f instead of being built again. Hits never depend on the boxes as long as the boxes contain their triangles, so the refitted
tree must answer ray queries and render frames bit for bit like a context built from scratch for the moved scene; the boxes themselves are read
back (read_accel) and checked in float64 (tests/accel_reference.py); the refitted tree's cost (refit_info) is held to the same reader's value;
"refit_max_sah_pct" turns a refit that degraded the tree into a build."""
import os

import numpy as np
import pytest

import accel_reference as AR
from traversal_scenes import _add, _base_scene, assert_hits_equal, make_rays, nested_rays, nested_sheets, with_tfar, world_triangles

# one float rounding each for the root area, the division and the result (3 x 2^-24 = 1.8e-7), per term at most 3 x 2^-24 from the float products
# and sums - the terms are positive, so their sum carries no more - and nothing from the double sum at these sizes: below 4e-7, held to 1e-6
SAH_REL = 1e-6


def random_rays(n, seed, lo=-5.0, hi=5.0):
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dr = np.zeros((n, 4), np.float32)
    dr[:, :3] = d
    dr[:, 3] = np.float32(3.402823466e+38)
    return pos, dr


def _scene(kind):
    from hydracore3_amd import synth
    if kind == "small":
        return synth.interior_scene(96, 64, objects=14, subdiv=2, tex_size=16)        # 5 K triangles in 16 instances
    return synth.interior_scene(160, 96, subdiv=1, tex_size=16)                        # 17 K triangles in 206 instances: the 4-wide tree is walked


def _device(sc, refit=1, layout=0, **opts):
    """A context whose single-level tree was built on the device, with device_refit as given."""
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, accel_layout=layout)
    g.set_option("device_build", 1); g.set_option("device_refit", refit)
    for k, v in opts.items():
        g.set_option(k, v)
    g.CommitScene(1)
    assert g.commit_time()["device_built"] and g.accel_info()["layout"] == "flat"
    return g


def _tables(g, moved):
    d = moved.desc(); d.vPos4f = None                                      # tables only: the normal matrices follow the instance matrices
    g._desc = d; g.scene = moved
    g.CommitDeviceData()
    g.InitRandomGens(g.N)


def _move_four(moved, seed=3):
    """Four instances move, turn and stretch; returns {instance: matrix}."""
    from hydracore3_amd import scene as S
    rng = np.random.default_rng(seed)
    out = {}
    for i in (2, 5, 9, 15):
        m = S.translate(*rng.uniform(-0.6, 0.6, 3)) @ np.asarray(moved.inst_matrices[i]) @ S.rotate_y(float(rng.uniform(0, 90))) @ S.scale(1.0, float(rng.uniform(0.7, 1.5)), 1.0)
        moved.inst_matrices[i] = m
        out[i] = m
    return out


def _exchange_ends(moved):
    """The objects (instances 2 ..) exchange their translations with the object at the opposite end of the room's grid: the root's box stays,
    the inner boxes, which keep their members, grow."""
    n = len(moved.inst_matrices)
    out = {}
    for k in range((n - 2) // 2):
        a, b = 2 + k, n - 1 - k
        ma, mb = np.array(moved.inst_matrices[a], np.float64), np.array(moved.inst_matrices[b], np.float64)
        ta, tb = ma[:3, 3].copy(), mb[:3, 3].copy()
        ma[:3, 3], mb[:3, 3] = tb, ta
        moved.inst_matrices[a], moved.inst_matrices[b] = ma, mb
        out[a], out[b] = ma, mb
    return out


def _apply(g, matrices, options=1):
    for i, m in matrices.items():
        g.UpdateInstance(i, m)
    g.CommitScene(options)


def _check_boxes(g, moved, what):
    nodes, tris, root = g.read_accel()
    wt, ids = world_triangles(moved)
    assert tris.shape[0] == wt.shape[0] == g.accel_info()["inst_tris"]
    cnt = AR.record_counts(nodes, root, tris.shape[0])
    assert np.all(cnt == 1), f"{what}: {int((cnt != 1).sum())} records are not reached exactly once"
    bad = AR.containment_violations(nodes, root, AR.record_world_vertices(tris, wt, ids))
    assert not bad, f"{what}: {len(bad)} violations, first: {bad[:3]}"
    return nodes, tris, root


# ---- 1. the refit happens and is exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "17K"])
def test_update_instance_refits_the_device_built_tree(kind):
    """UpdateInstance + CommitScene(BUILD_LOW) on a device-built tree under device_refit = 1 is a refit, and the context then answers 20 000
    nearest-hit and any-hit queries and renders (schedules 1 and 2, generators included) bit for bit like a host-built context of the moved
    scene, with the 4-wide tree and without it; a second round refits the refitted tree."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd import scene as S
    sc, moved = _scene(kind), _scene(kind)
    dev, narrow = _device(sc), _device(sc, wide_nodes=0)
    assert dev.refit_info()["levels"] > 0 and not dev.commit_time()["refitted"]
    dev.render(1)
    ms = _move_four(moved)
    for g in (dev, narrow):
        _apply(g, ms)
        _tables(g, moved)
    assert dev.commit_time()["refitted"] and not dev.commit_time()["device_built"]         # (without the refit of device-built trees: device_built)
    assert narrow.commit_time()["refitted"]
    print("device refit:", dev.commit_time(), dev.refit_info())
    fresh = HipIntegrator(moved)
    assert not fresh.commit_time()["device_built"]
    pos, dr = random_rays(20000, 17)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert (hf["geomId"] != 0xFFFFFFFF).mean() > 0.5
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    assert np.array_equal(narrow.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    assert not np.array_equal(hf.view(np.uint8), HipIntegrator(sc).RayQuery_NearestHit(pos, dr).view(np.uint8))
    dr2 = dr.copy(); dr2[:, 3] = np.random.default_rng(5).uniform(0.3, 9.0, dr.shape[0]).astype(np.float32)
    af = fresh.RayQuery_AnyHit(pos, dr2)
    assert np.array_equal(dev.RayQuery_AnyHit(pos, dr2), af) and np.array_equal(narrow.RayQuery_AnyHit(pos, dr2), af)
    for sched, spp in ((1, 3), (2, 4)):
        for g in (dev, narrow, fresh):
            g.set_schedule(sched)
        a, b, c = dev.render(spp), fresh.render(spp), narrow.render(spp)
        assert np.array_equal(a, b) and np.array_equal(c, b), sched
        assert np.array_equal(dev.random_gens(), fresh.random_gens()) and np.array_equal(narrow.random_gens(), fresh.random_gens())
        assert dev.last_schedule()[0] == sched
        if kind == "17K":
            assert dev.last_launch()["wide_nodes"] and not narrow.last_launch()["wide_nodes"]     # the requantised 4-wide nodes were walked
    # a second round of updates refits the refitted tree again
    m = S.translate(0.2, 0.1, -0.3) @ np.asarray(moved.inst_matrices[7])
    moved.inst_matrices[7] = m
    _apply(dev, {7: m}); _tables(dev, moved)
    assert dev.commit_time()["refitted"]
    again = HipIntegrator(moved)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), again.RayQuery_NearestHit(pos, dr).view(np.uint8))
    dev.set_schedule(0)
    assert np.array_equal(dev.render(3), again.render(3))


# ---- 2. the boxes themselves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("builder,kind", [("device", "small"), ("device", "17K"), ("host", "small")])
def test_refitted_boxes_contain_what_lies_below_them(builder, kind):
    """After a build and after a refit, of a device-built and of a host-built tree: every child box contains the float64 world positions of
    every vertex below it, every inner child's box contains both boxes of the node it references, every record is reached exactly once."""
    from hydracore3_amd.api import HipIntegrator
    sc, moved = _scene(kind), _scene(kind)
    g = _device(sc) if builder == "device" else HipIntegrator(sc)
    _check_boxes(g, sc, f"{builder} build, {kind}")
    _apply(g, _move_four(moved))
    assert g.commit_time()["refitted"]
    nodes, _, root = _check_boxes(g, moved, f"{builder} refit, {kind}")
    assert g.refit_info()["levels"] == AR.height(nodes, root) + 1
    _apply(g, _exchange_ends(moved))                                         # large motions: boxes that grow a lot are boxes all the same
    assert g.commit_time()["refitted"]
    _check_boxes(g, moved, f"{builder} second refit, {kind}")


# ---- 3. moved vertices ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_geom_refits_the_device_built_tree():
    """UpdateGeom_Triangles3f with unchanged indices + CommitScene on a device-built tree: a refit; the triangle records equal, byte for byte and
    record by record (instId, primId), a fresh device build's of the modified scene (whose Morton order is its own); queries and the frame
    equal a fresh context's; a later device build finds the moved positions; changed indices make the next commit a build."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd import scene as S
    sc, moved = _scene("small"), _scene("small")
    dev = _device(sc)
    dev.render(1)
    geom = 4
    to, vo = moved.mat_vert_offset[geom]
    nv, nt = moved.geom_vert_count[geom], moved.geom_tri_count[geom]
    moved.vpos = moved.vpos.copy(); moved.vpos[vo:vo + nv, 1] *= 1.6; moved.vpos[vo:vo + nv, 0] += 0.5
    idx = np.ascontiguousarray(moved.tri_indices[3 * to:3 * (to + nt)])
    dev.UpdateGeom_Triangles3f(geom, moved.vpos[vo:vo + nv], idx)
    dev.CommitScene(1)
    assert dev.commit_time()["refitted"]
    _tables(dev, moved)
    _, tris, _ = _check_boxes(dev, moved, "moved vertices")
    _, want, _ = _device(moved, refit=0).read_accel()
    key = lambda t: np.lexsort((t["primId"], t["instId"]))
    assert np.array_equal(tris[key(tris)].view(np.uint8), want[key(want)].view(np.uint8))
    old = _device(sc, refit=0).read_accel()[1]
    assert not np.array_equal(tris[key(tris)].view(np.uint8), old[key(old)].view(np.uint8))
    fresh = HipIntegrator(moved)
    pos, dr = random_rays(20000, 19)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    assert not np.array_equal(hf.view(np.uint8), HipIntegrator(sc).RayQuery_NearestHit(pos, dr).view(np.uint8))
    assert np.array_equal(dev.render(4), fresh.render(4))
    # vertices and an instance together; then a device build over the positions the refit path copied
    moved.vpos[vo:vo + nv, 2] *= 0.7
    m = S.translate(-0.3, 0.2, 0.4) @ np.asarray(moved.inst_matrices[6])
    moved.inst_matrices[6] = m
    dev.UpdateGeom_Triangles3f(geom, moved.vpos[vo:vo + nv], idx)
    _apply(dev, {6: m})
    assert dev.commit_time()["refitted"]
    hf = HipIntegrator(moved).RayQuery_NearestHit(pos, dr)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    dev.set_option("refit", 0); dev.CommitScene(1); dev.set_option("refit", 1)
    assert dev.commit_time()["device_built"]
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    _check_boxes(dev, moved, "device build after moved vertices")
    # an index change: the topology is no longer the tree's
    idx2 = idx.copy(); idx2[:3] = idx[[1, 2, 0]]
    dev.UpdateGeom_Triangles3f(geom, moved.vpos[vo:vo + nv], idx2)
    dev.CommitScene(1)
    assert dev.commit_time()["device_built"] and not dev.commit_time()["refitted"]


# ---- 4. the cost ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("builder,kind", [("device", "small"), ("device", "17K"), ("host", "small"), ("host", "17K")])
def test_refitted_cost_equals_the_readers(builder, kind):
    """refit_info()["after"] against the float64 sum over the read-back nodes, relative 1e-6 (SAH_REL); after a build it equals the build's
    estimate; the build's estimate, accel_info's and the schedule do not move with a refit."""
    from hydracore3_amd.api import HipIntegrator
    sc, moved = _scene(kind), _scene(kind)
    g = _device(sc) if builder == "device" else HipIntegrator(sc)
    info = g.refit_info()
    assert info["after"] == info["build"] == g.accel_info()["sah_node_visits"] and not info["rejected"] and info["levels"] > 0
    g.render(1)
    sched = g.last_schedule()[0]
    for step, ms in enumerate((_move_four(moved), _exchange_ends(moved))):
        _apply(g, ms)
        assert g.commit_time()["refitted"]
        after = g.refit_info()
        nodes, _, root = g.read_accel()
        want = AR.sah_estimate(nodes, root)
        rel = abs(after["after"] - want) / want
        print(f"{builder} {kind} step {step}: build {after['build']:.6f} after {after['after']:.6f} reader {want:.9f} rel {rel:.2e}")
        assert rel <= SAH_REL
        assert after["build"] == info["build"] == g.accel_info()["sah_node_visits"] and after["levels"] == info["levels"]
        _tables(g, moved)
        g.render(1)
        assert g.last_schedule()[0] == sched
    assert g.refit_info()["after"] > info["build"]                           # (the exchange degraded the tree)
    g.set_option("refit", 0); g.CommitScene(1 if builder == "device" else 4)
    info = g.refit_info()
    assert not g.commit_time()["refitted"] and info["after"] == info["build"] == g.accel_info()["sah_node_visits"]


# ---- 5. the guard -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refit_max_sah_pct_turns_a_degraded_refit_into_a_build():
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    sc, moved = _scene("small"), _scene("small")
    ms = _exchange_ends(moved)
    off = _device(sc)
    _apply(off, ms)
    info = off.refit_info()
    print(f"pair exchange: estimate {info['build']:.4f} at build time, {info['after']:.4f} after the refit ({info['after'] / info['build']:.3f} x)")
    assert off.commit_time()["refitted"] and not info["rejected"]
    assert info["after"] > 1.05 * info["build"], "the exchange must degrade the tree by more than 5 % for the guard to be tested"
    fresh = HipIntegrator(moved)
    pos, dr = random_rays(20000, 23)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert np.array_equal(off.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    guarded = _device(sc, refit_max_sah_pct=105)
    _apply(guarded, ms)
    ct, info = guarded.commit_time(), guarded.refit_info()
    assert ct["device_built"] and not ct["refitted"] and info["rejected"] and info["after"] == info["build"]
    assert np.array_equal(guarded.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    _check_boxes(guarded, moved, "build after a rejected refit")
    guarded.CommitScene(1)                                                   # nothing moved since: a refit of the new tree, accepted
    assert guarded.commit_time()["refitted"] and not guarded.refit_info()["rejected"]
    loose = _device(sc, refit_max_sah_pct=100000)
    _apply(loose, ms)
    assert loose.commit_time()["refitted"] and not loose.refit_info()["rejected"]
    # a host-built tree is followed by a host build, whatever CommitScene's options say
    host = HipIntegrator(sc)
    host.set_option("refit_max_sah_pct", 105)
    _apply(host, ms, options=1)
    ct = host.commit_time()
    assert not ct["refitted"] and not ct["device_built"] and host.refit_info()["rejected"]
    assert np.array_equal(host.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    for p in (1, 50, 99):
        with pytest.raises(HydraHipError):
            host.set_option("refit_max_sah_pct", p)
    host.set_option("refit_max_sah_pct", 100); host.set_option("refit_max_sah_pct", 0)


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------------------------
def _tiny(meshes_and_matrices):
    sc = _base_scene(32, 32, False, np.random.default_rng(1))
    for mesh, mats in meshes_and_matrices:
        g = _add(sc, mesh, 0)
        for m in mats:
            sc.add_instance(g, m)
    return sc


def _brute(g, sc, n, seed, what):
    from oracle.orc import OracleIntegrator
    tris, _ = world_triangles(sc)
    pos, dr, _ = make_rays(tris, n, seed)
    cpu = OracleIntegrator(sc)
    assert_hits_equal(g.RayQuery_NearestHit(pos, dr), cpu.ray_nearest(pos, dr, brute=True), what)
    assert np.array_equal(g.RayQuery_AnyHit(pos, dr), cpu.ray_any(pos, dr, brute=True)), what


@pytest.mark.gpu
def test_smallest_trees():
    """Three triangles: one node, one level, a leaf of two and a leaf of one; it refits. Two triangles: the root is a leaf, every commit is a
    build and there are no levels. 64 coincident triangles in 64 instances: equal Morton keys, a hierarchy decided by index; it refits when one
    instance moves away. All against brute force."""
    from hydracore3_amd import scene as S
    tri = lambda x: [[x, 0.0, 0.0], [x + 1.0, 0.0, 0.2], [x, 1.0, 0.1]]
    three = (np.array(tri(-3.0) + tri(0.0) + tri(3.5)), np.arange(9).reshape(3, 3))
    sc = _tiny([(three, [np.eye(4)])])
    g = _device(sc, layout=2)
    nodes, tris, root = g.read_accel()
    assert root == 0 and tris.shape[0] == 3 and AR.reachable(nodes, root) == [0]
    assert sorted(AR.leaf_range(int(nodes[r][0]))[1] for r in ("ref0", "ref1")) == [1, 2]
    assert g.refit_info()["levels"] == 1
    _brute(g, sc, 3000, 3, "three triangles, built")
    m = S.translate(0.5, -0.25, 1.0) @ S.rotate_y(40.0) @ S.scale(1.0, 2.0, 0.5)
    sc.inst_matrices[0] = m
    _apply(g, {0: m})
    assert g.commit_time()["refitted"] and g.refit_info()["levels"] == 1
    _check_boxes(g, sc, "three triangles")
    _brute(g, sc, 3000, 4, "three triangles, refitted")

    two = (np.array(tri(-1.0) + tri(1.0)), np.arange(6).reshape(2, 3))
    sc = _tiny([(two, [np.eye(4)])])
    g = _device(sc, layout=2)
    nodes, tris, root = g.read_accel()
    assert root & AR.REF_LEAF and AR.leaf_range(root) == (0, 2) and tris.shape[0] == 2 and nodes.shape[0] == 0
    assert g.refit_info()["levels"] == 0
    sc.inst_matrices[0] = m
    _apply(g, {0: m})
    assert g.commit_time()["device_built"] and not g.commit_time()["refitted"] and g.refit_info()["levels"] == 0
    _brute(g, sc, 3000, 5, "two triangles")

    one = (np.array(tri(0.0)), np.arange(3).reshape(1, 3))
    sc = _tiny([(one, [S.translate(0.3, 0.2, 0.1)] * 64)])
    g = _device(sc, layout=2)
    assert g.refit_info()["levels"] == 5                                     # 64 equal keys, leaves of two: a balanced tree of 31 nodes
    _check_boxes(g, sc, "64 coincident triangles")
    _brute(g, sc, 3000, 6, "64 coincident triangles, built")
    away = S.translate(2.0, -1.0, 0.5) @ S.rotate_y(70.0)
    sc.inst_matrices[37] = away
    _apply(g, {37: away})
    assert g.commit_time()["refitted"]
    _check_boxes(g, sc, "64 coincident triangles, one moved away")
    _brute(g, sc, 3000, 7, "64 coincident triangles, refitted")


@pytest.mark.gpu
def test_deep_tree_refits_level_by_level():
    """nested_sheets x 8 (a device-built BVH2 some 40 levels deep whose siblings' heights differ widely): one level per height of the emitted
    tree, none empty - the level count is the root's height + 1 - and after an instance moved the refitted tree equals brute force, walked as
    4-wide tree and as BVH2."""
    from hydracore3_amd import scene as S
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(4000, 1.003, instances=8)
    # (the move keeps every hypotenuse on x + y = 0: the rays through the empty half still meet every box and no sheet)
    m = S.translate(0.002, -0.002, 0.01) @ np.asarray(sc.inst_matrices[3]) @ S.scale(1.25, 1.25, 1.0)
    moved = nested_sheets(4000, 1.003, instances=8)
    moved.inst_matrices[3] = m
    pos, dr, _ = nested_rays(moved, 2048, 47, near=0.8)
    cpu = OracleIntegrator(moved, threads=len(os.sched_getaffinity(0)))
    h = cpu.ray_nearest(pos, dr, brute=True)
    dr = with_tfar(pos, dr, np.where(h["instId"] != 0xFFFFFFFF, h["t"], np.inf), 48)     # tfar open, random, or on the exact hit (as the deep-stack tests' rays)
    hb, ab = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=True)
    assert 0.2 < (hb["instId"] != 0xFFFFFFFF).mean() < 0.8
    for wide in (1, 0):
        g = _device(sc, layout=2, wide_nodes=wide)
        nodes, _, root = g.read_accel()
        h = AR.height(nodes, root)
        print(f"nested sheets x 8, device build: root height {h}, {g.refit_info()['levels']} refit levels")
        assert h >= 17 and g.refit_info()["levels"] == h + 1
        _apply(g, {3: m})
        assert g.commit_time()["refitted"]
        what = f"nested sheets x 8 refitted, wide_nodes {wide}"
        assert_hits_equal(g.RayQuery_NearestHit(pos, dr), hb, what)
        assert np.array_equal(g.RayQuery_AnyHit(pos, dr), ab), what
        if wide:
            _check_boxes(g, moved, what)


@pytest.mark.gpu
def test_options_decide_between_refit_and_build():
    """device_refit left at 0: an update of a device-built tree is another device build, as before. "refit", 0 overrides device_refit = 1. The
    two-level layout has nothing to read back."""
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    sc, moved = _scene("small"), _scene("small")
    ms = _move_four(moved)
    plain = _device(sc, refit=0)
    assert plain.refit_info()["levels"] == 0
    _apply(plain, ms)
    assert plain.commit_time()["device_built"] and not plain.commit_time()["refitted"]
    forced = _device(sc)
    forced.set_option("refit", 0)
    _apply(forced, ms)
    assert forced.commit_time()["device_built"] and not forced.commit_time()["refitted"]
    late = _device(sc, refit=0)                                              # the option arrives after the build: no level lists, so a build - which leaves them
    late.set_option("device_refit", 1)
    _apply(late, ms)
    assert late.commit_time()["device_built"] and late.refit_info()["levels"] > 0
    late.CommitScene(1)
    assert late.commit_time()["refitted"]
    pos, dr = random_rays(5000, 29)
    hf = HipIntegrator(moved).RayQuery_NearestHit(pos, dr)
    for g in (plain, forced, late):
        assert np.array_equal(g.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    with pytest.raises(HydraHipError):
        plain.set_option("device_refit", 2)
    with pytest.raises(HydraHipError):
        HipIntegrator(sc, accel_layout=1).read_accel()

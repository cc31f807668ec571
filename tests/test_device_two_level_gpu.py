"""The two-level layout built on the device (hpt_set_option("device_build_two_level", 1), hpt_lbvh.hip section 9): one batched BLAS build for all
meshes, a TLAS over the live instances, the TLAS alone after UpdateInstance, one BLAS in its slot after UpdateGeom_Triangles3f. Hits never depend
on the tree, so queries, frames and generators must equal a host-built two-level context's and brute force bit for bit; the tree itself is read
back (read_accel_two_level) and held to the float64 reader (tests/accel2_reference.py): reachability, containment, depths, and the estimate."""
import os

import numpy as np
import pytest

import accel_reference as AR
import accel2_reference as A2
from traversal_scenes import (FAMILIES, _add, _base_scene, assert_hits_equal, degenerate_and_duplicate, fan, lone_triangle, make_rays, nested_rays, nested_sheets, quad,
                              reference_hits, sliver, transform, with_tfar, world_triangles)
from test_device_refit_gpu import _move_four, _scene, _tables, random_rays

# The device and the reader form the same float32 half-areas (same expressions, no contraction) and sum them in float64. They differ in three
# roundings to float32 the device makes and the reader does not: the BLAS visits of a mesh (its weighted terms are positive, so the sum carries no
# more than one relative 2^-24), the TLAS visits, and the result: 3 x 2^-24 = 1.8e-7. The instance term's extra product and division are in float64
# on both sides (1e-16 each). Held to 2.5e-7.
SAH2_REL = 2.5e-7
LDS_STACK = 16


def coincident(n=64):
    p = np.tile(np.array([[-0.5, -0.4, 0.1], [0.7, -0.3, -0.1], [0.0, 0.8, 0.2]]), (n, 1))
    return p, np.arange(3 * n).reshape(n, 3)


def empty_mesh():
    return np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.zeros((0, 3), int)


def _edge_scene(kind):
    """The edge cases as scenes: (meshes, [(mesh, matrix)])."""
    rng = np.random.default_rng(5)
    sc = _base_scene(32, 32, False, rng)
    kinds = ["identity", "rotate", "scale", "mirror", "shear", "far"]
    if kind == "m1_i1":                                                       # the TLAS root is an instance leaf, the BLAS root a triangle leaf
        meshes, insts = [lone_triangle()], [(0, transform("rotate", rng))]
    elif kind == "m2_i2":                                                     # a folded pair and the smallest BLAS with a node
        meshes, insts = [quad(), fan(3)], [(0, transform("scale", rng)), (1, transform("mirror", rng))]
    elif kind == "m5_i3":                                                     # an empty mesh, instanced; a mesh never instanced; equal Morton keys inside a mesh
        meshes = [degenerate_and_duplicate(), empty_mesh(), coincident(), sliver(), lone_triangle()]
        insts = [(0, transform("mirror", rng)), (1, np.eye(4)), (2, transform("shear", rng))]
    elif kind == "m5_i11":                                                    # every transform kind; one mesh five times under one matrix (equal TLAS keys)
        meshes = [lone_triangle(), quad(), sliver(), coincident(), fan(3)]
        insts = [(k % 5, transform(kinds[k], rng)) for k in range(6)]
        same = transform("rotate", rng)
        insts += [(4, same)] * 5
    else:                                                                     # 300 meshes: the slot prefix crosses 8 bits
        meshes = [quad() for _ in range(300)]
        insts = [(k, transform(("rotate", "scale", "mirror")[k % 3], rng)) for k in range(300)]
    geoms = [_add(sc, m, k % 4) for k, m in enumerate(meshes)]
    for gi, m in insts:
        sc.add_instance(geoms[gi], m)
    return sc


def _ctx(sc, two_level=1, options=1, **opts):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, accel_layout=1)
    g.set_option("device_build_two_level", two_level)
    for k, v in opts.items():
        g.set_option(k, v)
    g.CommitScene(options)
    return g


def _device(sc, **opts):
    g = _ctx(sc, **opts)
    info = g.two_level_info()
    assert g.commit_time()["device_built"] and info["device_built"] and g.accel_info()["layout"] == "two-level", (g.commit_time(), info)
    return g


def _meshes(sc):
    """Per mesh: (nt, 3, 3) float64 object-space vertices by primitive, and the float32 bounds of the vertices its triangles use."""
    verts, bounds = [], {}
    for g in range(len(sc.geom_tri_count)):
        to, vo = sc.mat_vert_offset[g]
        nt = sc.geom_tri_count[g]
        idx = sc.tri_indices[3 * to:3 * (to + nt)].reshape(nt, 3).astype(np.int64) + vo
        p = sc.vpos[:, :3].astype(np.float32)[idx]
        verts.append(p.astype(np.float64))
        if nt:
            bounds[g] = (p.reshape(-1, 3).min(axis=0), p.reshape(-1, 3).max(axis=0))
    return verts, bounds


def _check_tree(g, sc, what):
    """Reachability, containment and depths of the read-back; returns (nodes, tris, insts, root)."""
    nodes, tris, insts, root = g.read_accel_two_level()
    verts, _ = _meshes(sc)
    ni = len(sc.inst_geom)
    assert insts.shape[0] == ni and tris.shape[0] == sum(sc.geom_tri_count)
    assert np.array_equal(insts["geomId"], np.asarray(sc.inst_geom, np.uint32))
    live = np.array([sc.geom_tri_count[gm] > 0 for gm in sc.inst_geom])
    assert np.array_equal(A2.instance_counts(nodes, root, ni), live.astype(np.int64)), f"{what}: instances reached {A2.instance_counts(nodes, root, ni)}"
    assert np.array_equal(insts["root"] == AR.REF_NONE, ~live)
    assert np.array_equal(insts["moving"], np.array([1 if i in sc.inst_motion else 0 for i in range(ni)], np.uint32))
    instanced = sorted(set(sc.inst_geom))
    cnt, owner = A2.blas_record_counts(nodes, insts, tris.shape[0])
    first = np.concatenate([[0], np.cumsum(sc.geom_tri_count)])
    for gm in instanced:
        assert np.all(cnt[first[gm]:first[gm + 1]] == 1) and np.all(owner[first[gm]:first[gm + 1]] == gm), f"{what}: mesh {gm}'s records"
        assert sorted(tris["primId"][first[gm]:first[gm + 1]]) == list(range(sc.geom_tri_count[gm]))
    bad = A2.blas_violations(nodes, tris, insts, verts)
    assert not bad, f"{what}: {len(bad)} BLAS violations, first: {bad[:3]}"
    bad = A2.tlas_violations(nodes, root, insts, verts, sc.inst_matrices, sc.inst_motion)
    assert not bad, f"{what}: {len(bad)} TLAS violations, first: {bad[:3]}"
    info = g.two_level_info()
    if info["device_built"]:
        assert info["tlas_depth"] == A2.depth(nodes, root), (info, A2.depth(nodes, root))
        roots = A2.blas_roots(insts)
        # (the reported depth covers every mesh, instanced or not; a mesh nobody instances has no record that names its root)
        assert info["blas_depth"] >= max(A2.depth(nodes, r) for r in roots.values())
        if len(instanced) == len(sc.geom_tri_count):
            assert info["blas_depth"] == max(A2.depth(nodes, r) for r in roots.values())
    return nodes, tris, insts, root


def _queries(sc, n, seed):
    """Rays of every family with mixed tfar, and the brute-force answers of the oracle (bit for bit what every traversal must return)."""
    from oracle.orc import OracleIntegrator
    wt, ids = world_triangles(sc)
    pos, dr, fam = make_rays(wt, n, seed)
    cpu = OracleIntegrator(sc)
    h = cpu.ray_nearest(pos, dr, brute=True)
    dr2 = with_tfar(pos, dr, np.where(h["instId"] != 0xFFFFFFFF, h["t"], np.inf), seed + 1)
    return pos, dr, dr2, h, cpu.ray_nearest(pos, dr2, brute=True), cpu.ray_any(pos, dr2, brute=True), (wt, ids, fam)


# ---- 1. mesh and instance edge cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["m1_i1", "m2_i2", "m5_i3", "m5_i11", "m300"])
def test_edge_scenes_equal_brute_force_and_the_host_built_tree(kind):
    from hydracore3_amd.api import HipIntegrator
    sc = _edge_scene(kind)
    dev = _device(sc)
    info = dev.two_level_info()
    nonempty = sum(1 for n in sc.geom_tri_count if n)
    assert info["blas_built"] == nonempty and info["blas_kept"] == 0 and not info["tlas_only"]
    nodes, tris, insts, root = _check_tree(dev, sc, kind)
    if kind == "m1_i1":
        assert root == AR.REF_LEAF | 0 and insts["root"][0] == AR.REF_LEAF | (1 << 28) and info["tlas_depth"] == 0 and info["blas_depth"] == 0
    if kind == "m2_i2":
        assert insts["root"][0] & AR.REF_LEAF and AR.leaf_range(int(insts["root"][0]))[1] == 2 and A2.depth(nodes, int(insts["root"][1])) == 1
    host = HipIntegrator(sc, accel_layout=1)
    assert not host.commit_time()["device_built"] and not host.two_level_info()["device_built"]
    pos, dr, dr2, h, h2, a2, (wt, ids, fam) = _queries(sc, 3000, 41)
    for g, name in ((dev, "device-built"), (host, "host-built")):
        assert_hits_equal(g.RayQuery_NearestHit(pos, dr), h, f"{kind} {name}")
        assert_hits_equal(g.RayQuery_NearestHit(pos, dr2), h2, f"{kind} {name}, tfar")
        assert np.array_equal(g.RayQuery_AnyHit(pos, dr2), a2), f"{kind} {name}, any hit"
    # the float64 reference of the forward-transformed meshes, on the rays it calls robust (grazing rays are held to brute force only, as in
    # test_traversal_edges.py: a handful of them hit in float where float64 misses robustly by the reference's bounds)
    hit, t, inst, prim, robust = reference_hits(wt, ids, sc.inst_matrices, pos, dr)
    got = dev.RayQuery_NearestHit(pos, dr)
    r = np.flatnonzero(robust & (fam != FAMILIES.index("grazing")))
    assert np.array_equal(got["instId"][r] != 0xFFFFFFFF, hit[r])
    rh = r[hit[r]]
    assert np.array_equal(got["instId"][rh].astype(np.int64), inst[rh]) and np.array_equal(got["primId"][rh].astype(np.int64), prim[rh])
    # the estimate, against the reader
    want = A2.estimate(nodes, insts, root, _meshes(sc)[1])
    have = dev.accel_info()["sah_node_visits"]
    print(f"{kind}: estimate {have:.7f}, reader {want:.9f}, {info}")
    assert abs(have - want) <= SAH2_REL * want


# ---- 2. the interior, forced two-level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "17K"])
def test_interior_queries_frames_and_generators_equal_the_host_built_context(kind):
    from hydracore3_amd.api import HipIntegrator
    sc = _scene(kind)
    dev, host = _device(sc), HipIntegrator(sc, accel_layout=1)
    nodes, tris, insts, root = _check_tree(dev, sc, kind)
    want = A2.estimate(nodes, insts, root, _meshes(sc)[1])
    have = dev.accel_info()["sah_node_visits"]
    print(f"interior {kind}: estimate {have:.6f} (host-built {host.accel_info()['sah_node_visits']:.6f}), reader {want:.9f}, {dev.two_level_info()}, {dev.commit_time()}")
    assert abs(have - want) <= SAH2_REL * want
    pos, dr = random_rays(20000, 17)
    hf = host.RayQuery_NearestHit(pos, dr)
    assert (hf["geomId"] != 0xFFFFFFFF).mean() > 0.5
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    dr2 = dr.copy(); dr2[:, 3] = np.random.default_rng(5).uniform(0.3, 9.0, dr.shape[0]).astype(np.float32)
    assert np.array_equal(dev.RayQuery_AnyHit(pos, dr2), host.RayQuery_AnyHit(pos, dr2))
    for sched, spp in ((1, 3), (2, 4)):
        dev.set_schedule(sched); host.set_schedule(sched)
        assert np.array_equal(dev.render(spp), host.render(spp)), sched
        assert np.array_equal(dev.random_gens(), host.random_gens())
        assert dev.last_schedule()[0] == sched


# ---- 3. UpdateInstance: the TLAS alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_instance_rebuilds_only_the_tlas():
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd import scene as S
    sc, moved = _scene("small"), _scene("small")
    dev = _device(sc)
    dev.render(1)
    n0, t0, i0, _ = dev.read_accel_two_level()
    ni = len(sc.inst_geom)
    ms = _move_four(moved)
    for i, m in ms.items():
        dev.UpdateInstance(i, m)
    dev.CommitScene(1)
    info = dev.two_level_info()
    assert dev.commit_time()["device_built"] and info["device_built"] and info["tlas_only"] and info["blas_built"] == 0 and info["blas_kept"] == len(sc.geom_tri_count)
    _tables(dev, moved)
    n1, t1, i1, _ = _check_tree(dev, moved, "TLAS-only update")
    assert np.array_equal(t0.view(np.uint8), t1.view(np.uint8)), "a triangle record changed"
    assert np.array_equal(n0[ni:].view(np.uint8), n1[ni:].view(np.uint8)), "a node outside the TLAS region changed"
    assert not np.array_equal(n0[:ni].view(np.uint8), n1[:ni].view(np.uint8)) and np.array_equal(i0["root"], i1["root"])
    fresh = HipIntegrator(moved, accel_layout=1)
    pos, dr = random_rays(20000, 17)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    assert not np.array_equal(hf.view(np.uint8), HipIntegrator(sc, accel_layout=1).RayQuery_NearestHit(pos, dr).view(np.uint8))
    assert np.array_equal(dev.render(3), fresh.render(3))
    m = S.translate(0.2, 0.1, -0.3) @ np.asarray(moved.inst_matrices[7])         # a second round, on the updated tree
    moved.inst_matrices[7] = m
    dev.UpdateInstance(7, m); dev.CommitScene(1); _tables(dev, moved)
    assert dev.two_level_info()["tlas_only"]
    again = HipIntegrator(moved, accel_layout=1)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), again.RayQuery_NearestHit(pos, dr).view(np.uint8))
    assert np.array_equal(dev.render(3), again.render(3))
    dev.set_option("refit", 0); dev.CommitScene(1)                               # "refit", 0: always a full build
    info = dev.two_level_info()
    assert info["device_built"] and not info["tlas_only"] and info["blas_kept"] == 0
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), again.RayQuery_NearestHit(pos, dr).view(np.uint8))


# ---- 4. moved vertices: one BLAS in its slot ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_geom_rebuilds_one_blas_in_place():
    from hydracore3_amd.api import HipIntegrator
    sc, moved = _scene("small"), _scene("small")
    dev = _device(sc)
    n0, t0, i0, _ = dev.read_accel_two_level()
    geom = 4
    to, vo = moved.mat_vert_offset[geom]
    nv, nt = moved.geom_vert_count[geom], moved.geom_tri_count[geom]
    moved.vpos = moved.vpos.copy(); moved.vpos[vo:vo + nv, 1] *= 1.6; moved.vpos[vo:vo + nv, 0] += 0.5
    idx = np.ascontiguousarray(moved.tri_indices[3 * to:3 * (to + nt)])
    dev.UpdateGeom_Triangles3f(geom, moved.vpos[vo:vo + nv], idx)
    dev.CommitScene(1)
    info = dev.two_level_info()
    meshes = sum(1 for n in sc.geom_tri_count if n)
    assert info["device_built"] and info["blas_built"] == 1 and info["blas_kept"] == meshes - 1 and not info["tlas_only"]
    _tables(dev, moved)
    n1, t1, i1, _ = _check_tree(dev, moved, "moved vertices")
    ni = len(sc.inst_geom)
    tfirst = int(np.sum(sc.geom_tri_count[:geom])); nfirst = ni + int(sum(max(n - 1, 0) for n in sc.geom_tri_count[:geom]))
    keep_t = np.ones(t0.shape[0], bool); keep_t[tfirst:tfirst + nt] = False
    keep_n = np.ones(n0.shape[0], bool); keep_n[:ni] = False; keep_n[nfirst:nfirst + nt - 1] = False
    assert np.array_equal(t0[keep_t].view(np.uint8), t1[keep_t].view(np.uint8)) and not np.array_equal(t0[~keep_t].view(np.uint8), t1[~keep_t].view(np.uint8))
    assert np.array_equal(n0[keep_n].view(np.uint8), n1[keep_n].view(np.uint8)), "another mesh's nodes changed"
    others = i0["geomId"] != geom                                                # (the rebuilt BLAS' root may sit at either end of its slot)
    assert np.array_equal(i0["root"][others], i1["root"][others]) and np.all((i1["root"][~others] >= nfirst) & (i1["root"][~others] < nfirst + nt - 1))
    fresh = HipIntegrator(moved, accel_layout=1)
    pos, dr = random_rays(20000, 19)
    hf = fresh.RayQuery_NearestHit(pos, dr)
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))
    assert not np.array_equal(hf.view(np.uint8), HipIntegrator(sc, accel_layout=1).RayQuery_NearestHit(pos, dr).view(np.uint8))
    idx2 = idx.copy(); idx2[:3] = idx[[1, 2, 0]]                                 # changed indices: a full build
    dev.UpdateGeom_Triangles3f(geom, moved.vpos[vo:vo + nv], idx2)
    dev.CommitScene(1)
    info = dev.two_level_info()
    assert info["device_built"] and info["blas_built"] == meshes and info["blas_kept"] == 0
    assert np.array_equal(dev.RayQuery_NearestHit(pos, dr).view(np.uint8), hf.view(np.uint8))


# ---- 5. a moving instance ---------------------------------------------------------------------------------------------------------------------------------
def _motion_scene():
    from hydracore3_amd import scene as S
    rng = np.random.default_rng(9)
    sc = _base_scene(48, 32, False, rng)
    geoms = [_add(sc, m, k % 4) for k, m in enumerate((fan(5), quad(), coincident(8)))]
    sc.add_instance(geoms[0], transform("rotate", rng))
    m0 = transform("scale", rng)
    sc.add_instance(geoms[1], m0, motion_matrix=S.translate(1.5, -0.5, 0.75) @ m0 @ S.rotate_y(35.0))
    sc.add_instance(geoms[2], transform("shear", rng))
    sc.add_instance(geoms[0], transform("mirror", rng))
    return sc


@pytest.mark.gpu
def test_moving_instance_equals_the_host_built_context():
    from hydracore3_amd.api import HipIntegrator
    sc = _motion_scene()
    dev, host = _device(sc), HipIntegrator(sc, accel_layout=1)
    _, _, insts, _ = _check_tree(dev, sc, "moving instance")                     # (the TLAS leaf of instance 1 holds both keys: tlas_violations)
    assert list(insts["moving"]) == [0, 1, 0, 0]
    wt, _ = world_triangles(sc)
    pos, dr, _ = make_rays(wt, 4000, 43)
    dr2 = dr.copy(); dr2[:, 3] = np.random.default_rng(6).uniform(0.3, 9.0, dr.shape[0]).astype(np.float32)
    differs = False
    for time in (0.0, 0.37, 1.0):
        a, b = dev.RayQuery_NearestHitMotion(pos, dr, time), host.RayQuery_NearestHitMotion(pos, dr, time)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), time
        assert np.array_equal(dev.RayQuery_AnyHitMotion(pos, dr2, time), host.RayQuery_AnyHitMotion(pos, dr2, time)), time
        differs = differs or not np.array_equal(a.view(np.uint8), dev.RayQuery_NearestHitMotion(pos, dr, 0.0).view(np.uint8))
    assert differs, "the motion moved no hit"
    assert np.array_equal(dev.render(4), host.render(4))
    assert np.array_equal(dev.random_gens(), host.random_gens())
    # a forced sweep does not hold moving instances: the option does not turn that error into a two-level build
    from hydracore3_amd.api import HydraHipError
    assert dev.L.hpt_set_accel_layout(dev.h, 3) == 0
    with pytest.raises(HydraHipError):
        dev.CommitScene(1)


# ---- 6. deep trees ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_deep_blas_under_two_instances_walks_the_hbm_part_of_the_stack():
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(4000, 1.003, instances=2)
    dev = _device(sc)
    info = dev.two_level_info()
    nodes, _, insts, root = _check_tree(dev, sc, "nested sheets x 2")
    stack = info["tlas_depth"] + 1 + info["blas_depth"] + 1
    print(f"nested sheets x 2: {info}, stack {stack}")
    assert stack > LDS_STACK and len(set(insts["root"][:2])) == 1
    pos, dr, _ = nested_rays(sc, 2048, 47, near=0.8)
    cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
    h = cpu.ray_nearest(pos, dr, brute=True)
    dr = with_tfar(pos, dr, np.where(h["instId"] != 0xFFFFFFFF, h["t"], np.inf), 48)
    dev.set_option("dbg_stack_witness", 1)
    assert_hits_equal(dev.RayQuery_NearestHit(pos, dr), cpu.ray_nearest(pos, dr, brute=True), "nested sheets x 2")
    words, filled = dev.stack_witness()
    assert filled > 0 and words > 0, f"no lane pushed beyond the LDS part of its stack ({words} of {filled})"
    assert np.array_equal(dev.RayQuery_AnyHit(pos, dr), cpu.ray_any(pos, dr, brute=True))


def bit_chain():
    """Tiny triangles whose box centres fall into Morton cells with ONE bit set, a different bit each (2^-k on one axis, k = 1 .. 21), plus the three
    unit points that make the bounds [0, 1]^3 and 64 coincident triangles at the origin: the Karras tree peels one triangle per level - some 60
    levels - and the equal keys add five more, past the 64-entry traversal stack whatever the TLAS adds."""
    e = 2.0 ** -30
    pts = [[2.0 ** -k if a == ax else 0.0 for a in range(3)] for ax in range(3) for k in range(1, 22)]
    tris = [[[x, y, z], [x + e, y, z], [x, y + e, z + e]] for x, y, z in pts]
    tris += [[[1.0, 0, 0], [1.0 - e, 0, 0], [1.0, e, e]], [[0, 1.0, 0], [e, 1.0, 0], [0, 1.0 - e, e]], [[0, 0, 1.0], [e, 0, 1.0], [0, e, 1.0 - e]]]
    tris += [[[0.0, 0, 0], [e, 0, 0], [0, e, e]]] * 64
    p = np.array(tris).reshape(-1, 3)
    return p, np.arange(p.shape[0]).reshape(-1, 3)


@pytest.mark.gpu
def test_a_tree_deeper_than_the_stack_goes_back_to_the_host_builder():
    from oracle.orc import OracleIntegrator
    rng = np.random.default_rng(3)
    sc = _base_scene(32, 32, False, rng)
    g0, g1 = _add(sc, bit_chain(), 0), _add(sc, quad(), 1)
    sc.add_instance(g0, np.eye(4)); sc.add_instance(g1, transform("rotate", rng)); sc.add_instance(g0, transform("scale", rng))
    g = _ctx(sc)
    assert not g.commit_time()["device_built"] and not g.two_level_info()["device_built"] and g.accel_info()["layout"] == "two-level"
    _check_tree(g, sc, "deep chain, host-built")
    wt, _ = world_triangles(sc)
    pos, dr, _ = make_rays(wt[-130:], 2000, 51)
    cpu = OracleIntegrator(sc)
    assert_hits_equal(g.RayQuery_NearestHit(pos, dr), cpu.ray_nearest(pos, dr, brute=True), "deep chain")


# ---- 7. the off switch ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_the_option_commits_are_the_host_builds():
    sc = _scene("small")
    a, b = _ctx(sc, two_level=0), _ctx(sc, two_level=0)
    c = _ctx(sc, two_level=1, device_build=0)
    d = _ctx(sc, two_level=1, options=4)                                         # BUILD_HIGH asks for the host's tree
    for g in (a, b, c, d):
        assert not g.commit_time()["device_built"] and not any(g.two_level_info().values())
    na, nb = a.read_accel_two_level(), b.read_accel_two_level()
    for x, y, z in zip(na[:3], nb[:3], c.read_accel_two_level()[:3]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))
    _check_tree(a, sc, "host-built two-level")
    from hydracore3_amd.api import HipIntegrator, HydraHipError
    with pytest.raises(HydraHipError):
        a.set_option("device_build_two_level", 2)
    with pytest.raises(HydraHipError):
        HipIntegrator(sc, accel_layout=2).read_accel_two_level()

"""Every traversal layout against brute force on adversarial scenes and rays (tests/traversal_scenes.py): instanced meshes under rotations,
non-uniform scales, mirrors, shears and far translations; odd meshes, slivers, zero-area and duplicated triangles; the per-lane pass' pair
bounds; rays at edges and vertices, grazing, leaving a surface, axis-parallel, from far away, with tnear < 0 (hits behind the origin) and tfar
on the exact hit. On the CPU the oracle's BVH equals its brute force bit for bit and both agree with a float64 reference on the rays whose
answer is robust; on the GPU every layout and sweep variant equals the oracle's brute force bit for bit, and sweep frames equal layout 1's."""
import numpy as np
import pytest

from conftest import assert_pixel_parity
from hydracore3_amd import scene as S
from hydracore3_amd.scene import INTEGRATOR_MIS_PT, INTEGRATOR_SHADOW_PT
from traversal_scenes import (FAMILIES, FLT_MAX, NO_HIT, assert_hits_equal, forced_sweep_scene, make_rays, reference_hits, sweep_scene, with_tfar,
                              world_triangles)

AUTO_SEEDS = (11, 12, 13)
FORCED_SEED = 21


def _scene(kind, seed):
    return sweep_scene(seed) if kind == "auto" else forced_sweep_scene(seed)


def _rays(sc, cpu, n, seed):
    """The ray families of make_rays, with tfar chosen against the oracle's brute-force t of the open ray."""
    tris, _ = world_triangles(sc)
    pos, dr, fam = make_rays(tris, n, seed)
    h = cpu.ray_nearest(pos, dr, brute=True)
    # Far origins (1e3 .. 1e5 away) keep an open or random tfar. A known limit, not fixed here: that far out the float triangle test's t and
    # its barycentrics carry errors of the size of the origin's ulp, and the boxes of every tree layout (device and oracle, tnear of either
    # sign) are padded relative to the box, not to the origin - with tfar exactly on such a hit a tree lost 2 of 80 000 rays, and the
    # oracle's BVH can return another triangle than its brute force at origins ~7e4 away.
    open_t = np.where((h["instId"] != NO_HIT) & (fam != FAMILIES.index("far")), h["t"], np.inf)
    return pos, with_tfar(pos, dr, open_t, seed + 1), fam


# ---- CPU: the oracle's BVH, its brute force and the float64 reference -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [("auto", s) for s in AUTO_SEEDS] + [("forced", FORCED_SEED)])
def test_oracle_bvh_and_brute_force_agree_with_float64(kind, seed):
    """ray_nearest / ray_any with brute=False equal brute=True bit for bit (tnear < 0 included); on the rays whose float64 answer is robust,
    hit or miss, (instId, primId) and t (1e-4 relative, plus 1e-6 of the origin's coordinates) equal the float64 reference of the forward-transformed meshes."""
    from oracle.orc import OracleIntegrator
    sc = _scene(kind, seed)
    if kind == "auto":
        assert sum(sc.geom_tri_count[g] for g in sc.inst_geom) <= 32 and len(sc.inst_geom) <= 5
    cpu = OracleIntegrator(sc)
    pos, dr, fam = _rays(sc, cpu, 12000, seed)
    hb, hn = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_nearest(pos, dr, brute=False)
    ab, an = cpu.ray_any(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=False)
    assert np.array_equal(ab != 0, hb["instId"] != NO_HIT)
    tris, ids = world_triangles(sc)
    hit, t, inst, prim, robust = reference_hits(tris, ids, sc.inst_matrices, pos, dr)
    # The oracle's BVH == its brute force, bit for bit, on every ray with tnear >= 0 and on every ray whose float64 answer is robust. A known
    # limit of the oracle, not fixed here: with tnear < 0 its BVH loses a non-robust hit on 1 of the 12 000 rays of auto-13 and of forced-21
    # (none in auto-11, auto-12); the count is held to that bound so that a new loss fails.
    keep = (pos[:, 3] >= 0.0) | robust
    lost = np.flatnonzero((hn["t"].view(np.uint32) != hb["t"].view(np.uint32)) | (hn["primId"] != hb["primId"]) | (hn["instId"] != hb["instId"]))
    print(f"{kind} {seed}: oracle BVH != brute force on rays {lost} (tnear {pos[lost, 3]})")
    assert lost.size <= 1
    assert_hits_equal(hn[keep], hb[keep], "oracle BVH vs brute force")
    assert np.array_equal(an[keep], ab[keep]) and np.sum(an != ab) <= 1
    behind = robust & hit & (t < 0.0)
    print(f"{kind} {seed}: {robust.mean():.1%} robust, {int((robust & hit).sum())} robust hits ({int(behind.sum())} behind the origin), "
          f"per family: {[f'{f} {robust[fam == i].mean():.0%}' for i, f in enumerate(FAMILIES)]}")
    assert robust.mean() > 0.15 and (robust & hit).sum() > 50 and behind.sum() > 25
    # (grazing rays are held to the brute force above and on the GPU, not to float64: a handful per scene of them hit in float where float64
    # misses robustly by these bounds - an open question about the bounds, not about any traversal)
    r = np.flatnonzero(robust & (fam != FAMILIES.index("grazing")))
    got = hb["instId"][r] != NO_HIT
    bad = r[got != hit[r]]
    assert bad.size == 0, f"hit / miss differs from float64 on {bad.size} robust rays, first {bad[:8]}"
    rh = r[hit[r]]
    assert np.array_equal(hb["instId"][rh].astype(np.int64), inst[rh]) and np.array_equal(hb["primId"][rh].astype(np.int64), prim[rh])
    assert np.all(np.abs(hb["t"][rh] - t[rh]) <= 1e-4 * np.maximum(np.abs(t[rh]), 1.0) + 1e-6 * np.abs(pos[rh, :3]).max(axis=1))


# ---- GPU: ray queries through every layout ----------------------------------------------------------------------------------------------------
def _variants(sc, auto_layout):
    """(name, integrator): the automatic layout, layouts 1, 2 and 3, layout 3 with every (sweep_cull, sweep_lanes), the device-built tree with
    and without wide_nodes."""
    from hydracore3_amd.api import HipIntegrator
    auto = HipIntegrator(sc)
    assert auto.accel_info()["layout"] == auto_layout
    yield "automatic", auto
    for layout in (1, 2, 3):
        yield f"layout {layout}", HipIntegrator(sc, accel_layout=layout)
    for cull in (0, 1):
        for lanes in (0, 1):
            g = HipIntegrator(sc, accel_layout=3)
            g.set_option("sweep_cull", cull); g.set_option("sweep_lanes", lanes)
            yield f"sweep cull {cull} lanes {lanes}", g
    for wide in (1, 0):
        g = HipIntegrator(sc, accel_layout=2)
        g.set_option("device_build", 1); g.set_option("wide_nodes", wide); g.CommitScene()
        assert g.commit_time()["device_built"]
        yield f"device build, wide_nodes {wide}", g


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", [("auto", s) for s in AUTO_SEEDS] + [("forced", FORCED_SEED)])
def test_every_layout_returns_the_brute_force_hits(kind, seed):
    """RayQuery_NearestHit / AnyHit of every layout and sweep variant == the oracle's brute force, bit for bit (t, prim, inst, geom, coords,
    occlusion flags), on the adversarial families with tnear down to -FLT_MAX and tfar on the exact hit."""
    from oracle.orc import OracleIntegrator
    sc = _scene(kind, seed)
    cpu = OracleIntegrator(sc)
    pos, dr, _ = _rays(sc, cpu, 20000, seed + 7)
    hb, ab = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=True)
    assert (hb["instId"] != NO_HIT).mean() > 0.2 and ((hb["instId"] != NO_HIT) & (hb["t"] < 0)).sum() > 300
    for name, g in _variants(sc, "sweep" if kind == "auto" else "flat"):
        assert_hits_equal(g.RayQuery_NearestHit(pos, dr), hb, f"{kind} {seed}, {name}")
        a = g.RayQuery_AnyHit(pos, dr)
        bad = np.flatnonzero(a != ab)
        assert bad.size == 0, f"{kind} {seed}, {name}: any-hit differs on {bad.size} rays, first {bad[:8]}"


@pytest.mark.gpu
def test_wide_and_device_built_trees_keep_hits_behind_the_origin():
    """The 4-wide compressed tree, the BVH2 and the device-built trees of a heavy scene on the tnear < 0 and far-origin families: equal to the
    oracle's brute force bit for bit."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd import synth
    from oracle.orc import OracleIntegrator
    sc = synth.interior_scene(160, 96, subdiv=1, tex_size=16)
    cpu = OracleIntegrator(sc)
    tris, _ = world_triangles(sc)
    pos, dr, _ = make_rays(tris, 3000, 41, families=("random", "far", "grazing"))
    pos[:, 3] = np.random.default_rng(42).choice(np.float32([-1.0, -1e2, -1e4, -FLT_MAX]), pos.shape[0])
    hb, ab = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=True)
    assert ((hb["instId"] != NO_HIT) & (hb["t"] < -10.0)).sum() > 100
    wide = HipIntegrator(sc)
    assert wide.accel_info()["layout"] == "flat" and wide.accel_info()["sah_node_visits"] >= 20.0
    wide.render(1)
    assert wide.last_launch()["wide_nodes"]
    variants = [("wide", wide)]
    narrow = HipIntegrator(sc); narrow.set_option("wide_nodes", 0); variants.append(("bvh2", narrow))
    variants.append(("two-level", HipIntegrator(sc, accel_layout=1)))
    for w in (1, 0):
        g = HipIntegrator(sc); g.set_option("device_build", 1); g.set_option("wide_nodes", w); g.CommitScene()
        assert g.commit_time()["device_built"]
        variants.append((f"device build, wide_nodes {w}", g))
    for name, g in variants:
        assert_hits_equal(g.RayQuery_NearestHit(pos, dr), hb, f"interior, {name}")
        assert np.array_equal(g.RayQuery_AnyHit(pos, dr), ab), name


@pytest.mark.gpu
def test_moving_instances_keep_hits_behind_the_origin():
    """RayQuery_NearestHitMotion with tnear < 0 on a random scene with a moving instance == ray_nearest_motion(brute=True), bit for bit."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd import synth
    from oracle.orc import OracleIntegrator
    seed = next(s for s in range(100) if synth.random_scene(s).inst_motion)
    sc = synth.random_scene(seed)
    gpu, cpu = HipIntegrator(sc), OracleIntegrator(sc)
    tris, _ = world_triangles(sc)
    pos, dr, _ = make_rays(tris, 6000, 43, families=("random", "aimed", "far", "offset"))
    pos[:, 3] = np.random.default_rng(44).choice(np.float32([0.0, -1.0, -1e2, -1e4, -FLT_MAX]), pos.shape[0])
    behind = 0
    for time in (0.0, 0.4, 1.0):
        hb = cpu.ray_nearest_motion(pos, dr, time, brute=True)
        assert_hits_equal(gpu.RayQuery_NearestHitMotion(pos, dr, time), hb, f"motion, time {time}")
        assert np.array_equal(gpu.RayQuery_AnyHitMotion(pos, dr, time), cpu.ray_any_motion(pos, dr, time, brute=True))
        behind += int(((hb["instId"] != NO_HIT) & (hb["t"] < -1.0)).sum())
    assert behind > 300


# ---- GPU: path tracing on the automatic-sweep scenes --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", AUTO_SEEDS)
def test_sweep_frames_equal_layout_1_and_the_oracle(seed):
    """Frames and generator states bit-identical between layout 3 (every sweep_cull, sweep_lanes) and layout 1, in RGB and spectral mode, MIS,
    shadow-PT and naive; the wavefront schedule (2, on the two-level tree) equal to the swept megakernel (1); per-pixel parity with the oracle."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    spp = 4
    for spectral in (False, True):
        sc = sweep_scene(seed, spectral=spectral)
        for integ, naive in ((INTEGRATOR_MIS_PT, False), (INTEGRATOR_SHADOW_PT, False), (INTEGRATOR_MIS_PT, True)):
            prm = sc.params(integ)
            ref = HipIntegrator(sc, prm, accel_layout=1)
            img = ref.render(spp, naive=naive)
            assert img[..., :3].mean() > 0
            for cull in (0, 1):
                for lanes in (0, 1):
                    g = HipIntegrator(sc, prm, accel_layout=3)
                    g.set_option("sweep_cull", cull); g.set_option("sweep_lanes", lanes)
                    what = f"spectral {spectral}, integrator {integ}, naive {naive}, cull {cull}, lanes {lanes}"
                    assert np.array_equal(g.render(spp, naive=naive).view(np.uint32), img.view(np.uint32)), what
                    assert np.array_equal(g.random_gens(), ref.random_gens()), what
            if naive:
                continue
            a, b = HipIntegrator(sc, prm), HipIntegrator(sc, prm, accel_layout=1)        # (the wavefront schedule walks the two-level tree)
            a.set_schedule(1); b.set_schedule(2)
            ia, ib = a.render(spp), b.render(spp)
            assert a.last_schedule()[0] == 1 and b.last_schedule()[0] == 2
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and np.array_equal(a.random_gens(), b.random_gens())
            cpu = OracleIntegrator(sc, prm)
            assert_pixel_parity(ia, cpu.render(spp), spp, a, cpu, max_divergent=8, what=f"seed {seed} spectral {spectral} integrator {integ}: ")


@pytest.mark.gpu
def test_sweep_dr_equals_layout_1():
    """PathTraceDR on an automatic-sweep scene, sweep against layout 1: the same frame and generators bit for bit, the same loss and gradient up
    to the order of the gradient's float atomics."""
    from hydracore3_amd.api import HipIntegrator
    out = {}
    for layout in (0, 1):
        sc = sweep_scene(AUTO_SEEDS[0], 32, 32)
        sc.materials = [S.material_gltf((0.6, 0.55, 0.5, 1.0), 0.0, 0.3), S.material_gltf((0.8, 0.8, 0.8, 1.0), 0.0, 0.5, 1.0, 1.5, 1),
                        S.material_gltf((0.9, 0.9, 0.9, 1.0), 1.0, 0.9), S.material_gltf((0.3, 0.5, 0.8, 1.0), 0.5, 0.7)]   # (what PathTraceDR takes)
        g = HipIntegrator(sc, accel_layout=layout)
        assert g.accel_info()["layout"] == ("sweep" if layout == 0 else "two-level")
        off, size = g.PutDiffTex2D(1, 8, 8, 4)
        rng = np.random.default_rng(5)
        data = rng.uniform(0.2, 0.9, size).astype(np.float32)
        ref = rng.uniform(0.0, 0.5, (sc.height, sc.width, 4)).astype(np.float32)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        grad = np.zeros_like(data)
        loss = g.PathTraceDR(g.N, 4, img, 4, ref, data, grad)
        out[layout] = (img, g.random_gens(), loss, grad)
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == pytest.approx(out[1][2], rel=1e-6)
    assert np.count_nonzero(out[1][3]) > 20
    assert np.allclose(out[0][3], out[1][3], rtol=1e-5, atol=1e-7 * np.abs(out[1][3]).max())

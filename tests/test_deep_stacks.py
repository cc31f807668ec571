"""The HBM half of the traversal stacks. Every tree-walking kernel keeps 16 stack entries of a lane in LDS and the deeper ones in a per-lane slice
of an HBM buffer whose pointer, stride and lane index each kernel family works out itself; no other scene of the suite makes a stack pointer
pass 16. nested_sheets (tests/traversal_scenes.py) does: its trees are 18 (BVH2) and 16 (4-wide, stack bound 49) levels deep and a ray near the
axis meets every node's box. hpt_set_option("dbg_stack_witness", 1) fills the buffer with a word no traversal pushes before every launch, and
stack_witness() counts the words a launch wrote: every GPU case here asserts that count, so a case that stopped reaching the deep path fails
rather than passes idly. On the CPU the oracle's BVH equals its brute force bit for bit and both agree with a float64 reference on the robust
rays; on the GPU ray queries equal the oracle's brute force bit for bit under every layout, frames and generators are bit-identical across the
four schedules (RGB and spectral; MIS, shadow-PT, naive), suspended wavefront rays carry their long stacks through HBM records exactly, and
PathTraceDR's three schedules agree with each other and with the oracle. Measured depths and witness counts: profiles/deep_stacks.md."""
import os
import re

import numpy as np
import pytest

from conftest import assert_pixel_parity
from hydracore3_amd.scene import INTEGRATOR_MIS_PT, INTEGRATOR_SHADOW_PT
from traversal_scenes import (NESTED_FAMILIES, NO_HIT, assert_hits_equal, nested_rays, nested_sheets, reference_hits, with_tfar, world_triangles)

LDS_STACK = 16
# test_interior_frame_matches_oracle allows 2 divergent pixels and 8 over the bar in 15 360; scaled to 96 x 64 = 6 144 and rounded up (0.8 -> 1,
# 3.2 -> 4); both far below 1 % of the pixels (61)
FRAME_MAX_DIVERGENT, FRAME_MAX_OVER = 1, 4


def _rays(sc, cpu, n, seed, near=0.5):
    pos, dr, fam = nested_rays(sc, n, seed, near)
    h = cpu.ray_nearest(pos, dr, brute=True)
    return pos, with_tfar(pos, dr, np.where(h["instId"] != NO_HIT, h["t"], np.inf), seed + 1), fam


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("instances", [1, 8])
def test_oracle_bvh_and_brute_force_agree_with_float64_on_nested_sheets(instances):
    """ray_nearest / ray_any with brute=False equal brute=True bit for bit on the nested-sheet rays; on the rays whose float64 answer is robust
    (instId, primId) and t (1e-4 relative) equal the float64 reference. More than a quarter of the rays are robust, hits and misses among them."""
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(1500, 1.008, instances=instances) if instances == 1 else nested_sheets(200, 1.06, instances=instances)
    cpu = OracleIntegrator(sc)
    pos, dr, fam = _rays(sc, cpu, 1536, 5 + instances)
    hb, hn = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_nearest(pos, dr, brute=False)
    ab, an = cpu.ray_any(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=False)
    assert np.array_equal(ab != 0, hb["instId"] != NO_HIT)
    assert_hits_equal(hn, hb, "oracle BVH vs brute force")
    assert np.array_equal(an, ab)
    tris, ids = world_triangles(sc)
    hit, t, inst, prim, robust = reference_hits(tris, ids, sc.inst_matrices, pos, dr, chunk=256)
    print(f"nested sheets x {instances}: {robust.mean():.1%} robust, {int((robust & hit).sum())} robust hits, {int((robust & ~hit).sum())} robust misses, "
          f"per family: {[f'{f} {robust[fam == i].mean():.0%}' for i, f in enumerate(NESTED_FAMILIES)]}")
    assert robust.mean() > 0.25 and (robust & hit).sum() > 50 and (robust & ~hit).sum() > 50
    r = np.flatnonzero(robust)
    got = hb["instId"][r] != NO_HIT
    bad = r[got != hit[r]]
    assert bad.size == 0, f"hit / miss differs from float64 on {bad.size} robust rays, first {bad[:8]}"
    rh = r[hit[r]]
    assert np.array_equal(hb["instId"][rh].astype(np.int64), inst[rh]) and np.array_equal(hb["primId"][rh].astype(np.int64), prim[rh])
    assert np.all(np.abs(hb["t"][rh] - t[rh]) <= 1e-4 * np.maximum(np.abs(t[rh]), 1.0) + 1e-6 * np.abs(pos[rh, :3]).max(axis=1))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
def _stack_bounds(log):
    """The stack bounds CommitScene prints under HPT_DEBUG_ACCEL: (BVH2 or two-level walk, 4-wide walk or 0)."""
    two = [int(m) for m in re.findall(r"(?:two-level|single-level) BVH: .*?stack (\d+)", log)]
    wide = [int(m) for m in re.findall(r"4-wide tree: .*?stack bound (\d+)", log)]
    for d, d4 in re.findall(r"device-built single-level BVH: \d+ triangles, depth (\d+),.*?4-wide: \d+ nodes, depth (\d+)", log):
        two.append(int(d) + 1); wide.append(3 * int(d4) + 1)
    assert two, log
    return two[-1], (wide[-1] if wide else 0)


def _witness(g, what):
    words, filled = g.stack_witness()
    print(f"[deep stacks] {what}: {words} of {filled} words of the HBM part written")
    assert filled > 0 and words > 0, f"{what}: no lane pushed beyond the LDS part of its stack ({words} of {filled} words written)"
    return words


@pytest.fixture(scope="module")
def query_case():
    """Scene, rays and the oracle's brute-force answers, once for the ray-query variants."""
    from oracle.orc import OracleIntegrator
    out = {}
    for instances in (1, 8):
        # (one instance: 20 000 sheets - the BVH2 walk of the 8 000-sheet scene passes 16 entries on too few lanes for the 5 % bar: 2.6 % measured)
        sc = nested_sheets(20000, 1.0006) if instances == 1 else nested_sheets(4000, 1.003, instances=8)
        cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
        pos, dr, _ = _rays(sc, cpu, 8192, 31 + instances, near=0.8)
        hb, ab = cpu.ray_nearest(pos, dr, brute=True), cpu.ray_any(pos, dr, brute=True)
        assert 0.2 < (hb["instId"] != NO_HIT).mean() < 0.8
        out[instances] = (sc, pos, dr, hb, ab)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("instances", [1, 8])
@pytest.mark.parametrize("config", ["layout 1", "layout 2", "layout 2 bvh2", "automatic", "layout 2 device-built"])
def test_ray_queries_on_deep_trees(query_case, config, instances, monkeypatch, capfd):
    """RayQuery_NearestHit / AnyHit == the oracle's brute force bit for bit where the stacks outgrow LDS; after each query the witness shows that
    at least 5 % of the rays' lanes wrote to HBM: a lane writes at most (stack bound of the tree it walks - 16) words - the bound CommitScene
    prints under HPT_DEBUG_ACCEL - so words / that bounds the lanes from below."""
    from hydracore3_amd.api import HipIntegrator
    sc, pos, dr, hb, ab = query_case[instances]
    monkeypatch.setenv("HPT_DEBUG_ACCEL", "1")
    g = HipIntegrator(sc, accel_layout={"layout 1": 1, "automatic": 0}.get(config, 2))
    if config == "layout 2 bvh2":
        g.set_option("wide_nodes", 0)
    if config == "layout 2 device-built":
        g.set_option("device_build", 1); g.CommitScene()
        if not g.commit_time()["device_built"]:
            pytest.skip("the device builder declined this scene (tree deeper than the traversal stack): the host build took over")
    log = capfd.readouterr().err
    two, wide = _stack_bounds(log)
    walked = two if config in ("layout 1", "layout 2 bvh2") else max(two, wide)
    what = f"nested sheets x {instances}, {config}"
    print(f"[deep stacks] {what}: stack bounds {two} (BVH2) / {wide} (4-wide); " + " | ".join(l.split("] ", 1)[-1] for l in log.splitlines() if "hydra_hip" in l))
    assert walked > LDS_STACK, (two, wide)       # (the host's trees stop at MAX_STACK; the device builder's 4-wide bound may pass it: the HBM part is sized by it)
    g.set_option("dbg_stack_witness", 1)
    assert_hits_equal(g.RayQuery_NearestHit(pos, dr), hb, what)
    w = _witness(g, what + ", nearest hit")
    lanes = w / (walked - LDS_STACK)
    print(f"[deep stacks] {what}: at least {lanes:.0f} of {pos.shape[0]} lanes ({lanes / pos.shape[0]:.1%}) wrote to HBM")
    assert lanes >= 0.05 * pos.shape[0], f"{what}: {w} words at <= {walked - LDS_STACK} per lane: fewer than 5 % of {pos.shape[0]} lanes may have written"
    a = g.RayQuery_AnyHit(pos, dr)
    bad = np.flatnonzero(a != ab)
    assert bad.size == 0, f"{what}: any-hit differs on {bad.size} rays, first {bad[:8]}"
    _witness(g, what + ", any hit")
    g.set_option("dbg_stack_witness", 0)
    assert g.stack_witness() == (0, 0)
    assert_hits_equal(g.RayQuery_NearestHit(pos, dr), hb, what + " (witness off)")
    assert g.stack_witness() == (0, 0)


def _render(sc, prm, layout, schedule, naive, groups=0):
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator(sc, prm, accel_layout=layout)
    g.set_schedule(schedule, 0, 0, groups)
    g.set_option("dbg_stack_witness", 1)
    return g, g.render(4, naive=naive)


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("integ,naive", [(INTEGRATOR_MIS_PT, False), (INTEGRATOR_SHADOW_PT, False), (INTEGRATOR_MIS_PT, True)])
def test_frames_equal_across_layouts_and_schedules(integ, naive, spectral):
    """96 x 64 at 4 spp: layout 2 under the megakernel == layout 1 under it; schedules 2 (1 and 3 groups), 3 and 4 on either layout == that frame,
    frame and generators bit for bit; every launch reports its schedule and an HBM part and wrote to it. The naive integrator runs under the
    megakernel only and the streaming schedule takes the 4-wide tree of RGB scenes only: where a schedule declines, the launch reports the one it
    fell back to. The megakernel's MIS frame is held to the oracle per pixel."""
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(spectral=spectral)
    prm = sc.params(integ)
    ref, img = _render(sc, prm, 1, 1, naive)
    assert img[..., :3].mean() > 0
    ll = ref.last_launch()
    assert ll["schedule"] == 1 and ll["deep_stack"] and not ll["wide_nodes"], ll
    _witness(ref, f"frame: layout 1, schedule 1, integrator {integ}, naive {naive}, spectral {spectral}")
    for layout in (1, 2):
        for schedule, groups in ((1, 0), (2, 1), (2, 3), (3, 0), (4, 0)):
            if (layout, schedule) == (1, 1) or (spectral and schedule == 4):
                continue
            what = f"frame: layout {layout}, schedule {schedule} ({groups} groups), integrator {integ}, naive {naive}, spectral {spectral}"
            g, out = _render(sc, prm, layout, schedule, naive, groups)
            ll = g.last_launch()
            # what each request runs: the naive integrator is the megakernel's (the spectral block-local kernel has a naive form too); the streaming
            # schedule needs a 4-wide tree (single-level layout): elsewhere it declines
            if naive and not (spectral and schedule == 3):
                expect = 1
            elif schedule == 4 and layout == 1:
                expect = None
            else:
                expect = schedule
            if expect is None:
                assert ll["schedule"] != 4, f"{what}: {ll}"
                print(f"[deep stacks] {what}: schedule 4 declined the scene (no 4-wide tree), schedule {ll['schedule']} ran")
            else:
                assert ll["schedule"] == expect, f"{what}: expected schedule {expect}, {ll}"
            heavy = g.accel_info()["sah_node_visits"] >= 20.0            # (hpt_host.hip: HEAVY_SAH_VISITS - from there the megakernel forms walk the 4-wide tree too)
            assert ll["wide_nodes"] == (layout == 2 and (ll["schedule"] in (2, 4) or heavy)), f"{what}: {ll}, heavy {heavy}"
            assert ll["deep_stack"], f"{what}: {ll}"
            assert np.array_equal(out.view(np.uint32), img.view(np.uint32)), what
            assert np.array_equal(g.random_gens(), ref.random_gens()), what
            _witness(g, what)
    if integ == INTEGRATOR_MIS_PT and not naive and not spectral:
        cpu = OracleIntegrator(sc, prm, threads=len(os.sched_getaffinity(0)))
        assert_pixel_parity(img, cpu.render(4), 4, ref, cpu, max_divergent=FRAME_MAX_DIVERGENT, max_over=FRAME_MAX_OVER, what="nested sheets 96x64 @ 4 spp, layout 1 megakernel: ")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_wavefront_suspension_carries_long_stacks(layout):
    """The settings of test_wavefront_ray_suspension_is_exact (1 trace block per CU, wf_grace 1, instrumented) on the nested sheets: thousands of
    rays are parked with a stack longer than the LDS part ([WF_SUSP_WORDS + stack][maxSusp] records) and resumed; frame and generators equal
    the megakernel's bit for bit."""
    from hydracore3_amd.api import HipIntegrator
    sc = nested_sheets(width=384, height=320)
    mega = HipIntegrator(sc, accel_layout=layout); mega.set_schedule(1)
    ref = mega.render(3)
    wf = HipIntegrator(sc, accel_layout=layout); wf.set_schedule(2, 56, 1, 1); wf.set_option("wf_grace", 1)
    wf.set_instrumentation(True)
    wf.set_option("dbg_stack_witness", 1)
    img = wf.render(3)
    ll = wf.last_launch()
    assert ll["schedule"] == 2 and ll["deep_stack"], ll
    suspended = list(wf.counters().values())[12]
    print(f"[deep stacks] suspension, layout {layout}: {suspended} rays suspended")
    assert suspended > 1000, suspended
    _witness(wf, f"suspension, layout {layout}")
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(wf.random_gens(), mega.random_gens())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_path_trace_dr_on_deep_trees(layout):
    """PathTraceDR with an 8 x 8 registered texture on the textured sheets under schedules 1, 2 and 3: frame and generators bit for bit, loss to
    1e-6, gradient to rtol 1e-5 / atol 1e-7 max (the bars of test_sweep_dr_equals_layout_1); schedule 1's loss and gradient against the oracle's
    at the bars of test_gradient_matches_oracle. Under schedule 3 the gradient staging shares the LDS columns of a stack that continues in HBM."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(width=48, height=32)
    rng = np.random.default_rng(5)
    out = {}
    for schedule in (1, 2, 3):
        g = HipIntegrator(sc, accel_layout=layout)
        g.set_schedule(schedule)
        g.set_option("dbg_stack_witness", 1)
        off, size = g.PutDiffTex2D(1, 8, 8, 4)
        if schedule == 1:
            data = rng.uniform(0.2, 0.9, size).astype(np.float32)
            ref = rng.uniform(0.0, 0.5, (sc.height, sc.width, 4)).astype(np.float32)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        grad = np.zeros_like(data)
        loss = g.PathTraceDR(g.N, 4, img, 4, ref, data, grad)
        ll = g.last_launch()
        assert ll["schedule"] == schedule and ll["deep_stack"], ll
        _witness(g, f"PathTraceDR, layout {layout}, schedule {schedule}")
        out[schedule] = (img, g.random_gens(), loss, grad)
    assert np.count_nonzero(out[1][3]) > 20
    for schedule in (2, 3):
        assert np.array_equal(out[schedule][0].view(np.uint32), out[1][0].view(np.uint32)), schedule
        assert np.array_equal(out[schedule][1], out[1][1]), schedule
        assert out[schedule][2] == pytest.approx(out[1][2], rel=1e-6)
        assert np.allclose(out[schedule][3], out[1][3], rtol=1e-5, atol=1e-7 * np.abs(out[1][3]).max()), schedule
    cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
    assert cpu.put_diff_tex2d(1, 8, 8, 4)[1:] == (0, 8 * 8 * 4)
    out_c = np.zeros((sc.height, sc.width, 4), np.float32)
    loss_c, grad_c = cpu.path_trace_dr(out_c, 4, ref, data)
    err = np.linalg.norm(out[1][3] - grad_c) / np.linalg.norm(grad_c)
    print(f"[deep stacks] PathTraceDR layout {layout}: loss gpu {out[1][2]:.6f} cpu {loss_c:.6f}, relative gradient error {err:.3e}")
    assert abs(out[1][2] - loss_c) <= 1e-4 * abs(loss_c)
    assert err < 1e-2
    big = np.abs(grad_c) > 1e-3 * np.abs(grad_c).max()
    assert np.allclose(out[1][3][big], grad_c[big], rtol=1e-2, atol=1e-5 * np.abs(grad_c).max())


# ---- the one-launch passes: each kernel has its own overflow pointer, stride (gridDim.x * 256) and lane index ---------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _linear_nested(width, height):
    """The nested sheets with their texture flagged linear: no pixel falls under the sRGB-decode exception of the primary-ray tests, so their bar
    here is equality everywhere."""
    sc = nested_sheets(width=width, height=height)
    for t in sc.textures:
        t.srgb = False
    return sc


@pytest.fixture(scope="module")
def primary_case():
    """Scene, oracle and the restatements of the primary-ray passes, once for both layouts."""
    import raytrace_reference as RT
    from oracle.orc import OracleIntegrator
    sc = _linear_nested(96, 64)
    cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
    cast = RT.cast_single_ray(sc, cpu)
    whitted = RT.ray_trace(sc, cpu, params=sc.params())
    assert cast["hit"].any() and not cast["srgb"].any() and not whitted["srgb"].any()
    assert whitted["lit"].any()
    return sc, cpu, cast, whitted


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_eval_gbuffer_on_deep_trees(layout):
    """EvalGBuffer == gbuffer_reference.py at the bars of test_gbuffer_gpu.py: raw samples and the reduced frame equal bit for bit (r, g, b behind
    the sRGB texture to 2 ulp), the frame equal to the restatement's reduction of the GPU's own samples."""
    import gbuffer_reference as R
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = nested_sheets(width=48, height=32)
    cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
    ref_frame, ref_raw = R.eval_gbuffer(sc, cpu)
    g = HipIntegrator(sc, accel_layout=layout)
    g.set_option("dbg_stack_witness", 1)
    frame, raw = g.EvalGBuffer(samples=True)
    _witness(g, f"EvalGBuffer, layout {layout}")
    assert (ref_raw["instId"] >= 0).any()
    R.assert_records_equal(raw, ref_raw, "nested sheets: raw samples", rgb_2ulp=R.srgb_textured(sc, ref_raw))
    own, _ = R.reduce_samples(raw, sc.width, sc.height)
    R.assert_records_equal(frame, R.scatter(own, g.packed_xy(), sc.width, sc.height), "nested sheets: frame vs reduction of the GPU's samples")
    loose = R.scatter(R.srgb_textured(sc, ref_raw).any(axis=1), cpu.packed_xy(), sc.width, sc.height, np.zeros((sc.height, sc.width), bool))
    R.assert_records_equal(frame, ref_frame, "nested sheets: frame vs restatement", rgb_2ulp=loose)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_cast_single_ray_and_ray_trace_on_deep_trees(primary_case, layout):
    """CastSingleRayBlock and RayTraceBlock (the scene's trace depth, 4 channels) == raytrace_reference.py bit for bit, the bar test_raytrace_gpu.py
    holds for pixels that read no sRGB texel - here all of them."""
    from hydracore3_amd.api import HipIntegrator
    sc, cpu, cast, whitted = primary_case
    g = HipIntegrator(sc, sc.params(), accel_layout=layout)
    g.set_option("dbg_stack_witness", 1)
    xy = g.packed_xy()
    assert np.array_equal(xy, cpu.packed_xy())
    out = np.full((sc.height, sc.width, 4), 0xDEADBEEF, np.uint32).view(np.float32)
    g.CastSingleRayBlock(g.N, out)
    _witness(g, f"CastSingleRayBlock, layout {layout}")
    bad = int(np.any(_bits(out) != _bits(cast["frame"]), axis=-1).sum())
    assert bad == 0, f"CastSingleRayBlock, layout {layout}: {bad} pixels differ"
    out = np.zeros((sc.height, sc.width, 4), np.float32)
    g.RayTraceBlock(g.N, 4, out)
    _witness(g, f"RayTraceBlock, layout {layout}")
    want = np.zeros_like(out)
    want[(xy >> 16) & 0xFFFF, xy & 0xFFFF, :3] = whitted["accum"]
    bad = int(np.any(_bits(out) != _bits(want), axis=-1).sum())
    assert bad == 0, f"RayTraceBlock, layout {layout}: {bad} pixels differ"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_ray_trace_dr_on_deep_trees(layout):
    """RayTraceDR with the 8 x 8 texture registered: colours of the hit pixels and the returned loss == raytrace_dr_reference.py bit for bit, missed
    pixels untouched (the bars of test_colours_and_losses_equal_the_restatement)."""
    import raytrace_dr_reference as DR
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = _linear_nested(96, 64)                          # (the restatement takes linear textures only)
    cpu = OracleIntegrator(sc, threads=len(os.sched_getaffinity(0)))
    rng = np.random.default_rng(5)
    data = rng.uniform(0.2, 0.9, 8 * 8 * 4).astype(np.float32)
    ref = rng.uniform(0.0, 0.5, (sc.height, sc.width, 4)).astype(np.float32)
    f32 = DR.ray_trace_dr(sc, cpu, {1: (0, 8, 8, 4)}, data, ref, pass_num=3)
    hit = f32["hit"]
    assert hit.any() and (~hit).any()
    g = HipIntegrator(sc, accel_layout=layout)
    g.set_option("dbg_stack_witness", 1)
    assert tuple(g.PutDiffTex2D(1, 8, 8, 4)) == (0, 8 * 8 * 4)
    frame = np.full((sc.height, sc.width, 4), -7.5, np.float32)
    grad = np.zeros_like(data)
    loss = g.RayTraceDR(g.N, 4, frame, 3, ref, data, grad)
    _witness(g, f"RayTraceDR, layout {layout}")
    xy = g.packed_xy()
    y, x = (xy >> 16) & 0xFFFF, xy & 0xFFFF
    assert np.array_equal(_bits(frame[y[hit], x[hit], :3]), _bits(f32["color"][hit])), "colours of hit pixels"
    assert np.all(frame[y[~hit], x[~hit]] == np.float32(-7.5)), "a missed pixel of out_color was written"
    assert np.float32(loss).view(np.uint32) == np.float32(f32["loss"]).view(np.uint32), (loss, f32["loss"])


# ---- the QMC, PSS and KMLT kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_qmc_per_sample_colours_on_deep_trees(layout):
    """PathTraceBlockQMC on the emissive nested sheets: the per-sample colours == the oracle's, bit for bit (test_qmc_gpu.py's helper and bar)."""
    import qmc_reference as Q
    from hydracore3_amd import api
    from test_qmc_gpu import _oracle_colours, _table
    w, h, spp = 48, 32, 4
    sc = nested_sheets(width=w, height=h, emissive=True)
    params = sc.params()
    g = api.HipIntegrator(sc, params, accel_layout=layout)
    g.set_option("dbg_stack_witness", 1)
    _, col, pix = g.render_qmc(spp, frame=False, records=True)
    _witness(g, f"PathTraceBlockQMC, layout {layout}")
    want, raw = _oracle_colours(sc, params, False, 0, w * h * spp)
    _, _, wpix = Q.sample_pixels(_table(), w * h * spp, w, h)
    assert np.array_equal(pix, wpix)
    hits = int(np.sum(np.any(raw[:, :3] != np.asarray(sc.env_color[:3], np.float32), axis=1)))
    assert hits > (w * h * spp) // 4, f"only {hits} samples see the sheets"
    diff = np.flatnonzero(np.any(col[:, :3].view(np.uint32) != want.view(np.uint32), axis=1))
    assert diff.size == 0, (diff[:8], col[diff[:4]], want[diff[:4]])
    assert len(np.unique(col[:, :3], axis=0)) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 2])
def test_pss_and_kmlt_on_deep_trees(layout):
    """hpt_path_trace_pss_dev == one PathTraceBlock pass bit for bit (test_kmlt_gpu.py's helper); one short KMLT run (64 chains x 32 steps) replayed
    from the device's own records: the recorded colours and pixels are F of the recorded proposals, and acceptance, compared pixel and step kind
    equal the restatement fed with those records."""
    import kmlt_reference as K
    from test_kmlt_gpu import CHAINS, STEPS, _base_vectors, _integ, _pss_equals_one_pass
    sc = nested_sheets(width=32, height=32)
    sc.trace_depth = 3
    g = _integ(sc, layout=layout)
    g.set_option("dbg_stack_witness", 1)
    x, _ = _base_vectors(g)
    g.path_trace_pss(x)
    _witness(g, f"primary-sample-space pass, layout {layout}")
    _pss_equals_one_pass(g)
    g = _integ(sc, layout=layout)
    g.set_option("dbg_stack_witness", 1)
    n = K.state_size(3)
    r = g.render_kmlt(2, chains=CHAINS, normalize=True, records=True, proposals=True)
    _witness(g, f"PathTraceBlockKMLT, layout {layout}")
    assert (r["chains"], r["steps"]) == (CHAINS, STEPS) and r["proposals"].shape == (CHAINS, STEPS, n)
    ref = K.run_chains(CHAINS, STEPS, n, (32, 32), recorded=r)
    col, pix = g.path_trace_pss(r["proposals"].reshape(-1, n))
    assert np.array_equal(col.view(np.uint32), r["color"].reshape(-1, 4).view(np.uint32))
    assert np.array_equal(pix, r["pixel"].reshape(-1))
    col0, pix0 = g.path_trace_pss(ref["init"])
    assert np.array_equal(col0.view(np.uint32), r["initColor"].view(np.uint32)) and np.array_equal(pix0, r["initPixel"])
    assert np.array_equal(r["isLarge"].astype(bool), ref["isLarge"])
    assert np.array_equal(r["a"].view(np.uint32), ref["a"].view(np.uint32))
    assert np.array_equal(r["accepted"].astype(bool), ref["accepted"])
    assert np.array_equal(r["oldPixel"], ref["oldPixel"])
    assert 0 < ref["accepted"].sum() < ref["accepted"].size

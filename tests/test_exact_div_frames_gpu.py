"""The sweep kernels with the replayed division (hpt_device.h: rcpIeee2 in traceSweep's triangle tests) against what the commit before it
(f3e96ac) computed, bit for bit.

The goldens under tests/golden/exact_div/ were written by THAT commit's library on an MI355X (`HYDRA_HIP_LIB=<library of f3e96ac> python
tests/test_exact_div_frames_gpu.py <dir>` runs this file's own renderers and saves what they return, after checking that the parent gives one
frame for every option set below):

  cornell_frame.npy, cornell_gens.npy   the Cornell box (test_035) at 64 x 64, 16 spp, through the sweep megakernel: RGB of the frame and the
                                        generators after the call (uint32, N x 2). The parent gave the same words with whole pixels and with
                                        pass_slice 4, with sweep_lanes 0 and 1, so the one pair of files serves the four cases
  branch_frame.npy, branch_gens.npy     synth.gltf_branch_scene at 64 x 64, 8 spp: waves that mix GGX and Lambert lobes, an emitter bound to a light
  hits.npy                              RayQuery_NearestHit / AnyHit of the sweep layout on traversal_scenes.sweep_scene(11) and 3000 rays of
                                        make_rays(seed 31) (edges, vertices, grazing, degenerate triangles: determinants at and near zero), tfar
                                        from with_tfar on the oracle's brute-force t; uint32 (3000, 7): t, primId, instId, geomId, u, v as words, any-hit
"""
import os
import sys

import numpy as np
import pytest

from conftest import scene_path
from hydracore3_amd import synth
from hydracore3_amd.scene import load_hydra_xml
from traversal_scenes import NO_HIT, make_rays, sweep_scene, with_tfar, world_triangles

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_div")
W = H = 64
CORNELL_SPP, BRANCH_SPP = 16, 8
N_RAYS = 3000
CORNELL_CASES = [(0, None), (4, None), (0, 0), (0, 1)]           # (pass_slice, sweep_lanes; None: the default)


def render(sc, spp, pass_slice=0, sweep_lanes=None):
    """(frame[..., :3], generators after the call) of one PathTraceBlock call through the sweep megakernel."""
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(sc)
    assert gpu.accel_info()["layout"] == "sweep"
    gpu.set_schedule(1)
    gpu.set_option("pass_slice", pass_slice)
    if sweep_lanes is not None:
        gpu.set_option("sweep_lanes", sweep_lanes)
    img = gpu.render(spp)
    assert gpu.last_schedule()[0] == 1 and gpu.last_launch()["pass_slice"] == pass_slice
    return np.ascontiguousarray(img[..., :3]), gpu.random_gens()


def cornell():
    return load_hydra_xml(scene_path("test_035"), W, H)


def query_hits(sweep_lanes):
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = sweep_scene(11)
    tris, _ = world_triangles(sc)
    pos, dr, _ = make_rays(tris, N_RAYS, 31)
    h = OracleIntegrator(sc).ray_nearest(pos, dr, brute=True)
    dr = with_tfar(pos, dr, np.where(h["instId"] != NO_HIT, h["t"], np.inf), 32)
    gpu = HipIntegrator(sc)
    assert gpu.accel_info()["layout"] == "sweep"
    gpu.set_option("sweep_lanes", sweep_lanes)
    n, a = gpu.RayQuery_NearestHit(pos, dr), gpu.RayQuery_AnyHit(pos, dr)
    hit = n["geomId"] != NO_HIT
    uv = np.where(hit[:, None], np.ascontiguousarray(n["coords"][:, :2], np.float32).view(np.uint32), 0)   # (a miss leaves its coordinates unset)
    return np.column_stack([np.ascontiguousarray(n["t"], np.float32).view(np.uint32), n["primId"], n["instId"], n["geomId"], uv,
                            np.asarray(a).astype(np.uint32)]).astype(np.uint32)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_equal_the_parents(frame, gens, name, what):
    gf, gg = np.load(os.path.join(GOLDEN, f"{name}_frame.npy")), np.load(os.path.join(GOLDEN, f"{name}_gens.npy"))
    assert np.isfinite(frame).all() and frame.mean() > 0
    diff = words(frame) != words(gf)
    assert not diff.any(), f"{what}: {int(diff.any(-1).sum())} pixels differ from the parent's frame, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(gens, gg), f"{what}: {int(np.any(gens != gg, axis=1).sum())} generators differ from the parent's"


@pytest.mark.parametrize("pass_slice,sweep_lanes", CORNELL_CASES)
def test_cornell_frame_and_generators_equal_the_parents(pass_slice, sweep_lanes):
    frame, gens = render(cornell(), CORNELL_SPP, pass_slice, sweep_lanes)
    assert_equal_the_parents(frame, gens, "cornell", f"pass_slice {pass_slice}, sweep_lanes {sweep_lanes}")


def test_mixed_lobes_and_bound_emitter_equal_the_parents():
    frame, gens = render(synth.gltf_branch_scene(W, H, False), BRANCH_SPP)
    assert_equal_the_parents(frame, gens, "branch", "branch scene")


@pytest.mark.parametrize("sweep_lanes", [0, 1])
def test_sweep_ray_queries_equal_the_parents(sweep_lanes):
    got, want = query_hits(sweep_lanes), np.load(os.path.join(GOLDEN, "hits.npy"))
    assert (want[:, 3] != NO_HIT).mean() > 0.2 and want[:, 6].any()
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, f"sweep_lanes {sweep_lanes}: {bad.size} rays differ from the parent's, first {bad[:8]}: {got[bad[:2]]} vs {want[bad[:2]]}"


SWITCH_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import test_exact_div_frames_gpu as t
from hydracore3_amd import api, synth
assert api.LIB_PATH.endswith("libhydra_hip_exactdiv0.so")
for ps, sl in t.CORNELL_CASES:
    t.assert_equal_the_parents(*t.render(t.cornell(), t.CORNELL_SPP, ps, sl), "cornell", f"switch off, pass_slice {ps}, sweep_lanes {sl}")
t.assert_equal_the_parents(*t.render(synth.gltf_branch_scene(t.W, t.H, False), t.BRANCH_SPP), "branch", "switch off, branch scene")
for sl in (0, 1):
    assert np.array_equal(t.query_hits(sl), np.load(t.os.path.join(t.GOLDEN, "hits.npy"))), f"switch off, ray queries, sweep_lanes {sl}"
print("switch off: equal")
"""


def test_library_built_with_the_switch_off_gives_the_same_files():
    """-DHPT_EXACT_DIV_FAST=0 (build(): libhydra_hip_exactdiv0.so, the units under test with the helpers as plain expressions): every case above
    again, in a child process that loads that library through HYDRA_HIP_LIB."""
    import subprocess
    import __graft_entry__ as g
    assert os.path.exists(g.EXACT_DIV_SWITCH_LIB)
    env = dict(os.environ, HYDRA_HIP_LIB=g.EXACT_DIV_SWITCH_LIB)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", SWITCH_CHILD, g.ROOT, os.path.dirname(os.path.abspath(__file__))],
                       capture_output=True, text=True, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "switch off: equal" in r.stdout


if __name__ == "__main__":
    # writes the goldens with whatever library HYDRA_HIP_LIB names (the parent commit's), after checking that every option set gives one frame
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    f0, g0 = render(cornell(), CORNELL_SPP)
    for ps, sl in CORNELL_CASES:
        f, g = render(cornell(), CORNELL_SPP, ps, sl)
        same = np.array_equal(words(f), words(f0)) and np.array_equal(g, g0)
        print(f"cornell, pass_slice {ps}, sweep_lanes {sl}: equal to the default's: {same}", flush=True)
        assert same
    fb, gb = render(synth.gltf_branch_scene(W, H, False), BRANCH_SPP)
    fb2, gb2 = render(synth.gltf_branch_scene(W, H, False), BRANCH_SPP)
    h0, h1 = query_hits(0), query_hits(1)
    print("branch scene repeats:", np.array_equal(words(fb), words(fb2)) and np.array_equal(gb, gb2), "ray queries, sweep_lanes 0 == 1:", np.array_equal(h0, h1),
          "hits", float((h0[:, 3] != NO_HIT).mean()), "occluded", float(h0[:, 6].mean()), flush=True)
    assert np.array_equal(words(fb), words(fb2)) and np.array_equal(gb, gb2) and np.array_equal(h0, h1)
    np.save(os.path.join(out, "cornell_frame.npy"), f0); np.save(os.path.join(out, "cornell_gens.npy"), g0)
    np.save(os.path.join(out, "branch_frame.npy"), fb); np.save(os.path.join(out, "branch_gens.npy"), gb)
    np.save(os.path.join(out, "hits.npy"), h0)
    print("mean radiance: cornell", float(f0.mean()) / CORNELL_SPP, "branch", float(fb.mean()) / BRANCH_SPP)

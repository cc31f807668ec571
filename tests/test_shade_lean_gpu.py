"""The shading and regeneration code of the path-tracing kernels against what the commit before the lean rewrite (5b29b65) computed.

gltfSampleAndEvalC chooses its lobe before it evaluates one, and the emissive branch of shadeVertex samples the light's texture only where the
value is read. Neither may move a bit of a frame, a generator, a loss or a gradient. The goldens
under tests/golden/shade_lean/ were written by THAT commit's library on an MI355X (`HYDRA_HIP_LIB=<library of 5b29b65> python
tests/test_shade_lean_gpu.py <dir>` runs this file's own renderers and saves what they return):

  frame.npy     the 64 x 64 x 3 frame of `branch_scene` (8 spp, depth 5) under the megakernel; the parent's wavefront and block-local schedules
                gave the same words, so the one file is the parent's output for schedules 1, 2 and 3
  gens.npy      the generators after that call (uint32, N x 2)
  spectral.npy  the same frame through the spectral kernel, as check words (see `check_words`): with the full frame the directory would pass
                the 100 KB it may hold; every word of the frame enters a row sum, a row xor and a position-weighted row sum, and their column counterparts
  dr_loss.npy, dr_grad.npy  PathTraceDR on the test_228 class, 32 x 32 at 4 spp, 16 x 16 x 4 albedo (see `render_dr`)
"""
import os
import sys

import numpy as np
import pytest

from conftest import scene_path, pixel_errors, assert_pixel_parity
from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.synth import dr_scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_lean")
W = H = 64
SPP = 8


def branch_scene(spectral=False):
    return synth.gltf_branch_scene(W, H, spectral)


def render_rgb(schedule):
    """(frame[..., :3], generators after the call, the schedule the call ran). The scene is small enough for the triangle sweep, which the
    megakernel and the wavefront pair take; the block-local schedule has no sweep form, so it renders the single-level layout."""
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(branch_scene(), accel_layout=2 if schedule == 3 else 0)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    img = gpu.render(SPP)
    return np.ascontiguousarray(img[..., :3]), gpu.random_gens(), gpu.last_schedule()[0]


def render_spectral():
    from hydracore3_amd.api import HipIntegrator
    return np.ascontiguousarray(HipIntegrator(branch_scene(spectral=True)).render(SPP)[..., :3])


def check_words(frame):
    """(6, 64) uint64 of a 64 x 64 x 3 float32 frame's words: per row the sum, the xor and the sum weighted by the position in the row, then the
    same per column. One changed word changes its row's and its column's sum; changes that cancel in all six would have to be constructed."""
    w = np.ascontiguousarray(frame, np.float32).view(np.uint32).astype(np.uint64)          # (H, W, 3)
    out = []
    for v in (w.reshape(w.shape[0], -1), w.transpose(1, 0, 2).reshape(w.shape[1], -1)):    # rows, then columns
        k = np.arange(1, v.shape[1] + 1, dtype=np.uint64)
        out += [v.sum(1, dtype=np.uint64), np.bitwise_xor.reduce(v, 1), (v * k).sum(1, dtype=np.uint64)]
    return np.stack(out)


DR_W = DR_H = 32
DR_SPP, DR_TEX = 4, 16


def render_dr():
    """hpt_path_trace_dr_dev on the test_228 class. The gradient is scattered with float atomics and the loss is one atomic per wave, so a call
    over the whole frame sums in the order its waves happen to finish. A window of 64 tids is fetched by ONE wave (the first to reach the queue
    takes all 64), whose own order is fixed: the frame is rendered as 16 such windows. Returns (loss per window (16,), the windows' gradients
    summed in window order in float64 (a sum of sixteen float32 is exact there unless their exponents lie more than 29 bits apart))."""
    from hydracore3_amd.api import HipIntegrator
    sc, tex_id = dr_scene(scene_path("test_228"), DR_W, DR_H, tex_size=DR_TEX)
    gpu = HipIntegrator(sc)
    gpu.set_schedule(1)
    off, size = gpu.PutDiffTex2D(tex_id, DR_TEX, DR_TEX, 4)
    assert (off, size) == (0, DR_TEX * DR_TEX * 4)
    yy, xx = np.mgrid[0:DR_H, 0:DR_W]
    ref = np.zeros((DR_H, DR_W, 4), np.float32)
    ref[..., 0] = 0.2 + 0.5 * ((xx // 4 + yy // 4) % 2)
    ref[..., 1] = 0.1 + xx / 64.0
    ref[..., 2] = 0.4 - yy / 128.0
    data = np.full((DR_TEX, DR_TEX, 4), 0.5, np.float32)
    ty, tx = np.mgrid[0:DR_TEX, 0:DR_TEX]
    data[..., 0] = 0.3 + tx / 40.0
    data[..., 1] = 0.7 - ty / 40.0
    data[..., 3] = 1.0
    dframe, dref, ddata = (gpu.dev_array(a) for a in (np.zeros((DR_H, DR_W, 4), np.float32), ref, data.reshape(-1)))
    dgrad, dloss = gpu.dev_array(np.zeros(size, np.float32)), gpu.dev_array(np.zeros(1, np.float32))
    losses, grad = [], np.zeros(size, np.float64)
    for w in range(DR_W * DR_H // 64):
        gpu.PathTraceDR_dev(dframe, DR_SPP, dref, ddata, dgrad, dloss, tid_begin=64 * w, tid=64)
        losses.append(dloss.download()[0])
        grad += dgrad.download().astype(np.float64)
    return np.asarray(losses, np.float32), grad


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.fixture(scope="module")
def megakernel():
    return render_rgb(1)


def test_branch_scene_holds_every_case():
    """The host's view of the scene: the lean kernels take it (gltf and emissive only), and the material table holds the eight cases."""
    sc = branch_scene()
    assert all(int(m["mtype"]) in (S.MAT_TYPE_GLTF, S.MAT_TYPE_LIGHT_SOURCE) for m in sc.materials)
    d = [(float(m["data"][S.GLTF_FLOAT_ALPHA]), 1.0 - float(m["data"][S.GLTF_FLOAT_GLOSINESS]), float(m["data"][S.GLTF_FLOAT_REFL_COAT]),
          float(m["data"][S.GLTF_FLOAT_IOR])) for m in sc.materials[:8]]
    assert d[0][0] == 0 and d[0][2] == 0 and d[0][3] == 0                                   # Lambert: diffuse lobe, f_i unread
    assert d[1][0] == 1 and d[2][:2] == (0.5, 0.0) and d[3][0] == 0.5 and abs(d[3][1] - 0.4) < 1e-6
    assert d[4][2] == 1 and d[4][3] == 1.5 and d[5][2] == 1 and d[5][3] == 0 and d[6][3] == 0
    lit, unlit = sc.materials[8], sc.materials[9]
    assert int(lit["lightId"]) == 0 and int(unlit["lightId"]) == S.UINT_MAX and int(lit["texid"][0]) == int(unlit["texid"][0]) != 0


def test_frame_and_generators_equal_the_parents(megakernel):
    frame, gens, sched = megakernel
    assert sched == 1
    assert np.isfinite(frame).all() and frame.mean() > 0
    gf, gg = np.load(os.path.join(GOLDEN, "frame.npy")), np.load(os.path.join(GOLDEN, "gens.npy"))
    diff = words(frame) != words(gf)
    assert not diff.any(), f"{int(diff.any(-1).sum())} pixels differ from the parent's frame, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(gens, gg), f"{int(np.any(gens != gg, axis=1).sum())} generators differ from the parent's"


@pytest.mark.parametrize("schedule", [2, 3])
def test_other_schedules_equal_the_parents(schedule):
    frame, gens, sched = render_rgb(schedule)
    assert sched == schedule
    assert np.array_equal(words(frame), words(np.load(os.path.join(GOLDEN, "frame.npy"))))
    assert np.array_equal(gens, np.load(os.path.join(GOLDEN, "gens.npy")))


def test_spectral_frame_equals_the_parents():
    frame = render_spectral()
    assert np.isfinite(frame).all() and frame.mean() > 0
    got, want = check_words(frame), np.load(os.path.join(GOLDEN, "spectral.npy"))
    assert np.array_equal(got, want), f"rows {np.flatnonzero(np.any(got[:3] != want[:3], 0))}, columns {np.flatnonzero(np.any(got[3:] != want[3:], 0))} differ"


def test_frame_matches_the_cpu_oracle():
    """The tolerance tests/test_gpu_parity.py holds the Cornell box to (assert_pixel_parity's defaults: every pixel under 1e-3, no divergent
    generator, RMS of the pixels under the bar below 1e-4). The parent commit's library on this scene, measured on an MI355X: largest per-pixel
    L2 1.857e-05, no pixel at or over the bar, no divergent generator, RMS 2.95e-07, 75.4 % of the pixels bit-identical with the oracle's."""
    from hydracore3_amd.api import HipIntegrator
    from oracle.orc import OracleIntegrator
    sc = branch_scene()
    gpu, cpu = HipIntegrator(sc), OracleIntegrator(sc)
    img_g, img_c = gpu.render(SPP), cpu.render(SPP)
    print(f"largest per-pixel L2 against the oracle: {float(pixel_errors(img_g, img_c, SPP).max()):.3e}")
    assert_pixel_parity(img_g, img_c, SPP, gpu, cpu, max_divergent=0, what=f"branch_scene {W}x{H} @ {SPP} spp: ")


def test_dr_loss_and_gradient_equal_the_parents():
    losses, grad = render_dr()
    assert np.isfinite(grad).all() and np.count_nonzero(grad) > 100 and (losses > 0).all()
    gl, gg = np.load(os.path.join(GOLDEN, "dr_loss.npy")), np.load(os.path.join(GOLDEN, "dr_grad.npy"))
    assert np.array_equal(words(losses), words(gl)), (losses, gl)
    bad = np.flatnonzero(words(grad) != words(gg))
    assert bad.size == 0, f"{bad.size} gradient elements differ from the parent's, first {bad[0]}: {grad[bad[0]]!r} vs {gg[bad[0]]!r}"


if __name__ == "__main__":
    # writes the goldens with whatever library HYDRA_HIP_LIB names (the parent commit's), after checking that it repeats itself
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    f1, g1, _ = render_rgb(1)
    for s in (1, 2, 3):
        f, g, ran = render_rgb(s)
        same = ran == s and np.array_equal(words(f), words(f1)) and np.array_equal(g, g1)
        print(f"schedule {s} (ran {ran}): frame and generators equal to the megakernel's: {same}", flush=True)
        if not same:                                                    # (never seen: the one frame.npy then would not do for this schedule)
            np.save(os.path.join(out, f"frame_s{s}.npy"), f); np.save(os.path.join(out, f"gens_s{s}.npy"), g)
    sp, sp2 = render_spectral(), render_spectral()
    l1, d1 = render_dr()
    l2, d2 = render_dr()
    np.save(os.path.join(out, "frame.npy"), f1); np.save(os.path.join(out, "gens.npy"), g1)
    np.save(os.path.join(out, "spectral.npy"), check_words(sp))
    np.save(os.path.join(out, "dr_loss.npy"), l1); np.save(os.path.join(out, "dr_grad.npy"), d1)
    print("mean radiance", float(f1.mean()) / SPP, "spectral", float(sp.mean()) / SPP, "nonzero gradient elements", int(np.count_nonzero(d1)), "losses", l1)
    print("spectral repeats:", np.array_equal(words(sp), words(sp2)), "DR windows repeat:", np.array_equal(words(l1), words(l2)), np.array_equal(words(d1), words(d2)), flush=True)
    assert np.array_equal(words(sp), words(sp2)) and np.array_equal(words(l1), words(l2)) and np.array_equal(words(d1), words(d2))

"""The CPU-side figures of tests/test_qmc_gpu.py::test_qmc_converges_to_the_path_tracer_s_image, measured with the oracle alone (no GPU).
usage: python profiles/qmc_convergence_cpu.py [test_035,test_228,dof] [256,1024]
Per scene and spp: the PSNR of the oracle's PathTraceBlock against ITSELF under two generator seeds (8-bit frames as the reference's
testing/run_tests.py compares them: mean over spp, clamped, gamma 2.2, cv2.PSNR's formula), and over eight seeds the RMSE of the linear frame
against a 16 x spp frame of a ninth seed: minimum, maximum and their ratio (the margin of the test's second assert).
Seed k = the generators InitRandomGens gives, rolled by 977 k pixels. Sizes: test_035 and its thin-lens variant (lens radius 0.08) 64 x 64,
test_228 48 x 32 - the sizes of the test."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402
from oracle.orc import OracleIntegrator  # noqa: E402


def scene_path(name):
    return os.path.join(ROOT, "tests", "golden", "scenes", name, "statex_00001.xml")


def ldr(img, spp):
    x = np.clip(img[..., :3].astype(np.float64) / spp, 0.0, 1.0) ** (1.0 / 2.2)
    return np.floor(x * 255.0 + 0.5)


def psnr(a, b):
    mse = np.mean((a - b) ** 2)
    return 10.0 * np.log10(255.0 ** 2 / mse) if mse > 0 else 361.2


def scene(name):
    if name == "dof":
        sc = load_hydra_xml(scene_path("test_035"), 64, 64)
        sc.cam_lens_radius = 0.08
        return sc
    return load_hydra_xml(scene_path(name), *((64, 64) if name == "test_035" else (48, 32)))


names = (sys.argv[1] if len(sys.argv) > 1 else "test_035,test_228,dof").split(",")
spps = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "256").split(",")]
for name in names:
    sc = scene(name)
    cpu = OracleIntegrator(sc)
    g0 = cpu.random_gens().copy()

    def render(seed, spp):
        cpu.set_random_gens(np.roll(g0, seed * 977, axis=0))
        return cpu.render(spp)
    for spp in spps:
        t = time.time()
        fr = [render(k, spp) for k in range(8)]
        ref = render(8, 16 * spp)
        rm = [float(np.sqrt(np.mean((f[..., :3].astype(np.float64) / spp - ref[..., :3].astype(np.float64) / (16 * spp)) ** 2))) for f in fr]
        print(f"{name} spp {spp}: two-seed PSNR {psnr(ldr(fr[0], spp), ldr(fr[1], spp)):.2f} dB; RMSE vs {16 * spp} spp over eight seeds: "
              f"min {min(rm):.5f} max {max(rm):.5f} ratio {max(rm) / min(rm):.3f}; {time.time() - t:.1f} s", flush=True)

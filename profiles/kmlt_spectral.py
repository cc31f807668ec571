"""Figures of profiles/kmlt_spectral.md: chain steps per second of spectral MLT next to spectral QMC's samples per second (second of two calls,
the kernel slot of GetExecutionTime), and the PSNR of a 1024-spp spectral KMLT frame against the CPU oracle's. `python profiles/kmlt_spectral.py
[rates] [interior] [psnr]` from the repository root."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hydracore3_amd import synth                                       # noqa: E402
from hydracore3_amd.api import HipIntegrator                           # noqa: E402
from hydracore3_amd.scene import load_hydra_xml                        # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def _rates(name, sc, spp):
    g = HipIntegrator(sc)
    g.set_option("kmlt_spectral", 1)
    g.set_option("qmc_spectral", 1)
    img = np.zeros((g.H, g.W, 4), np.float32)
    chains, steps = g.kmlt_chain_count(spp)
    for _ in range(2):
        img[:] = 0.0
        g.PathTraceBlockKMLT(g.N, 4, img, spp)
    ms = g.GetExecutionTime("PathTraceBlockKMLT")[0]
    print(f"{name} {g.W} x {g.H}, {spp} passes: spectral KMLT {chains} chains x {steps} steps, kernels {ms:.2f} ms, {chains * steps / ms / 1e3:.1f} M chain steps/s", flush=True)
    for _ in range(2):
        img[:] = 0.0
        g.PathTraceBlockQMC(g.N, 4, img, spp)
    ms = g.GetExecutionTime("PathTraceBlockQMC")[0]
    print(f"{name} {g.W} x {g.H}, {spp} passes: spectral QMC kernel {ms:.2f} ms, {g.N * spp / ms / 1e3:.1f} M samples/s", flush=True)


def rates():
    _rates("test_spectral", load_hydra_xml(os.path.join(SCENES, "test_spectral", "statex_00001.xml"), 1024, 1024, spectral=True), 8)


def interior():
    t = time.time()
    sc = synth.interior_scene()                                         # 1 M triangles, 1920 x 1080
    sc.spectral_mode = 1
    sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    print(f"interior scene built in {time.time() - t:.1f} s", flush=True)
    _rates("interior (1 M triangles) under m_spectral_mode", sc, 4)


def psnr():
    from oracle.orc import OracleIntegrator
    from test_qmc_spectral_gpu import _ldr, _psnr
    w, h, spp = 48, 32, 1024
    sc = load_hydra_xml(os.path.join(SCENES, "test_spectral", "statex_00001.xml"), w, h, spectral=True)
    ref = OracleIntegrator(sc).render(spp)
    for chains in (None, 16384, 1024):                                  # the default (the resident grid: few steps per chain at this size), then longer chains
        g = HipIntegrator(sc)
        g.set_option("kmlt_spectral", 1)
        if chains:
            g.set_option("kmlt_chains", chains)
        img = np.zeros((h, w, 4), np.float32)
        g.PathTraceBlockKMLT(g.N, 4, img, spp)
        # the normalised KMLT frame is a_passNum times the mean image, as the path tracer's sum over spp passes is
        print(f"test_spectral {w} x {h}, {spp} spp: PSNR(spectral KMLT, oracle spectral PathTraceBlock) = {_psnr(_ldr(img, spp), _ldr(ref, spp)):.2f} dB "
              f"(chains x steps {g.kmlt_chain_count(spp)}; mean {img[..., :3].mean() / spp:.4f} vs {ref[..., :3].mean() / spp:.4f})", flush=True)


if __name__ == "__main__":
    for what in (sys.argv[1:] or ["rates", "psnr"]):
        {"rates": rates, "interior": interior, "psnr": psnr}[what]()

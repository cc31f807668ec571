"""Diagnostic: traceSweep's per-lane pass on the Cornell box, instrumented build (STATS kernels), sweep_lanes 0 against 1 in one process:
share of wave-cycles per phase, exact triangle tests per ray, wave trips through the triangle code per wave-ray and lanes busy per trip.
Run on a GPU box: python profiles/sweep_lanes_phases.py [width height spp]"""
import sys; sys.path.insert(0, '.')
import numpy as np
from hydracore3_amd.api import HipIntegrator
from hydracore3_amd.scene import load_hydra_xml
w, h, spp = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (1024, 1024, 8)))
sc = load_hydra_xml('tests/golden/scenes/test_035/statex_00001.xml', w, h)
for lanes in (0, 1):
    g = HipIntegrator(sc); g.set_option('sweep_lanes', lanes); g.set_instrumentation(True)
    img = np.zeros((sc.height, sc.width, 4), np.float32); g.PathTraceBlock(g.N, 4, img, spp)
    c = g.counters(); tot = sum(c[k] for k in c if k.startswith('cyc_'))
    print('sweep_lanes', lanes, {k: round(c[k] / tot, 3) for k in c if k.startswith('cyc_')})
    print('   tris/ray', round(c['tris'] / c['rays'], 3), 'wave tri trips per wave-ray', round(c['wave_tri_iters'] * 64 / c['rays'], 3),
          'lanes busy per tri trip', round(c['tris'] / c['wave_tri_iters'], 2), 'mean radiance', float(img[..., :3].mean()))

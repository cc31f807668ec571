"""What the PathTraceVJP tests share (test_vjp_cpu.py, test_vjp_gpu.py): the cases, reference frames on the 1/64 grid and the oracle's
PathTraceDR gradients for them, computed once.

The oracle has no VJP. Its gradient is G(R) = sum over samples of 2 (C_s - R) dC_s for a reference frame R, so for two frames
G(R1) - G(R2) = sum 2 (R2 - R1) dC_s: the VJP of the adjoint A = 2 (R2 - R1), whatever R1 is. With R1 and R2 - R1 multiples of 1/64 below 2
every frame, difference and doubling is exact in float32."""
import functools

import numpy as np

import dr_texture_cases as T

SPP = 4
CASES = [T.BY_NAME["npot"], T.BY_NAME["single"], T.BY_NAME["mono_npot"], T.BY_NAME["two"], T.OVERFLOW]


def grid_frames(sc, seed=11):
    """(R1, D, sh): float32 [H, W, 4] on the 1/64 grid, R1 and sh in [0, 0.5), D in [0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    shape = (sc.height, sc.width, 4)
    r1 = (rng.integers(0, 32, shape) / 64.0).astype(np.float32)
    d = (rng.integers(32, 96, shape) / 64.0).astype(np.float32)
    sh = (rng.integers(0, 32, shape) / 64.0).astype(np.float32)
    return r1, d, sh


def adjoint_of(r1, r2):
    """A = 2 (R2 - R1) in out_color's row order: a_refImg's rows are bottom-up, the adjoint's are not."""
    return np.ascontiguousarray((2.0 * (r2 - r1))[::-1])


@functools.lru_cache(maxsize=None)
def oracle_gradient(case, which, spp=SPP):
    """The oracle's PathTraceDR gradient [case.size()] of `case` at `spp` for the reference frame R1 ("r1"), R1 + D ("r2"), R1 + sh ("r1s"),
    R1 + D + sh ("r2s") or dr_texture_cases.inputs' frame ("ref"); float64 copy, read-only."""
    from oracle.orc import OracleIntegrator
    sc = T.scene_of(case)
    data, ref = T.inputs(case, sc)
    r1, d, sh = grid_frames(sc)
    frame = {"r1": r1, "r2": r1 + d, "r1s": r1 + sh, "r2s": r1 + d + sh, "ref": ref}[which]
    cpu = OracleIntegrator(sc)
    T.register_cpu(cpu, case)
    g = T.oracle_dr(cpu, spp, frame, data)[1][:case.size()].astype(np.float64)
    g.setflags(write=False)
    return g


def linearity_bound(g1, g2):
    """Per element: 1e-3 (|G(R1)| + |G(R2)|) + element_atol(G(R1)) + element_atol(G(R2)) - assert_elements' terms, once per oracle gradient."""
    return 1e-3 * (np.abs(g1) + np.abs(g2)) + T.element_atol(g1, SPP) + T.element_atol(g2, SPP)

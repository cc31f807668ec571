"""numpy restatement of the sampler side of IntegratorQMC (mlt/rnd_qmc.cpp: qmc::rndFloat; mlt/integrator_qmc.cpp: SampleCameraRay, EnableQMC,
kernel_ContributeToImage). Not a test.

The generator-matrix table comes from the fixture tests/golden/qmc/niederreiter_11x31.json - numbers the reference's own program printed -
never from the library under test. Every product, sum and quotient is ONE float32 operation in the order the reference's source gives them.
"""
import json
import os

import numpy as np

from gbuffer_reference import FLT_MAX, _a, _mul4x3, _mul4x4, _normalize, f32

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qmc", "niederreiter_11x31.json")
DIMENSIONS, RESOLUTION = 11, 31


def load_fixture():
    """(table uint32 [11, 31], rnd_float records int64 [n, 3] = (pos, dim, bit pattern of the float))."""
    with open(FIXTURE) as f:
        d = json.load(f)
    assert d["dimensions"] == DIMENSIONS and d["resolution"] == RESOLUTION
    return np.asarray(d["table"], np.uint32).reshape(DIMENSIONS, RESOLUTION), np.asarray(d["rnd_float"], np.int64)


def rnd_float(table, pos, dim):
    """qmc::rndFloat(pos, dim, table): XOR of the columns the low 31 bits of pos select; (result + 1) converted to float (round to nearest) times
    INT_SCALE = 1.0f / float(0x80000001) = 2^-31."""
    pos = np.atleast_1d(np.asarray(pos, np.uint32))
    r = np.zeros(pos.shape, np.uint32)
    for bit in range(RESOLUTION):
        r ^= np.where((pos >> np.uint32(bit)) & np.uint32(1), table[dim, bit], np.uint32(0)).astype(np.uint32)
    scale = f32(1.0) / np.float32(0x80000001)
    assert scale == f32(2.0 ** -31)
    return _a((r + np.uint32(1)).astype(np.float32) * scale)


def sample_pixels(table, samples, width, height):
    """The pixel of every sample index (SampleCameraRay / kernel_ContributeToImage): x = uint(u0 * W), y = uint(u1 * H), clamped to W - 1, H - 1.
    Returns (x, y, y * W + x) as uint32 arrays; `samples`: a count (indices 0 .. samples - 1) or an array of indices."""
    s = np.arange(samples, dtype=np.uint32) if np.isscalar(samples) else np.asarray(samples, np.uint32)
    u0, u1 = rnd_float(table, s, 0), rnd_float(table, s, 1)
    x = np.minimum(_a(u0 * f32(width)).astype(np.uint32), np.uint32(width - 1))
    y = np.minimum(_a(u1 * f32(height)).astype(np.uint32), np.uint32(height - 1))
    return x, y, (y * np.uint32(width) + x).astype(np.uint32)


# IntegratorQMC::EnableQMC (integrator_qmc.cpp:11-86), written out by hand: (dof, spectral, motion) -> (dof, spd, motion, mat, lgt)
LAYOUTS = {
    (True, True, True): (2, 4, 5, 0, 0),
    (True, True, False): (2, 4, 0, 5, 7),
    (False, True, True): (2, 3, 2, 4, 6),
    (True, False, True): (2, 0, 4, 5, 7),
    (True, False, False): (2, 0, 0, 4, 6),
    (False, True, False): (2, 4, 0, 2, 5),
    (False, False, True): (2, 0, 4, 2, 5),
    (False, False, False): (2, 0, 0, 2, 4),
}


def map_samples_to_disc(x, y, rounded=False):
    """MapSamplesToDisc (include/cglobals.h:188-231) on float32 arrays. rounded: sin / cos evaluated in float64 and rounded once to float32
    (the correctly rounded sinf / cosf) instead of numpy's float32 routines."""
    r, phi = np.zeros_like(x), np.zeros_like(x)
    q = f32(0.25) * f32(3.141592654)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (x > y) & (x > -y); r = np.where(m, x, r); phi = np.where(m, _a(q * _a(y / x)), phi)
        m = (x < y) & (x > -y); r = np.where(m, y, r); phi = np.where(m, _a(q * _a(f32(2.0) - _a(x / y))), phi)
        m = (x < y) & (x < -y); r = np.where(m, -x, r); phi = np.where(m, _a(q * _a(f32(4.0) + _a(y / x))), phi)
        m = (x > y) & (x < -y); r = np.where(m, -y, r); phi = np.where(m, _a(q * _a(f32(6.0) - _a(x / y))), phi)
    if rounded:
        sn, cs = np.sin(phi.astype(np.float64)).astype(np.float32), np.cos(phi.astype(np.float64)).astype(np.float32)
    else:
        sn, cs = np.sin(_a(phi), dtype=np.float32), np.cos(_a(phi), dtype=np.float32)
    return _a(_a(r) * sn), _a(_a(r) * cs)                               # (r sin phi, r cos phi)


def camera_rays(table, params, samples, dof, motion_dim=0, rounded=False):
    """IntegratorQMC::SampleCameraRay for a pinhole or thin-lens camera, in CAMERA space (what PathTraceFromInputRaysBlock takes: it applies
    m_worldViewInv itself): RayPosAndW [n, 4], RayDirAndT [n, 4] with the time of dimension motion_dim (0: time 0) in .w."""
    s = np.arange(samples, dtype=np.uint32) if np.isscalar(samples) else np.asarray(samples, np.uint32)
    u0, u1 = rnd_float(table, s, 0), rnd_float(table, s, 1)
    pi = np.asarray(list(params.projInv), np.float32)
    zero, one = np.zeros_like(u0), np.ones_like(u0)
    px, py, pz, pw = _mul4x4(pi, _a(f32(2.0) * u0 - f32(1.0)), _a(f32(2.0) * u1 - f32(1.0)), zero, one)      # EyeRayDirNormalized (cglobals.h:49-55)
    dx, dy, dz = _normalize(_a(px / pw), _a(py / pw), _a(pz / pw))
    ox, oy, oz = zero.copy(), zero.copy(), zero.copy()
    if dof:
        assert params.camLensRadius > 0.0
        u2, u3 = rnd_float(table, s, 2), rnd_float(table, s, 3)
        t_focus = _a(f32(params.camTargetDist) / -dz)
        fx, fy, fz = _a(dx * t_focus), _a(dy * t_focus), _a(dz * t_focus)              # rayPos (0) + rayDir * tFocus
        fx, fy, fz = _a(zero + fx), _a(zero + fy), _a(zero + fz)
        sx, sy = map_samples_to_disc(_a(u2 - f32(0.5)), _a(u3 - f32(0.5)), rounded)
        k = _a(f32(params.camLensRadius) * f32(2.0))
        ox, oy = _a(ox + _a(k * sx)), _a(oy + _a(k * sy))
        dx, dy, dz = _normalize(_a(fx - ox), _a(fy - oy), _a(fz - oz))
    t = rnd_float(table, s, motion_dim) if motion_dim else zero
    pos = np.stack([ox, oy, oz, zero], axis=-1)
    dr = np.stack([dx, dy, dz, t], axis=-1)
    return np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(dr, np.float32)


def world_rays(params, pos, dr):
    """transform_ray3f(m_worldViewInv, ...) (cglobals.h:254-263) of camera-space rays: rayPosAndNear (near 0), rayDirAndFar (far FLT_MAX)."""
    wv = np.asarray(list(params.worldViewInv), np.float32)
    ox, oy, oz = _a(pos[:, 0]), _a(pos[:, 1]), _a(pos[:, 2])
    dx, dy, dz = _a(dr[:, 0]), _a(dr[:, 1]), _a(dr[:, 2])
    p1 = _mul4x3(wv, ox, oy, oz)
    p2 = _mul4x3(wv, _a(ox + f32(100.0) * dx), _a(oy + f32(100.0) * dy), _a(oz + f32(100.0) * dz))
    rx, ry, rz = _normalize(_a(p2[0] - p1[0]), _a(p2[1] - p1[1]), _a(p2[2] - p1[2]))
    zero = np.zeros_like(ox)
    return (np.ascontiguousarray(np.stack([p1[0], p1[1], p1[2], zero], axis=-1), np.float32),
            np.ascontiguousarray(np.stack([rx, ry, rz, np.full_like(ox, FLT_MAX)], axis=-1), np.float32))

"""numpy float32 restatement of Integrator::EvalGBuffer (integrator_gbuffer.cpp; integrator_pt.h:187-255). Not a test.

Every product, sum, quotient and square root below is ONE float32 operation on float32 arrays, written in the order the reference's source
gives them (no fused multiply-add, numpy's '/' and sqrt are correctly rounded), vectorised over pixels and looped over the sample indices
i, j. Inputs: the oracle's packed pixel list, its brute-force nearest hit, its texture sampler, and the SceneData arrays. Nothing here calls
the HIP library or comes from it.

Definitions the reference leaves open: rgba[3] of a hit is 1 (the reference reads color[3] of a float3,
integrator_gbuffer.cpp:190); DEG_TO_RAD is LiteMath's float(pi) / 180 in float32; the raw record of a sample is the one kernel_GetRayGBuff
writes (coverage 1 for a hit, 0 for a miss), before GBufferReduction overwrites its coverage.
"""
import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd.api import GBUFFER_DTYPE

GBUFFER_SAMPLES = 16
FLT_MAX = np.float32(3.402823466e+38)
NO_HIT = 0xFFFFFFFF
f32 = np.float32
DEG_TO_RAD = f32(np.float32(3.14159265358979323846) / np.float32(180.0))
FOV = f32(DEG_TO_RAD * f32(90.0))


def _a(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def plane_hammersley(n=GBUFFER_SAMPLES):
    """PlaneHammersley (integrator_gbuffer.cpp:8-24)."""
    out = np.zeros((n, 2), np.float32)
    for k in range(n):
        u, kk, p = f32(0.0), k, f32(0.5)
        while kk:
            if kk & 1:
                u = f32(u + p)
            p = f32(p * f32(0.5))
            kk >>= 1
        out[k, 0] = u
        out[k, 1] = f32(f32(f32(k) + f32(0.5)) / f32(n))
    return out


def _normalize(x, y, z):
    ln = np.sqrt(_a(_a(x * x + y * y) + z * z))                        # length = sqrt(dot), dot = (x*x + y*y) + z*z
    inv = _a(f32(1.0) / ln)
    return _a(x * inv), _a(y * inv), _a(z * inv)


def _mul4x4(m, x, y, z, w):
    """float4x4 * float4, column-major m: row r = ((x*m[r] + y*m[4+r]) + z*m[8+r]) + w*m[12+r]."""
    return tuple(_a(_a(_a(x * m[r] + y * m[4 + r]) + z * m[8 + r]) + w * m[12 + r]) for r in range(4))


def _mul4x3(m, x, y, z):
    return tuple(_a(_a(_a(m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]) for r in range(3))


def eye_rays(params, packed_xy):
    """kernel_InitEyeRayGB (integrator_gbuffer.cpp:91-108): rayPosAndNear, rayDirAndFar [n, 16, 4] for the pixels of packed_xy."""
    xy = np.asarray(packed_xy, np.uint32)
    h = plane_hammersley()
    x = (xy & np.uint32(0xFFFF)).astype(np.uint32)[:, None]
    y = ((xy & np.uint32(0xFFFF0000)) >> np.uint32(16)).astype(np.uint32)[:, None]
    fx = (x + np.uint32(params.winStartX)).astype(np.float32)          # the integer add comes first
    fy = (y + np.uint32(params.winStartY)).astype(np.float32)
    xn = _a(_a(fx + h[None, :, 0]) / f32(params.fbWidth))
    yn = _a(_a(fy + h[None, :, 1]) / f32(params.fbHeight))
    pi = np.asarray(list(params.projInv), np.float32)
    wv = np.asarray(list(params.worldViewInv), np.float32)
    zero, one = np.zeros_like(xn), np.ones_like(xn)
    px, py, pz, pw = _mul4x4(pi, _a(f32(2.0) * xn - f32(1.0)), _a(f32(2.0) * yn - f32(1.0)), zero, one)   # EyeRayDirNormalized (cglobals.h:49-55)
    dx, dy, dz = _normalize(_a(px / pw), _a(py / pw), _a(pz / pw))
    p1 = _mul4x3(wv, zero, zero, zero)                                 # transform_ray3f (cglobals.h:254-263)
    p2 = _mul4x3(wv, _a(zero + f32(100.0) * dx), _a(zero + f32(100.0) * dy), _a(zero + f32(100.0) * dz))
    rx, ry, rz = _normalize(_a(p2[0] - p1[0]), _a(p2[1] - p1[1]), _a(p2[2] - p1[2]))
    pos = np.stack([p1[0], p1[1], p1[2], zero], axis=-1)
    dr = np.stack([rx, ry, rz, np.full_like(xn, FLT_MAX)], axis=-1)
    return np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(dr, np.float32)


def shade_hits(sc, cpu, hits):
    """kernel_GetRayGBuff (integrator_gbuffer.cpp:110-200) for a flat array of CRT_Hit records (HIT_DTYPE)."""
    n = hits.shape[0]
    out = np.zeros(n, GBUFFER_DTYPE)
    out["norm"][:, 2] = 1.0
    out["matId"] = out["objId"] = out["instId"] = -1
    idx = np.flatnonzero(hits["geomId"] != NO_HIT)
    if idx.size == 0:
        return out
    hh = hits[idx]
    geom, inst, prim = hh["geomId"].astype(np.int64), hh["instId"].astype(np.int64), hh["primId"].astype(np.int64)
    mvo = np.asarray(sc.mat_vert_offset, np.int64).reshape(-1, 2)
    tri_off, vert_off = mvo[geom, 0], mvo[geom, 1]
    mat_id = np.asarray(sc.mat_id_by_prim, np.uint32)[tri_off + prim]   # no remap list, no blend resolution
    ti = np.asarray(sc.tri_indices, np.int64)
    vd = np.asarray(sc.vdata, np.float32).reshape(-1, 8)
    va, vb, vc = vd[ti[(tri_off + prim) * 3 + 0] + vert_off], vd[ti[(tri_off + prim) * 3 + 1] + vert_off], vd[ti[(tri_off + prim) * 3 + 2] + vert_off]
    u, v = _a(hh["coords"][:, 0]), _a(hh["coords"][:, 1])
    wa = _a(_a(f32(1.0) - u) - v)

    def mix(c):                                                          # (1 - u - v) * A + v * B + u * C
        return _a(_a(wa * va[:, c] + v * vb[:, c]) + u * vc[:, c])
    nx, ny, nz, tx, ty = mix(0), mix(1), mix(2), mix(3), mix(7)
    nm = np.stack([S.colmajor(np.linalg.inv(m).T) for m in sc.inst_matrices])[inst]     # m_normMatrices[instId] (integrator_pt_scene.cpp:877), as SceneData.desc() fills it

    def row(r):                                                          # mul3x3: row r = (m(r,0)*x + m(r,1)*y) + m(r,2)*z, element (r, c) = m[c*4 + r]
        return _a(_a(nm[:, 0 + r] * nx + nm[:, 4 + r] * ny) + nm[:, 8 + r] * nz)
    hx, hy, hz = _normalize(row(0), row(1), row(2))
    mats = np.array(sc.materials, dtype=S.MATERIAL_DTYPE)[mat_id.astype(np.int64) & 0x00FFFFFF]
    r0, r1 = mats["row0"][:, 0, :], mats["row1"][:, 0, :]
    tcx = _a(_a(r0[:, 0] * tx + r0[:, 1] * ty) + r0[:, 3])             # mulRows2x4
    tcy = _a(_a(r1[:, 0] * tx + r1[:, 1] * ty) + r1[:, 3])
    tex = np.zeros((idx.size, 4), np.float32)
    uv = np.ascontiguousarray(np.stack([tcx, tcy], axis=-1), np.float32)
    for t in np.unique(mats["texid"][:, 0]):
        sel = np.flatnonzero(mats["texid"][:, 0] == t)
        tex[sel] = cpu.tex_sample(int(t), uv[sel])
    rgb = _a(mats["colors"][:, 0, :3] * tex[:, :3])
    rgb[mats["mtype"] == S.MAT_TYPE_LIGHT_SOURCE] = 0.0
    o = np.zeros(idx.size, GBUFFER_DTYPE)
    o["depth"] = hh["t"]
    o["norm"] = np.stack([hx, hy, hz], axis=-1)
    o["texc"] = uv
    o["rgba"][:, :3] = rgb
    o["rgba"][:, 3] = 1.0
    o["coverage"] = 1.0
    o["matId"] = mat_id.view(np.int32)
    o["objId"] = hh["geomId"].view(np.int32)
    o["instId"] = hh["instId"].view(np.int32)
    out[idx] = o
    return out


def raw_samples(sc, cpu, params=None, block_num=None):
    """The [blockNum, 16] sample records of EvalGBuffer, from the oracle's brute-force hits."""
    params = cpu.params if params is None else params
    xy = cpu.packed_xy()
    xy = xy if block_num is None else xy[:block_num]
    pos, dr = eye_rays(params, xy)
    hits = cpu.ray_nearest(pos.reshape(-1, 4), dr.reshape(-1, 4), brute=True)
    return shade_hits(sc, cpu, hits).reshape(-1, GBUFFER_SAMPLES)


def _projected_pixel_size(dist, fov, w, h):
    ppx = _a(f32(fov / w) * dist)
    ppy = _a(f32(fov / h) * dist)
    big = np.where(ppx < ppy, ppy, ppx)                                  # std::max(ppx, ppy)
    return np.where(dist > 0, _a(f32(2.0) * big), f32(1000.0)).astype(np.float32)


def gbuff_diff(s1, s2, w, h):
    """gbuffDiff(s1, s2) (integrator_gbuffer.cpp:70-82) over arrays of records; not symmetric."""
    MANX = f32(0.15)
    pp = _projected_pixel_size(_a(s1["depth"]), FOV, f32(w), f32(h))
    madx = _a(pp * f32(2.0))
    d = _a(s1["norm"] - s2["norm"])
    dist = np.sqrt(_a(_a(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    dd = np.abs(_a(s1["depth"] - s2["depth"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ns = np.sqrt(_a(f32(1.0) - _a(dist / MANX)))
        ds = np.sqrt(_a(f32(1.0) - _a(dd / madx)))
        sim = _a(ns * ds)
    sim = np.where(dist >= MANX, f32(0.0), np.where(dd >= madx, f32(0.0), sim)).astype(np.float32)
    surf = _a(f32(1.0) - sim)
    obj = np.where((s1["instId"] == s2["instId"]) & (s1["objId"] == s2["objId"]), f32(0.0), f32(1.0)).astype(np.float32)
    mat = np.where(s1["matId"] == s2["matId"], f32(0.0), f32(1.0)).astype(np.float32)
    alpha = np.abs(_a(s1["rgba"][:, 3] - s2["rgba"][:, 3]))
    return _a(_a(_a(surf + obj) + mat) + alpha)


def reduce_samples(samples, w, h):
    """GBufferReduction (integrator_gbuffer.cpp:213-262) over [n, 16] records: returns (records [n], winner index [n])."""
    samples = np.ascontiguousarray(samples)
    n = samples.shape[0]
    min_diff = np.full(n, 100000000.0, np.float32)
    min_id = np.zeros(n, np.int64)
    cov = np.zeros((n, GBUFFER_SAMPLES), np.float32)
    summ = np.zeros((n, 4), np.float32)
    for i in range(GBUFFER_SAMPLES):
        diff = np.zeros(n, np.float32)
        c = np.zeros(n, np.float32)
        for j in range(GBUFFER_SAMPLES):                                 # j ascending, f32
            t = gbuff_diff(samples[:, i], samples[:, j], w, h)
            diff = _a(diff + t)
            c = _a(c + np.where(t < f32(1.0), f32(1.0), f32(0.0)).astype(np.float32))
        cov[:, i] = _a(c * f32(f32(1.0) / f32(GBUFFER_SAMPLES)))
        summ = _a(summ + samples["rgba"][:, i, :])                      # i ascending, f32
        better = diff < min_diff                                         # strict: the first smallest wins
        min_diff = np.where(better, diff, min_diff).astype(np.float32)
        min_id = np.where(better, i, min_id)
    out = samples[np.arange(n), min_id].copy()
    out["coverage"] = cov[np.arange(n), min_id]
    out["rgba"] = _a(summ * f32(f32(1.0) / f32(GBUFFER_SAMPLES)))
    return out, min_id


def scatter(records, packed_xy, w, h, into=None):
    """out_gbuffer[y * winWidth + x] = record of packed pixel b."""
    xy = np.asarray(packed_xy, np.uint32)[:records.shape[0]]
    frame = np.zeros((h, w), GBUFFER_DTYPE) if into is None else into.copy()
    frame[(xy >> 16) & 0xFFFF, xy & 0xFFFF] = records
    return frame


def eval_gbuffer(sc, cpu, params=None, block_num=None, into=None):
    """EvalGBuffer(blockNum, out): (frame [winHeight, winWidth], raw samples [blockNum, 16])."""
    params = cpu.params if params is None else params
    raw = raw_samples(sc, cpu, params, block_num)
    red, _ = reduce_samples(raw, params.winWidth, params.winHeight)
    return scatter(red, cpu.packed_xy(), params.winWidth, params.winHeight, into), raw


def srgb_textured(sc, raw):
    """True where a sample's base colour went through powf(x, 2.2): its material's texture has the sRGB flag (shape of raw)."""
    mats = np.array(sc.materials, dtype=S.MATERIAL_DTYPE)
    srgb = np.array([bool(t.srgb) for t in sc.textures])
    hit = raw["matId"] >= 0
    mid = np.where(hit, raw["matId"], 0).astype(np.int64) & 0x00FFFFFF
    return hit & srgb[mats["texid"][mid, 0]] & (mats["mtype"][mid] != S.MAT_TYPE_LIGHT_SOURCE)


def assert_records_equal(a, b, what="", rgb_2ulp=None):
    """Every field of every record, as uint32 views. rgb_2ulp (bool per record, or None): records whose r, g, b may differ by up to 2 ulp -
    the colours that went through the sRGB decode, where the host's powf is not correctly rounded for a few arguments in 10^4 (profiles/gbuffer.md);
    every other field of those records, and every field of all other records, must be equal."""
    assert a.shape == b.shape and a.dtype == GBUFFER_DTYPE and b.dtype == GBUFFER_DTYPE, (a.shape, b.shape)
    ua = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 15)
    ub = np.ascontiguousarray(b).view(np.uint32).reshape(-1, 15)
    ne = ua != ub
    if rgb_2ulp is not None:
        loose = np.asarray(rgb_2ulp, bool).reshape(-1)
        assert loose.shape[0] == ua.shape[0]
        ulps = np.abs(ua[:, 6:9].astype(np.int64) - ub[:, 6:9].astype(np.int64))      # non-negative floats: the distance in ulp
        assert np.all(a["rgba"].reshape(-1, 4)[:, :3] >= 0) and np.all(b["rgba"].reshape(-1, 4)[:, :3] >= 0)
        n_diff = int(np.sum(np.any(ne[:, 6:9], axis=1)))
        print(f"{what}: rgb differs on {n_diff} of {ua.shape[0]} records, {int(np.sum(np.any(ne[:, 6:9], axis=1) & ~loose))} of them without an sRGB texture; "
              f"largest distance {int(ulps.max())} ulp")
        ne[:, 6:9] &= ~(loose[:, None] & (ulps <= 2))
    bad = np.argwhere(ne)
    if bad.size:
        names = ["depth", "norm0", "norm1", "norm2", "texc0", "texc1", "r", "g", "b", "a", "shadow", "coverage", "matId", "objId", "instId"]
        cols = sorted({names[c] for c in bad[:, 1]})
        r = bad[0, 0]
        raise AssertionError(f"{what}: {np.unique(bad[:, 0]).size} of {ua.shape[0]} records differ in {cols}; first record {r}:\n{a.reshape(-1)[r]}\nvs\n{b.reshape(-1)[r]}")

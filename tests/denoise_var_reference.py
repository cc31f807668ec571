"""DenoiseFrameVar and the variance plane of adaptive sampling restated in numpy float32: the definition the kernels
denoiseVarPackKernel / denoiseVarPassKernel (hpt_denoise.hip) and adaptiveVarianceKernel (hpt_adaptive.hip) are held to, bit for bit.

As in denoise_reference: every operation is a float32 operation on float32 operands in the definition's order, IEEE division, no fused
multiply-add; a tap is evaluated for the whole frame at once and per pixel the order of the additions is the definition's."""
import numpy as np

from adaptive_reference import luminance
from denoise_reference import ALBEDO_FLOOR, DEPTH_FLOOR, KERNEL, _dist2, _floor, f32

G3 = np.array([1 / 4, 1 / 2, 1 / 4], f32)


def variance_of_mean(moments, packed_xy, tid_begin, tid_count, width, height, out=None):
    """adaptiveVarianceKernel: float32 [height * width]; out None: zeros are written into. Pixels outside the window keep their contents."""
    out = np.zeros(width * height, f32) if out is None else np.asarray(out, f32).reshape(-1)
    w = slice(tid_begin, tid_begin + tid_count)
    n = moments["passes"][w].astype(np.uint32)
    sy, sy2 = moments["sumY"][w].astype(f32), moments["sumY2"][w].astype(f32)
    with np.errstate(all="ignore"):
        fn = np.maximum(n, 2).astype(f32)
        mean = (sy / fn).astype(f32)
        d = ((sy2 / fn).astype(f32) - (mean * mean).astype(f32)).astype(f32)
        var = np.where(d > f32(0), d, f32(0)).astype(f32)
        v = (var / (fn - f32(1.0)).astype(f32)).astype(f32)
        v = np.where(n == 1, (sy * sy).astype(f32), v)
    v = np.where((n == 0) | ~(np.isfinite(sy) & np.isfinite(sy2)), f32(0), v).astype(f32)
    xy = packed_xy[w]
    out[(xy >> 16) * np.uint32(width) + (xy & 0xFFFF)] = v
    return out


def prefilter(v):
    """The 3 x 3 binomial mean at unit spacing over the in-frame taps (dy outer, dx inner): float32 [H, W]."""
    H, W = v.shape
    sum_g, sum_v = np.zeros((H, W), f32), np.zeros((H, W), f32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            g = G3[dy + 1] * G3[dx + 1]
            sum_g[P] = sum_g[P] + g
            sum_v[P] = sum_v[P] + g * v[Q]
    return (sum_v / sum_g).astype(f32)


def denoise_var(color, gbuffer, variance, iterations=5, normal_squarings=7, flags=1, norm_const=1.0, sigma_depth=0.05, sigma_albedo=0.1,
                sigma_lum=2.0, var_floor=1e-4, prefilter_on=True):
    """color float32 [H, W, 4]; gbuffer structured [H, W]; variance float32 [H, W]. Returns (float32 [H, W, 4], float32 [H, W])."""
    color, variance = np.asarray(color), np.asarray(variance)
    assert color.dtype == f32 and color.ndim == 3 and color.shape[2] == 4 and gbuffer.shape == color.shape[:2]
    assert variance.dtype == f32 and variance.shape == color.shape[:2]
    H, W = color.shape[:2]
    nc, sig_z, sig_a, sig_l, floor_v = f32(norm_const), f32(sigma_depth), f32(sigma_albedo), f32(sigma_lum), f32(var_floor)
    with np.errstate(all="ignore"):
        c = color[..., :3] * nc
        alpha = color[..., 3] * nc
        alb = np.ascontiguousarray(gbuffer["rgba"][..., :3], f32)
        alb_floor = _floor(alb, ALBEDO_FLOOR)
        v = np.where(np.isfinite(variance) & (variance > f32(0)), variance, f32(0)).astype(f32)
        v = (v * (nc * nc)).astype(f32)
        ya = luminance(alb_floor)
        ya2 = (ya * ya).astype(f32)
        if flags & 1:
            c = c / alb_floor
            v = (v / ya2).astype(f32)
        nrm = np.ascontiguousarray(gbuffer["norm"], f32)
        z = np.ascontiguousarray(gbuffer["depth"], f32)
        inst, mat = np.ascontiguousarray(gbuffer["instId"]), np.ascontiguousarray(gbuffer["matId"])
        sa2 = sig_a * sig_a
        sl2 = sig_l * sig_l
        for i in range(iterations):
            s = 1 << i
            sd = sig_z * f32(s)
            finite = np.isfinite(c).all(axis=-1)
            z_den = sd * _floor(np.abs(z), DEPTH_FLOOR)
            vbar = prefilter(v) if prefilter_on else v
            den_l = (sl2 * vbar + floor_v).astype(f32)
            lum = luminance(c)
            sum_w = np.zeros((H, W), f32)
            sum_c = np.zeros((H, W, 3), f32)
            sum_v = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = KERNEL[dy + 2] * KERNEL[dx + 2]
                    cq, vq = c[Q], v[Q]
                    if dy == 0 and dx == 0:
                        valid = finite[P]
                        w = np.full(valid.shape, h, f32)
                    else:
                        valid = (inst[P] == inst[Q]) & (mat[P] == mat[Q]) & finite[Q]
                        np_, nq = nrm[P], nrm[Q]
                        d = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
                        wn = np.where(d > f32(0), d, f32(0)).astype(f32)
                        for _ in range(normal_squarings):
                            wn = wn * wn
                        zero = np.zeros(valid.shape, f32)
                        xz = np.abs(z[P] - z[Q]) / z_den[P] if sig_z != 0 else zero
                        dl = lum[P] - lum[Q]
                        xl = np.where(finite[P], (dl * dl) / den_l[P], f32(0)).astype(f32) if sig_l != 0 else zero
                        xa = _dist2(alb[P], alb[Q]) / sa2 if sig_a != 0 else zero
                        w = (h * wn) / (((f32(1) + xz) * (f32(1) + xl)) * (f32(1) + xa))
                    assert w.dtype == f32 and cq.dtype == f32 and vq.dtype == f32
                    sum_w[P] = np.where(valid, sum_w[P] + w, sum_w[P])
                    sum_c[P] = np.where(valid[..., None], sum_c[P] + w[..., None] * cq, sum_c[P])
                    sum_v[P] = np.where(valid, sum_v[P] + (w * w) * vq, sum_v[P])
            some = sum_w != f32(0)
            c = np.where(some[..., None], sum_c / sum_w[..., None], f32(0)).astype(f32)
            v = np.where(some, sum_v / (sum_w * sum_w), f32(0)).astype(f32)
        if flags & 1:
            c = c * alb_floor
            v = (v * ya2).astype(f32)
        out = np.concatenate([c, alpha[..., None]], axis=-1)
    assert out.dtype == f32 and v.dtype == f32
    return out, v

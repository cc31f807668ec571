"""DenoiseFrame restated in numpy float32: the definition the device kernels of hpt_denoise.hip are held to, bit for bit.

Every operation is a float32 operation on float32 operands, in the order the definition gives: the taps dy = -2..2 (outer), dx = -2..2 (inner),
each added to float32 sums; IEEE division; no fused multiply-add (numpy has none). A tap is evaluated for the whole frame at once - per pixel the
order of the additions is the definition's."""
import numpy as np

f32 = np.float32
KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)           # the B3 spline: dyadic, exact
ALBEDO_FLOOR = f32(1e-3)
DEPTH_FLOOR = f32(1e-6)


def _floor(a, lo):
    """max(a, lo) as the kernel writes it: a > lo ? a : lo (a NaN gives lo)."""
    return np.where(a > lo, a, lo).astype(f32)


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(color, gbuffer, iterations=5, normal_squarings=7, flags=1, norm_const=1.0, sigma_color=0.6, sigma_depth=0.05, sigma_albedo=0.1):
    """color float32 [H, W, 4]; gbuffer: structured array [H, W] with depth, norm, rgba, matId, instId. Returns float32 [H, W, 4]."""
    color = np.asarray(color)
    assert color.dtype == f32 and color.ndim == 3 and color.shape[2] == 4 and gbuffer.shape == color.shape[:2]
    H, W = color.shape[:2]
    nc, sig_c, sig_z, sig_a = f32(norm_const), f32(sigma_color), f32(sigma_depth), f32(sigma_albedo)
    with np.errstate(all="ignore"):
        c = color[..., :3] * nc
        alpha = color[..., 3] * nc
        alb = np.ascontiguousarray(gbuffer["rgba"][..., :3], f32)
        alb_floor = _floor(alb, ALBEDO_FLOOR)
        if flags & 1:
            c = c / alb_floor
        nrm = np.ascontiguousarray(gbuffer["norm"], f32)
        z = np.ascontiguousarray(gbuffer["depth"], f32)
        inst, mat = np.ascontiguousarray(gbuffer["instId"]), np.ascontiguousarray(gbuffer["matId"])
        sa2 = sig_a * sig_a
        for i in range(iterations):
            s = 1 << i
            sd = sig_z * f32(s)
            sc = sig_c * f32(2.0 ** -i)
            sc2 = sc * sc
            finite = np.isfinite(c).all(axis=-1)
            z_den = sd * _floor(np.abs(z), DEPTH_FLOOR)
            sum_w = np.zeros((H, W), f32)
            sum_c = np.zeros((H, W, 3), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue                                          # every tap of this offset lies outside the frame
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = KERNEL[dy + 2] * KERNEL[dx + 2]
                    cq = c[Q]
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
                        xc = np.where(finite[P], _dist2(c[P], cq) / sc2, f32(0)).astype(f32) if sig_c != 0 else zero
                        xa = _dist2(alb[P], alb[Q]) / sa2 if sig_a != 0 else zero
                        w = (h * wn) / (((f32(1) + xz) * (f32(1) + xc)) * (f32(1) + xa))
                    assert w.dtype == f32 and cq.dtype == f32
                    sum_w[P] = np.where(valid, sum_w[P] + w, sum_w[P])
                    sum_c[P] = np.where(valid[..., None], sum_c[P] + w[..., None] * cq, sum_c[P])
            c = np.where((sum_w != f32(0))[..., None], sum_c / sum_w[..., None], f32(0)).astype(f32)
        if flags & 1:
            c = c * alb_floor
        out = np.concatenate([c, alpha[..., None]], axis=-1)
    assert out.dtype == f32
    return out

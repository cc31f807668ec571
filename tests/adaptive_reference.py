"""numpy float32 restatement of adaptive sampling's small kernels (hpt_adaptive.hip) and of the megakernel's luminance / moments bookkeeping
(hpt_kernels.hip, the ADAPT instantiations). Every operation is one IEEE f32 operation, in the kernels' order, so the device is held to this
bit for bit. Tids are positions in packed_xy (uint32, y << 16 | x); images are indexed y * width + x."""
import numpy as np

MOMENTS_DTYPE = np.dtype([("sumY", np.float32), ("sumY2", np.float32), ("passes", np.uint32), ("reserved", np.uint32)])
f32 = np.float32


def packed_xy(width, height, tile):
    """m_packedXY of PackXYBlock for a frame whose sides are multiples of `tile` (tile 1: row-major): tid -> y << 16 | x, tiles row by row."""
    out = np.zeros(width * height, np.uint32)
    y, x = np.mgrid[0:height, 0:width]
    off = ((x // tile) + (y // tile) * (width // tile)) * tile * tile + (y % tile) * tile + (x % tile)
    out[off.reshape(-1)] = ((y.astype(np.uint32) << 16) | x.astype(np.uint32)).reshape(-1)
    return out


def crafted_records():
    """Records at the planner's edges: (sumY, sumY2, passes): no passes; a variance that rounds negative; NaN and infinite sums; huge and zero
    variances; a plain one; one far past any pass limit."""
    rec = [(0.0, 0.0, 0), (3.0, 2.9999998, 3), (np.nan, 1.0, 5), (1.0, np.inf, 6), (-np.inf, 1.0, 2), (0.0, 2e12, 2), (0.0, 0.0, 3), (0.0, 1e-20, 3),
           (8.0, 20.0, 4), (8.0, 36.0, 4), (100.0, 300.0, 50), (1e-30, 1e-38, 7), (3e38, 3e38, 1), (5.0, 25.0, 1)]
    m = np.zeros(len(rec), MOMENTS_DTYPE)
    for i, (a, b, n) in enumerate(rec):
        m[i] = (f32(a), f32(b), n, 0)
    return m


def luminance(rgb):
    """rgb: float32 [..., 3], the three values a sample adds to the frame -> y = (0.2126 r + 0.7152 g) + 0.0722 b, each step rounded to f32."""
    rgb = np.asarray(rgb, f32)
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * rgb[..., 0] + f32(0.7152) * rgb[..., 1]).astype(f32) + f32(0.0722) * rgb[..., 2]).astype(f32)


def accumulate(moments, samples_y):
    """moments: MOMENTS_DTYPE [n] (changed in place and returned); samples_y: (y float32 [n], mask bool [n]) pairs in pass order - the pixels under
    the mask take the sample: sumY += y; sumY2 += y * y; passes += 1."""
    with np.errstate(all="ignore"):
        for y, mask in samples_y:
            y = np.asarray(y, f32)
            moments["sumY"] = np.where(mask, (moments["sumY"] + y).astype(f32), moments["sumY"])
            moments["sumY2"] = np.where(mask, (moments["sumY2"] + (y * y).astype(f32)).astype(f32), moments["sumY2"])
            moments["passes"] = np.where(mask, moments["passes"] + np.uint32(1), moments["passes"])
    moments["reserved"] = 0
    return moments


def total_passes(moments, tol, lum_floor, min_passes):
    """adaptiveTotal: (passes each record asks for in all, uint32; nonfinite mask)."""
    n = moments["passes"].astype(np.uint32)
    sy, sy2 = moments["sumY"].astype(f32), moments["sumY2"].astype(f32)
    with np.errstate(all="ignore"):
        fn = np.maximum(n, 1).astype(f32)
        mean = (sy / fn).astype(f32)
        var = np.fmax(((sy2 / fn).astype(f32) - (mean * mean).astype(f32)).astype(f32), f32(0.0))
        den = (f32(tol) * (np.abs(mean) + f32(lum_floor)).astype(f32)).astype(f32)
        tf = (var / (den * den).astype(f32)).astype(f32)
        tf = np.where(np.isnan(tf), f32(0.0), tf)
        big = tf >= f32(2147483648.0)
        total = np.where(big, np.uint32(0x7FFFFFFF), np.ceil(np.where(big, f32(0.0), tf)).astype(np.uint32))
    total = np.maximum(total, np.uint32(min_passes))
    nonfinite = (n != 0) & ~(np.isfinite(sy) & np.isfinite(sy2))
    total = np.where(nonfinite, n, total)
    total = np.where(n == 0, np.uint32(min_passes), total)
    return total.astype(np.uint32), nonfinite


def need_image(moments, packed_xy, tid_begin, tid_count, width, height, tol, lum_floor, min_passes):
    """adaptiveNeedKernel: uint32 [height * width], 0 outside the window."""
    need = np.zeros(width * height, np.uint32)
    w = slice(tid_begin, tid_begin + tid_count)
    total, _ = total_passes(moments[w], tol, lum_floor, min_passes)
    n = moments["passes"][w]
    xy = packed_xy[w]
    need[(xy >> 16) * np.uint32(width) + (xy & 0xFFFF)] = np.where(total > n, total - n, 0).astype(np.uint32)
    return need


def plan(moments, packed_xy, tid_begin, tid_count, width, height, tol, lum_floor, min_passes, max_passes, step, dilate):
    """adaptiveNeedKernel + adaptivePlanKernel: (counts uint32 [len(packed_xy)], zero outside the window; info dict)."""
    need = need_image(moments, packed_xy, tid_begin, tid_count, width, height, tol, lum_floor, min_passes).reshape(height, width)
    if dilate:
        pad = np.zeros((height + 2, width + 2), np.uint32)
        pad[1:-1, 1:-1] = need
        need = np.max([pad[dy:dy + height, dx:dx + width] for dy in range(3) for dx in range(3)], axis=0)
    w = slice(tid_begin, tid_begin + tid_count)
    xy = packed_xy[w]
    n = moments["passes"][w].astype(np.uint32)
    e = need[xy >> 16, xy & 0xFFFF].astype(np.uint32)
    e = np.minimum(e, np.uint32(max_passes) - np.minimum(n, np.uint32(max_passes)))
    e = np.minimum(e, np.uint32(step)).astype(np.uint32)
    counts = np.zeros(len(packed_xy), np.uint32)
    counts[w] = e
    _, nonfinite = total_passes(moments[w], tol, lum_floor, min_passes)
    info = {"passes": int(e.astype(np.uint64).sum()), "pixels": int((e > 0).sum()), "maxPasses": int(n.max()) if n.size else 0, "nonfinite": int(nonfinite.sum())}
    return counts, info


def resolve(frame, moments, packed_xy, tid_begin, tid_count, width, channels, out=None):
    """adaptiveResolveKernel on frames float32 [height * width * channels]; out None: a copy of frame is written into."""
    frame = np.asarray(frame, f32).reshape(-1, channels)
    out = frame.copy() if out is None else np.asarray(out, f32).reshape(-1, channels)
    w = slice(tid_begin, tid_begin + tid_count)
    xy = packed_xy[w]
    pix = (xy >> 16) * np.uint32(width) + (xy & 0xFFFF)
    p = moments["passes"][w]
    nc = min(channels, 3)
    with np.errstate(all="ignore"):
        q = (frame[pix, :nc] / np.maximum(p, 1).astype(f32)[:, None]).astype(f32)
    vals = np.where((p != 0)[:, None], q, f32(0.0))
    src4 = frame[pix, 3].copy() if channels > 3 else None
    out[pix, :nc] = vals
    if channels > 3:
        out[pix, 3] = src4
    return out.reshape(-1)

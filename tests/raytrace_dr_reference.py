"""numpy restatement of IntegratorDR::RayTraceDR (diff_render/integrator_dr.cpp:60-161, 168-273, 372-459). Not a test.

The eye ray, the closest hit and the vertex gather are raytrace_reference.py's (float32, hits from the oracle's brute-force query, the pixel
order from its packed list). What is restated here: Tex2DFetchAD / bilinearOffsets, kernel_CalcRayColor's colour, PixelLossRT and the gradient
that the reference takes from Enzyme. Nothing here calls the HIP library or comes from it.

float32 form (`ray_trace_dr`): every product, sum and difference is ONE float32 operation on float32 arrays in the source's order, the
gradient is accumulated in float32 in tid order (pixel, tap, channel). Its colours and per-pixel losses are what the GPU is held to bit for
bit; its gradient is what the GPU gives where no two pixels share an element.

float64 twin (`twin`): the same expressions in float64, and per gradient element the number of terms n and the sum of |term|. Two kinds:
  forward="f64": everything after the texture coordinate (a float32 value, taken as exact) in float64. The loss is then an exact quadratic
                 of every texel and the gradient its exact derivative: what finite differences are compared with.
  forward="f32": the terms are float64 products of the FLOAT32 pass's own diff, base colour and tap weights. Against this one the GPU's
                 element differs only by the roundings of its products and of its sum - at most 4 per term (one channel: three products,
                 two sums, the weight; four channels: two) and one per atomic add - which is the bound (n + 4) 2^-24 sum|term| of the
                 GPU test. For a one-channel texture |term| = (|2 d0 b0| + |2 d1 b1| + |2 d2 b2|) w: the roundings inside the channel sum
                 are relative to its absolute terms.

Definitions the reference leaves open:
 4. a miss returns before kernel_CalcRayColor runs: its pixel of out_color is untouched, its colour is 0, its loss |ref|^2;
 5. dot3(d, d) = (d.x * d.x + d.y * d.y) + d.z * d.z (LiteMath's is not in the tree);
 6. the gradient's products, per tap k: four channels ((2 * d_c) * base_c) * w_k to element off + o_k * 4 + c, c = 0..2; one channel
    ((2 * d_0 * base_0 + 2 * d_1 * base_1) + 2 * d_2 * base_2) * w_k to element off + o_k.
"""
import numpy as np

import raytrace_reference as RT
from gbuffer_reference import NO_HIT
from hydracore3_amd import scene as S


def registrations(case):
    """{texture id: (offset, w, h, channels)} of a dr_texture_cases.Case."""
    return {reg[0]: lay for reg, lay in zip(case.registrations(), case.layout())}


def fetch_ad(tc, w, h, ch, addr, data, off, dtype=np.float32):
    """Tex2DFetchAD's first branch (integrator_dr.cpp:101-157) for texture coordinates tc [n, 2]: (texColor [n, 4], tap offsets [n, 4] in
    texels, weights [n, 4]), computed in `dtype`."""
    F = dtype
    tc = np.asarray(tc, np.float32).astype(F)
    d = np.asarray(data).astype(F)                                                  # (a float64 array stays as it is: the twin's finite differences)
    ffx = tc[:, 0] * F(np.float32(w)) - F(0.5)
    ffy = tc[:, 1] * F(np.float32(h)) - F(0.5)
    if addr[0] == S.ADDR_CLAMP:
        ffx = np.where(ffx < 0, F(0.0), ffx)
    if addr[1] == S.ADDR_CLAMP:
        ffy = np.where(ffy < 0, F(0.0), ffy)
    px, py = np.trunc(ffx).astype(np.int64), np.trunc(ffy).astype(np.int64)          # (int)ffx truncates
    fx, fy = np.abs(ffx - px.astype(F)), np.abs(ffy - py.astype(F))
    fx1, fy1 = F(1.0) - fx, F(1.0) - fy
    wts = np.stack([fx1 * fy1, fx * fy1, fx1 * fy, fx * fy], axis=-1)
    sx, sy = np.where(ffx > 0, 1, -1), np.where(ffy > 0, 1, -1)                       # bilinearOffsets: % then + w for a negative remainder
    x0, x1, y0, y1 = np.mod(px, w), np.mod(px + sx, w), np.mod(py, h), np.mod(py + sy, h)
    offs = np.stack([y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1], axis=-1)
    assert wts.dtype == F and offs.min() >= 0 and offs.max() < w * h
    if ch == 4:
        f = d[off + offs[:, :, None] * 4 + np.arange(4)[None, None, :]]              # [n, tap, channel]
        out = ((f[:, 0] * wts[:, 0:1] + f[:, 1] * wts[:, 1:2]) + f[:, 2] * wts[:, 2:3]) + f[:, 3] * wts[:, 3:4]
    else:
        f = d[off + offs]
        v = ((f[:, 0] * wts[:, 0] + f[:, 1] * wts[:, 1]) + f[:, 2] * wts[:, 2]) + f[:, 3] * wts[:, 3]
        out = np.stack([v, v, v, v], axis=-1)
    assert out.dtype == F
    return out, offs, wts


def _scatter(size, elem, term, absterm, dtype):
    """Sequential accumulation in `dtype`, in the order given; also the number of terms and the sum of |term| (float64) per element."""
    grad = np.zeros(size, dtype)
    n = np.zeros(size, np.int64)
    sabs = np.zeros(size, np.float64)
    np.add.at(grad, elem, term.astype(dtype))                                       # unbuffered: one add per term, in index order
    np.add.at(n, elem, 1)
    np.add.at(sabs, elem, absterm.astype(np.float64))
    return grad, n, sabs


def _terms(diff, base, offs, wts, off, ch, dtype):
    """Definition 6 for the pixels of one parameter texture: (element [m], term [m], |term| [m]) in (pixel, tap, channel) order."""
    F = dtype
    diff, base, wts = diff.astype(F), base.astype(F), wts.astype(F)
    if ch == 4:
        dcb = (F(2.0) * diff) * base                                                # [n, 3]
        term = dcb[:, None, :] * wts[:, :, None]                                    # [n, tap, c]
        elem = off + offs[:, :, None] * 4 + np.arange(3)[None, None, :]
        return elem.reshape(-1), term.reshape(-1), np.abs(term).reshape(-1)
    p = (F(2.0) * diff) * base
    s = (p[:, 0] + p[:, 1]) + p[:, 2]
    term = s[:, None] * wts
    absterm = np.abs(p).sum(axis=-1)[:, None] * wts
    return (off + offs).reshape(-1), term.reshape(-1), absterm.reshape(-1)


def ray_trace_dr(sc, cpu, regs, data, ref, channels=4, pass_num=1, params=None, tid=None, grad_mode=1, into=None, dtype=np.float32, forward=None, geom=None):
    """RayTraceDR(tid, channels, out_color, a_passNum, a_refImg, a_data, a_dataGrad, a_gradSize). regs: {texture id: (offset, w, h, channels)};
    data [a_gradSize] or None; ref [winHeight, winWidth, channels] bottom-up. Returns a dict:
      frame [winHeight, winWidth, 4]: `into` (zeros without it) with the HIT pixels of the first tid packed pixels assigned (colour, 0);
      color [tid, 3], loss_px [tid] (the per-pixel loss), loss (sum of loss_px / pass_num in tid order, in `dtype`), hit [tid],
      param [tid] (the pixel's colour is a product with a parameter texel: it has gradient terms),
      grad, n, sum_abs [a_gradSize]: the gradient, its number of terms and the sum of |term| per element.
    dtype float32: the restatement. dtype float64: the twin, `forward` = another call's result whose float32 diff / weights the terms are made of
    (the "f32" kind of the module text) or None (the "f64" kind). geom: the "geom" entry of an earlier result under the same scene, params
    and tid (rays, hits and the ordinary sampler are then not computed again)."""
    F = dtype
    params = cpu.params if params is None else params
    xy = cpu.packed_xy()
    xy = xy if tid is None else xy[:tid]
    n = xy.shape[0]
    if geom is None:
        T = RT._Tables(sc, cpu)
        pos, dr = RT.eye_rays(params, xy)
        hits = cpu.ray_nearest(pos, dr, brute=True)                                  # kernel_RayTrace: RayQuery_NearestHit
        hit = hits["geomId"] != NO_HIT
        idx = np.flatnonzero(hit)
        geom = {"hit": hit}
        if idx.size:
            _, (tx, ty), mat_id = T.gather(hits[idx])
            mats = T.mats[mat_id.astype(np.int64) & 0x00FFFFFF]                      # no remap list
            plain, dec = T.base_times_tex(mats, tx, ty)                              # the ordinary sampler (integrator_dr.cpp:160)
            assert not dec.any(), "a texture with the sRGB flag in view: hold it to raytrace_reference's exception first"
            geom.update(tx=tx, ty=ty, mats=mats, plain=plain)
    hit = geom["hit"]
    idx = np.flatnonzero(hit)
    color = np.zeros((n, 3), F)                                                     # a miss: CastRayDR returns float4(0) (definition 4)
    param = np.zeros(n, bool)
    size = 0 if data is None else int(np.asarray(data).size)
    use_ad = grad_mode != 0 and data is not None
    pieces = []                                                                     # (pixel indices, offs, wts, base, off, ch) per parameter texture
    if idx.size:
        tx, ty, mats, plain = geom["tx"], geom["ty"], geom["mats"], geom["plain"]
        rgb = plain.astype(F)
        r0, r1 = mats["row0"][:, 0, :], mats["row1"][:, 0, :]
        tc = np.stack([RT._a(RT._a(r0[:, 0] * tx + r0[:, 1] * ty) + r0[:, 3]), RT._a(RT._a(r1[:, 0] * tx + r1[:, 1] * ty) + r1[:, 3])], axis=-1)
        base = mats["colors"][:, 0, :3]
        w = mats["colors"][:, 0, 3]
        texid = mats["texid"][:, 0]
        if use_ad:
            for t, (off, tw, th, ch) in regs.items():
                sel = np.flatnonzero(texid == t)
                if sel.size == 0:
                    continue
                tex = sc.textures[t]
                out, offs, wts = fetch_ad(tc[sel], tw, th, ch, (tex.addr_u, tex.addr_v), data, off, F)
                rgb[sel] = base[sel].astype(F) * out[:, :3]
                live = w[sel] <= 0                                                   # w > 0: the texel is not part of the colour
                pieces.append((idx[sel[live]], offs[live], wts[live], base[sel[live]], off, ch))
                param[idx[sel[live]]] = True
        splat = np.minimum(np.maximum(w, np.float32(0.0)), np.float32(1.0)).astype(F)
        color[idx] = np.where((w > 0)[:, None], splat[:, None], rgb)
    frame = np.zeros((params.winHeight, params.winWidth, 4), np.float32) if into is None else into.copy()
    py, px = RT._pixels(xy)
    if F == np.float32:
        frame[py[idx], px[idx], :3] = color[idx]
        frame[py[idx], px[idx], 3] = 0.0
    ref = np.asarray(ref, np.float32).reshape(params.winHeight, params.winWidth, channels)
    y_ref = np.uint32(params.winHeight) - py - np.uint32(1)
    diff = color - ref[y_ref, px, :3].astype(F)
    loss_px = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]   # definition 5
    assert diff.dtype == F and loss_px.dtype == F
    shares = loss_px / F(np.float32(pass_num))                                       # avgLoss += float(lossVal) / float(a_passNum), in tid order:
    loss = np.cumsum(shares, dtype=F)[-1] if n else F(0.0)                           # cumsum adds one element at a time, in `dtype`
    elems, terms, absterms = [], [], []
    src_diff = diff if forward is None else forward["diff"]
    src_pieces = pieces if forward is None else forward["pieces"]
    for pix, offs, wts, base_p, off, ch in src_pieces:
        e, t, a = _terms(src_diff[pix], base_p, offs, wts, off, ch, F)
        elems.append(e); terms.append(t); absterms.append(a)
    if elems:                                                                       # tid order: a stable sort of the pieces' pixels
        pix_all = np.concatenate([np.repeat(p[0], 12 if p[5] == 4 else 4) for p in src_pieces])
        order = np.argsort(pix_all, kind="stable")
        grad, cnt, sabs = _scatter(size, np.concatenate(elems)[order], np.concatenate(terms)[order], np.concatenate(absterms)[order], F)
    else:
        grad, cnt, sabs = np.zeros(size, F), np.zeros(size, np.int64), np.zeros(size, np.float64)
    return {"frame": frame, "color": color, "loss_px": loss_px, "loss": loss, "hit": hit, "param": param, "grad": grad, "n": cnt,
            "sum_abs": sabs, "diff": diff, "pieces": pieces, "xy": xy, "geom": geom}


def twin(sc, cpu, regs, data, ref, forward="f64", f32=None, **kw):
    """The float64 twin (module text). forward="f32" takes the float32 pass's result `f32` (computed here when not given)."""
    if forward == "f64":
        return ray_trace_dr(sc, cpu, regs, data, ref, dtype=np.float64, **kw)
    f32 = ray_trace_dr(sc, cpu, regs, data, ref, **kw) if f32 is None else f32
    return ray_trace_dr(sc, cpu, regs, data, ref, dtype=np.float64, forward=f32, **kw)


def wave_partials(loss_px, pass_num=1, wave=64):
    """What each wave's lane 0 holds after the kernel's reduction: loss / passNum per lane (0 past the last pixel), then the shuffle-down tree
    s += lane[i + o], o = 32 .. 1, in float32. Deterministic: no atomic is involved yet."""
    share = (np.asarray(loss_px, np.float32) / np.float32(pass_num)).astype(np.float32)
    pad = (-share.size) % wave
    s = np.concatenate([share, np.zeros(pad, np.float32)]).reshape(-1, wave)
    o = wave // 2
    while o:
        s = np.concatenate([(s[:, :wave - o] + s[:, o:]).astype(np.float32), s[:, wave - o:]], axis=1)
        o //= 2
    return np.ascontiguousarray(s[:, 0])


def wave_sum(loss_px, pass_num=1, wave=64, order=None):
    """What lossAccum receives from 0 when the waves' atomics land in `order` (default: wave order): the partial sums added in float32.
    order may be an int array [m, n_waves] of m orders at once; the result is then [m]."""
    w = wave_partials(loss_px, pass_num, wave)
    order = np.arange(w.size)[None, :] if order is None else np.atleast_2d(order)
    total = np.zeros(order.shape[0], np.float32)
    for k in range(order.shape[1]):
        total = (total + w[order[:, k]]).astype(np.float32)
    return total if total.size > 1 else total[0]

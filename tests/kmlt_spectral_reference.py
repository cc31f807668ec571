"""What spectral MLT adds to tests/kmlt_reference.py and tests/qmc_spectral_reference.py: the base class's draw order under m_spectral_mode laid
out as IntegratorKMLT's vectors, the colour PathTraceF forms from a path's raw components, and the normalisation's four statistics summed in
kmltStatsKernel's own order (so that they compare with ==; kmlt_reference.normalisation sums in numpy's). Not a test.

Everything else - the generator, the chains, SampleWavelengths, SpectralCamRespoceToRGB - is imported from those two modules.
"""
import numpy as np

import kmlt_reference as K
import qmc_spectral_reference as QS

F32 = np.float32
WAVE_SLOT, TIME_SLOT = 4, 5                                            # IntegratorKMLT::GetRandomNumbersSpec / GetRandomNumbersTime


def base_vectors(gens, packed_xy, params, motion):
    """The vectors x whose spectral F equals what a spectral PathTraceBlock pass computes, per tid, from the generator states `gens` [N, 2]:
    kernel_InitEyeRay2 draws the lens float4, the time when instances move, then ONE float for the wavelengths (integrator_pt.cpp:114-118);
    every bounce the light selection float, the light float4 and the material float4 (no blends here). x[0], x[1]: the film point the base
    camera forms from pixel and jitter. Returns (x [N, state size], wave sample [N])."""
    n = K.state_size(params.traceDepth)
    G = K.Gens.from_states(gens)
    xy = np.asarray(packed_xy, np.uint32)
    lens = G.float4()
    x = np.zeros((xy.size, n), F32)
    fx = (xy & 0xFFFF).astype(F32) + lens[:, 0]
    fy = (xy >> 16).astype(F32) + lens[:, 1]
    x[:, 0] = (fx + F32(params.winStartX)) / F32(params.fbWidth)
    x[:, 1] = (fy + F32(params.winStartY)) / F32(params.fbHeight)
    x[:, 2:4] = lens[:, 2:4]
    if motion:
        x[:, TIME_SLOT] = G.float1()
    x[:, WAVE_SLOT] = G.float1()
    for b in range(params.traceDepth):
        o = K.BOUNCE_START + K.PER_BOUNCE * b
        x[:, o + 3] = G.float1()
        x[:, o:o + 3] = G.float4()[:, :3]
        x[:, o + K.MATS_ID:o + K.MATS_ID + 4] = G.float4()
    return x, x[:, WAVE_SLOT].copy()


def chain_sums(is_large, colour):
    """The per-chain sums of the chain loop (integrator_kmlt.cpp:372-376) from a run's records, in step order: accumBrightness starts at 0.0
    (double) and a large step adds double(contribFunc(colour of its proposal)), whether accepted or not. is_large [C, steps], colour
    [C, steps, >= 3] -> (accumBrightness float64 [C], largeSteps int64 [C])."""
    is_large = np.asarray(is_large).astype(bool)
    y = K.contrib_func(np.asarray(colour, F32)[..., :3]).astype(np.float64)
    accum = np.zeros(is_large.shape[0], np.float64)
    for i in range(is_large.shape[1]):                                 # one double addition per large step, in step order
        accum = np.where(is_large[:, i], accum + y[:, i], accum)
    return accum, is_large.sum(axis=1).astype(np.int64)


def _block_sum(values):
    """kmltStatsKernel's sum of `values` (float64, any length) in its own order: thread t of 256 starts at 0.0 and adds elements t, t + 256,
    t + 512, ... one after the other; the 256 partial sums are then folded in LDS, sh[t] += sh[t + o] for t < o, o = 128, 64, ... 1."""
    v = np.asarray(values, np.float64).reshape(-1)
    rows = -(-v.size // 256)
    pad = np.zeros(rows * 256, np.float64)                             # (a thread whose share ends earlier adds nothing more: + 0.0 is exact)
    pad[:v.size] = v
    sh = np.zeros(256, np.float64)
    for row in pad.reshape(rows, 256):
        sh = sh + row
    o = 128
    while o > 0:
        sh[:o] = sh[:o] + sh[o:2 * o]
        o >>= 1
    return float(sh[0])


def stats_kernel(accum_brightness, large_steps, accept, frame_unnormalised, pixels_num, pass_num):
    """kmltStatsKernel (integrator_kmlt.cpp:441-470) operation by operation and in the kernel's summation order, so that its four doubles can be
    compared with ==: avgBrightness = sum over chains with a large step of accumBrightness / double(largeSteps), divided by their number;
    actualBrightness = sum of double(contribFunc(pixel)) over the first pixels_num pixels, divided by pixels_num; the acceptance rate; normConst =
    double(float(pass_num) * float(avg / actual)), or 1 when no chain made a large step or the frame is black."""
    large = np.asarray(large_steps, np.int64)
    has = large > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(has, np.asarray(accum_brightness, np.float64) / np.where(has, large, 1).astype(np.float64), 0.0)
    b, with_large = _block_sum(share), _block_sum(has.astype(np.float64))
    acc = _block_sum(np.asarray(accept, np.float64))
    px = np.asarray(frame_unnormalised, F32).reshape(-1, 4)[:pixels_num]
    actual = _block_sum(K.contrib_func(px[:, :3]).astype(np.float64))
    avg = b / with_large if with_large > 0.0 else 0.0
    actual = actual / float(pixels_num) if pixels_num else 0.0
    ok = with_large > 0.0 and actual != 0.0
    norm = float(F32(pass_num) * F32(avg / actual)) if ok else 1.0
    return np.array([avg, actual, acc / (float(pixels_num) * float(pass_num)), norm], np.float64)


def colour_from_raw(raw, waves, sc, terminate_waves=False):
    """PathTraceF's colour (integrator_kmlt.cpp:224-227) from the recorded raw components raw[i] = exposure * accumColor[i], for a scene whose
    exposure is 1 (then raw IS accumColor and exposure * SpectralCamRespoceToRGB(accumColor) is the conversion itself): float32 [n, 4], .w 0.
    terminate_waves: the path carries RAY_FLAG_WAVES_DIVERGED."""
    assert float(sc.exposure_mult) == 1.0, "raw / exposure is not exact for other exposures"
    return QS.contribution(QS.spectral_cam_response_to_rgb(raw, waves, sc, terminate_waves), 1.0, 4)

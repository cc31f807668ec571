"""numpy restatement of the spectral side of IntegratorQMC (spectrum.h: SampleWavelengths, SampleUniformSpectrum, SpectrumToXYZ, XYZToRGB;
integrator_spectrum.cpp: SpectralCamRespoceToRGB; mlt/integrator_qmc.cpp: GetRandomNumbersSpec, the layer scatter of kernel_ContributeToImage).
Not a test.

Every product, sum and quotient is ONE float32 operation in the order the reference's source gives them; arrays carry one sample per row, four
wavelengths per sample in the last axis. Tables (spectra, the CIE observer) are the scene's own: SceneData.spec_values / spec_offset_sz / cie_xyz.
"""
import numpy as np

import qmc_reference as Q
from gbuffer_reference import _a, f32

LAMBDA_MIN, LAMBDA_MAX = f32(360.0), f32(830.0)
SPECTRUM_SAMPLE_SZ = 4
CIE_Y_INTEGRAL = f32(106.856895)
N_CIE_SAMPLES = 471


def wave_samples(table, n, spd_dim):
    """IntegratorQMC::GetRandomNumbersSpec for samples 0 .. n - 1 (or an array of indices) when m_qmcSpdDim != 0: dimension spd_dim of the sample."""
    assert spd_dim != 0, "dimension 0 means the pseudo generator draws the number"
    s = np.arange(n, dtype=np.uint32) if np.isscalar(n) else np.asarray(n, np.uint32)
    return Q.rnd_float(table, s, spd_dim)


def sample_wavelengths(u, a=LAMBDA_MIN, b=LAMBDA_MAX):
    """SampleWavelengths (spectrum.h:58-75): res[0] = lerp(a, b, u) = a + u * (b - a); res[i] = res[i - 1] + (b - a) / 4, wrapped into [a, b]."""
    u = _a(np.atleast_1d(np.asarray(u, np.float32)))
    a, b = f32(a), f32(b)
    res = np.zeros(u.shape + (SPECTRUM_SAMPLE_SZ,), np.float32)
    res[..., 0] = _a(a + _a(u * f32(b - a)))
    delta = f32(f32(b - a) / f32(SPECTRUM_SAMPLE_SZ))
    for i in range(1, SPECTRUM_SAMPLE_SZ):
        r = _a(res[..., i - 1] + delta)
        res[..., i] = np.where(r > b, _a(a + _a(r - b)), r)
    return res


def sample_uniform_spectrum(values, offset, waves):
    """SampleUniformSpectrum (spectrum.h:106-126): the 1 nm table from LAMBDA_MIN, linear between neighbours, indices clamped to [0, WAVESN - 1]."""
    values = _a(np.asarray(values, np.float32))
    waves = _a(waves)
    wavesn = int(LAMBDA_MAX - LAMBDA_MIN)
    i1 = np.minimum(np.maximum(_a(waves - LAMBDA_MIN), f32(0.0)), f32(wavesn - 1)).astype(np.int32)       # float -> int truncates
    i2 = np.minimum(i1 + 1, wavesn - 1)
    x1 = _a(LAMBDA_MIN + i1.astype(np.float32))
    y1, y2 = values[offset + i1], values[offset + i2]
    return _a(y1 + _a(_a(waves - x1) * _a(y2 - y1)))


def xyz_to_rgb(x, y, z):
    """XYZToRGB (spectrum.h:211-218): a * x - b * y - c * z, left to right."""
    r = _a(_a(_a(f32(3.240479) * x) - _a(f32(1.537150) * y)) - _a(f32(0.498535) * z))
    g = _a(_a(_a(f32(-0.969256) * x) + _a(f32(1.875991) * y)) + _a(f32(0.041556) * z))
    b = _a(_a(_a(f32(0.055648) * x) - _a(f32(0.204043) * y)) + _a(f32(1.057311) * z))
    return np.stack([r, g, b], axis=-1)


def _average(v):
    """SpectrumAverage: the left-to-right sum over the four samples, divided by SPECTRUM_SAMPLE_SZ."""
    s = _a(v[..., 0])
    for i in range(1, SPECTRUM_SAMPLE_SZ):
        s = _a(s + v[..., i])
    return _a(s / f32(SPECTRUM_SAMPLE_SZ))


def spectrum_to_xyz(spec, waves, cie_xyz, terminate_waves=False):
    """SpectrumToXYZ (spectrum.h:151-208) with lambda_min / lambda_max = LAMBDA_MIN / LAMBDA_MAX. terminate_waves: a bool or a bool per sample;
    then pdf[0] is divided by 4 and the other three samples are dropped. cie_xyz: float32 [471, >= 3]."""
    spec, waves = _a(spec), _a(waves)
    cie = _a(np.asarray(cie_xyz, np.float32)).reshape(-1, np.asarray(cie_xyz).shape[-1])
    term = np.broadcast_to(np.asarray(terminate_waves, bool), spec.shape[:-1])
    pdf0 = f32(f32(1.0) / f32(LAMBDA_MAX - LAMBDA_MIN))
    pdf = np.full(spec.shape, pdf0, np.float32)
    pdf[..., 0] = np.where(term, f32(pdf0 / f32(SPECTRUM_SAMPLE_SZ)), pdf0)
    pdf[..., 1:] = np.where(term[..., None], f32(0.0), pdf0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(pdf != 0, _a(spec / pdf), f32(0.0)).astype(np.float32)
    offset = _a(np.floor(_a(waves + f32(0.5))) - LAMBDA_MIN).astype(np.int64)
    inside = (offset >= 0) & (offset < min(N_CIE_SAMPLES, cie.shape[0]))
    o = np.where(inside, offset, 0)
    out = []
    for k in range(3):
        c = np.where(inside, cie[o, k], f32(0.0)).astype(np.float32)
        out.append(_a(_average(_a(c * s)) / CIE_Y_INTEGRAL))
    return out


def spectral_cam_response_to_rgb(spec, waves, sc, terminate_waves=False):
    """SpectralCamRespoceToRGB (integrator_spectrum.cpp:68-124) for the scene sc: without a camera response spectrum the CIE route
    (SpectrumToXYZ, XYZToRGB); with one, the response spectra sampled at the wavelengths, xyz = sum_i spec[i] * response[i] from zero, and
    XYZToRGB when the response type is CAM_RESPONCE_XYZ (0)."""
    spec, waves = _a(spec), _a(waves)
    ids = [int(v) for v in sc.cam_response_spectrum_id]
    if ids[0] < 0:
        from hydracore3_amd.scene import cie_xyz_fit
        cie = sc.cie_xyz if sc.cie_xyz is not None else cie_xyz_fit()
        x, y, z = spectrum_to_xyz(spec, waves, np.asarray(cie, np.float32).reshape(N_CIE_SAMPLES, -1), terminate_waves)
        return xyz_to_rgb(x, y, z)
    offs = np.asarray(sc.spec_offset_sz, np.int64).reshape(-1, 2)
    rx = sample_uniform_spectrum(sc.spec_values, int(offs[ids[0], 0]), waves)
    ry = sample_uniform_spectrum(sc.spec_values, int(offs[ids[1], 0]), waves) if ids[1] >= 0 else rx
    rz = sample_uniform_spectrum(sc.spec_values, int(offs[ids[2], 0]), waves) if ids[2] >= 0 else ry
    xyz = []
    for r in (rx, ry, rz):
        acc = np.zeros(spec.shape[:-1], np.float32)
        for i in range(SPECTRUM_SAMPLE_SZ):
            acc = _a(acc + _a(spec[..., i] * r[..., i]))
        xyz.append(acc)
    if int(sc.cam_response_type) == 0:
        return xyz_to_rgb(*xyz)
    return np.stack(xyz, axis=-1)


def contribution(rgb, exposure, channels):
    """IntegratorQMC::kernel_ContributeToImage for channels <= 4: exposure * rgb, and for one channel its luma, as float32 [n, 4] records."""
    rgb = _a(rgb)
    c = _a(f32(exposure) * rgb)
    out = np.zeros(rgb.shape[:-1] + (4,), np.float32)
    if channels == 1:
        out[..., 0] = _a(_a(_a(f32(0.2126) * c[..., 0]) + _a(f32(0.7152) * c[..., 1])) + _a(f32(0.0722) * c[..., 2]))
    else:
        out[..., :3] = c
    return out


def layer_index(waves, channels):
    """The wavelength layer of kernel_ContributeToImage for channels > 4 (integrator_qmc.cpp:270-279, integrator_pt.cpp:643-655):
    t = (lambda - LAMBDA_MIN) / (LAMBDA_MAX - LAMBDA_MIN); min(int(float(channels) * t), channels - 1)."""
    waves = _a(np.asarray(waves, np.float32))
    t = _a(_a(waves - LAMBDA_MIN) / f32(LAMBDA_MAX - LAMBDA_MIN))
    return np.minimum(_a(f32(channels) * t).astype(np.int64), channels - 1)


def env_spectrum(sc, waves):
    """kernel_HitEnvironment for a path that leaves the scene with throughput 1: SampleUniformSpectrum(envSpec) * (envSpecMult / CIE_Y_integral)."""
    offs = np.asarray(sc.spec_offset_sz, np.int64).reshape(-1, 2)
    k = f32(f32(sc.env_spec_mult) / CIE_Y_INTEGRAL)
    return _a(sample_uniform_spectrum(sc.spec_values, int(offs[int(sc.env_spec_id), 0]), waves) * k)

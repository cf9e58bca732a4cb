"""References for the device low-res synthesis (fdn_kspace_downsample), in numpy alone (nothing from the package):

    pipeline(vel, mag, venc, crops, snr_linear, g, mag_scale=1, single=False)
        The degradation with SUPPLIED standard normals g, written from the formulas of include/fdn.h: x = mag mag_scale exp(i pi vel/venc);
        fftn; keep frequencies 0..c-1, -c..-1 per axis; sigma = sqrt(mean|F|^2 / snr); Re F += sigma g; ifftn; |z| ratio and angle/pi venc.
        float64 / complex128, or with single=True the same statements in float32 / complex64: the fp32 yardstick of the device's error.
    philox4x32_10(counter, key)       the generator in Python integers (four 32-bit words each way)
    philox_normals(n, seed, stream_id, first=0)   float64 standard normals of elements first .. first + n - 1, by the mapping of fdn.h
    rebuild(lr_vel, lr_mag, venc, ratio)          z = lr_mag / ratio * exp(i pi lr_vel / venc), in float64
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def crops_of(shape, crop_ratio):
    return tuple(int((n // 2) * crop_ratio) for n in shape)


def _keep(n, c):
    return np.r_[0:c, n - c:n]


def pipeline(vel, mag, venc, crops, snr_linear, g, mag_scale=1.0, single=False):
    real, cplx = (np.float32, np.complex64) if single else (np.float64, np.complex128)
    vel, mag, g = np.asarray(vel, real), np.asarray(mag, real), np.asarray(g, real)
    venc, mag_scale, snr_linear = real(venc), real(mag_scale), real(snr_linear)
    phase = (vel / venc * real(np.pi)).astype(real)
    x = ((mag * mag_scale) * np.exp(1j * phase.astype(cplx))).astype(cplx)
    F = np.fft.fftn(x)
    assert F.dtype == cplx
    for axis, c in enumerate(crops):
        F = np.take(F, _keep(F.shape[axis], c), axis=axis)
    F0 = F.copy()
    sigma = np.sqrt(np.mean(np.abs(F) ** 2, dtype=real) / snr_linear).astype(real)
    F = (F + (sigma * g)).astype(cplx)
    z = np.fft.ifftn(F)
    ratio = real(F.size / vel.size)
    return dict(z=z, F=F0, sigma=sigma, ratio=ratio, lr_mag=np.abs(z) * ratio, lr_vel=np.angle(z) / real(np.pi) * venc)


def rebuild(lr_vel, lr_mag, venc, ratio):
    return np.asarray(lr_mag, np.float64) / float(ratio) * np.exp(1j * np.pi * np.asarray(lr_vel, np.float64) / float(venc))


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _philox_words(e, seed, stream_id):
    """Words 0 and 1 for an array of element indices e (uint64), vectorised in uint64 arithmetic."""
    e = np.asarray(e, np.uint64)
    m = np.uint64(MASK)
    c0, c1 = e & m, e >> np.uint64(32)
    c2 = np.full_like(e, int(stream_id) & MASK)
    c3 = np.full_like(e, (int(stream_id) >> 32) & MASK)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1


def philox_normals(n, seed, stream_id, first=0):
    x0, x1 = _philox_words(np.arange(first, first + n, dtype=np.uint64), seed, stream_id)
    u1 = ((x0 >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (x1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

"""Float64 restatement of the eight input corruptions of include/rcu.h ("Input corruptions") in numpy / scipy, independent of rcu_amd.corruption:
the yardstick of tests/test_gpu_corruption.py and of tests/golden/generate_corruptions.py.  ``a`` is the amount as the kernels see it,
(float)amount; images are float32 ``[n, C, H, W]``, image i the slice with global index first_sample + i."""
import numpy as np
import scipy.ndimage

from oracle import mask_oracle as mo

KINDS = ('gaussian_noise', 'gaussian_blur', 'downsample', 'contrast', 'intensity_shift', 'bias_field', 'ghosting', 'channel_drop')
SHAPES = ((4, 15, 16), (3, 30, 30), (4, 70, 67), (1, 33, 64))        # (C, H, W) of the GPU tests, n = 3
FIRST_SAMPLE = 2 ** 32 + 5
_M64 = (1 << 64) - 1


def make_input(shape, n=3, seed=29):
    """Seeded z-score-like planes with structure (a smooth blob per channel under the noise) and a per-channel offset, float32 [n, C, H, W]."""
    c, h, w = shape
    rng = np.random.default_rng([seed, c, h, w])
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    x = rng.standard_normal((n, c, h, w))
    for i in range(n):
        for k in range(c):
            x[i, k] += 2.0 * np.exp(-((yy - 0.3 * k + 0.2 * i) ** 2 + (xx + 0.1 * k) ** 2) * 3.0) + 0.25 * k
    return x.astype(np.float32)


def normals(key, first_sample, n, hw, channels):
    """z[i, p, c] = z(K = key, g = first_sample + i, p, s = 0, class = c) of "Test-time logit sampling" with C = channels (float64 transcendentals of
    the float32 uniforms, as normals_np of tests/test_gpu_logit_sampling.py)."""
    q = (channels + 3) // 4
    g = np.uint64(first_sample) + np.arange(n, dtype=np.uint64)
    cnt = np.empty((n, hw, q, 4), dtype=np.uint32)
    cnt[..., 0] = np.arange(hw, dtype=np.uint32)[None, :, None]
    cnt[..., 1] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    cnt[..., 2] = (g >> np.uint64(32)).astype(np.uint32)[:, None, None]
    cnt[..., 3] = (np.uint32(0x80000000) | np.arange(q, dtype=np.uint32))[None, None, :]
    key = int(key) & _M64
    w = mo.philox4x32_10(cnt, (key & 0xFFFFFFFF, key >> 32))
    u = (((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)
    z = np.empty(u.shape, dtype=np.float64)
    for k in range(2):
        r = np.sqrt(-2.0 * np.log(u[..., 2 * k]))
        z[..., 2 * k] = r * np.cos(2.0 * np.pi * u[..., 2 * k + 1])
        z[..., 2 * k + 1] = r * np.sin(2.0 * np.pi * u[..., 2 * k + 1])
    return z.reshape(n, hw, q * 4)[..., :channels]


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def bias_coefficients(key, channels):
    coef = np.empty((channels, 8), dtype=np.float64)
    for c in range(channels):
        for e in range(8):
            t = splitmix64((int(key) + (8 * c + e + 1) * 0x9E3779B97F4A7C15) & _M64)
            coef[c, e] = 2.0 * ((t >> 11) / 2.0 ** 53) - 1.0
        coef[c] /= np.abs(coef[c]).sum()
    return coef


def bias_field(key, channels, h, w):
    """f_c(i, j), float64 [C, H, W]: sum over (u, v) in {0, 1, 2}^2 without (0, 0) of coef[c][3 u + v - 1] cos(pi u (i + 0.5) / H) cos(pi v (j + 0.5) / W)."""
    coef = bias_coefficients(key, channels)
    f = np.zeros((channels, h, w))
    for u in range(3):
        for v in range(3):
            if u == 0 and v == 0:
                continue
            au = np.cos(np.pi * u * (np.arange(h) + 0.5) / h)[:, None]
            bv = np.cos(np.pi * v * (np.arange(w) + 0.5) / w)[None, :]
            f += coef[:, 3 * u + v - 1, None, None] * (au * bv)[None]
    return f


def downsample(x, k):
    x = np.asarray(x, dtype=np.float64)
    y = np.empty_like(x)
    h, w = x.shape[-2:]
    for i0 in range(0, h, k):
        for j0 in range(0, w, k):
            y[..., i0:i0 + k, j0:j0 + k] = x[..., i0:i0 + k, j0:j0 + k].mean(axis=(-2, -1), keepdims=True)
    return y


def reference(kind, x, amount, key=0, first_sample=0):
    """float64 ``[n, C, H, W]`` (intensity_shift and channel_drop: the float32 numpy result, which the kernels must equal bit for bit)."""
    x32 = np.asarray(x, dtype=np.float32)
    x = x32.astype(np.float64)
    n, c, h, w = x.shape
    a = float(np.float32(amount))
    if kind == 'gaussian_noise':
        z = normals(key, first_sample, n, h * w, c)                       # [n, hw, C]
        return x + a * z.transpose(0, 2, 1).reshape(n, c, h, w)
    if kind == 'gaussian_blur':
        y = np.empty_like(x)
        for i in range(n):
            for k in range(c):
                y[i, k] = scipy.ndimage.gaussian_filter(x[i, k], sigma=float(amount), mode='reflect', truncate=4.0)
        return y
    if kind == 'downsample':
        return downsample(x, int(amount))
    if kind == 'contrast':
        m = x.mean(axis=(-2, -1), keepdims=True)
        return m + a * (x - m)
    if kind == 'intensity_shift':
        return x32 + np.float32(amount)
    if kind == 'bias_field':
        return x * np.exp(a * bias_field(key, c, h, w))[None]
    if kind == 'ghosting':
        return x + a * np.roll(x, -(h // 2), axis=-2)
    if kind == 'channel_drop':
        y = x32.copy()
        for k in range(c):
            if (int(amount) >> k) & 1:
                y[:, k] = 0
        return y
    raise ValueError(kind)


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def tolerance(kind, x, y, amount, z=None):
    """The bound of the kernel against ``reference``, elementwise or scalar (float64); 0 means bit-equal.
    gaussian_noise   a 2e-6 max(1, |z|) + 2^-23 max(1, |y|): the project's own tolerance for these normals, plus the rounding of the fmaf
    gaussian_blur    4 (r + 1) 2^-23 max|x|: two fmaf chains of 2 r + 1 taps with sum w = 1, plus the float32 taps
    downsample       (k^2 + 1) 2^-24 max|x|: a sequential float32 sum of k^2 terms and one division
    contrast         2^-21 max|x|;   bias_field  2e-6 |y|;   ghosting  one float32 ulp of y"""
    xmax = float(np.abs(x).max())
    a = float(np.float32(amount))
    if kind == 'gaussian_noise':
        return a * 2e-6 * np.maximum(1.0, np.abs(z)) + 2.0 ** -23 * np.maximum(1.0, np.abs(y))
    if kind == 'gaussian_blur':
        return 4 * (radius(amount) + 1) * 2.0 ** -23 * xmax
    if kind == 'downsample':
        return (int(amount) ** 2 + 1) * 2.0 ** -24 * xmax
    if kind == 'contrast':
        return 2.0 ** -21 * xmax
    if kind == 'bias_field':
        return 2e-6 * np.abs(y)
    if kind == 'ghosting':
        return np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    return 0.0


KEY = 0x0123456789ABCDEF % (2 ** 63 - 1)
# (kind, amount) of the per-kind checks; channel_drop's mask keeps channel 0 and drops channel 1 (and 3 where there is one), so it needs C >= 2
CASES = (('gaussian_noise', 0.3), ('gaussian_noise', 0.0), ('gaussian_blur', 0.5), ('gaussian_blur', 1.5), ('gaussian_blur', 3.0),
         ('downsample', 2), ('downsample', 3), ('downsample', 7), ('downsample', 16), ('contrast', 0.45), ('intensity_shift', 0.3),
         ('bias_field', 0.6), ('ghosting', 0.25), ('channel_drop', None))


def case_amount(kind, amount, channels):
    if kind != 'channel_drop':
        return amount
    return None if channels < 2 else float(sum(1 << k for k in (1, 3) if k < channels))


def case_name(kind, amount):
    return kind if amount is None else '{}_{:g}'.format(kind, amount)

"""numpy float64 restatement of the input pipeline's semantics (include/m3d.h,
m3d_normalize_image / m3d_augment_image / m3d_flip_boxes): the reference for
tests/test_gpu_preprocess.py, pinned by tests/test_normref.py.

normalize: percentiles by numpy's `linear` method written out (v = q / 100
(n - 1), lo = floor(v), g = v - lo, a = s[lo], b = s[min(lo + 1, n - 1)], the
two-branch lerp), clip, mean and population std, tanh(0.5 y), all in float64
and left unrounded.  Philox4x32-10 in pure numpy."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def percentile_linear(sorted64, q):
    n = sorted64.size
    v = (q / 100.0) * (n - 1)
    lo = int(np.floor(v))
    g = v - lo
    a, b = sorted64[lo], sorted64[min(lo + 1, n - 1)]
    return a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g)


def stats(volume):
    """(p1, p99, mean, std) of a volume in float64 (mean / std of the clipped volume)."""
    x = np.asarray(volume).astype(np.float64).ravel()
    s = np.sort(x)
    p1, p99 = percentile_linear(s, 1.0), percentile_linear(s, 99.0)
    c = np.clip(x, p1, p99)
    return float(p1), float(p99), float(np.mean(c)), float(np.std(c))


def normalize(raw, transpose=True):
    """raw (Z,Y,X) [or [H,W,D] with transpose=False] -> ([H,W,D] float64, unrounded; (p1, p99, mean, std))."""
    x = np.asarray(raw).astype(np.float64)
    if transpose:
        x = np.transpose(x, (1, 2, 0))
    p1, p99, mean, std = stats(x)
    y = np.clip(x, p1, p99) - mean
    if std > 0:
        y = y / std
    return np.tanh(0.5 * y), (p1, p99, mean, std)


def normalize_f32(raw, transpose=True):
    """The same formula evaluated in float32 from the float64 statistics:
    float32 clip bounds, mean, std and tanh -- the error bar of the GPU test."""
    x = np.asarray(raw).astype(np.float32)
    if transpose:
        x = np.transpose(x, (1, 2, 0))
    p1, p99, mean, std = (np.float32(v) for v in stats(x))
    y = np.clip(x, p1, p99) - mean
    if std > 0:
        y = y / std
    return np.tanh(y * np.float32(0.5))


def philox4x32_10(counter, key):
    """counter [...,4], key [2] (or [...,2]) uint32 -> [...,4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    key = np.asarray(key)
    k0, k1 = key[..., 0].astype(np.uint64), key[..., 1].astype(np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack(c, -1).astype(np.uint32)


def uniform53(a, b):
    """((a >> 5) 2^26 + (b >> 6)) 2^-53 in [0, 1)."""
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) \
        * (1.0 / 9007199254740992.0)


def _random(n, stream, seed):
    idx = np.arange(n, dtype=np.uint64)
    ctr = np.stack([idx & np.uint64(MASK), idx >> np.uint64(32), np.full(n, stream, np.uint64),
                    np.zeros(n, np.uint64)], -1).astype(np.uint32)
    return philox4x32_10(ctr, np.array([seed[0] & MASK, seed[1] & MASK], np.uint32))


def flip(a, mask):
    axes = [i for i in range(3) if mask & (1 << i)]
    return np.flip(a, axes) if axes else a


def augment(image, flip_mask=0, brightness_delta=0.0, noise_std=0.0, seed=(0, 0)):
    """-> (float32 image after the flips and the brightness leg, bit for bit;
    float64 Gaussian noise to add, or None).  Random numbers are counted by the
    linear index in the output."""
    v = np.ascontiguousarray(flip(np.asarray(image, np.float32), flip_mask))
    n = v.size
    if brightness_delta > 0:
        vmin, vmax = np.float32(v.min()), np.float32(v.max())
        scale = float(np.float32(brightness_delta)) * (float(vmax) - float(vmin) + 1e-6)
        r = _random(n, 0, seed)
        u = uniform53(r[:, 0], r[:, 1]).reshape(v.shape)
        noise = (-scale + 2.0 * scale * u).astype(np.float32)
        v = np.minimum(np.maximum(v + noise, vmin), vmax)
    gauss = None
    if noise_std > 0:
        r = _random(n, 1, seed)
        u1, u2 = uniform53(r[:, 0], r[:, 1]), uniform53(r[:, 2], r[:, 3])
        gauss = (float(noise_std) * np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)).reshape(v.shape)
    return v, gauss


def flip_boxes(boxes, shape, mask):
    b = np.array(boxes, np.float32).reshape(-1, 6)
    for axis in range(3):
        if mask & (1 << axis):
            lo, hi = np.float32(shape[axis]) - b[:, axis + 3], np.float32(shape[axis]) - b[:, axis]
            b[:, axis], b[:, axis + 3] = lo, hi
    return b


def volumes():
    """The normalisation volumes of tests/test_normref.py and tests/test_gpu_preprocess.py, as (Z,Y,X)."""
    rng = np.random.default_rng(11)
    u16 = rng.integers(0, 65536, (5, 7, 67)).astype(np.uint16)
    u16.flat[0], u16.flat[-1] = 0, 65535
    f32 = (rng.normal(size=(12, 40, 40)) * 3).astype(np.float32)
    f32[0, 0, :4] = [0.0, -0.0, -7.5, 9.25]
    return {
        "one": rng.integers(0, 256, (1, 1, 1)).astype(np.uint8),
        "g0": rng.integers(0, 4000, (1, 1, 101)).astype(np.uint16),
        "nine": rng.normal(size=(1, 3, 3)).astype(np.float32),
        "u16_full_range": u16,
        "u8_six_levels": (rng.integers(0, 6, (33, 9, 70)) * 40 + 3).astype(np.uint8),
        "f32_signed": f32,
        "odd": rng.integers(0, 1000, (3, 5, 7)).astype(np.uint16),
        "grid_cap": rng.integers(0, 256, (64, 96, 128)).astype(np.uint8),
    }


VOLUMES = volumes()

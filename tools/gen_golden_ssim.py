"""Writes tests/golden/g19_ssim.npz: two small image pairs and their SSIM as the reference computes it.

    python tools/gen_golden_ssim.py

The reference (main_sampling.py:520) calls
    skimage.metrics.structural_similarity(x, orig, data_range=x.max() - x.min(), channel_axis=0)
on float32 images that went through inverse_data_transform.  skimage is not a dependency of this project, so the figures
here are a RESTATEMENT of `skimage.metrics.structural_similarity`, not its output: the same statements in the same order on
`scipy.ndimage.uniform_filter` (the filter skimage calls), at skimage's defaults -- win_size 7, use_sample_covariance,
K1 = 0.01, K2 = 0.03, each channel plane on its own, the plane's mean over the map cropped by (win_size - 1) // 2 taken in
float64, the planes' values stored in the images' float type and averaged there.

Per pair k in {a: (3, 24, 28), b: (3, 64, 64)} the file holds
    x_k, y_k      float32 images in [-1.2, 1.2] (sample, original; the transform's clamp is exercised)
    ssim32_k      the restatement in float32 -- skimage's code path for float32 input
    ssim64_k      the same statements on the float32-transformed images promoted to float64
    range_k       the float32 data_range, max - min of the transformed x_k
"""
import os

import numpy as np
from scipy.ndimage import uniform_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_unit_range(v):
    """inverse_data_transform of the reference (rescaled data): clamp((v + 1) / 2, 0, 1) in float32."""
    return np.clip((v.astype(np.float32) + np.float32(1.0)) / np.float32(2.0), np.float32(0.0), np.float32(1.0))


def ssim_plane(im1, im2, data_range, win_size=7):
    K1, K2 = 0.01, 0.03
    NP = win_size ** im1.ndim
    cov_norm = NP / (NP - 1)
    ux = uniform_filter(im1, size=win_size)
    uy = uniform_filter(im2, size=win_size)
    uxx = uniform_filter(im1 * im1, size=win_size)
    uyy = uniform_filter(im2 * im2, size=win_size)
    uxy = uniform_filter(im1 * im2, size=win_size)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range
    C1 = (K1 * R) ** 2
    C2 = (K2 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    S = (A1 * A2) / (B1 * B2)
    pad = (win_size - 1) // 2
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def ssim(x01, y01, dtype):
    """channel_axis=0: every plane on its own, the values kept in `dtype` and averaged there."""
    data_range = x01.max() - x01.min()                     # float32, as the reference passes it
    x01, y01 = x01.astype(dtype), y01.astype(dtype)
    planes = np.empty(x01.shape[0], dtype=dtype)
    for ch in range(x01.shape[0]):
        planes[ch] = ssim_plane(x01[ch], y01[ch], dtype(data_range))
    return planes.mean()


def smooth_pair(rng, shape, noise, lo=-1.2):
    """A smooth random original (low-resolution noise, bilinearly enlarged) and a sample = original + noise."""
    c, h, w = shape
    low = rng.uniform(lo, 1.2, size=(c, 5, 5))
    yy, xx = np.linspace(0, 4, h), np.linspace(0, 4, w)
    y0, x0 = np.minimum(yy.astype(int), 3), np.minimum(xx.astype(int), 3)
    fy, fx = (yy - y0)[None, :, None], (xx - x0)[None, None, :]
    g = lambda dy, dx: low[:, y0 + dy][:, :, x0 + dx]
    orig = (g(0, 0) * (1 - fy) + g(1, 0) * fy) * (1 - fx) + (g(0, 1) * (1 - fy) + g(1, 1) * fy) * fx
    sample = orig + noise * rng.standard_normal(shape)
    # row-major copies: the fancy indexing above leaves `orig` in another memory order, which .npy would keep
    return (np.ascontiguousarray(np.clip(sample, -1.2, 1.2), dtype=np.float32),
            np.ascontiguousarray(orig, dtype=np.float32))


def main():
    rng = np.random.default_rng(19)
    out = {}
    # pair b stays above -0.6, so only the upper clamp acts and its data_range is not 1
    for key, shape, noise, lo in (('a', (3, 24, 28), 0.15, -1.2), ('b', (3, 64, 64), 0.04, -0.4)):
        x, y = smooth_pair(rng, shape, noise, lo)
        x01, y01 = to_unit_range(x), to_unit_range(y)
        out[f'x_{key}'], out[f'y_{key}'] = x, y
        out[f'ssim32_{key}'] = np.float32(ssim(x01, y01, np.float32))
        out[f'ssim64_{key}'] = np.float64(ssim(x01, y01, np.float64))
        out[f'range_{key}'] = np.float32(x01.max() - x01.min())
        print(key, shape, 'ssim32', out[f'ssim32_{key}'], 'ssim64', out[f'ssim64_{key}'], 'range', out[f'range_{key}'],
              'clamped', int((np.abs(x) > 1).sum()), int((np.abs(y) > 1).sum()))
    np.savez(os.path.join(ROOT, 'tests', 'golden', 'g19_ssim.npz'), **out)


if __name__ == '__main__':
    main()

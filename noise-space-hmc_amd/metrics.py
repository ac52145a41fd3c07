"""Report stage: the metrics the reference's `sample_image` takes of the collected samples (main_sampling.py:488-561),
on the device.

    psnr(samples, x_orig)            [B, S]   PSNR of every sample against its chain's original        (:517-519)
    ssim(samples, x_orig)            [B, S]   skimage's default SSIM, data_range = the sample's range  (:520)
    sample_moments(samples)          posterior-mean image, per-pixel std map, its min-max normalised picture (:494-497)
    summarize(samples, x_orig)       per-chain means and ddof=1 stds (:526-538) + the maps, one device->host read
    save_std_map(map01, path)        the `std_dev_map_{idx}.png` picture (:499-507)

`samples` is what `sampler.hmc` returns for B chains, float32 [B, S, C, H, W] in [-1, 1], with `x_orig` [B, C, H, W]; one
chain may be passed as [S, C, H, W] with a [1, C, H, W] (or [C, H, W]) original.  The kernels (csrc/metrics.hip) apply the
reference's inverse_data_transform themselves.  There is no CPU path and no host SSIM: skimage is not a dependency.
LPIPS (:521) is not served: it needs the `lpips` package and its VGG weights.
"""
import os

import numpy as np
import torch

from . import _lib
from . import kernels as K


def _block(samples, x_orig=None):
    """-> (samples [B, S, C, H, W], x_orig [B, C, H, W] or None, squeeze): the one-chain form gets its chain axis."""
    squeeze = samples.dim() == 4
    if squeeze:
        samples = samples[None]
        if x_orig is not None and x_orig.dim() == 3:
            x_orig = x_orig[None]
    if samples.dim() != 5:
        raise _lib.NhmcError(f'samples must be [B, S, C, H, W] or [S, C, H, W], got {tuple(samples.shape)}')
    for t in (samples, x_orig):
        if t is not None and not t.is_cuda:
            raise _lib.NhmcError(f'nhmc.metrics works on GPU tensors (got {t.device}); there is no CPU path')
    return samples, x_orig, squeeze


def psnr(samples, x_orig):
    """PSNR (dB) of each sample against its chain's original -> float32 [B, S] ([S] for the one-chain form); per sample
    the bits of `kernels.psnr`."""
    samples, x_orig, squeeze = _block(samples, x_orig)
    out = K.psnr_samples(samples, x_orig)
    return out[0] if squeeze else out


def ssim(samples, x_orig):
    """`skimage.metrics.structural_similarity(sample, orig, data_range=sample.max() - sample.min(), channel_axis=0)` of the
    transformed images, as the reference calls it -> float64 [B, S] ([S] for the one-chain form).  Needs H, W >= 7."""
    samples, x_orig, squeeze = _block(samples, x_orig)
    out = K.ssim(samples, x_orig)
    return out[0] if squeeze else out


def sample_moments(samples):
    """-> (mean [B, C, H, W], std_map [B, H, W], std_map_normalised [B, H, W]): the mean of the raw samples, the reference's
    `x.std(dim=0).mean(dim=0)` of the transformed ones and `(std - min) / (max - min)` of that map.  Needs S >= 2."""
    mean, std_map, _minmax, norm, squeeze = _moments(samples)
    return (mean[0], std_map[0], norm[0]) if squeeze else (mean, std_map, norm)


def _moments(samples):
    samples, _, squeeze = _block(samples)
    mean, std_map, minmax = K.sample_moments(samples)
    return mean, std_map, minmax, K.std_map_normalise(std_map, minmax), squeeze


def summarize(samples, x_orig):
    """Everything the report prints or saves for B chains with S samples each, with one device->host read.

    -> dict of float64 numpy arrays [B]: psnr_mean, psnr_std, ssim_mean, ssim_std (np.mean / np.std(ddof=1) over the
    chain's samples, :526-538; std is 0 for S = 1), std_map_min, std_map_max; `n_samples` (int); and the device tensors
    mean [B, C, H, W], std_map, std_map_normalised [B, H, W].  S = 1: PSNR and SSIM but no map (the reference's
    `len(xt) > 1`): the three tensors are None and the map's min / max NaN.  S = 0: all scalars NaN but the stds, which
    are 0 -- the CLI's row for a chain whose final phase collected nothing."""
    samples, x_orig, _ = _block(samples, x_orig)
    B, S = samples.shape[:2]
    nan, zero = np.full(B, np.nan), np.zeros(B)
    out = dict(psnr_mean=nan, psnr_std=zero, ssim_mean=nan.copy(), ssim_std=zero.copy(), std_map_min=nan.copy(),
               std_map_max=nan.copy(), n_samples=S, mean=None, std_map=None, std_map_normalised=None)
    if S == 0:
        return out
    cols = [psnr(samples, x_orig).double(), ssim(samples, x_orig)]
    if S > 1:
        out['mean'], out['std_map'], minmax, out['std_map_normalised'], _ = _moments(samples)
        cols.append(minmax.double())
    host = torch.cat(cols, dim=1).cpu().numpy()                              # the one read: [B, 2S (+2)]
    ps, ss = host[:, :S], host[:, S:2 * S]
    out['psnr_mean'], out['ssim_mean'] = ps.mean(axis=1), ss.mean(axis=1)
    if S > 1:
        out['psnr_std'], out['ssim_std'] = ps.std(axis=1, ddof=1), ss.std(axis=1, ddof=1)
        out['std_map_min'], out['std_map_max'] = host[:, 2 * S], host[:, 2 * S + 1]
    return out


HOT_BREAKS = (0.365079, 0.746032)          # where matplotlib's `hot` ramp saturates red, then green


def hot_colours(map01):
    """matplotlib's `hot` colour map written out: [H, W] in [0, 1] -> uint8 [H, W, 3]."""
    v = np.asarray(map01, dtype=np.float64)
    r, g = HOT_BREAKS
    rgb = np.stack([v / r, (v - r) / (g - r), (v - g) / (1.0 - g)], axis=-1)
    return np.round(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


def save_std_map(map01, path):
    """The normalised std map [H, W] as an 8-bit PNG in the `hot` colours, one pixel per map entry.

    Deviation from main_sampling.py:499-507: the reference draws the map into a matplotlib figure with a colour bar
    ("Std Dev") and the title "Pixel-wise Std Dev Across Samples" at 300 dpi; this writes the picture alone -- no colour
    bar, no title, no matplotlib."""
    from PIL import Image
    if isinstance(map01, torch.Tensor):
        map01 = map01.detach().cpu().numpy()
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(hot_colours(map01)).save(path)

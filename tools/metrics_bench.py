"""Times the report stage (nhmc.metrics) at the flagship batch: 64 chains x 20 samples x 3 x 256 x 256.

    python tools/metrics_bench.py [--chains 64] [--samples 20] [--size 256] [--reps 5]

HIP events around
    summarize      psnr + range + ssim + moments + normalise + the one device->host read
    psnr loop      the per-sample `kernels.psnr` loop the CLI ran before (one launch pair and one read per chain), as context
    ssim           `kernels.ssim` alone with the ranges given, against its algorithmic traffic of one read of every sample
                   and one of its original per sample, 2 * B * S * 4N bytes
and prints one JSON line.  A measurement aid, no gate.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nhmc.kernels as K  # noqa: E402
from nhmc import metrics  # noqa: E402


def timed(fn, reps):
    fn()                                                     # warm-up (allocator, first launch)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]                    # median, ms


def psnr_loop(samples, x_orig):
    rows = []
    for k in range(samples.shape[0]):
        ps = torch.stack([K.psnr(samples[k, j:j + 1], x_orig[k:k + 1])[0] for j in range(samples.shape[1])])
        rows.append([float(ps.mean()), float(ps.std())])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=64)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    B, S, N = a.chains, a.samples, 3 * a.size * a.size
    low = torch.rand(B, 3, a.size // 16, a.size // 16, device=dev, generator=g) * 2 - 1
    x_orig = torch.nn.functional.interpolate(low, size=a.size, mode='bicubic', align_corners=False).clamp(-1, 1).contiguous()
    samples = (x_orig[:, None] + 0.1 * torch.randn(B, S, 3, a.size, a.size, device=dev, generator=g)).contiguous()
    rng = K.sample_range(samples)
    res = {'chains': B, 'samples': S, 'size': a.size,
           'summarize_ms': timed(lambda: metrics.summarize(samples, x_orig), a.reps),
           'psnr_loop_ms': timed(lambda: psnr_loop(samples, x_orig), a.reps),
           'psnr_samples_ms': timed(lambda: K.psnr_samples(samples, x_orig), a.reps),
           'range_ms': timed(lambda: K.sample_range(samples), a.reps),
           'ssim_ms': timed(lambda: K.ssim(samples, x_orig, rng), a.reps),
           'moments_ms': timed(lambda: K.sample_moments(samples), a.reps)}
    res['ssim_algorithmic_bytes'] = 2 * B * S * 4 * N
    res['ssim_algorithmic_GBps'] = res['ssim_algorithmic_bytes'] / (res['ssim_ms'] * 1e-3) / 1e9
    print(json.dumps(res))


if __name__ == '__main__':
    main()

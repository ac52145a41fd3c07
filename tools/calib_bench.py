"""Times the calibration kernel (nhmc_calibration) at 8 images x 8 replicas x 20 samples x 3 x 256 x 256.

    python tools/calib_bench.py [--images 8] [--replicas 8] [--samples 20] [--size 256] [--reps 9]

HIP events around
    calibration    `kernels.calibration`: rank and z-score maps, the rank histogram and the eight sums of every image
    chain_diag     `kernels.chain_diag` on the same block: the same traffic, more arithmetic
    moments        `kernels.sample_moments` on the same block viewed as [images, replicas * samples, ...]: it reads the same
                   bytes with no load in flight ahead of its arithmetic and is the yardstick
in one process, their timed windows alternating (calibration, chain_diag, moments, calibration, ...), each against its
algorithmic traffic -- one read of every sample (and of x_orig), images * replicas * samples * 4N bytes, plus the maps it
writes -- as a fraction of the 8 TB/s HBM peak, and prints one JSON line.  A measurement aid, no gate.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nhmc.kernels as K  # noqa: E402

HBM_PEAK = 8e12
INNER = 10                                                   # calls per timed window: a window of a few ms, not one launch


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


def timed(fns, reps):
    """{name: fn} -> {name: median ms per call}, the windows of the functions alternating."""
    for fn in fns.values():
        fn()                                                 # warm-up (allocator, first launch)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window(fn))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--replicas', type=int, default=8)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    G, R, S, N = a.images, a.replicas, a.samples, 3 * a.size * a.size
    samples = (0.3 * torch.randn(G * R, S, 3, a.size, a.size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    x_orig = (0.3 * torch.randn(G, 3, a.size, a.size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    pooled = samples.view(G, R * S, 3, a.size, a.size)
    read = G * R * S * 4 * N
    ms = timed({'calibration': lambda: K.calibration(samples, x_orig, R), 'chain_diag': lambda: K.chain_diag(samples, R),
                'moments': lambda: K.sample_moments(pooled)}, a.reps)
    res = {'images': G, 'replicas': R, 'samples': S, 'size': a.size}
    nbytes = {'calibration': read + G * 4 * N + G * 8 * N,                   # + x_orig, + the z and counts maps
              'chain_diag': read + G * 8 * N,                                # + the two maps
              'moments': read + G * 4 * N + G * 4 * a.size * a.size}         # + the mean image and the std map
    for k in ('calibration', 'chain_diag', 'moments'):
        res[k + '_ms'] = ms[k]
        res[k + '_bytes'] = nbytes[k]
        res[k + '_GBps'] = nbytes[k] / (ms[k] * 1e-3) / 1e9
        res[k + '_fraction_of_8TBps'] = res[k + '_GBps'] * 1e9 / HBM_PEAK
    res['calibration_over_moments'] = ms['calibration'] / ms['moments']
    res['calibration_over_chain_diag'] = ms['calibration'] / ms['chain_diag']
    print(json.dumps(res))


if __name__ == '__main__':
    main()

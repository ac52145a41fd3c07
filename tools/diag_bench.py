"""Times the convergence kernel (nhmc_chain_diag) at 8 images x 8 replicas x 20 samples x 3 x 256 x 256.

    python tools/diag_bench.py [--images 8] [--replicas 8] [--samples 20] [--size 256] [--reps 9]

HIP events around
    chain_diag     `kernels.chain_diag`: split R-hat, ESS and the six summaries of every image
    moments        `kernels.sample_moments` on the same block viewed as [images, replicas * samples, ...]: it reads the same
                   bytes and is the yardstick
both against their algorithmic traffic -- one read of every sample, images * replicas * samples * 4N bytes, plus the maps
they write -- as a fraction of the 8 TB/s HBM peak, and prints one JSON line.  A measurement aid, no gate.
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


def timed(fn, reps):
    fn()                                                     # warm-up (allocator, first launch)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / INNER)
    return sorted(times)[len(times) // 2]                    # median, ms per call


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
    pooled = samples.view(G, R * S, 3, a.size, a.size)
    read = G * R * S * 4 * N
    res = {'images': G, 'replicas': R, 'samples': S, 'size': a.size,
           'chain_diag_ms': timed(lambda: K.chain_diag(samples, R), a.reps),
           'moments_ms': timed(lambda: K.sample_moments(pooled), a.reps)}
    res['chain_diag_bytes'] = read + G * 8 * N                               # + the two maps
    res['moments_bytes'] = read + G * 4 * N + G * 4 * a.size * a.size         # + the mean image and the std map
    for k in ('chain_diag', 'moments'):
        res[k + '_GBps'] = res[k + '_bytes'] / (res[k + '_ms'] * 1e-3) / 1e9
        res[k + '_fraction_of_8TBps'] = res[k + '_GBps'] * 1e9 / HBM_PEAK
    res['chain_diag_over_moments'] = res['chain_diag_ms'] / res['moments_ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()

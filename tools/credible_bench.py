"""Times the credible-interval kernels (nhmc_credible) at 8 images x 1 replica x 20 samples (n = 20, the register path) and
at 8 x 8 x 20 (n = 160, the general path), both at 3 x 256 x 256.

    python tools/credible_bench.py [--images 8] [--samples 20] [--size 256] [--reps 9] [--replicas 1 8]

HIP events around
    credible       `kernels.credible` at the rank of the 0.9 interval: the three maps and the six summaries of every image
    calibration    `kernels.calibration` on the same block: it reads the same bytes once, and is the yardstick
    torch_sort     `torch.sort(pooled, dim=1)` on the block viewed as [images, replicas * samples, ...]: what a user who
                   wants the interval does today (a second tensor of the block's size and an index tensor twice that)
in one process, their timed windows alternating (credible, calibration, torch_sort, credible, ...), the median of `reps`
windows of 10 calls each.  The two kernels are set against their algorithmic traffic -- one read of every sample and of
x_orig, n * 4 + 4 bytes per element, plus the maps they write, 12 bytes per element for the interval -- as a fraction of
the 8 TB/s HBM peak; the general path reads the draws 16 times, mostly from cache, so its figure is the useful rate, not
the traffic.  Prints one JSON line per configuration.  A measurement aid, no gate.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nhmc.kernels as K  # noqa: E402
from nhmc import metrics  # noqa: E402

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


def one(G, R, S, size, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    N, n = 3 * size * size, R * S
    samples = (0.3 * torch.randn(G * R, S, 3, size, size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    x_orig = (0.3 * torch.randn(G, 3, size, size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    pooled = samples.view(G, n, 3, size, size)
    k = metrics.coverage_rank(n, 0.9)
    ms = timed({'credible': lambda: K.credible(samples, x_orig, R, k), 'calibration': lambda: K.calibration(samples, x_orig, R),
                'torch_sort': lambda: torch.sort(pooled, dim=1)}, reps)
    read = G * n * 4 * N + G * 4 * N
    res = {'images': G, 'replicas': R, 'samples': S, 'size': size, 'n': n, 'k': k,
           'path': os.environ.get('NHMC_CREDIBLE_PATH') or ('register' if n <= 64 else 'general')}
    nbytes = {'credible': read + G * 12 * N, 'calibration': read + G * 8 * N}
    for name in ('credible', 'calibration', 'torch_sort'):
        res[name + '_ms'] = ms[name]
        if name in nbytes:
            res[name + '_bytes'] = nbytes[name]
            res[name + '_GBps'] = nbytes[name] / (ms[name] * 1e-3) / 1e9
            res[name + '_fraction_of_8TBps'] = res[name + '_GBps'] * 1e9 / HBM_PEAK
    res['credible_over_calibration'] = ms['credible'] / ms['calibration']
    res['credible_over_torch_sort'] = ms['credible'] / ms['torch_sort']
    print(json.dumps(res), flush=True)
    del samples, pooled
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--replicas', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for R in a.replicas:
        one(a.images, R, a.samples, a.size, a.reps, dev)


if __name__ == '__main__':
    main()

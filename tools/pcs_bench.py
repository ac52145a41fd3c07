"""Times the principal-component kernels (nhmc_sample_gram, nhmc_sample_project) at 8 images x 1 replica x 20 samples
(n = 20, two row blocks) and at 8 x 8 x 20 (n = 160, ten of sixteen row blocks), both at 3 x 256 x 256.

    python tools/pcs_bench.py [--images 8] [--samples 20] [--size 256] [--reps 9] [--replicas 1 8] [--count 3]
    python tools/pcs_bench.py --remarks-only          (no GPU: hipcc's resource usage of csrc/pcs.hip, per kernel)

HIP events around
    sample_gram      `kernels.sample_gram`: the [n, n] fp64 Gram matrix of every image's pooled draws about the first
    sample_project   `kernels.sample_project` with `count` coefficient rows: the direction images
    sample_moments   `kernels.sample_moments` on the same block: it reads the same bytes once, and is the yardstick
    torch_gram       `Xc = (X - X[:, :1]).double(); Xc @ Xc.mT` on the block viewed as [images, n, N]: what a user who wants
                     the Gram matrix does today (an fp64 copy of the block, then a batched GEMM)
in one process, their timed windows alternating, the median of `reps` windows of 10 calls each.  The kernels are set against
their algorithmic traffic -- one read of every sample and of x_orig, n * 4 + 4 bytes per element -- as a fraction of the
8 TB/s HBM peak, and the Gram kernel against the fp64 matrix work it issues: 2 * 256 * 4 flops per 16 x 16 x 4 MFMA over the
block pairs it runs.  Prints one JSON line per configuration.  A measurement aid, no gate.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12
INNER = 10                                                   # calls per timed window: a window of a few ms, not one launch


def remarks():
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/pcs.hip -> {kernel: {VGPRs, AGPRs, ScratchSize, Occupancy, LDS}}."""
    import importlib
    build = importlib.import_module('nhmc.build')
    src = os.path.join(build.CSRC, 'pcs.hip')
    cmd = [build.hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            name = subprocess.run(['c++filt', '-p', m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            name = name.replace('(anonymous namespace)::', '')
            out[name] = {}
            continue
        m = re.search(r'remark: +(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)', line)
        if m and name:
            out[name][m.group(1).split(' [')[0]] = int(m.group(2))
    return out


def window(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


def timed(torch, fns, reps):
    """{name: fn} -> {name: median ms per call}, the windows of the functions alternating."""
    for fn in fns.values():
        fn()                                                 # warm-up (allocator, first launch)
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window(torch, fn))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def one(torch, K, G, R, S, size, count, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    N, n = 3 * size * size, R * S
    samples = (0.3 * torch.randn(G * R, S, 3, size, size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    x_orig = (0.3 * torch.randn(G, 3, size, size, device=dev, generator=g)).clamp_(-1, 1).contiguous()
    coef = torch.randn(G, count, n, dtype=torch.float64, device=dev, generator=g)
    pooled = samples.view(G, n, N)

    def torch_gram():
        xc = (pooled - pooled[:, :1]).double()
        return xc @ xc.mT
    ms = timed(torch, {'sample_gram': lambda: K.sample_gram(samples, x_orig, R),
                       'sample_project': lambda: K.sample_project(samples, coef, R),
                       'sample_moments': lambda: K.sample_moments(samples), 'torch_gram': torch_gram}, reps)
    ours, theirs = K.sample_gram(samples, None, R)[:, :n - 1, :n - 1], torch_gram()[:, 1:, 1:]
    scale = torch.sqrt(torch.diagonal(theirs, dim1=1, dim2=2))
    read = G * n * 4 * N + G * 4 * N
    rb = (n + 15) // 16
    res = {'images': G, 'replicas': R, 'samples': S, 'size': size, 'n': n, 'count': count, 'row_blocks': rb,
           'gram_vs_torch_max_rel': float(((ours - theirs).abs() / (scale[:, :, None] * scale[:, None, :])).max())}
    nbytes = {'sample_gram': read, 'sample_project': G * n * 4 * N + G * count * 4 * N, 'sample_moments': G * n * 4 * N}
    for name, t in ms.items():
        res[name + '_ms'] = t
        if name in nbytes:
            res[name + '_bytes'] = nbytes[name]
            res[name + '_GBps'] = nbytes[name] / (t * 1e-3) / 1e9
            res[name + '_fraction_of_8TBps'] = res[name + '_GBps'] * 1e9 / HBM_PEAK
    res['sample_gram_mfma_TFLOPs'] = G * (rb * (rb + 1) // 2) * (N // 4) * 2 * 256 * 4 / (ms['sample_gram'] * 1e-3) / 1e12
    res['sample_gram_over_moments'] = ms['sample_gram'] / ms['sample_moments']
    res['sample_gram_over_torch_gram'] = ms['sample_gram'] / ms['torch_gram']
    print(json.dumps(res), flush=True)
    del samples, pooled
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--replicas', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--count', type=int, default=3)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--remarks-only', action='store_true')
    a = ap.parse_args()
    print(json.dumps({'resource_usage': remarks()}), flush=True)
    if a.remarks_only:
        return
    import torch
    import nhmc.kernels as K
    dev = torch.device('cuda:0')
    for R in a.replicas:
        one(torch, K, a.images, R, a.samples, a.size, a.count, a.reps, dev)


if __name__ == '__main__':
    main()

"""Fused GroupNorm (+ FiLM + SiLU) kernels of the score network against the HBM roofline, at the FFHQ U-Net's shapes
(64 chains), one-pass (csrc/gn_onepass.hip) and two-pass (csrc/gn_act.hip, NHMC_GN_ONEPASS=0) side by side in one process.
Passes over the activation that the bandwidth figures divide by:
    two-pass   forward = stats (R x) + apply (R x, W y) = 3;  backward = stats (R x, dy) + apply (R x, dy, W dx) = 5
    one-pass   forward = R x, W y = 2;                        backward = R x, dy, W dx = 3
    bwd+add    the backward with a second gradient added in the same pass (`add=`, what every block's first GroupNorm
               launches): one more read, 6 and 4 passes
    default    what kernels.gn_act_fwd / gn_act_bwd run without a switch (nhmc_gn_onepass_prefers): the one-pass forward,
               and the two-pass backward fed from the slab totals the one-pass forward leaves (fwd_splits = 1)
A shape the one-pass kernels do not cover prints its two-pass figures twice.
Usage: python tools/gn_bench.py [chains] [rounds]"""
import os
import sys
import torch
sys.path.insert(0, '.')
import nhmc.kernels as K

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device('cuda')


def timeit(f, n=10):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def mode(onepass):
    os.environ['NHMC_GN_ONEPASS'] = '1' if onepass else '0'


for Cc, res in ((128, 256), (256, 256), (128, 128), (256, 128), (384, 128), (256, 64), (512, 64), (512, 32), (1024, 16)):
    x = torch.randn(B, Cc, res, res, device=dev)
    dy = torch.randn_like(x)
    ad = torch.randn_like(x)
    gamma, beta = torch.randn(Cc, device=dev), torch.randn(Cc, device=dev)
    film = torch.randn(B, 2 * Cc, device=dev)
    nbytes = x.numel() * 4
    one = K.gn_onepass_splits(B, Cc, 32, res * res)
    t = {(o, d): [] for o in (False, True) for d in 'fba'}
    t['default', 'b'] = []
    for _ in range(ROUNDS):                       # interleaved rounds: the two variants see the same clocks
        for o in (False, True):
            mode(o)
            y, ws, splits = K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, film=film, onepass=True)
            t[o, 'f'].append(timeit(lambda: K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, film=film, onepass=True)))
            t[o, 'b'].append(timeit(lambda: K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, film, ws, splits, onepass=True)))
            t[o, 'a'].append(timeit(lambda: K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, film, ws, splits, add=ad, onepass=True)))
            if o:
                t['default', 'b'].append(timeit(lambda: K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, film, ws, splits)))
            del y
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    pf, pb = (2, 3) if one else (3, 5)
    ratio = lambda d: (f'{med[True, d] / med[False, d]:.3f}', f'{min(t[True, d]) / min(t[False, d]):.3f}')
    print(f'[{B},{Cc},{res},{res}] {nbytes / 2 ** 30:.2f} GiB  one-pass splits {one}\n'
          f'    two-pass: fwd {med[False, "f"] * 1e3:.0f} us = {3 * nbytes / med[False, "f"] / 1e9:.2f} TB/s (3 passes), '
          f'bwd {med[False, "b"] * 1e3:.0f} us = {5 * nbytes / med[False, "b"] / 1e9:.2f} TB/s (5 passes)\n'
          f'    one-pass: fwd {med[True, "f"] * 1e3:.0f} us = {pf * nbytes / med[True, "f"] / 1e9:.2f} TB/s ({pf} passes), '
          f'bwd {med[True, "b"] * 1e3:.0f} us = {pb * nbytes / med[True, "b"] / 1e9:.2f} TB/s ({pb} passes)\n'
          f'    bwd+add: two-pass {med[False, "a"] * 1e3:.0f} us = {6 * nbytes / med[False, "a"] / 1e9:.2f} TB/s (6 passes), '
          f'one-pass {med[True, "a"] * 1e3:.0f} us = {(pb + 1) * nbytes / med[True, "a"] / 1e9:.2f} TB/s ({pb + 1} passes), '
          f'one-pass / two-pass {ratio("a")[0]} (min over rounds {ratio("a")[1]})\n'
          f'    default route: bwd {med["default", "b"] * 1e3:.0f} us = {med["default", "b"] / med[False, "b"]:.3f} of the two-pass backward on a two-pass workspace\n'
          f'    one-pass / two-pass: fwd {med[True, "f"] / med[False, "f"]:.3f}  bwd {med[True, "b"] / med[False, "b"]:.3f}'
          f'   (min over rounds: fwd {min(t[True, "f"]) / min(t[False, "f"]):.3f}  bwd {min(t[True, "b"]) / min(t[False, "b"]):.3f})',
          flush=True)
    del x, dy, ad
os.environ.pop('NHMC_GN_ONEPASS', None)

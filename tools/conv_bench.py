"""The Winograd MFMA convolution (csrc/wino_conv.hip) against F.conv2d at the FFHQ U-Net's covered 3x3 shapes, forward and
backward-data, 64 chains, both alternating in one process.  The shapes are those of the model itself
(unet.conv3x3_shapes(), a walk over create_model(**FFHQ_CONFIG)) that the kernel covers in both directions.
Per (C, K, resolution, direction): 100 warm-up calls of each (the clocks ramp for longer than a few calls), then the
median of 3 rounds of 10 event-timed launches per variant on rotating buffers that together exceed the 256 MiB Infinity
Cache.  Prints microseconds, the ratio kernel / F.conv2d and
TFLOP/s in direct-convolution terms (2 * 9 * N * C * K * H * W).  Rows at or below 0.90 are what
nhmc_conv3x3_wino_prefers and nhmc_conv3x3_wino_narrow_prefers may list.
Usage: python tools/conv_bench.py [chains] [rounds] [--epilogue] [--only=C,K,res] [--latent] [--up] [--skip-bias]
--epilogue adds, per forward row, the kernel with its (acc + bias) + add epilogue against kernel + k_bias_add2.
--latent measures the latent sampler's two networks instead (ldm.conv3x3_shapes; chains defaults to 16, the chain count of
BASELINE configs[4]): the score network's covered shapes forward only (it is evaluated without gradient), the first-stage
decoder's forward and backward-data.  Rows at or below 0.90 with K % 64 == 32 are what nhmc_conv3x3_wino_k32_prefers may
list; the others go to the two tables above.
--up times, at the up-sampling ResBlocks' shapes that the wide kernel covers (up_shapes(); --only=C,K,res overrides), the
passes that carry a nearest 2x upsample to the convolution against the kernel's upsample forms (nhmc_conv3x3_wino_up), both
alternating in one process: conv1 forward, sr_Ht + kernel against IN_UP on the low-res tensor; conv2 forward with its
residual, sr_Ht + kernel with bias and add against ADD_UP; conv1 backward-data, kernel + sr_H + mul_(4) against OUT_POOL.
Prints microseconds of each, the ratio fused / materialised, and the convolution alone for scale.
--skip-bias times conv2's forward pass of the ResBlocks whose skip path is a 1x1 convolution and whose conv2 runs on the wide
kernel (skip_shapes(); --only=C,K,res overrides), both alternating in one process: the broadcast bias pass over the skip
tensor (`s.add_(b1)`, what the vendor path runs behind its GEMM) + the kernel with bias and add, against the kernel with the
skip bias in its epilogue (nhmc_conv3x3_wino_skip).  Prints microseconds of each, the ratio, and the bias pass alone."""
import sys
import torch
import torch.nn.functional as F
sys.path.insert(0, '.')
import nhmc.kernels as K
from nhmc import ldm, unet


def default_shapes(chains=64):
    """(C, K, resolution) of the 3x3 convolutions of one FFHQ_CONFIG forward pass that the kernel covers forward and
    backward-data at this chain count, in the order of unet.conv3x3_shapes()."""
    return tuple((c, k, res) for c, k, res, _ in unet.conv3x3_shapes()
                 if K.conv3x3_wino_covers(chains, c, k, res, res) and K.conv3x3_wino_covers(chains, k, c, res, res))


def latent_shapes(chains=16):
    """(C, K, resolution, directions) of the 3x3 convolutions of the latent sampler's networks that the kernel covers at this
    chain count, in the order of ldm.conv3x3_shapes: the U-Net's forward only (directions = (False,)), then the decoder's,
    forward and backward-data (covered in both)."""
    rows = [(c, k, res, (False,)) for c, k, res, _ in ldm.conv3x3_shapes('unet') if K.conv3x3_wino_k32_covers(chains, c, k, res, res)]
    rows += [(c, k, res, (False, True)) for c, k, res, _ in ldm.conv3x3_shapes('decoder')
             if K.conv3x3_wino_k32_covers(chains, c, k, res, res) and K.conv3x3_wino_k32_covers(chains, k, c, res, res)]
    return tuple(rows)


def up_shapes(chains=64):
    """(C, K, output resolution) of conv1 of every up-sampling ResBlock of FFHQ_CONFIG that the upsample forms cover."""
    with torch.device('meta'):
        model = unet.create_model(**unet.FFHQ_CONFIG)
    seen, hooks = [], []
    for mod in model.modules():
        if isinstance(mod, unet.ResBlock) and mod.up:
            hooks.append(mod.register_forward_hook(
                lambda m, args, out: seen.append((m.in_layers[2].in_channels, m.in_layers[2].out_channels, out.shape[-1]))))
    size = unet.FFHQ_CONFIG['image_size']
    with torch.no_grad():
        model(torch.empty(1, 3, size, size, device='meta'), torch.zeros(1, device='meta'))
    for h in hooks:
        h.remove()
    return tuple(s for s in sorted(set(seen), key=lambda s: -s[2])
                 if K.conv3x3_wino_up_covers(chains, s[0], s[1], s[2], s[2]) and K.conv3x3_wino_up_covers(chains, s[1], s[0], s[2], s[2]))


def up_mode(B, ROUNDS, only):
    """--up: see the module docstring."""
    dev = torch.device('cuda')
    print(f'chains {B}, rounds {ROUNDS}: us materialised | us fused | ratio (best of rounds) | us convolution alone')
    for Cc, Kk, res in only or up_shapes(B):
        w = torch.randn(Kk, Cc, 3, 3, device=dev) / (9 * Cc) ** 0.5
        bias = torch.randn(Kk, device=dev)
        low, full = res // 2, res
        nbuf = max(2, -(-(320 << 20) // (B * min(Cc, Kk) * low * low * 4)))
        lows = [torch.randn(B, Cc, low, low, device=dev) for _ in range(nbuf)]
        nfull = max(2, -(-(320 << 20) // (B * min(Cc, Kk) * full * full * 4)))
        fulls = [torch.randn(B, Cc, full, full, device=dev) for _ in range(nfull)]
        grads = [torch.randn(B, Kk, full, full, device=dev) for _ in range(nfull)]
        adds = [torch.randn(B, Kk, low, low, device=dev) for _ in range(nfull)]
        up = lambda t, ch: K.sr_Ht(t.reshape(B, -1), 2, ch, full, 1.0).view(B, ch, full, full)
        legs = (
            ('conv1 fwd  IN_UP   ', lows, lambda t: K.conv3x3_wino(up(t, Cc), w), lambda t: K.conv3x3_wino_up(t, w, K.WINO_IN_UP),
             lambda t: K.conv3x3_wino(fulls[0], w)),
            ('conv2 fwd  ADD_UP  ', list(zip(fulls, adds)), lambda t: K.conv3x3_wino(t[0], w, bias, up(t[1], Kk)),
             lambda t: K.conv3x3_wino_up(t[0], w, K.WINO_ADD_UP, bias, t[1]), lambda t: K.conv3x3_wino(t[0], w, bias, grads[0])),
            ('conv1 bwd  OUT_POOL', grads, lambda t: K.sr_H(K.conv3x3_wino(t, w, backward=True), 2).mul_(4.0),
             lambda t: K.conv3x3_wino_up(t, w, K.WINO_OUT_POOL, backward=True), lambda t: K.conv3x3_wino(t, w, backward=True)),
        )
        for name, bufs, mat, fused, alone in legs:
            if name.startswith('conv2') and Cc != Kk:
                continue
            for _ in range(100 // len(bufs) + 1):
                for t in bufs:
                    mat(t)
                    fused(t)
            tm, tf, ta = [], [], []
            for _ in range(ROUNDS):
                tm.append(timeit(mat, bufs))
                tf.append(timeit(fused, bufs))
                ta.append(timeit(alone, bufs))
            med = lambda v: sorted(v)[len(v) // 2]
            print(f'[{B},{Cc}->{Kk},{res}x{res}] {name}: {med(tm) * 1e3:8.0f} | {med(tf) * 1e3:8.0f} | {med(tf) / med(tm):.3f} '
                  f'({min(tf) / min(tm):.3f}) | {med(ta) * 1e3:8.0f}', flush=True)
        del lows, fulls, grads, adds, w


def skip_shapes(chains=64):
    """(C, K, resolution) of conv2 of every ResBlock of FFHQ_CONFIG with a 1x1 skip convolution that the skip-bias form covers."""
    with torch.device('meta'):
        model = unet.create_model(**unet.FFHQ_CONFIG)
    seen, hooks = [], []
    for mod in model.modules():
        if isinstance(mod, unet.ResBlock) and isinstance(mod.skip_connection, torch.nn.Conv2d):
            hooks.append(mod.register_forward_hook(
                lambda m, args, out: seen.append((m.out_layers[3].in_channels, m.out_layers[3].out_channels, out.shape[-1]))))
    size = unet.FFHQ_CONFIG['image_size']
    with torch.no_grad():
        model(torch.empty(1, 3, size, size, device='meta'), torch.zeros(1, device='meta'))
    for h in hooks:
        h.remove()
    return tuple((c, k, res, seen.count((c, k, res))) for c, k, res in sorted(set(seen), key=lambda s: -s[2])
                 if K.conv3x3_wino_skip_covers(chains, c, k, res, res))


def skip_mode(B, ROUNDS, only):
    """--skip-bias: see the module docstring."""
    dev = torch.device('cuda')
    print(f'chains {B}, rounds {ROUNDS}: us bias pass + kernel | us fused | ratio (best of rounds) | us bias pass alone | blocks per evaluation')
    for Cc, Kk, res, count in [o + (0,) for o in only] or skip_shapes(B):
        w = torch.randn(Kk, Cc, 3, 3, device=dev) / (9 * Cc) ** 0.5
        b2, b1 = torch.randn(Kk, device=dev), torch.randn(Kk, device=dev)
        nbuf = max(2, -(-(320 << 20) // (B * min(Cc, Kk) * res * res * 4)))
        bufs = [(torch.randn(B, Cc, res, res, device=dev), torch.randn(B, Kk, res, res, device=dev)) for _ in range(nbuf)]
        b1v = b1.view(1, -1, 1, 1)
        split = lambda t: K.conv3x3_wino(t[0], w, b2, t[1].add_(b1v))
        fused = lambda t: K.conv3x3_wino_skip(t[0], w, b2, t[1], b1)
        alone = lambda t: t[1].add_(b1v)
        for _ in range(100 // nbuf + 1):
            for t in bufs:
                split(t)
                fused(t)
        ts, tf, ta = [], [], []
        for _ in range(ROUNDS):
            ts.append(timeit(split, bufs))
            tf.append(timeit(fused, bufs))
            ta.append(timeit(alone, bufs))
        med = lambda v: sorted(v)[len(v) // 2]
        print(f'[{B},{Cc}->{Kk},{res}x{res}] conv2 fwd: {med(ts) * 1e3:8.0f} | {med(tf) * 1e3:8.0f} | {med(tf) / med(ts):.3f} '
              f'({min(tf) / min(ts):.3f}) | {med(ta) * 1e3:8.0f} | {count}', flush=True)
        del bufs, w


def timeit(f, bufs, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        f(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    dev = torch.device('cuda')
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    LATENT = '--latent' in sys.argv
    B = int(args[0]) if len(args) > 0 else 16 if LATENT else 64
    ROUNDS = int(args[1]) if len(args) > 1 else 3
    EPILOGUE = '--epilogue' in sys.argv
    if '--skip-bias' in sys.argv:
        return skip_mode(B, ROUNDS, [tuple(int(v) for v in a[7:].split(',')) for a in sys.argv[1:] if a.startswith('--only=')])
    if '--up' in sys.argv:
        return up_mode(B, ROUNDS, [tuple(int(v) for v in a[7:].split(',')) for a in sys.argv[1:] if a.startswith('--only=')])
    SHAPES = latent_shapes(B) if LATENT else tuple(s + ((False, True),) for s in default_shapes(B))
    print(f'chains {B}, rounds {ROUNDS}: us wino | us F.conv2d | ratio | TFLOP/s wino | TFLOP/s F.conv2d')
    ONLY = [tuple(int(v) for v in a[7:].split(',')) for a in sys.argv[1:] if a.startswith('--only=')]
    for Cc, Kk, res, directions in [o + ((False, True),) for o in ONLY] or SHAPES:
        w = (torch.randn(Kk, Cc, 3, 3, device=dev) / (9 * Cc) ** 0.5)
        flop = 2 * 9 * B * Cc * Kk * res * res
        for backward in directions:
            cin = Kk if backward else Cc
            nbuf = max(2, -(-(320 << 20) // (B * cin * res * res * 4)))
            bufs = [torch.randn(B, cin, res, res, device=dev) for _ in range(nbuf)]
            x_shape = (B, Cc, res, res)
            if backward:
                vendor = lambda t: torch.nn.grad.conv2d_input(x_shape, w, t, 1, 1)
            else:
                vendor = lambda t: F.conv2d(t, w, None, 1, 1)
            ours = lambda t: K.conv3x3_wino(t, w, backward=backward)
            for _ in range(100 // nbuf + 1):
                for t in bufs:
                    ours(t)
                    vendor(t)
            tv, to = [], []
            for _ in range(ROUNDS):                     # interleaved rounds: the two variants see the same clocks
                to.append(timeit(ours, bufs))
                tv.append(timeit(vendor, bufs))
            mo, mv = sorted(to)[len(to) // 2], sorted(tv)[len(tv) // 2]
            line = (f'[{B},{Cc}->{Kk},{res}x{res}] {"bwd" if backward else "fwd"}: {mo * 1e3:8.0f} | {mv * 1e3:8.0f} | {mo / mv:.3f} '
                    f'(best of rounds {min(to) / min(tv):.3f}) | {flop / mo / 1e9:6.1f} | {flop / mv / 1e9:6.1f}')
            if EPILOGUE and not backward:
                bias, add = torch.randn(Kk, device=dev), torch.randn(B, Kk, res, res, device=dev)
                fused = lambda t: K.conv3x3_wino(t, w, bias, add)
                split = lambda t: K.bias_add2(K.conv3x3_wino(t, w), bias, add)
                for t in bufs:
                    fused(t)
                    split(t)
                tf, ts = [], []
                for _ in range(ROUNDS):
                    tf.append(timeit(fused, bufs))
                    ts.append(timeit(split, bufs))
                mf, ms = sorted(tf)[len(tf) // 2], sorted(ts)[len(ts) // 2]
                line += f' | epilogue fused {mf * 1e3:.0f} us vs kernel + bias_add2 {ms * 1e3:.0f} us = {mf / ms:.3f}'
                del bias, add
            print(line, flush=True)
            del bufs
        del w


if __name__ == '__main__':
    main()

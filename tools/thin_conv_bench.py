"""The four thin 3x3 passes of the FFHQ U-Net on the vendor library's path, as the network calls them: `input_blocks[0]`
(3 -> 128, F.conv2d with its bias) and `out[2]` (128 -> 6, F.conv2d with its bias), forward and backward-data
(torch.nn.grad.conv2d_input), at 256 x 256 and 64 chains.  One side of each is a 2.15 GB tensor, the other at most 0.1 GB, so
the floor of a pass is one crossing of the wide tensor.
Per pass: 100 warm-up calls, then the median of `rounds` rounds of 10 event-timed launches on rotating buffers that together
exceed the 256 MiB Infinity Cache (tools/conv_bench.py's method).  Prints microseconds (median, best round), the GB/s of the
compulsory traffic (both tensors once; the broadcast bias pass of the forward calls is the library's own business and is
inside the time), that as a share of the 8 TB/s peak, and the GFMA of the pass.  Each pass also runs on the direct
packed-FMA kernels (csrc/thin_conv.hip: nhmc_conv3x3_thin_in where the input is thin, nhmc_conv3x3_thin_out where the output
is), alternating with the vendor call round by round in the same process: its microseconds, GB/s and the ratio kernel /
vendor (median, best of rounds).  The routing rule is <= 0.90 of the vendor sequence's time (nhmc_conv3x3_thin_in_prefers,
nhmc_conv3x3_thin_out_prefers).
Usage: python tools/thin_conv_bench.py [chains] [rounds] [resolution]"""
import sys
import torch
import torch.nn.functional as F
sys.path.insert(0, '.')
import nhmc.kernels as K

PEAK_GBS = 8000.0


def timeit(f, bufs, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        f(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def passes(B, res, dev):
    """(name, input channels of the call, the vendor call, the kernel's call or None, bytes of both tensors, FMAs)."""
    w_in = torch.randn(128, 3, 3, 3, device=dev) / 27 ** 0.5
    b_in = torch.randn(128, device=dev)
    w_out = torch.randn(6, 128, 3, 3, device=dev) / (9 * 128) ** 0.5
    b_out = torch.randn(6, device=dev)
    px = B * res * res
    return (
        ('input_blocks[0] fwd   3->128 + bias', 3, lambda t: F.conv2d(t, w_in, b_in, 1, 1),
         lambda t: K.conv3x3_thin_in(t, w_in, b_in), 4 * px * 131, 27 * 128 * px),
        ('input_blocks[0] bwd 128->3         ', 128, lambda t: torch.nn.grad.conv2d_input((B, 3, res, res), w_in, t, 1, 1),
         lambda t: K.conv3x3_thin_out(t, w_in, backward=True), 4 * px * 131, 27 * 128 * px),
        ('out[2]          fwd 128->6   + bias', 128, lambda t: F.conv2d(t, w_out, b_out, 1, 1),
         lambda t: K.conv3x3_thin_out(t, w_out, b_out), 4 * px * 134, 54 * 128 * px),
        ('out[2]          bwd   6->128       ', 6, lambda t: torch.nn.grad.conv2d_input((B, 128, res, res), w_out, t, 1, 1),
         lambda t: K.conv3x3_thin_in(t, w_out, backward=True), 4 * px * 134, 54 * 128 * px),
    )


def main():
    dev = torch.device('cuda')
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    B = int(args[0]) if len(args) > 0 else 64
    ROUNDS = int(args[1]) if len(args) > 1 else 3
    res = int(args[2]) if len(args) > 2 else 256
    print(f'chains {B}, {res}x{res}, rounds {ROUNDS}: us vendor (median, best) | GB/s of both tensors once | of {PEAK_GBS:.0f} | GFMA')
    for name, cin, vendor, ours, nbytes, fma in passes(B, res, dev):
        nbuf = max(2, -(-(320 << 20) // (B * 128 * res * res * 4)))        # the wide tensor is read or written by every call
        bufs = [torch.randn(B, cin, res, res, device=dev) for _ in range(nbuf)]
        for _ in range(100 // nbuf + 1):
            for t in bufs:
                vendor(t)
                if ours:
                    ours(t)
        tv, to = [], []
        for _ in range(ROUNDS):                         # interleaved rounds: the two variants see the same clocks
            tv.append(timeit(vendor, bufs))
            if ours:
                to.append(timeit(ours, bufs))
        tv.sort()
        to.sort()
        med, best = tv[len(tv) // 2], tv[0]
        line = (f'[{B}] {name}: {med * 1e3:8.0f} {best * 1e3:8.0f} | {nbytes / med / 1e6:7.0f} | {nbytes / med / 1e6 / PEAK_GBS:.3f} | '
                f'{fma / 1e9:5.1f}')
        if ours:
            mo = to[len(to) // 2]
            line += (f' | kernel {mo * 1e3:8.0f} {to[0] * 1e3:8.0f} us, {nbytes / mo / 1e6:7.0f} GB/s = {nbytes / mo / 1e6 / PEAK_GBS:.3f}, '
                     f'ratio {mo / med:.3f} (best of rounds {to[0] / best:.3f})')
        print(line, flush=True)
        del bufs


if __name__ == '__main__':
    main()

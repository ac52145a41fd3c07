"""A few launches of the one-pass GroupNorm kernels (csrc/gn_onepass.hip), forward and input gradient, at the largest and the
smallest FFHQ level, for a counter pass of their own:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES --kernel-trace --output-format csv -d DIR -- \\
        python tools/gn_launches.py [chains] [launches]

Elements per launch, for the instructions per element: chains x C x res^2 (64 x 128 x 256^2 = 536 870 912 and
64 x 1024 x 16^2 = 16 777 216); a wave64 instruction counts once for its 64 lanes."""
import sys

import torch

sys.path.insert(0, '.')
import nhmc.kernels as K

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3

for Cc, res in ((128, 256), (1024, 16)):
    x = torch.randn(B, Cc, res, res, device='cuda')
    dy = torch.randn_like(x)
    gamma, beta = torch.randn(Cc, device='cuda'), torch.randn(Cc, device='cuda')
    film = torch.randn(B, 2 * Cc, device='cuda')
    for _ in range(N):
        y, ws, splits = K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, film=film, onepass=True)
        dx = K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, film, ws, splits, onepass=True)
    torch.cuda.synchronize()
    print(f'[{B},{Cc},{res},{res}] {x.numel()} elements, splits {splits}, {N} launches each way', flush=True)
    del x, dy, y, dx

"""Oracle: probe bookkeeping of the FFHQ-width U-Net fixture G22 (test infrastructure, see oracle/__init__.py).

Shared by oracle/gen_golden_unet_256.py (which writes tests/golden/g22_unet_ffhq_256*.npz) and
tests/test_unet_ffhq_{cpu,gpu}.py (which read them), so that the three agree on what a "group" is:

  forward groups   the output of input_blocks[0..11], middle_block, output_blocks[0..11] and the network output (26)
  gradient groups  the gradient arriving at each of those 25 block outputs, and the input gradient, for one seeded
                   output gradient `gout` (26)

Every group is read at one seeded set of 4096 flat positions (taken modulo the tensor's size) and judged in the metric
max |value - float64 value| over the positions / max |float64 tensor| over the WHOLE tensor.  Nothing here imports the
reference; any module tree with `input_blocks`, `middle_block` and `output_blocks` (nhmc.unet's and the reference's
guided_diffusion/unet_ffhq.py:467-734 alike) can be evaluated.
"""
import hashlib

import numpy as np
import torch

SEED, SCALE = 606, 0.05                               # the weights of G6 (oracle/gen_golden.py g6_unet), at full width
T_STEPS = (750.0, 250.0)                              # a different step per sample: FiLM and `pre` strides
N_PROBE = 4096
BLOCKS = [f'in{i:02d}' for i in range(12)] + ['mid'] + [f'out{i:02d}' for i in range(12)]
FWD = BLOCKS + ['net']                                # execution order of the forward pass
GRAD = ['g_' + b for b in reversed(BLOCKS)] + ['gx']  # execution order of the backward pass
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]       # the engine leg's ladder (timesteps = 3)
ENGINE = ['eng_xt', 'eng_grad']                       # clipped decode and d(sum of losses)/dx of the engine leg


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def seeded_inputs(net, seed=SEED, scale=SCALE):
    """Loads `randn(shape, generator(seed)) * scale` over net.state_dict() in key order and draws, from the same
    generator after the weights, x [2, 3, 256, 256], the output gradient gout [2, 6, 256, 256], the probe positions and
    the engine leg's inputs (mask permutation, x, clean image, noise).  -> dict of CPU tensors (+ three weight hashes)."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: torch.randn(v.shape, generator=g) * scale for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    keys = list(sd)
    out = dict(weight_sha=[sha(sd[k]) for k in (keys[0], keys[len(keys) // 2], keys[-1])])
    out['x'] = torch.randn(2, 3, 256, 256, generator=g)
    out['gout'] = torch.randn(2, 6, 256, 256, generator=g)
    out['pos'] = torch.randint(0, 2 ** 31 - 1, (N_PROBE,), generator=g)
    hw = 256 * 256
    r = 3 * torch.randperm(hw, generator=g)[: int(hw * 0.92)].long()           # main_sampling.py:302-305 (inpaint_random)
    out['missing'] = torch.cat([r, r + 1, r + 2])
    out['eng_x'] = torch.randn(2, 3, 256, 256, generator=g)
    out['eng_img'] = torch.rand(2, 3, 256, 256, generator=g) * 2 - 1
    out['eng_noise'] = 0.1 * torch.randn(2, 3 * (hw - int(hw * 0.92)), generator=g)
    out['t'] = torch.tensor(T_STEPS)
    return out


def block_modules(net):
    return list(net.input_blocks) + [net.middle_block] + list(net.output_blocks)


def probe(t, pos):
    """(values at pos % numel as float64 on the CPU, max |t| as a float)."""
    flat = t.detach().reshape(-1)
    return flat[(pos % flat.numel()).to(flat.device)].double().cpu(), float(flat.abs().max())


def evaluate(net, x, t, gout, pos, digest=False):
    """One forward pass and one input-gradient pass of `net` with a forward hook on each of the 25 blocks and a tensor
    hook on each block output.  -> {group: (probe values, max |tensor|[, sha256 of the tensor])} for FWD + GRAD.
    Only the probes are kept: the 52 tensors of a float64 pass at B = 2 would be 3 GB."""
    rec, hooks = {}, []

    def keep(name, tensor):
        rec[name] = probe(tensor, pos) + ((sha(tensor),) if digest else ())

    def watch(name):
        def fwd(mod, args, out):
            keep(name, out)
            out.register_hook(lambda g: keep('g_' + name, g))
        return fwd
    for name, mod in zip(BLOCKS, block_modules(net)):
        hooks.append(mod.register_forward_hook(watch(name)))
    try:
        xl = x.detach().clone().requires_grad_(True)
        out = net(xl, t)
        keep('net', out)
        keep('gx', torch.autograd.grad(out, xl, gout)[0])
    finally:
        for h in hooks:
            h.remove()
    assert sorted(rec) == sorted(FWD + GRAD)
    return rec


def errors(rec, truth, groups):
    """{group: max |probe - float64 probe| / max |float64 tensor|}; truth[group] = (float64 probes, float64 max)."""
    return {k: float((rec[k][0] - truth[k][0]).abs().max() / truth[k][1]) for k in groups}


def first_over(err, bound, order):
    """The first group in execution order whose error exceeds its bound, or None."""
    for k in order:
        if not err[k] <= bound[k]:
            return k
    return None


def truth_of(g_fwd, g_grad):
    """{group: (float64 probes, float64 max)} from the two fixture files."""
    out = {}
    for g in (g_fwd, g_grad):
        for k in g:
            if k.startswith('probe_'):
                out[k[6:]] = (torch.from_numpy(g[k]), float(g['max_' + k[6:]]))
    return out

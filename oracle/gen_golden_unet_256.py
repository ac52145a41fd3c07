"""Generate tests/golden/g22_unet_ffhq_256.npz and g22_unet_ffhq_256_grad.npz: the score network at the width the
benchmark times (FFHQ_CONFIG: 93.6 M parameters, 128 to 512 channels, 256 x 256) against a float64 evaluation, as
probes.  Build container only (it imports the reference; never runs on the GPU box); about 4.5 minutes on 8 cores, most of
it in the float64 passes.

    python oracle/gen_golden_unet_256.py

What it imports.  The reference's `guided_diffusion.unet_ffhq.create_model`, called with the `model:` block of
configs/config_ffhq.yml (read from the reference tree, not restated), through oracle/gen_golden.py's
`import_reference`; from this repository `nhmc.unet` (its plain-torch CPU path), oracle.hmc_ref / ddim / schedule /
operators and oracle.unet_probe, which defines the groups, the probe positions and the metric.

What it computes.  Weights `randn * 0.05` under seed 606 over state_dict() in key order, then, from the same generator,
x [2, 3, 256, 256], the output gradient gout, the probe positions and the engine leg's inputs (oracle.unet_probe
.seeded_inputs: only the seed and the scale travel, the tests redraw everything).  t = [750, 250].
  * reference class, fp32, CPU: forward + input gradient with hooks on the 25 blocks -> the 52 groups;
  * nhmc.unet, fp32, CPU: the same;
  * nhmc.unet, float64 (`.double()` of the same module): the same -- the truth.  Its sinusoidal embedding is the fp32
    table cast up (nn.py:114-117 computes it in fp32 by definition), so the yardstick measures the network's
    arithmetic and not the rounding of t * freq.  The reference class is not used in float64: it casts to fp32 inside
    (nn.py:19, unet_ffhq.py:725);
  * engine leg: oracle.hmc_ref._data_loss_and_grad on the ladder [250, 500, 750] / [-1, 250, 500] with `inpaint_random`
    at 256 and B = 2, once with the float64 network and once with the fp32 reference class.

What it asserts.
  * nhmc.unet's fp32 CPU path equals the reference class BIT FOR BIT on every one of the 52 tensors (SHA-256 of the
    whole tensor, not of the probes).  Only this makes nhmc.unet in float64 an admissible truth, and it ties the
    fixture to the reference.
  * every fp32 error against the truth is non-zero and below 1e-4;
  * the clip masks of the engine leg's ladder (|x0| <= 1 at each step, the final clip) are the same in fp32 and in
    float64.  The gradient has a kink wherever a clip argument crosses +-1, and among the ladder's 1.2 M arguments,
    most of them of order one, some always lie close: the smallest distance is printed and stored (`eng_clip_margin`,
    9.6e-8 with these inputs), so the equality of the masks is asserted here and not assumed.

What it stores (arrays only).  Per group the float64 values at the 4096 positions, the float64 max |tensor| (the
metric's denominator) and `e32_<group>`: the fp32 reference class against the truth in that metric.  The same for the
engine leg's clipped decode and gradient, its float64 loss per chain and the fp32 class's relative loss error.
SHA-256 of x and of three weight tensors (first, a middle one, last) as reproducibility guards.  The gradient groups
go to a file of their own: 52 x 4096 float64 values do not fit one file under the repository's 1 MiB limit.
"""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import gen_golden as gg  # noqa: E402
from oracle import unet_probe as up  # noqa: E402


def reference_config():
    """The `model:` block of the reference's configs/config_ffhq.yml as create_model keywords (no checkpoint offline:
    the reference's own fallback is random initialisation, unet_ffhq.py:87-90)."""
    import yaml
    with open(os.path.join(gg.REF, 'configs', 'config_ffhq.yml')) as f:
        cfg = dict(yaml.safe_load(f)['model'])
    cfg['model_path'] = ''
    cfg['attention_resolutions'] = str(cfg['attention_resolutions'])
    return cfg


class Logged:
    """model(xt, t) that keeps each call's (xt, e): the clip arguments of the ladder are recomputed from them."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def __call__(self, xt, t):
        e = self.net(xt, t)
        self.calls.append((xt.detach(), e.detach()))
        return e


def clip_masks(calls, b):
    """([mask of |x0_t| <= 1 per step ..., mask of the final clip], smallest | |x0_t before its clip| - 1 |)."""
    from oracle import ddim, schedule
    masks, margin = [], float('inf')
    for (xt, e), i, j in zip(calls, reversed(up.SEQ), reversed(up.SEQ_NEXT)):
        n = xt.shape[0]
        at, at_next = schedule.alpha_bar(b, torch.full((n,), i).long()), schedule.alpha_bar(b, torch.full((n,), j).long())
        u = (xt - e[:, :3] * ddim.sqrt_rn(1 - at)) / ddim.sqrt_rn(at)
        masks.append(u.abs() <= 1)
        margin = min(margin, float((u.abs() - 1).abs().min()))
    # the ladder ends at alpha-bar = 1: the decode IS the last step's clipped x0, so the final clip has no argument of
    # its own to measure (its mask is kept all the same)
    masks.append(ddim.ddim_step(xt, e, at, at_next).abs() <= 1)
    return masks, margin


def main():
    from oracle import hmc_ref, operators, schedule
    t0 = time.time()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gg.import_reference()
    from guided_diffusion.unet_ffhq import create_model
    from nhmc import unet
    with contextlib.redirect_stdout(io.StringIO()):
        ref = create_model(**reference_config()).eval()      # trainable: its attention's checkpoint differentiates them
    mine = unet.create_model(**unet.FFHQ_CONFIG).eval().requires_grad_(False)
    inp = up.seeded_inputs(ref)
    assert up.seeded_inputs(mine)['weight_sha'] == inp['weight_sha']
    x, t, gout, pos = inp['x'], inp['t'], inp['gout'], inp['pos']

    ref32 = up.evaluate(ref, x, t, gout, pos, digest=True)
    print(f'reference fp32 done  {time.time() - t0:.0f} s', flush=True)
    mine32 = up.evaluate(mine, x, t, gout, pos, digest=True)
    for k in up.FWD + up.GRAD:
        assert mine32[k][2] == ref32[k][2] and mine32[k][1] == ref32[k][1] and torch.equal(mine32[k][0], ref32[k][0]), \
            f'nhmc.unet (fp32, CPU) is not the reference class bit for bit at {k}'
    print(f'nhmc.unet fp32 equals the reference class on all 52 tensors  {time.time() - t0:.0f} s', flush=True)

    # the engine leg in fp32 with the reference class, before the module goes to float64
    op = operators.InpaintRef(3, 256, inp['missing'])
    y = op.H(inp['eng_img']) + inp['eng_noise']
    b = schedule.betas_fp32()
    log32 = Logged(ref)
    xt32, _, loss32, grad32 = hmc_ref._data_loss_and_grad(inp['eng_x'].clone().requires_grad_(True), b, up.SEQ, up.SEQ_NEXT,
                                                         log32, op, y)
    masks32, _ = clip_masks(log32.calls, b)
    del log32
    print(f'engine leg fp32 done  {time.time() - t0:.0f} s', flush=True)

    f64 = mine.double()
    fp32_table = unet.sinusoid
    unet.sinusoid = lambda ts, dim, freqs=None: fp32_table(ts.float(), dim).double()     # the fp32 table, cast up
    try:
        truth = up.evaluate(f64, x.double(), t, gout.double(), pos)
        print(f'float64 done  {time.time() - t0:.0f} s', flush=True)
        log64 = Logged(f64)
        xt64, _, loss64, grad64 = hmc_ref._data_loss_and_grad(inp['eng_x'].double().requires_grad_(True), b, up.SEQ,
                                                             up.SEQ_NEXT, log64, op, y.double())
        masks64, margin = clip_masks(log64.calls, b)
    finally:
        unet.sinusoid = fp32_table
    print(f'engine leg float64 done  {time.time() - t0:.0f} s; smallest clip margin {margin:.3e}', flush=True)
    assert all(torch.equal(a, c) for a, c in zip(masks32, masks64)), 'a clip mask differs between fp32 and float64'

    e32 = up.errors(ref32, truth, up.FWD + up.GRAD)
    truth['eng_xt'], truth['eng_grad'] = up.probe(xt64, pos), up.probe(grad64, pos)
    e32.update(up.errors(dict(eng_xt=up.probe(xt32, pos), eng_grad=up.probe(grad32, pos)), truth, up.ENGINE))
    e32_loss = float(((loss32.double() - loss64).abs() / loss64.abs()).max())
    for k, v in e32.items():
        print(f'  e_cpu32 {k:8s} {v:.3e}   max |f64| {truth[k][1]:.4g}')
        assert 0 < v < 1e-4, k
    print(f'  e_cpu32 loss     {e32_loss:.3e}   loss {loss64.tolist()}')

    def arrays(groups):
        out = {}
        for k in groups:
            out['probe_' + k], out['max_' + k], out['e32_' + k] = truth[k][0].numpy(), np.array(truth[k][1]), np.array(e32[k])
        return out
    meta = dict(torch_version=np.array(torch.__version__), generator=np.array('oracle/gen_golden_unet_256.py'))
    first = dict(arrays(up.FWD + up.ENGINE), pos=pos.numpy().astype(np.int32), weight_seed=np.array(up.SEED),
                 weight_scale=np.array(up.SCALE), t=t.numpy(), x_sha256=np.array(up.sha(x)),
                 weight_sha256=np.array(inp['weight_sha']), eng_loss=loss64.numpy(), e32_eng_loss=np.array(e32_loss),
                 eng_clip_margin=np.array(margin))
    for name, arrs in (('g22_unet_ffhq_256.npz', first), ('g22_unet_ffhq_256_grad.npz', arrays(up.GRAD))):
        np.savez_compressed(os.path.join(gg.OUT, name), **arrs, **meta)
        size = os.path.getsize(os.path.join(gg.OUT, name))
        print(f'wrote {name}  ({size / 1024:.1f} KiB)')
        assert size <= 2 ** 20
    print(f'total {time.time() - t0:.0f} s')


if __name__ == '__main__':
    main()

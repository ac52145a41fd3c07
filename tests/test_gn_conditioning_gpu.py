"""GPU: the fused GroupNorm kernels (csrc/gn_act.hip, csrc/gn_onepass.hip) on slabs with a large common offset, nearly
flat and constant slabs, and offsets that enter through `pre` (oracle/gn_cases.py), forward and input gradient on every
route through nhmc.kernels.gn_act_fwd / gn_act_bwd, against the float64 definition and ATen's fp32 ops.

Everything is measured per (sample, group) slab, max |got - ref64| over the slab / max |ref64| over the slab:
  * forward: <= (2 r + 4) 2^-23 with r the slab's |mean| / std (gn_cases.bound); the constant slabs as
    gn_cases.check_forward says and, every element, within 1 ulp of the float64 value;
  * forward and input gradient: no further from float64 than 2 x ATen's fp32 ops on the same GPU tensors, + 1e-7 / 1e-6
    (the convention and the floors of tests/test_gn_act_gpu.py) -- the only criterion for the gradient;
  * control and straddle slabs: < 2e-6 forward, < 1e-5 backward as in tests/test_gn_act_gpu.py.
Each case prints its per-condition worst figures, kernel and ATen side by side (pytest -s)."""
import pytest
import torch

from oracle import gn_cases as gc

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.cuda()


def kernels(c, q, x, flags=0):
    """Forward and input gradient of case c on its route, for the input x (CPU, the problem's shape) -> (y, dx, ws)."""
    import nhmc.kernels as K
    p = q.p
    gamma, beta, film, pre, dy, add = (dev(t) for t in (q.gamma, q.beta, q.film, q.pre, q.dy, q.add))
    hw = p.shape[2] * p.shape[3]
    if c.route == 'two_source':
        x1, x2 = dev(x[:, :p.c1].contiguous()), dev(x[:, p.c1:].contiguous())
        y, ws, splits, x_cat = K.gn_act_fwd(x1, gamma, beta, gc.GROUPS, p.eps, p.act, film, pre, x2=x2, flags=flags)
        assert torch.equal(x_cat.cpu(), x)
        d1, d2 = K.gn_act_bwd(x_cat, dy, gamma, beta, gc.GROUPS, p.eps, p.act, film, ws, splits, pre, add=add, c1=p.c1, flags=flags)
        assert d1.is_contiguous() and d2.is_contiguous()
        return y, torch.cat([d1, d2], dim=1), ws
    one = True if c.route == 'one_pass' else None
    xd = dev(x)
    y, ws, splits = K.gn_act_fwd(xd, gamma, beta, gc.GROUPS, p.eps, p.act, film, pre, flags=flags, onepass=one)
    covered = K.gn_onepass_splits(q.B, q.C, gc.GROUPS, hw)
    assert splits == (covered if one else K._lib.load().nhmc_gn_splits(q.B, q.C, gc.GROUPS, hw))
    # the forward's workspace: partials only on the two-pass route, partials + slab totals on the one-pass route
    assert ws.numel() == q.B * gc.GROUPS * (splits + (1 if one else 0)) * 2
    dx = K.gn_act_bwd(xd, dy, gamma, beta, gc.GROUPS, p.eps, p.act, film, ws, splits, pre, add=add, flags=flags, onepass=one)
    return y, dx, ws


def aten(q):
    """ATen's fp32 ops and their autograd on the same GPU tensors -> (y, dx)."""
    p = q.p
    xa = dev(q.x).requires_grad_(True)
    ya = gc.aten_form(xa, dev(q.pre), dev(q.gamma), dev(q.beta), dev(q.film), gc.GROUPS, p.eps, p.act)
    (ga,) = torch.autograd.grad(ya, xa, dev(q.dy))
    return ya.detach(), ga if q.add is None else ga + dev(q.add)


def judge(q, label, y, dx, y_zero):
    """Print the table of the case, then hold every assertion of the module docstring."""
    ya, ga = aten(q)
    ey, ed = gc.slab_err(y, q.y64), gc.slab_err(dx, q.dx64)
    ay, ad = gc.slab_err(ya, q.y64), gc.slab_err(ga, q.dx64)
    print('\n' + label)
    print(gc.table(q, (('fwd kernel', ey), ('fwd ATen', ay), ('bwd kernel', ed), ('bwd ATen', ad))))
    has_r = ~gc.is_kind(q, 'constant')
    over = has_r & (ay > gc.bound(torch.where(has_r, q.r, torch.zeros_like(q.r))))
    for b, g in over.nonzero().tolist():
        print('ATen itself exceeds the forward bound:', q.conds[int(q.cond[b, g])].name, (b, g), float(ay[b, g]), float(gc.bound(q.r[b, g])))

    def slabs_of(mask, *cols):
        return '; '.join('%s (%d, %d) %s' % (q.conds[int(q.cond[b, g])].name, b, g, ' '.join('%.3e' % float(c[b, g]) for c in cols))
                         for b, g in mask.nonzero().tolist()[:12])
    gc.check_forward(q, y, label, y_zero=y_zero)
    if bool((~has_r).any()):
        # the kernels round the float64 value of the output once: 1 ulp on the constant slabs through FiLM and SiLU too
        ulps = int(gc.slabs(gc.ulp_distance(y, q.y64), q.B).amax(-1)[~has_r].max())
        assert ulps <= 1, (label, 'constant slabs', ulps, 'ulp')
    bad = ey > 2 * ay + gc.FLOOR_FWD
    assert not bool(bad.any()), label + ': forward further from float64 than 2 x ATen + 1e-7 (kernel, ATen): ' + slabs_of(bad, ey, ay)
    bad = ed > 2 * ad + gc.FLOOR_BWD
    assert not bool(bad.any()), label + ': gradient further from float64 than 2 x ATen + 1e-6 (kernel, ATen): ' + slabs_of(bad, ed, ad)
    today = gc.is_kind(q, 'control', 'straddle')
    assert float(ed[today].max()) < gc.TODAY_BWD, (label, 'control / straddle gradient', float(ed[today].max()))


@pytest.mark.parametrize('c', gc.CASES, ids=gc.case_id)
def test_conditioned_slabs_on_every_route(c, monkeypatch):
    """Measured on an MI355X (worst slab of a condition over all cases; kernel / ATen, forward and gradient alike within
    a factor two of these).  Forward: the kernels 3e-8 .. 9e-8 on every condition (the output is evaluated in fp64
    and rounded once; constant slabs 0 .. 1 ulp, with SiLU too); ATen control, straddle, offset 10 and pre 0 1e-7 ..
    6e-7, offset or pre 100 1e-6 .. 3e-5, offset or pre 1000 1e-5 .. 2.5e-4, flat 9e-5 .. 7e-4, constant 6e-5 .. 4e-4.
    Gradient: the kernels 3e-8 .. 4e-7 on every condition; ATen as in its forward.  With the statistics' squares rounded
    to fp32, as the kernels were before they were held to this test: offset 100 4e-5 .. 7e-4, offset 1000 1e-3 .. 8e-2,
    flat 4e-3 .. 1.7e-1, pre 1000 8e-4 .. 2.9e-1.  With exact statistics and an fp32 epilogue (gn_cases.exact_stats_fp32)
    two 8-element control slabs of one_pass-2x2-pre_sample-film_silu were 3 ulp off, 2.1e-7 and 3.6e-7, where ATen's
    roundings happened to cancel (4.3e-8, 9.1e-8): further than 2 x ATen + 1e-7."""
    import nhmc.kernels as K
    q = gc.problem(c.problem)
    hw = c.problem.shape[2] * c.problem.shape[3]
    if c.route == 'two_pass':
        monkeypatch.setenv('NHMC_GN_ONEPASS', '0')
    else:
        splits = K.gn_onepass_splits(q.B, q.C, gc.GROUPS, hw)
        assert splits > 1 if c.problem.shape == gc.SPLIT else splits == 1
    y, dx, ws = kernels(c, q, q.x)
    if c.problem.shape == gc.SPLIT:
        # every workgroup past its bounded wait: the same bits, statistics included
        for a, b in zip((y, dx, ws), kernels(c, q, q.x, flags=K.GN_ONEPASS_NOWAIT)):
            assert torch.equal(a, b)
    y_zero = kernels(c, q, torch.zeros_like(q.x))[0] if c.problem.kind == 'x' else None
    judge(q, gc.case_id(c), y, dx, y_zero)


def test_the_smallest_covered_shapes_are_the_smallest():
    """One float4 per channel plane is the least the kernels take; with two channels per group a slab can straddle."""
    import nhmc.kernels as K
    assert K.gn_onepass_splits(3, 64, gc.GROUPS, 4) == 1 and K.gn_onepass_splits(3, 128, gc.GROUPS, 4) == 1
    assert K.gn_onepass_splits(3, 64, gc.GROUPS, 2) == 0


def test_the_autograd_wiring_sees_the_same_numbers():
    """unet.group_norm_act on a conditioned input = gn_act_fwd / gn_act_bwd on their default route, bit for bit, and held
    to the same assertions."""
    import nhmc.kernels as K
    from nhmc import unet
    c = gc.CASES[0]
    q, p = gc.problem(c.problem), c.problem
    assert p.film and p.act and p.kind == 'x'
    gn = torch.nn.GroupNorm(gc.GROUPS, q.C, eps=p.eps).cuda().requires_grad_(False)
    gn.weight.copy_(dev(q.gamma))
    gn.bias.copy_(dev(q.beta))
    x = dev(q.x).requires_grad_(True)
    y = unet.group_norm_act(gn, x, act=p.act, film=dev(q.film))
    assert type(y.grad_fn).__name__.startswith('_GroupNormAct')
    (dx,) = torch.autograd.grad(y, x, dev(q.dy))
    y0, ws, splits = K.gn_act_fwd(dev(q.x), gn.weight, gn.bias, gc.GROUPS, p.eps, p.act, dev(q.film))
    d0 = K.gn_act_bwd(dev(q.x), dev(q.dy), gn.weight, gn.bias, gc.GROUPS, p.eps, p.act, dev(q.film), ws, splits)
    assert torch.equal(y.detach(), y0) and torch.equal(dx, d0)
    with torch.no_grad():
        y_zero = unet.group_norm_act(gn, torch.zeros_like(x), act=p.act, film=dev(q.film))
    judge(q, 'unet.group_norm_act ' + gc.case_id(c), y.detach(), dx, y_zero)

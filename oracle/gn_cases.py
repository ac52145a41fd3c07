"""Oracle: badly conditioned inputs for the fused GroupNorm kernels (test infrastructure, see oracle/__init__.py).
Shared by tests/test_gn_conditioning_cpu.py and tests/test_gn_conditioning_gpu.py.

The other GroupNorm tests draw x = 1.7 randn + 0.3: |mean| / std of a (sample, group) slab is about 0.2 there, and a
variance formed as E[v^2] - mean^2 loses nothing.  Here every slab of one tensor carries one planted condition -- a
large common offset of either sign, a nearly flat slab, a constant one, an offset that enters through `pre`, and two
controls -- and the conditions cycle over the groups with a different phase per sample, so that one launch covers all of
them and a slab's neighbours in the statistics workspace carry other conditions.

The float64 reference is the definition written out: v = x + pre, mean and the biased variance over the slab,
(v - mean) / sqrt(var + eps), gamma / beta, FiLM, SiLU, all in float64 on the fp32 inputs; the input gradient is
autograd's through that expression.

Errors are measured per slab, max |got - ref| over the slab divided by max |ref| over the same slab, never over the
tensor: a global maximum lets the control slabs hide the bad ones.  The forward bound per slab is (2 r + 4) 2^-23 with
r = |mean| / std of the slab: with exact statistics what remains is the rounding of `mean` to fp32 and, where `pre` is
given, of x + pre to fp32 -- each r 2^-24 in units of the slab's std -- plus the roundings of the epilogue.  A constant
slab has no r: there the normalised term must vanish and the output equal the float64 value of act(beta (1 + scale) +
shift) (check_forward says how that is held).

All problems are built once per process (cached), from seeds; the global torch RNG is left alone.
"""
import collections
import functools
import types

import torch

GROUPS = 32
# kind: control / straddle keep the tolerances of tests/test_gn_act_gpu.py on top of the bound
Cond = collections.namedtuple('Cond', 'name kind mean std')
# planted in x.  straddle: the channels of the group have means 0, 50, -50, 100, ... (std 1 each): the variance is
# genuinely large and nothing cancels -- a control that a change of the statistics' arithmetic must not disturb.
# seam (two-source problems only): the group that holds channels of both sources, +40 on one side, -40 on the other.
X_CONDS = (Cond('control', 'control', 0.3, 1.7), Cond('offset+10', 'offset', 10.0, 1.0), Cond('flat', 'flat', 3.0, 1e-4),
           Cond('offset-100', 'offset', -100.0, 1.0), Cond('constant', 'constant', 0.7, 0.0),
           Cond('offset+1000', 'offset', 1000.0, 1.0), Cond('straddle', 'straddle', None, 1.0),
           Cond('offset-10', 'offset', -10.0, 1.0), Cond('offset+100', 'offset', 100.0, 1.0),
           Cond('offset-1000', 'offset', -1000.0, 1.0))
SEAM = Cond('seam', 'straddle', None, 1.0)
# planted in `pre` (x ~ randn): the value of the group's channels, + 0.5 randn per channel
PRE_CONDS = (Cond('pre0', 'control', 0.0, 1.0), Cond('pre+100', 'pre', 100.0, 1.0), Cond('pre-1000', 'pre', -1000.0, 1.0),
             Cond('pre-100', 'pre', -100.0, 1.0), Cond('pre+1000', 'pre', 1000.0, 1.0))
STRADDLE_MEANS = (0.0, 50.0, -50.0, 100.0, -100.0, 150.0, -150.0, 200.0)
TODAY_FWD, TODAY_BWD = 2e-6, 1e-5         # tests/test_gn_act_gpu.py::test_fused_group_norm_matches_torch
FLOOR_FWD, FLOOR_BWD = 1e-7, 1e-6         # its floors under "no further from float64 than 2 x ATen"

# Problem: what is planted where.  kind: 'x' | 'pre_sample' ([B, C]) | 'pre_shared' ([C]); c1: channels of the first
# source of a two-source problem (inside a group), or None
Problem = collections.namedtuple('Problem', 'shape kind film act add eps c1')


def bound(r):
    """The forward bound of a slab with |mean| / std = r."""
    return (2.0 * r + 4.0) * 2.0 ** -23


def cond_index(b, g, n):
    """Which condition slab (b, g) carries: the cycle over the groups, its phase moved by 3 per sample."""
    return (g + 3 * b) % n


def _plant(n, mean, std, g):
    """n float64 values with exactly this mean and (population) std."""
    z = torch.randn(n, dtype=torch.float64, generator=g)
    z = z - z.mean()
    return mean + std * z / z.pow(2).mean().sqrt()


def _slab(cond, cpg, hw, lo, c1, g):
    """One slab [cpg, hw] in float64.  lo: its first channel."""
    if cond.kind == 'control':
        return cond.std * torch.randn(cpg, hw, dtype=torch.float64, generator=g) + cond.mean
    if cond.kind == 'constant':
        return torch.full((cpg, hw), cond.mean, dtype=torch.float64)
    if cond is SEAM:
        side = torch.tensor([40.0 if lo + k < c1 else -40.0 for k in range(cpg)], dtype=torch.float64)
        return torch.randn(cpg, hw, dtype=torch.float64, generator=g) + side[:, None]
    if cond.kind == 'straddle':
        means = torch.tensor([STRADDLE_MEANS[k % len(STRADDLE_MEANS)] for k in range(cpg)], dtype=torch.float64)
        return torch.randn(cpg, hw, dtype=torch.float64, generator=g) + means[:, None]
    return _plant(cpg * hw, cond.mean, cond.std, g).reshape(cpg, hw)


def slabs(t, B):
    """[B, C, ...] -> [B, GROUPS, elements of a slab]."""
    return t.reshape(B, GROUPS, -1)


def slab_err(got, ref):
    """-> [B, GROUPS] float64 (on the CPU): max |got - ref| over the slab / max |ref| over the slab."""
    B = ref.shape[0]
    d = slabs((got.detach().double() - ref.to(got.device)).abs(), B).amax(-1)
    return (d / slabs(ref.abs(), B).amax(-1).to(d.device).clamp_min(1e-300)).cpu()


def ulp_distance(got, ref):
    """Units in the last place of fp32 between `got` (fp32) and `ref` (float64) rounded to fp32, per element."""
    def ordered(t):
        i = t.detach().cpu().float().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (ordered(got) - ordered(ref.float())).abs()


def reference(x, pre, gamma, beta, film, groups, eps, act):
    """The definition, in the dtype of x (float64 for the reference) -> y."""
    B, C = x.shape[:2]
    v = x if pre is None else x + pre.reshape((1, C) if pre.dim() == 1 else (B, C))[:, :, None, None]
    s = v.reshape(B, groups, -1)
    mean = s.mean(-1, keepdim=True)
    var = (s - mean).pow(2).mean(-1, keepdim=True)
    u = ((s - mean) / (var + eps).sqrt()).reshape(v.shape) * gamma[None, :, None, None] + beta[None, :, None, None]
    if film is not None:
        u = u * (1 + film[:, :C, None, None]) + film[:, C:, None, None]
    return u * torch.sigmoid(u) if act else u


def aten_form(x, pre, gamma, beta, film, groups, eps, act):
    """ATen's own ops in the dtype and on the device of x: F.group_norm, then FiLM, then SiLU."""
    import torch.nn.functional as F
    B, C = x.shape[:2]
    v = x if pre is None else x + pre.reshape((1, C) if pre.dim() == 1 else (B, C))[:, :, None, None]
    h = F.group_norm(v, groups, gamma, beta, eps)
    if film is not None:
        sc, sh = film[:, :, None, None].chunk(2, dim=1)
        h = h * (1 + sc) + sh
    return F.silu(h) if act else h


@functools.lru_cache(maxsize=None)
def problem(p):
    """-> namespace: x (x1, x2 of a two-source problem too), pre, gamma, beta, film, dy, add (fp32, CPU; None where the
    problem has none), conds (the condition list), cond [B, G] (index into it), r [B, G] (|mean| / std of the slab as
    planted, inf on constant slabs), y64, dx64 (the float64 reference; dx64 includes `add`)."""
    B, C, H, W = p.shape
    G, cpg, hw = GROUPS, C // GROUPS, H * W
    g = torch.Generator().manual_seed(9000 + 7 * C + hw + 1000 * ('x', 'pre_sample', 'pre_shared').index(p.kind))
    q = types.SimpleNamespace(p=p, B=B, C=C, G=G, hw=hw)
    q.gamma, q.beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    q.film = 0.3 * torch.randn(B, 2 * C, generator=g) if p.film else None
    q.dy = torch.randn(p.shape, generator=g)
    q.add = torch.randn(p.shape, generator=g) if p.add else None
    base = X_CONDS if p.kind == 'x' else PRE_CONDS
    q.conds = base + ((SEAM,) if p.c1 is not None else ())
    q.cond = torch.empty(B, G, dtype=torch.long)
    x = torch.empty(B, G, cpg, hw, dtype=torch.float64)
    pre = torch.zeros(1 if p.kind == 'pre_shared' else B, G, cpg, dtype=torch.float64)
    for b in range(B):
        for gi in range(G):
            k = cond_index(0 if p.kind == 'pre_shared' else b, gi, len(base))
            if p.c1 is not None and gi * cpg < p.c1 < (gi + 1) * cpg:
                k = len(base)
            q.cond[b, gi] = k
            if p.kind == 'x':
                x[b, gi] = _slab(q.conds[k], cpg, hw, gi * cpg, p.c1, g)
            else:
                x[b, gi] = torch.randn(cpg, hw, dtype=torch.float64, generator=g)
                if b < pre.shape[0]:
                    pre[b, gi] = q.conds[k].mean + 0.5 * torch.randn(cpg, dtype=torch.float64, generator=g)
    q.x = x.float().reshape(p.shape).contiguous()
    q.pre = None if p.kind == 'x' else pre.float().reshape((C,) if p.kind == 'pre_shared' else (B, C)).contiguous()
    if p.c1 is not None:
        assert any(gi * cpg < p.c1 < (gi + 1) * cpg for gi in range(G)), 'c1 must fall inside a group'
        q.x1, q.x2 = q.x[:, :p.c1].contiguous(), q.x[:, p.c1:].contiguous()
    d = lambda t: None if t is None else t.double()                             # noqa: E731
    xd = q.x.double().requires_grad_(True)
    y = reference(xd, d(q.pre), d(q.gamma), d(q.beta), d(q.film), G, p.eps, p.act)
    (dx,) = torch.autograd.grad(y, xd, q.dy.double())
    q.y64, q.dx64 = y.detach(), dx if q.add is None else dx + q.add.double()
    v = xd.detach() if q.pre is None else xd.detach() + d(q.pre).reshape((1, C) if q.pre.dim() == 1 else (B, C))[:, :, None, None]
    s = slabs(v, B)
    std = (s - s.mean(-1, keepdim=True)).pow(2).mean(-1).sqrt()
    q.r = torch.where(std > 0, s.mean(-1).abs() / std.clamp_min(1e-300), torch.full_like(std, float('inf')))
    return q


def is_kind(q, *kinds):
    """[B, G] bool: the slabs whose condition is of one of these kinds."""
    m = torch.zeros_like(q.cond, dtype=torch.bool)
    for k, c in enumerate(q.conds):
        if c.kind in kinds:
            m |= q.cond == k
    return m


def worst(q, err):
    """{condition name: max of err [B, G] over the slabs of that condition}, in the order of the condition list."""
    return {c.name: float(err[q.cond == k].max()) for k, c in enumerate(q.conds) if bool((q.cond == k).any())}


def table(q, columns):
    """One line per condition: the bound, then the worst figure of each of `columns` = ((title, err [B, G]), ...)."""
    lines = ['%-12s %10s ' % ('condition', 'bound') + ' '.join('%10s' % t for t, _ in columns)]
    per = [worst(q, e) for _, e in columns]
    finite = torch.where(torch.isfinite(q.r), q.r, torch.zeros_like(q.r))
    for k, c in enumerate(q.conds):
        if not bool((q.cond == k).any()):
            continue
        b = '1 ulp' if c.kind == 'constant' else '%.2e' % bound(float(finite[q.cond == k].max()))
        lines.append('%-12s %10s ' % (c.name, b) + ' '.join('%10.2e' % w[c.name] for w in per))
    return '\n'.join(lines)


def exact_stats_fp32(q, x=None):
    """What the bound is derived from, on the CPU: the slab's mean and 1 / sqrt(var + eps) from float64 sums, rounded to
    fp32, then the kernels' epilogue in fp32 -- v = x + pre, ((v - mean) rstd) ga + be with ga = gamma (1 + scale),
    be = beta (1 + scale) + shift, u sigmoid(u).  x: another input in place of the problem's own (fp32, its shape)."""
    p, B, C = q.p, q.B, q.C
    x = q.x if x is None else x
    v = x if q.pre is None else x + q.pre.reshape((1, C) if q.pre.dim() == 1 else (B, C))[:, :, None, None]
    vd = x.double() if q.pre is None else x.double() + q.pre.double().reshape((1, C) if q.pre.dim() == 1 else (B, C))[:, :, None, None]
    s = slabs(vd, B)
    mean = s.mean(-1, keepdim=True)
    rstd = 1 / ((s - mean).pow(2).mean(-1, keepdim=True) + p.eps).sqrt()
    xh = ((slabs(v, B) - mean.float()) * rstd.float()).reshape(x.shape)
    ga, be = q.gamma[None, :, None, None].expand(B, C, 1, 1), q.beta[None, :, None, None].expand(B, C, 1, 1)
    if q.film is not None:
        sc = 1 + q.film[:, :C, None, None]
        ga, be = ga * sc, be * sc + q.film[:, C:, None, None]
    u = xh * ga + be
    return u * (1 / (1 + torch.exp(-u))) if p.act else u


def check_forward(q, y, label='', y_zero=None, constant=True):
    """The forward assertions that need no second implementation -> err [B, G]:
    the bound on every slab that has an r; today's tolerance on the control and straddle slabs; on the constant slabs
    (skipped with constant=False) that the normalised term vanishes and the float64 value of act(beta (1 + scale) +
    shift) is met.  The latter, in full: with y_zero, the same implementation's output for an all-zero x, the constant
    slabs of y must equal those of y_zero bit for bit (x - mean is exactly 0 in both, whatever rstd is); the slab's
    error must stay within bound(0), the epilogue's share of the bound; and it is at most 1 ulp per element where no
    SiLU follows.  (Through FiLM and SiLU an epilogue in fp32 is not within 1 ulp of the float64 value on every
    element: with exact statistics, exact_stats_fp32 is up to 6 ulp off where beta (1 + scale) and shift cancel,
    1.2 2^-23 of the slab's maximum.  The HIP kernels evaluate the output in fp64 and are held to 1 ulp there too,
    by tests/test_gn_conditioning_gpu.py.)"""
    err = slab_err(y, q.y64)
    const = is_kind(q, 'constant')
    lim = bound(torch.where(const, torch.zeros_like(q.r), q.r))
    bad = (~const) & (err > lim)
    assert not bool(bad.any()), label + ': forward bound (error, bound): ' + '; '.join(
        '%s (%d, %d) %.3e %.3e' % (q.conds[int(q.cond[b, g])].name, b, g, float(err[b, g]), float(lim[b, g]))
        for b, g in bad.nonzero().tolist()[:16])
    if constant and bool(const.any()):
        worst_ulps = int(slabs(ulp_distance(y, q.y64), q.B).amax(-1)[const].max())
        print(label, 'constant slabs: worst', worst_ulps, 'ulp,', float(err[const].max()), 'of the slab maximum')
        if y_zero is not None:
            assert torch.equal(slabs(y.detach().cpu(), q.B)[const], slabs(y_zero.detach().cpu(), q.B)[const]), \
                (label, 'the normalised term of a constant slab does not vanish')
        assert float(err[const].max()) <= bound(0.0), (label, 'constant slabs', float(err[const].max()))
        assert q.p.act or worst_ulps <= 1, (label, 'constant slabs', worst_ulps, 'ulp')
    today = is_kind(q, 'control', 'straddle')
    assert float(err[today].max()) < TODAY_FWD, (label, 'control / straddle forward', float(err[today].max()))
    return err


# ---- the case list ----------------------------------------------------------------------------------------------------
# route: two_pass (NHMC_GN_ONEPASS=0) | one_pass (onepass=True; shapes of more than one split also run with the
# bounded wait expired everywhere, and must give the same bits) | two_source (x2= forward, c1= backward)
Case = collections.namedtuple('Case', 'route problem')


def _case(route, shape, kind, film, act, add, eps, c1=None):
    return Case(route, Problem(shape, kind, film, act, add, eps, c1))


SMALL = (3, 64, 2, 2)            # the smallest shape with two channels per group: 8 elements per slab, one split
SPLIT = (3, 128, 64, 64)         # two splits per slab
PAIR = (3, 128, 2, 2)            # two sources of 66 + 62 channels: group 16 holds two channels of each
CASES = (
    _case('two_pass', (3, 64, 16, 16), 'x', True, True, False, 1e-5),
    _case('two_pass', (3, 128, 8, 8), 'x', False, False, True, 1e-6),
    _case('two_pass', (3, 128, 8, 8), 'x', True, True, False, 1e-6),
    _case('two_pass', (3, 64, 16, 16), 'pre_sample', False, True, False, 1e-6),
    _case('two_pass', (3, 128, 8, 8), 'pre_shared', True, False, True, 1e-5),
    _case('one_pass', SPLIT, 'x', True, True, True, 1e-6),
    _case('one_pass', SPLIT, 'pre_sample', False, False, False, 1e-5),
    _case('one_pass', SPLIT, 'pre_shared', True, True, False, 1e-5),
    _case('one_pass', SMALL, 'x', True, True, False, 1e-6),
    _case('one_pass', SMALL, 'x', False, False, True, 1e-5),
    _case('one_pass', SMALL, 'pre_sample', True, True, False, 1e-5),
    _case('one_pass', (3, 64, 16, 16), 'x', False, True, False, 1e-6),
    _case('one_pass', (3, 128, 8, 8), 'pre_shared', True, False, True, 1e-5),
    _case('two_source', PAIR, 'x', False, True, True, 1e-5, 66),
    _case('two_source', PAIR, 'x', True, False, False, 1e-6, 66),
)


def case_id(c):
    p = c.problem
    return '%s-%s-%s-%s%s%s-eps%g' % (c.route, 'x'.join(str(s) for s in p.shape[1:]), p.kind, 'film' if p.film else 'plain',
                                      '_silu' if p.act else '', '_add' if p.add else '', p.eps)

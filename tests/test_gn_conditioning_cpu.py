"""CPU: the badly conditioned GroupNorm inputs of oracle/gn_cases.py are sound before any kernel sees them: every
condition is planted where the recipe says, the float64 reference agrees with ATen's float64 group norm, and plain fp32
arithmetic (F.group_norm on the CPU, then FiLM and SiLU) meets the forward bound of tests/test_gn_conditioning_gpu.py on
every slab of every case.  A case that fp32 ATen cannot meet would be a wrong case, not a reason for a wider bound."""
import pytest
import torch

from oracle import gn_cases as gc

PROBLEMS = sorted(set(c.problem for c in gc.CASES), key=str)


def test_the_bound_is_the_stated_one():
    assert gc.bound(0.0) == 4 * 2.0 ** -23 and gc.bound(1000.0) == 2004 * 2.0 ** -23
    assert (gc.TODAY_FWD, gc.TODAY_BWD, gc.FLOOR_FWD, gc.FLOOR_BWD) == (2e-6, 1e-5, 1e-7, 1e-6)


def test_the_case_list_covers_what_it_claims():
    routes = {c.route for c in gc.CASES}
    assert routes == {'two_pass', 'one_pass', 'two_source'}
    for family in (('two_pass',), ('one_pass', 'two_source')):
        ps = [c.problem for c in gc.CASES if c.route in family]
        for field in ('film', 'act', 'add'):
            assert {getattr(p, field) for p in ps} == {False, True}, (family, field)
        assert {p.eps for p in ps} == {1e-5, 1e-6}
        assert {p.kind for p in ps} >= ({'x', 'pre_sample', 'pre_shared'} if family[0] == 'two_pass' else {'x'})
    assert {c.problem.kind for c in gc.CASES if c.route == 'one_pass'} == {'x', 'pre_sample', 'pre_shared'}
    assert {c.problem.shape for c in gc.CASES if c.route == 'two_pass'} == {(3, 64, 16, 16), (3, 128, 8, 8)}
    assert all(p.shape[0] >= 3 for p in PROBLEMS)
    assert len({gc.case_id(c) for c in gc.CASES}) == len(gc.CASES)


@pytest.mark.parametrize('p', PROBLEMS, ids=str)
def test_every_condition_is_planted_where_the_recipe_says(p):
    q = gc.problem(p)
    B, G = q.B, q.G
    for b in range(B):                                   # every condition in every sample (shared pre: in every tensor)
        assert set(q.cond[b].tolist()) >= set(range(len(gc.X_CONDS if p.kind == 'x' else gc.PRE_CONDS)))
    flat = q.cond.reshape(-1)
    assert bool((flat[1:] != flat[:-1]).all())           # neighbours in the workspace carry different conditions
    if p.kind != 'pre_shared':
        own = q.cond[0] < len(q.conds) - (p.c1 is not None)                     # the seam group is the same in every sample
        assert bool((q.cond[0] != q.cond[1])[own].all()) and bool((q.cond[1] != q.cond[2])[own].all())
    v = q.x.double() if q.pre is None else q.x.double() + q.pre.double().reshape((1, q.C) if q.pre.dim() == 1 else (B, q.C))[:, :, None, None]
    s = gc.slabs(v, B)
    for k, c in enumerate(q.conds):
        m = q.cond == k
        mean, std = s.mean(-1)[m], s.std(-1, unbiased=False)[m]
        if c.kind in ('offset', 'flat'):                 # planted exactly, up to the rounding of x to fp32
            assert float((mean - c.mean).abs().max()) <= abs(c.mean) * 2.0 ** -23
            assert float((std / c.std - 1).abs().max()) < 2e-3
            assert float((q.r[m] * c.std / abs(c.mean) - 1).abs().max()) < 2e-3
        elif c.kind == 'constant':
            assert bool((s[m] == float(torch.tensor(c.mean).float())).all()) and bool(torch.isinf(q.r[m]).all())
            assert c.mean != 2.0 ** round(torch.tensor(c.mean).log2().item())
        elif c.kind == 'pre' and s.shape[-1] >= 64:      # x ~ randn, the offset from `pre` (+ 0.5 randn per channel)
            assert float((mean - c.mean).abs().max()) < 2.0 and 0.7 < float(std.min()) and float(std.max()) < 2.5
        elif c.kind == 'straddle':                       # a genuinely large variance: nothing to cancel
            assert float(q.r[m].max()) < 1.5 and float(std.min()) > 15
    if p.c1 is not None:                                 # the seam group draws from both sources, which differ in mean
        cpg = q.C // G
        gi = p.c1 // cpg
        assert gi * cpg < p.c1 < (gi + 1) * cpg and bool((q.cond[:, gi] == len(q.conds) - 1).all())
        assert float(q.x1[:, gi * cpg:].mean()) > 35 and float(q.x2[:, :(gi + 1) * cpg - p.c1].mean()) < -35
        assert torch.equal(torch.cat([q.x1, q.x2], dim=1), q.x)


@pytest.mark.parametrize('p', PROBLEMS, ids=str)
def test_the_reference_is_atens_float64_group_norm(p):
    """The definition written out = F.group_norm + FiLM + SiLU evaluated in float64, value and input gradient, on
    every slab (ATen's float64 moments are Welford's: they do not cancel either)."""
    q = gc.problem(p)
    d = lambda t: None if t is None else t.double()      # noqa: E731
    xd = q.x.double().requires_grad_(True)
    y = gc.aten_form(xd, d(q.pre), d(q.gamma), d(q.beta), d(q.film), gc.GROUPS, p.eps, p.act)
    (dx,) = torch.autograd.grad(y, xd, q.dy.double())
    dx = dx if q.add is None else dx + q.add.double()
    ey, ed = gc.slab_err(y, q.y64), gc.slab_err(dx, q.dx64)
    # float64 carries r 2^-53 where fp32 carries r 2^-24: five digits below the bound is the least to expect
    lim = gc.bound(torch.where(torch.isinf(q.r), torch.zeros_like(q.r), q.r)) * 1e-5
    assert bool((ey <= lim).all()), float((ey / lim).max())
    assert bool((ed <= 1e-9).all()), float(ed.max())


@pytest.mark.parametrize('p', PROBLEMS, ids=str)
def test_fp32_aten_on_the_cpu_meets_the_forward_bound_on_every_slab(p):
    """Every slab that has an r.  The constant slabs are left to the next test: ATen folds the normalisation into
    x a + (beta - mean a) with a = gamma rstd, and on a constant slab rounds beta - 0.7 gamma / sqrt(eps), a number of
    several hundred: 2000 to 110000 ulp of beta off, with every constant value but 0."""
    q = gc.problem(p)
    y = gc.aten_form(q.x, q.pre, q.gamma, q.beta, q.film, gc.GROUPS, p.eps, p.act)
    err = gc.slab_err(y, q.y64)
    print(gc.table(q, (('ATen fp32', err),)))
    gc.check_forward(q, y, 'ATen fp32 on the CPU', constant=False)
    assert bool((~gc.is_kind(q, 'constant')).any())


@pytest.mark.parametrize('p', PROBLEMS, ids=str)
def test_exact_statistics_and_an_fp32_epilogue_meet_every_forward_assertion(p):
    """What the bound is derived from (float64 statistics rounded to fp32, the kernels' epilogue in fp32) meets it on
    every slab, the constant ones included."""
    q = gc.problem(p)
    y = gc.exact_stats_fp32(q)
    err = gc.check_forward(q, y, 'exact statistics, fp32 epilogue', y_zero=gc.exact_stats_fp32(q, torch.zeros_like(q.x)))
    print(gc.table(q, (('exact', err),)))

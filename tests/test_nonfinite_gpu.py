"""GPU: NaN and +-inf through the sampler's kernels.

The sampler's treatment of a diverged chain rests on non-finite values behaving as they do in the reference's torch ops
("Non-finite values"): a NaN decode must give a NaN loss, a NaN Hamiltonian and a rejection -- it must not be
clamped into a finite pixel on the way -- and whatever happens to one chain must leave the bits of the others alone.

Every kernel call here runs on B = 3 chains, chain 1 poisoned and chains 0 and 2 clean, with two assertions:

  (a) isolation: everything the call writes for chains 0 and 2 is `torch.equal` to the same call with chain 1 clean;
  (b) semantics of the poisoned call against the reference ops in fp32 on the CPU (the oracles of the finite tests):
      Tier 2 (elementwise kernels): equal NaN masks, equal +-inf entries, and the finite entries to the criterion of the
              kernel's finite test -- `torch.equal` where that is bit-exact -- including the zeros torch's clamp
              backward selects at masked elements;
      Tier 1 (kernels that mix pixels): non-finite wherever the reference is non-finite; a per-chain loss is NaN where
              the reference's is NaN and +-inf with the reference's sign.

Poison: the chain's first element, its last element and one element inside its middle channel -- three float4s, tiles
and channel planes -- as NaN, +inf, -inf, or all three together.  No huge finite values, so whether a sum comes out
non-finite does not depend on the order of summation.  3 x 20 x 20 (1200 elements, not a multiple of the tile) wherever
the kernel takes it, 32 x 32 where an operator needs a power of two or whole mask words.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ddim, hmc_ref, operators as oops, schedule as osched
from tests.test_nonfinite_cpu import DivergingScore, NoGradDivergingScore

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
KINDS = ['nan', 'pinf', 'ninf', 'mixed']
VALUES = dict(nan=[NAN, NAN, NAN], pinf=[INF, INF, INF], ninf=[-INF, -INF, -INF], mixed=[NAN, INF, -INF])
B = 3
SHAPE = (B, 3, 20, 20)
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
EPS = [0.05, 0.04, 0.03]
SIG = [1.7, 0.9, 0.1]
DEV = 'cuda'
K = None


@pytest.fixture(scope='module', autouse=True)
def _kernels():
    global K
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    import nhmc.kernels as kernels
    K = kernels
    yield


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return None if t is None else t.to(DEV).contiguous().clone()


def f64(v):
    return torch.tensor(v, dtype=torch.float64, device=DEV)


# ---- the poison -----------------------------------------------------------------------------------
def spots(shape, channels=None):
    """Flat indices, inside one chain, of the three poisoned elements (of its first `channels` channels)."""
    C = channels or shape[1]
    per = int(np.prod(shape[2:]))
    return [0, C * per - 1, (C // 2) * per + per // 2 + 1]


def poisoned(t, kind, channels=None):
    """A copy of t [B, C, ...] with chain 1 poisoned.  channels < C (a score output with learned-sigma channels, which
    the kernels do not read): the three spots lie in the channels that are read, and the very last element of the unread
    half is poisoned as well -- it must change nothing."""
    out = t.clone()
    flat = out[1].reshape(-1)
    assert flat.data_ptr() == out[1].data_ptr()
    for i, v in zip(spots(t.shape, channels), VALUES[kind]):
        flat[i] = v
    if channels and channels < t.shape[1]:
        flat[-1] = VALUES[kind][0]
    return out


# ---- the comparisons --------------------------------------------------------------------------------
def rows(t):
    return t.detach().reshape(B, -1)[[0, 2]]


def assert_isolated(clean, dirty, what):
    """(a): chains 0 and 2 of every output, bit for bit."""
    assert clean.keys() == dirty.keys()
    for k in clean:
        if clean[k] is None:
            assert dirty[k] is None
            continue
        a, b = rows(clean[k]).cpu(), rows(dirty[k]).cpu()
        assert bool(torch.isfinite(a.double()).all()), (what, k, 'the clean run is not finite')
        assert torch.equal(a, b), f'{what}: {k} of a clean chain changed with its neighbour ({int((a != b).sum())} elements)'


def assert_same_class(got, ref, what, tol=0.0, entrywise=False):
    """Tier 2.  tol = 0: the finite entries are `torch.equal`; otherwise relative to the largest finite reference entry
    (entrywise: to each entry, for per-chain scalars)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f'{what}: NaN masks differ: kernel {int(gn.sum())}, reference {int(rn.sum())}, ' \
                                f'{int((gn != rn).sum())} places; first at {int(torch.nonzero((gn != rn).reshape(-1))[0])}'
    for s in (INF, -INF):
        assert torch.equal(got == s, ref == s), f'{what}: {s} entries differ: kernel {int((got == s).sum())}, ' \
                                                f'reference {int((ref == s).sum())}'
    fin = torch.isfinite(ref)
    if not bool(fin.any()):
        return
    g, r = got[fin].double(), ref[fin].double()
    if tol == 0.0:
        assert torch.equal(got[fin], ref[fin]), f'{what}: {int((g != r).sum())} finite entries differ, worst {float((g - r).abs().max()):.3e}'
    elif entrywise:
        assert bool(((g - r).abs() <= tol * r.abs()).all()), (what, g.tolist(), r.tolist())
    else:
        err = float((g - r).abs().max() / r.abs().max().clamp_min(1e-30))
        assert err <= tol, (what, err)


def assert_not_laundered(got, ref, what):
    """Tier 1: wherever the reference is non-finite, so is the kernel."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~torch.isfinite(ref)
    assert not bool(torch.isfinite(got[bad]).any()), \
        f'{what}: {int(torch.isfinite(got[bad]).sum())} of {int(bad.sum())} non-finite reference values came out finite'


def assert_scalar_class(got, ref, what):
    """Tier 1 for a per-chain loss / H: NaN where the reference's is NaN, +-inf with its sign where it is +-inf."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for c in range(ref.numel()):
        r, g = float(ref.reshape(-1)[c]), float(got.reshape(-1)[c])
        if math.isnan(r):
            assert math.isnan(g), f'{what}[{c}]: reference NaN, kernel {g}'
        elif math.isinf(r):
            assert g == r, f'{what}[{c}]: reference {r}, kernel {g}'


def check(call, operands, name, kind, ref, compare, channels=None):
    """One kernel call, one poisoned operand: (a), then (b) through compare(got, want)."""
    clean = call(operands)
    dirty_in = dict(operands)
    dirty_in[name] = poisoned(operands[name], kind, channels)
    dirty = call(dirty_in)
    torch.cuda.synchronize()
    assert_isolated(clean, dirty, f'{name}/{kind}')
    want = ref(dirty_in)
    compare(dirty, want, f'{name}/{kind}')
    return dirty, want


def tier2(loss_tol=1e-6, tol=0.0):
    """compare(): every key Tier 2; the per-chain sums entrywise to loss_tol; the rest to `tol` (0: bit-exact)."""
    def compare(got, want, what):
        for k, r in want.items():
            if r is None:
                continue
            if k in ('loss', 'Sx', 'Sp'):
                assert_same_class(got[k], r, f'{what}: {k}', tol=loss_tol, entrywise=True)
            else:
                assert_same_class(got[k], r, f'{what}: {k}', tol=tol)
    return compare


def tier1(got, want, what):
    for k, r in want.items():
        if k == 'loss':
            assert_scalar_class(got[k], r, f'{what}: loss')
        else:
            assert_not_laundered(got[k], r, f'{what}: {k}')


def step_alphas():
    """three different DDIM steps, one per chain (c4 = 0 for chain 2: the last step)"""
    b = osched.betas_fp32()
    return osched.alpha_bar(b, torch.tensor([750, 500, 250])), osched.alpha_bar(b, torch.tensor([500, 250, -1]))


def last_step_alphas():
    b = osched.betas_fp32()
    return osched.alpha_bar(b, torch.full((B,), 250)), osched.alpha_bar(b, torch.full((B,), -1))


def leaf(t):
    return t.detach().clone().requires_grad_(True)


# =====================================================================================================
# Tier 2: the DDIM mix
# =====================================================================================================
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('final_clip', [False, True], ids=['noclip', 'finalclip'])
@pytest.mark.parametrize('ech', [3, 6])
@pytest.mark.parametrize('name', ['xt', 'e'])
def test_ddim_mix_fwd(name, ech, final_clip, kind):
    g_ = gen(1)
    ops = dict(xt=torch.randn(SHAPE, generator=g_), e=torch.randn((B, ech) + SHAPE[2:], generator=g_))
    at, atn = step_alphas()

    def call(o):
        return K.ddim_mix_fwd(dev(o['xt']), dev(o['e']), at, atn, final_clip=final_clip, want=('xt_next', 'x0_t', 'add_up'))

    def ref(o):
        x0, add = ddim.predict_x0(o['xt'], o['e'], at, atn)
        nxt = ddim.renoise(x0, add, atn)
        return dict(xt_next=nxt.clip(-1, 1) if final_clip else nxt, x0_t=x0, add_up=add)
    check(call, ops, name, kind, ref, tier2(), channels=3 if name == 'e' else None)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['x0_t', 'add_up'])
def test_ddim_map_back(name, kind):
    g_ = gen(2)
    ops = dict(x0_t=torch.randn(SHAPE, generator=g_).clip(-1, 1), add_up=torch.randn(SHAPE, generator=g_))
    _, atn = step_alphas()
    check(lambda o: dict(out=K.ddim_map_back(dev(o['x0_t']), dev(o['add_up']), atn)), ops, name, kind,
          lambda o: dict(out=ddim.renoise(o['x0_t'], o['add_up'], atn)), tier2())


def mix_operands(seed, ech=6):
    """xt, e with the first spot of chain 1 outside the x0 clip (u >> 1: its gradient is one of the zeros torch's clamp
    backward selects) and the second inside both clips (u = pre = 0)."""
    g_ = gen(seed)
    xt, e = torch.randn(SHAPE, generator=g_), torch.randn((B, ech) + SHAPE[2:], generator=g_)
    s = spots(SHAPE)
    xt[1].reshape(-1)[s[0]], e[1, :3].reshape(-1)[s[0]] = 30.0, 0.0
    xt[1].reshape(-1)[s[1]], e[1, :3].reshape(-1)[s[1]] = 0.0, 0.0
    return xt, e


MIX_BWD = [(v, n) for v in ('plain', 'finalclip', 'two_gradients', 'split', 'no_g_e')
           for n in ('gout', 'xt', 'e') + (('gout2',) if v == 'two_gradients' else ()) + (('g_x0',) if v == 'split' else ())]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('variant,name', MIX_BWD, ids=[f'{v}-{n}' for v, n in MIX_BWD])
def test_ddim_mix_bwd(variant, name, kind):
    """Against autograd through the oracle's DDIM step.  A masked element's gradient is ZERO in autograd whatever arrives
    there (clamp backward selects): gout = inf at chain 1's first spot, which lies outside the x0 clip, shows it."""
    xt, e = mix_operands(3)
    g_ = gen(30)
    ops = dict(xt=xt, e=e, gout=torch.randn(SHAPE, generator=g_), gout2=torch.randn(SHAPE, generator=g_),
               g_x0=torch.randn(SHAPE, generator=g_))
    at, atn = step_alphas()
    fc = variant in ('finalclip', 'two_gradients', 'no_g_e')

    def call(o):
        gx, ge = K.ddim_mix_bwd(dev(o['gout']), dev(o['xt']), dev(o['e']), at, atn, final_clip=fc,
                                gout2=dev(o['gout2']) if variant == 'two_gradients' else None,
                                g_x0=dev(o['g_x0']) if variant == 'split' else None, want_g_e=variant != 'no_g_e')
        assert (ge is None) == (variant == 'no_g_e')
        return dict(g_xt=gx, g_e=ge)

    def ref(o):
        x, ee = leaf(o['xt']), leaf(o['e'])
        if variant == 'split':
            x0, add = ddim.predict_x0(x, ee, at, atn)
            gx, ge = torch.autograd.grad((x0, add), (x, ee), (o['g_x0'], o['gout']))
        else:
            out = ddim.ddim_step(x, ee, at, atn)
            out = out.clip(-1, 1) if fc else out
            gx, ge = torch.autograd.grad(out, (x, ee), o['gout'] + o['gout2'] if variant == 'two_gradients' else o['gout'])
        return dict(g_xt=gx, g_e=None if variant == 'no_g_e' else ge)
    got, want = check(call, ops, name, kind, ref, tier2(), channels=3 if name == 'e' else None)
    if name == 'gout' and variant != 'split':
        assert float(want['g_xt'][1].reshape(-1)[spots(SHAPE)[0]]) == 0.0          # the case is in: torch selected a zero there


# =====================================================================================================
# Tier 2: the fused leapfrog update, the Hamiltonian, Metropolis
# =====================================================================================================
def leapfrog_operands(seed):
    g_ = gen(seed)
    return {k: torch.randn(SHAPE, generator=g_) for k in ('x', 'p', 'g', 'g2')}


def sums(ws, N):
    tiles = K.leapfrog_tiles(N)
    return K.sum_partials(ws, tiles, B, stride=2, offset=0), K.sum_partials(ws, tiles, B, stride=2, offset=1)


def leapfrog_ref(mode, o, with_g2):
    x, p, Sx, Sp = hmc_ref.leapfrog_update(mode, o['x'], o['p'], o['g'] + o['g2'] if with_g2 else o['g'],
                                           eps=np.array(EPS), sigma_y=np.array(SIG), m=1.3)
    return dict(x=x, p=p, Sx=Sx, Sp=Sp)


LF_NAMES = ['x', 'p', 'g', 'g2']


LF_CASES = [(n, g2) for g2 in (True, False) for n in LF_NAMES if g2 or n != 'g2']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name,with_g2', LF_CASES, ids=[n + ('' if g2 else '-one_gradient') for n, g2 in LF_CASES])
@pytest.mark.parametrize('mode', ['first', 'mid', 'last', 'first_out_of_place'])
def test_leapfrog(mode, name, with_g2, kind):
    """leapfrog_fused in its three modes and leapfrog_first, with and without the second gradient piece."""
    ops = leapfrog_operands(4)
    N = SHAPE[1] * SHAPE[2] * SHAPE[3]
    base = mode.split('_')[0]

    def call(o):
        x, p, ws = dev(o['x']), dev(o['p']), K.leapfrog_ws(B, N, DEV)
        if mode == 'first_out_of_place':
            x_in, x = x, torch.empty_like(x)
            K.leapfrog_first(x_in, x, p, dev(o['g']), f64(EPS), f64(SIG), 1.3 ** (-1), ws, g2=dev(o['g2']) if with_g2 else None)
            assert torch.equal(x_in.cpu().view(torch.int32), o['x'].view(torch.int32))           # the input is left alone
        else:
            K.leapfrog_fused(dict(first=K.LF_FIRST, mid=K.LF_MID, last=K.LF_LAST)[mode], x, p, dev(o['g']), f64(EPS), f64(SIG),
                             1.3 ** (-1), ws, g2=dev(o['g2']) if with_g2 else None)
        out = dict(x=x, p=p)
        if base != 'mid':
            out.update(ws=ws.clone(), Sx=sums(ws, N)[0], Sp=sums(ws, N)[1])
        return out
    check(call, ops, name, kind, lambda o: leapfrog_ref(base, o, with_g2), tier2())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', LF_NAMES + ['loss'])
def test_leapfrog_through_the_gradient_cache(name, kind):
    """grad_cache_store -> leapfrog_first_cached reads the slot; leapfrog_last_cached fills the other slot: the stored
    gradient (g + g2) and loss are what was handed in, and the updates are the uncached ones."""
    ops = leapfrog_operands(5)
    ops['loss'] = (torch.rand(B, generator=gen(50)).double() * 100).reshape(B, 1)
    N = SHAPE[1] * SHAPE[2] * SHAPE[3]
    sel = torch.tensor([0, 1, 1], dtype=torch.int32)

    def poisoned_loss(o):
        return o['loss'].reshape(B).contiguous()

    def call(o):
        g_pair = torch.zeros((2,) + SHAPE, device=DEV)
        loss_pair = torch.zeros(2, B, dtype=torch.float64, device=DEV)
        dsel = dev(sel)
        K.grad_cache_store(dev(o['g']), dev(o['g2']), dev(poisoned_loss(o)), g_pair, loss_pair, dsel)
        x_out, p1, ws1 = torch.empty(SHAPE, device=DEV), dev(o['p']), K.leapfrog_ws(B, N, DEV)
        K.leapfrog_first_cached(dev(o['x']), x_out, p1, g_pair, dsel, f64(EPS), f64(SIG), 1.3 ** (-1), ws1)
        x2, p2, ws2 = dev(o['x']), dev(o['p']), K.leapfrog_ws(B, N, DEV)
        K.leapfrog_last_cached(x2, p2, dev(o['g']), dev(o['g2']), g_pair, loss_pair, dsel, dev(poisoned_loss(o)), f64(EPS),
                               f64(SIG), 1.3 ** (-1), ws2)
        pick = lambda pair, flip: torch.stack([pair[(int(sel[c]) ^ flip), c] for c in range(B)])
        return dict(x_first=x_out, p_first=p1, ws_first=ws1, x_last=x2, p_last=p2, ws_last=ws2,
                    g_kept=pick(g_pair, 0), g_new=pick(g_pair, 1), loss_kept=pick(loss_pair, 0), loss_new=pick(loss_pair, 1),
                    Sx=sums(ws1, N)[0], Sp=sums(ws2, N)[1])

    def ref(o):
        a, b = leapfrog_ref('first', o, True), leapfrog_ref('last', o, True)
        return dict(x_first=a['x'], p_first=a['p'], x_last=b['x'], p_last=b['p'], g_kept=o['g'] + o['g2'], g_new=o['g'] + o['g2'],
                    loss_kept=poisoned_loss(o), loss_new=poisoned_loss(o), Sx=a['Sx'], Sp=b['Sp'])
    if name == 'loss':                                          # a per-chain scalar: one value at a time
        for v in VALUES[kind]:
            ops2 = dict(ops)
            ops2['loss'] = ops['loss'].clone()
            ops2['loss'][1] = v
            clean, dirty = call(ops), call(ops2)
            assert_isolated(clean, dirty, f'loss/{v}')
            tier2()(dirty, ref(ops2), f'loss/{v}')
        return
    check(call, ops, name, kind, ref, tier2())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', LF_NAMES)
@pytest.mark.parametrize('mode', ['first', 'mid', 'last'])
def test_leapfrog_mass(mode, name, kind):
    from tests.test_state_kernels_gpu import leapfrog_mass_ref
    ops = leapfrog_operands(6)
    M = torch.exp(torch.rand(SHAPE, generator=gen(60)) * 2 - 1)
    std, inv = torch.sqrt(M), 1.0 / M
    N = SHAPE[1] * SHAPE[2] * SHAPE[3]
    md = dict(first=K.LF_FIRST, mid=K.LF_MID, last=K.LF_LAST)[mode]

    def call(o):
        x, ws = dev(o['x']), K.leapfrog_ws(B, N, DEV)
        if md == K.LF_FIRST:                                    # `p` holds the standard-normal draw z; p = z * std comes out
            p = torch.empty(SHAPE, device=DEV)
            K.leapfrog_mass(md, x, p, dev(o['g']), dev(inv), f64(EPS), f64(SIG), ws, g2=dev(o['g2']), z=dev(o['p']), std_m=dev(std))
        else:
            p = dev(o['p'])
            K.leapfrog_mass(md, x, p, dev(o['g']), dev(inv), f64(EPS), f64(SIG), ws, g2=dev(o['g2']))
        out = dict(x=x, p=p)
        if md != K.LF_MID:
            out.update(ws=ws.clone(), Sx=sums(ws, N)[0], Sp=sums(ws, N)[1])
        return out

    def ref(o):
        x, p, _, _, Sx, Sp = leapfrog_mass_ref(md, o['x'], o['p'], o['g'], o['g2'], inv, std, EPS, SIG, None, None, None, 0)
        return dict(x=x, p=p, Sx=Sx, Sp=Sp)
    check(call, ops, name, kind, ref, tier2())


def ulps(H, n=2):
    fin = torch.isfinite(H)
    return n * float(np.spacing(np.float32(H[fin].abs().max()))) if bool(fin.any()) else 0.0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['x', 'p', 'loss'])
def test_hamiltonian(name, kind):
    """H on the sums a FIRST update leaves (eps = 0: the sums only) and a per-chain loss.  `loss`: the loss itself is
    NaN / +inf / -inf; `mixed`: a -inf loss against +inf sums, inf - inf = NaN."""
    ops = leapfrog_operands(7)
    N = SHAPE[1] * SHAPE[2] * SHAPE[3]
    loss = torch.rand(B, generator=gen(70)).double() * 5e3

    def H_of(o, lossv):
        ws = K.leapfrog_ws(B, N, DEV)
        K.leapfrog_fused(K.LF_FIRST, dev(o['x']), dev(o['p']), dev(torch.zeros(SHAPE)), 0.0, SIG, 1.0, ws)
        H, terms = K.hamiltonian(ws, N, dev(lossv), SIG, 1.0, want_terms=True)
        return dict(H=H, terms=terms, ws=ws)

    def H_ref(o, lossv):
        Sx, Sp = torch.sum(o['x'] ** 2, dim=(1, 2, 3)), torch.sum(o['p'] * o['p'], dim=(1, 2, 3))
        return hmc_ref.hamiltonian(Sx, lossv.float(), Sp, 1 / (2 * np.array(SIG) ** 2), 1.0)
    clean = H_of(ops, loss)
    cases = []
    if name == 'loss':
        for v in ([NAN, INF, -INF] if kind == 'mixed' else VALUES[kind][:1]):
            bad = loss.clone()
            bad[1] = v
            cases.append((ops, bad))
        if kind == 'mixed':
            bad = loss.clone()
            bad[1] = -INF
            cases.append((dict(ops, x=poisoned(ops['x'], 'pinf')), bad))
    else:
        cases.append((dict(ops, **{name: poisoned(ops[name], kind)}), loss))
    for o, lossv in cases:
        got, want = H_of(o, lossv), H_ref(o, lossv)
        assert_isolated(clean, got, f'{name}/{kind}')
        H = got['H'].cpu()
        assert torch.equal(torch.isnan(H), torch.isnan(want)), (H, want)
        for s in (INF, -INF):
            assert torch.equal(H == s, want == s), (H, want)
        fin = torch.isfinite(want)
        assert float((H[fin] - want[fin]).abs().max()) <= ulps(want)
        assert not bool(torch.isfinite(want[1]))                                     # the case is in


def test_metropolis_on_non_finite_hamiltonians():
    """min(1, exp(-dH)) with the documented deviation: dH = NaN (inf - inf included) rejects; dH = +inf rejects (ratio 0),
    dH = -inf accepts (ratio 1) -- whatever u in [0, 1) is drawn.  Finite neighbours decide as they do alone."""
    def rule(dh, uv):
        if math.isnan(dh):
            return 0                                                # the deviation: the reference's min(1, NaN) is 1
        return 1 if dh == -INF else int(uv < min(1.0, math.exp(-dh)))   # exp(-inf) = 0: dH = +inf never accepts
    vals = [0.0, 10.0, INF, -INF, NAN]
    H0 = torch.tensor([a for a in vals for _ in vals])
    H1 = torch.tensor([b for _ in vals for b in vals])
    for uv in (0.0, 0.5, 0.999):
        u = torch.full_like(H0, uv)
        acc, dH = K.metropolis(dev(H0), dev(H1), dev(u))
        d = H1 - H0
        want = [rule(x, uv) for x in d.tolist()]
        assert acc.cpu().tolist() == want, (uv, acc.cpu().tolist(), want)
        assert torch.equal(torch.isnan(dH.cpu()), torch.isnan(d)) and torch.equal(dH.cpu()[~torch.isnan(d)], d[~torch.isnan(d)])
        for i, x in enumerate(d.tolist()):
            if math.isnan(x) or x == INF:
                assert want[i] == 0
            if x == -INF:
                assert want[i] == 1
        fin = torch.isfinite(H0) & torch.isfinite(H1)
        alone, _ = K.metropolis(dev(H0[fin]), dev(H1[fin]), dev(u[fin]))
        assert torch.equal(acc.cpu()[fin], alone.cpu())


# =====================================================================================================
# Tier 2: the elementwise data terms and their fused last-step forms
# =====================================================================================================
class HdrRef:
    """obs_functions/Hfuncs.py:406-445: H(x) = clip(x / 0.5, -1, 1)."""

    def __init__(self, M):
        self.M = M

    def H(self, x):
        return torch.clip(x / 0.5, -1, 1).reshape(x.shape[0], -1)


def inpaint_pair(dim, whole_pixels, seed):
    """(reference operator, device operator) of a random mask that keeps the poisoned spots: whole pixels missing (the bit
    mask form, hw % 32 == 0) or single elements (the dense slot form)."""
    import nhmc.operators as ops
    hw = dim * dim
    sp = spots((B, 3, dim, dim))
    g_ = gen(seed)
    if whole_pixels:
        keep_px = {i % hw for i in sp}
        px = [int(i) for i in torch.randperm(hw, generator=g_)[: int(hw * 0.8)] if int(i) not in keep_px]
        r = 3 * torch.tensor(px)
        missing = torch.cat([r, r + 1, r + 2])
    else:
        keep_hwc = {(i % hw) * 3 + i // hw for i in sp}
        missing = torch.tensor([int(i) for i in torch.randperm(3 * hw, generator=g_)[: int(3 * hw * 0.6)] if int(i) not in keep_hwc])
    op = ops.Inpainting(3, dim, missing, DEV)
    assert (op.mask_words is not None) == whole_pixels
    return oops.InpaintRef(3, dim, missing), op


def elementwise_pair(which, dim=20):
    import nhmc.operators as ops
    if which == 'inpaint':
        return inpaint_pair(dim, False, 8)
    if which == 'inpaint_px':
        return inpaint_pair(32, True, 9)
    if which == 'hdr':
        return HdrRef(3 * dim * dim), ops.HDR(channels=3, img_dim=dim)
    if which == 'color':
        return oops.ColorRef(dim), ops.Colorization(dim, DEV)
    r = int(which[2:])
    d = 20 if r == 4 else 32                                   # 20: k_mix_bwd_sr4 with a ragged last wave (25 items of 64)
    return oops.BlockMeanRef(3, d, r), ops.SuperResolution(3, d, r, DEV)


LOSS_TOL = dict(inpaint=1e-6, inpaint_px=1e-6, hdr=1e-6, color=2e-6)        # the finite tests' bounds on the loss


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('apply_clip', [True, False], ids=['clip', 'noclip'])
@pytest.mark.parametrize('which', ['inpaint', 'hdr', 'color'])
def test_elementwise_data_terms(which, apply_clip, kind):
    ref_op, op = elementwise_pair(which)
    g_ = gen(10)
    ops = dict(xt=torch.randn(SHAPE, generator=g_) * 0.8)
    y = torch.randn(B, ref_op.M, generator=g_)
    dy = dev(y)

    def call(o):
        loss, g = op.data_term(dev(o['xt']), dy, apply_clip=apply_clip)
        return dict(loss=loss, g=g)

    def ref(o):
        loss, g = hmc_ref.data_term(o['xt'], ref_op, y, apply_clip=apply_clip)
        return dict(loss=loss, g=g)
    got, want = check(call, ops, 'xt', kind, ref, tier2(loss_tol=LOSS_TOL[which]))
    if kind == 'nan' and apply_clip:                             # clamp(NaN) is NaN: the loss sees it, and the clamp backward selects 0
        assert math.isnan(float(want['loss'][1])) and float(want['g'][1].reshape(-1)[0]) == 0.0


def last_vjp_ref(ref_op, o, at, atn, y):
    """autograd through the oracle's last DDIM step, its final clip and the data term -> loss [B], g_xt, g_e"""
    x, e = leaf(o['xt']), leaf(o['e'])
    dec = ddim.ddim_step(x, e, at, atn).clip(-1, 1)
    resid = y - ref_op.H(dec)
    per = (resid ** 2).reshape(B, -1).sum(1)
    gx, ge = torch.autograd.grad(per.sum(), (x, e))
    return dict(loss=per.detach(), g_xt=gx, g_e=ge)


FUSED = ['inpaint', 'inpaint_px', 'hdr', 'color', 'sr2', 'sr4', 'sr8', 'sr16']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['xt', 'e'])
@pytest.mark.parametrize('which', FUSED)
def test_fused_last_step_forms(which, name, kind):
    """ddim_mix_bwd_inpaint (slot form), ddim_mix_bwd_inpaint_px, mix_bwd_hdr, ddim_mix_bwd_color, ddim_mix_bwd_sr at
    ratios 2, 4, 8, 16.  The block-mean forms are held to the finite test's 2e-6; the others are bit-exact."""
    ref_op, op = elementwise_pair(which)
    d = ref_op.img_dim if hasattr(ref_op, 'img_dim') else 20
    g_ = gen(11)
    ops = dict(xt=torch.randn(B, 3, d, d, generator=g_) * 0.5, e=torch.randn(B, 6, d, d, generator=g_))
    y = torch.randn(B, ref_op.M, generator=g_)
    dy = dev(y)
    at, atn = last_step_alphas()

    def call(o):
        loss, gx, ge = op.fused_last_vjp(dev(o['xt']), dev(o['e']), at, atn, dy)
        return dict(loss=loss, g_xt=gx, g_e=ge)
    sr = which.startswith('sr')
    check(call, ops, name, kind, lambda o: last_vjp_ref(ref_op, o, at, atn, y),
          tier2(loss_tol=2e-6 if sr else LOSS_TOL[which], tol=2e-6 if sr else 0.0), channels=3 if name == 'e' else None)


# =====================================================================================================
# Tier 2: PSNR and the commits
# =====================================================================================================
def psnr_ref(a, b):
    return torch.stack([hmc_ref.psnr_unit(hmc_ref.to_unit_range(a[i]), hmc_ref.to_unit_range(b[i])) for i in range(a.shape[0])])


@pytest.mark.parametrize('kind', KINDS)
def test_psnr_of_a_non_finite_sample(kind):
    """clamp((x + 1) / 2, 0, 1) keeps a NaN (and sends +-inf to 1 / 0): a NaN sample has a NaN PSNR."""
    g_ = gen(12)
    a, other, orig = torch.randn(SHAPE, generator=g_), torch.randn(SHAPE, generator=g_), torch.rand(SHAPE, generator=g_) * 2 - 1
    do = dev(orig)

    def call(o):
        samples = torch.stack([o['a'], other], dim=1)
        return dict(psnr=K.psnr(dev(o['a']), do), rows=K.psnr_samples(dev(samples), do))

    def ref(o):
        return dict(psnr=psnr_ref(o['a'], orig), rows=torch.stack([psnr_ref(o['a'], orig), psnr_ref(other, orig)], dim=1))

    def compare(got, want, what):
        for k in want:
            g, r = got[k].cpu(), want[k]
            assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, k, g, r)
            fin = torch.isfinite(r)
            assert torch.equal(torch.isfinite(g), fin) and torch.allclose(g[fin], r[fin], rtol=0, atol=1e-4), (what, k, g, r)
    got, want = check(call, dict(a=a), 'a', kind, ref, compare)
    assert math.isnan(float(want['psnr'][1])) == (kind in ('nan', 'mixed'))
    assert torch.equal(got['rows'][:, 1], K.psnr(dev(other), do))                     # the chain's other sample: unchanged


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def payload(t, kind):
    """poisoned, plus a NaN with a payload (0x7fc12345) in a fourth place: a move is verbatim, sign and payload included"""
    out = poisoned(t, kind)
    out[1].reshape(-1).view(torch.int32)[7] = 0x7fc12345
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_commits_move_verbatim(kind):
    g_ = gen(13)
    x, x_prop, xt_prop, xt_last = (torch.randn(SHAPE, generator=g_) for _ in range(4))
    epochs, sampling, keep = 4, 2, 2
    accept = torch.tensor([1, 1, 0], dtype=torch.int32)
    epoch = torch.tensor([7, 6, 7], dtype=torch.int32)          # sample slots 1, 0, (1)

    def run(xp, xtp, xtl):
        dx, ds = dev(x), torch.zeros(B, sampling, *SHAPE[1:], device=DEV)
        K.accept_commit(dev(accept), dev(epoch), dx, dev(xp), dev(xtp), ds, epochs, sampling)
        lx, ll, ring = dev(x), dev(xtl), torch.zeros(B, keep, *SHAPE[1:], device=DEV)
        st = dict(has_prev=torch.ones(B, dtype=torch.int32, device=DEV), count=torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV))
        K.latent_commit(dev(accept), st, True, keep, lx, dev(xp), ll, dev(xtp), ring)
        return dict(x=dx, samples=ds, lx=lx, xt_last=ll, ring=ring)
    clean = run(x_prop, xt_prop, xt_last)
    bad = [payload(t, kind) for t in (x_prop, xt_prop, xt_last)]
    dirty = run(*bad)
    for k in clean:
        assert torch.equal(bits(rows(clean[k])), bits(rows(dirty[k]))), k
    assert torch.equal(bits(dirty['x'][1]), bits(bad[0][1])) and torch.equal(bits(dirty['lx'][1]), bits(bad[0][1]))
    assert torch.equal(bits(dirty['samples'][1, 0]), bits(bad[1][1])) and not bool(dirty['samples'][1, 1].any())
    assert torch.equal(bits(dirty['xt_last'][1]), bits(bad[1][1]))
    assert torch.equal(bits(dirty['ring'][1, 1]), bits(bad[2][1])) and not bool(dirty['ring'][1, 0].any())   # the previous decode
    assert torch.equal(bits(dirty['x'][2]), bits(x[2]))                                  # the rejected chain kept its place


# =====================================================================================================
# Tier 1: the data terms that mix pixels
# =====================================================================================================
class PhaseRef:
    """H(x) = |Fc x Fc^T| per plane with Fc the centred orthonormal DFT restricted to the unpadded columns (the
    operator's own float64 definition, in complex64)."""

    def __init__(self, op):
        self.Fc = torch.complex(op.Cm, op.Sm).to(torch.complex64)
        self.dim, self.M = op.img_dim, op.M

    def H(self, x):
        X = x.reshape(x.shape[0], 3, self.dim, self.dim).to(torch.complex64)
        return torch.matmul(torch.matmul(self.Fc, X), self.Fc.t()).abs().reshape(x.shape[0], -1)


def mixing_pair(which):
    import nhmc.operators as ops
    device = torch.device(DEV)
    if which.startswith('cs'):
        dim = int(which.split('_')[1])
        op = ops.build_operator('cs4', 3, dim, device, generator=gen(14))
        return oops.WalshHadamardRef(3, dim, 4, op.perm.cpu()), op, dim
    if which.startswith('spectral'):
        op = ops.build_operator('deblur_aniso', 3, 32, device, spectral_projected=which.endswith('projected'))
        assert op.projected == which.endswith('projected')
        U1, U2, V1, V2 = (op.factors[i].cpu() for i in range(4))
        return oops.SpectralBlurRef(U1, U2, V1, V2, op.Dmap.cpu().reshape(3, 32, 32)), op, 32
    if which == 'srconv':
        op = ops.build_operator('sr_bicubic2', 3, 64, device)
        return oops.SeparableStridedRef(ops.bicubic_taps(2), 3, 64, 2), op, 64
    if which == 'phase':
        op = ops.build_operator('phase_retrieval', 3, 32, device)
        return PhaseRef(op), op, 32
    assert which == 'sr4'
    return oops.BlockMeanRef(3, 20, 4), ops.SuperResolution(3, 20, 4, device), 20


MIXING = ['cs_32', 'cs_64', 'spectral', 'spectral_projected', 'srconv', 'phase', 'sr4']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('which', MIXING)
def test_mixing_data_terms(which, kind):
    """data_cs (32 and 64), data_spectral (eight products and projected), data_srconv, data_phase, data_sr."""
    ref_op, op, d = mixing_pair(which)
    g_ = gen(15)
    ops = dict(xt=torch.randn(B, 3, d, d, generator=g_) * 0.8)
    y = torch.randn(B, ref_op.M, generator=g_)
    dy = dev(y)

    def call(o):
        loss, g = op.data_term(dev(o['xt']), dy, apply_clip=True)
        return dict(loss=loss, g=g)

    def ref(o):
        loss, g = hmc_ref.data_term(o['xt'], ref_op, y)
        return dict(loss=loss, g=g)
    got, want = check(call, ops, 'xt', kind, ref, tier1)
    if kind in ('nan', 'mixed'):
        assert math.isnan(float(want['loss'][1]))                                     # the case is in


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['xt', 'e'])
@pytest.mark.parametrize('which', [w for w in MIXING if w != 'sr4'])
def test_mixing_data_terms_fused_with_the_last_step(which, name, kind):
    """data_cs_vjp, data_spectral(_proj)_vjp, data_srconv_vjp, data_phase_vjp on the decode the engine hands them."""
    ref_op, op, d = mixing_pair(which)
    g_ = gen(16)
    ops = dict(xt=torch.randn(B, 3, d, d, generator=g_) * 0.5, e=torch.randn(B, 6, d, d, generator=g_))
    y = torch.randn(B, ref_op.M, generator=g_)
    dy = dev(y)
    at, atn = last_step_alphas()

    def call(o):
        xt, e = dev(o['xt']), dev(o['e'])
        cur = K.ddim_mix_fwd(xt, e, at, atn, final_clip=True)['xt_next']
        loss, gx, ge = op.fused_last_vjp(xt, e, at, atn, dy, xt_next=cur)
        return dict(loss=loss, g_xt=gx, g_e=ge)
    got, want = check(call, ops, name, kind, lambda o: last_vjp_ref(ref_op, o, at, atn, y), tier1,
                      channels=3 if name == 'e' else None)
    if kind in ('nan', 'mixed'):
        assert math.isnan(float(want['loss'][1]))


# =====================================================================================================
# Tier 1: the score network's glue -- GroupNorm, bias + residual add, the Winograd convolution
# =====================================================================================================
def gn_torch(x, gamma, beta, fm, pb, groups, eps, act):
    xx = x + pb[:, :, None, None]
    h = F.group_norm(xx, groups, gamma, beta, eps)
    sc, sh = fm[:, :, None, None].chunk(2, dim=1)
    h = h * (1 + sc) + sh
    return F.silu(h) if act else h


GN_ROUTES = [('two_pass', (B, 64, 16, 16), 0), ('one_pass', (B, 128, 64, 64), 0), ('one_pass_nowait', (B, 128, 64, 64), 1)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['x', 'dy'])
@pytest.mark.parametrize('route,shape,nowait', GN_ROUTES, ids=[r[0] for r in GN_ROUTES])
def test_group_norm(route, shape, nowait, name, kind, monkeypatch):
    """gn_act_fwd / gn_act_bwd: a poisoned group of sample 1 is non-finite wherever torch's is, and the slabs of samples
    0 and 2 -- which share the workspaces with it -- keep their bits, statistics included."""
    groups, eps, act = 32, 1e-5, True
    g_ = gen(17 + shape[1])
    C = shape[1]
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g_), 0.1 * torch.randn(C, generator=g_)
    fm, pb = 0.3 * torch.randn(B, 2 * C, generator=g_), 0.5 * torch.randn(B, C, generator=g_)
    ops = dict(x=torch.randn(shape, generator=g_) * 1.7 + 0.3, dy=torch.randn(shape, generator=g_))
    one = route != 'two_pass'
    if one:
        assert K.gn_onepass_splits(B, C, groups, shape[2] * shape[3]) > 1             # more than one workgroup per slab
    else:
        monkeypatch.setenv('NHMC_GN_ONEPASS', '0')
    flags = K.GN_ONEPASS_NOWAIT if nowait else 0
    dgamma, dbeta, dfm, dpb = dev(gamma), dev(beta), dev(fm), dev(pb)

    def call(o):
        x, dy = dev(o['x']), dev(o['dy'])
        y, ws, splits = K.gn_act_fwd(x, dgamma, dbeta, groups, eps, act, dfm, dpb, flags=flags, onepass=True if one else None)
        dx = K.gn_act_bwd(x, dy, dgamma, dbeta, groups, eps, act, dfm, ws, splits, dpb, flags=flags, onepass=True if one else None)
        cut = B * groups * splits * 2                            # partials [slab][split][2]; one-pass: then the slab totals [slab][2]
        return dict(y=y, dx=dx, ws=ws[:cut], totals=ws[cut:] if ws.numel() > cut else None)

    def ref(o):
        x = leaf(o['x'])
        y = gn_torch(x, gamma, beta, fm, pb, groups, eps, act)
        (dx,) = torch.autograd.grad(y, x, o['dy'])
        return dict(y=y.detach(), dx=dx)
    got, want = check(call, ops, name, kind, ref, tier1)
    assert not bool(torch.isfinite(want['dx'][1]).all())


@pytest.mark.parametrize('route,shape,nowait', GN_ROUTES, ids=[r[0] for r in GN_ROUTES])
def test_group_norm_silu_at_the_ends(route, shape, nowait, monkeypatch):
    """The forward's SiLU where its argument leaves the range of exp, driven there by the FiLM shift of single channels
    of sample 1 (the statistics do not see it): u = -1e4 and -1e30 give 0 as torch's fp32 SiLU does (exp(-u) overflows),
    -inf gives NaN and +inf gives +inf as torch's do, +1e30 gives u; the other channels and samples keep their bits."""
    groups, eps, C = 32, 1e-5, shape[1]
    g_ = gen(29 + C)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g_), 0.1 * torch.randn(C, generator=g_)
    fm, pb = 0.3 * torch.randn(B, 2 * C, generator=g_), 0.5 * torch.randn(B, C, generator=g_)
    x = torch.randn(shape, generator=g_) * 1.7 + 0.3
    ends = {5: -INF, 6: -1e4, 7: -1e30, 40: INF, 41: 1e30}               # channel of sample 1 -> its shift
    fm_ends = fm.clone()
    for ch, v in ends.items():
        fm_ends[1, C + ch] = v
    one = route != 'two_pass'
    if one:
        assert K.gn_onepass_splits(B, C, groups, shape[2] * shape[3]) > 1
    else:
        monkeypatch.setenv('NHMC_GN_ONEPASS', '0')
    flags = K.GN_ONEPASS_NOWAIT if nowait else 0

    def call(f):
        return K.gn_act_fwd(dev(x), dev(gamma), dev(beta), groups, eps, True, dev(f), dev(pb), flags=flags, onepass=True if one else None)[0].cpu()
    clean, got = call(fm), call(fm_ends)
    want = gn_torch(x, gamma, beta, fm_ends, pb, groups, eps, True)
    rest = torch.ones(B, C, dtype=torch.bool)
    rest[1, list(ends)] = False
    assert torch.equal(got[rest], clean[rest]) and bool(torch.isfinite(clean).all())
    assert bool(torch.isnan(want[1, 5]).all()) and bool(torch.isnan(got[1, 5]).all())
    for ch in (6, 7):
        assert bool((want[1, ch] == 0).all()) and bool((got[1, ch] == 0).all()), (ch, got[1, ch].abs().max())
    assert bool((want[1, 40] == INF).all()) and bool((got[1, 40] == INF).all())
    assert float((got[1, 41] - want[1, 41]).abs().max()) <= 1e-6 * 1e30


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['h', 'other'])
def test_bias_add2(name, kind):
    g_ = gen(18)
    shape = (B, 5, 20, 20)
    ops = dict(h=torch.randn(shape, generator=g_), other=torch.randn(shape, generator=g_))
    bias = torch.randn(5, generator=g_)
    db = dev(bias)
    check(lambda o: dict(out=K.bias_add2(dev(o['h']), db, dev(o['other']))), ops, name, kind,
          lambda o: dict(out=(o['h'] + bias.view(1, -1, 1, 1)) + o['other']), tier2())


WINO = [('main', (B, 8, 64, 4, 64)), ('narrow', (B, 8, 64, 8, 32)), ('k32', (B, 8, 32, 4, 64))]       # n, c, k, h, w of the kernel


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('entry,shape', WINO, ids=[w[0] for w in WINO])
def test_winograd_conv(entry, shape, backward):
    """One NaN at a corner pixel and one at an interior pixel of image 1.  The transform spreads a NaN over the tiles
    that read it, so: non-finite at least wherever conv2d in fp32 is; images 0 and 2 keep their bits."""
    n, c, k, h, w = shape
    assert K.conv3x3_wino_k32_covers(*shape) and K.conv3x3_wino_covers(*shape) == (entry != 'k32')
    g_ = gen(19 + k + w)
    src = torch.randn(n, c, h, w, generator=g_)
    wt = torch.randn((c, k, 3, 3) if backward else (k, c, 3, 3), generator=g_) / (9 * c) ** 0.5
    dwt = dev(wt)
    bad = src.clone()
    bad[1, 0, 0, 0] = NAN
    bad[1, c // 2, h // 2, w // 2 + 1] = NAN
    clean = dict(y=K.conv3x3_wino(dev(src), dwt, backward=bool(backward)))
    dirty = dict(y=K.conv3x3_wino(dev(bad), dwt, backward=bool(backward)))
    assert_isolated(clean, dirty, entry)
    want = torch.nn.grad.conv2d_input((n, k, h, w), wt, bad, 1, 1) if backward else F.conv2d(bad, wt, padding=1)
    assert int(torch.isnan(want[1]).sum()) == k * (4 + 9) and bool(torch.isfinite(want[[0, 2]]).all())
    assert_not_laundered(dirty['y'], want, entry)


# =====================================================================================================
# Whole trajectories: a chain whose decode diverges
# =====================================================================================================
MARK = (1, 1, 16, 17)
KEYS = ('x_prop', 'p', 'xt', 'loss', 'H0', 'H1')
TRAJ_OPS = ['inpaint_random', 'sr4', 'cs4', 'hdr', 'deblur_gauss']


def traj_pair(deg, dim):
    import nhmc.operators as ops
    op = ops.build_operator(deg, 3, dim, torch.device(DEV), generator=gen(20))
    if deg == 'inpaint_random':
        return oops.InpaintRef(3, dim, op.missing_indices.cpu()), op
    if deg == 'sr4':
        return oops.BlockMeanRef(3, dim, 4), op
    if deg == 'cs4':
        return oops.WalshHadamardRef(3, dim, 4, op.perm.cpu()), op
    if deg == 'hdr':
        return HdrRef(3 * dim * dim), op
    U1, U2, V1, V2 = (op.factors[i].cpu() for i in range(4))
    return oops.SpectralBlurRef(U1, U2, V1, V2, op.Dmap.cpu().reshape(3, dim, dim)), op


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('score', ['grad', 'nograd'])
@pytest.mark.parametrize('deg', TRAJ_OPS)
def test_a_diverging_chain_is_rejected_and_its_neighbours_do_not_notice(deg, score, graph):
    """sampler.run_trajectory, L = 2.  With the no-grad score the gradient and the momentum of chain 1 stay finite: only
    the NaN of the final clip's output -- the loss of the data term -- tells that the decode diverged."""
    from nhmc import plugin, sampler
    dim, L = 32, 2
    ref_op, op = traj_pair(deg, dim)
    make = (lambda: DivergingScore()) if score == 'grad' else (lambda: NoGradDivergingScore())
    g_ = gen(21)
    x_orig = torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1
    y = (op.H(dev(x_orig)) + 0.1 * dev(torch.randn(B, ref_op.M, generator=g_))).contiguous()
    x, p = torch.randn(B, 3, dim, dim, generator=g_), torch.randn(B, 3, dim, dim, generator=g_)
    xm = x.clone()
    xm[MARK] = 41.0
    b = osched.betas_fp32()

    def run(x0):
        eng = sampler.LeapfrogEngine(plugin.HMC(make().to(DEV), op, 0.1).score, op, b.to(DEV), SEQ, SEQ_NEXT, torch.device(DEV))
        st = sampler.ChainState(B, 1.0, 0.05, DEV)
        st['eps_eff'].copy_(torch.tensor(EPS, dtype=torch.float64))
        st['sigma_y'].copy_(torch.tensor(SIG, dtype=torch.float64))
        got = sampler.run_trajectory(eng, dev(x0), dev(p), y, st, 1.0, L, graph=graph)
        torch.cuda.synchronize()
        return {k: got[k].clone() for k in KEYS}
    clean, got = run(x), run(xm)
    assert_isolated(clean, got, deg)
    want = hmc_ref.trajectory(xm, p.clone(), b, SEQ, SEQ_NEXT, make(), ref_op, y.cpu(), sigma_y=np.array(SIG), eps=np.array(EPS),
                              m=1.0, L=L)
    assert math.isnan(float(want['loss'][1])) and math.isnan(float(want['H1'][1])) and bool(torch.isnan(want['xt'][1]).any())
    assert math.isnan(float(got['loss'][1])), f'loss of the diverged chain: {float(got["loss"][1])}'
    assert math.isnan(float(got['H1'][1])), f'H1 of the diverged chain: {float(got["H1"][1])}'
    assert_not_laundered(got['xt'][1], want['xt'][1], 'xt')
    u = torch.full((B,), 0.25, device=DEV)
    accept, alone = K.metropolis(got['H0'], got['H1'], u)[0].cpu().tolist(), K.metropolis(clean['H0'], clean['H1'], u)[0].cpu().tolist()
    assert accept[1] == 0 and accept[0] == alone[0] and accept[2] == alone[2], (accept, alone)


def test_a_diverging_chain_never_accepts_in_a_short_run():
    """hmc_chains with the no-grad score, eight trajectories: chain 1 never accepts and collects no sample; the others run
    as they do without the marker."""
    import types
    from nhmc import plugin, sampler
    dim = 32
    ref_op, op = traj_pair('inpaint_random', dim)
    g_ = gen(22)
    x_orig = dev(torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1)
    y = (op.H(x_orig) + 0.1 * dev(torch.randn(B, ref_op.M, generator=g_))).contiguous()
    x = torch.randn(B, 3, dim, dim, generator=g_)
    xm = x.clone()
    xm[MARK] = 41.0
    opt = types.SimpleNamespace(tau=0.02, epsilon=0.01, m=1.0, sigma_0=1.5)     # L = 2, small steps: nearly every proposal is accepted

    def run(x0):
        algo = plugin.HMC(NoGradDivergingScore().to(DEV), op, 0.1)
        return sampler.hmc_chains(dev(x0), osched.betas_fp32().to(DEV), SEQ, SEQ_NEXT, algo, opt, y, op, x_orig,
                                  noise=sampler.PhiloxNoise(7, 0), epochs=1, sampling=2, max_iters=8)
    clean, got = run(x), run(xm)
    assert got.iters == clean.iters
    assert int(got.n_accept[1]) == 0 and not bool(got.samples[1].any()), (got.n_accept.tolist(), float(got.samples[1].abs().max()))
    assert torch.equal(got.x[1].cpu(), xm[1])
    for k in ('samples', 'x', 'n_accept'):
        assert torch.equal(rows(getattr(clean, k)), rows(getattr(got, k))), k
    assert int(clean.n_accept.sum()) > 0 and bool(clean.samples[[0, 2]].any())        # the run did accept and collect

"""GPU: the general 2-D PSF blur kernels (csrc/blur2d.hip) and the `deblur_motion` degradation through the layers above.

The float64 restatement `blur_ref` (tests/test_blur2d_cpu.py, pinned there against F.conv2d and autograd) is the
reference.  The kernel's tile is 32 rows x 64 columns and it stages the tap list 512 taps at a time, so the image sizes are
16 (below the tile), 32 and 64 (one tile high / one tile wide), 80 (no multiple of either: partial tiles on both axes,
3 x 2 tiles) and 128 (4 x 2 tiles), and the tap counts include 511, 512 and 513.
"""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hmc_ref, schedule as osched
from tests.test_blur2d_cpu import blur_ref, data_ref, taps_of

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
DEV = 'cuda'
U = 2.0 ** -24
SIZES = (16, 32, 64, 80, 128)
TAP_CHUNK = 512                                        # BL_TAPC of csrc/blur2d.hip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_op(k, C, d):
    from nhmc import operators
    return operators.Blur2D(k, C, d, DEV)


def psf(name, seed=0):
    """The PSFs of the issue.  `dyadic=True` variants (for the exactly summable data) are built by `dyadic_psf`."""
    from nhmc import operators
    g_ = gen(1000 + seed)
    if name == 'k1':
        return torch.tensor([[0.75]])
    if name == 'shift':                                 # a single off-centre tap at (dy, dx) = (-R, +R), K = 9
        k = torch.zeros(9, 9)
        k[0, 8] = 1.0
        return k
    if name == 'motion':
        return operators.motion_kernel(61, 0.5, g_)
    if name == 'dense15':                               # dense, signed
        return torch.randn(15, 15, generator=g_) * 0.1
    if name == 'dense63':                               # T = 3969, R = 31 larger than the smallest image
        return (torch.rand(63, 63, generator=g_) + 0.05) / 2000.0
    if name.startswith('taps'):                         # K = 23 (529 entries) with exactly T non-zeros: around the tap chunk
        T = int(name[4:])
        k = torch.randn(23, 23, generator=g_) * 0.05
        k[k == 0] = 0.01
        drop = torch.randperm(529, generator=g_)[: 529 - T]
        k.view(-1)[drop] = 0
        assert int((k != 0).sum()) == T
        return k
    raise KeyError(name)


def dyadic_psf(name, seed=0):
    """Weights on the grid 2^-4 with |w| <= 1/4 on the support of `psf(name)`."""
    k = psf(name, seed)
    g_ = gen(2000 + seed)
    q = torch.randint(1, 5, k.shape, generator=g_).float() / 16.0
    sgn = torch.where(torch.rand(k.shape, generator=g_) < 0.5, -1.0, 1.0)
    return torch.where(k != 0, q * sgn, torch.zeros_like(k))


def abs_taps(taps):
    return taps[0], taps[1].abs()


def gamma(T):
    return (T + 2) * U / (1 - (T + 2) * U)


def images(B, C, d, seed, scale=0.8):
    g_ = gen(seed)
    x = torch.randn(B, C, d, d, generator=g_) * scale
    y = torch.randn(B, C, d, d, generator=g_) * 0.5
    return x, y


# ---- 1. shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', SIZES)
def test_single_tap_is_a_pure_shift(d):
    """(H x)[r][s] = x[r - 4][s + 4] with zero fill, H^T the shift back: bit for bit against indexing.  Catches a flipped
    or transposed convention and every halo off-by-one."""
    op = make_op(psf('shift'), 3, d)
    assert op.taps()[0].tolist() == [[-4, 4]]
    x, _ = images(3, 3, d, 10 + d)
    want = torch.zeros_like(x)
    want[..., 4:, :d - 4] = x[..., :d - 4, 4:]
    got = op.H(x.to(DEV)).reshape(x.shape).cpu()
    assert torch.equal(got, want)
    back = torch.zeros_like(x)
    back[..., :d - 4, 4:] = x[..., 4:, :d - 4]
    assert torch.equal(op.Ht(x.to(DEV)).reshape(x.shape).cpu(), back)


# ---- 2. exactly summable data ------------------------------------------------------------------------------------
def dyadic_images(B, C, d, seed):
    g_ = gen(seed)
    x = torch.randint(-3, 4, (B, C, d, d), generator=g_).float() / 2.0              # {0, +-1/2, +-1, +-3/2}
    x[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 1.25, -1.25])                         # on the bounds / outside them
    x[-1, -1, d - 1, d - 4:] = torch.tensor([-1.25, 1.0, 1.25, -1.0])
    y = torch.randint(-64, 65, (B, C, d, d), generator=g_).float() / 32.0           # multiples of 2^-5 in [-2, 2]
    return x, y


def exactly_summable(w, operand, grid_bits):
    """Every partial sum of sum_t w_t a_t, in any order, is a multiple of 2^-grid_bits below 2^24 of them: exact in fp32."""
    return float(w.double().abs().sum()) * float(operand.double().abs().max()) * 2.0 ** grid_bits < 2.0 ** 24


@pytest.mark.parametrize('name,C,d', [('motion', 3, 16), ('motion', 3, 80), ('motion', 3, 128), ('dense15', 3, 32),
                                      ('dense15', 3, 64), ('dense15', 1, 80), ('taps511', 3, 80)])
def test_exactly_summable_data_gives_the_restatement_bit_for_bit(name, C, d):
    B = 3
    k = dyadic_psf(name)
    op = make_op(k, C, d)
    taps = op.taps()
    x, y = dyadic_images(B, C, d, 20 + d)
    # the precondition, on the host: grids x 2^-2, w 2^-4, y 2^-5 -> products 2^-6 (H, H^T of x), 2^-5 (H of clip x),
    # residual 2^-5, -2 r 2^-4, its products with w 2^-8
    assert bool((x * 4 == (x * 4).round()).all()) and bool((k * 16 == (k * 16).round()).all()) and bool((y * 32 == (y * 32).round()).all())
    assert exactly_summable(taps[1], x, 6)
    _, g_ref, r_ref = data_ref(x, y, taps, True)
    assert exactly_summable(taps[1], x.clip(-1, 1), 5) and exactly_summable(taps[1], 2 * r_ref, 8)
    xd, yd = x.to(DEV), y.to(DEV)
    assert torch.equal(op.H(xd).reshape(x.shape).cpu().double(), blur_ref(x, taps))
    assert torch.equal(op.Ht(xd).reshape(x.shape).cpu().double(), blur_ref(x, taps, transpose=True))
    for clip in (True, False):
        l_ref, g_ref, r_ref = data_ref(x, y, taps, clip)
        if not clip:
            assert exactly_summable(taps[1], 2 * r_ref, 8 + 1)                      # x itself on 2^-2: one more bit
        loss, g = op.data_term(xd, yd.reshape(B, -1), clip)
        assert torch.equal(g.cpu().double(), g_ref), (name, d, clip)
        rel = ((loss.cpu() - l_ref).abs() / l_ref).max()
        print(f'{name} d={d} clip={clip}: loss rel err {float(rel):.2e} (bound {2.0 ** -23:.2e})')
        assert float(rel) <= 2.0 ** -23                                             # the only roundings: the fp32 squares
        if clip:
            assert bool((g[0, 0, 0, 2:4] == 0).all()) and bool((g_ref[0, 0, 0, :2] != 0).all())
    # the adjoint identity is exact on this data (every term a small dyadic number, float64 sums exact)
    w_img = y
    lhs = (op.H(xd).reshape(x.shape).cpu().double() * w_img.double()).sum()
    rhs = (x.double() * op.Ht(w_img.to(DEV)).reshape(x.shape).cpu().double()).sum()
    assert float(lhs) == float(rhs)


# ---- 3 + 4. real-valued data against float64, derived bounds; the adjoint ----------------------------------------
REAL_CASES = [('k1', 3, 16), ('k1', 3, 80), ('motion', 3, 16), ('motion', 3, 64), ('motion', 3, 128), ('dense15', 3, 32),
              ('dense15', 3, 80), ('dense15', 1, 128), ('dense63', 3, 16), ('dense63', 3, 80), ('taps511', 3, 80),
              ('taps512', 3, 80), ('taps513', 3, 80), ('taps513', 3, 16)]


@pytest.mark.parametrize('name,C,d', REAL_CASES)
def test_real_data_within_the_summation_bound_and_adjoint(name, C, d):
    """fp32 sum of T products in any order, FMA or not: |H x - ref| <= gamma (|w| * |x|), gamma = (T + 2) u / (1 - (T + 2) u);
    residual d_r <= gamma (|w| * |v|) + u |r|; gradient |g - ref| <= gamma (|w| *T |2 r|) + |w| *T 2 d_r + u |ref|; loss
    sum (2 |r| d_r + d_r^2) + u sum (|r| + d_r)^2 (the fp32 squares)."""
    B = 3
    k = psf(name)
    op = make_op(k, C, d)
    taps = op.taps()
    T = taps[1].numel()
    gm = gamma(T)
    x, y = images(B, C, d, 30 + d)
    x[0, 0, 0, :2] = torch.tensor([1.0, -1.0])
    xd, yd = x.to(DEV), y.to(DEV)
    Hx, Htx = op.H(xd).reshape(x.shape).cpu().double(), op.Ht(xd).reshape(x.shape).cpu().double()
    bH, bHt = gm * blur_ref(x.abs(), abs_taps(taps)), gm * blur_ref(x.abs(), abs_taps(taps), transpose=True)
    eH, eHt = (Hx - blur_ref(x, taps)).abs(), (Htx - blur_ref(x, taps, transpose=True)).abs()
    share = lambda e, b: float((e / b.clamp_min(1e-300)).max())
    print(f'{name} T={T} d={d}: H {share(eH, bH):.3f} of the bound, H^T {share(eHt, bHt):.3f}')
    assert bool((eH <= bH).all()) and bool((eHt <= bHt).all())
    # adjoint: <H x, w> = <x, H^T w> in float64 from the fp32 outputs, within the two bounds
    w_img = y.double()
    Htw = op.Ht(yd).reshape(x.shape).cpu().double()
    bHtw = gm * blur_ref(y.abs(), abs_taps(taps), transpose=True)
    gap = abs(float((Hx * w_img).sum() - (x.double() * Htw).sum()))
    tol = float((bH * w_img.abs()).sum() + (x.double().abs() * bHtw).sum())
    print(f'    adjoint gap {gap:.3e} (bound {tol:.3e})')
    assert gap <= tol
    for clip in (True, False):
        l_ref, g_ref, r = data_ref(x, y, taps, clip)
        v = x.clip(-1, 1) if clip else x
        d_r = gm * blur_ref(v.abs(), abs_taps(taps)) + U * r.abs()
        bg = gm * blur_ref(2 * r.abs(), abs_taps(taps), transpose=True) + blur_ref(2 * d_r, abs_taps(taps), transpose=True) + U * g_ref.abs()
        loss, g = op.data_term(xd, yd.reshape(B, -1), clip)
        eg = (g.cpu().double() - g_ref).abs()
        if clip:
            outside = (x.abs() > 1)
            assert bool((g.cpu()[outside] == 0).all()) and bool((g.cpu()[0, 0, 0, :2] != 0).all())
        bl = ((2 * r.abs() * d_r + d_r ** 2) * (1 + U)).sum(dim=(1, 2, 3)) + U * ((r.abs() + d_r) ** 2).sum(dim=(1, 2, 3))
        el = (loss.cpu() - l_ref).abs()
        print(f'    clip={clip}: gradient {share(eg, bg):.3f} of the bound, loss {float((el / bl).max()):.3f}')
        assert bool((eg <= bg).all()) and bool((el <= bl).all())


# ---- 5. fused equals split ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,d,ec', [('motion', 80, 6), ('dense15', 32, 3), ('taps513', 128, 6), ('dense63', 16, 6)])
def test_fused_last_vjp_is_the_split_path_bit_for_bit(name, d, ec):
    import nhmc.kernels as K
    B, C = 3, 3
    op = make_op(psf(name), C, d)
    g_ = gen(50 + d)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    y = (torch.randn(B, C * d * d, generator=g_) * 0.5).to(DEV)
    ab = (1 - osched.betas_fp32()).cumprod(0)
    at = ab[torch.tensor([250, 500, 750])].float().to(DEV)                          # another DDIM step per chain
    an = torch.tensor([1.0, float(ab[250]), float(ab[500])]).to(DEV)
    cur = K.ddim_mix_fwd(x, e, at, an, final_clip=True)['xt_next']
    loss_s, g = op.data_term(cur, y, apply_clip=False)                              # the engine's path with fuse_last = False
    gx_s, ge_s = K.ddim_mix_bwd(g, x, e, at, an, final_clip=True)
    assert float(gx_s.abs().max()) > 0 and float(ge_s[:, :C].abs().max()) > 0
    for kw in (dict(xt_next=cur), dict()):
        loss_f, gx_f, ge_f = op.fused_last_vjp(x, e, at, an, y, **kw)
        assert torch.equal(loss_f, loss_s) and torch.equal(gx_f, gx_s) and torch.equal(ge_f, ge_s)
    none, gx_n, ge_n = op.fused_last_vjp(x, e, at, an, y, xt_next=cur, loss_out=K.NO_LOSS)
    assert none is None and torch.equal(gx_n, gx_s) and torch.equal(ge_n, ge_s)
    into = torch.empty(B, dtype=torch.float64, device=DEV)
    assert op.fused_last_vjp(x, e, at, an, y, loss_out=into)[0] is into and torch.equal(into, loss_s)
    buf = torch.full_like(e, 7.0)                                                   # a persistent g_e: the sigma half is not rewritten
    _, _, ge_b = op.fused_last_vjp(x, e, at, an, y, g_e_out=buf)
    assert ge_b is buf and torch.equal(buf[:, :C], ge_s[:, :C]) and bool((buf[:, C:] == 7.0).all())


# ---- 6. hygiene --------------------------------------------------------------------------------------------------
GUARD = 256                                             # elements on both sides of every written buffer


def guarded(n, dtype, value):
    full = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + n]


def intact(full, n, value):
    return bool((full[:GUARD] == value).all()) and bool((full[GUARD + n:] == value).all())


@pytest.mark.parametrize('name,d', [('motion', 80), ('dense15', 16), ('taps513', 64)])
def test_buffers_are_guarded_and_calls_reproduce(name, d):
    """Raw entries on buffers with sentinels on both sides: output, tmp, partials, g_e; two calls give the same bits."""
    import nhmc
    from nhmc import kernels as K
    lib = nhmc._lib.load()
    B, C, ec = 3, 3, 6
    op = make_op(psf(name), C, d)
    t = op._taps
    n = B * C * d * d
    g_ = gen(60 + d)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    y = (torch.randn(B, C, d, d, generator=g_) * 0.5).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    at, an = torch.full((B,), 0.52, device=DEV), torch.ones(B, device=DEV)
    tiles = K.blur2d_tiles(C, d)
    assert tiles == C * -(-d // 64) * -(-d // 32)
    P, st = (lambda v: ctypes.c_void_p(v.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        of, o = guarded(n, torch.float32, 3.0)
        for tr in (0, 1):
            assert lib.nhmc_blur2d_apply(P(x), *t.args(), tr, P(o), B, C, d, st) == 0
            torch.cuda.synchronize()
            assert intact(of, n, 3.0) and torch.equal(o.reshape(x.shape), (op.Ht if tr else op.H)(x).reshape(x.shape))
        gf, g = guarded(n, torch.float32, 3.0)
        tf, tmp = guarded(n, torch.float32, 5.0)
        wf, ws = guarded(B * tiles, torch.float64, -9.0)
        assert lib.nhmc_data_blur2d(P(x), P(y), *t.args(), 1, P(g), P(ws), P(tmp), B, C, d, st) == 0
        torch.cuda.synchronize()
        assert intact(gf, n, 3.0) and intact(tf, n, 5.0) and intact(wf, B * tiles, -9.0)
        assert bool((ws != -9.0).all()) and bool((tmp != 5.0).any())
        loss, g_py = op.data_term(x, y.reshape(B, -1), True)
        assert torch.equal(g.reshape(x.shape), g_py) and torch.equal(K.sum_partials(ws.clone(), tiles, B), loss)
        cur = K.ddim_mix_fwd(x, e, at, an, final_clip=True)['xt_next']
        gf2, g2 = guarded(n, torch.float32, 3.0)
        ef, ge = guarded(B * ec * d * d, torch.float32, 4.0)
        wf2, ws2 = guarded(B * tiles, torch.float64, -9.0)
        assert lib.nhmc_data_blur2d_vjp(P(cur), P(y), *t.args(), P(x), P(e), ec, P(at), P(an), P(g2), P(ge), 1, P(ws2), P(tmp),
                                        B, C, d, st) == 0
        torch.cuda.synchronize()
        assert intact(gf2, n, 3.0) and intact(ef, B * ec * d * d, 4.0) and intact(wf2, B * tiles, -9.0) and intact(tf, n, 5.0)
        assert bool((ge.reshape(e.shape)[:, C:] == 0).all()) and bool((ge.reshape(e.shape)[:, :C] != 4.0).all())
        runs.append([v.clone() for v in (o, g, ws, tmp, g2, ge, ws2)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_poisoned_chain_changes_no_bit_of_the_others():
    import nhmc.kernels as K
    B, C, d, ec = 3, 3, 80, 6
    op = make_op(psf('motion'), C, d)
    g_ = gen(70)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    y = (torch.randn(B, C * d * d, generator=g_) * 0.5).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    at, an = torch.full((B,), 0.52, device=DEV), torch.ones(B, device=DEV)
    clean = (op.H(x), op.Ht(x)) + tuple(op.data_term(x, y, True)) + tuple(op.fused_last_vjp(x, e, at, an, y))
    xp, yp, ep = x.clone(), y.clone(), e.clone()
    xp[1, :, ::3, ::5] = float('nan')
    xp[1, 0, 1, 1], xp[1, 1, 2, 2] = float('inf'), float('-inf')
    yp[1, ::7] = float('inf')
    ep[1, :, 5, :] = float('nan')
    bad = (op.H(xp), op.Ht(xp)) + tuple(op.data_term(xp, yp, True)) + tuple(op.fused_last_vjp(xp, ep, at, an, yp))
    for a, b in zip(clean, bad):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert not bool(torch.isfinite(b[1].double()).all())


def test_nan_reaches_exactly_its_taps_and_inf_stays_out_from_under_a_zero():
    C, d = 3, 80
    k = psf('dense15').clone()
    k[7, 7] = 0.0                                                                   # a zero entry at the centre: not a tap
    k[3, :] = 0.0
    op = make_op(k, C, d)
    off = op.taps()[0]
    x, _ = images(1, C, d, 80)
    r0, s0 = 33, 62                                                                 # near a tile seam on both axes
    xn = x.clone()
    xn[0, 1, r0, s0] = float('nan')
    for transpose in (False, True):
        got = (op.Ht if transpose else op.H)(xn.to(DEV)).reshape(x.shape).cpu()
        want = torch.zeros(C, d, d, dtype=torch.bool)
        for dy, dx in off.tolist():
            r, s = (r0 + dy, s0 + dx) if transpose else (r0 - dy, s0 - dx)          # the outputs whose tap lands on (r0, s0)
            if 0 <= r < d and 0 <= s < d:
                want[1, r, s] = True
        assert torch.equal(torch.isnan(got[0]), want)
        assert not bool(want[1, r0, s0])
    xi = x.clone()
    xi[0, 1, r0, s0] = float('inf')
    got = op.H(xi.to(DEV)).reshape(x.shape).cpu()
    clean = op.H(x.to(DEV)).reshape(x.shape).cpu()
    assert bool(torch.isfinite(got[0, 1, r0, s0])) and got[0, 1, r0, s0] == clean[0, 1, r0, s0]     # no 0 * inf = NaN
    assert bool(torch.isfinite(got[0, 1, r0 + 4, :]).all())                         # the zeroed PSF row (dy = -4): inf never arrives
    assert not bool(torch.isfinite(got[0, 1]).all())
    assert torch.equal(got[0, 0], clean[0, 0]) and torch.equal(got[0, 2], clean[0, 2])


# ---- 7. whole runs -----------------------------------------------------------------------------------------------
class ConvRef:
    """The test-local torch operator that drives the oracle: F.conv2d on the CPU."""

    def __init__(self, k, C, d):
        self.k, self.C, self.R, self.M = k[None, None].expand(C, 1, -1, -1).contiguous(), C, (k.shape[0] - 1) // 2, C * d * d

    def H(self, x):
        return F.conv2d(x, self.k.to(x.dtype), padding=self.R, groups=self.C).reshape(x.shape[0], -1)


def test_outer_loop_matches_oracle_chains_with_the_motion_blur(tiny_score):
    """tests/test_sampler_gpu.py::test_outer_loop_matches_oracle_chains with the deblur_motion operator at 16 x 16 (K = 15)."""
    from nhmc import operators, plugin, sampler
    dim, B = 16, 3
    g_ = gen(23)
    op = operators.build_operator('deblur_motion', 3, dim, torch.device(DEV), generator=g_)
    assert op.kernel.shape == (15, 15)
    ref = ConvRef(op.kernel, 3, dim)
    x = torch.randn(B, 3, dim, dim, generator=g_)
    x_orig = torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1
    y = ref.H(x_orig) + 0.1 * torch.randn(B, ref.M, generator=g_)
    P = [torch.randn(B, 3, dim, dim, generator=g_) for _ in range(64)]
    Un = [torch.rand(B, generator=g_) for _ in range(64)]
    kw = dict(epochs=3, sampling=2)
    tr = {}

    class F64Score(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = copy.deepcopy(net).double()

        def forward(self, x, t):
            return self.net(x.double(), t.double()).float()

    want = hmc_ref.hmc_chains(x, osched.betas_fp32(), SEQ, SEQ_NEXT, F64Score(tiny_score), ref, y, x_orig, tau=1.0, epsilon=0.05,
                              m=1.0, sigma_0=0.1, draw_p=lambda it: P[it], draw_u=lambda it: Un[it], trace=tr, **kw)
    algo = plugin.HMC(F64Score(tiny_score).cuda(), op, 0.1)
    opt = types.SimpleNamespace(tau=1.0, epsilon=0.05, m=1.0, sigma_0=0.1)
    res = sampler.hmc_chains(x.cuda(), osched.betas_fp32().cuda(), SEQ, SEQ_NEXT, algo, opt, y.cuda(), op, x_orig.cuda(),
                             noise=sampler.TapeNoise(lambda it: P[it], lambda it: Un[it]), collect_trace=True, **kw)
    assert res.iters == len(tr['accept'])
    for it, rec in enumerate(res.trace):
        want_acc, got_acc = tr['accept'][it], rec['accept'].numpy().astype(bool)
        margin = np.abs(Un[it].numpy() - np.minimum(1.0, np.exp(-tr['dH'][it])))
        assert np.all((want_acc == got_acc) | (margin < 1e-3)), (it, want_acc, got_acc, margin)
        assert np.array_equal(rec['epoch'].numpy(), tr['epoch'][it])
    assert res.epoch.cpu().tolist() == [7] * B
    a, b = res.samples.double().cpu(), want.double().cpu()
    assert float((a - b).abs().max() / b.abs().max()) < 1e-4


def test_whole_run_fused_split_and_graph_replay_are_the_same_bits(monkeypatch):
    from nhmc import operators, plugin, sampler
    from tests.test_graph_run_gpu import PointwiseScore, same_run
    dim, B = 32, 3
    op = operators.build_operator('deblur_motion', 3, dim, torch.device(DEV), generator=gen(5))
    assert op.kernel.shape == (31, 31)
    g_ = gen(6)
    x_orig = (torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1).to(DEV)
    y = (op.H(x_orig) + 0.1 * torch.randn(B, op.M, generator=g_).to(DEV)).contiguous()
    x = torch.randn(B, 3, dim, dim, generator=g_).to(DEV)
    algo = plugin.HMC(PointwiseScore().to(DEV), op, 0.1)
    opt = types.SimpleNamespace(tau=0.3, epsilon=0.05, m=1.0, sigma_0=0.1)
    epochs, sampling = 4, 2

    def run(**kw):
        return sampler.hmc_chains(x, osched.betas_fp32().to(DEV), SEQ, SEQ_NEXT, algo, opt, y, op, x_orig,
                                  noise=sampler.PhiloxNoise(5, 0), collect_trace=True, epochs=epochs, sampling=sampling,
                                  compact=False, **kw)
    fused = run()
    assert bool(torch.isfinite(fused.samples).all()) and fused.epoch.cpu().tolist() == [epochs + 2 * sampling] * B
    assert float(fused.samples.abs().max()) > 0
    same_run(fused, run(graph=True), epochs + 2 * sampling, every_dH=True)
    seen = []

    class SplitEngine(sampler.LeapfrogEngine):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.fuse_last = False
            seen.append(self)
    monkeypatch.setattr(sampler, 'LeapfrogEngine', SplitEngine)
    split = run()
    assert len(seen) == 1 and seen[0].fuse_last is False
    same_run(fused, split, epochs + 2 * sampling, every_dH=True)


# ---- 8. the command lines ----------------------------------------------------------------------------------------
UNET_32 = dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True, class_cond=False,
               use_checkpoint=False, attention_resolutions='16', num_heads=4, num_head_channels=16, num_heads_upsample=-1,
               use_scale_shift_norm=True, dropout=0.0, resblock_updown=True, use_fp16=False, use_new_attention_order=False,
               model_path='')


def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    import yaml
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    cfg = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True}, 'model': UNET_32,
           'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    argv = ['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'deblur_motion', '--sigma_0', '0.05', '--tau', '0.1',
            '--epsilon', '0.05', '--synthetic', '2', '--chains', '2', '--philox', '--hmc_epochs', '4', '--hmc_sampling', '2']
    # the vendor library's convolutions are reproducible only in its deterministic mode (tests/test_nonlinear_gpu.py)
    with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
        table = cli.main(argv + ['-i', str(tmp_path / 'out')])
        out = capsys.readouterr().out
        assert table.shape == (2, 3) and bool(torch.isfinite(table).all())
        assert 'image 0: PSNR' in out and 'image 1: SSIM' in out and 'Total Average PSNR' in out and 'Total Average SSIM' in out
        assert not (tmp_path / 'out' / 'blur_kernel.png').exists()
        again = cli.main(argv + ['-i', str(tmp_path / 'out2'), '--save_images'])
        assert torch.equal(table, again)                                            # same bits on a second call
    from PIL import Image
    png = np.asarray(Image.open(tmp_path / 'out2' / 'blur_kernel.png'))
    assert png.shape == (31, 31, 3) and png.min() == 0 and png.max() == 255         # min-max normalised


def test_latent_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """The latent entry: the operator acts on the decoded image, through the unfused path."""
    import yaml
    from nhmc import cli
    from tests.test_ldm_cpu import DEC_SMALL, UNET_SMALL
    cfg = {'data': {'dataset': 'tiny', 'image_size': 64, 'channels': 3, 'rescaled': True},
           'model_type': 'ffhq_latent',
           'model': {'target': 'ldm.models.diffusion.ddpm.LatentDiffusion',
                     'params': {'linear_start': 0.0015, 'linear_end': 0.0195, 'timesteps': 1000, 'image_size': 16, 'channels': 3,
                                'first_stage_key': 'image', 'cond_stage_config': '__is_unconditional__',
                                'unet_config': {'target': 'ldm.modules.diffusionmodules.openaimodel.UNetModel', 'params': UNET_SMALL},
                                'first_stage_config': {'target': 'ldm.models.autoencoder.VQModelInterface',
                                                       'params': {'embed_dim': 3, 'n_embed': 256, 'ckpt_path': 'models/first_stage_models/vq-f4/model.ckpt',
                                                                  'ddconfig': DEC_SMALL, 'lossconfig': {'target': 'torch.nn.Identity'}}}}}}
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny_latent.yml').write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    # On this random-weight latent model the leapfrog's energy error is large for every operator (inpaint_random, the
    # other latent tests' degradation, at their settings: dH of 50 ... 1600 in all 70 epochs, no sample collected, which
    # those tests allow).  dH falls with the step size as it should (measured with this operator at sigma_y = 1: 230 at
    # eps = 0.01, 5.9 at 0.0012), so the run below takes a small step and no sigma anneal (2 sigma_0 = sigma_y) and does
    # collect samples: the table is finite.
    argv = ['--dataset', 'tiny', '--algo', 'hmc_latent', '--timesteps', '3', '--deg', 'deblur_motion', '--sigma_0', '0.5', '--tau', '0.0005',
            '--epsilon', '0.0005', '--sigma_y', '1.0', '--synthetic', '2', '--chains', '2', '--philox', '--hmc_epochs', '3',
            '--hmc_sampling', '2', '-i', str(tmp_path / 'out')]
    with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
        table = cli.main_latent(argv)
        out = capsys.readouterr().out
        assert table.shape == (2, 3) and table[:, 0].tolist() == [0.0, 1.0] and bool(torch.isfinite(table).all())
        assert 'image 0: PSNR' in out and 'Total Average PSNR' in out and 'Total Average SSIM' in out
        assert torch.equal(table, cli.main_latent(argv))
    assert not (tmp_path / 'out' / 'blur_kernel.png').exists()

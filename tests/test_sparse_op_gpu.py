"""GPU: the sparse-operator kernels (csrc/sparse_op.hip) and the `ct<V>` / `sparse` degradations through the layers above.

The float64 restatement `sparse_ref` (tests/test_sparse_op_cpu.py, pinned there against the dense product and autograd) is
the reference; here it is evaluated as a float64 dense product of the densified canonical lists (`dense_of`), which
`test_dense_reference_is_the_restatement` ties to the loop.  The kernels lay the 64 lanes of a wave across the planes
P = B * C, transpose 64 x 64 tiles and read a row's entries 64 at a time, so the plane counts are 1, 9, 64, 65 and 66, the
image sizes 8, 16, 20 (n = 400: no power-of-two tiling) and 32, and the row lengths include 0, 1, 2, 63, 64, 65 and n.
"""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import hmc_ref, schedule as osched
from tests.test_sparse_op_cpu import sparse_ref

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
DEV = 'cuda'
U = 2.0 ** -24
PLANES = {1: (1, 1), 9: (3, 3), 64: (64, 1), 65: (65, 1), 66: (22, 3)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def random_csr(m, n, row_lengths, seed, dyadic=False):
    """Rows of prescribed lengths (cycled over the m rows, cut at n): distinct random columns, ascending; values N(0, 0.3^2),
    or on the grid 2^-4 with |w| <= 1/4 -> ((row_ptr, col, val), (m, n))."""
    g_ = gen(seed)
    rp, col, val = [0], [], []
    for i in range(m):
        L = min(row_lengths[i % len(row_lengths)], n)
        c = torch.sort(torch.randperm(n, generator=g_)[:L]).values
        if dyadic:
            v = torch.randint(1, 5, (L,), generator=g_).float() / 16.0 * torch.where(torch.rand(L, generator=g_) < 0.5, -1.0, 1.0)
        else:
            v = torch.randn(L, generator=g_) * 0.3
            v[v == 0] = 0.1
        col.append(c)
        val.append(v)
        rp.append(rp[-1] + L)
    return (torch.tensor(rp, dtype=torch.int32), torch.cat(col).int(), torch.cat(val).float()), (m, n)


def matrix(name, d, dyadic=False):
    """The matrices of the issue -> ((row_ptr, col, val), (m, n))."""
    from nhmc import operators
    n = d * d
    if name == 'mixed':                                 # empty rows, the wave-width seams of the entry chunks, a dense row
        return random_csr(70, n, (0, 1, 2, 63, 64, 65, n), 300 + d, dyadic)
    if name == 'tall':                                  # A^T has long rows (about 125 entries)
        return random_csr(1000, n, (1, 3, 8, 20), 310 + d, dyadic)
    if name == 'one':
        return random_csr(1, n, (n // 2,), 320 + d, dyadic)
    if name == 'perm':
        perm = torch.randperm(n, generator=gen(330 + d))
        return (torch.arange(n + 1, dtype=torch.int32), perm.int(), torch.ones(n)), (n, n)
    if name.startswith('radon'):
        a = operators.radon_matrix(d, int(name[5:]))
        val = a.values().clone()
        if dyadic:                                      # dyadic values on its pattern
            g_ = gen(340 + d)
            val = torch.randint(1, 5, val.shape, generator=g_).float() / 16.0 * torch.where(torch.rand(val.shape, generator=g_) < 0.5, -1.0, 1.0)
        return (a.crow_indices().int(), a.col_indices().int(), val), tuple(a.shape)
    raise KeyError(name)


def make_op(name, C, d, dyadic=False):
    from nhmc import operators
    triple, shape = matrix(name, d, dyadic)
    op = operators.SparseLinear(triple, C, d, DEV, shape=shape)
    assert all(torch.equal(a, b) for a, b in zip(op.csr(), triple))                 # the generator's lists are canonical
    return op


def dense_of(op):
    """The canonical list densified in float64 -> A [m, n]."""
    rp, col, val = op.csr()
    rows = torch.repeat_interleave(torch.arange(op.m), (rp[1:] - rp[:-1]).long())
    return torch.zeros(op.m, op.img_dim ** 2, dtype=torch.float64).index_put_((rows, col.long()), val.double())


def row_lengths(op, transpose=False):
    rp = op.csr(transpose)[0].long()
    return (rp[1:] - rp[:-1]).double()


def gamma(T):
    return (T + 2) * U / (1 - (T + 2) * U)


def data_ref(xt, y, A, apply_clip=True):
    """tests/test_sparse_op_cpu.py::data_ref on the dense float64 matrix: xt [B, C, n], y [B, C, m]."""
    xt, y = xt.double(), y.double()
    v = xt.clip(-1, 1) if apply_clip else xt
    r = y - v @ A.t()
    g = (-2 * r) @ A
    if apply_clip:
        g = g * ((xt >= -1) & (xt <= 1))
    return (r ** 2).sum(dim=(1, 2)), g, r


def planes(B, C, op, seed, scale=0.8):
    """-> x [B, C, n], y [B, C, m] on the host."""
    g_ = gen(seed)
    return torch.randn(B, C, op.img_dim ** 2, generator=g_) * scale, torch.randn(B, C, op.m, generator=g_) * 0.5


def dev_img(x, op):
    return x.reshape(x.shape[0], x.shape[1], op.img_dim, op.img_dim).to(DEV)


def H_of(op, x):
    return op.H(dev_img(x, op)).reshape(x.shape[0], x.shape[1], op.m).cpu()


def Ht_of(op, w):
    return op.Ht(w.reshape(w.shape[0], -1).to(DEV)).reshape(w.shape[0], w.shape[1], -1).cpu()


def data_of(op, x, y, clip):
    loss, g = op.data_term(dev_img(x, op), y.reshape(y.shape[0], -1).to(DEV), clip)
    return loss.cpu(), g.reshape(x.shape).cpu()


def test_dense_reference_is_the_restatement():
    op = make_op('mixed', 3, 8)
    A = dense_of(op)
    x, y = planes(2, 3, op, 5)
    assert torch.allclose(sparse_ref(x, op.csr()), x.double() @ A.t(), rtol=0, atol=1e-13)
    assert torch.allclose(sparse_ref(y, op.csr(), transpose=64), y.double() @ A, rtol=0, atol=1e-13)
    assert torch.allclose(sparse_ref(y, op.csr(True)), y.double() @ A, rtol=0, atol=1e-13)     # the transposed list is A^T


# ---- 1. a permutation is a pure gather -----------------------------------------------------------------------------
@pytest.mark.parametrize('P', [9, 65])
@pytest.mark.parametrize('d', [8, 16, 20, 32])
def test_permutation_is_a_pure_gather(d, P):
    """(H x)[i] = x[perm[i]] and H^T scatters back, bit for bit against indexing: catches a transposed operand, a wrong
    plane stride and every tile edge of the two transposes."""
    B, C = PLANES[P]
    op = make_op('perm', C, d)
    perm = op.csr()[1].long()
    x, _ = planes(B, C, op, 10 + d)
    assert torch.equal(H_of(op, x), x[..., perm])
    back = torch.zeros_like(x)
    back[..., perm] = x
    assert torch.equal(Ht_of(op, x), back)


# ---- 2. exactly summable data --------------------------------------------------------------------------------------
def dyadic_planes(B, C, op, seed):
    g_ = gen(seed)
    n = op.img_dim ** 2
    x = torch.randint(-3, 4, (B, C, n), generator=g_).float() / 2.0                 # {0, +-1/2, +-1, +-3/2}: the grid 2^-2 too
    x[0, 0, :4] = torch.tensor([1.0, -1.0, 1.25, -1.25])                            # on the bounds / outside them
    x[-1, -1, n - 4:] = torch.tensor([-1.25, 1.0, 1.25, -1.0])
    y = torch.randint(-64, 65, (B, C, op.m), generator=g_).float() / 32.0           # multiples of 2^-5 in [-2, 2]
    return x, y


def exactly_summable(abs_row_sum, operand, grid_bits):
    """Every partial sum of a row's sum_k val_k a_k, in any order, is a multiple of 2^-grid_bits below 2^24 of them: exact
    in fp32.  abs_row_sum: the largest sum_k |val_k| over the rows of the list in question."""
    return float(abs_row_sum) * float(operand.double().abs().max()) * 2.0 ** grid_bits < 2.0 ** 24


@pytest.mark.parametrize('P', [9, 66])
@pytest.mark.parametrize('name,d', [('mixed', 8), ('mixed', 20), ('tall', 8), ('radon6', 16)])
def test_exactly_summable_data_gives_the_restatement_bit_for_bit(name, d, P):
    B, C = PLANES[P]
    op = make_op(name, C, d, dyadic=True)
    A = dense_of(op)
    x, y = dyadic_planes(B, C, op, 20 + d)
    val = op.csr()[2]
    # the precondition, on the host: grids x 2^-2, w 2^-4, y 2^-5 -> products 2^-6 (A x, A^T x), residual 2^-6, -2 r 2^-5, its
    # products with w 2^-9
    assert bool((x * 4 == (x * 4).round()).all()) and bool((val * 16 == (val * 16).round()).all()) and bool((y * 32 == (y * 32).round()).all())
    assert float(val.abs().max()) <= 0.25
    rs, cs = A.abs().sum(1).max(), A.abs().sum(0).max()
    assert exactly_summable(rs, x, 6) and exactly_summable(cs, y, 9)
    assert torch.equal(H_of(op, x).double(), x.double() @ A.t())
    assert torch.equal(Ht_of(op, y).double(), y.double() @ A)
    for clip in (True, False):
        l_ref, g_ref, r_ref = data_ref(x, y, A, clip)
        assert exactly_summable(cs, 2 * r_ref, 9) and exactly_summable(1.0, r_ref, 6)
        loss, g = data_of(op, x, y, clip)
        assert torch.equal(g.double(), g_ref), (name, d, clip)
        rel = ((loss - l_ref).abs() / l_ref).max()
        print(f'{name} d={d} P={P} clip={clip}: loss rel err {float(rel):.2e} (bound {2.0 ** -23:.2e})')
        assert float(rel) <= 2.0 ** -23                                             # the only roundings: the fp32 squares
        if clip:
            assert bool((g[0, 0, 2:4] == 0).all())
    # the adjoint identity is exact on this data (every term a small dyadic number, float64 sums exact)
    lhs = (H_of(op, x).double() * y.double()).sum()
    rhs = (x.double() * Ht_of(op, y).double()).sum()
    assert float(lhs) == float(rhs)


# ---- 3. real-valued data against float64, derived bounds; the adjoint ------------------------------------------------
REAL_CASES = [('mixed', 8), ('mixed', 20), ('mixed', 32), ('tall', 8), ('one', 16), ('perm', 20), ('radon6', 16), ('radon7', 20)]


@pytest.mark.parametrize('P', [1, 9, 65])
@pytest.mark.parametrize('name,d', REAL_CASES)
def test_real_data_within_the_summation_bound_and_adjoint(name, d, P):
    """fp32 sum of T_i products in any order, FMA or not: |A x - ref|_i <= gamma(T_i) (|A| |x|)_i, gamma(T) = (T + 2) u /
    (1 - (T + 2) u); residual d_r <= gamma (|A| |v|) + u |r|; gradient |g - ref| <= gamma^T (|A|^T |2 r|) + |A|^T 2 d_r +
    u |ref|; loss sum (2 |r| d_r + d_r^2) + u sum (|r| + d_r)^2 (the fp32 squares) -- composed as in
    tests/test_blur2d_gpu.py::test_real_data_within_the_summation_bound_and_adjoint, with the row's own length."""
    B, C = PLANES[P]
    op = make_op(name, C, d)
    A = dense_of(op)
    Aa = A.abs()
    gm, gmt = gamma(row_lengths(op)), gamma(row_lengths(op, True))                  # [m], [n]
    x, y = planes(B, C, op, 30 + d)
    x[0, 0, :2] = torch.tensor([1.0, -1.0])
    Hx, Htw = H_of(op, x).double(), Ht_of(op, y).double()
    bH, bHt = gm * (x.double().abs() @ Aa.t()), gmt * (y.double().abs() @ Aa)
    eH, eHt = (Hx - x.double() @ A.t()).abs(), (Htw - y.double() @ A).abs()
    share = lambda e, b: float((e / b.clamp_min(1e-300)).max())
    print(f'{name} d={d} P={P}: H {share(eH, bH):.3f} of the bound, H^T {share(eHt, bHt):.3f}')
    assert bool((eH <= bH).all()) and bool((eHt <= bHt).all())
    empty = row_lengths(op) == 0
    assert bool((Hx[..., empty] == 0).all()) and not bool(torch.signbit(Hx[..., empty]).any())          # an empty row gives +0
    # adjoint: <A x, w> = <x, A^T w> in float64 from the fp32 outputs, within the two bounds
    gap = abs(float((Hx * y.double()).sum() - (x.double() * Htw).sum()))
    tol = float((bH * y.double().abs()).sum() + (x.double().abs() * bHt).sum())
    print(f'    adjoint gap {gap:.3e} (bound {tol:.3e})')
    assert gap <= tol
    for clip in (True, False):
        l_ref, g_ref, r = data_ref(x, y, A, clip)
        v = (x.clip(-1, 1) if clip else x).double()
        d_r = gm * (v.abs() @ Aa.t()) + U * r.abs()
        bg = gmt * ((2 * r.abs()) @ Aa) + (2 * d_r) @ Aa + U * g_ref.abs()
        loss, g = data_of(op, x, y, clip)
        eg = (g.double() - g_ref).abs()
        if clip:
            outside = x.abs() > 1
            assert bool((g[outside] == 0).all())
        bl = ((2 * r.abs() * d_r + d_r ** 2) * (1 + U)).sum(dim=(1, 2)) + U * ((r.abs() + d_r) ** 2).sum(dim=(1, 2))
        el = (loss - l_ref).abs()
        print(f'    clip={clip}: gradient {share(eg, bg):.3f} of the bound, loss {float((el / bl).max()):.3f}')
        assert bool((eg <= bg).all()) and bool((el <= bl).all())


# ---- 4. batch invariance -------------------------------------------------------------------------------------------
def test_a_chain_gives_the_same_bits_alone_and_inside_a_larger_batch():
    """Chain 1 of a batch of 3 (P = 9), alone (P = 3) and as chain 1 of B = 22 (P = 66); chain 21 of that batch, whose planes
    63 ... 65 straddle the wave width, alone as well."""
    C, d = 3, 20
    op = make_op('mixed', C, d)
    x, y = planes(22, C, op, 40)
    x[:, 0, :3] = torch.tensor([1.0, -1.2, 1.0])
    full = (H_of(op, x), Ht_of(op, y)) + data_of(op, x, y, True)[::-1] + data_of(op, x, y, False)[::-1]
    for sel in (slice(1, 2), slice(0, 3), slice(21, 22)):
        part = (H_of(op, x[sel]), Ht_of(op, y[sel])) + data_of(op, x[sel], y[sel], True)[::-1] + data_of(op, x[sel], y[sel], False)[::-1]
        for a, b in zip(full, part):
            assert torch.equal(a[sel], b)
    one = (H_of(op, x[1:2]), data_of(op, x[1:2], y[1:2], True))
    three = (H_of(op, x[:3]), data_of(op, x[:3], y[:3], True))
    assert torch.equal(one[0][0], three[0][1]) and torch.equal(one[1][0][0], three[1][0][1]) and torch.equal(one[1][1][0], three[1][1][1])
    # ... and does not depend on the channel count: plane (chain 1, channel 0) as a C = 1 operator
    op1 = make_op('mixed', 1, d)
    assert torch.equal(H_of(op1, x[1:2, :1]), full[0][1:2, :1]) and torch.equal(Ht_of(op1, y[1:2, :1]), full[1][1:2, :1])


# ---- 5. fused equals split -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,d,ec', [('mixed', 20, 6), ('mixed', 20, 3), ('radon6', 16, 6), ('radon6', 16, 3)])
def test_fused_last_vjp_is_the_split_path_bit_for_bit(name, d, ec):
    import nhmc.kernels as K
    B, C = 3, 3
    op = make_op(name, C, d)
    g_ = gen(50 + d)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    y = (torch.randn(B, op.M, generator=g_) * 0.5).to(DEV)
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


# ---- 6. hygiene ----------------------------------------------------------------------------------------------------
GUARD = 256                                             # elements on both sides of every written buffer


def guarded(n, dtype, value):
    full = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + n]


def intact(full, n, value):
    return bool((full[:GUARD] == value).all()) and bool((full[GUARD + n:] == value).all())


@pytest.mark.parametrize('name,d,B', [('mixed', 20, 3), ('radon6', 16, 22), ('tall', 8, 3)])
def test_buffers_are_guarded_and_calls_reproduce(name, d, B):
    """Raw entries on buffers with sentinels on both sides: output, tmp, partials, g_e; two calls give the same bits."""
    import nhmc
    from nhmc import kernels as K
    lib = nhmc._lib.load()
    C, ec = 3, 6
    op = make_op(name, C, d)
    mat = op._mat
    n_img, n_obs = B * C * d * d, B * C * op.m
    g_ = gen(60 + d)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    y = (torch.randn(B, C, op.m, generator=g_) * 0.5).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    at, an = torch.full((B,), 0.52, device=DEV), torch.ones(B, device=DEV)
    tiles = K.sparse_tiles(C, op.m)
    n_tmp = lib.nhmc_sparse_tmp_floats(B, C, op.m, d * d)
    P, st = (lambda v: ctypes.c_void_p(v.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        tf, tmp = guarded(n_tmp, torch.float32, 5.0)
        of, o = guarded(n_obs, torch.float32, 3.0)
        assert lib.nhmc_sparse_apply(P(x), *mat.args(), P(o), P(tmp), B, C, st) == 0
        torch.cuda.synchronize()
        assert intact(of, n_obs, 3.0) and intact(tf, n_tmp, 5.0) and torch.equal(o.reshape(B, -1), op.H(x))
        otf, ot = guarded(n_img, torch.float32, 3.0)
        assert lib.nhmc_sparse_apply(P(y), *mat.args(True), P(ot), P(tmp), B, C, st) == 0
        torch.cuda.synchronize()
        assert intact(otf, n_img, 3.0) and intact(tf, n_tmp, 5.0) and torch.equal(ot.reshape(B, -1), op.Ht(y.reshape(B, -1)))
        gf, g = guarded(n_img, torch.float32, 3.0)
        wf, ws = guarded(B * tiles, torch.float64, -9.0)
        assert lib.nhmc_data_sparse(P(x), P(y), *mat.both(), op.m, mat.nnz, 1, P(g), P(ws), P(tmp), B, C, d, st) == 0
        torch.cuda.synchronize()
        assert intact(gf, n_img, 3.0) and intact(tf, n_tmp, 5.0) and intact(wf, B * tiles, -9.0)
        assert bool((ws != -9.0).all()) and bool((tmp != 5.0).any())                # every partial is written
        loss, g_py = op.data_term(x, y.reshape(B, -1), True)
        assert torch.equal(g.reshape(x.shape), g_py) and torch.equal(K.sum_partials(ws.clone(), tiles, B), loss)
        cur = K.ddim_mix_fwd(x, e, at, an, final_clip=True)['xt_next']
        gf2, g2 = guarded(n_img, torch.float32, 3.0)
        ef, ge = guarded(B * ec * d * d, torch.float32, 4.0)
        wf2, ws2 = guarded(B * tiles, torch.float64, -9.0)
        assert lib.nhmc_data_sparse_vjp(P(cur), P(y), *mat.both(), op.m, mat.nnz, P(x), P(e), ec, P(at), P(an), P(g2), P(ge), 1,
                                        P(ws2), P(tmp), B, C, d, st) == 0
        torch.cuda.synchronize()
        assert intact(gf2, n_img, 3.0) and intact(ef, B * ec * d * d, 4.0) and intact(wf2, B * tiles, -9.0) and intact(tf, n_tmp, 5.0)
        assert bool((ws2 != -9.0).all())
        assert bool((ge.reshape(e.shape)[:, C:] == 0).all()) and bool((ge.reshape(e.shape)[:, :C] != 4.0).all())
        runs.append([v.clone() for v in (o, ot, g, ws, g2, ge, ws2)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 7. poison -----------------------------------------------------------------------------------------------------
def test_a_poisoned_chain_changes_no_bit_of_the_others():
    B, C, d, ec = 3, 3, 20, 6
    op = make_op('mixed', C, d)
    g_ = gen(70)
    x = (torch.randn(B, C, d, d, generator=g_) * 0.9).to(DEV)
    y = (torch.randn(B, op.M, generator=g_) * 0.5).to(DEV)
    e = torch.randn(B, ec, d, d, generator=g_).to(DEV)
    at, an = torch.full((B,), 0.52, device=DEV), torch.ones(B, device=DEV)
    clean = (op.H(x), op.Ht(y)) + tuple(op.data_term(x, y, True)) + tuple(op.fused_last_vjp(x, e, at, an, y))
    xp, yp, ep = x.clone(), y.clone(), e.clone()
    xp[1, :, ::3, ::5] = float('nan')
    xp[1, 0, 1, 1], xp[1, 1, 2, 2] = float('inf'), float('-inf')
    yp[1, ::5] = float('inf')                                                       # (every 7th row of `mixed` is empty)
    ep[1, :, 5, :] = float('nan')
    bad = (op.H(xp), op.Ht(yp)) + tuple(op.data_term(xp, yp, True)) + tuple(op.fused_last_vjp(xp, ep, at, an, yp))
    for a, b in zip(clean, bad):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert not bool(torch.isfinite(b[1].double()).all())


def test_nan_reaches_exactly_its_entries_and_inf_stays_out_from_under_a_zero():
    from nhmc import operators
    C, d = 3, 20
    n = d * d
    (rp, col, val), (m, _) = matrix('mixed', d)
    rp, col, val = rp.clone(), col.clone(), val.clone()
    early = set(col[:int(rp[3])].tolist())                                          # a column that row 3 (63 entries) is the first to read
    j0 = next(c for c in col[int(rp[3]):int(rp[4])].tolist() if c not in early)
    under = (col.long() == j0).nonzero().reshape(-1)
    rows_of = torch.repeat_interleave(torch.arange(m), (rp[1:] - rp[:-1]).long())
    hit = rows_of[under]
    assert hit.numel() >= 3
    zeroed = int(hit[0])                                                            # that row's entry on j0 becomes an explicit zero
    val[under[0]] = 0.0
    op = operators.SparseLinear((rp, col, val), C, d, DEV, shape=(m, n))
    assert op.csr()[2].numel() == val.numel() - 1                                   # a zero is not an entry
    A = dense_of(op)
    x, w = planes(2, C, op, 80)
    xn = x.clone()
    xn[1, 1, j0] = float('nan')
    want = torch.zeros(2, C, m, dtype=torch.bool)
    want[1, 1] = A[:, j0] != 0
    assert int(want.sum()) == hit.numel() - 1 and not bool(want[1, 1, zeroed])
    assert torch.equal(torch.isnan(H_of(op, xn)), want)
    i0 = 6                                                                          # the fully dense row
    wn = w.clone()
    wn[0, 2, i0] = float('nan')
    want_t = torch.zeros(2, C, n, dtype=torch.bool)
    want_t[0, 2] = A[i0] != 0
    assert bool(want_t[0, 2].all())
    assert torch.equal(torch.isnan(Ht_of(op, wn)), want_t)
    wn = w.clone()
    wn[0, 2, 1] = float('nan')                                                      # a row with one entry
    want_t[0, 2] = A[1] != 0
    assert int(want_t.sum()) == 1 and torch.equal(torch.isnan(Ht_of(op, wn)), want_t)
    xi = x.clone()
    xi[1, 1, j0] = float('inf')
    got, clean = H_of(op, xi), H_of(op, x)
    assert bool(torch.isfinite(got[1, 1, zeroed])) and got[1, 1, zeroed] == clean[1, 1, zeroed]          # no 0 * inf = NaN
    assert torch.equal(~torch.isfinite(got), want)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1, 0], clean[1, 0]) and torch.equal(got[1, 2], clean[1, 2])


# ---- 8. whole runs -------------------------------------------------------------------------------------------------
class DenseRef:
    """The test-local torch operator that drives the oracle: the dense matrix product on the CPU."""

    def __init__(self, A, C):
        self.A, self.C, self.M = A, C, C * A.shape[0]

    def H(self, x):
        return (x.reshape(x.shape[0], self.C, -1) @ self.A.to(x.dtype).t()).reshape(x.shape[0], -1)


def test_outer_loop_matches_oracle_chains_with_the_ct_operator(tiny_score):
    """tests/test_blur2d_gpu.py::test_outer_loop_matches_oracle_chains_with_the_motion_blur with ct6 at 16 x 16."""
    from nhmc import operators, plugin, sampler
    dim, B = 16, 3
    g_ = gen(23)
    op = operators.build_operator('ct6', 3, dim, torch.device(DEV))
    assert isinstance(op, operators.SparseLinear) and op.M == 3 * 162
    ref = DenseRef(dense_of(op), 3)
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
    op = operators.build_operator('ct8', 3, dim, torch.device(DEV))
    assert isinstance(op, operators.SparseLinear)
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


# ---- 9. the command lines ------------------------------------------------------------------------------------------
UNET_32 = dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True, class_cond=False,
               use_checkpoint=False, attention_resolutions='16', num_heads=4, num_head_channels=16, num_heads_upsample=-1,
               use_scale_shift_norm=True, dropout=0.0, resblock_updown=True, use_fp16=False, use_new_attention_order=False,
               model_path='')


CLI_ARGV = ['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--sigma_0', '0.05', '--tau', '0.1', '--epsilon', '0.05',
            '--synthetic', '2', '--chains', '2', '--philox', '--hmc_epochs', '4', '--hmc_sampling', '2']


def run_cli(folder, extra):
    """cli.main in `folder` (which holds configs/config_tiny.yml) -> the table."""
    import os
    from nhmc import cli
    here = os.getcwd()
    os.chdir(folder)
    try:
        # the vendor library's convolutions are reproducible only in its deterministic mode (tests/test_nonlinear_gpu.py)
        with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
            return cli.main(CLI_ARGV + extra)
    finally:
        os.chdir(here)


@pytest.fixture(scope='module')
def ct8_run(tmp_path_factory):
    """One `--deg ct8` run at 32 x 32, shared by the two command-line tests -> (folder, table)."""
    import yaml
    folder = tmp_path_factory.mktemp('ct8')
    (folder / 'configs').mkdir()
    cfg = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True}, 'model': UNET_32,
           'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}
    (folder / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(cfg))
    return folder, run_cli(folder, ['--deg', 'ct8', '-i', str(folder / 'out')])


def test_cli_end_to_end(ct8_run, capsys):
    folder, table = ct8_run
    assert table.shape == (2, 3) and bool(torch.isfinite(table).all())
    again = run_cli(folder, ['--deg', 'ct8', '-i', str(folder / 'out2')])
    out = capsys.readouterr().out
    assert 'image 0: PSNR' in out and 'image 1: SSIM' in out and 'Total Average PSNR' in out and 'Total Average SSIM' in out
    assert torch.equal(table, again)                                                # same bits on a second call


def test_cli_takes_the_operator_from_a_file(ct8_run):
    from nhmc import operators
    folder, table = ct8_run
    a = operators.radon_matrix(32, 8)
    np.savez(str(folder / 'ct8.npz'), data=a.values().numpy(), indices=a.col_indices().numpy().astype(np.int32),
             indptr=a.crow_indices().numpy().astype(np.int32), shape=np.array(a.shape, dtype=np.int64), format=np.array('csr'))
    plugged = run_cli(folder, ['--deg', 'sparse', '--operator', str(folder / 'ct8.npz'), '-i', str(folder / 'out3')])
    assert torch.equal(table, plugged)                                              # the same matrix from a file: the same bits
    with pytest.raises(SystemExit, match='no such file'):
        run_cli(folder, ['--deg', 'sparse', '--operator', str(folder / 'missing.npz'), '-i', str(folder / 'out4')])
    with pytest.raises(SystemExit, match='go together'):
        run_cli(folder, ['--deg', 'sparse', '-i', str(folder / 'out4')])


def test_latent_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """The latent entry: the operator acts on the decoded image, through the unfused path.  The small latent config and the
    step sizes of tests/test_blur2d_gpu.py::test_latent_cli_end_to_end (see the note there)."""
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
    argv = ['--dataset', 'tiny', '--algo', 'hmc_latent', '--timesteps', '3', '--deg', 'ct8', '--sigma_0', '0.5', '--tau', '0.0005',
            '--epsilon', '0.0005', '--sigma_y', '1.0', '--synthetic', '2', '--chains', '2', '--philox', '--hmc_epochs', '3',
            '--hmc_sampling', '2', '-i', str(tmp_path / 'out')]
    with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
        table = cli.main_latent(argv)
        out = capsys.readouterr().out
        assert table.shape == (2, 3) and table[:, 0].tolist() == [0.0, 1.0] and bool(torch.isfinite(table).all())
        assert 'image 0: PSNR' in out and 'Total Average PSNR' in out and 'Total Average SSIM' in out

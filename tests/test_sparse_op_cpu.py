"""CPU: sparse linear operators (operators.SparseLinear, --deg ct<V>, --deg sparse --operator) -- the float64 restatement
of the definition in include/nhmc.h, the canonical CSR pair, the parallel-beam matrix, the operator class, the C-ABI surface,
both parsers and the npz loader."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('nhmc_sparse_check', 'nhmc_sparse_tiles', 'nhmc_sparse_tmp_floats', 'nhmc_sparse_apply', 'nhmc_data_sparse',
           'nhmc_data_sparse_vjp')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sparse_ref(x, csr, transpose=False):
    """The definition, as a loop over the lists, in float64.  csr = (row_ptr, col, val) of A [m, n]; x [..., n] -> [..., m],
    or with transpose x [..., m] -> [..., n] (the scatter form of the same entries)."""
    rp, col, val = (t.tolist() for t in csr)
    m = len(rp) - 1
    x = x.double()
    if not transpose:
        out = torch.zeros(*x.shape[:-1], m, dtype=torch.float64)
        for i in range(m):
            for k in range(rp[i], rp[i + 1]):
                out[..., i] += val[k] * x[..., col[k]]
        return out
    n = transpose
    out = torch.zeros(*x.shape[:-1], n, dtype=torch.float64)
    for i in range(m):
        for k in range(rp[i], rp[i + 1]):
            out[..., col[k]] += val[k] * x[..., i]
    return out


def data_ref(xt, y, csr, apply_clip=True):
    """Loss per chain and autograd's gradient from the definition, in float64: g = A^T(-2 r) 1[|xt| <= 1].
    xt [B, C, n], y [B, C, m]."""
    xt, y = xt.double(), y.double()
    v = xt.clip(-1, 1) if apply_clip else xt
    r = y - sparse_ref(v, csr)
    g = sparse_ref(-2 * r, csr, transpose=xt.shape[-1])
    if apply_clip:
        g = g * ((xt >= -1) & (xt <= 1))
    return (r ** 2).sum(dim=(1, 2)), g, r


def random_dense(m, n, g_, density=0.3):
    a = torch.randn(m, n, generator=g_, dtype=torch.float64)
    a[torch.rand(m, n, generator=g_) > density] = 0
    a[0, n - 1] = 0.5                                                               # asymmetric: a transposition would show
    return a


def csr_of_dense(a):
    m, n = a.shape
    rp, col, val = [0], [], []
    for i in range(m):
        for j in range(n):
            if float(a[i, j]) != 0.0:
                col.append(j)
                val.append(float(a[i, j]))
        rp.append(len(col))
    return torch.tensor(rp), torch.tensor(col, dtype=torch.int64), torch.tensor(val, dtype=torch.float64)


def densify(csr, m, n):
    rp, col, val = (t.tolist() for t in csr)
    a = torch.zeros(m, n, dtype=torch.float64)
    for i in range(m):
        for k in range(rp[i], rp[i + 1]):
            a[i, col[k]] += val[k]
    return a


@pytest.mark.parametrize('m', [1, 5, 70])
def test_restatement_is_the_dense_product_and_its_autograd(m):
    """Pins the convention: rows of A index the observation, the clamp mask inside or ON the bounds."""
    d = 8
    n = d * d
    g_ = gen(200 + m)
    a = random_dense(m, n, g_)
    csr = csr_of_dense(a)
    x = torch.randn(2, 3, n, generator=g_, dtype=torch.float64) * 0.8
    x[0, 0, :4] = torch.tensor([1.0, -1.0, 1.25, -1.25], dtype=torch.float64)       # on the bounds: gradient; outside: none
    a[:, :4] = torch.randn(m, 4, generator=g_, dtype=torch.float64)                 # every row sees those four pixels
    csr = csr_of_dense(a)
    y = torch.randn(2, 3, m, generator=g_, dtype=torch.float64)
    assert torch.allclose(sparse_ref(x, csr), x @ a.t(), rtol=0, atol=1e-12)
    assert torch.allclose(sparse_ref(y, csr, transpose=n), y @ a, rtol=0, atol=1e-12)
    for clip in (True, False):
        leaf = x.clone().requires_grad_(True)
        v = leaf.clip(-1, 1) if clip else leaf
        loss = ((y - v @ a.t()) ** 2).sum()
        (ga,) = torch.autograd.grad(loss, leaf)
        l, g, _ = data_ref(x, y, csr, clip)
        assert abs(float(l.sum() - loss.detach())) <= 1e-12 * float(loss.detach()) and torch.allclose(g, ga, rtol=0, atol=1e-11)
        if clip:
            assert bool((ga[0, 0, 2:4] == 0).all()) and bool((g[0, 0, 2:4] == 0).all())
            assert bool((ga[0, 0, :2] != 0).all()) and bool((g[0, 0, :2] != 0).all())


def test_canonicalisation():
    from nhmc import operators
    # unsorted, with duplicates, an explicit zero, and an entry that is 0 in fp32
    rows = torch.tensor([2, 0, 2, 1, 0, 2, 1, 0])
    cols = torch.tensor([5, 3, 1, 0, 3, 5, 7, 9])
    vals = torch.tensor([1.0, 2.0, -3.0, 0.0, 0.5, 0.25, 1e-60, 4.0], dtype=torch.float64)
    m, d = 4, 4
    n = d * d
    coo = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, size=(m, n))
    op = operators.SparseLinear(coo, 3, d, 'cpu')
    rp, col, val = op.csr()
    assert rp.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert rp.tolist() == [0, 2, 2, 4, 4]                                           # rows 1 and 3 are empty: zeros are no entries
    assert col.tolist() == [3, 9, 1, 5] and val.tolist() == [2.5, 4.0, -3.0, 1.25]
    # the same matrix through every input form
    dense = torch.zeros(m, n, dtype=torch.float64).index_put_((rows, cols), vals, accumulate=True)
    forms = [dense.to_sparse(), dense.to_sparse_csr(), dense.float().to_sparse_csr()]
    crow = torch.tensor([0, 3, 5, 8])                                               # triple with unsorted columns and duplicates
    order = torch.argsort(rows, stable=True)
    forms_triple = ((crow.tolist() + [8], cols[order], vals[order]), (m, n))
    got = [operators.SparseLinear(f, 3, d, 'cpu').csr() for f in forms]
    got.append(operators.SparseLinear(forms_triple[0], 3, d, 'cpu', shape=forms_triple[1]).csr())
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is not None:
        s = sp.coo_matrix((vals.numpy(), (rows.numpy(), cols.numpy())), shape=(m, n))
        got += [operators.SparseLinear(s, 3, d, 'cpu').csr(), operators.SparseLinear(s.tocsr(), 3, d, 'cpu').csr(),
                operators.SparseLinear(s.tocsc(), 3, d, 'cpu').csr()]
    for lists in got:
        assert all(torch.equal(a, b) for a, b in zip(lists, (rp, col, val)))

    class Duck:                                                                     # scipy's surface, without scipy
        shape = (m, n)

        def tocoo(self):
            class Coo:
                row, col, data, shape = rows.numpy(), cols.numpy(), vals.numpy(), (m, n)
            return Coo()
    assert all(torch.equal(a, b) for a, b in zip(operators.SparseLinear(Duck(), 3, d, 'cpu').csr(), (rp, col, val)))
    # the transposed list: A^T exactly, rows of A ascending within its rows
    g_ = gen(9)
    a = random_dense(70, 64, g_).float()
    op = operators.SparseLinear(a.to_sparse(), 1, 8, 'cpu')
    assert torch.equal(densify(op.csr(), 70, 64), a.double())
    t = op.csr(transpose=True)
    assert t[0].numel() == 65 and torch.equal(densify(t, 64, 70), a.double().t())
    trp, tcol, _ = (v.tolist() for v in t)
    for j in range(64):
        seg = tcol[trp[j]:trp[j + 1]]
        assert seg == sorted(seg) and len(set(seg)) == len(seg)
    frp, fcol, _ = (v.tolist() for v in op.csr())
    for i in range(70):
        seg = fcol[frp[i]:frp[i + 1]]
        assert seg == sorted(seg) and len(set(seg)) == len(seg)


def radon_ref(d, V):
    """The construction restated as a float64 loop -> dense [V D, d^2] float64 of the fp32 weights."""
    D = 2 * math.ceil(d / math.sqrt(2)) + 3
    c = (d - 1) / 2
    a = torch.zeros(V * D, d * d, dtype=torch.float64)
    for v in range(V):
        th = math.pi * v / V
        for r in range(d):
            for s in range(d):
                u = (s - c) * math.cos(th) + (c - r) * math.sin(th) + (D - 1) / 2
                i0 = math.floor(u)
                f = u - i0
                assert 0 <= i0 and i0 + 1 < D
                a[v * D + i0, r * d + s] += float(np.float32((1 - f) / d))
                a[v * D + i0 + 1, r * d + s] += float(np.float32(f / d))
    return a, D


@pytest.mark.parametrize('d,V', [(8, 4), (20, 7), (16, 6)])
def test_radon_matrix(d, V):
    from nhmc import operators
    a = operators.radon_matrix(d, V)
    assert a.layout == torch.sparse_csr and a.dtype == torch.float32
    ref, D = radon_ref(d, V)
    assert tuple(a.shape) == (V * D, d * d)
    crow, col, val = a.crow_indices(), a.col_indices(), a.values()
    assert int(col.min()) >= 0 and int(col.max()) < d * d and int(crow[-1]) == val.numel()
    dense = a.to_dense().double()
    assert torch.allclose(dense, ref, rtol=0, atol=2.0 ** -24 / d)                  # cos / sin of torch against math: an ulp of u
    # the float64 weights: every column sums to V / d, view 0 of the all-ones image sums to d
    op = operators.SparseLinear(a, 1, d, 'cpu')
    assert all(torch.equal(x, y) for x, y in zip(op.csr(), (crow.int(), col.int(), val)))      # already canonical
    c = (d - 1) / 2
    colsum = torch.zeros(d * d, dtype=torch.float64)
    view0 = 0.0
    for v in range(V):
        th = math.pi * v / V
        for r in range(d):
            for s in range(d):
                u = (s - c) * math.cos(th) + (c - r) * math.sin(th) + (D - 1) / 2
                f = u - math.floor(u)
                colsum[r * d + s] += (1 - f) / d + f / d
                if v == 0:
                    view0 += (1 - f) + f
    assert float((colsum - V / d).abs().max()) <= 1e-12 and abs(view0 - d * d) <= 1e-9
    assert float((dense.sum(0) - V / d).abs().max()) <= 2 * V * 2.0 ** -24 / d + 1e-12         # the fp32 roundings of 2 V weights
    assert abs(float(dense[:D].sum()) * d - d * d) <= 1e-3                                      # view 0 of ones: d per image row
    b = operators.radon_matrix(d, V)
    assert torch.equal(b.crow_indices(), crow) and torch.equal(b.col_indices(), col) and torch.equal(b.values(), val)
    if (d, V) == (16, 6):
        cnt = crow[1:] - crow[:-1]
        assert (D, V * D, val.numel(), int((cnt == 0).sum()), int(cnt.max())) == (27, 162, 3072, 36, 37)


def test_build_operator_serves_ct():
    from nhmc import operators
    from nhmc._lib import NhmcError
    op = operators.build_operator('ct6', 3, 16, 'cpu')
    assert isinstance(op, operators.SparseLinear) and op.M == 3 * 162 and op.is_linear() is True
    params = inspect.signature(op.fused_last_vjp).parameters
    assert list(params)[:5] == ['xt_in', 'e', 'at', 'at_next', 'y'] and 'g_e_out' in params and 'loss_out' in params
    assert 'xt_next' in params and op.fused_wants_decode is True
    assert list(inspect.signature(op.data_term).parameters) == ['xt', 'y', 'apply_clip', 'loss_out']
    with pytest.raises(NotImplementedError):
        op.H_pinv(torch.zeros(1, op.M))
    with pytest.raises(NhmcError):                                                  # no kernel, no result on the CPU
        op.H(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NhmcError):
        op.Ht(torch.zeros(1, op.M))
    with pytest.raises(NhmcError):
        op.data_term(torch.zeros(1, 3, 16, 16), torch.zeros(1, op.M))
    with pytest.raises(NotImplementedError):
        operators.build_operator('deblur_nonlinear', 3, 64, 'cpu')                  # unchanged
    with pytest.raises(NotImplementedError):
        operators.build_operator('ctx', 3, 16, 'cpu')
    assert isinstance(operators.build_operator('cs4', 3, 16, 'cpu', generator=gen(1)), operators.WalshHadamardCS)
    assert isinstance(operators.build_operator('color', 3, 16, 'cpu'), operators.Colorization)


def test_constructor_validation():
    from nhmc import operators
    from nhmc._lib import NhmcError
    good = torch.eye(16).to_sparse()
    assert operators.SparseLinear(good, 3, 4, 'cpu').M == 3 * 16
    with pytest.raises(NhmcError):
        operators.SparseLinear(good, 3, 8, 'cpu')                                   # 16 columns, 64 pixels
    with pytest.raises(NhmcError):
        operators.SparseLinear(torch.eye(36).to_sparse(), 3, 6, 'cpu')              # img_dim % 4
    with pytest.raises(NhmcError):
        operators.SparseLinear(torch.zeros(0, 16).to_sparse(), 3, 4, 'cpu')         # m = 0
    with pytest.raises(NhmcError):
        operators.SparseLinear(([0], [], []), 3, 4, 'cpu', shape=(0, 16))
    with pytest.raises(NhmcError):
        operators.SparseLinear(torch.zeros(3, 16).to_sparse(), 3, 4, 'cpu')         # no entry
    with pytest.raises(NhmcError):
        operators.SparseLinear(([0, 1, 2], [3, 16], [1.0, 1.0]), 3, 4, 'cpu', shape=(2, 16))     # a column out of range
    with pytest.raises(NhmcError):
        operators.SparseLinear(([0, 1, 2], [3, -1], [1.0, 1.0]), 3, 4, 'cpu', shape=(2, 16))
    with pytest.raises(NhmcError):
        operators.SparseLinear(([0, 2, 1, 3], [3, 4, 5], [1.0, 1.0, 1.0]), 3, 4, 'cpu', shape=(3, 16))    # not monotone
    with pytest.raises(NhmcError):
        operators.SparseLinear(([0, 1, 2], [3, 4], [1.0, 1.0]), 3, 4, 'cpu')        # the triple needs shape=
    with pytest.raises(NhmcError):
        operators.SparseLinear(torch.eye(16), 3, 4, 'cpu')                          # a dense tensor is not a sparse operator
    assert operators.SparseLinear(([0, 1, 2], [3, 4], [1.0, 1.0]), 3, 4, 'cpu', shape=(2, 16)).M == 6


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    assert re.search(r'#define NHMC_ABI_VERSION 2\b', src)                          # additive change
    assert 'a zero is not an entry' in src and 'inf' in src                         # the non-finite rule is stated
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    names = set(re.findall(r'\b(nhmc_[A-Za-z0-9_]+)\s*\(', src))
    import nhmc
    lib = nhmc._lib.load()
    for name in SYMBOLS:
        assert name in names and name in nhmc._lib.SIGNATURES and hasattr(lib, name), name


def test_argument_validation_of_the_entry_points():
    import ctypes
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4, b16, c16 = P(0), P(0x1000), P(0x1004), P(0x2000), P(0x3000)
    apply = lambda x=a16, rp=a16, col=a16, val=a16, rows=5, cols=64, nnz=7, out=b16, tmp=c16, B=1, C=3: \
        lib.nhmc_sparse_apply(x, rp, col, val, rows, cols, nnz, out, tmp, B, C, null)
    assert apply(x=null) == 1 and apply(rp=null) == 1 and apply(col=null) == 1 and apply(val=null) == 1
    assert apply(out=null) == 1 and apply(tmp=null) == 1 and apply(out=a16) == 1
    assert apply(x=a4) == 2 and apply(out=P(0x2004)) == 2 and apply(tmp=P(0x3008)) == 2 and apply(col=P(0x1002)) == 2
    assert apply(nnz=0) == 3 and apply(rows=0) == 3 and apply(cols=0) == 3 and apply(B=70000) == 3 and apply(B=0) == 3
    data = lambda xt=a16, y=a16, rp=a16, trp=a16, m=5, nnz=7, g=b16, ws=a16, tmp=c16, B=1, C=3, dim=8: \
        lib.nhmc_data_sparse(xt, y, rp, a16, a16, trp, a16, a16, m, nnz, 1, g, ws, tmp, B, C, dim, null)
    assert data(xt=null) == 1 and data(y=null) == 1 and data(rp=null) == 1 and data(trp=null) == 1 and data(g=null) == 1
    assert data(ws=null) == 1 and data(tmp=null) == 1 and data(tmp=b16) == 1
    assert data(y=a4) == 2 and data(dim=10) == 2 and data(dim=18) == 2
    assert data(nnz=0) == 3 and data(m=0) == 3 and data(B=65536) == 3 and data(dim=0) == 3
    vjp = lambda **kw: lib.nhmc_data_sparse_vjp(a16, a16, a16, a16, a16, a16, a16, a16, kw.get('m', 5), kw.get('nnz', 7),
                                                P(0x4000), a16, kw.get('ec', 6), a16, a16, b16, kw.get('ge', P(0x5000)), 0,
                                                a16, c16, kw.get('B', 1), 3, kw.get('dim', 8), null)
    assert vjp(ec=5) == 3 and vjp(ge=null) == 1 and vjp(nnz=0) == 3 and vjp(dim=18) == 2 and vjp(B=70000) == 3
    assert vjp(ge=P(0x5004)) == 2
    assert lib.nhmc_sparse_tiles(3, 162) == 3 * lib.nhmc_sparse_tiles(1, 162) and lib.nhmc_sparse_tiles(1, 1) == 1
    assert lib.nhmc_sparse_tmp_floats(2, 3, 162, 256) >= 2 * 3 * (162 + 256)
    # the host copy of a list
    rp = (ctypes.c_int32 * 4)(0, 2, 2, 3)
    col = (ctypes.c_int32 * 3)(0, 15, 7)
    chk = lambda m=3, n=16, nnz=3: lib.nhmc_sparse_check(rp, col, m, n, nnz)
    assert chk() == 0
    assert lib.nhmc_sparse_check(null, col, 3, 16, 3) == 1 and lib.nhmc_sparse_check(rp, null, 3, 16, 3) == 1
    rp[0] = 1
    assert chk() == 3                                                               # row_ptr[0] != 0
    rp[0], rp[1], rp[2] = 0, 2, 1
    assert chk() == 3                                                               # decreasing
    rp[2] = 2
    assert chk(nnz=2) == 3                                                          # row_ptr[m] != nnz
    col[1] = 16
    assert chk() == 3                                                               # col = n
    col[1] = -1
    assert chk() == 3
    col[1] = 15
    assert chk() == 0 and chk(m=0) == 3 and chk(nnz=0) == 3


def test_parsers_and_the_npz_loader(tmp_path):
    from nhmc import cli, operators
    from nhmc._lib import NhmcError
    for latent in (False, True):
        parser = cli.get_parser(latent=latent)
        opt, _ = parser.parse_known_args(['--deg', 'ct30', '--dataset', 'tiny', '--sigma_0', '0.05'])
        assert opt.deg == 'ct30' and opt.operator is None
        opt, _ = parser.parse_known_args(['--deg', 'sparse', '--operator', 'a.npz', '--dataset', 'tiny', '--sigma_0', '0.05'])
        assert opt.deg == 'sparse' and opt.operator == 'a.npz'
    a = operators.radon_matrix(16, 6)
    path = str(tmp_path / 'ct6.npz')
    np.savez(path, data=a.values().numpy(), indices=a.col_indices().numpy().astype(np.int32),
             indptr=a.crow_indices().numpy().astype(np.int32), shape=np.array(a.shape, dtype=np.int64), format=np.array('csr'))
    triple, shape = operators.load_sparse_npz(path)
    assert shape == (162, 256)
    want = operators.build_operator('ct6', 3, 16, 'cpu').csr()
    got = operators.build_operator('sparse', 3, 16, 'cpu', operator_file=path)
    assert isinstance(got, operators.SparseLinear) and all(torch.equal(x, y) for x, y in zip(got.csr(), want))
    assert all(torch.equal(x, y) for x, y in zip(got.csr(transpose=True), operators.build_operator('ct6', 3, 16, 'cpu').csr(True)))
    with pytest.raises(NhmcError, match='columns'):
        operators.build_operator('sparse', 3, 32, 'cpu', operator_file=path)        # 256 columns, 1024 pixels
    with pytest.raises(NhmcError, match='no such file'):
        operators.build_operator('sparse', 3, 16, 'cpu', operator_file=str(tmp_path / 'missing.npz'))
    with pytest.raises(NhmcError, match='--operator'):
        operators.build_operator('sparse', 3, 16, 'cpu')
    csc = str(tmp_path / 'csc.npz')
    np.savez(csc, data=a.values().numpy(), indices=a.col_indices().numpy(), indptr=a.crow_indices().numpy(),
             shape=np.array(a.shape), format=np.array('csc'))
    with pytest.raises(NhmcError, match='csc'):
        operators.load_sparse_npz(csc)
    other = str(tmp_path / 'other.npz')
    np.savez(other, weights=np.zeros(3))
    with pytest.raises(NhmcError, match='lacks'):
        operators.load_sparse_npz(other)
    text = tmp_path / 'text.npz'
    text.write_text('not an archive')
    with pytest.raises(NhmcError, match='not an .npz'):
        operators.load_sparse_npz(str(text))

"""CPU: the host side of the Fourier-sampling operator (`--deg mri<R>`, `--deg fourier --kspace_mask FILE.npy`): the
Cartesian mask, the mask-file loader, build_operator's routing and the float64 factors against torch.fft.  The oracle,
here and in tests/test_fourier_gpu.py, is the centred orthonormal 2-D FFT in float64.
"""
import numpy as np
import pytest
import torch


def fft2c(x):
    """Centred orthonormal 2-D DFT of the last two axes (DC at [d/2, d/2]), complex128."""
    x = torch.fft.ifftshift(x.to(torch.complex128), dim=(-2, -1))
    return torch.fft.fftshift(torch.fft.fft2(x, norm='ortho'), dim=(-2, -1))


def ifft2c(k):
    k = torch.fft.ifftshift(k.to(torch.complex128), dim=(-2, -1))
    return torch.fft.fftshift(torch.fft.ifft2(k, norm='ortho'), dim=(-2, -1))


class FourierRef:
    """The float64 oracle operator: H(x) = [W o Re fft2c(x) ; W o Im fft2c(x)] -> [B, M] in x's dtype (computed in float64,
    rounded once; differentiable), Ht its adjoint."""

    def __init__(self, weights, channels, dim):
        self.W = torch.as_tensor(weights).double()
        self.channels, self.dim, self.M = channels, dim, 2 * channels * dim * dim

    def planes(self, x):
        Y = fft2c(x.reshape(x.shape[0], self.channels, self.dim, self.dim).double())
        return torch.stack([self.W * Y.real, self.W * Y.imag], dim=2)               # [B, C, 2, d, d] float64

    def H(self, x):
        return self.planes(x).reshape(x.shape[0], -1).to(x.dtype)

    def Ht(self, v):
        v = v.reshape(v.shape[0], self.channels, 2, self.dim, self.dim).double()
        return ifft2c(self.W * torch.complex(v[:, :, 0], v[:, :, 1])).real.reshape(v.shape[0], -1)


@pytest.mark.parametrize('d', [32, 64, 256])
@pytest.mark.parametrize('R', [2, 4, 8])
def test_cartesian_mask_columns_and_central_block(d, R):
    from nhmc import operators
    m = operators.cartesian_mask(d, R, torch.Generator().manual_seed(d + R))
    assert m.shape == (d, d) and m.dtype == torch.float32
    assert bool(((m == 0) | (m == 1)).all()) and torch.equal(m, m[:1].expand(d, d))   # whole columns
    cols = m[0]
    keep = d // R
    c = min(keep, max(1, int(0.32 * d / R + 0.5)))
    assert int(cols.sum()) == keep
    lo = d // 2 - c // 2
    assert bool((cols[lo:lo + c] == 1).all())
    assert cols[d // 2] == 1                                                          # DC is measured
    # the rest: the first keep - c entries of randperm over the remaining columns in ascending order
    rest = torch.tensor([j for j in range(d) if not lo <= j < lo + c])
    want = torch.zeros(d)
    want[lo:lo + c] = 1
    want[rest[torch.randperm(d - c, generator=torch.Generator().manual_seed(d + R))[:keep - c]]] = 1
    assert torch.equal(cols, want)


def test_cartesian_mask_counts_stated_in_the_definition():
    from nhmc import operators
    for d, R, keep, c in ((256, 2, 128, 41), (256, 4, 64, 20), (256, 8, 32, 10), (32, 8, 4, 1)):
        cols = operators.cartesian_mask(d, R, torch.Generator().manual_seed(0))[0]
        assert int(cols.sum()) == keep
        assert min(keep, max(1, int(0.32 * d / R + 0.5))) == c
        assert bool((cols[d // 2 - c // 2: d // 2 - c // 2 + c] == 1).all())
    assert torch.equal(operators.cartesian_mask(32, 1), torch.ones(32, 32))           # R = 1 keeps everything
    for bad in ((32, 0), (32, 33), (0, 1)):
        with pytest.raises(operators.NhmcError):
            operators.cartesian_mask(*bad)


def test_cartesian_mask_is_deterministic_under_a_seed():
    from nhmc import operators
    a = operators.cartesian_mask(64, 4, torch.Generator().manual_seed(7))
    b = operators.cartesian_mask(64, 4, torch.Generator().manual_seed(7))
    c = operators.cartesian_mask(64, 4, torch.Generator().manual_seed(8))
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(11)                                                             # generator=None: the global RNG
    d1 = operators.cartesian_mask(64, 4)
    torch.manual_seed(11)
    assert torch.equal(d1, operators.cartesian_mask(64, 4))


def test_build_operator_routes():
    from nhmc import operators
    op = operators.build_operator('mri4', 3, 32, 'cpu')
    assert isinstance(op, operators.FourierSampling) and op.M == 6144 and op.is_linear()
    assert int(op.weights[0].sum()) == 8
    with pytest.raises(NotImplementedError):
        op.H_pinv(torch.zeros(1, op.M))
    with pytest.raises(NotImplementedError):
        operators.build_operator('deblur_nonlinear', 3, 32, 'cpu')
    for deg in ('mri0', 'mri33'):
        with pytest.raises(operators.NhmcError):
            operators.build_operator(deg, 3, 32, 'cpu')
    with pytest.raises(operators.NhmcError, match='kspace_mask'):
        operators.build_operator('fourier', 3, 32, 'cpu')
    with pytest.raises(operators.NhmcError, match='32'):
        operators.FourierSampling(torch.ones(48, 48), 3, 48, 'cpu')


def test_weights_are_checked():
    from nhmc import operators
    ok = torch.rand(32, 32)
    op = operators.FourierSampling(ok, 3, 32, 'cpu')
    assert torch.equal(op.weights, ok) and op.factors.numel() == 6 * 32 * 32
    assert operators.FourierSampling(ok.numpy() > 0.5, 1, 32, 'cpu').weights.dtype == torch.float32   # a boolean mask
    for bad in (torch.zeros(32, 32), -ok, ok.clone().index_put_((torch.tensor(3), torch.tensor(4)), torch.tensor(float('nan'))),
                ok.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(float('inf'))), torch.ones(32), torch.ones(32, 64),
                torch.ones(1, 32, 32), torch.ones(32, 32, dtype=torch.complex64)):
        with pytest.raises(operators.NhmcError):
            operators.FourierSampling(bad, 3, 32, 'cpu')


def test_mask_file_loader(tmp_path):
    from nhmc import operators
    good = np.random.default_rng(0).random((32, 32))
    np.save(tmp_path / 'good.npy', good)
    w = operators.load_kspace_mask(str(tmp_path / 'good.npy'), 32)
    assert w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(good.astype(np.float32)))
    np.save(tmp_path / 'bool.npy', good > 0.5)
    assert torch.equal(operators.load_kspace_mask(str(tmp_path / 'bool.npy'), 32), torch.from_numpy((good > 0.5).astype(np.float32)))
    op = operators.build_operator('fourier', 3, 32, 'cpu', kspace_mask_file=str(tmp_path / 'good.npy'))
    assert isinstance(op, operators.FourierSampling) and op.M == 6144 and torch.equal(op.weights, w)

    nan = good.copy()
    nan[1, 2] = np.nan
    cases = {'rank1.npy': np.ones(32), 'rank3.npy': np.ones((1, 32, 32)), 'size.npy': np.ones((64, 64)), 'rect.npy': np.ones((32, 64)),
             'neg.npy': -good, 'nan.npy': nan, 'zero.npy': np.zeros((32, 32)), 'complex.npy': good + 1j, 'text.npy': np.full((32, 32), 'a')}
    for name, arr in cases.items():
        np.save(tmp_path / name, arr)
        with pytest.raises(operators.NhmcError, match='kspace_mask'):
            operators.load_kspace_mask(str(tmp_path / name), 32)
    with pytest.raises(operators.NhmcError, match='no such file'):
        operators.load_kspace_mask(str(tmp_path / 'absent.npy'), 32)
    (tmp_path / 'junk.npy').write_bytes(b'not an array')
    with pytest.raises(operators.NhmcError, match='not a .npy'):
        operators.load_kspace_mask(str(tmp_path / 'junk.npy'), 32)
    np.save(tmp_path / 'object.npy', np.array([[{}] * 32] * 32, dtype=object), allow_pickle=True)
    with pytest.raises(operators.NhmcError):                                          # a pickle is never loaded
        operators.load_kspace_mask(str(tmp_path / 'object.npy'), 32)
    np.savez(tmp_path / 'archive.npz', w=good)
    with pytest.raises(operators.NhmcError):
        operators.load_kspace_mask(str(tmp_path / 'archive.npz'), 32)


@pytest.mark.parametrize('d', [32, 96])
def test_host_factors_reproduce_fft2c(d):
    """F X F^T with F = Cm + i Sm is the centred orthonormal 2-D FFT, and the operator's adjoint formula is its adjoint."""
    from nhmc import operators
    g = torch.Generator().manual_seed(d)
    W = torch.rand(d, d, generator=g).double() * (torch.rand(d, d, generator=g) > 0.4)
    op = operators.FourierSampling(W, 2, d, 'cpu')
    assert op.Cm.dtype == torch.float64
    F = torch.complex(op.Cm, op.Sm)
    X = torch.randn(3, 2, d, d, generator=g, dtype=torch.float64)
    Y = F @ X.to(torch.complex128) @ F.t()
    want = fft2c(X)
    assert float((Y - want).abs().max()) < 1e-12 * max(1.0, float(want.abs().max()))
    assert float((F.conj().t() @ F - torch.eye(d)).abs().max()) < 1e-12               # unitary
    # Ht(v) = Re[F^H (W o v) conj(F)] is the adjoint of the oracle's H, and the oracle's Ht says the same
    ref = FourierRef(op.weights, 2, d)
    v = torch.randn(3, ref.M, generator=g, dtype=torch.float64)
    vc = torch.complex(*v.reshape(3, 2, 2, d, d).unbind(2))
    ht = (F.conj().t() @ (op.weights.double() * vc) @ F.conj()).real.reshape(3, -1)
    assert float((ht - ref.Ht(v)).abs().max()) < 1e-12 * float(ht.abs().max())
    lhs, rhs = float((ref.H(X) * v).sum()), float((X.reshape(3, -1) * ht).sum())
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)

"""CPU: the host side of the modulated Fourier operator (`--deg mcmri<R>`, `--deg cdp<K>`): the coil maps, the diffraction
masks, the map-file loader, build_operator's routing, the constructor's refusals and the float64 oracle of
tests/test_modfourier_gpu.py -- the centred orthonormal 2-D FFT of the image times each complex map, in float64.
"""
import os

import numpy as np
import pytest
import torch

from tests.test_fourier_cpu import FourierRef, fft2c, ifft2c


class ModFourierRef:
    """The float64 oracle operator: Y_{c,k} = fft2c(S_k o x_c);  linear: H(x) = [W o Re Y ; W o Im Y] [B, C, K, 2, d, d],
    modulus: H(x) = W o |Y| [B, C, K, d, d]; -> [B, M] in x's dtype (computed in float64, rounded once; differentiable).
    Ht: the adjoint of the linear form."""

    def __init__(self, maps, channels, dim, weights=None, modulus=False):
        self.S = torch.as_tensor(maps).to(torch.complex128)
        self.W = torch.ones(dim, dim, dtype=torch.float64) if weights is None else torch.as_tensor(weights).double()
        self.channels, self.dim, self.K, self.modulus = channels, dim, self.S.shape[0], modulus
        self.M = (1 if modulus else 2) * channels * self.K * dim * dim

    def spectrum(self, x):
        x = x.reshape(x.shape[0], self.channels, 1, self.dim, self.dim).double()
        return fft2c(self.S * x)                                                        # [B, C, K, d, d] complex128

    def planes(self, x):
        Y = self.spectrum(x)
        if self.modulus:
            return self.W * Y.abs()
        return torch.stack([self.W * Y.real, self.W * Y.imag], dim=3)

    def H(self, x):
        return self.planes(x).reshape(x.shape[0], -1).to(x.dtype)

    def Ht(self, v):
        assert not self.modulus
        v = v.reshape(v.shape[0], self.channels, self.K, 2, self.dim, self.dim).double()
        back = ifft2c(self.W * torch.complex(v[:, :, :, 0], v[:, :, :, 1]))
        return (self.S.conj() * back).sum(dim=2).real.reshape(v.shape[0], -1)


# ---- the two constructions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,K', [(32, 4), (32, 1), (64, 8), (96, 3), (32, 32)])
def test_coil_maps_sum_of_squares_is_one(d, K):
    from nhmc import operators
    s = operators.coil_maps(d, K)
    assert s.shape == (K, d, d) and s.dtype == torch.complex64
    assert torch.equal(s, operators.coil_maps(d, K))                                  # deterministic, no RNG
    # the float64 definition, restated
    c = (d - 1) / 2
    row, col = torch.arange(d, dtype=torch.float64)[:, None] - c, torch.arange(d, dtype=torch.float64)[None, :] - c
    maps = []
    for k in range(K):
        th = torch.tensor(2 * np.pi * k / K, dtype=torch.float64)
        mag = torch.exp(-((row - 0.6 * d * torch.sin(th)) ** 2 + (col - 0.6 * d * torch.cos(th)) ** 2) / (2 * (0.5 * d) ** 2))
        maps.append(torch.polar(mag, np.pi * (col * torch.cos(th) + row * torch.sin(th)) / d + th))
    want = torch.stack(maps)
    want = want / (want.abs() ** 2).sum(dim=0).sqrt()
    assert float(((want.abs() ** 2).sum(dim=0) - 1).abs().max()) < 1e-12
    assert float((s.to(torch.complex128) - want).abs().max()) < 2e-7                  # rounded to complex64 once
    if (d, K) == (32, 4):                                                             # the figures the definition states
        assert 0.068 < float(want.abs().min()) < 0.070 and 0.90 < float(want.abs().max()) < 0.92


def test_coil_maps_refusals():
    from nhmc import operators
    for bad in ((32, 0), (32, 33), (32, -1), (0, 4)):
        with pytest.raises(operators.NhmcError):
            operators.coil_maps(*bad)


def test_diffraction_masks_unit_modulus_and_seeding():
    from nhmc import operators
    a = operators.diffraction_masks(32, 4, torch.Generator().manual_seed(3))
    b = operators.diffraction_masks(32, 4, torch.Generator().manual_seed(3))
    c = operators.diffraction_masks(32, 4, torch.Generator().manual_seed(4))
    assert a.shape == (4, 32, 32) and a.dtype == torch.complex64
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float((a.abs() - 1).abs().max()) < 1e-6
    u = torch.rand(4, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    assert float((a.to(torch.complex128) - torch.polar(torch.ones_like(u), 2 * np.pi * u)).abs().max()) < 2e-7
    torch.manual_seed(11)                                                             # generator=None: the global RNG
    d1 = operators.diffraction_masks(32, 2)
    torch.manual_seed(11)
    assert torch.equal(d1, operators.diffraction_masks(32, 2))
    for bad in ((32, 0), (32, 33), (0, 2)):
        with pytest.raises(operators.NhmcError):
            operators.diffraction_masks(*bad)


# ---- routes --------------------------------------------------------------------------------------------------------
def test_build_operator_routes():
    from nhmc import operators
    op = operators.build_operator('mcmri4', 3, 32, 'cpu', n_coils=4)
    assert isinstance(op, operators.ModulatedFourier) and op.is_linear() and op.M == 2 * 3 * 4 * 32 * 32
    assert op.maps.dtype == torch.complex64 and torch.equal(op.maps, operators.coil_maps(32, 4))
    assert int(op.weights[0].sum()) == 8 and op.weights.shape == (32, 32)            # the mask of mri4
    assert operators.build_operator('mcmri4', 3, 32, 'cpu').maps.shape[0] == 8         # the default coil count
    with pytest.raises(NotImplementedError):
        op.H_pinv(torch.zeros(1, op.M))
    cd = operators.build_operator('cdp4', 3, 32, 'cpu', generator=torch.Generator().manual_seed(1))
    assert isinstance(cd, operators.ModulatedFourier) and not cd.is_linear() and cd.M == 3 * 4 * 32 * 32
    assert torch.equal(cd.maps, operators.diffraction_masks(32, 4, torch.Generator().manual_seed(1)))
    assert torch.equal(cd.weights, torch.ones(32, 32)) and cd.forward == cd.H
    with pytest.raises(NotImplementedError):
        cd.Ht(torch.zeros(1, cd.M))
    with pytest.raises(NotImplementedError):
        cd.H_pinv(torch.zeros(1, cd.M))
    for deg in ('mcmri0', 'mcmri33', 'cdp0', 'cdp33'):
        with pytest.raises(operators.NhmcError):
            operators.build_operator(deg, 3, 32, 'cpu')
    # the routes that were there are what they were
    assert isinstance(operators.build_operator('mri4', 3, 32, 'cpu'), operators.FourierSampling)
    assert isinstance(operators.build_operator('cs4', 3, 32, 'cpu'), operators.WalshHadamardCS)


def test_constructor_refusals():
    from nhmc import operators
    ok = operators.coil_maps(32, 2)
    op = operators.ModulatedFourier(ok, 3, 32, 'cpu')
    assert torch.equal(op.maps, ok) and torch.equal(op.weights, torch.ones(32, 32)) and op.M == 2 * 3 * 2 * 32 * 32
    assert op.S.shape == (2, 2, 32, 32) and torch.equal(op.S[:, 0], ok.real) and torch.equal(op.S[:, 1], ok.imag)
    real = operators.ModulatedFourier(torch.ones(1, 32, 32), 1, 32, 'cpu', modulus=True)      # a real map is taken
    assert real.maps.dtype == torch.complex64 and real.M == 32 * 32
    assert operators.ModulatedFourier(ok.numpy(), 3, 32, 'cpu').maps.dtype == torch.complex64  # an array too
    nan = ok.clone()
    nan[1, 2, 3] = complex(0.0, float('nan'))
    inf = ok.clone()
    inf[0, 0, 0] = complex(float('inf'), 0.0)
    for bad, what in ((ok[0], 'maps'), (ok[None], 'maps'), (torch.ones(2, 32, 64), 'maps'), (torch.ones(2, 16, 16), 'maps'),
                      (nan, 'finite'), (inf, 'finite'), (torch.zeros(2, 32, 32), 'zero'), (torch.ones(33, 32, 32), '33'),
                      (torch.ones(0, 32, 32), '0')):
        with pytest.raises(operators.NhmcError, match=what):
            operators.ModulatedFourier(bad, 3, 32, 'cpu')
    with pytest.raises(operators.NhmcError, match='32'):
        operators.ModulatedFourier(torch.ones(2, 48, 48), 3, 48, 'cpu')
    # the weights: FourierSampling's checks
    w = torch.rand(32, 32)
    for bad in (torch.zeros(32, 32), -w, torch.ones(32), torch.ones(32, 64), torch.ones(32, 32, dtype=torch.complex64),
                w.clone().index_put_((torch.tensor(3), torch.tensor(4)), torch.tensor(float('nan')))):
        with pytest.raises(operators.NhmcError, match='weights'):
            operators.ModulatedFourier(ok, 3, 32, 'cpu', weights=bad)
    assert torch.equal(operators.ModulatedFourier(ok, 3, 32, 'cpu', weights=w).weights, w)


def test_coil_map_file_loader(tmp_path):
    from nhmc import operators
    good = operators.coil_maps(32, 3).numpy()
    np.save(tmp_path / 'good.npy', good)
    s = operators.load_coil_maps(str(tmp_path / 'good.npy'), 32)
    assert s.dtype == torch.complex64 and torch.equal(s, torch.from_numpy(good))
    np.save(tmp_path / 'real.npy', np.abs(good).astype(np.float64))
    assert operators.load_coil_maps(str(tmp_path / 'real.npy'), 32).dtype == torch.complex64
    op = operators.build_operator('mcmri4', 3, 32, 'cpu', coil_maps_file=str(tmp_path / 'good.npy'))
    assert torch.equal(op.maps, s) and op.M == 2 * 3 * 3 * 32 * 32

    nan = good.copy()
    nan[0, 1, 2] = np.nan
    cases = {'rank2.npy': np.ones((32, 32)), 'rank4.npy': np.ones((1, 1, 32, 32)), 'size.npy': np.ones((2, 64, 64)),
             'rect.npy': np.ones((2, 32, 64)), 'nan.npy': nan, 'zero.npy': np.zeros((2, 32, 32)), 'many.npy': np.ones((33, 32, 32)),
             'none.npy': np.ones((0, 32, 32)), 'text.npy': np.full((2, 32, 32), 'a'), 'bool.npy': np.ones((2, 32, 32), dtype=bool)}
    for name, arr in cases.items():
        np.save(tmp_path / name, arr)
        with pytest.raises(operators.NhmcError, match='coil_maps') as info:
            operators.load_coil_maps(str(tmp_path / name), 32)
        assert '\n' not in str(info.value) and name in str(info.value)               # one line, naming the file
    with pytest.raises(operators.NhmcError, match='64 x 64'):
        operators.load_coil_maps(str(tmp_path / 'size.npy'), 32)
    with pytest.raises(operators.NhmcError, match='no such file'):
        operators.load_coil_maps(str(tmp_path / 'absent.npy'), 32)
    (tmp_path / 'junk.npy').write_bytes(b'not an array')
    with pytest.raises(operators.NhmcError, match='not a .npy'):
        operators.load_coil_maps(str(tmp_path / 'junk.npy'), 32)
    np.save(tmp_path / 'object.npy', np.array([[[{}] * 32] * 32] * 2, dtype=object), allow_pickle=True)
    with pytest.raises(operators.NhmcError):                                          # a pickle is never loaded
        operators.load_coil_maps(str(tmp_path / 'object.npy'), 32)
    np.savez(tmp_path / 'archive.npz', s=good)
    with pytest.raises(operators.NhmcError):
        operators.load_coil_maps(str(tmp_path / 'archive.npz'), 32)


# ---- the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,K', [(32, 4), (96, 2)])
def test_the_oracle_is_adjoint_and_restates_the_factors(d, K):
    """<H x, v> = <x, Ht v> for the oracle, and the definition with F = Cm + i Sm gives the oracle's spectrum."""
    from nhmc import operators
    g = torch.Generator().manual_seed(d + K)
    W = torch.rand(d, d, generator=g).double() * (torch.rand(d, d, generator=g) > 0.4)
    S = operators.coil_maps(d, K)
    ref = ModFourierRef(S, 2, d, W)
    X = torch.randn(3, 2, d, d, generator=g, dtype=torch.float64)
    v = torch.randn(3, ref.M, generator=g, dtype=torch.float64)
    lhs, rhs = float((ref.H(X) * v).sum()), float((X.reshape(3, -1) * ref.Ht(v)).sum())
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)
    op = operators.ModulatedFourier(S, 2, d, 'cpu', weights=W)
    F = torch.complex(op.Cm, op.Sm)
    Y = F @ (S.to(torch.complex128) * X[:, :, None]) @ F.t()
    assert float((Y - ref.spectrum(X)).abs().max()) < 1e-12 * float(Y.abs().max())
    # the decomposition the kernels use: A = Sre o x, B = Sim o x, Y = Y_A + i Y_B
    YA, YB = fft2c(S.real.double() * X[:, :, None]), fft2c(S.imag.double() * X[:, :, None])
    assert float((torch.complex(YA.real - YB.imag, YA.imag + YB.real) - Y).abs().max()) < 1e-12 * float(Y.abs().max())
    # and its adjoint: U = Re[F^H q conj(F)], V = Im[...], g = sum_k (Sre U + Sim V)
    q = W * torch.complex(*v.reshape(3, 2, K, 2, d, d).unbind(3))
    back = F.conj().t() @ q @ F.conj()
    ht = (S.real.double() * back.real + S.imag.double() * back.imag).sum(dim=2).reshape(3, -1)
    assert float((ht - ref.Ht(v)).abs().max()) < 1e-12 * float(ht.abs().max())


def test_one_unit_map_is_the_fourier_oracle():
    d = 32
    g = torch.Generator().manual_seed(9)
    W = torch.rand(d, d, generator=g) * (torch.rand(d, d, generator=g) > 0.4)
    ref, old = ModFourierRef(torch.ones(1, d, d), 3, d, W), FourierRef(W, 3, d)
    x = torch.randn(2, 3, d, d, generator=g, dtype=torch.float64)
    assert ref.M == old.M and torch.equal(ref.H(x), old.H(x))
    v = torch.randn(2, ref.M, generator=g, dtype=torch.float64)
    assert float((ref.Ht(v) - old.Ht(v)).abs().max()) < 1e-13
    mod = ModFourierRef(torch.ones(1, d, d), 3, d, modulus=True)
    assert mod.M == 3 * d * d and float((mod.planes(x)[:, :, 0] - fft2c(x).abs()).abs().max()) < 1e-13


# ---- the header ----------------------------------------------------------------------------------------------------
def test_the_header_states_the_definition():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = ' '.join(open(os.path.join(root, 'include', 'nhmc.h')).read().replace('*', ' ').split())
    for phrase in ('A = Sre_k o v, B = Sim_k o v', 'Re Y = Re Y_A - Im Y_B, Im Y = Im Y_A + Re Y_B',
                   'H(x) = [w o Re Y ; w o Im Y] [n_chains][C][K][2][d][d], M = 2 C K d^2',
                   'H(x) = w o a [n_chains][C][K][d][d], M = C K d^2', 'q = a == 0 ? 0 : (w r) (Y / a)',
                   'U_k = Re[F^H q_k conj(F)] = adj(q_re, q_im), V_k = Im[F^H q_k conj(F)] = adj(q_im, -q_re)',
                   'g = -2 sum_k (Sre_k o U_k + Sim_k o V_k)', 'The sum over k ascends from 0.0f', '48 d^3 FLOP per (plane, map)',
                   'n_chains channels 2 n_maps > 65535', 'at most 8 d^2', '6.4 GB', 'Shape is checked before alignment'):
        assert phrase in text, phrase
    for entry in ('nhmc_modfourier_tiles', 'nhmc_modfourier_tmp_floats', 'nhmc_modfourier_H', 'nhmc_modfourier_Ht',
                  'nhmc_data_modfourier', 'nhmc_data_modfourier_vjp'):
        assert f'{entry}(' in text
    assert '#define NHMC_ABI_VERSION 2' in text
    from nhmc import _lib
    assert all(name in _lib.SIGNATURES for name in ('nhmc_modfourier_H', 'nhmc_modfourier_Ht', 'nhmc_data_modfourier',
                                                    'nhmc_data_modfourier_vjp', 'nhmc_modfourier_tiles',
                                                    'nhmc_modfourier_tmp_floats'))

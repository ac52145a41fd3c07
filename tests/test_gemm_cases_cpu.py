"""CPU: the case list of tests/test_gemm_tiles_gpu.py (oracle/gemm_cases.py) is what it claims to be -- its fp32 oracles
agree with their float64 twins, the tile path recorded for every product is the one csrc/spectral_gemm.hip takes, the
library's own tile counts agree, and the list as a whole reaches every tile size on both block-remap branches, on
rectangular grids and, for the transposing epilogue and the loss partials, on more than one tile."""
import pytest
import torch

from oracle import gemm_cases as gc

ids = lambda cases: [c.id for c in cases]


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


@pytest.mark.parametrize('c', gc.SANDWICH, ids=ids(gc.SANDWICH))
def test_sandwich_fp32_oracle_agrees_with_float64(c):
    p = gc.sandwich_problem(c.args)
    worst = max(gc.rel(p.out32, p.out64), gc.rel(p.out32_mul, p.out64_mul))
    print(f'{c.id}: fp32 vs float64 {worst:.2e}')
    assert worst <= 2e-6


@pytest.mark.parametrize('c', gc.SPECTRAL + gc.SRCONV, ids=ids(gc.SPECTRAL + gc.SRCONV))
def test_operator_fp32_oracle_agrees_with_float64(c):
    """H, Ht, H_pinv, the data-term gradient (with and without the clip) and the loss: the fp32 CPU evaluation is the
    yardstick the 2e-5 bound of the GPU tests is held against."""
    p = gc.spectral_problem(c.args) if c.family == 'spectral' else gc.srconv_problem(c.args)
    maps = max(gc.rel(getattr(p.f32, k), getattr(p.f64, k)) for k in ('H', 'Ht', 'H_pinv', 'grad_clip', 'grad_noclip'))
    loss = max(gc.rel(p.f32.loss_clip, p.f64.loss_clip), gc.rel(p.f32.loss_noclip, p.f64.loss_noclip))
    print(f'{c.family} {c.id}: fp32 vs float64 maps and gradients {maps:.2e}, loss {loss:.2e}')
    assert maps <= 2e-6 and loss <= 2e-6
    assert bool((p.f64.grad_clip == 0)[p.xt.abs() > 1].all()) and bool((p.xt.abs() > 1).any())    # the clip is active


@pytest.mark.parametrize('c', gc.CASES, ids=[f'{c.family}-{c.id}' for c in gc.CASES])
def test_recorded_tile_paths_are_the_kernels(c, lib):
    for pr in c.products:
        assert gc.tile_path(pr.R, pr.C, pr.n_img) == pr.path, (c.id, pr.name)
    tiles = {pr.path[1] * pr.path[2] for pr in c.products if pr.loss}
    if c.family == 'spectral':
        d, B, C = c.args
        assert tiles == {lib.nhmc_spectral_tiles(C, d) // C} and lib.nhmc_spectral_tiles(C, d) % C == 0
    if c.family == 'srconv':
        d, stride, B = c.args
        assert tiles == {lib.nhmc_srconv_tiles(3, d // stride) // 3} and lib.nhmc_srconv_tiles(3, d // stride) % 3 == 0


def test_tile_path_restates_the_library():
    """tile_of2 through the one host function that exposes it, on every size class."""
    import nhmc
    lib = nhmc._lib.load()
    for sd in (32, 64, 96, 128, 160, 192, 256, 320, 384, 512):
        T, rows, cols, _ = gc.tile_path(sd, sd, 1)
        assert lib.nhmc_srconv_tiles(5, sd) == 5 * rows * cols and lib.nhmc_spectral_tiles(5, sd) == 5 * rows * cols
        assert T == (128 if sd % 128 == 0 else 64 if sd % 64 == 0 else 32)
    assert gc.tile_path(256, 64, 1)[:3] == (64, 4, 1) and gc.tile_path(128, 96, 2)[:3] == (32, 4, 3)
    assert gc.tile_path(96, 96, 8)[3] and not gc.tile_path(96, 96, 3)[3] and gc.tile_path(128, 128, 8)[3]


def test_the_list_covers_every_tile_size_on_every_branch():
    products = [pr for c in gc.CASES for pr in c.products]
    for T in (32, 64, 128):
        mine = [pr.path for pr in products if pr.path[0] == T]
        assert any(p[3] for p in mine) and any(not p[3] for p in mine), f'T = {T}: both remap branches'
        assert any(p[1] != p[2] for p in mine), f'T = {T}: a rectangular tile grid'
        assert any(p[3] and p[1] * p[2] > 1 for p in mine), f'T = {T}: the remap with several tiles per image'
        for family, cases in (('spectral', gc.SPECTRAL), ('srconv', gc.SRCONV)):
            tout = [pr.path for c in cases for pr in c.products if pr.tout and pr.path[0] == T]
            assert any(p[1] * p[2] > 1 for p in tout), f'T = {T}, {family}: the transposing epilogue on several tiles'
    for cases in (gc.SPECTRAL, gc.SRCONV):                                 # loss partials on several tiles per plane
        assert {pr.path[0] for c in cases for pr in c.products if pr.loss and pr.path[1] * pr.path[2] > 1} >= {32, 64}
    assert {c.args[0] for c in gc.SPECTRAL} >= {96, 128, 192, 256, 384}
    assert any(c.args[2] == 1 for c in gc.SPECTRAL) and any(c.args[2] == 4 for c in gc.SPECTRAL)
    at256 = [c.args[1] * c.args[2] for c in gc.SPECTRAL if c.args[0] == 256]
    assert len(at256) >= 2 and all(n % 2 == 1 for n in at256)              # odd image counts through k_pair256


def test_operator_data_is_generic():
    """Nothing a swapped factor, a dropped transpose or a wrong channel index could hide behind."""
    for c in gc.SPECTRAL:
        d, B, C = c.args
        op = gc.random_spectral(d, C, 100 + d + C)
        mats = dict(U1=op.U1, U2=op.U2, V1=op.V1, V2=op.V2)
        names = sorted(mats)
        for i, a in enumerate(names):
            assert float((mats[a].t() @ mats[a] - torch.eye(d)).abs().max()) < 1e-5          # the projected form's condition
            assert float((mats[a] - mats[a].t()).abs().max()) > 0.1
            for b in names[i + 1:]:
                assert float((mats[a] - mats[b]).abs().max()) > 0.1 and float((mats[a] - mats[b].t()).abs().max()) > 0.1
        zeros = float((op.D == 0).float().mean())
        assert 0.05 < zeros < 0.15 and float(op.D[op.D != 0].min()) >= 0.2 and float(op.D.max()) <= 1.0
        for i in range(C):
            assert float((op.D[i] - op.D[i].t()).abs().max()) > 0.1
            for j in range(i + 1, C):
                assert float((op.D[i] - op.D[j]).abs().max()) > 0.1 and float((op.D[i] - op.D[j].t()).abs().max()) > 0.1
    for c in gc.SRCONV:
        d, stride, B = c.args
        op = gc.random_srconv(d, stride, 3, 200 + d)
        sd = d // stride
        assert op.U.shape == (sd, sd) and op.V.shape == (d, d) and op.s.shape == (sd,)
        assert float((op.U - op.V[:sd, :sd]).abs().max()) > 0.1 and float((op.U - op.U.t()).abs().max()) > 0.1
        small = op.s < 3e-2
        assert bool(small[::7].all()) and int(small.sum()) == len(range(0, sd, 7)) and float(op.s[~small].min()) >= 0.3
        assert float(op.ref32.S[0].abs().max()) == 0.0 and float(op.ref32.Sinv[0].abs().max()) == 0.0


def test_embed_pads_with_zeros_in_the_top_left_block():
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5) + 1
    e = gc.embed(t, 8)
    assert e.shape == (2, 8, 8) and torch.equal(e[:, :3, :5], t) and float(e.sum()) == float(t.sum())
    r = gc.embed(t, (4, 6))
    assert r.shape == (2, 4, 6) and torch.equal(r[:, :3, :5], t) and float(r[:, 3:].abs().sum() + r[:, :, 5:].abs().sum()) == 0.0

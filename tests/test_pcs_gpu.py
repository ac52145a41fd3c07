"""GPU: principal components of the posterior samples -- the Gram kernel (nhmc_sample_gram, csrc/pcs.hip) bit for bit on
data whose products and sums are exact in fp64 (which pins the fp64 MFMA's operand and result maps on both sides of every
row-block bound), within the worst-case bound of an fp64 sum on real-valued data, its symmetry, NaN handling and what it
leaves untouched; the projection kernel against its float64 restatement; `metrics.pcs` and `metrics.summarize(pcs=...)`
against the SVD restatement of tests/test_pcs_cpu.py; and the two CLIs' report."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_calib_gpu import cloud
from test_diag_gpu import TINY
from test_pcs_cpu import GAP, KEYS, ensemble, gram_float64, pcs_float64, rel

pytestmark = pytest.mark.gpu

G = 3
SHAPES = [(3, 8, 8),          # 192 elements: less than a slab, less than two tiles of the widest kernel
          (1, 4, 193),        # 772: a ragged tail in every tile width
          (3, 20, 20),        # 1200: a full slab and a ragged one
          (3, 64, 64)]        # 12288: twelve slabs
# n -> the (K, S) splits it is run with: K = 1 and, where 4 divides n, K = 4
SPLITS = {n: [(1, n)] + ([(4, n // 4)] if n % 4 == 0 else []) for n in (2, 16, 17, 20, 33, 64, 65, 160, 256)}


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def int_block(n, shape, seed):
    """-> (x float32 [G, n, C, H, W], t float32 [G, C, H, W]) with values k / 64, |k| <= 64: a difference is a multiple of
    1 / 64 below 2 in magnitude, a product a multiple of 2^-12 below 4, and a sum of 12288 of them is far inside fp64's 53
    bits -- every order of summation gives the same bits."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-64, 65, (G, n) + shape, generator=g).float() / 64.0
    t = torch.randint(-64, 65, (G,) + shape, generator=g).float() / 64.0
    rows = torch.cat([x.reshape(G, n, -1), t.reshape(G, 1, -1)], dim=1)
    for gi in range(G):
        assert len({r.numpy().tobytes() for r in rows[gi]}) == n + 1              # distinct rows
    return x, t


def ref_grams(x, t):
    """x [G, n, ...], t [G, ...] or None on the host -> [G, n, n] float64, the restatement per image."""
    n = x.shape[1]
    return np.stack([gram_float64(x[gi].reshape(n, -1).numpy(), None if t is None else t[gi].flatten().numpy())
                     for gi in range(x.shape[0])])


@pytest.mark.parametrize('n', sorted(SPLITS))
def test_gram_of_integer_data_bit_for_bit(n):
    """A wrong lane map of the fp64 MFMA result (the f32 one, say) runs clean and misplaces three of four results: the rows
    are distinct and the matrix is not a function of |a - b|, so any misplacement changes bits."""
    import nhmc.kernels as K_
    for shape in SHAPES:
        x, t = int_block(n, shape, seed=n)
        want = ref_grams(x, t)
        assert not np.array_equal(want[0], want[0][::-1, ::-1]) and np.isfinite(want).all()
        xd, td = x.cuda(), t.cuda()
        for K, S in SPLITS[n]:
            got = K_.sample_gram(xd.reshape((G * K, S) + shape), td, K)
            assert got.shape == (G, n, n) and got.dtype == torch.float64
            assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), (n, shape, K)


REAL = [(1, 2), (1, 20), (5, 13), (8, 20), (4, 64)]          # (K, S): n = 2, 20, 65, 160, 256


@pytest.mark.parametrize('K,S', REAL)
def test_gram_of_real_valued_data(K, S):
    """|S_ab - ref_ab| <= (E + 2) 2^-52 sqrt(ref_aa ref_bb): the operands u = d - d_1 are exact in fp64 on both sides (two
    fp32 values), so the two differ by the rounding of E products and E - 1 additions each, which in any order is at most
    (E + 1) 2^-53 sum |u_a u_b| <= (E + 1) 2^-53 |u_a| |u_b| per side (Cauchy-Schwarz), and the bound is taken against the
    restatement's own diagonal, itself off by a relative (E + 1) 2^-53: the extra 1 in E + 2."""
    import nhmc.kernels as K_
    n = K * S
    for shape in SHAPES:
        x, t = cloud(G, K, S, *shape)
        E = x[0, 0].numel()
        want = ref_grams(x.reshape((G, n) + shape), t)
        xd, td = x.cuda(), t.cuda()
        got_d = K_.sample_gram(xd, td, K)
        got = got_d.cpu().numpy()
        diag = np.sqrt(np.einsum('gaa->ga', want))
        bound = (E + 2) * 2.0 ** -52 * diag[:, :, None] * diag[:, None, :]
        err = np.abs(got - want)
        print(f'n {n} shape {shape}: largest error / bound {np.max(err / bound):.3e}')
        assert np.isfinite(got).all() and np.all(err <= bound)
        assert np.array_equal(got.view(np.int64), got.transpose(0, 2, 1).copy().view(np.int64))       # exactly symmetric
        assert torch.equal(bits(K_.sample_gram(xd, td, K)), bits(got_d))                             # equal inputs, equal bits
        bare = K_.sample_gram(xd, None, K).cpu().numpy()
        assert np.isnan(bare[:, n - 1, :]).all() and np.isnan(bare[:, :, n - 1]).all()
        assert np.array_equal(bare[:, :n - 1, :n - 1].view(np.int64), got[:, :n - 1, :n - 1].view(np.int64))


@pytest.mark.parametrize('K,S', [(1, 20), (8, 20)])
def test_non_finite_draws(K, S):
    """A NaN (or inf) draw of image 1 poisons exactly its row and column, a NaN first draw the whole matrix of image 1; the
    other images keep their bits."""
    import nhmc.kernels as K_
    n, shape = K * S, (1, 4, 193)
    x, t = cloud(G, K, S, *shape)
    clean = K_.sample_gram(x.cuda(), t.cuda(), K).cpu().numpy()
    pooled = x.reshape(G, n, -1)                              # a view
    for value in (float('nan'), float('-inf')):
        for draw, elem in ((7, 5), (n - 1, 771), (17, 300)):
            keep = pooled[1, draw, elem].item()
            pooled[1, draw, elem] = value
            got = K_.sample_gram(x.cuda(), t.cuda(), K).cpu().numpy()
            pooled[1, draw, elem] = keep
            hit = np.zeros((n, n), dtype=bool)
            hit[draw - 1, :] = hit[:, draw - 1] = True        # draw i + 1 is row i
            assert np.isnan(got[1][hit]).all() and np.array_equal(got[1][~hit].view(np.int64), clean[1][~hit].view(np.int64))
            assert np.array_equal(got[[0, 2]].view(np.int64), clean[[0, 2]].view(np.int64))
        keep = pooled[1, 0, 400].item()
        pooled[1, 0, 400] = value
        got = K_.sample_gram(x.cuda(), t.cuda(), K).cpu().numpy()
        pooled[1, 0, 400] = keep
        assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2]].view(np.int64), clean[[0, 2]].view(np.int64))
    keep = t[1].flatten()[9].item()                           # and the original's row is the last
    t[1].view(-1)[9] = float('nan')
    got = K_.sample_gram(x.cuda(), t.cuda(), K).cpu().numpy()
    t[1].view(-1)[9] = keep
    assert np.isnan(got[1, n - 1]).all() and np.isnan(got[1, :, n - 1]).all()
    assert np.array_equal(got[1, :n - 1, :n - 1].view(np.int64), clean[1, :n - 1, :n - 1].view(np.int64))
    assert np.array_equal(got[[0, 2]].view(np.int64), clean[[0, 2]].view(np.int64))


@pytest.mark.parametrize('K,S', [(1, 20), (4, 16), (8, 20)])
def test_nothing_outside_the_buffers_is_written(K, S):
    """gram, out and ws sit inside larger buffers filled with a sentinel; it survives around them."""
    import nhmc
    lib = nhmc._lib.load()
    n, J, pad, mark = K * S, 3, 64, 12345.0
    P = lambda ten: ctypes.c_void_p(ten.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for shape in ((1, 4, 193), (3, 64, 64)):
        x, t = cloud(G, K, S, *shape)
        E = x[0, 0].numel()
        xd, td = x.cuda(), t.cuda()
        n_ws = lib.nhmc_sample_gram_ws_bytes(G, n, E) // 8
        assert n_ws > 0 and n_ws % (G * lib.nhmc_sample_gram_slabs(E) * 256) == 0
        gram = torch.full((G * n * n + 2 * pad,), mark, dtype=torch.float64, device='cuda')
        ws = torch.full((n_ws + 2 * pad,), mark, dtype=torch.float64, device='cuda')
        assert lib.nhmc_sample_gram(P(xd), P(td), P(gram[pad:]), P(ws[pad:]), G, K, S, E, stream) == 0
        coef = torch.randn(G, J, n, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).cuda()
        out = torch.full((G * J * E + 2 * pad,), mark, dtype=torch.float32, device='cuda')
        assert lib.nhmc_sample_project(P(xd), P(coef), P(out[pad:]), G, K, S, J, E, stream) == 0
        torch.cuda.synchronize()
        for buf in (gram, ws, out):
            assert (buf[:pad] == mark).all() and (buf[-pad:] == mark).all()
        import nhmc.kernels as K_
        assert torch.equal(bits(gram[pad:pad + G * n * n]), bits(K_.sample_gram(xd, td, K).flatten()))
        assert torch.equal(bits(out[pad:pad + G * J * E]), bits(K_.sample_project(xd, coef, K).flatten()))


def ulp32(v):
    return np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('K,S', [(1, 2), (1, 20), (5, 13), (4, 64)])
@pytest.mark.parametrize('J', [1, 3, 8])
def test_projection(K, S, J):
    """Random coefficients (no eigen conditioning): within 1 fp32 ulp of the float64 restatement, plus what n fp64 fmas may
    differ from numpy's float64 sum in another order, n 2^-52 sum_i |c_i (d_i - d_1)| -- felt only where the sum cancels to
    nothing.  Zero coefficients give zero images."""
    import nhmc.kernels as K_
    n = K * S
    g = torch.Generator().manual_seed(100 * n + J)
    for shape in ((1, 4, 193), (3, 20, 20)):
        x, _ = cloud(G, K, S, *shape)
        coef = torch.randn(G, J, n, dtype=torch.float64, generator=g)
        got = K_.sample_project(x.cuda(), coef.cuda(), K)
        assert got.shape == (G, J) + shape and got.dtype == torch.float32
        d = x.reshape(G, n, -1).numpy().astype(np.float64)
        u = d - d[:, :1]
        want = np.einsum('gjn,gne->gje', coef.numpy(), u)
        slack = n * 2.0 ** -52 * np.einsum('gjn,gne->gje', np.abs(coef.numpy()), np.abs(u))
        err = np.abs(got.reshape(G, J, -1).cpu().numpy().astype(np.float64) - want)
        print(f'n {n} J {J} shape {shape}: largest error {np.max(err / ulp32(want)):.3f} ulp')
        assert np.all(err <= ulp32(want) + slack)
        zero = K_.sample_project(x.cuda(), torch.zeros_like(coef).cuda(), K)
        assert torch.count_nonzero(zero).item() == 0
        assert torch.equal(bits(K_.sample_project(x.cuda(), coef.cuda(), K)), bits(got))


def separated(K, S, shape, seed):
    """Three images of the well-separated ensemble of tests/test_pcs_cpu.py as an fp32 block [G * K, S, C, H, W] with its
    originals [G, C, H, W], scaled into [-1, 1]."""
    n, E = K * S, int(np.prod(shape))
    sets = [ensemble(n, E, seed=seed + gi) for gi in range(G)]
    scale = 0.9 / max(np.abs(np.concatenate([d.ravel(), t])).max() for d, t, _ in sets)
    x = torch.from_numpy(np.stack([d for d, _, _ in sets]) * scale).float().reshape((G * K, S) + shape).contiguous()
    t = torch.from_numpy(np.stack([t for _, t, _ in sets]) * scale).float().reshape((G,) + shape).contiguous()
    return x, t


def check_against_the_restatement(res, x, t, K, count):
    n = K * x.shape[1]
    pooled, truth = x.reshape(G, n, -1).numpy(), t.reshape(G, -1).numpy()
    assert res['directions'].shape == (G, count) + tuple(x.shape[2:]) and res['directions'].dtype == torch.float32
    assert res['eigenvalues'].shape == (G, n - 1)
    dirs = res['directions'].reshape(G, count, -1).cpu().numpy().astype(np.float64)
    for gi in range(G):
        ref = pcs_float64(pooled[gi], truth[gi], count)
        print(f'n {n} image {gi}:', {k: (float(res[k][gi]), ref[k]) for k in KEYS}, 'gaps', ref['gaps'][:count])
        assert res['pc_count'][gi] == ref['pc_count'] and res['pc_rank'][gi] == ref['pc_rank']
        for k in KEYS[2:]:
            assert rel(res[k][gi], ref[k]) <= 1e-9, k
        assert np.all(np.abs(res['eigenvalues'][gi] - ref['eigenvalues']) <= 1e-9 * ref['eigenvalues'])
        for j in range(ref['pc_count']):
            if ref['gaps'][j] >= GAP:
                v = dirs[gi, j]
                assert rel(np.linalg.norm(v), np.sqrt(ref['eigenvalues'][j])) <= 1e-6       # one standard deviation, in fp32
                assert v @ ref['directions'][j] / np.linalg.norm(v) >= 1.0 - 1e-9
        assert np.all(ref['gaps'][:min(3, ref['pc_count'])] >= GAP)                         # the first three are compared
        assert np.all(dirs[gi, ref['pc_count']:] == 0.0)


@pytest.mark.parametrize('K,S', [(1, 20), (4, 5), (5, 13)])
def test_pcs_end_to_end(K, S):
    import nhmc.kernels as K_
    from nhmc import metrics
    shape, n = (3, 20, 20), K * S
    x, t = separated(K, S, shape, seed=40 + n)
    xd, td = x.cuda(), t.cuda()
    res = metrics.pcs(xd, td, replicas=K, count=3)
    assert tuple(res) == ('directions', 'eigenvalues') + metrics.PCS_KEYS
    check_against_the_restatement(res, x, t, K, 3)
    # the trace of the covariance is what nhmc_calibration sums
    sum_var = K_.calibration(xd, td, K)[3][:, 1].cpu().numpy()
    assert np.all(np.abs(res['eigenvalues'].sum(axis=1) - sum_var) <= 1e-9 * sum_var)
    # without the original: the same directions, no error figures
    bare = metrics.pcs(xd, None, replicas=K, count=3)
    assert torch.equal(bits(bare['directions']), bits(res['directions']))
    assert np.isnan(bare['pc_err_in_span']).all() and np.isnan(bare['pc_z_rms']).all()
    assert np.array_equal(bare['pc_var_top'], res['pc_var_top'])
    # more directions than there are well-separated ones: served, and the first three still agree
    check_against_the_restatement(metrics.pcs(xd, td, replicas=K, count=8), x, t, K, 8)
    # all draws equal: no component, NaN figures, zero images
    flat = metrics.pcs(torch.full_like(xd, 0.25), td, replicas=K, count=3)
    assert (flat['pc_count'] == 0).all() and (flat['pc_rank'] == 0).all() and torch.count_nonzero(flat['directions']).item() == 0
    assert all(np.isnan(flat[k]).all() for k in KEYS[2:])


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(bits(a[k]), bits(b[k])), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_summarize_carries_the_components(monkeypatch):
    from nhmc import metrics
    K, S, shape = 2, 6, (3, 16, 16)
    x, t = separated(K, S, shape, seed=7)
    xd, td = x.cuda(), t.cuda()
    per_chain = td.repeat_interleave(K, dim=0)
    new = ('directions', 'eigenvalues') + metrics.PCS_KEYS
    reads = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **kw: (reads.append(1), cpu(self, *a, **kw))[1])
    for kw in (dict(replicas=K), dict(replicas=K, calibration=0.8, credible=0.9), dict(), dict(credible=0.9),
               dict(calibration=0.8), dict(replicas=K, calibration=0.8), dict(calibration=0.9, credible=0.8)):
        x_o = td if 'replicas' in kw else per_chain
        reps = kw.get('replicas', 1)
        plain = metrics.summarize(xd, x_o, **kw)
        del reads[:]
        out = metrics.summarize(xd, x_o, pcs=3, **kw)
        assert len(reads) == 1                                                    # the Gram rode in the one read
        assert list(out) == list(plain) + list(new) and not set(new) & set(plain)     # after all others
        _same(plain, {k: out[k] for k in plain})                                    # which keep their bits
        _same(metrics.pcs(xd, x_o, replicas=reps, count=3), {k: out[k] for k in new})
        assert out['directions'].shape == (x_o.shape[0], 3) + shape
        _same(plain, metrics.summarize(xd, x_o, pcs=None, **kw))                      # None is omitting it
        if 'calibration' in kw:       # sum lambda is sum_var: spread_skill^2 = (n + 1) / n sum_var / sum_err2, psnr = 10 lg(4 E / sum_err2)
            n, E = reps * S, int(np.prod(shape))
            sum_err2 = 4.0 * E / 10.0 ** (out['psnr_of_mean'] / 10.0)
            sum_var = out['spread_skill'] ** 2 * n / (n + 1.0) * sum_err2
            assert np.all(np.abs(out['eigenvalues'].sum(axis=1) - sum_var) <= 1e-9 * sum_var)
    check_against_the_restatement(metrics.summarize(xd, td, replicas=K, pcs=3), x, t, K, 3)
    # fewer than two pooled samples: the keys are there, without values
    one = metrics.summarize(xd[:, :1].contiguous(), per_chain, pcs=3)
    assert one['directions'] is None and one['eigenvalues'] is None
    assert all(np.isnan(one[k]).all() and one[k].shape == (G * K,) for k in metrics.PCS_KEYS)
    assert np.isfinite(one['psnr_mean']).all() and list(one)[-len(new):] == list(new)
    # more than 256: the same
    many = metrics.summarize(xd[:1, :1].expand(1, 257, *shape).contiguous(), td[:1], pcs=3)
    assert many['directions'] is None and all(np.isnan(many[k]).all() for k in metrics.PCS_KEYS)


CLI_ARGS = ['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05', '--tau', '0.1',
            '--epsilon', '0.05', '--synthetic', '2', '--philox', '--hmc_epochs', '2', '--hmc_sampling', '4', '--save_images']
POOLED = ['--chains', '4', '--replicas', '2', '--calibration', '--credible']


def _check_rows(rows, cli, stdout, out_dir, size, count):
    from PIL import Image
    for r in rows:
        s = r['image']
        line = [ln for ln in stdout.splitlines() if ln.startswith(f'image {s}: principal components: ')]
        if r['pc_var_first'] is None:
            assert all(r[k] is None for k in cli.PCS_COLUMNS[2:]) and not line
            assert not os.path.exists(os.path.join(out_dir, f'{s}_pc1_plus.png'))
            continue
        assert isinstance(r['pc_count'], int) and isinstance(r['pc_rank'], int)
        assert 1 <= r['pc_count'] == min(count, r['pc_rank']) and r['pc_rank'] <= r['n_samples'] - 1
        assert 0.0 < r['pc_var_first'] <= r['pc_var_top'] <= 1.0 + 1e-12 and 1.0 - 1e-12 <= r['pc_eff_rank'] <= r['pc_rank']
        assert 0.0 <= r['pc_err_in_span'] <= 1.0 + 1e-9 and r['pc_z_rms'] >= 0.0
        assert len(line) == 1 and f'{r["pc_count"]} of rank {r["pc_rank"]}, variance share first ' in line[0]
        assert f' top-{r["pc_count"]} ' in line[0] and ', effective rank ' in line[0]
        assert ', error inside the span ' in line[0] and ', z rms along them ' in line[0]
        for j in range(1, count + 1):
            for side in ('plus', 'minus'):
                path = os.path.join(out_dir, f'{s}_pc{j}_{side}.png')
                if j <= r['pc_count']:
                    assert Image.open(path).size == (size, size), path
                else:
                    assert not os.path.exists(path)
    assert len([ln for ln in stdout.splitlines() if ln.startswith('Total Average principal components: ')]) == 1


def test_cli_reports_the_components(tmp_path, monkeypatch, capsys):
    import yaml
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)
    out_dir, report = tmp_path / 'out', tmp_path / 'report' / 'metrics.json'
    cli.main(CLI_ARGS + POOLED + ['-i', str(out_dir), '--metrics_out', str(report), '--pcs'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    assert len(rows) == 2 and [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert tuple(r) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS + cli.PCS_COLUMNS
        assert r['n_samples'] == 8 and r['pc_count'] == 3
    _check_rows(rows, cli, stdout, out_dir, 32, 3)
    assert stdout.index('image 0: credible interval: ') < stdout.index('image 0: principal components: ')
    # without the flag: the former columns and lines, no such line, no such picture
    out2, report2 = tmp_path / 'out2', tmp_path / 'report2.json'
    cli.main(CLI_ARGS + POOLED + ['-i', str(out2), '--metrics_out', str(report2)])
    stdout2, rows2 = capsys.readouterr().out, json.loads(report2.read_text())
    assert 'principal' not in stdout2 and 'image 0: credible interval: ' in stdout2
    assert all(tuple(r) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS for r in rows2)
    assert not os.path.exists(out2 / '0_pc1_plus.png')
    kind = lambda text: [(ln.split(':')[0], ln.split(':')[1].split()[0]) if ln.startswith('image ') else ln.split(':')[0]
                         for ln in text.splitlines()]           # which line, not its figures: two runs differ in the last digits
    assert kind('\n'.join(ln for ln in stdout.splitlines() if 'principal components' not in ln)) == kind(stdout2)


def test_cli_with_the_flag_alone(tmp_path, monkeypatch, capsys):
    import yaml
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    cli.main(CLI_ARGS + ['--chains', '2', '-i', str(out_dir), '--metrics_out', str(report), '--pcs', '2'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    assert [r['image'] for r in rows] == [0, 1] and all(tuple(r) == cli.COLUMNS + cli.PCS_COLUMNS for r in rows)
    assert all(r['n_samples'] == 4 and r['pc_count'] == 2 for r in rows)
    _check_rows(rows, cli, stdout, out_dir, 32, 2)


def test_cli_with_calibration_and_the_flag(tmp_path, monkeypatch, capsys):
    """`--calibration --pcs` without `--credible`: the Gram follows the calibration block in the single read.  Every
    `summarize` call of the run is held to `metrics.pcs` on the same samples, bit for bit (the Gram is deterministic)."""
    import yaml
    from nhmc import cli, metrics
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)
    real, seen = metrics.summarize, []

    def checked(samples, x_orig, **kw):
        out = real(samples, x_orig, **kw)
        alone = metrics.pcs(samples, x_orig, replicas=kw.get('replicas', 1), count=kw['pcs'])
        _same(alone, {k: out[k] for k in alone})
        seen.append(kw)
        return out
    monkeypatch.setattr(metrics, 'summarize', checked)
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    cli.main(CLI_ARGS + ['--chains', '2', '-i', str(out_dir), '--metrics_out', str(report), '--pcs', '2', '--calibration'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    assert seen and all(kw['pcs'] == 2 and kw['calibration'] == 0.9 and kw['credible'] is None for kw in seen)
    assert all(tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS + cli.PCS_COLUMNS for r in rows)
    assert all(r['n_samples'] == 4 and r['pc_count'] == 2 and r['pc_rank'] == 3 for r in rows)
    _check_rows(rows, cli, stdout, out_dir, 32, 2)


def test_latent_cli_reports_the_components(tmp_path, monkeypatch, capsys):
    """The latent entry on the small latent config of test_diag_gpu.py's latent CLI test, one chain per image."""
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
    args = ['--dataset', 'tiny', '--algo', 'hmc_latent', '--timesteps', '3', '--deg', 'inpaint_random', '--sigma_0', '0.05',
            '--tau', '0.1', '--epsilon', '0.1', '--sigma_y', '1.0', '--synthetic', '2', '--chains', '2', '--philox',
            '--save_images', '--calibration', '0.8', '--credible', '0.8']
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    cli.main_latent(args + ['-i', str(out_dir), '--metrics_out', str(report), '--pcs', '2'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    assert [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS + cli.PCS_COLUMNS
        if r['n_samples'] < 2:
            assert all(r[k] is None for k in cli.PCS_COLUMNS)
    _check_rows(rows, cli, stdout, out_dir, 64, 2)
    out2, report2 = tmp_path / 'out2', tmp_path / 'metrics2.json'
    cli.main_latent(args + ['-i', str(out2), '--metrics_out', str(report2)])
    stdout2, rows2 = capsys.readouterr().out, json.loads(report2.read_text())
    assert 'principal' not in stdout2
    assert all(tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS for r in rows2)

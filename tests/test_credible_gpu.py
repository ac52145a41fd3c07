"""GPU: credible interval and median of the posterior samples -- the kernels (nhmc_credible, csrc/credible.hip) against the
torch.sort restatement of their definition in tests/test_credible_cpu.py, bit for bit on both paths, NaN as torch.sort
has it, the summary, that the interval is the one `metrics.calibration` reports the coverage of, what the kernels leave
untouched, `metrics.summarize` carrying it, and the two CLIs' report."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_credible_cpu import SUMS, credible_ref
from test_diag_gpu import TINY

pytestmark = pytest.mark.gpu

# (G, K, S) for every n = K * S: the ends of the register path's bounds 8, 16, 32, 64, 128, both paths, the cap
SHAPES = {2: (3, 1, 2), 3: (1, 3, 1), 7: (1, 1, 7), 8: (1, 2, 4), 9: (3, 3, 3), 16: (2, 4, 4), 17: (1, 1, 17), 20: (2, 1, 20),
          21: (2, 3, 7), 32: (1, 1, 32), 33: (1, 3, 11), 64: (2, 2, 32), 65: (1, 5, 13), 128: (1, 2, 64), 129: (1, 3, 43),
          160: (1, 8, 20), 1024: (1, 16, 64)}
ELEMS = (4, 252, 256, 260, 768)             # below one tile, around the tile edge, three tiles


def cloud(G, K, S, E, seed=97, planted=True):
    """-> (x float32 [G * K, S, 1, 1, E], t float32 [G, 1, 1, E]) on the host, test_calib_gpu.cloud's recipe: per element
    a cloud of width amp (1e-4 to 0.3 along the elements) about a base in [-0.8, 0.8], each replica offset by half a width,
    the original 1.3 widths from the base, all clamped to [-1, 1] so that clipped ties occur.  Planted: element 0 all draws
    equal, 1 quantised to 4 levels, 2 a mix of -0.0 and +0.0, 3 one +inf and one -inf draw among the others."""
    g = torch.Generator().manual_seed(seed + 1000 * E + G * K * S)
    f64 = torch.float64
    amp = torch.logspace(-4, -0.5, E, dtype=f64)
    base = torch.rand(G, 1, 1, E, generator=g, dtype=f64) * 1.6 - 0.8
    off = 0.5 * amp * torch.randn(G, K, 1, E, generator=g, dtype=f64)
    x = (base + off + amp * torch.randn(G, K, S, E, generator=g, dtype=f64)).clamp(-1, 1).float()
    t = (base[:, 0, 0] + 1.3 * amp * torch.randn(G, E, generator=g, dtype=f64)).clamp(-1, 1).float()
    if planted:
        x[..., 0] = 0.75
        x[..., 1] = torch.randint(0, 4, (G, K, S), generator=g).float() * 0.25 - 0.5
        x[..., 2] = torch.where(torch.rand(G, K, S, generator=g) < 0.5, -0.0, 0.0)
        flat = x.reshape(G, K * S, E)                        # a view: the pooled draws
        flat[:, 0, 3], flat[:, K * S - 1, 3] = float('inf'), float('-inf')
    return x.reshape(G * K, S, 1, 1, E).contiguous(), t.reshape(G, 1, 1, E).contiguous()


def ranks(n):
    return list(range(1, n // 2 + 1)) if n <= 21 else sorted({1, 2, n // 2})


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_maps(got, ref, where):
    """== on every element where the restatement is a number (so -0.0 may answer +0.0), NaN exactly where it is NaN."""
    for name, g in zip(('lower', 'median', 'upper'), got):
        g, w = g.flatten().cpu().numpy(), ref[name]
        assert g.dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(w)), (name, where)
        assert torch.equal(torch.from_numpy(np.nan_to_num(g, nan=7.0)), torch.from_numpy(np.nan_to_num(w, nan=7.0))), (name, where)


@pytest.mark.parametrize('n', sorted(SHAPES))
def test_order_statistics_exactly(n):
    import nhmc.kernels as K_
    G, K, S = SHAPES[n]
    for E in ELEMS:
        x, t = cloud(G, K, S, E)
        pooled = x.reshape(G, n, E).numpy()
        xd, td = x.cuda(), t.cuda()
        for k in ranks(n):
            lower, median, upper, summary = K_.credible(xd, td, K, k)
            assert lower.shape == (G, 1, 1, E) and summary.shape == (G, 6) and summary.dtype == torch.float64
            for gi in range(G):
                ref = credible_ref(pooled[gi], t[gi].flatten().numpy(), k)
                same_maps((lower[gi], median[gi], upper[gi]), ref, (n, E, k, gi))
                assert ref['n_nan'] == 0 and summary[gi, 5].item() == 0.0
                assert summary[gi, 3].item() == ref['n_inside'] and summary[gi, 4].item() == ref['n_point'] >= 1


@pytest.mark.parametrize('n', [20, 160])
def test_nan_as_torch_sort_has_it(n):
    """Group 1 of three holds an element with one NaN draw, one with exactly k and one with nothing else: the outputs are
    NaN where the restatement's are, n_nan is exact, the two width figures are NaN, and the other groups do not notice."""
    import nhmc.kernels as K_
    G, K, S, E, k = 3, n // 20, 20, 260, 2
    x, t = cloud(G, K, S, E, planted=False)
    clean = K_.credible(x.cuda(), t.cuda(), K, k)
    pooled = x.reshape(G, n, E)                               # a view
    pooled[1, 5, 10] = float('nan')
    pooled[1, 3, 257], pooled[1, n - 1, 257] = float('nan'), float('nan')
    pooled[1, :, 130] = float('nan')
    got = K_.credible(x.cuda(), t.cuda(), K, k)
    ref = credible_ref(pooled[1].numpy(), t[1].flatten().numpy(), k)
    assert not np.isnan(ref['upper'][10]) and np.isnan(ref['upper'][257]) and not np.isnan(ref['lower'][257])
    assert np.isnan(ref['lower'][130]) and np.isnan(ref['median'][130]) and ref['n_nan'] == 2
    same_maps([m[1] for m in got[:3]], ref, n)
    s = got[3].cpu().numpy()
    assert np.isnan(s[1, 0]) and np.isnan(s[1, 1]) and np.isnan(s[1, 2])
    assert s[1, 3] == ref['n_inside'] and s[1, 4] == ref['n_point'] and s[1, 5] == 2.0
    for gi in (0, 2):
        for a, b in zip(got, clean):
            assert torch.equal(bits(a[gi]), bits(b[gi]))
        assert np.isfinite(s[gi]).all() and s[gi, 5] == 0.0


@pytest.mark.parametrize('n,E', [(20, 260), (20, 768), (160, 260), (160, 768)])
def test_summary(n, E):
    """The three counts and max_width exactly; the two sums within 1e-9 relative of the restatement's float64 sums, the
    bound tests/test_calib_gpu.py holds the same kind of fixed-order fp64 partials to.  Without the original, [2] and [3]
    are NaN and the other four keep their bits."""
    import nhmc.kernels as K_
    G, K, S = 2, n // 20, 20
    x, t = cloud(G, K, S, E, planted=False)
    x[..., 0] = -1.0                                          # a point element whatever k is
    pooled = x.reshape(G, n, E).numpy()
    for k in (1, n // 4, n // 2):
        got = K_.credible(x.cuda(), t.cuda(), K, k)[3].cpu().numpy()
        bare = K_.credible(x.cuda(), None, K, k)[3].cpu().numpy()
        for gi in range(G):
            ref = credible_ref(pooled[gi], t[gi].flatten().numpy(), k)
            print(f'n {n} E {E} k {k} image {gi}:', {name: (float(got[gi, i]), ref[name]) for i, name in enumerate(SUMS)})
            assert ref['n_point'] >= 1 and ref['n_inside'] < E and ref['max_width'] > 0
            for i, name in enumerate(SUMS):
                if name in ('sum_width', 'sum_err2_median'):
                    assert abs(got[gi, i] - ref[name]) <= 1e-9 * abs(ref[name]), name
                else:
                    assert got[gi, i] == ref[name], name
        assert np.isnan(bare[:, 2]).all() and np.isnan(bare[:, 3]).all()
        assert np.array_equal(bare[:, [0, 1, 4, 5]].view(np.int64), got[:, [0, 1, 4, 5]].view(np.int64))


@pytest.mark.parametrize('n', [20, 160])
def test_it_is_the_interval_calibration_speaks_of(n):
    import nhmc.kernels as K_
    from nhmc import metrics
    G, K, S, C, H, W = 2, n // 20, 20, 3, 16, 16
    g = torch.Generator().manual_seed(11 + n)
    x = (0.2 * torch.randn(G * K, S, C, H, W, generator=g)).cuda()
    t = (0.2 * torch.randn(G, C, H, W, generator=g)).cuda()
    for level in (0.5, 0.8, 0.9):
        cal = metrics.calibration(x, t, replicas=K, level=level)
        assert (cal['n_tied'] == 0).all()                     # tie-free: every element has a rank
        got = metrics.credible(x, t, replicas=K, level=level)
        k = metrics.coverage_rank(n, level)
        assert tuple(got) == ('lower', 'median', 'upper') + metrics.CREDIBLE_KEYS and (got['ci_rank'] == k).all()
        raw = K_.credible(x, t, K, k)[3].cpu().numpy()
        for gi in range(G):
            inside = int(cal['hist'][gi][k:n - k + 1].sum())
            assert int(raw[gi, 3]) == inside and raw[gi, 3] == float(inside)
        assert np.array_equal(got['ci_level'], cal['coverage_nominal']) and np.array_equal(got['ci_inside'], cal['coverage'])


@pytest.mark.parametrize('n', [20, 64])
def test_both_paths_return_the_same_bits(n, monkeypatch):
    import nhmc.kernels as K_
    G, K, S = SHAPES[n]
    x, t = cloud(G, K, S, 260)
    pooled = x.reshape(G, n, 260).numpy()
    xd, td = x.cuda(), t.cuda()
    for k in (1, 3, n // 2):
        monkeypatch.setenv('NHMC_CREDIBLE_PATH', 'register')
        reg = K_.credible(xd, td, K, k)
        monkeypatch.setenv('NHMC_CREDIBLE_PATH', 'general')
        gen = K_.credible(xd, td, K, k)
        monkeypatch.delenv('NHMC_CREDIBLE_PATH')
        for a, b in zip(reg, gen):
            assert torch.equal(bits(a), bits(b))
        for gi in range(G):                                   # and the general path is right where the other one serves
            same_maps([m[gi] for m in gen[:3]], credible_ref(pooled[gi], None, k), (n, k, gi))


@pytest.mark.parametrize('n', [20, 160])
def test_nothing_outside_the_buffers_is_written(n):
    """Outputs, summary and workspace sit inside larger buffers filled with a sentinel (E = 260: a partial second tile);
    the sentinel survives around them, and a second call returns equal bits."""
    import nhmc
    lib = nhmc._lib.load()
    G, K, S, E, k, pad, mark = 2, n // 20, 20, 260, 2, 64, 12345.0
    x, t = cloud(G, K, S, E)
    xd, td = x.cuda(), t.cuda()
    n_ws = lib.nhmc_credible_ws_bytes(G, E) // 8
    assert n_ws == G * 2 * 8
    P = lambda ten: ctypes.c_void_p(ten.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        maps = [torch.full((G * E + 2 * pad,), mark, dtype=torch.float32, device='cuda') for _ in range(3)]
        summary = torch.full((G * 6 + 2 * pad,), mark, dtype=torch.float64, device='cuda')
        ws = torch.full((n_ws + 2 * pad,), mark, dtype=torch.float64, device='cuda')
        inner = [m[pad:pad + G * E] for m in maps] + [summary[pad:pad + G * 6], ws[pad:pad + n_ws]]
        assert lib.nhmc_credible(P(xd), P(td), *[P(i) for i in inner], G, K, S, E, k, stream) == 0
        torch.cuda.synchronize()
        for buf in maps + [summary, ws]:
            assert (buf[:pad] == mark).all() and (buf[-pad:] == mark).all()
        return [i.clone() for i in inner[:4]]
    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    pooled = x.reshape(G, n, E).numpy()
    for gi in range(G):
        same_maps([m.reshape(G, E)[gi] for m in first[:3]], credible_ref(pooled[gi], None, k), (n, gi))


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(bits(a[k]), bits(b[k])), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_summarize_carries_the_interval():
    from nhmc import metrics
    G, K, S, C, H, W = 2, 3, 4, 3, 16, 16
    g = torch.Generator().manual_seed(7)
    orig = (torch.rand(G, C, H, W, generator=g) * 1.6 - 0.8).contiguous()
    samples = (orig.repeat_interleave(K, dim=0)[:, None] + 0.2 * torch.randn(G * K, S, C, H, W, generator=g)).contiguous()
    samples, orig = samples.cuda(), orig.cuda()
    per_chain = orig.repeat_interleave(K, dim=0)
    new = ('lower', 'median', 'upper') + metrics.CREDIBLE_KEYS
    for kw in (dict(replicas=K), dict(replicas=K, calibration=0.8), dict(), dict(calibration=0.9)):
        x_o = orig if 'replicas' in kw else per_chain
        plain = metrics.summarize(samples, x_o, **kw)
        out = metrics.summarize(samples, x_o, credible=0.9, **kw)
        assert list(out) == list(plain) + list(new) and not set(new) & set(plain)     # after all others
        _same(plain, {k: out[k] for k in plain})                                    # which keep their bits
        _same(metrics.credible(samples, x_o, replicas=kw.get('replicas', 1), level=0.9), {k: out[k] for k in new})
        assert out['lower'].shape == (x_o.shape[0], C, H, W) and (out['ci_rank'] == 1).all()
        assert (out['ci_level'] == (11.0 / 13.0 if 'replicas' in kw else 3.0 / 5.0)).all()
        _same(plain, metrics.summarize(samples, x_o, credible=None, **kw))            # None is omitting it
    # fewer than two pooled samples: the keys are there, without values
    one = metrics.summarize(samples[:, :1].contiguous(), per_chain, credible=0.9)
    assert one['lower'] is None and one['median'] is None and one['upper'] is None
    assert all(np.isnan(one[k]).all() and one[k].shape == (G * K,) for k in metrics.CREDIBLE_KEYS)
    assert np.isfinite(one['psnr_mean']).all() and list(one)[-len(new):] == list(new)


CLI_ARGS = ['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05', '--tau', '0.1',
            '--epsilon', '0.05', '--synthetic', '2', '--chains', '4', '--replicas', '2', '--philox', '--hmc_epochs', '4',
            '--hmc_sampling', '6', '--save_images', '--calibration']


def _check_rows(rows, cli, E):
    for r in rows:
        if r['ci_rank'] is None:
            assert all(r[k] is None for k in cli.CREDIBLE_COLUMNS)
            continue
        assert isinstance(r['ci_rank'], int) and isinstance(r['n_point'], int) and isinstance(r['n_nan'], int)
        assert r['ci_level'] == r['coverage_nominal'] and r['n_nan'] == 0
        if r['n_tied'] == 0:
            assert r['ci_inside'] == r['coverage']
        else:                                                  # a tied element is inside, and has no rank
            assert r['ci_inside'] >= r['coverage'] * (1 - r['n_tied'] / E)
        assert np.isfinite(r['psnr_of_median']) and 0.0 <= r['ci_width_mean'] <= r['ci_width_max'] <= 1.0


def test_cli_reports_the_credible_interval(tmp_path, monkeypatch, capsys):
    import yaml
    from PIL import Image
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)
    out_dir, report = tmp_path / 'out', tmp_path / 'report' / 'metrics.json'
    cli.main(CLI_ARGS + ['-i', str(out_dir), '--metrics_out', str(report), '--credible'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    for s in (0, 1):
        line = [ln for ln in stdout.splitlines() if ln.startswith(f'image {s}: credible interval: ')]
        assert len(line) == 1 and 'order statistics 1 and 12 of 12 draws (level 0.8462)' in line[0]
        assert ', width mean ' in line[0] and ', original inside ' in line[0] and ', PSNR of the median ' in line[0]
        assert ', point elements ' in line[0]
    assert len([ln for ln in stdout.splitlines() if ln.startswith('Total Average credible interval: ')]) == 1
    assert len(rows) == 2 and [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert tuple(r) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS
        assert r['n_samples'] == 12 and r['ci_rank'] == 1
    _check_rows(rows, cli, 3 * 32 * 32)
    for s in (0, 1):
        for name in (f'{s}_median.png', f'{s}_lower.png', f'{s}_upper.png', f'ci_width_map_{s}.png', f'{s}_mean.png'):
            assert Image.open(os.path.join(out_dir, name)).size == (32, 32), name
    # without the flag: the former columns, no such line, no such picture
    out2, report2 = tmp_path / 'out2', tmp_path / 'report2.json'
    cli.main(CLI_ARGS + ['-i', str(out2), '--metrics_out', str(report2)])
    stdout2, rows2 = capsys.readouterr().out, json.loads(report2.read_text())
    assert 'credible' not in stdout2 and 'image 0: calibration: ' in stdout2
    assert all(tuple(r) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS for r in rows2)
    assert not os.path.exists(out2 / '0_median.png') and not os.path.exists(out2 / 'ci_width_map_0.png')


def test_latent_cli_reports_the_credible_interval(tmp_path, monkeypatch, capsys):
    """The latent entry on the small latent config of test_diag_gpu.py's latent CLI test, one chain per image."""
    import yaml
    from PIL import Image
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
            '--save_images', '--calibration', '0.8']
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    cli.main_latent(args + ['-i', str(out_dir), '--metrics_out', str(report), '--credible', '0.8'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    assert [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS
        s, n = r['image'], r['n_samples']
        line = [ln for ln in stdout.splitlines() if ln.startswith(f'image {s}: credible interval: ')]
        if n >= 2:
            k = min(n // 2, max(1, int(np.floor((1 - 0.8) / 2 * (n + 1) + 0.5))))
            assert r['ci_rank'] == k and r['ci_level'] == (n + 1 - 2 * k) / (n + 1.0)
            assert len(line) == 1 and f'order statistics {k} and {n + 1 - k} of {n} draws (level {r["ci_level"]:.4f})' in line[0]
            for name in (f'{s}_median.png', f'{s}_lower.png', f'{s}_upper.png', f'ci_width_map_{s}.png'):
                assert Image.open(os.path.join(out_dir, name)).size == (64, 64), name
        else:
            assert r['ci_rank'] is None and not line and not os.path.exists(out_dir / f'{s}_median.png')
    _check_rows(rows, cli, 3 * 64 * 64)
    assert len([ln for ln in stdout.splitlines() if ln.startswith('Total Average credible interval: ')]) == 1
    out2, report2 = tmp_path / 'out2', tmp_path / 'metrics2.json'
    cli.main_latent(args + ['-i', str(out2), '--metrics_out', str(report2)])
    stdout2, rows2 = capsys.readouterr().out, json.loads(report2.read_text())
    assert 'credible' not in stdout2 and all(tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS for r in rows2)

"""GPU: the report stage (nhmc.metrics on csrc/metrics.hip) against float64 restatements of the reference's definitions
(main_sampling.py:488-561): SSIM, PSNR, the posterior-mean image and the std map, `summarize`, and the CLI's report.

Inputs are smooth random images plus noise.  Every chain has its own original and the originals differ, so a wrong
sample -> original index shows."""
import json
import os

import numpy as np
import pytest
import torch

from test_metrics_cpu import ssim_float64

pytestmark = pytest.mark.gpu


def unit(v):
    return ((v.float() + 1.0) / 2.0).clamp(0.0, 1.0)


_BLOCKS = {}


def block(shape):
    """-> (samples [B, S, C, H, W], x_orig [B, C, H, W]) float32 on the host, made once per shape and left unchanged: a
    smooth original per chain (a 4 x 4 grid, bicubically enlarged, reaching past 1 so the clamp acts) plus noise
    whose amplitude grows along the rows, so the std map has a range."""
    if shape not in _BLOCKS:
        B, S, C, H, W = shape
        g = torch.Generator().manual_seed(1000 * H + W + S)
        low = torch.rand(B, C, 4, 4, generator=g) * 1.7 - 0.5
        orig = torch.nn.functional.interpolate(low, size=(H, W), mode='bicubic', align_corners=True)
        amp = torch.linspace(0.05, 0.4, H)[:, None].expand(H, W)
        samples = orig[:, None] + amp * torch.randn(B, S, C, H, W, generator=g)
        _BLOCKS[shape] = (samples.contiguous(), orig.contiguous())
    return _BLOCKS[shape]


def dev(t):
    return t.to('cuda')


SSIM_SHAPES = [(1, 1, 1, 7, 8),          # a single row of two windows
               (2, 3, 3, 24, 28),        # ragged against the 16 x 32 tile
               (2, 2, 3, 40, 72),        # several tiles in both directions, ragged edges
               (1, 2, 3, 256, 256)]      # the workload's plane


@pytest.mark.parametrize('shape', SSIM_SHAPES)
def test_ssim_matches_the_float64_definition(shape):
    """1e-9 absolute: both sides are fp64 arithmetic on exact products; only the summation order differs."""
    from nhmc import metrics
    samples, orig = block(shape)
    B, S = shape[:2]
    rng = unit(samples).flatten(2)
    assert float((rng.max(2).values - rng.min(2).values).min()) >= 0.5
    got = metrics.ssim(dev(samples), dev(orig))
    assert got.shape == (B, S) and got.dtype == torch.float64
    want = torch.tensor([[ssim_float64(samples[b, s], orig[b]) for s in range(S)] for b in range(B)], dtype=torch.float64)
    err = float((got.cpu() - want).abs().max())
    print(f'ssim {shape}: max |gpu - float64| = {err:.3e}')
    assert err <= 1e-9
    if B > 1:       # the originals differ enough that chain 1 against chain 0's original would not pass
        assert abs(ssim_float64(samples[1, 0], orig[0]) - float(want[1, 0])) > 1e-3
    assert torch.equal(metrics.ssim(dev(samples), dev(orig)), got)                     # same bits on a second call


@pytest.mark.parametrize('key', ['a', 'b'])
def test_ssim_matches_the_reference_float32_path(golden, key):
    """G19: the reference's float32 path (a restatement of skimage's, tools/gen_golden_ssim.py) to 1e-6."""
    from nhmc import metrics
    g = golden('g19_ssim.npz')
    x, y = torch.from_numpy(g[f'x_{key}']), torch.from_numpy(g[f'y_{key}'])
    got = float(metrics.ssim(dev(x[None]), dev(y[None]))[0])                           # the one-chain form
    print(f'ssim G19 {key}: gpu - float32 path = {got - float(g[f"ssim32_{key}"]):+.3e}, '
          f'gpu - float64 = {got - float(g[f"ssim64_{key}"]):+.3e}')
    assert abs(got - float(g[f'ssim32_{key}'])) <= 1e-6
    from nhmc import kernels as K
    assert float(K.sample_range(dev(x[None, None]))[0, 0]) == float(g[f'range_{key}'])


@pytest.mark.parametrize('shape', [(2, 3, 3, 16, 16), (1, 20, 3, 64, 64)])
def test_psnr_has_the_bits_of_the_per_sample_kernel(shape):
    from nhmc import metrics
    import nhmc.kernels as K
    samples, orig = (dev(t) for t in block(shape))
    B, S = shape[:2]
    got = metrics.psnr(samples, orig)
    want = torch.stack([torch.stack([K.psnr(samples[b, s:s + 1].contiguous(), orig[b:b + 1])[0] for s in range(S)])
                        for b in range(B)])
    assert got.shape == (B, S) and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(metrics.psnr(samples, orig), got)
    assert torch.equal(metrics.psnr(samples[0], orig[:1]), got[0])                     # the one-chain form


@pytest.mark.parametrize('shape', [(2, 2, 3, 8, 8), (2, 3, 3, 40, 72), (1, 20, 3, 64, 64)])
def test_sample_moments(shape):
    from nhmc import metrics
    samples, _ = block(shape)
    B, S, C, H, W = shape
    mean, std_map, norm = metrics.sample_moments(dev(samples))
    assert mean.shape == (B, C, H, W) and std_map.shape == (B, H, W) and norm.shape == (B, H, W)
    # one fp32 ulp on [-1, 1] around the float64 mean rounded to fp32
    want_mean = samples.double().mean(1).float()
    err_mean = float((mean.cpu() - want_mean).abs().max())
    want_std = unit(samples).double().std(dim=1, unbiased=True).mean(dim=1)
    err_std = float((std_map.cpu().double() - want_std).abs().max())
    lo, hi = want_std.flatten(1).min(1).values, want_std.flatten(1).max(1).values
    assert float((hi - lo).min()) >= 0.05
    want_norm = (want_std - lo[:, None, None]) / (hi - lo)[:, None, None]
    err_norm = float((norm.cpu().double() - want_norm).abs().max())
    print(f'moments {shape}: mean {err_mean:.3e}  std map {err_std:.3e}  normalised {err_norm:.3e}')
    assert err_mean <= 1.2e-7 and err_std <= 1e-6 and err_norm <= 1e-5
    assert float(norm.min()) == 0.0 and float(norm.max()) == 1.0
    again = metrics.sample_moments(dev(samples))
    assert all(torch.equal(a, b) for a, b in zip(again, (mean, std_map, norm)))


def test_summarize():
    from nhmc import metrics
    shape = (2, 3, 3, 24, 28)
    samples, orig = (dev(t) for t in block(shape))
    out = metrics.summarize(samples, orig)
    ps = metrics.psnr(samples, orig).double().cpu().numpy()
    ss = metrics.ssim(samples, orig).cpu().numpy()
    assert np.array_equal(out['psnr_mean'], ps.mean(axis=1)) and np.array_equal(out['psnr_std'], ps.std(axis=1, ddof=1))
    assert np.array_equal(out['ssim_mean'], ss.mean(axis=1)) and np.array_equal(out['ssim_std'], ss.std(axis=1, ddof=1))
    mean, std_map, norm = metrics.sample_moments(samples)
    assert torch.equal(out['mean'], mean) and torch.equal(out['std_map'], std_map)
    assert torch.equal(out['std_map_normalised'], norm) and out['n_samples'] == 3
    assert np.array_equal(out['std_map_min'], std_map.flatten(1).min(1).values.double().cpu().numpy())
    assert np.array_equal(out['std_map_max'], std_map.flatten(1).max(1).values.double().cpu().numpy())
    # one sample of one chain: PSNR and SSIM, but no map
    one = metrics.summarize(samples[1, :1], orig[1:2])
    assert one['n_samples'] == 1 and one['mean'] is None and one['std_map'] is None and one['std_map_normalised'] is None
    assert one['psnr_mean'][0] == ps[1, 0] and one['ssim_mean'][0] == ss[1, 0]
    assert one['psnr_std'][0] == 0.0 and one['ssim_std'][0] == 0.0
    assert np.isnan(one['std_map_min'][0]) and np.isnan(one['std_map_max'][0])
    # no sample: the NaN row
    none = metrics.summarize(samples[1, :0], orig[1:2])
    assert none['n_samples'] == 0 and none['mean'] is None
    assert np.isnan(none['psnr_mean'][0]) and np.isnan(none['ssim_mean'][0]) and np.isnan(none['std_map_min'][0])
    assert none['psnr_std'][0] == 0.0 and none['ssim_std'][0] == 0.0


def test_cli_reports_ssim_and_the_std_map(tmp_path, monkeypatch, capsys):
    import yaml
    from PIL import Image
    from nhmc import cli
    cfgdir = tmp_path / 'configs'
    cfgdir.mkdir()
    cfg = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True},
           'model': dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True,
                         class_cond=False, use_checkpoint=False, attention_resolutions='16', num_heads=4,
                         num_head_channels=16, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0.0,
                         resblock_updown=True, use_fp16=False, use_new_attention_order=False, model_path=''),
           'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}
    (cfgdir / 'config_tiny.yml').write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    out_dir, report = tmp_path / 'out', tmp_path / 'report' / 'metrics.json'
    table = cli.main(['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05',
                      '-i', str(out_dir), '--tau', '0.1', '--epsilon', '0.05', '--synthetic', '2', '--chains', '2',
                      '--philox', '--metrics_out', str(report), '--save_images'])
    stdout = capsys.readouterr().out
    assert 'Total Average PSNR' in stdout and 'Total Average SSIM: ' in stdout
    assert 'image 0: SSIM ' in stdout and 'image 1: SSIM ' in stdout
    rows = json.loads(report.read_text())
    assert len(rows) == 2 and [r['image'] for r in rows] == [0, 1]
    for r, (idx, mean, std) in zip(rows, table.tolist()):
        assert np.isfinite(r['ssim_mean']) and -1.0 <= r['ssim_mean'] <= 1.0
        assert r['std_map_max'] >= r['std_map_min'] >= 0.0
        assert r['image'] == int(idx) and np.float32(r['psnr_mean']) == np.float32(mean)
        assert np.float32(r['psnr_std']) == np.float32(std) and r['n_samples'] == 20
    for name in ('std_dev_map_0.png', 'std_dev_map_1.png', '0_mean.png', '1_mean.png'):
        assert Image.open(os.path.join(out_dir, name)).size == (32, 32)

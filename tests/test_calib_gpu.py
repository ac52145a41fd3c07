"""GPU: calibration of the posterior samples -- the kernel (nhmc_calibration, csrc/calibration.hip) against the two-pass
float64 restatement of its definition in tests/test_calib_cpu.py, its argument validation, the statistic on an ensemble
whose answer is known, `metrics.summarize` carrying it, and the two CLIs' calibration report."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_calib_cpu import SUMS, calib_float64, sums_of
from test_diag_gpu import TINY

pytestmark = pytest.mark.gpu

CALIB_SHAPES = [(2, 3, 20, 3, 8, 8),        # the workload's S, pooling over replicas, group indexing, one partial tile
                (1, 1, 2, 1, 4, 4),         # the minimum n
                (1, 1, 7, 1, 8, 8),         # n that is no multiple of any unroll
                (2, 8, 20, 3, 16, 16),      # n = 160, three tiles per image
                (1, 1, 65, 1, 8, 12),       # n = 65
                (1, 16, 64, 1, 4, 4)]       # the cap, n = 1024, a 1025-bin histogram


def cloud(G, K, S, C, H, W, seed=4321):
    """-> (x float32 [G * K, S, C, H, W], t float32 [G, C, H, W]) on the host: per element a cloud of width amp (1e-4 to
    0.3 along the elements) about a base in [-0.8, 0.8], each replica offset by half a width, the original 1.3 widths from
    the base, all clamped to [-1, 1]; then the special elements: 3 flat and tied, 5 and 6 flat with the original elsewhere,
    9 tied with the first draw of replica 0, 11 and 12 with the original at the clamp."""
    g = torch.Generator().manual_seed(seed)
    E, f64 = C * H * W, torch.float64
    amp = torch.logspace(-4, -0.5, E, dtype=f64)
    base = torch.rand(G, 1, 1, E, generator=g, dtype=f64) * 1.6 - 0.8
    off = 0.5 * amp * torch.randn(G, K, 1, E, generator=g, dtype=f64)
    x = (base + off + amp * torch.randn(G, K, S, E, generator=g, dtype=f64)).clamp(-1, 1).float()
    t = (base[:, 0, 0] + 1.3 * amp * torch.randn(G, E, generator=g, dtype=f64)).clamp(-1, 1).float()
    x[..., 3], t[:, 3] = 1.0, 1.0
    x[..., 5], t[:, 5] = 1.0, 0.5
    x[..., 6], t[:, 6] = -1.0, -0.25
    t[:, 9] = x[:, 0, 0, 9]
    t[:, 11], t[:, 12] = -1.0, 1.0
    return x.reshape(G * K, S, C, H, W).contiguous(), t.reshape(G, C, H, W).contiguous()


def ulp32(v):
    return np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)


def same_bits(a, b):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize('shape', CALIB_SHAPES)
def test_calibration_matches_the_float64_definition(shape):
    """Counts, histogram, n_tied and n_flat exactly.  z: NaN, +inf and -inf at the same places, finite values within 1 ulp
    of fp32 of the restatement rounded to fp32 or 1e-9 absolute (both sides are fp64 and differ in summation order only).
    The eight sums, and the figures derived from them, 1e-9 relative.  A second call returns equal bits."""
    import nhmc.kernels as K_
    from nhmc import metrics
    G, K, S, C, H, W = shape
    E, n = C * H * W, K * S
    x, t = cloud(*shape)
    xd, td = x.cuda(), t.cuda()
    got = metrics.calibration(xd, td, replicas=K, level=0.9)
    raw = K_.calibration(xd, td, K)
    assert got['z'].shape == (G, C, H, W) and got['z'].dtype == torch.float32
    assert got['below'].dtype == torch.int32 and got['equal'].dtype == torch.int32 and got['below'].shape == (G, C, H, W)
    assert got['hist'].shape == (G, n + 1) and got['hist'].dtype == np.int64
    assert raw[2].dtype == torch.int64 and np.array_equal(raw[2].cpu().numpy(), got['hist'])
    sums = raw[3].cpu().numpy()
    pooled, truth = x.reshape(G, n, E).numpy(), t.reshape(G, E).numpy()
    for gi in range(G):
        want = calib_float64(pooled[gi], truth[gi])
        smin = want['s'][want['s'] > 0].min()
        print(f'calibration {shape} image {gi}: tied {want["n_tied"]} flat {want["n_flat"]} end bins {want["hist"][0]} '
              f'{want["hist"][-1]} smallest s > 0 {smin:.2e}')
        # what the recipe is for (2 to 9 tied elements over these shapes: 3 and 9, and where a clamped draw meets a clamped original)
        assert want['n_flat'] == 3 and want['n_tied'] >= 2 and want['hist'][0] > 0 and want['hist'][-1] > 0
        assert np.array_equal(got['below'][gi].flatten().cpu().numpy(), want['below'])
        assert np.array_equal(got['equal'][gi].flatten().cpu().numpy(), want['equal'])
        assert np.array_equal(got['hist'][gi], want['hist'])
        assert got['n_tied'][gi] == want['n_tied'] and got['n_flat'][gi] == want['n_flat']
        z, wz = got['z'][gi].flatten().cpu().numpy().astype(np.float64), want['z']
        assert np.array_equal(np.isnan(z), np.isnan(wz)) and np.isnan(wz[3])
        assert np.array_equal(np.isposinf(z), np.isposinf(wz)) and np.isposinf(wz[6])
        assert np.array_equal(np.isneginf(z), np.isneginf(wz)) and np.isneginf(wz[5])
        fin = np.isfinite(wz)
        w32 = wz[fin].astype(np.float32)
        err = np.abs(z[fin] - w32.astype(np.float64))
        print(f'  z: max error {(err / ulp32(w32)).max():.2f} ulp over {int(fin.sum())} finite elements')
        assert ((err <= ulp32(w32)) | (err <= 1e-9)).all()
        for i, name in enumerate(SUMS):
            g_, w_ = float(sums[gi, i]), float(want[name])
            print(f'  {name}: {g_!r} against {w_!r}')
            assert g_ == w_ or abs(g_ - w_) <= 1e-9 * abs(w_), name
        derived = metrics.calibration_from_sums(sums_of(want), want['hist'][None], E, 0.9)
        for name in metrics.CALIBRATION_KEYS:
            g_, w_ = float(got[name][gi]), float(derived[name][0])
            print(f'  {name}: {g_!r} against {w_!r}')
            assert g_ == w_ or abs(g_ - w_) <= 1e-9 * abs(w_), name
    same_bits(metrics.calibration(xd, td, replicas=K, level=0.9), got)
    again = K_.calibration(xd, td, K)
    assert torch.equal(again[1], raw[1]) and torch.equal(again[2], raw[2])
    assert torch.equal(again[3].view(torch.int64), raw[3].view(torch.int64))


def test_argument_validation():
    """Through the C ABI with pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ok = (2, 2, 20, 1024, null)                                               # groups, replicas, samples, n_elem, stream
    ARG, ALIGN, SHAPE = 1, 2, 3
    all16 = [a16] * 7                                                         # samples, x_orig, z, counts, hist, summary, ws
    for i in range(7):                                                        # each pointer in turn
        ptrs = list(all16)
        ptrs[i] = null
        assert lib.nhmc_calibration(*ptrs, *ok) == ARG
    assert lib.nhmc_calibration(*all16, 0, 2, 20, 1024, null) == ARG
    assert lib.nhmc_calibration(*all16, 2, 0, 20, 1024, null) == ARG
    assert lib.nhmc_calibration(*all16, 2, 2, 0, 1024, null) == ARG
    assert lib.nhmc_calibration(*all16, 2, 2, 20, 0, null) == ARG
    assert lib.nhmc_calibration(*all16, -1, 2, 20, 1024, null) == ARG
    for i in range(4):                                                        # the four bases that take vector accesses
        ptrs = list(all16)
        ptrs[i] = a4
        assert lib.nhmc_calibration(*ptrs, *ok) == ALIGN
    assert lib.nhmc_calibration(*all16, 2, 2, 20, 1022, null) == ALIGN       # n_elem % 4
    assert lib.nhmc_calibration(*all16, 2, 1, 1, 1024, null) == SHAPE        # K * S = 1
    assert lib.nhmc_calibration(*all16, 2, 25, 41, 1024, null) == SHAPE      # K * S = 1025
    assert lib.nhmc_calibration(*all16, 2, 1, 1025, 1024, null) == SHAPE
    assert lib.nhmc_calibration(*all16, 65536, 2, 20, 1024, null) == SHAPE   # groups ride in gridDim.y
    assert lib.nhmc_calibration(a4, *all16[1:], 2, 1, 1, 1024, null) == ALIGN            # ALIGN before SHAPE
    assert lib.nhmc_calibration(null, *all16[1:], 2, 1, 1, 1022, null) == ARG            # ARG before both
    assert lib.nhmc_calibration_tiles(3 * 256 * 256) == 768 and lib.nhmc_calibration_tiles(64) == 1
    assert lib.nhmc_calibration_tiles(257) == 2 and lib.nhmc_calibration_tiles(0) == 0
    assert lib.nhmc_calibration_ws_bytes(8, 3 * 256 * 256) == 8 * 768 * 8 * 8 and lib.nhmc_calibration_ws_bytes(0, 64) == 0
    assert lib.nhmc_calibration_ws_bytes(1, 16) == 64 and lib.nhmc_calibration_ws_bytes(3, 0) == 0
    # the binding's own shape checks
    import nhmc.kernels as K
    with pytest.raises(nhmc._lib.NhmcError, match='multiple'):
        K.calibration(torch.zeros(3, 4, 1, 4, 4, device='cuda'), torch.zeros(1, 1, 4, 4, device='cuda'), 2)
    with pytest.raises(nhmc._lib.NhmcError, match='does not match'):
        K.calibration(torch.zeros(4, 4, 1, 4, 4, device='cuda'), torch.zeros(4, 1, 4, 4, device='cuda'), 2)
    with pytest.raises(nhmc._lib.NhmcError, match='no CPU path'):
        K.calibration(torch.zeros(2, 4, 1, 4, 4), torch.zeros(2, 1, 4, 4), 1)
    with pytest.raises(nhmc._lib.NhmcError, match='status 3'):
        K.calibration(torch.zeros(2, 1, 1, 4, 4, device='cuda'), torch.zeros(2, 1, 4, 4, device='cuda'), 1)


def test_exchangeable_ensemble_is_calibrated_and_a_narrow_one_is_not():
    """21 exchangeable rows, row 0 the truth: a flat rank histogram (every bin within 5 binomial standard deviations of
    E / 21, which the restatement meets on its own), coverage within 4 standard errors of nominal, spread / skill within
    0.05 of 1.  The same draws shrunk by half about zero are over-confident: coverage more than 0.1 below nominal and
    spread / skill below 0.7."""
    from nhmc import metrics
    n, C, H, W = 20, 3, 64, 64
    E = C * H * W
    x = 0.2 * torch.randn(n + 1, E, generator=torch.Generator().manual_seed(2024))
    truth, draws = x[0].reshape(1, C, H, W).contiguous(), x[1:].reshape(1, n, C, H, W).contiguous()
    ref = calib_float64(x[1:].numpy(), x[0].numpy())
    expect, sd = E / 21.0, np.sqrt(E / 21.0 * (1 - 1 / 21.0))
    assert ref['n_tied'] == 0 and ref['n_flat'] == 0 and (np.abs(ref['hist'] - expect) < 5 * sd).all()
    got = metrics.calibration(draws.cuda(), truth.cuda(), level=0.9)
    nominal = 19.0 / 21.0
    print('exchangeable:', {k: float(got[k][0]) for k in metrics.CALIBRATION_KEYS},
          'largest bin deviation in sd', float(np.abs(got['hist'][0] - expect).max() / sd))
    assert got['n_tied'][0] == 0 and got['n_flat'][0] == 0 and got['hist'][0].sum() == E
    assert np.array_equal(got['hist'][0], ref['hist']) and (np.abs(got['hist'][0] - expect) < 5 * sd).all()
    assert got['coverage_nominal'][0] == nominal
    assert abs(got['coverage'][0] - nominal) < 4 * np.sqrt(nominal * (1 - nominal) / E)
    assert abs(got['spread_skill'][0] - 1.0) < 0.05
    narrow = metrics.calibration((0.5 * draws).cuda(), truth.cuda(), level=0.9)
    print('narrow:', {k: float(narrow[k][0]) for k in metrics.CALIBRATION_KEYS})
    assert narrow['coverage'][0] < nominal - 0.1 and narrow['spread_skill'][0] < 0.7


def test_summarize_carries_the_calibration():
    from nhmc import metrics
    G, K, S, C, H, W = 2, 3, 4, 3, 16, 16
    g = torch.Generator().manual_seed(7)
    orig = (torch.rand(G, C, H, W, generator=g) * 1.6 - 0.8).contiguous()
    samples = (orig.repeat_interleave(K, dim=0)[:, None] + 0.2 * torch.randn(G * K, S, C, H, W, generator=g)).contiguous()
    samples, orig = samples.cuda(), orig.cuda()
    new = ('z', 'below', 'equal', 'hist') + metrics.CALIBRATION_KEYS
    # replicas = 3: the pooled n is 3 * S, and everything else is what the call without the flag returns
    out = metrics.summarize(samples, orig, replicas=K, calibration=0.9)
    plain = metrics.summarize(samples, orig, replicas=K)
    cal = metrics.calibration(samples, orig, replicas=K, level=0.9)
    assert out['n_samples'] == K * S and out['hist'].shape == (G, K * S + 1) and out['coverage_nominal'][0] == 11.0 / 13.0
    assert list(out) == list(plain) + list(new) and not set(new) & set(plain)
    same_bits({k: out[k] for k in new}, cal)
    same_bits(plain, {k: out[k] for k in plain})
    # one chain per image
    per_chain = orig.repeat_interleave(K, dim=0)
    out = metrics.summarize(samples, per_chain, calibration=0.5)
    cal = metrics.calibration(samples, per_chain, level=0.5)
    assert out['hist'].shape == (G * K, S + 1) and out['coverage_nominal'][0] == 3.0 / 5.0 and 'rhat' not in out
    same_bits({k: out[k] for k in new}, cal)
    # calibration=None: today's result, keys and bits -- against a call that omits the argument
    for kw in (dict(), dict(replicas=K)):
        x_o = orig if kw else per_chain
        a, b = metrics.summarize(samples, x_o, **kw), metrics.summarize(samples, x_o, calibration=None, **kw)
        assert list(a) == list(b) and 'coverage' not in a and 'z' not in a
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert torch.equal(a[k], b[k])
            elif isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k], equal_nan=True)
            else:
                assert a[k] == b[k]
    # fewer than two pooled samples: the keys are there, without values
    one = metrics.summarize(samples[:, :1].contiguous(), per_chain, calibration=0.9)
    assert one['z'] is None and one['hist'] is None and np.isnan(one['coverage']).all() and np.isnan(one['n_flat']).all()
    assert np.isfinite(one['psnr_mean']).all()


def test_cli_reports_calibration(tmp_path, monkeypatch, capsys):
    import yaml
    from PIL import Image
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)
    out_dir, report = tmp_path / 'out', tmp_path / 'report' / 'metrics.json'
    cli.main(['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05',
              '-i', str(out_dir), '--tau', '0.1', '--epsilon', '0.05', '--synthetic', '2', '--chains', '4',
              '--replicas', '2', '--philox', '--hmc_epochs', '4', '--hmc_sampling', '6',
              '--metrics_out', str(report), '--save_images', '--calibration'])
    stdout, rows = capsys.readouterr().out, json.loads(report.read_text())
    for s in (0, 1):
        line = [ln for ln in stdout.splitlines() if ln.startswith(f'image {s}: calibration: coverage ')]
        assert len(line) == 1 and ' at nominal 0.8462, spread/skill ' in line[0] and ', z rms ' in line[0]
        assert ', |err|~std r ' in line[0] and ', PSNR of the posterior mean ' in line[0] and ', tied ' in line[0]
        assert f'image {s}: R-hat max ' in stdout
    assert len([ln for ln in stdout.splitlines() if ln.startswith('Total Average calibration: coverage ')]) == 1
    assert len(rows) == 2 and [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert set(r) == set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS) | set(cli.CALIBRATION_COLUMNS)
        assert tuple(r) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS
        assert r['n_samples'] == 12 and 0.0 <= r['coverage'] <= 1.0 and r['coverage_nominal'] == 11.0 / 13.0
        assert isinstance(r['n_tied'], int) and isinstance(r['n_flat'], int)
        assert r['psnr_of_mean'] >= r['psnr_mean']                           # the mean of the samples never scores below their average
        assert np.isfinite(r['spread_skill']) and np.isfinite(r['z_rms']) and -1.0 <= r['err_std_corr'] <= 1.0
    for s in (0, 1):
        assert Image.open(os.path.join(out_dir, f'calibration_map_{s}.png')).size == (32, 32)
        assert Image.open(os.path.join(out_dir, f'std_dev_map_{s}.png')).size == (32, 32)


def test_latent_cli_reports_calibration(tmp_path, monkeypatch, capsys):
    """The latent entry with the flag on the small latent config of test_diag_gpu.py's latent CLI test, one chain per
    image: the rows carry the columns, finite where two samples or more were collected."""
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
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    cli.main_latent(['--dataset', 'tiny', '--algo', 'hmc_latent', '--timesteps', '3', '--deg', 'inpaint_random',
                     '--sigma_0', '0.05', '-i', str(out_dir), '--tau', '0.1', '--epsilon', '0.1', '--sigma_y', '1.0',
                     '--synthetic', '2', '--chains', '2', '--philox', '--metrics_out', str(report), '--calibration', '0.8'])
    stdout = capsys.readouterr().out
    rows = json.loads(report.read_text())
    assert [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert tuple(r) == cli.COLUMNS + cli.CALIBRATION_COLUMNS
        s, n = r['image'], r['n_samples']
        if n >= 2:
            assert all(r[k] is not None and np.isfinite(r[k]) for k in cli.CALIBRATION_COLUMNS)
            k = min(n // 2, max(1, int(np.floor((1 - 0.8) / 2 * (n + 1) + 0.5))))
            assert r['coverage_nominal'] == (n + 1 - 2 * k) / (n + 1.0) and 0.0 <= r['coverage'] <= 1.0
            assert f'image {s}: calibration: coverage ' in stdout
        else:
            assert all(r[k] is None for k in cli.CALIBRATION_COLUMNS) and f'image {s}: calibration' not in stdout
    assert 'Total Average calibration: ' in stdout

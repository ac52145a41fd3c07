"""GPU: several chains per image -- the split R-hat / ESS kernel (nhmc_chain_diag, csrc/metrics.hip) against the float64
restatement of its definition in tests/test_diag_cpu.py, the pooled `metrics.summarize`, the replica chains' inputs
through the sampler, and the CLI's convergence report."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from test_diag_cpu import diag_float64

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]


def chains(G, K, S, C, H, W, seed=1234):
    """-> float32 [G * K, S, C, H, W] on the host: per element an AR(1) chain of unit stationary variance whose phi runs
    linearly over [-0.5, 0.9] along the elements; every fifth element carries a per-replica offset of 1.5 sigma times a
    standard normal draw; all scaled by 0.25 and clamped to [-1, 1].  Element 3 is 1.0 everywhere (constant), element 7
    is linspace(-1, 1, K)[r] in replica r (stuck)."""
    g = torch.Generator().manual_seed(seed)
    E = C * H * W
    phi = torch.linspace(-0.5, 0.9, E, dtype=torch.float64)
    x = torch.empty(G, K, S, E, dtype=torch.float64)
    x[:, :, 0] = torch.randn(G, K, E, generator=g, dtype=torch.float64)
    for t in range(1, S):
        x[:, :, t] = phi * x[:, :, t - 1] + (1 - phi * phi).sqrt() * torch.randn(G, K, E, generator=g, dtype=torch.float64)
    offset = 1.5 * torch.randn(G, K, 1, 1, generator=g, dtype=torch.float64)
    x[..., ::5] += offset
    x = (0.25 * x).clamp(-1.0, 1.0)
    x[..., 3] = 1.0
    x[..., 7] = torch.linspace(-1.0, 1.0, K, dtype=torch.float64)[None, :, None]
    return x.float().reshape(G * K, S, C, H, W).contiguous()


DIAG_SHAPES = [(2, 3, 20, 3, 8, 8),         # the workload's S, group indexing, one partial tile
               (1, 2, 7, 1, 8, 8),          # odd S, n = 3, only P_0
               (1, 4, 4, 1, 4, 4),          # the minimum S, every ESS at the cap
               (2, 8, 20, 3, 16, 16),       # several tiles per group, K = 8
               (1, 1, 64, 1, 8, 8),         # n = 32, the largest instantiation, single chain
               (1, 2, 30, 1, 8, 12)]        # n = 15: the instantiation between the workload's and the largest
THRESHOLD = 1.1
# The two discrete decisions, from the restatement on the host CPU for these shapes with seed 1234: the smallest |P_k| over
# every evaluated k is 3.0e-4 and the smallest |rhat - 1.1| is 1.7e-6, so the 1e-9 exclusion below removes nothing.


def ulp32(v):
    return np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('shape', DIAG_SHAPES)
def test_chain_diag_matches_the_float64_definition(shape):
    """Maps: the restatement rounded to fp32, within 1 ulp of fp32 (both sides are fp64 arithmetic that differs only in
    summation order), NaN and inf at the same places.  Summaries: 1e-9 relative, n_constant exact."""
    from nhmc import metrics
    G, K, S, C, H, W = shape
    E = C * H * W
    x = chains(*shape)
    got = metrics.convergence(x.cuda(), K, THRESHOLD)
    assert got['rhat'].shape == (G, C, H, W) and got['ess'].shape == (G, C, H, W) and got['rhat'].dtype == torch.float32
    xs = x.reshape(G, K, S, E).numpy()
    for gi in range(G):
        want = diag_float64(xs[gi], THRESHOLD)
        # elements within 1e-9 of a discrete decision (the ESS cut P_k <= 0, the threshold count) are left out; the cap
        # on their number is a condition of the test
        excluded = (want['p_margin'] < 1e-9) | (want['thr_margin'] < 1e-9)
        print(f'chain_diag {shape} image {gi}: min |P_k| {want["p_margin"].min():.3e}  min |rhat - thr| '
              f'{want["thr_margin"].min():.3e}  excluded {int(excluded.sum())} of {E}')
        assert excluded.sum() <= 0.001 * E
        keep = ~excluded
        for name in ('rhat', 'ess'):
            g_ = got[name][gi].flatten().cpu().numpy().astype(np.float64)[keep]
            w_ = want[name][keep]
            assert np.array_equal(np.isnan(g_), np.isnan(w_)), name
            assert np.array_equal(np.isposinf(g_), np.isposinf(w_)) and not np.isneginf(g_).any(), name
            fin = np.isfinite(w_)
            w32 = w_[fin].astype(np.float32)
            err = np.abs(g_[fin] - w32.astype(np.float64)) / ulp32(w32)
            print(f'  {name}: max error {err.max() if err.size else 0.0:.2f} ulp over {int(fin.sum())} finite elements')
            assert (err <= 1.0).all(), name
        assert np.isnan(want['rhat'][3]) and got['n_constant'][gi] == want['n_constant'] >= 1
        if K > 1:
            assert np.isposinf(want['rhat'][7]) and np.isposinf(got['rhat_max'][gi])
        for name in ('rhat_max', 'rhat_mean', 'rhat_frac_above', 'ess_min', 'ess_mean'):
            g_, w_ = float(got[name][gi]), float(want[name])
            print(f'  {name}: {g_!r} against {w_!r}')
            assert (g_ == w_) or abs(g_ - w_) <= 1e-9 * abs(w_), name
        if S < 6:
            cap = 2 * K * (S // 2) * np.log10(2 * K * (S // 2))
            assert np.allclose(want['ess'][~np.isnan(want['ess'])], cap, rtol=1e-15)
    again = metrics.convergence(x.cuda(), K, THRESHOLD)                      # equal inputs, equal bits
    assert torch.equal(again['rhat'].view(torch.int32), got['rhat'].view(torch.int32))
    assert torch.equal(again['ess'].view(torch.int32), got['ess'].view(torch.int32))
    for name in metrics.CONVERGENCE_KEYS:
        assert np.array_equal(again[name], got[name], equal_nan=True)


def test_argument_validation():
    """Through the C ABI with pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ok = (2, 2, 20, 1024, 1.1, null)                                          # groups, replicas, samples, n_elem, threshold, stream
    ARG, ALIGN, SHAPE = 1, 2, 3
    for i in range(5):                                                        # each pointer in turn
        ptrs = [a16] * 5
        ptrs[i] = null
        assert lib.nhmc_chain_diag(*ptrs, *ok) == ARG
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 0, 2, 20, 1024, 1.1, null) == ARG
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 0, 20, 1024, 1.1, null) == ARG
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 2, 0, 1024, 1.1, null) == ARG
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 2, 20, 0, 1.1, null) == ARG
    assert lib.nhmc_chain_diag(a4, a16, a16, a16, a16, *ok) == ALIGN
    assert lib.nhmc_chain_diag(a16, a4, a16, a16, a16, *ok) == ALIGN
    assert lib.nhmc_chain_diag(a16, a16, a4, a16, a16, *ok) == ALIGN
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 2, 20, 1022, 1.1, null) == ALIGN          # n_elem % 4
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 2, 3, 1024, 1.1, null) == SHAPE           # n_samples < 4
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 2, 66, 1024, 1.1, null) == SHAPE          # n_samples / 2 > 32
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 2, 205, 20, 1024, 1.1, null) == SHAPE        # K * S > 4096
    assert lib.nhmc_chain_diag(a16, a16, a16, a16, a16, 65536, 2, 20, 1024, 1.1, null) == SHAPE      # groups ride in gridDim.y
    assert lib.nhmc_chain_diag(a4, a16, a16, a16, a16, 2, 2, 3, 1024, 1.1, null) == ALIGN            # ALIGN before SHAPE
    assert lib.nhmc_chain_diag_tiles(3 * 256 * 256) == 768 and lib.nhmc_chain_diag_tiles(64) == 1
    assert lib.nhmc_chain_diag_tiles(257) == 2 and lib.nhmc_chain_diag_tiles(0) == 0
    assert lib.nhmc_chain_diag_ws_bytes(8, 3 * 256 * 256) == 8 * 768 * 8 * 8 and lib.nhmc_chain_diag_ws_bytes(0, 64) == 0
    # the binding's own shape checks
    import nhmc.kernels as K
    with pytest.raises(nhmc._lib.NhmcError, match='multiple'):
        K.chain_diag(torch.zeros(3, 4, 1, 4, 4, device='cuda'), 2)
    with pytest.raises(nhmc._lib.NhmcError, match='chains, samples, C, H, W'):
        K.chain_diag(torch.zeros(4, 1, 4, 4, device='cuda'), 2)


def test_pooled_summary_uses_all_replicas():
    from nhmc import metrics
    G, K, S, C, H, W = 2, 3, 4, 3, 16, 16
    g = torch.Generator().manual_seed(7)
    low = torch.rand(G, C, 4, 4, generator=g) * 1.7 - 0.5
    orig = torch.nn.functional.interpolate(low, size=(H, W), mode='bicubic', align_corners=True).contiguous()
    amp = torch.linspace(0.05, 0.4, H)[:, None].expand(H, W)
    samples = (orig.repeat_interleave(K, dim=0)[:, None] + amp * torch.randn(G * K, S, C, H, W, generator=g)).contiguous()
    samples, orig = samples.cuda(), orig.cuda()
    out = metrics.summarize(samples, orig, replicas=K)
    pooled = samples.reshape(G, K * S, C, H, W)
    mean, std_map, norm = metrics.sample_moments(pooled)
    assert torch.equal(out['mean'], mean) and torch.equal(out['std_map'], std_map)
    assert torch.equal(out['std_map_normalised'], norm) and out['n_samples'] == K * S and out['replicas'] == K
    ps = metrics.psnr(pooled, orig).double().cpu().numpy()
    ss = metrics.ssim(pooled, orig).cpu().numpy()
    assert ps.shape == (G, K * S)
    assert np.array_equal(out['psnr_mean'], ps.mean(axis=1)) and np.array_equal(out['psnr_std'], ps.std(axis=1, ddof=1))
    assert np.array_equal(out['ssim_mean'], ss.mean(axis=1)) and np.array_equal(out['ssim_std'], ss.std(axis=1, ddof=1))
    # a single replica's samples give another mean: all K * S were used
    assert not np.array_equal(out['psnr_mean'], ps[:, :S].mean(axis=1))
    conv = metrics.convergence(samples, K)
    assert torch.equal(out['rhat'], conv['rhat']) and torch.equal(out['ess'], conv['ess'])
    assert out['rhat'].shape == (G, C, H, W)
    for name in metrics.CONVERGENCE_KEYS:
        assert out[name].shape == (G,) and np.array_equal(out[name], conv[name], equal_nan=True)
    assert np.isfinite(out['rhat_mean']).all() and np.isfinite(out['ess_mean']).all()
    # replicas = 1: what a call without the argument returns, keys and bits
    per_chain = orig.repeat_interleave(K, dim=0)
    a, b = metrics.summarize(samples, per_chain), metrics.summarize(samples, per_chain, replicas=1)
    assert list(a) == list(b) and 'rhat' not in a and 'replicas' not in a
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k])
        else:
            assert a[k] == b[k]
    # fewer than 4 samples per replica: pooled metrics, no R-hat
    few = metrics.summarize(samples[:, :3].contiguous(), orig, replicas=K)
    assert few['n_samples'] == 3 * K and few['rhat'] is None and np.isnan(few['rhat_mean']).all()
    assert np.isfinite(few['psnr_mean']).all()


class PointwiseScore(torch.nn.Module):
    """A float64 stand-in score with no cross-sample and no cross-pixel operation: a chain's values do not depend on the
    batch it is evaluated in, bit for bit."""

    def forward(self, x, t):
        a = (t.double() / 1000.0).view(-1, 1, 1, 1)
        e = (torch.tanh(x.double() * 0.7) * (0.5 + a)).to(x.dtype)
        return torch.cat([e, torch.zeros_like(e)], dim=1)


class EveryKth:
    """The noise of chains 0, K, 2K, ... of a Philox source: the streams replica 0 of each image has among K replicas
    (the global chain id of replica r of image s is s * K + r)."""

    def __init__(self, source, K):
        self.source, self.K = source, K

    def momentum(self, it, like, scale):
        wide = like.new_empty((like.shape[0] * self.K,) + tuple(like.shape[1:]))
        return self.source.momentum(it, wide, scale)[::self.K].contiguous()

    def uniform(self, it, n, device):
        return self.source.uniform(it, n * self.K, device)[::self.K].contiguous()


def test_replicas_leave_replica_zero_alone():
    """2 images x 2 replicas built by `replica_inputs` against the 2-image single-chain run built by `draw_inputs`, both
    with the Philox streams s * K + r: chain 2s returns the samples of image s bit for bit, so adding replicas changes
    neither replica 0's inputs nor its trajectory.  (At K = 1 the stream id s * K + r is the image index, today's.)"""
    from nhmc import cli, operators, plugin, sampler
    from oracle import schedule as osched
    dim, K, seed = 16, 2, 5678
    dev = torch.device('cuda')
    op = operators.build_operator('sr4', 3, dim, dev)
    algo = plugin.HMC(PointwiseScore().to(dev), op, 0.1)
    b = osched.betas_fp32().to(dev)
    x_orig = (torch.rand(2, 3, dim, dim, generator=torch.Generator().manual_seed(31)) * 2 - 1).to(dev)
    y_clean = op.H(x_orig)
    opt = types.SimpleNamespace(tau=0.2, epsilon=0.05, m=1.0, sigma_0=0.1, quiet=True)
    kw = dict(epochs=3, sampling=4)

    one = [cli.draw_inputs(seed, s, y_clean[s], 0.1, (3, dim, dim)) for s in range(2)]
    single = sampler.hmc_chains(torch.stack([d[1] for d in one]), b, SEQ, SEQ_NEXT, algo, opt, torch.stack([d[0] for d in one]),
                                op, x_orig, noise=EveryKth(sampler.PhiloxNoise(seed, 0), K), **kw)
    rep = [cli.replica_inputs(seed, s, K, y_clean[s], 0.1, (3, dim, dim)) for s in range(2)]
    multi = sampler.hmc_chains(torch.cat([d[1] for d in rep]).contiguous(), b, SEQ, SEQ_NEXT, algo, opt,
                               torch.cat([d[0] for d in rep]).contiguous(), op, x_orig.repeat_interleave(K, dim=0),
                               noise=sampler.PhiloxNoise(seed, cli.chain_id_base([0, 1], K)), **kw)
    assert multi.samples.shape == (4, 4, 3, dim, dim) and single.samples.shape == (2, 4, 3, dim, dim)
    assert float(single.samples.abs().max()) > 0.0
    for s in range(2):
        assert torch.equal(multi.samples[K * s], single.samples[s]) and torch.equal(multi.x[K * s], single.x[s])
        assert not torch.equal(multi.samples[K * s + 1], multi.samples[K * s])          # the other replica went elsewhere


TINY = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True},
        'model': dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True,
                      class_cond=False, use_checkpoint=False, attention_resolutions='16', num_heads=4,
                      num_head_channels=16, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0.0,
                      resblock_updown=True, use_fp16=False, use_new_attention_order=False, model_path=''),
        'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}


def test_cli_reports_convergence(tmp_path, monkeypatch, capsys):
    import yaml
    from PIL import Image
    from nhmc import cli
    (tmp_path / 'configs').mkdir()
    (tmp_path / 'configs' / 'config_tiny.yml').write_text(yaml.safe_dump(TINY))
    monkeypatch.chdir(tmp_path)

    def run(replicas, tag):
        out_dir, report = tmp_path / f'out{tag}', tmp_path / f'report{tag}' / 'metrics.json'
        cli.main(['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05',
                  '-i', str(out_dir), '--tau', '0.1', '--epsilon', '0.05', '--synthetic', '2', '--chains', '4',
                  '--replicas', str(replicas), '--philox', '--hmc_epochs', '4', '--hmc_sampling', '6',
                  '--metrics_out', str(report), '--save_images'])
        return capsys.readouterr().out, json.loads(report.read_text()), out_dir

    stdout, rows, out_dir = run(2, 'k2')
    for s in (0, 1):
        line = [ln for ln in stdout.splitlines() if ln.startswith(f'image {s}: R-hat max ')]
        assert len(line) == 1 and ' ESS min ' in line[0] and ' of 12 draws, constant elements ' in line[0] and '(> 1.1: ' in line[0]
        assert f'image {s}: PSNR ' in stdout and f'image {s}: SSIM ' in stdout
    assert len(rows) == 2 and [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert set(r) == set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS)
        assert r['replicas'] == 2 and r['n_samples'] == 12
        assert np.isfinite(r['rhat_mean']) and np.isfinite(r['ess_mean']) and r['rhat_mean'] > 0.9
        assert 0.0 <= r['rhat_frac_above'] <= 1.0 and 0 <= r['n_constant'] < 3 * 32 * 32 and r['ess_min'] <= r['ess_mean']
    for name in ('rhat_map_0.png', 'rhat_map_1.png', 'std_dev_map_0.png', 'std_dev_map_1.png', '0_mean.png', '1_mean.png'):
        assert Image.open(os.path.join(out_dir, name)).size == (32, 32)

    stdout, rows, out_dir = run(1, 'k1')
    assert 'R-hat' not in stdout and len(rows) == 2
    for r in rows:
        assert tuple(r) == cli.COLUMNS and r['n_samples'] == 6
    assert not os.path.exists(os.path.join(out_dir, 'rhat_map_0.png'))
    assert os.path.exists(os.path.join(out_dir, 'std_dev_map_0.png'))


def test_latent_cli_reports_convergence(tmp_path, monkeypatch, capsys):
    """The latent entry with 2 replicas per image on the small latent config of test_ldm_gpu.py's CLI test: an image's
    replicas are cut to their common sample count, decoded together and reported as one pooled image."""
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
    out_dir, report = tmp_path / 'out', tmp_path / 'metrics.json'
    table = cli.main_latent(['--dataset', 'tiny', '--algo', 'hmc_latent', '--timesteps', '3', '--deg', 'inpaint_random',
                             '--sigma_0', '0.05', '-i', str(out_dir), '--tau', '0.1', '--epsilon', '0.1', '--sigma_y', '1.0',
                             '--synthetic', '2', '--chains', '4', '--replicas', '2', '--philox', '--metrics_out', str(report),
                             '--save_images'])
    stdout = capsys.readouterr().out
    rows = json.loads(report.read_text())
    assert table.shape == (2, 3) and [r['image'] for r in rows] == [0, 1]
    for r in rows:
        assert set(r) == set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS) and r['replicas'] == 2
        assert r['n_samples'] % 2 == 0 and r['n_samples'] <= 20              # two replicas, the same count of each
        s = r['image']
        if r['n_samples'] >= 8:                                              # 4 samples per replica or more: R-hat is defined
            assert np.isfinite(r['rhat_mean']) and np.isfinite(r['ess_mean']) and f'image {s}: R-hat max ' in stdout
            assert Image.open(os.path.join(out_dir, f'rhat_map_{s}.png')).size == (64, 64)
        else:
            assert r['rhat_mean'] is None and f'image {s}: R-hat' not in stdout
        if r['n_samples']:
            assert np.isfinite(r['psnr_mean']) and f'image {s}: PSNR ' in stdout
    assert 'Total Average PSNR' in stdout

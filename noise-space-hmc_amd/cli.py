"""Command line with the reference's flags (`get_parser`, main_sampling.py:923-1015) for the HMC path.

    python main_sampling.py --dataset ffhq --algo hmc --timesteps 3 --deg inpaint_random --sigma_0 0.05 \
        -i exp/samples/ffhq/inpaint_random/hmc --tau 1.0 --epsilon 0.05          (README.md:79 of the reference)

Same flag names and defaults; unknown flags are ignored as in the reference (`parse_known_args`, :1031).  Only
`--algo hmc` (and `--algo hmc_latent` through `main_latent`, the counterpart of main_sampling_latent.py:791-918 with
its own defaults: `--epsilon 0.1`, no `--annealed_temp`) and the degradations on the hot path are served -- the nine
linear ones and the two nonlinear ones that need nothing from outside, `hdr` and `phase_retrieval` (matched as the
reference matches them, `'hdr' in deg` / `'phase' in deg`, :315-322; `sigma_0` is doubled for them too, :348); anything
else (`deblur_nonlinear` needs the external bkse network) raises `NotImplementedError` (the reference's own error for an unknown algo, :256-257).  Additions, all optional: `--chains` images are
sampled in parallel as independent chains (the reference is batch-1), `--score_chunk` bounds the U-Net batch,
`--synthetic K` uses K synthetic images when no dataset folder is present, `--philox` switches the noise to the
shard-invariant counter-based generator.  Under torchrun the images are sharded over ranks and the per-image
metrics are gathered once at the end (RCCL).  The measurement noise and the start point of image s are drawn from a
generator keyed by (seed, s) -- never from the global stream -- so with `--philox` (implied when WORLD_SIZE > 1) an
image's result does not depend on the number of ranks (nor, up to the score network's batch-size-dependent
convolution rounding, on `--chains`).  `--spectral_projected` switches the two blur operators to the four-product data
term (operators.Deblurring2D).

`--deg deblur_motion` (not wired in the reference) blurs with a seeded camera-shake PSF (operators.motion_kernel, drawn
from the global torch RNG right after the seed is set, so every rank holds the same one) through the general 2-D blur
kernels (operators.Blur2D); with `--save_images` rank 0 also writes `blur_kernel.png`, the PSF min-max normalised, once.

`--deg ct<V>` (not in the reference) is sparse-view parallel-beam CT with V views (operators.radon_matrix) through the
sparse-operator kernels (operators.SparseLinear).  `--deg sparse --operator FILE.npz` samples the posterior of any linear
forward model: FILE.npz holds a CSR matrix [m, image_size^2] in the layout `scipy.sparse.save_npz` writes (`data`,
`indices`, `indptr`, `shape`), applied to every channel plane alike; it is read with numpy alone.

`--deg mri<R>` (not in the reference) is Cartesian accelerated MRI at acceleration R: the centred orthonormal 2-D DFT of
every channel plane, kept on image_size // R whole columns of k-space (operators.cartesian_mask, drawn from the global
torch RNG right after the seed is set, so every rank holds the same mask), through the Fourier-sampling kernels
(operators.FourierSampling); the measurement is [Re ; Im] per plane, M = 2 C image_size^2, read only where the mask is
set.  `--deg fourier --kspace_mask FILE.npy` takes any real weight map [image_size, image_size] (>= 0, DC at the centre)
instead: partial Fourier, band limits, a measured sampling density.  With `--save_images` rank 0 also writes
`kspace_mask.png`, the weights scaled to their maximum, once.

`--deg mcmri<R>` (not in the reference) is multi-coil accelerated MRI (SENSE): `--coils K` receive coils (default 8, 1 ...
32), each seeing the image times its complex sensitivity map (operators.coil_maps, deterministic), all undersampled by the
Cartesian mask of `mri<R>`, through the modulated-Fourier kernels (operators.ModulatedFourier); the measurement is
[Re ; Im] per plane and coil, M = 2 C K image_size^2.  `--coil_maps FILE.npy` takes the maps from a complex or real
[K, image_size, image_size] array instead; it goes only with `mcmri<R>`.  With `--save_images` rank 0 also writes
`kspace_mask.png` and `coil_maps.png`, the K magnitudes side by side scaled to their maximum, once.  `--deg cdp<K>` (not in
the reference) is coded diffraction: the K moduli |F (M_k o x) F^T| behind K random unit-modulus masks
(operators.diffraction_masks, drawn from the global torch RNG right after the seed is set), M = C K image_size^2 -- the
well-posed form of `phase_retrieval`; nonlinear, through the same kernels.

`--replicas K` spends the chains on K replica chains per image instead (a batch then holds `--chains` // K images, chain
i * K + r being replica r of the batch's image i): all replicas see the same measurement, replica 0 starts where the
single chain starts, replicas r >= 1 start from their own N(0,1) draw keyed by (seed, s, r), and the Philox stream of
replica r of image s is s * K + r.  The report pools an image's K * S samples and adds the split R-hat / ESS line
(nhmc.metrics.convergence).  With K = 1, the default, nothing changes.

`--calibration [LEVEL]` (LEVEL = 0.9 when bare) adds, per image, where the original lies in the cloud of its pooled samples
(nhmc.metrics.calibration): the coverage of the central interval nearest to LEVEL against its nominal value, spread / skill,
the RMS z-score, the correlation of |error| with the sample std and the PSNR of the posterior mean -- CALIBRATION_COLUMNS
in the JSON rows and, with `--save_images`, `calibration_map_{s}.png`.  Without the flag nothing changes.

`--credible [LEVEL]` (LEVEL = 0.9 when bare) adds, per image, the interval that coverage is computed for and the median
(nhmc.metrics.credible): the order statistics d_(k) and d_(n+1-k) of the image's pooled draws per element and their median --
CREDIBLE_COLUMNS in the JSON rows, after the calibration columns, and, with `--save_images`, `{s}_median.png`,
`{s}_lower.png`, `{s}_upper.png` and `ci_width_map_{s}.png`.  Without the flag nothing changes.

`--pcs [COUNT]` (COUNT = 3 when bare, 1 ... 8) adds, per image, the principal components of its pooled samples
(nhmc.metrics.pcs): how many there are, the share of the variance the first and the first COUNT carry, the effective rank,
the share of the error that lies inside the samples' span and its RMS z-score along the components -- PCS_COLUMNS in the
JSON rows, after all other columns, and, with `--save_images`, `{s}_pc{j}_plus.png` and `{s}_pc{j}_minus.png`: the posterior
mean moved two standard deviations along component j.  Without the flag nothing changes.
"""
import argparse
import glob
import os
import sys
import random

import numpy as np
import torch

from . import ldm, metrics, operators, plugin, sampler, schedule, sharding, unet


def get_parser(latent=False):
    """`get_parser` of main_sampling.py:923-1015, or of main_sampling_latent.py:791-897 with latent=True."""
    p = argparse.ArgumentParser()
    p.add_argument('--seed', type=int, default=5678, help='Random seed')
    p.add_argument('--exp', type=str, default='exp', help='Path for saving running related data.')
    p.add_argument('--dataset', type=str, nargs='?', default='celeba', help='dataset')
    p.add_argument('--default_lr', action='store_true')
    p.add_argument('--lr', type=float, nargs='?', default=1.0, help='Step-Size')
    p.add_argument('--N', type=int, default=1, help='N repeats')
    p.add_argument('--deg', type=str, required=True, help='Degradation')
    p.add_argument('--sigma_0', type=float, required=True, help='Sigma_0')
    p.add_argument('--tau', type=float, default=1.0, help='Tau for HMC')
    p.add_argument('--epsilon', type=float, default=0.1 if latent else 0.05, help='Epsilon for HMC')
    p.add_argument('--sigma_y', type=float, default=0.5, help='sigma_y for HMC (measurement noise)')
    p.add_argument('--m', type=float, default=1.0, help='Mass Matrix Variance')
    if not latent:
        p.add_argument('--annealed_temp', action='store_true', default=False)
    p.add_argument('--noise', type=str, default='ddpm', help='Type of Noise')
    p.add_argument('--num_timesteps', type=int, nargs='?', default=1000)
    p.add_argument('--timesteps', type=int, nargs='?', default=10)
    p.add_argument('--subset_start', type=int, default=-1)
    p.add_argument('--subset_end', type=int, default=-1)
    p.add_argument('--algo', type=str, nargs='?', default='resample')
    p.add_argument('--refine', action='store_true')
    p.add_argument('-i', '--image_folder', type=str, default='exp/samples/ffhq/00000')
    # additions
    p.add_argument('--chains', type=int, default=1, help='images sampled in parallel (independent chains)')
    p.add_argument('--score_chunk', type=int, default=None,
                   help='chains per score-network call; default: as many of --chains as the free device memory holds')
    p.add_argument('--synthetic', type=int, default=0, help='use this many synthetic images')
    p.add_argument('--philox', action='store_true', help='counter-based, shard-invariant noise')
    p.add_argument('--save_images', action='store_true')
    p.add_argument('--metrics_out', type=str, default=None,
                   help='write the per-image report (PSNR, SSIM, std-map range) as a JSON list to this path')
    p.add_argument('--spectral_projected', action='store_true',
                   help='deblur_aniso / deblur_gauss: residual in the left singular basis, 4 products instead of 8 (rounds differently)')
    p.add_argument('--operator', type=str, default=None, metavar='FILE.npz',
                   help='--deg sparse: the forward model as a CSR matrix [m, image_size^2] in the layout scipy.sparse.save_npz '
                        'writes (data, indices, indptr, shape), applied to every channel plane')
    p.add_argument('--kspace_mask', type=str, default=None, metavar='FILE.npy',
                   help='--deg fourier: the k-space weight map, a real [image_size, image_size] array (>= 0, DC at the '
                        'centre; a binary mask is the common case), shared by all channels')
    p.add_argument('--coils', type=int, default=8, help='--deg mcmri<R>: the number of synthetic receive coils (1 ... 32)')
    p.add_argument('--coil_maps', type=str, default=None, metavar='FILE.npy',
                   help='--deg mcmri<R>: the coil sensitivities, a complex or real [K, image_size, image_size] array, instead '
                        'of the synthetic ones')
    p.add_argument('--graph', dest='use_graph', action='store_true',
                   help='replay each decode+gradient chunk as a hipGraph (helps single-chain runs: ~1.2x)')
    p.add_argument('--hmc_epochs', type=int, default=60, help='annealing epochs (reference: 60, main_sampling.py:665)')
    p.add_argument('--hmc_sampling', type=int, default=20, help='collected samples (reference: 20, :666)')
    p.add_argument('--replicas', type=int, default=1,
                   help='replica chains per image, from overdispersed starts; --chains must be a multiple of it. The report '
                        'pools their samples and adds split R-hat and ESS per pixel')
    p.add_argument('--rhat_threshold', type=float, default=1.1,
                   help="R-hat above which a pixel counts as not converged (Gelman's classic 1.1; with the 10 draws per "
                        'split chain of a 20-sample run the stricter 1.01 flags sampling noise)')
    p.add_argument('--calibration', type=float, nargs='?', const=0.9, default=None, metavar='LEVEL',
                   help='report the calibration of the samples against the original: coverage of the central interval '
                        'nearest to LEVEL (0.9 when the flag is bare), spread/skill, z-score RMS, |error|~std correlation')
    p.add_argument('--credible', type=float, nargs='?', const=0.9, default=None, metavar='LEVEL',
                   help='report the central credible interval nearest to LEVEL (0.9 when the flag is bare) and the median of '
                        "the samples per pixel: the interval's width, the share of the original inside it, PSNR of the median")
    p.add_argument('--pcs', type=int, nargs='?', const=3, default=None, choices=range(1, 9), metavar='COUNT',
                   help='report the first COUNT (3 when the flag is bare, 1 ... 8) principal components of the samples: their '
                        'share of the variance, the effective rank, the share of the error inside their span and its z-score')
    return p


FFHQ_DEFAULTS = {
    'data': {'dataset': 'ffhq', 'image_size': 256, 'channels': 3, 'rescaled': True},
    'model': dict(unet.FFHQ_CONFIG, model_path='models/ffhq_10m.pt'),
    'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000},
}


FFHQ_LATENT_DEFAULTS = {
    'data': {'dataset': 'ffhq', 'image_size': 256, 'channels': 3, 'rescaled': True},
    'model': {'target': 'ldm.models.diffusion.ddpm.LatentDiffusion', 'params': ldm.FFHQ_LDM},
}


def load_config(dataset, latent=False):
    """configs/config_{dataset}.yml (main_sampling.py:1033) or configs/config_{dataset}_latent.yml
    (main_sampling_latent.py:904); the FFHQ values are built in for a checkout without the reference's configs/."""
    path = f'configs/config_{dataset}_latent.yml' if latent else f'configs/config_{dataset}.yml'
    if os.path.exists(path):
        import yaml
        with open(path) as f:
            return yaml.safe_load(f)
    if dataset == 'ffhq':
        return FFHQ_LATENT_DEFAULTS if latent else FFHQ_DEFAULTS
    raise FileNotFoundError(path)


def load_images(folder, size, start, end, synthetic, seed):
    files = sorted(glob.glob(os.path.join(folder, '**', '*.png'), recursive=True)) if os.path.isdir(folder) else []
    if files and not synthetic:
        from PIL import Image
        if start >= 0 and end > 0:
            files = files[start:end]
        imgs = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB').resize((size, size)), dtype=np.float32) / 255.0)
                .permute(2, 0, 1) for f in files]
        return torch.stack(imgs) * 2 - 1                                     # data_transform: rescaled -> [-1,1]
    n = synthetic or 1
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, size // 16, size // 16, generator=g)
    return torch.nn.functional.interpolate(low, size=size, mode='bicubic', align_corners=False).clamp(0, 1) * 2 - 1


def auto_score_chunk(opt, device, probe, world=1):
    """Chains per score call when --score_chunk is not given.  Called AFTER the networks are on the device: `probe()` runs
    one decode + gradient of ONE chain through the engine the run will use (pixel path: three U-Net autograd graphs,
    3.45 GiB at FFHQ size; latent path: a no-grad LDM U-Net ladder + the VQ-f4 decoder's graph at 256 x 256), the peak it
    adds is the per-chain cost, and the free memory left -- divided by the ranks that share the card in a shared-GPU
    rehearsal (NHMC_SHARED_GPU=1) -- is filled to 1 / 1.12."""
    if opt.score_chunk:
        return opt.score_chunk
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    base = torch.cuda.memory_allocated(device)
    probe()
    torch.cuda.synchronize(device)
    per_chain = max(1, torch.cuda.max_memory_allocated(device) - base)
    torch.cuda.empty_cache()
    sharers = world if os.environ.get('NHMC_SHARED_GPU') == '1' else 1
    free = torch.cuda.mem_get_info(device)[0] / sharers
    return max(1, min(opt.chains, int(free / (per_chain * 1.12))))


def run_with_oom_backoff(opt, run):
    """run() with the score chunk halved after an out-of-memory error (a wrong estimate must not abort a run that
    takes hours).  Local to the rank: the sampler has no collective inside a run, so ranks need not agree."""
    import gc
    while True:
        try:
            return run()
        except torch.OutOfMemoryError:
            chunk = opt.score_chunk or opt.chains
            if chunk <= 1:
                raise
            opt.score_chunk = (chunk + 1) // 2
            gc.collect()
            torch.cuda.empty_cache()
            print(f'[nhmc] out of memory at {chunk} chains per score call; retrying with --score_chunk {opt.score_chunk}',
                  file=sys.stderr, flush=True)


def image_generator(seed, s):
    """Generator of image s: measurement noise and start point are keyed by (seed, global image index), on the host,
    so they do not depend on the rank that samples the image, on WORLD_SIZE or on --chains."""
    return torch.Generator().manual_seed((int(seed) * 1000003 + int(s)) & 0x7FFFFFFFFFFFFFFF)


def draw_inputs(seed, s, y_clean, sigma_0, x_shape):
    """-> (y_0, x_start) for image s: y_0 = H(x_orig) + sigma_0 * N(0,1) (main_sampling.py:447-448) and the
    N(0,1) start point (:460-466), both from `image_generator(seed, s)`.  y_clean: [M] on any device."""
    g = image_generator(seed, s)
    noise = torch.randn(y_clean.shape, generator=g)
    x = torch.randn(x_shape, generator=g)
    return y_clean + sigma_0 * noise.to(y_clean.device), x.to(y_clean.device)


def replica_generator(seed, s, r):
    """Generator of the start point of replica r >= 1 of image s, keyed by (seed, s, r) on the host; replica 0 uses
    `image_generator(seed, s)`.  The multiplier differs from image_generator's, so no (s, r) lands on an image's key."""
    return torch.Generator().manual_seed(((int(seed) * 1000003 + int(s)) * 998244353 + int(r)) & 0x7FFFFFFFFFFFFFFF)


def replica_inputs(seed, s, K, y_clean, sigma_0, x_shape):
    """-> (y_0 [K, M], x_start [K, *x_shape]) for the K replica chains of image s.  All replicas share one measurement,
    the y_0 of `draw_inputs`; replica 0 starts at `draw_inputs`' start point (its bits), replica r >= 1 at an N(0,1)
    draw from `replica_generator(seed, s, r)` -- starts that are overdispersed against the posterior.  Nothing here
    depends on the batch the image is sampled in."""
    y_0, x0 = draw_inputs(seed, s, y_clean, sigma_0, x_shape)
    xs = [x0] + [torch.randn(x_shape, generator=replica_generator(seed, s, r)).to(y_clean.device) for r in range(1, K)]
    return y_0[None].expand(K, *y_0.shape), torch.stack(xs)


def common_samples(replicas):
    """The latent sampler's sample count is ragged over chains: an image's replicas [S_r, ...] are cut to the last
    S_c = min S_r samples of each -> ([K * S_c, ...] replica-major, S_c)."""
    s_c = min(z.shape[0] for z in replicas)
    return torch.cat([z[z.shape[0] - s_c:] for z in replicas]), s_c


def chain_id_base(batch, K=1):
    """Philox stream id of the batch's first chain: replica r of image s has the global chain id s * K + r."""
    return batch[0] * K


def check_replicas(opt):
    """--chains must hold whole images; raised before anything touches the GPU."""
    if opt.replicas < 1 or opt.chains % opt.replicas:
        raise SystemExit(f'--chains {opt.chains} must be a positive multiple of --replicas {opt.replicas}: a batch holds '
                         f'chains // replicas images, each with all its replicas')


def image_batches(n_images, rank, world, chains):
    """Global image indices this rank samples, in batches of `chains`: contiguous block partition over ranks
    (sharding.chain_range), batches never straddle ranks.  With K replicas per image pass `chains // K`."""
    lo, hi = sharding.chain_range(n_images, rank, world)
    return [list(range(s, min(hi, s + chains))) for s in range(lo, hi, chains)]


def _setup(opt, latent):
    config = load_config(opt.dataset, latent)
    rank, local_rank, world = sharding.init_process_group()
    device = torch.device('cuda', local_rank)
    torch.cuda.set_device(device)
    torch.manual_seed(opt.seed)
    np.random.seed(opt.seed)
    random.seed(opt.seed)
    size, ch = config['data']['image_size'], config['data']['channels']
    # mask = first torch RNG draw, as in the reference
    operator_file = getattr(opt, 'operator', None)
    kspace_mask_file = getattr(opt, 'kspace_mask', None)
    coil_maps_file = getattr(opt, 'coil_maps', None)
    multi_coil = opt.deg.startswith('mcmri') and opt.deg[5:].isdigit()
    if coil_maps_file and not multi_coil:
        raise SystemExit('--coil_maps FILE.npy goes only with --deg mcmri<R>')
    if opt.deg == 'sparse' or operator_file:
        if opt.deg != 'sparse' or not operator_file:
            raise SystemExit('--deg sparse and --operator FILE.npz go together')
        try:
            op = operators.build_operator(opt.deg, ch, size, device, operator_file=operator_file)
        except operators.NhmcError as exc:
            raise SystemExit(str(exc))
    elif opt.deg == 'fourier' or kspace_mask_file or (opt.deg.startswith('mri') and opt.deg[3:].isdigit()):
        if (opt.deg == 'fourier') != bool(kspace_mask_file):
            raise SystemExit('--deg fourier and --kspace_mask FILE.npy go together')
        try:
            op = operators.build_operator(opt.deg, ch, size, device, kspace_mask_file=kspace_mask_file)
        except operators.NhmcError as exc:
            raise SystemExit(str(exc))
    elif multi_coil or (opt.deg.startswith('cdp') and opt.deg[3:].isdigit()):
        try:
            op = operators.build_operator(opt.deg, ch, size, device, n_coils=getattr(opt, 'coils', 8), coil_maps_file=coil_maps_file)
        except operators.NhmcError as exc:
            raise SystemExit(str(exc))
    else:
        op = operators.build_operator(opt.deg, ch, size, device, spectral_projected=opt.spectral_projected or None)
    if opt.save_images and rank == 0 and isinstance(op, operators.Blur2D):
        k = op.kernel
        span = float(k.max() - k.min())
        k01 = (k - k.min()) / span if span > 0 else torch.ones_like(k)
        sampler._save_png((2 * k01 - 1)[None].expand(3, -1, -1), os.path.join(opt.image_folder, 'blur_kernel.png'))
    if opt.save_images and rank == 0 and (isinstance(op, operators.FourierSampling) or multi_coil):
        w01 = op.weights / op.weights.max()                                 # max > 0: the constructor checked
        sampler._save_png((2 * w01 - 1)[None].expand(3, -1, -1), os.path.join(opt.image_folder, 'kspace_mask.png'))
    if opt.save_images and rank == 0 and multi_coil:                        # the K magnitudes side by side
        mag = torch.cat(list(op.maps.abs()), dim=1)
        sampler._save_png((2 * mag / mag.max() - 1)[None].expand(3, -1, -1), os.path.join(opt.image_folder, 'coil_maps.png'))
    opt.sigma_0 = 2 * opt.sigma_0                                           # [-1,1] scaling, main_sampling.py:348
    if world > 1 and not opt.philox:
        if rank == 0:
            print('WORLD_SIZE > 1: switching to the counter-based noise (--philox) so results do not depend on the sharding')
        opt.philox = True
    if opt.philox:
        opt.philox_seed = opt.seed
    opt.quiet = opt.chains > 1 or rank != 0
    opt.progress_every = 10 if rank == 0 else 0                           # stderr heartbeat for long quiet runs
    skip = opt.num_timesteps // (opt.timesteps + 1)                          # main_sampling.py:469-471
    seq = list(range(skip, opt.num_timesteps, skip))
    images = load_images(os.path.join(opt.exp, 'datasets', opt.dataset), size, opt.subset_start, opt.subset_end,
                         opt.synthetic, opt.seed)
    return config, rank, world, device, op, seq, [-1] + seq[:-1], images


COLUMNS = ('image', 'psnr_mean', 'psnr_std', 'ssim_mean', 'ssim_std', 'std_map_min', 'std_map_max', 'n_samples')
REPLICA_COLUMNS = ('replicas',) + metrics.CONVERGENCE_KEYS          # appended to COLUMNS with --replicas K > 1
CALIBRATION_COLUMNS = metrics.CALIBRATION_KEYS                      # appended last with --calibration
CREDIBLE_COLUMNS = metrics.CREDIBLE_KEYS                            # appended after those with --credible
PCS_COLUMNS = metrics.PCS_KEYS                                      # appended after all others with --pcs
INT_COLUMNS = ('image', 'n_samples', 'replicas', 'n_constant', 'n_tied', 'n_flat', 'ci_rank', 'n_point', 'n_nan', 'pc_count',
               'pc_rank')


def _report(rows, n_images, rank, world, device, metrics_out=None, replicas=1, rhat_threshold=1.1, calibration=None,
            credible=None, pcs=None):
    """Gathers the per-image rows (COLUMNS, with K > 1 replicas + REPLICA_COLUMNS, with --calibration + CALIBRATION_COLUMNS,
    with --credible + CREDIBLE_COLUMNS, with --pcs + PCS_COLUMNS) over the ranks in global image order, prints the report on
    rank 0 and returns the [n, 3] table (image, PSNR mean, PSNR std over its samples)."""
    columns = COLUMNS + (REPLICA_COLUMNS if replicas > 1 else ()) + (CALIBRATION_COLUMNS if calibration is not None else ()) + \
        (CREDIBLE_COLUMNS if credible is not None else ()) + (PCS_COLUMNS if pcs is not None else ())
    local = torch.tensor(rows, dtype=torch.float64, device=device).reshape(-1, len(columns))
    full = sharding.gather_chains(local, n_images, rank, world).cpu()
    table = full[:, :3].float()
    if rank == 0:
        for (idx, mean, std), row in zip(table.tolist(), full.tolist()):
            s_mean, s_std = row[3], row[4]
            print(f'image {int(idx)}: PSNR {mean:.3f} (std over samples {std:.4f})' if mean == mean else
                  f'image {int(idx)}: no sample was collected (every proposal of the final phase was rejected)')
            if mean == mean:
                print(f'image {int(idx)}: SSIM {s_mean:.5f} (std over samples {s_std:.5f})')
            c = dict(zip(columns, row))
            if replicas > 1 and mean == mean and c['n_constant'] != c['n_constant']:
                print(f'image {int(idx)}: no R-hat / ESS: fewer than 4 samples per replica ({int(c["n_samples"])} draws in all)')
            elif replicas > 1 and mean == mean:
                print(f'image {int(idx)}: R-hat max {c["rhat_max"]:.3f} mean {c["rhat_mean"]:.4f} '
                      f'(> {rhat_threshold:g}: {100.0 * c["rhat_frac_above"]:.2f}%)  ESS min {c["ess_min"]:.1f} '
                      f'mean {c["ess_mean"]:.1f} of {int(c["n_samples"])} draws, constant elements {int(c["n_constant"])}')
            if calibration is not None and c['n_flat'] == c['n_flat']:      # NaN: fewer than two pooled samples
                print(f'image {int(idx)}: calibration: coverage {c["coverage"]:.4f} at nominal {c["coverage_nominal"]:.4f}, '
                      f'spread/skill {c["spread_skill"]:.3f}, z rms {c["z_rms"]:.3f}, |err|~std r {c["err_std_corr"]:.3f}, '
                      f'PSNR of the posterior mean {c["psnr_of_mean"]:.3f}, tied {int(c["n_tied"])} flat {int(c["n_flat"])}')
            if credible is not None and c['ci_rank'] == c['ci_rank']:       # NaN: fewer than two pooled samples
                k_, n_ = int(c['ci_rank']), int(c['n_samples'])
                print(f'image {int(idx)}: credible interval: order statistics {k_} and {n_ + 1 - k_} of {n_} draws '
                      f'(level {c["ci_level"]:.4f}), width mean {c["ci_width_mean"]:.4f} max {c["ci_width_max"]:.4f}, '
                      f'original inside {c["ci_inside"]:.4f}, PSNR of the median {c["psnr_of_median"]:.3f}, '
                      f'point elements {int(c["n_point"])}')
            if pcs is not None and c['pc_var_first'] == c['pc_var_first']:  # NaN: no component (n < 2, n > 256, no variance)
                print(f'image {int(idx)}: principal components: {int(c["pc_count"])} of rank {int(c["pc_rank"])}, variance '
                      f'share first {c["pc_var_first"]:.4f} top-{int(c["pc_count"])} {c["pc_var_top"]:.4f}, effective rank '
                      f'{c["pc_eff_rank"]:.2f}, error inside the span {c["pc_err_in_span"]:.4f}, z rms along them '
                      f'{c["pc_z_rms"]:.3f}')
        print(f'Total Average PSNR: {float(table[:, 1].nanmean()):.3f}  images: {table.shape[0]}')
        # main_sampling.py:560: the average over the images, and in parentheses the mean over the images of each
        # image's std over its samples
        print('Total Average SSIM: {:.5f} ({:.5f})'.format(float(full[:, 3].nanmean()), float(full[:, 4].nanmean())))
        if calibration is not None:
            avg = {k: float(full[:, columns.index(k)].nanmean()) for k in CALIBRATION_COLUMNS}
            print(f'Total Average calibration: coverage {avg["coverage"]:.4f} at nominal {avg["coverage_nominal"]:.4f}, '
                  f'spread/skill {avg["spread_skill"]:.3f}, z rms {avg["z_rms"]:.3f}, |err|~std r {avg["err_std_corr"]:.3f}, '
                  f'PSNR of the posterior mean {avg["psnr_of_mean"]:.3f}')
        if credible is not None:
            avg = {k: float(full[:, columns.index(k)].nanmean()) for k in CREDIBLE_COLUMNS}
            print(f'Total Average credible interval: level {avg["ci_level"]:.4f}, width mean {avg["ci_width_mean"]:.4f} '
                  f'max {avg["ci_width_max"]:.4f}, original inside {avg["ci_inside"]:.4f}, '
                  f'PSNR of the median {avg["psnr_of_median"]:.3f}')
        if pcs is not None:
            avg = {k: float(full[:, columns.index(k)].nanmean()) for k in PCS_COLUMNS}
            print(f'Total Average principal components: variance share first {avg["pc_var_first"]:.4f} top-{pcs} '
                  f'{avg["pc_var_top"]:.4f}, effective rank {avg["pc_eff_rank"]:.2f}, error inside the span '
                  f'{avg["pc_err_in_span"]:.4f}, z rms along them {avg["pc_z_rms"]:.3f}')
        if metrics_out:
            import json
            as_json = lambda k, v: (int(v) if k in INT_COLUMNS and v == v else (v if v == v else None))
            os.makedirs(os.path.dirname(metrics_out) or '.', exist_ok=True)
            with open(metrics_out, 'w') as f:
                json.dump([{k: as_json(k, v) for k, v in zip(columns, row)} for row in full.tolist()], f, indent=1)
    sharding.barrier()
    return table


def _metric_rows(batch, summary):
    """One COLUMNS row per image of `batch` from a `metrics.summarize` result (entry i of it for image i); a pooled
    summary (replicas > 1) appends REPLICA_COLUMNS, one with the calibration figures CALIBRATION_COLUMNS, one with the
    credible interval's CREDIBLE_COLUMNS, one with the principal components' PCS_COLUMNS."""
    pooled = summary.get('replicas', 1) > 1
    return [[float(s)] + [float(summary[c][i]) for c in COLUMNS[1:-1]] + [float(summary['n_samples'])] +
            ([float(summary['replicas'])] + [float(summary[c][i]) for c in metrics.CONVERGENCE_KEYS] if pooled else []) +
            ([float(summary[c][i]) for c in CALIBRATION_COLUMNS] if 'coverage' in summary else []) +
            ([float(summary[c][i]) for c in CREDIBLE_COLUMNS] if 'ci_level' in summary else []) +
            ([float(summary[c][i]) for c in PCS_COLUMNS] if 'pc_count' in summary else [])
            for i, s in enumerate(batch)]


def _save_report_images(summary, k, s, one_sample, folder):
    """`{s}_mean.png` and, with two samples or more, `std_dev_map_{s}.png` (main_sampling.py:494-507); `rhat_map_{s}.png`
    and `calibration_map_{s}.png` where the summary holds those maps; with the credible interval's maps `{s}_median.png`,
    `{s}_lower.png`, `{s}_upper.png` and `ci_width_map_{s}.png`; with principal components `{s}_pc{j}_plus.png` and
    `{s}_pc{j}_minus.png`, the mean moved by +-2 standard deviations along component j = 1 ... pc_count."""
    if summary.get('z') is not None:
        metrics.save_calibration_map(summary['z'][k], os.path.join(folder, f'calibration_map_{s}.png'))
    if summary.get('median') is not None:
        for name in ('median', 'lower', 'upper'):
            sampler._save_png(summary[name][k], os.path.join(folder, f'{s}_{name}.png'))
        metrics.save_ci_width_map(summary['lower'][k], summary['upper'][k], os.path.join(folder, f'ci_width_map_{s}.png'))
    if summary.get('directions') is not None and summary['mean'] is not None and summary['pc_count'][k] == summary['pc_count'][k]:
        for j in range(int(summary['pc_count'][k])):
            step = 2.0 * summary['directions'][k, j]
            sampler._save_png(summary['mean'][k] + step, os.path.join(folder, f'{s}_pc{j + 1}_plus.png'))
            sampler._save_png(summary['mean'][k] - step, os.path.join(folder, f'{s}_pc{j + 1}_minus.png'))
    if summary['mean'] is None:
        sampler._save_png(one_sample, os.path.join(folder, f'{s}_mean.png'))
        return
    sampler._save_png(summary['mean'][k], os.path.join(folder, f'{s}_mean.png'))
    metrics.save_std_map(summary['std_map_normalised'][k], os.path.join(folder, f'std_dev_map_{s}.png'))
    if summary.get('rhat') is not None:
        metrics.save_rhat_map(summary['rhat'][k], os.path.join(folder, f'rhat_map_{s}.png'))


def main(argv=None):
    opt, _unknown = get_parser().parse_known_args(argv)
    if opt.algo == 'hmc_latent':
        raise NotImplementedError('--algo hmc_latent is served by main_sampling_latent.py (nhmc.cli.main_latent), as in the reference')
    if opt.algo != 'hmc':
        raise NotImplementedError(f"--algo {opt.algo}: this build serves the noise-space HMC path (--algo hmc) only")
    check_replicas(opt)
    config, rank, world, device, op, seq, seq_next, images = _setup(opt, latent=False)
    size, ch = config['data']['image_size'], config['data']['channels']
    mc = dict(config['model'])
    mc.pop('var_type', None)
    model = unet.create_model(**mc).to(device).eval().requires_grad_(False)
    algo = plugin.HMC(model, op, opt.sigma_0)
    d = config['diffusion']
    b = torch.from_numpy(schedule.get_beta_schedule(d['beta_schedule'], beta_start=d['beta_start'], beta_end=d['beta_end'],
                                                    num_diffusion_timesteps=d['num_diffusion_timesteps'])).float().to(device)

    def probe():
        eng = sampler.LeapfrogEngine(algo.score, op, b, seq, seq_next, device)
        eng.decode_and_grad(torch.zeros(1, ch, size, size, device=device), torch.zeros(1, op.M, device=device))
    if world > 1 and rank != 0:
        sharding.barrier()                                               # rank 0 probes (and fills MIOpen's cache) first
    opt.score_chunk = auto_score_chunk(opt, device, probe, world)
    if world > 1 and rank == 0:
        sharding.barrier()
    if world > 1:
        # the first score-network call on a machine fills MIOpen's on-disk kernel cache (~1 min): one rank does it at
        # the shape the run will use, the others wait instead of racing through the same compiles
        if rank == 0:
            n0 = max(1, min(opt.chains, opt.score_chunk or opt.chains))
            xw = torch.zeros(n0, ch, size, size, device=device, requires_grad=True)
            with torch.enable_grad():
                out = model(xw, torch.full((n0,), 500.0, device=device))
            torch.autograd.grad(out, xw, torch.ones_like(out))
            torch.cuda.synchronize()
        sharding.barrier()
    rows, K = [], opt.replicas
    for batch in image_batches(images.shape[0], rank, world, opt.chains // K):
        x_orig = images[batch[0]:batch[-1] + 1].to(device).contiguous()
        n = x_orig.shape[0] * K                                             # chains: image-major, replica r of image i at i * K + r
        drawn = [replica_inputs(opt.seed, s, K, yk, opt.sigma_0, (ch, size, size)) for s, yk in zip(batch, op.H(x_orig))]
        y_0 = torch.cat([d_[0] for d_ in drawn]).contiguous()
        x = torch.cat([d_[1] for d_ in drawn]).contiguous()
        x_chain = x_orig if K == 1 else x_orig.repeat_interleave(K, dim=0)   # the sampler's PSNR trace wants one per chain
        opt.chain_id0 = chain_id_base(batch, K)
        out = run_with_oom_backoff(opt, lambda: sampler.hmc(x, n, b, seq, seq_next, algo, opt, y_0, op, x_chain))
        samples = out[None] if n == 1 else out                              # [n, 20, C, H, W]
        summary = metrics.summarize(samples.contiguous(), x_orig, replicas=K, rhat_threshold=opt.rhat_threshold,
                                    calibration=opt.calibration, credible=opt.credible,
                                    pcs=opt.pcs)
        rows += _metric_rows(batch, summary)
        if opt.save_images and samples.shape[1]:
            for k, s in enumerate(batch):
                _save_report_images(summary, k, s, samples[k * K, 0], opt.image_folder)
    return _report(rows, images.shape[0], rank, world, device, opt.metrics_out, K, opt.rhat_threshold, opt.calibration,
                   opt.credible, opt.pcs)


def main_latent(argv=None):
    """main_sampling_latent.py:899-918 + `sample_image` (:351-560) for `--algo hmc_latent`: the latent model comes from
    configs/config_{dataset}_latent.yml + models/ldm/model.ckpt (:124-127), the operator acts on the decoded
    256 x 256 image, the sampler returns latents and `decode_first_stage` turns them into images (:477)."""
    opt, _unknown = get_parser(latent=True).parse_known_args(argv)
    if opt.algo != 'hmc_latent':
        raise NotImplementedError(f"--algo {opt.algo}: the latent entry serves --algo hmc_latent only")
    check_replicas(opt)
    config, rank, world, device, op, seq, seq_next, images = _setup(opt, latent=True)
    model = ldm.create_latent_model(config['model'], ckpt='models/ldm/model.ckpt', quiet=rank != 0).to(device)
    algo = plugin.HMCLatent(model, op, opt.sigma_0)
    zc, zs = model.channels, model.image_size

    def probe():
        table = torch.cat([model.alphas_cumprod_prev[0:1], model.alphas_cumprod], dim=0)
        eng = sampler.LeapfrogEngine(algo.score, op, None, seq, seq_next, device, alpha_table=table,
                                     image_map=model.differentiable_decode_first_stage)
        eng.decode_and_grad(torch.zeros(1, zc, zs, zs, device=device), torch.zeros(1, op.M, device=device))
    opt.score_chunk = auto_score_chunk(opt, device, probe, world)
    if world > 1:
        sharding.barrier()
    rows, K = [], opt.replicas
    for batch in image_batches(images.shape[0], rank, world, opt.chains // K):
        x_orig = images[batch[0]:batch[-1] + 1].to(device).contiguous()
        n = x_orig.shape[0] * K
        drawn = [replica_inputs(opt.seed, s, K, yk, opt.sigma_0, (zc, zs, zs)) for s, yk in zip(batch, op.H(x_orig))]
        y_0 = torch.cat([d_[0] for d_ in drawn]).contiguous()
        x = torch.cat([d_[1] for d_ in drawn]).contiguous()
        x_chain = x_orig if K == 1 else x_orig.repeat_interleave(K, dim=0)
        opt.chain_id0 = chain_id_base(batch, K)
        out = run_with_oom_backoff(opt, lambda: sampler.hmc_latent(x, n, seq, seq_next, algo, opt, y_0, op, x_chain))
        per_chain = [out] if n == 1 else out                               # latents [<=10, C, h, w] per chain
        for k, s in enumerate(batch):
            lat, s_c = common_samples(per_chain[k * K:(k + 1) * K])
            imgs = model.decode_first_stage(lat) if s_c else x_orig.new_empty((0,) + tuple(x_orig.shape[1:]))
            imgs = imgs.reshape((K, s_c) + tuple(imgs.shape[1:])).contiguous()
            summary = metrics.summarize(imgs if K > 1 else imgs[0], x_orig[k:k + 1], replicas=K,
                                        rhat_threshold=opt.rhat_threshold, calibration=opt.calibration,
                                        credible=opt.credible, pcs=opt.pcs)
            rows += _metric_rows([s], summary)
            if opt.save_images and s_c:
                _save_report_images(summary, 0, s, imgs[0, 0], opt.image_folder)
    return _report(rows, images.shape[0], rank, world, device, opt.metrics_out, K, opt.rhat_threshold, opt.calibration,
                   opt.credible, opt.pcs)


if __name__ == '__main__':
    main()

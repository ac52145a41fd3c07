"""Report stage: the metrics the reference's `sample_image` takes of the collected samples (main_sampling.py:488-561),
on the device.

    psnr(samples, x_orig)            [B, S]   PSNR of every sample against its chain's original        (:517-519)
    ssim(samples, x_orig)            [B, S]   skimage's default SSIM, data_range = the sample's range  (:520)
    sample_moments(samples)          posterior-mean image, per-pixel std map, its min-max normalised picture (:494-497)
    summarize(samples, x_orig)       per-chain means and ddof=1 stds (:526-538) + the maps, one device->host read
    save_std_map(map01, path)        the `std_dev_map_{idx}.png` picture (:499-507)
    convergence(samples, replicas)   split R-hat and ESS per element over an image's replica chains, with summaries
    save_rhat_map(rhat, path)        the `rhat_map_{idx}.png` picture
    calibration(samples, x_orig)     rank and z-score of the original among an image's pooled draws: coverage of the
                                     central interval, spread / skill, |error| ~ std correlation, PSNR of the mean
    save_calibration_map(z, path)    the `calibration_map_{idx}.png` picture
    credible(samples, x_orig)        the interval calibration speaks of, as maps: the order statistics d_(k) and d_(n+1-k)
                                     of an image's pooled draws and their median, per element, with summaries
    save_ci_width_map(lower, upper, path)   the `ci_width_map_{idx}.png` picture
    pcs(samples, x_orig)             the principal components of an image's pooled draws: direction images, eigenvalues,
                                     the variance they carry and how much of the error lies along them
    pcs_from_gram(gram, count)       the host part of it: the eigen-solve of the kernel's n x n Gram matrix

With K replica chains per image (not in the reference, which runs one chain) the block is [G * K, S, C, H, W], chain
g * K + r being replica r of image g, and `summarize(..., replicas=K)` pools an image's K * S samples.

`samples` is what `sampler.hmc` returns for B chains, float32 [B, S, C, H, W] in [-1, 1], with `x_orig` [B, C, H, W]; one
chain may be passed as [S, C, H, W] with a [1, C, H, W] (or [C, H, W]) original.  The kernels (csrc/metrics.hip) apply the
reference's inverse_data_transform themselves.  There is no CPU path and no host SSIM: skimage is not a dependency.
LPIPS (:521) is not served: it needs the `lpips` package and its VGG weights.
"""
import os

import numpy as np
import torch

from . import _lib
from . import kernels as K


def _block(samples, x_orig=None):
    """-> (samples [B, S, C, H, W], x_orig [B, C, H, W] or None, squeeze): the one-chain form gets its chain axis."""
    squeeze = samples.dim() == 4
    if squeeze:
        samples = samples[None]
        if x_orig is not None and x_orig.dim() == 3:
            x_orig = x_orig[None]
    if samples.dim() != 5:
        raise _lib.NhmcError(f'samples must be [B, S, C, H, W] or [S, C, H, W], got {tuple(samples.shape)}')
    for t in (samples, x_orig):
        if t is not None and not t.is_cuda:
            raise _lib.NhmcError(f'nhmc.metrics works on GPU tensors (got {t.device}); there is no CPU path')
    return samples, x_orig, squeeze


def psnr(samples, x_orig):
    """PSNR (dB) of each sample against its chain's original -> float32 [B, S] ([S] for the one-chain form); per sample
    the bits of `kernels.psnr`."""
    samples, x_orig, squeeze = _block(samples, x_orig)
    out = K.psnr_samples(samples, x_orig)
    return out[0] if squeeze else out


def ssim(samples, x_orig):
    """`skimage.metrics.structural_similarity(sample, orig, data_range=sample.max() - sample.min(), channel_axis=0)` of the
    transformed images, as the reference calls it -> float64 [B, S] ([S] for the one-chain form).  Needs H, W >= 7."""
    samples, x_orig, squeeze = _block(samples, x_orig)
    out = K.ssim(samples, x_orig)
    return out[0] if squeeze else out


def sample_moments(samples):
    """-> (mean [B, C, H, W], std_map [B, H, W], std_map_normalised [B, H, W]): the mean of the raw samples, the reference's
    `x.std(dim=0).mean(dim=0)` of the transformed ones and `(std - min) / (max - min)` of that map.  Needs S >= 2."""
    mean, std_map, _minmax, norm, squeeze = _moments(samples)
    return (mean[0], std_map[0], norm[0]) if squeeze else (mean, std_map, norm)


def _moments(samples):
    samples, _, squeeze = _block(samples)
    mean, std_map, minmax = K.sample_moments(samples)
    return mean, std_map, minmax, K.std_map_normalise(std_map, minmax), squeeze


CONVERGENCE_KEYS = ('rhat_max', 'rhat_mean', 'rhat_frac_above', 'ess_min', 'ess_mean', 'n_constant')


def convergence(samples, replicas, rhat_threshold=1.1):
    """Split R-hat and effective sample size per element over the `replicas` chains of every image (the definition is
    in include/nhmc.h).  samples [G * K, S, C, H, W] with 4 <= S <= 65 -> dict: rhat, ess (device, float32 [G, C, H, W];
    NaN where the element is constant, rhat +inf where the chains sit at different constants) and CONVERGENCE_KEYS as
    float64 numpy [G], with one device->host read."""
    samples, _, _ = _block(samples)
    rhat, ess, summary = K.chain_diag(samples, replicas, rhat_threshold)
    host = summary.cpu().numpy()
    return dict(rhat=rhat, ess=ess, **{k: host[:, i].copy() for i, k in enumerate(CONVERGENCE_KEYS)})


CALIBRATION_KEYS = ('psnr_of_mean', 'spread_skill', 'z_rms', 'err_std_corr', 'coverage', 'coverage_nominal', 'n_tied',
                    'n_flat')
CALIBRATION_SUMS = ('sum_err2', 'sum_var', 'sum_abs_err', 'sum_std', 'sum_abs_err_std', 'sum_z2', 'n_tied', 'n_flat')


def coverage_rank(n, level):
    """k of the central interval [d_(k), d_(n+1-k)] between order statistics of n draws that comes nearest to `level`:
    min(n // 2, max(1, floor((1 - level) / 2 * (n + 1) + 0.5)))."""
    return min(n // 2, max(1, int(np.floor((1.0 - level) / 2.0 * (n + 1) + 0.5))))


def coverage_from_hist(hist, level=0.9):
    """hist [..., n + 1], the rank histogram of the untied elements -> (coverage, coverage_nominal): the share of them
    whose original lies in [d_(k), d_(n+1-k)], i.e. has k <= below <= n - k, and the level (n + 1 - 2k) / (n + 1) such an
    interval has for an exchangeable ensemble.  No untied element: coverage NaN."""
    hist = np.asarray(hist)
    n = hist.shape[-1] - 1
    k = coverage_rank(n, level)
    total = hist.sum(axis=-1).astype(np.float64)
    inside = hist[..., k:n - k + 1].sum(axis=-1).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        coverage = inside / total
    return coverage, np.full(coverage.shape, (n + 1 - 2 * k) / (n + 1.0))


def calibration_from_sums(sums, hist, n_elem, level=0.9):
    """The reported figures from the kernel's sums, in float64 on the host.  sums [G, 8] in the order CALIBRATION_SUMS
    (include/nhmc.h), hist [G, n + 1], n_elem = C * H * W -> dict of CALIBRATION_KEYS, float64 [G]:
        psnr_of_mean      10 log10(4 E / sum_err2): the inverse data transform halves a difference
        spread_skill      sqrt((n + 1) / n * sum_var / sum_err2): 1 for an exchangeable ensemble, below 1 when over-confident
        z_rms             sqrt(sum_z2 / (E - n_flat))
        err_std_corr      Pearson's r between |t - mu| and s over the E elements
        coverage, coverage_nominal   `coverage_from_hist`
        n_tied, n_flat    the two counts
    A ratio over nothing is NaN (or inf), never an error."""
    sums = np.asarray(sums, dtype=np.float64)
    err2, var, aerr, std, aerr_std, z2, tied, flat = (sums[..., i] for i in range(8))
    n = np.asarray(hist).shape[-1] - 1
    E = float(n_elem)
    with np.errstate(divide='ignore', invalid='ignore'):
        cov = aerr_std / E - (aerr / E) * (std / E)
        var_a, var_s = err2 / E - (aerr / E) ** 2, var / E - (std / E) ** 2
        coverage, nominal = coverage_from_hist(hist, level)
        return dict(psnr_of_mean=10.0 * np.log10(4.0 * E / err2),
                    spread_skill=np.sqrt((n + 1.0) / n * var / err2),
                    z_rms=np.sqrt(z2 / (E - flat)),
                    err_std_corr=cov / np.sqrt(var_a * var_s),
                    coverage=coverage, coverage_nominal=nominal, n_tied=tied.copy(), n_flat=flat.copy())


def _split_counts(counts):
    return counts & 0xFFFF, counts >> 16                                     # below + 65536 * equal, both <= 1024


def calibration(samples, x_orig, replicas=1, level=0.9):
    """Where the original lies in the sample cloud (the definition is in include/nhmc.h).  samples [G * K, S, C, H, W] with
    2 <= K * S <= 1024, x_orig [G, C, H, W] -> dict: the device maps `z` (float32 [G, C, H, W]: (original - mean) / std
    of the image's K * S pooled draws; +-inf or NaN where they are all equal), `below`, `equal` (int32: draws below / equal
    to the original), `hist` (numpy int64 [G, K * S + 1], the rank histogram of the untied elements) and CALIBRATION_KEYS
    as float64 numpy [G] at the central interval nearest to `level`, with one device->host read."""
    samples, x_orig, _ = _block(samples, x_orig)
    z, counts, hist, sums = K.calibration(samples, x_orig, replicas)
    host = torch.cat([sums, hist.double()], dim=1).cpu().numpy()             # the one read; counts <= E are exact in fp64
    return _calibration_result(z, counts, host, z[0].numel(), level)


def _calibration_result(z, counts, host, n_elem, level):
    hist = np.rint(host[:, 8:]).astype(np.int64)
    below, equal = _split_counts(counts)
    return dict(z=z, below=below, equal=equal, hist=hist, **calibration_from_sums(host[:, :8], hist, n_elem, level))


def _no_calibration(G):
    return dict(z=None, below=None, equal=None, hist=None, **{k: np.full(G, np.nan) for k in CALIBRATION_KEYS})


CREDIBLE_KEYS = ('ci_rank', 'ci_level', 'ci_width_mean', 'ci_width_max', 'psnr_of_median', 'ci_inside', 'n_point', 'n_nan')
CREDIBLE_SUMS = ('sum_width', 'max_width', 'sum_err2_median', 'n_inside', 'n_point', 'n_nan')


def credible_from_sums(sums, n, k, n_elem):
    """The reported figures from the kernel's summary, in float64 on the host.  sums [G, 6] in the order CREDIBLE_SUMS
    (include/nhmc.h), n pooled draws, k the interval's rank, n_elem = C * H * W = E -> dict of CREDIBLE_KEYS, float64 [G]:
        ci_rank           k: the interval is [d_(k), d_(n+1-k)]
        ci_level          (n + 1 - 2k) / (n + 1), the same number as `coverage_nominal`
        ci_width_mean     sum_width / (2 E), ci_width_max = max_width / 2: on the [0, 1] image scale, the inverse data
                          transform halves a difference
        psnr_of_median    10 log10(4 E / sum_err2_median), the convention of `psnr_of_mean`
        ci_inside         n_inside / E: the share of the elements whose original lies in the interval, ties included
        n_point, n_nan    the two counts: elements whose interval is a point, elements whose upper bound is NaN
    A ratio over nothing is NaN (or inf), never an error."""
    sums = np.asarray(sums, dtype=np.float64)
    width, wmax, err2, inside, point, nan = (sums[..., i] for i in range(6))
    E = float(n_elem)
    with np.errstate(divide='ignore', invalid='ignore'):
        return dict(ci_rank=np.full(width.shape, float(k)), ci_level=np.full(width.shape, (n + 1 - 2 * k) / (n + 1.0)),
                    ci_width_mean=width / (2.0 * E), ci_width_max=wmax / 2.0,
                    psnr_of_median=10.0 * np.log10(4.0 * E / err2), ci_inside=inside / E, n_point=point.copy(),
                    n_nan=nan.copy())


def credible(samples, x_orig=None, replicas=1, level=0.9):
    """The central credible interval and the median of an image's pooled draws, per element (the definition is in
    include/nhmc.h).  samples [G * K, S, C, H, W] with 2 <= K * S <= 1024, x_orig [G, C, H, W] or None -> dict: the device
    maps `lower`, `median`, `upper` (float32 [G, C, H, W]: d_(k), the median and d_(n+1-k) of the n = K * S draws, with
    k = coverage_rank(n, level): the interval whose coverage `calibration` reports at the same level) and CREDIBLE_KEYS as
    float64 numpy [G], with one device->host read.  Without x_orig, psnr_of_median and ci_inside are NaN."""
    samples, x_orig, _ = _block(samples, x_orig)
    n = int(replicas) * samples.shape[1]
    k = coverage_rank(n, level)
    lower, median, upper, sums = K.credible(samples, x_orig, replicas, k)
    return dict(lower=lower, median=median, upper=upper, **credible_from_sums(sums.cpu().numpy(), n, k, lower[0].numel()))


def _no_credible(G):
    return dict(lower=None, median=None, upper=None, **{k: np.full(G, np.nan) for k in CREDIBLE_KEYS})


PCS_KEYS = ('pc_count', 'pc_rank', 'pc_var_first', 'pc_var_top', 'pc_eff_rank', 'pc_err_in_span', 'pc_z_rms')
PCS_MAX_N, PCS_MAX_COUNT = 256, 8
PCS_RANK_TOL = 1e-12                          # an eigenvalue counts while it is above this share of the first


def pcs_from_gram(gram, count=3):
    """The principal components of the sample covariance from the kernel's Gram matrix, in float64 numpy on the host.
    gram [G, n, n] (include/nhmc.h: rows u_1 ... u_{n-1} = d_{i+1} - d_1 and u_n = t - d_1, the last NaN without an
    original) -> dict of PCS_KEYS as float64 [G], `eigenvalues` [G, n - 1] (descending) and `coef` [G, count, n], the
    coefficients `kernels.sample_project` turns into sqrt(lambda_j) v_j: one posterior standard deviation along
    component j, in image units.

    With u_0 = 0 the centred Gram of the n draws is C = J Sd J, J = I - 11^T / n, Sd the Gram of u_0 ... u_{n-1}; its
    eigenpairs (lambda (n - 1), V) give the covariance's: lambda_j and the unit direction v_j = sum_i a_ji (d_i - d_1) with
    a_j = V[:, j] / sqrt((n - 1) lambda_j), whose sum is 0.  Sign: the coefficient of largest magnitude is positive, the
    lowest index winning a tie.  With eps = t - mean and q_j = <eps, v_j>, both from the Gram's last row:
        pc_rank          #{lambda_j > 1e-12 lambda_1}; 0 if lambda_1 <= 0 or the draws' Gram holds a non-finite value
        pc_count         min(count, pc_rank): the directions served, the other rows of `coef` are zero
        pc_var_first     lambda_1 / sum lambda,  pc_var_top = sum_{j <= pc_count} lambda_j / sum lambda
        pc_eff_rank      (sum lambda)^2 / sum lambda^2
        pc_err_in_span   sum_{j <= pc_rank} q_j^2 / |eps|^2: the share of the error inside the samples' span
        pc_z_rms         sqrt(mean_{j <= pc_count} q_j^2 / lambda_j): 1 when the error along the components is the size
                         they predict -- the correlated counterpart of `z_rms`
    The last two are NaN without an original or with |eps|^2 = 0; everything but the two counts is NaN at rank 0."""
    gram = np.asarray(gram, dtype=np.float64)
    G, n = gram.shape[0], gram.shape[-1]
    count = int(count)
    out = {k: np.full(G, np.nan) for k in PCS_KEYS}
    out['pc_count'], out['pc_rank'] = np.zeros(G), np.zeros(G)
    eigenvalues, coef = np.full((G, n - 1), np.nan), np.zeros((G, count, n))
    centre = np.eye(n) - np.full((n, n), 1.0 / n)
    for g in range(G):
        Sd = np.zeros((n, n))
        Sd[1:, 1:] = gram[g, :n - 1, :n - 1]
        if not np.isfinite(Sd).all():
            continue
        lam, V = np.linalg.eigh(centre @ Sd @ centre / (n - 1.0))
        lam, V = lam[::-1][:n - 1], V[:, ::-1][:, :n - 1]
        eigenvalues[g] = lam
        if not np.isfinite(lam).all() or not lam[0] > 0.0:
            continue
        rank = int((lam > PCS_RANK_TOL * lam[0]).sum())
        served = min(count, rank)
        total = lam.sum()
        a = V[:, :rank] / np.sqrt((n - 1.0) * lam[:rank])                    # [n, rank]: unit directions
        big = np.abs(a).argmax(axis=0)
        a = a * np.where(a[big, np.arange(rank)] < 0.0, -1.0, 1.0)
        coef[g, :served] = (a[:, :served] * np.sqrt(lam[:served])).T
        out['pc_count'][g], out['pc_rank'][g] = served, rank
        out['pc_var_first'][g], out['pc_var_top'][g] = lam[0] / total, lam[:served].sum() / total
        out['pc_eff_rank'][g] = total * total / (lam * lam).sum()
        last = gram[g, n - 1]
        if not np.isfinite(last).all():
            continue
        gw = np.concatenate([[0.0], last[:n - 1]])                            # <t - d_1, u_i>, i = 0 ... n - 1
        eps2 = last[n - 1] - 2.0 * gw.mean() + Sd.mean()                      # |t - d_1 - mean u|^2
        if not eps2 > 0.0:
            continue
        q = a.T @ (gw - Sd.mean(axis=0))                                      # sum a_j = 0: the mean's own part drops out
        out['pc_err_in_span'][g] = (q * q).sum() / eps2
        out['pc_z_rms'][g] = np.sqrt((q[:served] ** 2 / lam[:served]).mean())
    return dict(out, eigenvalues=eigenvalues, coef=coef)


def _pcs_count(count):
    count = int(count)
    if not 1 <= count <= PCS_MAX_COUNT:
        raise _lib.NhmcError(f'pcs: count must be 1 ... {PCS_MAX_COUNT}, got {count}')
    return count


def _pcs_result(samples, replicas, host_gram, count):
    """The host part after the read: the eigen-solve, then the projection with uploaded coefficients."""
    res = pcs_from_gram(host_gram, count)
    coef = torch.from_numpy(np.ascontiguousarray(res.pop('coef'))).to(samples.device)
    return dict(directions=K.sample_project(samples, coef, replicas), eigenvalues=res.pop('eigenvalues'), **res)


def pcs(samples, x_orig=None, replicas=1, count=3):
    """The principal components of an image's pooled draws (the Gram matrix is defined in include/nhmc.h, the figures in
    `pcs_from_gram`).  samples [G * K, S, C, H, W] with 2 <= K * S <= 256, x_orig [G, C, H, W] or None, 1 <= count <= 8
    -> dict: `directions` (device, float32 [G, count, C, H, W]: sqrt(lambda_j) v_j, zero past pc_count), `eigenvalues`
    (float64 numpy [G, K * S - 1]) and PCS_KEYS as float64 numpy [G], with one device->host read.  Nothing of the size of
    the covariance is formed: the n x n Gram matrix comes from the device, its eigenvectors from numpy."""
    samples, x_orig, _ = _block(samples, x_orig)
    count = _pcs_count(count)
    gram = K.sample_gram(samples, x_orig, replicas)
    return _pcs_result(samples, replicas, gram.cpu().numpy(), count)


def _no_pcs(G):
    return dict(directions=None, eigenvalues=None, **{k: np.full(G, np.nan) for k in PCS_KEYS})


def summarize(samples, x_orig, replicas=1, rhat_threshold=1.1, calibration=None, credible=None, pcs=None):
    """Everything the report prints or saves for B chains with S samples each, with one device->host read.

    -> dict of float64 numpy arrays [B]: psnr_mean, psnr_std, ssim_mean, ssim_std (np.mean / np.std(ddof=1) over the
    chain's samples, :526-538; std is 0 for S = 1), std_map_min, std_map_max; `n_samples` (int); and the device tensors
    mean [B, C, H, W], std_map, std_map_normalised [B, H, W].  S = 1: PSNR and SSIM but no map (the reference's
    `len(xt) > 1`): the three tensors are None and the map's min / max NaN.  S = 0: all scalars NaN but the stds, which
    are 0 -- the CLI's row for a chain whose final phase collected nothing.

    replicas = K > 1: samples is [G * K, S, C, H, W] (chain g * K + r is replica r of image g) and x_orig [G, C, H, W].
    Everything above is then per image over its K * S pooled samples (`n_samples` = K * S; the block is contiguous, so
    pooling is a view), and the dict gains `replicas`, CONVERGENCE_KEYS as float64 numpy [G] and the device maps `rhat`,
    `ess` [G, C, H, W].  With S < 4 split R-hat is undefined: the summaries are NaN and the two maps None.

    calibration = level (0.9, say; None, the default, changes nothing): the dict gains what `calibration` returns for the
    pooled K * S samples -- `z`, `below`, `equal`, `hist` and CALIBRATION_KEYS -- in the same single read.  With fewer
    than two pooled samples the four are None and the figures NaN.

    credible = level (None, the default, changes nothing): the dict gains, after everything else, what `credible` returns
    for the pooled K * S samples -- `lower`, `median`, `upper` and CREDIBLE_KEYS -- in the same single read.  With fewer
    than two pooled samples the three maps are None and the figures NaN.

    pcs = count (None, the default, changes nothing): the dict gains, after everything else, what `pcs` returns for the
    pooled K * S samples -- `directions`, `eigenvalues` and PCS_KEYS.  The Gram matrix rides in the same single read; the
    projection is launched after it with uploaded coefficients.  With fewer than two or more than 256 pooled samples
    `directions` and `eigenvalues` are None and the figures NaN."""
    replicas = int(replicas)
    if replicas == 1 and calibration is None and credible is None and pcs is None:
        return _summarize(samples, x_orig)
    samples, x_orig, _ = _block(samples, x_orig)
    B, S = samples.shape[:2]
    if replicas < 1 or B % replicas:
        raise _lib.NhmcError(f'summarize: {B} chains are not a multiple of {replicas} replicas')
    G = B // replicas
    diag = K.chain_diag(samples, replicas, rhat_threshold) if replicas > 1 and S >= 4 else None
    cal = K.calibration(samples, x_orig, replicas) if calibration is not None and replicas * S >= 2 else None
    n = replicas * S
    rank = coverage_rank(n, credible) if credible is not None and n >= 2 else None
    cred = None if rank is None else K.credible(samples, x_orig, replicas, rank)
    count = None if pcs is None else _pcs_count(pcs)
    gram = K.sample_gram(samples, x_orig, replicas) if count is not None and 2 <= n <= PCS_MAX_N else None
    extra = ([] if diag is None else [diag[2]]) + ([] if cal is None else [cal[3], cal[2].double()]) + \
        ([] if cred is None else [cred[3]]) + ([] if gram is None else [gram.reshape(G, n * n)])
    out = _summarize(samples.reshape((G, replicas * S) + tuple(samples.shape[2:])), x_orig,
                     extra=torch.cat(extra, dim=1) if extra else None)
    host = out.pop('extra', None)
    if replicas > 1:
        out['replicas'] = replicas
        out['rhat'], out['ess'] = (None, None) if diag is None else diag[:2]
        for i, k in enumerate(CONVERGENCE_KEYS):
            out[k] = np.full(G, np.nan) if diag is None else host[:, i].copy()
    # the blocks of `extra`, in its order; each one that rode along moves the offset on, whatever the other flags are
    at = 0 if diag is None else len(CONVERGENCE_KEYS)
    at_cal, at = at, at + (0 if cal is None else len(CALIBRATION_SUMS) + n + 1)
    at_cred, at = at, at + (0 if cred is None else len(CREDIBLE_SUMS))
    at_gram = at
    if calibration is not None:
        out.update(_no_calibration(G) if cal is None else _calibration_result(
            cal[0], cal[1], host[:, at_cal:at_cred], cal[0][0].numel(), calibration))
    if credible is not None:
        out.update(_no_credible(G) if cred is None else dict(
            lower=cred[0], median=cred[1], upper=cred[2],
            **credible_from_sums(host[:, at_cred:at_gram], n, rank, cred[0][0].numel())))
    if count is not None:
        out.update(_no_pcs(G) if gram is None else _pcs_result(
            samples, replicas, host[:, at_gram:at_gram + n * n].reshape(G, n, n), count))
    return out


def _summarize(samples, x_orig, extra=None):
    """`summarize` for one replica per image; `extra` (float64 [B, n] on the device) rides along in the one read and
    comes back as out['extra']."""
    samples, x_orig, _ = _block(samples, x_orig)
    B, S = samples.shape[:2]
    nan, zero = np.full(B, np.nan), np.zeros(B)
    out = dict(psnr_mean=nan, psnr_std=zero, ssim_mean=nan.copy(), ssim_std=zero.copy(), std_map_min=nan.copy(),
               std_map_max=nan.copy(), n_samples=S, mean=None, std_map=None, std_map_normalised=None)
    if extra is not None:
        out['extra'] = None
    if S == 0:
        return out
    cols = [psnr(samples, x_orig).double(), ssim(samples, x_orig)]
    if S > 1:
        out['mean'], out['std_map'], minmax, out['std_map_normalised'], _ = _moments(samples)
        cols.append(minmax.double())
    n_own = sum(c.shape[1] for c in cols)
    if extra is not None:
        cols.append(extra)
    host = torch.cat(cols, dim=1).cpu().numpy()                              # the one read: [B, 2S (+2) (+n)]
    ps, ss = host[:, :S], host[:, S:2 * S]
    out['psnr_mean'], out['ssim_mean'] = ps.mean(axis=1), ss.mean(axis=1)
    if S > 1:
        out['psnr_std'], out['ssim_std'] = ps.std(axis=1, ddof=1), ss.std(axis=1, ddof=1)
        out['std_map_min'], out['std_map_max'] = host[:, 2 * S], host[:, 2 * S + 1]
    if extra is not None:
        out['extra'] = host[:, n_own:]
    return out


HOT_BREAKS = (0.365079, 0.746032)          # where matplotlib's `hot` ramp saturates red, then green


def hot_colours(map01):
    """matplotlib's `hot` colour map written out: [H, W] in [0, 1] -> uint8 [H, W, 3]."""
    v = np.asarray(map01, dtype=np.float64)
    r, g = HOT_BREAKS
    rgb = np.stack([v / r, (v - r) / (g - r), (v - g) / (1.0 - g)], axis=-1)
    return np.round(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)


def save_std_map(map01, path):
    """The normalised std map [H, W] as an 8-bit PNG in the `hot` colours, one pixel per map entry.

    Deviation from main_sampling.py:499-507: the reference draws the map into a matplotlib figure with a colour bar
    ("Std Dev") and the title "Pixel-wise Std Dev Across Samples" at 300 dpi; this writes the picture alone -- no colour
    bar, no title, no matplotlib."""
    from PIL import Image
    if isinstance(map01, torch.Tensor):
        map01 = map01.detach().cpu().numpy()
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(hot_colours(map01)).save(path)


def save_rhat_map(rhat, path):
    """The R-hat map of one image, [C, H, W] (or [H, W]), as an 8-bit PNG in the `hot` colours: the maximum over the
    channels, mapped clip((r - 1) / 0.5, 0, 1) -- black at R-hat <= 1, white from 1.5.  A constant element (NaN) maps to 0,
    chains stuck at different constants (+inf) to 1."""
    from PIL import Image
    if isinstance(rhat, torch.Tensor):
        rhat = rhat.detach().cpu().numpy()
    r = np.asarray(rhat, dtype=np.float64)
    if r.ndim == 3:
        r = np.fmax.reduce(r, axis=0)                                        # the maximum that ignores NaN
    map01 = np.clip((np.nan_to_num(r, nan=1.0, posinf=np.inf) - 1.0) / 0.5, 0.0, 1.0)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(hot_colours(map01)).save(path)


def save_calibration_map(z, path):
    """The z-score map of one image, [C, H, W] (or [H, W]), as an 8-bit PNG in the `hot` colours: the maximum over the
    channels of |z|, mapped clip(|z| / 3, 0, 1) -- black where the original sits at the mean of the draws, white from three
    standard deviations.  NaN (all draws equal to the original) maps to 0, inf (all draws equal, the original elsewhere)
    to 1."""
    from PIL import Image
    if isinstance(z, torch.Tensor):
        z = z.detach().cpu().numpy()
    a = np.nan_to_num(np.abs(np.asarray(z, dtype=np.float64)), nan=0.0, posinf=np.inf)
    if a.ndim == 3:
        a = a.max(axis=0)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(hot_colours(np.clip(a / 3.0, 0.0, 1.0))).save(path)


def save_ci_width_map(lower, upper, path):
    """The width of one image's credible interval, `upper - lower` [C, H, W] (or [H, W]), as an 8-bit PNG in the `hot`
    colours: the mean over the channels, min-max normalised -- the std map's picture (`save_std_map`) of the interval, so
    that the two can be laid side by side.  A map that is flat, or holds a NaN width, has no range and comes out black."""
    from PIL import Image
    width = (upper - lower).float()
    if width.dim() == 3:
        width = width.mean(dim=0)
    width = width[None].contiguous()
    minmax = torch.stack([width.min(), width.max()])[None].contiguous()
    map01 = np.nan_to_num(K.std_map_normalise(width, minmax)[0].cpu().numpy(), nan=0.0, posinf=1.0, neginf=0.0)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    Image.fromarray(hot_colours(map01)).save(path)

"""CPU: the calibration report without a device -- a two-pass float64 numpy restatement of the definition in include/nhmc.h
("Calibration of the posterior samples"; tests/test_calib_gpu.py holds the kernel to it), the host functions that turn the
kernel's sums and rank histogram into the reported figures, and the CLI's host side: the flag, the columns, the lines."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = ('sum_err2', 'sum_var', 'sum_abs_err', 'sum_std', 'sum_abs_err_std', 'sum_z2', 'n_tied', 'n_flat')


def calib_float64(draws, truth):
    """draws [n, E] (the pooled draws of one image, d_1 first), truth [E] -> dict, float64 and two-pass throughout: below,
    equal [E]; mu, s, z [E] (flat = all draws equal: v = 0 exactly; z = +-inf or NaN there); hist [n + 1] over the untied
    elements; and the eight per-image sums of the header under their names."""
    x32, t32 = np.asarray(draws), np.asarray(truth)
    d, t = x32.astype(np.float64), t32.astype(np.float64)
    n, E = d.shape
    below, equal = (x32 < t32).sum(axis=0), (x32 == t32).sum(axis=0)
    mu = d.sum(axis=0) / n
    v = ((d - mu) ** 2).sum(axis=0) / (n - 1)
    flat = (d == d[0]).all(axis=0)
    v[flat] = 0.0
    mu[flat] = d[0][flat]
    s = np.sqrt(v)
    with np.errstate(divide='ignore', invalid='ignore'):
        z = (t - mu) / s
    err = np.abs(t - mu)
    return dict(below=below, equal=equal, mu=mu, s=s, z=z, hist=np.bincount(below[equal == 0], minlength=n + 1),
                sum_err2=float((err ** 2).sum()), sum_var=float(v.sum()), sum_abs_err=float(err.sum()), sum_std=float(s.sum()),
                sum_abs_err_std=float((err * s).sum()), sum_z2=float((z[s > 0] ** 2).sum()), n_tied=int((equal > 0).sum()),
                n_flat=int((s == 0).sum()))


def sums_of(ref):
    return np.array([[ref[k] for k in SUMS]], dtype=np.float64)


# ---- the restatement on inputs whose answer is known ----------------------------------------------------------------
def test_restatement_on_a_hand_built_case():
    draws = np.array([[0.0, 1.0, -1.0, 0.5], [2.0, 1.0, -1.0, 0.25], [4.0, 1.0, -1.0, 0.0]], dtype=np.float32)
    truth = np.array([3.0, 1.0, -0.25, 0.25], dtype=np.float32)
    got = calib_float64(draws, truth)
    assert got['below'].tolist() == [2, 0, 3, 1] and got['equal'].tolist() == [0, 3, 0, 1]
    assert got['mu'].tolist() == [2.0, 1.0, -1.0, 0.25] and got['s'].tolist() == [2.0, 0.0, 0.0, 0.25]
    assert got['z'][0] == 0.5 and np.isnan(got['z'][1]) and np.isposinf(got['z'][2]) and got['z'][3] == 0.0
    assert got['hist'].tolist() == [0, 0, 1, 1]                               # elements 0 and 2; 1 and 3 are tied
    assert (got['n_tied'], got['n_flat']) == (2, 2)
    assert got['sum_err2'] == 1.0 + 0.75 ** 2 and got['sum_var'] == 4.0 + 0.0625 and got['sum_z2'] == 0.25
    assert got['sum_abs_err'] == 1.75 and got['sum_std'] == 2.25 and got['sum_abs_err_std'] == 2.0


# ---- coverage from hand-built histograms ------------------------------------------------------------------------------
def test_coverage_rank_and_nominal_level():
    from nhmc import metrics
    assert [metrics.coverage_rank(20, lv) for lv in (0.9, 0.8, 0.5)] == [1, 2, 5]
    assert metrics.coverage_rank(2, 0.9) == 1 and metrics.coverage_rank(2, 0.1) == 1          # capped at n // 2
    assert metrics.coverage_rank(3, 0.0) == 1 and metrics.coverage_rank(1024, 0.9) == 51
    hist = np.arange(1, 22, dtype=np.int64)                                   # n = 20: bin b holds b + 1 elements
    total = hist.sum()
    for level, k in ((0.9, 1), (0.8, 2), (0.5, 5)):
        cov, nom = metrics.coverage_from_hist(hist, level)
        assert nom == (21 - 2 * k) / 21.0
        assert cov == hist[k:20 - k + 1].sum() / total
    cov, nom = metrics.coverage_from_hist(hist, 0.9)
    assert nom == 19.0 / 21.0 and cov == (total - 1 - 21) / total
    cov, nom = metrics.coverage_from_hist(np.array([[3, 5, 2], [0, 0, 0]]), 0.9)          # n = 2, two images, one empty
    assert cov[0] == 0.5 and np.isnan(cov[1]) and nom.tolist() == [1.0 / 3.0, 1.0 / 3.0]


def test_derivation_from_the_sums_agrees_with_the_restatement():
    """The host derivation from the eight sums and the histogram against the same figures taken directly from the
    restatement's per-element values (np.corrcoef, np.mean): float64 on both sides, 1e-9 relative covers the one-pass
    Pearson form's cancellation (r around 0.1 to 0.9 here, so a factor of ten at most over the 1e-16 of the sums)."""
    from nhmc import metrics
    rng = np.random.default_rng(5)
    n, E = 20, 3000
    amp = np.logspace(-2, -0.5, E)
    draws = (amp * rng.standard_normal((n, E))).astype(np.float32)
    truth = (1.5 * amp * rng.standard_normal(E)).astype(np.float32)
    draws[:, 4], truth[4] = 1.0, 1.0                                          # flat and tied
    draws[:, 8], truth[8] = -1.0, 0.0                                         # flat
    ref = calib_float64(draws, truth)
    got = metrics.calibration_from_sums(sums_of(ref), ref['hist'][None], E, 0.8)
    assert set(got) == set(metrics.CALIBRATION_KEYS) and all(v.shape == (1,) and v.dtype == np.float64 for v in got.values())
    err = np.abs(truth.astype(np.float64) - ref['mu'])
    want = dict(psnr_of_mean=10 * np.log10(1.0 / np.mean((err / 2) ** 2)),
                spread_skill=np.sqrt((n + 1) / n * np.mean(ref['s'] ** 2) / np.mean(err ** 2)),
                z_rms=np.sqrt(np.mean(ref['z'][ref['s'] > 0] ** 2)), err_std_corr=np.corrcoef(err, ref['s'])[0, 1],
                coverage=ref['hist'][2:19].sum() / ref['hist'].sum(), coverage_nominal=17.0 / 21.0, n_tied=1.0, n_flat=2.0)
    for k in metrics.CALIBRATION_KEYS:
        assert abs(got[k][0] - want[k]) <= 1e-9 * abs(want[k]), k
    assert got['spread_skill'][0] < 0.8                                       # the truth was drawn 1.5 times wider
    # nothing to divide by: NaN or inf, no exception
    empty = metrics.calibration_from_sums(np.zeros((1, 8)), np.zeros((1, 3), dtype=np.int64), 16, 0.9)
    assert np.isnan(empty['coverage'][0]) and np.isnan(empty['spread_skill'][0]) and np.isposinf(empty['psnr_of_mean'][0])


def test_exchangeable_ensemble_is_calibrated_and_a_narrow_one_is_not():
    """The restatement does its job: 21 exchangeable rows, one of them the truth."""
    from nhmc import metrics
    n, E = 20, 3 * 64 * 64
    x = (0.2 * torch.randn(n + 1, E, generator=torch.Generator().manual_seed(2024))).numpy()
    ref = calib_float64(x[1:], x[0])
    assert ref['n_tied'] == 0 and ref['n_flat'] == 0 and ref['hist'].sum() == E
    got = metrics.calibration_from_sums(sums_of(ref), ref['hist'][None], E, 0.9)
    nominal = 19.0 / 21.0
    assert got['coverage_nominal'][0] == nominal
    assert abs(got['coverage'][0] - nominal) < 4 * np.sqrt(nominal * (1 - nominal) / E)
    assert abs(got['spread_skill'][0] - 1.0) < 0.05
    assert np.abs(ref['hist'] - E / 21.0).max() < 5 * np.sqrt(E / 21.0 * (1 - 1 / 21.0))
    narrow = calib_float64(0.5 * x[1:], x[0])
    got = metrics.calibration_from_sums(sums_of(narrow), narrow['hist'][None], E, 0.9)
    assert got['coverage'][0] < nominal - 0.1 and got['spread_skill'][0] < 0.7


# ---- the picture --------------------------------------------------------------------------------------------------
def test_calibration_map_picture(tmp_path):
    from PIL import Image
    from nhmc import metrics
    z = np.zeros((3, 2, 3), dtype=np.float32)
    z[0, 0] = [0.0, -1.5, 3.0]
    z[1, 0] = [np.nan, 0.5, -7.0]
    z[:, 1, 0] = [np.nan, np.nan, np.nan]
    z[2, 1, 1] = -np.inf
    path = tmp_path / 'maps' / 'calibration_map_0.png'
    metrics.save_calibration_map(torch.from_numpy(z), str(path))
    img = np.asarray(Image.open(path))
    want = metrics.hot_colours(np.array([[0.0, 0.5, 1.0], [0.0, 1.0, 0.0]]))
    assert img.shape == (2, 3, 3) and np.array_equal(img, want)


# ---- parser, columns, report lines --------------------------------------------------------------------------------
ARGS = ['--deg', 'sr4', '--sigma_0', '0.05']


@pytest.mark.parametrize('latent', [False, True])
def test_calibration_flag(latent):
    from nhmc import cli
    parse = lambda extra: cli.get_parser(latent).parse_known_args(ARGS + extra)[0].calibration
    assert parse([]) is None
    assert parse(['--calibration']) == 0.9
    assert parse(['--calibration', '0.5']) == 0.5
    assert parse(['--calibration', '--chains', '4']) == 0.9


def test_columns():
    from nhmc import cli, metrics
    assert cli.CALIBRATION_COLUMNS == metrics.CALIBRATION_KEYS == (
        'psnr_of_mean', 'spread_skill', 'z_rms', 'err_std_corr', 'coverage', 'coverage_nominal', 'n_tied', 'n_flat')
    assert not set(cli.CALIBRATION_COLUMNS) & (set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS))
    assert {'n_tied', 'n_flat'} <= set(cli.INT_COLUMNS)


def _summary(n_samples, psnr, replicas=1, cal=None):
    col = lambda v: np.full(1, v, dtype=np.float64)
    from nhmc import metrics
    out = dict(psnr_mean=col(psnr), psnr_std=col(0.5), ssim_mean=col(0.8), ssim_std=col(0.01), std_map_min=col(0.0),
               std_map_max=col(0.2), n_samples=n_samples, mean=None, std_map=None, std_map_normalised=None)
    if replicas > 1:
        out.update(replicas=replicas, rhat=None, ess=None,
                   **{k: col(v) for k, v in zip(metrics.CONVERGENCE_KEYS, (1.3, 1.05, 0.25, 7.5, 30.0, 4.0))})
    if cal is not None:
        out.update(z=None, below=None, equal=None, hist=None, **{k: col(v) for k, v in zip(metrics.CALIBRATION_KEYS, cal)})
    return out


def test_report_lines_and_rows(tmp_path, capsys):
    """On the host: image 0 has the figures, image 1 collected one sample (NaN figures: no line, null in the JSON).  With
    replicas the calibration columns come after the replica columns; without the flag the rows are today's."""
    from nhmc import cli
    nan = float('nan')
    rows = cli._metric_rows([0], _summary(20, 25.0, cal=(27.0, 0.81, 1.4, 0.35, 0.75, 19 / 21, 3.0, 2.0)))
    rows += cli._metric_rows([1], _summary(1, 24.0, cal=(nan,) * 8))
    assert all(len(r) == len(cli.COLUMNS) + len(cli.CALIBRATION_COLUMNS) for r in rows)
    report = tmp_path / 'metrics.json'
    cli._report(rows, 2, 0, 1, torch.device('cpu'), str(report), calibration=0.9)
    out = capsys.readouterr().out
    assert ('image 0: calibration: coverage 0.7500 at nominal 0.9048, spread/skill 0.810, z rms 1.400, |err|~std r 0.350, '
            'PSNR of the posterior mean 27.000, tied 3 flat 2') in out
    assert 'image 1: PSNR 24.000' in out and 'image 1: calibration' not in out
    assert ('Total Average calibration: coverage 0.7500 at nominal 0.9048, spread/skill 0.810, z rms 1.400, '
            '|err|~std r 0.350, PSNR of the posterior mean 27.000') in out
    got = json.loads(report.read_text())
    assert tuple(got[0]) == cli.COLUMNS + cli.CALIBRATION_COLUMNS
    assert got[0]['n_tied'] == 3 and isinstance(got[0]['n_tied'], int) and isinstance(got[0]['n_flat'], int)
    assert got[0]['coverage'] == 0.75 and all(got[1][k] is None for k in cli.CALIBRATION_COLUMNS)
    rows = cli._metric_rows([0], _summary(12, 25.0, replicas=2, cal=(27.0, 0.81, 1.4, 0.35, 0.75, 11 / 13, 0.0, 0.0)))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9)
    out = capsys.readouterr().out
    assert 'image 0: R-hat max ' in out and 'image 0: calibration: coverage 0.7500 at nominal 0.8462' in out
    assert tuple(json.loads(report.read_text())[0]) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS
    rows = cli._metric_rows([0], _summary(20, 25.0))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report))
    assert 'calibration' not in capsys.readouterr().out and tuple(json.loads(report.read_text())[0]) == cli.COLUMNS


# ---- header and binding --------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    import nhmc
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('nhmc_calibration_tiles', 'nhmc_calibration_ws_bytes', 'nhmc_calibration'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in nhmc._lib.SIGNATURES
    assert len(nhmc._lib.SIGNATURES['nhmc_calibration'][1]) == 12
    assert 'Calibration of the posterior samples' in src and 'NHMC_ABI_VERSION 2' in re.sub(r'\s+', ' ', src)

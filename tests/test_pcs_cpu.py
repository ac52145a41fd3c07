"""CPU: the principal components of the posterior samples without a device -- `metrics.pcs_from_gram` (the eigen-solve of
the n x n Gram matrix of include/nhmc.h, "Principal components of the posterior samples") against a direct float64
restatement that takes the SVD of the centred block and projects the error explicitly, the degenerate inputs, the entries'
argument validation, and the CLI's host side: the flag, the columns, the lines.  tests/test_pcs_gpu.py holds the kernels to
the Gram's definition and imports the restatement from here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from test_calib_cpu import calib_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('pc_count', 'pc_rank', 'pc_var_first', 'pc_var_top', 'pc_eff_rank', 'pc_err_in_span', 'pc_z_rms')
GAP = 0.05                                   # directions are compared where (lambda_j - lambda_{j+1}) / lambda_1 >= GAP


def gram_float64(draws, truth=None):
    """draws [n, E] (the pooled draws of one image, d_1 first), truth [E] or None -> [n, n] float64, the header's
    definition: rows u_1 ... u_{n-1} = d_{i+1} - d_1 and u_n = t - d_1 (NaN without an original), G = U U^T."""
    d = np.asarray(draws).astype(np.float64)
    n, E = d.shape
    last = np.full(E, np.nan) if truth is None else np.asarray(truth).astype(np.float64) - d[0]
    U = np.concatenate([d[1:] - d[0], last[None]], axis=0)
    with np.errstate(invalid='ignore'):
        return U @ U.T


def pcs_float64(draws, truth=None, count=3):
    """The restatement: the SVD of the centred draws.  -> dict of KEYS (floats), `eigenvalues` [n - 1], `directions`
    [pc_count, E] (unit vectors, signed by the rule: the draw with the coefficient of largest magnitude counts positive --
    the coefficients of v_j over the centred draws are U[:, j] / s_j) and `gaps` [n - 1], (lambda_j - lambda_{j+1}) /
    lambda_1 with lambda_n = 0."""
    d = np.asarray(draws).astype(np.float64)
    n, E = d.shape
    mean = d.mean(axis=0)
    Uu, s, Vt = np.linalg.svd(d - mean, full_matrices=False)
    lam = (s * s / (n - 1.0))[:n - 1]
    nan = float('nan')
    out = dict(pc_count=0, pc_rank=0, pc_var_first=nan, pc_var_top=nan, pc_eff_rank=nan, pc_err_in_span=nan, pc_z_rms=nan,
               eigenvalues=lam, directions=np.zeros((0, E)), gaps=np.zeros(n - 1))
    if not (np.isfinite(lam).all() and lam[0] > 0.0):
        return out
    rank = int((lam > 1e-12 * lam[0]).sum())
    served = min(count, rank)
    sign = np.array([1.0 if Uu[np.abs(Uu[:, j]).argmax(), j] > 0.0 else -1.0 for j in range(rank)])
    V = Vt[:rank] * sign[:, None]
    out.update(pc_count=served, pc_rank=rank, pc_var_first=lam[0] / lam.sum(), pc_var_top=lam[:served].sum() / lam.sum(),
               pc_eff_rank=lam.sum() ** 2 / (lam * lam).sum(), directions=V[:served],
               gaps=(lam - np.append(lam[1:], 0.0)) / lam[0])
    if truth is not None:
        eps = np.asarray(truth).astype(np.float64) - mean
        if eps @ eps > 0.0:
            q = V @ eps
            out.update(pc_err_in_span=(q * q).sum() / (eps @ eps), pc_z_rms=np.sqrt((q[:served] ** 2 / lam[:served]).mean()))
    return out


def ensemble(n, E, seed, noise=None, n_dir=3):
    """-> (draws [n, E], truth [E], basis [min(n_dir, n - 1), E]) float64: draws = base + Z diag(1, 1/2, 1/4 ...) W + noise,
    W orthonormal rows, Z centred orthogonal score columns of norm sqrt(n - 1), so that without the noise floor the
    covariance's eigenvalues are exactly 1, 1/4, 1/16; the truth sits off the mean along every direction and outside.
    The floor: white noise of total variance `noise`^2, by default 1e-3 (n - 1), which puts the floor's eigenvalues near
    1e-3 of the first.  A Gram matrix squares the condition number: an eigenpair of the floor comes out of it with a relative
    error near 2^-52 n lambda_1 / lambda_floor, so a floor at 1e-3 leaves the 1e-10 these tests ask for two orders of
    room at n = 160, while one at 1e-6 would not (and no fp32 sample block has one: fp32 rounding alone is 1e-7)."""
    rng = np.random.default_rng(seed)
    k = min(n_dir, n - 1)
    noise = np.sqrt(1e-3 * (n - 1)) if noise is None else noise
    W = np.linalg.qr(rng.standard_normal((E, k + 1)))[0].T                     # k directions and one for the truth
    Z = rng.standard_normal((n, k))
    Z = np.linalg.qr(Z - Z.mean(axis=0))[0] * np.sqrt(n - 1.0)
    scales = 0.5 ** np.arange(k)
    base = rng.uniform(-0.5, 0.5, E)
    draws = base + (Z * scales) @ W[:k] + noise / np.sqrt(E) * rng.standard_normal((n, E))
    truth = draws.mean(axis=0) + (np.array([0.7, -0.4, 0.2])[:k] * scales) @ W[:k] + 0.3 * W[k]
    return draws, truth, W[:k]


def directions_of(res, draws, g=0):
    """Unit directions from `pcs_from_gram`'s coefficient block: coef_j (d - d_1) = sqrt(lambda_j) v_j."""
    c = int(res['pc_count'][g])
    d = np.asarray(draws, dtype=np.float64)
    return (res['coef'][g, :c] @ (d - d[0])) / np.sqrt(res['eigenvalues'][g, :c])[:, None]


def rel(a, b):
    return abs(a - b) / abs(b)


ENSEMBLES = [(2, 192), (3, 200), (20, 768), (65, 1200), (160, 1000)]


@pytest.mark.parametrize('n,E', ENSEMBLES)
def test_derivation_against_the_svd(n, E):
    from nhmc import metrics
    draws, truth, _ = ensemble(n, E, seed=n)
    ref = pcs_float64(draws, truth, 3)
    got = metrics.pcs_from_gram(gram_float64(draws, truth)[None], 3)
    assert tuple(got)[:len(KEYS)] == KEYS == metrics.PCS_KEYS and got['eigenvalues'].shape == (1, n - 1)
    assert got['coef'].shape == (1, 3, n)
    print(f'n {n} E {E}:', {k: (float(got[k][0]), ref[k]) for k in KEYS}, 'gaps', ref['gaps'][:3])
    assert got['pc_count'][0] == ref['pc_count'] == min(3, n - 1) and got['pc_rank'][0] == ref['pc_rank'] == n - 1
    assert np.all(np.abs(got['eigenvalues'][0] - ref['eigenvalues']) <= 1e-10 * ref['eigenvalues'])
    for k in KEYS[2:]:
        assert rel(got[k][0], ref[k]) <= 1e-10, k
    c = ref['pc_count']
    assert np.all(ref['gaps'][:c] >= GAP)                                       # every compared direction is well separated
    v = directions_of(got, draws)
    for j in range(c):
        assert abs(np.linalg.norm(v[j]) - 1.0) <= 1e-9
        assert v[j] @ ref['directions'][j] >= 1.0 - 1e-9                        # the sign rule gives the same sign
        big = np.abs(got['coef'][0, j]).argmax()
        assert got['coef'][0, j, big] > 0.0 and abs(got['coef'][0, j].sum()) <= 1e-12 * np.abs(got['coef'][0, j]).sum() * n
    assert np.all(got['coef'][0, c:] == 0.0)                                    # missing directions: zero coefficients
    # without the original the variance figures keep their bits and the two error figures are NaN
    bare = metrics.pcs_from_gram(gram_float64(draws)[None], 3)
    for k in KEYS[:5]:
        assert bare[k][0] == got[k][0], k
    assert np.isnan(bare['pc_err_in_span'][0]) and np.isnan(bare['pc_z_rms'][0])
    assert np.array_equal(bare['coef'], got['coef']) and np.array_equal(bare['eigenvalues'], got['eigenvalues'])


def test_several_images_and_counts():
    from nhmc import metrics
    sets = [ensemble(20, 300, seed=s) for s in (1, 2, 3)]
    gram = np.stack([gram_float64(d, t) for d, t, _ in sets])
    for count in (1, 3, 8):
        got = metrics.pcs_from_gram(gram, count)
        assert got['coef'].shape == (3, count, 20)
        for g, (d, t, _) in enumerate(sets):
            ref = pcs_float64(d, t, count)
            assert got['pc_count'][g] == count == ref['pc_count']
            for k in KEYS[2:]:
                assert rel(got[k][g], ref[k]) <= 1e-10, (count, g, k)


def test_exact_low_rank_case():
    """Three directions and no noise: rank 3 exactly, all the variance in them; an error inside the span is all inside, one
    orthogonal to it all outside."""
    from nhmc import metrics
    draws, _, W = ensemble(20, 400, seed=5, noise=0.0)
    mean = draws.mean(axis=0)
    inside = mean + 0.3 * W[0] - 0.2 * W[1] + 0.1 * W[2]
    other = np.linalg.qr(np.concatenate([W, np.random.default_rng(9).standard_normal((1, 400))]).T)[0].T[3]
    assert np.abs(W @ other).max() <= 1e-14
    got = metrics.pcs_from_gram(np.stack([gram_float64(draws, inside), gram_float64(draws, mean + 0.25 * other)]), 3)
    print({k: got[k].tolist() for k in KEYS})
    assert got['pc_rank'].tolist() == [3.0, 3.0] and got['pc_count'].tolist() == [3.0, 3.0]
    assert np.all(got['pc_eff_rank'] <= 3.0) and np.all(np.abs(got['pc_var_top'] - 1.0) <= 1e-12)
    assert np.all(np.abs(got['eigenvalues'][:, :3] - np.array([1.0, 0.25, 0.0625])) <= 1e-12)
    assert abs(got['pc_err_in_span'][0] - 1.0) <= 1e-12 and abs(got['pc_err_in_span'][1]) <= 1e-12
    want = np.sqrt(((0.3 / 1.0) ** 2 + (0.2 / 0.5) ** 2 + (0.1 / 0.25) ** 2) / 3.0)
    assert abs(got['pc_z_rms'][0] - want) <= 1e-12 and got['pc_z_rms'][1] <= 1e-6


@pytest.mark.parametrize('n,E', [(20, 768), (65, 1200)])
def test_total_variance_is_the_calibration_definitions(n, E):
    """sum lambda = the trace of the covariance = the calibration definition's sum_var on the same block."""
    from nhmc import metrics
    draws, truth, _ = ensemble(n, E, seed=100 + n)
    d32, t32 = draws.astype(np.float32), truth.astype(np.float32)
    got = metrics.pcs_from_gram(gram_float64(d32, t32)[None], 3)
    want = calib_float64(d32, t32)['sum_var']
    assert rel(got['eigenvalues'][0].sum(), want) <= 1e-12


def test_degenerate_inputs():
    from nhmc import metrics
    flat = np.full((5, 64), 0.25)
    truth = np.linspace(-1, 1, 64)
    draws, _, _ = ensemble(5, 64, seed=3)
    poisoned = gram_float64(draws, truth)
    poisoned[1, :] = poisoned[:, 1] = np.nan                                   # a NaN draw
    good = gram_float64(draws, truth)
    got = metrics.pcs_from_gram(np.stack([gram_float64(flat, truth), poisoned, good]), 3)
    for g in (0, 1):
        assert got['pc_count'][g] == 0 and got['pc_rank'][g] == 0
        assert all(np.isnan(got[k][g]) for k in KEYS[2:]) and np.all(got['coef'][g] == 0.0)
    assert got['pc_count'][2] == 3 and got['pc_rank'][2] == 4 and all(np.isfinite(got[k][2]) for k in KEYS)
    # the original at the mean: the variance figures stand, the error has no direction
    at_mean = metrics.pcs_from_gram(gram_float64(draws, draws.mean(axis=0))[None], 3)
    assert at_mean['pc_count'][0] == 3 and np.isfinite(at_mean['pc_var_first'][0])


# ---- report plumbing -------------------------------------------------------------------------------------------------
ARGS = ['--deg', 'sr4', '--sigma_0', '0.05']


@pytest.mark.parametrize('latent', [False, True])
def test_pcs_flag(latent, capsys):
    from nhmc import cli
    parse = lambda extra: cli.get_parser(latent).parse_known_args(ARGS + extra)
    assert parse([])[0].pcs is None
    assert parse(['--pcs'])[0].pcs == 3 and parse(['--pcs'])[1] == []
    assert parse(['--pcs', '5'])[0].pcs == 5 and parse(['--pcs', '1'])[0].pcs == 1 and parse(['--pcs', '8'])[0].pcs == 8
    assert parse(['--pcs', '--chains', '4'])[0].pcs == 3
    both = parse(['--pcs', '2', '--credible', '--calibration'])[0]
    assert both.pcs == 2 and both.credible == 0.9 and both.calibration == 0.9
    for bad in ('0', '9', '-1'):
        with pytest.raises(SystemExit):
            parse(['--pcs', bad])
    capsys.readouterr()


def test_columns():
    from nhmc import cli, metrics
    assert cli.PCS_COLUMNS == metrics.PCS_KEYS == KEYS
    others = set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS) | set(cli.CALIBRATION_COLUMNS) | set(cli.CREDIBLE_COLUMNS)
    assert not set(cli.PCS_COLUMNS) & others
    assert {'pc_count', 'pc_rank'} <= set(cli.INT_COLUMNS)


CAL = (27.0, 0.81, 1.4, 0.35, 0.75, 11 / 13, 3.0, 2.0)
CRED = (1.0, 11 / 13, 0.125, 0.5, 26.5, 0.875, 7.0, 0.0)


def _summary(n_samples, psnr, replicas=1, cal=None, cred=None, pcs=None):
    from nhmc import metrics
    col = lambda v: np.full(1, v, dtype=np.float64)
    out = dict(psnr_mean=col(psnr), psnr_std=col(0.5), ssim_mean=col(0.8), ssim_std=col(0.01), std_map_min=col(0.0),
               std_map_max=col(0.2), n_samples=n_samples, mean=None, std_map=None, std_map_normalised=None)
    if replicas > 1:
        out.update(replicas=replicas, rhat=None, ess=None,
                   **{k: col(v) for k, v in zip(metrics.CONVERGENCE_KEYS, (1.3, 1.05, 0.25, 7.5, 30.0, 4.0))})
    if cal is not None:
        out.update(z=None, below=None, equal=None, hist=None, **{k: col(v) for k, v in zip(metrics.CALIBRATION_KEYS, cal)})
    if cred is not None:
        out.update(lower=None, median=None, upper=None, **{k: col(v) for k, v in zip(metrics.CREDIBLE_KEYS, cred)})
    if pcs is not None:
        out.update(directions=None, eigenvalues=None, **{k: col(v) for k, v in zip(metrics.PCS_KEYS, pcs)})
    return out


def test_report_lines_and_rows(tmp_path, capsys):
    """On the host: image 0 has the figures, image 1 collected one sample (NaN figures: no line, null in the JSON), image 2
    has draws that are all equal (the two counts are 0, the figures null, no line).  The columns come after all others;
    without the keyword `_report` does what a call that omits it does."""
    from nhmc import cli
    nan = float('nan')
    pcs = (3.0, 11.0, 0.625, 0.875, 2.5, 0.75, 1.25)
    rows = cli._metric_rows([0], _summary(12, 25.0, replicas=2, cal=CAL, cred=CRED, pcs=pcs))
    rows += cli._metric_rows([1], _summary(1, 24.0, replicas=2, cal=(nan,) * 8, cred=(nan,) * 8, pcs=(nan,) * 7))
    rows += cli._metric_rows([2], _summary(12, 23.0, replicas=2, cal=CAL, cred=CRED, pcs=(0.0, 0.0) + (nan,) * 5))
    columns = cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS + cli.PCS_COLUMNS
    assert all(len(r) == len(columns) for r in rows)
    report = tmp_path / 'metrics.json'
    cli._report(rows, 3, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9, credible=0.9, pcs=3)
    out = capsys.readouterr().out
    line = ('image 0: principal components: 3 of rank 11, variance share first 0.6250 top-3 0.8750, effective rank 2.50, '
            'error inside the span 0.7500, z rms along them 1.250')
    assert out.count(line) == 1 and out.count(': principal components: ') == 1     # image 0 alone
    assert 'image 1: PSNR 24.000' in out and 'image 1: principal' not in out and 'image 2: principal' not in out
    total = [ln for ln in out.splitlines() if ln.startswith('Total Average principal components:')]
    assert total == ['Total Average principal components: variance share first 0.6250 top-3 0.8750, effective rank 2.50, '
                     'error inside the span 0.7500, z rms along them 1.250']
    assert out.index('image 0: credible interval: ') < out.index('image 0: principal components: ')
    assert out.index('Total Average credible interval: ') < out.index('Total Average principal components: ')
    got = json.loads(report.read_text())
    assert all(tuple(r) == columns for r in got)
    assert got[0]['pc_count'] == 3 and got[0]['pc_rank'] == 11 and isinstance(got[0]['pc_count'], int)
    assert isinstance(got[0]['pc_rank'], int) and got[0]['pc_var_first'] == 0.625 and got[0]['pc_z_rms'] == 1.25
    assert all(got[1][k] is None for k in cli.PCS_COLUMNS)
    assert got[2]['pc_count'] == 0 and got[2]['pc_rank'] == 0 and all(got[2][k] is None for k in cli.PCS_COLUMNS[2:])
    # one chain per image, the flag alone
    rows = cli._metric_rows([0], _summary(20, 25.0, pcs=pcs))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), pcs=5)
    text = capsys.readouterr().out
    assert 'image 0: principal components: 3 of rank 11' in text and 'top-5 0.8750' in text
    assert tuple(json.loads(report.read_text())[0]) == cli.COLUMNS + cli.PCS_COLUMNS
    # pcs=None is a call without the keyword, and the column tuple is what it was
    rows = cli._metric_rows([0], _summary(12, 25.0, replicas=2, cal=CAL, cred=CRED))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9, credible=0.9)
    a_out, a_json = capsys.readouterr().out, report.read_text()
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9, credible=0.9, pcs=None)
    assert capsys.readouterr().out == a_out and report.read_text() == a_json and 'principal' not in a_out
    assert tuple(json.loads(a_json)[0]) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS
    assert cli.COLUMNS == ('image', 'psnr_mean', 'psnr_std', 'ssim_mean', 'ssim_std', 'std_map_min', 'std_map_max', 'n_samples')


# ---- no CPU path, header, binding, validation -------------------------------------------------------------------------
def test_no_cpu_path():
    import nhmc
    import nhmc.kernels as K_
    from nhmc import metrics
    x, t = torch.zeros(2, 4, 1, 4, 4), torch.zeros(2, 1, 4, 4)
    with pytest.raises(nhmc._lib.NhmcError, match='no CPU path'):
        K_.sample_gram(x, t, 1)
    with pytest.raises(nhmc._lib.NhmcError, match='no CPU path'):
        K_.sample_project(x, torch.zeros(2, 3, 4, dtype=torch.float64), 1)
    with pytest.raises(nhmc._lib.NhmcError, match='no CPU path'):
        metrics.pcs(x, t)
    with pytest.raises(nhmc._lib.NhmcError, match='no CPU path'):
        metrics.summarize(x, t, pcs=3)


def test_header_and_binding_declare_the_entries():
    import nhmc
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('nhmc_sample_gram_slabs', 'nhmc_sample_gram_ws_bytes', 'nhmc_sample_gram', 'nhmc_sample_project'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in nhmc._lib.SIGNATURES
    # four pointers, n_groups, n_replicas, n_samples, n_elem and the stream; three pointers, four ints, n_elem, the stream
    assert len(nhmc._lib.SIGNATURES['nhmc_sample_gram'][1]) == 9 and len(nhmc._lib.SIGNATURES['nhmc_sample_project'][1]) == 9
    assert 'Principal components of the posterior samples' in src
    assert 'NHMC_ABI_VERSION 2' in re.sub(r'\s+', ' ', src) and nhmc._lib.load().nhmc_abi_version() == 2


def test_argument_validation():
    """Through the C ABI with pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ARG, ALIGN, SHAPE = 1, 2, 3
    ok = (2, 2, 10, 1024, null)                               # groups, replicas, samples, n_elem, stream

    def gram(ptrs=(a16,) * 4, dims=ok):                       # samples, x_orig, gram, ws
        return lib.nhmc_sample_gram(*ptrs, *dims)

    def with_ptr(k, i, p):
        ptrs = [a16] * k
        ptrs[i] = p
        return ptrs
    for i in (0, 2, 3):                                       # every pointer but x_orig
        assert gram(with_ptr(4, i, null)) == ARG
    for dims in ((0, 2, 10, 1024, null), (2, 0, 10, 1024, null), (2, 2, 0, 1024, null), (2, 2, 10, 0, null),
                 (-1, 2, 10, 1024, null)):
        assert gram(dims=dims) == ARG
    for i in range(3):                                        # samples, x_orig, gram
        assert gram(with_ptr(4, i, a4)) == ALIGN
    assert gram(dims=(2, 2, 10, 6, null)) == ALIGN            # n_elem % 4
    assert gram(dims=(2, 1, 1, 1024, null)) == SHAPE          # n = 1
    assert gram(dims=(2, 1, 257, 1024, null)) == SHAPE        # n = 257
    assert gram(dims=(2, 257, 1, 1024, null)) == SHAPE
    assert gram(dims=(65536, 2, 10, 1024, null)) == SHAPE     # groups ride in gridDim.y
    assert gram(with_ptr(4, 1, null), (2, 1, 1, 1024, null)) == SHAPE     # a null x_orig is no error: the shape is
    assert gram(with_ptr(4, 2, a4), (2, 1, 1, 1024, null)) == ALIGN       # ALIGN before SHAPE
    assert gram(with_ptr(4, 2, null), (2, 1, 1, 6, null)) == ARG          # ARG before both

    okp = (2, 2, 10, 3, 1024, null)                           # groups, replicas, samples, n_out, n_elem, stream

    def project(ptrs=(a16,) * 3, dims=okp):                   # samples, coef, out
        return lib.nhmc_sample_project(*ptrs, *dims)
    for i in range(3):
        assert project(with_ptr(3, i, null)) == ARG and project(with_ptr(3, i, a4)) == ALIGN
    for dims in ((0, 2, 10, 3, 1024, null), (2, 0, 10, 3, 1024, null), (2, 2, 0, 3, 1024, null), (2, 2, 10, 3, 0, null)):
        assert project(dims=dims) == ARG
    assert project(dims=(2, 2, 10, 3, 1022, null)) == ALIGN
    assert project(dims=(2, 1, 1, 3, 1024, null)) == SHAPE    # n = 1
    assert project(dims=(2, 1, 257, 3, 1024, null)) == SHAPE  # n = 257
    assert project(dims=(2, 2, 10, 9, 1024, null)) == SHAPE   # n_out = 9
    assert project(dims=(2, 2, 10, 0, 1024, null)) == SHAPE   # n_out = 0
    assert project(dims=(65536, 2, 10, 3, 1024, null)) == SHAPE
    assert project(with_ptr(3, 2, a4), (2, 2, 10, 9, 1024, null)) == ALIGN
    # the slab count depends on the sizes alone
    assert lib.nhmc_sample_gram_slabs(3 * 256 * 256) == 192 and lib.nhmc_sample_gram_slabs(1024) == 1
    assert lib.nhmc_sample_gram_slabs(1028) == 2 and lib.nhmc_sample_gram_slabs(4) == 1 and lib.nhmc_sample_gram_slabs(0) == 0
    # per slab and group: rb = ceil(n / 16) block rows x (rb / 2 + 1) cyclic offsets x 256 doubles
    tiles = {2: 1 * 1, 16: 1 * 1, 17: 2 * 2, 32: 2 * 2, 33: 3 * 2, 64: 4 * 3, 65: 5 * 3, 128: 8 * 5, 129: 9 * 5, 160: 10 * 6,
             256: 16 * 9}
    for n, t in tiles.items():
        assert lib.nhmc_sample_gram_ws_bytes(3, n, 5000) == 3 * 5 * t * 256 * 8, n
    assert lib.nhmc_sample_gram_ws_bytes(0, 20, 64) == 0 and lib.nhmc_sample_gram_ws_bytes(1, 1, 64) == 0
    assert lib.nhmc_sample_gram_ws_bytes(1, 257, 64) == 0 and lib.nhmc_sample_gram_ws_bytes(1, 20, 0) == 0

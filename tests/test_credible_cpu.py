"""CPU: the credible-interval report without a device -- a torch.sort / float64 restatement of the definition in
include/nhmc.h ("Credible interval and median of the posterior samples"; tests/test_credible_gpu.py holds the kernel to
it), the host function that turns the kernel's summary into the reported figures, the entry's argument validation, and the
CLI's host side: the flag, the columns, the lines."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMS = ('sum_width', 'max_width', 'sum_err2_median', 'n_inside', 'n_point', 'n_nan')


def credible_ref(pooled, truth, k):
    """pooled [n, E] float32 (the pooled draws of one image), truth [E] float32 or None, 1 <= k <= n // 2 -> dict: lower,
    median, upper [E] float32 -- d_(k), the median and d_(n+1-k) of torch.sort's order (ascending, NaN above +inf); the
    median of an even n is one float32 add and one float32 multiply -- and the six sums of the header under their names,
    in float64 (np.sum and np.max both propagate NaN, which is the header's rule)."""
    x = torch.as_tensor(np.ascontiguousarray(pooled, dtype=np.float32))
    n = x.shape[0]
    assert 1 <= k <= n // 2
    d = torch.sort(x, dim=0).values.numpy()
    lower, upper = d[k - 1].copy(), d[n - k].copy()
    with np.errstate(invalid='ignore', over='ignore'):
        median = d[(n - 1) // 2].copy() if n % 2 else (d[n // 2 - 1] + d[n // 2]) * np.float32(0.5)
        assert median.dtype == np.float32
        width = upper.astype(np.float64) - lower.astype(np.float64)
        out = dict(lower=lower, median=median, upper=upper, sum_width=float(width.sum()), max_width=float(np.max(width)),
                   sum_err2_median=float('nan'), n_inside=float('nan'), n_point=int((upper == lower).sum()),
                   n_nan=int(np.isnan(upper).sum()))
        if truth is not None:
            t = np.asarray(truth, dtype=np.float32)
            out['sum_err2_median'] = float(((t.astype(np.float64) - median.astype(np.float64)) ** 2).sum())
            out['n_inside'] = int(((lower <= t) & (t <= upper)).sum())
    return out


def sums_of(ref):
    return np.array([[ref[k] for k in SUMS]], dtype=np.float64)


# ---- the restatement on an input whose answer is known ---------------------------------------------------------------
HAND = np.array([[0.5, 1.0, 0.0, 3.0],
                 [-1.0, 1.0, np.nan, 1.0],
                 [0.25, 1.0, -0.5, 2.0],
                 [0.25, 1.0, 2.0, 0.0]], dtype=np.float32)     # element 0 holds a tie, 1 is flat, 2 has a NaN draw
HAND_TRUTH = np.array([0.25, 1.0, 1.0, 5.0], dtype=np.float32)


def test_restatement_on_a_hand_built_case():
    got = credible_ref(HAND, HAND_TRUTH, 1)                   # sorted: (-1 .25 .25 .5) (1 1 1 1) (-.5 0 2 nan) (0 1 2 3)
    assert got['lower'].tolist() == [-1.0, 1.0, -0.5, 0.0] and got['median'].tolist() == [0.25, 1.0, 1.0, 1.5]
    assert got['upper'][[0, 1, 3]].tolist() == [0.5, 1.0, 3.0] and np.isnan(got['upper'][2])
    assert np.isnan(got['sum_width']) and np.isnan(got['max_width'])
    assert (got['n_inside'], got['n_point'], got['n_nan']) == (2, 1, 1) and got['sum_err2_median'] == 12.25
    got = credible_ref(HAND, HAND_TRUTH, 2)
    assert got['lower'].tolist() == [0.25, 1.0, 0.0, 1.0] and got['upper'].tolist() == [0.25, 1.0, 2.0, 2.0]
    assert got['median'].tolist() == [0.25, 1.0, 1.0, 1.5]
    assert (got['sum_width'], got['max_width'], got['n_inside'], got['n_point'], got['n_nan']) == (3.0, 2.0, 3, 2, 0)
    got = credible_ref(HAND[:3], None, 1)                     # odd n: (-1 .25 .5) (1 1 1) (-.5 0 nan) (1 2 3)
    assert got['median'].tolist() == [0.25, 1.0, 0.0, 2.0] and got['lower'].tolist() == [-1.0, 1.0, -0.5, 1.0]
    assert np.isnan(got['upper'][2]) and got['n_nan'] == 1 and np.isnan(got['sum_err2_median']) and np.isnan(got['n_inside'])
    inf = np.array([[np.inf], [-np.inf], [0.0]], dtype=np.float32)
    got = credible_ref(inf, np.zeros(1, dtype=np.float32), 1)
    assert got['lower'][0] == -np.inf and got['upper'][0] == np.inf and got['median'][0] == 0.0 and got['max_width'] == np.inf
    got = credible_ref(inf[:2], None, 1)                      # (-inf + inf) * 0.5: NaN, as np.median has it
    with np.errstate(invalid='ignore'):
        assert np.isnan(got['median'][0]) and np.isnan(np.median(inf[:2, 0]))


def test_figures_from_the_sums():
    from nhmc import metrics
    assert metrics.CREDIBLE_KEYS == ('ci_rank', 'ci_level', 'ci_width_mean', 'ci_width_max', 'psnr_of_median', 'ci_inside',
                                     'n_point', 'n_nan')
    got = metrics.credible_from_sums(sums_of(credible_ref(HAND, HAND_TRUTH, 2)), 4, 2, 4)
    assert tuple(got) == metrics.CREDIBLE_KEYS and all(v.shape == (1,) and v.dtype == np.float64 for v in got.values())
    want = dict(ci_rank=2.0, ci_level=0.2, ci_width_mean=0.375, ci_width_max=1.0, psnr_of_median=10 * np.log10(16 / 12.25),
                ci_inside=0.75, n_point=2.0, n_nan=0.0)
    for name in metrics.CREDIBLE_KEYS:
        assert got[name][0] == want[name], name
    for n, level in ((20, 0.9), (20, 0.5), (160, 0.8), (12, 0.9)):           # the same number as coverage_nominal
        k = metrics.coverage_rank(n, level)
        nominal = metrics.coverage_from_hist(np.ones(n + 1, dtype=np.int64), level)[1]
        assert metrics.credible_from_sums(np.zeros((1, 6)), n, k, 16)['ci_level'][0] == nominal
    # nothing to divide by: NaN or inf, no exception; NaN sums stay NaN
    empty = metrics.credible_from_sums(np.zeros((2, 6)), 4, 1, 0)
    assert np.isnan(empty['ci_width_mean']).all() and np.isnan(empty['ci_inside']).all() and empty['ci_rank'].tolist() == [1, 1]
    assert np.isposinf(metrics.credible_from_sums(np.zeros((1, 6)), 4, 1, 16)['psnr_of_median'][0])
    poisoned = metrics.credible_from_sums(sums_of(credible_ref(HAND, None, 1)), 4, 1, 4)
    assert all(np.isnan(poisoned[k][0]) for k in ('ci_width_mean', 'ci_width_max', 'psnr_of_median', 'ci_inside'))
    assert poisoned['n_nan'][0] == 1.0 and poisoned['n_point'][0] == 1.0


# ---- parser, columns, report lines --------------------------------------------------------------------------------
ARGS = ['--deg', 'sr4', '--sigma_0', '0.05']


@pytest.mark.parametrize('latent', [False, True])
def test_credible_flag(latent):
    from nhmc import cli
    parse = lambda extra: cli.get_parser(latent).parse_known_args(ARGS + extra)
    assert parse([])[0].credible is None and parse([])[0].calibration is None
    assert parse(['--credible'])[0].credible == 0.9 and parse(['--credible'])[1] == []
    assert parse(['--credible', '0.5'])[0].credible == 0.5
    assert parse(['--credible', '--chains', '4'])[0].credible == 0.9
    both = parse(['--credible', '0.8', '--calibration'])[0]
    assert both.credible == 0.8 and both.calibration == 0.9


def test_columns():
    from nhmc import cli, metrics
    assert cli.CREDIBLE_COLUMNS == metrics.CREDIBLE_KEYS
    assert not set(cli.CREDIBLE_COLUMNS) & (set(cli.COLUMNS) | set(cli.REPLICA_COLUMNS) | set(cli.CALIBRATION_COLUMNS))
    assert {'ci_rank', 'n_point', 'n_nan'} <= set(cli.INT_COLUMNS)


CAL = (27.0, 0.81, 1.4, 0.35, 0.75, 11 / 13, 3.0, 2.0)


def _summary(n_samples, psnr, replicas=1, cal=None, cred=None):
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
    return out


def test_report_lines_and_rows(tmp_path, capsys):
    """On the host: image 0 has the figures, image 1 collected one sample (NaN figures: no line, null in the JSON).  The
    credible columns come last, after the replica and the calibration columns; without the keyword `_report` does what a
    call that omits it does."""
    from nhmc import cli
    nan = float('nan')
    cred = (1.0, 11 / 13, 0.125, 0.5, 26.5, 0.875, 7.0, 0.0)
    rows = cli._metric_rows([0], _summary(12, 25.0, replicas=2, cal=CAL, cred=cred))
    rows += cli._metric_rows([1], _summary(1, 24.0, replicas=2, cal=(nan,) * 8, cred=(nan,) * 8))
    columns = cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS + cli.CREDIBLE_COLUMNS
    assert all(len(r) == len(columns) for r in rows)
    report = tmp_path / 'metrics.json'
    cli._report(rows, 2, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9, credible=0.9)
    out = capsys.readouterr().out
    line = ('image 0: credible interval: order statistics 1 and 12 of 12 draws (level 0.8462), width mean 0.1250 max 0.5000, '
            'original inside 0.8750, PSNR of the median 26.500, point elements 7')
    assert out.count(line) == 1 and out.count('credible interval: order statistics') == 1
    assert 'image 1: PSNR 24.000' in out and 'image 1: credible' not in out
    total = [ln for ln in out.splitlines() if ln.startswith('Total Average credible interval:')]
    assert total == ['Total Average credible interval: level 0.8462, width mean 0.1250 max 0.5000, original inside 0.8750, '
                     'PSNR of the median 26.500']
    assert out.index('image 0: calibration: ') < out.index('image 0: credible interval: ')
    got = json.loads(report.read_text())
    assert tuple(got[0]) == columns and tuple(got[1]) == columns
    assert got[0]['ci_rank'] == 1 and got[0]['n_point'] == 7 and got[0]['n_nan'] == 0
    assert all(isinstance(got[0][k], int) for k in ('ci_rank', 'n_point', 'n_nan'))
    assert got[0]['ci_level'] == 11 / 13 and got[0]['ci_inside'] == 0.875 and got[0]['ci_width_max'] == 0.5
    assert all(got[1][k] is None for k in cli.CREDIBLE_COLUMNS)
    # one chain per image, the flag alone
    rows = cli._metric_rows([0], _summary(20, 25.0, cred=(1.0, 19 / 21, 0.125, 0.5, 26.5, 0.875, 7.0, 0.0)))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), credible=0.9)
    assert 'order statistics 1 and 20 of 20 draws (level 0.9048)' in capsys.readouterr().out
    assert tuple(json.loads(report.read_text())[0]) == cli.COLUMNS + cli.CREDIBLE_COLUMNS
    # credible=None is a call without the keyword
    rows = cli._metric_rows([0], _summary(12, 25.0, replicas=2, cal=CAL))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9)
    a_out, a_json = capsys.readouterr().out, report.read_text()
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2, calibration=0.9, credible=None)
    assert capsys.readouterr().out == a_out and report.read_text() == a_json and 'credible' not in a_out
    assert tuple(json.loads(a_json)[0]) == cli.COLUMNS + cli.REPLICA_COLUMNS + cli.CALIBRATION_COLUMNS


# ---- header, binding, validation ------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    import nhmc
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('nhmc_credible_tiles', 'nhmc_credible_ws_bytes', 'nhmc_credible'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in nhmc._lib.SIGNATURES
    # seven pointers, n_groups, n_replicas, n_samples, n_elem, k and the stream
    assert len(nhmc._lib.SIGNATURES['nhmc_credible'][1]) == 13
    assert 'Credible interval and median of the posterior samples' in src
    assert 'NHMC_ABI_VERSION 2' in re.sub(r'\s+', ' ', src) and nhmc._lib.load().nhmc_abi_version() == 2


def test_argument_validation(monkeypatch):
    """Through the C ABI with pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    monkeypatch.delenv('NHMC_CREDIBLE_PATH', raising=False)
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ARG, ALIGN, SHAPE = 1, 2, 3
    all16 = [a16] * 7                                         # samples, x_orig, lower, median, upper, summary, ws
    ok = (2, 2, 10, 1024, 1, null)                            # groups, replicas, samples, n_elem, k, stream

    def call(ptrs=all16, dims=ok):
        return lib.nhmc_credible(*ptrs, *dims)

    def with_ptr(i, p):
        ptrs = list(all16)
        ptrs[i] = p
        return ptrs
    for i in (0, 2, 3, 4, 5, 6):                              # every pointer but x_orig
        assert call(with_ptr(i, null)) == ARG
    for dims in ((0, 2, 10, 1024, 1, null), (2, 0, 10, 1024, 1, null), (2, 2, 0, 1024, 1, null), (2, 2, 10, 0, 1, null),
                 (-1, 2, 10, 1024, 1, null)):
        assert call(dims=dims) == ARG
    for i in range(5):                                        # the five bases that take vector accesses
        assert call(with_ptr(i, a4)) == ALIGN
    assert call(dims=(2, 2, 10, 6, 1, null)) == ALIGN         # n_elem % 4
    assert call(dims=(2, 1, 1, 1024, 1, null)) == SHAPE       # n = 1
    assert call(dims=(2, 25, 41, 1024, 1, null)) == SHAPE     # n = 1025
    assert call(dims=(2, 1, 1025, 1024, 1, null)) == SHAPE
    assert call(dims=(65536, 2, 10, 1024, 1, null)) == SHAPE  # groups ride in gridDim.y
    assert call(dims=(2, 2, 10, 1024, 0, null)) == SHAPE      # k = 0
    assert call(dims=(2, 2, 10, 1024, 11, null)) == SHAPE     # k = n / 2 + 1
    assert call(dims=(2, 3, 7, 1024, 11, null)) == SHAPE      # odd n = 21: n / 2 = 10
    assert call(with_ptr(1, null), (2, 1, 1, 1024, 1, null)) == SHAPE     # a null x_orig is no error: the shape is
    assert call(with_ptr(1, null), (2, 2, 10, 1024, 11, null)) == SHAPE
    assert call(with_ptr(3, a4), (2, 1, 1, 1024, 1, null)) == ALIGN       # ALIGN before SHAPE
    assert call(with_ptr(2, null), (2, 1, 1, 6, 1, null)) == ARG          # ARG before both
    monkeypatch.setenv('NHMC_CREDIBLE_PATH', 'sideways')      # neither register nor general
    assert call(dims=(2, 1, 1, 1024, 1, null)) == SHAPE and call(with_ptr(2, null)) == ARG
    monkeypatch.delenv('NHMC_CREDIBLE_PATH')
    assert lib.nhmc_credible_tiles(3 * 256 * 256) == 768 and lib.nhmc_credible_tiles(64) == 1
    assert lib.nhmc_credible_tiles(257) == 2 and lib.nhmc_credible_tiles(0) == 0
    assert lib.nhmc_credible_ws_bytes(8, 3 * 256 * 256) == 8 * 768 * 8 * 8 and lib.nhmc_credible_ws_bytes(0, 64) == 0
    assert lib.nhmc_credible_ws_bytes(1, 16) == 64 and lib.nhmc_credible_ws_bytes(3, 0) == 0

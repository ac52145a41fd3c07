"""CPU: the multi-chain report without a device -- a float64 numpy restatement of the split R-hat / ESS definition of
include/nhmc.h ("Convergence of replica chains"; tests/test_diag_gpu.py holds the kernel to it), sanity checks of that
restatement on inputs whose answer is known, and the CLI's host side: the flags, the batching and `replica_inputs`."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def diag_float64(x, threshold=1.1):
    """x [K, S, E] (replica, draw, element) -> dict, every step as the header words it, float64 throughout:
    rhat, ess [E]; the six summaries; W, Bn, V [E]; `p_margin` [E], the smallest |P_k| over the k the ESS evaluated (inf
    where it evaluated none), and `thr_margin` [E] = |rhat - threshold| (inf where rhat is not finite) -- how far each
    element is from the two discrete decisions."""
    x = np.asarray(x, dtype=np.float64)
    K, S, E = x.shape
    n, M = S // 2, 2 * K
    split = np.empty((M, n, E))
    split[0::2], split[1::2] = x[:, :n], x[:, S - n:]
    mu = split.sum(axis=1) / n                                               # [M, E]
    d = split - mu[:, None]
    a = np.zeros((M, max(n - 1, 1), E))                                      # a[m, t], t = 0 .. n - 2
    for t in range(0, max(n - 1, 1)):
        a[:, t] = (d[:, :n - t] * d[:, t:]).sum(axis=1) / n
    W = (a[:, 0] * n / (n - 1)).sum(axis=0) / M
    Bn = (mu - mu[0]).var(axis=0, ddof=1)                                    # about the first mean, as the header says
    V = W * (n - 1) / n + Bn
    rhat, ess = np.full(E, np.nan), np.full(E, np.nan)
    p_margin = np.full(E, np.inf)
    mean_a = a.sum(axis=0) / M                                               # [n - 1, E]
    for e in range(E):
        if V[e] == 0.0:
            continue
        if W[e] == 0.0:
            rhat[e] = np.inf
            continue
        rhat[e] = np.sqrt(V[e] / W[e])
        rho = lambda t: 1.0 if t == 0 else 1.0 - (W[e] - mean_a[t, e]) / V[e]
        kept, k = [], 0
        while 2 * k + 1 <= n - 2:
            p = rho(2 * k) + rho(2 * k + 1)
            p_margin[e] = min(p_margin[e], abs(p))
            if p <= 0.0:
                break
            kept.append(min(p, kept[-1]) if kept else p)
            k += 1
        tau = max(-1.0 + 2.0 * sum(kept), 1.0 / np.log10(M * n))
        ess[e] = M * n / tau
    constant = np.isnan(rhat)
    finite = np.isfinite(rhat)
    thr_margin = np.where(finite, np.abs(np.where(finite, rhat, 0.0) - threshold), np.inf)
    some = lambda m, f: f() if m.any() else np.nan
    return dict(rhat=rhat, ess=ess, W=W, Bn=Bn, V=V, p_margin=p_margin, thr_margin=thr_margin,
                rhat_max=some(~constant, lambda: rhat[~constant].max()),
                rhat_mean=some(finite, lambda: rhat[finite].mean()),
                rhat_frac_above=some(~constant, lambda: float((rhat[~constant] > threshold).sum()) / (~constant).sum()),
                ess_min=some(~np.isnan(ess), lambda: np.nanmin(ess)),
                ess_mean=some(~np.isnan(ess), lambda: np.nanmean(ess)),
                n_constant=int(constant.sum()))


# ---- the restatement on inputs whose answer is known ----------------------------------------------------------------
def test_identical_replicas_leave_only_the_split_half_part():
    """K copies of one chain: the M = 2K split means are K copies of the two half means (h0, h1), so the ddof = 1
    variance of the means is K (h0 - h1)^2 / (2 (2K - 1)) and W is the one chain's own."""
    rng = np.random.default_rng(0)
    one = rng.standard_normal((1, 20, 5))
    for K in (1, 2, 5):
        got = diag_float64(np.repeat(one, K, axis=0))
        h0, h1 = one[0, :10].mean(axis=0), one[0, 10:].mean(axis=0)
        assert np.allclose(got['Bn'], K * (h0 - h1) ** 2 / (2.0 * (2 * K - 1)), rtol=1e-12, atol=0)
        assert np.allclose(got['W'], diag_float64(one)['W'], rtol=1e-12, atol=0)


def test_variance_of_the_means_about_the_first_mean_is_the_plain_one():
    """The restatement (like the kernel) takes the ddof = 1 variance of the M means about the first mean; on elements
    that vary that is the plain variance of the means up to rounding (1e-12 relative: the means are O(1), their spread
    O(0.3), so either form loses at most a few digits of float64)."""
    x = np.random.default_rng(4).standard_normal((5, 20, 300)) + 0.5
    n = 10
    split = np.concatenate([x[:, :n], x[:, n:]])                              # the 2K half chains (order is immaterial)
    plain = (split.sum(axis=1) / n).var(axis=0, ddof=1)
    assert np.allclose(diag_float64(x)['Bn'], plain, rtol=1e-12, atol=0)


def test_iid_draws_look_converged():
    x = np.random.default_rng(1).standard_normal((8, 20, 4000))
    got = diag_float64(x)
    assert 0.97 <= got['rhat_mean'] <= 1.05
    assert got['ess_mean'] > 100.0 and got['n_constant'] == 0
    assert got['ess_min'] > 0 and np.isfinite(got['rhat_max'])


def test_offset_replicas_are_flagged():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, 20, 500)) + 3.0 * np.arange(4)[:, None, None]
    got = diag_float64(x)
    assert float(got['rhat'].min()) > 1.5 and got['rhat_frac_above'] == 1.0


def test_constant_and_stuck_elements():
    x = np.random.default_rng(3).standard_normal((3, 8, 6))
    x[:, :, 1] = 0.1                                        # all equal: constant
    x[:, :, 4] = np.array([-1.0, 0.0, 1.0])[:, None]        # a different constant per replica: stuck
    got = diag_float64(x)
    assert np.isnan(got['rhat'][1]) and np.isnan(got['ess'][1]) and got['n_constant'] == 1
    assert np.isposinf(got['rhat'][4]) and np.isnan(got['ess'][4])
    assert np.isposinf(got['rhat_max']) and np.isfinite(got['rhat_mean'])
    assert got['rhat_frac_above'] >= 1.0 / 5.0               # the stuck element counts, the constant one is not in the share
    assert np.isfinite(np.delete(got['rhat'], [1, 4])).all() and np.isfinite(np.delete(got['ess'], [1, 4])).all()


def test_fewer_than_six_draws_give_the_cap():
    for S in (4, 5):
        got = diag_float64(np.random.default_rng(S).standard_normal((3, S, 7)))
        assert np.allclose(got['ess'], 12 * np.log10(12.0), rtol=1e-15)


# ---- parser and batching -------------------------------------------------------------------------------------------
ARGS = ['--deg', 'sr4', '--sigma_0', '0.05']


@pytest.mark.parametrize('latent', [False, True])
def test_replica_flags(latent):
    from nhmc import cli
    opt, _ = cli.get_parser(latent).parse_known_args(ARGS)
    assert opt.replicas == 1 and opt.rhat_threshold == 1.1
    cli.check_replicas(opt)
    opt, _ = cli.get_parser(latent).parse_known_args(ARGS + ['--chains', '8', '--replicas', '4', '--rhat_threshold', '1.05'])
    assert opt.replicas == 4 and opt.rhat_threshold == 1.05
    cli.check_replicas(opt)


@pytest.mark.parametrize('entry', ['main', 'main_latent'])
def test_chains_must_be_a_multiple_of_replicas(entry, monkeypatch):
    """The error comes before anything touches the GPU: there is none here, and set-up must not be reached."""
    from nhmc import cli
    monkeypatch.setattr(cli, '_setup', lambda *a, **k: pytest.fail('set-up was reached'))
    algo = 'hmc' if entry == 'main' else 'hmc_latent'
    with pytest.raises(SystemExit, match='multiple of --replicas 4'):
        getattr(cli, entry)(ARGS + ['--algo', algo, '--chains', '6', '--replicas', '4'])


def test_batches_hold_chains_over_replicas_images():
    from nhmc import cli
    chains, K = 8, 4
    batches = cli.image_batches(5, 0, 1, chains // K)
    assert batches == [[0, 1], [2, 3], [4]]
    assert [cli.chain_id_base(b, K) for b in batches] == [0, 8, 16]
    assert [cli.chain_id_base(b) for b in cli.image_batches(5, 0, 1, 2)] == [0, 2, 4]          # K = 1: the image index


# ---- replica_inputs ------------------------------------------------------------------------------------------------
def test_replica_inputs():
    from nhmc import cli
    seed, shape, K = 5678, (3, 4, 4), 3
    y_clean = torch.randn(6, 11, generator=torch.Generator().manual_seed(1))
    for s in (0, 4):
        y_one, x_one = cli.draw_inputs(seed, s, y_clean[s], 0.1, shape)
        y, x = cli.replica_inputs(seed, s, K, y_clean[s], 0.1, shape)
        assert y.shape == (K, 11) and x.shape == (K,) + shape
        assert torch.equal(x[0], x_one)                                       # replica 0: the single chain's bits
        assert all(torch.equal(y[r], y_one) for r in range(K))                # one measurement for all replicas
        assert not torch.equal(x[1], x[0]) and not torch.equal(x[2], x[0]) and not torch.equal(x[2], x[1])
        assert abs(float(x[1:].mean())) < 0.3 and 0.7 < float(x[1:].std()) < 1.3
        # K = 1 is draw_inputs with a replica axis
        y1, x1 = cli.replica_inputs(seed, s, 1, y_clean[s], 0.1, shape)
        assert torch.equal(y1[0], y_one) and torch.equal(x1[0], x_one) and x1.shape[0] == 1
        # a replica does not depend on how many there are, nor on the batch (nothing but seed, s, r enters)
        assert torch.equal(cli.replica_inputs(seed, s, 2, y_clean[s], 0.1, shape)[1][1], x[1])
    # images differ, and so do seeds
    assert not torch.equal(cli.replica_inputs(seed, 0, K, y_clean[0], 0.1, shape)[1][1],
                           cli.replica_inputs(seed, 1, K, y_clean[0], 0.1, shape)[1][1])
    assert not torch.equal(cli.replica_inputs(seed, 0, K, y_clean[0], 0.1, shape)[1][1],
                           cli.replica_inputs(seed + 1, 0, K, y_clean[0], 0.1, shape)[1][1])


def test_replica_inputs_do_not_depend_on_the_batch():
    """What cli.main draws per batch, for two batchings of the same images."""
    from nhmc import cli
    y_clean = torch.randn(5, 7, generator=torch.Generator().manual_seed(2))
    K = 2

    def run(images_per_batch):
        rows = {}
        for batch in cli.image_batches(5, 0, 1, images_per_batch):
            drawn = [cli.replica_inputs(1, s, K, y_clean[s], 0.1, (1, 4, 4)) for s in batch]
            y, x = torch.cat([d[0] for d in drawn]), torch.cat([d[1] for d in drawn])
            for i, s in enumerate(batch):
                for r in range(K):
                    rows[cli.chain_id_base(batch, K) + i * K + r] = (s, r, y[i * K + r].clone(), x[i * K + r].clone())
        return rows
    a, b = run(1), run(3)
    assert sorted(a) == sorted(b) == list(range(10))                          # global chain ids s * K + r
    for cid in a:
        assert a[cid][:2] == b[cid][:2] == (cid // K, cid % K)
        assert torch.equal(a[cid][2], b[cid][2]) and torch.equal(a[cid][3], b[cid][3])


def test_common_samples_keeps_the_last_of_each_replica():
    from nhmc import cli
    reps = [torch.arange(n * 2, dtype=torch.float32).reshape(n, 2) + 100 * r for r, n in enumerate((5, 3, 4))]
    lat, s_c = cli.common_samples(reps)
    assert s_c == 3 and lat.shape == (9, 2)
    assert torch.equal(lat[:3], reps[0][2:]) and torch.equal(lat[3:6], reps[1]) and torch.equal(lat[6:], reps[2][1:])
    one, s_1 = cli.common_samples(reps[:1])                                   # K = 1: the chain's own samples
    assert s_1 == 5 and torch.equal(one, reps[0])
    none, s_0 = cli.common_samples([reps[0], reps[1][:0]])                    # a replica that collected nothing
    assert s_0 == 0 and none.shape == (0, 2)


# ---- the report's rows, printed lines and JSON on the host ----------------------------------------------------------
def _summary(G, n_samples, replicas, psnr, conv):
    """What metrics.summarize returns for G images, with the scalars the rows take."""
    col = lambda v: np.full(G, v, dtype=np.float64)
    out = dict(psnr_mean=col(psnr), psnr_std=col(0.5 if psnr == psnr else 0.0), ssim_mean=col(0.8 if psnr == psnr else np.nan),
               ssim_std=col(0.01 if psnr == psnr else 0.0), std_map_min=col(0.0 if n_samples > 1 else np.nan),
               std_map_max=col(0.2 if n_samples > 1 else np.nan), n_samples=n_samples, mean=None, std_map=None,
               std_map_normalised=None)
    if replicas > 1:
        from nhmc import metrics
        out.update(replicas=replicas, rhat=None, ess=None, **{k: col(v) for k, v in zip(metrics.CONVERGENCE_KEYS, conv)})
    return out


def test_report_with_replicas_survives_rows_without_convergence_values(tmp_path, capsys):
    """--replicas 2, world 1, on the host: image 0 has everything, image 1 fewer than 4 samples per replica (pooled PSNR
    and SSIM, NaN convergence values), image 2 no sample at all.  The report prints what it has and writes None for what
    it has not; it must not fail after the sampling is done."""
    import json
    from nhmc import cli
    nan = float('nan')
    rows = cli._metric_rows([0], _summary(1, 12, 2, 24.0, (1.3, 1.05, 0.25, 7.5, 30.0, 4.0)))
    rows += cli._metric_rows([1], _summary(1, 6, 2, 23.0, (nan,) * 6))
    rows += cli._metric_rows([2], _summary(1, 0, 2, nan, (nan,) * 6))
    assert all(len(r) == len(cli.COLUMNS) + len(cli.REPLICA_COLUMNS) for r in rows)
    report = tmp_path / 'r' / 'metrics.json'
    table = cli._report(rows, 3, 0, 1, torch.device('cpu'), str(report), replicas=2, rhat_threshold=1.1)
    out = capsys.readouterr().out
    assert table.shape == (3, 3)
    assert 'image 0: R-hat max 1.300 mean 1.0500 (> 1.1: 25.00%)  ESS min 7.5 mean 30.0 of 12 draws, constant elements 4' in out
    assert 'image 1: PSNR 23.000' in out and 'image 1: SSIM ' in out
    assert 'image 1: no R-hat / ESS: fewer than 4 samples per replica (6 draws in all)' in out and 'image 1: R-hat' not in out
    assert 'image 2: no sample was collected' in out and 'image 2: R-hat' not in out and 'image 2: no R-hat' not in out
    assert 'Total Average PSNR: 23.500  images: 3' in out
    got = json.loads(report.read_text())
    assert [r['image'] for r in got] == [0, 1, 2] and all(r['replicas'] == 2 for r in got)
    assert got[0]['n_constant'] == 4 and got[0]['rhat_mean'] == 1.05 and got[0]['n_samples'] == 12
    for r in got[1:]:
        assert all(r[k] is None for k in cli.metrics.CONVERGENCE_KEYS)
    assert got[1]['psnr_mean'] == 23.0 and got[1]['n_samples'] == 6
    assert got[2]['psnr_mean'] is None and got[2]['n_samples'] == 0
    # every element constant (S >= 4): the counts are there, the means are not
    rows = cli._metric_rows([0], _summary(1, 8, 2, 20.0, (nan, nan, nan, nan, nan, 48.0)))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report), replicas=2)
    assert 'image 0: R-hat max nan mean nan' in capsys.readouterr().out
    assert json.loads(report.read_text())[0]['n_constant'] == 48
    # one replica per image: the columns and lines of before
    rows = cli._metric_rows([0], _summary(1, 20, 1, 25.0, ()))
    cli._report(rows, 1, 0, 1, torch.device('cpu'), str(report))
    assert 'R-hat' not in capsys.readouterr().out and tuple(json.loads(report.read_text())[0]) == cli.COLUMNS


# ---- header and binding --------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entries():
    import nhmc
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('nhmc_chain_diag_tiles', 'nhmc_chain_diag_ws_bytes', 'nhmc_chain_diag'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in nhmc._lib.SIGNATURES
    assert len(nhmc._lib.SIGNATURES['nhmc_chain_diag'][1]) == 11
    assert 'Geyer' in src and 'NHMC_ABI_VERSION 2' in re.sub(r'\s+', ' ', src)

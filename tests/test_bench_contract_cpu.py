"""CPU: the command-line contract of bench.py the driver depends on (flags, defaults, the keys of the one JSON line),
checked without a GPU; the numbers themselves are produced on the MI355X box."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_flags_and_defaults(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    a = bench.parse()
    assert (a.gpus, a.batch or bench.B_PER_GPU, a.deg, a.latent) == (1, 64, 'inpaint_random', False) and 1 <= a.steps <= 10 and a.warmup >= 1
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '5', '--warmup', '2'])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (8, 5, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--latent'])
    a = bench.parse()
    assert a.latent and (a.batch or bench.B_LATENT) == 16                        # configs[4]: 128 chains over 8 GPUs


def test_json_line_carries_the_contract_keys():
    src = open(os.path.join(ROOT, 'bench.py')).read()
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert re.search(r"'%s'\s*:" % key, src), key
    for key in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):          # roofline object
        assert re.search(r"\b%s=" % key, src), key
    for key in ('value', 'unit', 'cores', 'kind', 'sample'):                       # cpu_baseline object
        assert re.search(r"\b%s=" % key, src), key
    assert "'scaling': 'weak'" in src and "'vs_baseline': None" in src and "'dtype': 'f32'" in src


def test_traffic_file_is_what_bench_reads():
    t = json.load(open(os.path.join(ROOT, 'profiles', 'traffic_leapfrog.json')))
    alg = 5 * 64 * 3 * 256 * 256 * 4                                               # 5T x 64 chains
    assert abs(t['hbm_bytes_per_launch'] - alg) / alg < 0.01                       # PMC traffic = algorithmic bytes
    assert t['kernel'].startswith('k_leapfrog<1, false')


def test_only_the_cpu_baseline_leg_touches_the_oracle():
    src = open(os.path.join(ROOT, 'bench.py')).read()
    uses = [m.start() for m in re.finditer(r'\boracle\b', src)]
    lo, hi = src.index('def cpu_baseline'), src.index('def single_chain_rate')
    code_uses = [u for u in uses if 'import' in src[src.rfind('\n', 0, u):src.find('\n', u)]]
    assert code_uses and all(lo < u < hi for u in code_uses)


def test_full_and_dump_outputs_flags(monkeypatch, tmp_path):
    import pytest
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '4', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 4, 2)        # a plain run: headline steps only
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', str(tmp_path)])
    a = bench.parse()
    assert a.full and a.dump_outputs == str(tmp_path)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--kernel-only'])                 # its legs are --full legs
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_writes_whole_small_arrays_and_a_fixed_sample_of_large_ones(tmp_path):
    import numpy as np
    import torch
    import bench
    small = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    big = torch.randn(3 * 2 ** 20, generator=torch.Generator().manual_seed(1))
    f64 = torch.linspace(0, 1, 10, dtype=torch.float64)
    half = torch.ones(5, dtype=torch.float16)
    budget = 4 * 2 ** 20
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), dict(small=small, big=big, f64=f64, half=half), budget=budget)
    got = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in ('small', 'big', 'f64', 'half')}
    assert got['small'].dtype == np.float32 and got['small'].shape == (2, 3, 4) and (got['small'] == small.numpy()).all()
    assert got['f64'].dtype == np.float64 and (got['f64'] == f64.numpy()).all()
    assert got['half'].dtype == np.float32 and (got['half'] == 1).all()
    share = budget // 4
    assert got['big'].dtype == np.float32 and got['big'].nbytes == share               # sampled down to its share
    assert np.isin(got['big'], big.numpy()).all()
    assert (np.load(tmp_path / 'b' / 'big.npy') == got['big']).all()                    # the same indices every run
    total = sum(os.path.getsize(tmp_path / 'a' / f'{n}.npy') for n in got)
    assert total <= budget + 4 * 256                                                    # + the .npy headers
    assert bench.DUMP_BYTES + 3 * 256 <= 64 * 10 ** 6                                   # the contract: at most 64 MB

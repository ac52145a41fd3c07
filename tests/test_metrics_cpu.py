"""CPU: the report-stage entries (nhmc.h "Report stage", nhmc.metrics) validate their arguments before any device work,
size their workspaces consistently, have no CPU path, colour the std map with matplotlib's `hot` ramp, and the SSIM
fixture agrees with the definition the kernels implement."""
import ctypes

import numpy as np
import pytest
import torch

P = ctypes.c_void_p
NULL, A16, A4 = P(0), P(0x1000), P(0x1004)
ARG, ALIGN, SHAPE = 1, 2, 3


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


def ssim_float64(x, y):
    """The definition of nhmc.h "Report stage" restated in torch float64: x (sample), y (original) [C, H, W] float32 in
    the sampler's [-1, 1] scale.  Window means over the windows that lie wholly inside the image (avg_pool2d, 7 x 7,
    stride 1, no padding) -- the plane cropped by 3 pixels on every side."""
    unit = lambda v: ((v.float() + 1.0) / 2.0).clamp(0.0, 1.0)
    x32, y32 = unit(x), unit(y)
    R = float(x32.max() - x32.min())                        # the fp32 difference the reference passes as data_range
    x, y = x32.double()[:, None], y32.double()[:, None]
    win = lambda v: torch.nn.functional.avg_pool2d(v, 7, stride=1)
    ux, uy, uxx, uyy, uxy = win(x), win(y), win(x * x), win(y * y), win(x * y)
    cov_norm = 49.0 / 48.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.mean(dim=(1, 2, 3)).mean())


def test_new_entries_refuse_bad_arguments_before_any_launch(lib):
    n = 3 * 8 * 8
    # null pointers -> ARG
    assert lib.nhmc_psnr_samples(NULL, A16, A16, A16, 1, 2, n, NULL) == ARG
    assert lib.nhmc_psnr_samples(A16, A16, A16, NULL, 1, 2, n, NULL) == ARG
    assert lib.nhmc_sample_range(NULL, A16, A16, 2, n, NULL) == ARG
    assert lib.nhmc_sample_range(A16, A16, A16, 0, n, NULL) == ARG
    assert lib.nhmc_ssim(A16, NULL, A16, A16, A16, 1, 2, 3, 8, 8, NULL) == ARG
    assert lib.nhmc_ssim(A16, A16, NULL, A16, A16, 1, 2, 3, 8, 8, NULL) == ARG
    assert lib.nhmc_sample_moments(A16, NULL, A16, A16, A16, 1, 2, 3, 8, 8, NULL) == ARG
    assert lib.nhmc_sample_moments(A16, A16, A16, A16, NULL, 1, 2, 3, 8, 8, NULL) == ARG
    assert lib.nhmc_std_map_normalise(A16, NULL, A16, 1, 64, NULL) == ARG
    # a misaligned base -> ALIGN
    assert lib.nhmc_psnr_samples(A4, A16, A16, A16, 1, 2, n, NULL) == ALIGN
    assert lib.nhmc_psnr_samples(A16, A4, A16, A16, 1, 2, n, NULL) == ALIGN
    assert lib.nhmc_sample_range(A4, A16, A16, 2, n, NULL) == ALIGN
    assert lib.nhmc_ssim(A4, A16, A16, A16, A16, 1, 2, 3, 8, 8, NULL) == ALIGN
    assert lib.nhmc_sample_moments(A4, A16, A16, A16, A16, 1, 2, 3, 8, 8, NULL) == ALIGN
    assert lib.nhmc_std_map_normalise(A4, A16, A16, 1, 64, NULL) == ALIGN
    # N % 4 != 0 -> ALIGN (3 x 7 x 7 = 147), and before the shape is looked at (S = 1, H = 6)
    assert lib.nhmc_psnr_samples(A16, A16, A16, A16, 1, 2, 147, NULL) == ALIGN
    assert lib.nhmc_sample_range(A16, A16, A16, 2, 147, NULL) == ALIGN
    assert lib.nhmc_ssim(A16, A16, A16, A16, A16, 1, 2, 3, 7, 7, NULL) == ALIGN
    assert lib.nhmc_ssim(A16, A16, A16, A16, A16, 1, 2, 3, 6, 7, NULL) == ALIGN
    assert lib.nhmc_sample_moments(A16, A16, A16, A16, A16, 1, 1, 3, 7, 7, NULL) == ALIGN
    # shapes -> SHAPE: H = 6 (or W = 6) has no 7 x 7 window; one sample has no standard deviation
    assert lib.nhmc_ssim(A16, A16, A16, A16, A16, 1, 2, 2, 6, 8, NULL) == SHAPE
    assert lib.nhmc_ssim(A16, A16, A16, A16, A16, 1, 2, 2, 8, 6, NULL) == SHAPE
    assert lib.nhmc_sample_moments(A16, A16, A16, A16, A16, 1, 1, 3, 8, 8, NULL) == SHAPE
    assert lib.nhmc_ssim(A16, A16, A16, A16, A16, 70000, 1, 3, 8, 8, NULL) == SHAPE
    assert lib.nhmc_psnr_samples(A16, A16, A16, A16, 3277, 20, n, NULL) == SHAPE        # 65540 rows


@pytest.mark.parametrize('shape', [(3, 256, 256), (1, 7, 8)])
def test_ssim_tiles_and_workspace_agree(lib, shape):
    c, h, w = shape
    tiles = lib.nhmc_ssim_tiles(h, w)
    assert tiles == -(-(h - 6) // 16) * -(-(w - 6) // 32)              # 16 x 32 window positions per tile
    assert {(3, 256, 256): 128, (1, 7, 8): 1}[shape] == tiles
    range_doubles = 2 * lib.nhmc_data_tiles(c * h * w)                   # nhmc_sample_range shares the workspace
    for n in (1, 40):
        assert lib.nhmc_ssim_ws_bytes(n, c, h, w) == 8 * n * max(c * tiles, range_doubles)
    assert lib.nhmc_ssim_tiles(6, 256) == 0 and lib.nhmc_ssim_tiles(256, 6) == 0
    assert lib.nhmc_moments_tiles(h * w) == -(-(h * w) // 256)


def test_metrics_have_no_cpu_path():
    from nhmc import metrics
    from nhmc._lib import NhmcError
    samples, x_orig = torch.zeros(2, 3, 3, 8, 8), torch.zeros(2, 3, 8, 8)
    for call in (lambda: metrics.psnr(samples, x_orig), lambda: metrics.ssim(samples, x_orig),
                 lambda: metrics.sample_moments(samples), lambda: metrics.summarize(samples, x_orig),
                 lambda: metrics.ssim(samples[0], x_orig[:1])):
        with pytest.raises(NhmcError, match='no CPU path'):
            call()


def test_hot_ramp():
    from nhmc import metrics
    rgb = metrics.hot_colours(np.array([[0.0, 1.0, 0.365079, 0.746032]]))
    assert rgb.dtype == np.uint8 and rgb.shape == (1, 4, 3)
    assert rgb[0, 0].tolist() == [0, 0, 0] and rgb[0, 1].tolist() == [255, 255, 255]
    assert rgb[0, 2].tolist() == [255, 0, 0] and rgb[0, 3].tolist() == [255, 255, 0]


def test_save_std_map_writes_a_png_of_the_maps_size(tmp_path):
    from PIL import Image
    from nhmc import metrics
    path = tmp_path / 'sub' / 'std_dev_map_0.png'
    metrics.save_std_map(torch.linspace(0, 1, 5 * 9).reshape(5, 9), str(path))
    img = Image.open(path)
    assert img.size == (9, 5) and img.mode == 'RGB'
    assert img.getpixel((0, 0)) == (0, 0, 0) and img.getpixel((8, 4)) == (255, 255, 255)


@pytest.mark.parametrize('key, shape', [('a', (3, 24, 28)), ('b', (3, 64, 64))])
def test_fixture_matches_the_float64_definition(golden, key, shape):
    g = golden('g19_ssim.npz')
    x, y = torch.from_numpy(g[f'x_{key}']), torch.from_numpy(g[f'y_{key}'])
    assert x.shape == shape and x.dtype == torch.float32 and float(x.abs().max()) > 1.0      # the clamp is exercised
    assert y.shape == shape and y.dtype == torch.float32
    assert x.is_contiguous() and y.is_contiguous()              # row-major, as the kernels' wrappers demand
    assert abs(ssim_float64(x, y) - float(g[f'ssim64_{key}'])) <= 1e-12
    # the float32 figure (skimage's code path for float32 input) lies within the GPU test's 1e-6 of it
    assert abs(float(g[f'ssim32_{key}']) - float(g[f'ssim64_{key}'])) <= 1e-6


def test_report_lines_and_json(tmp_path, capsys):
    """cli._report on one rank: the PSNR lines and the [n, 3] table keep their form; the SSIM lines, the reference's
    `Total Average SSIM` line (main_sampling.py:560) and the JSON rows are added; a chain without samples is a NaN row."""
    import json
    from nhmc import cli
    nan = float('nan')
    rows = [[0.0, 20.5, 0.25, 0.8, 0.01, 0.0, 0.2, 20.0], [1.0, nan, 0.0, nan, 0.0, nan, nan, 0.0],
            [2.0, 22.5, 0.0, 0.6, 0.0, nan, nan, 1.0]]
    path = tmp_path / 'sub' / 'metrics.json'
    table = cli._report(rows, 3, 0, 1, torch.device('cpu'), str(path))
    out = capsys.readouterr().out.splitlines()
    assert out == ['image 0: PSNR 20.500 (std over samples 0.2500)', 'image 0: SSIM 0.80000 (std over samples 0.01000)',
                   'image 1: no sample was collected (every proposal of the final phase was rejected)',
                   'image 2: PSNR 22.500 (std over samples 0.0000)', 'image 2: SSIM 0.60000 (std over samples 0.00000)',
                   'Total Average PSNR: 21.500  images: 3', 'Total Average SSIM: 0.70000 ({:.5f})'.format(0.01 / 3)]
    assert table.shape == (3, 3) and table.dtype == torch.float32 and bool(torch.isnan(table[1, 1]))
    got = json.loads(path.read_text())
    assert [r['image'] for r in got] == [0, 1, 2] and [r['n_samples'] for r in got] == [20, 0, 1]
    assert got[0] == dict(image=0, psnr_mean=20.5, psnr_std=0.25, ssim_mean=0.8, ssim_std=0.01, std_map_min=0.0,
                          std_map_max=0.2, n_samples=20)
    assert got[1]['psnr_mean'] is None and got[1]['ssim_mean'] is None and got[2]['std_map_max'] is None

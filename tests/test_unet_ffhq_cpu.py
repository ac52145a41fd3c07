"""CPU: fixture G22 (tests/golden/g22_unet_ffhq_256*.npz, oracle/gen_golden_unet_256.py) is the one the GPU tests think
it is.  The weights and inputs are redrawn from the seed and hashed, so a drift of torch's generator says so instead of
showing up as a numeric mismatch; then nhmc.unet's plain-torch fp32 path at FFHQ_CONFIG and B = 2 must stand exactly as
far from the stored float64 probes as the reference class did when the fixture was made (the generator asserted the
two equal bit for bit), which it can only do if the probes are indexed as stored and are not degenerate.

"As far" is equality up to the rounding of the metric itself.  The metric is the largest of 4096 fp32 rounding errors,
and torch's CPU convolutions and matrix products sum in an order that follows the thread count and the host.  With 2 or
8 threads on the generator's host the fp32 bits, and so the 52 errors, are reproduced exactly; with 3, 5 or 7 threads the
bits differ and single groups move between 0.60 x and 1.50 x of the stored error, each the maximum of another draw of
the same rounding noise.  The test therefore allows a factor 3 either way (ROUNDING: twice the observed spread, for
hosts that were not tried), where a probe read at a wrong index or from a wrong tensor is off by the tensor's own
scale, 1e6 x the error."""
import pytest
import torch

from oracle import unet_probe as up

ROUNDING = 3.0


@pytest.fixture(scope='module')
def drawn(golden):
    from nhmc import unet
    net = unet.create_model(**unet.FFHQ_CONFIG).eval().requires_grad_(False)
    return net, up.seeded_inputs(net), golden('g22_unet_ffhq_256.npz'), golden('g22_unet_ffhq_256_grad.npz')


def test_seed_redraws_the_weights_and_inputs_of_the_fixture(drawn):
    _, inp, g, g_grad = drawn
    assert int(g['weight_seed']) == up.SEED and float(g['weight_scale']) == up.SCALE and g['t'].tolist() == list(up.T_STEPS)
    assert inp['weight_sha'] == g['weight_sha256'].tolist(), "torch's generator no longer draws the fixture's weights"
    assert up.sha(inp['x']) == str(g['x_sha256']), "torch's generator no longer draws the fixture's x"
    assert torch.equal(inp['pos'], torch.from_numpy(g['pos']).long())
    truth = up.truth_of(g, g_grad)
    assert sorted(truth) == sorted(up.FWD + up.GRAD + up.ENGINE)
    assert all(v[0].shape == (up.N_PROBE,) and v[0].dtype == torch.float64 and v[1] > 0 for v in truth.values())


def test_fp32_cpu_path_stands_where_the_reference_class_stood(drawn):
    net, inp, g, g_grad = drawn
    truth = up.truth_of(g, g_grad)
    err = up.errors(up.evaluate(net, inp['x'], inp['t'], inp['gout'], inp['pos']), truth, up.FWD + up.GRAD)
    stored = {k: float((g_grad if k in up.GRAD else g)['e32_' + k]) for k in err}
    for k in up.FWD + up.GRAD:
        print(f'{k:8s} fp32 CPU {err[k]:.3e}   stored e_cpu32 {stored[k]:.3e}')
    for k in up.FWD + up.GRAD:
        assert 0 < err[k] < 1e-4, k                                  # neither degenerate nor mis-indexed
        assert stored[k] / ROUNDING < err[k] < stored[k] * ROUNDING, k

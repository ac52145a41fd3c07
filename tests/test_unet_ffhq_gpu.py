"""GPU: the score network the benchmark times -- unet.create_model(**unet.FFHQ_CONFIG), 93.6 M parameters, 128 to 512
channels, 256 x 256 -- on its HIP routes against the float64 probes of fixture G22 (oracle/gen_golden_unet_256.py).

One image pair (B = 2) is the smallest input on which the production routes fire: the Winograd tables are keyed by the
workload's (c, k, h, w) and say other batch sizes follow the n = 64 rows, and the one-pass GroupNorm's split counts do
not depend on n.  So this runs, layer for layer, the kernels bench.py runs.

The bound.  A group (oracle.unet_probe: 26 forward tensors, 26 gradients; the metric is max |err| at 4096 probes over
max |float64 tensor|) passes when

    err_custom <= M * max(err_vendor, e_cpu32),

err_vendor being the same network in the same process on the vendor route (NHMC_WINO=0, NHMC_FUSED_GN=0: MIOpen and
ATen) and e_cpu32 the reference class in fp32 on the CPU, stored in the fixture.  Neither is the code under test.
M = 2 r: the 2 is what tests/test_wino_conv_gpu.py grants the kernel over its fp32 restatement, r is the largest ratio
of that restatement's error to the direct fp32 convolution's, both against float64, measured on the CPU with that
file's `case()` at shape (1, C, 64, 4, 64) for the kernel's input-channel counts of this network's routed convolutions
(`restatement_ratio()` below; `python -m tests.test_unet_ffhq_gpu` prints it, no GPU needed):

    forward        C = 128: 1.49   256: 2.38   384: 3.08   512: 2.54   768: 3.98   1024: 3.42
    backward-data  C = 128: 1.43   256: 2.68   512: 3.67
    r = 3.98, M = 7.96

First run on an MI355X: the three tests take 18 s, 13 s of them the first pass of a process over these shapes on both
routes (code objects and the vendor library's solvers being loaded; a second pass in the same process takes 0.7 s).
Per group: custom, vendor, e_cpu32, each x 1e-6 (the loss: relative error; DESIGN.md section 5 has the full figures):

    in00      0.10  0.10  0.08   in01      0.87  0.88  0.15   in02      1.88  1.89  0.16
    in03      1.84  1.84  0.20   in04      2.33  2.33  0.22   in05      1.91  1.94  0.29
    in06      2.91  2.86  0.29   in07      2.70  2.70  0.37   in08      3.03  3.02  0.27
    in09      2.76  2.85  0.48   in10      2.69  2.66  0.29   in11      3.17  3.23  0.30
    mid       2.62  2.66  0.25   out00     2.27  2.34  0.36   out01     3.05  2.96  0.63
    out02     2.32  2.31  0.62   out03     3.86  3.75  0.83   out04     3.17  3.30  0.83
    out05     3.21  3.33  0.82   out06     2.82  2.74  1.02   out07     2.39  2.44  0.71
    out08     2.54  2.82  0.79   out09     2.26  2.48  0.73   out10     2.11  1.86  0.52
    out11     1.29  1.31  0.35   net       0.90  0.97  0.50   g_out11   0.66  0.68  0.09
    g_out10   0.75  0.82  0.17   g_out09   0.68  0.66  0.25   g_out08   0.67  0.78  0.22
    g_out07   0.60  0.67  0.21   g_out06   0.79  0.71  0.34   g_out05   0.65  0.82  0.29
    g_out04   0.62  0.63  0.28   g_out03   0.81  0.92  0.30   g_out02   0.89  0.92  0.48
    g_out01   0.96  1.06  0.50   g_out00   1.12  1.06  0.50   g_mid     1.09  1.11  0.62
    g_in11    0.93  0.91  0.51   g_in10    1.20  1.24  0.71   g_in09    1.09  1.11  0.70
    g_in08    1.13  1.07  0.63   g_in07    1.80  1.72  0.41   g_in06    1.21  0.99  0.34
    g_in05    0.80  0.79  0.34   g_in04    1.00  0.98  0.31   g_in03    0.70  0.77  0.20
    g_in02    0.81  0.81  0.25   g_in01    0.73  0.85  0.26   g_in00    0.95  1.02  0.20
    gx        0.89  0.90  0.31   loss      0.17  0.17  0.02   eng_xt    2.95  2.98  1.45
    eng_grad  0.98  0.80  0.50

The custom route stands where the vendor route stands, within 0.8 - 1.25 x of it in every group; both are 1.8 - 12 x
the CPU's fp32 error in the forward groups from in01 on and 1.5 - 7.5 x in the gradients.  The largest custom / bound
ratio is 0.15 (g_in06, eng_grad).
"""
import pytest
import torch

from oracle import schedule
from oracle import unet_probe as up

pytestmark = pytest.mark.gpu

R = 3.98
M = 2 * R
VENDOR = {'NHMC_WINO': '0', 'NHMC_FUSED_GN': '0'}


def routed_rows(n=2):
    """{(backward, c, k, h, w)} in the KERNEL's terms (c channels in, k out) of the rows of unet.conv3x3_shapes() that
    unet.wino_route sends to the Winograd kernel for a batch of n with an input that requires grad."""
    from nhmc import unet
    rows = set()
    for c, k, res, _ in unet.conv3x3_shapes():
        conv = torch.nn.Conv2d(c, k, 3, padding=1, device='cuda').requires_grad_(False)
        route = unet.wino_route(conv, torch.empty(n, c, res, res, device='cuda', requires_grad=True))
        if route is not None and route[0]:
            rows.add((False, c, k, res, res))
        if route is not None and route[1]:
            rows.add((True, k, c, res, res))
    return rows


def restatement_ratio():
    """r of the module docstring: {(backward, C): restatement error / direct convolution error} on the CPU."""
    from nhmc import unet
    import nhmc.kernels as K
    from tests.test_wino_conv_gpu import case
    out = {}
    for c, k, res, _ in unet.conv3x3_shapes():
        for backward, cin, kout in ((0, c, k), (1, k, c)):
            if K.conv3x3_wino_k32_covers(2, cin, kout, res, res) and (backward, cin) not in out:
                cs = case((1, cin, 64, 4, 64), backward)
                out[backward, cin] = cs['yard'] / cs['direct']
    return out


@pytest.fixture(scope='module')
def ffhq(golden):
    """The network, built once: seeded weights on the card, frozen; the seeded inputs; the float64 probes."""
    from nhmc import unet
    net = unet.create_model(**unet.FFHQ_CONFIG).eval()
    inp = up.seeded_inputs(net)
    g, g_grad = golden('g22_unet_ffhq_256.npz'), golden('g22_unet_ffhq_256_grad.npz')
    assert inp['weight_sha'] == g['weight_sha256'].tolist() and up.sha(inp['x']) == str(g['x_sha256'])
    e32 = {k[4:]: float(v) for f in (g, g_grad) for k, v in f.items() if k.startswith('e32_')}
    return dict(net=net.cuda().requires_grad_(False), inp=inp, truth=up.truth_of(g, g_grad), e32=e32, g=g)


def network_errors(ffhq):
    inp = ffhq['inp']
    rec = up.evaluate(ffhq['net'], inp['x'].cuda(), inp['t'].cuda(), inp['gout'].cuda(), inp['pos'])
    return up.errors(rec, ffhq['truth'], up.FWD + up.GRAD)


def check_bound(custom, vendor, e32, orders):
    bound = {k: M * max(vendor[k], e32[k]) for k in custom}
    for k in custom:
        print(f'{k:9s} custom {custom[k]:.3e}   vendor {vendor[k]:.3e}   e_cpu32 {e32[k]:.3e}   bound {bound[k]:.3e}')
    for order in orders:
        bad = up.first_over(custom, bound, order)
        assert bad is None, (f'{bad} is the first group in execution order over its bound: custom {custom[bad]:.3e} > '
                             f'{M} * max(vendor {vendor[bad]:.3e}, e_cpu32 {e32[bad]:.3e})')


def test_forward_and_input_gradient_on_the_production_routes(ffhq, monkeypatch):
    """Defaults (Winograd on, fused and one-pass GroupNorm on) against the float64 probes, group by group, bounded by
    M times the worse of the vendor route and the reference's own fp32 error.  A failure names the first block in
    execution order (for gradients: reverse order) that is over its bound -- the place to start reading."""
    custom = network_errors(ffhq)
    for k, v in VENDOR.items():
        monkeypatch.setenv(k, v)
    vendor = network_errors(ffhq)
    print()
    check_bound(custom, vendor, ffhq['e32'], (up.FWD, up.GRAD))


def _null(p):
    return p is None or getattr(p, 'value', p) in (None, 0)


def test_the_production_routes_really_ran(ffhq, monkeypatch):
    """One evaluation with the nhmc.kernels front ends (and, for the GroupNorm forms, which share two front ends, the
    library entries behind them) wrapped: the Winograd kernel saw exactly the rows of conv3x3_shapes() that wino_route
    selects at B = 2, in both geometries and both directions; every GroupNorm form, the bias/residual epilogue and the
    resample kernels ran; on the vendor route none of them did."""
    import nhmc.kernels as K
    lib = K._lib.load()
    seen, count = set(), {}

    def bump(name):
        count[name] = count.get(name, 0) + 1

    def front(name, note=None):
        inner = getattr(K, name)

        def wrapped(*a, **kw):
            bump(name)
            if note is not None:
                note(*a, **kw)
            return inner(*a, **kw)
        monkeypatch.setattr(K, name, wrapped)

    def entry(name, note=None):
        inner = getattr(lib, name)

        def wrapped(*a):
            bump(name)
            if note is not None:
                note(*a)
            return inner(*a)
        monkeypatch.setattr(lib, name, wrapped)

    def wino(x, weight, bias=None, add=None, backward=False):
        seen.add((bool(backward), x.shape[1], weight.shape[1 if backward else 0], x.shape[2], x.shape[3]))
        if add is not None and bias is not None:
            bump('epilogue')
    front('conv3x3_wino', wino)
    front('bias_add2', lambda *a: bump('epilogue'))
    front('sr_H')
    front('sr_Ht')
    entry('nhmc_gn_act_fwd')
    entry('nhmc_gn_act_bwd_fs', lambda *a: None if _null(a[12]) else bump('fork_bwd'))
    entry('nhmc_gn_onepass_fwd', lambda *a: None if _null(a[1]) else bump('two_source_fwd'))
    # a[12]: the skip path's gradient, added in the kernel; a[15] < a[19]: the gradient leaves as two tensors (c1 < C)
    entry('nhmc_gn_onepass_bwd', lambda *a: None if _null(a[12]) else bump('fork_bwd' if a[15] == a[19] else 'two_source_bwd'))

    want = routed_rows()
    network_errors(ffhq)
    print('\nkernel calls:', dict(sorted(count.items())))
    assert seen == want, f'missing {sorted(want - seen)}  unexpected {sorted(seen - want)}'
    for backward in (False, True):
        widths = {w for b, _, _, _, w in seen if b == backward}
        assert widths == {256, 128, 64, 32, 16}, (backward, widths)     # wide: 256 / 128 / 64; narrow: 32 / 16
    for form in ('nhmc_gn_act_bwd_fs', 'nhmc_gn_onepass_fwd', 'nhmc_gn_onepass_bwd', 'two_source_fwd', 'two_source_bwd',
                 'fork_bwd', 'epilogue', 'sr_H', 'sr_Ht'):
        assert count.get(form, 0) >= 1, form
    seen.clear()
    count.clear()
    for k, v in VENDOR.items():
        monkeypatch.setenv(k, v)
    network_errors(ffhq)
    assert not seen and not count, (seen, count)


def test_engine_decode_and_gradient_with_this_network(ffhq, monkeypatch):
    """LeapfrogEngine.decode_and_grad on the ladder [250, 500, 750] / [-1, 250, 500] with `inpaint_random` at 256, the
    fused last VJP on, B = 2: clipped decode and gradient under the bound rule above against the engine on the vendor
    route; the loss relatively within M * max(vendor's relative loss error, e_cpu32 of the loss); a hipGraph replay
    within the 1e-5 tests/test_hygiene_gpu.py uses between solver choices.

    The gradient has a kink wherever a clip argument of the ladder crosses +-1; the fixture's masks are those of float64
    and of the fp32 reference class alike, its closest argument lies 9.6e-8 from the kink (`eng_clip_margin`).  Should
    eng_grad alone ever leave its bound, with the decode and the loss inside theirs and on both routes, a mask bit
    that the card rounds to the other side is the first thing to rule out; on the first run none did."""
    from nhmc import operators, sampler
    from oracle.operators import InpaintRef
    from tests.test_kernels_gpu import rel
    inp, g, truth = ffhq['inp'], ffhq['g'], ffhq['truth']
    dev = torch.device('cuda')
    op = operators.Inpainting(3, 256, inp['missing'], dev)
    y = (InpaintRef(3, 256, inp['missing']).H(inp['eng_img']) + inp['eng_noise']).cuda()
    x = inp['eng_x'].cuda()
    eng = sampler.LeapfrogEngine(ffhq['net'], op, schedule.betas_fp32().cuda(), up.SEQ, up.SEQ_NEXT, dev)
    assert eng.fuse_last and hasattr(op, 'fused_last_vjp')
    loss64 = torch.from_numpy(g['eng_loss'])

    def run(**kw):
        xt, loss, ga, gb = eng.decode_and_grad(x, y, **kw)
        return xt, loss, ga, gb

    def errs(out):
        xt, loss, ga, gb = out
        e = up.errors(dict(eng_xt=up.probe(xt, inp['pos']), eng_grad=up.probe(ga + gb, inp['pos'])), truth, up.ENGINE)
        return e, float(((loss.cpu() - loss64).abs() / loss64.abs()).max())
    eager = [t.clone() for t in run()]
    custom, custom_loss = errs(eager)
    graphed = run(graph=True)
    for name, a, b_ in zip(('xt', 'loss', 'g_direct', 'g_score'), eager, graphed):
        assert rel(b_, a) < 1e-5, name
    for k, v in VENDOR.items():
        monkeypatch.setenv(k, v)
    vendor, vendor_loss = errs(run())
    print()
    e32_loss = float(g['e32_eng_loss'])
    print(f'loss      custom {custom_loss:.3e}   vendor {vendor_loss:.3e}   e_cpu32 {e32_loss:.3e}')
    check_bound(custom, vendor, ffhq['e32'], (up.ENGINE,))
    assert custom_loss <= M * max(vendor_loss, e32_loss)


if __name__ == '__main__':
    ratios = restatement_ratio()
    for (backward, c), v in sorted(ratios.items()):
        print(f'{"backward-data" if backward else "forward"} C = {c}: {v:.2f}')
    print(f'r = {max(ratios.values()):.2f}')

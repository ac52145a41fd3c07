"""GPU: the observation cache is bypassed while a hipGraph is captured, for every operator that uses it; and the strided
operands of kernels.py (film, g_pair) get their device and dtype check before a pointer reaches the library."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cs(dev):
    from nhmc import operators
    return operators.build_operator('cs2', 3, 16, dev, generator=torch.Generator().manual_seed(3)), 16


def _srconv(dev):
    from nhmc import operators
    return operators.SRConv(operators.bicubic_taps(2), 3, 32, dev, stride=1), 32


def _aniso(dev):
    from nhmc import operators
    return operators.build_operator('deblur_aniso', 3, 32, dev), 32


def _aniso_projected(dev):
    from nhmc import operators
    return operators.build_operator('deblur_aniso', 3, 32, dev, spectral_projected=True), 32


@pytest.mark.parametrize('case', [_cs, _srconv, _aniso, _aniso_projected], ids=lambda f: f.__name__.strip('_'))
def test_a_captured_data_term_reads_the_buffer_not_the_cache(case):
    """The engine's graph path (sampler.LeapfrogEngine._graphed_chunk): two warm-up calls on a side stream fill the cache
    with the form of the static buffer's first content, the capture must neither read nor extend it, and a replay after
    the buffer was refilled gives the bits of an eager call on the new observation."""
    from nhmc.operators import ObservationCache
    dev = torch.device('cuda')
    op, d = case(dev)
    (cache,) = [v for v in vars(op).values() if isinstance(v, ObservationCache)]
    B = 2
    g_ = torch.Generator().manual_seed(d)
    x = (0.7 * torch.randn(B, 3, d, d, generator=g_)).cuda()
    y_a = op.H((0.5 * torch.randn(B, 3, d, d, generator=g_)).cuda()) + 0.1 * torch.randn(B, op.M, generator=g_).cuda()
    y_b = op.H((0.5 * torch.randn(B, 3, d, d, generator=g_)).cuda()) + 0.1 * torch.randn(B, op.M, generator=g_).cuda()
    ys = y_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            loss_a, grad_a = op.data_term(x, ys)
    torch.cuda.current_stream().wait_stream(side)
    n0 = len(cache)
    assert n0 == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = op.data_term(x, ys)
    assert len(cache) == n0
    ys.copy_(y_b)
    graph.replay()
    torch.cuda.synchronize()
    want_loss, want_grad = op.data_term(x, y_b.clone())
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    assert not torch.equal(want_loss, loss_a) and not torch.equal(want_grad, grad_a)      # the warm-up form's numbers differ


class _Stub:
    """Stands in for libnhmc: records the entries asked for; nothing of the library can run."""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def entry(*args):
            self.names.append(name)
            return 1 if name.endswith(('_splits', '_prefers', '_tiles')) else 0
        return entry


def _gn_launched(names):
    return [n for n in names if n.startswith('nhmc_gn_') and n.endswith('fwd')]


def test_film_is_checked_before_the_groupnorm_launch(monkeypatch):
    import nhmc.kernels as K
    from nhmc import _lib
    x = torch.zeros(2, 64, 8, 8, device='cuda')
    gamma, beta = torch.ones(64, device='cuda'), torch.zeros(64, device='cuda')
    film = torch.zeros(2, 128, device='cuda')
    for bad in (film.cpu(), film.half()):
        stub = _Stub()
        monkeypatch.setattr(_lib, 'load', lambda: stub)
        with pytest.raises(_lib.NhmcError):
            K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, bad)
        assert not _gn_launched(stub.names)
    stub = _Stub()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, film)
    assert len(_gn_launched(stub.names)) == 1


def test_g_pair_is_checked_before_the_cached_leapfrog_launch(monkeypatch):
    import nhmc.kernels as K
    from nhmc import _lib
    B = 2
    x, x_out, p = (torch.zeros(B, 3, 8, 8, device='cuda') for _ in range(3))
    g_pair = torch.zeros(2, B, 3, 8, 8, device='cuda')
    sel = torch.zeros(B, dtype=torch.int32, device='cuda')
    eps = sig = torch.ones(B, dtype=torch.float64, device='cuda')
    ws = torch.zeros(B * 2, dtype=torch.float64, device='cuda')
    stub = _Stub()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    with pytest.raises(_lib.NhmcError):
        K.leapfrog_first_cached(x, x_out, p, g_pair.half(), sel, eps, sig, 1.0, ws)
    assert 'nhmc_leapfrog_first_cached' not in stub.names
    K.leapfrog_first_cached(x, x_out, p, g_pair, sel, eps, sig, 1.0, ws)
    assert stub.names.count('nhmc_leapfrog_first_cached') == 1

"""GPU: whole HMC runs under hipGraph replay (`graph=True`, `--graph`) against the eager launches, bit for bit.

The other graph tests call `LeapfrogEngine.decode_and_grad` on one fixed batch and allow 1e-5, because their score
networks convolve and MIOpen may pick another solver inside a capture.  A whole run cannot be compared at a tolerance: a
last-bit difference flips a Metropolis decision some trajectories later and the two runs part for good.  So the score
here (`PointwiseScore`) is built from elementwise ATen ops, `torch.roll` along H and W, and per-channel constants held
in registered buffers -- no library GEMM or convolution, no reduction, no host-to-device copy in `forward`:

  * it launches the same kernels, in the same order, captured or not: nothing in it selects an algorithm at run time;
  * every output element is a fixed expression of a few input elements OF THE SAME SAMPLE, so an output does not depend
    on the batch the sample sits in, nor on the sample's place in it.

The project's own kernels are stream-ordered launches with fixed summation orders.  A replayed run must therefore equal
the eager run in every bit, and a compacted run the uncompacted one: every comparison in this module is `torch.equal`
(or `==` on integers); there is no tolerance anywhere.

What a run under replay does that a single `decode_and_grad` does not: the graph's own gradient buffers go straight
into the fused update / the gradient cache and are overwritten by the next replay of the same graph; the static
observation buffer is refilled with another chunk's y at every replay (anything derived from y and cached across the
capture would serve the wrong chunk); compaction captures new graphs in the middle of a run, with every per-chain
tensor re-ordered; and the engine's ladder counters and its graph bookkeeping are read by the caller afterwards.
"""
import types

import numpy as np
import pytest
import torch

from oracle import schedule as osched

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
DEV = 'cuda'


def gen(seed):
    return torch.Generator().manual_seed(seed)


class PointwiseScore(torch.nn.Module):
    """[n,3,H,W], t[n] -> [n,6,H,W] (learn_sigma layout) or [n,3,H,W].  Differentiable in x, depends on t, couples
    neighbouring pixels through `torch.roll`; sample b's output depends on sample b alone."""

    def __init__(self, learn_sigma=True, seed=0):
        super().__init__()
        g_ = gen(seed)
        c = lambda mean, std: (mean + std * torch.randn(1, 3, 1, 1, generator=g_))
        self.learn_sigma = learn_sigma
        for name, v in (('w_x', c(0.7, 0.1)), ('w_h', c(0.0, 0.2)), ('w_w', c(0.0, 0.2)), ('bias', c(0.0, 0.1)),
                        ('w_s', c(1.0, 0.2)), ('w_v', c(0.5, 0.1))):
            self.register_buffer(name, v)

    def eps(self, x, t):
        a = (t / 1000.0).view(-1, 1, 1, 1)
        u = x * self.w_x + torch.roll(x, 1, 2) * self.w_h + torch.roll(x, -1, 3) * self.w_w + self.bias
        return torch.tanh(u) * (0.5 + a) + torch.sin(x * self.w_s) * (a * 0.25)

    def forward(self, x, t):
        e = self.eps(x, t)
        return torch.cat([e, torch.tanh(e * self.w_v) * 0.1], dim=1) if self.learn_sigma else e


class NoGradScore(PointwiseScore):
    """The score without gradient (what the latent model's `apply_model` is): three channels, evaluated under no_grad, so
    the engine sees `outs[s] is None` and asks the mix VJP for no g_e."""

    def __init__(self, seed=0):
        super().__init__(learn_sigma=False, seed=seed)

    def forward(self, x, t):
        with torch.no_grad():
            return self.eps(x, t)


def test_the_stand_in_score_is_what_the_comparisons_need():
    """differentiable in x, t-dependent, sample-local, and the same bits whatever batch a sample is evaluated in"""
    net = PointwiseScore().to(DEV)
    x = torch.randn(5, 3, 16, 16, generator=gen(1)).to(DEV).requires_grad_(True)
    t = torch.tensor([750., 750., 500., 250., 250.], device=DEV)
    e = net(x, t)
    assert e.shape == (5, 6, 16, 16) and e.requires_grad
    (g,) = torch.autograd.grad(e[:, :3], x, torch.ones_like(e[:, :3]))
    assert float(g.abs().max()) > 0
    assert not torch.equal(e[0], net(x[:1], t[2:3])[0])                              # t matters
    for lo, hi in ((0, 2), (2, 3), (3, 5)):                                          # batch invariance, forward and backward
        xs = x[lo:hi].detach().requires_grad_(True)
        es = net(xs, t[lo:hi])
        assert torch.equal(es, e[lo:hi])
        (gs,) = torch.autograd.grad(es[:, :3], xs, torch.ones_like(es[:, :3]))
        assert torch.equal(gs, g[lo:hi])
    x2 = x.detach().clone()
    x2[3] += 1.0                                                                     # another sample changes: mine does not
    assert torch.equal(net(x2, t)[:3], e[:3]) and torch.equal(net(x2, t)[4], e[4])
    n = NoGradScore().to(DEV)(x, t)
    assert n.shape == (5, 3, 16, 16) and not n.requires_grad


# --------------------------------------------------------------------------------------------- #
# 1. one trajectory, every operator
# --------------------------------------------------------------------------------------------- #
OPERATORS = ['inpaint_random', 'inpaint_slots', 'sr4', 'color', 'cs4', 'deblur_aniso', 'deblur_gauss', 'sr_bicubic2',
             'hdr', 'phase_retrieval']
EPS = np.array([0.05, 0.04, 0.03, 0.0, 0.05])          # chain 3 frozen (eps_eff = 0): the vectors of
SIG = np.array([1.7, 0.9, 0.1, 0.5, 1.0])              # test_sampler_gpu.py::test_trajectory_does_not_depend_on_the_score_chunking
KEYS = ('x_prop', 'p', 'xt', 'loss', 'H0', 'H1')


def build_op(deg, dim, seed):
    import nhmc.operators as ops
    if deg == 'inpaint_slots':                          # single elements missing, not whole pixels: the ragged slot form
        missing = torch.randperm(3 * dim * dim, generator=gen(seed))[: int(3 * dim * dim * 0.6)]
        op = ops.Inpainting(3, dim, missing, DEV)
        assert op.mask_words is None
        return op
    op = ops.build_operator(deg, 3, dim, torch.device(DEV), generator=gen(seed))
    if deg == 'inpaint_random':
        assert op.mask_words is not None               # the pixel-mask form
    if deg == 'deblur_aniso':
        assert not op.projected                        # the default eight-product form
    return op


def observe(op, B, dim, g_):
    x_orig = (torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1).to(DEV)
    y = op.H(x_orig)
    return x_orig, (y + 0.1 * torch.randn(y.shape, generator=g_).to(DEV)).contiguous()


def engine_for(net, op, chunk):
    from nhmc import plugin, sampler
    algo = plugin.HMC(net, op, 0.1)
    return sampler.LeapfrogEngine(algo.score, op, osched.betas_fp32().to(DEV), SEQ, SEQ_NEXT, torch.device(DEV), chunk=chunk)


def state_for(B):
    from nhmc import sampler
    st = sampler.ChainState(B, 1.0, 0.05, DEV)
    st['eps_eff'].copy_(torch.as_tensor(EPS[:B].copy()))
    st['sigma_y'].copy_(torch.as_tensor(SIG[:B].copy()))
    return st


def trajectory(eng, x, p, y, L, graph, cache=None):
    """-> clones of the six results (xt / loss are the engine's buffers); the caller's x must come back untouched"""
    from nhmc import sampler
    x0 = x.clone()
    got = sampler.run_trajectory(eng, x0, p.clone(), y, state_for(x.shape[0]), 1.0, L, graph=graph, cache=cache)
    torch.cuda.synchronize()
    assert torch.equal(x0, x)
    return {k: got[k].clone() for k in KEYS}


def assert_same(a, b, what):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)
        assert bool(torch.isfinite(a[k].double()).all()), (what, k)


@pytest.mark.parametrize('chunk', [None, 2])
@pytest.mark.parametrize('deg', OPERATORS)
def test_trajectory_under_replay_is_the_eager_trajectory(deg, chunk):
    """B = 5: chunk 2 gives ragged chunks 2, 2, 1 -- the size-2 graph is replayed twice per step with different x and y,
    a second graph serves the tail.  The second trajectory goes through the SAME graphs with the observations flipped
    along the batch and a new position: anything derived from y and kept across the capture shows here."""
    B, L = 5, 4
    dim = 64 if deg == 'sr_bicubic2' else 32
    op = build_op(deg, dim, 100)
    g_ = gen(101)
    _, y = observe(op, B, dim, g_)
    x, p = (torch.randn(B, 3, dim, dim, generator=g_).to(DEV) for _ in range(2))
    net = PointwiseScore().to(DEV)
    eager, graphed = engine_for(net, op, chunk), engine_for(net, op, chunk)
    want = trajectory(eager, x, p, y, L, False)
    got = trajectory(graphed, x, p, y, L, True)
    assert_same(want, got, 'first')
    assert torch.equal(got['x_prop'][3], x[3])                                    # the frozen chain did not move
    assert not torch.equal(got['x_prop'][0], x[0])
    n_graphs = len(graphed._graphs)
    assert n_graphs == graphed.graphs_captured == (1 if chunk is None else 2)
    y2 = y.flip(0).contiguous()
    x2, p2 = (torch.randn(B, 3, dim, dim, generator=g_).to(DEV) for _ in range(2))
    want2 = trajectory(eager, x2, p2, y2, L, False)
    got2 = trajectory(graphed, x2, p2, y2, L, True)
    assert_same(want2, got2, 'flipped')
    assert not torch.equal(want2['loss'], want['loss'])
    assert len(graphed._graphs) == graphed.graphs_captured == n_graphs            # pure replays
    # the counters: (L + 1) ladders per trajectory and chunk, replayed or launched
    chunks = len(eager._chunks(B))
    assert eager.n_ladders == graphed.n_ladders == 2 * (L + 1) * chunks
    assert eager.n_chain_ladders == graphed.n_chain_ladders == 2 * (L + 1) * B


@pytest.mark.parametrize('chunk', [None, 2])
def test_trajectory_with_the_gradient_cache_under_replay(chunk):
    """prime -> FIRST from the cache -> LAST into the free slots, then (after a mixed accept) a second trajectory whose
    first half step reads both slots: the cache's g / loss / sel are the eager run's"""
    import nhmc.kernels as K
    from nhmc import sampler
    B, L, dim = 5, 4, 32
    op = build_op('inpaint_random', dim, 110)
    g_ = gen(111)
    _, y = observe(op, B, dim, g_)
    x, p, p2 = (torch.randn(B, 3, dim, dim, generator=g_).to(DEV) for _ in range(3))
    accept = torch.tensor([1, 0, 1, 0, 0], dtype=torch.int32, device=DEV)
    net = PointwiseScore().to(DEV)
    res = {}
    for graph in (False, True):
        eng = engine_for(net, op, chunk)
        cache = sampler.GradCache(x)
        first = trajectory(eng, x, p, y, L, graph, cache=cache)
        assert cache.valid
        snap = [t.clone() for t in (cache.g, cache.loss, cache.sel)]
        K.grad_cache_flip(accept, cache.sel)
        x_next = torch.where(accept.bool().view(-1, 1, 1, 1), first['x_prop'], x).contiguous()
        second = trajectory(eng, x_next, p2, y, L, graph, cache=cache)
        res[graph] = (first, second, snap, [t.clone() for t in (cache.g, cache.loss, cache.sel)], eng)
    assert_same(res[False][0], res[True][0], 'first')
    assert_same(res[False][1], res[True][1], 'second')
    for i in (2, 3):
        for a, b, k in zip(res[False][i], res[True][i], ('g', 'loss', 'sel')):
            assert torch.equal(a, b), (i, k)
    assert res[True][3][2].tolist() == [1, 0, 1, 0, 0]
    chunks = 1 if chunk is None else 3
    for eng in (res[False][4], res[True][4]):
        assert eng.n_ladders == (2 * L + 1) * chunks and eng.n_chain_ladders == (2 * L + 1) * B
    assert res[True][4].graphs_captured == (1 if chunk is None else 2)


@pytest.mark.parametrize('chunk', [None, 2])
def test_trajectory_with_a_score_without_gradient_under_replay(chunk):
    B, L, dim = 5, 4, 32
    op = build_op('inpaint_random', dim, 120)
    g_ = gen(121)
    _, y = observe(op, B, dim, g_)
    x, p = (torch.randn(B, 3, dim, dim, generator=g_).to(DEV) for _ in range(2))
    net = NoGradScore().to(DEV)
    eager, graphed = engine_for(net, op, chunk), engine_for(net, op, chunk)
    xt, loss, ga, gb = eager.decode_and_grad(x, y)
    assert gb is None                                                              # the path this test is about
    assert_same(trajectory(eager, x, p, y, L, False), trajectory(graphed, x, p, y, L, True), 'no-grad score')
    y2 = y.flip(0).contiguous()
    assert_same(trajectory(eager, p, x, y2, L, False), trajectory(graphed, p, x, y2, L, True), 'no-grad score, flipped')
    assert graphed.graphs_captured == (1 if chunk is None else 2)


# --------------------------------------------------------------------------------------------- #
# 2. - 4. whole runs
# --------------------------------------------------------------------------------------------- #
RUN_FIELDS = ('samples', 'x', 'xt', 'epoch', 'n_accept', 'n_reject', 'psnr')


def problem(B, dim, seed):
    from nhmc import plugin
    op = build_op('inpaint_random', dim, seed)
    g_ = gen(seed + 1)
    x_orig, y = observe(op, B, dim, g_)
    x = torch.randn(B, 3, dim, dim, generator=g_).to(DEV)
    return plugin.HMC(PointwiseScore().to(DEV), op, 0.1), op, x, y, x_orig


def run(prob, opt, seed, **kw):
    from nhmc import sampler
    algo, op, x, y, x_orig = prob
    return sampler.hmc_chains(x, osched.betas_fp32().to(DEV), SEQ, SEQ_NEXT, algo, opt, y, op, x_orig,
                              noise=sampler.PhiloxNoise(seed, 0), collect_trace=True, **kw)


def same_run(a, b, total, every_dH=False):
    """every result field, every trace entry; dH of a chain for as long as the chain runs (a finished chain's dH is that
    of a frozen chain in an uncompacted run and not computed at all in a compacted one), or every dH"""
    assert a.iters == b.iters and len(a.trace) == len(b.trace) == a.iters
    for k in RUN_FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for i, (ra, rb) in enumerate(zip(a.trace, b.trace)):
        for k in ('accept', 'epoch', 'sigma_y', 'eps'):
            assert torch.equal(ra[k], rb[k]), (i, k)
        running = ra['epoch'] < total
        assert torch.equal(ra['dH'][running], rb['dH'][running]), (i, 'dH')
        if every_dH:
            assert torch.equal(ra['dH'], rb['dH']), (i, 'dH')


RUN2 = dict(B=3, dim=16, seed=130, philox=5, opt=types.SimpleNamespace(tau=0.3, epsilon=0.05, m=1.0, sigma_0=0.1),
            epochs=6, sampling=2)


@pytest.fixture(scope='module')
def eager_runs():
    """the references of test 2, one per (reuse, chunk), computed once"""
    prob, out = problem(RUN2['B'], RUN2['dim'], RUN2['seed']), {}

    def get(reuse, chunk):
        if (reuse, chunk) not in out:
            out[reuse, chunk] = run(prob, RUN2['opt'], RUN2['philox'], epochs=RUN2['epochs'], sampling=RUN2['sampling'],
                                    reuse=reuse, chunk=chunk, compact=False, graph=False)
        return out[reuse, chunk]
    return prob, get


@pytest.mark.parametrize('chunk', [None, 2])
@pytest.mark.parametrize('reuse', [False, True])
def test_whole_run_under_replay_is_the_eager_run_and_counts_its_ladders(eager_runs, reuse, chunk):
    prob, get = eager_runs
    B, epochs, sampling, eps0 = RUN2['B'], RUN2['epochs'], RUN2['sampling'], RUN2['opt'].epsilon
    total = epochs + 2 * sampling
    eager = get(reuse, chunk)
    # the eager run alone shows that the run contains what the comparison is about
    assert int(eager.n_accept.min()) == total                                      # every chain ran to its end
    assert int(eager.n_reject.sum()) > 0
    eps_seen = {float(e) for r in eager.trace for e in r['eps']}
    assert eps_seen - {eps0, 0.01}, eps_seen        # the eps / tau anneal (x 0.95 from the second reject in a row on)
    print('iters', eager.iters, 'rejects', eager.n_reject.tolist(), 'eps seen', sorted(eps_seen))
    graphed = run(prob, RUN2['opt'], RUN2['philox'], epochs=epochs, sampling=sampling, reuse=reuse, chunk=chunk,
                  compact=False, graph=True)
    same_run(eager, graphed, total, every_dH=True)
    L, chunks = eager.L, (1 if chunk is None else -(-B // chunk))
    assert L == graphed.L == 5                                                      # floor(0.3 / 0.05) in floating point
    per_run = (eager.iters * L + 1) if reuse else eager.iters * (L + 1)
    assert eager.ladders == per_run * chunks and eager.chain_ladders == per_run * B
    assert graphed.ladders == per_run * chunks, (graphed.ladders, per_run * chunks)
    assert graphed.chain_ladders == per_run * B, (graphed.chain_ladders, per_run * B)
    assert eager.graphs_captured == eager.graphs_live_max == 0
    assert graphed.graphs_captured == graphed.graphs_live_max == (1 if chunk is None or chunk >= B else 2)


RUN3 = dict(B=6, dim=16, seed=140, philox=9, opt=types.SimpleNamespace(tau=0.2, epsilon=0.05, m=1.0, sigma_0=0.1),
            epochs=5, sampling=2)
COMPACTIONS = [(1, None), (2, None), (None, 2), (None, 4)]          # (compact_quantum, chunk)


@pytest.fixture(scope='module')
def compaction_runs():
    """test 3's reference (eager, uncompacted) and, per (quantum, chunk), the eager compacted and the graphed compacted
    run -- each computed once, shared by tests 3 and 4"""
    prob, out = problem(RUN3['B'], RUN3['dim'], RUN3['seed']), {}
    kw = dict(epochs=RUN3['epochs'], sampling=RUN3['sampling'])
    full = run(prob, RUN3['opt'], RUN3['philox'], compact=False, **kw)
    total = RUN3['epochs'] + 2 * RUN3['sampling']
    finish = [max(i for i, r in enumerate(full.trace) if int(r['epoch'][c]) < total) for c in range(RUN3['B'])]

    def get(quantum, chunk):
        if (quantum, chunk) not in out:
            out[quantum, chunk] = tuple(run(prob, RUN3['opt'], RUN3['philox'], compact=True, compact_quantum=quantum,
                                            chunk=chunk, graph=graph, **kw) for graph in (False, True))
        return out[quantum, chunk]
    return full, finish, total, get


def batch_sizes(finish, B, iters, q):
    """chains in the batch at every trajectory of a compacted run: the running ones, rounded up to the quantum"""
    return [min(B, -(-sum(1 for f in finish if f >= i) // q) * q) for i in range(iters)]


@pytest.mark.parametrize('quantum,chunk', COMPACTIONS)
def test_compacted_run_under_replay_is_the_eager_uncompacted_run(compaction_runs, quantum, chunk):
    """six chains that finish at different trajectories; compaction captures new graphs mid-run, with the per-chain
    state, the cache slots and y_0 re-ordered"""
    full, finish, total, get = compaction_runs
    B = RUN3['B']
    assert len(set(finish)) > 2, finish                                 # staggered finishes, or the test shows nothing
    assert int(full.n_reject.sum()) > 0 and int(full.n_accept.min()) == total
    eager_c, graph_c = get(quantum, chunk)
    same_run(full, eager_c, total)
    same_run(full, graph_c, total)
    sizes = batch_sizes(finish, B, full.iters, quantum or chunk)
    assert len(set(sizes)) > 1, sizes                                   # the batch did shrink
    assert full.chain_trajectories == full.iters * B
    assert graph_c.chain_trajectories == eager_c.chain_trajectories == sum(sizes)
    assert graph_c.chain_ladders == eager_c.chain_ladders == sum(sizes) * full.L + B
    assert graph_c.ladders == eager_c.ladders


@pytest.mark.parametrize('quantum,chunk', COMPACTIONS)
def test_graphs_are_captured_per_chunk_size_and_dropped_when_the_batch_shrinks(compaction_runs, quantum, chunk):
    """expected values derived from the chunking of the batch sizes the eager trace implies, not measured"""
    from nhmc import sampler
    full, finish, total, get = compaction_runs
    B = RUN3['B']
    eager_c, graph_c = get(quantum, chunk)
    eng = sampler.LeapfrogEngine(lambda x, t: x, None, osched.betas_fp32().to(DEV), SEQ, SEQ_NEXT, torch.device(DEV), chunk=chunk)
    per_size = [{hi - lo for lo, hi in eng._chunks(n)} for n in batch_sizes(finish, B, full.iters, quantum or chunk)]
    assert graph_c.graphs_captured == len(set().union(*per_size)), (graph_c.graphs_captured, per_size)
    assert graph_c.graphs_live_max == max(len(s) for s in per_size), (graph_c.graphs_live_max, per_size)
    assert graph_c.graphs_live_max == {None: 1, 2: 1, 4: 2}[chunk]
    assert eager_c.graphs_captured == eager_c.graphs_live_max == 0


def test_engine_drops_what_a_smaller_batch_cannot_use():
    """`retain_chunks_of`: graph records, persistent g_e buffers and per-chain tables of the sizes that cannot occur go,
    the others stay and still replay the eager bits"""
    B, dim = 5, 16
    op = build_op('inpaint_random', dim, 150)
    g_ = gen(151)
    _, y = observe(op, B, dim, g_)
    x = torch.randn(B, 3, dim, dim, generator=g_).to(DEV)
    net = PointwiseScore().to(DEV)
    eng = engine_for(net, op, 2)
    eng.decode_and_grad(x, y, graph=True)                                           # chunks 2, 2, 1
    assert sorted(k[0][0] for k in eng._graphs) == [1, 2] and sorted(eng._per_n) == [1, 2]
    assert sorted(k[0] for k in eng._ge) == [1, 2]
    eng.retain_chunks_of(4)                                                         # chunks 2, 2
    assert [k[0][0] for k in eng._graphs] == [2] and list(eng._per_n) == [2] and [k[0] for k in eng._ge] == [2]
    want = engine_for(net, op, 2).decode_and_grad(x[:4], y[:4])
    got = eng.decode_and_grad(x[:4], y[:4], graph=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert eng.graphs_captured == 2 and eng.graphs_live_max == 2
    eng.retain_chunks_of(1)
    assert not eng._graphs and not eng._per_n and not eng._ge
    got = eng.decode_and_grad(x[:1], y[:1], graph=True)                             # captured again, alone
    assert all(torch.equal(a, b) for a, b in zip(engine_for(net, op, 2).decode_and_grad(x[:1], y[:1]), got))
    assert eng.graphs_captured == 3 and eng.graphs_live_max == 2 and len(eng._graphs) == 1


# --------------------------------------------------------------------------------------------- #
# 5. the command line
# --------------------------------------------------------------------------------------------- #
def test_cli_runs_with_graph_replay(tmp_path, monkeypatch, capsys):
    """`--graph` end to end on the small config of test_cli_runs_the_reference_command_line: the real U-Net with its fused
    GroupNorm glue inside the capture.  Values are not compared with the eager command line: MIOpen inside a capture may
    round differently."""
    import yaml
    from nhmc import cli, sampler
    cfgdir = tmp_path / 'configs'
    cfgdir.mkdir()
    cfg = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True},
           'model': dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True,
                         class_cond=False, use_checkpoint=False, attention_resolutions='16', num_heads=4,
                         num_head_channels=16, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0.0,
                         resblock_updown=True, use_fp16=False, use_new_attention_order=False, model_path=''),
           'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}
    (cfgdir / 'config_tiny.yml').write_text(yaml.safe_dump(cfg))
    monkeypatch.chdir(tmp_path)
    calls = []
    real = sampler.LeapfrogEngine._graphed_chunk

    def spy(self, x, y, xt_out, loss_out):
        calls.append(x.shape[0])
        return real(self, x, y, xt_out, loss_out)

    monkeypatch.setattr(sampler.LeapfrogEngine, '_graphed_chunk', spy)
    table = cli.main(['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', 'sr4', '--sigma_0', '0.05',
                      '-i', str(tmp_path / 'out'), '--tau', '0.1', '--epsilon', '0.05', '--synthetic', '2', '--chains', '2',
                      '--graph', '--hmc_epochs', '3', '--hmc_sampling', '2', '--philox', '--ni', '--doc', 'ignored'])
    assert len(calls) > 0
    assert table.shape == (2, 3) and bool(torch.isfinite(table).all())
    assert 'Total Average PSNR' in capsys.readouterr().out

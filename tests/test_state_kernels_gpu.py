"""GPU: the per-chain state kernels of the latent and diagonal-mass samplers, each on its own, with several chains.

`nhmc_latent_commit` + `nhmc_schedule_end_latent` and `nhmc_schedule_begin_mass` against the plain restatement of the
reference's bookkeeping (oracle/state_ref.py, validated on the CPU in tests/test_state_model_cpu.py);
`nhmc_leapfrog_mass` against the reference's fp32 tensor expressions op by op; `nhmc_mass_from_variance` against
oracle.mass_ref.mass_from_variance with ties broken by index.

Every comparison of state is exact: the state is int32 and fp64 (`tau * 0.9` is the same IEEE double product in Python
and on the device), the commit kernels move bits, and the leapfrog kernel is built without contraction so that each of
its fp32 operations is one torch operation.  Only the two Hamiltonian sums (a different summation order) are compared
with float64 at 1e-6 relative.
"""
import itertools

import pytest
import torch

from oracle import mass_ref, state_ref

pytestmark = pytest.mark.gpu

KEEP, STEPS, FINAL_FROM, SENTINEL = 3, 14, 5, -7.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def accept_patterns():
    """One accept sequence per branch of main_sampling_latent.py:689-733 (final phase = step >= FINAL_FROM)."""
    rnd = [torch.randint(0, 2, (STEPS,), generator=gen(s)).tolist() for s in (31, 32)]
    return [
        [1] * STEPS,                                            # always: the ring wraps three times
        [0] * STEPS,                                            # never: eps shrinks seven times, nothing is committed
        [1 if s < FINAL_FROM else 0 for s in range(STEPS)],     # annealing phase only: count stays 0
        [0] * 6 + [1, 0, 1, 1, 0, 1, 1, 1],                     # first accept inside the final phase (has_prev == 0 there)
        [s % 2 for s in range(STEPS)],                          # alternating: the reject counter never reaches 2
        [1 if s % 3 == 2 else 0 for s in range(STEPS)],         # reject, reject, accept: eps shrinks, `rejected` resets
        rnd[0], rnd[1],
    ]


def sigma_on_accept(step):
    return 0.45 - 0.02 * step                                   # a different value each step


def latent_state(B, dev):
    from nhmc import sampler
    st = sampler.ChainState(B, 0.3, 0.1, dev)
    tau = [0.3 + 0.01 * c for c in range(B)]                    # per-chain values: a wrong chain index shows
    eps = [0.1 + 0.001 * c for c in range(B)]
    sig = [0.5 + 0.01 * c for c in range(B)]
    for k, v in (('tau', tau), ('eps', eps), ('sigma_y', sig)):
        st.t[k] = torch.tensor(v, dtype=torch.float64, device=dev)
    st.t['count'] = torch.zeros(B, dtype=torch.int32, device=dev)
    st.t['has_prev'] = torch.zeros(B, dtype=torch.int32, device=dev)
    return st, tau, eps, sig


def assert_scalar_state(st, books, step):
    host = {k: st[k].cpu().tolist() for k in ('count', 'has_prev', 'rejected', 'n_accept', 'tau', 'eps', 'sigma_y')}
    want = dict(count=[b.count for b in books], has_prev=[int(b.has_prev) for b in books],
                rejected=[b.rejected for b in books], n_accept=[b.n_accept for b in books],
                tau=[b.tau for b in books], eps=[b.eps for b in books], sigma_y=[b.sigma_y for b in books])
    for k in want:
        assert host[k] == want[k], (step, k, host[k], want[k])


@pytest.mark.parametrize('shape,with_ring', [((8, 3, 20, 20), True), ((8, 4, 24, 24), True), ((8, 3, 20, 20), False)])
def test_latent_commit_and_schedule_end_follow_the_book(shape, with_ring):
    """A scripted 14-step run, commit then schedule end as in hmc_latent_chains, one chain per accept pattern; after every
    step the whole device state equals LatentBook's.  (8, 3, 20, 20) is 300 float4 per chain (a partial tile),
    (8, 4, 24, 24) is 576 (a full 512-float4 tile plus a tail).  with_ring=False: samples=None, everything else as before."""
    import nhmc.kernels as K
    from nhmc import sampler
    dev = torch.device('cuda')
    pats = accept_patterns()
    B = shape[0]
    assert B == len(pats)
    g_ = gen(40)
    x0, xt0 = torch.randn(shape, generator=g_), torch.randn(shape, generator=g_)
    st, tau, eps, sig = latent_state(B, dev)
    books = [state_ref.LatentBook(tau[c], eps[c], sig[c], KEEP, x=x0[c], x_accept=xt0[c]) for c in range(B)]
    x, xt_last = x0.to(dev), xt0.to(dev)
    ring = torch.full((B, KEEP) + shape[1:], SENTINEL, device=dev) if with_ring else None
    for step in range(STEPS):
        final = step >= FINAL_FROM
        x_prop, xt_prop = torch.randn(shape, generator=g_), torch.randn(shape, generator=g_)
        accept = torch.tensor([p[step] for p in pats], dtype=torch.int32, device=dev)
        K.latent_commit(accept, st, final, KEEP, x, x_prop.to(dev), xt_last, xt_prop.to(dev), ring)
        K.schedule_end_latent(accept, st, sigma_on_accept(step), final)
        for c, b in enumerate(books):
            b.step(bool(pats[c][step]), final, sigma_on_accept(step), x_prop[c], xt_prop[c])
        assert_scalar_state(st, books, step)
        xh, xth = x.cpu(), xt_last.cpu()
        for c, b in enumerate(books):
            assert torch.equal(xh[c], b.x) and torch.equal(xth[c], b.x_accept), (step, c)
        if with_ring:
            rh = ring.cpu()
            got = sampler.ring_samples(rh, [b.count for b in books], KEEP)
            for c, b in enumerate(books):
                want = b.samples()
                assert got[c].shape == want.shape and torch.equal(got[c], want), (step, c)
                for slot in set(range(KEEP)) - set(b.written_slots()):
                    assert bool((rh[c, slot] == SENTINEL).all()), (step, c, slot)
    counts = [b.count for b in books]
    assert counts[0] == STEPS - FINAL_FROM and counts[1] == counts[2] == 0 and counts[3] == 5   # the branches were reached
    assert books[1].eps < eps[1] * 0.9 ** 6 and books[5].rejected == 0 and books[5].eps < eps[5]


def test_schedule_end_latent_at_300_chains():
    """The eight patterns tiled to 300 chains: the second block of the one-thread-per-chain kernel."""
    import nhmc.kernels as K
    dev = torch.device('cuda')
    B = 300
    pats = [accept_patterns()[c % 8] for c in range(B)]
    st, tau, eps, sig = latent_state(B, dev)
    books = [state_ref.LatentBook(tau[c], eps[c], sig[c], KEEP) for c in range(B)]
    dummy = torch.zeros(1)
    for step in range(STEPS):
        final = step >= FINAL_FROM
        accept = torch.tensor([p[step] for p in pats], dtype=torch.int32, device=dev)
        K.schedule_end_latent(accept, st, sigma_on_accept(step), final)
        for c, b in enumerate(books):
            b.step(bool(pats[c][step]), final, sigma_on_accept(step), dummy, dummy)
        assert_scalar_state(st, books, step)


def mass_epoch_cases(burn, epochs, sampling):
    total = burn + epochs + 4 * sampling
    return [(0, 1.0), (burn - 1, 1.0), (burn, 1.0), (burn + epochs // 3, 1.0), (burn + epochs // 3 + 1, 1.0),
            (epochs - 1, 1.0), (epochs, 1.0), (epochs, 0.1), (epochs, 0.05), (epochs + 1, 1.0), (total - 1, 1.0),
            (total, 1.0), (total + 5, 1.0)]


@pytest.mark.parametrize('burn,epochs,sampling', [(2, 9, 2), (5, 40, 10)])
def test_schedule_begin_mass_table_at_300_chains(burn, epochs, sampling):
    """Every branch of main_sampling.py:803-816,842 and both sides of each boundary, 300 chains in one call: all six
    outputs equal state_ref.mass_schedule; sigma_y of a chain that takes no branch is untouched."""
    import nhmc.kernels as K
    from nhmc import sampler
    dev = torch.device('cuda')
    B = 300
    cases = mass_epoch_cases(burn, epochs, sampling)
    table = state_ref.mass_sigma_table(0.1, burn, epochs)
    ep = [cases[c % len(cases)][0] for c in range(B)]
    tau = [cases[c % len(cases)][1] for c in range(B)]
    eps = [0.05 + 1e-4 * c for c in range(B)]
    sig = [-1.0 - c for c in range(B)]                          # what an untouched sigma_y must still be
    st = sampler.ChainState(B, 0.0, 0.0, dev)
    st.t['epoch'] = torch.tensor(ep, dtype=torch.int32, device=dev)
    for k, v in (('tau', tau), ('eps', eps), ('sigma_y', sig)):
        st.t[k] = torch.tensor(v, dtype=torch.float64, device=dev)
    st.t['eps_eff'].fill_(-3.0)
    st.t['active'].fill_(-3)
    st.t['welford_on'] = torch.full((B,), -3, dtype=torch.int32, device=dev)
    K.schedule_begin_mass(st, torch.tensor(table, dtype=torch.float64, device=dev), burn, epochs, sampling)
    got = list(zip(*(st[k].cpu().tolist() for k in ('tau', 'eps', 'sigma_y', 'eps_eff', 'active', 'welford_on'))))
    untouched = 0
    for c in range(B):
        want = state_ref.mass_schedule(ep[c], tau[c], eps[c], sig[c], table, burn, epochs, sampling)
        assert got[c] == want, (c, ep[c], got[c], want)
        untouched += want[2] == sig[c]
    assert untouched >= B // len(cases) * 4                     # epochs + 1, total - 1, total, total + 5
    assert st['epoch'].cpu().tolist() == ep


# ---- nhmc_leapfrog_mass ------------------------------------------------------------------------
def col(v):
    """Per-chain Python doubles -> fp32 [B, 1, 1, 1]: the kernel's (float) of the fp64 scalar."""
    return torch.tensor(v, dtype=torch.float64).float().view(-1, 1, 1, 1)


def leapfrog_mass_ref(mode, x, pz, g, g2, inv, std, eps, sig, won, mean, m2, l):
    """main_sampling.py:819,824,829,833,840,843-848,850 in fp32 tensor operations, one per kernel operation.
    -> x, p, mean, m2, Sx, Sp (the sums in float64; None for MID)."""
    import nhmc.kernels as K
    ef, eh = col(eps), col([e / 2.0 for e in eps])
    kf = col([1.0 / (2.0 * (s * s)) for s in sig])
    gv = g + g2 if g2 is not None else g
    Sx = Sp = None
    if mode == K.LF_FIRST:
        p = pz * std
        Sx, Sp = (x * x).double().sum((1, 2, 3)), (inv * (p * p)).double().sum((1, 2, 3))
        p = p - eh * (x + kf * gv)
        return x + (ef * p) * inv, p, mean, m2, Sx, Sp
    G = x + kf * gv
    p = pz - ef * G
    if mode == K.LF_LAST:
        p = p + eh * G
    if won is not None:
        on = torch.tensor(won).bool().view(-1, 1, 1, 1)
        mean_in, m2_in = (torch.zeros_like(x), torch.zeros_like(x)) if l == 0 else (mean, m2)    # :805-806
        delta = x - mean_in
        mean_new = mean_in + delta / (l + 1)
        m2_new = m2_in + delta * (x - mean_new)
        mean, m2 = torch.where(on, mean_new, mean), torch.where(on, m2_new, m2)
    if mode == K.LF_LAST:
        Sx, Sp = (x * x).double().sum((1, 2, 3)), (inv * (p * p)).double().sum((1, 2, 3))
        return x, p, mean, m2, Sx, Sp
    return x + (ef * p) * inv, p, mean, m2, Sx, Sp


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('mode', ['first', 'mid', 'last'])
@pytest.mark.parametrize('shape', [(3, 3, 16, 16), (3, 3, 20, 20), (2, 3, 36, 36), (2, 3, 64, 64)])
def test_leapfrog_mass_bit_for_bit(shape, mode):
    """192 / 300 float4 per chain (part of one tile), 972 (a tile and a tail), 3072 (six full tiles); per-chain eps and
    sigma_y with one chain at eps = 0; with and without the second gradient piece; Welford off, on at l = 0 (mean / m2
    handed in full of a sentinel that must not be read), on at l = 2 (a division by 3) and l = 3, mixed per chain."""
    import nhmc.kernels as K
    dev = torch.device('cuda')
    mode = dict(first=K.LF_FIRST, mid=K.LF_MID, last=K.LF_LAST)[mode]
    B, N = shape[0], shape[1] * shape[2] * shape[3]
    g_ = gen(50 + N % 97)
    x, pz, g, g2, mean0, m20 = (torch.randn(shape, generator=g_) for _ in range(6))
    M = torch.exp(torch.rand(shape, generator=g_) * 2 - 1)
    std, inv = torch.sqrt(M), 1.0 / M
    eps = [0.05, 0.0, 0.05 * 0.95][:B]                          # chain 1 is frozen
    sig = [0.9, 0.37, 0.1][:B]
    mixed = [1, 0, 1][:B] if B == 3 else [0, 1]
    wel_cases = [(None, 0)] if mode == K.LF_FIRST else \
        [(None, 0), ([0] * B, 3), ([1] * B, 0), (mixed, 0), (mixed, 2), (mixed, 3), ([1] * B, 3)]
    tiles = K.leapfrog_tiles(N)
    for has_g2, (won, l) in itertools.product((False, True), wel_cases):
        tag = (has_g2, won, l)
        mean_in = torch.full(shape, 123.0) if (won is not None and l == 0) else mean0
        m2_in = torch.full(shape, 123.0) if (won is not None and l == 0) else m20
        want = leapfrog_mass_ref(mode, x, pz, g, g2 if has_g2 else None, inv, std, eps, sig, won, mean_in, m2_in, l)
        dx, dmean, dm2 = x.to(dev), mean_in.to(dev), m2_in.to(dev)
        ws = torch.full((B * tiles * 2,), -1.0, dtype=torch.float64, device=dev)
        kw = dict(g2=g2.to(dev) if has_g2 else None)
        if won is not None:
            kw.update(welford_on=torch.tensor(won, dtype=torch.int32, device=dev), mean=dmean, m2=dm2, l=l)
        e64, s64 = (torch.tensor(v, dtype=torch.float64, device=dev) for v in (eps, sig))
        if mode == K.LF_FIRST:
            dp = torch.full(shape, 9.0, device=dev)
            K.leapfrog_mass(mode, dx, dp, g.to(dev), inv.to(dev), e64, s64, ws, z=pz.to(dev), std_m=std.to(dev), **kw)
        else:
            dp = pz.to(dev)
            K.leapfrog_mass(mode, dx, dp, g.to(dev), inv.to(dev), e64, s64, ws, **kw)
        assert torch.equal(dx.cpu(), want[0]), tag
        assert torch.equal(dp.cpu(), want[1]), tag
        assert torch.equal(dmean.cpu(), want[2]) and torch.equal(dm2.cpu(), want[3]), tag
        if mode == K.LF_LAST:
            assert torch.equal(want[0], x)                      # LAST leaves the position alone
        else:
            assert torch.equal(want[0][1], x[1]), tag           # eps = 0: the frozen chain did not move
        if mode != K.LF_MID:
            assert rel(K.sum_partials(ws, tiles, B, 2, 0), want[4]) < 1e-6, tag
            assert rel(K.sum_partials(ws, tiles, B, 2, 1), want[5]) < 1e-6, tag
        else:
            assert bool((ws == -1.0).all()), tag                # MID writes no sums


# ---- nhmc_mass_from_variance -------------------------------------------------------------------
def variance_input(shape):
    """Chain 0: random with a run of ties, strided ties and zeros of both signs; chain 1: all zero (the state between
    epochs // 3 and burn + epochs // 3, before Welford runs); chain 2 (if any): random with strided zeros."""
    m2 = torch.rand(shape, generator=gen(60))
    f = m2[0].view(-1)
    f[100:140] = 0.25
    f[7::11] = 0.5
    f[3::13] = 0.0
    f[5::26] = -0.0
    m2[1].zero_()
    if shape[0] > 2:
        m2[2].view(-1)[::7] = 0.0
    return m2


@pytest.mark.parametrize('shape,L,flags', [
    ((3, 3, 20, 20), 5, [1, 1, 0]), ((3, 3, 20, 20), 5, [0, 1, 1]), ((3, 3, 20, 20), 2, [1, 1, 1]),
    ((2, 3, 64, 64), 5, [1, 0]), ((2, 3, 64, 64), 5, [0, 1]),
    ((2, 3, 256, 256), 5, [1, 0]), ((2, 3, 256, 256), 5, [0, 1])])
def test_mass_from_variance_segment_lengths(shape, L, flags):
    """Segments of 1200, 12288 and 196608 (production) keys: the segmented sort takes other paths by segment length.
    Bit for bit against the stable CPU rank transform on the same host tables; unflagged chains untouched."""
    import nhmc.kernels as K
    from nhmc.schedule import mass_tables
    dev = torch.device('cuda')
    N = shape[1] * shape[2] * shape[3]
    m2 = variance_input(shape)
    assert bool(torch.signbit(m2[0]).any()) and float(m2[1].abs().max()) == 0.0
    inv, std = torch.full(shape, 5.0, device=dev), torch.full(shape, 7.0, device=dev)
    K.mass_from_variance(m2.to(dev), L, torch.tensor(flags, dtype=torch.int32, device=dev), inv, std, mass_tables(N, dev))
    inv, std = inv.cpu(), std.cpu()
    for c, flag in enumerate(flags):
        if not flag:
            assert bool((inv[c] == 5.0).all()) and bool((std[c] == 7.0).all()), c
            continue
        # mass_tables evaluates the oracle's own expressions on this host: the same tables on both sides, the same bits
        _, std_ref, inv_ref = mass_ref.mass_from_variance(m2[c], L, stable=True)
        assert torch.equal(std[c].view(-1), std_ref) and torch.equal(inv[c].view(-1), inv_ref), c

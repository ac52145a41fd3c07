"""CPU: the plain restatement of the per-chain bookkeeping (oracle/state_ref.py) against the oracle loops themselves,
before tests/test_state_kernels_gpu.py compares the device state kernels with it."""
import pytest
import torch

from oracle import chain_cases as cc, mass_ref, state_ref


@pytest.mark.parametrize('c', [0, 8])
def test_latent_book_replays_the_latent_oracle(c):
    """LatentBook driven with the oracle's own (accept, proposal, decode) sequence returns the oracle's samples and walks
    through its per-epoch sigma_y / eps, exactly.  Chain 0 collects nothing and shrinks eps; chain 8 wraps the ring."""
    case = cc.latent_chain(c)
    tr, o = case.trace, cc.LATENT_OPT
    epochs, keep = cc.LATENT_EPOCHS, cc.LATENT_SAMPLING
    print(f'latent chain {c}: final-phase accepts {case.final_accepts}, min margin {min(case.margins):.4f}, '
          f'last eps {tr["eps"][-1]:.6f}')
    if c == 0:
        assert case.final_accepts == 0 and min(tr['eps']) < o['epsilon']
    else:
        assert case.final_accepts > keep
    book = state_ref.LatentBook(o['tau'], o['epsilon'], o['sigma_y'], keep, x=case.x[0])
    for epoch, accept in enumerate(tr['accept']):
        assert book.sigma_y == tr['sigma_y'][epoch] and book.eps == tr['eps'][epoch]
        final = epoch >= epochs
        sig = o['sigma_0'] if final else o['sigma_y'] * (o['sigma_0'] / o['sigma_y']) ** (epoch / epochs)
        book.step(accept, final, sig, tr['x_prop'][epoch][0], tr['xt_prop'][epoch][0])
    assert book.count == case.final_accepts and book.n_accept == sum(tr['accept'])
    got = book.samples()
    assert got.shape == case.want.shape and torch.equal(got, case.want)


def test_latent_book_pushes_nothing_at_a_first_accept_inside_the_final_phase():
    book = state_ref.LatentBook(0.3, 0.1, 0.5, 3, x=torch.zeros(4))
    a, b = torch.ones(4), torch.full((4,), 2.0)
    book.step(True, True, 0.1, a, a + 10)
    assert book.count == 0 and book.has_prev and (book.tau, book.eps, book.sigma_y) == (0.1, 0.01, 0.1)
    book.step(True, True, 0.1, b, b + 10)
    assert book.count == 1 and torch.equal(book.samples(), (a + 10)[None]) and torch.equal(book.x, b)
    book.step(False, True, 0.1, a, a)
    book.step(False, True, 0.1, a, a)
    assert (book.tau, book.eps, book.rejected) == (0.1 * 0.9, 0.01 * 0.9, 0) and torch.equal(book.x, b)


@pytest.mark.parametrize('burn,epochs', [(2, 9), (5, 40)])
def test_mass_schedule_sigma_is_the_oracles(burn, epochs):
    sigma_0 = 0.1
    table = state_ref.mass_sigma_table(sigma_0, burn, epochs)
    assert len(table) == epochs + 1 and table[epochs] == sigma_0
    for epoch in range(epochs):
        out = state_ref.mass_schedule(epoch, 0.2, 0.05, -1.0, table, burn, epochs, 2)
        assert out[2] == mass_ref.sigma_y_mass(epoch, sigma_0, burn, epochs)
        assert out[:2] == (0.2, 0.05) and out[3:5] == (0.05, 1)


def test_mass_schedule_hand_derived_rows():
    """burn = 2, epochs = 9, sampling = 2: 19 epochs in all, epochs // 3 == 3.  Rows worked out from
    main_sampling.py:803-816,842 by hand; -1.0 stands for "sigma_y as it came in"."""
    s0, keep = 0.1, -1.0
    table = state_ref.mass_sigma_table(s0, 2, 9)
    rows = [
        # epoch, tau in -> tau, eps, sigma_y, eps_eff, active, welford_on
        (0, 0.2, (0.2, 0.05, s0 + 0.9, 0.05, 1, 0)),
        (1, 0.2, (0.2, 0.05, s0 + 0.9, 0.05, 1, 0)),
        (2, 0.2, (0.2, 0.05, s0 + 0.9 * (1 - 0 / 9) ** 3, 0.05, 1, 0)),
        (5, 0.2, (0.2, 0.05, s0 + 0.9 * (1 - 3 / 9) ** 3, 0.05, 1, 0)),       # 5 - 2 > 3 is false
        (6, 0.2, (0.2, 0.05, s0 + 0.9 * (1 - 4 / 9) ** 3, 0.05, 1, 1)),
        (8, 0.2, (0.2, 0.05, s0 + 0.9 * (1 - 6 / 9) ** 3, 0.05, 1, 1)),
        (9, 1.0, (0.1, 0.01, s0, 0.01, 1, 1)),                                # the clamp fires
        (9, 0.1, (0.1, 0.05, s0, 0.05, 1, 1)),                                # 0.1 > 0.1 is false
        (9, 0.05, (0.05, 0.05, s0, 0.05, 1, 1)),
        (10, 1.0, (1.0, 0.05, keep, 0.05, 1, 1)),                             # no branch: nothing touched
        (18, 1.0, (1.0, 0.05, keep, 0.05, 1, 1)),
        (19, 1.0, (1.0, 0.05, keep, 0.0, 0, 0)),                              # past the loop condition
        (24, 1.0, (1.0, 0.05, keep, 0.0, 0, 0)),
    ]
    for epoch, tau, want in rows:
        assert state_ref.mass_schedule(epoch, tau, 0.05, keep, table, 2, 9, 2) == want, epoch
    # the defaults (5, 40, 10): 85 epochs, epochs // 3 == 13
    table = state_ref.mass_sigma_table(s0, 5, 40)
    assert state_ref.mass_schedule(18, 0.2, 0.05, keep, table, 5, 40, 10)[4:] == (1, 0)
    assert state_ref.mass_schedule(19, 0.2, 0.05, keep, table, 5, 40, 10)[4:] == (1, 1)
    assert state_ref.mass_schedule(40, 0.2, 0.05, keep, table, 5, 40, 10) == (0.1, 0.01, s0, 0.01, 1, 1)
    assert state_ref.mass_schedule(84, 0.2, 0.05, keep, table, 5, 40, 10) == (0.2, 0.05, keep, 0.05, 1, 1)
    assert state_ref.mass_schedule(85, 0.2, 0.05, keep, table, 5, 40, 10) == (0.2, 0.05, keep, 0.0, 0, 0)

"""Oracle: the per-chain bookkeeping of the latent and diagonal-mass samplers (test infrastructure, see oracle/__init__.py).

Plain Python per chain, no kernels: what the device state kernels (`nhmc_latent_commit`, `nhmc_schedule_end_latent`,
`nhmc_schedule_begin_mass`) must leave behind after every outer iteration.  Each rule cites the reference line it
transcribes; tests/test_state_model_cpu.py drives both with the oracle loops' own sequences before anything on the
device is compared with them.
"""
import torch


class LatentBook:
    """One chain of main_sampling_latent.py:691-733, as oracle/latent_ref.py:82-98 states it.

    x         accepted latent position (the reference's `x`)
    x_accept  decode of the last accepted proposal (the project's `xt_last`)
    finals    every latent appended at :709, oldest first; `count == len(finals)`
    has_prev  whether `x_accept` exists yet.  The reference would raise at :709 (`x_accept` unbound) if the first
              accept of a run fell into the final phase; the project defines that case as "nothing is appended".
    """

    def __init__(self, tau, eps, sigma_y, keep, x=None, x_accept=None):
        self.tau, self.eps, self.sigma_y, self.keep = float(tau), float(eps), float(sigma_y), int(keep)
        self.x, self.x_accept = x, x_accept
        self.finals, self.rejected, self.n_accept, self.has_prev = [], 0, 0, False

    @property
    def count(self):
        return len(self.finals)

    def step(self, accept, final_phase, sigma_y_on_accept, x_prop, xt_prop):
        if accept:                                           # :689
            self.n_accept += 1                               # :690
            self.rejected = 0                                # :691
            self.sigma_y = float(sigma_y_on_accept)          # :695 (annealing) or :706 (sigma_0): the caller evaluates it
            if final_phase:                                  # :705, `epoch >= epochs`
                self.tau = 0.1                               # :707
                self.eps = 0.01                              # :708
                if self.has_prev:
                    self.finals.append(self.x_accept)        # :709, BEFORE x_accept is reassigned
            self.x_accept = xt_prop.clone()                  # :713
            self.x = x_prop.clone()                          # :714
            self.has_prev = True
        else:
            self.rejected += 1                               # :727
            if self.rejected >= 2:                           # :728
                self.tau = self.tau * 0.9                    # :729
                self.eps = self.eps * 0.9                    # :731
                self.rejected = 0                            # :732

    def samples(self):
        """:760, the last `keep` appended latents, oldest first ([0, ...] when nothing was appended)."""
        last = self.finals[-self.keep:]
        if not last:
            shape = tuple(self.x.shape) if self.x is not None else ()
            return torch.zeros((0,) + shape)
        return torch.stack(last)

    def written_slots(self):
        """Slots of a `keep`-deep ring (push i lands in slot i % keep) that hold an appended latent."""
        return sorted({i % self.keep for i in range(self.count)})


def mass_sigma_table(sigma_0, burn, epochs):
    """main_sampling.py:808-813 for epoch = 0 .. epochs, in Python floats (entry `epochs` is :813's sigma_0)."""
    table = []
    for epoch in range(epochs):
        if epoch < burn:                                                         # :808
            table.append(sigma_0 + 0.9)                                          # :809
        else:                                                                    # :810
            table.append(sigma_0 + 0.9 * (1 - (epoch - burn) / epochs) ** 3)     # :811
    return table + [sigma_0]                                                     # :813


def mass_schedule(epoch, tau, eps, sigma_y, sigma_table, burn, epochs, sampling):
    """Top of one outer iteration of main_sampling.py:803-816 and the Welford switch of :842, as oracle/mass_ref.py:51-61,73
    states them, for one chain -> (tau, eps, sigma_y, eps_eff, active, welford_on).

    `active` is the loop condition of :803; a chain past it is frozen by the project (eps_eff = 0, nothing else
    touched) while the other chains of the batch go on."""
    active = epoch < burn + epochs + 4 * sampling                                # :803
    if active:
        if epoch < burn:                                                         # :808
            sigma_y = sigma_table[epoch]
        elif epoch < epochs:                                                     # :810
            sigma_y = sigma_table[epoch]
        elif epoch == epochs:                                                    # :812
            sigma_y = sigma_table[epochs]                                        # :813
            if tau > 0.1:                                                        # :814
                tau = 0.1                                                        # :815
                eps = 0.01                                                       # :816
    welford_on = active and (epoch - burn) > epochs // 3                         # :842
    return tau, eps, sigma_y, (eps if active else 0.0), int(active), int(welford_on)

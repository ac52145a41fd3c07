"""operators.ObservationCache: the one policy behind the cached observation forms of Deblurring2D, WalshHadamardCS and
SRConv.  Plain Python over tensors, so CPU tensors show all of it but the capture bypass (tests/test_obs_cache_gpu.py)."""
import torch

import nhmc  # noqa: F401
from nhmc.operators import ObservationCache


class Doubler:
    def __init__(self):
        self.calls = 0

    def __call__(self, t):
        self.calls += 1
        return t.clone() * 2


def test_hit_returns_the_same_object():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0).reshape(2, 3)
    a = cache.get(y, make)
    b = cache.get(y, make)
    assert make.calls == 1 and a is b and len(cache) == 1 and torch.equal(a, y * 2)


def test_an_in_place_write_misses():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0).reshape(2, 3)
    cache.get(y, make)
    y.add_(1)
    b = cache.get(y, make)
    assert make.calls == 2 and torch.equal(b, (torch.arange(6.0).reshape(2, 3) + 1) * 2)


def test_same_storage_under_another_shape_is_another_entry():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0).reshape(2, 3)
    v = y.view(3, 2)
    assert v.data_ptr() == y.data_ptr() and v._version == y._version
    a, b = cache.get(y, make), cache.get(v, make)
    assert make.calls == 2 and len(cache) == 2 and a.shape == (2, 3) and b.shape == (3, 2)
    assert cache.get(y, make) is a and cache.get(v, make) is b and make.calls == 2


def test_kind_is_part_of_the_key():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0).reshape(2, 3)
    a, b = cache.get(y, make, 'projected'), cache.get(y, make, 'transposed')
    assert make.calls == 2 and len(cache) == 2 and a is not b
    assert cache.get(y, make, 'projected') is a and make.calls == 2


def test_a_non_contiguous_observation_is_computed_and_never_stored():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0).reshape(2, 3)
    cache.get(y, make)
    n0 = len(cache)
    yt = y.t()
    assert not yt.is_contiguous()
    a, b = cache.get(yt, make), cache.get(yt, make)
    assert make.calls == 3 and a is not b and torch.equal(a, yt * 2) and len(cache) == n0


def test_the_oldest_of_sixteen_entries_is_evicted():
    cache, make = ObservationCache(), Doubler()
    ys = [torch.full((4,), float(i)) for i in range(17)]
    outs = [cache.get(y, make) for y in ys]
    assert len(cache) == 16 and make.calls == 17
    assert cache.get(ys[16], make) is outs[16] and make.calls == 17           # the 17th is a hit
    again = cache.get(ys[0], make)                                             # the first was evicted: recomputed
    assert make.calls == 18 and again is not outs[0] and torch.equal(again, outs[0]) and len(cache) == 16
    assert cache.get(ys[16], make) is outs[16] and make.calls == 18


def test_an_entry_pins_its_storage():
    """The key holds an address: while the entry lives no other tensor may be given that address."""
    cache, make = ObservationCache(), Doubler()
    y = torch.zeros(1024)
    ptr = y.data_ptr()
    cache.get(y, make)
    del y
    fresh = [torch.empty(1024) for _ in range(64)]
    assert all(t.data_ptr() != ptr for t in fresh) and len(cache) == 1


def test_clear_empties_it():
    cache, make = ObservationCache(), Doubler()
    y = torch.arange(6.0)
    cache.get(y, make)
    cache.clear()
    assert len(cache) == 0
    cache.get(y, make)
    assert make.calls == 2 and len(cache) == 1

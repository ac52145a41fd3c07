"""CPU: the granule swizzle of the Winograd convolution's LDS operands (csrc/wino_conv.hip), enumerated against the two
banking rules of the LDS that matter to it.

An operand row (a channel's K row of U, or a tile's row of V) is 16 floats = 64 bytes = four 16-byte granules; granule g of
row R is kept at granule g ^ s(R).

  read   ds_read_b128: a wave is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same
         + 32; bank of byte address a = (a / 4) mod 64.  Lane l reads one granule, the same g in every lane, of row base + l
         (base a multiple of 32).
  store  ds_write_b128: groups of 8 contiguous lanes, bank = (a / 4) mod 32.  V: lane l stores one granule, the same g in
         every lane, of row base + l.  U: lane l stores granule l % 4 of row base + l / 4.

A group is free of conflicts when its lanes' 4-bank spans are disjoint.  The swizzle of the kernel,
s(R) = ((R >> 1) & 3) ^ (3 if R & 8 else 0), is free on all three; the earlier one, (R >> 2) & 3, was built for the read and
puts rows R and R + 2 of a V store on the same four banks."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

new = lambda r: ((r >> 1) & 3) ^ (3 if (r >> 3) & 1 else 0)
old = lambda r: (r >> 2) & 3

READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS[:2]]
STORE_GROUPS = [list(range(8 * i, 8 * i + 8)) for i in range(8)]


def worst(groups, banks, row_of_lane, granule_of_lane, s):
    """The largest number of distinct addresses that meet on one bank within one lane group."""
    most = 0
    for group in groups:
        hits = {}
        for lane in group:
            row = row_of_lane(lane)
            byte = 64 * row + 16 * (granule_of_lane(lane) ^ s(row))
            for dword in range(4):
                hits.setdefault((byte // 4 + dword) % banks, set()).add(byte)
        most = max(most, max(len(v) for v in hits.values()))
    return most


def read_ways(s):
    return max(worst(READ_GROUPS, 64, lambda l: base + l, lambda l: g, s) for base in (0, 32, 64, 96) for g in range(4))


def v_store_ways(s):
    return max(worst(STORE_GROUPS, 32, lambda l: base + l, lambda l: g, s) for base in (0, 64) for g in range(4))


def u_store_ways(s):
    return max(worst(STORE_GROUPS, 32, lambda l: base + l // 4, lambda l: l % 4, s) for base in (0, 16, 32, 48))


def test_the_new_swizzle_is_conflict_free_on_the_read_and_on_both_stores():
    assert read_ways(new) == 1
    assert v_store_ways(new) == 1
    assert u_store_ways(new) == 1


def test_the_earlier_swizzle_reads_clean_and_stores_v_with_a_two_way_conflict():
    assert read_ways(old) == 1
    assert u_store_ways(old) == 1
    assert v_store_ways(old) == 2


def test_no_swizzle_conflicts_four_ways_on_the_read():
    assert read_ways(lambda r: 0) == 4


def test_the_new_swizzle_is_the_stated_linear_map():
    """Row bit 1 -> granule bit 0, bit 2 -> bit 1, bit 3 -> both; bits 0, 4 and above do not enter."""
    assert [new(1 << b) for b in range(8)] == [0, 1, 2, 3, 0, 0, 0, 0]
    for r in range(256):
        for q in range(256):
            assert new(r ^ q) == new(r) ^ new(q)


@pytest.mark.parametrize('site', ['uw', 'vswz', 'swz'])
def test_the_kernel_source_uses_one_swizzle_function_at_every_site(site):
    src = open(os.path.join(ROOT, 'noise-space-hmc_amd', 'csrc', 'wino_conv.hip')).read()
    line = next(l for l in src.splitlines() if re.search(r'\bconst int ' + site + r'\b', l) or re.search(r',\s*' + site + r'\s*=', l))
    assert 'wc_swz(' in line, line

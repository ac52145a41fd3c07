"""CPU: the index map of the eight-wave Winograd kernel's epilogue exchange (csrc/wino_conv.hip, k_conv3x3_wino8), restated
from the kernel's constants and enumerated.

Wave w = 4 fh + 2 th + kh holds frequencies 8 fh + j, j = 0 .. 7, of accumulator registers r = 0 .. 15 of its lane.  The
output transform of register r (a channel row) runs in wave fh = r >> 3 of the pair (w, w ^ 4), so wave fh sends registers
8 (1 - fh) .. + 7 of each of its frequencies and keeps the others.  The float4 (j, q) = registers 8 (1 - fh) + 4 q .. + 3 of
frequency j is written at float4 index (16 w + 2 j + q) * 64 + lane and read by the same lane of wave w ^ 4.

  write  ds_write_b128: groups of 8 contiguous lanes, bank = (a / 4) mod 32
  read   ds_read_b128: four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; bank =
         (a / 4) mod 64   (the rules tests/test_wino_swizzle_cpu.py enumerates for the operands)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'noise-space-hmc_amd', 'csrc', 'wino_conv.hip')).read()

WAVES, LANES, XSLOTS = 8, 64, 16
LDS_WORDS = 4 * 16 * 8 * 64                       # WC_LDS_BYTES / 4: two stages of U + V

READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS += [[l + 32 for l in g] for g in READ_GROUPS[:2]]
STORE_GROUPS = [list(range(8 * i, 8 * i + 8)) for i in range(8)]


def slot(wave, lane, j, q):
    """float4 index a wave writes for (frequency j of its half, register quad q of the half it sends)."""
    return (wave * XSLOTS + 2 * j + q) * LANES + lane


def word_written(wave, lane, f, r):
    """LDS word of M_f[r] of the lane, sent by the wave that holds frequency f; None if that wave keeps register r."""
    fh = wave >> 2
    if f >> 3 != fh or r >> 3 == fh:
        return None
    return 4 * slot(wave, lane, f & 7, (r & 7) >> 2) + (r & 3)


def word_read(wave, lane, f, r):
    """LDS word from which the wave takes M_f[r]: a frequency of its partner's half, a register of its own."""
    fh = wave >> 2
    if f >> 3 == fh or r >> 3 != fh:
        return None
    return 4 * slot(wave ^ 4, lane, f & 7, (r & 7) >> 2) + (r & 3)


def test_the_source_holds_the_constants_restated_here():
    assert re.search(r'constexpr int WC8_XSLOTS = 16;', SRC)
    assert re.search(r'constexpr int WC_LDS_BYTES = 4 \* WC_OPER \* 4;', SRC) and re.search(r'WC_OPER = 16 \* WC_CHUNK \* 64;', SRC)
    assert 'xw = wave * WC8_XSLOTS * 64 + lane, xr = (wave ^ 4) * WC8_XSLOTS * 64 + lane' in SRC
    assert 'xch[xw + (2 * j + q) * 64] = ' in SRC and 'got[j][q] = xch[xr + (2 * j + q) * 64]' in SRC
    assert 'constexpr int RS = decltype(half)::value ? 0 : 8;' in SRC          # the registers sent
    assert 'constexpr int F = decltype(half)::value, RK = 8 * F;' in SRC        # the registers kept
    assert '__launch_bounds__(512, 2) void k_conv3x3_wino8' in SRC


def test_the_writes_are_a_bijection_onto_the_128_kb():
    words = [word_written(w, l, f, r) for w in range(WAVES) for l in range(LANES) for f in range(16) for r in range(16)]
    words = [x for x in words if x is not None]
    assert len(words) == LDS_WORDS == 128 * 1024 // 4
    assert sorted(words) == list(range(LDS_WORDS))


def test_every_pair_a_wave_needs_arrives_exactly_once():
    """What wave w reads for (f, r) is what its partner, same lane, wrote for (f, r); with its own 8 x 8 kept values the lane
    has all 16 frequencies of its 8 registers, each once."""
    for w in range(WAVES):
        fh = w >> 2
        for l in (0, 1, 31, 32, 63):
            have = {}
            for f in range(16):
                for r in range(16):
                    if f >> 3 == fh and r >> 3 == fh:
                        have[(f, r)] = have.get((f, r), 0) + 1               # kept in registers
                    rd = word_read(w, l, f, r)
                    if rd is not None:
                        assert rd == word_written(w ^ 4, l, f, r)
                        have[(f, r)] = have.get((f, r), 0) + 1
            assert have == {(f, 8 * fh + rr): 1 for f in range(16) for rr in range(8)}


def test_no_wave_reads_a_word_another_pair_wrote():
    for w in range(WAVES):
        mine = {word_read(w, l, f, r) for l in range(LANES) for f in range(16) for r in range(16)} - {None}
        theirs = {word_written(w ^ 4, l, f, r) for l in range(LANES) for f in range(16) for r in range(16)} - {None}
        assert mine == theirs and len(mine) == XSLOTS * LANES * 4


def ways(groups, banks, wave):
    """The largest number of distinct 16-byte slots that meet on one bank within one lane group of one b128 instruction."""
    most = 0
    for j in range(8):
        for q in range(2):
            for group in groups:
                hits = {}
                for lane in group:
                    byte = 16 * slot(wave, lane, j, q)
                    for dword in range(4):
                        hits.setdefault((byte // 4 + dword) % banks, set()).add(byte)
                assert len({16 * slot(wave, lane, j, q) for lane in group}) == len(group)      # distinct slots
                most = max(most, max(len(v) for v in hits.values()))
    return most


def test_the_b128_lane_groups_are_free_of_bank_conflicts():
    for w in range(WAVES):
        assert ways(STORE_GROUPS, 32, w) == 1
        assert ways(READ_GROUPS, 64, w ^ 4) == 1

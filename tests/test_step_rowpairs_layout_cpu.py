"""The row-pair LDS image of the accepted point and the fixed accept block of the headline step kernels
(XLayout and AcceptBlock of csrc/smcmc_step_deal.h), DP = 50.

tests/cpp/step_rowpairs_layout.C (plain g++, no HIP) prints the byte address of every (row, lane), the addresses of the
moment fold's operand reads formed as step_kernel forms them, and the accept block of every family.  LDS has 64 banks of
four bytes; a ds_read_b64 is served a half-wave at a time, a 16-byte access a quarter-wave at a time.  Lanes that read
the same address are one broadcast access, so what must hold is that DIFFERENT addresses of a half-wave share no bank;
where the 32 addresses are all different (the tile rows below the ones row's tile) that is 64 distinct banks.  The tile
row of the ones row and the strip read clamp the rows past the ones row onto it: fewer addresses, still no shared bank."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, BANKS = 50, 64


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_rowpairs") / "step_rowpairs_layout.exe")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'root-simple-mcmc_amd', 'csrc')}",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", "step_rowpairs_layout.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {"slot": {}, "operand": {}, "unclamped": {}, "strip": {}, "accept": {}, "word": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "layout":
            out["layout"] = dict(zip(("DP", "ROWS", "HELD", "BYTES", "PAIR_STRIDE", "LANE"), v))
        elif w[0] == "slot":
            out["slot"][(v[0], v[1])] = v[2]
        elif w[0] in ("operand", "unclamped"):
            out[w[0]].setdefault((v[0], v[1]), {})[v[2]] = v[3]
        elif w[0] == "strip":
            out["strip"].setdefault(v[0], {})[v[1]] = v[2]
        elif w[0] == "plain":
            out["plain"] = v
        elif w[0] == "accept":
            out["accept"][v[0]] = {"fixed": bool(v[1]), "block": v[2], "lowest": v[3]}
        else:
            assert w[0] == "word"
            out["word"][v[0]] = (v[1], v[2])
    return out


def _banks(address, nbytes):
    assert address % 4 == 0
    return {(address // 4 + k) % BANKS for k in range(nbytes // 4)}


def test_every_row_and_lane_has_a_slot_of_its_own(printed):
    lay, slot = printed["layout"], printed["slot"]
    assert lay == {"DP": DP, "ROWS": DP + 1, "HELD": DP + 2, "BYTES": 26 * (64 * 16 + 32), "PAIR_STRIDE": 64 * 16 + 32, "LANE": 2}
    assert sorted(slot) == [(r, c) for r in range(DP + 2) for c in range(64)]
    for (r, c), a in slot.items():
        assert a == (r >> 1) * lay["PAIR_STRIDE"] + c * 16 + (r & 1) * 8, (r, c)
        assert a % 8 == 0 and 0 <= a and a + 8 <= lay["BYTES"], (r, c)
    assert len(set(slot.values())) == len(slot)
    # four workgroups per CU: the image, the decomposition's (50 x 50 triangular, rows padded to even: 1 300 doubles) and
    # the normal transform's tables (384 doubles) within a quarter of the 160 KB
    assert lay["BYTES"] + 8 * (1300 + 384) <= 40960
    # the largest immediate offset of a lane's 16-byte accesses stays inside the 16-bit field
    assert max(slot[(r, 0)] for r in range(DP)) < 1 << 16


def test_other_instantiations_keep_rows_of_66_doubles(printed):
    v = printed["plain"]
    assert v[:3] == [DP, DP + 1, (DP + 1) * 66 * 8]
    triples = [v[3 + 3 * k: 6 + 3 * k] for k in range((len(v) - 3) // 3)]
    assert len(triples) == 12
    for r, c, a in triples:
        assert a == 8 * (r * 66 + c)


def _assert_no_shared_bank(addresses, what, full):
    """addresses: lane -> byte address of a ds_read_b64, one half-wave."""
    distinct = sorted(set(addresses.values()))
    banks = [b for a in distinct for b in _banks(a, 8)]
    assert len(set(banks)) == len(banks) == 2 * len(distinct), what
    if full:
        assert len(distinct) == 32 and len(set(banks)) == BANKS, what


def test_operand_reads_are_conflict_free(printed):
    lay = printed["layout"]
    tiles = sorted({t for t, _ in printed["operand"]})
    assert tiles == [0, 1, 2, 3]
    for (t, kk), lanes in sorted(printed["operand"].items()):
        assert sorted(lanes) == list(range(64))
        assert all(a + 8 <= lay["BYTES"] for a in lanes.values()), (t, kk)
        for half in (0, 1):
            hw = {lane: lanes[lane] for lane in range(32 * half, 32 * half + 32)}
            # tile rows 0-2 hold rows 0 .. 47, all of them live: 32 different addresses; tile row 3 holds 48, 49, the
            # ones row and thirteen rows clamped onto it
            _assert_no_shared_bank(hw, f"tile row {t}, k-quad {kk}, half-wave {half}", full=t < 3)
    # the layout's formula alone, rows 16 t + (lane & 15) as they stand: 32 addresses, 64 banks, for every tile row
    assert sorted(printed["unclamped"]) == sorted(printed["operand"])
    for (t, kk), lanes in sorted(printed["unclamped"].items()):
        for half in (0, 1):
            hw = {lane: lanes[lane] for lane in range(32 * half, 32 * half + 32)}
            _assert_no_shared_bank(hw, f"unclamped tile row {t}, k-quad {kk}, half-wave {half}", full=True)
    # the strip read: rows 48 + (lane & 3), chains 4 kk + (lane >> 4) -- eight (row, chain) pairs per half-wave at the most
    assert sorted(printed["strip"]) == list(range(16))
    for kk, lanes in sorted(printed["strip"].items()):
        assert all(a + 8 <= lay["BYTES"] for a in lanes.values()), kk
        for half in (0, 1):
            hw = {lane: lanes[lane] for lane in range(32 * half, 32 * half + 32)}
            _assert_no_shared_bank(hw, f"strip, k-quad {kk}, half-wave {half}", full=False)


def test_operand_reads_address_the_rows_they_fold(printed):
    """The read of tile row t, k-quad kk by lane l is the slot of row min(16 t + (l & 15), DP), chain 4 kk + (l >> 4)."""
    slot = printed["slot"]
    for (t, kk), lanes in printed["operand"].items():
        for lane, a in lanes.items():
            assert a == slot[(min(16 * t + (lane & 15), DP), 4 * kk + (lane >> 4))]
    for kk, lanes in printed["strip"].items():
        for lane, a in lanes.items():
            assert a == slot[(min(48 + (lane & 3), DP), 4 * kk + (lane >> 4))]


# the lane groups a 16-byte read is served in, one LDS cycle each: sixteen lanes, not the contiguous quarters
READ_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
                    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
                    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def test_a_quarter_wave_of_column_accesses_covers_the_banks_once(printed):
    """A lane = chain 16-byte access of a row pair: every sixteen lanes served together -- the contiguous quarters and
    the groups the hardware forms for ds_read_b128 -- cover the 64 banks exactly once; a 16-byte write goes eight
    contiguous lanes at a time over 32 banks, once each."""
    slot = printed["slot"]
    assert sorted(c for g in READ_B128_GROUPS for c in g) == list(range(64))
    quarters = [list(range(16 * q, 16 * q + 16)) for q in range(4)]
    for pair in range((DP + 2) // 2):
        for group in quarters + READ_B128_GROUPS:
            banks = []
            for c in group:
                a = slot[(2 * pair, c)]
                assert a % 16 == 0 and slot[(2 * pair + 1, c)] == a + 8
                banks += sorted(_banks(a, 16))
            assert sorted(banks) == list(range(BANKS)), (pair, group)
        for eighth in range(8):
            banks = [(slot[(2 * pair, c)] // 4 + k) % 32 for c in range(8 * eighth, 8 * eighth + 8) for k in range(4)]
            assert sorted(banks) == list(range(32)), (pair, eighth)


def test_accept_block_is_fixed_for_the_50_family_alone(printed):
    for d, (restated, detmath) in printed["word"].items():
        assert restated == detmath == 2 * ((d + 1) // 2), d
    acc = printed["accept"]
    assert sorted(acc) == [7, 15, 31, 47, 50, 63]
    assert [acc[dp]["lowest"] for dp in sorted(acc)] == [1, 8, 16, 32, 48, 51]
    assert acc[50]["fixed"] and acc[50]["block"] == 12
    for dp in (7, 15, 31, 47, 63):
        assert not acc[dp]["fixed"], dp
    assert [printed["word"][d][0] >> 2 for d in (48, 49, 50)] == [12, 12, 12]
    assert [printed["word"][d][0] & 3 for d in (48, 49, 50)] == [0, 2, 2]

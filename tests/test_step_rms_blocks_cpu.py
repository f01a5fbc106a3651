"""The fold rows that read the zero row (XLayout::ZERO_ROW of csrc/smcmc_step_deal.h, ZROW of step_kernel), DP = 50.

With the moment fold the row-pair image of the accepted point holds, next to the ones row DP, a row DP + 1 that is +0 in
every lane.  The headline kernel's operand reads of the tile rows past the ones row go there instead of being clamped
onto the ones row and zeroed by a select.  tests/cpp/step_zero_row.C (plain g++, no HIP) prints the byte addresses of
those reads as step_kernel forms them.  LDS has 64 banks of four bytes and serves a ds_read_b64 a half-wave (32 lanes) at
a time: lanes that read the same address are one broadcast, so what must hold is that DIFFERENT addresses of a half-wave
share no bank -- the bank of byte address a is (a / 4) % 64.

(The other half of the change this file was named for, the StepRMS terms taken block by block, was built and measured
and is not in the kernels: profiles/step_rms_blocks_notes.md.  Its plan and the checks of it went with it.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, BANKS, PAIR_STRIDE = 50, 64, 64 * 16 + 32


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_zero_row") / "step_zero_row.exe")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'root-simple-mcmc_amd', 'csrc')}",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", "step_zero_row.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {"slot": {}, "zoperand": {}, "zstrip": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "zero":
            out["zero"] = dict(zip(("ZERO_ROW", "ROWS", "HELD", "BYTES", "PAIR_STRIDE"), v))
        elif w[0] == "slot":
            out["slot"][(v[0], v[1])] = v[2]
        elif w[0] == "zoperand":
            out["zoperand"].setdefault((v[0], v[1]), {})[v[2]] = v[3]
        else:
            assert w[0] == "zstrip", line
            out["zstrip"].setdefault(v[0], {})[v[1]] = v[2]
    return out


def _address(r, c):
    return (r >> 1) * PAIR_STRIDE + 16 * c + 8 * (r & 1)


def test_zero_row_lies_inside_the_declared_image(printed):
    z = printed["zero"]
    assert z == {"ZERO_ROW": DP + 1, "ROWS": DP + 1, "HELD": DP + 2, "BYTES": 26 * PAIR_STRIDE, "PAIR_STRIDE": PAIR_STRIDE}
    for c in range(64):
        ones, zero = printed["slot"][(DP, c)], printed["slot"][(DP + 1, c)]
        # the ones row's partner: the second half of the 16 bytes the prologue writes as (1 or 0, +0) in every lane
        assert ones % 16 == 0 and zero == ones + 8 and zero + 8 <= z["BYTES"], c
    # the size of the launch's one round does not move: image, decomposition (1 300 doubles) and tables (384) in 40 960 bytes
    assert z["BYTES"] + 8 * (1300 + 384) <= 40960


def test_operand_reads_address_the_rows_they_fold_or_the_zero_row(printed):
    z = printed["zero"]
    assert sorted(printed["zoperand"]) == [(t, kk) for t in range(4) for kk in range(16)]
    assert sorted(printed["zstrip"]) == list(range(16))
    for (t, kk), lanes in printed["zoperand"].items():
        assert sorted(lanes) == list(range(64))
        for lane, a in lanes.items():
            r = 16 * t + (lane & 15)
            assert a == _address(r if r <= DP else z["ZERO_ROW"], 4 * kk + (lane >> 4)), (t, kk, lane)
            assert 0 <= a and a + 8 <= z["BYTES"], (t, kk, lane)
    for kk, lanes in printed["zstrip"].items():
        assert sorted(lanes) == list(range(64))
        for lane, a in lanes.items():
            r = 48 + (lane & 3)
            assert a == _address(r if r <= DP else z["ZERO_ROW"], 4 * kk + (lane >> 4)), (kk, lane)
            assert 0 <= a and a + 8 <= z["BYTES"], (kk, lane)
    # no read of a row past the ones row lands on the ones row any more, and none of a live row on the zero row
    zero_slots = {printed["slot"][(DP + 1, c)] for c in range(64)}
    for (t, kk), lanes in printed["zoperand"].items():
        for lane, a in lanes.items():
            assert (a in zero_slots) == (16 * t + (lane & 15) > DP), (t, kk, lane)


def _assert_half_waves(lanes, what):
    for half in (0, 1):
        distinct = sorted({lanes[lane] for lane in range(32 * half, 32 * half + 32)})
        banks = []
        for a in distinct:
            assert a % 4 == 0
            banks += [(a // 4) % BANKS, (a // 4 + 1) % BANKS]   # ds_read_b64: two banks
        # equal addresses are one broadcast; different ones share no bank
        assert len(set(banks)) == len(banks) == 2 * len(distinct), f"{what}, half-wave {half}"
    return len({lanes[lane] for lane in range(32)})


def test_zero_row_operand_reads_are_conflict_free(printed):
    for (t, kk), lanes in sorted(printed["zoperand"].items()):
        n = _assert_half_waves(lanes, f"tile row {t}, k-quad {kk}")
        # tile rows 0-2: 32 addresses on 64 banks; tile row 3: rows 48, 49, the ones row and the zero row of two chains
        assert n == (32 if t < 3 else 8), (t, kk)
    for kk, lanes in sorted(printed["zstrip"].items()):
        assert _assert_half_waves(lanes, f"strip, k-quad {kk}") == 8, kk

"""The LDS of the headline step kernels' workgroup (StepWorkgroupLds of csrc/smcmc_step_deal.h): four wavefronts, each
with an image of the accepted point of its own, one decomposition, and the two tables of the normal transform in copies
(NormalTableLayout) placed so that a gather -- ds_read_b128 at an index that differs from lane to lane and comes from a
random word -- cannot conflict.

tests/cpp/step_shared_tables.C (plain g++, no HIP) prints the byte offsets of the parts, every lane's part of a gather's
address, every (copy, entry) slot and what the prologue stages into it, and the wavefront-to-group mapping.  LDS has 64
banks of four bytes, bank (address / 4) % 64; a 16-byte read is served sixteen lanes at a time: the lane groups are those
of tests/test_step_rowpairs_layout_cpu.py, the contiguous quarters and the groups the hardware forms.  Lanes that read
the same address are one broadcast access.  What must hold, for ANY indices: in the table with sixteen copies the lanes
served together share no bank unless they read the same address; in the table with eight copies a bank is asked for by
two different addresses at the most."""
import os
import subprocess

import numpy as np
import pytest

from test_step_rowpairs_layout_cpu import READ_B128_GROUPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANKS, LDS_PER_CU = 64, 163840
QUARTERS = [list(range(16 * q, 16 * q + 16)) for q in range(4)]
GROUPS = QUARTERS + READ_B128_GROUPS
ENTRIES = {"log": 64, "angle": 128}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_shared_tables") / "step_shared_tables.exe")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'root-simple-mcmc_amd', 'csrc')}",
           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "cpp", "step_shared_tables.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {"lds": {}, "image": {}, "table": {}, "lane": {}, "entry": {}, "slot": {}, "group": {}, "blocks": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] in ("table", "lane", "entry", "slot"):
            name, v = w[1], [int(x) for x in w[2:]]
            if w[0] == "table":
                out["table"][name] = dict(zip(("entries", "copies", "stride", "shift", "bytes", "slots"), v))
            elif w[0] == "lane":
                out["lane"].setdefault(name, {})[v[0]] = v[1]
            elif w[0] == "entry":
                out["entry"].setdefault(name, {})[(v[0], v[1])] = v[2]
            else:
                out["slot"].setdefault(name, {})[v[0]] = (v[1], v[2])
            continue
        v = [int(x) for x in w[1:]]
        if w[0] == "lds":
            out["lds"][v[1]] = dict(zip(("DP", "MOMENTS", "IMAGE_BYTES", "US", "US_BYTES", "LOG", "LOG_BYTES", "ANGLE",
                                         "ANGLE_BYTES", "TOTAL", "LIMIT"), v))
        elif w[0] == "image":
            out["image"][(v[1], v[2])] = v[3]
        elif w[0] == "group":
            out["group"][(v[0], v[1])] = v[2]
        else:
            assert w[0] == "blocks"
            out["blocks"][v[0]] = v[1]
    return out


def test_parts_are_disjoint_aligned_and_fit_the_cu(printed):
    assert sorted(printed["lds"]) == [0, 1]
    for moments, lds in printed["lds"].items():
        assert lds["DP"] == 50 and lds["LIMIT"] == LDS_PER_CU
        pairs = 26 if moments else 25                     # row pairs of the image: 50 rows, and the ones row with its partner
        assert lds["IMAGE_BYTES"] == pairs * (64 * 16 + 32)
        assert lds["US_BYTES"] == 8 * 1300                # 50 x 50 triangular, rows padded to even
        assert lds["LOG_BYTES"] == printed["table"]["log"]["bytes"] and lds["ANGLE_BYTES"] == printed["table"]["angle"]["bytes"]
        parts = [(printed["image"][(moments, w)], lds["IMAGE_BYTES"]) for w in range(4)]
        parts += [(lds["US"], lds["US_BYTES"]), (lds["LOG"], lds["LOG_BYTES"]), (lds["ANGLE"], lds["ANGLE_BYTES"])]
        assert all(start % 16 == 0 and size % 16 == 0 and size > 0 for start, size in parts)
        parts.sort()
        assert parts[0][0] == 0
        for (a, n), (b, _) in zip(parts, parts[1:]):
            assert a + n <= b, "two parts overlap"
        assert parts[-1][0] + parts[-1][1] == lds["TOTAL"] <= LDS_PER_CU
    # the split is one that exists: sixteen copies of both tables do not fit beside four images and the decomposition
    assert 4 * 26 * (64 * 16 + 32) + 8 * 1300 + 16 * 16 * (64 + 128) > LDS_PER_CU


def _addresses(printed, name, lanes, index):
    t = printed["table"][name]
    return {lane: printed["lane"][name][lane] + (int(index[lane]) << t["shift"]) for lane in lanes}


def _worst_bank(addresses):
    """The most different addresses that ask for one bank (1: conflict-free)."""
    asked = {}
    for a in set(addresses.values()):
        assert a % 16 == 0
        for k in range(4):
            asked.setdefault((a // 4 + k) % BANKS, set()).add(a)
    return max(len(s) for s in asked.values())


def _index_vectors(entries):
    rng = np.random.default_rng(20251021)
    yield "all equal", np.full(64, entries - 1)
    yield "all equal, entry 0", np.zeros(64, dtype=int)
    yield "all different", np.arange(64) % entries
    yield "all different, sixteen apart", (np.arange(64) * 16) % entries
    yield "all different, descending", (entries - 1 - np.arange(64)) % entries
    for n in range(3000):
        yield f"random {n}", rng.integers(0, entries, 64)
    for n in range(200):   # few different entries: many lanes of a group on one of two or three
        yield f"random, few entries {n}", rng.choice(rng.integers(0, entries, 3), 64)


@pytest.mark.parametrize("name", ["log", "angle"])
def test_gathers_do_not_conflict_whatever_the_indices(printed, name):
    t = printed["table"][name]
    assert t["entries"] == ENTRIES[name] and t["stride"] == 16 * t["copies"] == 1 << t["shift"]
    copies = sorted(printed["table"][n]["copies"] for n in ENTRIES)
    assert copies[1] == 16 and copies[0] >= 8, "one table cannot conflict at all, the other two-way at the most"
    limit = 1 if t["copies"] == 16 else 2
    assert sorted(c for g in READ_B128_GROUPS for c in g) == list(range(64))
    worst = 0
    for what, index in _index_vectors(t["entries"]):
        for group in GROUPS:
            a = _addresses(printed, name, group, index)
            assert all(0 <= v and v + 16 <= t["bytes"] for v in a.values()), what
            w = _worst_bank(a)
            assert w <= limit, (name, what, group)
            worst = max(worst, w)
    assert worst == limit   # (eight copies: the bound is reached, the test can tell two-way from none)


@pytest.mark.parametrize("name", ["log", "angle"])
def test_one_copy_would_conflict(printed, name):
    """The model tells the layouts apart: one copy of a table (every other kernel's) conflicts on the same vectors."""
    rng = np.random.default_rng(7)
    index = rng.integers(0, ENTRIES[name], 64)
    assert max(_worst_bank({lane: 16 * int(index[lane]) for lane in group}) for group in GROUPS) > 2


@pytest.mark.parametrize("name", ["log", "angle"])
def test_every_slot_is_distinct_and_staged_from_its_entry(printed, name):
    t, entry, slot, lane_part = printed["table"][name], printed["entry"][name], printed["slot"][name], printed["lane"][name]
    assert sorted(entry) == [(c, k) for c in range(t["copies"]) for k in range(t["entries"])]
    assert len(set(entry.values())) == len(entry) == t["slots"]
    assert all(a % 16 == 0 and 0 <= a and a + 16 <= t["bytes"] for a in entry.values())
    # the staging covers the table once, and what it writes where a gather of (copy, k) reads is entry k
    assert sorted(slot) == list(range(t["slots"]))
    staged = {byte: source for byte, source in slot.values()}
    assert len(staged) == t["slots"]
    for (c, k), a in entry.items():
        assert staged[a] == k, (c, k)
    # a lane's gather of entry k is the slot of (its copy, k)
    for lane in range(64):
        c = lane & (t["copies"] - 1)
        assert lane_part[lane] == 16 * c
        for k in range(t["entries"]):
            assert lane_part[lane] + (k << t["shift"]) == entry[(c, k)]


def test_wavefronts_are_the_chain_groups_of_one_wavefront_workgroups(printed):
    """Wavefront w of block b is what block 4 b + w of the one-wavefront launch was; the grid covers every group."""
    for groups in (1, 2, 5):
        nblocks = printed["blocks"][groups]
        assert nblocks == -(-groups // 4)
        seen = [printed["group"][(b, w)] for b in range(nblocks) for w in range(4)]
        assert seen == list(range(4 * nblocks))
        live = [g for g in seen if g < groups]
        assert live == list(range(groups)), "every group once, in order"
        assert len(seen) - len(live) < 4, "only the last block has wavefronts past the last group"

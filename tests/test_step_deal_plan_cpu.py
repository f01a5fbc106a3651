"""The plan that deals the moment fold's matrix instructions over the pieces of a step (csrc/smcmc_step_deal.h), DP = 50.

tests/cpp/step_deal_plan.C (plain g++, no HIP) prints the plan and the uniform deal of the kernels without a plan.  The
invariants checked here are what the kernel's single-buffered operands (ma[], ms, raw[]) need, and the first two are the
whole bit-identity argument: tiles are independent accumulators, and per tile the k-quads fold in ascending order."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def deals(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_deal") / "step_deal_plan.exe")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'root-simple-mcmc_amd', 'csrc')}",
           os.path.join(ROOT, "tests", "cpp", "step_deal_plan.C"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {"geometry": None}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "geometry":
            out["geometry"] = dict(zip(("G", "NQ", "NT", "NT16", "PREFETCH"), map(int, w[1:])))
        elif w[1] == "score":
            out.setdefault(w[0], {"slots": []})["score"] = int(w[2])
        else:
            assert w[1] == "slot" and int(w[2]) == len(out[w[0]]["slots"]) and w[5] == ":"
            items = []
            for tok in w[6:]:
                m = re.fullmatch(r"(\d+)\.(\d+)(p?)", tok)
                items.append((int(m.group(1)), int(m.group(2)), m.group(3) == "p"))
            out[w[0]]["slots"].append({"fill": int(w[4]), "items": items})
    return out


def _model_score(deal, geo):
    total = 0
    for slot in deal["slots"]:
        for n, (kk, tile, pf) in enumerate(slot["items"]):
            behind = (geo["PREFETCH"] if pf else 0) + (slot["fill"] if n + 1 == len(slot["items"]) else 0)
            duration = 64 if tile < geo["NT16"] else 16
            total += min(4 * behind, duration - 4)
    return total


def test_geometry_of_the_headline_family(deals):
    assert deals["geometry"] == {"G": 104, "NQ": 16, "NT": 10, "NT16": 6, "PREFETCH": 5}
    assert len(deals["plan"]["slots"]) == len(deals["uniform"]["slots"]) == 104


@pytest.mark.parametrize("name", ["plan", "uniform"])
def test_invariants(deals, name):
    geo, deal = deals["geometry"], deals[name]
    seq = [(g, kk, tile, pf) for g, slot in enumerate(deal["slots"]) for kk, tile, pf in slot["items"]]
    # each of the 160 instructions exactly once
    assert sorted((kk, tile) for _, kk, tile, _ in seq) == [(kk, t) for kk in range(geo["NQ"]) for t in range(geo["NT"])]
    # per accumulator tile kk ascends
    for tile in range(geo["NT"]):
        kks = [kk for _, kk, t, _ in seq if t == tile]
        assert kks == sorted(kks) == list(range(geo["NQ"]))
    # all instructions of k-quad kk lie behind its operand preparation (in front of its first instruction) and before
    # that of kk + 1: the sequence is k-quad by k-quad
    assert [kk for _, kk, _, _ in seq] == sorted(kk for _, kk, _, _ in seq)
    first = {}
    for n, (g, kk, _, _) in enumerate(seq):
        first.setdefault(kk, (n, g))
    # the prefetch of kk + 1: once, behind the first instruction of kk and in that instruction's slot ...
    prefetch = {}
    for n, (g, kk, _, pf) in enumerate(seq):
        if pf:
            assert kk + 1 < geo["NQ"] and kk + 1 not in prefetch
            assert n >= first[kk][0] and g == first[kk][1]
            prefetch[kk + 1] = (n, g)
    assert sorted(prefetch) == list(range(1, geo["NQ"]))
    # ... and a piece_ready (a slot boundary) between it and the preparation that consumes it
    for kk in range(1, geo["NQ"]):
        assert prefetch[kk][1] < first[kk][1]
    # the printed score is the model's
    assert deal["score"] == _model_score(deal, geo)


def test_at_most_one_16x16_per_slot(deals):
    geo = deals["geometry"]
    assert geo["G"] >= geo["NQ"] * geo["NT16"]   # enough slots
    for g, slot in enumerate(deals["plan"]["slots"]):
        big = [n for n, (_, tile, _) in enumerate(slot["items"]) if tile < geo["NT16"]]
        assert len(big) <= 1, f"slot {g}"
        # what follows the slot issues in the shadow of its last instruction: the 16x16 stands last
        assert not big or big[0] == len(slot["items"]) - 1, f"slot {g}"


def test_fills_follow_the_pieces(deals):
    """Slot g is followed by the reads of piece g + 2 and a wait; a block's last piece opens with its wait alone and is
    followed by the next block's first piece.  D = 50: rows 0, 1 have four pieces, 2-17 three, 18-33 two, 34-49 one."""
    reads, closes = [], []
    for i in range(50):
        j0 = i & ~1
        cols = list(range(j0, 50, 16))
        for c in cols:
            reads.append(sum(1 for k in range(8) if c + 2 * k < 50))
            closes.append(c == cols[-1] and (i % 4 == 3 or i == 49))
    assert len(reads) == 104
    want = []
    for g in range(104):
        if g == 103:
            want.append(0)
        elif closes[g]:
            want.append(reads[g + 1] + 1)
        elif closes[g + 1]:
            want.append(1)
        else:
            want.append(reads[g + 2] + 1)
    for name in ("plan", "uniform"):
        assert [s["fill"] for s in deals[name]["slots"]] == want, name


def test_plan_scores_no_less_than_the_uniform_deal(deals):
    assert deals["plan"]["score"] >= deals["uniform"]["score"]

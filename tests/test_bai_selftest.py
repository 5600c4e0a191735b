"""build/bai_selftest (host/selftest/bai_selftest.cpp, ASan + UBSan): host/bai_build.hpp — the host's part of --write-index, the
code fade_amd.BaiBuilder and the driver run — on its own hand cases and random call splits, and on calls this test
describes to it, whose .bai it must give back byte for byte as tests/bai_model.py builds it."""
import os
import random
import subprocess

import pytest

import bai_model as bm
from test_bai_model import laid_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
EXE = os.path.join(CSRC, "build", "bai_selftest")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/bai_selftest"])
    return EXE


def test_hand_cases_and_random_call_splits(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "bai_selftest ok", p.stdout.decode() + p.stderr.decode()


def _describe(n_ref, calls):
    lines = ["R %d" % n_ref]
    for base, c in calls:
        lines.append("C %d %d %d %d" % (base, c["n"], c["first_key"], c["last_key"]))
        lines += ["c %d %d %d %d" % x for x in c["chunks"]]
        lines += ["l %d %d %d" % x for x in c["linear"]]
        lines += ["r %d %d %d %d %d" % x for x in c["refs"]]
        lines.append("E")
    return "\n".join(lines + ["F"]) + "\n"


def _records(seed):
    rng = random.Random(seed)
    specs = []
    for tid in rng.sample(range(6), 3):
        pos = rng.choice([0, 20_000])
        for _ in range(rng.choice([1, 50, 500])):
            pos += rng.choice([0, 1, 40, 3000, 20_000])
            specs.append((tid, pos, rng.choice([0, 1, 100, 150, 30_000, 200_000]), 4 if rng.random() < 0.05 else 0))
    specs.sort(key=lambda s: s[0])
    specs += [(-1, -1, 0, 4)] * rng.randrange(4)
    return laid_out(specs, size=rng.choice([60, 333]), block=rng.choice([0x7f00, 0xff00, 0x500]), member=rng.choice([700, 30_000]))


@pytest.mark.parametrize("seed", range(5))
def test_calls_described_to_it_give_the_models_bytes(exe, tmp_path, seed):
    recs = _records(seed)
    rng = random.Random(100 + seed)
    cuts = sorted(rng.sample(range(len(recs) + 1), min(6, len(recs)))) + [len(recs), len(recs)]
    calls, at = [], 0
    for c in cuts:
        part = recs[at:c]
        base = part[0]["u"] >> 16 if part else 12_345
        call = bm.per_call(part)
        down = base << 16
        calls.append((base, dict(call, chunks=[(t, b, u - down, v - down) for t, b, u, v in call["chunks"]],
                                 linear=[(t, w, o - down) for t, w, o in call["linear"]],
                                 refs=[(t, u - down, v - down, nm, nu) for t, u, v, nm, nu in call["refs"]])))
        at = c
    f = tmp_path / "calls.txt"
    f.write_text(_describe(6, calls))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()
    assert bytes.fromhex(p.stdout.decode().strip()) == bm.build(6, recs)


def test_a_call_whose_keys_step_back_is_refused_and_changes_nothing(exe, tmp_path):
    recs = _records(1)
    a, b = bm.per_call(recs[:10]), bm.per_call(recs[5:12])
    f = tmp_path / "calls.txt"
    f.write_text(_describe(6, [(0, a), (0, b)]))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out = p.stdout.decode().splitlines()
    assert p.returncode == 0 and out[0] == "ERR -1 bam stream: record 10: not in coordinate order (--write-index needs coordinate-sorted output)"
    assert bytes.fromhex(out[1]) == bm.build(6, recs[:10])

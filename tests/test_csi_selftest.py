"""build/csi_selftest (host/selftest/csi_selftest.cpp, ASan + UBSan): host/csi_build.hpp — the host's part of --write-index --csi,
the code fade_amd.CsiBuilder and the driver run — on its own hand cases and random call splits, and on calls this test
describes to it, whose payload it must give back byte for byte as tests/csi_model.py builds it."""
import os
import random
import subprocess

import pytest

import csi_model as cm
from test_csi_model import GEOMETRIES, seeded_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
EXE = os.path.join(CSRC, "build", "csi_selftest")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/csi_selftest"])
    return EXE


def test_hand_cases_and_random_call_splits(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "csi_selftest ok", p.stdout.decode() + p.stderr.decode()


def _describe(n_ref, geometry, calls):
    lines = ["R %d %d %d" % ((n_ref,) + tuple(geometry))]
    for base, c in calls:
        lines.append("C %d %d %d %d" % (base, c["n"], c["first_key"], c["last_key"]))
        lines += ["c %d %d %d %d" % x for x in c["chunks"]]
        lines += ["l %d %d %d" % x for x in c["linear"]]
        lines += ["r %d %d %d %d %d" % x for x in c["refs"]]
        lines.append("E")
    return "\n".join(lines + ["F"]) + "\n"


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("seed", range(3))
def test_calls_described_to_it_give_the_models_payload(exe, tmp_path, geometry, seed):
    recs = seeded_records(geometry[0], geometry[1], seed=seed)
    rng = random.Random(100 + seed)
    cuts = sorted(rng.sample(range(len(recs) + 1), 6)) + [len(recs), len(recs)]
    calls, at = [], 0
    for c in cuts:
        part = recs[at:c]
        base = part[0]["u"] >> 16 if part else 12_345
        call = cm.per_call(part, *geometry)
        down = base << 16
        calls.append((base, dict(call, chunks=[(t, b, u - down, v - down) for t, b, u, v in call["chunks"]],
                                 linear=[(t, w, o - down) for t, w, o in call["linear"]],
                                 refs=[(t, u - down, v - down, nm, nu) for t, u, v, nm, nu in call["refs"]])))
        at = c
    f = tmp_path / "calls.txt"
    f.write_text(_describe(3, geometry, calls))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()
    assert bytes.fromhex(p.stdout.decode().strip()) == cm.build(3, recs, *geometry)


def test_a_call_whose_keys_step_back_is_refused_and_changes_nothing(exe, tmp_path):
    recs = seeded_records(4, 2, seed=1)
    a, b = cm.per_call(recs[:10], 4, 2), cm.per_call(recs[5:12], 4, 2)
    f = tmp_path / "calls.txt"
    f.write_text(_describe(3, (4, 2), [(0, a), (0, b)]))
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out = p.stdout.decode().splitlines()
    assert p.returncode == 0 and out[0] == "ERR -1 bam stream: record 10: not in coordinate order (--write-index needs coordinate-sorted output)"
    assert bytes.fromhex(out[1]) == cm.build(3, recs[:10], 4, 2)


def test_a_geometry_that_is_not_valid_is_not_built(exe, tmp_path):
    f = tmp_path / "calls.txt"
    f.write_text("R 1 14 7\nF\n")
    p = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 4 and not p.stdout and b"not valid" in p.stderr

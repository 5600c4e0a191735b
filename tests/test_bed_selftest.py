"""build/bed_selftest (host/selftest/bed_selftest.cpp, ASan + UBSan): host/bed_lite.hpp — the BED parser behind `fade stats
--repeats` and fadehip_intervals_load_bed — on its own hand cases (every rule, every error with its line, every file fed
whole, byte by byte and split at every position), and on files this test writes, whose names and intervals it must give back as
tests/intervals_model.py's bed_text spelt them."""
import os
import subprocess

import pytest

import intervals_model as im
import repeats_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
EXE = os.path.join(CSRC, "build", "bed_selftest")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/bed_selftest"])
    return EXE


def test_hand_cases_fed_whole_byte_by_byte_and_split_everywhere(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "bed_selftest ok", p.stdout.decode() + p.stderr.decode()


def _parsed(exe, path):
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()
    lines = p.stdout.decode("latin-1").splitlines()
    if lines and lines[0].startswith("ERR "):
        return lines[0]
    names = [l[2:] for l in lines if l.startswith("N ")]
    return names, [tuple(int(x) for x in l[2:].split()) for l in lines if l.startswith("I ")]


def test_a_file_of_seeded_intervals_comes_back_as_written(exe, tmp_path):
    ivs = rc.intervals(5000, 3)  # (more than one read of 4096 bytes)
    f = tmp_path / "r.bed"
    f.write_bytes(b"#chrom\tstart\tend\ntrack name=x\n" + im.bed_text([(rc.NAMES[c], s, e) for c, s, e in ivs]).replace(b"\n", b"\tAluY\t0\t+\r\n"))
    names, got = _parsed(exe, f)
    order = []  # ids in order of first appearance
    for c, _, _ in ivs:
        if rc.NAMES[c] not in order:
            order.append(rc.NAMES[c])
    assert names == order and got == [(order.index(rc.NAMES[c]), s, e) for c, s, e in ivs]


def test_an_error_names_its_line(exe, tmp_path):
    f = tmp_path / "bad.bed"
    f.write_bytes(b"chr1\t1\t2\n" * 700 + b"chr1\t5\t4\n" + b"chr1\t1\t2\n")
    assert _parsed(exe, f) == "ERR line 701: start is not below end"
    f.write_bytes(b"chr1\t1\t2\nchr1 3 4")
    assert _parsed(exe, f) == "ERR line 2: fewer than three tab-separated fields"

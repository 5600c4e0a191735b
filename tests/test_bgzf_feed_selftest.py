"""build/bgzf_feed_selftest (host/selftest/bgzf_feed_selftest.cpp, ASan + UBSan): host/bgzf_feed.hpp — the input side of the
file-path drivers (`fade annotate -b`, `fade out / extract / stats --gpus 1`): where the first record lies, the members of
every read at every read size, the batches inflated on the pool, and what it refuses — against zlib and a sequential walk
over small BGZF files the selftest builds itself."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
EXE = os.path.join(CSRC, "build", "bgzf_feed_selftest")


def test_cut_sweep_first_record_refusals_and_extract_records():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/bgzf_feed_selftest"])
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout.decode().strip() == "bgzf_feed_selftest ok", p.stdout.decode() + p.stderr.decode()

"""The device BGZF compressor's output, pinned byte for byte in BOTH block geometries (fade_amd/csrc/bgzf_deflate.hpp).
tests/test_gpu_bgzf.py and tests/test_gpu_bgzf_edges.py hold the output to zlib (it inflates to the input) and both geometries
to the CPU model (host/selftest/gpu_deflate_model.cpp), which is the reference.  This file is a regression pin beside it, on
payloads of plain character at the block boundaries: the SHA-256 and the length of every case's stream are compared with tests/golden/bgzf_device_digests.json, recorded on an MI355X from the commit the file
names (tools/bgzf_record_digests.py, which builds its payloads through build_cases below and refuses a digest that is not
the same in three runs).  A change that means to alter the compressor's bytes records the file anew and says so."""
import hashlib
import json
import os

import numpy as np
import pytest

import fade_amd
from test_gpu_bgzf import bam_payload

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_device_digests.json")
CUT = {64: 0xff00, 32: 0x7f00}  # FADEHIP_BGZF_GEOM -> bytes of a block


def build_cases(geom):
    """{name: payload} for one geometry, deterministic: sizes around its block boundary (one byte, one piece of 64, a byte
    short of a block, a block, a block and a byte, two blocks and a ragged third) of zeros, uniform noise (the stored-block
    path), period-7 bytes and random ACGT, and two BAM record streams (uniform and run-heavy qualities)."""
    cut = CUT[geom]
    rng = np.random.default_rng(1000 + geom)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    cases = {}
    for n in (1, 64, cut - 1, cut, cut + 1, 2 * cut + 17):
        cases["zeros %d" % n] = bytes(n)
        cases["noise %d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cases["period 7 %d" % n] = (((np.arange(n) % 7) * 31) & 255).astype(np.uint8).tobytes()
        cases["acgt %d" % n] = acgt[rng.integers(0, 4, n)].tobytes()
    for runny in (False, True):
        cases["bam runny=%d" % runny] = bam_payload(300, 500 + geom + int(runny), runny)
    return cases


def sha256(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("geom", [64, 32])
def test_case_builder_produces_the_recorded_inputs(golden, geom):
    """(no GPU) A drifted case builder fails here, not as a mismatch of the device's output."""
    cases, want = build_cases(geom), golden["cases"][str(geom)]
    assert list(cases) == list(want)
    assert len(cases) == 4 * 6 + 2
    for name, data in cases.items():
        assert (len(data), sha256(data)) == (want[name]["input_length"], want[name]["input_sha256"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [64, 32])
def test_output_bytes_are_the_recorded_ones(monkeypatch, golden, geom):
    monkeypatch.setenv("FADEHIP_BGZF_GEOM", str(geom))
    want = golden["cases"][str(geom)]
    c = fade_amd.Context(device=0)
    try:
        for name, data in build_cases(geom).items():
            out = bytes(c.bgzf_deflate(data))
            assert (len(out), sha256(out)) == (want[name]["length"], want[name]["sha256"]), \
                "geometry %d, %s: not the bytes of %s" % (geom, name, golden["recorded_from"])
    finally:
        c.close()

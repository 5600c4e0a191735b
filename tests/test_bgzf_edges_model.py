"""(no GPU) The CPU model of the device BGZF compressor (fade_amd/csrc/host/selftest/gpu_deflate_model.cpp, both block
geometries) on the payloads of tests/bgzf_edge_cases.py: zlib inflates every block to its input, and every payload reaches
the limit it was built for — read off the model's stream by the tests' own token parser.  The model runs as an ASan + UBSan
build, so an index past a full match list, say, fails here too.  tests/test_gpu_bgzf_edges.py holds the device to these bytes."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import bgzf_edge_cases as E

GEOMS = [64, 32]
CASES = {g: E.build_edge_cases(g) for g in GEOMS}


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bgzf_edges")
    return {g: E.model_streams(g, CASES[g], tmp) for g in GEOMS}


def test_the_parser_reads_what_zlib_writes():
    """The token parser against an encoder it shares nothing with: dynamic and stored blocks of zlib's."""
    rng = np.random.default_rng(7)
    text = b"".join(b"the quick brown fox %d jumps over the lazy dog\n" % int(x) for x in rng.integers(0, 99, 400))
    for data in (text, bytes(3000), rng.integers(0, 7, 5000, dtype=np.uint8).tobytes()):
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        raw = c.compress(data) + c.flush()
        p = E.deflate_tokens(raw)
        assert p["btype"] == 2 and p["out"] == data and p["used"] == len(raw)
        assert sum(1 if len(t) == 2 else t[1] for t in p["tokens"]) == len(data)
        assert all(t[2] <= t[0] and 3 <= t[1] <= 258 for t in E.matches(p["tokens"]))
    noise = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    p = E.deflate_tokens(c.compress(noise) + c.flush())
    assert p["btype"] == 0 and p["out"] == noise


def test_the_heap_huffman_on_known_tables():
    assert E.optimal_depth([1, 1, 1, 1]) == 2
    assert E.optimal_depth([1, 1, 2, 3, 5, 8, 13, 21]) == 7           # Fibonacci: a chain
    assert E.optimal_depth([E._fib(k) for k in range(1, 23)]) == 21
    assert E.optimal_depth([0, 5, 0]) == 0


@pytest.mark.parametrize("geom", GEOMS)
def test_the_builder_is_small_and_deterministic(geom):
    cut, again = E.CUT[geom], E.build_edge_cases(geom)
    assert list(again) == list(CASES[geom]) and all(again[k] == v for k, v in CASES[geom].items())
    assert all(0 < len(v) < 3 * cut for v in CASES[geom].values())        # two blocks and a ragged tail at most
    assert sum(len(v) for v in CASES[geom].values()) < (3 << 19) * cut // 0x7f00  # about a megabyte for the larger geometry
    assert all(name in CASES[geom] for name in E.CAP_CASES[geom])


@pytest.mark.parametrize("geom", GEOMS)
def test_the_builder_gives_the_recorded_inputs(geom):
    """A drifted builder (a random generator that changed its stream, say) fails here, not as a limit that was not reached."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_edge_inputs.json")) as f:
        want = json.load(f)[str(geom)]
    assert list(want) == list(CASES[geom])
    for name, data in CASES[geom].items():
        assert (len(data), hashlib.sha256(data).hexdigest()) == (want[name]["input_length"], want[name]["input_sha256"]), name


@pytest.mark.parametrize("geom,name", [(g, n) for g in GEOMS for n in CASES[g]])
def test_the_model_reaches_the_edge(streams, geom, name):
    data, got, cut = CASES[geom][name], streams[geom][name], E.CUT[geom]
    assert len(got) == (len(data) + cut - 1) // cut
    for k, s in enumerate(got):
        assert zlib.decompress(s, -15) == data[k * cut:(k + 1) * cut], (name, k)
    E.reach(geom, name, data, got)

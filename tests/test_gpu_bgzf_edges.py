"""The device BGZF compressor, in both block geometries, on the payloads of tests/bgzf_edge_cases.py — each built to reach a
limit of the algorithm (a full match list, the 32,768 distance gate, MAX_MATCH and the block's end, the 15-bit code-length
limit, a block without a match, full alphabets, the stored-block threshold, seams, bucket eviction) —: every member holds
exactly the bytes of the CPU model (host/selftest/gpu_deflate_model.cpp), whose streams tests/test_bgzf_edges_model.py shows
to reach those limits; gzip and the device's own inflater give the input back."""
import gzip

import pytest

import fade_amd
import bgzf_edge_cases as E
from test_gpu_bgzf import EOF_MARK, members

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[64, 32])
def edge(request, tmp_path_factory):
    """(geometry, its cases, the model's streams, a context pinned to the geometry)"""
    geom = request.param
    cases = E.build_edge_cases(geom)
    want = E.model_streams(geom, cases, tmp_path_factory.mktemp("bgzf_edges_gpu"))
    mp = pytest.MonkeyPatch()
    mp.setenv("FADEHIP_BGZF_GEOM", str(geom))  # (read when a context compresses for the first time)
    c = fade_amd.Context(device=0)
    try:
        c.bgzf_deflate(bytes(16))
        yield geom, cases, want, c
    finally:
        c.close()
        mp.undo()


def test_every_member_is_the_model_byte_for_byte(edge):
    geom, cases, want, c = edge
    wrong = []
    for name, data in cases.items():
        out = bytes(c.bgzf_deflate(data))
        got = [m[0] for m in members(out)]
        assert len(got) == len(want[name]) == (len(data) + E.CUT[geom] - 1) // E.CUT[geom], name
        wrong += ["%s: member %d differs from the model (%d / %d bytes)" % (name, j, len(g), len(w))
                  for j, (g, w) in enumerate(zip(got, want[name])) if g != w]
        assert gzip.decompress(out + EOF_MARK) == data, name
        assert c.bgzf_inflate(out).tobytes() == data, name
    assert not wrong, "geometry %d:\n%s" % (geom, "\n".join(wrong))


def test_a_full_match_list_gives_the_same_bytes_every_time(edge):
    """Within 64 records of the list's capacity the 0xff00 geometry's parser once counted positions whose lengths depended on
    how far its extenders had run ahead (bgzf_deflate_g64.hpp role_parser): three runs, one output — and the model's."""
    geom, cases, want, c = edge
    for name in E.CAP_CASES[geom]:
        outs = [bytes(c.bgzf_deflate(cases[name])) for _ in range(3)]
        assert outs[1] == outs[0] and outs[2] == outs[0], name
        assert [m[0] for m in members(outs[0])] == want[name], name

"""tests/recstore_model.py against cases worked by hand: the key and its ties, refID -1 last, pos -1, the drain's cut with a
record larger than max_payload, the three @HD cases; and build/recstore_selftest (host/recstore_host.hpp — the cut and the
@HD edit as the library and the driver compile them — on the same cases, under ASan + UBSan)."""
import os
import struct
import subprocess

import clip_cases as cc
import recstore_model as rm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fade_amd", "csrc")


def _rec(name, tid, pos, bases=4):
    return cc.build_rec(name, tid, pos, 0, 0, -1, -1, 0, "%dM" % bases if tid >= 0 else "*", "ACGT" * (bases // 4), "5" * bases, b"")


def test_key_is_refid_then_pos_plus_one_as_unsigned():
    assert rm.key(_rec("a", 0, 0)) == 1
    assert rm.key(_rec("a", 0, -1)) == 0                        # pos -1: first on its reference
    assert rm.key(_rec("a", 3, 99)) == (3 << 32) | 100
    assert rm.key(_rec("a", -1, -1)) == 0xffffffff00000000      # unmapped: behind every reference
    assert rm.key(_rec("a", -1, 5)) == 0xffffffff00000006
    assert rm.key(_rec("a", 70000, 1 << 30)) == (70000 << 32) | ((1 << 30) + 1)


def test_order_is_stable_and_puts_refid_minus_one_last():
    recs = [_rec("u1", -1, -1), _rec("b", 1, 5), _rec("a", 0, 7), _rec("c", 1, 5), _rec("d", 0, -1), _rec("u2", -1, -1), _rec("e", 1, 4), _rec("f", 1, 5)]
    names = [cc.decode_rec(r)["qname"] for r in rm.order(recs)]
    assert names == ["d", "a", "e", "b", "c", "f", "u1", "u2"]   # b, c, f share a key and keep their order; so do u1, u2
    assert rm.order([]) == []
    assert rm.split(b"".join(recs)) == recs


def test_drain_cut_by_hand():
    sizes = [10, 10, 50, 10, 10, 10]
    assert rm.drain_cut(sizes, 0, 20) == 2       # 10 + 10 fit exactly
    assert rm.drain_cut(sizes, 0, 29) == 2
    assert rm.drain_cut(sizes, 0, 1) == 1        # at least one record
    assert rm.drain_cut(sizes, 2, 20) == 3       # a record larger than max_payload leaves alone
    assert rm.drain_cut(sizes, 2, 60) == 4
    assert rm.drain_cut(sizes, 3, 1000) == 6     # the rest
    assert rm.drain_cut(sizes, 5, 0) == 6
    recs = [_rec("r%d" % k, 0, 100 - k, bases=4 * (1 + k % 3)) for k in range(7)]
    for mp in (1, 60, 61, 130, 10**9):
        d = rm.drains(recs, mp)
        assert [r for run in d for r in run] == rm.order(recs)
        assert all(len(run) == 1 or sum(map(len, run)) <= mp for run in d)
        assert all(sum(map(len, run)) + len(nxt[0]) > mp for run, nxt in zip(d, d[1:]))   # maximal


def test_the_three_hd_cases():
    sq = "@SQ\tSN:c0\tLN:100\n"
    assert rm.header_sorted("@HD\tVN:1.5\tSO:unsorted\n" + sq) == "@HD\tVN:1.5\tSO:coordinate\n" + sq
    assert rm.header_sorted("@HD\tVN:1.4\tSO:queryname\tGO:query\n" + sq) == "@HD\tVN:1.4\tSO:coordinate\tGO:query\n" + sq
    assert rm.header_sorted("@HD\tVN:1.6\n" + sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq
    assert rm.header_sorted(sq) == "@HD\tVN:1.6\tSO:coordinate\n" + sq
    assert rm.header_sorted("") == "@HD\tVN:1.6\tSO:coordinate\n"
    assert rm.header_sorted("@HDX\tVN:1\n") == "@HD\tVN:1.6\tSO:coordinate\n@HDX\tVN:1\n"


def test_recstore_selftest_under_asan_and_ubsan():
    subprocess.check_call(["make", "-C", CSRC, "-s", "build/recstore_selftest"])
    p = subprocess.run([os.path.join(CSRC, "build", "recstore_selftest")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout.decode().strip() == "recstore_selftest ok", p.stdout.decode() + p.stderr.decode()


def test_keys_of_packed_fields_round_trip():
    r = _rec("x", 65536 + 3, 0x01020304)
    assert struct.unpack_from("<ii", r, 4) == (65539, 0x01020304)

"""fadehip_clip_batch (Context.clip_batch): the device function behind `fade annotate --clip` (bam_device.hpp clip_plan /
clip_write_head) on constructed records, against oracle/pyfilter.clip_read — field by field, and as BAM bytes against the
host's build_rec layout (tests/clip_cases.py).  Both-sides clips are covered HERE: the oracle makes no both-sides call on
the random inputs of the file-path tests."""
import numpy as np
import pytest

import clip_cases as cc
import fade_amd

pytestmark = pytest.mark.gpu

CASES = cc.cases()


def _fields(rec):
    tid = cc.CONTIGS.index(rec["rname"]) if rec["rname"] != "*" else -1
    return dict(qname=rec["qname"], tid=tid, pos=rec["pos"], mapq=rec["mapq"], flag=rec["flag"], mtid=tid if rec["rnext"] == "=" else -1,
                mpos=rec["pnext"] - 1, tlen=rec["tlen"], cigar=rec["cigar"], seq=rec["seq"], qual=rec["qual"])


def test_clip_batch_against_pyfilter_field_by_field_and_as_bytes(ctx):
    recs = [cc.to_bam(c["rec"], c["aux"]) for c in CASES]
    got = ctx.clip_batch(recs, [c["rs"] for c in CASES], [c["tl"] for c in CASES], [c["tr"] for c in CASES])
    assert len(got) == len(CASES)
    bad = []
    for c, g in zip(CASES, got):
        new, want = cc.expected(c)
        d = cc.decode_rec(g)
        f = _fields(new)
        for k, v in f.items():
            if d[k] != v:
                bad.append((c["name"], k, d[k], v))
        if d["pad"] != 0:
            bad.append((c["name"], "pad nibble", d["pad"], 0))
        reset = bool(c["rs"] & 6) and new["tags"] == {}
        if d["aux"] != (b"" if reset else c["aux"]):
            bad.append((c["name"], "aux", len(d["aux"]), len(c["aux"])))
        if g != want:
            bad.append((c["name"], "bytes", g[:48].hex(), want[:48].hex()))
    assert not bad, bad[:12]


@pytest.mark.parametrize("order_seed", [1, 2])
def test_clip_batch_in_any_order_and_repeated(ctx, order_seed):
    """The records at other offsets (every alignment of the output) and a batch larger than one block of the kernels."""
    rng = np.random.default_rng(order_seed)
    idx = rng.integers(0, len(CASES), size=1500)
    recs = [cc.to_bam(CASES[i]["rec"], CASES[i]["aux"]) for i in idx]
    got = ctx.clip_batch(recs, [CASES[i]["rs"] for i in idx], [CASES[i]["tl"] for i in idx], [CASES[i]["tr"] for i in idx])
    want = {i: cc.expected(CASES[i])[1] for i in set(int(x) for x in idx)}
    assert [g == want[int(i)] for g, i in zip(got, idx)].count(False) == 0


def test_clip_batch_refuses_malformed_records(ctx):
    good = cc.to_bam(CASES[0]["rec"], CASES[0]["aux"])
    assert ctx.clip_batch([], [], [], []) == []
    cut = good[:40]                                                   # block_size says more than there is
    lname0 = good[:12] + b"\0" + good[13:]                            # l_read_name 0
    big_lseq = good[:20] + (10 ** 6).to_bytes(4, "little") + good[24:]  # l_seq beyond the record
    neg_lseq = good[:20] + (-3).to_bytes(4, "little", signed=True) + good[24:]
    for k, bad in enumerate([cut, lname0, big_lseq, neg_lseq]):
        batch = [good] * k + [bad, good]
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.clip_batch(batch, [2] * len(batch), [3] * len(batch), [0] * len(batch))
        assert e.value.code == -1 and ("record %d" % k) in str(e.value), str(e.value)
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.clip_batch([good], [2], [-1], [0])
    assert e.value.code == -1
    # the context still works
    assert ctx.clip_batch([good], [CASES[0]["rs"]], [CASES[0]["tl"]], [CASES[0]["tr"]])[0] == cc.expected(CASES[0])[1]

"""The gate kernel takes four records per thread: a block owns a tile of 1,024 records, thread t the records
4t .. 4t+3, whole tiles with one wide load per array, a tile cut short by n_reads record by record.  Level 2 against
oracle.annotate_one at the sizes where that changes path (a single record, a quad short of / at / past its end, a tile short
of / at / past its end, two tiles and a cut one), with every record of a tile an item (p_sc = 1.0) and one in ten, each batch
mixed with the records the gate treats apart; the same batch as separate arrays and as the canonical pinned block, and run
again without an upload.  A record that fails a check fails the batch with the message it always had, wherever in its quad it
sits, and leaves its quad neighbours alone."""
import numpy as np
import pytest

import fade_amd
from fade_amd import format_tags, synth

pytestmark = pytest.mark.gpu

FLOOR, WINDOW, LQ = 5, 100, 150
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2051)
M, S, H = 0, 4, 5
REF_OPS = (0, 2, 3, 7, 8)
_refs = {}


def _op(n, op):
    return (n << 4) | op


@pytest.fixture(scope="module")
def genome():
    return synth.Genome(2, 30_000, 77)


def _batch(g, n, p_sc):
    """n reads of 150 bases, clipped with probability p_sc by more than the floor (so p_sc = 1.0 makes every record an item);
    every eleventh record is replaced by one of the kinds the gate tells apart."""
    b = synth.make_reads(g, n, 1000 + n, read_len=LQ, window=WINDOW, p_sc=p_sc, clip_min=FLOOR + 1, clip_max=50,
                         p_unmapped=0.0, p_sa=0.02, p_planted=0.5)
    clen = int(g.lengths[0])
    co = b["cigar_off"].astype(np.int64)
    ops = [[int(x) for x in b["cigar_ops"][co[i]:co[i + 1]]] for i in range(n)]
    tid, pos, flag, sa = b["tid"].copy(), b["pos"].copy(), b["flag"].copy(), b["has_sa"].copy()
    for j in range(3, n, 11):
        kind = (j // 11 + n) % 10
        if kind == 0:    # unmapped
            ops[j], tid[j], pos[j] = [], -1, -1
            flag[j] |= 4
        elif kind == 1:  # no S op
            ops[j] = [_op(LQ, M)]
        elif kind == 2:  # hard clips outside soft clips, left
            ops[j] = [_op(5, H), _op(20, S), _op(LQ - 20, M), _op(3, H)]
        elif kind == 3:  # hard clips outside soft clips on both sides
            ops[j] = [_op(4, H), _op(9, S), _op(LQ - 30, M), _op(21, S), _op(2, H)]
        elif kind == 4:  # clips on both sides
            ops[j] = [_op(12, S), _op(LQ - 30, M), _op(18, S)]
        elif kind == 5:  # a clip of exactly floor_len: not re-aligned
            ops[j] = [_op(FLOOR, S), _op(LQ - FLOOR, M)]
        elif kind == 6:  # floor_len + 1: re-aligned
            ops[j] = [_op(LQ - FLOOR - 1, M), _op(FLOOR + 1, S)]
        elif kind == 7:  # has_sa
            ops[j] = [_op(30, S), _op(LQ - 30, M)]
            sa[j] = 1
        elif kind == 8:  # at the contig's start: the window is cut on the left
            ops[j], pos[j] = [_op(25, S), _op(LQ - 25, M)], 0
        else:            # at the contig's end: cut on the right
            ops[j], pos[j] = [_op(LQ - 25, M), _op(25, S)], clen - (LQ - 25)
    out = dict(b, tid=tid, pos=pos, flag=flag, has_sa=sa)
    out["cigar_off"] = np.concatenate([[0], np.cumsum([len(o) for o in ops])]).astype(np.uint32)
    out["cigar_ops"] = np.array([x for o in ops for x in o], dtype=np.uint32)
    return out


def _gate_model(b, clen):
    """anno.d:61-74 + util.d:37-62 + analysis.d:34-59 per record: {read: (win_start, win_len, clip_left, clip_right, aligned_len)}
    of the records that are re-aligned."""
    out = {}
    co = b["cigar_off"].astype(np.int64)
    for i in range(len(b["pos"])):
        n_soft, clip_l, clip_r, aligned, first = 0, 0, 0, 0, True
        for c in b["cigar_ops"][co[i]:co[i + 1]]:
            op, ln = int(c) & 15, int(c) >> 4
            n_soft += op == S
            aligned += ln if op in REF_OPS else 0
            if op == H:
                continue
            if first and op != S:
                first = False
            elif first:
                clip_l = ln
            elif op == S:
                clip_r = ln
        if (int(b["flag"][i]) & 4) or n_soft == 0 or not (clip_l > FLOOR or clip_r > FLOOR):
            continue
        start = max(int(b["pos"][i]) - WINDOW, 0)
        end = min(int(b["pos"][i]) + aligned + WINDOW, clen)
        if end > start:
            out[i] = (start, end - start, clip_l, clip_r, aligned)
    return out


def _reference(oracle, g, b, key):
    if key not in _refs:
        G = oracle.GenomeHolder(g.names, [a.tobytes() for a in g.ascii_contigs()])
        reads, keep = oracle.make_reads(b)
        rs, tags = np.zeros(len(b["pos"]), dtype=np.uint8), {}
        for i in range(len(rs)):
            a = oracle.annotate_one(G, reads[i], floor_len=FLOOR, window=WINDOW)
            rs[i] = a["rs"]
            if a["has_tags"]:
                tags[i] = dict(rs=a["rs"], am=a["am"], as_=a["as_"], ar=a["ar"], ab=a["ab"])
        _refs[key] = (rs, tags, _gate_model(b, int(g.lengths[0])))
    return _refs[key]


def _key(res):
    rs, aln, st = res
    order = np.lexsort((aln["win_start"], aln["read_idx"]))
    return rs.tobytes(), aln[order].tobytes(), tuple(int(x) for x in st)


def _check(g, b, res, ref):
    rs, aln, st = res
    ors, otags, model = ref
    assert np.array_equal(rs, ors), "rs differs at %r" % np.nonzero(rs != ors)[0][:10]
    a = aln[np.lexsort((aln["win_start"], aln["read_idx"]))]
    want = sorted(model)
    assert [int(x) for x in a["read_idx"]] == want
    for k, f in enumerate(("win_start", "win_len", "clip_left", "clip_right", "aligned_len")):
        assert [int(x) for x in a[f]] == [model[i][k] for i in want], f
    assert format_tags(b, g.names, rs, aln) == otags
    c = np.zeros(8, dtype=np.int64)  # stats.d:45-54 over the batch
    for v in ors:
        c += [1, v & 1, (v >> 5) & 1, ((v >> 1 | v >> 2) & 1) & (v >> 5) & 1, (v >> 1 | v >> 2) & 1,
              ((v >> 1) & (v >> 3) | (v >> 2) & (v >> 4)) & 1, (v >> 1) & 1, (v >> 2) & 1]
    assert list(st) == list(c)


@pytest.mark.parametrize("p_sc", [1.0, 0.1], ids=["every_record_an_item", "one_in_ten"])
@pytest.mark.parametrize("n", SIZES)
def test_quads_and_cut_tiles_against_the_oracle(ctx, oracle, genome, n, p_sc):
    g = genome
    ctx.genome_upload(g.names, g.ascii_contigs())
    b = _batch(g, n, p_sc)
    ref = _reference(oracle, g, b, (n, p_sc))
    if p_sc == 1.0 and n >= 1024:  # the first tile is full of items but for the mixed-in records
        assert sum(1 for i in ref[2] if i < 1024) > 900
    apart = ctx.annotate(b, FLOOR, WINDOW)  # separate arrays, gathered into the slot's staging block
    _check(g, b, apart, ref)
    ctx.annotate_upload(1, ctx.pinned_batch(ctx.with_bounds(b)))  # the canonical pinned block, with the caller's bounds
    ctx.annotate_run(1, FLOOR, WINDOW)
    block = ctx.annotate_collect(1)
    ctx.annotate_run(1, FLOOR, WINDOW)  # the resident batch again: no second upload
    again = ctx.annotate_collect(1)
    assert _key(block) == _key(apart)
    assert _key(again) == _key(block)


def _decreasing_cigar_off(b, j):
    co = b["cigar_off"].copy()
    co[j + 1] = co[j] - 1
    return dict(b, cigar_off=co)


def _l_seq_outside(b, j):
    ls = b["l_seq"].copy()
    ls[j] = LQ + 1  # announced: 150 .. 150
    return dict(b, l_seq=ls)


def _without_bases(b, j):
    so = b["seq_off"].astype(np.int64)
    cut = so[j + 1] - so[j]
    assert cut > 0
    so[j + 1:] -= cut
    return dict(b, seq_off=so.astype(np.uint32), seq_packed=np.concatenate([b["seq_packed"][:so[j]], b["seq_packed"][so[j] + cut:]]))


def _bad_tid(b, j):
    tid = b["tid"].copy()
    tid[j] = 2  # the genome has contigs 0 and 1
    return dict(b, tid=tid)


ERRORS = {
    "decreasing_cigar_off": (_decreasing_cigar_off, "cigar_off / seq_off are not non-decreasing"),
    "l_seq_outside_the_bounds": (_l_seq_outside, "a read outside them"),
    "clipped_without_bases": (_without_bases, "seq_packed slice is shorter than its l_seq"),
    "bad_tid": (_bad_tid, "tid is not a contig of the uploaded genome"),
}


@pytest.mark.parametrize("what", list(ERRORS))
def test_a_bad_record_fails_the_batch_wherever_it_sits_in_its_quad(ctx, oracle, genome, what):
    """The bad record at quad positions 0 - 3 of a whole tile and in the cut tile (records 2048 - 2050 of 2,051); the twin batch
    with that record sound gives the oracle's rs and alignments, its quad neighbours included."""
    g, n = genome, 2051
    ctx.genome_upload(g.names, g.ascii_contigs())
    b = _batch(g, n, 1.0)
    ref = _reference(oracle, g, b, (n, 1.0))
    good = ctx.with_bounds(b)
    assert (good["l_seq_min"], good["l_seq_max"]) == (LQ, LQ)
    spoil, message = ERRORS[what]
    for j in (1044, 1045, 1046, 1047, 2048):
        assert j in ref[2] and j % 11 != 3  # one of the plain clipped records, re-aligned when sound
        with pytest.raises(fade_amd.FadeHipError) as e:
            ctx.annotate(spoil(good, j), FLOOR, WINDOW)
        assert e.value.code == -1 and message in str(e.value), str(e.value)
        res = ctx.annotate(good, FLOOR, WINDOW)
        quad = [r for r in range(j & ~3, min((j & ~3) + 4, n))]
        assert [int(res[0][r]) for r in quad] == [int(ref[0][r]) for r in quad]
        got = set(int(x) for x in res[1]["read_idx"])
        assert all((r in got) == (r in ref[2]) for r in quad)
        _check(g, b, res, ref)

"""fadehip_genome_upload_fasta: the genome read from the FASTA file through its .fai entries and packed on the device, seen
through fadehip_genome_fetch, against the residues the cases were built from and against fadehip_genome_upload of the same
residues into a second context.

The matrix runs with FADEHIP_FASTA_CHUNK=4096, so files of a few hundred kB cross dozens of chunk edges, and every case goes
up plain and BGZF-compressed (members of 1,001 payload bytes — odd, so members end inside lines, inside CRLF and between the
two bases of a packed byte — with an empty member in the middle and one at the end).  tests/fasta_cases.py lays the files
out: 1, 7 and 60 bases a line and one line longer than the contig, LF and CRLF, last lines full, partial and without a
terminator at the end of the file, contigs of 0, 1, 15, 16, 17 and 4,097 bases, lower case, every IUPAC letter and bytes
outside IUPAC.  Each file goes up in file order with every base, and in reverse order with fewer bases than the contigs hold
(an even and an odd number) and, for one-line contigs, a line_bases beyond the contig.

genome_fetch reads inside one contig, so the pad bases behind a contig are seen from both sides only: a fetch that ends at the
contig's last base (the byte it shares with the pad when the length is odd) and the next contig's first bases.
"""
import gzip
import os

import numpy as np
import pytest

import fade_amd
import fasta_cases as FC
import genome_scale as GS

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE, E_RESIDUE = -1, -5, -6, -7
FILES = {"lf_partial": (b"\n", 11, "partial"), "crlf_full": (b"\r\n", 12, "full")}


@pytest.fixture(scope="module")
def two():
    """The context under test and the one that takes the parsed residues through fadehip_genome_upload."""
    a, b = fade_amd.Context(device=0), fade_amd.Context(device=0)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (contigs, path of the plain file, path of the BGZF file, hand-computed entries), written once."""
    d = tmp_path_factory.mktemp("fasta")
    out = {}
    for name, (term, seed, tail) in FILES.items():
        contigs = FC.matrix_contigs(term, seed, tail)
        plain, bgz = d / (name + ".fa"), d / (name + ".fa.gz")
        text, entries = FC.write_fasta(plain, contigs)
        sizes = FC.odd_sizes(len(text))
        assert sizes.count(0) == 2 and sizes[-1] == 0 and len(sizes) > 200
        bgz.write_bytes(b"".join(FC.bgzf_members(text, sizes)))
        assert gzip.decompress(bgz.read_bytes()) == text
        out[name] = (contigs, str(plain), str(bgz), entries)
    return out


def _upload(ctx, path, entries):
    ents = (fade_amd._lib.FaiEntry * len(entries))()
    for k, e in enumerate(entries):
        ents[k].length, ents[k].offset, ents[k].line_bases, ents[k].line_width = e.length, e.offset, e.line_bases, e.line_width
    ctx._chk(ctx._L.fadehip_genome_upload_fasta(ctx._h, os.fsencode(path), len(entries), ents))


def _reordered(contigs, entries, term):
    """Reverse file order; 4,097-base contigs give 4,000 or 3,999 bases, 17-base ones 16, the big one an odd number; a contig on
    one line says line_bases 5,000."""
    seq = {c.name: c.seq for c in contigs}
    out = []
    for k, e in enumerate(reversed(entries)):
        n = e.length
        if n == 4097:
            n = 4000 if k % 2 else 3999
        elif n == 17:
            n = 16
        elif n > 100_000:
            n = 150_001
        if 0 < e.length <= e.line_bases and e.line_width > e.line_bases:
            e = e._replace(line_bases=5000, line_width=5000 + len(term))
        out.append(e._replace(length=n))
    return out, [seq[e.name][:e.length] for e in out]


def _windows(n):
    """(start, n) inside a contig of n bases: whole, odd starts and lengths, the last base alone and with its neighbours."""
    w = {(0, n), (0, min(n, 5))}
    if n >= 3:
        w |= {(1, n - 2), (1, n - 1), (n - 1, 1), (n - 3, 3), (n // 2 | 1, min(33, n - (n // 2 | 1)))}
    if n >= 4200:
        w |= {(4095, 3), (2047, 2051)}
    return sorted(w)


def _fetch_all(ctx, lengths):
    return {(t, s, n): ctx.genome_fetch(t, s, n) for t, L in enumerate(lengths) for s, n in _windows(L)}


_reference = {}


@pytest.mark.parametrize("packing", ["plain", "bgzf"])
@pytest.mark.parametrize("order", ["file_order", "reversed_fewer_bases"])
@pytest.mark.parametrize("name", sorted(FILES))
def test_matrix(two, files, monkeypatch, name, order, packing):
    ctx, ref = two
    contigs, plain, bgz, entries = files[name]
    if order == "file_order":
        ents, seqs = entries, [c.seq for c in contigs]
    else:
        ents, seqs = _reordered(contigs, entries, FILES[name][0])
        assert {len(s) for s in seqs} >= {0, 1, 15, 16, 3999, 4000, 150_001}
    lengths = [len(s) for s in seqs]
    monkeypatch.setenv("FADEHIP_FASTA_CHUNK", "4096")
    _upload(ctx, plain if packing == "plain" else bgz, ents)
    got = _fetch_all(ctx, lengths)
    for (t, s, n), letters in got.items():
        assert letters == FC.expected_letters(seqs[t][s:s + n]), (ents[t].name, s, n)
    assert any(b"=" in v for v in got.values()) and any(n == 0 for _, _, n in got)
    # the same residues through fadehip_genome_upload, in a second context: byte for byte
    if (name, order) not in _reference:
        ref.genome_upload([e.name for e in ents], [bytes(s) for s in seqs])
        _reference[(name, order)] = _fetch_all(ref, lengths)
    assert got == _reference[(name, order)]
    for t, L in enumerate(lengths):  # what lies outside a contig is not served
        for s, n in ((0, L + 1), (L, 1), (-1, 1), (1, -1)):
            with pytest.raises(fade_amd.FadeHipError) as e:
                ctx.genome_fetch(t, s, n)
            assert e.value.code == E_INVALID
    with pytest.raises(fade_amd.FadeHipError) as e:
        ctx.genome_fetch(len(lengths), 0, 0)
    assert e.value.code == E_INVALID


def test_default_chunk_gives_the_same_genome(two, files):
    """Without FADEHIP_FASTA_CHUNK (64 MB chunks: the file is one chunk) the genome is the one the small chunks gave."""
    ctx, _ = two
    assert "FADEHIP_FASTA_CHUNK" not in os.environ
    contigs, plain, bgz, entries = files["crlf_full"]
    for path in (plain, bgz):
        _upload(ctx, path, entries)
        for t, c in enumerate(contigs):
            assert ctx.genome_fetch(t, 0, len(c.seq)) == FC.expected_letters(c.seq), (path, c.name)


def test_python_layer_reads_the_index(two, files):
    """Context.genome_upload_fasta: path + ".fai" from fasta_index.build_fai, every contig or the named ones in the caller's order."""
    from fade_amd import fasta_index
    ctx, _ = two
    contigs, plain, _, entries = files["lf_partial"]
    assert [tuple(e) for e in fasta_index.build_fai(plain)] == [tuple(e) for e in entries]
    ctx.genome_upload_fasta(plain)
    assert ctx.contig_names == [c.name for c in contigs]
    assert ctx.genome_fetch(len(contigs) - 1, 0, len(contigs[-1].seq)) == FC.expected_letters(contigs[-1].seq)
    pick = ["tail", "c17_w7", "big"]
    ctx.genome_upload_fasta(plain, names=pick)
    assert ctx.contig_names == pick
    seq = {c.name: c.seq for c in contigs}
    for t, n in enumerate(pick):
        assert ctx.genome_fetch(t, 0, len(seq[n])) == FC.expected_letters(seq[n])


def test_fetch_before_any_upload_is_a_state_error():
    c = fade_amd.Context(device=0)
    try:
        with pytest.raises(fade_amd.FadeHipError) as e:
            c.genome_fetch(0, 0, 1)
        assert e.value.code == E_STATE
    finally:
        c.close()


def test_errors_leave_a_context_that_then_uploads_correctly(two, files, tmp_path, monkeypatch):
    ctx, _ = two
    monkeypatch.setenv("FADEHIP_FASTA_CHUNK", "4096")
    contigs, plain, bgz, entries = files["lf_partial"]
    big = next(k for k, e in enumerate(entries) if e.name == "big")

    def fails(path, ents, code, *words):
        with pytest.raises(fade_amd.FadeHipError) as e:
            _upload(ctx, path, ents)
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    def good():
        _upload(ctx, plain, entries)
        for t in (0, big, len(entries) - 1):
            assert ctx.genome_fetch(t, 0, entries[t].length) == FC.expected_letters(contigs[t].seq)

    def stale(k, **kw):
        return [e._replace(**kw) if j == k else e for j, e in enumerate(entries)]

    # a stale index: the contig's number is in the message
    for path in (plain, bgz):
        fails(path, stale(big, line_width=entries[big].line_width + 1), E_INVALID, "index does not match the FASTA", "contig %d " % big)
        fails(path, stale(big, offset=entries[big].offset - 1), E_INVALID, "index does not match the FASTA", "contig %d " % big)
        fails(path, stale(3, offset=entries[3].offset + 1), E_INVALID, "index does not match the FASTA", "contig 3 ")
        last = len(entries) - 1
        fails(path, stale(last, length=entries[last].length + 1000), E_INVALID, "index does not match the FASTA", "contig %d " % last, "beyond the file")
        good()
    # '=' is no residue
    text = open(plain, "rb").read()
    at = entries[big].offset + 61 * 1000 + 17
    eq = tmp_path / "eq.fa"
    eq.write_bytes(text[:at] + b"=" + text[at + 1:])
    fails(str(eq), entries, E_RESIDUE, "'='")
    eqz = tmp_path / "eq.fa.gz"
    eqz.write_bytes(b"".join(FC.bgzf_members(eq.read_bytes(), FC.odd_sizes(len(text)))))
    fails(str(eqz), entries, E_RESIDUE, "'='")
    good()
    # a member whose CRC32 is wrong
    ms = FC.bgzf_members(text, FC.odd_sizes(len(text)))
    k = len(ms) // 3
    assert len(ms[k]) > 100
    ms[k] = ms[k][:-8] + bytes([ms[k][-8] ^ 1]) + ms[k][-7:]
    crc = tmp_path / "crc.fa.gz"
    crc.write_bytes(b"".join(ms))
    fails(str(crc), entries, E_INVALID, "CRC32")
    # a member that says a wrong ISIZE
    ms = FC.bgzf_members(text, FC.odd_sizes(len(text)))
    ms[k] = ms[k][:-4] + (1000).to_bytes(4, "little")
    isz = tmp_path / "isize.fa.gz"
    isz.write_bytes(b"".join(ms))
    fails(str(isz), entries, E_INVALID)
    good()
    # gzip without BGZF framing is not for this entry point
    gz = tmp_path / "plain.fa.gz"
    gz.write_bytes(gzip.compress(text))
    fails(str(gz), entries, E_UNSUPPORTED, "BGZF")
    fails(str(tmp_path / "missing.fa"), entries, E_INVALID, "cannot open")
    monkeypatch.setenv("FADEHIP_FASTA_CHUNK", "4095")
    fails(plain, entries, E_INVALID, "FADEHIP_FASTA_CHUNK")
    monkeypatch.setenv("FADEHIP_FASTA_CHUNK", "4096")
    good()


def test_packed_bases_past_2p32_and_file_offsets_past_2p32(tmp_path):
    """One contig of chr1's length in a 250 MB file, nineteen entries on that one file range (4.7 G packed bases), a short
    contig behind it in the file, and one past file offset 2^32 (a hole: no disk).  Windows that straddle packed base 2^31 and
    2^32, both ends of the aliases around them, and the contigs at the packed buffer's end."""
    rng = np.random.Generator(np.random.PCG64(20261018))
    L, LB = GS.CHR1_LEN, 60
    bases = GS.ACGT[rng.integers(0, 4, size=L, dtype=np.uint8)]
    full = L // LB
    lines = np.full((full, LB + 1), 10, dtype=np.uint8)
    lines[:, :LB] = bases[:full * LB].reshape(full, LB)
    short = FC.random_residues(rng, 1001)
    far = FC.random_residues(rng, 777)
    fa = tmp_path / "scale.fa"
    head = b">chr1 of the scale test\n"
    with open(fa, "wb") as f:
        f.write(head)
        lines.tofile(f)
        f.write(bases[full * LB:].tobytes() + b"\n")
        short_off = f.tell() + len(b">short\n")
        f.write(b">short\n" + b"\n".join(short[a:a + LB] for a in range(0, len(short), LB)) + b"\n")
        dense_end = f.tell()
        f.seek((1 << 32) + 12345)
        far_off = f.tell() + len(b">far\n")
        f.write(b">far\n" + b"\n".join(far[a:a + LB] for a in range(0, len(far), LB)) + b"\n")
    del lines
    hole_kept = os.stat(fa).st_blocks * 512 < dense_end + (64 << 20)
    chr1 = FC.Entry("chr1", L, len(head), LB, LB + 1)
    entries = [chr1] * 19 + [FC.Entry("short", len(short), short_off, LB, LB + 1)]
    if hole_kept:
        entries.append(FC.Entry("far", len(far), far_off, LB, LB + 1))
    base, total = GS.packed_bases([e.length for e in entries])
    assert base[19] > 1 << 32 and far_off > 1 << 32
    ctx = fade_amd.Context(device=0)
    try:
        _upload(ctx, str(fa), entries)
        for g in (1 << 31, 1 << 32):
            t = int(np.searchsorted(base, g, side="right")) - 1
            p = g - int(base[t])
            assert 1000 < p < L - 1000 and 0 < t < 19
            for s, n in ((p - 51, 101), (p - 1, 2), (p, 1), (p - 37, 37), (p + 1, 64)):
                assert ctx.genome_fetch(t, s, n) == bases[s:s + n].tobytes(), (g, s, n)
        for t in (0, 8, 17, 18):
            assert ctx.genome_fetch(t, 0, 99) == bases[:99].tobytes()
            assert ctx.genome_fetch(t, L - 99, 99) == bases[L - 99:].tobytes()
        assert ctx.genome_fetch(18, 123_456_789, 300_001) == bases[123_456_789:123_456_789 + 300_001].tobytes()
        assert ctx.genome_fetch(19, 0, len(short)) == FC.expected_letters(short)
        if hole_kept:
            assert ctx.genome_fetch(20, 0, len(far)) == FC.expected_letters(far)
            assert ctx.genome_fetch(20, 776, 1) == FC.expected_letters(far[776:])
    finally:
        ctx.close()
    if not hole_kept:
        pytest.skip("the file system stored the hole in front of offset 2^32 (st_blocks): that leg did not run; the rest passed")

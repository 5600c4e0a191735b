"""fade_amd.fasta_index on the CPU: build_fai writes what the cases' builder worked out by hand while laying the file out
(samtools faidx's columns), read_fai reads it back, and files samtools would refuse are refused."""
import pytest

import fasta_cases as FC
from fade_amd import fasta_index


def _cases():
    return [("lf_partial", FC.matrix_contigs(b"\n", 1, "partial")), ("crlf_full", FC.matrix_contigs(b"\r\n", 2, "full")),
            ("crlf_partial", FC.matrix_contigs(b"\r\n", 3, "partial")), ("lf_full", FC.matrix_contigs(b"\n", 4, "full"))]


@pytest.mark.parametrize("name,contigs", _cases(), ids=[c[0] for c in _cases()])
def test_build_fai_agrees_with_the_hand_computed_entries_and_round_trips(tmp_path, name, contigs):
    fa = tmp_path / (name + ".fa")
    text, entries = FC.write_fasta(fa, contigs)
    built = fasta_index.build_fai(str(fa))
    assert [tuple(e) for e in built] == [tuple(e) for e in entries]
    assert [tuple(e) for e in fasta_index.read_fai(str(fa) + ".fai")] == [tuple(e) for e in entries]
    # the entries say where every base is: offset + b // line_bases * line_width + b % line_bases
    for c, e in zip(contigs, entries):
        assert e.length == len(c.seq)
        for b in {0, 1, e.length // 2, e.length - 2, e.length - 1} & set(range(e.length)):
            at = e.offset + b // e.line_bases * e.line_width + b % e.line_bases
            assert text[at] == c.seq[b], (c.name, b)


def test_read_fai_round_trips_a_written_index(tmp_path):
    entries = [FC.Entry("a", 0, 3, 0, 0), FC.Entry("b c", 5_000_000_000, 4_294_967_299, 60, 62)]
    FC.write_fai(tmp_path / "x.fai", entries)
    assert [tuple(e) for e in fasta_index.read_fai(str(tmp_path / "x.fai"))] == [tuple(e) for e in entries]


@pytest.mark.parametrize("text", [
    b">a\nACGT\nAC\nACGT\n",           # a short line in the middle
    b">a\nACGT\nACGTA\n",              # a longer line after the first
    b">a\nACGT\r\nACGT\nAC\n",         # terminators of different widths
    b">a\nACGT\n\nACGT\n",             # bases after an empty line
    b"ACGT\n>a\nACGT\n",               # bases before the first header
    b">\nACGT\n",                      # a header without a name
    b">a\nAC\n>a\nAC\n",               # a name twice
    b"",                               # nothing
], ids=["short_middle", "longer_later", "mixed_terminators", "empty_line_inside", "no_header", "no_name", "duplicate", "empty"])
def test_build_fai_rejects_what_samtools_rejects(tmp_path, text):
    fa = tmp_path / "bad.fa"
    fa.write_bytes(text)
    with pytest.raises(ValueError):
        fasta_index.build_fai(str(fa))
    assert not (tmp_path / "bad.fa.fai").exists()


def test_build_fai_accepts_the_legal_odd_ends(tmp_path):
    fa = tmp_path / "ok.fa"
    fa.write_bytes(b">a x\nACGT\nAC\n\n>b\n>c\tz\nACGT\nACGT")
    got = [tuple(e) for e in fasta_index.build_fai(str(fa))]
    assert got == [("a", 6, 5, 4, 5), ("b", 0, 17, 0, 0), ("c", 8, 22, 4, 5)]


def test_read_fai_rejects_lines_that_are_no_index(tmp_path):
    for text in ("a\t10\t3\n", "a\tten\t3\t4\t5\n", "a\t10\t3\t6\t5\n", "a\t10\t3\t0\t0\n"):
        p = tmp_path / "bad.fai"
        p.write_text(text)
        with pytest.raises(ValueError):
            fasta_index.read_fai(str(p))

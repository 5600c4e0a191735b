"""FASTA files for the indexed genome path (fadehip_genome_upload_fasta, fade_amd.fasta_index), built byte by byte so that the
.fai entries are known by construction, and a BGZF writer that cuts its members where the caller says.

A case is a list of Contig: name, the residues as the file holds them (any case, any byte a line may hold), the bases per
line, the line terminator, and whether the contig's last line has one.  write_fasta returns the file's text, the .fai entries
worked out by hand while writing (samtools faidx's columns); expected_letters says what the device must hold.
"""
import collections
import struct
import zlib

import numpy as np

Contig = collections.namedtuple("Contig", "name seq line_bases term last_newline")
Entry = collections.namedtuple("Entry", "name length offset line_bases line_width")

IUPAC = b"ACMGRSVTWYHKDBN"
LETTERS = b"=ACMGRSVTWYHKDBN"
# bytes a FASTA line may hold that are no IUPAC letter: they pack as code 0 and read back as '='
NON_IUPAC = b"XxUuZz*-.0Ee"
_UPPER = np.full(256, ord("="), dtype=np.uint8)
for _c in IUPAC:
    _UPPER[_c] = _c
    _UPPER[_c | 0x20] = _c


def expected_letters(seq):
    """What genome_fetch returns for residues seq: IUPAC letters upper-cased, every other byte '='."""
    return _UPPER[np.frombuffer(bytes(seq), dtype=np.uint8)].tobytes()


def random_residues(rng, n, alphabet=b"ACGTacgtNn"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, len(a), size=n)].tobytes()


def fasta_text(contigs):
    """(file bytes, [Entry]) — the entries are computed here, from the layout being written, not by reading it back."""
    out, entries = bytearray(), []
    for k, c in enumerate(contigs):
        assert c.last_newline or k == len(contigs) - 1, "only the file's last line may lack its terminator"
        out += b">" + c.name.encode() + b" description of " + c.name.encode() + c.term
        offset, n = len(out), len(c.seq)
        lines = [c.seq[a:a + c.line_bases] for a in range(0, n, c.line_bases)]
        for j, ln in enumerate(lines):
            out += ln
            if j < len(lines) - 1 or c.last_newline:
                out += c.term
        if n == 0:
            entries.append(Entry(c.name, 0, offset, 0, 0))
        else:
            lb = len(lines[0])
            lw = lb + (len(c.term) if len(lines) > 1 or c.last_newline else 0)
            entries.append(Entry(c.name, n, offset, lb, lw))
    return bytes(out), entries


def write_fasta(path, contigs):
    text, entries = fasta_text(contigs)
    with open(path, "wb") as f:
        f.write(text)
    return text, entries


def write_fai(path, entries):
    with open(path, "w") as f:
        for e in entries:
            f.write("%s\t%d\t%d\t%d\t%d\n" % e)


# ---- BGZF (SAM spec 4.1): gzip members with the 'BC' extra subfield, raw DEFLATE from zlib
def bgzf_member(payload, level=6):
    assert len(payload) <= 65536
    if payload:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(payload) + co.flush()
    else:
        body = b"\x03\x00"
    bsize = 12 + 6 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + body +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf_members(data, sizes):
    """data cut into members of exactly these payload sizes (0: an empty member); the sizes must add up to len(data)."""
    assert sum(sizes) == len(data), (sum(sizes), len(data))
    out, at = [], 0
    for s in sizes:
        out.append(bgzf_member(data[at:at + s]))
        at += s
    return out


def odd_sizes(n, payload=1001):
    """Member payloads of `payload` bytes (odd: members end inside lines, inside CRLF and between the two bases of a packed
    byte), an empty member in the middle, the remainder, and the empty end-of-file member."""
    full = [payload] * (n // payload)
    rest = [n % payload] if n % payload else []
    mid = len(full) // 2
    return full[:mid] + [0] + full[mid:] + rest + [0]


# ---- the matrix of tests/test_gpu_genome_fasta.py and tests/test_fasta_index.py
LENGTHS = (0, 1, 15, 16, 17, 4097)


def matrix_contigs(term, seed, tail):
    """Contigs of every length in LENGTHS at 1, 7 and 60 bases per line and on one line longer than the contig (last lines
    full — 16 at 1, 4097 = 17 * 241 at 241 — and partial), one of a few hundred kB with lower case, every IUPAC letter and bytes
    outside IUPAC, and the file's last contig: `tail` = "partial" (a partial last line without a terminator) or "full" (a
    full one without)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rich = IUPAC + IUPAC.lower() + NON_IUPAC
    out = []
    for lb in (1, 7, 60, 5000):
        for n in LENGTHS:
            out.append(Contig("c%d_w%d" % (n, lb), random_residues(rng, n, rich if n == 4097 else b"ACGTacgtNn"), lb, term, True))
    out.append(Contig("full_lines", random_residues(rng, 4097, rich), 241, term, True))
    out.append(Contig("big", random_residues(rng, 200_003, rich), 60, term, True))
    if tail == "partial":
        out.append(Contig("tail", random_residues(rng, 100, rich), 60, term, False))
    else:
        out.append(Contig("tail", random_residues(rng, 120, rich), 60, term, False))
    return out

"""The .fai index of a FASTA file (samtools faidx): one line per contig, NAME LENGTH OFFSET LINEBASES LINEWIDTH.

read_fai parses one, build_fai writes one for a plain (uncompressed) FASTA by samtools' rules.  The entries are what
Context.genome_upload_fasta hands to fadehip_genome_upload_fasta: with them the device finds every base in the file's bytes.
"""
import collections
import os

FaiEntry = collections.namedtuple("FaiEntry", "name length offset line_bases line_width")


def read_fai(path):
    """The entries of a .fai file, in file order."""
    out = []
    with open(path, "rb") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip(b"\r\n")
            if not line:
                continue
            cols = line.split(b"\t")
            try:
                if len(cols) < 5:
                    raise ValueError
                e = FaiEntry(cols[0].decode(), int(cols[1]), int(cols[2]), int(cols[3]), int(cols[4]))
            except ValueError:
                raise ValueError("%s line %d is not NAME LENGTH OFFSET LINEBASES LINEWIDTH" % (path, no)) from None
            if e.length < 0 or e.offset < 0 or e.line_bases < 0 or e.line_width < e.line_bases or (e.length and not e.line_bases):
                raise ValueError("%s line %d: impossible values" % (path, no))
            out.append(e)
    return out


def scan_fasta(fasta_path):
    """The .fai entries of a plain FASTA.  The name is the header's first whitespace-delimited word; the lines of a contig
    have one length (bases and bytes) except the last, which may be shorter; anything else raises ValueError."""
    entries, seen = [], set()
    name = None
    length = offset = line_bases = line_width = 0
    short_seen = False  # a line shorter than the contig's first was seen: no bases may follow it
    pos = 0

    def close():
        if name is not None:
            entries.append(FaiEntry(name, length, offset, line_bases, line_width))

    with open(fasta_path, "rb") as f:
        if f.read(2) == b"\x1f\x8b":
            raise ValueError("%s is compressed: index the uncompressed text" % fasta_path)
        f.seek(0)
        for raw in f:
            width = len(raw)
            if raw.startswith(b">"):
                close()
                words = raw[1:].split()
                if not words:
                    raise ValueError("%s: a header without a name at byte %d" % (fasta_path, pos))
                name = words[0].decode()
                if name in seen:
                    raise ValueError("%s: contig %s appears twice" % (fasta_path, name))
                seen.add(name)
                length, offset, line_bases, line_width, short_seen = 0, pos + width, 0, 0, False
            else:
                if name is None:
                    raise ValueError("%s does not start with '>'" % fasta_path)
                bases = len(raw.rstrip(b"\r\n"))
                if bases:
                    if short_seen:
                        raise ValueError("%s: contig %s has lines of different lengths (byte %d)" % (fasta_path, name, pos))
                    if not line_bases:
                        line_bases, line_width = bases, width
                    elif bases > line_bases or (bases == line_bases and width != line_width and width != bases):
                        raise ValueError("%s: contig %s has lines of different lengths (byte %d)" % (fasta_path, name, pos))
                    if bases < line_bases or width != line_width:
                        short_seen = True
                    length += bases
                else:
                    short_seen = True  # an empty line: only the contig's end may follow
            pos += width
    close()
    if not entries:
        raise ValueError("no sequences in %s" % fasta_path)
    return entries


def build_fai(fasta_path):
    """Write fasta_path + ".fai" for a plain FASTA (samtools faidx's rules) and return its entries."""
    entries = scan_fasta(fasta_path)
    out = os.fspath(fasta_path) + ".fai"
    tmp = out + ".tmp%d" % os.getpid()
    with open(tmp, "w") as f:
        for e in entries:
            f.write("%s\t%d\t%d\t%d\t%d\n" % e)
    os.replace(tmp, out)
    return entries

"""`fade annotate` with an index beside the FASTA (<fasta>.fai): the genome goes up through fadehip_genome_upload_fasta, and
stdout is byte for byte what the same command writes under FADE_FASTA_INDEX=0 (the whole-file loader) — SAM, BAM from the
device's file path, BAM from the host pipeline, two lanes — for the goldens' FASTA as committed, rewritten as 7-column CRLF lines
with the contigs reversed, and BGZF-compressed.  Every variant lies in a directory of its own under the same relative names,
so the command line (which the @PG header records) is the same everywhere."""
import gzip
import os
import subprocess

import pytest

import fasta_cases as FC
from fade_amd import fasta_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ("anno_c1", "anno_c2", "anno_c5")
VARIANTS = ("as_committed", "crlf7_reversed", "bgzf")
# (name, arguments in front of the two files, environment, input)
COMMANDS = (("sam", [], {}, "in.sam"), ("bam_device", ["-b"], {}, "in.bam"), ("bam_host", ["-b"], {"FADE_BAM_DEVICE": "0"}, "in.bam"),
            ("two_lanes", ["-b", "--gpus", "2"], {"FADE_DEVICE_MAP": "0,0"}, "in.bam"))


def _params(tag):
    for line in open(os.path.join(GOLD, tag + ".expected.tsv")):
        if line.startswith("#floor_len"):
            kv = dict(x.split("=") for x in line[1:].split())
            return ["--min-length", kv["floor_len"], "-w", kv["window"]]
    raise AssertionError(tag)


def _run(cwd, args, env=None):
    e = dict(os.environ)
    e.pop("FADE_FASTA_INDEX", None)
    e.update(env or {})
    return subprocess.run([FADE] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)


def _contigs_of(path):
    names, seqs = [], []
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode())
            seqs.append(b"")
        else:
            seqs[-1] += line
    return names, seqs


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """(tag, variant) -> directory holding in.sam, in.bam, ref.fa and ref.fa.fai."""
    out = {}
    for tag in TAGS:
        names, seqs = _contigs_of(os.path.join(GOLD, tag + ".fa"))
        sam = open(os.path.join(GOLD, tag + ".sam"), "rb").read()
        bam = None
        for v in VARIANTS:
            d = tmp_path_factory.mktemp("%s_%s" % (tag, v))
            (d / "in.sam").write_bytes(sam)
            if v == "as_committed":
                (d / "ref.fa").write_bytes(open(os.path.join(GOLD, tag + ".fa"), "rb").read())
                fasta_index.build_fai(str(d / "ref.fa"))
                p = _run(d, ["out", "-b", "in.sam"])
                assert p.returncode == 0, p.stderr.decode()[-2000:]
                bam = p.stdout
            else:
                contigs = [FC.Contig(n, s, 7, b"\r\n", True) for n, s in reversed(list(zip(names, seqs)))]
                text, entries = FC.fasta_text(contigs)
                if v == "bgzf":
                    (d / "ref.fa").write_bytes(b"".join(FC.bgzf_members(text, FC.odd_sizes(len(text)))))
                    FC.write_fai(d / "ref.fa.fai", entries)
                else:
                    (d / "ref.fa").write_bytes(text)
                    assert [tuple(e) for e in fasta_index.build_fai(str(d / "ref.fa"))] == [tuple(e) for e in entries]
            (d / "in.bam").write_bytes(bam)
            out[(tag, v)] = d
    return out


_whole_file = {}


def _reference(dirs, tag, cmd):
    """stdout of the command under FADE_FASTA_INDEX=0, on the FASTA as committed."""
    name, front, env, inp = cmd
    if (tag, name) not in _whole_file:
        p = _run(dirs[(tag, "as_committed")], ["annotate"] + _params(tag) + front + ["--timing", inp, "ref.fa"], dict(env, FADE_FASTA_INDEX="0"))
        assert p.returncode == 0 and p.stdout, p.stderr.decode()[-2000:]
        assert b"whole-file FASTA loader" in p.stderr and b"indexed FASTA path" not in p.stderr
        _whole_file[(tag, name)] = p.stdout
    return _whole_file[(tag, name)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tag", TAGS)
def test_stdout_is_what_the_whole_file_loader_gives(dirs, tag, variant):
    for cmd in COMMANDS:
        name, front, env, inp = cmd
        p = _run(dirs[(tag, variant)], ["annotate"] + _params(tag) + front + ["--timing", inp, "ref.fa"], env)
        assert p.returncode == 0, (name, p.stderr.decode()[-2000:])
        assert b"[timing] genome: indexed FASTA path" in p.stderr and b"whole-file FASTA loader" not in p.stderr, (name, p.stderr.decode()[-2000:])
        assert p.stdout == _reference(dirs, tag, cmd), (tag, variant, name)


def test_the_switch_and_plain_gzip_take_the_whole_file_loader(dirs, tmp_path):
    tag = "anno_c2"
    d = dirs[(tag, "crlf7_reversed")]
    args = ["annotate"] + _params(tag) + ["--timing", "in.sam", "ref.fa"]
    off = _run(d, args, {"FADE_FASTA_INDEX": "0"})
    assert off.returncode == 0 and b"whole-file FASTA loader" in off.stderr and b"indexed FASTA path" not in off.stderr
    assert off.stdout == _reference(dirs, tag, COMMANDS[0])
    (tmp_path / "in.sam").write_bytes((d / "in.sam").read_bytes())
    (tmp_path / "ref.fa").write_bytes(gzip.compress((d / "ref.fa").read_bytes()))
    (tmp_path / "ref.fa.fai").write_bytes((d / "ref.fa.fai").read_bytes())
    gz = _run(tmp_path, args)
    assert gz.returncode == 0 and b"whole-file FASTA loader" in gz.stderr, gz.stderr.decode()[-2000:]
    assert gz.stdout == off.stdout


def test_a_stale_index_ends_the_run(dirs, tmp_path):
    tag = "anno_c2"
    d = dirs[(tag, "as_committed")]
    for k in ("in.sam", "in.bam", "ref.fa"):
        (tmp_path / k).write_bytes((d / k).read_bytes())
    lines = (d / "ref.fa.fai").read_text().splitlines()
    f = lines[0].split("\t")
    f[4] = str(int(f[4]) + 1)  # a line width that is off by one
    (tmp_path / "ref.fa.fai").write_text("\n".join(["\t".join(f)] + lines[1:]) + "\n")
    for name, front, env, inp in COMMANDS:
        p = _run(tmp_path, ["annotate"] + _params(tag) + front + [inp, "ref.fa"], env)
        assert p.returncode == 1 and p.stdout == b"", (name, p.returncode, len(p.stdout), p.stderr.decode()[-2000:])
        assert b"ref.fa.fai" in p.stderr and b"index does not match the FASTA" in p.stderr, (name, p.stderr.decode()[-2000:])
    # contigs the header names must be in the index, and long enough there: today's two messages, word for word
    (tmp_path / "ref.fa.fai").write_text("\n".join(lines[1:]) + "\n")
    p = _run(tmp_path, ["annotate"] + _params(tag) + ["in.sam", "ref.fa"])
    assert p.returncode == 1 and p.stdout == b"" and b"of the BAM header is not in ref.fa" in p.stderr, p.stderr.decode()[-2000:]
    f = lines[0].split("\t")
    f[1] = str(int(f[1]) - 1)
    (tmp_path / "ref.fa.fai").write_text("\n".join(["\t".join(f)] + lines[1:]) + "\n")
    p = _run(tmp_path, ["annotate"] + _params(tag) + ["in.sam", "ref.fa"])
    assert p.returncode == 1 and p.stdout == b"" and b"is shorter in the FASTA (" in p.stderr, p.stderr.decode()[-2000:]

"""`fade out [-c] --gpus 1 -b / -u` and `fade extract --gpus 1 -b / -u` on BAM files: the file path on the device over records
annotated earlier (FADEHIP_BAM_FROM_TAGS) against the host loops of the same binary — the header, the records byte for byte,
the warnings and the stats block — with the device and with the host inflating, on the annotated golden sets (name-sorted and
shuffled), on 30,000 annotated reads in many calls, and on a BAM that holds a header and nothing else."""
import pytest

import samutil
from test_cli_extract import _annotated_sam
from test_gpu_annotate_clip import _bam_of, _ok, _run, _split
from test_gpu_annotate_eject import W_GROUPS, W_RECORDS
from test_gpu_bam_from_tags import SETS, _shuffled

pytestmark = pytest.mark.gpu

SUBS = {"out": ["out"], "out_c": ["out", "-c"], "extract": ["extract"]}
EOF_MEMBER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _said(err):
    """What a run printed beside its --timing lines."""
    return [l for l in err.decode().splitlines() if not l.startswith("[timing]")]


def _both(sub, fmt, bam, env=None):
    """(the host loop's run, [the device runs with the device and with the host inflating])"""
    host = _ok(_run(SUBS[sub] + [fmt, str(bam)]))
    assert b"file path on the device" not in host.stderr
    devs = []
    for inflate in ("device", "host"):
        e = dict(env or {}, FADE_BAM_INFLATE=inflate)
        p = _ok(_run(SUBS[sub] + ["--gpus", "1", "--timing", fmt, str(bam)], e))
        assert p.stderr.count(b"begins; file path on the device") == 1 and ("inflate on the %s" % inflate).encode() in p.stderr, p.stderr.decode()
        assert _said(p.stderr) == _said(host.stderr), inflate
        assert _split(p.stdout) == _split(host.stdout), inflate  # the header without @PG, the records byte for byte
        pg = [l for l in samutil.bam_to_sam_records(p.stdout)[0].splitlines() if l.startswith("@PG")]
        assert pg[-1].startswith("@PG\tID:fade-extract\tPN:fade") and " --gpus 1 " in pg[-1]
        assert p.stdout.endswith(EOF_MEMBER)
        devs.append(p)
    return host, devs


@pytest.fixture(scope="module", params=[(t, o) for t in SETS for o in ("sorted", "shuffled")], ids=lambda p: "%s-%s" % p)
def gold_bam(request, tmp_path_factory):
    tag, order = request.param
    d = tmp_path_factory.mktemp("outdev_%s_%s" % (tag, order))
    lines = _annotated_sam(tag).splitlines()
    if order == "shuffled":
        lines = _shuffled(lines)
    sam, bam = d / "anno.sam", d / "anno.bam"
    sam.write_text("\n".join(lines) + "\n")
    _bam_of(sam, bam)
    return order, bam


@pytest.mark.parametrize("sub", list(SUBS))
def test_golden_sets_every_subcommand_and_format_equals_the_host_loop(gold_bam, sub):
    order, bam = gold_bam
    for fmt in ("-b", "-u"):
        host, devs = _both(sub, fmt, bam)
        n_rec = len(samutil.bam_to_sam_records(host.stdout)[2])
        assert n_rec >= 6
        if sub == "out":
            mine, other = (W_GROUPS, W_RECORDS) if order == "sorted" else (W_RECORDS, W_GROUPS)
            assert all(p.stderr.count(mine) == 1 and other not in p.stderr for p in devs)
        if sub != "extract":
            assert all(p.stderr.count(b"read count:") == 1 and p.stderr.count(b"Artifact rate") == 3 for p in devs)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """The 30,000 reads of the eject test's `big` input (C5, names read<i // 2>: name-sorted pairs), annotated on the device:
    a BAM of ~130 BGZF members whose records carry rs and, the artifact calls, am."""
    from fade_amd import synth
    d = tmp_path_factory.mktemp("outdevbig")
    cfg, g, b = synth.make_config("C5", 30000, contig_len=400_000)
    names = ["read%d" % (i // 2) for i in range(len(b["pos"]))]
    b["qname"] = names
    sam, fa, bam, anno = d / "in.sam", d / "ref.fa", d / "in.bam", d / "anno.bam"
    sam.write_text(samutil.batch_to_sam(b, g.names, [int(x) for x in g.lengths], names))
    fa.write_bytes(g.fasta_bytes())
    bam.write_bytes(_ok(_run(["out", "-b", str(sam)])).stdout)
    anno.write_bytes(_ok(_run(["annotate", "-w", "100", "-b", str(bam), str(fa)])).stdout)
    assert len(anno.read_bytes()) > 100 * 20000  # (more than a hundred members)
    return anno


@pytest.mark.parametrize("sub", list(SUBS))
def test_30000_annotated_reads_in_many_calls_equal_the_host_loop(big, sub):
    host, devs = _both(sub, "-b", big, {"FADE_BAM_CHUNK_MB": "1"})
    n = len(samutil.bam_to_sam_records(host.stdout)[2])
    assert (1000 < n < 30000) if sub != "out_c" else n == 30000
    if sub == "out":
        assert all(p.stderr.count(W_GROUPS) == 1 for p in devs)


def test_a_bam_of_a_header_alone_gives_the_header_the_eof_member_and_nan_rates(tmp_path):
    sam, bam = tmp_path / "empty.sam", tmp_path / "empty.bam"
    sam.write_text("\n".join(l for l in _annotated_sam("anno_c1").splitlines() if l.startswith("@")) + "\n")
    _bam_of(sam, bam)
    for sub in SUBS:
        host, devs = _both(sub, "-b", bam)
        for p in devs:
            head, body = _split(p.stdout)
            assert len(head) >= 2 and samutil.bam_to_sam_records(p.stdout)[2] == []
            if sub != "extract":
                assert b"read count:\t0" in p.stderr and p.stderr.count(b"nan") == 6

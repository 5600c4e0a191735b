"""The device inflater (fade_amd/csrc/bgzf_inflate.hpp) on DEFLATE streams zlib would never write: the hand-built corpus of
tests/deflate_cases.py, each stream a BGZF member.  zlib's inflate decided every verdict and every byte (asserted by the
generator, on the CPU: tests/test_inflate_corpus.py, which also holds host/inflate_fast.hpp and the hts_lite reader to
the same corpus).  Valid streams must inflate to zlib's bytes at every byte alignment and wave slot they meet; every stream
zlib refuses must come back as an error status — incomplete code-length sets included, which the kernel used to take;
and the three inflaters of `fade annotate -b` must give one verdict on BAM files whose members the builder wrote.
Bytes behind the final block inside a member (zlib: fine, `unused_data`) are accepted by all three; whether htslib's
bgzf.c agrees was not checked."""
import gzip
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import fade_amd
import deflate_cases as C
from test_gpu_inflate import EOF_MARK, member

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")


def _extra(n):
    """A further gzip subfield of 4 + n bytes in front of BC: moves the DEFLATE stream by n bytes mod 4."""
    return b"XY" + struct.pack("<H", n) + bytes(range(1, n + 1))


def _first_difference(got, cases):
    """Name and offset of the first case whose bytes differ in a concatenated output."""
    at = 0
    for name, _, _, payload in cases:
        part = got[at:at + len(payload)]
        if part != payload:
            k = next((i for i in range(min(len(part), len(payload))) if part[i] != payload[i]), min(len(part), len(payload)))
            return "%s: first difference at offset %d of %d (output offset %d)" % (name, k, len(payload), at + k)
        at += len(payload)
    return "lengths differ: %d bytes came out, %d expected" % (len(got), at)


def test_valid_streams_inflate_to_zlibs_bytes(ctx):
    t0 = time.perf_counter()
    valid = C.valid_cases()
    compared = 0
    # every case as the only member of a call, its stream at byte alignment k mod 4; the streams whose codes run over
    # several turns of the reader's 256-byte window at all four
    for k, (name, raw, _, payload) in enumerate(valid):
        many = name.startswith(("codes_of_", "stored_block_after_", "300_blocks", "500_empty", "200_stored"))
        for n in (range(4) if many else (k % 4,)):
            try:
                got = ctx.bgzf_inflate(member(payload, raw=raw, extra=_extra(n))).tobytes()
            except fade_amd.FadeHipError as e:
                raise AssertionError("%s (stream moved by %d bytes): refused, zlib inflates it: %s" % (name, n, e))
            assert got == payload, "%s (stream moved by %d bytes): %s" % (name, n, _first_difference(got, [valid[k]]))
        compared += 1
    assert compared == len(valid)
    # all of them in one call, in three orders: other alignments, other wave slots, other neighbours
    rng = np.random.default_rng(31)
    orders = [list(range(len(valid))), list(range(len(valid)))[::-1], rng.permutation(len(valid)).tolist()]
    for order in orders:
        cases = [valid[k] for k in order]
        stream = b"".join(member(payload, raw=raw, extra=_extra((k + j) % 4) if (k + j) % 5 else b"") for j, (k, (_, raw, _, payload)) in enumerate(zip(order, cases)))
        want = b"".join(c[3] for c in cases)
        try:
            got = ctx.bgzf_inflate(stream + EOF_MARK, out_cap=len(want) + 65536).tobytes()
        except fade_amd.FadeHipError as e:
            raise AssertionError("a call of %d valid members was refused: %s" % (len(cases), e))
        assert got == want, _first_difference(got, cases)
        assert len(cases) == len(valid)
    print("%d valid cases, each alone and in 3 orders of one call: %.1f s" % (compared, time.perf_counter() - t0))


def test_invalid_streams_are_refused(ctx):
    t0 = time.perf_counter()
    invalid = C.invalid_cases()
    good = member(b"a good member in front")
    taken = []
    for name, raw, verdict, claimed in invalid:
        try:
            ctx.bgzf_inflate(good + member(claimed, raw=raw))
            taken.append(name)
        except fade_amd.FadeHipError:
            pass
    assert not taken, "the device takes %d of %d streams that zlib refuses: %s" % (len(taken), len(invalid), ", ".join(taken))
    # and the context still works
    name, raw, _, payload = C.valid_cases()[0]
    assert ctx.bgzf_inflate(good + member(payload, raw=raw)).tobytes() == b"a good member in front" + payload
    print("%d invalid cases refused: %.1f s" % (len(invalid), time.perf_counter() - t0))


def test_the_three_inflaters_agree_through_the_file_path(tmp_path):
    """The hand-built BAM files of deflate_cases.handbuilt_bams through `fade annotate -b` with each of the three inflaters.
    Valid files: the output must be, byte for byte, what the host pipeline with zlib's inflate (FADE_BGZF_CODEC=zlib)
    makes of the same records in a BAM that zlib wrote.  Invalid files: a non-zero exit with the INFLATER's message — the
    record parser refusing what a lenient inflater handed it does not pass, and six of the files carry real records
    behind the fault, so that a lenient inflater would make the run succeed.  With the device inflating, the faulty member
    is put behind 17 MiB of good members: the reader that fetches the header inflates a file's first 16 MiB on the host."""
    t0 = time.perf_counter()
    sam, valid, invalid, n_members, zlib_written, (header_len, padding) = C.handbuilt_bams(tmp_path)
    rng = np.random.default_rng(41)
    fa = tmp_path / "ref.fa"
    genome = "".join("ACGT"[k] for k in rng.integers(0, 4, 20000))
    fa.write_text(">chr1\n" + "\n".join(genome[o:o + 70] for o in range(0, len(genome), 70)) + "\n")
    host_message = b"does not inflate to its ISIZE / CRC32"  # hts_lite.hpp's reader and fade_main.cpp's pool
    envs = {"device": ({"FADE_BAM_INFLATE": "device"}, b"members failed)"),  # fadehip_bam.hip: "bam stream: call .., member ..: <INF_E_*> (.. members failed)"
            "host pool": ({"FADE_BAM_INFLATE": "host"}, host_message),
            "host pipeline": ({"FADE_BAM_DEVICE": "0"}, host_message)}

    def run(bam, env, far=False):
        # (every file under one name: the @PG line of the output's header holds the command line)
        one = tmp_path / "in.bam"
        data = bam.read_bytes()
        one.write_bytes(data[:header_len] + padding + data[header_len:] if far else data)
        return subprocess.run([FADE, "annotate", "-w", "100", "-b", str(one), str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                              env=dict(os.environ, **env))

    p = run(zlib_written, {"FADE_BAM_DEVICE": "0", "FADE_BGZF_CODEC": "zlib"})
    assert p.returncode == 0, p.stderr.decode()[-1500:]
    reference = gzip.decompress(p.stdout)
    assert reference.count(b"read") >= 300
    for name, bam in valid.items():
        for who, (env, _) in envs.items():
            p = run(bam, env)
            assert p.returncode == 0, (name, who, p.stderr.decode()[-1500:])
            assert gzip.decompress(p.stdout) == reference, "%s: inflate on the %s gives other records than zlib" % (name, who)
    for name, bam in invalid.items():
        for who, (env, message) in envs.items():
            # (with the device inflating, the faulty member lies beyond the 16 MiB that the header's reader inflates on the
            # host: the verdict is the kernel's)
            p = run(bam, env, far=who == "device")
            assert p.returncode != 0, "%s: `fade annotate` with inflate on the %s takes a member zlib refuses" % (name, who)
            assert message in p.stderr, "%s: inflate on the %s: the run failed, but not by the inflater's verdict: %s" % (name, who, p.stderr.decode()[-400:])
    print("%d valid files (%d hand-built members) and %d invalid files through 3 inflaters: %.1f s" % (len(valid), n_members, len(invalid), time.perf_counter() - t0))

"""The two CPU inflaters on DEFLATE streams zlib would never write (tests/deflate_builder.py, tests/deflate_cases.py):
host/inflate_fast.hpp (`FastInflate::inflate`, the lock-step `inflate2`) through csrc/build/inflate_corpus under ASan +
UBSan, and the hts_lite reader through `fade out` on BAM files whose record members were re-encoded by the builder.  The
reference for every verdict and every byte is zlib's inflate; nothing is compared with what the code under test
returned earlier.  tests/test_gpu_inflate_handbuilt.py holds the device kernel to the same corpus."""
import os
import struct
import subprocess
import zlib

import numpy as np

import deflate_builder as B
import deflate_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
FADE = os.path.join(ROOT, "fade_amd", "fade")
INFLATE_MESSAGE = b"does not inflate to its ISIZE / CRC32"  # hts_lite.hpp's BgzfIn: the inflater's verdict, not the record parser's


def test_builder_writes_what_zlib_reads():
    """The writer's own parts against zlib: canonical codes, the three block kinds, every way of run-length coding a
    header, explicit length / distance symbols."""
    assert B.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]  # RFC 1951 3.2.2's example
    assert B.complete_shape(5) == [2, 2, 2, 3, 3] and B.kraft_left(B.complete_shape(24, 15)) == 0
    for n, longest in ((16, 15), (286, 15), (30, 9), (19, 7), (8, 7), (2, 1)):
        shape = B.complete_shape(n, longest)
        assert len(shape) == n and max(shape) == longest and B.kraft_left(shape) == 0
    for length in range(3, 259):
        s, x, v = B.length_symbol(length)
        assert B.LBASE[s - 257] + v == length and v < (1 << x) + (x == 0)
    for dist in (1, 2, 3, 4, 5, 7, 8, 24576, 24577, 32767, 32768):
        s, x, v = B.dist_symbol(dist)
        assert B.DBASE[s] + v == dist and v < (1 << x) + (x == 0)
    data = b"it was the best of times, it was the worst of times"
    lit = B.assign(286, sorted(set(data)) + [256, 259, 285], B.complete_shape(len(set(data)) + 3, 9))
    for rle in ("none", "greedy", "long"):
        s = B.Stream().stored(data[:7]).fixed(list(data[7:20]) + [(5, 3)]).dynamic(list(data) + [(5, 4), (258, 1)], True, lit, [2, 2, 2, 2], rle=rle)
        v = B.expected(s.raw())
        assert v[0] == "ok" and v[1] == bytes(s.payload) and v[2] == b"", rle
    assert B.expected(B.Stream().fixed(list(data), False).raw())[0] == "truncated"
    assert B.expected(B.Stream().reserved().raw())[0] == "error"


def test_zlib_takes_every_valid_case_and_refuses_every_invalid_one():
    valid, invalid = C.valid_cases(), C.invalid_cases()  # (the assertions are the generator's own)
    names = [c[0] for c in valid]
    assert sum(n.startswith("random_") for n in names) == C.N_RANDOM_MEMBERS
    for want in (["hclen_%d" % k for k in range(5, 20)] + ["codes_of_%d_bits" % k for k in (9, 10, 11, 12, 15)] +
                 ["%s_header_at_bit_%d" % (k, a) for k in ("stored", "fixed", "dynamic") for a in range(8)] +
                 ["final_end_of_block_ends_at_bit_%d" % a for a in range(8)] +
                 ["pending_%d_then_%s" % (n, w) for n in (0, 1, 63, 64, 65) for w in ("stored", "match", "end")] +
                 ["size_%d" % n for n in (0, 1, 63, 64, 65)] +
                 ["size_%d_%s" % (n, w) for n in (65280, 65535, 65536) for w in ("literals_only", "one_literal_and_matches", "stored_blocks")]):
        assert want in names, want
    for name, raw, verdict, payload in valid:
        assert verdict == "ok" and zlib.decompressobj(-15).decompress(raw) == payload, name
    for name, raw, verdict, claimed in invalid:
        assert verdict in ("error", "truncated"), name
    print("%d valid cases (%d named, %d from the random composer), %d invalid cases" % (
        len(valid), len(valid) - C.N_RANDOM_MEMBERS, C.N_RANDOM_MEMBERS, len(invalid)))


def write_corpus(path, cases):
    with open(path, "wb") as f:
        f.write(b"FCRP" + struct.pack("<I", len(cases)))
        for name, raw, verdict, payload in cases:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm + struct.pack("<I", len(raw)) + raw)
            f.write(struct.pack("<II", 1 if verdict == "ok" else 0, len(payload)) + payload)


def test_inflate_fast_on_the_whole_corpus_under_sanitizers(tmp_path):
    """FastInflate::inflate (exact output size between guard bytes; out_len one less and one more must fail) and
    FastInflate::inflate2 (the case as either stream, against itself, the previous case and a stored-only stream) on
    every valid and every invalid case: 0 failures."""
    subprocess.run(["make", "-s", "-C", CSRC, "build/inflate_corpus"], check=True, timeout=600)
    cases = list(C.valid_cases()) + list(C.invalid_cases())
    # interleave the invalid cases with the valid ones, so that "the previous case" is of the other kind as well
    mixed, inv = [], list(C.invalid_cases())
    for k, c in enumerate(C.valid_cases()):
        mixed.append(c)
        if k % 9 == 4 and inv:
            mixed.append(inv.pop(0))
    mixed += inv
    assert len(mixed) == len(cases)
    corpus = tmp_path / "corpus.bin"
    write_corpus(corpus, mixed)
    p = subprocess.run([os.path.join(CSRC, "build", "inflate_corpus"), str(corpus)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out = p.stdout.decode()
    print(out[-3000:])
    assert p.returncode == 0, out[-6000:] + p.stderr.decode()[-3000:]
    assert "%d valid and %d invalid cases" % (len(C.valid_cases()), len(C.invalid_cases())) in out and ": 0 failures" in out


def test_hts_lite_reader_on_handbuilt_members(tmp_path):
    """`fade out` must reproduce the records of every valid file and exit non-zero with its corrupt-member message on every
    invalid one (the inflater's message: a lenient inflater whose bytes the record parser then refuses does not pass), with
    inflate_fast.hpp (FADE_BGZF_CODEC=fast) and, as a check of the test itself, with zlib."""
    sam, valid, invalid, n_members, _, _ = C.handbuilt_bams(tmp_path)
    strip = lambda t: [l for l in t.decode().splitlines() if not l.startswith("@PG")]
    q = subprocess.run([FADE, "out", "-t", "2", str(sam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert q.returncode == 0 and len(strip(q.stdout)) == 300 + 2
    for codec in ("fast", "zlib"):
        env = dict(os.environ, FADE_BGZF_CODEC=codec)
        for name, bam in valid.items():
            r = subprocess.run([FADE, "out", "-t", "2", str(bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
            assert r.returncode == 0, (codec, name, r.stderr.decode()[-500:])
            assert strip(r.stdout) == strip(q.stdout), (codec, name)
        for name, bam in invalid.items():
            r = subprocess.run([FADE, "out", "-t", "2", str(bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
            assert r.returncode != 0 and INFLATE_MESSAGE in r.stderr, (codec, name, r.returncode, r.stderr.decode()[-300:])
    print("%d valid files (%d hand-built members), %d invalid files, each through FADE_BGZF_CODEC=fast and =zlib" % (len(valid), n_members, len(invalid)))

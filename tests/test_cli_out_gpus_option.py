"""`fade out [-c] --gpus 1` and `fade extract --gpus 1`, the part that needs no device: the option is accepted, SAM input and
FADE_BAM_DEVICE=0 take the host loops (whose output the option must not change), and more than one device is refused."""
import os
import subprocess

import pytest

from test_cli_extract import _annotated_sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FADE = os.path.join(ROOT, "fade_amd", "fade")


@pytest.fixture(scope="module")
def anno(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build()
    d = tmp_path_factory.mktemp("out_gpus")
    sam, bam = d / "in.sam", d / "in.bam"
    sam.write_text(_annotated_sam("anno_c2"))
    with open(bam, "wb") as fo:
        subprocess.check_call([os.path.join(ROOT, "tools", "sam2bam"), str(sam)], stdout=fo)
    return sam, bam


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([FADE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)


def _no_pg(out):
    return [l for l in out.decode().splitlines() if not l.startswith("@PG")]


@pytest.mark.parametrize("sub", [["out"], ["out", "-c"], ["extract"]], ids=["out", "out_c", "extract"])
def test_gpus_1_on_sam_input_prints_what_the_host_loop_prints(anno, sub):
    sam, _ = anno
    plain, with_opt = _run(sub + [str(sam)]), _run(sub + ["--gpus", "1", str(sam)])
    assert plain.returncode == 0 and with_opt.returncode == 0, with_opt.stderr.decode()
    assert _no_pg(with_opt.stdout) == _no_pg(plain.stdout) and len(_no_pg(plain.stdout)) > 20
    assert with_opt.stderr == plain.stderr and b"device" not in with_opt.stderr
    assert any("--gpus 1" in l for l in with_opt.stdout.decode().splitlines() if l.startswith("@PG"))
    # --gpus=1 and a SAM output of a BAM file take the host loop too
    assert _no_pg(_run(sub + ["--gpus=1", str(sam)]).stdout) == _no_pg(plain.stdout)
    assert _no_pg(_run(sub + ["--gpus", "1", str(anno[1])]).stdout) == _no_pg(plain.stdout)


@pytest.mark.parametrize("sub", [["out"], ["out", "-c"], ["extract"]], ids=["out", "out_c", "extract"])
def test_more_than_one_device_is_refused_by_name(anno, sub):
    for n in ("2", "8", "0"):
        p = _run(sub + ["--gpus", n, "-b", str(anno[1])])
        assert p.returncode == 1 and p.stdout == b"" and b"--gpus" in p.stderr, p.stderr.decode()
    p = _run(sub + ["--gpus", "two", str(anno[0])])
    assert p.returncode == 1 and b"Invalid value for option --gpus" in p.stderr


@pytest.mark.parametrize("fmt", ["-b", "-u"])
@pytest.mark.parametrize("sub", [["out"], ["out", "-c"], ["extract"]], ids=["out", "out_c", "extract"])
def test_fade_bam_device_0_is_the_host_loop_byte_for_byte(anno, sub, fmt):
    _, bam = anno
    import gzip
    host = _run(sub + [fmt, str(bam)])
    off = _run(sub + ["--gpus", "1", fmt, str(bam)], {"FADE_BAM_DEVICE": "0"})
    assert host.returncode == 0 and off.returncode == 0, off.stderr.decode()
    assert off.stderr == host.stderr and b"file path on the device" not in off.stderr

    def split(out):
        raw = gzip.decompress(out)
        l_text = int.from_bytes(raw[4:8], "little")
        return [l for l in raw[8:8 + l_text].decode().splitlines() if not l.startswith("@PG")], raw[8 + l_text:]

    assert split(off.stdout) == split(host.stdout) and len(split(host.stdout)[1]) > 1000

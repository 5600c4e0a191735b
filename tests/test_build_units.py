"""The cut of libfadehip.so into translation units ("Translation units"), from source text and the build's
logs: every device header belongs to one unit, and no kernel is compiled twice.  No GPU here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fade_amd", "csrc")
DEVICE_HEADERS = ("fadehip_kernels.hpp", "sw_stats.hpp", "bam_device.hpp", "bgzf_deflate.hpp", "bgzf_inflate.hpp")


def _units():
    return sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))


def test_device_headers_and_kernels_belong_to_one_unit():
    import __graft_entry__ as ge
    ge.build()
    units = _units()
    assert len(units) >= 4, units
    includes = {u: set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, u + ".hip")).read(), flags=re.M)) for u in units}
    for h in DEVICE_HEADERS:
        assert os.path.exists(os.path.join(CSRC, h)), h
        owners = [u for u in units if h in includes[u]]
        assert len(owners) == 1, "%s is included by %s" % (h, owners or "no unit")
    for u in units:
        assert "fadehip_host.hpp" in includes[u], u
    # the unit of the context (it fills c_ascii_code through the alignment unit, never itself) includes no header with a kernel
    ctx_units = [u for u in units if re.search(r"^int fadehip_create\(", open(os.path.join(CSRC, u + ".hip")).read(), flags=re.M)]
    assert len(ctx_units) == 1 and not includes[ctx_units[0]] & set(DEVICE_HEADERS), ctx_units
    seen = {}  # kernel -> the unit whose log names it
    for u in units:
        log = os.path.join(CSRC, "build", u + ".log")
        assert os.path.exists(log), "the build left no log for %s.hip" % u
        for name in re.findall(r"Function Name: (\S+)", open(log).read()):
            assert name not in seen, "%s is compiled in %s.hip and in %s.hip" % (name, seen[name], u)
            seen[name] = u
    assert ctx_units[0] not in seen.values()
    assert len(seen) >= 100, len(seen)  # (the logs do carry the remarks)

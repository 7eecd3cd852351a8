"""Progressive rendering, CPU side: the header, the ctypes binding and the Rust `-sys` crate agree on rtg_params.sample_begin
and the two flags, and rtg_params keeps its size and layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
SYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")


def _header_flags():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", open(HEADER).read())}


def test_header_declares_the_flags_and_the_field():
    flags = _header_flags()
    assert flags["RTG_FLAG_PARTIAL"] == 4 and flags["RTG_FLAG_RESUME"] == 8
    assert len(set(flags.values())) == len(flags), flags   # one bit each
    body = re.search(r"typedef struct rtg_params \{(.*?)\} rtg_params;", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S),
                     flags=re.S).group(1)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls[-1] == ["uint32_t", "sample_begin"], decls[-1]   # where `reserved` was
    assert "reserved" not in body


def test_capi_matches_the_header(pkg):
    capi = pkg.capi
    flags = _header_flags()
    assert capi.FLAG_PARTIAL == flags["RTG_FLAG_PARTIAL"] and capi.FLAG_RESUME == flags["RTG_FLAG_RESUME"]
    assert capi.FLAG_COUNTERS == flags["RTG_FLAG_COUNTERS"] and capi.FLAG_TRACE_KERNEL == flags["RTG_FLAG_TRACE_KERNEL"]
    assert C.sizeof(capi.Params) == 56
    assert capi.Params.sample_begin.offset == 52 and capi.Params.flags.offset == 48
    assert [f for f, _ in capi.Params._fields_][-1] == "sample_begin"


def test_rust_sys_crate_matches_the_header():
    rs = open(SYS_RS).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (RTG_FLAG_[A-Z_]+): u32 = (\d+);", rs)}
    for name, value in _header_flags().items():
        assert consts.get(name) == value, (name, consts.get(name), value)
    rs_body = re.search(r"pub struct rtg_params \{(.*?)\n\}", re.sub(r"//[^\n]*", "", rs), flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", rs_body)[-2:] == ["flags", "sample_begin"]


def test_make_params_sets_the_slice(pkg):
    capi = pkg.capi
    p = capi.make_params(64, 32, 10)
    assert p.flags == 0 and p.sample_begin == 0
    p = capi.make_params(64, 32, 10, sample_begin=4, resume=True, partial=True, flags=capi.FLAG_COUNTERS)
    assert p.flags == capi.FLAG_COUNTERS | capi.FLAG_PARTIAL | capi.FLAG_RESUME and p.sample_begin == 4 and p.ns == 10
    p = capi.make_params(64, 32, 10, partial=True)
    assert p.flags == capi.FLAG_PARTIAL


def test_resume_without_a_running_sum_is_refused_on_the_host(pkg):
    """resume=True with sample_begin > 0 and no out= has nothing to continue: refused before the library is called."""
    import pytest
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            pass
    with pytest.raises(ValueError):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, sample_begin=2, resume=True)

"""Ray queries, CPU side (include/rtiow_gpu_query.h): the header declares exactly its four entry points and the library exports
them; they stay out of the ABI of rtiow_gpu.h and of its mirrors; the params struct in the binding; the scene option; and the
refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ["query_closest", "query_closest_device", "query_occluded", "query_occluded_device"]
ERR_INVALID = -1


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return re.findall(r"\b(rtg_\w+)\s*\(", text)


def test_the_header_declares_exactly_the_four_entry_points(pkg):
    assert sorted(_declared(os.path.join(INCLUDE, "rtiow_gpu_query.h"))) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.QUERY_SYMBOLS == NAMES
    text = open(os.path.join(INCLUDE, "rtiow_gpu_query.h")).read()
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text


def test_the_library_exports_them(pkg):
    be = pkg.load()
    for n in NAMES:
        assert hasattr(be.lib, "rtg_" + n), n


def test_they_stay_out_of_the_abi_and_its_mirrors(pkg):
    capi = pkg.capi
    assert len(capi.ABI_SYMBOLS) == 42 and not set(NAMES) & set(capi.ABI_SYMBOLS)
    main = open(os.path.join(INCLUDE, "rtiow_gpu.h")).read()
    rs = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")).read()
    for n in NAMES + ["rtg_query_params"]:
        assert n not in main and n not in rs, n
    assert len(set(_declared(os.path.join(INCLUDE, "rtiow_gpu.h")))) == 42


def test_params_struct(pkg):
    Q = pkg.capi.QueryParams
    assert C.sizeof(Q) == 32
    assert [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("struct_size", 0), ("reserved", 4), ("seed", 8), ("first_index", 16),
                                                                   ("t_min", 24), ("reserved2", 28)]
    body = re.search(r"typedef struct rtg_query_params \{(.*?)\} rtg_query_params;", open(os.path.join(INCLUDE, "rtiow_gpu_query.h")).read(), re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t|float) (\w+);", body, re.M)
    assert fields == [("uint32_t", "struct_size"), ("uint32_t", "reserved"), ("uint64_t", "seed"), ("uint64_t", "first_index"),
                      ("float", "t_min"), ("uint32_t", "reserved2")]
    p = pkg.capi.make_query_params(seed=5, t_min=0.25, first_index=7)
    assert (p.struct_size, p.reserved, p.seed, p.first_index, p.t_min, p.reserved2) == (32, 0, 5, 7, 0.25, 0)


def test_scene_option(pkg):
    assert "query_lds" in pkg.capi.Scene.ENV_OPTIONS


def test_a_null_scene_is_refused(pkg):
    be = pkg.load()
    p = pkg.capi.make_query_params()
    rays = np.zeros((2, 8), np.float32)
    out, mat, occ = np.full((2, 8), 7, np.float32), np.full(2, 7, np.uint32), np.full(2, 7, np.uint8)
    assert be._query_closest(None, 2, rays.ctypes.data, C.byref(p), out.ctypes.data, mat.ctypes.data, None) == ERR_INVALID
    assert be._query_closest_device(None, 2, rays.ctypes.data, C.byref(p), out.ctypes.data, mat.ctypes.data, None, None) == ERR_INVALID
    assert be._query_occluded(None, 2, rays.ctypes.data, C.byref(p), occ.ctypes.data, None) == ERR_INVALID
    assert be._query_occluded_device(None, 2, rays.ctypes.data, C.byref(p), occ.ctypes.data, None, None) == ERR_INVALID
    assert "null" in be.last_error()
    assert (out == 7).all() and (mat == 7).all() and (occ == 7).all()

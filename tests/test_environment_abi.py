"""The scene's environment, CPU side (include/rtiow_gpu_environment.h; Builder.environment; environment.py): the header declares
exactly its four entry points with the prototypes the binding and the Rust module give them, and they stay out of the ABI of
rtiow_gpu.h; the refusals, clear and replace; a builder without an environment flattens to the words it always did; the host
probe against the numpy definition, bit for bit; the Radiance reader and writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
import environment_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu_environment.h")
ENV_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "environment.rs")
NAMES = ["builder_set_environment", "builder_get_environment", "debug_environment_host", "debug_environment"]
INVALID_ID = 0xFFFFFFFF
FEAT_TEXTURE, FEAT_ENVIRONMENT, FEAT_NOT_LEAN = 8, 4096, 1 | 2 | 4 | 8 | 16 | 1024   # csrc/flat_scene.h, csrc/rtg_kernels.inc
ERR_INVALID, ERR_UNSUPPORTED = -1, -5   # include/rtiow_gpu.h
f32 = np.float32
SEED = 0xDEADBEEF


def _prototypes(text, strip, pattern):
    text = re.sub(strip, "", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()] for m in re.finditer(pattern, text, flags=re.S)}


def test_the_header_declares_exactly_the_four_entry_points(pkg):
    text = open(HEADER).read()
    c_fns = _prototypes(text, r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    assert sorted(c_fns) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.ENVIRONMENT_SYMBOLS == NAMES
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_builder_set_environment"]] == ["b", "p"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_builder_get_environment"]] == ["b", "out", "sin_cos[2]"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_debug_environment_host"]] == ["b", "n", "d", "out"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_debug_environment"]] == ["s", "n", "d", "out"]
    # the parameter block, field for field, and the binding's copy of it: size and offsets as declared
    block = re.search(r"typedef struct rtg_environment_params \{(.*?)\} rtg_environment_params;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = [f.strip().split()[-1] for part in block.split(";") for f in part.split(",") if f.strip()]
    assert fields == ["struct_size", "texture", "scale[3]", "rotate_y_degrees", "reserved_in[2]"]
    P = pkg.capi.EnvironmentParams
    assert [n for n, _ in P._fields_] == ["struct_size", "texture", "scale", "rotate_y_degrees", "reserved_in"]
    assert C.sizeof(P) == 32
    assert [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 20, 24]


def test_the_library_exports_them_with_the_binding_s_prototypes(pkg):
    be = pkg.load()
    for n, argc in zip(NAMES, (2, 3, 4, 4)):
        fn = getattr(be.lib, "rtg_" + n)
        assert fn.restype is C.c_int and len(fn.argtypes) == argc, n
    assert be.lib.rtg_builder_set_environment.argtypes[1] is C.POINTER(pkg.capi.EnvironmentParams)


def test_they_stay_out_of_the_abi_and_the_rust_module_follows_the_header(pkg):
    capi = pkg.capi
    for other in (capi.ABI_SYMBOLS, capi.QUERY_SYMBOLS, capi.RAY_FRAME_SYMBOLS, capi.IMAGE_SYMBOLS, capi.MESH_SYMBOLS, capi.SURFACE_SYMBOLS):
        assert not set(NAMES) & set(other)
    main = open(os.path.join(ROOT, "include", "rtiow_gpu.h")).read()
    assert "rtg_builder_set_environment" not in main and "rtg_environment_params" not in main and "rtg_debug_environment" not in main
    c_fns = _prototypes(open(HEADER).read(), r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    rs_fns = _prototypes(open(ENV_RS).read(), r"//[^\n]*", r"pub fn (rtg_\w+)\s*\(([^)]*)\)")
    assert sorted(rs_fns) == sorted(c_fns)
    for name in c_fns:
        assert len(rs_fns[name]) == len(c_fns[name]), name
    lib_rs = open(os.path.join(os.path.dirname(ENV_RS), "lib.rs")).read()
    assert "pub mod environment;" in lib_rs
    for n in NAMES:
        assert "rtg_" + n not in lib_rs, n


# ---- flattenings ---------------------------------------------------------------------------------------------------------------
def _flat(b, world):
    """Everything rtg_debug_flatten and rtg_debug_flatten_pool2 say about the world: program words, feature word, the second
    program's words and table.  (The material and texture words ride in no probe of their own; the feature word's albedo bits are
    made from them.)"""
    words, feats = b.flatten(world)
    p2 = b.flatten_pool2(world)
    return dict(words=np.asarray(words).copy(), features=int(feats), p2=[np.asarray(x).copy() for x in p2])


def _same_flat(a, b):
    return a["features"] == b["features"] and np.array_equal(a["words"], b["words"]) and len(a["p2"]) == len(b["p2"]) and all(
        np.array_equal(x, y) for x, y in zip(a["p2"], b["p2"]))


def _get(b):
    e = b.get_environment()
    return (e["texture"], tuple(bits(e["scale"]).tolist()), bits(f32(e["rotate_y"])).item(), bits(e["s"]).item(), bits(e["c"]).item())


def _worlds(pkg):
    S = pkg.scenes
    return {"cornell": lambda b: S.cornell_box_scene(b, 32, 32)[0],
            "book1": lambda b: S.random_scene(b, 48, 32)[0],
            "book2": lambda b: S.book_final_scene(b, 32, 32, pkg.small_rng.SmallRng(SEED))[0],
            "mesh": lambda b: S.cornell_surface_scene(b, 32, 32)[0]}


def test_every_refusal_leaves_the_builder_as_it_was(pkg):
    be = pkg.load()
    I, P = pkg.image, pkg.capi.EnvironmentParams
    b = be.builder()
    world = pkg.scenes.random_scene(b, 48, 32)[0]
    con = b.constant((0.1, 0.2, 0.3))
    img = b.image(EC.image((5, 3)), I.spherical())
    surf = b.surface(img)
    n_tex = surf + 1

    def refused(p, builder=b.h):
        rc = be._builder_set_environment(builder, None if p is None else C.byref(p))
        return rc == ERR_INVALID and be.last_error() != ""

    def all_refusals():
        p = P.new(con)
        p.struct_size -= 4
        assert refused(p)
        p = P.new(con)
        p.struct_size += 4
        assert refused(p)
        for i in (0, 1):
            p = P.new(con)
            p.reserved_in[i] = 1
            assert refused(p), i
            p = P.new(None)            # ... a clear with reserved_in set is refused too
            p.reserved_in[i] = 7
            assert refused(p), i
        assert refused(P.new(n_tex)) and refused(P.new(10 ** 6)) and refused(P.new(INVALID_ID - 1))   # out of range
        assert refused(P.new(img + 1))                                       # an image's continuation slot
        assert refused(P.new(surf))                                          # a miss has no surface coordinates
        for deg in (np.inf, -np.inf, np.nan):
            assert refused(P.new(con, rotate_y=deg)), deg
        assert refused(None) and refused(P.new(con), builder=None)

    # on a builder without an environment: nothing appears
    before, flat0 = _get(b), _flat(b, world)
    assert before[0] is None
    all_refusals()
    assert _get(b) == before and _same_flat(_flat(b, world), flat0)
    # on a builder with one: it stays, bit for bit
    b.environment(img, scale=(0.5, 2.0, 3.0), rotate_y=33.3)
    before, flat1 = _get(b), _flat(b, world)
    assert before[0] == img and not _same_flat(flat1, flat0)
    all_refusals()
    assert _get(b) == before and _same_flat(_flat(b, world), flat1)
    # no texture was made or lost on the way
    assert b.constant((0.0, 0.0, 0.0)) == n_tex


def test_get_reports_what_was_set_and_the_pair_of_rotate_y(pkg):
    be = pkg.load()
    b = be.builder()
    e = b.get_environment()
    assert e["texture"] is None and e["struct_size"] == 32 and tuple(e["scale"]) == (1.0, 1.0, 1.0) and e["rotate_y"] == 0.0
    assert (float(e["s"]), float(e["c"])) == (0.0, 1.0)
    con = b.constant((1.0, 1.0, 1.0))
    for deg in EC.ROTATIONS + [1e-3, 720.5, -1e6]:
        for scale in EC.SCALES:
            b.environment(con, scale=scale, rotate_y=deg)
            e = b.get_environment()
            assert e["texture"] == con and e["rotate_y"] == float(f32(deg))
            assert_bit_equal(e["scale"], np.array(scale, f32))
            # the very pair rtg_object_rotate_y makes: read it back from the flattened PUSH record of a rotated sphere
            words, _ = b.flatten([b.rotate_y(deg, b.sphere(1.0, b.lambertian(con)))])
            push = np.asarray(words).reshape(-1, 8)[0]
            assert (push[7] & 0xff) == 4                                      # OP_PUSH: lo = (sin, cos, -, -)
            assert (int(push[0]), int(push[1])) == (bits(e["s"]).item(), bits(e["c"]).item()), deg
    s0, c0 = b.get_environment()["s"], b.get_environment()["c"]
    assert b.get_environment()["rotate_y"] == float(f32(-1e6)) and abs(float(s0) ** 2 + float(c0) ** 2 - 1.0) < 1e-6
    b.environment(None)
    assert b.get_environment()["texture"] is None


@pytest.mark.parametrize("name", ["cornell", "book1", "book2", "mesh"])
def test_no_change_without_it_and_the_new_bit_with_it(pkg, name):
    """Before any environment call, and again after set-then-clear: the program words, the feature word and the second program
    the builder always gave.  With an environment: the new bit and FEAT_TEXTURE, no second program, not a lean program -- and the
    same program records otherwise (book-1 gains nothing but, where the world has one, a hoisted-segment record)."""
    be = pkg.load()
    b = be.builder()
    world = _worlds(pkg)[name](b)
    flat0 = _flat(b, world)
    assert not flat0["features"] & FEAT_ENVIRONMENT
    con = b.constant((0.25, 0.5, 1.0))
    img = b.image(EC.image((8, 4)), pkg.image.spherical())
    flat_tex = _flat(b, world)     # (textures nobody refers to change no word)
    assert _same_flat(flat_tex, flat0)
    for tex in (con, img):
        b.environment(tex, scale=(1.0, 0.5, 2.0), rotate_y=33.3)
        with_env = _flat(b, world)
        assert with_env["features"] & FEAT_ENVIRONMENT and with_env["features"] & FEAT_TEXTURE
        assert with_env["features"] & FEAT_NOT_LEAN                           # never a lean program
        assert with_env["features"] & ~(FEAT_ENVIRONMENT | FEAT_TEXTURE) == flat0["features"] & ~FEAT_TEXTURE
        words2, items, n_media, n_wrapped = with_env["p2"]
        assert len(words2) == 0 and len(items) == 0 and (int(n_media), int(n_wrapped)) == (0, 0)   # no second program
        b.environment(None)
        assert _same_flat(_flat(b, world), flat0), "set, then clear"
    # a second call replaces the first
    b.environment(con)
    b.environment(img, scale=(2.0, 2.0, 2.0), rotate_y=90.0)
    e = b.get_environment()
    assert e["texture"] == img and tuple(e["scale"]) == (2.0, 2.0, 2.0) and e["rotate_y"] == 90.0
    b.environment(None)
    assert _same_flat(_flat(b, world), flat0)


# ---- the host probe --------------------------------------------------------------------------------------------------------------
def test_the_directions_cover_the_cases():
    d = EC.directions()
    assert d.shape == (4096, 3) and np.isnan(d).any() and np.isinf(d).any() and (d == 0).all(axis=1).any()
    tiny = np.finfo(f32).tiny
    assert ((np.abs(d) < tiny) & (d != 0)).any()                               # denormal components
    seam = (d[:, 0] < 0) & (d[:, 2] == 0) & np.isfinite(d).all(axis=1)
    assert (seam & np.signbit(d[:, 2])).any() and (seam & ~np.signbit(d[:, 2])).any()


@pytest.mark.parametrize("size", EC.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_probe_equals_the_numpy_definition(pkg, size):
    be = pkg.load()
    I, E = pkg.image, pkg.environment
    b = be.builder()
    img = EC.image(size)
    d = EC.directions()
    n = 0
    for prm in EC.settings(I):
        t = b.image(img, prm)
        for deg in EC.ROTATIONS:
            for scale in EC.SCALES:
                b.environment(t, scale=scale, rotate_y=deg)
                e = b.get_environment()
                want = E.colour(d, img, prm, scale, e["s"], e["c"])
                assert_bit_equal(b.environment_host(d), want, "%s, %g degrees, scale %r" % (EC.name(prm), deg, scale))
                n += 1
    assert n == 8 * 4 * 3


def test_the_host_probe_on_a_constant_and_on_the_other_kinds(pkg):
    be = pkg.load()
    E = pkg.environment
    b = be.builder()
    b.set_perlin_tables(*pkg.scenes.perlin_tables(SEED))
    d = EC.directions()
    con = b.constant(EC.CONSTANT)
    for deg in EC.ROTATIONS:
        for scale in EC.SCALES:
            b.environment(con, scale=scale, rotate_y=deg)
            e = b.get_environment()
            assert_bit_equal(b.environment_host(d), E.colour(d, EC.CONSTANT, None, scale, e["s"], e["c"]), "constant")
    ptr = d.ctypes.data_as(C.POINTER(C.c_float))
    out = np.empty_like(d)
    for other in (b.checker(con, b.constant((0.0, 0.0, 0.0))), b.perlin(0.7)):
        b.environment(other)
        assert be._debug_environment_host(b.h, len(d), ptr, out.ctypes.data_as(C.POINTER(C.c_float))) == ERR_UNSUPPORTED
    b.environment(None)
    assert be._debug_environment_host(b.h, len(d), ptr, out.ctypes.data_as(C.POINTER(C.c_float))) == ERR_INVALID   # no environment
    assert be._debug_environment_host(None, len(d), ptr, ptr) == ERR_INVALID and be._debug_environment_host(b.h, 1, None, ptr) == ERR_INVALID


def test_the_direction_is_rot_of_the_unit_vector(pkg):
    """environment.direction against float64 on ordinary directions (the definition is float32: agreement to rounding), and its
    own special cases: a unit axis comes back rotated exactly, a zero direction gives NaN."""
    E = pkg.environment
    rs = np.random.RandomState(3)
    d = rs.randn(1000, 3).astype(f32)
    for deg in EC.ROTATIONS:
        s, c = E.rotate_y_pair(deg)
        q = E.direction(d, s, c)
        u = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
        ref = np.stack([u[:, 0] * float(c) + u[:, 2] * float(s), u[:, 1], -u[:, 0] * float(s) + u[:, 2] * float(c)], axis=1)
        assert np.abs(q - ref).max() < 4e-7
    assert_bit_equal(E.direction([[0, 2, 0]], f32(0.6), f32(0.8)), [[0, 1, 0]])
    assert_bit_equal(E.direction([[3, 0, 0]], f32(0.6), f32(0.8)), [[0.8, 0, -0.6]])
    assert np.isnan(E.direction([[0, 0, 0]], f32(0.0), f32(1.0))).all()


def test_a_lat_long_map_has_row_0_at_plus_y(pkg):
    """An image with mapping 1 about (0, 0, 0) under the environment: +y reads the top row, -y the bottom row, and the texel
    directions of environment.texel_directions read their own texel under the nearest filter."""
    be = pkg.load()
    I, E = pkg.image, pkg.environment
    b = be.builder()
    w, h = 8, 4
    img = EC.image((w, h))
    prm = E.lat_long_params(filter=I.NEAREST)
    b.environment(b.image(img, prm))
    d = E.texel_directions(w, h).reshape(-1, 3).astype(f32)
    assert_bit_equal(b.environment_host(d), img.reshape(-1, 3), "texel directions")
    up = b.environment_host(np.array([[0.01, 1, 0.0], [0.01, -1, 0.0]], f32))
    assert (up[0] == img[0]).all(axis=-1).any() and (up[1] == img[h - 1]).all(axis=-1).any()


# ---- Radiance RGBE ---------------------------------------------------------------------------------------------------------------
def _representable(shape, seed):
    """Texels save_hdr can represent: three 8-bit mantissas of which the largest has its top bit set, a shared exponent."""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 256, shape + (3,))
    top = rs.randint(0, 3, shape)
    np.put_along_axis(m, top[..., None], rs.randint(128, 256, shape)[..., None], axis=-1)
    e = rs.randint(-20, 20, shape)
    x = np.ldexp(m.astype(np.float64), (e - 8)[..., None]).astype(f32)
    x[rs.rand(*shape) < 0.1] = 0.0
    return x


@pytest.mark.parametrize("shape", [(4, 8), (3, 40)], ids=["8x4", "40x3"])
@pytest.mark.parametrize("rle", [True, False], ids=["rle", "flat"])
def test_load_hdr_returns_what_save_hdr_can_represent(pkg, tmp_path, shape, rle):
    E = pkg.environment
    x = _representable(shape, 11 * shape[1])
    x[0, :6] = x[0, 0]                       # a run, so that the run-length writer has one to encode
    path = str(tmp_path / "x.hdr")
    E.save_hdr(path, x, rle=rle)
    raw = open(path, "rb").read()
    body = raw[raw.index(b"\n\n") + 2:]
    body = body[body.index(b"\n") + 1:]
    assert (body[:2] == b"\x02\x02") == rle and (len(body) == 4 * x.shape[0] * x.shape[1]) == (not rle)
    got = E.load_hdr(path)
    assert got.dtype == f32 and got.shape == x.shape
    assert_bit_equal(got, x, "round trip")
    # what it cannot represent is truncated towards zero, never raised: at most one mantissa step of the largest channel
    y = (np.random.RandomState(5).rand(*shape, 3) * 50).astype(f32)
    E.save_hdr(path, y, rle=rle)
    z = E.load_hdr(path)
    step = np.ldexp(1.0, np.frexp(y.max(axis=-1).astype(np.float64))[1] - 8)[..., None]
    assert (z <= y).all() and (y - z < step).all()


def test_a_hand_written_flat_file_decodes_to_known_values(pkg, tmp_path):
    E = pkg.environment
    path = str(tmp_path / "two.hdr")
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\n# a comment\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y 1 +X 2\n")
        f.write(bytes([128, 64, 0, 129, 255, 1, 2, 0]))   # (128, 64, 0) * 2^(129 - 136);  exponent byte 0: black
    got = E.load_hdr(path)
    assert got.shape == (1, 2, 3)
    assert_bit_equal(got, np.array([[[1.0, 0.5, 0.0], [0.0, 0.0, 0.0]]], f32))
    with open(path, "wb") as f:
        f.write(b"not a picture\n\n-Y 1 +X 1\n\0\0\0\0")
    with pytest.raises(ValueError):
        E.load_hdr(path)


def test_sun_sky_is_a_finite_sky_with_a_sun(pkg):
    sky = pkg.environment.sun_sky(64, 32)
    assert sky.shape == (32, 64, 3) and sky.dtype == f32 and np.isfinite(sky).all() and (sky >= 0).all()
    assert sky.max() > 20.0 and np.median(sky) < 1.0            # a small bright sun over an ordinary sky
    assert (sky[:16].reshape(-1, 3).mean(axis=0)[2] > sky[16:].reshape(-1, 3).mean(axis=0)[2])   # blue above, ground below

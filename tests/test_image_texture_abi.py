"""Image textures, CPU side (include/rtiow_gpu_image.h; Builder.image; image.py): the header declares exactly its four entry
points with the prototypes the binding and the Rust module give them, and they stay out of the ABI of rtiow_gpu.h; the
refusals; the host probe against the numpy definition, bit for bit; rt_atan2f against the definition and against float64; the
flattener's classification of images."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import assert_bit_equal
import image_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu_image.h")
IMAGE_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "image.rs")
NAMES = ["texture_image", "debug_texture_host", "debug_texture", "debug_atan2f_host"]
INVALID_ID = 0xFFFFFFFF
FEAT_TEXTURE, FEAT_WIDE_ALBEDO, FEAT_BRIGHT_ALBEDO = 8, 32, 64   # csrc/flat_scene.h


def _prototypes(text, strip, pattern):
    text = re.sub(strip, "", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()] for m in re.finditer(pattern, text, flags=re.S)}


def test_the_header_declares_exactly_the_four_entry_points(pkg):
    text = open(HEADER).read()
    c_fns = _prototypes(text, r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    assert sorted(c_fns) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.IMAGE_SYMBOLS == NAMES
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_texture_image"]] == ["b", "params", "w", "h", "rgb"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_debug_texture_host"]] == ["b", "texture", "n", "p", "out"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_debug_texture"]] == ["s", "texture", "n", "p", "out"]
    assert [a.split()[-1].lstrip("*") for a in c_fns["rtg_debug_atan2f_host"]] == ["n", "y", "x", "out"]
    # the parameter block, field for field, and the binding's copy of it
    block = re.search(r"typedef struct rtg_image_params \{(.*?)\} rtg_image_params;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = [f.strip().split()[-1] for part in block.split(";") for f in part.split(",") if f.strip()]
    assert fields == ["struct_size", "mapping", "filter", "wrap_u", "wrap_v", "reserved_in", "m[8]"]
    assert [n for n, _ in pkg.capi.ImageParams._fields_] == ["struct_size", "mapping", "filter", "wrap_u", "wrap_v", "reserved_in", "m"]
    assert C.sizeof(pkg.capi.ImageParams) == 6 * 4 + 8 * 4


def test_the_library_exports_them_with_the_binding_s_prototypes(pkg):
    be = pkg.load()
    for n, argc, res in zip(NAMES, (5, 5, 5, 4), (C.c_uint32, C.c_int, C.c_int, C.c_int)):
        fn = getattr(be.lib, "rtg_" + n)
        assert fn.restype is res and len(fn.argtypes) == argc, n
    assert be.lib.rtg_texture_image.argtypes[1] is C.POINTER(pkg.capi.ImageParams)


def test_they_stay_out_of_the_abi_and_the_rust_module_follows_the_header(pkg):
    capi = pkg.capi
    assert not set(NAMES) & set(capi.ABI_SYMBOLS) and not set(NAMES) & set(capi.QUERY_SYMBOLS) and not set(NAMES) & set(capi.RAY_FRAME_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "rtiow_gpu.h")).read()
    assert "rtg_texture_image" not in main and "rtg_image_params" not in main
    c_fns = _prototypes(open(HEADER).read(), r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    rs_fns = _prototypes(open(IMAGE_RS).read(), r"//[^\n]*", r"pub fn (rtg_\w+)\s*\(([^)]*)\)")
    assert sorted(rs_fns) == sorted(c_fns)
    for name in c_fns:
        assert len(rs_fns[name]) == len(c_fns[name]), name
    lib_rs = open(os.path.join(os.path.dirname(IMAGE_RS), "lib.rs")).read()
    assert "pub mod image;" in lib_rs
    for n in NAMES:
        assert "rtg_" + n not in lib_rs, n


def test_every_refusal_leaves_the_builder_as_it_was(pkg):
    be = pkg.load()
    I, P = pkg.image, pkg.capi.ImageParams
    b = be.builder()
    first = b.constant((0.1, 0.2, 0.3))
    img = np.zeros((2, 3, 3), np.float32)
    ptr = img.ctypes.data_as(C.POINTER(C.c_float))
    good = P.new(I.params())

    def refused(p, w=3, h=2, rgb=ptr, builder=b.h):
        got = be._texture_image(builder, None if p is None else C.byref(p), w, h, rgb)
        return got == INVALID_ID and be.last_error() != ""

    for field in ("mapping", "filter", "wrap_u", "wrap_v"):
        for value in (2, 0xFFFFFFFF):
            p = P.new(I.params())
            setattr(p, field, value)
            assert refused(p), (field, value)
    p = P.new(I.params())
    p.struct_size -= 4
    assert refused(p)
    p = P.new(I.params())
    p.struct_size += 4
    assert refused(p)
    p = P.new(I.params(reserved_in=1))
    assert refused(p)
    for i in range(3, 8):   # the spherical mapping takes a centre only
        m = np.zeros(8, np.float32)
        m[i] = 1.0
        assert refused(P.new(I.params(I.SPHERICAL, m=m))), i
    assert refused(None) and refused(good, rgb=None) and refused(good, builder=None)
    # the limits: no side of 0 or above 16384, no more than 2^24 texels (refused before a texel is read)
    for w, h in ((0, 2), (3, 0), (16385, 1), (1, 16385), (16384, 1025), (8192, 2049)):
        assert refused(good, w=w, h=h), (w, h)
    # the builder's texture count has not moved: the next id is the one behind `first`
    assert b.constant((0.0, 0.0, 0.0)) == first + 1
    # ... and an accepted image takes two: its record and the record of its mapping floats, which no call accepts as a texture
    t = b.image(img, I.params())
    assert t == first + 2
    assert be._material_lambertian(b.h, t + 1) == INVALID_ID and be._material_diffuse_light(b.h, t + 1, 1.0) == INVALID_ID
    assert be._material_isotropic(b.h, t + 1) == INVALID_ID
    assert be._texture_checker(b.h, t + 1, t) == INVALID_ID and be._texture_checker(b.h, t, t + 1) == INVALID_ID
    pts = np.zeros((1, 3), np.float32)
    assert be._debug_texture_host(b.h, t + 1, 1, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert b.constant((0.0, 0.0, 0.0)) == first + 4
    b.lambertian(t), b.isotropic(t), b.diffuse_light(t, 2.0), b.checker(t, first), b.checker(first, t)   # all accepted


def test_the_largest_image_is_accepted(pkg):
    """The longest side, both ways: 16384 x 1 and 1 x 16384 (an image of 2^24 texels is 256 MB of packets, too large for a quick
    test: the arithmetic of that limit is covered by the refusals just above it)."""
    be = pkg.load()
    I = pkg.image
    b = be.builder()
    rs = np.random.RandomState(5)
    for shape in ((1, 16384, 3), (16384, 1, 3)):
        img = rs.rand(*shape).astype(np.float32)
        for flt in (I.NEAREST, I.BILINEAR):
            prm = I.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0, filter=flt)
            t = b.image(img, prm)
            p = (rs.rand(256, 3) * 4 - 2).astype(np.float32)
            assert_bit_equal(b.texture_host(t, p), I.sample(img, prm, p), str(shape))


@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_host_probe_equals_the_numpy_definition(pkg, size):
    be = pkg.load()
    I = pkg.image
    b = be.builder()
    img = IC.image(size)
    n = 0
    for prm in IC.settings(I, size):
        t = b.image(img, prm)
        p = IC.points(I, prm, size)
        assert_bit_equal(b.texture_host(t, p), I.sample(img, prm, p), IC.name(prm))
        n += len(p)
    assert n > 16 * 200


@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: "%dx%d" % s)
def test_bilinear_returns_the_texel_at_a_texel_centre(pkg, size):
    """Planar, u = x and v = y: at ((i + 0.5) / w, 1 - (j + 0.5) / h) both weights are exactly 0 wherever the float32
    coordinate arithmetic lands on the centre exactly (everywhere when w and h are powers of two, at least a quarter of the
    centres for the other sizes); there bilinear returns the texel itself.  Every centre is also compared with the definition."""
    be = pkg.load()
    I = pkg.image
    w, h = size
    img = IC.image(size)
    prm = I.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0, filter=I.BILINEAR)
    p = IC.centres(size)
    u, v = I.uv(prm, p)
    x, y = u * np.float32(w) - np.float32(0.5), (np.float32(1.0) - v) * np.float32(h) - np.float32(0.5)
    exact = (x == np.floor(x)) & (y == np.floor(y))
    assert exact.sum() >= max(1, (w * h) // 4)
    b = be.builder()
    got = b.texture_host(b.image(img, prm), p)
    assert_bit_equal(got[exact], img.reshape(-1, 3)[exact], "centres")
    assert_bit_equal(got, I.sample(img, prm, p), "centres against the definition")


def test_a_constant_image_returns_its_value_exactly(pkg):
    be = pkg.load()
    I = pkg.image
    rs = np.random.RandomState(11)
    b = be.builder()
    for size in ((1, 1), (4, 4), (5, 3)):
        c = (rs.rand(3) * 3).astype(np.float32)
        img = np.broadcast_to(c, (size[1], size[0], 3)).copy()
        for flt in (I.NEAREST, I.BILINEAR):
            for prm in (I.planar((0.3, 0.1, -0.2), 0.25, (0.05, -0.4, 0.7), -0.5, filter=flt),
                        I.spherical((0.5, -0.25, 1.0), filter=flt, wrap_v=I.CLAMP)):
                p = ((rs.rand(4096, 3) - 0.5) * 40).astype(np.float32)
                got = b.texture_host(b.image(img, prm), p)
                assert_bit_equal(got, np.broadcast_to(c, got.shape), "constant image")
                assert_bit_equal(I.sample(img, prm, p), np.broadcast_to(c, got.shape), "constant image, definition")


def test_the_probe_refuses_what_it_does_not_evaluate(pkg):
    be = pkg.load()
    b = be.builder()
    b.set_perlin_tables(*pkg.scenes.perlin_tables(1))
    c = b.constant((0.25, 0.5, 0.75))
    p = np.zeros((3, 3), np.float32)
    assert (b.texture_host(c, p) == np.float32([0.25, 0.5, 0.75])).all()
    for t in (b.checker(c, c), b.perlin(0.1)):
        with pytest.raises(pkg.capi.RtError) as e:
            b.texture_host(t, p)
        assert e.value.code == pkg.capi.ERR_UNSUPPORTED
    with pytest.raises(pkg.capi.RtError) as e:
        b.texture_host(99, p)
    assert e.value.code == pkg.capi.ERR_INVALID


# ---- rt_atan2f ---------------------------------------------------------------------------------------------------------------
def _ordered(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(u < 0, -(u & 0x7FFFFFFF), u)


def test_atan2f_equals_the_definition_and_float64(pkg, capsys):
    """2^20 random pairs over all exponents (random bit patterns) plus the grid of special values: the host probe equals
    image.atan2f bit for bit, and lies within 1 ulp of the float32 nearest to numpy's float64 arctan2 -- the bound an accurate
    float64 result rounded once guarantees.  Signed zeros, +-pi, the infinities and NaN come out as C's atan2f gives them."""
    be = pkg.load()
    I = pkg.image
    y, x = IC.atan2_pairs()
    got = be.atan2f_host(y, x)
    assert_bit_equal(got, I.atan2f(y, x), "rt_atan2f against image.atan2f")
    with np.errstate(all="ignore"):
        want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    dist = np.abs(_ordered(got[~nan]) - _ordered(want[~nan]))
    # +0 and -0 are 0 apart in this order: the sign of a zero result is checked on its own
    zero = want == 0
    assert (np.signbit(got[zero]) == np.signbit(want[zero])).all()
    with capsys.disabled():
        print("\nrt_atan2f: worst distance from the correctly rounded float32 of float64 arctan2 over %d pairs: %d ulp (%d pairs differ)"
              % (len(y), int(dist.max()), int((dist > 0).sum())))
    assert dist.max() <= 1
    # the special values, spelled out
    pi, inf = np.float32(np.pi), np.float32(np.inf)
    f = lambda a, c: be.atan2f_host(np.float32([a]), np.float32([c]))[0]
    for a, c, r in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, pi), (-0.0, -0.0, -pi), (0.0, -1.0, pi), (-0.0, -1.0, -pi),
                    (1.0, 0.0, pi / 2), (-1.0, -0.0, -pi / 2), (inf, inf, pi / 4), (inf, -inf, np.float32(3 * np.pi / 4)),
                    (-inf, -inf, np.float32(-3 * np.pi / 4)), (1.0, inf, 0.0), (-1.0, inf, -0.0), (1.0, -inf, pi), (inf, 1.0, pi / 2),
                    (1.0, 1.0, pi / 4), (-1.0, 1.0, -pi / 4)):
        got1 = f(a, c)
        assert got1.view(np.uint32) == np.float32(r).view(np.uint32), (a, c, got1, r)
    assert np.isnan(f(np.nan, 1.0)) and np.isnan(f(1.0, np.nan)) and np.isnan(f(np.nan, np.nan))


# ---- the flattener's classification --------------------------------------------------------------------------------------------
def _features(be, pkg, make_texture, material="lambertian"):
    b = be.builder()
    t = make_texture(b)
    m = b.diffuse_light(t, 2.0) if material == "light" else getattr(b, material)(t)
    return b.flatten([b.sphere(1.0, m)])[1]


def test_the_flattener_classifies_images_by_their_texels(pkg):
    be = pkg.load()
    I = pkg.image
    prm = I.params()
    rs = np.random.RandomState(3)
    unit = rs.rand(4, 5, 3).astype(np.float32)
    unit[0, 0] = (0.0, 1.0, 0.5)   # the ends of [0, 1] are inside
    bright, negative, nan, huge, infinite = (unit.copy() for _ in range(5))
    bright[2, 3, 1] = 1.5
    negative[3, 4, 2] = -1e-6
    nan[1, 1, 0] = np.nan
    huge[0, 2, 0] = 4.5
    infinite[0, 2, 0] = np.inf
    img = lambda a: (lambda b: b.image(a, prm))
    albedo = FEAT_WIDE_ALBEDO | FEAT_BRIGHT_ALBEDO
    for material in ("lambertian", "isotropic"):
        assert _features(be, pkg, img(unit), material) & (FEAT_TEXTURE | albedo) == FEAT_TEXTURE
        assert _features(be, pkg, img(bright), material) & (FEAT_TEXTURE | albedo) == FEAT_TEXTURE | FEAT_BRIGHT_ALBEDO
        for wide in (negative, nan, huge, infinite):
            f = _features(be, pkg, img(wide), material)
            assert f & FEAT_TEXTURE and f & FEAT_WIDE_ALBEDO
    for a in (unit, bright, negative, nan):   # an emitter's texture is no albedo
        assert _features(be, pkg, img(a), "light") & (FEAT_TEXTURE | albedo) == FEAT_TEXTURE
    # a 4-in-[0, 4] image is bright, not wide
    four = unit.copy()
    four[0, 0, 0] = 4.0
    assert _features(be, pkg, img(four)) & albedo == FEAT_BRIGHT_ALBEDO
    # a checker over two images inherits the worse class of its children; the walk descends through nested checkers
    chk = lambda a0, a1: (lambda b: b.checker(b.image(a0, prm), b.image(a1, prm)))
    assert _features(be, pkg, chk(unit, unit)) & (FEAT_TEXTURE | albedo) == FEAT_TEXTURE
    assert _features(be, pkg, chk(unit, bright)) & albedo == FEAT_BRIGHT_ALBEDO
    assert _features(be, pkg, chk(bright, unit)) & albedo == FEAT_BRIGHT_ALBEDO
    assert _features(be, pkg, chk(bright, negative)) & FEAT_WIDE_ALBEDO
    assert _features(be, pkg, chk(nan, unit)) & FEAT_WIDE_ALBEDO
    nested = lambda b: b.checker(b.constant((0.5, 0.5, 0.5)), b.checker(b.image(unit, prm), b.image(negative, prm)))
    assert _features(be, pkg, nested) & FEAT_WIDE_ALBEDO
    assert _features(be, pkg, chk(unit, negative), "light") & albedo == 0
    # the primitive of a textured material carries F_TEXTURED (bit 19 of the flag word)
    b = be.builder()
    words, _ = b.flatten([b.sphere(1.0, b.lambertian(b.image(unit, prm)))])
    assert int(words[0, 7]) & (1 << 19)


def test_from_u8_and_bake(pkg):
    be = pkg.load()
    I = pkg.image
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    lin = I.from_u8(u8)
    assert lin.dtype == np.float32 and lin.shape == (16, 16, 3) and lin[0, 0, 0] == 0 and lin[15, 15, 0] == 1
    # the inverse of the tonemap's quantisation: sqrt(x) * 255.99, truncated, gives the byte back
    back = np.floor(np.float32(255.99) * np.sqrt(lin)).astype(np.int64)
    assert (np.abs(back - u8) <= 1).all() and (back[u8 > 0] == u8[u8 > 0]).mean() > 0.95
    assert np.array_equal(I.from_u8(u8, gamma=False), u8.astype(np.float32) / np.float32(255))
    # bake: a closure of p at the texel centres of a planar mapping; the nearest filter then returns the closure's value there
    prm = I.planar((0.25, 0, 0), 0.5, (0, 0, 0.5), 0.25, filter=I.NEAREST)
    fn = lambda p: np.stack([p[:, 0], p[:, 2], p[:, 0] * p[:, 2]], axis=1)
    w, h = 8, 4
    img = I.bake(fn, prm, w, h)
    assert img.shape == (h, w, 3) and img.dtype == np.float32
    centres = I.texel_centres(prm, w, h)
    u, v = I.uv(prm, centres)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.allclose(u, (ii.reshape(-1) + 0.5) / w, atol=1e-6) and np.allclose(v, 1 - (jj.reshape(-1) + 0.5) / h, atol=1e-6)
    b = be.builder()
    assert_bit_equal(b.texture_host(b.image(img, prm), centres), fn(centres).astype(np.float32), "baked closure")
    with pytest.raises(ValueError):
        I.texel_centres(I.spherical(), 4, 4)

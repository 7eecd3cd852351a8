"""Scene builders of the reference, transliterated against the builder API (capi.Builder).

Each function takes a builder `b` (HIP product or, in tests, the oracle -- same calls) and returns
`(world, camera, exposure)` exactly like the reference's scene functions:

  cornell_box / cornell_box_with_boxes      src/lib.rs:103-193
  cornell_box_scene / motion_test / volume_test / simple_light_scene / book_final_scene
                                            src/main.rs:11-319
  bench_scene                               benches/scene.rs:8-36
  random_scene (book 1)                     src/lib.rs:238-319 (dead code in the reference, written
                                            against an older enum API) re-expressed in the live API
                                            as SURVEY.md 8(d) specifies.

All scalar arithmetic is done in numpy float32 so the scene data equals what the f32 Rust code builds.
"""
import numpy as np

from .small_rng import SmallRng, perlin_tables

f32 = np.float32
X, Y, Z = 0, 1, 2  # object::StaticX / StaticY / StaticZ


def v(x, y, z):
    return np.array([x, y, z], dtype=f32)


def vfrom(x):
    return np.array([x, x, x], dtype=f32)


# ---------------------------------------------------------------------------------------------
# src/lib.rs
# ---------------------------------------------------------------------------------------------
def cornell_box(b):
    """lib.rs:103-166"""
    def diffuse_color(c):
        return b.lambertian(b.constant(c))

    red = diffuse_color(v(0.65, 0.05, 0.05))
    white = diffuse_color(vfrom(0.73))
    green = diffuse_color(v(0.12, 0.45, 0.15))
    light = b.diffuse_light(b.constant(vfrom(1.0)), 15.0)
    return [
        b.rect(Y, (213.0, 343.0), (227.0, 332.0), 554.0, light),
        b.rect(Y, (0.0, 555.0), (0.0, 555.0), 0.0, white),                      # floor
        b.flip_normals(b.rect(Z, (0.0, 555.0), (0.0, 555.0), 555.0, white)),    # rear wall
        b.flip_normals(b.rect(Y, (0.0, 555.0), (0.0, 555.0), 555.0, white)),    # ceiling
        b.rect(X, (0.0, 555.0), (0.0, 555.0), 0.0, red),                        # right wall
        b.flip_normals(b.rect(X, (0.0, 555.0), (0.0, 555.0), 555.0, green)),    # left wall
    ]


def cornell_box_with_boxes(b):
    """lib.rs:168-193"""
    scene = cornell_box(b)
    white = b.lambertian(b.constant(vfrom(0.73)))
    scene.append(b.translate(v(130.0, 0.0, 65.0),
                             b.rotate_y(-18.0, b.rect_prism(v(0, 0, 0), v(165.0, 165.0, 165.0), white))))
    scene.append(b.translate(v(265.0, 0.0, 295.0),
                             b.rotate_y(15.0, b.rect_prism(v(0, 0, 0), v(165.0, 330.0, 165.0), white))))
    return scene


# ---------------------------------------------------------------------------------------------
# src/main.rs
# ---------------------------------------------------------------------------------------------
def _cornell_camera(be, nx, ny):
    """main.rs:12-27 (shared by cornell_box_scene, motion_test, volume_test, simple_light_scene)"""
    exposure = (0.0, 1.0)
    cam = be.camera_look(v(278.0, 278.0, -800.0), v(278.0, 278.0, 0.0), v(0.0, 1.0, 0.0), 40.0,
                         float(f32(nx) / f32(ny)), 0.0, 10.0, exposure)
    return cam, exposure


def cornell_box_scene(b, nx, ny):
    """main.rs:11-30"""
    cam, exposure = _cornell_camera(b.be, nx, ny)
    return cornell_box_with_boxes(b), cam, exposure


def cornell_mesh_scene(b, nx, ny, subdivisions=2, sah=False):
    """Not in the reference: the Cornell box with two triangle meshes (include/rtiow_gpu_mesh.h) in place of its two prisms --
    an icosphere of 20 * 4^subdivisions triangles where the short box stood, and the tall box as a 12-triangle box mesh under
    the reference's own Translate{RotateY}."""
    from . import triangle
    cam, exposure = _cornell_camera(b.be, nx, ny)
    scene = cornell_box(b)
    white = b.lambertian(b.constant(vfrom(0.73)))
    vs, fs = triangle.icosphere(subdivisions, radius=82.5, centre=(212.5, 82.5, 147.5))
    scene.append(b.mesh(vs, fs, white, sah=sah))
    vb, fb = triangle.box((0.0, 0.0, 0.0), (165.0, 330.0, 165.0))
    scene.append(b.translate(v(265.0, 0.0, 295.0), b.rotate_y(15.0, b.mesh(vb, fb, white, sah=sah))))
    return scene, cam, exposure


def surface_test_image(w=8, h=4):
    """A small image whose every texel differs: what cornell_surface_scene maps on its box mesh."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x + 1.0) / (w + 1.0), (y + 1.0) / (h + 1.0), 0.25 + 0.5 * ((x + y) % 2)], axis=-1)
    return img.astype(np.float32)


def box_uvs(vertices):
    """Per-vertex UVs for triangle.box(): (x, y) of the vertex scaled to the unit square.  The faces orthogonal to z show the
    image once; the others stretch a row or a column of it."""
    p = np.asarray(vertices, dtype=np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return ((p[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)


def cornell_surface_scene(b, nx, ny, subdivisions=2, sah=False, image=None, filter=0, box_wrapped=True, smooth=True):
    """Not in the reference: cornell_mesh_scene with surface attributes (include/rtiow_gpu_surface.h) -- the icosphere with
    per-vertex normals (smooth shading), the tall box mesh with per-vertex UVs and an image mapped on its surface through
    Builder.surface, under the reference's own Translate{RotateY}, and an emissive UV-textured triangle below the ceiling.
    Returns (scene, cam, exposure, info): info names the image texture, its parameters and the box mesh's object id."""
    from . import image as image_mod, triangle
    cam, exposure = _cornell_camera(b.be, nx, ny)
    scene = cornell_box(b)
    white = b.lambertian(b.constant(vfrom(0.73)))
    vs, fs, ns, _ = triangle.icosphere_attr(subdivisions, radius=82.5, centre=(212.5, 82.5, 147.5))
    scene.append(b.mesh(vs, fs, white, sah=sah, normals=ns if smooth else None))
    img = surface_test_image() if image is None else image
    prm = image_mod.planar((1.0, 0.0, 0.0), 0.0, (0.0, 1.0, 0.0), 0.0, filter=filter)   # ordinary UV mapping: v up, row 0 at the top
    tex = b.image(img, prm)
    mapped = b.lambertian(b.surface(tex))
    vb, fb = triangle.box((0.0, 0.0, 0.0), (165.0, 330.0, 165.0))
    box = b.mesh(vb, fb, mapped, sah=sah, uvs=box_uvs(vb))
    scene.append(b.translate(v(265.0, 0.0, 295.0), b.rotate_y(15.0, box)) if box_wrapped else box)
    glow = b.diffuse_light(b.surface(b.image(surface_test_image(4, 4), prm)), 4.0)
    scene.append(b.triangle_attr(v(100.0, 500.0, 100.0), v(200.0, 500.0, 100.0), v(100.0, 500.0, 200.0), glow,
                                 uvs=((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))))
    return scene, cam, exposure, {"image": img, "params": prm, "texture": tex, "box": box}


def motion_test(b, nx, ny):
    """main.rs:33-67"""
    cam, exposure = _cornell_camera(b.be, nx, ny)
    scene = cornell_box(b)
    mat = b.lambertian(b.constant(vfrom(0.73)))
    scene.append(b.translate(v(278.0, 278.0, 278.0),
                             b.linear_move(b.sphere(65.0, mat), v(0.0, 100.0, 0.0))))
    return scene, cam, exposure


def volume_test(b, nx, ny):
    """main.rs:70-108"""
    cam, exposure = _cornell_camera(b.be, nx, ny)
    scene = cornell_box(b)
    boundary = b.sphere(180.0, b.lambertian(b.constant(vfrom(0.73))))  # material does not matter
    medium = b.constant_medium(boundary, 0.01, b.isotropic(b.constant(v(0.2, 0.2, 1.0))))
    scene.append(b.translate(v(278.0, 278.0, 278.0), medium))
    return scene, cam, exposure


def simple_light_scene(b, nx, ny, rng, spheres=1000):
    """main.rs:111-159"""
    cam, exposure = _cornell_camera(b.be, nx, ny)
    world = cornell_box(b)
    for _ in range(spheres):
        mat = b.lambertian(b.constant(vfrom(0.3)))
        offset = f32(277.0) + f32(257.0) * rng.gen_vec3()
        world.append(b.translate(offset, b.sphere(20.0, mat)))
    world.append(b.flip_normals(b.sphere(1000.0, b.diffuse_light(b.constant(vfrom(0.1)), 1.0))))
    return world, cam, exposure


def book_final_scene(b, nx, ny, rng, perlin_seed=0xDEADBEEF):
    """main.rs:161-319 (book 2 final scene).  Perlin tables: fixed, from SmallRng(perlin_seed)."""
    exposure = (0.0, 1.0)
    cam = b.be.camera_look(v(478.0, 278.0, -600.0), v(278.0, 278.0, 0.0), v(0.0, 1.0, 0.0), 40.0,
                           float(f32(nx) / f32(ny)), 0.0, 10.0, exposure)
    b.set_perlin_tables(*perlin_tables(perlin_seed))

    ground = b.lambertian(b.constant(v(0.48, 0.83, 0.53)))
    world = []

    # Make random floor. main.rs:192-203
    boxes = []
    W = f32(100.0)
    for i in range(20):
        for j in range(20):
            c0 = v(f32(-1000.0) + f32(i) * W, 0.0, f32(-1000.0) + f32(j) * W)
            c1 = c0 + v(W, f32(100.0) * (rng.gen_f32() + f32(0.01)), W)
            boxes.append(b.rect_prism(c0, c1, ground))
    world.append(b.bvh(boxes, exposure))

    # Make light. main.rs:206-215
    world.append(b.rect(Y, (123.0, 423.0), (147.0, 412.0), 554.0,
                        b.diffuse_light(b.constant(vfrom(1.0)), 7.0)))

    # Brown blurry sphere. main.rs:218-229
    world.append(b.translate(v(400.0, 400.0, 200.0),
                             b.linear_move(b.sphere(50.0, b.lambertian(b.constant(v(0.7, 0.3, 0.1)))),
                                           v(30.0, 0.0, 0.0))))
    glass = b.dielectric(1.5)
    # Glass sphere. main.rs:234-240
    world.append(b.translate(v(260.0, 150.0, 45.0), b.sphere(50.0, glass)))
    # Silvery sphere. main.rs:243-252
    world.append(b.translate(v(0.0, 150.0, 145.0), b.sphere(50.0, b.metal(v(0.8, 0.8, 0.9), 1.0))))
    # Blue glass sphere. main.rs:255-269
    boundary = b.translate(v(360.0, 150.0, 145.0), b.sphere(70.0, glass))
    world.append(boundary)
    world.append(b.constant_medium(boundary, 0.2, b.isotropic(b.constant(v(0.2, 0.4, 0.9)))))
    # Fog. main.rs:272-281
    world.append(b.constant_medium(b.sphere(5000.0, glass), 0.0001, b.isotropic(b.constant(vfrom(1.0)))))
    # Perlin marbled sphere. main.rs:284-292
    world.append(b.translate(v(220.0, 280.0, 300.0), b.sphere(80.0, b.lambertian(b.perlin(0.05)))))
    # Cube made of random spheres. main.rs:295-316
    white = b.lambertian(b.constant(vfrom(0.73)))
    spheres = [b.translate(f32(165.0) * rng.gen_vec3(), b.sphere(10.0, white)) for _ in range(1000)]
    world.append(b.translate(v(-100.0, 270.0, 395.0), b.rotate_y(15.0, b.bvh(spheres, exposure))))
    return world, cam, exposure


def bench_scene(b, nx, ny):
    """benches/scene.rs:8-36: Cornell box + prisms in a BVH, book-1 camera."""
    world = [b.bvh(cornell_box_with_boxes(b), (0.0, 1.0))]
    cam = b.be.camera_look(v(13.0, 2.0, 3.0), v(0, 0, 0), v(0.0, 1.0, 0.0), 20.0, float(f32(nx) / f32(ny)),
                           0.1, 10.0, (0.0, 1.0))
    return world, cam, (0.0, 1.0)


# ---------------------------------------------------------------------------------------------
# Book-1 random spheres (BASELINE.json north-star workload)
# ---------------------------------------------------------------------------------------------
DOME_COLOUR = (0.7, 0.8, 1.0)   # the emission of book-1's sky dome


def random_scene_objects(b, rng, dome=True):
    """lib.rs:238-319 re-expressed in the live API: each sphere is
    Translate{offset: center, Sphere{radius, material}}; no motion (book 1); constant grey ground;
    the three r=1 spheres follow the book layout (glass / Lambertian / metal); a FlipNormals sky-dome
    emitter (same idiom as main.rs:150-156) replaces the sky, because a miss is black (lib.rs:100).  dome=False leaves the
    emitter out: the world for a call with a background (include/rtiow_gpu.h RTG_FLAG_BACKGROUND)."""
    world = [b.translate(v(0.0, -1000.0, 0.0), b.sphere(1000.0, b.lambertian(b.constant(vfrom(0.5)))))]
    for a in range(-11, 11):
        for bb in range(-11, 11):
            center = v(f32(a) + f32(0.9) * rng.gen_f32(), 0.2, f32(bb) + f32(0.9) * rng.gen_f32())
            d = center - v(4.0, 0.2, 0.0)
            dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if dist > f32(0.9):
                choose_mat = rng.gen_f32()
                if choose_mat < f32(0.8):
                    mat = b.lambertian(b.constant(rng.gen_vec3() * rng.gen_vec3()))
                elif choose_mat < f32(0.95):
                    albedo = f32(0.5) * (f32(1.0) + rng.gen_vec3())
                    mat = b.metal(albedo, float(f32(0.5) * rng.gen_f32()))
                else:
                    mat = b.dielectric(1.5)
                world.append(b.translate(center, b.sphere(0.2, mat)))
    world.append(b.translate(v(0.0, 1.0, 0.0), b.sphere(1.0, b.dielectric(1.5))))
    world.append(b.translate(v(-4.0, 1.0, 0.0), b.sphere(1.0, b.lambertian(b.constant(v(0.4, 0.2, 0.1))))))
    world.append(b.translate(v(4.0, 1.0, 0.0), b.sphere(1.0, b.metal(v(0.7, 0.6, 0.5), 0.0))))
    if dome:
        world.append(b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(v(*DOME_COLOUR)), 1.0))))
    return world


def random_scene(b, nx, ny, rng=None, use_bvh=True, sky="dome"):
    """Book-1 random spheres + the benches/scene.rs:16-30 camera; whole scene under bvh::from_scene
    (the USE_BVH = true path of main.rs:340-345).
    sky="dome" (default): the world ends with the sky-dome emitter; returns (world, camera, exposure).
    sky="background": the world without the dome, and a fourth item, the background= of the render calls that gives the same
    image (capi.Scene.par_cast; a constant background of the dome's emission): (world, camera, exposure, background)."""
    if sky not in ("dome", "background"):
        raise ValueError('sky must be "dome" or "background"')
    if rng is None:
        rng = SmallRng(0xDEADBEEF)  # main.rs:333
    exposure = (0.0, 1.0)
    objs = random_scene_objects(b, rng, dome=sky == "dome")
    if use_bvh == "sah":      # non-parity option: same image, ~36 % fewer Aabb tests per ray
        world = [b.bvh_sah(objs, exposure)]
    else:
        world = [b.bvh(objs, exposure)] if use_bvh else objs
    cam = b.be.camera_look(v(13.0, 2.0, 3.0), v(0, 0, 0), v(0.0, 1.0, 0.0), 20.0, float(f32(nx) / f32(ny)),
                           0.1, 10.0, exposure)
    if sky == "background":
        return world, cam, exposure, {"bottom": DOME_COLOUR}
    return world, cam, exposure


def book1_environment_scene(b, nx, ny, rng=None, use_bvh=True, sky=None, filter=1, scale=(1.0, 1.0, 1.0), rotate_y=0.0):
    """Not in the reference: book-1 without its dome, under an environment map (include/rtiow_gpu_environment.h;
    Builder.environment).  `sky`: a lat-long image float32 [h, w, 3], row 0 = world +y (default: environment.sun_sky(64, 32)).
    The builder carries the environment when this returns, so the scene made from the world renders under it.
    Returns (world, camera, exposure, info): info names the image texture and the environment's parameters."""
    from . import environment as environment_mod, image as image_mod
    if sky is None:
        sky = environment_mod.sun_sky(64, 32)
    world, cam, exposure, _ = random_scene(b, nx, ny, rng=rng, use_bvh=use_bvh, sky="background")
    prm = image_mod.spherical(filter=filter, wrap_u=image_mod.REPEAT, wrap_v=image_mod.CLAMP)
    tex = b.image(sky, prm)
    b.environment(tex, scale=scale, rotate_y=rotate_y)
    return world, cam, exposure, dict(texture=tex, image=np.asarray(sky, dtype=f32), params=prm, scale=scale, rotate_y=rotate_y)

"""Shared by test_ray_frame_abi.py and test_ray_frame_gpu.py (include/rtiow_gpu_rays.h; Scene.cast_rays): the scenes the ray-frame
tests render, per-pixel rays through pixel centres, and the float64 check of the library's restated camera rays."""
import numpy as np

from camera_ref import look
from fuzz_scenes import random_camera, random_world

F = np.float64


def build(pkg, be, name, nx, ny):
    """(scene, camera) of a named scene on backend `be`."""
    S = pkg.scenes
    b = be.builder()
    if name == "book1":
        world, cam, _ = S.random_scene(b, nx, ny)
    elif name == "cornell":
        world, cam, _ = S.cornell_box_scene(b, nx, ny)
    elif name == "volume":
        world, cam, _ = S.volume_test(b, nx, ny)
    elif name == "motion":
        world, cam, _ = S.motion_test(b, nx, ny)
    elif name == "deep":
        world, cam = deep_graph(pkg, be, b, nx, ny)
    else:
        raise KeyError(name)
    return b.scene(world), cam


def deep_graph(pkg, be, b, nx, ny):
    """The first FEAT_DEEP graph among the fuzz seeds (flat_scene.h FEAT_DEEP = 128), the same on every backend."""
    for seed in range(9000, 9064):
        probe = pkg.load().builder()   # (the product's flattener runs on the host and names the program's features)
        if probe.flatten(random_world(pkg, probe, np.random.RandomState(seed), general_boundaries=True, deep_shapes=True))[1] & 128:
            rs = np.random.RandomState(seed)
            world = random_world(pkg, b, rs, general_boundaries=True, deep_shapes=True)
            return world, random_camera(pkg, be, rs, nx, ny)
    raise AssertionError("no FEAT_DEEP graph among the fuzz seeds")


def pinhole_rays(cam, nx, ny, time=0.0):
    """One ray per pixel from the camera's origin through the pixel's centre on its image plane: float32 [nx * ny, 7], pixel
    p = row * nx + x, row 0 = top."""
    o, llc = np.array(list(cam.origin), F), np.array(list(cam.lower_left_corner), F)
    hor, ver = np.array(list(cam.horizontal), F), np.array(list(cam.vertical), F)
    row, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    u, v = ((x + 0.5) / nx).reshape(-1, 1), ((ny - 1 - row + 0.5) / ny).reshape(-1, 1)
    rays = np.empty((nx * ny, 7), np.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = llc + u * hor + v * ver - o
    rays[:, 6] = time
    return rays


def aimed_rays(target, nx, ny, distance=5.0, spread=0.5):
    """nx * ny rays from distinct origins on a plane `distance` in front of `target` (towards +z), every one aimed at `target`."""
    row, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    o = np.stack([spread * (x.reshape(-1) / max(nx - 1, 1) - 0.5), spread * (row.reshape(-1) / max(ny - 1, 1) - 0.5),
                  np.full(nx * ny, distance)], axis=-1) + np.asarray(target, F)
    rays = np.zeros((nx * ny, 7), np.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = np.asarray(target, F) - o
    return rays


def check_camera_rays(rays, pose, nx, ny, ns, tol):
    """`rays` (camera_rays' per-sample layout) against the camera of `pose` (camera_ref.look's arguments) in float64: every origin
    in the lens disc, every origin + direction on the image plane inside its own pixel, every time in [0, 1)."""
    c = look(*pose)
    r = np.asarray(rays, F).reshape(ns, ny, nx, 7)
    off = r[..., 0:3] - c["origin"]
    a, b, along = off @ c["u"], off @ c["v"], off @ c["w"]
    assert np.abs(along).max() <= tol, ("origin off the lens plane", np.abs(along).max())
    assert (np.sqrt(a * a + b * b) <= c["lens_radius"] + tol).all(), "origin outside the lens disc"
    assert np.sqrt(a * a + b * b).max() > 0.5 * c["lens_radius"], "the lens disc is not used"
    point = r[..., 0:3] + r[..., 3:6] - c["lower_left_corner"]     # on the image plane: s * horizontal + t * vertical
    assert np.abs(point @ c["w"]).max() <= tol, ("origin + direction off the image plane", np.abs(point @ c["w"]).max())
    s = (point @ c["u"]) / float(c["horizontal"] @ c["u"])
    t = (point @ c["v"]) / float(c["vertical"] @ c["v"])
    row, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    y = ny - 1 - row
    rel = tol / min(float(c["horizontal"] @ c["u"]), float(c["vertical"] @ c["v"]))
    assert ((s >= x / nx - rel) & (s <= (x + 1) / nx + rel)).all(), "a ray leaves its pixel's column"
    assert ((t >= y / ny - rel) & (t <= (y + 1) / ny + rel)).all(), "a ray leaves its pixel's row (row 0 is the top: y = ny - 1)"
    assert ((r[..., 6] >= 0.0) & (r[..., 6] < 1.0)).all(), "a time outside [0, 1)"
    assert np.unique(r[..., 6]).size > 0.9 * r[..., 6].size, "the times repeat"

"""An independent float64 statement of the camera: the block Camera::look makes from its arguments, and the share of a pixel's
samples -- over pixel jitter, lens point and ray time -- whose ray meets an emitter.  For test_camera_oracle.py (the CPU
restatement) and test_camera_gpu.py (the HIP kernels).  Only numpy and math; nothing here is computed by the library except
the blocks and frames under test.

A. look: w = unit(from - at), u = unit(up x w), v = w x u; half_height = tan(fov / 2), half_width = aspect * half_height;
   llc = from - half_width f u - half_height f v - f w; horizontal = 2 half_width f u; vertical = 2 half_height f v;
   lens_radius = aperture / 2.  check_look compares every field of the block camera_look returns over POSES.
   Measured on the CPU restatement (test_camera_oracle.py prints them): worst deviation of origin / lower_left_corner /
   horizontal / vertical, relative to max(1, |from|, focus * half_width): 7.52e-07 (WORST_POINT; the 150 degree pose); of
   u / v, absolute: 2.49e-07 (WORST_BASIS; a pose whose `up` lies 3 degrees from the view: the cross product cancels there).  TOL_POINT and TOL_BASIS are 4 x those.
   lens_radius and the exposure are compared exactly.
B. shares: the worlds hold only emitters of colour L_EMIT on black, so a pixel's undivided sum is k L_EMIT with an integer k,
   binomial(ns, p).  p is computed here per pixel:
     rect worlds -- the lens plane is parallel to the rect, so "lens point (lx, ly) sends the ray through focal-plane point T
       into the rect" is an interval in lx times an interval in ly: the share is the area of the unit disc cut by a box, by
       the exact chord in ly and a midpoint rule over lens cells in lx (a cell the lx interval cuts counts by its covered
       part), then a midpoint rule over the footprint.  Without a lens (aperture 0, or the rect on the focal plane) the share is
       the covered part of the footprint in closed form.  Under LinearMove: the exact length of the time interval in which
       the displaced rect covers T (no lens), or a midpoint rule over the exposure (lens).
     spheres -- for a fixed lens point and footprint abscissa, |(C - O') x dir|^2 < r^2 |dir|^2 is a quadratic inequality in
       the footprint ordinate t; its solution set, cut to each row, is exact; midpoint rules over the abscissa and the lens.
   accept is the one acceptance of a frame against an expectation (thresholds as in test_light_sampling_gpu.py).
   `variant=` plants a wrong camera (VARIANTS); test_camera_oracle.py shows accept rejecting each.
   Measured on the CPU restatement, 32 x 24 x 1024, default seed (test_camera_oracle.py -s prints them; HISTORY.md has the table
   with every planted variant's chi2):
     world              class  chi2 / dof  worst |z|  frame z  others (worst |k - ns p|)  sure
     rect -z / +x 2.5     164   161.1 / 164     2.94     +0.07    604 (4.2)                 600
     rect -z / +x 4        56    50.5 /  56     2.32     +0.39    712 (0.0)                 712
     rect -z / +x 7       146   145.7 / 146     2.45     +0.90    622 (3.9)                 600
     spheres              164   164.5 / 164     3.85     +0.13    604 (3.6)                   -
     moving               152   132.6 / 152     2.57     +0.32    616 (5.7)                 590
     moving_lens          199   222.8 / 199     3.01     +0.48    569 (4.4)                 537
   (the views along -z and +x give the same counts, and so do the two worlds with company.)  Doubling every quadrature
   resolution moves a class pixel's share by 0.057 of its standard error at the most (spheres; the rect worlds 0.009)."""
import functools
import math

import numpy as np

F = np.float64
f32 = np.float32

WORST_POINT, WORST_BASIS = 7.6e-7, 2.5e-7      # measured: see the docstring
TOL_POINT, TOL_BASIS = 4 * WORST_POINT, 4 * WORST_BASIS
L_EMIT = (1.0, 0.5, 0.25)
NX, NY, NS = 32, 24, 1024
LOOK_VARIANTS = ("u_negated", "v_is_u_cross_w", "fov_is_half_angle", "no_focus_in_horizontal")
VARIANTS = ("pinhole", "radius_is_aperture", "square_lens", "radial_lens", "no_offset_in_direction", "centred_jitter", "rows_up",
            "mirrored", "unit_exposure", "shutter_opens_only", "mid_exposure", "moves_backwards", "time_from_lens_x")


def _r32(x):
    """What the binding hands the library: the value rounded to float32 (here as float64)."""
    return np.asarray(np.asarray(x, dtype=f32), dtype=F)


def _unit(a):
    return a / math.sqrt(float(a @ a))


# ---------------------------------------------------------------------------------------------------------------------------
# A. the camera block
# ---------------------------------------------------------------------------------------------------------------------------
def look(look_from, look_at, up, fov, aspect, aperture, focus_dist, variant=None):
    """The camera block of the arguments (rounded to float32 as the binding passes them), in float64."""
    o, at, up = _r32(look_from), _r32(look_at), _r32(up)
    fov, aspect, aperture, f = (float(_r32(x)) for x in (fov, aspect, aperture, focus_dist))
    w = _unit(o - at)
    u = _unit(np.cross(up, w))
    v = np.cross(w, u)
    if variant == "u_negated":
        u = -u
    if variant == "v_is_u_cross_w":
        v = np.cross(u, w)
    hh = math.tan(math.radians(fov) if variant == "fov_is_half_angle" else math.radians(fov) / 2.0)
    hw = aspect * hh
    return {"origin": o, "lower_left_corner": o - hw * f * u - hh * f * v - f * w,
            "horizontal": 2.0 * hw * (1.0 if variant == "no_focus_in_horizontal" else f) * u, "vertical": 2.0 * hh * f * v,
            "u": u, "v": v, "w": w, "lens_radius": aperture / 2.0, "focus": f, "half_width": hw, "half_height": hh}


def _pose(look_from, look_at, up, fov, aspect, aperture, focus):
    return {"from": look_from, "at": look_at, "up": up, "fov": fov, "aspect": aspect, "aperture": aperture, "focus": focus}


def _near_view(look_from, look_at, degrees):
    """An `up` that lies `degrees` from the view direction from -> at."""
    d = _unit(np.asarray(look_at, F) - np.asarray(look_from, F))
    side = _unit(np.cross(d, (0.3, 1.0, 0.2)))
    a = math.radians(degrees)
    return tuple(float(x) for x in math.cos(a) * d + math.sin(a) * side)


POSES = [
    _pose((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.1, 10.0),                   # book 1's
    _pose((2.0, 1.5, 4.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 30.0, 4.0 / 3.0, 0.6, 5.0),               # oblique
    _pose((-3.0, 4.0, -2.0), (1.0, -1.0, 0.5), (0.2, 1.0, -0.3), 90.0, 0.75, 0.25, 0.5),               # up not perpendicular; aspect < 1
    _pose((0.5, -0.25, 1.0), (0.5, -0.25, 0.0), (0.0, 1.0, 0.0), 40.0, 4.0 / 3.0, 0.5, 4.0),            # along -z
    _pose((0.5, -0.25, 1.0), (1.5, -0.25, 1.0), (0.0, 1.0, 0.0), 40.0, 4.0 / 3.0, 0.5, 4.0),            # along +x
    _pose((1.0, 2.0, 3.0), (4.0, 1.0, -2.0), (1.0, 0.1, 0.1), 150.0, 2.0, 0.0, 10.0),                  # up far from +y; very wide
    _pose((1.0, 2.0, 3.0), (4.0, 1.0, -2.0), _near_view((1.0, 2.0, 3.0), (4.0, 1.0, -2.0), 3.0), 20.0, 1.0, 1.0, 10.0),
    _pose((0.0, 0.0, 0.0), (0.0, -1.0, 0.2), _near_view((0.0, 0.0, 0.0), (0.0, -1.0, 0.2), 177.0), 90.0, 0.5, 0.1, 1000.0),
    _pose((6.0, 0.5, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.02, 1.0, 0.0, 10.0),                   # the beam poses' field of view
    _pose((600.0, 500.0, -620.0), (599.0, 499.5, -618.0), (0.0, 1.0, 0.0), 20.0, 1.5, 2.0, 1000.0),    # far from the origin
    _pose((-1000.0, 10.0, 5.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.02, 2.5, 0.5, 1000.0),              # far, narrow, up = +z
    _pose((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0),         # the Cornell box's
    _pose((0.0, 5.0, 0.0), (0.1, 0.0, 0.1), (1.0, 0.0, 0.0), 150.0, 0.4, 0.05, 0.5),                   # looking down
    _pose((3.0, -2.0, 7.0), (-2.0, 6.0, 1.0), (-0.5, -1.0, 0.3), 90.0, 1.7, 0.3, 0.5),                 # up pointing down: a rolled view
]
POINT_FIELDS, BASIS_FIELDS = ("origin", "lower_left_corner", "horizontal", "vertical"), ("u", "v")


def check_look(be, variant=None):
    """Every field of be.camera_look over POSES against look(): asserts the tolerances, returns the worst deviations
    (points, basis)."""
    worst_pt = worst_uv = 0.0
    for i, pose in enumerate(POSES):
        args = (pose["from"], pose["at"], pose["up"], pose["fov"], pose["aspect"], pose["aperture"], pose["focus"])
        cam = be.camera_look(*args, exposure=(0.25, 0.75))
        ref = look(*args, variant=variant)
        scale = max(1.0, math.sqrt(float(ref["origin"] @ ref["origin"])), ref["focus"] * ref["half_width"])
        for name in POINT_FIELDS:
            dev = float(np.abs(np.array(getattr(cam, name), F) - ref[name]).max()) / scale
            worst_pt = max(worst_pt, dev)
            assert dev <= TOL_POINT, ("pose %d: %s is off by %.3e of the pose's scale (tolerance %.3e)" % (i, name, dev, TOL_POINT))
        for name in BASIS_FIELDS:
            dev = float(np.abs(np.array(getattr(cam, name), F) - ref[name]).max())
            worst_uv = max(worst_uv, dev)
            assert dev <= TOL_BASIS, ("pose %d: %s is off by %.3e (tolerance %.3e)" % (i, name, dev, TOL_BASIS))
        assert cam.lens_radius == f32(ref["lens_radius"]), ("pose %d: lens_radius" % i, cam.lens_radius, ref["lens_radius"])
        assert (cam.exposure_start, cam.exposure_end) == (0.25, 0.75), ("pose %d: exposure" % i)
    return worst_pt, worst_uv


# ---------------------------------------------------------------------------------------------------------------------------
# B. the worlds
# ---------------------------------------------------------------------------------------------------------------------------
FROM = (0.5, -0.25, 1.0)
FOV, ASPECT, FOCUS = 40.0, NX / NY, 4.0
# the rect in pixel coordinates of the frame (x from the left, y from the BOTTOM): margins 5.3 left, 10.3 right, 4.4 below,
# 7.4 above -- a mirrored or upside-down frame differs; no edge on a pixel boundary
RECT_PIXELS = ((5.3, 21.7), (4.4, 16.6))


def _rect_world(view, dist, aperture=0.5, exposure=(0.0, 1.0), motion=None, company=False):
    """A rect perpendicular to the view, `dist` in front of FROM, covering RECT_PIXELS of a pinhole's frame.  company: the list
    also holds a Bvh of two emitter spheres BEHIND the camera (COMPANY), which no camera ray reaches: the same frame, but a
    world that has a second flat program, so that the pool-2 kernel can be made to render it."""
    hh = math.tan(math.radians(FOV) / 2.0)
    hw = ASPECT * hh
    iu = tuple(float(f32((2.0 * x / NX - 1.0) * hw * dist)) for x in RECT_PIXELS[0])
    iv = tuple(float(f32((2.0 * y / NY - 1.0) * hh * dist)) for y in RECT_PIXELS[1])
    if view == "-z":      # u = +x, v = +y
        at = (FROM[0], FROM[1], FROM[2] - 1.0)
        rect = (2, (FROM[0] + iu[0], FROM[0] + iu[1]), (FROM[1] + iv[0], FROM[1] + iv[1]), FROM[2] - dist)
    else:                 # "+x": u = +z, v = +y
        at = (FROM[0] + 1.0, FROM[1], FROM[2])
        rect = (0, (FROM[1] + iv[0], FROM[1] + iv[1]), (FROM[2] + iu[0], FROM[2] + iu[1]), FROM[0] + dist)
    return {"kind": "rect", "camera": (FROM, at, (0.0, 1.0, 0.0), FOV, ASPECT, aperture, FOCUS), "exposure": exposure,
            "rect": rect, "motion": motion, "company": company}


MOTION = (1.2, 0.0, 0.0)
WORLDS = {
    "rect_-z_2.5": _rect_world("-z", 2.5), "rect_-z_4": _rect_world("-z", 4.0), "rect_-z_7": _rect_world("-z", 7.0),
    "rect_+x_2.5": _rect_world("+x", 2.5), "rect_+x_4": _rect_world("+x", 4.0), "rect_+x_7": _rect_world("+x", 7.0),
    # three emitter spheres nearer than (depth 3), at (5) and beyond (8) the focal distance of an oblique camera
    "spheres": {"kind": "spheres", "camera": ((2.0, 1.5, 4.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 30.0, ASPECT, 0.6, 5.0),
                "exposure": (0.0, 1.0),
                "spheres": (((0.19, 0.99, 1.58), 0.25), ((0.15, -0.38, -0.3), 0.4), ((-0.16, 0.36, -3.84), 0.6))},
    "moving": _rect_world("-z", 4.0, aperture=0.0, exposure=(0.25, 0.75), motion=MOTION),
    "moving_lens": _rect_world("-z", 7.0, aperture=0.5, exposure=(0.25, 0.75), motion=MOTION),
    "rect_-z_2.5_company": _rect_world("-z", 2.5, company=True),
    "moving_lens_company": _rect_world("-z", 7.0, aperture=0.5, exposure=(0.25, 0.75), motion=MOTION, company=True),
}
COMPANY = (((0.5, -0.25, 6.0), 0.25), ((1.5, 0.5, 7.0), 0.25))     # (the -z view looks away from them)
FOCAL_PLANE = ("rect_-z_4", "rect_+x_4")
MIN_CLASS = {name: (20 if name in FOCAL_PLANE else 0 if name.endswith("_7") else 100) for name in WORLDS}
# the variants that change the lens alone, and those that change the ray's time alone (coincides)
_LENS = ("pinhole", "radius_is_aperture", "square_lens", "radial_lens", "no_offset_in_direction")
_TIME = ("unit_exposure", "shutter_opens_only", "mid_exposure", "moves_backwards", "time_from_lens_x")


def coincides(variant, name):
    """The planted variant gives the true expectation on this world (or is not defined there): nothing to reject."""
    spec = WORLDS[name]
    if variant in _TIME and spec.get("motion") is None:
        return True
    if variant == "time_from_lens_x":
        return not name.startswith("moving_lens")
    if variant == "no_offset_in_direction":      # (without the offset the focal plane itself is blurred)
        return spec["camera"][5] == 0.0
    if variant in _LENS:
        return name in FOCAL_PLANE or spec["camera"][5] == 0.0
    return False


def build(pkg, b, name):
    """(world, camera) of WORLDS[name] over the builder `b`."""
    S = pkg.scenes
    spec = WORLDS[name]
    light = b.diffuse_light(b.constant(S.v(*L_EMIT)), 1.0)
    if spec["kind"] == "rect":
        axis, r0, r1, k = spec["rect"]
        obj = b.rect(axis, r0, r1, k, light)
        if spec["motion"] is not None and spec["company"]:    # (a moving rect is no item of the second program; a moving Bvh is)
            obj = b.bvh([obj], (0.0, 1.0))
        if spec["motion"] is not None:
            obj = b.linear_move(obj, S.v(*spec["motion"]))
        world = [obj]
        if spec["company"]:
            world.append(b.bvh([b.translate(S.v(*c), b.sphere(r, light)) for c, r in COMPANY], (0.0, 1.0)))
    else:
        world = [b.bvh([b.translate(S.v(*c), b.sphere(r, light)) for c, r in spec["spheres"]], (0.0, 1.0))]
    c = spec["camera"]
    cam = b.be.camera_look(S.v(*c[0]), S.v(*c[1]), S.v(*c[2]), c[3], c[4], c[5], c[6], exposure=spec["exposure"])
    return world, cam


# ---------------------------------------------------------------------------------------------------------------------------
# B. the expectation
# ---------------------------------------------------------------------------------------------------------------------------
def _lens_measure(kind, x, y0, y1):
    """Probability mass of the lens points with abscissa in dx around x and ordinate in [y0, y1], per dx: the uniform disc,
    or the planted "square" (uniform on [-1, 1]^2) and "radial" (radius uniform, not its square root) lenses."""
    c = np.ones_like(x) if kind == "square" else np.sqrt(np.maximum(1.0 - x * x, 0.0))
    y0, y1 = np.clip(y0, -c, c), np.clip(y1, -c, c)
    if kind == "radial":
        ax = np.abs(x)
        out = (np.arcsinh(y1 / ax) - np.arcsinh(y0 / ax)) / (2.0 * math.pi)
    else:
        out = (y1 - y0) / (4.0 if kind == "square" else math.pi)
    return np.maximum(out, 0.0)


def _overlap(lo, hi, a0, a1):
    """Share of each interval [lo, hi] that lies in [a0, a1]."""
    return np.clip(np.minimum(hi, a1) - np.maximum(lo, a0), 0.0, None) / (hi - lo)


def _camera_model(spec, variant):
    cam = look(*spec["camera"])
    R = cam["lens_radius"]
    if variant == "pinhole":
        R = 0.0
    if variant == "radius_is_aperture":
        R = 2.0 * R
    kind = {"square_lens": "square", "radial_lens": "radial"}.get(variant, "disc")
    kappa = 0.0 if variant == "no_offset_in_direction" else 1.0      # the share of the lens offset taken off the direction
    jitter = -0.5 if variant == "centred_jitter" else 0.0
    return cam, R, kind, kappa, jitter


def _orient(p, variant):
    """Shares by (y from the bottom, x) to the frame's rows: row 0 is the top."""
    p = p if variant == "rows_up" else p[::-1]
    return np.ascontiguousarray(p[:, ::-1] if variant == "mirrored" else p)


def rect_shares(spec, nx, ny, variant=None, res=1):
    """(p [ny, nx] by frame row, sure [ny, nx]: +1 / -1 where geometry alone puts every sample inside / outside, else 0)."""
    cam, R, kind, kappa, jitter = _camera_model(spec, variant)
    o, u, v, w = cam["origin"], cam["u"], cam["v"], cam["w"]
    for c, r in COMPANY if spec["company"] else ():
        assert float((_r32(c) - o) @ w) > r + 1.0, "the company must stand behind the camera"
    m, L, nt = 32 * res, 1024 * res, 64 * res
    # the rect in camera coordinates: abscissa along u, ordinate along v, depth along -w
    axis, r0, r1, k = spec["rect"]
    a0, a1 = [a for a in range(3) if a != axis]
    corners = np.zeros((4, 3))
    corners[:, axis] = float(f32(k))
    corners[:, a0] = [float(f32(x)) for x in (r0[0], r0[0], r0[1], r0[1])]
    corners[:, a1] = [float(f32(x)) for x in (r1[0], r1[1], r1[0], r1[1])]
    cu, cv, cd = (corners - o) @ u, (corners - o) @ v, -((corners - o) @ w)
    assert np.ptp(cd) < 1e-9 and cd[0] > 0, "the rect must be perpendicular to the view and in front of it"
    (ua, ub), (va, vb), dist = (cu.min(), cu.max()), (cv.min(), cv.max()), cd[0]
    mo = np.zeros(3) if spec["motion"] is None else _r32(spec["motion"])
    mu = float(mo @ u) * (-1.0 if variant == "moves_backwards" else 1.0)
    assert abs(mo @ v) < 1e-12 and abs(mo @ w) < 1e-12, "the motion must be along u"
    e0, e1 = (float(f32(x)) for x in spec["exposure"])
    t0, t1 = (0.0, 1.0) if variant == "unit_exposure" else (e0, e1)
    if variant == "shutter_opens_only":
        t0 = t1 = e0
    if variant == "mid_exposure":
        t0 = t1 = 0.5 * (e0 + e1)
    if mu == 0.0:
        t0 = t1 = 0.0
    if t0 == t1:                       # one instant: a rect that stands displaced
        ua, ub, mu_eff = ua + t0 * mu, ub + t0 * mu, 0.0
    else:
        mu_eff = mu
    # the focal-plane point of (s, t) in the same coordinates, scaled to the rect's depth
    rel = cam["lower_left_corner"] - o
    focus = -float(rel @ w)
    tau = dist / focus
    assert abs(cam["vertical"] @ u) < 1e-12 and abs(cam["horizontal"] @ v) < 1e-12
    su0, su1 = tau * float(rel @ u), tau * float(cam["horizontal"] @ u)
    sv0, sv1 = tau * float(rel @ v), tau * float(cam["vertical"] @ v)
    kl = (1.0 - kappa * tau) * R        # the ray meets the rect's plane at tau T + kl (lx, ly)
    px_u = (np.arange(nx + 1) + jitter) / nx * su1 + su0      # pixel edges at the rect's depth
    px_v = (np.arange(ny + 1) + jitter) / ny * sv1 + sv0
    s_mid = su0 + su1 * (np.arange(nx * m) + 0.5 + jitter * m) / (nx * m)
    t_mid = sv0 + sv1 * (np.arange(ny * m) + 0.5 + jitter * m) / (ny * m)
    if abs(kl) < 1e-9:                  # no lens, or the rect on the focal plane: closed forms
        cover_v = _overlap(px_v[:-1], px_v[1:], va, vb)
        if mu_eff == 0.0:
            cover_u = _overlap(px_u[:-1], px_u[1:], ua, ub)
        else:
            if variant == "time_from_lens_x":
                raise ValueError("time_from_lens_x needs a lens")
            ta, tb = np.sort(np.stack([(s_mid - ua) / mu_eff, (s_mid - ub) / mu_eff]), axis=0)   # when the rect covers s
            share = np.clip(np.minimum(tb, t1) - np.maximum(ta, t0), 0.0, None) / (t1 - t0)
            cover_u = share.reshape(nx, m).mean(axis=1)
        p = np.outer(cover_v, cover_u)
    else:
        edges = np.linspace(-1.0, 1.0, L + 1)
        xc, dl = 0.5 * (edges[:-1] + edges[1:]), 2.0 / L
        ylo, yhi = np.sort(np.stack([(va - t_mid) / kl, (vb - t_mid) / kl]), axis=0)
        B = _lens_measure(kind, xc[None, :], ylo[:, None], yhi[:, None]).reshape(ny, m, L).mean(axis=1)
        if variant == "time_from_lens_x":
            times = [e0 + (e1 - e0) * 0.5 * (xc + 1.0)]
        elif mu_eff == 0.0:
            times = [0.0]
        else:
            times = list(t0 + (t1 - t0) * (np.arange(nt) + 0.5) / nt)
        A = np.zeros((nx, L))
        for time in times:
            shift = np.asarray(time * mu_eff)[None] if np.ndim(time) else time * mu_eff
            xlo, xhi = np.sort(np.stack(np.broadcast_arrays((ua + shift - s_mid[:, None]) / kl, (ub + shift - s_mid[:, None]) / kl)), axis=0)
            part = np.clip(np.minimum(xhi, edges[None, 1:]) - np.maximum(xlo, edges[None, :-1]), 0.0, None) / dl
            A += part.reshape(nx, m, L).mean(axis=1)
        A /= len(times)
        p = (B @ A.T) * dl
    # sure by geometry (the true camera's, whatever the variant): the footprint grown by the circle of confusion, the motion
    # over the exposure and 1e-3 of a pixel lies wholly inside or wholly outside the rect
    true = look(*spec["camera"])
    coc = true["lens_radius"] * abs(1.0 - tau)
    true_mu = float(mo @ u)
    sweep = sorted((e0 * true_mu, e1 * true_mu)) if spec["motion"] is not None else (0.0, 0.0)
    eu = np.arange(nx + 1) / nx * su1 + su0
    ev = np.arange(ny + 1) / ny * sv1 + sv0
    ua_t, ub_t = cu.min(), cu.max()

    def axis_sure(e, lo_in, hi_in, lo_out, hi_out):
        g = coc + 1e-3 * abs(e[1] - e[0])
        lo, hi = np.minimum(e[:-1], e[1:]) - g, np.maximum(e[:-1], e[1:]) + g
        return (lo >= lo_in) & (hi <= hi_in), (hi <= lo_out) | (lo >= hi_out)
    in_u, out_u = axis_sure(eu, ua_t + sweep[1], ub_t + sweep[0], ua_t + sweep[0], ub_t + sweep[1])
    in_v, out_v = axis_sure(ev, va, vb, va, vb)
    sure = np.where(in_v[:, None] & in_u[None, :], 1, np.where(out_v[:, None] | out_u[None, :], -1, 0))
    return _orient(p, variant), _orient(sure, None)


def _lens_points(kind, n):
    """Lens points (lx, ly) of equal weight: n rings of 2 n midpoints each, the rings' radii the square roots of midpoints --
    cells of equal area of the unit disc; "radial": the radii themselves the midpoints; "square": an n x n grid of [-1, 1]^2."""
    if kind == "square":
        g = -1.0 + (np.arange(n) + 0.5) * 2.0 / n
        return np.stack([np.repeat(g, n), np.tile(g, n)], axis=1)
    rho = (np.arange(n) + 0.5) / n
    rho = rho if kind == "radial" else np.sqrt(rho)
    phi = (np.arange(2 * n) + 0.5) * math.pi / n
    return np.stack([np.outer(rho, np.cos(phi)).ravel(), np.outer(rho, np.sin(phi)).ravel()], axis=1)


def sphere_shares(spec, nx, ny, variant=None, res=1):
    """p [ny, nx] by frame row for the spheres world (no sure pixels: the quadrature's zeros and ones are not exact).
    For a fixed lens point and footprint abscissa s the ray's direction is G + t V, linear in the footprint ordinate t, and
    |(C - O') x (G + t V)|^2 < r^2 |G + t V|^2 is a quadratic inequality in t: its solution set, cut to every row's [y / ny,
    (y + 1) / ny], is exact.  Midpoint rules over s and over lens cells of equal area.  (Exact in t, not in the lens ordinate:
    the sphere on the focal plane has a share that is a step in T, which no affordable footprint grid resolves.)"""
    cam, R, kind, kappa, jitter = _camera_model(spec, variant)
    o, u, v = cam["origin"], cam["u"], cam["v"]
    m, n = 128 * res, 12 * res      # (the abscissa is what converges last: measured, test_the_quadrature_has_converged)
    lens = _lens_points(kind, n) if R != 0.0 else np.zeros((1, 2))
    rel, H, V = cam["lower_left_corner"] - o, cam["horizontal"], cam["vertical"]
    s = (np.arange(nx * m) + 0.5 + jitter * m) / (nx * m)
    rows = (np.arange(ny + 1) + jitter) / ny
    VV = float(V @ V)
    total = np.zeros((ny, nx))
    seen = np.zeros((ny, nx), bool)
    for c, r in spec["spheres"]:
        c, r = _r32(c), float(f32(r))
        assert float((c - o) @ cam["w"]) < -r, "the sphere must stand in front of the camera"
        acc = np.zeros((ny, nx))
        for at in range(0, len(lens), 64):
            off = R * (lens[at:at + 64, :1] * u + lens[at:at + 64, 1:] * v)                        # [lens, xyz]
            A = (c - o) - off                                                                      # C - O'
            G = (rel + s[:, None] * H)[None, :, :] - kappa * off[:, None, :]                       # [lens, s, xyz]
            P = np.cross(A[:, None, :], G)
            Q = np.cross(A, V)[:, None, :]
            q2 = (Q * Q).sum(-1) - r * r * VV + 0.0 * G[..., 0]
            q1 = 2.0 * (P * Q).sum(-1) - 2.0 * r * r * (G @ V)
            q0 = (P * P).sum(-1) - r * r * (G * G).sum(-1)
            # q2 t^2 + q1 t + q0 < 0: between the roots (q2 > 0) or outside them (q2 < 0); both signs are handled
            assert (np.abs(q2) > 1e-12 * VV).all()
            disc = q1 * q1 - 4.0 * q2 * q0
            sq = np.sqrt(np.maximum(disc, 0.0))
            lo, hi = np.sort(np.stack([(-q1 - sq) / (2.0 * q2), (-q1 + sq) / (2.0 * q2)]), axis=0)
            # (only the columns and rows that some solution interval of this batch touches: the rest adds nothing)
            c0, c1, y0, y1 = 0, nx, 0, ny
            if (q2 > 0.0).all():
                hit = disc > 0.0
                if not hit.any():
                    continue
                cols = np.nonzero(hit.any(axis=0))[0]
                c0, c1 = cols[0] // m, cols[-1] // m + 1
                y0 = int(np.clip(np.searchsorted(rows, lo[hit].min()) - 1, 0, ny - 1))
                y1 = int(np.clip(np.searchsorted(rows, hi[hit].max()), y0 + 1, ny))
            cut, edges = slice(c0 * m, c1 * m), rows[y0:y1 + 1]
            inside = np.clip(np.minimum(hi[:, cut, None], edges[1:]) - np.maximum(lo[:, cut, None], edges[:-1]), 0.0, None)
            inside = np.where((disc > 0.0)[:, cut, None], inside, 0.0)
            part = np.where((q2 > 0.0)[:, cut, None], inside, (edges[1:] - edges[:-1]) - inside)     # [lens, s, row]
            acc[y0:y1, c0:c1] += part.reshape(len(off), c1 - c0, m, y1 - y0).sum(axis=(0, 2)).T
        share = acc * ny / (len(lens) * m)
        assert variant is not None or not (seen & (share > 0.0)).any(), "the spheres' images must be disjoint (the sum is their union)"
        seen |= share > 0.0
        total += share
    return _orient(total, variant)


@functools.lru_cache(maxsize=None)
def shares(name, variant=None, res=1, nx=NX, ny=NY):
    """(p, sure) of WORLDS[name]: computed once per (world, variant, resolution) and shared (read only) among the tests."""
    spec = WORLDS[name]
    if spec["kind"] == "rect":
        p, sure = rect_shares(spec, nx, ny, variant, res)
    else:
        p, sure = sphere_shares(spec, nx, ny, variant, res), None
    p = np.clip(p, 0.0, 1.0)
    p.setflags(write=False)
    if sure is not None:
        sure.setflags(write=False)
    return p, sure


# ---------------------------------------------------------------------------------------------------------------------------
# B. frames and their acceptance
# ---------------------------------------------------------------------------------------------------------------------------
def counts_of(frame, ns, partial):
    """The integer k of every pixel of a frame whose samples are all L_EMIT or zero: `frame` the undivided sums (partial) or the
    means over ns, a power of two.  Asserts that k is an integer and the channels stand 4 : 2 : 1 bit for bit."""
    frame = np.asarray(frame, f32)
    assert ns & (ns - 1) == 0 and ns <= 1 << 24
    sums = frame if partial else (frame * f32(ns)).astype(f32)
    k = sums[..., 0]
    assert (k == np.rint(k)).all() and (k >= 0).all() and (k <= ns).all(), "a pixel's sum is not a whole number of emitter hits"
    for ch, scale in ((1, 0.5), (2, 0.25)):
        want = (k * f32(scale)).astype(f32)
        assert np.array_equal(sums[..., ch].view(np.uint32), want.view(np.uint32)), "channel %d is not %g of channel 0, bit for bit" % (ch, scale)
    return k.astype(np.int64)


def render_counts(pkg, be, name, options=(), nx=NX, ny=NY, ns=NS, seed=0xDEADBEEF):
    """Counts of one par_cast frame of WORLDS[name] on `be`, scene options (name, value) set first.  The HIP library renders
    the undivided sums (partial=True); the restatement's binding hands back the mean whatever the flag."""
    b = be.builder()
    world, cam = build(pkg, b, name)
    scene = b.scene(world)
    for o, v in options:
        scene.set_option(o, v)
    partial = be.prefix == "rtg_"
    return counts_of(scene.par_cast(cam, nx, ny, ns, seed=seed, partial=partial), ns, partial)


def figures(k, p, ns):
    """The statistics accept asserts on: class sizes, z scores, chi2."""
    k, p = np.asarray(k, F), np.asarray(p, F)
    var = ns * p * (1.0 - p)
    cls = var >= 9.0
    dev = k - ns * p
    with np.errstate(all="ignore"):
        z = np.where(cls, dev / np.sqrt(np.where(cls, var, 1.0)), 0.0)
    dof = int(cls.sum())
    chi2 = float((z * z).sum())
    slack = np.abs(dev) - (4.0 + 5.0 * np.sqrt(var))
    total = var.sum()
    return {"class": dof, "worst_z": float(np.abs(z).max()) if dof else 0.0, "chi2": chi2, "dof": dof,
            "chi2_z": (chi2 - dof) / math.sqrt(2.0 * dof) if dof else 0.0,
            "frame_z": float(dev.sum() / math.sqrt(total)) if total > 0 else (0.0 if dev.sum() == 0 else math.inf),
            "others": int((~cls).sum()), "worst_other": float(np.abs(dev)[~cls].max()) if (~cls).any() else 0.0,
            "other_excess": float(slack[~cls].max()) if (~cls).any() else -math.inf}


def accept(k, p, ns, sure=None, min_class=0, what=""):
    """The one acceptance of a frame's counts `k` against the shares `p`: raises AssertionError, else returns figures()."""
    fig = figures(k, p, ns)
    assert fig["class"] >= min_class, "%s: %d pixels in the statistical class, fewer than %d" % (what, fig["class"], min_class)
    assert fig["worst_z"] <= 5.0, "%s: a pixel of the statistical class is %.2f standard errors off" % (what, fig["worst_z"])
    assert fig["chi2_z"] <= 5.0, "%s: chi2 %.1f over %d pixels" % (what, fig["chi2"], fig["dof"])
    assert abs(fig["frame_z"]) <= 4.0, "%s: the frame's total is %.2f standard errors off" % (what, fig["frame_z"])
    assert fig["other_excess"] <= 0.0, "%s: a pixel outside the statistical class is %.1f hits off" % (what, fig["worst_other"])
    fig["sure"] = 0
    if sure is not None:
        k = np.asarray(k)
        bad = ((sure > 0) & (k != ns)) | ((sure < 0) & (k != 0))
        assert not bad.any(), "%s: %d pixels that geometry puts wholly inside or outside the emitter say otherwise" % (what, bad.sum())
        fig["sure"] = int((sure != 0).sum())
    return fig


def line(name, fig):
    return "%-14s class %3d  chi2 %6.1f / %3d  worst |z| %.2f  frame z %+.2f  others %3d (worst %.1f)  sure %3d" % (
        name, fig["class"], fig["chi2"], fig["dof"], fig["worst_z"], fig["frame_z"], fig["others"], fig["worst_other"], fig.get("sure", 0))


def check_world(pkg, be, name, options=(), counts=None):
    """B on one frame of WORLDS[name] (or on `counts` already rendered): accept against the true expectation.  Returns
    (counts, figures)."""
    k = render_counts(pkg, be, name, options) if counts is None else counts
    p, sure = shares(name)
    fig = accept(k, p, NS, sure, MIN_CLASS[name], "%s %s" % (name, dict(options)))
    print(line(name, fig))
    return k, fig

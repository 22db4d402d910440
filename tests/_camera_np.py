"""The placed camera restated in numpy (include/rt_tile.h "placed camera"): the basis and the camera vectors of a pose in np.float32,
one ufunc per rounding, and Camera::get_ray for a pose drawing from the oracle's RNG (get_ray; ray_dots gives the two squared lengths
the same steps normalise; rays_of / strip_rays the records of a strip).  Test infrastructure: the product's own
arithmetic is csrc/rt_plan.h (host) and the kernels' camera arm (device)."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32

# tan(fov / 2) is the C library's tanf, as Camera::new's f32::tan and the host planner's std::tan(float) are (numpy's float32 tan is an
# implementation of its own and need not round alike)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.argtypes = [ctypes.c_float]
_libm.tanf.restype = ctypes.c_float


def _tanf(x):
    return f32(_libm.tanf(float(f32(x))))


def _cross(a, b):
    """(a x b), each component a*b - c*d with the two products rounded separately."""
    return np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]),
                     f32(a[2] * b[0]) - f32(a[0] * b[2]),
                     f32(a[0] * b[1]) - f32(a[1] * b[0])], f32)


def _dot3(a):
    """glam's dot3 of a vector with itself: (x x + y y) + z z, every product and sum rounded."""
    return f32(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2]))


def _length(a):
    return np.sqrt(_dot3(a))


def basis(origin, target, up):
    """(u, v, w) of a pose, or None where the library refuses it (a component that is not finite, a zero or non-finite length)."""
    o, t, p = (np.asarray(x, f32) for x in (origin, target, up))
    if not (np.isfinite(o).all() and np.isfinite(t).all() and np.isfinite(p).all()):
        return None
    with np.errstate(all="ignore"):
        d = (o - t).astype(f32)
        ld = _length(d)
        if not (ld > 0) or not np.isfinite(ld):
            return None
        w = (d / ld).astype(f32)
        c = _cross(p, w)
        lc = _length(c)
        if not (lc > 0) or not np.isfinite(lc):
            return None
        u = (c / lc).astype(f32)
        v = _cross(w, u)
    return u, v, w


def camera_vectors(rq, origin=None, target=None, up=None):
    """dict(org, llc, hor, ver, lens_u, lens_v: (3,) float32; lens_radius, focus_distance, u_den, v_den: float32) of the request's
    camera placed by the pose; origin None: the reference camera, its vectors written literally as Camera::new gives them."""
    with np.errstate(all="ignore"):
        aspect = f32(f32(rq.width) / f32(rq.height))
        vh = f32(f32(2.0) * _tanf(f32(f32(rq.fov) / f32(2.0))))
        vw = f32(aspect * vh)
        lr = f32(f32(rq.aperture) / f32(2.0))
        z = f32(0.0)
        if origin is None:
            org = np.zeros(3, f32)
            hor, ver, foc = np.array([vw, z, z], f32), np.array([z, vh, z], f32), np.array([z, z, f32(rq.focal_length)], f32)
            lens_u, lens_v = np.array([lr, z, z], f32), np.array([z, lr, z], f32)
        else:
            u, v, w = basis(origin, target, up)
            org = np.asarray(origin, f32)
            hor, ver, foc = (vw * u).astype(f32), (vh * v).astype(f32), (f32(rq.focal_length) * w).astype(f32)
            lens_u, lens_v = (lr * u).astype(f32), (lr * v).astype(f32)
        llc = (org - (hor / f32(2.0)).astype(f32)).astype(f32)
        llc = (llc - (ver / f32(2.0)).astype(f32)).astype(f32)
        llc = (llc - foc).astype(f32)
        return dict(org=org, llc=llc, hor=hor, ver=ver, lens_u=lens_u, lens_v=lens_v, lens_radius=lr,
                    focus_distance=f32(rq.focus_distance), u_den=f32(f32(aspect * f32(rq.height)) - f32(1.0)),
                    v_den=f32(f32(rq.height) - f32(1.0)))


def _normalize(a):
    """Ray::new's normalisation: division by the length (NaN for a zero vector)."""
    with np.errstate(all="ignore"):
        return (a / _length(a)).astype(f32)


def _normalize_or_zero(a):
    """glam normalize_or_zero: a * (1 / length), zero unless the reciprocal is finite and positive."""
    with np.errstate(all="ignore"):
        r = f32(f32(1.0) / _length(a))
        if np.isfinite(r) and r > 0:
            return (a * r).astype(f32)
    return np.zeros(3, f32)


def _ray_steps(oracle, cv, x, y_cam, state):
    """Camera::get_ray (camera.rs:109-129) step by step; returns (o, d, dot1, dot2), dot1 and dot2 the two squared lengths the steps
    normalise: of llc + u hor + v ver - org and of focal_point - o."""
    x1, x2 = (f32(t) for t in oracle.draw(state, 2))
    with np.errstate(all="ignore"):
        offset = ((x1 * cv["lens_u"]).astype(f32) + (x2 * cv["lens_v"]).astype(f32)).astype(f32)
        u = f32(f32(f32(x) + f32(oracle.draw(state, 0)[0])) / cv["u_den"])
        v = f32(f32(f32(y_cam) + f32(oracle.draw(state, 0)[0])) / cv["v_den"])
        t = (cv["llc"] + (u * cv["hor"]).astype(f32)).astype(f32)
        t = (t + (v * cv["ver"]).astype(f32)).astype(f32)
        t = (t - cv["org"]).astype(f32)
        d1 = _normalize(_normalize_or_zero(t))
        focal_point = (cv["org"] + (cv["focus_distance"] * d1).astype(f32)).astype(f32)
        o = (cv["org"] + offset).astype(f32)
        pre = (focal_point - o).astype(f32)
        d = _normalize(_normalize_or_zero(pre))
        return o, d, _dot3(t), _dot3(pre)


def get_ray(oracle, cv, rq, x, y_cam, state):
    """Camera::get_ray (camera.rs:109-129) of the camera vectors cv for pixel column x, camera row y_cam, drawing from `state`
    (advanced in place): the UnitDisc pair, then the u and the v jitter.  Returns (o, d): the lens point and the direction handed to
    ray_color."""
    return _ray_steps(oracle, cv, x, y_cam, state)[:2]


def ray_dots(oracle, cv, rq, x, y_cam, state):
    """The two squared lengths get_ray normalises for the same arguments (the operands of the device's two square roots before the
    last): (dot1 of llc + u hor + v ver - org, dot2 of focal_point - o), float32 each.  `state` is advanced as by get_ray."""
    return _ray_steps(oracle, cv, x, y_cam, state)[2:]


def sample_state(oracle, rq, x, yg, s):
    """The stream of sample s of pixel (x, global row yg) of the request's job: SmallRng::seed_from_u64(seed + 4 PHI ((yg W + x) S + s))."""
    return oracle.seed_from_u64(oracle.sample_seed(rq.seed, yg * rq.width + x, rq.spp, s))


def strip_records(rq, begin=0, end=None):
    """(x, global row, sample) of every record of samples [begin, end) of the request's strip, in the record order of
    rt_scene_camera_rays: pixel-major, sample-minor."""
    end = rq.spp if end is None else end
    hs = rq.height // rq.divisions
    return [(x, hs * rq.division_no + yl, s) for yl in range(hs) for x in range(rq.width) for s in range(begin, end)]


def rays_of(oracle, rq, pose, records, dots=False):
    """The camera rays of `records` ((x, global row, sample) each) of the request under `pose` ((origin, target, up) or None): (rays as
    a RAY_DTYPE array, states (n, 4) uint64 after get_ray's draws) and, with dots, an (n, 2) float32 array of ray_dots."""
    cv = camera_vectors(rq, *(pose if pose is not None else (None, None, None)))
    n = len(records)
    rays = np.zeros(n, oracle.RAY_DTYPE)
    states = np.zeros((n, 4), np.uint64)
    dd = np.zeros((n, 2), f32)
    for i, (x, yg, s) in enumerate(records):
        st = sample_state(oracle, rq, x, yg, s)
        o, d, dd[i, 0], dd[i, 1] = _ray_steps(oracle, cv, x, rq.height - 1 - yg, st)
        rays[i] = (o[0], o[1], o[2], rq.t_min, d[0], d[1], d[2], rq.t_max)
        states[i] = st
    return (rays, states, dd) if dots else (rays, states)


def strip_rays(oracle, rq, pose=None, begin=0, end=None, dots=False):
    """The camera rays of samples [begin, end) of every pixel of the request's strip under `pose` ((origin, target, up) or None), in
    the record order of rt_scene_camera_rays: (rays as a RAY_DTYPE array, states (n, 4) uint64 after get_ray's draws[, dots])."""
    return rays_of(oracle, rq, pose, strip_records(rq, begin, end), dots)

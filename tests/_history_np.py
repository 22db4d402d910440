"""The film history restated in numpy from the text of ray_tracer_s8_amd/history_csrc/rt_history.h: np.float32
throughout, one ufunc per rounding, whole planes at a time.  Test infrastructure: the product's own arithmetic is
history_csrc/rt_history_math.h (host and device).  Also the seeded synthetic frames the CPU and the GPU tests share."""
import numpy as np

import _camera_np as cnp

f32 = np.float32
NONE = np.uint32(0xFFFFFFFF)
REFERENCE_POSE = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))          # rt_camera_defaults
STATE = ("accum", "moments", "length", "depth", "index", "normal")


def _dot(a, b):
    """(a0 b0 + a1 b1) + a2 b2 of two vectors given as sequences of three planes or scalars."""
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(f32)


def cameras(rq, pose, prev_rq=None, prev_pose=None):
    """"Cameras, on the host": the current frame's vectors, and with prev_rq the previous frame's basis and plane.  pose: (origin,
    target, up) or None for the reference camera."""
    cur = cnp.camera_vectors(rq, *(pose if pose is not None else (None, None, None)))
    prev = None
    if prev_rq is not None:
        o, t, up = prev_pose if prev_pose is not None else REFERENCE_POSE
        u, v, w = cnp.basis(o, t, up)
        vh = f32(f32(2.0) * cnp._tanf(f32(f32(prev_rq.fov) / f32(2.0))))
        vw = f32(f32(f32(prev_rq.width) / f32(prev_rq.height)) * vh)
        pv = cnp.camera_vectors(prev_rq, o, t, up)
        prev = dict(org=np.asarray(o, f32), u=u, v=v, w=w, f=f32(prev_rq.focal_length), vw=vw, vh=vh, u_den=pv["u_den"], v_den=pv["v_den"])
    hs = rq.height // rq.divisions
    return dict(cur=cur, prev=prev, H=rq.height, y0=rq.division_no * hs)


def reproject(cam, W, R, z):
    """Steps 3 and 4 for every pixel of the film: (fx, fy, zp, front) as (R, W) planes; front: cz > 0."""
    c, p, H, y0 = cam["cur"], cam["prev"], cam["H"], cam["y0"]
    with np.errstate(all="ignore"):
        xs = np.arange(W, dtype=np.uint32).astype(f32)[None, :]
        rows = (np.uint32(H) - (np.uint32(y0) + np.arange(R, dtype=np.uint32)) - np.uint32(1)).astype(f32)[:, None]
        u = ((xs + f32(0.5)) / c["u_den"]).astype(f32)
        v = ((rows + f32(0.5)) / c["v_den"]).astype(f32)
        e = [(((c["llc"][i] + u * c["hor"][i]) + v * c["ver"][i]) - c["org"][i]).astype(f32) for i in range(3)]
        k = (f32(1.0) / np.sqrt(_dot(e, e))).astype(f32)
        ok = (k > 0) & (k < np.inf)
        e1 = [np.where(ok, e[i] * k, f32(0.0)).astype(f32) for i in range(3)]
        l = np.sqrt(_dot(e1, e1))
        d = [(e1[i] / l).astype(f32) for i in range(3)]
        q = [((c["org"][i] + z * d[i]) - p["org"][i]).astype(f32) for i in range(3)]
        cx, cy, cz = _dot(q, p["u"]), _dot(q, p["v"]), (-_dot(q, p["w"])).astype(f32)
        t = (p["f"] / cz).astype(f32)
        sx, sy = (cx * t).astype(f32), (cy * t).astype(f32)
        fx = ((sx / p["vw"] + f32(0.5)) * p["u_den"] - f32(0.5)).astype(f32)
        cv = ((sy / p["vh"] + f32(0.5)) * p["v_den"] - f32(0.5)).astype(f32)
        fy = ((f32(H - 1) - cv) - f32(y0)).astype(f32)
        zp = np.sqrt(_dot(q, q))
    return fx, fy, zp, cz > 0


def accumulate(cam, frame, prev, alpha, n_max, k_depth, k_normal=None):
    """One frame.  frame: dict(C (R, W, 3), M (R, W, 2), depth (R, W) f32, hits, index (R, W) uint32, normal (R, W, 3) or absent);
    prev: the state dict the last call returned, or None for a first frame (cam["prev"] is then not read).  Returns the next state:
    dict(accum, moments, length, depth, index, normal)."""
    C, M = np.asarray(frame["C"], f32), np.asarray(frame["M"], f32)
    depth, hits, idx = np.asarray(frame["depth"], f32), frame["hits"].view(np.uint32), frame["index"].view(np.uint32)
    R, W = depth.shape
    normals = k_normal is not None
    n = frame["normal"] if normals else None
    alpha, n_max, kd = f32(alpha), f32(n_max), f32(k_depth)
    kn2 = f32(f32(k_normal) * f32(k_normal)) if normals else f32(0)
    outC, outM = C.copy(), M.copy()
    outN = np.ones((R, W), f32)
    with np.errstate(all="ignore"):
        hit = hits != 0
        z = np.where(hit, depth / hits.astype(f32), f32(0.0)).astype(f32)
        nxt = dict(accum=outC, moments=outM, length=outN, depth=z, index=idx.copy(), normal=n.copy() if normals else None)
        if prev is None:
            return nxt
        act = hit & (idx != NONE)
        fx, fy, zp, front = reproject(cam, W, R, z)
        act &= front
        act &= (fx > f32(-1.0)) & (fx < f32(W)) & (fy > f32(-1.0)) & (fy < f32(R))
        fx, fy = np.where(act, fx, f32(0.0)), np.where(act, fy, f32(0.0))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0t = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = (fx - flx).astype(f32), (fy - fly).astype(f32)
        zlim = (kd * zp).astype(f32)
        if normals:
            nv = [n[..., i] for i in range(3)]
            nn = _dot(nv, nv)
        zero = np.zeros((R, W), f32)
        sw, s1, s2, sn = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        sc = [zero.copy() for _ in range(3)]
        anyt = np.zeros((R, W), bool)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = x0 + dx, y0t + dy
                adm = act & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < R)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, R - 1)              # (no address outside the film)
                Nq, iq, zq = prev["length"][qy, qx], prev["index"][qy, qx], prev["depth"][qy, qx]
                adm &= Nq >= f32(1.0)
                adm &= (iq != NONE) & (iq == idx)
                adm &= np.abs((zp - zq).astype(f32)) <= zlim
                if normals:
                    nq = [prev["normal"][qy, qx, i] for i in range(3)]
                    c = _dot(nv, nq)
                    adm &= (c > 0) & ((c * c).astype(f32) >= (kn2 * (nn * _dot(nq, nq)).astype(f32)).astype(f32))
                w = ((ax if dx else (f32(1.0) - ax).astype(f32)) * (ay if dy else (f32(1.0) - ay).astype(f32))).astype(f32)
                anyt |= adm
                sw = np.where(adm, sw + w, sw).astype(f32)
                for i in range(3):
                    sc[i] = np.where(adm, sc[i] + (w * prev["accum"][qy, qx, i]).astype(f32), sc[i]).astype(f32)
                s1 = np.where(adm, s1 + (w * prev["moments"][qy, qx, 0]).astype(f32), s1).astype(f32)
                s2 = np.where(adm, s2 + (w * prev["moments"][qy, qx, 1]).astype(f32), s2).astype(f32)
                sn = np.where(adm, sn + (w * Nq).astype(f32), sn).astype(f32)
        has = anyt & (sw > 0)
        N = ((sn / sw).astype(f32) + f32(1.0)).astype(f32)
        N = np.where(N > n_max, n_max, N).astype(f32)
        a = (f32(1.0) / N).astype(f32)
        a = np.where(alpha > a, alpha, a).astype(f32)
        b = (f32(1.0) - a).astype(f32)
        for i in range(3):
            outC[..., i] = np.where(has, (b * (sc[i] / sw).astype(f32)).astype(f32) + (a * C[..., i]).astype(f32), C[..., i])
        outM[..., 0] = np.where(has, (b * (s1 / sw).astype(f32)).astype(f32) + (a * M[..., 0]).astype(f32), M[..., 0])
        outM[..., 1] = np.where(has, (b * (s2 / sw).astype(f32)).astype(f32) + (a * M[..., 1]).astype(f32), M[..., 1])
        outN[...] = np.where(has, N, f32(1.0))
    return nxt


# ---- seeded synthetic frames ---------------------------------------------------------------------------------------------------------
def synthetic_frame(rng, rq, pose, R, k_depth, k_normal, e=4):
    """A frame of a film of R rows under `pose` that looks at the wall z = -5, tiled into primitives 0.7 wide: depth is the centre
    ray's distance to the wall, so that consecutive frames reproject onto each other, then perturbed so that every admission test
    has both outcomes: pixels without hits, RT_HIT_NONE, other indices, depths and normals just inside and just outside k_depth
    and k_normal, normals of zero length.  Colour sums and moments are random sums at e samples with a few fireflies."""
    W, H = rq.width, rq.height
    cam = cameras(rq, pose)
    c = cam["cur"]
    with np.errstate(all="ignore"):                # (a 1 x 1 frame has u_den = v_den = 0: its ray is NaN, and takes no history)
        xs = (np.arange(W) + 0.5) / float(c["u_den"])
        ys = (H - (cam["y0"] + np.arange(R)) - 1 + 0.5) / float(c["v_den"])
        d = (c["llc"].astype(np.float64)[None, None] + xs[None, :, None] * c["hor"].astype(np.float64)[None, None]
             + ys[:, None, None] * c["ver"].astype(np.float64)[None, None] - c["org"].astype(np.float64)[None, None])
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        d = np.where(np.isfinite(d).all(-1, keepdims=True), d, np.array([0.0, 0.0, -1.0]))
    t = (-5.0 - float(c["org"][2])) / np.where(d[..., 2] < -1e-6, d[..., 2], -1e-6)
    X = c["org"].astype(np.float64)[None, None] + t[..., None] * d
    index = (np.floor(X[..., 0] / 0.7).astype(np.int64) % 100 + 128 * (np.floor(X[..., 1] / 0.7).astype(np.int64) % 100)).astype(np.uint32)
    hits = rng.integers(1, e + 1, (R, W)).astype(np.uint32)
    pick = rng.random((R, W))
    scale = np.ones((R, W))
    for lo, hi, s in ((0.00, 0.06, 1 + 0.6 * k_depth), (0.06, 0.12, 1 + 1.6 * k_depth), (0.12, 0.15, 1 - 1.6 * k_depth)):
        scale[(pick >= lo) & (pick < hi)] = s
    z = (t * scale).astype(f32)
    pick = rng.random((R, W))
    index[pick < 0.05] = NONE
    other = (pick >= 0.05) & (pick < 0.10)
    index[other] = index[other] + np.uint32(7)
    hits[(pick >= 0.10) & (pick < 0.16)] = 0
    depth = (z * hits.astype(f32)).astype(f32)
    # normals: the wall's +z times hits, tilted about y by an angle whose cosine against the untilted one is just inside or outside
    kn = 0.9 if k_normal is None else float(k_normal)
    ang = np.zeros((R, W))
    pick = rng.random((R, W))
    ang[(pick < 0.06)] = np.arccos(min(1.0, kn)) * 0.9
    ang[(pick >= 0.06) & (pick < 0.12)] = np.arccos(min(1.0, kn)) * 1.1 + 0.02
    ang[(pick >= 0.12) & (pick < 0.14)] = 2.5
    normal = np.stack([np.sin(ang), np.zeros((R, W)), np.cos(ang)], -1) * hits[..., None]
    normal[(pick >= 0.14) & (pick < 0.16)] = 0.0
    normal = normal.astype(f32)
    Cc = (rng.random((R, W, 3)) * e).astype(f32)
    Cc[rng.random((R, W)) < 0.01] *= f32(40.0)
    y = ((Cc[..., 0] + Cc[..., 1]) + Cc[..., 2]).astype(f32)
    M = np.stack([y, (y * y / f32(e)) * (f32(1.0) + rng.random((R, W)).astype(f32))], -1).astype(f32)
    return dict(C=Cc, M=M, depth=depth, hits=hits, index=index, normal=normal)

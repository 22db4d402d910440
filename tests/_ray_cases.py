"""Caller-ray cases shared by tests/test_oracle_batch.py (CPU) and tests/test_gpu_ray_fuzz.py (GPU): the ray populations of the
differential fuzz, its case generator, the scenes of the plan branches and the g++ plan harnesses as plain functions.  Everything
here is a pure function of a case number and of the CPU oracle's answers — nothing reads a GPU result."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from ray_tracer_s8_amd import _abi, scenes

from test_gpu_fuzz import _big_case, _mixed_case, _random_case, _world_order

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
HOST = ROOT / "tests" / "host"
F = _abi
NONE = _abi.RT_HIT_NONE
T_MIN, T_MAX = np.float32(0.001), np.float32(1000.0)          # the reference's window (S/shapes/mod.rs:12-13)
BOUNCES = [0, 1, 3, 10, 25, 62]
SPPS = [1, 2, 5]


# ---------------------------------------------------------------- the g++ harnesses over the product's host code
def _harness(name, extra=()):
    src, out = HOST / f"{name}.cpp", HOST / "_build" / f"lib{name}.so"
    deps = [src, CSRC / "rt_plan.h", CSRC / "rt_consts.h", CSRC / "rt_bvh.h", ROOT / "include" / "rt_tile.h"]
    out.parent.mkdir(exist_ok=True)
    if not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", f"-I{CSRC}",
                        f"-I{ROOT / 'include'}", *extra, "-o", str(out), str(src)], check=True)
    return C.CDLL(str(out))


def trace_plan(n_sph, n_tri, depth, inverted, flags, bounces):
    """rtplan::plan_trace (tests/host/trace_plan_host.cpp) for a scene shape."""
    lib = _harness("trace_plan_host")
    lib.trace_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    sh = np.array([n_sph, n_tri, depth, int(inverted)], np.uint32)
    out = np.zeros(7, np.uint64)
    lib.trace_plan(sh.ctypes.data, flags, bounces, out.ctypes.data)
    return dict(engine=int(out[0]), scan_mode=int(out[1]), full_chain=bool(out[2]), block=int(out[3]), path32=bool(out[4]),
                path_off=int(out[5]), lds=int(out[6]))


def query_plan(n_sph, n_tri, depth, inverted, flags):
    """rtplan::plan_query (tests/host/query_plan_host.cpp) for a scene shape."""
    lib = _harness("query_plan_host")
    lib.query_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    sh = np.array([n_sph, n_tri, depth, int(inverted)], np.uint32)
    out = np.zeros(4, np.uint64)
    lib.query_plan(sh.ctypes.data, flags, out.ctypes.data)
    return dict(engine=int(out[0]), scan_mode=int(out[1]), full_chain=bool(out[2]), lds=int(out[3]))


def trav_stack():
    lib = _harness("trace_plan_host")
    lib.trace_trav_stack.restype = C.c_uint32
    return int(lib.trace_trav_stack())


def prim_boxes(sph, tri):
    """The primitives' boxes as the reference forms them (sphere.rs:65-72 centre -+ radius, mesh.rs:46-96 min / max), float32."""
    out = []
    if sph is not None and len(sph):
        c = np.stack([sph["cx"], sph["cy"], sph["cz"]], 1).astype(np.float32)
        r = sph["radius"].astype(np.float32)[:, None]
        out.append(np.concatenate([c - r, c + r], 1))
    if tri is not None and len(tri):
        v = np.stack([tri["a"], tri["b"], tri["c"]], 1).astype(np.float32)
        out.append(np.concatenate([v.min(1), v.max(1)], 1))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def tree_depth(sph, tri):
    """Depth of the product's tree over the scene in storage order (tests/host/bvh_host.cpp host_bvh_check; structure checked)."""
    lib = _harness("bvh_host")
    b = prim_boxes(sph, tri)
    out = np.zeros(3, np.uint32)
    rc = lib.host_bvh_check(b.ctypes.data_as(C.c_void_p), C.c_uint32(len(b)), out.ctypes.data_as(C.c_void_p))
    assert rc not in (1, 2, 7), rc       # node count, leaf order, depth (3 - 6: inverted boxes and the quantised twin, not used here)
    return int(out[2])


# ---------------------------------------------------------------- rays
def make_rays(o, d, t_min=T_MIN, t_max=T_MAX):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    r = np.empty(len(o), _abi.RAY_DTYPE)
    r["ox"], r["oy"], r["oz"] = o.T
    r["dx"], r["dy"], r["dz"] = d.T
    r["t_min"] = np.broadcast_to(np.asarray(t_min, np.float32), (len(o),))
    r["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), (len(o),))
    return r


def od(rays):
    return np.stack([rays["ox"], rays["oy"], rays["oz"]], 1), np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)


def _unit(g, n):
    v = g.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _surface_points(g, sph, tri, n):
    """n points exactly on primitives, as float32 arithmetic gives them: sphere surface points c + r u, triangle vertices and
    edge midpoints; and for each the centre of its primitive (a direction towards it hits something)."""
    ns, nt = len(sph), len(tri)
    pts, ctr = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    pick = g.integers(0, ns + nt, n)
    u = _unit(g, n)
    which = g.integers(0, 6, n)
    for k in range(n):
        j = int(pick[k])
        if j < ns:
            c = np.array([sph["cx"][j], sph["cy"][j], sph["cz"][j]], np.float32)
            pts[k] = c + np.float32(sph["radius"][j]) * u[k]
            ctr[k] = c
        else:
            t = tri[j - ns]
            a, b, c = (np.asarray(t[f], np.float32) for f in ("a", "b", "c"))
            pts[k] = (a, b, c, (a + b) / np.float32(2), (b + c) / np.float32(2), (a + c) / np.float32(2))[which[k]]
            ctr[k] = (a + b + c) / np.float32(3)
    return pts, ctr


def ray_population(oracle, g, sph, tri, n, wi=None, aim_at=()):
    """n rays drawn from the scene's bounds, every window the ray's own.  Origins outside, inside and exactly on primitives;
    directions isotropic, aimed at a primitive, axis-aligned with +-0 components, and scaled by 1e-20 ... 1e20; windows: the
    reference's, narrow ones that cut the nearest hit off (from the oracle's hit under the reference's window), t_max = inf,
    t_min == t_max, t_min > t_max.  aim_at: primitives (storage indices) that get rays of their own with the reference's window
    (the duplicated ones of a tie case).  Returns (rays, narrow mask, the oracle's backend-1 hits under the reference's window)."""
    ns, nt = len(sph), len(tri)
    assert ns + nt > 0
    pts = [np.stack([sph["cx"], sph["cy"], sph["cz"]], 1)] if ns else []
    if nt:
        pts += [np.asarray(tri[f], np.float32) for f in ("a", "b", "c")]
    p = np.concatenate(pts).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = 0.5 * (hi - lo) + 1.0
    surf, ctr = _surface_points(g, sph, tri, n)
    kind = g.integers(0, 4, n)                                   # 0 outside / around, 1 inside the bounds, 2 on a primitive, 3 at a centre
    o = g.uniform(lo - ext, hi + ext, (n, 3)).astype(np.float32)
    inside = g.uniform(lo, hi, (n, 3)).astype(np.float32)
    o[kind == 1] = inside[kind == 1]
    o[kind == 2] = surf[kind == 2]
    o[kind == 3] = ctr[kind == 3]
    # directions
    d = _unit(g, n)
    dk = g.integers(0, 4, n)                                     # 0 isotropic, 1 aimed, 2 axis-aligned, 3 aimed with jitter
    tgt, tctr = _surface_points(g, sph, tri, n)
    aimed = (tctr - o).astype(np.float32)
    aimed[kind == 3] = (tgt - o)[kind == 3]                      # (from a centre: towards another primitive's surface)
    d[dk == 1] = aimed[dk == 1]
    jit = aimed + (0.05 * np.linalg.norm(aimed, axis=1, keepdims=True) * g.normal(size=(n, 3))).astype(np.float32)
    d[dk == 3] = jit[dk == 3]
    ax = np.zeros((n, 3), np.float32)
    ax[np.arange(n), g.integers(0, 3, n)] = 1.0
    ax *= g.choice([-1.0, 1.0], (n, 1)).astype(np.float32)
    ax = np.where(ax == 0, g.choice([0.0, -0.0], (n, 3)).astype(np.float32), ax)       # +-0 components
    d[dk == 2] = ax[dk == 2]
    zero = np.all(d == 0, 1)
    d[zero] = (0.0, 0.0, -1.0)
    scale = np.where(g.uniform(size=n) < 0.3, 10.0 ** g.uniform(-20, 20, n), 1.0).astype(np.float32)
    scale[dk == 2] = np.where(g.uniform(size=int((dk == 2).sum())) < 0.5, scale[dk == 2], 1.0)
    d = (d * scale[:, None]).astype(np.float32)
    # the rays of their own of the primitives to aim at: from outside the primitive straight at it, and from its surface inwards
    if len(aim_at):
        eo, ed = [], []
        for j in aim_at:
            for u in _unit(g, 6):
                if j < ns:
                    c, r = np.array([sph["cx"][j], sph["cy"][j], sph["cz"][j]], np.float32), np.float32(abs(sph["radius"][j]))
                    eo.append(c + np.float32(1.5) * r * u)
                    ed.append(-u)
                else:
                    t = tri[j - ns]
                    a, b, c = (np.asarray(t[f], np.float32) for f in ("a", "b", "c"))
                    m = (a + b + c) / np.float32(3)
                    nrm = np.cross(b - a, c - a).astype(np.float32)
                    s = np.float32(1.0 if u[0] > 0 else -1.0) * np.float32(0.1)
                    eo.append(m + s * nrm)
                    ed.append(-s * nrm)
        k = min(len(eo), n // 4)
        o[:k], d[:k] = np.array(eo[:k], np.float32), np.array(ed[:k], np.float32)
    rays = make_rays(o, d)
    # windows, per ray
    ref = oracle.intersect_batch(sph, tri, rays, backend=1, world_index=wi)
    dist = np.linalg.norm(ref["point"].astype(np.float64) - o, axis=1)
    wk = g.choice(6, n, p=[0.45, 0.2, 0.1, 0.1, 0.075, 0.075])
    if len(aim_at):
        wk[:min(6 * len(aim_at), n // 4)] = 0
    narrow = np.zeros(n, bool)
    for i in range(n):
        if wk[i] == 1 and ref["hit"][i] and dist[i] > 0.002:     # the nearest hit cut off: from the front ...
            rays["t_min"][i] = np.float32(dist[i] * (1 + 1e-3))
            narrow[i] = True
        elif wk[i] == 2 and ref["hit"][i] and dist[i] > 0.002:   # ... and by a window that ends before it
            rays["t_max"][i] = np.float32(dist[i] * (1 - 1e-3))
            narrow[i] = True
        elif wk[i] == 3:
            rays["t_max"][i] = np.inf
        elif wk[i] == 4:
            rays["t_min"][i] = rays["t_max"][i] = np.float32(g.uniform(0.5, 20.0))
        elif wk[i] == 5:
            rays["t_min"][i], rays["t_max"][i] = np.float32(10.0), np.float32(g.uniform(0.0, 5.0))
    return rays, narrow, ref


def states(n, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)


def duplicated(sph, tri):
    """Storage indices of the primitives whose geometry another primitive shares exactly."""
    out = []
    for arr, geo, base in ((sph, ("cx", "cy", "cz", "radius"), 0), (tri, ("a", "b", "c"), len(sph))):
        if not len(arr):
            continue
        key = np.concatenate([np.asarray(arr[f], np.float32).reshape(len(arr), -1) for f in geo], 1)
        _, inv, cnt = np.unique(key.view(np.uint32), axis=0, return_inverse=True, return_counts=True)
        out += [base + int(k) for k in np.nonzero(cnt[inv.reshape(-1)] > 1)[0]]
    return out


# ---------------------------------------------------------------- the fuzz cases
CONFIG_NAMES = ["default", "bvh_traverse", "full_chain", "exact_scan", "linear_scan", "no_bvh_cull", "ignored_flags"]
N_RAYS = {"small": 512, "big": 768, "mixed": 768}


def case_scene(kind, i):
    """(sph, tri, world_index or None, tile request of the generator) of case i.  small: test_gpu_fuzz._random_case (the next
    non-empty one when the draw is an empty world: an empty world has no hits to compare) with _world_order's permuted world
    and duplicates on every third case; big: _big_case; mixed: _mixed_case (odd cases permuted, with duplicates)."""
    if kind == "small":
        j = i
        sph, tri, rq, _ = _random_case(j)
        while len(sph) + len(tri) == 0 or (i % 3 == 1 and len(sph) + len(tri) < 2):
            j += 1000
            sph, tri, rq, _ = _random_case(j)
        sph, tri, wi = _world_order(i, sph, tri)
        return sph, tri, wi, rq
    if kind == "big":
        sph, rq, _ = _big_case(i)
        return sph, np.zeros(0, _abi.TRIANGLE_DTYPE), None, rq
    sph, tri, wi, rq, _ = _mixed_case(i)
    return sph, tri, wi, rq


def case_config(kind, i):
    """The CONFIGS entry of case i: cycling, shifted once per round so that every config meets every scene size."""
    off = {"small": 0, "big": 3, "mixed": 5}[kind]
    return CONFIG_NAMES[(i + i // len(CONFIG_NAMES) + off) % len(CONFIG_NAMES)]


def fuzz_case(oracle, kind, i, configs):
    """Everything case i needs, and the conditions that keep it from passing vacuously, asserted from the oracle alone.
    The bounce limit is drawn from BOUNCES; a draw >= 10 on a scene where no ray of the population reaches 4 segments (a
    single sphere, say) is drawn again from the limits below 10, so that every case with a deep limit has deep paths."""
    sph, tri, wi, rq = case_scene(kind, i)
    cfg = case_config(kind, i)
    flags, engine, backend = configs[cfg]
    g = np.random.default_rng({"small": 31000, "big": 32000, "mixed": 33000}[kind] + i)
    dup = duplicated(sph, tri) if wi is not None else []
    rays, narrow, ref = ray_population(oracle, g, sph, tri, N_RAYS[kind], wi, aim_at=dup[:16])
    mb, spp = int(g.choice(BOUNCES)), int(g.choice(SPPS))
    st0 = states(len(rays), 9000 + i)
    seed = int(g.integers(0, 2**63))
    kw = dict(backend=backend, world_index=wi)
    hits = oracle.intersect_batch(sph, tri, rays, **kw)
    assert hits["hit"].any() and not hits["hit"].all(), (kind, i, "hits and misses")
    if narrow.any():                                             # a narrow window changes the closest hit of some ray
        wide = rays.copy()
        wide["t_min"][narrow], wide["t_max"][narrow] = T_MIN, T_MAX
        unw = oracle.intersect_batch(sph, tri, wide, **kw)
        cut = narrow & ((hits["index"] != unw["index"]) | np.any(hits["point"].view(np.uint32) != unw["point"].view(np.uint32), 1))
        assert cut.any(), (kind, i, "no narrow window changed a hit")
    if dup:                                                      # a real tie: some ray's hit is a duplicated primitive
        pos = np.arange(len(sph) + len(tri), dtype=np.uint32) if wi is None else wi
        assert np.isin(hits["index"][hits["hit"]], pos[dup]).any(), (kind, i, "no ray hits a duplicated primitive")

    def longest_path(bounces):
        return int(oracle.trace_batch(sph, tri, rays, spp=1, max_bounces=bounces, states=st0, **kw)[1].max())

    if mb >= 10 and longest_path(mb) < 4:
        mb = int(g.choice([0, 1, 3]))
    assert mb < 10 or longest_path(mb) >= 4, (kind, i, mb, "no path reaches 4 segments")
    trace = oracle.trace_batch(sph, tri, rays, spp=spp, max_bounces=mb, states=st0, **kw)
    return dict(sph=sph, tri=tri, wi=wi, rq=rq, cfg=cfg, flags=flags, engine=engine, backend=backend, rays=rays, narrow=narrow,
                mb=mb, spp=spp, states=st0, seed=seed, hits=hits, trace=trace, dup=dup)


# ---------------------------------------------------------------- scenes of the plan branches
def field70000():
    """scenes.rand65536(n=70000) with sixty of its spheres made perfect mirrors that do not emit: a ray that starts inside one
    is reflected inside it until the depth runs out."""
    sph = scenes.rand65536(n=70000).copy()
    k = np.arange(100, 70000, 1165)[:60]
    sph["roughness"][k], sph["emission"][k] = 1.0, 0.0
    return sph, k


def mirror_rays(g, sph, k, per=4):
    """Rays from the centres of the spheres k, any direction."""
    c = np.stack([sph["cx"][k], sph["cy"][k], sph["cz"][k]], 1).astype(np.float32)
    return make_rays(np.repeat(c, per, 0), _unit(g, per * len(k)))


def odd_radii_world():
    """The negative-, zero-, tiny- and subnormal-radius spheres of test_gpu_parity (odd_radii, subnormal_values) in one field."""
    g = np.random.default_rng(860)
    n = 1500
    sph = np.zeros(n, _abi.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"] = g.uniform(-12, 12, n), g.uniform(-2, 8, n), g.uniform(-30, -2, n)
    sph["radius"] = g.uniform(0.1, 0.5, n)
    sph["radius"][:150] = 0.0
    sph["radius"][150:450] = -g.uniform(0.1, 0.5, 300)
    sph["radius"][450:600] = 1e-6
    sph["radius"][600:700] = 1e-41
    sph["cx"][700:720] = g.uniform(-1, 1, 20) * 1e-40
    for c in ("albedo_r", "albedo_g", "albedo_b"):
        sph[c] = g.uniform(0.2, 0.9, n)
    sph["roughness"] = g.choice([0.0, 0.5, 1.0], n)
    sph["emission"] = np.where(g.uniform(size=n) < 0.02, 4.0, 0.0)
    return sph


def pile_world():
    """test_gpu_parity.test_thousands_of_identical_spheres: 2 000 copies of each of two spheres and a ground."""
    sph = np.zeros(4001, _abi.SPHERE_DTYPE)
    sph["cx"][:2000], sph["cy"][:2000], sph["cz"][:2000], sph["radius"][:2000] = -1.5, 0.5, -6.0, 1.5
    sph["cx"][2000:4000], sph["cy"][2000:4000], sph["cz"][2000:4000], sph["radius"][2000:4000] = 1.8, 0.2, -5.0, 1.2
    sph["cx"][4000], sph["cy"][4000], sph["cz"][4000], sph["radius"][4000] = 0.0, -101.0, -6.0, 100.0
    g = np.random.default_rng(5)
    for c in ("albedo_r", "albedo_g", "albedo_b"):
        sph[c] = g.uniform(0.2, 0.95, 4001)
    sph["roughness"][:2000] = 1.0
    return sph


def chain_world(n):
    """n spheres whose tree is a chain: centres 7^k (k = -5, -4, ...) along x, y and z in turn, radius a quarter of that.  On the
    axis the builder splits, the largest centroid falls in the last of the six SAH buckets and every other one in the first (1/7
    of the extent), so every split peels exactly one sphere off and the depth is n - 1.  From 7^-5 = 6e-5 (above the builder's
    epsilon of 1e-5, below which it halves) to 7^20 = 8e16 at most: count x surface area, the SAH cost, stays finite in float32
    (beyond 7^21 it is inf, no split beats inf, and the reference's builder keeps two EMPTY child boxes)."""
    assert n <= 78
    sph = np.zeros(n, _abi.SPHERE_DTYPE)
    g = np.random.default_rng(7000 + n)
    for j in range(n):
        k, axis = j // 3 - 5, j % 3
        x = np.float32(7.0) ** np.float32(k)
        sph[("cx", "cy", "cz")[axis]][j] = x
        sph["radius"][j] = np.float32(0.25) * x
    for c in ("albedo_r", "albedo_g", "albedo_b"):
        sph[c] = g.uniform(0.3, 0.95, n)
    sph["roughness"] = g.choice([0.0, 1.0, 1.0], n)
    return sph


def chain_rays(g, sph, n):
    """Rays among the spheres of chain_world: from the centres and surfaces of some towards others, and from far outside."""
    c = np.stack([sph["cx"], sph["cy"], sph["cz"]], 1).astype(np.float32)
    a, b = g.integers(0, len(sph), n), g.integers(0, len(sph), n)
    u = _unit(g, n)
    o = (c[a] + (sph["radius"][a] * g.choice([0.0, 1.0, 3.0], n)).astype(np.float32)[:, None] * u).astype(np.float32)
    tgt = (c[b] + (sph["radius"][b] * np.float32(0.7))[:, None] * _unit(g, n)).astype(np.float32)
    d = np.where((g.uniform(size=n) < 0.8)[:, None], tgt - o, _unit(g, n)).astype(np.float32)
    d[np.all(d == 0, 1)] = (1.0, 0.0, 0.0)
    return make_rays(o, d, T_MIN, np.inf)

"""The host's scene derivation (csrc/rt_scene_host.h build_host_scene, through the g++ harness tests/host/scene_host.cpp): from the
primitive lists to every array the library uploads and every SceneShape value the engine rules read, on the CPU.

(a) pinned: tests/golden/scene_host.json holds, per corpus scene, a SHA-256 of the input, the scalar outputs (floats as bit
    patterns) and a SHA-256 of every output array, recorded from the function as it stood in rt_api.hip before it moved to the
    header.  A change to a threshold, a layout or the storage order re-records the golden ON PURPOSE and says why.
(b) properties of the same outputs, so that such a change has more than a hash to be judged by.
(c) the engine plan_launch (rt_plan.h, through tests/host/plan_host.cpp) chooses for each derived shape."""
import ctypes as C
import hashlib
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _rule_scenes
import test_launch_plan as LP
from ray_tracer_s8_amd import scenes
from ray_tracer_s8_amd._abi import SPHERE_DTYPE, TRIANGLE_DTYPE
from test_launch_plan import lib as plan_lib  # noqa: F401  (the plan harness, as a fixture of this module)

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ray_tracer_s8_amd" / "csrc"
SRC = ROOT / "tests" / "host" / "scene_host.cpp"
OUT = ROOT / "tests" / "host" / "_build" / "libscene_host.so"
DEPS = [SRC, CSRC / "rt_scene_host.h", CSRC / "rt_bvh.h", CSRC / "rt_consts.h"]
GOLDEN = ROOT / "tests" / "golden" / "scene_host.json"
LEAF_BIT = 0x80000000
REORDER_MIN_PRIMS = 64
FRAMES = {"2560x1440": (2560, 1440), "256x256": (256, 256)}


def load(path):
    l = C.CDLL(str(path))
    l.scene_scalar_names.restype = C.c_char_p
    l.scene_array_names.restype = C.c_char_p
    l.scene_build.restype = C.c_void_p
    l.scene_build.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    l.scene_free.argtypes = [C.c_void_p]
    l.scene_scalars.argtypes = [C.c_void_p, C.c_void_p]
    l.scene_array.restype = C.c_void_p
    l.scene_array.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    l.scene_world_is_permutation.argtypes = [C.c_void_p, C.c_uint32]
    l.scene_tri_measures.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    return l


@pytest.fixture(scope="module")
def host():
    OUT.parent.mkdir(exist_ok=True)
    if not OUT.exists() or OUT.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", f"-I{CSRC}",
                        f"-I{ROOT / 'include'}", "-o", str(OUT), str(SRC)], check=True)
    return load(OUT)


# ------------------------------------------------------------------------------------------------------------ corpus


def _spheres(g, n, centre=(0.0, 1.0, -12.0), spread=6.0, rr=(0.1, 0.4)):
    s = np.zeros(n, SPHERE_DTYPE)
    c = g.uniform(-spread, spread, (n, 3)) + np.array(centre)
    s["cx"], s["cy"], s["cz"] = c[:, 0], c[:, 1], c[:, 2]
    s["radius"] = g.uniform(*rr, n)
    s["albedo_r"], s["albedo_g"], s["albedo_b"] = g.uniform(0.1, 0.9, (3, n))
    s["roughness"] = g.random(n)
    s["emission"] = np.where(g.random(n) < 0.1, 3.0, 0.0)
    return s


def _triangles(g, n, centre=(0.0, 1.0, -12.0), spread=6.0, size=0.2):
    t = np.zeros(n, TRIANGLE_DTYPE)
    p = g.uniform(-spread, spread, (n, 3)) + np.array(centre)
    t["a"], t["b"], t["c"] = p, p + g.normal(0.0, size, (n, 3)), p + g.normal(0.0, size, (n, 3))
    t["albedo_r"], t["albedo_g"], t["albedo_b"] = g.uniform(0.1, 0.9, (3, n))
    t["roughness"] = g.random(n)
    t["emission"] = np.where(g.random(n) < 0.1, 3.0, 0.0)
    return t


def _right_triangle(leg):
    """Legs of `leg` along x and y at the origin: K = |e1||e2| = leg^2 (the host compares K * 1.0001 with 0.25)."""
    t = np.zeros(1, TRIANGLE_DTYPE)
    t["a"], t["b"], t["c"] = (1.0, 2.0, -12.0), (1.0 + leg, 2.0, -12.0), (1.0, 2.0 + leg, -12.0)
    t["albedo_r"] = t["albedo_g"] = t["albedo_b"] = 0.5
    return t


def _directed():
    """Small scenes at the edges of build_host_scene: (name, spheres, triangles, world_index or None, reorder)."""
    S0, T0 = np.zeros(0, SPHERE_DTYPE), np.zeros(0, TRIANGLE_DTYPE)
    rng = lambda i: np.random.default_rng(7700 + i)                                # noqa: E731
    out = [("empty", S0, T0, None, True), ("one sphere", _spheres(rng(0), 1), T0, None, True),
           ("one triangle", S0, _triangles(rng(1), 1), None, True)]
    for n in (REORDER_MIN_PRIMS - 1, REORDER_MIN_PRIMS):                           # the reorder boundary, spheres and triangles mixed
        g = rng(n)
        sp, tr = _spheres(g, 40), _triangles(g, n - 40)
        wi = g.permutation(n).astype(np.uint32)
        out += [(f"{n} prims", sp, tr, None, True), (f"{n} prims, world_index", sp, tr, wi, True),
                (f"{n} prims, reorder off", sp, tr, None, False), (f"{n} prims, world_index, reorder off", sp, tr, wi, False)]
    g = rng(2)
    sp, tr = _spheres(g, 150), _triangles(g, 50)
    out += [("200 prims, reversed world_index", sp, tr, np.arange(200, dtype=np.uint32)[::-1].copy(), True),
            ("200 prims, random world_index", sp, tr, g.permutation(200).astype(np.uint32), True)]
    sp = _spheres(rng(3), 10)
    sp["radius"][4] = -0.3
    out.append(("negative radius", sp, T0, None, True))
    out.append(("70 identical spheres", np.repeat(_spheres(rng(4), 1), 70), T0, None, True))
    g = rng(5)                                                                     # 20 spheres over 8 x the median, radii with ties
    sp = np.concatenate([_spheres(g, 100, rr=(0.08, 0.12)), _spheres(g, 20, spread=20.0, rr=(1.0, 3.0))])
    sp["radius"][[103, 110, 117]] = 2.5
    sp["radius"][[101, 119]] = 3.5
    out.append(("20 big spheres", sp[g.permutation(120)], T0, None, True))
    g = rng(6)                                                                     # 10 big spheres + 8 big triangles > 16
    sp = np.concatenate([_spheres(g, 30, rr=(0.08, 0.12)), _spheres(g, 10, spread=20.0, rr=(1.0, 3.0))])
    tr = np.concatenate([_triangles(g, 40, size=0.1), _triangles(g, 8, size=2.0)])
    out.append(("big spheres and big triangles over 16", sp, tr, None, True))
    out.append(("10 big spheres, 6 big triangles", sp, tr[:46], None, True))       # ... and exactly 16: still culled
    tr = _triangles(rng(7), 5)
    tr["b"][2, 1] = np.inf
    out.append(("non-finite vertex", S0, tr, None, True))
    small = _triangles(rng(8), 6, size=0.1)
    out.append(("K just below 0.25", S0, np.concatenate([small, _right_triangle(0.49997)]), None, True))
    out.append(("K just above 0.25", S0, np.concatenate([small, _right_triangle(0.49998)]), None, True))
    sp = _spheres(rng(9), 5)
    sp["radius"] = 0.0
    out.append(("zero radii only", sp, T0, None, True))
    for x in (63.0, 65.0):                                                         # median 2^-16 2|c|^2 / r^2 = x^2 / 4096 ... across 0.5
        out.append((f"field at x = {x:g}", _spheres(rng(10), 80, centre=(x, 0.0, 0.0), spread=0.4, rr=(0.5, 0.5)), T0, None, True))
    return out


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        out, seen = [], {}
        for name in ("c1", "c2", "c3", "c4", "c5", "mesh", "c3_ref", "mesh_ref"):      # (c4, c3_ref and mesh_ref share c3's and mesh's worlds)
            key = "mesh" if name.startswith("mesh") else "c3" if name in ("c4", "c3_ref") else name
            if key not in seen:
                seen[key] = scenes.config_world(name)[:2]
            out.append((f"config {name}", *seen[key], None, True))
        out += [(f"rule {name}", sp, tr, None, True) for name, sp, tr in _rule_scenes.cases()]
        _CORPUS = out + _directed()
        assert len({e[0] for e in _CORPUS}) == len(_CORPUS)
    return _CORPUS


def input_hash(entry):
    _, sp, tr, wi, reorder = entry
    h = hashlib.sha256()
    for part in (np.ascontiguousarray(sp, SPHERE_DTYPE).tobytes(), b"|", np.ascontiguousarray(tr, TRIANGLE_DTYPE).tobytes(), b"|",
                 wi.astype("<u4").tobytes() if wi is not None else b"none", b"|1" if reorder else b"|0"):
        h.update(part)
    return h.hexdigest()


ARRAY_DTYPES = dict(geom=np.float32, geom_pk=np.float32, geom_px=np.float32, mat=np.float32, emis=np.float32, tri=np.float32,
                    tri_box=np.float32, geom_r=np.float32, big=np.uint32, world_rank=np.uint32, nodes=np.uint32, leaf_of=np.uint32,
                    trav=np.uint32, travq=np.uint32)


def derive(lib, entry, reorder=None):
    """build_host_scene on one corpus entry: ({scalar: int, or float32 for the floats}, {array: ndarray})."""
    _, sp, tr, wi, ro = entry
    sp, tr = np.ascontiguousarray(sp, SPHERE_DTYPE), np.ascontiguousarray(tr, TRIANGLE_DTYPE)
    wi = np.ascontiguousarray(wi, np.uint32) if wi is not None else None
    h = lib.scene_build(sp.ctypes.data if len(sp) else None, len(sp), tr.ctypes.data if len(tr) else None, len(tr),
                        wi.ctypes.data if wi is not None else None, int(ro if reorder is None else reorder))
    try:
        names = lib.scene_scalar_names().decode().split(",")
        words = np.zeros(len(names), np.uint32)
        lib.scene_scalars(h, words.ctypes.data)
        scal = {n[:-2] if n.endswith(":f") else n: (w.view(np.float32) if n.endswith(":f") else int(w)) for n, w in zip(names, words)}
        arrs = {}
        for n in lib.scene_array_names().decode().rstrip(",").split(","):
            nb = C.c_uint64(0)
            p = lib.scene_array(h, n.encode(), C.byref(nb))
            assert p, n
            arrs[n] = np.frombuffer(C.string_at(p, nb.value), ARRAY_DTYPES[n]).copy()
    finally:
        lib.scene_free(h)
    return scal, arrs


def shape_of(scal):
    return {f: float(scal[f]) for f in LP.SHAPE_FIELDS}


def engines(plan, scal):
    """The engine of the default request (rt_tile_request_defaults: 20 strips, 100 samples, 10 bounces) at each frame size, default
    knobs, grid 0."""
    return {k: LP.engine(plan, shape_of(scal), width=w, height=h, divisions=20, spp=100, max_bounces=10) for k, (w, h) in FRAMES.items()}


def record(lib, plan, entry):
    """What the golden holds of one corpus entry."""
    scal, arrs = derive(lib, entry)
    return {"input": input_hash(entry),
            "scalars": {k: (f"{int(v.view(np.uint32)):08x}" if isinstance(v, np.float32) else v) for k, v in scal.items()},
            "arrays": {k: hashlib.sha256(a.tobytes()).hexdigest() for k, a in arrs.items()},
            "engine": engines(plan, scal)}


@pytest.fixture(scope="module")
def derived(host):
    """Every corpus entry derived once: name -> (entry, scalars, arrays)."""
    return {e[0]: (e, *derive(host, e)) for e in corpus()}


# ------------------------------------------------------------------------------------------------------------ (a), (c): pinned


def test_corpus_is_the_issue_s():
    names = [e[0] for e in corpus()]
    assert sum(n.startswith("config ") for n in names) == 8 and sum(n.startswith("rule ") for n in names) == 26
    assert len(names) == 8 + 26 + len(_directed())
    assert set(json.loads(GOLDEN.read_text())) == set(names)


def test_inputs_are_the_recorded_ones():
    """First: a drift of a scene generator is a generator drift, not a change of the derivation."""
    gold = json.loads(GOLDEN.read_text())
    drift = [e[0] for e in corpus() if input_hash(e) != gold[e[0]]["input"]]
    assert not drift, f"scene generators changed: {drift}"


def test_every_byte_and_every_scalar_is_the_recorded_one(host, derived):
    gold = json.loads(GOLDEN.read_text())
    for name, (entry, scal, arrs) in derived.items():
        g = gold[name]
        assert input_hash(entry) == g["input"], f"{name}: the scene generator changed"
        got = {k: (f"{int(v.view(np.uint32)):08x}" if isinstance(v, np.float32) else v) for k, v in scal.items()}
        assert got == g["scalars"], (name, {k: (got[k], g["scalars"][k]) for k in got if got[k] != g["scalars"][k]})
        bad = [k for k, a in arrs.items() if hashlib.sha256(a.tobytes()).hexdigest() != g["arrays"][k]]
        assert not bad and set(arrs) == set(g["arrays"]), (name, bad)


def test_the_engine_of_each_scene_is_the_recorded_one(plan_lib, derived):  # noqa: F811
    gold = json.loads(GOLDEN.read_text())
    got = {name: engines(plan_lib, scal) for name, (_, scal, _) in derived.items()}
    assert got == {name: gold[name]["engine"] for name in got}
    assert len({e for g in got.values() for e in g.values()}) >= 5          # (the corpus spreads over the engine table)


# ------------------------------------------------------------------------------------------------------------ (b): properties


def _is_perm(a, n):
    return len(a) == n and np.array_equal(np.sort(a), np.arange(n, dtype=np.uint32))


def _boxes(arrs, ns, nt):
    """The primitive boxes, from the stored records: (np, 6)."""
    g = arrs["geom_r"].reshape(-1, 4)[:ns]
    sb = np.concatenate([g[:, :3] - g[:, 3:], g[:, :3] + g[:, 3:]], 1)
    t = arrs["tri"][:nt * 9].reshape(nt, 3, 3)
    with np.errstate(invalid="ignore"):
        tb = np.concatenate([t.min(1), t.max(1)], 1)
    return np.concatenate([sb, tb]).astype(np.float32)


def _leaf_refs(arrs, scal):
    """Every reference of trav, travq and root_ref, in place order: (kind, index, value)."""
    n = scal["n_internal"]
    tv, tq = arrs["trav"].reshape(-1, 16)[:n], arrs["travq"].reshape(-1, 8)[:n]
    return np.concatenate([tv[:, 3], tv[:, 7], tq[:, 6], tq[:, 7], np.array([scal["root_ref"], scal["bvh_root_ref"]], np.uint32)])


def _records(scal, arrs):
    """Per primitive (record, material, emission, world position) as rows of words, sorted: (the spheres', the triangles')."""
    ns, nt = scal["n_sph"], scal["n_tri"]
    wr = arrs["world_rank"] if scal["has_order"] else np.arange(ns + nt, dtype=np.uint32)
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)                                                    # noqa: E731
    common = [u(arrs["mat"]).reshape(-1, 4)[:ns + nt], u(arrs["emis"])[:ns + nt, None], wr[:ns + nt, None]]
    sph = np.concatenate([u(arrs["geom_r"]).reshape(-1, 4)[:ns]] + [c[:ns] for c in common], 1)
    tri = np.concatenate([u(arrs["tri"])[:9 * nt].reshape(nt, 9)] + [c[ns:] for c in common], 1)
    return sph[np.lexsort(sph.T[::-1])], tri[np.lexsort(tri.T[::-1])]


def test_reorder_is_a_renumbering(host, derived):
    """new_of is a permutation that keeps spheres below n_sph; leaf references, leaf ranks and world ranks move with the records; the
    records themselves are the same multiset with the reorder on and off."""
    for name, (entry, scal, arrs) in derived.items():
        ns, nt = scal["n_sph"], scal["n_tri"]
        n = ns + nt
        assert scal["bvh_root_ref"] == scal["root_ref"] and scal["bvh_depth_tree"] == scal["bvh_depth"]
        reordered = entry[4] and n >= REORDER_MIN_PRIMS
        assert scal["has_order"] == int((entry[3] is not None and n > 0) or reordered), name
        if scal["has_order"]:
            assert _is_perm(arrs["world_rank"], n), name
        else:
            assert arrs["world_rank"].tolist() == [0], name
        if not entry[4]:
            continue
        scal0, arrs0 = derive(host, entry, reorder=0)
        assert all(np.array_equal(a, b) for a, b in zip(_records(scal, arrs), _records(scal0, arrs0))), name
        if not reordered:
            assert all(np.array_equal(arrs[k], arrs0[k]) for k in arrs), name
            continue
        # world_rank[i] = world_index[old_of[i]] (the identity when none came): that gives old_of, the inverse of new_of
        old_of = arrs["world_rank"] if entry[3] is None else np.argsort(entry[3]).astype(np.uint32)[arrs["world_rank"]]
        assert _is_perm(old_of, n) and (old_of[:ns] < ns).all() and (old_of[ns:] >= ns).all(), name
        lo = arrs["leaf_of"][:n].astype(np.int64)
        assert (np.diff(lo[:ns]) >= 0).all() and (np.diff(lo[ns:]) >= 0).all(), name
        assert np.array_equal(lo, arrs0["leaf_of"][:n][old_of]), name
        # every leaf reference names the primitive whose box it named before
        r1, r0 = _leaf_refs(arrs, scal), _leaf_refs(arrs0, scal0)
        leaf = (r0 & LEAF_BIT) != 0
        assert np.array_equal(leaf, (r1 & LEAF_BIT) != 0) and np.array_equal(r1[~leaf], r0[~leaf]), name
        p1, p0 = r1[leaf] & ~np.uint32(LEAF_BIT), r0[leaf] & ~np.uint32(LEAF_BIT)
        assert np.array_equal(old_of[p1], p0), name
        b1, b0 = _boxes(arrs, ns, nt), _boxes(arrs0, ns, nt)
        assert np.array_equal(b1[p1], b0[p0], equal_nan=True), name
        assert np.array_equal(arrs["nodes"], arrs0["nodes"]), name             # (the tree itself does not move)


def test_packed_records(derived):
    """Padding spheres, the pair layouts, and the expanded form's w: rounded down from its double value, by less than one ulp."""
    for name, (entry, scal, arrs) in derived.items():
        ns, pad = scal["n_sph"], scal["n_sph_pad"]
        assert pad == (ns + 7) // 8 * 8 and len(arrs["geom"]) == 4 * max(pad, 1), name
        geom, gr = arrs["geom"].reshape(-1, 4), arrs["geom_r"].reshape(-1, 4)
        assert np.array_equal(geom[:ns, :3], gr[:ns, :3]) and np.array_equal(geom[:ns, 3], gr[:ns, 3] * gr[:ns, 3]), name
        assert (geom[ns:pad, 3] == -np.inf).all() and (geom[ns:pad, :3] == 0).all(), name
        assert scal["inverted_boxes"] == int((gr[:ns, 3] < 0).any()), name
        unpair = lambda pk: np.stack([pk[0::2, 0], pk[0::2, 2], pk[1::2, 0], pk[1::2, 2],                   # noqa: E731
                                      pk[0::2, 1], pk[0::2, 3], pk[1::2, 1], pk[1::2, 3]], 1).reshape(-1, 4)
        if pad:
            assert np.array_equal(unpair(arrs["geom_pk"].reshape(-1, 4)), geom), name
            px = unpair(arrs["geom_px"].reshape(-1, 4))
            assert np.array_equal(px[:, :3], geom[:, :3]) and (px[ns:, 3] == np.inf).all(), name
            c, rr = geom[:ns, :3].astype(np.float64), geom[:ns, 3].astype(np.float64)
            cc = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
            w = cc - rr - 2.0 ** -16 * (cc + rr)
            wf = px[:ns, 3]
            assert (wf.astype(np.float64) <= w).all() and (np.nextafter(wf, np.float32(np.inf)).astype(np.float64) > w).all(), name
        nt = scal["n_tri"]
        tb = arrs["tri_box"].reshape(-1, 4)
        assert len(tb) == 2 * nt + 1 and len(arrs["tri"]) == 9 * nt + 1, name
        if nt:
            b = _boxes(arrs, ns, nt)[ns:]
            assert np.array_equal(tb[0:2 * nt:2, :3], b[:, :3], equal_nan=True) and np.array_equal(tb[1:2 * nt:2, :3], b[:, 3:], equal_nan=True), name


def test_big_list_slack_and_triangle_maxima(host, derived):
    for name, (entry, scal, arrs) in derived.items():
        ns, nt, n_big = scal["n_sph"], scal["n_tri"], scal["n_big"]
        big = arrs["big"][:n_big]
        assert n_big <= 16 and len(arrs["big"]) == max(n_big, 1), name
        rad = np.abs(arrs["geom_r"].reshape(-1, 4)[:ns, 3])
        bs = big[big < ns]
        if ns:
            med = np.partition(rad, ns // 2)[ns // 2]
            assert (rad[bs] > np.float32(8.0) * med).all(), name
            over = np.flatnonzero(rad > np.float32(8.0) * med)
            want = sorted(over.tolist(), key=lambda i: (-rad[i], i))[:16]
            assert bs.tolist() == want, name
        rest = np.setdiff1d(np.arange(ns), bs)
        assert scal["r_slack"] == (rad[rest].max() if len(rest) else np.float32(0)), name
        if not nt:
            assert len(bs) == n_big and not scal["tri_ok"] and not scal["xcull_pays"], name
            continue
        assert not scal["cull_pays"], name
        tris = np.zeros(nt, TRIANGLE_DTYPE)
        tris["a"], tris["b"], tris["c"] = (arrs["tri"][:9 * nt].reshape(nt, 3, 3)[:, k] for k in range(3))
        m = np.zeros((nt, 4), np.float32)                                     # kk, dg, es, em
        host.scene_tri_measures(tris.ctypes.data, nt, m.ctypes.data)
        want = np.zeros(4, np.float32)
        if scal["tri_ok"]:
            bt = big[big >= ns] - ns
            assert np.array_equal(big, np.concatenate([bs, bt + ns])) and (np.diff(bt) > 0).all(), name
            med_d = np.partition(m[:, 1], nt // 2)[nt // 2]
            assert bt.tolist() == np.flatnonzero((m[:, 0] > np.float32(0.25)) | (m[:, 1] > np.float32(8.0) * med_d)).tolist(), name
            rest = np.setdiff1d(np.arange(nt), bt)
            if len(rest):
                want = m[rest].max(0)
        else:
            assert len(bs) == n_big, name                                     # (the spheres' list stays as it was)
        assert [scal["tri_k"], scal["tri_diag"], scal["tri_es"], scal["tri_e"]] == want.tolist(), name


def test_directed_scenes_take_the_edges(derived):
    """The directed scenes do what they were built for (so that the pins above pin the edges)."""
    d = {k: v[1] for k, v in derived.items()}
    assert d["empty"]["n_internal"] == 0 and d["one sphere"]["root_ref"] == LEAF_BIT and d["one triangle"]["tri_ok"]
    assert not d["63 prims"]["has_order"] and d["64 prims"]["has_order"] and not d["64 prims, reorder off"]["has_order"]
    assert d["negative radius"]["inverted_boxes"] and not d["64 prims"]["inverted_boxes"]
    assert d["20 big spheres"]["n_big"] == 16
    assert not d["big spheres and big triangles over 16"]["tri_ok"] and d["big spheres and big triangles over 16"]["n_big"] == 10
    assert d["10 big spheres, 6 big triangles"]["tri_ok"] and d["10 big spheres, 6 big triangles"]["n_big"] == 16
    assert not d["non-finite vertex"]["tri_ok"]
    assert d["K just below 0.25"]["tri_ok"] and d["K just below 0.25"]["n_big"] == 0 and d["K just below 0.25"]["tri_k"] <= 0.25
    assert d["K just above 0.25"]["tri_ok"] and d["K just above 0.25"]["n_big"] == 1
    assert not d["zero radii only"]["expanded"]
    assert d["field at x = 63"]["expanded"] and not d["field at x = 65"]["expanded"]


def test_world_permutation_predicate(host):
    ok = lambda a: bool(host.scene_world_is_permutation(np.asarray(a, np.uint32).ctypes.data, len(a)))      # noqa: E731
    assert ok([0]) and ok([2, 0, 1]) and ok(list(range(99, -1, -1)))
    assert not ok([1]) and not ok([0, 0]) and not ok([0, 1, 3]) and not ok([2, 2, 0]) and not ok([0xFFFFFFFF, 0])

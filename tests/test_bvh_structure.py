"""Structure of the two BVH builds — the oracle's (oracle/rt_oracle.cpp bvh_build) and the product's (ray_tracer_s8_amd/csrc/rt_bvh.h,
through tests/host/bvh_host.cpp) — stated as properties of the finished tree, whatever the split heuristic did:
  * every shape index sits in exactly one leaf, and every node but the root is the child of exactly one node;
  * the box a node stores for a child is EXACTLY the f32 min / max join of the boxes of the shapes under that child (so it is the
    join of that child's own two child boxes: consistent, and as tight as a box can be);
  * parent and child indices agree (the product keeps both directions: TravNode references and FlatNode parents), the leaves'
    depth-first order is the order of their node numbers, and the recorded depth is the longest root-to-leaf path.
Inputs: the 21 unit boxes in a row, axis-aligned cubes as 12 triangles each (1 200 and 12 000 triangles), clustered boxes, and sets in
which every box occurs several times."""
import ctypes as C

import numpy as np
import pytest

from test_host_bvh import host, _p  # noqa: F401  (the harness fixture)

LEAF_BIT = 0x80000000
NO_PARENT = 0xFFFFFFFF


def row_of_21():
    return np.array([[x - 0.5, -0.5, -0.5, x + 0.5, 0.5, 0.5] for x in range(-10, 11)], np.float32)


def cube_triangles(n_tri, seed):
    """boxes of the 12 triangles (two per face) of n_tri / 12 axis-aligned cubes at seeded places: face triangles are flat on an axis"""
    g = np.random.default_rng(seed)
    n_cubes = n_tri // 12
    c = g.uniform(-40.0, 40.0, (n_cubes, 1, 3)).astype(np.float32)
    h = g.uniform(0.1, 1.5, (n_cubes, 1, 1)).astype(np.float32)
    corner = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    tris = []
    for axis in range(3):
        for side in (-1, 1):
            q = [k for k in range(8) if corner[k, axis] == side]         # the face's four corners; q[0], q[3] are opposite
            tris += [(q[0], q[1], q[3]), (q[0], q[2], q[3])]
    v = c[:, None] + h[:, None] * corner[np.array(tris)][None]           # (cubes, 12, 3 vertices, 3)
    v = v.reshape(-1, 3, 3).astype(np.float32)
    return np.concatenate([v.min(1), v.max(1)], axis=1)


def clustered(n, seed):
    g = np.random.default_rng(seed)
    centres = g.uniform(-100.0, 100.0, (8, 3))
    c = (centres[g.integers(0, 8, n)] + g.normal(size=(n, 3)) * 0.05).astype(np.float32)
    r = g.uniform(0.001, 0.05, (n, 1)).astype(np.float32)
    return np.concatenate([c - r, c + r], axis=1)


def duplicated(n, copies, seed):
    g = np.random.default_rng(seed)
    c = g.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    r = g.uniform(0.1, 1.0, (n, 1)).astype(np.float32)
    b = np.concatenate([c - r, c + r], axis=1)
    return np.tile(b, (copies, 1))[g.permutation(n * copies)]


SETS = {"row21": row_of_21, "cubes1200": lambda: cube_triangles(1200, 1), "cubes12000": lambda: cube_triangles(12000, 2),
        "clustered": lambda: clustered(3000, 3), "duplicated": lambda: duplicated(250, 8, 4), "identical": lambda: duplicated(1, 33, 5),
        "one": lambda: row_of_21()[:1], "two": lambda: row_of_21()[:2]}


def _join(a, b):
    return np.concatenate([np.fmin(a[:3], b[:3]), np.fmax(a[3:], b[3:])])


def _same_box(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_tree(children, root, shape_box, n):
    """children: ref -> None for a leaf, else (left ref, right ref, stored left box, stored right box); shape_of(ref) for leaves is
    given by `shape_box` (ref -> (shape index, box)).  Walks the tree once, left first; returns (leaf shapes in depth-first order,
    depth).  Asserts single membership, single parenthood and that every stored box is the exact join beneath it."""
    seen_nodes, order = set(), []
    depth = 0
    boxes = {}
    stack = [(root, 0, False)]
    while stack:
        ref, d, done = stack.pop()
        kids = children(ref)
        if kids is None:
            assert ref not in seen_nodes, ("a leaf with two parents", ref)
            seen_nodes.add(ref)
            shape, box = shape_box(ref)
            order.append(shape)
            boxes[ref] = box
            depth = max(depth, d)
            continue
        left, right, lbox, rbox = kids
        if not done:
            assert ref not in seen_nodes, ("a node with two parents", ref)
            seen_nodes.add(ref)
            stack.append((ref, d, True))
            stack.append((right, d + 1, False))
            stack.append((left, d + 1, False))                           # (popped first: left before right)
            continue
        assert _same_box(lbox, boxes[left]), ("left child box is not the join of what lies under it", ref, lbox, boxes[left])
        assert _same_box(rbox, boxes[right]), ("right child box is not the join of what lies under it", ref, rbox, boxes[right])
        boxes[ref] = _join(boxes[left], boxes[right])
    assert sorted(order) == list(range(n)), "not every shape in exactly one leaf"
    assert len(seen_nodes) == 2 * n - 1
    return order, depth


def oracle_tree(oracle, b):
    topo, cb = oracle.bvh_dump(b)
    n = len(b)
    assert len(topo) == 2 * n - 1

    def children(k):
        if topo[k, 0]:
            return None
        left, right = int(topo[k, 2]), int(topo[k, 3])
        assert k < left < right < len(topo), ("children are created after their parent, left subtree first", k, left, right)
        return left, right, cb[k, 0], cb[k, 1]
    order, depth = check_tree(children, 0, lambda k: (int(topo[k, 1]), b[int(topo[k, 1])]), n)
    return order, depth


def product_tree(lib, b):
    n = len(b)
    flat, trav = np.zeros((max(2 * n - 1, 1), 8), np.float32), np.zeros((max(n - 1, 1), 16), np.float32)
    leaf_of, meta = np.zeros(n, np.uint32), np.zeros(4, np.uint32)
    lib.host_bvh_dump(_p(np.ascontiguousarray(b, np.float32)), C.c_uint32(n), _p(flat), _p(trav), _p(leaf_of), _p(meta))
    n_nodes, n_int, root, depth = (int(x) for x in meta)
    assert n_nodes == 2 * n - 1 and n_int == n - 1
    tu = trav.view(np.uint32)

    def children(ref):
        if ref & LEAF_BIT:
            return None
        assert ref < n_int
        t = trav[ref]
        return int(tu[ref, 3]), int(tu[ref, 7]), np.concatenate([t[0:3], t[4:7]]), np.concatenate([t[8:11], t[12:15]])
    order, walked_depth = check_tree(children, root, lambda ref: (ref & ~LEAF_BIT, b[ref & ~LEAF_BIT]), n)
    assert walked_depth == depth, "the recorded depth is not the longest root-to-leaf path"
    # the other direction: FlatNode parents.  A leaf's node holds the shape's own box; leaf nodes are numbered in depth-first order;
    # every node but the root has a parent with a smaller number, every internal node is the parent of exactly two nodes, and its
    # box is the join of theirs; the longest parent chain is the depth.
    parent = flat.view(np.uint32)[:n_nodes, 3]
    box = np.concatenate([flat[:n_nodes, 0:3], flat[:n_nodes, 4:7]], axis=1)
    assert len(set(leaf_of.tolist())) == n and (np.diff(leaf_of[order]) > 0).all()
    assert parent[0] == NO_PARENT and (parent[1:] < np.arange(1, n_nodes)).all()
    is_leaf = np.zeros(n_nodes, bool)
    is_leaf[leaf_of] = True
    # the root is no one's child, so no box is stored for it: its FlatNode holds the empty box (+inf, -inf) the builder starts
    # from, whether it is an internal node or (n == 1) the only leaf; every other leaf holds its shape's own box
    inf = np.float32(np.inf)
    assert _same_box(box[0], [inf, inf, inf, -inf, -inf, -inf])
    for p_ in range(n):
        assert _same_box(box[leaf_of[p_]], b[p_]) if n > 1 else leaf_of[p_] == 0
    kids = {}
    for k in range(1, n_nodes):
        kids.setdefault(int(parent[k]), []).append(k)
    assert all(len(v) == 2 for v in kids.values()) and set(kids) == set(np.nonzero(~is_leaf)[0].tolist())
    for k, (l, r) in kids.items():
        if k:                                                             # (the root's own box is the empty box, asserted above)
            assert _same_box(box[k], _join(box[l], box[r])), ("FlatNode box is not the join of its children's", k)
    chain = np.zeros(n_nodes, np.int64)
    for k in range(1, n_nodes):
        chain[k] = chain[parent[k]] + 1
    assert int(chain.max()) == depth
    return order, depth


@pytest.mark.parametrize("name", list(SETS))
def test_both_trees_are_consistent_tight_and_complete(host, oracle, name):  # noqa: F811
    b = np.ascontiguousarray(SETS[name](), np.float32)
    assert (b[:, :3] <= b[:, 3:]).all()
    o_order, o_depth = oracle_tree(oracle, b)
    p_order, p_depth = product_tree(host, b)
    assert o_order == p_order and o_depth == p_depth, "the two builds disagree on the leaves' order or the depth"
    if name == "row21":
        assert len(o_order) == 21
    if name.startswith("cubes"):
        assert len(b) in (1200, 12000) and (b[:, :3] == b[:, 3:]).any(axis=1).all()       # every face triangle is flat on an axis

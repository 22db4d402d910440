"""The directed operand corpus of tests/_operand_cases.py, without a GPU:
(a) every class the module lists holds at least FLOOR directed records, counted by the classifier alone — so the GPU tests of
    tests/test_gpu_operands.py cannot pass without having taken each decision of the reference both ways and at equality;
(b) the oracle's C++ batch (rt_oracle_operands_batch) equals the numpy restatement (oracle/restate_ops_np.py) bit for bit on the
    whole directed corpus — two independent statements of the nested form;
(c) a numpy twin of the device's straight-line select form of exact_sphere (rt_kernel.hip.h) equals the nested form on the corpus,
    and the mutations a later change could make by accident are told apart by the directed records of the class that names them."""
import numpy as np
import pytest

import _operand_cases as OC
from oracle import restate_ops_np as RS

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _floor(classes, names, what):
    short = {k: int(classes[k].sum()) for k in names if int(classes[k].sum()) < OC.FLOOR}
    assert not short, (what, "classes below the floor of", OC.FLOOR, short)


def test_every_sphere_class_and_pair_holds_the_floor():
    c = OC.classify_sphere(OC.sphere_directed())
    _floor(c, OC.SPHERE_CLASSES, "sphere")
    short = {p: int((c[p[0]] & c[p[1]]).sum()) for p in OC.SPHERE_PAIRS if int((c[p[0]] & c[p[1]]).sum()) < OC.FLOOR}
    assert not short, ("sphere (disc, window) pairs below the floor", short)
    # the pairs NOT listed do not occur at all: the list is the reachable set
    disc, win = OC.SPHERE_CLASSES[0:4], OC.SPHERE_CLASSES[14:18]
    for a in disc:
        for b in win:
            if (a, b) not in OC.SPHERE_PAIRS:
                assert not (c[a] & c[b]).any(), (a, b)


def test_every_triangle_class_holds_the_floor():
    _floor(OC.classify_triangle(OC.triangle_directed()), OC.TRIANGLE_CLASSES, "triangle")


def test_every_box_class_holds_the_floor_with_and_without_a_finite_inverse():
    c = OC.classify_aabb(OC.aabb_directed())
    _floor(c, OC.AABB_CLASSES, "aabb")
    assert int((~c["finite"]).sum()) >= OC.FLOOR
    for k in OC.AABB_CLASSES:
        if k in OC.AABB_ZERO_DIR:
            assert not (c[k] & c["finite"]).any(), k                      # a zero component: 1 / d is infinite
        else:
            assert int((c[k] & c["finite"]).sum()) >= OC.FLOOR, (k, "with a finite inverse direction")
    ch = OC.chain_records(OC.aabb_directed())
    lo, hi, olo, ohi = ch[:, 6:9], ch[:, 9:12], ch[:, 12:15], ch[:, 15:18]
    assert (olo <= lo).all() and (ohi >= hi).all() and len(ch) >= 4096     # the outer box contains the leaf box


def test_every_as_u8_class_holds_the_floor():
    _floor(OC.classify_as_u8(OC.as_u8_directed()), OC.AS_U8_CLASSES, "as_u8")


# ---------------------------------------------------------------- (b) C++ batch against numpy
@pytest.mark.parametrize("ray_new", [False, True])
def test_cpp_sphere_batch_equals_the_numpy_form(oracle, ray_new):
    rec = OC.sphere_directed()
    got = oracle.operands_batch(oracle.SPHERE_NORM if ray_new else oracle.SPHERE, rec)
    want = RS.sphere(rec, ray_new)
    assert np.array_equal(got[:, 0] != 0, want["hit"]), np.nonzero((got[:, 0] != 0) != want["hit"])[0][:5]
    ok = _same(got[:, 1].view(np.float32), want["t"])
    assert ok.all(), (np.nonzero(~ok)[0][:5], rec[~ok][:2])
    if ray_new:
        for k in range(3):
            assert _same(got[:, 2 + k].view(np.float32), want["d"][k]).all(), k


def test_cpp_triangle_batch_equals_the_numpy_form(oracle):
    rec = OC.triangle_directed()
    got = oracle.operands_batch(oracle.TRIANGLE, rec)
    want = RS.triangle(rec)
    assert np.array_equal(got[:, 0] != 0, want["hit"]), np.nonzero((got[:, 0] != 0) != want["hit"])[0][:5]
    assert _same(got[:, 1].view(np.float32), want["t"]).all()


def test_cpp_box_batches_equal_the_numpy_form(oracle):
    rec = OC.aabb_directed()
    col = lambda r, i: [r[:, 3 * i + k] for k in range(3)]      # noqa: E731
    got = oracle.operands_batch(oracle.AABB, rec)
    passes, _, _, finite = RS.aabb(col(rec, 0), col(rec, 1), col(rec, 2), col(rec, 3))
    assert np.array_equal(got[:, 0] != 0, passes) and np.array_equal(got[:, 1], got[:, 0]) and np.array_equal(got[:, 2] != 0, finite)
    ch = OC.chain_records(rec)
    got = oracle.operands_batch(oracle.CHAIN, ch)
    leaf = RS.aabb(col(ch, 0), col(ch, 1), col(ch, 2), col(ch, 3))
    outer = RS.aabb(col(ch, 0), col(ch, 1), col(ch, 4), col(ch, 5))
    assert np.array_equal(got[:, 0] != 0, leaf[0]) and np.array_equal(got[:, 1] != 0, outer[0])
    fin = got[:, 2] != 0
    assert not (fin & leaf[0] & ~outer[0]).any(), "a finite ray passes a leaf box and not a box that contains it"
    assert int((fin & leaf[0]).sum()) >= 1024


def test_cpp_as_u8_and_normalize_batches_equal_the_numpy_form(oracle):
    v = OC.as_u8_directed()
    assert np.array_equal(oracle.operands_batch(oracle.AS_U8, v)[:, 0], RS.as_u8(v)[:, 0].astype(np.uint32))
    rec = OC.normalize_directed()
    got = oracle.operands_batch(oracle.NORMALIZE, rec)
    with np.errstate(all="ignore"):
        cols = [rec[:, k] for k in range(3)]
        nrm = RS.normalize(cols)
        ok, tn = RS.try_normalize(cols)
    assert int(ok.sum()) >= OC.FLOOR and int((~ok).sum()) >= OC.FLOOR
    assert np.array_equal(got[:, 3] != 0, ok)
    for k in range(3):
        assert _same(got[:, k].view(np.float32), nrm[k]).all(), k
        assert _same(got[:, 4 + k].view(np.float32), np.where(ok, tn[k], F(0.0))).all(), k


def test_cpp_rng_batch_equals_the_single_call_probes(oracle):
    seeds = OC.rng_seeds()[:600]
    got = oracle.operands_batch(oracle.RNG, seeds)
    for i in (0, 1, 2, 3, 7, 8, 9, 100, 599):
        s64 = int(seeds[i, 0]) | (int(seeds[i, 1]) << 32)
        st = oracle.seed_from_u64(s64)
        assert np.array_equal(got[i, 0:8].view(np.uint64), st)
        nxt = oracle.xoshiro_from_state(st, 12)
        assert np.array_equal(got[i, 8:12], (nxt[:4] >> np.uint64(32)).astype(np.uint32))
        st2 = st.copy()
        for _ in range(4):
            oracle.draw(st2, 0)                                            # (advance past the four next_u32 words)
        u = [oracle.draw(st2, 0)[0] for _ in range(4)]
        m = [oracle.draw(st2, 1)[0] for _ in range(4)]
        assert np.array_equal(got[i, 12:16], _bits(u)) and np.array_equal(got[i, 16:20], _bits(m))
        assert np.array_equal(got[i, 20:28].view(np.uint64), st2)


# ---------------------------------------------------------------- (c) the select form and its mutations
def select_form_sphere(rec, mutation=None):
    """exact_sphere of rt_kernel.hip.h, operation for operation, on arrays: every record computes both quotient roots and selects.
    mutation "ge2": `> 2.0f` written as `>= 2.0f`."""
    r = np.ascontiguousarray(rec).view(np.float32)
    with np.errstate(all="ignore"):
        o, d, cen = [r[:, k] for k in range(3)], [r[:, 3 + k] for k in range(3)], [r[:, 6 + k] for k in range(3)]
        rr, t_min, t_max = r[:, 9] * r[:, 9], r[:, 10], r[:, 11]
        oc = RS.sub(o, cen)
        b = RS.dot([F(2.0) * x for x in d], oc)
        ln = np.sqrt(RS.dot(oc, oc))
        c = ln * ln - rr
        disc = b * b - F(4.0) * c
        sq = np.sqrt(disc)
        bneg = b < F(0.0)
        same, diff = np.where(bneg, -b + sq, -b - sq), np.where(bneg, -b - sq, -b + sq)
        a0x2 = F(2.0) * c
        big = (lambda x: np.abs(x) >= F(2.0)) if mutation == "ge2" else (lambda x: np.abs(x) > F(2.0))
        big_s, big_d = big(same), big(diff)
        q1, q2, hs, hd = a0x2 / same, a0x2 / diff, same / F(2.0), diff / F(2.0)
        x1 = np.where(big_s, q1, hd)
        x2 = np.where(big_s, np.where(big_d, q2, hs), hs)
        one = disc == F(0.0)
        r1 = -b / F(2.0)
        x = np.where(one, r1, np.where(x1 < x2, x1, x2))
        y = np.where(one, r1, np.where(x1 < x2, x2, x1))
        xin, yin = (x >= t_min) & (x < t_max), (y >= t_min) & (y < t_max)
        t = np.where(xin & yin, np.where(x < y, x, y), np.where(xin, x, y))
        return ~(disc < F(0.0)) & (xin | yin), t.astype(np.float32)


def test_select_form_equals_the_nested_form_on_the_corpus():
    rec = OC.sphere_directed()
    want = RS.sphere(rec, False)
    hit, t = select_form_sphere(rec)
    assert np.array_equal(hit, want["hit"]), np.nonzero(hit != want["hit"])[0][:5]
    assert _same(t[hit], want["t"][hit]).all()


def device_form_triangle(rec, mutation=None):
    """exact_triangle of rt_kernel.hip.h, line for line on arrays (its early returns as masks); mutation "lt1": `u <= 1.0f` written
    as `u < 1.0f`.  Returns (hit, t as the device leaves it: dist where the root tests pass, else the 0 it was given)."""
    r = np.ascontiguousarray(rec).view(np.float32)
    with np.errstate(all="ignore"):
        o, d = [r[:, k] for k in range(3)], [r[:, 3 + k] for k in range(3)]
        A, B, C = ([r[:, 6 + 3 * i + k] for k in range(3)] for i in range(3))
        t_min, t_max = r[:, 15], r[:, 16]
        a_to_b, a_to_c = RS.sub(B, A), RS.sub(C, A)
        u_vec = RS.cross(d, a_to_c)
        det = RS.dot(a_to_b, u_vec)
        live = ~((det < RS.EPSILON) & (det > -RS.EPSILON))
        inv_det = F(1.0) / det
        a_to_origin = RS.sub(o, A)
        u = RS.dot(a_to_origin, u_vec) * inv_det
        live &= (u >= F(0.0)) & ((u < F(1.0)) if mutation == "lt1" else (u <= F(1.0)))
        v_vec = RS.cross(a_to_origin, a_to_b)
        v = RS.dot(d, v_vec) * inv_det
        live &= ~((v < F(0.0)) | (u + v > F(1.0)))
        dist = RS.dot(a_to_c, v_vec) * inv_det
        live &= dist > RS.EPSILON
        return live & (dist >= t_min) & (dist < t_max), np.where(live, dist, F(0.0)).astype(np.float32)


def test_sphere_corpus_meets_the_equalities_through_ray_new_too():
    """SPHERE_NORM renormalises the scaled directions: the exact-equality classes are counted again under Ray::new"""
    c = OC.classify_sphere(OC.sphere_directed(), True)
    _floor(c, OC.SPHERE_EXACT + ("disc<0", "disc>0", "b<0", "b>=0", "x1<x2", "!(x1<x2)", "window both", "window first only",
                                 "window second only", "window none"), "sphere through Ray::new")


def test_directed_records_tell_the_mutations_apart():
    """Twins of the DEVICE code with one token changed, on the directed corpus alone.
    `u <= 1.0f` as `u < 1.0f` (exact_triangle): every hit of class "u==1" becomes a miss, at least FLOOR of them, nothing else moves.
    `> 2.0f` as `>= 2.0f` (exact_sphere): at least FLOOR records change a bit of t, all of the classes "|same|==2" / "|diff|==2"."""
    rec = OC.triangle_directed()
    c = OC.classify_triangle(rec)
    want = RS.triangle(rec)
    hit, t = device_form_triangle(rec)
    assert np.array_equal(hit, want["hit"]) and _same(t[hit], want["t"][hit]).all()
    mh, _ = device_form_triangle(rec, "lt1")
    changed = mh != hit
    assert int(changed.sum()) >= OC.FLOOR and (changed <= c["u==1"]).all()
    assert np.array_equal(changed, hit & c["u==1"]) and not mh[changed].any()
    rec = OC.sphere_directed()
    c = OC.classify_sphere(rec)
    hit, t = select_form_sphere(rec)
    mh, mt = select_form_sphere(rec, "ge2")
    changed = (hit != mh) | (hit & ~_same(t, mt))
    assert (changed <= (c["|same|==2"] | c["|diff|==2"])).all()
    assert int(changed.sum()) >= OC.FLOOR, int(changed.sum())

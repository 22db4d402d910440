"""The arithmetic of the next-event-estimation integrator (rt_scene_trace_nee, rt_tile.h "next-event estimation") in float32 numpy, one
IEEE operation per numpy operation in the order the header writes them: the two MIS weights, the area view of an emitter the bounce
reached with its samplable test, and the seeded states.  tests/test_nee_host.py pins the weights and the samplable test against
csrc/rt_nee_math.h under g++.  The integrator itself — the forward fold and the sampled rule — is tests/_lights_np.py's `nee`."""
import numpy as np

from ray_tracer_s8_amd import _abi

import _bounce_np as B
import _direct_np as D

F32 = np.float32
ONE = F32(1)
LIGHT_ONLY, MIS = _abi.RT_NEE_LIGHT_ONLY, _abi.RT_NEE_MIS
MODES = (LIGHT_ONLY, MIS)


# ---------------------------------------------------------------- the arithmetic of csrc/rt_nee_math.h
def light_weight(W):
    """wl = 1 / (1 + W)"""
    with np.errstate(all="ignore"):
        return ONE / (ONE + F32(W))


def bounce_weight(W):
    """wb = 1 - 1 / (1 + W')"""
    with np.errstate(all="ignore"):
        return ONE - ONE / (ONE + F32(W))


def emitter_view(n, d, nh, distance, sphere):
    """(cs', cl', d2', samplable) of an emitter the bounce reached: n the previous hit's normal, d the segment's unit direction, nh and
    distance this hit's rt_hit normal and distance."""
    with np.errstate(all="ignore"):
        cs = D.dot(n, d)
        c = D.dot(nh, d)
        cl = -c if sphere else np.abs(c)
        d2 = F32(distance) * F32(distance)
        samplable = bool(cs > 0 and cl > 0 and d2 > 0 and np.isfinite(d2))
    return cs, cl, d2, samplable


def view_weight(cs, cl, d2, sphere, size, M):
    """W' of that view: the weight of a light sample with this geometry (size: the radius, or the triangle's area)."""
    return D.sphere_weight(cs, cl, size, M, d2) if sphere else D.triangle_weight(cs, cl, size, M, d2)


def sample_states(seed, n, spp, s):
    """The seeded state of sample s of every ray: seed_from_u64(seed + 4 PHI (i spp + s))."""
    from oracle import oracle as orc
    return np.array([orc.seed_from_u64((seed + B.PHI4 * (i * spp + s)) & B.M64) for i in range(n)], np.uint64).reshape(n, 4)

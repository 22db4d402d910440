"""The launch-path knob matrix: the requests and the knob settings that tests/test_gpu_knobs.py renders on the GPU and whose plans
tests/test_launch_plan.py checks on the CPU.  One list for both, so that they cannot drift apart.  Plain data: no GPU, no library.

The knobs are the process-level ones of csrc/rt_api.hip (DebugKnob) that reach the sample-unit scheduler of csrc/rt_kernel.hip.h
through rtplan::Knobs: slots, commit threshold, the split of the queue into whole tiles and parts, the refill threshold of the walks,
output staging, compacted root tests, and the counting of per-strip costs."""

# ---- requests: name -> (width, height, spp, grp, U).  Every frame is cut into 2 strips; both are rendered in ONE batched launch
# (waves cross the strip boundary) and strip 1 once more alone.  grp: pixels per slot, U = grp * spp: units per slot, as plan_launch
# derives them (checked in tests/test_launch_plan.py).
#   150x6x1    grp 8, U 8: one acquisition step opens up to 8 slots.  Tiles of 64, 64 and 22 pixels: the last one is one full
#              16-pixel part and a 6-pixel one, its other two parts lie beyond the right edge.  A row is 450 bytes: whole tiles of
#              rows 0 and 2 of a strip start dword-aligned and are staged, those of row 1 are not.
#   70x6x3     grp 3, U 9: a 16-pixel part (48 units) is five slots and a short sixth.  The 6-pixel tile has one part inside the frame.
#   70x6x7     grp 2, U 14.
#   150x6x8    grp 1: a pixel's sum is one commit batch of 8.
#   70x6x17    more than 16 samples: every tile in parts whatever the grid; the sum is 2 x 8 + 1.
#   70x6x33    parts of 4 pixels (sub_shift 4): the 6-pixel tile is 4 + 2 pixels and fourteen parts beyond the edge.
#   70x4x100   the reference's sample count: the sum is 12 x 8 + 4.
REQUESTS = {
    "150x6x1": (150, 6, 1, 8, 8),
    "70x6x3": (70, 6, 3, 3, 9),
    "70x6x7": (70, 6, 7, 2, 14),
    "150x6x8": (150, 6, 8, 1, 8),
    "70x6x17": (70, 6, 17, 1, 17),
    "70x6x33": (70, 6, 33, 1, 33),
    "70x4x100": (70, 4, 100, 1, 100),
}
DIVISIONS = 2
MAX_BOUNCES = 4
SEED = 0x6B6E6F62

# the progressive job: 11 samples of strip 1 of 70 x 6 in three passes (s_begin > 0, gap > 0, the running sum read and written)
PASS_JOB = (70, 6, 11, [(0, 3), (3, 4), (4, 11)])

SLOTS_MIN = 1          # the smallest number of slots at which a wave always progresses (the argument: tests/test_gpu_knobs.py)
ALL_PARTS = 10 ** 6    # RT_TAIL_TILES: more tiles than any launch here has

# engines (rt_tile_stats.engine); "3c" / "5c": engines 3 and 5 through the capped-stack kernels (RT_FORCE_CAPPED=1, RT_STACK_LDS=3)
ENGINE_KEYS = [0, 1, 2, 3, 4, 5, 6, 7, "3c", "5c"]
CAPPED = {"RT_FORCE_CAPPED": 1, "RT_STACK_LDS": 3}
FAMILY = {0: "resident scan", 1: "streamed scan", 2: "L2 exact", 6: "L2 exact", 3: "L2 quantised", 5: "L2 quantised",
          "3c": "capped", "5c": "capped", 4: "LDS tree", 7: "LDS tree culled"}
_ALL = tuple(ENGINE_KEYS)
_WALKS = (2, 3, 4, 5, 6, 7, "3c", "5c")          # the refill threshold is read by the traversal kernels only
_STAGING = (1, 2, 3, 5, 6, "3c", "5c")           # the kernels output staging is compiled into
_EXACT_L2 = (2, 6)                               # the kernels with compacted root tests

# ---- settings: name -> (knobs, engines it runs on, tiles_big the plan must show: "none", "all", "all_but_one")
SETTINGS = {
    "default": ({}, _ALL, "none"),
    "slots_min": ({"RT_SLOTS": SLOTS_MIN}, _ALL, "none"),
    "slots_5": ({"RT_SLOTS": 5}, _ALL, "none"),
    "slots_32": ({"RT_SLOTS": 32}, _ALL, "none"),
    "commit_1": ({"RT_COMMIT_SLOTS": 1}, _ALL, "none"),
    "slots_5_commit_5": ({"RT_SLOTS": 5, "RT_COMMIT_SLOTS": 5}, _ALL, "none"),
    "slots_32_commit_32": ({"RT_SLOTS": 32, "RT_COMMIT_SLOTS": 32}, _ALL, "none"),
    "tail_0": ({"RT_TAIL_TILES": 0}, _ALL, "all"),                    # every queue entry a whole tile
    "tail_1": ({"RT_TAIL_TILES": 1}, _ALL, "all_but_one"),            # whole tiles and the parts of one: the tiles_big boundary
    "tail_all": ({"RT_TAIL_TILES": ALL_PARTS}, _ALL, "none"),
    "refill_1": ({"RT_REFILL_EIGHTHS": 1}, _WALKS, "none"),
    "refill_8": ({"RT_REFILL_EIGHTHS": 8}, _WALKS, "none"),
    "no_stage": ({"RT_NO_STAGE": 1}, _STAGING, "none"),
    # (only whole tiles are staged, and these small launches have none by default: with tail_0 above, staging on and off on whole tiles)
    "no_stage_whole_tiles": ({"RT_TAIL_TILES": 0, "RT_NO_STAGE": 1}, _STAGING, "all"),
    "compact_0": ({"RT_COMPACT": 0}, _EXACT_L2, "none"),
    "strip_cost_0": ({"RT_STRIP_COST": 0}, _ALL, "none"),
    "starved": ({"RT_SLOTS": SLOTS_MIN, "RT_COMMIT_SLOTS": 1, "RT_TAIL_TILES": 0, "RT_REFILL_EIGHTHS": 8, "RT_NO_STAGE": 1}, _ALL, "all"),
    "wide": ({"RT_SLOTS": 32, "RT_COMMIT_SLOTS": 32, "RT_TAIL_TILES": ALL_PARTS, "RT_REFILL_EIGHTHS": 1}, _ALL, "none"),
}

# DebugKnob name -> rtplan::Knobs field (tests/host/plan_host.cpp); RT_STRIP_COST is not a plan knob
PLAN_KNOB = {"RT_SLOTS": "slots", "RT_COMMIT_SLOTS": "commit_slots", "RT_TAIL_TILES": "tail_tiles", "RT_REFILL_EIGHTHS": "refill_eighths",
             "RT_NO_STAGE": "no_stage", "RT_COMPACT": "compact", "RT_FORCE_CAPPED": "force_capped", "RT_STACK_LDS": "stack_lds",
             "RT_LDS_TREE": "lds_tree", "RT_CULL_WALK": "cull_walk"}


def settings_for(engine_key):
    """The settings that run on an engine, "default" first."""
    return [name for name, (_, engines, _) in SETTINGS.items() if engine_key in engines]


def plan_knobs(setting):
    """The setting as keyword arguments of test_launch_plan.plan."""
    return {PLAN_KNOB[k]: v for k, v in SETTINGS[setting][0].items() if k in PLAN_KNOB}


def tuples():
    """Every (request, strips in the launch, setting) the GPU matrix launches: the batched frame and strip 1 alone."""
    return [(rq, n, s) for rq in REQUESTS for n in (DIVISIONS, 1) for s in SETTINGS]

// rt_consts.h — the sizes the kernels are compiled with and the host plans their launches by (rt_kernel.hip.h, rt_plan.h).
// Plain C++: also built by g++ in the CPU harness tests/host/plan_host.cpp.  The RT_* macros are experiment overrides (-D).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__ inline
#else
#define RT_HOST_DEVICE inline
#endif

#ifndef RT_MAXC
#define RT_MAXC 16
#endif
#ifndef RT_MAXL
#define RT_MAXL 8
#endif
#ifndef RT_MINL                 // the host may shrink the leaf lists down to this many slots to fit one more workgroup per CU
#define RT_MINL 4
#endif
#ifndef RT_MAXL_LTREE
#define RT_MAXL_LTREE 12
#endif

namespace rtk {

constexpr int BLOCK = 256;       // 4 waves
constexpr int LTREE_BLOCK = 1024;   // LDS-resident tree kernels: one workgroup of 16 waves per CU
constexpr int UNROLL = 8;        // broad-phase unroll; chunk sizes are padded to this
constexpr int MAXC = RT_MAXC;    // candidate list slots per lane (per chunk)
constexpr int CHUNK = 2048;      // max spheres per LDS chunk (32 KiB): list entries carry an 8-bit group index
constexpr int MAX_BATCH = 64;    // strips per launch
constexpr int TRAV_STACK = 64;   // traversal stack entries per lane (host falls back to the linear scan beyond)
constexpr int MAXL = RT_MAXL;    // leaf-candidate slots per lane in traversal mode (flushed when full)
constexpr int MINL = RT_MINL;
constexpr int MAXL_EXACT = 7;     // exact-node kernel: fixed (see the kernel)
constexpr int LNODE_DW = 19;      // LDS-tree kernel: dwords per staged node (see the staging code); odd, so that the
                                  // nodes start on all 32 banks
// bias of the LDS-tree kernel's node references: reference 0x8000 = the dword behind node DONE (see the staging code)
RT_HOST_DEVICE uint32_t lt_r0(uint32_t n_internal) { return 0x8000u - (n_internal + 1u) * (uint32_t)LNODE_DW; }
constexpr int MAXL_LTREE = RT_MAXL_LTREE;     // LDS-tree kernel (16-bit entries): a block of RT_STEPS_PER_CHECK_LTREE appends always fits;
constexpr int MAXL_LTREE_MAX = 16;            // the host gives a tree that leaves room up to this many slots (KParams::maxl; c3 14: +0.5 %)
constexpr uint32_t LEAF_BIT = 0x80000000u;
// Output staging (north_star: "coalesced HBM stores of the tile"): a wave collects the RGB8 bytes of up to STAGE_SLOTS of
// its 64x1 tiles in LDS and writes a finished tile as 48 whole dwords = three whole 64-byte lines.  Byte stores of
// single pixels reached HBM as partial lines: 1.3x (c3) to 13x (c5) write amplification (profiles/r01_*, r02_*).
constexpr uint32_t STAGE_TILE_BYTES = 192;
constexpr uint32_t STAGE_TILES = 3;               // output staging: tiles a wave may have open
constexpr uint32_t SLOTS_MAX = 32;                // sample units: pixel slots per wave (rt_kernel.hip.h "Sample units")
constexpr uint32_t COST_COPIES = 16;              // partial sums of the per-strip cost (KParams::strip_cost)

}  // namespace rtk

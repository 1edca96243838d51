// rsort_device.hpp -- device helpers shared by the kernel translation units (rsort_kernels.hip,
// rsort_segmented.hip, rsort_topk.hip): lane and wave primitives, the lane-ordered and ballot rankings with their rank
// check, and the wave / workgroup scans. Device code only; every function is inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsort_internal.hpp"

namespace rsort {

// ------------------------------------------------------------------------------ helpers
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// Lane count of a wave-uniform mask as an opaque 32-bit scalar. `__popcll(m) < c` is folded into a
// 64-bit unsigned compare of the i64 popcount, which the SALU cannot do (no s_cmp_lt_u64): it went
// to the VALU (v_cmp_lt_u64 on SGPR operands) on every key of the rank loops. s_bcnt1 into a 32-bit
// SGPR keeps the test on the SALU (s_cmp + s_cbranch_scc). s_bcnt1 also writes SCC: declared, or the
// compiler may place it between another compare and the branch on that compare (it did, round 6: a
// tile's rank-check test `tno & 7` branched on this count instead).
__device__ __forceinline__ uint32_t wave_count(uint64_t m) {
    uint32_t c;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(c) : "s"(m) : "scc");
    return c;
}

// Lane-ordered returning LDS add of 1 to cnt[d] for every lane of a wave (the kRankAtomic
// premise: same-address lanes are served in lane order, so lane l gets old + #lower lanes with
// digit d). Same-address lanes serialise in the LDS (about 2 cycles each: 127 cycles when all 64
// lanes share a counter, dev/lds_rate_lab.hip) and clustered input -- runs of equal keys, as
// every pass after the first sees for duplicate-heavy data -- does exactly that. So when the
// digit held by the first active lane is common (>= 16 lanes: a run crossing the slot's start,
// or a slot inside one run), it is added once, by that lane, for all its lanes, whose ranks come
// from mbcnt; a run that starts inside the slot is served lane by lane (once per run). Uniform
// data pays one compare, a popcount and a scalar branch. Exact under any exec mask.
__device__ __forceinline__ uint32_t rank_add(uint32_t *cnt, uint32_t d) {
    const uint32_t da = __builtin_amdgcn_readfirstlane(d);
    const uint64_t ma = __ballot(d == da);
    if (wave_count(ma) < 16) return atomicAdd(&cnt[d], 1u);
    const uint32_t la = (uint32_t)__builtin_ctzll(ma);
    uint32_t o = 0;
    if (d != da) o = atomicAdd(&cnt[d], 1u);
    if (lane_id() == la) o = atomicAdd(&cnt[da], (uint32_t)__popcll(ma));
    const uint32_t base = __builtin_amdgcn_readlane(o, la);
    return d == da ? base + (uint32_t)__popcll(ma & lanes_below()) : o;
}

// Non-returning form for histograms (same aggregation; exact under any exec mask).
__device__ __forceinline__ void count_add(uint32_t *cnt, uint32_t d, uint32_t inc = 1u) {
    const uint32_t da = __builtin_amdgcn_readfirstlane(d);
    const uint64_t ma = __ballot(d == da);
    if (wave_count(ma) < 16) {
        atomicAdd(&cnt[d], inc);
        return;
    }
    if (d != da) atomicAdd(&cnt[d], inc);
    if (lane_id() == (uint32_t)__builtin_ctzll(ma)) atomicAdd(&cnt[da], inc * (uint32_t)__popcll(ma));
}

// One returning add for all lanes of a wave: the lanes whose digit is c (mask m) are served by the
// first of them, adding their count, and get base + their rank among m (mbcnt); every other lane
// adds 1 (lane-ordered). One ds_add_rtn instruction.
__device__ __forceinline__ uint32_t agg_add(uint32_t *cnt, uint32_t d, uint32_t c, uint64_t m) {
    const uint32_t la = (uint32_t)__builtin_ctzll(m);
    const bool mine = d == c;
    uint32_t o = 0;
    if (!mine || lane_id() == la) o = atomicAdd(&cnt[d], mine ? (uint32_t)__popcll(m) : 1u);
    const uint32_t base = __builtin_amdgcn_readlane(o, la);
    return mine ? base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) : o;
}

// rank_add for clustered input (the clustered-pass kernels, rs_scatter_lines<..., CL = 1>): when the
// first lane's digit is not common, the wave's last aggregated digit (`hot`, wave-uniform) is the
// second candidate -- a run of a hot key covers many consecutive slots, but where it holds ~2/3 of
// a slot's lanes the first lane holds another key a third of the time, and then ~40 lanes would
// serialise on one counter (dev/lines_exp.hip, Zipf pass 1: 2.35 -> 2.16 ms; it costs ~12 % on
// unclustered input, so only the clustered kernels use it).
__device__ __forceinline__ uint32_t rank_add_hot(uint32_t *cnt, uint32_t d, uint32_t &hot) {
    const uint32_t da = __builtin_amdgcn_readfirstlane(d);
    const uint64_t ma = __ballot(d == da);
    if (wave_count(ma) >= 16) {
        hot = da;
        return agg_add(cnt, d, da, ma);
    }
    const uint64_t mh = __ballot(d == hot);
    if (wave_count(mh) >= 8) return agg_add(cnt, d, hot, mh);
    return atomicAdd(&cnt[d], 1u);
}

// rank_add_hot in two halves, so a tile's KPT slots issue their returning adds back to back and
// wait for the LDS once: hot_issue picks the slot's aggregated digit c (~0u: none) and its lanes m
// exactly as rank_add_hot and issues the slot's one add; hot_rank, after every slot is issued, turns
// the returns into ranks (the aggregated lanes read their leader's return).
template <bool HOT>
__device__ __forceinline__ uint32_t hot_issue(uint32_t *cnt, uint32_t d, uint32_t &hot, uint32_t &c, uint64_t &m) {
    const uint32_t da = __builtin_amdgcn_readfirstlane(d);
    const uint64_t ma = __ballot(d == da);
    if (wave_count(ma) >= 16) {
        hot = da;
        c = da;
        m = ma;
    } else if (!HOT) {
        c = 0xFFFFFFFFu;
        m = 0ull;
    } else {
        const uint64_t mh = __ballot(d == hot);
        const bool agg = wave_count(mh) >= 8;
        c = agg ? hot : 0xFFFFFFFFu;
        m = agg ? mh : 0ull;
    }
    const bool mine = d == c;
    uint32_t o = 0;
    if (!mine || lane_id() == (uint32_t)__builtin_ctzll(m)) o = atomicAdd(&cnt[d], mine ? (uint32_t)__popcll(m) : 1u);
    return o;
}
__device__ __forceinline__ uint32_t hot_rank(uint32_t o, uint32_t d, uint32_t c, uint64_t m) {
    if (c == 0xFFFFFFFFu) return o;
    const uint32_t base = __builtin_amdgcn_readlane(o, (uint32_t)__builtin_ctzll(m));
    return d == c ? base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) : o;
}

// Row stride of per-wave digit counters [wave][digit] read column-wise by digit groups: TPD threads
// per digit, thread `sub` taking rows sub * WPT .. + WPT - 1. With rows R apart (R a multiple of
// 64) the TPD threads of a digit hit one bank; a stride with WPT * RS = 64 / TPD (mod 64) puts the
// 64 / TPD digits x TPD threads of a wave on 64 different banks (k = 8, 1024 threads: 260;
// dev/lines_exp.hip "lx pad": step 2 2.1K -> 1.75K cycles per tile, C3 pass -1.5 %). Groups wider
// than the wave count (WPT = 0 here) read one row per thread and keep R.
template <uint32_t R, uint32_t TPD, uint32_t WPT>
constexpr uint32_t counter_stride() {
    if (TPD < 2 || WPT == 0 || 64 % TPD != 0) return R;
    for (uint32_t p = 0; p < 64; ++p)
        if (((R + p) * WPT) % 64 == (64 / TPD) % 64) return R + p;
    return R;
}

// Value of lane (first lane of this lane's aligned group of TPD lanes) + q, for q < TPD: DPP
// quad permutes (one VALU, no LDS) for groups of up to 4 lanes, ds_bpermute otherwise.
template <uint32_t TPD>
__device__ __forceinline__ uint32_t group_lane(uint32_t x, uint32_t q) {
    if constexpr (TPD == 1) {
        return x;
    } else if constexpr (TPD == 2) {
        // quad_perm (0,0,2,2) / (1,1,3,3)
        return q == 0 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xA0, 0xF, 0xF, false)
                      : (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xF5, 0xF, 0xF, false);
    } else if constexpr (TPD == 4) {
        switch (q) {
            case 0: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x00, 0xF, 0xF, false);
            case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x55, 0xF, 0xF, false);
            case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xAA, 0xF, 0xF, false);
            default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xFF, 0xF, 0xF, false);
        }
    } else {
        return (uint32_t)__shfl((int)x, (int)((lane_id() & ~(TPD - 1u)) + q));
    }
}

// Exclusive prefix (pre) of x over the lanes of this lane's aligned group of TPD lanes below it
// (sub = lane % TPD) and the group's total. Small groups: one group_lane per member; groups of
// 16..64 lanes: the DPP row scan of wave_incl_scan cut to the group, plus one bpermute for the
// total. Every lane of the wave must call it.
template <uint32_t TPD>
__device__ __forceinline__ void group_scan(uint32_t x, uint32_t sub, uint32_t &pre, uint32_t &tot) {
    if constexpr (TPD <= 8) {
        pre = 0;
        tot = 0;
#pragma unroll
        for (uint32_t q = 0; q < TPD; ++q) {
            const uint32_t y = group_lane<TPD>(x, q);
            if (q < sub) pre += y;
            tot += y;
        }
    } else {
        static_assert(TPD == 16 || TPD == 32 || TPD == 64, "groups of 16, 32 or 64 lanes");
        uint32_t v = x;
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
        if constexpr (TPD >= 32)
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
        if constexpr (TPD == 64)
            v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
        pre = v - x;
        tot = (uint32_t)__shfl((int)v, (int)((lane_id() & ~(TPD - 1u)) + TPD - 1u));
    }
}

// Mask (lo, hi halves) of the lanes of this wave whose BITS-bit digit equals this lane's:
// AND over bits b of (ballot(bit b) XNOR my bit b), one v_bitop3 per half per bit
// (truth table 0x90 = a & ~(b ^ c) with a = mask, b = ballot half, c = my bit as 0 / ~0).
template <int BITS>
__device__ __forceinline__ void peer_mask(uint32_t d, uint32_t &mlo, uint32_t &mhi) {
    mlo = ~0u;
    mhi = ~0u;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        int s = __builtin_amdgcn_sbfe((int)d, b, 1);
        asm volatile("" : "+v"(s));  // keep s opaque: the ballot then compares s itself (1 VALU)
        const uint64_t bal = __ballot(s);
        mlo = __builtin_amdgcn_bitop3_b32(mlo, (uint32_t)bal, (uint32_t)s, 0x90);
        mhi = __builtin_amdgcn_bitop3_b32(mhi, (uint32_t)(bal >> 32), (uint32_t)s, 0x90);
    }
}

// Ranking of one whole-wave slot: adds its 64 BITS-bit digits to the wave's counter row and returns each lane's
// stable rank among the row's keys of its digit so far: rank_add, or (kRankCount) the ballot peer match.
template <int BITS, int RANK>
__device__ __forceinline__ uint32_t slot_rank(uint32_t *row, uint32_t d) {
    if constexpr (RANK == kRankAtomic) {
        return rank_add(row, d);
    } else {
        uint32_t mlo, mhi;
        peer_mask<BITS>(d, mlo, mhi);
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
        const uint32_t old = row[d];
        if (pre == 0) row[d] = old + (uint32_t)(__builtin_popcount(mlo) + __builtin_popcount(mhi));
        return old + pre;
    }
}

// Per-tile check of the kRankAtomic premise (the reference checks every sort,
// Parallel7.cu:679-687). The line and pairs kernels and rs_scatter run it on the first slot of a full tile
// (every kRankCheckEvery-th tile of a chunk): each lane's rank r from the lane-ordered returning adds must
// be base + (#lower lanes with its digit), with ONE base for all lanes of a digit. The lanes of a digit
// come from BITS ballots (peer_mask), the base of the digit's first lane from one ds_bpermute. A change of
// the lane order would permute the ranks among a digit's lanes -- the same keys in a wrong order, an
// unstable sort that no checksum of the keys can see -- and duplicated ranks (lost keys) fail the same
// test. Returns 1 where it failed. fault != 0 (test hook rsort_inject_rank_fault, ScatterArgs::rank_fault):
// the first two lanes of every digit swap their ranks first, as a broken lane order would. ~40 VALU and
// one bpermute per wave and checked tile; every lane of the wave must take part (full tiles only).
template <int BITS>
__device__ __forceinline__ uint32_t rank_check(uint32_t d, uint32_t &r, uint32_t fault) {
    uint32_t mlo, mhi;
    peer_mask<BITS>(d, mlo, mhi);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
    if (fault != 0u) {
        const uint32_t peers = (uint32_t)__builtin_popcount(mlo) + (uint32_t)__builtin_popcount(mhi);
        if (peers >= 2u && below < 2u) r = below == 0u ? r + 1u : r - 1u;
    }
    const uint32_t b = r - below;
    const uint32_t first = mlo != 0u ? (uint32_t)__builtin_ctz(mlo) : 32u + (uint32_t)__builtin_ctz(mhi);
    return (uint32_t)__shfl((int)b, (int)first) != b ? 1u : 0u;
}

// Tiles between rank checks in a chunk (a power of 2): the check on every tile cost C3 / C4 ~1 % (same-box
// A/B); every 8th, starting with each chunk's first tile, checks 8-64 tiles per chunk and pass at C3 / C4.
constexpr uint32_t kRankCheckEvery = 8;

// End of a scatter workgroup: a wave any of whose lanes saw a failed rank_check sets kCheckRankOrder in the
// sort's check word (rsort_plan_check; the host entries return RSORT_ERR_CHECK). Every lane must call it.
__device__ __forceinline__ void report_order(uint32_t *check, uint32_t bad) {
    if (check != nullptr && __ballot(bad != 0u) != 0ull && lane_id() == 0) atomicOr(check, kCheckRankOrder);
}

// Inclusive wave64 scan with DPP row shifts + row broadcasts (no LDS, no bpermute):
// row_shr:1,2,4,8 scan each row of 16 lanes, row_bcast:15 / row_bcast:31 carry row totals.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return x;
}

// Exclusive scan of one value per thread across the workgroup. All threads must call it.
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_ws, uint32_t &total) {
    constexpr int W = THREADS / kWave;
    const uint32_t w = threadIdx.x / kWave;
    const uint32_t inc = wave_incl_scan(v);
    if (lane_id() == kWave - 1) s_ws[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const uint32_t s = s_ws[i];
        pre += ((uint32_t)i < w) ? s : 0u;
        tot += s;
    }
    total = tot;
    __syncthreads();
    return pre + inc - v;
}

// Same, with one barrier: the caller guarantees another barrier before s_ws is written again.
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_scan1(uint32_t v, uint32_t *s_ws, uint32_t &total) {
    constexpr int W = THREADS / kWave;
    const uint32_t w = threadIdx.x / kWave;
    const uint32_t inc = wave_incl_scan(v);
    if (lane_id() == kWave - 1) s_ws[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const uint32_t s = s_ws[i];
        pre += ((uint32_t)i < w) ? s : 0u;
        tot += s;
    }
    total = tot;
    return pre + inc - v;
}

}  // namespace rsort

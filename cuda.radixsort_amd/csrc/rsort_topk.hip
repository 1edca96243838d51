// rsort_topk.hip -- the select kernels of rsort_u32_topk_device (include/rsort.h, "top-k selection"): a radix
// select over x = key ^ m in three levels of 8 / 12 / 12 bits from the top (rsort_internal.hpp, TopkArgs).
//
// Every kernel but the picks runs on a host-known grid of G workgroups; workgroup g owns one contiguous slice of
// whole tiles of its list and computes it from the list's length, which is n for the input and a device-side
// count for the candidate list A -- the host knows no size but n and k. All ordering between workgroups is by
// kernel boundaries: no look-back, no flags, nothing crosses workgroups inside a kernel but integer atomic adds
// into the zeroed bin totals, whose sum does not depend on their order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rsort.h"
#include "rsort_device.hpp"
#include "rsort_internal.hpp"

namespace rsort {
namespace {

constexpr int kWaves = kTopkThreads / kWave;

// This workgroup's slice [start, end) of a list of len entries: whole tiles, ceil(tiles / G) each.
__device__ __forceinline__ void tk_slice(uint64_t len, uint64_t &start, uint64_t &end) {
    const uint64_t tiles = (len + kTopkTile - 1) / kTopkTile;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x;
    start = min(len, (uint64_t)blockIdx.x * per * kTopkTile);
    end = min(len, start + per * kTopkTile);
}

__device__ __forceinline__ const uint32_t *tk_totals(const TopkArgs &a, int level) {
    return a.totals + (level == 0 ? 0u : level == 1 ? kTopkBins0 : kTopkBins0 + kTopkBins);
}

// Level 0: the top 8 bits of every x of the input, eight sub-counter rows (a wave adds into row wave % 8; a run of
// equal digits is added once per wave, count_add) -> this slice's row of counts and of their exclusive prefix over
// the digits, and the totals. Level 1: bits 12..23 of the candidates (all share the top digit). Level 2: bits
// 0..11 of the candidates whose upper 20 bits are the chosen ones.
template <int LEVEL>
__global__ __launch_bounds__(kTopkThreads) void tk_count(TopkArgs a) {
    constexpr uint32_t BINS = LEVEL == 0 ? kTopkBins0 : kTopkBins;
    constexpr uint32_t SUBS = LEVEL == 0 ? 8 : 1;
    __shared__ uint32_t s_h[BINS * SUBS];
    __shared__ uint32_t s_ws[kWaves];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < BINS * SUBS; i += kTopkThreads) s_h[i] = 0;
    __syncthreads();
    const uint64_t len = LEVEL == 0 ? a.n : (uint64_t)a.state[kTkCand];
    const uint32_t *keys = LEVEL == 0 ? a.kin : a.ak;
    const uint32_t m = LEVEL == 0 ? a.m : 0u;  // (A holds x already)
    const bool vec = LEVEL == 0 ? a.vec != 0u : true;  // (A is 256-B aligned, a slice starts on a tile)
    const uint32_t prefix = LEVEL == 2 ? a.state[kTkPrefix] : 0u;
    uint32_t *h = s_h + (LEVEL == 0 ? ((t / kWave) & 7u) * BINS : 0u);
    auto add = [&](uint32_t key) {
        const uint32_t x = key ^ m;
        if constexpr (LEVEL == 0) {
            count_add(h, x >> 24);
        } else if constexpr (LEVEL == 1) {
            count_add(h, (x >> 12) & 0xFFFu);
        } else {
            if ((x >> 12) == prefix) count_add(h, x & 0xFFFu);
        }
    };
    uint64_t start, end;
    tk_slice(len, start, end);
    for (uint64_t base = start; base < end; base += kTopkTile) {
        if (vec && base + kTopkTile <= end) {
            const uint4 v = reinterpret_cast<const uint4 *>(keys + base)[t];
            add(v.x);
            add(v.y);
            add(v.z);
            add(v.w);
        } else {
#pragma unroll
            for (int j = 0; j < kTopkKpt; ++j) {
                const uint64_t i = base + (uint64_t)j * kTopkThreads + t;
                if (i < end) add(keys[i]);
            }
        }
    }
    __syncthreads();
    uint32_t *tot = const_cast<uint32_t *>(tk_totals(a, LEVEL));
    if constexpr (LEVEL == 0) {
        uint32_t c = 0;
        if (t < BINS)
            for (uint32_t s = 0; s < SUBS; ++s) c += s_h[s * BINS + t];
        uint32_t total;
        const uint32_t pre = block_excl_scan<kTopkThreads>(c, s_ws, total);
        if (t < BINS) {  // (every workgroup writes its row, an empty slice zeros: the pick reads all G rows)
            a.rows_cnt[(size_t)blockIdx.x * BINS + t] = c;
            a.rows_pre[(size_t)blockIdx.x * BINS + t] = pre;
            if (c) atomicAdd(&tot[t], c);
        }
    } else {
        for (uint32_t i = t; i < BINS; i += kTopkThreads) {
            const uint32_t c = s_h[i];
            if (c) atomicAdd(&tot[i], c);
        }
    }
}

// One workgroup: the scan of a level's totals, the bin b that holds the want-th candidate (want = k at level 0,
// else what the level above left) and the rest wanted from inside b; the chosen digits so far become the prefix.
// Level 0 also turns the slice rows into every slice's exclusive offsets for its entries below b (into W) and in
// b (into A), one slice per thread.
template <int LEVEL>
__global__ __launch_bounds__(kTopkThreads) void tk_pick(TopkArgs a, uint32_t grid) {
    constexpr uint32_t BINS = LEVEL == 0 ? kTopkBins0 : kTopkBins;
    constexpr uint32_t PER = LEVEL == 0 ? 1 : kTopkBins / kTopkThreads;
    __shared__ uint32_t s_ws[kWaves];
    __shared__ uint32_t s_pick[4];  // {b, rest, entries in b, entries below b}
    const uint32_t t = threadIdx.x;
    const uint32_t *tot = tk_totals(a, LEVEL);
    const uint32_t want = LEVEL == 0 ? a.k : a.state[kTkKrem];
    const uint32_t oldp = LEVEL == 0 ? 0u : a.state[kTkPrefix];
    if (t < 4) s_pick[t] = 0;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
        const uint32_t bin = t * PER + j;
        c[j] = bin < BINS ? tot[bin] : 0u;
        sum += c[j];
    }
    uint32_t total;
    uint32_t ex = block_excl_scan<kTopkThreads>(sum, s_ws, total);
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
        if (ex < want && want - ex <= c[j]) {  // (exactly one bin: 1 <= want <= the level's total)
            s_pick[0] = t * PER + j;
            s_pick[1] = want - ex;
            s_pick[2] = c[j];
            s_pick[3] = ex;
        }
        ex += c[j];
    }
    __syncthreads();
    const uint32_t b = s_pick[0];
    if (t == 0) {
        a.state[kTkKrem] = s_pick[1];
        a.state[kTkPrefix] = LEVEL == 0 ? b : (oldp << 12) | b;
        if constexpr (LEVEL == 0) {
            a.state[kTkCand] = s_pick[2];
            a.state[kTkBelow0] = s_pick[3];
        }
    }
    if constexpr (LEVEL == 0) {
        const uint32_t below = t < grid ? a.rows_pre[(size_t)t * BINS + b] : 0u;
        const uint32_t equal = t < grid ? a.rows_cnt[(size_t)t * BINS + b] : 0u;
        const uint32_t pb = block_excl_scan<kTopkThreads>(below, s_ws, total);
        const uint32_t pe = block_excl_scan<kTopkThreads>(equal, s_ws, total);
        if (t < grid) {
            a.offs0[2 * t] = pb;
            a.offs0[2 * t + 1] = pe;
        }
    }
}

// The candidates' entries against the k-th x, T: every slice's counts {x < T, x == T}.
__global__ __launch_bounds__(kTopkThreads) void tk_tie_count(TopkArgs a) {
    __shared__ uint32_t s_c[2];
    const uint32_t t = threadIdx.x;
    if (t < 2) s_c[t] = 0;
    __syncthreads();
    const uint64_t len = a.state[kTkCand];
    const uint32_t T = a.state[kTkPrefix];
    uint64_t start, end;
    tk_slice(len, start, end);
    uint32_t less = 0, equal = 0;
    for (uint64_t base = start; base < end; base += kTopkTile) {
        if (base + kTopkTile <= end) {
            const uint4 v = reinterpret_cast<const uint4 *>(a.ak + base)[t];
            less += (v.x < T) + (v.y < T) + (v.z < T) + (v.w < T);
            equal += (v.x == T) + (v.y == T) + (v.z == T) + (v.w == T);
        } else {
#pragma unroll
            for (int j = 0; j < kTopkKpt; ++j) {
                const uint64_t i = base + (uint64_t)j * kTopkThreads + t;
                const uint32_t x = i < end ? a.ak[i] : 0u;
                less += (i < end && x < T) ? 1u : 0u;
                equal += (i < end && x == T) ? 1u : 0u;
            }
        }
    }
    less = wave_incl_scan(less);
    equal = wave_incl_scan(equal);
    if (lane_id() == kWave - 1) {
        atomicAdd(&s_c[0], less);
        atomicAdd(&s_c[1], equal);
    }
    __syncthreads();
    if (t < 2) a.offs1[2 * blockIdx.x + t] = s_c[t];  // (every workgroup: the emit reads all G pairs)
}

// The two ranking kernels: each workgroup walks its slice tile by tile, every wave a contiguous 256 entries as
// four wave-striped loads, and ranks two classes of entries in input order with ballots (wave_count of the lanes
// below, the wave's running counts, the waves' prefix inside the tile, the slice's running bases).
//   MODE 0, level 0's compact: the input's entries below the chosen top digit -> W, those with it -> A (x, and the
//     value or, with indices, the position: the loop index, nothing is read for it).
//   MODE 1, the emit: A's entries with x < T -> W behind level 0's, then the first k_rem with x == T behind those.
//     Its slice's bases are the sums of the lower slices' tie counts, which every workgroup adds up itself; the
//     first workgroup writes the report words.
template <int MODE>
__global__ __launch_bounds__(kTopkThreads) void tk_rank(TopkArgs a) {
    __shared__ uint32_t s_ws[kWaves], s_w0[kWaves], s_w1[kWaves];
    const uint32_t t = threadIdx.x, w = t / kWave, lane = lane_id(), g = blockIdx.x;
    const uint64_t len = MODE == 0 ? a.n : (uint64_t)a.state[kTkCand];
    const uint32_t *ksrc = MODE == 0 ? a.kin : a.ak;
    const uint32_t *vsrc = MODE == 0 ? a.vin : a.av;
    const uint32_t m = MODE == 0 ? a.m : 0u;
    const uint32_t T = a.state[kTkPrefix];  // MODE 0: the chosen top digit; MODE 1: the k-th x
    uint32_t *const k0 = a.wk, *const v0 = a.wv;
    uint32_t *const k1 = MODE == 0 ? a.ak : a.wk, *const v1 = MODE == 0 ? a.av : a.wv;
    uint32_t base0, base1, lim0 = a.k, lim1;  // (lim: one past the last position a class may write)
    if constexpr (MODE == 0) {
        base0 = a.offs0[2 * g];
        base1 = a.offs0[2 * g + 1];
        lim1 = (uint32_t)a.n;
    } else {
        const uint32_t l = t < gridDim.x ? a.offs1[2 * t] : 0u, e = t < gridDim.x ? a.offs1[2 * t + 1] : 0u;
        uint32_t lpre, epre, ltot, etot;
        block_excl_scan<kTopkThreads>(t < g ? l : 0u, s_ws, lpre);
        block_excl_scan<kTopkThreads>(t < g ? e : 0u, s_ws, epre);
        block_excl_scan<kTopkThreads>(l, s_ws, ltot);
        block_excl_scan<kTopkThreads>(e, s_ws, etot);
        const uint32_t below0 = a.state[kTkBelow0], krem = a.state[kTkKrem];
        base0 = below0 + lpre;
        base1 = below0 + ltot + epre;
        lim1 = min(a.k, below0 + ltot + krem);
        if (g == 0 && t == 0) {
            a.state[kTkRoute] = RSORT_TOPK_SELECT;
            a.state[kTkKth] = T ^ a.m;
            a.state[kTkBefore] = below0 + ltot;
            a.state[kTkTaken] = krem;
            a.state[kTkEqual] = etot;
        }
    }
    uint64_t start, end;
    tk_slice(len, start, end);
    for (uint64_t base = start; base < end; base += kTopkTile) {
        uint32_t x[kTopkKpt], c[kTopkKpt], r[kTopkKpt], n0 = 0, n1 = 0;
#pragma unroll
        for (int j = 0; j < kTopkKpt; ++j) {
            const uint64_t i = base + (uint64_t)w * (kWave * kTopkKpt) + (uint64_t)j * kWave + lane;
            const bool ok = i < end;
            x[j] = ok ? ksrc[i] ^ m : 0u;
            const uint32_t d = MODE == 0 ? x[j] >> 24 : x[j];
            c[j] = !ok ? 2u : d < T ? 0u : d == T ? 1u : 2u;
            const uint64_t m0 = __ballot(c[j] == 0u), m1 = __ballot(c[j] == 1u);
            r[j] = c[j] == 0u ? n0 + (uint32_t)__popcll(m0 & lanes_below()) : n1 + (uint32_t)__popcll(m1 & lanes_below());
            n0 += wave_count(m0);
            n1 += wave_count(m1);
        }
        if (lane == 0) {
            s_w0[w] = n0;
            s_w1[w] = n1;
        }
        __syncthreads();
        uint32_t p0 = 0, p1 = 0, t0 = 0, t1 = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const uint32_t u0 = s_w0[i], u1 = s_w1[i];
            p0 += (uint32_t)i < w ? u0 : 0u;
            p1 += (uint32_t)i < w ? u1 : 0u;
            t0 += u0;
            t1 += u1;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTopkKpt; ++j) {
            if (c[j] == 2u) continue;
            const uint64_t i = base + (uint64_t)w * (kWave * kTopkKpt) + (uint64_t)j * kWave + lane;
            const uint32_t pos = (c[j] == 0u ? base0 + p0 : base1 + p1) + r[j];
            if (pos >= (c[j] == 0u ? lim0 : lim1)) continue;  // (class 1 of the emit: the ties beyond the first k_rem)
            uint32_t *kd = c[j] == 0u ? k0 : k1, *vd = c[j] == 0u ? v0 : v1;
            kd[pos] = x[j];
            if (a.pairs) vd[pos] = (MODE == 0 && a.indices) ? (uint32_t)i : vsrc[i];
        }
        base0 += t0;
        base1 += t1;
    }
}

__global__ __launch_bounds__(256) void tk_copy(TopkCopyArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.k; i += stride) {
        const uint32_t key = a.kin[a.rev ? a.n - 1 - i : i] ^ a.m;
        a.kout[i] = key;
        if (a.vout != nullptr) a.vout[i] = a.vin[i];
        if (a.state != nullptr && i == a.k - 1) {
            a.state[kTkRoute] = RSORT_TOPK_SORT;
            a.state[kTkKth] = key;
            a.state[6] = 0;
            a.state[7] = 0;
        }
    }
}

bool grid_ok(uint32_t grid) { return grid >= 1 && grid <= kTopkMaxGrid; }

}  // namespace

hipError_t launch_topk_count(int level, const TopkArgs &a, uint32_t grid, hipStream_t s) {
    if (!grid_ok(grid) || level < 0 || level > 2) return hipErrorInvalidValue;
    if (level == 0) hipLaunchKernelGGL(tk_count<0>, dim3(grid), dim3(kTopkThreads), 0, s, a);
    else if (level == 1) hipLaunchKernelGGL(tk_count<1>, dim3(grid), dim3(kTopkThreads), 0, s, a);
    else hipLaunchKernelGGL(tk_count<2>, dim3(grid), dim3(kTopkThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_pick(int level, const TopkArgs &a, uint32_t grid, hipStream_t s) {
    if (!grid_ok(grid) || level < 0 || level > 2) return hipErrorInvalidValue;
    if (level == 0) hipLaunchKernelGGL(tk_pick<0>, dim3(1), dim3(kTopkThreads), 0, s, a, grid);
    else if (level == 1) hipLaunchKernelGGL(tk_pick<1>, dim3(1), dim3(kTopkThreads), 0, s, a, grid);
    else hipLaunchKernelGGL(tk_pick<2>, dim3(1), dim3(kTopkThreads), 0, s, a, grid);
    return hipGetLastError();
}

hipError_t launch_topk_compact(const TopkArgs &a, uint32_t grid, hipStream_t s) {
    if (!grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tk_rank<0>, dim3(grid), dim3(kTopkThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_tie_count(const TopkArgs &a, uint32_t grid, hipStream_t s) {
    if (!grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tk_tie_count, dim3(grid), dim3(kTopkThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_emit(const TopkArgs &a, uint32_t grid, hipStream_t s) {
    if (!grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tk_rank<1>, dim3(grid), dim3(kTopkThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_copy(const TopkCopyArgs &a, hipStream_t s) {
    if (a.k == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((a.k + 1023) / 1024, 4096);
    hipLaunchKernelGGL(tk_copy, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

int topk_blocks_per_cu() {
    const void *fns[] = {(const void *)tk_count<0>, (const void *)tk_count<1>, (const void *)tk_count<2>,
                         (const void *)tk_tie_count, (const void *)tk_rank<0>, (const void *)tk_rank<1>};
    int least = 0;
    for (const void *fn : fns) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, kTopkThreads, 0) != hipSuccess) return 0;
        least = least == 0 ? nb : std::min(least, nb);
    }
    return least;
}

}  // namespace rsort

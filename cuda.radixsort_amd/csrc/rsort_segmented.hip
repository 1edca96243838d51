// rsort_segmented.hip -- the segmented sort: many independent segments of one array in one call.
//
// Five launches after a 256-B memset of the counters (include/rsort.h, rsort_u32_segmented_device):
//
//   rs_seg_classify  one thread per segment: validates [off[i], off[i+1]) against n BEFORE anything uses it,
//                    appends the segment's index to the list of its kind -- wave (<= kSegWaveKeys keys), small
//                    (<= kSegSmallKeys), lds (<= kSegLdsKeys) or multi-tile -- and counts it; a bad pair of offsets
//                    is counted as rejected, sets kCheckOffsets and enters no list, so no kernel ever sees it
//   rs_seg_wave      one WAVE per segment, four segments per 256-thread workgroup, no workgroup barrier
//   rs_seg_lds       one workgroup per segment (grid-stride over a class list), two shapes: the segment lives in
//                    registers in wave-striped order, four 8-bit counting passes rank it with per-wave LDS
//                    counter rows (the product form of dev/msd_lab.hip's bucket_sort16), each pass writes the
//                    keys to their LDS position and reads them back, the last one stores the segment with
//                    16-B quads where the output address allows
//   rs_seg_tiles     one 1024-thread workgroup per segment longer than the LDS capacity: one read counts all four
//                    digit histograms, then four passes in -> tmp -> out -> tmp -> out walk the segment's tiles in
//                    order with running digit bases. One CU sorts the whole segment: the correctness net.
//
// Partial slots: a segment is ranked as if it had roundup(n, 64) keys, the missing ones being 0xFFFFFFFF pads
// in the highest lanes of its last slot. A pad holds digit 255 in every pass and follows every real key in
// input order, so the stable counting sort leaves the pads at positions >= n in every pass (they are never
// stored) and no real key's rank depends on them. Every ranked slot is then a whole wave: rank_add needs no
// masked form and the ballot peer match (which needs all 64 lanes) serves partial slots too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsort_device.hpp"
#include "rsort_hooks.hpp"
#include "rsort_internal.hpp"

namespace rsort {

namespace {

constexpr uint32_t kPadKey = 0xFFFFFFFFu;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------ classification
__global__ __launch_bounds__(256) void rs_seg_classify(SegClassifyArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    // a SegKind, kSegRejected, or nothing to do (empty, or past the last segment)
    constexpr uint32_t kNone = kSegRejected + 1;
    uint32_t cls = kNone;
    if (i < a.num_segments) {
        const uint32_t b = a.off[i], e = a.off[i + 1];
        if (b > e || (uint64_t)e > a.n) cls = kSegRejected;
        else if (e - b == 0) cls = kNone;
        else if (e - b <= (uint32_t)kSegWaveKeys) cls = kSegWave;
        else if (e - b <= (uint32_t)kSegSmallKeys) cls = kSegSmall;
        else if (e - b <= (uint32_t)kSegLdsKeys) cls = kSegLds;
        else cls = kSegTiles;
    }
    // one global add per wave and kind: its lanes take consecutive list slots (any order will do)
#pragma unroll
    for (uint32_t c = 0; c <= (uint32_t)kSegRejected; ++c) {
        const uint64_t m = __ballot(cls == c);
        if (m == 0ull) continue;
        const uint32_t first = (uint32_t)__builtin_ctzll(m);
        uint32_t base = 0;
        if (lane_id() == first) {
            base = atomicAdd(&a.counters[c], (uint32_t)__popcll(m));
            if (c == (uint32_t)kSegRejected) atomicOr(&a.counters[kSegCheckWord], kCheckOffsets);
        }
        base = __builtin_amdgcn_readlane(base, first);
        if (cls == c && c < (uint32_t)kSegKinds)
            a.lists[c % kSegKinds][base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i;
    }
}

// ------------------------------------------------------------------------------ the store of a sorted segment
// o[4q .. 4q + 3] = x[4q .. 4q + 3] for the quads covering x[a, a + n): o is the segment's output moved down by
// a < 4 words to a 16-B boundary, so whole quads inside the segment go out as 16-B stores and the words at its
// two ends one by one. Thread `t` of `threads` takes every threads-th quad.
__device__ __forceinline__ void store_segment(uint32_t *o, const uint32_t *x, uint32_t a, uint32_t n, uint32_t t,
                                              uint32_t threads) {
    const uint32_t nq = (a + n + 3) / 4;
    for (uint32_t q = t; q < nq; q += threads) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(&x[4 * q]);
        if (4 * q >= a && 4 * q + 4 <= a + n) {
            *reinterpret_cast<u32x4 *>(o + 4 * q) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (4 * q + i >= a && 4 * q + i < a + n) o[4 * q + i] = v[i];
        }
    }
}

// ------------------------------------------------------------------------------ one wave per segment
// Segments of up to 64 x kSegWaveKpt keys: lane l holds keys l, 64 + l, ...; the wave has its own counter row and
// tile in LDS and never meets a workgroup barrier (a wave's LDS instructions complete in order; the wave
// barriers only keep the compiler from moving them). The 256 digit counters are scanned four to a lane.
template <int PAIRS, int RANK>
__global__ __launch_bounds__(256) void rs_seg_wave(SegSortArgs a) {
    constexpr int W = 256 / kWave, KPT = kSegWaveKpt;
    constexpr uint32_t CAP = kWave * KPT;
    __shared__ __attribute__((aligned(16))) uint32_t s_k[W][CAP + 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_v[PAIRS ? W : 1][PAIRS ? CAP + 4 : 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[W][256];
    const uint32_t w = threadIdx.x / kWave, lane = lane_id();
    uint32_t *row = s_cnt[w], *xk = s_k[w], *xv = s_v[PAIRS ? w : 0];
    const uint32_t nseg = *a.count;
    uint32_t order_bad = 0;
    for (uint32_t b = blockIdx.x * W + w; b < nseg; b += gridDim.x * W) {
        const uint32_t sg = a.list[b];
        const uint32_t s = a.off[sg], n = a.off[sg + 1] - s;  // (classified: 0 < n <= CAP, s + n <= a.n)
        const uint32_t ak = (uint32_t)(((uintptr_t)(a.kout + s) >> 2) & 3u);
        const uint32_t av = PAIRS ? (uint32_t)(((uintptr_t)(a.vout + s) >> 2) & 3u) : 0u;
        uint32_t key[KPT], val[PAIRS ? KPT : 1];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t i = j * kWave + lane;
            key[j] = i < n ? a.kin[s + i] : kPadKey;
            if constexpr (PAIRS) val[j] = i < n ? a.vin[s + i] : 0u;
        }
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t sh = pass * 8;
            *reinterpret_cast<u32x4 *>(&row[4 * lane]) = u32x4{0u, 0u, 0u, 0u};
            __builtin_amdgcn_wave_barrier();
            uint32_t rk[KPT];
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                rk[j] = 0;
                if ((uint32_t)(j * kWave) < n) {  // (wave-uniform: the slot holds a key; lanes past n hold pads)
                    const uint32_t d = (key[j] >> sh) & 255u;
                    rk[j] = slot_rank<8, RANK>(row, d);
                    if constexpr (RANK == kRankAtomic) {
                        if (j == 0 && (uint32_t)kWave <= n) order_bad |= rank_check<8>(d, rk[j], a.rank_fault);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            {
                // exclusive scan of the 256 counts: lane l owns digits 4 l .. 4 l + 3
                const u32x4 c = *reinterpret_cast<const u32x4 *>(&row[4 * lane]);
                const uint32_t sum = c[0] + c[1] + c[2] + c[3];
                const uint32_t ex = wave_incl_scan(sum) - sum;
                *reinterpret_cast<u32x4 *>(&row[4 * lane]) = u32x4{ex, ex + c[0], ex + c[0] + c[1], ex + c[0] + c[1] + c[2]};
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                if ((uint32_t)(j * kWave) < n) {
                    const uint32_t p = row[(key[j] >> sh) & 255u] + rk[j];  // (< roundup(n, 64) <= CAP)
                    xk[ak + p] = key[j];
                    if constexpr (PAIRS) xv[av + p] = val[j];
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (pass < 3) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    if ((uint32_t)(j * kWave) < n) {
                        key[j] = xk[ak + j * kWave + lane];
                        if constexpr (PAIRS) val[j] = xv[av + j * kWave + lane];
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        store_segment(a.kout + s - ak, xk, ak, n, lane, (uint32_t)kWave);
        if constexpr (PAIRS) store_segment(a.vout + s - av, xv, av, n, lane, (uint32_t)kWave);
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (RANK == kRankAtomic) report_order(a.check, order_bad);
}

// ------------------------------------------------------------------------------ in-LDS sort
// Wave w holds keys [w * span, (w + 1) * span) of the segment, slot j its keys w * span + 64 j + lane; span is
// the segment's share per wave rounded up to whole slots (<= 64 KPT), so a segment shorter than the capacity
// still spreads over all waves. (wave, slot, lane) order is input order: the ranks are stable.
template <int THREADS, int KPT, int PAIRS, int RANK>
__global__ __launch_bounds__(THREADS) void rs_seg_lds(SegSortArgs a) {
    constexpr int W = THREADS / kWave;
    constexpr uint32_t CAP = THREADS * KPT;
    __shared__ __attribute__((aligned(16))) uint32_t s_k[CAP + 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_v[PAIRS ? CAP + 4 : 4];
    __shared__ uint32_t s_cnt[W * 256];
    __shared__ uint32_t s_ws[W];
    const uint32_t t = threadIdx.x, w = t / kWave, lane = lane_id();
    const uint32_t nseg = *a.count;
    uint32_t order_bad = 0;
    for (uint32_t b = blockIdx.x; b < nseg; b += gridDim.x) {
        const uint32_t sg = a.list[b];
        const uint32_t s = a.off[sg], n = a.off[sg + 1] - s;  // (classified: 0 < n <= CAP, s + n <= a.n)
        const uint32_t n64 = (n + 63u) & ~63u;
        const uint32_t span = ((n64 / 64u + W - 1) / W) * 64u;
        const uint32_t i0 = w * span + lane;
        // s_k[ak + i] holds key i: quads of s_k are then 16-B aligned in kout (any 4-B-aligned base)
        const uint32_t ak = (uint32_t)(((uintptr_t)(a.kout + s) >> 2) & 3u);
        const uint32_t av = PAIRS ? (uint32_t)(((uintptr_t)(a.vout + s) >> 2) & 3u) : 0u;
        uint32_t key[KPT], val[PAIRS ? KPT : 1];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t i = i0 + j * kWave;
            const bool in = (uint32_t)(j * kWave) < span && i < n;
            key[j] = in ? a.kin[s + i] : kPadKey;
            if constexpr (PAIRS) val[j] = in ? a.vin[s + i] : 0u;
        }
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t sh = pass * 8;
            uint32_t *row = &s_cnt[w * 256];
            for (uint32_t i = lane; i < 256; i += kWave) row[i] = 0;
            uint32_t rk[KPT];
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                rk[j] = 0;
                // (wave-uniform: the slot holds a key; its lanes past n hold pads)
                if ((uint32_t)(j * kWave) < span && w * span + j * kWave < n) {
                    const uint32_t d = (key[j] >> sh) & 255u;
                    rk[j] = slot_rank<8, RANK>(row, d);
                    if constexpr (RANK == kRankAtomic) {
                        if (j == 0 && w * span + kWave <= n) order_bad |= rank_check<8>(d, rk[j], a.rank_fault);
                    }
                }
            }
            __syncthreads();
            // per digit: exclusive prefix over the waves' rows (in place), then over the digits
            uint32_t tot = 0;
            if (t < 256) {
#pragma unroll
                for (int x = 0; x < W; ++x) {
                    const uint32_t c = s_cnt[x * 256 + t];
                    s_cnt[x * 256 + t] = tot;
                    tot += c;
                }
            }
            uint32_t all;
            const uint32_t dbase = block_excl_scan<THREADS>(t < 256 ? tot : 0u, s_ws, all);
            if (t < 256) {
#pragma unroll
                for (int x = 0; x < W; ++x) s_cnt[x * 256 + t] += dbase;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                if ((uint32_t)(j * kWave) < span && w * span + j * kWave < n) {
                    const uint32_t p = row[(key[j] >> sh) & 255u] + rk[j];  // (< n64 <= CAP)
                    s_k[ak + p] = key[j];
                    if constexpr (PAIRS) s_v[av + p] = val[j];
                }
            }
            __syncthreads();
            if (pass < 3) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    if ((uint32_t)(j * kWave) < span && w * span + j * kWave < n) {
                        const uint32_t i = i0 + j * kWave;
                        key[j] = s_k[ak + i];
                        if constexpr (PAIRS) val[j] = s_v[av + i];
                    }
                }
                __syncthreads();
            }
        }
        store_segment(a.kout + s - ak, s_k, ak, n, t, (uint32_t)THREADS);
        if constexpr (PAIRS) store_segment(a.vout + s - av, s_v, av, n, t, (uint32_t)THREADS);
        __syncthreads();
    }
    if constexpr (RANK == kRankAtomic) report_order(a.check, order_bad);
}

// ------------------------------------------------------------------------------ multi-tile sort
// Tiles of 1024 x 8 keys, wave w holding keys [512 w, 512 w + 512) of the tile. No tile buffer: a key goes
// straight to base[digit] + rank in the pass's output, and base[digit] then moves on by the tile's count.
template <int PAIRS, int RANK>
__global__ __launch_bounds__(1024) void rs_seg_tiles(SegSortArgs a) {
    constexpr int THREADS = 1024, W = THREADS / kWave, KPT = 8;
    constexpr uint32_t SPAN = kWave * KPT, TILE = THREADS * KPT;
    __shared__ uint32_t s_cnt[W * 256];
    __shared__ uint32_t s_base[4 * 256];  // [pass][digit]: where the digit's next key goes, from the segment's start
    __shared__ uint32_t s_ws[W];
    const uint32_t t = threadIdx.x, w = t / kWave, lane = lane_id();
    const uint32_t nseg = *a.count;
    uint32_t order_bad = 0;
    for (uint32_t b = blockIdx.x; b < nseg; b += gridDim.x) {
        const uint32_t sg = a.list[b];
        const uint32_t s = a.off[sg], n = a.off[sg + 1] - s;  // (classified: s + n <= a.n)
        // all four digit histograms from one read of the segment, scanned into the passes' digit bases
        s_base[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += THREADS) {
            const uint32_t k = a.kin[s + i];
#pragma unroll
            for (int p = 0; p < 4; ++p) count_add(&s_base[p * 256], (k >> (8 * p)) & 255u);
        }
        __syncthreads();
        {
            // one scan over the 4 x 256 counts; pass p's own start is p * n (every histogram holds n keys)
            uint32_t all;
            const uint32_t ex = block_excl_scan<THREADS>(s_base[t], s_ws, all);
            s_base[t] = ex - (t >> 8) * n;
        }
        __syncthreads();
        for (int pass = 0; pass < 4; ++pass) {
            const uint32_t sh = pass * 8;
            // in -> tmp -> out -> tmp -> out, all at the segment's own offsets
            const uint32_t *ksrc = pass == 0 ? a.kin : (pass & 1) ? a.ktmp : a.kout;
            uint32_t *kdst = (pass & 1) ? a.kout : a.ktmp;
            const uint32_t *vsrc = pass == 0 ? a.vin : (pass & 1) ? a.vtmp : a.vout;
            uint32_t *vdst = (pass & 1) ? a.vout : a.vtmp;
            uint32_t *gb = &s_base[pass * 256];
            uint32_t *row = &s_cnt[w * 256];
            for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
                const uint32_t nt = n - t0 < TILE ? n - t0 : TILE;
                const uint32_t i0 = w * SPAN + lane;
                uint32_t key[KPT], val[PAIRS ? KPT : 1], rk[KPT];
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    const uint32_t i = i0 + j * kWave;
                    key[j] = i < nt ? ksrc[s + t0 + i] : kPadKey;
                    if constexpr (PAIRS) val[j] = i < nt ? vsrc[s + t0 + i] : 0u;
                }
                for (uint32_t i = lane; i < 256; i += kWave) row[i] = 0;
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    rk[j] = 0;
                    if (w * SPAN + j * kWave < nt) {  // (wave-uniform; pads only in the segment's last slot)
                        const uint32_t d = (key[j] >> sh) & 255u;
                        rk[j] = slot_rank<8, RANK>(row, d);
                        if constexpr (RANK == kRankAtomic) {
                            if (j == 0 && w * SPAN + kWave <= nt) order_bad |= rank_check<8>(d, rk[j], a.rank_fault);
                        }
                    }
                }
                __syncthreads();
                if (t < 256) {
                    uint32_t run = gb[t];
#pragma unroll
                    for (int x = 0; x < W; ++x) {
                        const uint32_t c = s_cnt[x * 256 + t];
                        s_cnt[x * 256 + t] = run;
                        run += c;
                    }
                    gb[t] = run;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    if (i0 + j * kWave < nt) {
                        const uint32_t p = row[(key[j] >> sh) & 255u] + rk[j];  // (< n: a real key's rank)
                        kdst[s + p] = key[j];
                        if constexpr (PAIRS) vdst[s + p] = val[j];
                    }
                }
                // (the next tile's waves touch only their own counter row until the next barrier)
            }
            // The next pass re-reads what this workgroup wrote, and nobody else reads or writes these
            // words: the barrier's workgroup-scope release / acquire is enough (one CU, one L1), no
            // agent-scope fence.
            __syncthreads();
        }
    }
    if constexpr (RANK == kRankAtomic) report_order(a.check, order_bad);
}

template <int PAIRS, int RANK>
const void *seg_kernel_of(int kind) {
    switch (kind) {
        case kSegWave: return (const void *)rs_seg_wave<PAIRS, RANK>;
        case kSegSmall: return (const void *)rs_seg_lds<kSegSmallThreads, kSegSmallKpt, PAIRS, RANK>;
        case kSegLds: return (const void *)rs_seg_lds<kSegLdsThreads, kSegLdsKpt, PAIRS, RANK>;
        default: return (const void *)rs_seg_tiles<PAIRS, RANK>;
    }
}

const void *seg_kernel(int kind, int pairs, int rank) {
    const bool at = rank == kRankAtomic;
    if (pairs) return at ? seg_kernel_of<1, kRankAtomic>(kind) : seg_kernel_of<1, kRankCount>(kind);
    return at ? seg_kernel_of<0, kRankAtomic>(kind) : seg_kernel_of<0, kRankCount>(kind);
}

int seg_threads(int kind) { return kind == kSegWave || kind == kSegSmall ? 256 : 1024; }

bool seg_args_ok(int kind, int rank) {
    return kind >= 0 && kind < kSegKinds && (rank == kRankAtomic || rank == kRankCount);
}

}  // namespace

hipError_t launch_seg_classify(const SegClassifyArgs &a, hipStream_t s) {
    if (a.num_segments == 0) return hipSuccess;
    const uint32_t grid = (a.num_segments + 255u) / 256u;
    hipLaunchKernelGGL(rs_seg_classify, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_seg_sort(int kind, int pairs, int rank_algo, const SegSortArgs &a, uint32_t grid, hipStream_t s) {
    if (!seg_args_ok(kind, rank_algo)) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    const void *fn = seg_kernel(kind, pairs ? 1 : 0, rank_algo);
    SegSortArgs args = a;
    void *params[] = {&args};
    return hipLaunchKernel(fn, dim3(grid), dim3(seg_threads(kind)), params, 0, s);
}

int seg_blocks_per_cu(int kind, int pairs, int rank_algo) {
    if (!seg_args_ok(kind, rank_algo)) return 0;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_kernel(kind, pairs ? 1 : 0, rank_algo),
                                                     seg_threads(kind), 0) != hipSuccess)
        return 0;
    return nb;
}

}  // namespace rsort

// rsort_hybrid.hip -- the hybrid route of keys-only k = 8 sorts of about 2^29..2^30 keys (sort_planned,
// rsort_capi.cpp): two MSD passes + an in-LDS finish, three 8-B/key passes over the keys instead of four.
//
//   rs_hyb_gate      64 workgroups, before any histogram: each reads 1024 keys at a fixed stride over its 64th of
//                    the input and counts their top-16-bit buckets in LDS; a bucket with `threshold` of a
//                    workgroup's keys (a share no uniform sample reaches, gate_threshold in rsort_capi.cpp) says
//                    "skewed" and the sort takes the LSD passes with no extra key read
//   (rs_histogram)   the JOINT mode at shift 24 with the second digit at shift 16: the per-chunk digit-3 table
//                    of pass A and the joint counts J[digit 2][digit 3] = the 65536 bucket sizes
//   rs_hyb_bounds    one workgroup: the largest bucket, the mode word (hybrid when it fits kHybCapacity, else
//                    LSD: the sort has then paid one extra histogram read), the digit-3 groups' starts = pass B's
//                    chunks, and J scanned IN PLACE in (digit 3, digit 2) order: J[e][g] becomes the start of
//                    bucket (g, e), which is both the table pass B reads ([digit][chunk]: chunk = digit-3 group,
//                    digit = digit 2) and the bucket starts of the last phase
//   (rs_scatter_lines) pass A: shift 24, fixed chunks; pass B: shift 16 over the digit-3 groups
//   rs_bucket_sort16 one workgroup per bucket (grid-stride): the bucket's keys share their top 16 bits and are
//                    sorted by the low 16 in two 8-bit counting passes inside LDS (the product form of
//                    dev/msd_lab.hip's bucket_sort16, grown from rs_seg_lds: padded whole-wave slots, lane-
//                    ordered ranks with the per-wave rank check), one read and one write of the keys; only the
//                    low halves are kept (packed registers, a 16-bit LDS tile), two workgroups resident per CU
//
// Every kernel of both routes tests the mode word (done[kHybMode]) and leaves at once when the other route
// runs: no host synchronisation picks the route.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "rsort_device.hpp"
#include "rsort_hooks.hpp"
#include "rsort_internal.hpp"

namespace rsort {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------ sample gate
// kHybGateGroups workgroups, each over one contiguous part of the input: its 1024 threads read one key each at a
// fixed stride over that part and count the keys' top-16-bit buckets in 2^16 16-bit LDS counters (two per word,
// 128 KB). The returning add tells each thread its bucket's count: the one that takes a bucket to `threshold`
// raises the flag word (zeroed with the joint counts before this launch; every writer writes 1). One workgroup
// reading all 65536 keys took 123 us -- 64 dependent rounds of loads 64 KB apart from one CU; 64 workgroups with
// one load per thread take a few. rs_hyb_bounds, the next single-workgroup kernel, turns the flag into the verdict.
__global__ __launch_bounds__(1024) void rs_hyb_gate(HybArgs a) {
    constexpr uint32_t T = 1024;
    __shared__ uint32_t s_c[kHybBuckets / 2];
    const uint32_t t = threadIdx.x;
    const uint64_t m = a.n < (uint64_t)kHybSample ? a.n : (uint64_t)kHybSample;
    const uint64_t stride = m ? a.n / m : 1;  // (sample i is key i * stride < n)
    const uint64_t i = (uint64_t)blockIdx.x * T + t;
    const uint32_t k = i < m ? __builtin_nontemporal_load(a.kin + i * stride) : 0u;
    for (uint32_t x = t; x < kHybBuckets / 2; x += T) s_c[x] = 0u;
    __syncthreads();
    if (i < m) {
        const uint32_t bk = k >> 16, sh = (bk & 1u) << 4;
        const uint32_t before = (atomicAdd(&s_c[bk >> 1], 1u << sh) >> sh) & 0xFFFFu;
        if (before + 1u >= a.threshold) a.joint[kHybGateFlag] = 1u;
    }
}

// ------------------------------------------------------------------------------ exact count -> mode, starts
// Thread (q, g) owns J[64 q .. 64 q + 63][g] (digit-2 values of digit-3 group g), read 16 at a time: once for
// the group totals and the largest bucket, then -- after the totals' scan, the groups' starts -- again for each
// column's running prefix, written back over J (all 64 in registers spilled under the 128-VGPR limit of 1024
// threads: every load 4 KB apart needs its own address).
__global__ __launch_bounds__(1024) void rs_hyb_bounds(HybArgs a) {
    constexpr uint32_t R = kJointBins, Q = 1024 / R, EP = R / Q;
    __shared__ uint32_t s_part[Q][R];
    __shared__ uint32_t s_start[R];
    __shared__ uint32_t s_ws[1024 / kWave];
    __shared__ uint32_t s_max;
    const uint32_t t = threadIdx.x;
    // the first single-workgroup launch of an eligible sort: a clean record (pass 0's histogram writes it for the
    // others) and the gate's verdict
    const bool skew = a.joint[kHybGateFlag] != 0u;
    if (t == 0) {
        a.done[0] = 0u;
        a.done[kDoneErr] = 0u;
        a.done[kHybGate] = skew ? kGateSkewed : kGatePass;
        a.done[kHybEligible] = 1u;
    }
    if (skew && !a.force) {  // (the joint count did not run: J is still clear for the LSD passes)
        if (t == 0) {
            a.done[kHybMode] = kHybLsd;
            a.done[kHybMax] = 0u;
        }
        return;
    }
    const uint32_t g = t % R, q = t / R;
    constexpr uint32_t B = 16;
    uint32_t *col = a.joint + (q * EP) * R + g;
    uint32_t sum = 0, mx = 0;
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < EP; i0 += B) {
        uint32_t v[B];
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) v[i] = col[(i0 + i) * R];
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) {
            sum += v[i];
            mx = max(mx, v[i]);
        }
    }
    s_part[q][g] = sum;
    if (t == 0) s_max = 0u;
    __syncthreads();
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    if (lane_id() == 0) atomicMax(&s_max, mx);
    uint32_t tot = 0;
    if (t < R) {
#pragma unroll
        for (uint32_t i = 0; i < Q; ++i) tot += s_part[i][t];
    }
    uint32_t total = 0;
    const uint32_t start = block_excl_scan<1024>(tot, s_ws, total);  // (its barriers: s_max is final after it)
    const uint32_t big = s_max;
    if ((uint64_t)total != a.n || big > kHybCapacity) {
        // LSD after all: its pass 0 adds its own joint counts into a cleared J
#pragma unroll 4
        for (uint32_t i = 0; i < EP; ++i) col[i * R] = 0u;
        if (t == 0) {
            a.done[kHybMode] = kHybLsd;
            a.done[kHybMax] = big;
        }
        return;
    }
    if (t < R) {
        s_start[t] = start;
        a.bounds[1 + t] = start;
    }
    if (t == 0) {
        a.bounds[0] = kGroupsWhole;
        a.bounds[1 + R] = total;
    }
    __syncthreads();
    uint32_t run = s_start[g];
    for (uint32_t i = 0; i < q; ++i) run += s_part[i][g];
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < EP; i0 += B) {
        uint32_t v[B];
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) v[i] = col[(i0 + i) * R];
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) {
            col[(i0 + i) * R] = run;
            run += v[i];
        }
    }
    // rsort_cut_plan_stats: this route makes no cut plan (rs_joint_bounds stores these words on every other route;
    // a workspace's content on entry is arbitrary -- tests/test_gpu_workspace_state.py, the hybrid_run case)
    if (t < 4) {
        a.gflags[kBoundsStat + t] = 0u;
        a.gflags[kBoundsWords + kBoundsStat + t] = 0u;
    }
    if (t == 0) {
        a.done[kHybMode] = kHybRun;
        a.done[kHybMax] = big;
        // rsort_group_flags: the second pass ran on digit groups, there is no fourth
        a.gflags[0] = kGroupsWhole;
        a.gflags[kBoundsWords] = kGroupsFixed;
    }
}

// ------------------------------------------------------------------------------ bucket phase
// A wave-uniform value the compiler may not trace back: the tests `j < slots` of each unrolled loop are then a
// scalar compare and branch where they stand. Without it the 18 results are computed once per bucket and kept as
// 64-bit lane masks over all loops (36 SGPRs, which spilled).
__device__ __forceinline__ uint32_t fresh_scalar(uint32_t x) {
    x = __builtin_amdgcn_readfirstlane(x);  // (folded away where x is in an SGPR already)
    asm volatile("" : "+s"(x));
    return x;
}
// The same for a per-lane value: addresses made of it are computed where they are used, not once before the
// bucket loop and held in registers through it.
__device__ __forceinline__ uint32_t fresh_vector(uint32_t x) {
    asm volatile("" : "+v"(x));
    return x;
}

// Bucket b = (digit 3, digit 2) = (b >> 8, b & 255) is keys [start(b), start(b + 1)) of pass B's output.
// Wave w holds keys [w * span, (w + 1) * span) of the bucket, slot j its keys w * span + 64 j + lane (span: the
// bucket's share per wave in whole slots), the missing keys of the last slot being pads that every pass ranks
// last (rsort_segmented.hip, "Partial slots"): every ranked slot is a whole wave.
//
// All keys of a bucket share their top 16 bits = b, so only the low halves are kept: slots 2 i and 2 i + 1 of a
// thread in the two halves of one register (KPT / 2 registers), their ranks (below 64 KPT per wave) packed the
// same way, and the tile the passes stage into holds 16-bit entries (36 KiB for 18432 keys). The output widens
// each entry with b << 16 again. A key that pass A or B had put into the wrong bucket would so come out as
// another key: every loaded key's top half is compared with b (kCheckTable in the check word). Pads are 0xFFFF;
// they sit in the bucket's last slot, so a real key ending in 0xFFFF ranks before them in both passes.
//
// With 64 VGPRs and 53 KiB of LDS two 1024-thread workgroups are resident per CU (kHybResident; tested through
// rsort_hybrid_kernel_info): one ranks while the other waits for its loads or at a barrier. Barriers per
// counting pass: ranks -> column prefix (the first 256 threads, 16 counts each held in registers over the next
// one) -> s_ws -> rows written -> staged; the read-back of pass 0 and the output need none of their own (the
// next write of the tile comes three barriers later).
template <int THREADS, int KPT>
__global__ __launch_bounds__(THREADS, kHybResident *THREADS / 256) void rs_bucket_sort16(HybArgs a) {
    constexpr int W = THREADS / kWave, KP = KPT / 2, SW = 256 / kWave;
    constexpr uint32_t CAP = THREADS * KPT;
    static_assert(CAP == kHybCapacity && CAP % kWave == 0, "the capacity the exact count checks");
    static_assert(KPT % 2 == 0 && KPT * kWave <= 65536 && CAP <= 65536, "ranks and positions in 16 bits");
    static_assert(THREADS >= 256, "one thread per digit in the column prefix");
    __shared__ __attribute__((aligned(16))) uint16_t s_k[CAP + 8];
    __shared__ uint32_t s_cnt[W * 256];
    __shared__ uint32_t s_ws[SW];
    if (a.done[kHybMode] != kHybRun) return;
    RS_HYB_STAMP_DECL
    const uint32_t t = threadIdx.x, lane = lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane(t / kWave);  // (a scalar: the slot tests stay on the SALU)
    uint32_t *row = &s_cnt[w * 256];
    uint32_t order_bad = 0, table_bad = 0;
    for (uint32_t b = blockIdx.x; b < kHybBuckets; b += gridDim.x) {
        // the bucket's start and size (a bucket above the capacity -- the exact count rules it out -- is skipped
        // and recorded, never staged)
        const uint32_t s = a.joint[(b & 255u) * kJointBins + (b >> 8)];
        const uint32_t b1 = b + 1u;
        const uint32_t e = b1 < kHybBuckets ? a.joint[(b1 & 255u) * kJointBins + (b1 >> 8)] : (uint32_t)a.n;
        uint32_t n = e - s;
        if (e < s || n > CAP || (uint64_t)e > a.n) {
            table_bad = 1u;
            n = 0u;
        }
        const uint32_t span = ((((n + 63u) / 64u) + W - 1) / W) * 64u, base = w * span;
        // slots of this wave that hold a key (the last may hold pads too), and whether its first is full
        const uint32_t slots0 = base < n ? (min(span, n - base) + 63u) / 64u : 0u;
        const bool full0 = base + kWave <= n;
        const uint32_t hi = b << 16;
        uint32_t key[KP];
        {
            // (every load of a live slot is in bounds: the lanes past n of the bucket's last slot read its last key)
            const uint32_t left = base < n ? n - base : 0u;  // keys from this wave's first on
            const uint32_t *in = a.kin + s + base;
            const uint32_t slots = fresh_scalar(slots0), ll = fresh_vector(lane);
            uint32_t diff = 0;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                uint32_t k[2] = {hi | 0xFFFFu, hi | 0xFFFFu};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t j = 2 * i + h, x = j * kWave + ll;
                    if (j < slots) {
                        const uint32_t v = __builtin_nontemporal_load(in + min(x, left - 1u));
                        k[h] = x < left ? v : k[h];
                    }
                    diff |= k[h] ^ hi;
                }
                key[i] = (k[0] & 0xFFFFu) | (k[1] << 16);
            }
            table_bad |= diff >> 16;
            asm volatile("" : "+v"(table_bad));  // (here, or the 18 loaded words stay live to the end of the bucket)
        }
        RS_HYB_STAMP_LOADED(0);
        // s_k[ak + i] holds key i: quads of s_k (8 B) are then 16-B aligned in kout (any 4-B-aligned base)
        const uint32_t ak = (uint32_t)(((uintptr_t)(a.kout + s) >> 2) & 3u);
        uint16_t *tile = s_k + ak;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t sh = pass * 8;
            for (uint32_t i = lane; i < 256; i += kWave) row[i] = 0;
            uint32_t rk[KP];
            uint32_t slots = fresh_scalar(slots0);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                rk[i] = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t j = 2 * i + h;
                    if (j < slots) {  // (wave-uniform: the slot holds a key; its lanes past n hold pads)
                        const uint32_t d = (key[i] >> (16 * h + sh)) & 255u;
                        uint32_t r = rank_add(row, d);
                        if (j == 0 && full0) order_bad |= rank_check<8>(d, r, a.rank_fault);
                        rk[i] |= r << (16 * h);
                    }
                }
            }
            __syncthreads();
            // per digit: the waves' counts become their exclusive prefix over the waves plus the digit's start
            uint32_t c[W], tot = 0;
            if (t < 256) {
#pragma unroll
                for (int x = 0; x < W; ++x) {
                    c[x] = s_cnt[x * 256 + t];
                    tot += c[x];
                }
                const uint32_t inc = wave_incl_scan(tot);
                if (lane == kWave - 1) s_ws[w] = inc;
                tot = inc - tot;
            }
            __syncthreads();
            if (t < 256) {
#pragma unroll
                for (int x = 0; x < SW; ++x) tot += (uint32_t)x < w ? s_ws[x] : 0u;
#pragma unroll
                for (int x = 0; x < W; ++x) {
                    s_cnt[x * 256 + t] = tot;
                    tot += c[x];
                }
            }
            __syncthreads();
            slots = fresh_scalar(slots0);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t j = 2 * i + h;
                    if (j < slots) {
                        const uint32_t kh = key[i] >> (16 * h);
                        const uint32_t p = row[(kh >> sh) & 255u] + ((rk[i] >> (16 * h)) & 0xFFFFu);  // (< roundup(n, 64))
                        tile[p] = (uint16_t)kh;
                    }
                }
            }
            __syncthreads();
            if (pass == 0) {
                // pass 1 ranks pass 0's output in position order (its stability is what sorts the bucket)
                const uint16_t *mine = tile + base + lane;
                slots = fresh_scalar(slots0);
#pragma unroll
                for (int i = 0; i < KP; ++i) {
                    uint32_t lo = 0xFFFFu, up = 0xFFFFu;
                    if ((uint32_t)(2 * i) < slots) lo = mine[(2 * i) * kWave];
                    if ((uint32_t)(2 * i + 1) < slots) up = mine[(2 * i + 1) * kWave];
                    key[i] = lo | (up << 16);
                }
            }
            RS_HYB_STAMP(1 + pass);
        }
        // out[s - ak + 4 q .. + 3] = b << 16 | s_k[4 q .. + 3]: whole quads inside the bucket as 16-B stores,
        // the words at its two ends one by one
        {
            uint32_t *o = a.kout + s - ak;
            const uint32_t nq = (ak + n + 3u) / 4u;
            for (uint32_t q = fresh_vector(t); q < nq; q += THREADS) {
                const uint2 h2 = *reinterpret_cast<const uint2 *>(&s_k[4 * q]);
                const u32x4 v = {hi | (h2.x & 0xFFFFu), hi | (h2.x >> 16), hi | (h2.y & 0xFFFFu), hi | (h2.y >> 16)};
                if (4 * q >= ak && 4 * q + 4 <= ak + n) {
                    hooks::store_quad_nt(o + 4 * q, v);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        if (4 * q + i >= ak && 4 * q + i < ak + n) hooks::store_word(o + 4 * q + i, v[i]);
                }
            }
        }
        RS_HYB_STAMP(3);
        RS_HYB_STAMP_BUCKET();
    }
    RS_HYB_STAMP_FLUSH();
    if (a.done != nullptr && __ballot(table_bad != 0u) != 0ull && lane == 0) atomicOr(a.done + kDoneErr, kCheckTable);
    report_order(a.done + kDoneErr, order_bad);
}

const void *bucket_kernel() { return (const void *)rs_bucket_sort16<kHybThreads, kHybKpt>; }

}  // namespace

hipError_t launch_hyb_gate(const HybArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(rs_hyb_gate, dim3(kHybGateGroups), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_hyb_bounds(const HybArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(rs_hyb_bounds, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_hyb_bucket(const HybArgs &a, uint32_t grid, hipStream_t s) {
    if (grid == 0) return hipErrorInvalidValue;
    const void *fn = bucket_kernel();
    HybArgs args = a;
    void *params[] = {&args};
    return hipLaunchKernel(fn, dim3(grid), dim3(kHybThreads), params, 0, s);
}

void hyb_note_bucket() {
    char name[48];
    snprintf(name, sizeof(name), "rs_bucket_sort16<%d, %d>", kHybThreads, kHybKpt);
    note_kernel_used(bucket_kernel(), name);
}

int hyb_blocks_per_cu() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bucket_kernel(), kHybThreads, 0) != hipSuccess) return 0;
    return nb;
}

hipError_t hyb_kernel_info(int info[4]) {
    hipFuncAttributes fa{};
    const hipError_t e = hipFuncGetAttributes(&fa, bucket_kernel());
    if (e != hipSuccess) return e;
    info[0] = kHybThreads;
    info[1] = (int)fa.sharedSizeBytes;
    info[2] = (int)fa.localSizeBytes;
    info[3] = hyb_blocks_per_cu();
    return hipSuccess;
}

}  // namespace rsort

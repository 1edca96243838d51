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
//                    ordered ranks with the per-wave rank check), one read and one write of the keys
//
// Every kernel of both routes tests the mode word (done[kHybMode]) and leaves at once when the other route
// runs: no host synchronisation picks the route.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsort_device.hpp"
#include "rsort_hooks.hpp"
#include "rsort_internal.hpp"

namespace rsort {

namespace {

constexpr uint32_t kPadKey = 0xFFFFFFFFu;
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
    if (t == 0) {
        a.done[kHybMode] = kHybRun;
        a.done[kHybMax] = big;
        // rsort_group_flags: the second pass ran on digit groups, there is no fourth
        a.gflags[0] = kGroupsWhole;
        a.gflags[kBoundsWords] = kGroupsFixed;
    }
}

// ------------------------------------------------------------------------------ bucket phase
// Bucket b = (digit 3, digit 2) = (b >> 8, b & 255) is keys [start(b), start(b + 1)) of pass B's output.
// Wave w holds keys [w * span, (w + 1) * span) of the bucket, slot j its keys w * span + 64 j + lane (span: the
// bucket's share per wave in whole slots), the missing keys of the last slot being 0xFFFFFFFF pads that every
// pass ranks last (rsort_segmented.hip, "Partial slots"): every ranked slot is a whole wave.
// (Measured and not kept, dev/LOG.md: loading the next bucket's keys into the dead key registers while this one
// is stored -- no gain, the phase waits on its LDS passes and barriers, not on HBM.)
template <int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void rs_bucket_sort16(HybArgs a) {
    constexpr int W = THREADS / kWave;
    constexpr uint32_t CAP = THREADS * KPT;
    static_assert(CAP == kHybCapacity && CAP % kWave == 0, "the capacity the exact count checks");
    __shared__ __attribute__((aligned(16))) uint32_t s_k[CAP + 4];
    __shared__ uint32_t s_cnt[W * 256];
    __shared__ uint32_t s_ws[W];
    if (a.done[kHybMode] != kHybRun) return;
    const uint32_t t = threadIdx.x, w = t / kWave, lane = lane_id();
    uint32_t *row = &s_cnt[w * 256];
    uint32_t order_bad = 0, size_bad = 0;
    // bucket b's start and size (0 past the last bucket; a bucket above the capacity -- the exact count rules
    // it out -- is skipped and recorded, never staged)
    auto bucket = [&](uint32_t b, uint32_t &s, uint32_t &n) {
        s = 0u;
        n = 0u;
        if (b >= kHybBuckets) return;
        s = a.joint[(b & 255u) * kJointBins + (b >> 8)];
        const uint32_t b1 = b + 1u;
        const uint32_t e = b1 < kHybBuckets ? a.joint[(b1 & 255u) * kJointBins + (b1 >> 8)] : (uint32_t)a.n;
        n = e - s;
        if (e < s || n > CAP || (uint64_t)e > a.n) {
            size_bad = 1u;
            n = 0u;
        }
    };
    auto span_of = [&](uint32_t n) { return ((((n + 63u) / 64u) + W - 1) / W) * 64u; };
    uint32_t key[KPT];
    auto load = [&](uint32_t s, uint32_t n) {
        const uint32_t span = span_of(n), i0 = w * span + lane;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t i = i0 + j * kWave;
            const bool in = (uint32_t)(j * kWave) < span && i < n;
            key[j] = in ? __builtin_nontemporal_load(a.kin + s + i) : kPadKey;
        }
    };
    for (uint32_t b = blockIdx.x; b < kHybBuckets; b += gridDim.x) {
        uint32_t s, n;
        bucket(b, s, n);
        load(s, n);
        const uint32_t span = span_of(n), i0 = w * span + lane;
        // s_k[ak + i] holds key i: quads of s_k are then 16-B aligned in kout (any 4-B-aligned base)
        const uint32_t ak = (uint32_t)(((uintptr_t)(a.kout + s) >> 2) & 3u);
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t sh = pass * 8;
            for (uint32_t i = lane; i < 256; i += kWave) row[i] = 0;
            uint32_t rk[KPT];
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                rk[j] = 0;
                // (wave-uniform: the slot holds a key; its lanes past n hold pads)
                if ((uint32_t)(j * kWave) < span && w * span + j * kWave < n) {
                    const uint32_t d = (key[j] >> sh) & 255u;
                    rk[j] = rank_add(row, d);
                    if (j == 0 && w * span + kWave <= n) order_bad |= rank_check<8>(d, rk[j], a.rank_fault);
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
                    const uint32_t p = row[(key[j] >> sh) & 255u] + rk[j];  // (< roundup(n, 64) <= CAP)
                    s_k[ak + p] = key[j];
                }
            }
            if (pass == 0) {
                __syncthreads();
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    if ((uint32_t)(j * kWave) < span && w * span + j * kWave < n) key[j] = s_k[ak + i0 + j * kWave];
                }
            }
            __syncthreads();
        }
        // out[s - ak + 4 q .. + 3] = s_k[4 q .. + 3]: whole quads inside the bucket as 16-B stores, the words at
        // its two ends one by one
        {
            uint32_t *o = a.kout + s - ak;
            const uint32_t nq = (ak + n + 3u) / 4u;
            for (uint32_t q = t; q < nq; q += THREADS) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(&s_k[4 * q]);
                if (4 * q >= ak && 4 * q + 4 <= ak + n) {
                    hooks::store_quad_nt(o + 4 * q, v);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        if (4 * q + i >= ak && 4 * q + i < ak + n) hooks::store_word(o + 4 * q + i, v[i]);
                }
            }
        }
        __syncthreads();
    }
    if (a.done != nullptr && __ballot(size_bad != 0u) != 0ull && lane == 0) atomicOr(a.done + kDoneErr, kCheckTable);
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
    note_kernel_used(bucket_kernel(), "rs_bucket_sort16<1024, 18>");
}

int hyb_blocks_per_cu() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bucket_kernel(), kHybThreads, 0) != hipSuccess) return 0;
    return nb;
}

}  // namespace rsort

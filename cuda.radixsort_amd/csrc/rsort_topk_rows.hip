// rsort_topk_rows.hip -- the select kernels of rsort_u32_topk_rows_device (include/rsort.h, "row-wise top-k"): the
// k smallest or largest keys of every row of a rows x cols matrix, one radix select per row.
//
// cols is one number for the whole call, so the host picks the kernel (rsort_internal.hpp, TopkRowsClass) and there
// is no classification and there are no lists:
//   tr_select<wave>   cols <= 256: one WAVE per row, four rows per 256-thread workgroup, no workgroup barrier
//   tr_select<small>  cols <= 1024: one 256-thread workgroup per row, 4 keys per lane
//   tr_select<lds>    cols <= 16384: one 1024-thread workgroup per row, 16 keys per lane
//   tr_stream         longer rows: one 1024-thread workgroup walks the row from global memory, once per level and
//                     once more to emit. One CU selects from the whole row: the correctness net.
// tr_select reads a row once. Its keys stay in registers as x = key ^ m in the segmented sort's wave-striped order
// (wave w holds entries [w * span, (w + 1) * span), slot j of it entries w * span + 64 j + lane), so (wave, slot,
// lane) order is column order. An entry past cols takes part in nothing -- no count, no ballot bit, no write: there
// is no pad value, every test carries the entry's own validity.
//
// Select: four 8-bit levels from the top. The candidates (entries whose upper bits equal the digits chosen so far)
// add their digit into 256 LDS counters (count_add), one wave scans them four to a lane and picks the digit that
// holds the want-th candidate and what is wanted from inside it. After the last level the k-th x, T, is known and
// k_rem of the entries equal to it are to be taken; a level whose picked digit holds exactly what is wanted ends
// the select early (T is then the chosen digits, and entries are compared by those bits alone). (A bit-by-bit select
// from registers alone -- one ballot and one scalar popcount per bit and slot, no counters -- was built for the wave
// kernel and measured 6.5x slower at 2^20 x 64: DESIGN §5c, profiles/topk_rows_wave_select.json.)
// Emit: an entry is taken when x < T, or x == T and fewer than k_rem entries equal to T precede it in its row. Its
// place among the row's k outputs is (entries < T before it) + min(entries == T before it, k_rem): the survivors
// land in column order. Both counts come from ballots in column order, the waves' running counts and, across the
// waves of a row, their prefix through LDS. Every position is compared with k before it is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rsort.h"
#include "rsort_device.hpp"
#include "rsort_internal.hpp"

namespace rsort {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t below_in(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One whole wave over a level's 256 counts (16-B aligned, lane l owns digits 4 l .. 4 l + 3): the digit that holds
// the want-th candidate (1 <= want <= the counts' sum), what is wanted from inside it, and its count.
// Wave-uniform results. A want beyond the sum (never, by the contract) picks lane 0's: the emit bounds every write.
__device__ __forceinline__ void tr_pick(const uint32_t *row, uint32_t want, uint32_t &digit, uint32_t &rem,
                                        uint32_t &count) {
    const uint32_t lane = lane_id();
    const u32x4 c = *reinterpret_cast<const u32x4 *>(&row[4 * lane]);
    const uint32_t sum = c[0] + c[1] + c[2] + c[3];
    const uint32_t inc = wave_incl_scan(sum), ex = inc - sum;
    const uint64_t mm = __ballot(ex < want && want <= inc);
    const uint32_t src = mm != 0ull ? (uint32_t)__builtin_ctzll(mm) : 0u;
    uint32_t d = 0, r = want - ex, n = c[0];
    if (r > c[0]) {
        r -= c[0], d = 1, n = c[1];
        if (r > c[1]) {
            r -= c[1], d = 2, n = c[2];
            if (r > c[2]) r -= c[2], d = 3, n = c[3];
        }
    }
    digit = __builtin_amdgcn_readlane(4 * lane + d, src);
    rem = __builtin_amdgcn_readlane(r, src);
    count = __builtin_amdgcn_readlane(n, src);
}

// The waves' counts s[0 .. W) (one per wave of the row, in column order) -> the sum before wave `wave` (wave-uniform,
// a scalar) and the total: W lanes scan them, no per-wave compare (whose W lane masks would stay alive in SGPRs).
template <int W>
__device__ __forceinline__ void waves_prefix(const uint32_t *s, uint32_t wave, uint32_t &before, uint32_t &total) {
    const uint32_t lane = lane_id();
    const uint32_t inc = wave_incl_scan(lane < (uint32_t)W ? s[lane] : 0u);
    total = __builtin_amdgcn_readlane(inc, kWave - 1);
    before = wave != 0u ? __builtin_amdgcn_readlane(inc, wave - 1u) : 0u;
}

// What a row's select leaves: report word kTrBadRows counts the rows whose emit did not write exactly k entries.
__device__ __forceinline__ void tr_stamp(const TopkRowsArgs &a, uint32_t cls) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.state[kTrClass] = cls;
        a.state[kTrSorted] = a.raw ? 0u : 1u;
    }
}

// WPR waves share a row: 1 (the wave kernel: THREADS / 64 rows per workgroup at a time) or all of the workgroup's.
template <int CLS, int THREADS, int KPT, int WPR>
__global__ __launch_bounds__(THREADS) void tr_select(TopkRowsArgs a) {
    constexpr int W = THREADS / kWave, RPW = W / WPR;
    static_assert(WPR == 1 || WPR == W, "a row is one wave's or the whole workgroup's");
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[RPW][256];
    __shared__ uint32_t s_pick[3];
    __shared__ uint32_t s_w0[W], s_w1[W];
    const uint32_t t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t / kWave), lane = lane_id();
    const uint32_t w = WPR == 1 ? 0u : wave;  // this wave's place in its row
    uint32_t *cnt = s_cnt[WPR == 1 ? wave : 0u];
    const uint32_t cols = a.cols, k = a.k;
    const uint32_t span = ((cols + 63u) / 64u + WPR - 1) / WPR * 64u;  // (<= 64 KPT: the class's limit)
    const uint32_t i0 = w * span + lane;
    // (one wave's LDS instructions complete in order: its barrier only keeps the compiler from moving them)
    auto sync = [] {
        if constexpr (WPR == 1) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            __syncthreads();
        }
    };
    // okm: bit j = slot j of this lane holds an entry of a row (the same for every row: cols is the call's). One
    // VGPR, made opaque before every phase: the compiler then tests it where it is used instead of keeping KPT lane
    // masks alive in SGPRs through the whole row loop. A slot without an entry loads its row's first key instead
    // of being predicated (so the loads need no lane masks either); nothing ever looks at its x.
    uint32_t okm = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const bool in = (uint32_t)(j * kWave) < span && i0 + j * kWave < cols;
        okm |= in ? 1u << j : 0u;
    }
    auto ok = [&](int j) { return ((okm >> j) & 1u) != 0u; };
    tr_stamp(a, (uint32_t)CLS);
    for (uint32_t r = blockIdx.x * RPW + (WPR == 1 ? wave : 0u); r < a.rows; r += gridDim.x * RPW) {
        const uint32_t *krow = a.kin + (size_t)r * cols;
        uint32_t x[KPT];
        asm volatile("" : "+v"(okm));
#pragma unroll
        for (int j = 0; j < KPT; ++j) x[j] = krow[ok(j) ? i0 + j * kWave : 0u] ^ a.m;
        // T: the digits chosen so far, the k-th x's bits above bit sh; entries are compared by those bits alone
        uint32_t T = 0, krem = k, sh = 0;
#pragma unroll
        for (int level = 0; level < 4; ++level) {
            sh = 24 - 8 * level;
            if constexpr (WPR == 1) *reinterpret_cast<u32x4 *>(&cnt[4 * lane]) = u32x4{0u, 0u, 0u, 0u};
            else if (t < 256) cnt[t] = 0;
            sync();
            asm volatile("" : "+v"(okm));
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const bool cand = ok(j) && (level == 0 || (x[j] >> ((sh + 8) & 31u)) == T);
                if (cand) count_add(cnt, (x[j] >> sh) & 255u);
            }
            sync();
            uint32_t d, rem, n;
            if constexpr (WPR == 1) {
                tr_pick(cnt, krem, d, rem, n);
            } else {
                if (wave == 0) {
                    tr_pick(cnt, krem, d, rem, n);
                    if (lane == 0) {
                        s_pick[0] = d;
                        s_pick[1] = rem;
                        s_pick[2] = n;
                    }
                }
                __syncthreads();
                d = s_pick[0];
                rem = s_pick[1];
                n = s_pick[2];
            }
            T = (T << 8) | d;
            krem = rem;
            // the picked digit holds exactly what is wanted: every entry with the chosen digits is taken,
            // whatever its lower bits (the same words for every lane of the row: all leave together)
            if (n == rem) break;
        }
        // the row's entries below T and equal to T: counted per lane and summed over the wave (no ballots here, so
        // none stays alive for the ranking below), then ranked in column order
        uint32_t cl = 0, ce = 0;
        asm volatile("" : "+v"(okm));
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            cl += (ok(j) && (x[j] >> sh) < T) ? 1u : 0u;
            ce += (ok(j) && (x[j] >> sh) == T) ? 1u : 0u;
        }
        const uint32_t n0 = __builtin_amdgcn_readlane(wave_incl_scan(cl), kWave - 1);
        const uint32_t n1 = __builtin_amdgcn_readlane(wave_incl_scan(ce), kWave - 1);
        uint32_t r0 = 0, r1 = 0, t0 = n0, t1 = n1;
        if constexpr (WPR > 1) {
            if (lane == 0) {
                s_w0[wave] = n0;
                s_w1[wave] = n1;
            }
            __syncthreads();  // (s_w0 / s_w1 are next written after the next row's select barriers)
            waves_prefix<W>(s_w0, wave, r0, t0);
            waves_prefix<W>(s_w1, wave, r1, t1);
        }
        uint32_t *ko = a.kout + (size_t)r * k;
        uint32_t *vo = a.pairs ? a.vout + (size_t)r * k : nullptr;
        const uint32_t *vrow = a.pairs == kTrValues ? a.vin + (size_t)r * cols : nullptr;
        uint32_t ns = span / kWave, Te = T;  // (Te: the compares above are not kept for this loop, KPT masks each)
        asm volatile("" : "+v"(okm), "+s"(ns), "+v"(Te));
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if ((uint32_t)j < ns) {
                const bool lt = ok(j) && (x[j] >> sh) < Te, eq = ok(j) && (x[j] >> sh) == Te;
                const uint64_t m0 = __ballot(lt), m1 = __ballot(eq);
                const uint32_t b0 = r0 + below_in(m0), b1 = r1 + below_in(m1);
                const uint32_t pos = b0 + min(b1, krem);
                if ((lt || (eq && b1 < krem)) && pos < k) {
                    const uint32_t i = i0 + j * kWave;
                    ko[pos] = a.raw ? x[j] ^ a.m : x[j];
                    if (a.pairs) vo[pos] = a.pairs == kTrIndices ? i : vrow[i];
                }
                r0 += wave_count(m0);
                r1 += wave_count(m1);
            }
        }
        if (t0 + min(t1, krem) != k && lane == 0 && w == 0) atomicAdd(&a.state[kTrBadRows], 1u);
    }
}

// Rows longer than the LDS class: tiles of 1024 x 4 entries, wave w holding entries [256 w, 256 w + 256) of the
// tile. Only the input is read again, which nothing writes: no fence. A level whose picked digit holds exactly
// what is wanted stops the select: every entry with the chosen digits is taken, whatever its lower bits (`sh`).
__global__ __launch_bounds__(1024) void tr_stream(TopkRowsArgs a) {
    constexpr int THREADS = 1024, W = THREADS / kWave, KPT = 4;
    constexpr uint32_t SPAN = kWave * KPT, TILE = THREADS * KPT;
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[256];
    __shared__ uint32_t s_pick[3];
    __shared__ uint32_t s_w0[W], s_w1[W];
    const uint32_t t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t / kWave), lane = lane_id();
    const uint64_t cols = a.cols;
    const uint32_t k = a.k;
    tr_stamp(a, (uint32_t)kTrStream);
    for (uint32_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const uint32_t *krow = a.kin + (size_t)r * cols;
        uint32_t T = 0, krem = k, sh = 24;
        for (int level = 0; level < 4; ++level) {
            sh = 24 - 8 * level;
            if (t < 256) s_cnt[t] = 0;
            __syncthreads();
            for (uint64_t i = t; i < cols; i += THREADS) {
                const uint32_t x = krow[i] ^ a.m;
                if (level == 0 || (x >> ((sh + 8) & 31u)) == T) count_add(s_cnt, (x >> sh) & 255u);
            }
            __syncthreads();
            if (wave == 0) {
                uint32_t d, rem, n;
                tr_pick(s_cnt, krem, d, rem, n);
                if (lane == 0) {
                    s_pick[0] = d;
                    s_pick[1] = rem;
                    s_pick[2] = n;
                }
            }
            __syncthreads();
            T = (T << 8) | s_pick[0];
            krem = s_pick[1];
            if (s_pick[2] == krem) break;  // (the same words for every thread: all leave together)
        }
        // T holds the chosen digits above bit sh; entries are compared by those bits alone
        uint32_t *ko = a.kout + (size_t)r * k;
        uint32_t *vo = a.pairs ? a.vout + (size_t)r * k : nullptr;
        const uint32_t *vrow = a.pairs == kTrValues ? a.vin + (size_t)r * cols : nullptr;
        uint32_t base0 = 0, base1 = 0;
        for (uint64_t tb = 0; tb < cols; tb += TILE) {
            uint32_t x[KPT], c[KPT], cl = 0, ce = 0;  // c: 0 below T, 1 equal, 2 above or past the row's end
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint64_t i = tb + wave * SPAN + j * kWave + lane;
                const bool ok = i < cols;
                x[j] = ok ? krow[i] ^ a.m : 0u;
                c[j] = !ok ? 2u : (x[j] >> sh) < T ? 0u : (x[j] >> sh) == T ? 1u : 2u;
                cl += c[j] == 0u ? 1u : 0u;
                ce += c[j] == 1u ? 1u : 0u;
            }
            const uint32_t n0 = __builtin_amdgcn_readlane(wave_incl_scan(cl), kWave - 1);
            const uint32_t n1 = __builtin_amdgcn_readlane(wave_incl_scan(ce), kWave - 1);
            __syncthreads();  // (the previous tile's readers of s_w0 / s_w1, and the pick's of s_pick, are done)
            if (lane == 0) {
                s_w0[wave] = n0;
                s_w1[wave] = n1;
            }
            __syncthreads();
            uint32_t r0, r1, t0, t1;
            waves_prefix<W>(s_w0, wave, r0, t0);
            waves_prefix<W>(s_w1, wave, r1, t1);
            r0 += base0;
            r1 += base1;
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const uint64_t m0 = __ballot(c[j] == 0u), m1 = __ballot(c[j] == 1u);
                const uint32_t b0 = r0 + below_in(m0), b1 = r1 + below_in(m1);
                const uint32_t pos = b0 + min(b1, krem);
                if ((c[j] == 0u || (c[j] == 1u && b1 < krem)) && pos < k) {
                    const uint64_t i = tb + wave * SPAN + j * kWave + lane;
                    ko[pos] = a.raw ? x[j] ^ a.m : x[j];
                    if (a.pairs) vo[pos] = a.pairs == kTrIndices ? (uint32_t)i : vrow[i];
                }
                r0 += wave_count(m0);
                r1 += wave_count(m1);
            }
            base0 += t0;
            base1 += t1;
        }
        if (base0 + min(base1, krem) != k && t == 0) atomicAdd(&a.state[kTrBadRows], 1u);
        __syncthreads();  // (the next row's first writes to s_cnt / s_pick come after every reader of this row)
    }
}

// off[i] = i * k, i <= rows: the finishing sort's segments are the rows of the rows x k output.
__global__ __launch_bounds__(256) void tr_offsets(uint32_t *off, uint32_t rows, uint32_t k) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= rows; i += stride)
        off[i] = (uint32_t)(i * k);
}

using SelectFn = void (*)(TopkRowsArgs);

SelectFn select_fn(int cls) {
    switch (cls) {
        case kTrWave: return tr_select<kTrWave, 256, kSegWaveKpt, 1>;
        case kTrSmall: return tr_select<kTrSmall, kSegSmallThreads, kSegSmallKpt, kSegSmallThreads / kWave>;
        case kTrLds: return tr_select<kTrLds, kSegLdsThreads, kSegLdsKpt, kSegLdsThreads / kWave>;
        case kTrStream: return tr_stream;
        default: return nullptr;
    }
}

int threads_of(int cls) { return cls == kTrWave || cls == kTrSmall ? 256 : 1024; }

}  // namespace

hipError_t launch_topk_rows_select(int cls, const TopkRowsArgs &a, uint32_t grid, hipStream_t s) {
    const SelectFn fn = select_fn(cls);
    if (fn == nullptr || grid == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads_of(cls)), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_rows_offsets(uint32_t *off, uint32_t rows, uint32_t k, hipStream_t s) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)rows + 1 + 255) / 256, 4096);
    hipLaunchKernelGGL(tr_offsets, dim3(grid), dim3(256), 0, s, off, rows, k);
    return hipGetLastError();
}

int topk_rows_blocks_per_cu(int cls) {
    const SelectFn fn = select_fn(cls);
    int nb = 0;
    if (fn == nullptr) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)fn, threads_of(cls), 0) != hipSuccess)
        return 0;
    return nb;
}

}  // namespace rsort

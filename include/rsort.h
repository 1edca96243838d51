/*
 * rsort.h -- C ABI of the MI355X (gfx950) LSD radix sort (library: cuda.radixsort_amd/librsort.so).
 *
 * Drop-in boundary for the device sort of truongchauhien/CUDA.RadixSort. Every entry point
 * takes plain pointers and sizes (no C++ or torch types) and returns an rsort_status
 * (0 = ok) instead of the reference's print-and-exit CHECK (SourceCode/common/common.h:6-16);
 * include/radixsort.hpp restores the reference's exact C++ signatures and exit-on-error
 * behaviour on top of this ABI.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   rsort_u32            sortByDevice(h_in, n, h_out, numBits, blockSize)   Parallel7.cu:530-639
 *                        (host -> host, synchronous, device memory owned by the callee)
 *   rsort_u32_ex         the same plus the reference's per-phase timers       Parallel7.cu:532-538,633-638
 *   rsort_u32_device     the per-digit loop of sortByDevice on device buffers  Parallel7.cu:561-623
 *   rsort_pass_histogram histogram() + histogramKernel                        Parallel7.cu:318-359
 *   rsort_pass_scan      transpose() + scan() + transpose()                   Parallel7.cu:361-528, :596-598
 *   rsort_pass_scatter   sortLocallyDataBlocks() + scatter()                  Parallel7.cu:79-316, :568, :612
 *   rsort_pass_local_sort sortLocallyDataBlocks() alone                       Parallel7.cu:193-251
 *   rsort_u32_vendor     sortByThrust (the vendor comparator)                 Parallel7.cu:69-73
 *   (no counterpart)     rsort_u32_pairs*: key + u32 payload (BASELINE config 4)
 *   (no counterpart)     rsort_u32_segmented*: many independent segments of one array in one call
 *   (no counterpart)     rsort_u32_topk*: the k smallest or largest keys and their input positions
 *   (no counterpart)     rsort_u32_topk_rows*: the same for every row of a matrix in one call
 *   (no counterpart)     rsort_partition_device / rsort_bucket_starts: the multi-GPU
 *                        key-range partition step (BASELINE config 5)
 *
 * Semantics shared by every sort entry point:
 *   - keys are uint32_t, sorted ascending; k_bits in [1, 13] digit bits per pass (13: the reference's SMEM limit), passes at
 *     bit 0, k, 2k, ... < 32 (the last digit is short when k does not divide 32, exactly as
 *     Baseline1.cu:30-49);
 *   - output is bit-exact with Baseline1.cu's sortByHost; pairs are STABLE (equal keys keep
 *     their input order), i.e. equal to Baseline1's loop carrying the payload;
 *   - 0 <= n < 2^32; n == 0 is a no-op; `in` is never written; in == out is allowed;
 *   - device entry points are stream-ordered on `stream` (a hipStream_t, NULL = the null
 *     stream), do no allocation, no host synchronisation and are graph-capturable; they use
 *     the caller's workspace (rsort_workspace_size bytes, any alignment >= 256 B);
 *   - the workspace's content on entry is arbitrary (every word a call reads it has written first), and successive
 *     calls of any plans and entry points may share one workspace on one stream;
 *   - the device is the caller's current HIP device.
 */
#ifndef RSORT_H_
#define RSORT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define RSORT_API
#else
#define RSORT_API __attribute__((visibility("default")))
#endif

typedef enum rsort_status {
    RSORT_OK = 0,
    RSORT_ERR_ARG = 1,        /* NULL pointer where data is required, bad option value */
    RSORT_ERR_BITS = 2,       /* k_bits outside [1, 13] */
    RSORT_ERR_SIZE = 3,       /* n < 0 or n >= 2^32 */
    RSORT_ERR_ALIGN = 4,      /* device buffer not 4-byte aligned */
    RSORT_ERR_ALLOC = 5,      /* hipMalloc / host allocation failed */
    RSORT_ERR_HIP = 6,        /* a HIP runtime call or kernel launch failed */
    RSORT_ERR_WORKSPACE = 7,  /* workspace too small */
    RSORT_ERR_NODEV = 8,      /* no HIP device visible */
    RSORT_ERR_CAPACITY = 9,   /* multi-GPU: this rank receives more keys than its output holds */
    RSORT_ERR_COMM = 10,      /* multi-GPU: an RCCL call failed */
    RSORT_ERR_CHECK = 11      /* host entries: an on-device self-check of the sort failed (rsort_plan_check) */
} rsort_status;

/* Local-rank algorithm inside a tile (all give the same, unique, stable result). */
typedef enum rsort_rank_algo {
    RSORT_RANK_MATCH = 0,  /* default: per-wave LDS digit counters; a key's rank is one
                              returning LDS add where the device serves same-address lanes in
                              lane order (probed once per device, rsort_lane_order_probe),
                              else the ballot peer-match below */
    RSORT_RANK_SPLIT = 1,  /* k successive block-local 1-bit splits, ballot/popcount scans
                              (the reference's algorithm, Parallel5.cu:79-159 / P7:79-191) */
    RSORT_RANK_BALLOT = 2  /* per-wave LDS digit counters + wave64 ballot peer-match */
} rsort_rank_algo;

/* Phases reported by the profiler (the reference's MEASURE_PORTION_EXECUTION_TIME buckets,
 * Parallel7.cu:634-637; the local sort is fused into the scatter kernel here). */
typedef enum rsort_phase {
    RSORT_PHASE_HISTOGRAM = 0,
    RSORT_PHASE_SCAN = 1,
    RSORT_PHASE_SCATTER = 2, /* fused block-local sort + rank + scatter: the measured pass */
    RSORT_PHASE_COPY = 3,    /* device-to-device copies (in-place sorts with an odd pass count) */
    RSORT_PHASE_PARTITION = 4, /* the multi-GPU key-range partition's scatter kernel (its histogram
                                  and scan count as HISTOGRAM and SCAN), kept apart from the sort's
                                  scatter passes so each has its own roofline figure */
    RSORT_PHASE_COUNT = 5
} rsort_phase;

typedef struct rsort_phase_times {
    double ms[RSORT_PHASE_COUNT];         /* summed kernel time per phase (hipEvent pairs) */
    int64_t launches[RSORT_PHASE_COUNT];  /* launches per phase */
    int64_t keys[RSORT_PHASE_COUNT];      /* keys processed per phase (sum over launches) */
} rsort_phase_times;

/* Geometry of one sort: tiles of tile_keys keys are locally sorted by one workgroup;
 * chunk_keys = tiles_per_chunk * tile_keys keys form one row of the chunk x digit table
 * (the reference's "block" of Baseline4.cu:79/Parallel7.cu:541, with the table stored
 * column-major [digit][chunk]). */
typedef struct rsort_plan {
    int64_t n;
    int32_t k_bits;
    int32_t passes;          /* ceil(32 / k_bits) */
    int32_t bins;            /* 2^k_bits */
    int32_t threads;         /* workgroup size */
    int32_t tile_keys;       /* keys per tile */
    int32_t pairs;           /* 1: key + value */
    int64_t tiles_per_chunk;
    int64_t chunk_keys;
    int64_t num_chunks;      /* workgroups per histogram / scatter launch */
    int64_t table_entries;   /* bins * num_chunks */
    int64_t scan_blocks;     /* workgroups of the table scan */
    size_t workspace_bytes;  /* for rsort_u32_device / rsort_u32_pairs_device */
} rsort_plan;

RSORT_API const char *rsort_status_string(int status);
RSORT_API int rsort_version(void); /* major * 10000 + minor * 100 + patch */

/* Geometry for (n, k_bits, pairs). tiles_per_chunk = 0 picks it from the current device's
 * CU count and the scatter kernel's occupancy (a fixed default when no device is visible). */
RSORT_API int rsort_plan_make(int64_t n, int k_bits, int pairs, int64_t tiles_per_chunk,
                              rsort_plan *plan);
/* Workspace bytes of a device sort: the ping-pong keys (4n, and 4n more for values), the chunk table and
 * scan sums (a few hundred KB), 256 B of check words, and by plan kind: k = 8 plans with 256 chunks (every
 * 2^23..2^31-key sort on a 256-CU MI355X) a FIXED ~65 MiB more -- the joint counts (256 KB), the cut plan
 * and its piece counts (~0.5 MB) and the per-chunk joint-count rows (256^3 words = 64 MiB + 256 KB), which
 * only skewed chunks write but every such plan reserves (near 2^23 keys that is more than the keys); k = 3,
 * 4 plans two more chunk tables. */
RSORT_API size_t rsort_workspace_size(int64_t n, int k_bits, int pairs);

/* ---------------------------------------------------------------- whole sort, device */
RSORT_API int rsort_u32_device(const uint32_t *d_in, uint32_t *d_out, int64_t n, int k_bits,
                               void *d_workspace, size_t workspace_bytes, void *stream);
RSORT_API int rsort_u32_pairs_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                                     uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t n,
                                     int k_bits, void *d_workspace, size_t workspace_bytes,
                                     void *stream);
/* Same, with an explicit plan (from rsort_plan_make) -- lets tests pin the geometry. Every entry point that
 * takes a plan checks it first: RSORT_ERR_ARG for inconsistent fields and for a (k_bits, pairs, threads x tile_keys)
 * no scatter kernel exists for -- a plan is the planner's, or one the planner could have made. */
/* rsort_sort_planned with flags: RSORT_SORT_NO_HYBRID keeps this sort off the hybrid route (rsort_set_hybrid)
 * whatever the process-wide setting says. */
#define RSORT_SORT_NO_HYBRID 1
RSORT_API int rsort_sort_planned_ex(const rsort_plan *plan, const uint32_t *d_keys_in,
                                    const uint32_t *d_vals_in, uint32_t *d_keys_out,
                                    uint32_t *d_vals_out, void *d_workspace, size_t workspace_bytes,
                                    void *stream, int flags);
RSORT_API int rsort_sort_planned(const rsort_plan *plan, const uint32_t *d_keys_in,
                                 const uint32_t *d_vals_in, uint32_t *d_keys_out,
                                 uint32_t *d_vals_out, void *d_workspace, size_t workspace_bytes,
                                 void *stream);

/* ---------------------------------------------------------------- whole sort, host -> host */
/* Synchronous drop-in for sortByDevice (Parallel7.cu:530): H2D, sort, D2H on the current
 * device with a library-owned, per-device cached workspace. */
RSORT_API int rsort_u32(const uint32_t *in, uint32_t *out, int64_t n, int k_bits);
/* Same; block_size is accepted for signature compatibility and has NO effect (the reference sets its
 * tile size from it, Parallel7.cu:541; here the gfx950 tile geometry follows k, n and pairs); `times`
 * (may be NULL) receives the per-phase kernel times of this call. */
RSORT_API int rsort_u32_ex(const uint32_t *in, uint32_t *out, int64_t n, int k_bits,
                           int block_size, rsort_phase_times *times);
RSORT_API int rsort_u32_pairs(const uint32_t *keys_in, const uint32_t *vals_in,
                              uint32_t *keys_out, uint32_t *vals_out, int64_t n, int k_bits);

/* ---------------------------------------------------------------- segmented sort */
/* Many independent segments of one array in one call (no reference counterpart; what a caller otherwise
 * does with one rsort_u32_device call, a dozen launches, per segment).
 *   - Segments: d_offsets holds num_segments + 1 u32 on the device; segment i is [off[i], off[i + 1]) of the
 *     n keys. Segments that overlap each other are undefined.
 *   - Output: segment i of the output is the ascending sort of segment i of the input, bit-exact with
 *     Baseline1.cu's sortByHost applied to the segment; with values the sort is STABLE (Baseline1's loop
 *     carrying the payload). There is no k_bits argument: the result does not depend on it, and the kernels
 *     use 8-bit digits.
 *   - Limits: 0 <= n < 2^32, 0 <= num_segments < 2^31; n == 0 or num_segments == 0 is a no-op that needs no
 *     buffers; empty segments are allowed (they belong to no class below).
 *   - Elements that lie in no segment (before off[0], after off[num_segments]) are not written.
 *   - in == out is allowed for keys and for values; partial overlap is undefined; `in` is otherwise never
 *     written.
 *   - A segment with off[i] > off[i + 1] or off[i + 1] > n is REJECTED on the device before any access that
 *     uses it: nothing is read or written for it, it is counted as rejected and RSORT_CHECK_OFFSETS is set in
 *     the call's check word (rsort_segmented_check); all other segments are sorted normally.
 *   - Stream-ordered on `stream`, no allocation, no host synchronisation, graph-capturable; the current
 *     device; buffers (keys, values, offsets, workspace) may have any 4-byte alignment.
 *   - Three classes by length, decided on the device (rsort_segmented_capacity gives the two limits, the same
 *     for keys and pairs): up to *small_keys keys the segment is sorted inside LDS by one wave (up to 256 keys)
 *     or one 256-thread workgroup, several per CU; up to *lds_keys by a 1024-thread workgroup; a longer
 *     segment is sorted by ONE workgroup in four passes through the workspace. That multi-tile path is the correctness net, not a fast path -- one CU sorts the whole
 *     segment -- so a caller with multi-million-key segments should sort each with rsort_u32_device.
 *   - Ranking follows rsort_set_rank_algo as every sort does: lane-ordered returning LDS adds by default (where
 *     rsort_lane_order_probe() == 1), with the rank check on every wave's first slot whenever it is full, in
 *     every pass (RSORT_CHECK_RANK_ORDER in the check word; rsort_inject_rank_fault applies); the ballot peer
 *     match otherwise (RSORT_RANK_BALLOT, RSORT_RANK_SPLIT, or a failed probe).
 *   - Workspace bytes, with r(x) = x rounded up to a multiple of 256:
 *         r(4 n) * (pairs ? 2 : 1)  the multi-tile path's ping-pong keys (and values)
 *       + 4 * r(4 num_segments)     the lists of segment indices, one per kernel
 *       + 256                       the class counters and check words
 *   - Errors, returned before any HIP call: RSORT_ERR_SIZE (n), RSORT_ERR_ARG (num_segments out of range,
 *     exactly one of the two value pointers, NULL keys / offsets / workspace), RSORT_ERR_ALIGN,
 *     RSORT_ERR_WORKSPACE.
 *   - rsort_profile_begin/end: the classification counts as RSORT_PHASE_HISTOGRAM, the sort kernels as
 *     RSORT_PHASE_SCATTER. */
/* LDS capacities of the segmented sort, in keys (multiples of 64): segments of up to *small_keys keys
 * take the small workgroup shape, up to *lds_keys the large one; longer ones the multi-tile path. */
RSORT_API int    rsort_segmented_capacity(int pairs, int *small_keys, int *lds_keys);
RSORT_API size_t rsort_segmented_workspace_size(int64_t n, int64_t num_segments, int pairs);
RSORT_API int    rsort_u32_segmented_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                                            uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t n,
                                            const uint32_t *d_offsets, int64_t num_segments,
                                            void *d_workspace, size_t workspace_bytes, void *stream);
/* after the call has completed on `stream`: *flags = check bits (RSORT_CHECK_RANK_ORDER, RSORT_CHECK_OFFSETS);
 * class_counts (may be NULL) receives {small, lds, multi-tile, rejected} segment counts. Synchronises the
 * stream. Like the sort entry points above, the device entry cannot return these itself. */
#define RSORT_CHECK_OFFSETS 4
RSORT_API int    rsort_segmented_check(int64_t n, int64_t num_segments, int pairs, const void *d_workspace,
                                       int *flags, int64_t *class_counts, void *stream);
/* host -> host, synchronous, library-owned cached workspace (as rsort_u32). The offsets are checked on the
 * host first (RSORT_ERR_ARG for a decreasing pair or one beyond n, before the device is touched); only the
 * covered range [off[0], off[num_segments]) is copied in and out. RSORT_ERR_NODEV without a device (there is
 * no CPU fallback); RSORT_ERR_CHECK when the rank check failed. */
RSORT_API int    rsort_u32_segmented(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                                     uint32_t *vals_out, int64_t n, const uint32_t *offsets,
                                     int64_t num_segments);

/* ---------------------------------------------------------------- top-k selection */
/* The k smallest or largest keys of n, and where they sit in the input, without sorting all n (no reference
 * counterpart; what a caller otherwise does with rsort_u32_pairs_device over an iota array and a slice).
 *   - Result, unique: let m = 0xFFFFFFFF with RSORT_TOPK_LARGEST, else 0. Take the STABLE ascending sort of the
 *     entries by key ^ m (equal keys stay in input order); the output is its first k entries, keys_out[0..k) and
 *     vals_out[0..k). So the smallest come smallest first and the largest come largest first; among the keys equal
 *     to the k-th key those at the lowest input positions are taken, and stay in input order. A keys-only result
 *     is simply the sorted multiset. With RSORT_TOPK_UNSORTED the same k (key, value) entries come back in an
 *     unspecified order.
 *   - Values: d_vals_in / d_vals_out both given: each key's u32 payload travels with it. RSORT_TOPK_INDICES:
 *     d_vals_in must be NULL and d_vals_out receives each key's position in the input (no iota array is read).
 *     `pairs` in the size, report and grid functions means "values or INDICES".
 *   - Limits: 0 <= n < 2^32, 0 <= k <= n; k == 0 (so also n == 0) is a no-op that needs no buffers.
 *   - Buffers: any 4-byte alignment (keys, values, outputs, workspace). The outputs must not overlap the inputs;
 *     the inputs are never written. Stream-ordered on `stream`, no allocation, no host synchronisation,
 *     graph-capturable; the current device; the workspace's content on entry is arbitrary.
 *   - Routes (rsort_set_topk_route, process-wide): RSORT_TOPK_SELECT, a radix select -- two reads of the input
 *     (the top 8 bits of key ^ m are counted per slice, then the entries below the digit that holds the k-th go to
 *     the result and those with it to a candidate list), two more counts over the candidates (12 bits each), after
 *     which the k-th key is known exactly, one count and one append over the candidates, and rsort_sort_planned of
 *     the k entries. Every kernel runs on a host-known grid (rsort_topk_grids) of 1024-thread workgroups over
 *     tiles of 4096 entries; the candidate list's length stays on the device. RSORT_TOPK_SORT: the whole sort of
 *     the n entries (of an iota array with INDICES, of a transformed copy with LARGEST and values) and a copy of
 *     the first k: what a caller without the select does; same contract, bit-identical output. RSORT_TOPK_AUTO
 *     (default): SELECT for k <= rsort_topk_auto_limit(n, pairs), else SORT.
 *   - Workspace bytes (rsort_topk_workspace_size; with a route forced pass that route, with RSORT_TOPK_AUTO it is
 *     what the automatic route for (n, k) needs), with r(x) = x rounded up to a multiple of 256 and p = pairs ? 2 : 1:
 *       SELECT:   256                      the state and report words
 *               + r(4 * 8448)              the bin totals of the three levels (256 + 4096 + 4096)
 *               + 2 * 1024 * 256 * 4       the per-slice digit counts of level 0 and their prefixes (up to 1024 slices)
 *               + 2 * r(8 * 1024)          the per-slice offsets of level 0 and of the last step
 *               + p * r(4 k)               the selected entries
 *               + p * r(4 n)               the candidates (all n when the top digit separates nothing)
 *               + rsort_workspace_size(k, 8, pairs)   the finishing sort
 *               + 256                      alignment slack
 *       SORT:     256 + p * r(4 n) + rsort_workspace_size(n, 8, pairs) + 256
 *   - Errors, returned before any HIP call: RSORT_ERR_SIZE (n), RSORT_ERR_ARG (k out of range, unknown flag bits,
 *     exactly one of the two value pointers, INDICES with a non-NULL d_vals_in or a NULL d_vals_out, NULL keys /
 *     output / workspace), RSORT_ERR_ALIGN, RSORT_ERR_WORKSPACE.
 *   - rsort_profile_begin/end: the counts are RSORT_PHASE_HISTOGRAM, the picks RSORT_PHASE_SCAN, the compaction and
 *     the append RSORT_PHASE_SCATTER, the copies RSORT_PHASE_COPY; the finishing sort reports its own phases. */
#define RSORT_TOPK_LARGEST  1   /* the k largest instead of the k smallest */
#define RSORT_TOPK_UNSORTED 2   /* the same k entries, in no particular order */
#define RSORT_TOPK_INDICES  4   /* d_vals_in must be NULL; d_vals_out receives each key's input position */

#define RSORT_TOPK_AUTO 0
#define RSORT_TOPK_SELECT 1
#define RSORT_TOPK_SORT 2

RSORT_API size_t rsort_topk_workspace_size(int64_t n, int64_t k, int pairs, int route);
RSORT_API int    rsort_u32_topk_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, int64_t n, int64_t k,
                                       int flags, uint32_t *d_keys_out, uint32_t *d_vals_out, void *d_workspace,
                                       size_t workspace_bytes, void *stream);
/* host -> host, synchronous, library-owned cached workspace (as rsort_u32). RSORT_ERR_NODEV without a device;
 * RSORT_ERR_CHECK when the sort the call ran failed a self-check (report8[6] below is not 0). */
RSORT_API int    rsort_u32_topk(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t k, int flags,
                                uint32_t *keys_out, uint32_t *vals_out);
/* After the call has completed on `stream` in `d_workspace`: report8[0] = the route taken (RSORT_TOPK_SELECT or
 * RSORT_TOPK_SORT), [1] = the k-th key (as stored, not xor-ed), [2] = the selected entries strictly before it in
 * the order, [3] = the entries equal to it that were taken, [4] = the entries equal to it in the input, [5] = the
 * candidates left after the first digit, [6] = the self-checks of the sort the call ran, as rsort_plan_check reports
 * them (RSORT_CHECK_* bits, 0 = clean): the finishing sort of the k entries on the SELECT route, the whole sort on
 * the SORT route; 0 when the call ran no sort (RSORT_TOPK_UNSORTED on the SELECT route), whatever the workspace held
 * before; [7] = 0 (reserved). On the SORT route [0], [1] and [6] are filled and [2..5] are -1. All 0 for k == 0.
 * The device entry is stream-ordered and cannot return the check: this report is the only way to learn of it.
 * n, k and pairs must be the call's (the sort's workspace lies behind regions they size). Synchronises the stream,
 * as rsort_segmented_check does. */
RSORT_API int    rsort_topk_report(int64_t n, int64_t k, int pairs, const void *d_workspace, int64_t *report8,
                                   void *stream);
/* Process-wide, like rsort_set_hybrid; returns the old route, or -RSORT_ERR_ARG for an unknown one (nothing changes). */
RSORT_API int    rsort_set_topk_route(int route);
RSORT_API int    rsort_get_topk_route(void);
/* RSORT_TOPK_AUTO selects for k <= *k_max: n / 16 keys only, n / 2 with values or indices. From the uniform-key rows
 * of profiles/topk.json, the largest measured k / n at which SELECT beat SORT at both 2^26 and 2^30 keys:
 * keys only 1.30x at n / 16 (2^30; n / 4 is 8 % slower there), pairs 1.15x and 1.20x at n / 2, the largest k measured --
 * margins many times the ~1 % run-to-run spread. Keys whose top digit separates nothing (all below 2^24, say) make
 * SELECT read everything five times: keys only it is then 17 % (small k) to 27 % (k = n / 16) slower than SORT at 2^30
 * keys, and still ahead with values or indices; AUTO cannot know the keys before it reads them. */
RSORT_API int    rsort_topk_auto_limit(int64_t n, int pairs, int64_t *k_max);
/* The workgroups each select kernel of a call with these arguments is launched with now, on the current device:
 * grids[0..3] = the level-0 count, the compaction, the last count, the append (one number, G: the kernels share
 * their slices). G = min(CUs x resident workgroups per CU, 1024, max(64, tiles of 4096 keys in n)), capped by the
 * hook below; a workgroup with more than one tile walks them in turn, one beyond the list has an empty slice.
 * All 0 for k == 0. RSORT_ERR_NODEV without a device (the occupancy is the device's). */
RSORT_API int    rsort_topk_grids(int64_t n, int64_t k, int pairs, int *grids);
/* TEST HOOK (never set in production): workgroups > 0 caps G; 0 (the default) is no limit. Process-wide; returns the
 * previous setting, or -RSORT_ERR_ARG for a negative value (nothing changes). */
RSORT_API int    rsort_set_topk_grid_limit(int workgroups);

/* ---------------------------------------------------------------- row-wise top-k */
/* The k smallest or largest keys of EVERY ROW of a rows x cols matrix in one call (no reference counterpart; what a
 * caller otherwise does with the segmented sort of all rows x cols keys and a slice, or with one rsort_u32_topk_device
 * call -- eleven launches, a memset and a finishing sort -- per row).
 *   - Input: `rows` contiguous rows of `cols` keys, row r = [r * cols, (r + 1) * cols). Output: rows x k, contiguous.
 *   - `flags`: RSORT_TOPK_LARGEST | RSORT_TOPK_UNSORTED | RSORT_TOPK_INDICES, with the meaning they have in
 *     rsort_u32_topk_device, applied to each row on its own. Let m = 0xFFFFFFFF with LARGEST, else 0: row r of the
 *     output is the first k entries of the STABLE ascending sort of row r by key ^ m. Among the keys equal to a row's
 *     k-th key those at the lowest columns are taken, and they stay in column order. With values the payload travels
 *     with its key; with INDICES d_vals_in must be NULL and d_vals_out receives the COLUMN of each key, 0 .. cols - 1.
 *     With UNSORTED each row returns the same k entries in an unspecified order. `pairs` in the size, check and grid
 *     functions means "values or INDICES".
 *   - Limits: 0 <= rows < 2^31, 0 <= cols, rows * cols < 2^32, 0 <= k <= cols; rows == 0, cols == 0 or k == 0 is a
 *     no-op that needs no buffers.
 *   - Buffers: any 4-byte alignment (keys, values, outputs, workspace). The outputs must not overlap the inputs; the
 *     inputs are never written. The workspace's content on entry is arbitrary. Stream-ordered on `stream`, no
 *     allocation, no host synchronisation, graph-capturable; the current device.
 *   - Kernels: cols is the call's, so the class is picked on the host (rsort_topk_rows_grids reports it):
 *       0 wave    1 .. 256 columns      one wave per row, four rows per 256-thread workgroup, no workgroup barrier
 *       1 small   257 .. 1024           one 256-thread workgroup per row, 4 keys per lane
 *       2 lds     1025 .. 16384         one 1024-thread workgroup per row, 16 keys per lane
 *       3 stream  more                  one 1024-thread workgroup walks the row from global memory
 *     Classes 0-2 read a row once, keep it in registers and run a radix select of the row's k-th key ^ m (up to four
 *     8-bit levels over 256 LDS counters, per workgroup or, in the wave class, per wave; a level whose digit holds
 *     exactly what is wanted is the last), then write the entries below it and the first of those equal to it, in
 *     column order. Values are gathered for the selected entries only. The stream class reads its row once per level
 *     and once more to write. It is the correctness net, not a fast path -- one CU selects from the whole row -- so
 *     a caller with a handful of multi-million-key rows should loop rsort_u32_topk_device over them (8 x 2^23 keys,
 *     k = 64: 16.8 ms here, 0.96 ms for that loop).
 *   - Kernel resources (gfx950; VGPR / SGPR / LDS bytes; no scratch, no spills): wave 36 / 53 / 4096, small
 *     37 / 65 / 1068, lds 95 / 65 / 1164 (1024 threads: within 128 VGPRs), stream 38 / 84 / 1164.
 *   - Measured (MI355X, 2^26 uniform keys, keys only, sorted; DESIGN §5c, profiles/topk_rows.json), against the
 *     segmented sort of all rows and a slice: 2^16 x 2^10, k = 16: 0.243 ms (0.385); 2^12 x 2^14, k = 16: 0.174 ms
 *     (0.377), k = 1024: 0.241 (0.383); 2^8 x 2^18, k = 64: 0.541 (1.790). NOT faster: 2^20 x 64, k = 2 or 8:
 *     1.54-1.61 ms (0.85), 0.8 of it the finishing sort of 2^20 k-key rows -- UNSORTED takes 0.28 ms there; and
 *     k = cols / 2 at 2^12 x 2^14: 0.456 (0.423).
 *   - Sorted output (no UNSORTED): the select leaves every row's k entries in column order and
 *     rsort_u32_segmented_device's kernels sort the rows x k output in place (stable, so the result is the
 *     contract's), after one small kernel that writes the offsets i * k; LARGEST adds one pass over the rows x k
 *     keys. UNSORTED runs the select alone.
 *   - Workspace bytes, with r(x) = x rounded up to a multiple of 256:
 *         256                                                      the state and check words
 *       + r(4 (rows + 1))                                          the finishing sort's offsets
 *       + rsort_segmented_workspace_size(rows * k, rows, pairs)    the finishing sort
 *       + 256                                                      alignment slack
 *   - Errors, returned before any HIP call, in this order: RSORT_ERR_SIZE (rows, cols or rows * cols out of range),
 *     RSORT_ERR_ARG (k out of range, unknown flag bits, exactly one of the two value pointers, INDICES with a non-NULL
 *     d_vals_in or a NULL d_vals_out, NULL keys / output / workspace with work to do), RSORT_ERR_ALIGN,
 *     RSORT_ERR_WORKSPACE.
 *   - rsort_profile_begin/end: the select is RSORT_PHASE_SCATTER, the offsets and the LARGEST pass RSORT_PHASE_COPY;
 *     the finishing sort reports its own phases. */
RSORT_API size_t rsort_topk_rows_workspace_size(int64_t rows, int64_t cols, int64_t k, int pairs);
RSORT_API int    rsort_u32_topk_rows_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, int64_t rows,
                                            int64_t cols, int64_t k, int flags, uint32_t *d_keys_out,
                                            uint32_t *d_vals_out, void *d_workspace, size_t workspace_bytes,
                                            void *stream);
/* host -> host, synchronous, library-owned cached workspace (as rsort_u32). RSORT_ERR_NODEV without a device (there
 * is no CPU fallback); RSORT_ERR_CHECK when the check below is not clean. */
RSORT_API int    rsort_u32_topk_rows(const uint32_t *keys, const uint32_t *vals, int64_t rows, int64_t cols, int64_t k,
                                     int flags, uint32_t *keys_out, uint32_t *vals_out);
/* After the call has completed on `stream` in `d_workspace`: *flags = the finishing sort's check bits
 * (RSORT_CHECK_RANK_ORDER; 0 after an UNSORTED call); report4 (may be NULL) = {the kernel class 0..3, the rows whose
 * select wrote a number of entries other than k (must be 0), 0, 0}. All 0 for a no-op call. Synchronises the stream. */
RSORT_API int    rsort_topk_rows_check(int64_t rows, int64_t cols, int64_t k, int pairs, const void *d_workspace,
                                       int *flags, int64_t *report4, void *stream);
/* grids2 = {the select kernel's workgroups, its class} for a call with these arguments now, on the current device:
 * min(rows [a quarter of it, rounded up, in the wave class], CUs x resident workgroups per CU x 4), capped by the hook
 * below; each workgroup (each wave in the wave class) strides over the rows. Both 0 for a no-op call;
 * RSORT_ERR_NODEV without a device otherwise (the occupancy is the device's). */
RSORT_API int    rsort_topk_rows_grids(int64_t rows, int64_t cols, int64_t k, int pairs, int *grids2);
/* TEST HOOK (never set in production), as rsort_set_topk_grid_limit: workgroups > 0 caps the select kernel's grid; 0
 * (the default) is no limit. Process-wide; returns the previous setting, or -RSORT_ERR_ARG for a negative value. */
RSORT_API int    rsort_set_topk_rows_grid_limit(int workgroups);

/* ---------------------------------------------------------------- one digit pass, device */
/* digit(key) = (key >> shift) & (bins - 1). Table layout: d_table[digit * num_chunks + chunk]. */
RSORT_API int rsort_pass_histogram(const rsort_plan *plan, const uint32_t *d_keys, int shift,
                                   uint32_t *d_table, void *stream);
/* In-place exclusive scan of the column-major table; d_block_sums holds plan->scan_blocks
 * u32 of scratch. */
RSORT_API int rsort_pass_scan(const rsort_plan *plan, uint32_t *d_table, uint32_t *d_block_sums,
                              void *stream);
/* Fused block-local sort + global rank + scatter of one pass (vals may be NULL when
 * plan->pairs == 0). d_table is the scanned table of the same pass.
 * rsort_pass_scatter and rsort_pass_local_sort take no workspace and so have no check word: the self-checks that
 * rsort_plan_check reports for a whole sort are not recorded for a single pass, and no call returns them. */
RSORT_API int rsort_pass_scatter(const rsort_plan *plan, const uint32_t *d_keys_in,
                                 const uint32_t *d_vals_in, uint32_t *d_keys_out,
                                 uint32_t *d_vals_out, int shift, const uint32_t *d_table,
                                 void *stream);
/* Block-local stable sort of every tile by the digit, written in tile order (the state
 * sortLocallyDataBlocks leaves behind, Parallel7.cu:568). */
RSORT_API int rsort_pass_local_sort(const rsort_plan *plan, const uint32_t *d_keys_in,
                                    const uint32_t *d_vals_in, uint32_t *d_keys_out,
                                    uint32_t *d_vals_out, int shift, void *stream);

/* ---------------------------------------------------------------- options / profiling */
RSORT_API int rsort_set_rank_algo(int algo); /* rsort_rank_algo, process-wide */
RSORT_API int rsort_get_rank_algo(void);
/* Histograms carried between passes (default on), so passes read no keys for their histogram:
 *  - k = 8 plans with 256 chunks (digit-group chunks): every second pass takes the previous
 *    pass's digit groups as its chunks (the pass before counts (digit, next digit) pairs while
 *    it reads the keys); where the groups are unbalanced (skewed keys) it takes equal chunks
 *    and reads only the keys of the groups those chunks cut (all but each cut group's largest
 *    segment);
 *  - k = 3, 4 keys-only plans (next-digit counts): every pass adds the next pass's chunk table
 *    from where it writes each key; only pass 0 reads keys for a histogram.
 * Off: every pass counts its own histogram. Same output either way; process-wide. */
RSORT_API int rsort_set_group_chunks(int enable);
RSORT_API int rsort_get_group_chunks(void);
/* The hybrid route: keys-only k = 8 sorts read and write the keys three times instead of four.
 *
 * One joint histogram counts the 65536 (digit 3, digit 2) pairs; two MSD scatter passes (by digit 3 over fixed
 * chunks, by digit 2 over the digit-3 groups -- the same whole-line scatter kernel as the LSD passes) leave the
 * keys in 65536 contiguous buckets ordered by their top 16 bits; one kernel then sorts each bucket by its low 16
 * bits inside LDS (two 8-bit counting passes, lane-ordered ranks with the per-wave rank check) and writes it
 * once. The output of a keys-only sort is unique, so it is bit-identical to the LSD passes' output.
 *
 * A sort is ELIGIBLE (decided on the host, per call) when it is keys-only with k = 8, its plan has the 256 chunks
 * of line tiles of the digit-group path and that path is on (rsort_set_group_chunks, the default ranking with a
 * passed lane-order probe, both key outputs 4-B aligned with positions below 2^32), in != out (the route goes
 * in -> out -> workspace -> out and never writes `in`; an in-place sort stays on the LSD passes and pays no
 * staging copy), and n lies in the automatic range (rsort_hybrid_range: from the measured break-even size up to
 * where the mean bucket n / 65536 reaches rsort_hybrid_capacity()). rsort_u32_multi*'s local sorts and
 * partitions never are (a rank's keys cover 1 / N of the key space).
 *
 * An eligible sort decides the route ON THE DEVICE, with no host synchronisation, in two steps:
 *   1. the sample gate: one small launch (~5 us) reads 65536 keys at a fixed stride over the whole input, 64
 *      workgroups of 1024 keys, each counting the top-16-bit buckets of its 64th of the input; a bucket holding
 *      rsort_hybrid_gate_threshold(n) of a workgroup's 1024 keys (7 at 2^30 keys) -- a count a bucket within the
 *      capacity reaches less than once in a billion sorts (Poisson tail), i.e. a bucket of ~0.7 % of that part of
 *      the input, hundreds of times the capacity's share -- says SKEWED and the sort takes the LSD passes with no
 *      extra key read. Zipf, hot-key, all-equal and small-integer keys end here (and so may an input each 64th
 *      of which is clustered in a few buckets although the whole is balanced).
 *   2. the exact count: the joint histogram gives every bucket's size; the hybrid runs when the largest is at
 *      most rsort_hybrid_capacity() keys, else the LSD passes do -- and this sort has read the keys once more
 *      than an ineligible one (one histogram read, ~8 % of the LSD sort's time at 2^30 keys). The inputs that pay
 *      it: moderately skewed ones, whose largest top-16-bit bucket is above the capacity but holds less than
 *      ~0.7 % of the keys (e.g. keys drawn from a few thousand distinct 16-bit prefixes, or uniform keys with
 *      one prefix twice as likely as the rest).
 * Both kernel sequences are enqueued; every kernel tests the device-side mode word and those of the route not
 * taken leave at once (about two dozen empty launches when the hybrid runs, seven when the LSD passes do).
 *
 * rsort_set_hybrid (process-wide): RSORT_HYBRID_AUTO (default) as above; RSORT_HYBRID_OFF: no sort is eligible,
 * exactly the LSD passes; RSORT_HYBRID_FORCE (a test hook): the n range and the gate's verdict are ignored (the
 * gate still runs and reports), never the exact capacity check. */
#define RSORT_HYBRID_AUTO 0
#define RSORT_HYBRID_OFF 1
#define RSORT_HYBRID_FORCE 2
RSORT_API int rsort_set_hybrid(int mode);
RSORT_API int rsort_get_hybrid(void);
/* Keys one (digit 3, digit 2) bucket may hold for the hybrid route to run (18432). */
RSORT_API int rsort_hybrid_capacity(void);
/* The bucket kernel as built and as the current device holds it: info[0] = threads per workgroup, info[1] = its
 * static LDS bytes, info[2] = its scratch (spill) bytes per lane, info[3] = workgroups of it resident per CU (the
 * occupancy query the bucket grid is sized by). The kernel is written for two resident workgroups and no scratch;
 * a build that loses either still sorts, slower. */
RSORT_API int rsort_hybrid_kernel_info(int *info);
/* The automatic n range of the hybrid route, both ends inclusive. */
RSORT_API int rsort_hybrid_range(int64_t *min_keys, int64_t *max_keys);
/* The sample gate's threshold for a sort of n keys (keys of one gate workgroup's 1024 in one top-16-bit bucket),
 * or -RSORT_ERR_SIZE. */
RSORT_API int rsort_hybrid_gate_threshold(int64_t n);
/* After a sort with `plan` and `d_workspace` has completed on `stream`: report[0] = 1 if the sort was eligible,
 * report[1] = the gate's verdict (RSORT_GATE_NONE: not eligible, RSORT_GATE_PASS, RSORT_GATE_SKEWED), report[2] =
 * the largest bucket of the exact count (0 when it did not run), report[3] = 1 if the hybrid route sorted the
 * keys, 0 if the LSD passes did. Synchronises the stream. After a hybrid sort rsort_group_flags reports {1, 0}:
 * its second pass ran on the digit-3 groups and there is no fourth. */
#define RSORT_GATE_NONE 0
#define RSORT_GATE_PASS 1
#define RSORT_GATE_SKEWED 2
RSORT_API int rsort_hybrid_report(const rsort_plan *plan, const void *d_workspace, int *report, void *stream);
/* After a sort with `plan` and `d_workspace` has completed on `stream`: flags[i] says how odd
 * pass 2i+1 took its chunks (i < 2): 1 = the digit groups, 2 = equal chunks cutting unbalanced
 * groups (counted pieces), 0 = fixed chunks with a counted histogram (group chunks off, or plans
 * without them). Synchronises the stream. */
RSORT_API int rsort_group_flags(const rsort_plan *plan, const void *d_workspace, int *flags,
                                void *stream);
/* After a k = 8 digit-group sort with `plan` and `d_workspace` has completed on `stream`: how the cut plans
 * of passes 1 and 3 (rsort_group_flags 2) took the counts of their pieces, stats[4 * i + j] for pass 2i+1:
 * j = 0 key ranges counted from the keys, 1 row tasks (sums of the previous pass's per-chunk joint-count
 * rows), 2 direct adds (a chunk part whose keys all share one next digit), 3 key ranges counted negatively
 * (the complement of a piece inside a chunk). All 0 for a pass on whole groups or fixed chunks, and for
 * plans without digit groups. Synchronises the stream (tests and diagnostics). */
RSORT_API int rsort_cut_plan_stats(const rsort_plan *plan, const void *d_workspace, int *stats, void *stream);
/* After a sort with `plan` and `d_workspace` has completed on `stream`: *flags = 0 when every
 * on-device self-check of that sort passed; bit 0 (RSORT_CHECK_TABLE) = a k = 3, 4 pass found the
 * next-digit table it reads not holding n keys (the pass then wrote nothing; with RSORT_FEAT_TAIL_SCAN:
 * a tail scan found it so even after an acquire fence and a second sweep), or the hybrid route's bucket kernel
 * found a bucket's bounds outside the capacity or the input, or a key whose top 16 bits are not its bucket's --
 * the kernel keeps only the low halves and rebuilds the top half from the bucket index, so it compares EVERY key
 * it loads (full 4-B loads) with that index: a key the two MSD passes misplaced is reported, never silently
 * turned into another key; bit 1 (RSORT_CHECK_RANK_ORDER)
 * = a lane-ordered scatter kernel's per-tile rank check failed: the device no longer served the lanes of
 * a returning LDS add in lane order (the premise of the default ranking, rsort_lane_order_probe), so
 * equal digits may have been written out of order -- in either case the sort's output is not
 * trustworthy. Every plan has the check words (256 B of the workspace); the rank check runs on the first
 * slot of every 8th full tile of each chunk (its first included), every pass. Synchronises the stream. The sort entry points are stream-ordered and do not
 * wait for the device, so they CANNOT return this check: they return RSORT_OK for such a sort, and
 * this call is the only way to learn of it. rsort_u32_device / rsort_u32_pairs_device use the plan
 * rsort_plan_make(n, k_bits, pairs, 0) gives, so pass that plan and the same workspace. The host
 * entries (rsort_u32, rsort_u32_ex, rsort_u32_pairs) wait for the device anyway: they read the check
 * themselves and return RSORT_ERR_CHECK for such a sort. Never observed failing. */
#define RSORT_CHECK_TABLE 1
#define RSORT_CHECK_RANK_ORDER 2
RSORT_API int rsort_plan_check(const rsort_plan *plan, const void *d_workspace, int *flags, void *stream);
/* Which carried-histogram scheme a sort with `plan` takes under the current process settings
 * (rsort_set_rank_algo, rsort_set_group_chunks), for outputs the whole-line kernels can write (any
 * 4-B-aligned keys output): a bitmask, or -RSORT_ERR_ARG for an invalid plan.
 *   RSORT_FEAT_GROUPS       k = 8, 256 chunks: digit-group chunks on the odd passes
 *   RSORT_FEAT_NEXT_DIGIT   k = 3, 4 keys: next-digit counts (only pass 0 reads keys for a histogram)
 *   RSORT_FEAT_RAW_TABLES   ... each pass after the first derives its starts from the raw counts in
 *                           every workgroup (plans of at most 1280 chunks: the per-workgroup sum
 *                           reads the whole R x C table)
 *   RSORT_FEAT_TAIL_SCAN    ... the last workgroup of each pass scans the next table instead (plans
 *                           with more chunks, e.g. a small tiles_per_chunk) */
#define RSORT_FEAT_GROUPS 1
#define RSORT_FEAT_NEXT_DIGIT 2
#define RSORT_FEAT_RAW_TABLES 4
#define RSORT_FEAT_TAIL_SCAN 8
RSORT_API int rsort_plan_features(const rsort_plan *plan);
/* TEST HOOK (never set in production): enable != 0 makes every raw-table sort (RSORT_FEAT_RAW_TABLES)
 * corrupt one word of the table pass 1 reads, as a lost update would; that pass's workgroups then
 * find the table not holding n keys, write nothing, and record it: rsort_plan_check reports bit 0 and
 * the host entries return RSORT_ERR_CHECK. Process-wide; returns the previous setting. */
RSORT_API int rsort_inject_table_fault(int enable);
/* TEST HOOK (never set in production): enable != 0 makes every lane-ordered scatter kernel swap the ranks
 * of the first two lanes of each digit in the slot its rank check looks at -- what a device serving
 * same-address LDS adds out of lane order would do. The sort is then unstable (wrong for keys, pairs out
 * of order), and the check catches it: rsort_plan_check reports bit 1 (RSORT_CHECK_RANK_ORDER), the host
 * entries return RSORT_ERR_CHECK. Process-wide; returns the previous setting. */
RSORT_API int rsort_inject_rank_fault(int enable);
/* TEST HOOK (never set in production): a window of the CALLING THREAD over the two hooks above, so a test can fault
 * one sort of an entry that runs several (the multi-GPU sort: sample sort, lower half, upper half) and none of its
 * neighbours. The thread's sort calls -- every sort the library runs through its LSD driver, whichever entry
 * makes it -- are numbered from 0 once the window is set; only calls first .. first + count - 1 see
 * rsort_inject_table_fault / rsort_inject_rank_fault, the others run as with both cleared. count < 0 clears the
 * window (the default): every call sees the hooks. The partition's scatter, a single pass (rsort_pass_*) and the
 * segmented sort are not sort calls and lie in no window: they follow the process-wide hooks while the calling thread
 * has no window, as ever, and see neither hook while it has one (so a rank of the multi-GPU sort can fault one of its
 * sorts and not its partition). RSORT_ERR_ARG for first < 0 with count >= 0.
 * rsort_fault_window_calls: the sort calls the calling thread has started since it last set (or cleared) the
 * window -- what a test asserts its numbering with. */
RSORT_API int     rsort_inject_fault_window(int64_t first, int64_t count);
RSORT_API int64_t rsort_fault_window_calls(void);
/* The workgroups rsort_u32_segmented_device launches each of its four kernels with, for a call with these
 * arguments on the current device under the current process settings (rsort_set_rank_algo, the limit below):
 * grids[0..3] = the one-wave kernel (four segments per workgroup), the small workgroup shape, the large one, the
 * multi-tile kernel; 0 where the arguments allow no segment of the kind. Each is min(the most segments of the
 * kind that n keys in num_segments segments can hold, CUs x resident workgroups per CU x 4): a list longer than
 * its grid is strided over. The sort and this report share one computation. RSORT_ERR_NODEV without a device
 * (the occupancy is the device's). */
RSORT_API int rsort_segmented_grids(int64_t n, int64_t num_segments, int pairs, int *grids);
/* TEST HOOK (never set in production): workgroups > 0 caps the grid of every segmented-sort kernel, so small
 * inputs make each workgroup (or wave) sort several segments in turn; 0 (the default) is no limit. Process-wide;
 * returns the previous setting, or -RSORT_ERR_ARG for a negative value (nothing changes). */
RSORT_API int rsort_set_segmented_grid_limit(int workgroups);
/* The scatter kernel instantiations this library has launched since the last reset, ';'-joined
 * into buf (at most len - 1 characters and a NUL); returns the full length. reset != 0 clears the
 * record. A k = 8 digit-group sort launches a plain and a clustered-input kernel for each pass
 * after the first (the device picks one, the other leaves at once): both are listed. A hybrid-eligible sort
 * (rsort_set_hybrid) lists the bucket kernel rs_bucket_sort16 too; rsort_hybrid_report says whether it worked. */
RSORT_API size_t rsort_scatter_kernels_used(char *buf, size_t len, int reset);
/* The names of every scatter kernel instantiation the library's dispatch can launch: what its one selection
 * function returns over its whole argument domain (digit bits, keys / pairs, ranking, digit mode, tile shape,
 * line-capable outputs, n <= 2^26, fewer than four partition buckets, a clustered-input twin), ';'-joined as
 * above; returns the full length. Runs on the host alone: no device is needed. Every name
 * rsort_scatter_kernels_used reports is one of these, rs_bucket_sort16 (the hybrid route's own kernel) apart. */
RSORT_API size_t rsort_scatter_kernels_known(char *buf, size_t len);
/* 1 if the current device's LDS returns same-address atomic adds in lane order (the default
 * ranking relies on it and falls back to ballots otherwise), 0 if not, < 0 on error. The
 * probe runs once per device (a few microseconds) and is cached. It allocates and synchronises: before a
 * device entry is captured into a graph, call this (or one uncaptured sort) once on that device. */
RSORT_API int rsort_lane_order_probe(void);
/* Between begin and end, every launch made by this library records hipEvents around its
 * phases; end synchronises those events and returns the per-phase sums. */
RSORT_API int rsort_profile_begin(void);
RSORT_API int rsort_profile_end(rsort_phase_times *out);

/* ---------------------------------------------------------------- multi-GPU building blocks */
/* Stable partition of n keys (and values) into num_buckets (<= 32) key ranges:
 * bucket(key) = #{i : key >= splitters[i]} for the num_buckets-1 ascending host-side
 * splitters. Output is bucket-major and stable; d_bucket_starts[num_buckets + 1] receives
 * the exclusive bucket offsets (last = n). Workspace: rsort_partition_workspace_size. */
RSORT_API size_t rsort_partition_workspace_size(int64_t n, int num_buckets, int pairs);
RSORT_API int rsort_partition_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                                     uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t n,
                                     const uint32_t *splitters, int num_buckets,
                                     uint32_t *d_bucket_starts, void *d_workspace,
                                     size_t workspace_bytes, void *stream);
/* After rsort_partition_device(n, num_buckets, pairs) has completed on `stream` in `d_workspace`: its
 * on-device self-check, as rsort_plan_check reports a sort's (bit 1: its scatter's rank check failed).
 * Synchronises the stream. rsort_u32_multi* reads it after every partition and returns RSORT_ERR_CHECK
 * on every rank when any rank's failed (as it does for its sample sort; its local sorts' checks are the rank's own). */
RSORT_API int rsort_partition_check(int64_t n, int num_buckets, int pairs, const void *d_workspace, int *flags,
                                    void *stream);
/* Histogram of the top `top_bits` (1..12) bits of n keys into d_hist[2^top_bits] (u32,
 * overwritten). Workspace: rsort_workspace_size(n, top_bits, 0). */
RSORT_API int rsort_top_histogram(const uint32_t *d_keys, int64_t n, int top_bits,
                                  uint32_t *d_hist, void *d_workspace, size_t workspace_bytes,
                                  void *stream);
/* The same histogram over a sample: the keys of every `stride`-th block of 256 (block b is
 * counted iff b % stride == 0; stride 1 = every key). No workspace. The multi-GPU sort chooses
 * its splitters from this (stride 16: a sixteenth of the keys read). */
RSORT_API int rsort_top_histogram_sampled(const uint32_t *d_keys, int64_t n, int top_bits,
                                          int stride, uint32_t *d_hist, void *stream);

/* ---------------------------------------------------------------- multi-GPU planning (host only) */
/* The host-side decisions of the multi-GPU sort, as pure functions (no device, no communicator):
 * rsort_u32_multi* and cuda.radixsort_amd/multi.py both call them, and tests drive them on the
 * CPU at any world size. Every rank calls them with the same gathered inputs and gets the same
 * answer, so the ranks agree on every decision (including errors) without another collective.
 *
 * 1. Sampling. Given every rank's key count, the sampling stride (the same on every rank) and
 *    each rank's sample count: rank r samples key[min(n_r - 1, j * stride + stride / 2)] for
 *    j < count[r] and pads its row to row_len with 0xFFFFFFFF. Every sample then stands for
 *    `stride` keys, so the sorted union of the rows gives the global quantiles directly: the
 *    i-th of world - 1 splitters is sorted[floor(i * total_samples / world)]. */
#define RSORT_MAX_RANKS 16
typedef struct rsort_sample_plan {
    int32_t world;
    int64_t stride;                  /* keys per sample, >= 1 */
    int64_t count[RSORT_MAX_RANKS];  /* samples taken by each rank */
    int64_t row_len;                 /* samples per rank in the gathered buffer (max count, >= 1) */
    int64_t total;                   /* sum of count */
} rsort_sample_plan;
RSORT_API int rsort_multi_sample_plan(int world, const int64_t *n_per_rank, int64_t samples_per_rank,
                                      rsort_sample_plan *out);
/* The device side of step 1: d_out[j] = d_keys[min(n - 1, j * stride + stride / 2)] for j < count,
 * 0xFFFFFFFF for count <= j < row_len. */
RSORT_API int rsort_sample_device(const uint32_t *d_keys, int64_t n, int64_t stride, int64_t count,
                                  int64_t row_len, uint32_t *d_out, void *stream);
/* Index into the sorted gathered samples of splitter i (1 <= i < world). */
RSORT_API int64_t rsort_multi_quantile_index(const rsort_sample_plan *sp, int i);

/* 2. Splitters. From the world - 1 quantile keys v_1 <= ... <= v_{world-1}: the partition's
 * splitters and, for each rank boundary, where it cuts. Every distinct v gets a bucket of its own,
 * [v, v + 1) ("equal keys"), between the buckets of the keys below and above it, and boundary r
 * cuts INSIDE the equal-keys bucket of v_r at the position that balances the ranks: a run of equal
 * keys (a hot key, duplicate-heavy input) is split across ranks in global (source rank, position)
 * order, which keeps the sort stable. (2 * (world - 1) <= 30 splitters: within the partition's 32
 * buckets at every world size.) */
typedef struct rsort_multi_splitters {
    int32_t world;
    int32_t nsplit;                                 /* partition splitters (buckets = nsplit + 1) */
    uint32_t split[2 * (RSORT_MAX_RANKS - 1)];      /* non-decreasing */
    int32_t cut_bucket[RSORT_MAX_RANKS];            /* boundary r (1..world-1) lies in this bucket */
    int32_t cut_inside[RSORT_MAX_RANKS];            /* 1: anywhere inside it (equal keys); 0: at its start */
} rsort_multi_splitters;
RSORT_API int rsort_multi_splitters_make(int world, const uint32_t *quantile_keys, rsort_multi_splitters *out);
/* The same with a hot flag per quantile key (hot[r - 1] for boundary r; nullptr: every key hot, which is
 * rsort_multi_splitters_make). Only a hot key -- one whose run in the sorted sample is long enough that
 * sending all its copies to one rank would unbalance the ranks -- gets its equal-keys bucket; the others
 * are plain splitters (boundary r at the start of v_r's bucket: all copies of v_r go to rank r), one
 * bucket fewer each. Equal consecutive quantile keys are always one hot run. rsort_u32_multi* flags a key
 * hot when the sample holds it `world * 128`-th of the samples away on either side (a run of >= ~1/64 of
 * a rank's share): distinct keys get world - 1 splitters instead of 2 (world - 1). */
RSORT_API int rsort_multi_splitters_make_hot(int world, const uint32_t *quantile_keys, const int *hot,
                                             rsort_multi_splitters *out);

/* 3. Exchange. counts[s * buckets + b] = keys of rank s's partition in bucket b (the row every
 * rank gathers after partitioning); capacity[r] = output room of rank r. For rank `me`: what it
 * sends to each rank (offset and count in its partitioned buffer), what it receives from each
 * rank (in source-rank order: offset and count in its output), its output count and global
 * offset. RSORT_ERR_CAPACITY (with over_capacity = the first rank concerned) when ANY rank would
 * receive more than its capacity -- every rank sees the same matrix, so all ranks return it
 * together, before any key moves. */
typedef struct rsort_exchange_plan {
    int32_t world, me;
    int64_t send_off[RSORT_MAX_RANKS], send_cnt[RSORT_MAX_RANKS];
    int64_t recv_off[RSORT_MAX_RANKS], recv_cnt[RSORT_MAX_RANKS];
    int64_t n_recv;        /* keys this rank ends with */
    int64_t offset;        /* global rank of its first key */
    int64_t total;         /* keys over all ranks */
    int64_t max_message;   /* largest message between two different ranks, anywhere (keys) */
    int32_t over_capacity; /* -1, or the lowest rank whose output would overflow */
} rsort_exchange_plan;
RSORT_API int rsort_multi_exchange_plan(int world, int me, int buckets, const int64_t *counts,
                                        const rsort_multi_splitters *sp, const int64_t *capacity,
                                        rsort_exchange_plan *out);

/* 4. Exchange rounds. Messages of up to max_message keys (the plan's max_message), at most `limit`
 * keys each: *rounds equal pieces of *piece keys, a multiple of 64 keys (rounded up where that stays
 * within the limit -- a message under the limit is one round -- else down: never above the limit;
 * >= 64), rounds * piece >= max_message. (0, 0) for max_message 0. */
RSORT_API int rsort_multi_exchange_rounds(int64_t max_message, int64_t limit, int64_t *rounds, int64_t *piece);

/* ---------------------------------------------------------------- multi-GPU sort */
/* One rank per GPU (the reference is single-GPU, Parallel7.cu:10). Every rank
 * passes its n local keys (and values); on return rank r's d_keys_out[0 .. *out_n) holds the keys
 * of global ranks [*out_offset, *out_offset + *out_n) of the sorted union, i.e. concatenating the
 * ranks' outputs in rank order gives Baseline1's result; pairs stay stable (equal keys keep their
 * (source rank, position) order). Steps: all-gather of the key counts -> a regular sample of the
 * keys, all-gathered and sorted on the device -> world - 1 quantile keys -> splitters with a
 * bucket of its own for each hot quantile key, so a run of equal keys is split across
 * ranks -> stable partition -> all-gather of the bucket counts and capacities -> the exchange
 * plan (the same on every rank) -> one exchange (own range by a device copy, the rest point to
 * point in rounds of <= 2^28 keys per message) -> local LSD sort. Synchronises `stream` five
 * times: four for counts the host needs, and once at the end for the local sorts' self-checks, so the call
 * returns only when its local sort has finished (it is not asynchronous in its last step).
 * capacity: room in d_keys_out / d_vals_out. RSORT_ERR_CAPACITY when ANY rank would receive more
 * than its capacity: every rank returns it, before any key moves (balanced output needs about
 * total / world plus the sampling error, ~0.1 %). Up to RSORT_MAX_RANKS ranks.
 * Errors: a failure on one rank before the exchange (bad k_bits / sizes / pointers, a workspace
 * too small, a device error in sampling, sample sort or partition) travels in a status word of the
 * next all-gather, and EVERY rank returns the lowest rank's status together -- no rank is left
 * waiting in a collective (a rank that dies instead is caught by the RCCL timeout below). Only a transport that cannot run at all (NULL
 * transport or workspace, a workspace smaller than the collectives' control buffers) returns at
 * once on that rank. Failures in or after the exchange (the exchange itself, the local sort) are
 * the failing rank's own.
 * Self-checks (rsort_plan_check's bits): every sort and the partition this call runs is checked, and a failed
 * check is RSORT_ERR_CHECK, never a silent RSORT_OK. The sample sort's and the partition's are read before the
 * exchange and travel like any other failure there: every rank returns RSORT_ERR_CHECK together, before any key
 * moves. The local sorts' -- each half's under the overlap, the direct sort's at world 1 -- are copied into the
 * control area right behind each sort (the halves share one sort workspace, so the upper half's sort would clear
 * what the lower half's recorded) and read at the end: RSORT_ERR_CHECK on that rank alone, whose output is then not
 * trustworthy; the other ranks' slices are right. */
RSORT_API size_t rsort_multi_workspace_size(int64_t n, int64_t capacity, int k_bits, int pairs, int world);
/* Over an RCCL communicator (`nccl_comm` is an ncclComm_t; RCCL result codes are all checked,
 * RSORT_ERR_COMM on failure). Every RCCL call is bounded: the sort waits for each collective and
 * exchange round to complete (host-polled), and when one has not completed within the communicator
 * timeout (rsort_set_comm_timeout) -- a peer that died or never joined -- or RCCL reports an
 * asynchronous error, it aborts the communicator (ncclCommAbort) and returns RSORT_ERR_COMM. The
 * communicator is then gone: do not use or destroy it again (rsort_rccl_comm_destroy knows it). */
RSORT_API int rsort_u32_multi(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n,
                              uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t capacity,
                              int64_t *out_n, int64_t *out_offset, int k_bits, void *nccl_comm,
                              void *d_workspace, size_t workspace_bytes, void *stream);

/* RCCL communicators with bounded setup (replaces ncclGetUniqueId / ncclCommInitRank for the
 * callers of rsort_u32_multi): the id (NCCL_UNIQUE_ID_BYTES = 128 bytes) is made on one rank and
 * sent to the others out of band; init creates the rank's communicator on the current device,
 * non-blocking (ncclCommInitRankConfig, blocking = 0), and polls it until it is ready -- or, after
 * timeout_ms (<= 0: the rsort_set_comm_timeout value), aborts it and returns RSORT_ERR_COMM, so a
 * peer that never joins cannot hang this rank. destroy: ncclCommDestroy, or nothing for a
 * communicator a timeout already aborted. */
RSORT_API int rsort_rccl_unique_id(void *id128);
RSORT_API int rsort_rccl_comm_init(void **comm, int world, int rank, const void *id128, int timeout_ms);
RSORT_API int rsort_rccl_comm_destroy(void *comm);
/* How long one RCCL step of rsort_u32_multi (a collective, an exchange round, the communicator's
 * setup) may take before the communicator is aborted: default 300000 ms. Process-wide; returns the
 * previous value; values <= 0 leave it unchanged. */
RSORT_API int rsort_set_comm_timeout(int timeout_ms);

/* Options of rsort_u32_multi* (process-wide; returns the previous flags):
 *  RSORT_MULTI_OVERLAP  every rank's key range is cut in two at a sampled quantile (the planning
 *                       functions run for 2 x world ranks, world <= 8): the lower halves are
 *                       exchanged first, and each rank sorts its lower half on a second stream
 *                       while the upper halves are exchanged; same output.
 *  RSORT_MULTI_NO_OVERLAP  never cut the ranges in two.
 *  Neither: the overlap runs for 2 <= world <= 8 (RSORT_MULTI_AUTO_OVERLAP_MAX_WORLD; 2 x world <=
 *                       RSORT_MAX_RANKS virtual ranks), where it is predicted faster at every size
 *                       (components measured on one GPU; at world 8 the partition into
 *                       16 buckets costs 2.49 ms, as the 8 buckets without halves).
 *  RSORT_MULTI_FULL     run the whole protocol also at world 1 (sample, partition into one
 *                       bucket, self exchange): for tests and overhead measurements. By default
 *                       one rank sorts its keys directly (the partition would be a copy). */
#define RSORT_MULTI_OVERLAP 1
#define RSORT_MULTI_FULL 2
#define RSORT_MULTI_NO_OVERLAP 4
#define RSORT_MULTI_AUTO_OVERLAP_MAX_WORLD 8
RSORT_API int rsort_set_multi_options(int flags);

/* Per-phase record of a multi-GPU sort (rsort_u32_multi*), for the N-GPU bench line. Off by
 * default; while on, every multi-GPU sort records hipEvents on its stream at the phase boundaries
 * and synchronises its stream before returning (so it is no longer asynchronous), and the calling
 * thread's last sort is kept for rsort_multi_last_stats. Phases on the caller's stream:
 *   plan       count all-gather, sampling, sample all-gather + device sort, splitters
 *   partition  the stable partition, the count/capacity all-gather, the exchange plan
 *   exchange   every exchange round (and the own range's device copy beside it)
 *   local_sort the LSD sort of what arrived
 * With RSORT_MULTI_OVERLAP the lower half's sort runs on a second stream during the upper half's
 * exchange: `exchange` then ends when the last message has arrived and `local_sort` is the rest. */
typedef struct rsort_multi_stats {
    int32_t world;       /* ranks of the communicator (rsort_u32_multi: ncclCommCount) */
    int32_t rank;        /* this rank (rsort_u32_multi: ncclCommUserRank) */
    int32_t halves;      /* 1, or 2 when the overlap ran (RSORT_MULTI_OVERLAP, or its automatic use) */
    int32_t direct;      /* 1: world 1 without RSORT_MULTI_FULL, sorted directly (phases: local_sort) */
    int64_t rounds;      /* exchange rounds (messages per peer and array) */
    int64_t bytes_per_key; /* 4 (keys) or 8 (key + value) */
    int64_t send_keys[RSORT_MAX_RANKS]; /* keys this rank sent to each rank (own entry: the device copy) */
    int64_t recv_keys[RSORT_MAX_RANKS]; /* keys it received from each rank */
    int64_t n_in, n_out; /* keys in, keys out on this rank */
    double ms_plan, ms_partition, ms_exchange, ms_local_sort, ms_total;
} rsort_multi_stats;
RSORT_API int rsort_multi_set_profiling(int enable); /* process-wide; returns the previous setting */
/* The calling thread's last multi-GPU sort made while profiling was on (RSORT_ERR_ARG if none). */
RSORT_API int rsort_multi_last_stats(rsort_multi_stats *out);

/* TEST HOOK (fault injection for the error-agreement tests; never set in production): the next
 * multi-GPU sorts of rank `rank` fail with `status` at `stage` (1: the sample sort, after the sample
 * all-gather; 2: the partition), as a device failure there would. rank < 0 clears the hook. */
RSORT_API int rsort_multi_inject_failure(int rank, int stage, int status);

/* Largest message of one exchange round, in keys (default and maximum 2^28 = 1 GiB; >= 64).
 * Messages are cut into equal pieces of a multiple of 64 keys, never above the limit, even when it
 * is not a multiple of 64 (rsort_multi_exchange_rounds). Process-wide; returns the previous value. Tests
 * set small values to force several rounds. */
RSORT_API int64_t rsort_set_exchange_piece(int64_t keys);

/* The communication the multi-GPU sort needs, as a plug-in (RCCL is one implementation, the
 * in-process loopback below another; MPI or a host transport could be a third). Both calls are
 * made by every rank in the same order; they return 0 or a nonzero rsort_status. */
typedef struct rsort_transport {
    void *ctx;
    int32_t world, rank;
    /* every rank contributes `bytes` device bytes at d_send; d_recv (world * bytes) receives the
     * contributions in rank order. Stream-ordered on `stream` (or synchronous). */
    int (*allgather)(void *ctx, const void *d_send, void *d_recv, size_t bytes, void *stream);
    /* one round of messages: for each peer p != rank, send send_bytes[p] bytes from d_send[p] and
     * receive recv_bytes[p] bytes into d_recv[p] (0 = none; entry `rank` is always 0). */
    int (*exchange)(void *ctx, void *const *d_send, const size_t *send_bytes, void *const *d_recv,
                    const size_t *recv_bytes, void *stream);
} rsort_transport;
RSORT_API int rsort_u32_multi_transport(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n,
                                        uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t capacity,
                                        int64_t *out_n, int64_t *out_offset, int k_bits,
                                        const rsort_transport *transport, void *d_workspace,
                                        size_t workspace_bytes, void *stream);
/* A transport over HOST memory (MPI, gloo, sockets, ...), wrapped into an rsort_transport: the
 * wrapper synchronises the stream, stages the device bytes through host buffers it owns, calls
 * the host functions (same contract as rsort_transport, host pointers) and copies the results back
 * to the device. bench.py's N-rank rehearsal on one card and the gloo tests run the C protocol this
 * way; the product path on a multi-GPU node is RCCL (rsort_u32_multi). The wrapper keeps a copy of
 * *host; free it with rsort_host_transport_free after the last sort. */
typedef struct rsort_host_transport {
    void *ctx;
    int32_t world, rank;
    int (*allgather)(void *ctx, const void *h_send, void *h_recv, size_t bytes);
    int (*exchange)(void *ctx, void *const *h_send, const size_t *send_bytes, void *const *h_recv,
                    const size_t *recv_bytes);
} rsort_host_transport;
RSORT_API int rsort_host_transport_wrap(const rsort_host_transport *host, rsort_transport *out);
RSORT_API void rsort_host_transport_free(rsort_transport *wrapped);

/* In-process loopback world: `world` ranks, one host thread each, calling
 * rsort_u32_multi_transport concurrently on their own streams (one device, or devices with peer
 * access). Collectives are a host rendezvous plus device-to-device copies; a rank that waits more
 * than 120 s fails with RSORT_ERR_COMM (and so do the others). For testing the multi-GPU path on
 * one GPU (RCCL refuses two ranks on one device). */
RSORT_API int rsort_loopback_create(int world, void **group);
RSORT_API int rsort_loopback_transport(void *group, int rank, rsort_transport *out);
RSORT_API void rsort_loopback_destroy(void *group);

/* ---------------------------------------------------------------- vendor comparator */
/* rocPRIM's device radix sort (what sortByThrust resolves to on ROCm), for the
 * "vendor ceiling" column. */
RSORT_API size_t rsort_vendor_workspace_size(int64_t n);
RSORT_API int rsort_u32_vendor_device(const uint32_t *d_in, uint32_t *d_out, int64_t n,
                                      void *d_workspace, size_t workspace_bytes, void *stream);
RSORT_API int rsort_u32_vendor(const uint32_t *in, uint32_t *out, int64_t n);
/* rocPRIM's segmented radix sort over the same offsets as rsort_u32_segmented_device (keys only; the
 * offsets must be valid: rocPRIM does not check them). A comparator only. */
RSORT_API size_t rsort_vendor_segmented_workspace_size(int64_t n, int64_t num_segments);
RSORT_API int rsort_u32_vendor_segmented_device(const uint32_t *d_in, uint32_t *d_out, int64_t n,
                                                const uint32_t *d_offsets, int64_t num_segments,
                                                void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- output check */
/* d_out[0] = sum over i of fmix64(d_vals[i] << 32 | d_keys[i]) mod 2^64 (d_vals may be NULL: 0),
 * an order-independent fingerprint of the (key, value) multiset; d_out[1] = #{i : d_keys[i] >
 * d_keys[i + 1]}. A correct sort keeps d_out[0] and has d_out[1] == 0 (bench.py checks its timed
 * output this way; the parity tests compare with the oracle instead). d_out: 2 u64, device. */
RSORT_API int rsort_fingerprint_device(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n,
                                       uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------- synthetic workloads */
/* key[i] = high 32 bits of splitmix64(seed + i). */
RSORT_API int rsort_gen_uniform(uint32_t *d_out, int64_t n, uint64_t seed, void *stream);
/* key[i] = fmix32(rank), rank = lower_bound(d_cdf[0..ranks), u_i) with u_i the uniform
 * stream above; d_cdf is the inclusive Zipf CDF scaled to u32 (last entry 2^32-1). */
RSORT_API int rsort_gen_zipf(uint32_t *d_out, int64_t n, uint64_t seed, const uint32_t *d_cdf,
                             int64_t ranks, void *stream);
/* d_out[i] = base + i */
RSORT_API int rsort_gen_iota(uint32_t *d_out, int64_t n, uint32_t base, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RSORT_H_ */

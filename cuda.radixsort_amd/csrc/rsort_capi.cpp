// rsort_capi.cpp -- host driver + C ABI (include/rsort.h) of the gfx950 LSD radix sort.
//
// Replaces the reference's per-digit driver sortByDevice (Parallel7.cu:530-639) and the
// dispatcher's device branch (Parallel7.cu:641-662). Differences by design:
//   * workspace is planned once (rsort_plan) and passed in, not cudaMalloc'ed per call or
//     kept in function statics (P7:203-218, :489-505); the host entry caches one per device;
//   * one stream, no host synchronisation inside the pass loop (P7 syncs after every launch
//     and round-trips the block sums through the host every pass, P7:224-235, :514-519);
//   * errors are returned as rsort_status, never exit() (common.h:6-16).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "rsort.h"
#include "rsort_internal.hpp"

using namespace rsort;

namespace {

constexpr int kVersion = 100;  // 0.1.0
std::atomic<int> g_rank_algo{RSORT_RANK_MATCH};
std::atomic<int> g_group_chunks{1};
std::atomic<int> g_table_fault{0};  // rsort_inject_table_fault (tests)
std::atomic<int> g_rank_fault{0};   // rsort_inject_rank_fault (tests)
// rsort_inject_fault_window (tests): which of the calling thread's sort calls (entries into sort_planned, numbered
// from 0 since the window was set) see the two hooks above; count < 0: no window, every one does
struct FaultWindow {
    int64_t first = 0, count = -1, started = 0;
};
thread_local FaultWindow t_fault_window;
// numbers this sort call; true when the hooks apply to it
bool fault_window_admits() {
    FaultWindow &w = t_fault_window;
    const int64_t i = w.started++;
    return w.count < 0 || (i >= w.first && i - w.first < w.count);
}
// the rank hook for what is no sort call (the partition's scatter, a single pass, the segmented sort): in no
// window, so it applies only while the calling thread has none
uint32_t rank_fault_unnumbered() { return (t_fault_window.count < 0 && g_rank_fault.load()) ? 1u : 0u; }
std::atomic<int> g_hybrid{RSORT_HYBRID_AUTO};  // rsort_set_hybrid
std::atomic<int> g_seg_grid_limit{0};  // rsort_set_segmented_grid_limit (tests); 0: no limit

// Hybrid-eligible sorts enqueue both kernel sequences; every launch carries the device-side mode word and the
// value it works under (HistArgs::mode). {nullptr, 0}: no test.
struct Gate {
    const uint32_t *mode = nullptr;
    uint32_t want = 0;
};

// ------------------------------------------------------------------------------ profiler
struct ProfRec {
    int phase;
    int64_t keys;
    hipEvent_t a, b;
    Gate gate;  // a launch of a hybrid-eligible sort: counted only if its route ran (rsort_profile_end)
};

struct Profiler {
    std::mutex mu;
    bool on = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;

    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};
Profiler g_prof;
thread_local int t_prof_paused = 0;  // profile_pause

// RAII scope: records a start event now and a stop event on destruction (same stream).
struct PhaseScope {
    bool active = false;
    ProfRec rec{};
    hipStream_t s;
    PhaseScope(int phase, int64_t keys, hipStream_t stream, Gate gate = Gate{}) : s(stream) {
        if (t_prof_paused > 0) return;
        std::lock_guard<std::mutex> g(g_prof.mu);
        if (!g_prof.on) return;
        rec.phase = phase;
        rec.keys = keys;
        rec.gate = gate;
        rec.a = g_prof.get();
        rec.b = g_prof.get();
        if (!rec.a || !rec.b) return;
        if (hipEventRecord(rec.a, s) != hipSuccess) return;
        active = true;
    }
    ~PhaseScope() {
        if (!active) return;
        std::lock_guard<std::mutex> g(g_prof.mu);
        if (hipEventRecord(rec.b, s) == hipSuccess) g_prof.recs.push_back(rec);
    }
};

bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

bool have_device() {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess && count > 0;
}

// The whole-line scatter kernels can write these outputs: any 4-B-aligned kout (launch_scatter
// counts positions from its 128-B-aligned base, i.e. every position moves up by the < 32 keys
// between that base and kout -- so n plus that shift must still fit the kernels' 32-bit positions);
// values at a multiple of 16 B from the keys.
bool line_capable(const void *kout, const void *vout, int pairs, int64_t n) {
    if (!aligned4(kout)) return false;
    if (n + (int64_t)(((uintptr_t)kout & 127u) / 4u) >= ((int64_t)1 << 32)) return false;
    return !pairs || ((((uintptr_t)vout - (uintptr_t)kout) & 15u) == 0);
}

// ------------------------------------------------------------------------------ planning
int device_cus() {
    int dev = 0, c = 0;
    if (!have_device()) return 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return c;
}

// The planning and route lab switches (A/B runs under RSORT_LAB=1: lab_env), read once.
struct Lab {
    // log2 of the smallest k = 4 keys-only sort on 1024-thread line tiles
    int k4_lines_lg = (int)lab_int("RSORT_K4_LINES_LG", 16, 32, 28);
    // 0: cut plans with equal key counts per chunk
    bool cut_weights = lab_flag("RSORT_CUT_WEIGHTS", true);
    // 0: cut plans count all their pieces from the keys (no per-chunk joint-count rows; the round-4 scheme)
    bool piece_rows = lab_flag("RSORT_PIECE_ROWS", true);
    // 1: next-digit plans scan each pass's table in its last workgroup (the round-3 scheme) instead of every
    // workgroup of the next pass summing the raw counts
    bool nx_tail = lab_flag("RSORT_NX_TAIL", false);
};
const Lab &lab() {
    static const Lab v;
    return v;
}

// Tile geometry for one sort: for k = 5..8, keys-only sorts write whole 64-B lines from
// 16384-key tiles (rs_scatter_lines), pairs from 8192-key tiles; k <= 4 keys
// use 8192-key tiles; everything else 4096-key tiles -- as do inputs too small to give every
// CU two large tiles.
int choose_geom(int64_t n, int k, int pairs, int rank, int partition, int cus) {
    const int64_t enough = 2 * (int64_t)(cus > 0 ? cus : 256);
    // partitions: 4096-key tiles (measured at 2^30 keys into 8 ranges: 1024-thread 16384-key
    // tiles need 4-bit bucket digits, i.e. 15 splitter compares per key, and were 1.3x slower)
    if (k >= 13) return kGeomXL;
    // keys-only partitions of large inputs: 8192-key tiles of 512 threads (3-bit bucket digits keep
    // a digit's thread group inside one wave; runs of ~1024 keys per bucket and tile)
    if (partition && !pairs && n >= enough * geom_tile_keys(kGeomK4)) return kGeomK4;
    if (partition || rank == RSORT_RANK_SPLIT) return kGeomSmall;
    if (k >= 5 && k <= 8 && !pairs && n >= enough * geom_tile_keys(kGeomLines)) return kGeomLines;
    // k = 4 keys from 2^28 on: the same 1024-thread line tiles (dev/scatter_lab LAB_K4 at 2^30:
    // 1.61 ms per pass against 1.75 ms with 4096-key tiles; at 2^26 0.120 against 0.113)
    if (k == 4 && !pairs && n >= ((int64_t)1 << lab().k4_lines_lg)) return kGeomLines;
    if (k >= 5 && k <= 8 && pairs && n >= enough * geom_tile_keys(kGeomLinesPairs)) return kGeomLinesPairs;
    // k = 3, 4 keys run 4096-key tiles through rs_scatter_lines (kGeomSmall's shape; whole 128-B
    // lines: 2^26 keys, k = 4: 0.117 vs 0.144 ms per pass, dev/scatter_lab.hip); k <= 2 keeps
    // rs_scatter's 8192-key tiles
    if (k <= 2 && !pairs && n >= enough * geom_tile_keys(kGeomK4)) return kGeomK4;
    return kGeomSmall;
}

// Digit-group chunks (rs_histogram_joint, rsort_kernels.hip): k = 8 plans with exactly 2^8
// chunks of line tiles. Every second pass then reads no keys for its histogram.
bool joint_plan(const rsort_plan &p) {
    return p.k_bits == kJointBits && p.num_chunks == (int64_t)kJointBins && p.passes >= 2 &&
           (geom_from_shape(p.threads, p.tile_keys, p.pairs) == (p.pairs ? kGeomLinesPairs : kGeomLines));
}

// Next-digit counts (rs_scatter_lines, k = 3, 4 keys): each pass adds the next pass's chunk table
// from where it writes every key, so only pass 0 reads keys for a histogram. Needs the line
// kernel (lane-ordered ranks, line-capable outputs: checked per sort) and a second table.
bool next_plan(const rsort_plan &p) {
    const int g = geom_from_shape(p.threads, p.tile_keys, p.pairs);
    return (p.k_bits == 3 || p.k_bits == 4) && !p.pairs && p.passes >= 2 && (g == kGeomSmall || g == kGeomLines);
}

// The workspace of a plan: THE statement of its layout (DESIGN §3 "Workspace state"). One walk gives every
// region's pointer (nullptr where ws is: sizing) and the total, rsort_plan::workspace_bytes.
struct Carve {
    uint32_t *tmp_k, *tmp_v;  // ping-pong keys (and values)
    uint32_t *table, *bsums;  // chunk x digit table, scan block sums
    uint32_t *starts;         // bucket starts (partition / top histogram)
    uint32_t *done;           // check words (tail-scan counter, check word, hybrid report: kDoneErr, kHyb*)
    // digit-group plans (kJointRegionBytes; rows_cnt: the word behind the joint counts, cleared with them)
    uint32_t *joint, *rows_cnt, *bounds, *plan, *pcounts, *rows;
    uint32_t *table2, *table3;  // next-digit SORT plans: the next pass's table, the third of a raw-table rotation
    size_t bytes;
};

Carve carve(const rsort_plan &p, void *ws, bool partition = false) {
    Carve c{};
    Bump b(ws);
    const size_t keys = (size_t)p.n * 4, table = (size_t)p.table_entries * 4;
    c.tmp_k = b.take(keys);
    if (p.pairs) c.tmp_v = b.take(keys);
    c.table = b.take(table);
    c.bsums = b.take((size_t)p.scan_blocks * 4);
    c.starts = b.take((size_t)(p.bins + 1) * 4);
    c.done = b.take(256);
    if (joint_plan(p)) {
        uint32_t **const region[] = {&c.joint, &c.bounds, &c.plan, &c.pcounts, &c.rows};
        static_assert(sizeof(region) / sizeof(region[0]) == sizeof(kJointRegionBytes) / sizeof(kJointRegionBytes[0]), "");
        for (size_t i = 0; i < sizeof(region) / sizeof(region[0]); ++i) *region[i] = b.take(kJointRegionBytes[i]);
        if (c.joint) c.rows_cnt = c.joint + kJointBins * kJointBins;
    }
    if (!partition && next_plan(p)) {
        c.table2 = b.take(table);
        c.table3 = b.take(table);
    }
    c.bytes = b.off;
    return c;
}

int plan_fill(int64_t n, int k, int pairs, int64_t tpc, rsort_plan *p, int partition = 0) {
    if (!p) return RSORT_ERR_ARG;
    if (k < kMinBits || k > kMaxBits) return RSORT_ERR_BITS;
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    if (tpc < 0) return RSORT_ERR_ARG;
    memset(p, 0, sizeof(*p));
    const int rank = g_rank_algo.load();
    const int cus = device_cus();
    const int geom = choose_geom(n, k, pairs, rank, partition, cus);
    const int tile = geom_tile_keys(geom);
    p->n = n;
    p->k_bits = k;
    p->passes = (32 + k - 1) / k;
    p->bins = 1 << k;
    p->threads = kGeomShape[geom].threads;
    p->tile_keys = tile;
    p->pairs = pairs ? 1 : 0;
    const int64_t tiles = std::max<int64_t>(1, (n + tile - 1) / tile);
    if (tpc == 0) {
        // one resident wave of workgroups: as many chunks as the scatter kernel keeps resident
        // (of the kernel this plan's scatter runs: a partition's digit is a bucket)
        int bpc = cus > 0 ? scatter_blocks_per_cu(k, pairs, internal_rank(partition ? RSORT_RANK_MATCH : rank), geom,
                                                  partition ? kDigitSplit : kDigitShift) : 0;
        if (bpc <= 0) bpc = 2;
        const int64_t target = std::max<int64_t>(1, (int64_t)(cus > 0 ? cus : 256) * bpc);
        tpc = (tiles + target - 1) / target;
    }
    p->tiles_per_chunk = tpc;
    p->chunk_keys = tpc * tile;
    p->num_chunks = (tiles + tpc - 1) / tpc;
    p->table_entries = (int64_t)p->bins * p->num_chunks;
    p->scan_blocks = (p->table_entries + kScanSegment - 1) / kScanSegment;
    p->workspace_bytes = carve(*p, nullptr, partition).bytes;
    return RSORT_OK;
}

// Digit bits of a partition of n keys into num_buckets key ranges: enough for the buckets, and
// enough that the whole-line scatter kernel of the partition's tile shape (choose_geom) gives
// each digit at most one wave of threads.
int partition_bits(int64_t n, int num_buckets, int pairs) {
    const int geom = choose_geom(n, 0, pairs, RSORT_RANK_MATCH, 1, device_cus());
    int bits = 1;
    while ((1 << bits) < num_buckets || (kGeomShape[geom].threads >> bits) > kWave) ++bits;
    return bits;
}

// ------------------------------------------------------------------------------ pass pieces
// A launch = a builder (what every launch of the plan shares) + the optional fields its caller sets by name + a
// runner (the launch-time decisions and the profiler's phase scope; the gate is the struct's own mode / mode_want).
struct PassIo {
    const uint32_t *kin, *vin;
    uint32_t *kout, *vout;
};

HistArgs hist_args(const rsort_plan &p, const uint32_t *keys, int shift, uint32_t *table) {
    HistArgs a{};
    a.keys = keys;
    a.table = table;
    a.n = (uint64_t)p.n;
    a.chunk_keys = (uint64_t)p.chunk_keys;
    a.num_chunks = (uint32_t)p.num_chunks;
    a.shift = (uint32_t)shift;
    a.vec = (((uintptr_t)keys & 15u) == 0) ? 1u : 0u;
    a.split = 1;
    return a;
}

ScanArgs scan_args(const rsort_plan &p, uint32_t *table, uint32_t *bsums) {
    ScanArgs a{};
    a.table = table;
    a.block_sums = bsums;
    a.m = (uint64_t)p.table_entries;
    a.nblocks = (uint32_t)p.scan_blocks;
    return a;
}

ScatterArgs scatter_args(const rsort_plan &p, const PassIo &io, int shift, const uint32_t *table) {
    ScatterArgs a{};
    a.kin = io.kin;
    a.vin = io.vin;
    a.kout = io.kout;
    a.vout = io.vout;
    a.table = table;
    a.n = (uint64_t)p.n;
    a.chunk_keys = (uint64_t)p.chunk_keys;
    a.num_chunks = (uint32_t)p.num_chunks;
    a.shift = (uint32_t)shift;
    a.rank_fault = rank_fault_unnumbered();  // (a sort's passes take their sort call's: SortCtx::scatter)
    return a;
}

// a launch of a hybrid-eligible sort: works only while *g.mode == g.want (HistArgs::mode)
template <class Args>
Args gated(Args a, Gate g) {
    a.mode = g.mode;
    a.mode_want = g.want;
    return a;
}

int run_histogram(const rsort_plan &p, HistArgs a, int dmode, hipStream_t s) {
    if (a.zero) a.zero_n = (uint64_t)p.table_entries;
    // few, long chunks (one scatter workgroup per CU): several histogram workgroups per chunk,
    // their counts added into a zeroed table
    const int cus = device_cus();
    const int64_t want = 4 * (int64_t)(cus > 0 ? cus : 256);  // 1024-thread workgroups (hist_bits)
    if (a.bounds != nullptr) {
        // a digit-group pass (256 chunks of one workgroup each): copies the joint counts, counts the
        // cut plan's pieces, or counts one chunk per 1024-thread workgroup (as fast as split
        // workgroups, 0.62 ms per 2^30 keys, and no table memset launch)
        a.wide = 1;
    } else if (p.num_chunks < want && p.chunk_keys >= 8 * 4096) {
        a.split = (uint32_t)std::min<int64_t>({(want + p.num_chunks - 1) / p.num_chunks, p.chunk_keys / 4096, 64});
    }
    PhaseScope ps(RSORT_PHASE_HISTOGRAM, p.n, s, Gate{a.mode, a.mode_want});
    if (a.split > 1 && hipMemsetAsync(a.table, 0, (size_t)p.table_entries * 4, s) != hipSuccess) return RSORT_ERR_HIP;
    return hip_status(launch_histogram(p.k_bits, dmode, a, s));
}

// Joint pass (pass p of a joint_plan counting for pass p + 1; a.joint set): one workgroup per chunk counts
// this pass's table and the joint counts. a.joint_enable: nullptr, or the previous odd pass's mode: the joint count
// runs after whole digit groups and after a cut plan (both leave the joint counts cleared: the copy-mode histogram,
// the cut plan's scan), not after fixed chunks. After a cut plan the input is clustered: the joint count
// adds runs of equal pairs once (rs_histogram's run path), so pass 3 gets its own cut plan too.
int run_histogram_joint(const rsort_plan &p, const HistArgs &a, bool zero_joint, hipStream_t s) {
    PhaseScope ps(RSORT_PHASE_HISTOGRAM, p.n, s, Gate{a.mode, a.mode_want});
    // the first joint count of a sort clears the counts; a later one finds them cleared by the
    // copy-mode histogram that used them (or, where that pass fell back, is disabled by joint_enable)
    // (the rows counter sits after the joint counts: cleared with them)
    // (16 bytes past the counts, inside the 256-B-aligned region: a fill of a multiple of 16 bytes is one
    // kernel, the 4-byte tail of an odd size was a second one, ~5 us per sort)
    if (zero_joint && hipMemsetAsync(a.joint, 0, (size_t)kJointBins * kJointBins * 4 + 16, s) != hipSuccess)
        return RSORT_ERR_HIP;
    return hip_status(launch_histogram_joint(a, s));
}

// The next pass's chunks from the joint counts (rs_joint_bounds), after this pass's table is scanned
// (a.ctab: a cut plan's pieces become row tasks where every chunk wrote its rows).
int run_joint_bounds(const rsort_plan &p, JointBoundsArgs a, hipStream_t s) {
    a.n = (uint64_t)p.n;
    // a group may take one tile more than a fixed chunk; a cut-plan chunk boundary moves to a
    // group boundary up to half a tile (and a quarter chunk) away
    a.max_keys = (uint64_t)p.chunk_keys + (uint64_t)p.tile_keys;
    a.snap = (uint32_t)std::min<int64_t>(p.tile_keys / 2, p.n / (4 * (int64_t)kJointBins));
    // the first cut plan of a sort (pass 1's, from pass 0's joint counts) balances estimated cost
    // (rs_joint_bounds; RSORT_CUT_WEIGHTS=0 turns it off for A/B runs)
    a.weighted = (a.enable == nullptr && lab().cut_weights) ? 1u : 0u;
    PhaseScope ps(RSORT_PHASE_HISTOGRAM, p.n, s, Gate{a.mode, a.mode_want});
    return hip_status(launch_joint_bounds(a, s));
}

int run_scan(const rsort_plan &p, ScanArgs a, hipStream_t s) {
    if (a.zero) a.zero_n = (uint64_t)p.table_entries;
    PhaseScope ps(RSORT_PHASE_SCAN, p.table_entries, s, Gate{a.mode, a.mode_want});
    return hip_status(launch_scan(a, s));
}

int run_scatter(const rsort_plan &p, const ScatterArgs &a, int dmode, hipStream_t s) {
    const int rank = internal_rank((dmode == kDigitShift) ? g_rank_algo.load() : RSORT_RANK_MATCH);
    const int geom = geom_from_shape(p.threads, p.tile_keys, p.pairs);
    if (!scatter_available(p.k_bits, p.pairs, rank, dmode, geom)) return RSORT_ERR_ARG;
    const int aligned16 = line_capable(a.kout, a.vout, p.pairs, p.n);
    if ((a.bounds || a.next_table || a.raw_table) &&
        !(rank == kRankAtomic && aligned16 && !a.local_only && dmode == kDigitShift))
        return RSORT_ERR_ARG;  // group chunks, next-digit counts, raw tables: rs_scatter_lines only
    // a multi-GPU partition's scatter (splitter digits) is recorded apart from the sort's passes
    PhaseScope ps(dmode == kDigitSplit ? RSORT_PHASE_PARTITION : RSORT_PHASE_SCATTER, p.n, s, Gate{a.mode, a.mode_want});
    return hip_status(launch_scatter(p.k_bits, p.pairs, rank, dmode, geom, a.local_only ? 0 : aligned16, a, s));
}

int check_plan(const rsort_plan *p) {
    if (!p) return RSORT_ERR_ARG;
    if (p->k_bits < kMinBits || p->k_bits > kMaxBits) return RSORT_ERR_BITS;
    if (!key_count_ok(p->n)) return RSORT_ERR_SIZE;
    // the tile shape must be one a kernel of this digit width exists for (keys or pairs): a plan is the planner's,
    // or a hand-made one that could be, never a shape that would only fail at its first launch
    const int geom = geom_from_shape(p->threads, p->tile_keys, p->pairs);
    if (geom < 0 || !scatter_shape_available(p->k_bits, p->pairs ? 1 : 0, geom)) return RSORT_ERR_ARG;
    if (p->tiles_per_chunk <= 0 || p->num_chunks <= 0 ||
        p->num_chunks * p->tiles_per_chunk * p->tile_keys < p->n ||
        p->chunk_keys != p->tiles_per_chunk * p->tile_keys || p->bins != (1 << p->k_bits) ||
        p->table_entries != (int64_t)p->bins * p->num_chunks)
        return RSORT_ERR_ARG;
    return RSORT_OK;
}

// ------------------------------------------------------------------------------ hybrid route
// (rsort_hybrid.hip.) The automatic n range: from kHybMinKeys (measured: DESIGN §3, profiles/hybrid_ab.json;
// RSORT_HYB_MIN_KEYS under RSORT_LAB=1 for A/B runs) up to where the MEAN bucket n / 65536 reaches the capacity.
// The bucket phase pays a fixed cost per bucket (65536 buckets whatever n), which two resident workgroups per CU
// overlap: the route now wins at every measured size -- 2^28 keys 2.17 against 2.27 ms (-4.5 %), 2^29 3.44 against
// 4.15 (-17 %), 3 x 2^28 4.80 against 6.16 (-22 %), 7 x 2^27 5.48 against 7.13 (-23 %). The range starts at the
// smallest size measured (tests/test_hybrid.py keeps it above 2^27, where the digit-group tests pin the LSD passes).
constexpr int64_t kHybMinKeys = (int64_t)1 << 28;
constexpr int64_t kHybMaxKeys = (int64_t)kHybCapacity * kHybBuckets;
int64_t hyb_min_keys() {
    static const int64_t v = lab_int("RSORT_HYB_MIN_KEYS", 1, ((long long)1 << 32) - 1, kHybMinKeys);
    return v;
}

// Bucket-kernel workgroups per resident slot (grid-stride over the buckets; a workgroup that ends early leaves its
// slot to a fresh one instead of the slowest deciding). 2^30 uniform keys, two resident workgroups per CU, same-box
// bench runs: 6.52 ms with 1, 6.41 with 2, 6.33 with 4, 6.28 with 8 and with 16, 6.40 with 32 (DESIGN §3 "Hybrid
// route"; RSORT_HYB_GRID_MULT under RSORT_LAB=1 for A/B runs).
constexpr int kHybGridMult = 8;

// The sample gate's threshold. Each of the gate's kHybGateGroups workgroups reads m = min(n, kHybSample) /
// kHybGateGroups keys at a fixed stride over its part of the input and counts them by their top 16 bits. A bucket
// the hybrid can still hold has at most kHybCapacity of the n keys, so its count in one workgroup is (for keys
// whose value does not depend on their position) at most Poisson with lambda = m * capacity / n: 0.0176 at 2^30
// keys, 0.0234 at 3 x 2^28. The threshold is the smallest T with 65536 buckets x 64 workgroups x
// P(Poisson(lambda) >= T) < 1e-9 -- no acceptable input, uniform keys (lambda = m / 65536) least of all, reaches
// it in a billion sorts: T = 7 of 1024 keys at 2^30. A bucket that does reach it holds ~0.7 % of a 64th of the
// input, hundreds of times the capacity's share: Zipf and hot keys (shares of 7 % and 25 %), all-equal and
// small-integer keys (every key in one bucket). Inputs skewed less than that -- and inputs whose parts are each
// clustered in a few buckets the gate may call skewed although the whole is balanced: they take the LSD passes --
// pass the gate and are decided by the exact count, for one extra histogram read.
// (tail bound: P(X >= k) <= pmf(k) / (1 - lambda / (k + 1)) for k + 1 > lambda)
uint32_t gate_threshold(int64_t n) {
    const double m = (double)std::min<int64_t>(n, kHybSample) / (double)kHybGateGroups;
    const double lam = m * std::max(1.0 / (double)kHybBuckets, (double)kHybCapacity / (double)std::max<int64_t>(n, 1));
    double lp = -lam;  // log pmf(0)
    for (uint32_t k = 0; k < 65535u; ++k) {
        if ((double)(k + 1) > lam) {
            const double tail = exp(lp) / (1.0 - lam / (double)(k + 1));
            if (tail * (double)kHybBuckets * (double)kHybGateGroups < 1e-9) return std::max(k, 2u);
        }
        lp += log(lam) - log((double)(k + 1));
    }
    return 65535u;
}

// Whether a sort takes the hybrid route's launches (the device still decides): keys only, k = 8, a joint plan on
// the digit-group path (lane-ordered ranks, both outputs line-capable: `joint`), in != out, n in the range.
bool hybrid_eligible(const rsort_plan &p, bool joint, bool inplace, bool allow) {
    const int hm = g_hybrid.load();
    if (!allow || hm == RSORT_HYBRID_OFF || !joint || p.pairs || inplace || p.passes != 4) return false;
    if (hm == RSORT_HYBRID_FORCE) return true;
    return p.n >= hyb_min_keys() && p.n <= kHybMaxKeys;
}

// What the pass loops of one sort share. Every LSD launch carries the gate `lsd` ({}: not hybrid-eligible) and
// every scatter the check word; pass i reads (sk, sv) and the last pass lands in (kout, vout).
struct SortCtx {
    const rsort_plan &p;
    const Carve c;
    hipStream_t s;
    Gate lsd;
    const uint32_t *sk, *sv;
    uint32_t *kout, *vout;
    uint32_t rank_fault;  // the test hooks, as this sort call sees them (rsort_inject_fault_window)
    bool table_fault;

    HistArgs hist(int i, uint32_t *table) const { return gated(hist_args(p, sk, i * p.k_bits, table), lsd); }
    ScanArgs scan(uint32_t *table) const { return gated(scan_args(p, table, c.bsums), lsd); }
    ScatterArgs scatter(int i, const uint32_t *table) const {
        const bool to_out = ((p.passes - 1 - i) % 2) == 0;
        const PassIo io{sk, sv, to_out ? kout : c.tmp_k, to_out ? vout : c.tmp_v};
        ScatterArgs a = gated(scatter_args(p, io, i * p.k_bits, table), lsd);
        a.check = c.done + kDoneErr;
        a.rank_fault = rank_fault;
        return a;
    }
    // runs a pass's scatter; what it wrote is the next pass's input
    int run_pass(const ScatterArgs &a) {
        const int st = run_scatter(p, a, kDigitShift, s);
        sk = a.kout;
        sv = a.vout;
        return st;
    }
    int hybrid_prologue();
    int plain_passes();
    int group_passes(bool hyb);
    int next_digit_passes(bool rawt);
};

// Hybrid route (not in place: sk is the sort's input): gate, joint count of (digit 3, digit 2), mode + bucket
// starts, pass A in -> out, pass B out -> tmp, bucket phase tmp -> out; then the LSD passes (gated by `lsd` from
// here on), which run when the mode word says so. Every kernel of the unselected route leaves at once.
int SortCtx::hybrid_prologue() {
    int st;
    const bool force = g_hybrid.load() == RSORT_HYBRID_FORCE;
    const Gate run{c.done + kHybMode, kHybRun};
    lsd = Gate{c.done + kHybMode, kHybLsd};
    uint32_t *hb = c.plan;  // pass B's chunks (the cut-plan area: the LSD passes use it only when they run)
    HybArgs h{};
    h.kin = sk;
    h.kout = kout;
    h.joint = c.joint;
    h.bounds = hb;
    h.gflags = c.bounds;
    h.done = c.done;
    h.n = (uint64_t)p.n;
    h.threshold = gate_threshold(p.n);
    h.force = force ? 1u : 0u;
    h.rank_fault = rank_fault;
    hyb_note_bucket();
    {
        // the one clear of the joint counts, with the rows counter and the gate's flag behind them: the LSD
        // passes find them cleared -- never counted after a skewed verdict, cleared again by rs_hyb_bounds
        // after an overflow
        PhaseScope ps(RSORT_PHASE_HISTOGRAM, std::min<int64_t>(p.n, kHybSample), s);
        if (hipMemsetAsync(c.joint, 0, (size_t)kJointBins * kJointBins * 4 + 16, s) != hipSuccess) return RSORT_ERR_HIP;
        if ((st = hip_status(launch_hyb_gate(h, s)))) return st;
    }
    // the joint count runs when the gate's flag stayed 0 (FORCE: always)
    HistArgs jc = gated(hist_args(p, sk, 24, c.table), force ? Gate{} : Gate{c.joint + kHybGateFlag, 0u});
    jc.joint = c.joint;
    jc.shift2 = 16;
    if ((st = run_histogram_joint(p, jc, false, s))) return st;
    {
        PhaseScope ps(RSORT_PHASE_HISTOGRAM, p.n, s);
        if ((st = hip_status(launch_hyb_bounds(h, s)))) return st;
    }
    if ((st = run_scan(p, gated(scan_args(p, c.table, c.bsums), run), s))) return st;
    ScatterArgs pa = gated(scatter_args(p, PassIo{sk, nullptr, kout, nullptr}, 24, c.table), run);
    pa.check = c.done + kDoneErr;
    pa.rank_fault = rank_fault;
    if ((st = run_scatter(p, pa, kDigitShift, s))) return st;
    ScatterArgs pb = gated(scatter_args(p, PassIo{kout, nullptr, c.tmp_k, nullptr}, 16, c.joint), run);
    pb.bounds = hb;
    pb.check = c.done + kDoneErr;
    pb.rank_fault = rank_fault;
    if ((st = run_scatter(p, pb, kDigitShift, s))) return st;
    const int cus = std::max(1, device_cus());
    const int bpc = std::max(1, hyb_blocks_per_cu());
    static const int mult = (int)lab_int("RSORT_HYB_GRID_MULT", 1, 256, kHybGridMult);
    const uint32_t grid = (uint32_t)std::min<int64_t>(kHybBuckets, (int64_t)cus * bpc * mult);
    h.kin = c.tmp_k;
    PhaseScope ps(RSORT_PHASE_SCATTER, p.n, s, run);
    return hip_status(launch_hyb_bucket(h, grid, s));
}

// Plain LSD passes: histogram, scan, scatter.
int SortCtx::plain_passes() {
    int st;
    for (int i = 0; i < p.passes; ++i) {
        HistArgs h = hist(i, c.table);
        if (i == 0) h.done = c.done;  // pass 0's histogram clears the check words (rsort_plan_check: a clean record)
        if ((st = run_histogram(p, h, kDigitShift, s))) return st;
        if ((st = run_scan(p, scan(c.table), s))) return st;
        if ((st = run_pass(scatter(i, c.table)))) return st;
    }
    return RSORT_OK;
}

// Digit-group chunks (joint_plan: k = 8, four passes): two pairs of passes. The even pass of a pair counts, with
// its own table, the joint counts of (its digit, the next); rs_joint_bounds makes the odd pass's chunks of them
// (`bounds`: whole digit groups or a cut plan), and the odd pass then reads no keys for its histogram.
// hyb: the hybrid prologue ran (it cleared the check words and the joint counts).
int SortCtx::group_passes(bool hyb) {
    uint32_t *const rows = lab().piece_rows ? c.rows : nullptr, *const rows_cnt = rows ? c.rows_cnt : nullptr;
    int st;
    for (int g = 0; g < p.passes / 2; ++g) {
        uint32_t *const bounds = c.bounds + g * kBoundsWords;                    // this pair's chunks
        const uint32_t *const prev = g > 0 ? bounds - kBoundsWords : nullptr;    // the pair's before
        int i = 2 * g;
        // even pass: the joint count (after a pair that fell back to fixed chunks: off), the table's scan, the
        // next pass's chunks (after the scan: a cut plan finds the previous chunks' positions in it)
        HistArgs jc = hist(i, c.table);
        jc.joint = c.joint;
        jc.joint_enable = prev;
        jc.rows = rows;
        jc.rows_cnt = rows_cnt;
        if (i == 0 && !hyb) jc.done = c.done;  // pass 0's histogram clears the check words
        if ((st = run_histogram_joint(p, jc, /*zero_joint=*/i == 0 && !hyb, s))) return st;
        if ((st = run_scan(p, scan(c.table), s))) return st;
        JointBoundsArgs jb = gated(JointBoundsArgs{}, lsd);
        jb.joint = c.joint;
        jb.enable = prev;
        jb.bounds = bounds;
        jb.plan = c.plan;
        jb.pcounts = c.pcounts;
        jb.ctab = c.table;
        jb.rows_cnt = rows_cnt;
        jb.rowone = rows ? rows + kRowsWords : nullptr;
        if ((st = run_joint_bounds(p, jb, s))) return st;
        // passes after the first: where the previous odd pass's groups were unbalanced (skewed, duplicate-heavy
        // keys: runs of equal keys in this pass's input), the clustered-input kernel runs (rank_add_hot), else
        // the plain one -- chosen on the device
        ScatterArgs even = scatter(i, c.table);
        even.cl_select = prev;
        if ((st = run_pass(even))) return st;

        // odd pass: the table is the joint counts (copied), or assembled by the scan from the cut plan's pieces
        i = 2 * g + 1;
        HistArgs h = hist(i, c.table);
        h.bounds = bounds;
        h.copy_src = c.joint;
        h.plan = c.plan;
        h.pcounts = c.pcounts;
        h.rows = rows;
        if ((st = run_histogram(p, h, kDigitShift, s))) return st;
        ScanArgs sc = scan(c.table);
        sc.group_flag = bounds;
        sc.joint = c.joint;
        sc.plan = c.plan;
        sc.pcounts = c.pcounts;
        if ((st = run_scan(p, sc, s))) return st;
        ScatterArgs odd = scatter(i, c.table);
        odd.bounds = bounds;
        odd.cl_select = bounds;
        if ((st = run_pass(odd))) return st;
    }
    return RSORT_OK;
}

// Next-digit counts (next_plan: k = 3, 4 keys): only pass 0 reads keys for a histogram; every pass adds the next
// pass's table from where it writes each key. Pass i reads `tab` and adds into `nxt`. Tail scans alternate two
// tables: the workgroup of pass i that finishes last scans nxt and clears tab. Raw tables (rawt) rotate three: every
// workgroup of a pass derives its offsets from the raw counts, and clears its part of `clr` for the pass after next.
int SortCtx::next_digit_passes(bool rawt) {
    const int P = p.passes, tables = rawt ? 3 : 2;
    uint32_t *const rot[3] = {c.table, c.table2, c.table3};
    int st;
    for (int i = 0; i < P; ++i) {
        uint32_t *const tab = rot[i % tables];
        uint32_t *const nxt = i + 1 < P ? rot[(i + 1) % tables] : nullptr;
        uint32_t *const clr = (rawt && i + 2 < P) ? rot[(i + 2) % tables] : nullptr;
        if (i == 0) {
            // pass 0's table is counted from the keys (its histogram clears the check words and, raw tables, nxt)
            // and, tail scans, scanned by launches, which also clear nxt and arm the tail counter
            HistArgs h = hist(0, tab);
            h.done = c.done;
            if (rawt) h.zero = nxt;
            if ((st = run_histogram(p, h, kDigitShift, s))) return st;
            if (!rawt) {
                ScanArgs sc = scan(tab);
                sc.zero = nxt;
                sc.done = c.done;
                if ((st = run_scan(p, sc, s))) return st;
            }
        }
        ScatterArgs a = scatter(i, tab);
        a.next_table = nxt;
        a.raw_table = rawt ? 1u : 0u;
        a.zero_table = clr;
        if (nxt && !rawt) a.tail_zero = tab;
        if (nxt || rawt) a.done = c.done;
        if ((st = run_pass(a))) return st;
        // test hook: corrupt the raw table pass 1 reads (its total is then not n: every pass-1 workgroup
        // writes nothing and records the failure for rsort_plan_check / RSORT_ERR_CHECK)
        if (i == 0 && rawt && nxt && table_fault &&
            hipMemsetD32Async((hipDeviceptr_t)nxt, 0xFFFFFFFFu, 1, s) != hipSuccess)
            return RSORT_ERR_HIP;
    }
    return RSORT_OK;
}

int sort_planned(const rsort_plan &p, const uint32_t *kin, const uint32_t *vin, uint32_t *kout,
                 uint32_t *vout, void *ws, size_t wsb, hipStream_t s, bool allow_hybrid = true) {
    const bool faults = fault_window_admits();  // (every entry is a numbered sort call, whatever it then does)
    int st = check_plan(&p);
    if (st) return st;
    if (p.n == 0) return RSORT_OK;
    if (!kin || !kout || !ws || (p.pairs && (!vin || !vout))) return RSORT_ERR_ARG;
    if (!aligned4(kin) || !aligned4(kout) || (p.pairs && (!aligned4(vin) || !aligned4(vout))))
        return RSORT_ERR_ALIGN;
    if (wsb < p.workspace_bytes) return RSORT_ERR_WORKSPACE;
    SortCtx x{p, carve(p, ws), s, Gate{}, kin, vin, kout, vout,
              (faults && g_rank_fault.load()) ? 1u : 0u, faults && g_table_fault.load() != 0};
    const Carve &c = x.c;
    const bool inplace = (kin == kout) || (p.pairs && vin == vout);
    if (inplace && (p.passes % 2 == 1)) {
        // pass 0 must not read the buffer it writes: stage the input in the ping-pong buffer
        PhaseScope ps(RSORT_PHASE_COPY, p.n, s);
        if (hipMemcpyAsync(c.tmp_k, kin, (size_t)p.n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return RSORT_ERR_HIP;
        if (p.pairs &&
            hipMemcpyAsync(c.tmp_v, vin, (size_t)p.n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return RSORT_ERR_HIP;
        x.sk = c.tmp_k;
        x.sv = c.tmp_v;
    }
    // The routes, one per sort (joint needs k = 8, nextc k = 3 or 4). Digit-group chunks on every second pass
    // (joint_plan): needs rs_scatter_lines for both outputs (lane-ordered ranks, 16-B aligned ping-pong buffers)
    const bool joint = joint_plan(p) && g_group_chunks.load() != 0 &&
                       internal_rank(g_rank_algo.load()) == kRankAtomic && line_capable(kout, vout, p.pairs, p.n) &&
                       line_capable(c.tmp_k, c.tmp_v, p.pairs, p.n);
    if (joint_plan(p) && !joint &&
        hipMemsetAsync(c.bounds, 0, (size_t)2 * kBoundsWords * 4, s) != hipSuccess)  // rsort_group_flags: none
        return RSORT_ERR_HIP;
    // next-digit counts (k = 3, 4): the same kernel conditions as digit groups
    const bool nextc = next_plan(p) && g_group_chunks.load() != 0 && internal_rank(g_rank_algo.load()) == kRankAtomic &&
                       line_capable(kout, nullptr, 0, p.n) && line_capable(c.tmp_k, nullptr, 0, p.n);
    // next-digit plans: every pass after the first derives its offsets from the raw counts the pass
    // before added, instead of the last workgroup of each pass scanning them (RSORT_NX_TAIL=1: that older way)
    // (raw tables only up to kRawTableMaxChunks chunks: each workgroup reads the whole table)
    const bool rawt = nextc && !lab().nx_tail && p.num_chunks <= kRawTableMaxChunks;
    const bool hyb = hybrid_eligible(p, joint, inplace || kin == c.tmp_k, allow_hybrid);
    if (hyb && (st = x.hybrid_prologue())) return st;
    return joint ? x.group_passes(hyb) : nextc ? x.next_digit_passes(rawt) : x.plain_passes();
}

// ------------------------------------------------------------------------------ host entry cache
struct DevCache {
    std::mutex mu;
    int device = -1;
    void *buf = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;

    // (under mu) makes the stream and grows the buffer to at least `need` bytes
    int reserve(size_t need) {
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return RSORT_ERR_HIP;
        if (cap >= need) return RSORT_OK;
        if (buf) (void)hipFree(buf);
        buf = nullptr;
        cap = 0;
        if (hipMalloc(&buf, need) != hipSuccess) return RSORT_ERR_ALLOC;
        cap = need;
        return RSORT_OK;
    }
};
std::mutex g_cache_mu;
std::vector<DevCache *> g_caches;

DevCache *cache_for(int dev) {
    std::lock_guard<std::mutex> g(g_cache_mu);
    for (DevCache *c : g_caches)
        if (c->device == dev) return c;
    DevCache *c = new DevCache();
    c->device = dev;
    g_caches.push_back(c);
    return c;
}

// What the host entries share: the current device's cache, locked for the helper's lifetime, its buffer handed out
// in 256-B-aligned regions (what the alignment-dependent routes count on: 16-B aligned keys, values at a multiple
// of 16 B from them) and the copies on the cache's stream. A null device region is an optional array its call does
// without: it copies nothing.
struct Staging {
    std::unique_lock<std::mutex> lock;
    DevCache *dc = nullptr;
    hipStream_t s = nullptr;
    Bump regions{nullptr};

    int open() {
        int dev = 0;
        if (!have_device()) return RSORT_ERR_NODEV;
        if (hipGetDevice(&dev) != hipSuccess) return RSORT_ERR_HIP;
        dc = cache_for(dev);
        lock = std::unique_lock<std::mutex>(dc->mu);
        return RSORT_OK;
    }
    // the buffer of one call: at least `total` bytes, its regions taken from the start
    int reserve(size_t total) {
        const int st = dc->reserve(total);
        if (st) return st;
        regions = Bump(dc->buf);
        s = dc->stream;
        return RSORT_OK;
    }
    uint32_t *words(size_t n) { return regions.take(n * 4); }
    // words [at, at + n) of a host array and its device region
    int upload(uint32_t *dev, const uint32_t *host, size_t n, size_t at = 0) {
        return dev ? hip_status(hipMemcpyAsync(dev + at, host + at, n * 4, hipMemcpyHostToDevice, s)) : RSORT_OK;
    }
    int download(uint32_t *host, const uint32_t *dev, size_t n, size_t at = 0) {
        return dev ? hip_status(hipMemcpyAsync(host + at, dev + at, n * 4, hipMemcpyDeviceToHost, s)) : RSORT_OK;
    }
    // a call that failed after its first launch: the stream is idle before the buffer is anyone else's
    int drain(int st) {
        (void)hipStreamSynchronize(s);
        return st;
    }
};

int host_sort(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout,
              int64_t n, int k, rsort_phase_times *times) {
    const int pairs = vin != nullptr;
    rsort_plan p;
    int st = plan_fill(n, k, pairs, 0, &p);
    if (st) return st;
    if (n == 0) {
        if (times) memset(times, 0, sizeof(*times));
        return RSORT_OK;
    }
    if (!kin || !kout || (pairs && !vout)) return RSORT_ERR_ARG;
    Staging h;
    const size_t nw = (size_t)n, nb = align256(nw * 4);
    if ((st = h.open()) || (st = h.reserve(nb * (pairs ? 4 : 2) + p.workspace_bytes))) return st;
    uint32_t *const d_kin = h.words(nw), *const d_vin = pairs ? h.words(nw) : nullptr;
    uint32_t *const d_kout = h.words(nw), *const d_vout = pairs ? h.words(nw) : nullptr;
    void *const ws = h.regions.take(p.workspace_bytes);
    if ((st = h.upload(d_kin, kin, nw)) || (st = h.upload(d_vin, vin, nw))) return st;
    if (times) rsort_profile_begin();
    st = sort_planned(p, d_kin, d_vin, d_kout, d_vout, ws, p.workspace_bytes, h.s);
    if (times) {
        const int st2 = rsort_profile_end(times);
        if (!st) st = st2;
    }
    if (st) return h.drain(st);
    if ((st = h.download(kout, d_kout, nw)) || (st = h.download(vout, d_vout, nw))) return st;
    // this entry waits for the device anyway: the sort's self-checks (rsort_plan_check) are read here
    uint32_t check = 0;
    if ((st = read_words(&check, carve(p, ws).done + kDoneErr, 1, h.s))) return st;
    return check ? RSORT_ERR_CHECK : RSORT_OK;
}

// ------------------------------------------------------------------------------ segmented sort
// Workspace of rsort_u32_segmented_device: the multi-tile path's ping-pong keys (and values), one list per kernel
// kind (room for every segment in each: the kinds are only known on the device) and the counters.
struct SegCarve {
    uint32_t *ktmp, *vtmp, *lists[kSegKinds], *counters;
    size_t bytes;
};

SegCarve seg_carve(int64_t n, int64_t nseg, int pairs, void *ws) {
    SegCarve c{};
    Bump b(ws);
    c.ktmp = b.take((size_t)n * 4);
    if (pairs) c.vtmp = b.take((size_t)n * 4);
    for (int i = 0; i < kSegKinds; ++i) c.lists[i] = b.take((size_t)nseg * 4);
    c.counters = b.take(256);
    c.bytes = b.off;
    return c;
}

int seg_sizes(int64_t n, int64_t nseg) {
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    return (nseg < 0 || nseg >= ((int64_t)1 << 31)) ? RSORT_ERR_ARG : RSORT_OK;
}

int seg_rank() { return internal_rank(g_rank_algo.load()) == kRankAtomic ? kRankAtomic : kRankCount; }

// The grid of every kind's kernel (seg_sort launches with it, rsort_segmented_grids reports it): the most
// segments the kind can have, capped by four resident waves of workgroups -- the lists' lengths are only known on
// the device, so the count comes from n and the segment count, and every workgroup strides over its list. The
// test hook rsort_set_segmented_grid_limit caps every kind further.
void seg_grids(int64_t n, int64_t nseg, int pairs, int rank, uint32_t grids[kSegKinds]) {
    const int cus = std::max(1, device_cus());
    const int limit = g_seg_grid_limit.load();
    for (int kind = 0; kind < kSegKinds; ++kind) {
        // each segment of a kind holds more keys than the kind below takes; a wave-kind workgroup sorts four
        // segments at a time
        const int below = kind == kSegSmall ? kSegWaveKeys : kind == kSegLds ? kSegSmallKeys : kind == kSegTiles ? kSegLdsKeys : 0;
        int64_t most = below ? std::min<int64_t>(nseg, n / below) : nseg;
        if (kind == kSegWave) most = (most + 3) / 4;
        grids[kind] = 0;
        if (most == 0) continue;
        const int bpc = std::max(1, seg_blocks_per_cu(kind, pairs, rank));
        int64_t grid = std::min<int64_t>(most, (int64_t)cus * bpc * 4);
        if (limit > 0) grid = std::min<int64_t>(grid, limit);
        grids[kind] = (uint32_t)grid;
    }
}

int seg_sort(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n,
             const uint32_t *off, int64_t nseg, void *ws, size_t ws_bytes, hipStream_t s) {
    int st = seg_sizes(n, nseg);
    if (st) return st;
    if ((vin != nullptr) != (vout != nullptr)) return RSORT_ERR_ARG;
    if (n == 0 || nseg == 0) return RSORT_OK;
    if (!kin || !kout || !off || !ws) return RSORT_ERR_ARG;
    if (!aligned4(kin) || !aligned4(kout) || !aligned4(vin) || !aligned4(vout) || !aligned4(off) || !aligned4(ws))
        return RSORT_ERR_ALIGN;
    const int pairs = vin != nullptr;
    const SegCarve c = seg_carve(n, nseg, pairs, ws);
    if (ws_bytes < c.bytes) return RSORT_ERR_WORKSPACE;

    const int rank = seg_rank();
    if (hipMemsetAsync(c.counters, 0, 256, s) != hipSuccess) return RSORT_ERR_HIP;
    {
        PhaseScope ps(RSORT_PHASE_HISTOGRAM, nseg, s);
        SegClassifyArgs a{};
        a.off = off;
        for (int i = 0; i < kSegKinds; ++i) a.lists[i] = c.lists[i];
        a.counters = c.counters;
        a.n = (uint64_t)n;
        a.num_segments = (uint32_t)nseg;
        if ((st = hip_status(launch_seg_classify(a, s)))) return st;
    }
    // Every kernel is launched with seg_grids' grid; one whose list is empty returns at once.
    uint32_t grids[kSegKinds];
    seg_grids(n, nseg, pairs, rank, grids);
    for (int kind = 0; kind < kSegKinds; ++kind) {
        const uint32_t grid = grids[kind];
        if (grid == 0) continue;
        PhaseScope ps(RSORT_PHASE_SCATTER, n, s);
        SegSortArgs a{};
        a.kin = kin;
        a.vin = vin;
        a.kout = kout;
        a.vout = vout;
        a.ktmp = c.ktmp;
        a.vtmp = c.vtmp;
        a.off = off;
        a.list = c.lists[kind];
        a.count = c.counters + kind;
        a.check = c.counters + kSegCheckWord;
        a.rank_fault = rank_fault_unnumbered();
        if ((st = hip_status(launch_seg_sort(kind, pairs, rank, a, grid, s)))) return st;
    }
    return RSORT_OK;
}

int seg_host_sort(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout, int64_t n,
                  const uint32_t *off, int64_t nseg) {
    int st = seg_sizes(n, nseg);
    if (st) return st;
    if ((vin != nullptr) != (vout != nullptr)) return RSORT_ERR_ARG;
    if (n == 0 || nseg == 0) return RSORT_OK;
    if (!kin || !kout || !off) return RSORT_ERR_ARG;
    for (int64_t i = 0; i < nseg; ++i)
        if (off[i] > off[i + 1] || (int64_t)off[i + 1] > n) return RSORT_ERR_ARG;
    const int pairs = vin != nullptr;
    Staging h;
    if ((st = h.open())) return st;
    // the segments are contiguous: together they cover [lo, lo + m), and only that range travels
    const size_t lo = off[0], m = (size_t)off[nseg] - off[0];
    if (m == 0) return RSORT_OK;
    const size_t nw = (size_t)n, ow = (size_t)nseg + 1;
    const size_t wsb = seg_carve(n, nseg, pairs, nullptr).bytes;
    if ((st = h.reserve(align256(nw * 4) * (pairs ? 4 : 2) + align256(ow * 4) + wsb))) return st;
    uint32_t *const d_kin = h.words(nw), *const d_vin = pairs ? h.words(nw) : nullptr;
    uint32_t *const d_kout = h.words(nw), *const d_vout = pairs ? h.words(nw) : nullptr;
    uint32_t *const d_off = h.words(ow);
    void *const ws = h.regions.take(wsb);
    if ((st = h.upload(d_kin, kin, m, lo)) || (st = h.upload(d_vin, vin, m, lo)) || (st = h.upload(d_off, off, ow)))
        return st;
    if ((st = seg_sort(d_kin, d_vin, d_kout, d_vout, n, d_off, nseg, ws, wsb, h.s))) return h.drain(st);
    if ((st = h.download(kout, d_kout, m, lo)) || (st = h.download(vout, d_vout, m, lo))) return st;
    uint32_t check = 0;
    if ((st = read_words(&check, seg_carve(n, nseg, pairs, ws).counters + kSegCheckWord, 1, h.s))) return st;
    return check ? RSORT_ERR_CHECK : RSORT_OK;
}

// ------------------------------------------------------------------------------ top-k selection
// (rsort_topk.hip.) Workspace of rsort_u32_topk_device, by route; the state words come first on both, so
// rsort_topk_report finds them without knowing the route. The caller's pointer may have any 4-byte alignment: the
// regions start at its next multiple of 256 (the 256 B of slack in the formula).
// AUTO selects for k <= n / kTopkAutoDiv[pairs] (rsort_topk_auto_limit). Measured (profiles/topk.json,
// uniform keys at 2^26 and 2^30): keys only, SELECT is 1.30x faster than SORT at k = n / 16 at 2^30 and 8 % slower at
// n / 4; with values or indices it is still 1.15x (2^26) and 1.20x (2^30) faster at k = n / 2, the largest k measured.
constexpr int64_t kTopkAutoDiv[2] = {16, 2};

struct TopkCarve {
    uint32_t *state, *totals, *rows_cnt, *rows_pre, *offs0, *offs1, *wk, *wv, *ak, *av;  // SELECT
    uint32_t *sk, *sv;                                                                   // SORT
    void *sort_ws;
    size_t sort_bytes, bytes;
};

// route: RSORT_TOPK_SELECT or RSORT_TOPK_SORT; plan: the finishing sort's (k entries) or the whole sort's (n)
TopkCarve topk_carve(int64_t n, int64_t k, int pairs, int route, const rsort_plan &plan, void *ws) {
    TopkCarve c{};
    Bump b(ws, /*round_base=*/true);
    c.state = b.take(256);
    if (route == RSORT_TOPK_SELECT) {
        c.totals = b.take((size_t)kTopkTotalsWords * 4);
        c.rows_cnt = b.take((size_t)kTopkMaxGrid * kTopkBins0 * 4);
        c.rows_pre = b.take((size_t)kTopkMaxGrid * kTopkBins0 * 4);
        c.offs0 = b.take((size_t)kTopkMaxGrid * 8);
        c.offs1 = b.take((size_t)kTopkMaxGrid * 8);
        c.wk = b.take((size_t)k * 4);
        if (pairs) c.wv = b.take((size_t)k * 4);
        c.ak = b.take((size_t)n * 4);
        if (pairs) c.av = b.take((size_t)n * 4);
    } else {
        c.sk = b.take((size_t)n * 4);
        if (pairs) c.sv = b.take((size_t)n * 4);
    }
    c.sort_bytes = plan.workspace_bytes;  // (a sum of whole regions itself)
    c.sort_ws = b.take(c.sort_bytes);
    c.bytes = b.off + 256;
    return c;
}

std::atomic<int> g_topk_route{RSORT_TOPK_AUTO};
std::atomic<int> g_topk_grid_limit{0};  // rsort_set_topk_grid_limit (tests); 0: no limit

constexpr int kTopkFlags = RSORT_TOPK_LARGEST | RSORT_TOPK_UNSORTED | RSORT_TOPK_INDICES;

int topk_sizes(int64_t n, int64_t k) {
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    return (k < 0 || k > n) ? RSORT_ERR_ARG : RSORT_OK;
}

int64_t topk_auto_limit(int64_t n, int pairs) { return n / kTopkAutoDiv[pairs ? 1 : 0]; }

// `route` as given (AUTO, SELECT, SORT) -> the route a call for (n, k) takes
int topk_resolve(int route, int64_t n, int64_t k, int pairs) {
    if (route != RSORT_TOPK_AUTO) return route;
    return k <= topk_auto_limit(n, pairs) ? RSORT_TOPK_SELECT : RSORT_TOPK_SORT;
}

// The finishing sort's plan (k entries) on SELECT, the whole sort's (n) on SORT.
int topk_plan(int64_t n, int64_t k, int pairs, int route, rsort_plan *p) {
    return plan_fill(route == RSORT_TOPK_SELECT ? k : n, 8, pairs, 0, p);
}

// G, the workgroups of every select kernel of one call (the launches and rsort_topk_grids share it): what the
// device holds at once, at most one workgroup per tile of the input but never fewer than 64 (the candidate list's
// kernels run on the same grid), capped by the picks' one-slice-per-thread limit and by the test hook.
uint32_t topk_grid(int64_t n) {
    const int64_t cus = std::max(1, device_cus()), bpc = std::max(1, topk_blocks_per_cu());
    const int64_t tiles = (n + kTopkTile - 1) / kTopkTile;
    int64_t g = std::min<int64_t>({cus * bpc, (int64_t)kTopkMaxGrid, std::max<int64_t>(64, tiles)});
    const int limit = g_topk_grid_limit.load();
    if (limit > 0) g = std::min<int64_t>(g, limit);
    return (uint32_t)g;
}

// The argument checks the device and the host entries of the top-k and the row-wise top-k share. size_st: the
// status of the call's own size test (topk_sizes, topk_rows_sizes); nothing: its sizes leave nothing to do (*noop).
int topk_check(int size_st, bool nothing, const void *kin, const void *vin, int flags, const void *kout,
               const void *vout, bool *noop) {
    *noop = false;
    if (size_st) return size_st;
    if (flags & ~kTopkFlags) return RSORT_ERR_ARG;
    if (flags & RSORT_TOPK_INDICES) {
        if (vin != nullptr) return RSORT_ERR_ARG;
    } else if ((vin != nullptr) != (vout != nullptr)) {
        return RSORT_ERR_ARG;
    }
    if (nothing) {
        *noop = true;
        return RSORT_OK;
    }
    if ((flags & RSORT_TOPK_INDICES) && vout == nullptr) return RSORT_ERR_ARG;
    if (!kin || !kout) return RSORT_ERR_ARG;
    return RSORT_OK;
}

// In front of the sort a call runs, behind the memset of its state words: that sort's check word is the call's
// (rsort_topk_report; a call that runs none leaves the word as its memset left it, 0).
int topk_mark_sorted(const TopkCarve &c, hipStream_t s) {
    return hip_status(hipMemsetD32Async((hipDeviceptr_t)(c.state + kTkSorted), 1, 1, s));
}

int topk_select(const uint32_t *kin, const uint32_t *vin, int64_t n, int64_t k, int flags, uint32_t *kout,
                uint32_t *vout, const TopkCarve &c, const rsort_plan &plan, hipStream_t s) {
    const int pairs = vout != nullptr;
    const uint32_t m = (flags & RSORT_TOPK_LARGEST) ? 0xFFFFFFFFu : 0u;
    const uint32_t grid = topk_grid(n);
    TopkArgs a{};
    a.kin = kin;
    a.vin = vin;
    a.state = c.state;
    a.totals = c.totals;
    a.rows_cnt = c.rows_cnt;
    a.rows_pre = c.rows_pre;
    a.offs0 = c.offs0;
    a.offs1 = c.offs1;
    a.wk = c.wk;
    a.wv = c.wv;
    a.ak = c.ak;
    a.av = c.av;
    a.n = (uint64_t)n;
    a.k = (uint32_t)k;
    a.m = m;
    a.pairs = pairs ? 1u : 0u;
    a.indices = (flags & RSORT_TOPK_INDICES) ? 1u : 0u;
    a.vec = (((uintptr_t)kin & 15u) == 0) ? 1u : 0u;
    int st;
    // the state words and the three levels' totals are adjacent: one memset node
    if (hipMemsetAsync(c.state, 0, 256 + align256((size_t)kTopkTotalsWords * 4), s) != hipSuccess) return RSORT_ERR_HIP;
    auto count = [&](int level, int64_t keys) {
        PhaseScope ps(RSORT_PHASE_HISTOGRAM, keys, s);
        return hip_status(launch_topk_count(level, a, grid, s));
    };
    auto pick = [&](int level) {
        PhaseScope ps(RSORT_PHASE_SCAN, level == 0 ? kTopkBins0 : kTopkBins, s);
        return hip_status(launch_topk_pick(level, a, grid, s));
    };
    if ((st = count(0, n)) || (st = pick(0))) return st;
    {
        PhaseScope ps(RSORT_PHASE_SCATTER, n, s);
        if ((st = hip_status(launch_topk_compact(a, grid, s)))) return st;
    }
    // (the candidate list's length is the device's: the profile counts no keys for its kernels)
    if ((st = count(1, 0)) || (st = pick(1)) || (st = count(2, 0)) || (st = pick(2))) return st;
    {
        PhaseScope ps(RSORT_PHASE_HISTOGRAM, 0, s);
        if ((st = hip_status(launch_topk_tie_count(a, grid, s)))) return st;
    }
    {
        PhaseScope ps(RSORT_PHASE_SCATTER, 0, s);
        if ((st = hip_status(launch_topk_emit(a, grid, s)))) return st;
    }
    // W holds the k entries as x = key ^ m, equal keys in input order
    TopkCopyArgs cp{};
    cp.kout = kout;
    cp.n = cp.k = (uint64_t)k;
    cp.m = m;
    if (flags & RSORT_TOPK_UNSORTED) {
        cp.kin = c.wk;
        cp.vin = c.wv;
        cp.vout = vout;
    } else {
        if ((st = topk_mark_sorted(c, s))) return st;
        if ((st = sort_planned(plan, c.wk, c.wv, kout, vout, c.sort_ws, c.sort_bytes, s))) return st;
        if (m == 0) return RSORT_OK;
        cp.kin = kout;  // the sorted x back to keys, in place
    }
    PhaseScope ps(RSORT_PHASE_COPY, k, s);
    return hip_status(launch_topk_copy(cp, s));
}

// The whole sort and a slice: what a caller without the select does. The sorted arrays (n entries) live in the
// workspace. Keys only: the input is sorted as it is and the k largest are its last k, reversed. With values or
// indices the sort must be stable in x = key ^ m, so LARGEST sorts a transformed copy; INDICES sorts an iota array.
int topk_sort(const uint32_t *kin, const uint32_t *vin, int64_t n, int64_t k, int flags, uint32_t *kout,
              uint32_t *vout, const TopkCarve &c, const rsort_plan &plan, hipStream_t s) {
    const bool pairs = vout != nullptr, largest = (flags & RSORT_TOPK_LARGEST) != 0;
    int st;
    if (hipMemsetAsync(c.state, 0xFF, 256, s) != hipSuccess) return RSORT_ERR_HIP;
    if ((st = topk_mark_sorted(c, s))) return st;
    const uint32_t *ks = kin, *vs = vin;
    if (pairs && largest) {
        PhaseScope ps(RSORT_PHASE_COPY, n, s);
        TopkCopyArgs x{};
        x.kin = kin;
        x.kout = c.sk;
        x.n = x.k = (uint64_t)n;
        x.m = 0xFFFFFFFFu;
        if ((st = hip_status(launch_topk_copy(x, s)))) return st;
        ks = c.sk;
    }
    if (flags & RSORT_TOPK_INDICES) {
        PhaseScope ps(RSORT_PHASE_COPY, n, s);
        if ((st = hip_status(launch_gen_iota(c.sv, (uint64_t)n, 0, s)))) return st;
        vs = c.sv;
    }
    if ((st = sort_planned(plan, ks, vs, c.sk, c.sv, c.sort_ws, c.sort_bytes, s))) return st;
    TopkCopyArgs cp{};
    cp.kin = c.sk;
    cp.vin = c.sv;
    cp.kout = kout;
    cp.vout = vout;
    cp.state = c.state;
    cp.n = (uint64_t)n;
    cp.k = (uint64_t)k;
    cp.m = (pairs && largest) ? 0xFFFFFFFFu : 0u;
    cp.rev = (!pairs && largest) ? 1u : 0u;
    PhaseScope ps(RSORT_PHASE_COPY, k, s);
    return hip_status(launch_topk_copy(cp, s));
}

int topk_device(const uint32_t *kin, const uint32_t *vin, int64_t n, int64_t k, int flags, uint32_t *kout,
                uint32_t *vout, void *ws, size_t ws_bytes, hipStream_t s) {
    bool noop;
    int st = topk_check(topk_sizes(n, k), k == 0, kin, vin, flags, kout, vout, &noop);
    if (st || noop) return st;
    if (!ws) return RSORT_ERR_ARG;
    if (!aligned4(kin) || !aligned4(vin) || !aligned4(kout) || !aligned4(vout) || !aligned4(ws)) return RSORT_ERR_ALIGN;
    const int pairs = vout != nullptr;
    const int route = topk_resolve(g_topk_route.load(), n, k, pairs);
    rsort_plan plan;
    if ((st = topk_plan(n, k, pairs, route, &plan))) return st;
    const TopkCarve c = topk_carve(n, k, pairs, route, plan, ws);
    if (ws_bytes < c.bytes) return RSORT_ERR_WORKSPACE;
    return route == RSORT_TOPK_SELECT ? topk_select(kin, vin, n, k, flags, kout, vout, c, plan, s)
                                      : topk_sort(kin, vin, n, k, flags, kout, vout, c, plan, s);
}

size_t topk_workspace_size(int64_t n, int64_t k, int pairs, int route) {
    if (topk_sizes(n, k) || route < RSORT_TOPK_AUTO || route > RSORT_TOPK_SORT) return 0;
    route = topk_resolve(route, n, k, pairs);
    rsort_plan plan;
    if (topk_plan(n, k, pairs, route, &plan)) return 0;
    return topk_carve(n, k, pairs, route, plan, nullptr).bytes;
}

// report8 (rsort_topk_report) of the call for (n, k, pairs) that last ran in ws, k > 0. The state words come first
// whatever the layout behind them; the sort's workspace is found from the route the call recorded.
int topk_read_report(int64_t n, int64_t k, int pairs, void *ws, int64_t *report8, hipStream_t s) {
    const rsort_plan none{};
    const TopkCarve c0 = topk_carve(0, 0, 0, RSORT_TOPK_SORT, none, ws);
    uint32_t h[kTkSorted + 1] = {0};
    int st;
    if ((st = read_words(h, c0.state, kTkSorted + 1, s))) return st;
    const int route = (int)h[kTkRoute];
    const bool sorted = route == RSORT_TOPK_SORT;
    for (int i = 0; i < 8; ++i) report8[i] = 0;
    for (int i = 0; i < 6; ++i) report8[i] = (sorted && i >= 2) ? -1 : (int64_t)h[i];
    if (h[kTkSorted] != 1u || (route != RSORT_TOPK_SELECT && route != RSORT_TOPK_SORT)) return RSORT_OK;
    rsort_plan plan;
    if ((st = topk_plan(n, k, pairs, route, &plan))) return st;
    const TopkCarve c = topk_carve(n, k, pairs, route, plan, ws);
    uint32_t check = 0;
    if ((st = read_words(&check, sort_check_word(plan, c.sort_ws), 1, s))) return st;
    report8[6] = (int64_t)(check & (kCheckTable | kCheckRankOrder));
    return RSORT_OK;
}

int topk_host(const uint32_t *kin, const uint32_t *vin, int64_t n, int64_t k, int flags, uint32_t *kout,
              uint32_t *vout) {
    bool noop;
    int st = topk_check(topk_sizes(n, k), k == 0, kin, vin, flags, kout, vout, &noop);
    if (st || noop) return st;
    const int pairs = vout != nullptr;  // (values, or indices: then there is no vin)
    Staging h;
    const size_t nw = (size_t)n, kw = (size_t)k;
    const size_t wsb = topk_workspace_size(n, k, pairs, g_topk_route.load());
    if ((st = h.open()) || (st = h.reserve(2 * align256(nw * 4) + 2 * align256(kw * 4) + wsb))) return st;
    uint32_t *const d_kin = h.words(nw), *const d_vin = vin ? h.words(nw) : nullptr;
    uint32_t *const d_kout = h.words(kw), *const d_vout = pairs ? h.words(kw) : nullptr;
    void *const ws = h.regions.take(wsb);
    if ((st = h.upload(d_kin, kin, nw)) || (st = h.upload(d_vin, vin, nw))) return st;
    if ((st = topk_device(d_kin, d_vin, n, k, flags, d_kout, d_vout, ws, wsb, h.s))) return h.drain(st);
    if ((st = h.download(kout, d_kout, kw)) || (st = h.download(vout, d_vout, kw))) return st;
    // this entry waits for the device anyway: the self-checks of the sort the call ran are read here
    int64_t rep[8];
    if ((st = topk_read_report(n, k, pairs, ws, rep, h.s))) return st;
    return rep[6] ? RSORT_ERR_CHECK : RSORT_OK;
}

// ------------------------------------------------------------------------------ row-wise top-k
// (rsort_topk_rows.hip.) Workspace of rsort_u32_topk_rows_device: the state words, the finishing sort's offsets
// (i * k) and the segmented sort's own workspace for rows segments of k entries. As for the top-k, the regions
// start at the caller's pointer rounded up to 256 (the slack in the formula).
struct TopkRowsCarve {
    uint32_t *state, *off;
    void *seg_ws;
    size_t seg_bytes, bytes;
};

TopkRowsCarve topk_rows_carve(int64_t rows, int64_t k, int pairs, void *ws) {
    TopkRowsCarve c{};
    Bump b(ws, /*round_base=*/true);
    c.state = b.take(256);
    c.off = b.take((size_t)(rows + 1) * 4);
    c.seg_bytes = seg_carve(rows * k, rows, pairs, nullptr).bytes;
    c.seg_ws = b.take(c.seg_bytes);
    c.bytes = b.off + 256;
    return c;
}

std::atomic<int> g_topk_rows_grid_limit{0};  // rsort_set_topk_rows_grid_limit (tests); 0: no limit

int topk_rows_sizes(int64_t rows, int64_t cols, int64_t k) {
    if (rows < 0 || rows >= ((int64_t)1 << 31) || !key_count_ok(cols)) return RSORT_ERR_SIZE;
    if (!key_count_ok(rows * cols)) return RSORT_ERR_SIZE;  // (< 2^63: both factors are in range)
    return (k < 0 || k > cols) ? RSORT_ERR_ARG : RSORT_OK;
}

// The select kernel's workgroups (the launch and rsort_topk_rows_grids share it): one per row (per four rows in
// the wave class), at most four resident waves of workgroups, capped by the test hook; each strides over the rows.
uint32_t topk_rows_grid(int64_t rows, int cls) {
    const int64_t cus = std::max(1, device_cus());
    const int64_t bpc = std::max(1, topk_rows_blocks_per_cu(cls));
    int64_t g = std::min<int64_t>(cls == kTrWave ? (rows + 3) / 4 : rows, cus * bpc * 4);
    const int limit = g_topk_rows_grid_limit.load();
    if (limit > 0) g = std::min<int64_t>(g, limit);
    return (uint32_t)g;
}

// nothing to do: no rows, no columns or k = 0
bool topk_rows_empty(int64_t rows, int64_t cols, int64_t k) { return rows == 0 || cols == 0 || k == 0; }

int topk_rows_device(const uint32_t *kin, const uint32_t *vin, int64_t rows, int64_t cols, int64_t k, int flags,
                     uint32_t *kout, uint32_t *vout, void *ws, size_t ws_bytes, hipStream_t s) {
    bool noop;
    int st = topk_check(topk_rows_sizes(rows, cols, k), topk_rows_empty(rows, cols, k), kin, vin, flags, kout, vout,
                        &noop);
    if (st || noop) return st;
    if (!ws) return RSORT_ERR_ARG;
    if (!aligned4(kin) || !aligned4(vin) || !aligned4(kout) || !aligned4(vout) || !aligned4(ws)) return RSORT_ERR_ALIGN;
    const int pairs = vout != nullptr;
    const TopkRowsCarve c = topk_rows_carve(rows, k, pairs, ws);
    if (ws_bytes < c.bytes) return RSORT_ERR_WORKSPACE;

    const int cls = topk_rows_class(cols);
    const bool sorted = !(flags & RSORT_TOPK_UNSORTED);
    const uint32_t m = (flags & RSORT_TOPK_LARGEST) ? 0xFFFFFFFFu : 0u;
    if (hipMemsetAsync(c.state, 0, 256, s) != hipSuccess) return RSORT_ERR_HIP;
    {
        PhaseScope ps(RSORT_PHASE_SCATTER, rows * cols, s);
        TopkRowsArgs a{};
        a.kin = kin;
        a.vin = vin;
        a.kout = kout;
        a.vout = vout;
        a.state = c.state;
        a.rows = (uint32_t)rows;
        a.cols = (uint32_t)cols;
        a.k = (uint32_t)k;
        a.m = m;
        a.pairs = !pairs ? kTrKeys : (flags & RSORT_TOPK_INDICES) ? kTrIndices : kTrValues;
        a.raw = sorted ? 0u : 1u;
        if ((st = hip_status(launch_topk_rows_select(cls, a, topk_rows_grid(rows, cls), s))))
            return st;
    }
    if (!sorted) return RSORT_OK;
    // the rows x k output holds x = key ^ m, every row's survivors in column order: the stable segmented sort of
    // its rows, in place, is the contract's order
    {
        PhaseScope ps(RSORT_PHASE_COPY, rows + 1, s);
        if ((st = hip_status(launch_topk_rows_offsets(c.off, (uint32_t)rows, (uint32_t)k, s)))) return st;
    }
    if ((st = seg_sort(kout, vout, kout, vout, rows * k, c.off, rows, c.seg_ws, c.seg_bytes, s))) return st;
    if (m == 0) return RSORT_OK;
    TopkCopyArgs cp{};
    cp.kin = kout;  // the sorted x back to keys, in place
    cp.kout = kout;
    cp.n = cp.k = (uint64_t)(rows * k);
    cp.m = m;
    PhaseScope ps(RSORT_PHASE_COPY, rows * k, s);
    return hip_status(launch_topk_copy(cp, s));
}

size_t topk_rows_workspace_size(int64_t rows, int64_t cols, int64_t k, int pairs) {
    if (topk_rows_sizes(rows, cols, k)) return 0;
    return topk_rows_carve(rows, k, pairs, nullptr).bytes;
}

// {flags, report4} of the call that last ran in ws
int topk_rows_read_check(int64_t rows, int64_t k, int pairs, void *ws, int *flags, int64_t *report4, hipStream_t s) {
    const TopkRowsCarve c = topk_rows_carve(rows, k, pairs, ws);
    uint32_t h[kTrSorted + 1] = {0}, check = 0;
    int st;
    if ((st = read_words(h, c.state, kTrSorted + 1, s))) return st;
    if (h[kTrSorted]) {
        const SegCarve sc = seg_carve(rows * k, rows, pairs, c.seg_ws);
        if ((st = read_words(&check, sc.counters + kSegCheckWord, 1, s))) return st;
    }
    *flags = (int)(check & kCheckRankOrder);
    if (report4) {
        report4[0] = (int64_t)h[kTrClass];
        report4[1] = (int64_t)h[kTrBadRows];
    }
    return RSORT_OK;
}

int topk_rows_host(const uint32_t *kin, const uint32_t *vin, int64_t rows, int64_t cols, int64_t k, int flags,
                   uint32_t *kout, uint32_t *vout) {
    bool noop;
    int st = topk_check(topk_rows_sizes(rows, cols, k), topk_rows_empty(rows, cols, k), kin, vin, flags, kout, vout,
                        &noop);
    if (st || noop) return st;
    const int pairs = vout != nullptr;
    Staging h;
    const size_t nw = (size_t)(rows * cols), kw = (size_t)(rows * k);
    const size_t wsb = topk_rows_workspace_size(rows, cols, k, pairs);
    if ((st = h.open()) || (st = h.reserve(2 * align256(nw * 4) + 2 * align256(kw * 4) + wsb))) return st;
    uint32_t *const d_kin = h.words(nw), *const d_vin = vin ? h.words(nw) : nullptr;
    uint32_t *const d_kout = h.words(kw), *const d_vout = pairs ? h.words(kw) : nullptr;
    void *const ws = h.regions.take(wsb);
    if ((st = h.upload(d_kin, kin, nw)) || (st = h.upload(d_vin, vin, nw))) return st;
    if ((st = topk_rows_device(d_kin, d_vin, rows, cols, k, flags, d_kout, d_vout, ws, wsb, h.s))) return h.drain(st);
    if ((st = h.download(kout, d_kout, kw)) || (st = h.download(vout, d_vout, kw))) return st;
    int check = 0;
    int64_t rep[4] = {0, 0, 0, 0};
    if ((st = topk_rows_read_check(rows, k, pairs, ws, &check, rep, h.s))) return st;
    return (check || rep[1]) ? RSORT_ERR_CHECK : RSORT_OK;
}

// rsort_set_*_grid_limit (test hooks): the limit before, or -RSORT_ERR_ARG
int set_grid_limit(std::atomic<int> &limit, int workgroups) {
    return workgroups < 0 ? -RSORT_ERR_ARG : limit.exchange(workgroups);
}

}  // namespace

void rsort::profile_pause(int delta) { t_prof_paused += delta; }

const uint32_t *rsort::sort_check_word(const rsort_plan &p, const void *ws) {
    return carve(p, const_cast<void *>(ws)).done + kDoneErr;
}

// ================================================================================ C ABI
extern "C" {

const char *rsort_status_string(int status) {
    switch (status) {
        case RSORT_OK: return "ok";
        case RSORT_ERR_ARG: return "invalid argument";
        case RSORT_ERR_BITS: return "k_bits outside [1, 13]";
        case RSORT_ERR_SIZE: return "n outside [0, 2^32)";
        case RSORT_ERR_ALIGN: return "device buffer not 4-byte aligned";
        case RSORT_ERR_ALLOC: return "allocation failed";
        case RSORT_ERR_HIP: return "HIP runtime error";
        case RSORT_ERR_WORKSPACE: return "workspace too small";
        case RSORT_ERR_NODEV: return "no HIP device";
        case RSORT_ERR_CAPACITY: return "output capacity too small for the received keys";
        case RSORT_ERR_COMM: return "RCCL communication error";
        case RSORT_ERR_CHECK: return "an on-device self-check of the sort failed";
        default: return "unknown status";
    }
}

int rsort_version(void) { return kVersion; }

int rsort_plan_make(int64_t n, int k_bits, int pairs, int64_t tiles_per_chunk, rsort_plan *plan) {
    return plan_fill(n, k_bits, pairs, tiles_per_chunk, plan);
}

size_t rsort_workspace_size(int64_t n, int k_bits, int pairs) {
    rsort_plan p;
    if (plan_fill(n, k_bits, pairs, 0, &p) != RSORT_OK) return 0;
    return p.workspace_bytes;
}

int rsort_sort_planned(const rsort_plan *plan, const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                       uint32_t *d_keys_out, uint32_t *d_vals_out, void *d_workspace,
                       size_t workspace_bytes, void *stream) {
    return rsort_sort_planned_ex(plan, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_workspace, workspace_bytes, stream, 0);
}

int rsort_sort_planned_ex(const rsort_plan *plan, const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                          uint32_t *d_keys_out, uint32_t *d_vals_out, void *d_workspace,
                          size_t workspace_bytes, void *stream, int flags) {
    if (!plan || (flags & ~RSORT_SORT_NO_HYBRID)) return RSORT_ERR_ARG;
    return sort_planned(*plan, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_workspace,
                        workspace_bytes, (hipStream_t)stream, !(flags & RSORT_SORT_NO_HYBRID));
}

int rsort_u32_device(const uint32_t *d_in, uint32_t *d_out, int64_t n, int k_bits,
                     void *d_workspace, size_t workspace_bytes, void *stream) {
    rsort_plan p;
    const int st = plan_fill(n, k_bits, 0, 0, &p);
    if (st) return st;
    return sort_planned(p, d_in, nullptr, d_out, nullptr, d_workspace, workspace_bytes,
                        (hipStream_t)stream);
}

int rsort_u32_pairs_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                           uint32_t *d_keys_out, uint32_t *d_vals_out, int64_t n, int k_bits,
                           void *d_workspace, size_t workspace_bytes, void *stream) {
    rsort_plan p;
    const int st = plan_fill(n, k_bits, 1, 0, &p);
    if (st) return st;
    return sort_planned(p, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_workspace,
                        workspace_bytes, (hipStream_t)stream);
}

int rsort_u32(const uint32_t *in, uint32_t *out, int64_t n, int k_bits) {
    return host_sort(in, nullptr, out, nullptr, n, k_bits, nullptr);
}

int rsort_u32_ex(const uint32_t *in, uint32_t *out, int64_t n, int k_bits, int block_size,
                 rsort_phase_times *times) {
    (void)block_size;
    return host_sort(in, nullptr, out, nullptr, n, k_bits, times);
}

int rsort_u32_pairs(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                    uint32_t *vals_out, int64_t n, int k_bits) {
    if (n > 0 && (!vals_in || !vals_out)) return RSORT_ERR_ARG;
    return host_sort(keys_in, vals_in, keys_out, vals_out, n, k_bits, nullptr);
}

int rsort_segmented_capacity(int pairs, int *small_keys, int *lds_keys) {
    if (!small_keys || !lds_keys) return RSORT_ERR_ARG;
    (void)pairs;  // (keys and pairs share both limits: the large shape's LDS holds 16384 keys and their values)
    *small_keys = kSegSmallKeys;
    *lds_keys = kSegLdsKeys;
    return RSORT_OK;
}

size_t rsort_segmented_workspace_size(int64_t n, int64_t num_segments, int pairs) {
    if (seg_sizes(n, num_segments)) return 0;
    return seg_carve(n, num_segments, pairs ? 1 : 0, nullptr).bytes;
}

int rsort_u32_segmented_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                               uint32_t *d_vals_out, int64_t n, const uint32_t *d_offsets, int64_t num_segments,
                               void *d_workspace, size_t workspace_bytes, void *stream) {
    return seg_sort(d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, d_offsets, num_segments, d_workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int rsort_segmented_check(int64_t n, int64_t num_segments, int pairs, const void *d_workspace, int *flags,
                          int64_t *class_counts, void *stream) {
    int st;
    if (!flags) return RSORT_ERR_ARG;
    *flags = 0;
    if (class_counts) memset(class_counts, 0, 4 * sizeof(int64_t));
    if ((st = seg_sizes(n, num_segments))) return st;
    if (n == 0 || num_segments == 0) return RSORT_OK;
    if (!d_workspace) return RSORT_ERR_ARG;
    const SegCarve c = seg_carve(n, num_segments, pairs ? 1 : 0, const_cast<void *>(d_workspace));
    uint32_t h[kSegCheckWord + 1] = {0};
    if ((st = read_words(h, c.counters, kSegCheckWord + 1, (hipStream_t)stream))) return st;
    *flags = (int)(h[kSegCheckWord] & (kCheckRankOrder | kCheckOffsets));
    if (class_counts) {  // (one wave or one small workgroup per segment: both are the small class)
        class_counts[0] = (int64_t)h[kSegWave] + (int64_t)h[kSegSmall];
        class_counts[1] = (int64_t)h[kSegLds];
        class_counts[2] = (int64_t)h[kSegTiles];
        class_counts[3] = (int64_t)h[kSegRejected];
    }
    return RSORT_OK;
}

int rsort_segmented_grids(int64_t n, int64_t num_segments, int pairs, int *grids) {
    int st;
    if (!grids) return RSORT_ERR_ARG;
    for (int i = 0; i < kSegKinds; ++i) grids[i] = 0;
    if ((st = seg_sizes(n, num_segments))) return st;
    if (n == 0 || num_segments == 0) return RSORT_OK;
    if (!have_device()) return RSORT_ERR_NODEV;
    uint32_t g[kSegKinds];
    seg_grids(n, num_segments, pairs ? 1 : 0, seg_rank(), g);
    for (int i = 0; i < kSegKinds; ++i) grids[i] = (int)g[i];
    return RSORT_OK;
}

int rsort_set_segmented_grid_limit(int workgroups) { return set_grid_limit(g_seg_grid_limit, workgroups); }

int rsort_u32_segmented(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                        int64_t n, const uint32_t *offsets, int64_t num_segments) {
    return seg_host_sort(keys_in, vals_in, keys_out, vals_out, n, offsets, num_segments);
}

size_t rsort_topk_workspace_size(int64_t n, int64_t k, int pairs, int route) {
    return topk_workspace_size(n, k, pairs ? 1 : 0, route);
}

int rsort_u32_topk_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, int64_t n, int64_t k, int flags,
                          uint32_t *d_keys_out, uint32_t *d_vals_out, void *d_workspace, size_t workspace_bytes,
                          void *stream) {
    return topk_device(d_keys_in, d_vals_in, n, k, flags, d_keys_out, d_vals_out, d_workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int rsort_u32_topk(const uint32_t *keys, const uint32_t *vals, int64_t n, int64_t k, int flags, uint32_t *keys_out,
                   uint32_t *vals_out) {
    return topk_host(keys, vals, n, k, flags, keys_out, vals_out);
}

int rsort_topk_report(int64_t n, int64_t k, int pairs, const void *d_workspace, int64_t *report8, void *stream) {
    int st;
    if (!report8) return RSORT_ERR_ARG;
    for (int i = 0; i < 8; ++i) report8[i] = 0;
    if ((st = topk_sizes(n, k))) return st;
    if (k == 0) return RSORT_OK;
    if (!d_workspace) return RSORT_ERR_ARG;
    return topk_read_report(n, k, pairs ? 1 : 0, const_cast<void *>(d_workspace), report8, (hipStream_t)stream);
}

int rsort_set_topk_route(int route) {
    if (route < RSORT_TOPK_AUTO || route > RSORT_TOPK_SORT) return -RSORT_ERR_ARG;
    return g_topk_route.exchange(route);
}

int rsort_get_topk_route(void) { return g_topk_route.load(); }

int rsort_topk_auto_limit(int64_t n, int pairs, int64_t *k_max) {
    if (!k_max) return RSORT_ERR_ARG;
    *k_max = 0;
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    *k_max = topk_auto_limit(n, pairs ? 1 : 0);
    return RSORT_OK;
}

int rsort_topk_grids(int64_t n, int64_t k, int pairs, int *grids) {
    int st;
    (void)pairs;  // (keys and pairs run the same kernels)
    if (!grids) return RSORT_ERR_ARG;
    for (int i = 0; i < 4; ++i) grids[i] = 0;
    if ((st = topk_sizes(n, k))) return st;
    if (k == 0) return RSORT_OK;
    if (!have_device()) return RSORT_ERR_NODEV;
    const int g = (int)topk_grid(n);
    for (int i = 0; i < 4; ++i) grids[i] = g;
    return RSORT_OK;
}

int rsort_set_topk_grid_limit(int workgroups) { return set_grid_limit(g_topk_grid_limit, workgroups); }

size_t rsort_topk_rows_workspace_size(int64_t rows, int64_t cols, int64_t k, int pairs) {
    return topk_rows_workspace_size(rows, cols, k, pairs ? 1 : 0);
}

int rsort_u32_topk_rows_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, int64_t rows, int64_t cols,
                               int64_t k, int flags, uint32_t *d_keys_out, uint32_t *d_vals_out, void *d_workspace,
                               size_t workspace_bytes, void *stream) {
    return topk_rows_device(d_keys_in, d_vals_in, rows, cols, k, flags, d_keys_out, d_vals_out, d_workspace,
                            workspace_bytes, (hipStream_t)stream);
}

int rsort_u32_topk_rows(const uint32_t *keys, const uint32_t *vals, int64_t rows, int64_t cols, int64_t k, int flags,
                        uint32_t *keys_out, uint32_t *vals_out) {
    return topk_rows_host(keys, vals, rows, cols, k, flags, keys_out, vals_out);
}

int rsort_topk_rows_check(int64_t rows, int64_t cols, int64_t k, int pairs, const void *d_workspace, int *flags,
                          int64_t *report4, void *stream) {
    int st;
    if (!flags) return RSORT_ERR_ARG;
    *flags = 0;
    if (report4) memset(report4, 0, 4 * sizeof(int64_t));
    if ((st = topk_rows_sizes(rows, cols, k))) return st;
    if (topk_rows_empty(rows, cols, k)) return RSORT_OK;
    if (!d_workspace) return RSORT_ERR_ARG;
    return topk_rows_read_check(rows, k, pairs ? 1 : 0, const_cast<void *>(d_workspace), flags, report4,
                                (hipStream_t)stream);
}

int rsort_topk_rows_grids(int64_t rows, int64_t cols, int64_t k, int pairs, int *grids2) {
    int st;
    (void)pairs;  // (keys and pairs run the same kernels)
    if (!grids2) return RSORT_ERR_ARG;
    grids2[0] = grids2[1] = 0;
    if ((st = topk_rows_sizes(rows, cols, k))) return st;
    if (topk_rows_empty(rows, cols, k)) return RSORT_OK;
    if (!have_device()) return RSORT_ERR_NODEV;
    const int cls = topk_rows_class(cols);
    grids2[0] = (int)topk_rows_grid(rows, cls);
    grids2[1] = cls;
    return RSORT_OK;
}

int rsort_set_topk_rows_grid_limit(int workgroups) { return set_grid_limit(g_topk_rows_grid_limit, workgroups); }

int rsort_pass_histogram(const rsort_plan *plan, const uint32_t *d_keys, int shift,
                         uint32_t *d_table, void *stream) {
    int st = check_plan(plan);
    if (st) return st;
    if (shift < 0 || shift > 31) return RSORT_ERR_ARG;
    if (plan->n == 0) return RSORT_OK;
    if (!d_keys || !d_table) return RSORT_ERR_ARG;
    return run_histogram(*plan, hist_args(*plan, d_keys, shift, d_table), kDigitShift, (hipStream_t)stream);
}

int rsort_pass_scan(const rsort_plan *plan, uint32_t *d_table, uint32_t *d_block_sums, void *stream) {
    int st = check_plan(plan);
    if (st) return st;
    if (plan->n == 0) return RSORT_OK;
    if (!d_table || !d_block_sums) return RSORT_ERR_ARG;
    return run_scan(*plan, scan_args(*plan, d_table, d_block_sums), (hipStream_t)stream);
}

int rsort_pass_scatter(const rsort_plan *plan, const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                       uint32_t *d_keys_out, uint32_t *d_vals_out, int shift, const uint32_t *d_table,
                       void *stream) {
    int st = check_plan(plan);
    if (st) return st;
    if (shift < 0 || shift > 31) return RSORT_ERR_ARG;
    if (plan->n == 0) return RSORT_OK;
    if (!d_keys_in || !d_keys_out || !d_table || (plan->pairs && (!d_vals_in || !d_vals_out)))
        return RSORT_ERR_ARG;
    const PassIo io{d_keys_in, d_vals_in, d_keys_out, d_vals_out};
    return run_scatter(*plan, scatter_args(*plan, io, shift, d_table), kDigitShift, (hipStream_t)stream);
}

int rsort_pass_local_sort(const rsort_plan *plan, const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                          uint32_t *d_keys_out, uint32_t *d_vals_out, int shift, void *stream) {
    int st = check_plan(plan);
    if (st) return st;
    if (shift < 0 || shift > 31) return RSORT_ERR_ARG;
    if (plan->n == 0) return RSORT_OK;
    if (!d_keys_in || !d_keys_out || (plan->pairs && (!d_vals_in || !d_vals_out)))
        return RSORT_ERR_ARG;
    if (d_keys_in == d_keys_out) return RSORT_ERR_ARG;
    // local-only mode never reads the offset table
    ScatterArgs a = scatter_args(*plan, PassIo{d_keys_in, d_vals_in, d_keys_out, d_vals_out}, shift, /*table=*/nullptr);
    a.local_only = 1;
    return run_scatter(*plan, a, kDigitShift, (hipStream_t)stream);
}

int rsort_set_rank_algo(int algo) {
    if (algo != RSORT_RANK_MATCH && algo != RSORT_RANK_SPLIT && algo != RSORT_RANK_BALLOT) return RSORT_ERR_ARG;
    g_rank_algo.store(algo);
    return RSORT_OK;
}

int rsort_get_rank_algo(void) { return g_rank_algo.load(); }

int rsort_set_group_chunks(int enable) {
    g_group_chunks.store(enable ? 1 : 0);
    return RSORT_OK;
}

int rsort_get_group_chunks(void) { return g_group_chunks.load(); }

int rsort_set_hybrid(int mode) {
    if (mode != RSORT_HYBRID_AUTO && mode != RSORT_HYBRID_OFF && mode != RSORT_HYBRID_FORCE) return RSORT_ERR_ARG;
    g_hybrid.store(mode);
    return RSORT_OK;
}

int rsort_get_hybrid(void) { return g_hybrid.load(); }

int rsort_hybrid_capacity(void) { return (int)kHybCapacity; }

int rsort_hybrid_kernel_info(int *info) {
    if (!info) return RSORT_ERR_ARG;
    return hyb_kernel_info(info) == hipSuccess ? RSORT_OK : RSORT_ERR_HIP;
}

int rsort_hybrid_range(int64_t *min_keys, int64_t *max_keys) {
    if (!min_keys || !max_keys) return RSORT_ERR_ARG;
    *min_keys = hyb_min_keys();
    *max_keys = kHybMaxKeys;
    return RSORT_OK;
}

int rsort_hybrid_gate_threshold(int64_t n) {
    if (n == 0 || !key_count_ok(n)) return -RSORT_ERR_SIZE;
    return (int)gate_threshold(n);
}

int rsort_hybrid_report(const rsort_plan *plan, const void *d_workspace, int *report, void *stream) {
    if (!plan || !report || !d_workspace) return RSORT_ERR_ARG;
    int st = check_plan(plan);
    if (st) return st;
    for (int i = 0; i < 4; ++i) report[i] = 0;
    if (plan->n == 0) return RSORT_OK;
    const Carve c = carve(*plan, const_cast<void *>(d_workspace));
    uint32_t h[4] = {0, 0, 0, 0};
    if ((st = read_words(h, c.done + kHybMode, 4, (hipStream_t)stream))) return st;
    report[0] = (int)h[kHybEligible - kHybMode];
    report[1] = (int)h[kHybGate - kHybMode];  // RSORT_GATE_*
    report[2] = (int)h[kHybMax - kHybMode];
    report[3] = h[0] == kHybRun ? 1 : 0;
    return RSORT_OK;
}

int rsort_group_flags(const rsort_plan *plan, const void *d_workspace, int *flags, void *stream) {
    if (!plan || !flags || !d_workspace) return RSORT_ERR_ARG;
    int st = check_plan(plan);
    if (st) return st;
    flags[0] = flags[1] = 0;
    if (!joint_plan(*plan) || plan->n == 0) return RSORT_OK;
    // (a digit-group plan has four passes: both odd passes' bounds exist)
    uint32_t h[2 * kBoundsWords];
    if ((st = read_words(h, carve(*plan, const_cast<void *>(d_workspace)).bounds, 2 * kBoundsWords, (hipStream_t)stream)))
        return st;
    flags[0] = (int)h[0];  // kGroupsFixed / kGroupsWhole / kGroupsCut
    flags[1] = (int)h[kBoundsWords];
    return RSORT_OK;
}

int rsort_cut_plan_stats(const rsort_plan *plan, const void *d_workspace, int *stats, void *stream) {
    if (!plan || !stats || !d_workspace) return RSORT_ERR_ARG;
    int st = check_plan(plan);
    if (st) return st;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (!joint_plan(*plan) || plan->n == 0) return RSORT_OK;
    uint32_t h[2 * kBoundsWords];
    if ((st = read_words(h, carve(*plan, const_cast<void *>(d_workspace)).bounds, 2 * kBoundsWords, (hipStream_t)stream)))
        return st;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) stats[4 * i + j] = (int)h[i * kBoundsWords + kBoundsStat + j];
    return RSORT_OK;
}

int rsort_plan_features(const rsort_plan *plan) {
    if (check_plan(plan) != RSORT_OK) return -RSORT_ERR_ARG;
    const rsort_plan &p = *plan;
    const bool atomic = internal_rank(g_rank_algo.load()) == kRankAtomic;
    const bool on = g_group_chunks.load() != 0 && atomic;
    int f = 0;
    if (joint_plan(p) && on) f |= RSORT_FEAT_GROUPS;
    if (next_plan(p) && on) {
        f |= RSORT_FEAT_NEXT_DIGIT;
        f |= (!lab().nx_tail && p.num_chunks <= kRawTableMaxChunks) ? RSORT_FEAT_RAW_TABLES : RSORT_FEAT_TAIL_SCAN;
    }
    return f;
}

int rsort_inject_table_fault(int enable) { return g_table_fault.exchange(enable ? 1 : 0); }

int rsort_inject_rank_fault(int enable) { return g_rank_fault.exchange(enable ? 1 : 0); }

int rsort_inject_fault_window(int64_t first, int64_t count) {
    if (count >= 0 && first < 0) return RSORT_ERR_ARG;
    t_fault_window = FaultWindow{count < 0 ? 0 : first, count < 0 ? -1 : count, 0};
    return RSORT_OK;
}

int64_t rsort_fault_window_calls(void) { return t_fault_window.started; }

int rsort_plan_check(const rsort_plan *plan, const void *d_workspace, int *flags, void *stream) {
    if (!plan || !flags || !d_workspace) return RSORT_ERR_ARG;
    int st = check_plan(plan);
    if (st) return st;
    *flags = 0;
    if (plan->n == 0) return RSORT_OK;
    uint32_t h = 0;
    if ((st = read_words(&h, carve(*plan, const_cast<void *>(d_workspace)).done + kDoneErr, 1, (hipStream_t)stream)))
        return st;
    *flags = (int)(h & (kCheckTable | kCheckRankOrder));
    return RSORT_OK;
}

size_t rsort_scatter_kernels_used(char *buf, size_t len, int reset) {
    return scatter_kernels_used(buf, len, reset);
}

size_t rsort_scatter_kernels_known(char *buf, size_t len) { return scatter_kernels_known(buf, len); }

int rsort_lane_order_probe(void) {
    if (!have_device()) return -RSORT_ERR_NODEV;
    return lane_order_probe();
}

int rsort_profile_begin(void) {
    std::lock_guard<std::mutex> g(g_prof.mu);
    for (auto &r : g_prof.recs) {
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.recs.clear();
    g_prof.on = true;
    return RSORT_OK;
}

int rsort_profile_end(rsort_phase_times *out) {
    std::vector<ProfRec> recs;
    {
        std::lock_guard<std::mutex> g(g_prof.mu);
        g_prof.on = false;
        recs.swap(g_prof.recs);
    }
    rsort_phase_times t;
    memset(&t, 0, sizeof(t));
    int st = RSORT_OK;
    // launches of hybrid-eligible sorts carry their route (Gate): those of the route that did not run left at once
    // and are not counted. The mode word is read here, after the events: it is the LAST sort's in that workspace
    // (a profile over sorts of different inputs in one workspace counts them all by the last one's route).
    std::vector<std::pair<const uint32_t *, uint32_t>> modes;
    auto mode_of = [&](const uint32_t *m) {
        for (auto &kv : modes)
            if (kv.first == m) return kv.second;
        uint32_t v = 0xFFFFFFFFu;
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, m, 4, hipMemcpyDeviceToHost) != hipSuccess)
            v = 0xFFFFFFFFu;  // (unreadable, e.g. a freed workspace: count every launch)
        modes.emplace_back(m, v);
        return v;
    };
    for (auto &r : recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) {
            st = RSORT_ERR_HIP;
            continue;
        }
        if (r.gate.mode != nullptr) {
            const uint32_t v = mode_of(r.gate.mode);
            if (v != 0xFFFFFFFFu && v != r.gate.want) continue;
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            st = RSORT_ERR_HIP;
            continue;
        }
        t.ms[r.phase] += ms;
        t.launches[r.phase] += 1;
        t.keys[r.phase] += r.keys;
    }
    {
        std::lock_guard<std::mutex> g(g_prof.mu);
        for (auto &r : recs) {
            g_prof.pool.push_back(r.a);
            g_prof.pool.push_back(r.b);
        }
    }
    if (out) *out = t;
    return st;
}

size_t rsort_partition_workspace_size(int64_t n, int num_buckets, int pairs) {
    if (num_buckets < 1 || num_buckets > kMaxSplitters + 1) return 0;
    const int bits = partition_bits(n, num_buckets, pairs);
    rsort_plan p;
    if (plan_fill(n, bits, pairs, 0, &p, /*partition=*/1) != RSORT_OK) return 0;
    return p.workspace_bytes;
}

int rsort_partition_device(const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                           uint32_t *d_vals_out, int64_t n, const uint32_t *splitters, int num_buckets,
                           uint32_t *d_bucket_starts, void *d_workspace, size_t workspace_bytes,
                           void *stream) {
    if (num_buckets < 1 || num_buckets > kMaxSplitters + 1) return RSORT_ERR_ARG;
    if (num_buckets > 1 && !splitters) return RSORT_ERR_ARG;
    for (int i = 1; i + 1 < num_buckets; ++i)
        if (splitters[i] < splitters[i - 1]) return RSORT_ERR_ARG;
    const int pairs = d_vals_in != nullptr;
    const int bits = partition_bits(n < 0 ? 0 : n, num_buckets, pairs);
    rsort_plan p;
    int st = plan_fill(n, bits, pairs, 0, &p, /*partition=*/1);
    if (st) return st;
    if (!d_bucket_starts) return RSORT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        return hip_status(hipMemsetAsync(d_bucket_starts, 0, (size_t)(num_buckets + 1) * 4, s));
    }
    if (!d_keys_in || !d_keys_out || !d_workspace || (pairs && !d_vals_out)) return RSORT_ERR_ARG;
    if (d_keys_in == d_keys_out) return RSORT_ERR_ARG;
    if (workspace_bytes < p.workspace_bytes) return RSORT_ERR_WORKSPACE;
    const Carve c = carve(p, d_workspace, /*partition=*/true);
    const int ns = num_buckets - 1;
    // (the check words as a sort's: cleared by the histogram, the scatter's rank check recorded there)
    HistArgs h = hist_args(p, d_keys_in, 0, c.table);
    ScatterArgs a = scatter_args(p, PassIo{d_keys_in, d_vals_in, d_keys_out, d_vals_out}, 0, c.table);
    h.nsplit = a.nsplit = (uint32_t)ns;  // (the digit is a bucket: kDigitSplit)
    for (int i = 0; i < ns; ++i) h.splitters[i] = a.splitters[i] = splitters[i];
    h.done = c.done;
    a.check = c.done + kDoneErr;
    if ((st = run_histogram(p, h, kDigitSplit, s))) return st;
    if ((st = run_scan(p, scan_args(p, c.table, c.bsums), s))) return st;
    if ((st = run_scatter(p, a, kDigitSplit, s))) return st;
    return hip_status(launch_gather_starts(c.table, (uint32_t)p.num_chunks, (uint32_t)num_buckets,
                                           (uint64_t)n, d_bucket_starts, s));
}

int rsort_partition_check(int64_t n, int num_buckets, int pairs, const void *d_workspace, int *flags, void *stream) {
    if (!flags || !d_workspace || num_buckets < 1 || num_buckets > kMaxSplitters + 1) return RSORT_ERR_ARG;
    *flags = 0;
    rsort_plan p;
    int st = plan_fill(n < 0 ? 0 : n, partition_bits(n < 0 ? 0 : n, num_buckets, pairs ? 1 : 0), pairs ? 1 : 0, 0, &p,
                       /*partition=*/1);
    if (st) return st;
    if (n <= 0) return RSORT_OK;
    const Carve c = carve(p, const_cast<void *>(d_workspace), /*partition=*/true);
    uint32_t h = 0;
    if ((st = read_words(&h, c.done + kDoneErr, 1, (hipStream_t)stream))) return st;
    *flags = (int)(h & (kCheckTable | kCheckRankOrder));
    return RSORT_OK;
}

int rsort_top_histogram(const uint32_t *d_keys, int64_t n, int top_bits, uint32_t *d_hist,
                        void *d_workspace, size_t workspace_bytes, void *stream) {
    rsort_plan p;
    int st = plan_fill(n, top_bits, 0, 0, &p);
    if (st) return st;
    if (!d_hist) return RSORT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return hip_status(hipMemsetAsync(d_hist, 0, (size_t)p.bins * 4, s));
    if (!d_keys || !d_workspace) return RSORT_ERR_ARG;
    if (workspace_bytes < p.workspace_bytes) return RSORT_ERR_WORKSPACE;
    const Carve c = carve(p, d_workspace);
    if ((st = run_histogram(p, hist_args(p, d_keys, 32 - top_bits, c.table), kDigitShift, s))) return st;
    if ((st = run_scan(p, scan_args(p, c.table, c.bsums), s))) return st;
    hipError_t e = launch_gather_starts(c.table, (uint32_t)p.num_chunks, (uint32_t)p.bins,
                                        (uint64_t)n, c.starts, s);
    if (e != hipSuccess) return RSORT_ERR_HIP;
    return hip_status(launch_diff_starts(c.starts, (uint32_t)p.bins, d_hist, s));
}

int rsort_top_histogram_sampled(const uint32_t *d_keys, int64_t n, int top_bits, int stride, uint32_t *d_hist,
                                void *stream) {
    if (top_bits < 1 || top_bits > kMaxBits) return RSORT_ERR_BITS;
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    if (stride < 1 || !d_hist || (n > 0 && !d_keys)) return RSORT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_hist, 0, ((size_t)1 << top_bits) * 4, s) != hipSuccess) return RSORT_ERR_HIP;
    if (n == 0) return RSORT_OK;
    PhaseScope ps(RSORT_PHASE_HISTOGRAM, (n + stride - 1) / stride, s);
    return hip_status(launch_top_hist_sampled(d_keys, (uint64_t)n, (uint32_t)top_bits, (uint32_t)stride, d_hist, s));
}

int rsort_sample_device(const uint32_t *d_keys, int64_t n, int64_t stride, int64_t count, int64_t row_len,
                        uint32_t *d_out, void *stream) {
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    if (stride < 1 || count < 0 || row_len < count || (row_len > 0 && !d_out) || (count > 0 && n > 0 && !d_keys))
        return RSORT_ERR_ARG;
    return hip_status(launch_sample(d_keys, (uint64_t)n, (uint64_t)stride, (uint64_t)count, (uint64_t)row_len, d_out,
                                    (hipStream_t)stream));
}

int rsort_fingerprint_device(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n, uint64_t *d_out,
                             void *stream) {
    if (!key_count_ok(n)) return RSORT_ERR_SIZE;
    if (!d_out || (n > 0 && !d_keys)) return RSORT_ERR_ARG;
    return hip_status(launch_fingerprint(d_keys, d_vals, (uint64_t)n, (unsigned long long *)d_out, (hipStream_t)stream));
}

int rsort_gen_uniform(uint32_t *d_out, int64_t n, uint64_t seed, void *stream) {
    if (n < 0) return RSORT_ERR_SIZE;
    if (n == 0) return RSORT_OK;
    if (!d_out) return RSORT_ERR_ARG;
    return hip_status(launch_gen_uniform(d_out, (uint64_t)n, seed, (hipStream_t)stream));
}

int rsort_gen_zipf(uint32_t *d_out, int64_t n, uint64_t seed, const uint32_t *d_cdf, int64_t ranks,
                   void *stream) {
    if (n < 0) return RSORT_ERR_SIZE;
    if (n == 0) return RSORT_OK;
    if (!d_out || !d_cdf || ranks <= 0) return RSORT_ERR_ARG;
    return hip_status(launch_gen_zipf(d_out, (uint64_t)n, seed, d_cdf, (uint64_t)ranks, (hipStream_t)stream));
}

int rsort_gen_iota(uint32_t *d_out, int64_t n, uint32_t base, void *stream) {
    if (n < 0) return RSORT_ERR_SIZE;
    if (n == 0) return RSORT_OK;
    if (!d_out) return RSORT_ERR_ARG;
    return hip_status(launch_gen_iota(d_out, (uint64_t)n, base, (hipStream_t)stream));
}

}  // extern "C"

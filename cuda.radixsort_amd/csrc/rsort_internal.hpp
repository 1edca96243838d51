// rsort_internal.hpp -- shared between the HIP kernels (rsort_kernels.hip, rsort_segmented.hip, rsort_topk.hip) and
// the host drivers (rsort_capi.cpp, rsort_multi.cpp). Not part of the public ABI (include/rsort.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "rsort.h"

namespace rsort {

constexpr int kWave = 64;
constexpr int kHistThreads = 256;          // workgroup size of the histogram kernel
constexpr int kMinBits = 1;
constexpr int kMaxBits = 13;            // the reference's SMEM limit (Parallel7.cu:740-745)
constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 16;
constexpr int kScanSegment = kScanThreads * kScanPerThread;  // table entries per scan block
constexpr int kMaxSplitters = 31;          // partition: <= 32 buckets (2 x 16 ranks' equal-key splitters)

enum DigitMode : int { kDigitShift = 0, kDigitSplit = 1 };

// Scatter-kernel tile geometries (threads x keys per thread). Measured on MI355X at 2^30 keys
// (dev/scatter_lab): the digit runs a tile writes must be long enough to fill 128-B lines, so
// k = 5..8 uses 16384-key tiles; k <= 4 has long runs already; k >= 9 and small inputs use
// 4096-key tiles (LDS for 2^k per-wave counters; enough workgroups to fill 256 CUs).
// kGeomLines (k = 5..8 keys): 16384-key tiles of 1024 threads written as whole 128-B lines
// (rs_scatter_lines; one workgroup per CU, its LDS holds the tile plus every digit's carry).
// kGeomLinesPairs (k = 5..8 pairs): 8192-pair tiles of 1024 threads x 8 (keys + values); k = 7, 8
// through rs_scatter_pairs (128-B lines in both arrays), k = 5, 6 through rs_scatter_lines (64-B lines).
// kGeomXL (k = 13): 4096-key tiles of 128 threads (2 waves), so the 2 x 8192 per-wave counters fit
// in LDS beside the tile (112 KB keys-only).
// kGeomLarge (512 x 32) holds an index but has no kernel: the planner never picks it, and check_plan refuses a plan
// whose (k, pairs, shape) no kernel exists for.
enum Geom : int { kGeomSmall = 0, kGeomLarge = 1, kGeomK4 = 2, kGeomLines = 3, kGeomLinesPairs = 4, kGeomXL = 5,
                  kGeomCount = 6 };
struct GeomShape {
    int threads;
    int kpt;
};
constexpr GeomShape kGeomShape[kGeomCount] = {{256, 16}, {512, 32}, {512, 16}, {1024, 16}, {1024, 8}, {128, 32}};
// rs_scatter_lines line width. Keys-only stages whole 128-B lines (the L2 line: runs that start or
// end mid-line cost about a third more HBM time, dev/runlen_lab.hip); its pairs instances keep 64-B
// lines (two 128-B carry areas do not fit in LDS beside 8192-key tiles of keys and values) --
// rs_scatter_pairs writes 128-B lines for pairs with its own layout.
constexpr int kLineKeys = 32;
constexpr int kLineKeysPairs = 16;
inline int geom_tile_keys(int g) { return kGeomShape[g].threads * kGeomShape[g].kpt; }
inline int geom_from_shape(int threads, int tile_keys, int pairs) {
    (void)pairs;
    for (int g = 0; g < kGeomCount; ++g)
        if (kGeomShape[g].threads == threads && geom_tile_keys(g) == tile_keys) return g;
    return -1;
}

// Internal ranking variants (rs_scatter's RANK template argument).
// kRankSplit: the reference's 1-bit splits; kRankCount: ballot peer match; kRankAtomic: lane-ordered
// returning LDS adds (the default where rs_lane_order_probe confirms the lane order).
enum RankAlgo : int { kRankSplit = 1, kRankCount = 3, kRankAtomic = 4 };
// Public rsort_rank_algo -> internal variant for the current device (probes lane order once).
int internal_rank(int public_algo);
// 1 / 0: same-address ds_add_rtn lanes are served in lane order on the current device; < 0 error.
int lane_order_probe();

struct HistArgs {
    const uint32_t *keys;
    uint32_t *table;        // [bins][num_chunks]
    uint64_t n;
    uint64_t chunk_keys;
    uint32_t num_chunks;
    uint32_t shift;
    uint32_t vec;           // keys 16-byte aligned: uint4 loads
    uint32_t split;         // workgroups per chunk (> 1: partial counts added into a zeroed table)
    uint32_t nsplit;
    uint32_t splitters[kMaxSplitters];
    // Digit-group chunks (kJointBits plans, see rs_histogram_joint). bounds != nullptr and
    // bounds[0] == kGroupsWhole: this pass's table is copy_src (the previous pass's joint counts),
    // copied instead of counted, and copy_src is cleared as it is read (the next counting pass adds
    // into it). bounds[0] == kGroupsCut: the workgroups count the cut plan's pieces (plan, below)
    // into pcounts; the scan assembles the table.
    const uint32_t *bounds;
    uint32_t *copy_src;
    const uint32_t *plan;
    uint32_t *pcounts;
    uint32_t wide;          // 1: 1024-thread workgroups also with split == 1 (one per chunk, no memset)
    // rs_histogram_joint only: the joint counts [next digit][digit] are added into `joint`
    // (zeroed); joint_enable == nullptr or *joint_enable != kGroupsFixed turns the joint count on.
    uint32_t *joint;
    const uint32_t *joint_enable;
    // raw-table next-digit plans (k = 3, 4), pass 0: the histogram also clears `zero` (zero_n words: the
    // table pass 0's scatter counts into) and the check words done[0], done[kDoneErr]; its table is
    // then read raw by the scatter (ScatterArgs::raw_table), with no scan launches
    uint32_t *zero;
    uint64_t zero_n;
    uint32_t *done;
    // joint-count histograms: != nullptr -> a workgroup whose chunk is skewed (a digit holds more
    // than twice its share) or that follows a cut plan (*joint_enable == kGroupsCut) also writes its
    // joint counts as rows[c][digit][next digit] (R x R words per chunk) and bumps *rows_cnt; a cut
    // plan made when every chunk wrote them takes its pieces' counts from the rows (rs_joint_bounds).
    // Piece-mode launches: the rows the plan's row tasks sum.
    uint32_t *rows;
    uint32_t *rows_cnt;
    // joint-count histograms: the second digit's shift when it is not shift + kJointBits (0: that default).
    // The hybrid route counts (digit 3, digit 2): shift = 24, shift2 = 16.
    uint32_t shift2;
    // hybrid-eligible sorts (rsort_hybrid.hip): != nullptr -> the kernel works only when *mode == mode_want
    // and leaves at once otherwise (both kernel sequences are enqueued, the device picks one)
    const uint32_t *mode;
    uint32_t mode_want;
};

struct ScatterArgs {
    const uint32_t *kin;
    const uint32_t *vin;
    uint32_t *kout;
    uint32_t *vout;
    const uint32_t *table;  // scanned [bins][num_chunks]
    uint64_t n;
    uint64_t chunk_keys;
    uint32_t num_chunks;
    uint32_t shift;
    uint32_t local_only;    // 1: write each tile's local order back in place of the tile
    uint32_t nsplit;
    uint32_t splitters[kMaxSplitters];
    unsigned long long *stamps;  // unused by the library; dev/lines_exp.hip's per-phase cycle stamps
    // rs_scatter_lines only: bounds != nullptr and bounds[0] != 0 -> chunk c is the key range
    // [bounds[1 + c], bounds[2 + c]) (a digit group of the previous pass) instead of
    // [c * chunk_keys, (c + 1) * chunk_keys)
    const uint32_t *bounds;
    // rs_scatter_lines with k <= 4 only: != nullptr -> the next pass's chunk table (zeroed), into
    // which this pass adds every written key's next digit by its destination chunk
    uint32_t *next_table;
    // with next_table: the workgroup that finishes last scans next_table in place (exclusive,
    // the rs_scan_* result), clears tail_zero (the table the next pass counts into; this pass's
    // own, read by every workgroup before it finished) and re-arms *done (zero on entry)
    uint32_t *tail_zero;
    uint32_t *done;
    // k = 8 line kernels: != nullptr -> launch_scatter launches the plain and the clustered-input
    // variant (rank_add_hot); *cl_select == kGroupsWhole runs the plain one, anything else (a pass
    // whose digit groups were unbalanced: skewed, duplicate-heavy keys) the clustered one
    const uint32_t *cl_select;
    // whole-line kernels only (set by launch_scatter): kout / vout are moved down to kout's 128-B-
    // aligned base and every output position up by pos_shift (< 32) keys, so lines are cache lines
    // for any 4-B-aligned output
    uint32_t pos_shift;
    // rs_scatter_lines with k <= 4 (next-digit plans, passes after the first): raw_table = 1 -> `table`
    // holds the previous pass's unscanned counts and every workgroup derives its own offsets from the
    // whole table (no tail scan); done[kDoneErr] is set when the table's total is not n. zero_table:
    // != nullptr -> each workgroup clears its R words of this R x num_chunks table (the one the pass
    // after next counts into)
    uint32_t raw_table;
    uint32_t *zero_table;
    // the lane-ordered kernels (rs_scatter_lines, rs_scatter_pairs, rs_scatter with kRankAtomic): != nullptr ->
    // the sort's check word (done + kDoneErr), where a workgroup whose per-tile rank check failed sets
    // kCheckRankOrder; rank_fault != 0: the test hook that swaps two ranks per digit in every checked slot
    uint32_t *check;
    uint32_t rank_fault;
    // hybrid-eligible sorts: as HistArgs::mode (whole-line kernels only)
    const uint32_t *mode;
    uint32_t mode_want;
};

struct ScanArgs {
    uint32_t *table;
    uint32_t *block_sums;
    uint64_t m;             // table entries
    uint32_t nblocks;
    uint32_t *zero;         // optional: zero_n words cleared by the first launch
    uint64_t zero_n;
    uint32_t *done;         // optional: a tail-scan counter (ScatterArgs::done) zeroed by the first launch
    // digit-group plans, odd passes: *group_flag == kGroupsCut -> the first launch assembles the
    // table from the joint counts and the piece counts (cut_entry), the second clears `joint`
    const uint32_t *group_flag;
    uint32_t *joint;
    const uint32_t *plan;
    const uint32_t *pcounts;
    // hybrid-eligible sorts: as HistArgs::mode
    const uint32_t *mode;
    uint32_t mode_want;
};

// Launchers (rsort_kernels.hip). All return hipSuccess or the launch error.
hipError_t launch_histogram(int bits, int dmode, const HistArgs &a, hipStream_t s);
// Digit-group chunks: k = 8 and exactly 2^8 chunks. Pass p counts, besides its own per-chunk
// table, the joint counts of (digit p, digit p + 1) over all keys; pass p + 1's chunks are then
// the digit-p groups of pass p's output, whose per-chunk counts ARE those joint counts, so pass
// p + 1 reads no keys for its histogram.
constexpr int kJointBits = 8;
constexpr uint32_t kJointBins = 1u << kJointBits;
// {flag, chunk starts[0..R], the cut plan's stats}: rs_joint_bounds writes, per odd pass, how its cut plan
// takes its pieces -- key ranges, row tasks (summed joint-count rows), direct adds, negatively counted ranges
// (all 0 for whole groups / fixed chunks); rsort_cut_plan_stats reads them
constexpr uint32_t kBoundsStat = kJointBins + 2;
constexpr uint32_t kBoundsWords = kBoundsStat + 4;
// bounds[0]: how the next pass takes its chunks
//   kGroupsFixed  fixed chunks, histogram counted from the keys (group path off)
//   kGroupsWhole  the digit groups are the chunks (each fits max_keys): table = joint counts
//   kGroupsCut    unbalanced groups (skewed keys): n / R-key chunks, each boundary snapped to a
//                 group boundary within `snap` keys or cutting a group. A cut group's segments
//                 but its largest are counted from the keys ("pieces"), the largest is its
//                 joint column minus the others, every whole group in a chunk is its joint column.
constexpr uint32_t kGroupsFixed = 0, kGroupsWhole = 1, kGroupsCut = 2;
// Cut plan (workspace, rs_joint_bounds): header {key ranges, counted keys, row tasks}, per chunk c a
// descriptor {first group gA | last group gB << 8 | head mode << 16 | tail mode << 18 | empty << 20}
// (head: chunk c's part of gA, slot 2c; tail: its part of gB != gA, slot 2c + 1), per cut group
// {first chunk | last chunk << 8 | derived slot << 16}, the key ranges counted from the keys {start,
// end, slot | kPieceNeg if counted negatively | derived slot << 16, offset among the counted keys}, and
// the row tasks {slot | derived slot << 16, group, first chunk, end chunk} (or direct adds, kRowDirect:
// an end inside a previous chunk whose keys of the group all have one next digit): a counted piece (a cut
// group's part of a chunk, but the group's largest) is the keys of the previous pass's chunks [first,
// end) in that group -- the sum of their joint-count rows (HistArgs::rows) -- plus or minus the keys at
// its two ends (key ranges); without rows the whole piece is one key range. pcounts: kPieceSlots rows
// of R digit counts, one per slot (mod 2^32: a negative range may take a row below zero for a while).
constexpr uint32_t kSegWhole = 0, kSegCounted = 1, kSegDerived = 2;
constexpr uint32_t kPlanDesc = 16;
constexpr uint32_t kPlanGroup = kPlanDesc + kJointBins;
constexpr uint32_t kPlanPieces = kPlanGroup + kJointBins;
constexpr uint32_t kPlanMaxRanges = 4 * kJointBins;  // (<= 255 counted pieces, <= 2 key ranges each)
constexpr uint32_t kPlanRows = kPlanPieces + 4 * kPlanMaxRanges;
constexpr uint32_t kPlanWords = kPlanRows + 4 * 3 * kJointBins;  // (<= 3 tasks per counted piece)
constexpr uint32_t kRowDirect = 0x80000000u;  // row task {slot, kRowDirect | next digit, keys, 0}: a direct add
constexpr uint32_t kPieceSlots = 2 * kJointBins;
constexpr uint32_t kPieceNeg = 0x8000u;  // key range flag (slot word): counted negatively
// joint-count rows: R chunks x R digits x R next digits (64 MiB; then R x R words: each row's one
// next digit, or ~0), and the spills one chunk's rows can hold in LDS (a 16-bit counter spills every
// 2^15 keys: chunk_keys / 2^15 <= 512 at n < 2^32)
constexpr uint64_t kRowsWords = (uint64_t)kJointBins * kJointBins * kJointBins;
constexpr uint32_t kMaxRowSpills = 512;
constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// What a digit-group plan's workspace holds beyond any other plan's of the same n, in layout order (the
// workspace walk, carve in rsort_capi.cpp, takes each 256-B aligned).
constexpr size_t kJointRegionBytes[] = {
    (size_t)kJointBins * kJointBins * 4 + 4,                // joint counts [next digit][digit], rows counter
    (size_t)2 * kBoundsWords * 4,                           // group bounds of passes 1 and 3
    (size_t)kPlanWords * 4,                                 // cut plan
    (size_t)kPieceSlots * kJointBins * 4,                   // its piece counts
    ((size_t)kRowsWords + kJointBins * kJointBins) * 4};    // per-chunk joint-count rows (64 MiB), one-digit words
constexpr size_t joint_extra_bytes() {
    size_t b = 0;
    for (size_t r : kJointRegionBytes) b += align256(r);
    return b;
}
// Their sum: a caller that sizes a workspace for one n and sorts a smaller one (the multi-GPU local sort) adds it.
constexpr size_t kJointExtraBytes = joint_extra_bytes();
hipError_t launch_histogram_joint(const HistArgs &a, hipStream_t s);
// From the joint counts [next digit][group]: the next pass's chunks into bounds[1..R+1] and its
// mode into bounds[0] (above): kGroupsWhole when every group fits in max_keys keys, else the cut
// plan (plan, pcounts rows zeroed); kGroupsFixed when the counts do not add up to n or enable
// says the joint count was off (HistArgs::joint_enable).
struct JointBoundsArgs {
    const uint32_t *joint, *enable;
    uint32_t *bounds, *plan, *pcounts;
    uint64_t n, max_keys;
    uint32_t snap;          // a cut-plan chunk boundary moves to a group boundary up to this many keys away
    uint32_t weighted;      // != 0: a cut plan's chunks get equal estimated cost instead of equal key counts
    // ctab: the counting pass's scanned table; rows_cnt: HistArgs::rows_cnt (read and re-armed here); rowone: the
    // rows' one-digit words (HistArgs::rows + kRowsWords) -- all given and every chunk's rows written: the cut
    // plan's pieces are row tasks + their end keys (or direct adds)
    const uint32_t *ctab, *rowone;
    uint32_t *rows_cnt;
    const uint32_t *mode;   // hybrid-eligible sorts: as HistArgs::mode
    uint32_t mode_want;
};
hipError_t launch_joint_bounds(const JointBoundsArgs &a, hipStream_t s);
// rank_algo: internal RankAlgo. aligned16: the whole-line kernels may run -- keys-only: always
// (any 4-B-aligned kout; launch_scatter shifts positions to kout's 128-B-aligned base); pairs: when
// (vout - kout) % 16 == 0 (otherwise the same plan runs rs_scatter with the same tiles).
hipError_t launch_scatter(int bits, int pairs, int rank_algo, int dmode, int geom, int aligned16,
                          const ScatterArgs &a, hipStream_t s);
// Whether a (bits, pairs, rank_algo, dmode, geom) scatter kernel is compiled in.
bool scatter_available(int bits, int pairs, int rank_algo, int dmode, int geom);
// Whether any scatter kernel is compiled in for digits of `bits` bits on tiles of geometry `geom` (keys or pairs),
// whatever the ranking and the digit mode: the shapes a plan may carry (check_plan).
bool scatter_shape_available(int bits, int pairs, int geom);
hipError_t launch_scan(const ScanArgs &a, hipStream_t s);
hipError_t launch_gather_starts(const uint32_t *table, uint32_t num_chunks, uint32_t bins,
                                uint64_t n, uint32_t *starts, hipStream_t s);
hipError_t launch_diff_starts(const uint32_t *starts, uint32_t bins, uint32_t *hist,
                              hipStream_t s);
hipError_t launch_top_hist_sampled(const uint32_t *keys, uint64_t n, uint32_t top_bits, uint32_t stride,
                                   uint32_t *hist, hipStream_t s);
hipError_t launch_sample(const uint32_t *keys, uint64_t n, uint64_t stride, uint64_t count, uint64_t row_len,
                         uint32_t *out, hipStream_t s);
hipError_t launch_fingerprint(const uint32_t *keys, const uint32_t *vals, uint64_t n, unsigned long long *out,
                              hipStream_t s);
hipError_t launch_gen_uniform(uint32_t *out, uint64_t n, uint64_t seed, hipStream_t s);
hipError_t launch_gen_zipf(uint32_t *out, uint64_t n, uint64_t seed, const uint32_t *cdf,
                           uint64_t ranks, hipStream_t s);
hipError_t launch_gen_iota(uint32_t *out, uint64_t n, uint32_t base, hipStream_t s);
hipError_t launch_widen(const uint32_t *in, unsigned long long *out, uint32_t n, hipStream_t s);
// Resident scatter workgroups per CU (occupancy query), 0 on error.
int scatter_blocks_per_cu(int bits, int pairs, int rank_algo, int geom, int dmode = kDigitShift);
// Names of the scatter kernel instantiations launched since the last reset, ';'-joined into buf
// (truncated to len - 1 characters); returns the full length. reset != 0 clears the record.
size_t scatter_kernels_used(char *buf, size_t len, int reset);
// Names of every scatter kernel instantiation the dispatch can hand out (its selection function over its whole
// argument domain), ';'-joined like scatter_kernels_used. Host only: no device is needed.
size_t scatter_kernels_known(char *buf, size_t len);
// A kernel of another translation unit (the hybrid route's bucket kernel) for that record: registered by name
// on first use and noted as launched.
void note_kernel_used(const void *fn, const char *name);
// rsort_profile_*: while a thread's pause count is > 0 its launches record no phase events (the
// multi-GPU sort's sample sort, which is part of its plan phase, not of the measured passes)
void profile_pause(int delta);
// Workspace check words (every plan: 256 B after the tables): done[0] is the tail-scan counter of next-digit
// plans; done[kDoneErr] is the sort's check word, cleared by pass 0's histogram and read by rsort_plan_check /
// the host entries. Its bits: kCheckTable -- a tail scan or a raw-table pass found a table whose total is not
// n (next-digit plans); kCheckRankOrder -- a lane-ordered scatter kernel's per-tile rank check failed.
constexpr uint32_t kDoneErr = 1;
constexpr uint32_t kCheckTable = 1u, kCheckRankOrder = 2u;
// Where the check word of a sort with plan `p` lies in its workspace `ws` (the host driver's carve): for the
// callers that keep it past the workspace's next user (the multi-GPU sort's halves share one workspace).
const uint32_t *sort_check_word(const rsort_plan &p, const void *ws);

// ------------------------------------------------------------------------------ hybrid route
// (rsort_hybrid.hip; sort_planned in rsort_capi.cpp.) Keys-only k = 8 sorts of ~2^29..2^30 keys whose top 16
// bits spread evenly: two MSD passes by digits 3 and 2 (the line scatter kernel) leave 65536 contiguous buckets,
// and one kernel sorts each bucket by its low 16 bits inside LDS -- three 8-B/key passes instead of four.
// The route is picked on the device: done[kHybMode] is the mode word every kernel of both sequences tests
// (HistArgs::mode), done[kHybGate .. kHybEligible] the report rsort_hybrid_report reads. Pass 0's histogram
// clears the four words with the check words (an ineligible sort: all 0); an eligible sort's exact-count kernel
// (rs_hyb_bounds) writes them.
constexpr uint32_t kHybMode = 4, kHybGate = 5, kHybMax = 6, kHybEligible = 7;
constexpr uint32_t kHybLsd = 0, kHybRun = 2;                       // done[kHybMode]
constexpr uint32_t kGateNone = 0, kGatePass = 1, kGateSkewed = 2;  // done[kHybGate]
// the bucket kernel's shape, rs_bucket_sort16<kHybThreads, kHybKpt>, and the workgroups of it that a CU is to hold
// at once (its register limit: kHybResident * kHybThreads / 256 waves per SIMD)
constexpr int kHybThreads = 1024, kHybKpt = 18, kHybResident = 2;
constexpr uint32_t kHybCapacity = kHybThreads * kHybKpt;  // keys one bucket may hold (18432)
constexpr uint32_t kHybBuckets = kJointBins * kJointBins;
constexpr uint32_t kHybSample = 65536;  // keys the gate reads, at a fixed stride over the whole input ...
constexpr uint32_t kHybGateGroups = 64;  // ... by this many workgroups, each counting its own 1024
// the gate's flag word: after the joint counts and the rows counter, inside the 16 bytes cleared with them
constexpr uint32_t kHybGateFlag = kJointBins * kJointBins + 1;
struct HybArgs {
    const uint32_t *kin;     // gate: the sort's input; bucket phase: pass B's output
    uint32_t *kout;          // bucket phase: the sort's output
    uint32_t *joint;         // [digit 2][digit 3]: the joint counts, scanned in place into the bucket starts
    uint32_t *bounds;        // pass B's chunks {kGroupsWhole, the digit-3 groups' starts[0..R]}
    uint32_t *gflags;        // the sort's group bounds (rsort_group_flags): a hybrid sort reports {groups, none}
    uint32_t *done;          // the check and report words
    uint64_t n;
    uint32_t threshold;      // gate: a top-16-bit bucket with this many sampled keys is skewed
    uint32_t force;          // RSORT_HYBRID_FORCE: the gate reports its verdict and passes anyway
    uint32_t rank_fault;
};
// gate -> joint[kHybGateFlag] != 0: skewed (the joint count then leaves at once: HistArgs::mode points at the
// flag); bounds: clears the check words, writes the verdict and the mode word -- kHybLsd after a skewed verdict,
// else kHybRun when the largest bucket fits kHybCapacity (joint scanned, bounds written) or kHybLsd (joint
// cleared for the LSD passes' own joint count); bucket: the in-LDS finish, grid workgroups (grid-stride over the
// buckets).
hipError_t launch_hyb_gate(const HybArgs &a, hipStream_t s);
hipError_t launch_hyb_bounds(const HybArgs &a, hipStream_t s);
hipError_t launch_hyb_bucket(const HybArgs &a, uint32_t grid, hipStream_t s);
// Lists the bucket kernel in rsort_scatter_kernels_used (called when a sort enqueues the hybrid launches, before
// its first scatter: the record keeps first-use order and its readers take the last plain kernel as the pass's).
void hyb_note_bucket();
// Resident bucket-kernel workgroups per CU (occupancy query), 0 on error.
int hyb_blocks_per_cu();
// rsort_hybrid_kernel_info: {threads per workgroup, static LDS bytes, scratch bytes per lane, hyb_blocks_per_cu()}
hipError_t hyb_kernel_info(int info[4]);

// ------------------------------------------------------------------------------ segmented sort
// (rsort_segmented.hip; rsort_u32_segmented_device.) Four kernels by segment length. Up to kSegWaveKeys keys ONE
// WAVE sorts the segment (4 keys per lane, no workgroup barrier; 4 waves = 4 segments per 256-thread workgroup);
// up to kSegSmallKeys keys a workgroup of 256 threads x 4 keys does (~8 KB of LDS for keys, ~12 KB for pairs:
// 8 workgroups per CU either way); up to kSegLdsKeys keys one of 1024 threads x 16 keys (64 KB of tile, twice
// that for pairs, + 16 KB of per-wave counter rows: one workgroup per CU); longer ones the multi-tile kernel.
// The public classes (rsort_segmented_capacity, rsort_segmented_check) count the first two as "small".
constexpr int kSegWaveKpt = 4;
constexpr int kSegSmallThreads = 256, kSegSmallKpt = 4;
constexpr int kSegLdsThreads = 1024, kSegLdsKpt = 16;
constexpr int kSegWaveKeys = kWave * kSegWaveKpt;
constexpr int kSegSmallKeys = kSegSmallThreads * kSegSmallKpt;
constexpr int kSegLdsKeys = kSegLdsThreads * kSegLdsKpt;
// Kernel kinds (launch_seg_sort) = list and counter indices; kSegRejected has a counter only.
enum SegKind : int { kSegWave = 0, kSegSmall = 1, kSegLds = 2, kSegTiles = 3, kSegRejected = 4, kSegKinds = 4 };
// The call's 256 B of counters and check words: [kind] segments of that kind (the lengths of the lists),
// [kSegRejected] rejected ones, [kSegCheckWord] the check word -- kCheckRankOrder as in a sort's, kCheckOffsets
// when a segment was rejected.
constexpr uint32_t kSegCheckWord = 8;
constexpr uint32_t kCheckOffsets = 4u;
struct SegClassifyArgs {
    const uint32_t *off;        // num_segments + 1 offsets
    uint32_t *lists[kSegKinds]; // per kind: room for num_segments indices
    uint32_t *counters;         // the 256 B above, cleared before the launch
    uint64_t n;
    uint32_t num_segments;
};
struct SegSortArgs {
    const uint32_t *kin;
    const uint32_t *vin;
    uint32_t *kout;
    uint32_t *vout;
    uint32_t *ktmp;           // multi-tile kernel: the workspace ping-pong (n keys, n values)
    uint32_t *vtmp;
    const uint32_t *off;
    const uint32_t *list;     // the class list and its length
    const uint32_t *count;
    uint32_t *check;          // the check word (lane-ordered kernels: kCheckRankOrder)
    uint32_t rank_fault;      // rsort_inject_rank_fault
};
hipError_t launch_seg_classify(const SegClassifyArgs &a, hipStream_t s);
// kind: SegKind; rank_algo: kRankAtomic or kRankCount; grid: workgroups (grid-stride over the list)
hipError_t launch_seg_sort(int kind, int pairs, int rank_algo, const SegSortArgs &a, uint32_t grid, hipStream_t s);
// Resident workgroups per CU of a segmented-sort kernel (occupancy query), 0 on error.
int seg_blocks_per_cu(int kind, int pairs, int rank_algo);
// ------------------------------------------------------------------------------ top-k selection
// (rsort_topk.hip; rsort_u32_topk_device.) A radix select over x = key ^ m (m = ~0 for the k largest): three
// levels of 8 / 12 / 12 bits from the top. Every kernel but the picks runs on G workgroups of kTopkThreads
// threads; workgroup g owns a contiguous slice of whole kTopkTile-key tiles of its list, whose length (n, or the
// device-side candidate count) it reads itself. Level 0 reads the input twice (count, compact): the entries
// below the chosen top digit go to W, those with it to the candidate list A. Levels 1 and 2 count over A; then the
// k-th x, T, is known and one count + one emit over A append x < T and the first k_rem entries x == T to W.
constexpr int kTopkThreads = 1024, kTopkKpt = 4;
constexpr int kTopkTile = kTopkThreads * kTopkKpt;
constexpr uint32_t kTopkMaxGrid = 1024;           // G <= this: the picks handle one slice per thread
constexpr uint32_t kTopkBins0 = 256, kTopkBins = 4096;
constexpr uint32_t kTopkTotalsWords = kTopkBins0 + 2 * kTopkBins;  // the bin totals of levels 0, 1, 2
// The call's 256 B of state, first in the workspace (rsort_topk_report reads words 0..7). A SELECT call clears
// it with the totals; a SORT call fills it with ~0 and writes the route, the k-th key and the reserved words.
// kTkSorted: the host sets it to 1 (a memset node) in front of the sort the call runs -- the finishing sort of k,
// or the whole sort -- so rsort_topk_report reads that sort's check word only where one ran (as kTrSorted).
enum TopkWord : uint32_t { kTkRoute = 0, kTkKth = 1, kTkBefore = 2, kTkTaken = 3, kTkEqual = 4, kTkCand = 5,
                           kTkKrem = 8, kTkPrefix = 9, kTkBelow0 = 10, kTkSorted = 11, kTkWords = 64 };
struct TopkArgs {
    const uint32_t *kin, *vin;   // the input (vin == nullptr: keys only, or indices)
    uint32_t *state, *totals;
    uint32_t *rows_cnt, *rows_pre;  // level 0: [slice][top digit] counts and their exclusive prefix over the digits
    uint32_t *offs0, *offs1;        // per slice {below, equal}: level 0's exclusive offsets; the tie counts
    uint32_t *wk, *wv, *ak, *av;    // W (k entries), A (up to n)
    uint64_t n;
    uint32_t k, m;
    uint32_t pairs, indices, vec;   // vec: kin is 16-byte aligned
};
// level 0..2; grid workgroups (<= kTopkMaxGrid), the same for every launch of one call
hipError_t launch_topk_count(int level, const TopkArgs &a, uint32_t grid, hipStream_t s);
hipError_t launch_topk_pick(int level, const TopkArgs &a, uint32_t grid, hipStream_t s);
hipError_t launch_topk_compact(const TopkArgs &a, uint32_t grid, hipStream_t s);
hipError_t launch_topk_tie_count(const TopkArgs &a, uint32_t grid, hipStream_t s);
hipError_t launch_topk_emit(const TopkArgs &a, uint32_t grid, hipStream_t s);
// kout[i] = kin[rev ? n - 1 - i : i] ^ m (and vout[i] = vin[i]) for i < k; kin == kout is allowed when !rev.
// state != nullptr: the SORT route's report words (the route, the k-th key = kout[k - 1], the reserved zeros).
struct TopkCopyArgs {
    const uint32_t *kin, *vin;
    uint32_t *kout, *vout, *state;
    uint64_t n, k;
    uint32_t m, rev;
};
hipError_t launch_topk_copy(const TopkCopyArgs &a, hipStream_t s);
// Fewest resident workgroups per CU over the select kernels (occupancy query), 0 on error.
int topk_blocks_per_cu();

// ------------------------------------------------------------------------------ row-wise top-k
// (rsort_topk_rows.hip; rsort_u32_topk_rows_device.) One radix select per row of a rows x cols matrix, four 8-bit
// levels from the top. cols is the call's, so the host picks the kernel: the segmented sort's limits and shapes.
enum TopkRowsClass : int { kTrWave = 0, kTrSmall = 1, kTrLds = 2, kTrStream = 3 };
inline int topk_rows_class(int64_t cols) {
    return cols <= kSegWaveKeys ? kTrWave : cols <= kSegSmallKeys ? kTrSmall : cols <= kSegLdsKeys ? kTrLds : kTrStream;
}
// TopkRowsArgs::pairs
enum TopkRowsPairs : uint32_t { kTrKeys = 0, kTrValues = 1, kTrIndices = 2 };
// The call's 256 B of state, first in the workspace and cleared by the call's one memset: words 0..3 are what
// rsort_topk_rows_check reports; kTrSorted: a finishing sort follows (its check word is then valid).
enum TopkRowsWord : uint32_t { kTrClass = 0, kTrBadRows = 1, kTrSorted = 8 };
struct TopkRowsArgs {
    const uint32_t *kin, *vin;   // rows x cols (vin: kTrValues only)
    uint32_t *kout, *vout;       // rows x k
    uint32_t *state;
    uint32_t rows, cols, k, m;
    uint32_t pairs;              // TopkRowsPairs
    uint32_t raw;                // 1 (UNSORTED): the outputs are keys; 0: x = key ^ m, for the finishing sort
};
// cls: TopkRowsClass; grid workgroups, each striding over the rows
hipError_t launch_topk_rows_select(int cls, const TopkRowsArgs &a, uint32_t grid, hipStream_t s);
// off[i] = i * k for i <= rows
hipError_t launch_topk_rows_offsets(uint32_t *off, uint32_t rows, uint32_t k, hipStream_t s);
// Resident workgroups per CU of a class's select kernel (occupancy query), 0 on error.
int topk_rows_blocks_per_cu(int cls);

// ------------------------------------------------------------------------------ host helpers
// (both host drivers, rsort_capi.cpp and rsort_multi.cpp)
inline int hip_status(hipError_t e) { return e == hipSuccess ? RSORT_OK : RSORT_ERR_HIP; }

// Copies `bytes` bytes (read_words: `words` words) of device memory to the host, behind everything enqueued on s,
// and waits for them.
inline int read_bytes(void *host, const void *dev, size_t bytes, hipStream_t s) {
    if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return RSORT_ERR_HIP;
    return hip_status(hipStreamSynchronize(s));
}
inline int read_words(uint32_t *host, const uint32_t *dev, size_t words, hipStream_t s) {
    return read_bytes(host, dev, words * 4, s);
}

// a key count every entry takes: [0, 2^32)
inline bool key_count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 32); }

// The one bump allocator of the workspace layouts (carve, seg_carve, topk_carve, topk_rows_carve, multi_bytes) and of
// the host entries' staging buffer (Staging): regions in the order they are taken, each a multiple of 256 B long,
// `off` the bytes taken so far. A null base is sizing: take returns nullptr and only `off` counts. round_base: the
// regions start at the base's next multiple of 256 (a caller's workspace of any 4-byte alignment).
struct Bump {
    char *base;
    size_t off = 0;
    explicit Bump(void *p, bool round_base = false)
        : base(round_base ? (char *)(((uintptr_t)p + 255u) & ~(uintptr_t)255u) : (char *)p) {}
    uint32_t *take(size_t bytes) {
        uint32_t *q = base ? (uint32_t *)(base + off) : nullptr;
        off += align256(bytes);
        return q;
    }
};

// Raw next-digit tables (every workgroup of a pass sums the whole R x C table for its own starts) cost
// O(R x C) reads per workgroup, O(R x C^2) per pass: only plans of at most this many chunks (about one
// resident wave: C2 has 1024) take them; larger ones keep the tail scan (DESIGN §8 measured
// 2048 chunks 1.155 vs 1.088 ms, 4096 chunks 1.578 vs 1.207 ms per C2 sort against tail scans).
constexpr int64_t kRawTableMaxChunks = 1280;
// Lab switches (A/B runs, dev/lab.sh): the library reads getenv(name) only when RSORT_LAB=1 is set
// too, so a shipped library picks its plans from n, k and the device alone. nullptr otherwise.
inline const char *lab_env(const char *name) {
    const char *lab = getenv("RSORT_LAB");
    if (lab == nullptr || lab[0] != '1') return nullptr;
    return getenv(name);
}
// A boolean lab switch: unset or empty -> def; "0..." -> off; anything else -> on.
inline bool lab_flag(const char *name, bool def) {
    const char *e = lab_env(name);
    return (e == nullptr || e[0] == '\0') ? def : e[0] != '0';
}
// An integer lab switch: its value when inside [lo, hi], else def.
inline long long lab_int(const char *name, long long lo, long long hi, long long def) {
    const char *e = lab_env(name);
    const long long x = e ? atoll(e) : lo - 1;
    return (x >= lo && x <= hi) ? x : def;
}

}  // namespace rsort

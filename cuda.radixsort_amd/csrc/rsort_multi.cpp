// rsort_multi.cpp -- the multi-GPU sort (C ABI): rsort_u32_multi over an RCCL communicator and
// rsort_u32_multi_transport over any rsort_transport (the in-process loopback below is one).
//
// No reference counterpart (the reference sorts on one GPU, Parallel7.cu:10/:697); this is
// SURVEY.md §8e / BASELINE config 5, the same protocol as cuda.radixsort_amd/multi.py (which
// drives the same pure planning functions through torch.distributed):
//   1. all-gather every rank's key count; the sampling plan (rsort_multi_sample_plan)
//   2. a regular sample of the local keys, all-gathered, sorted on the device: the world - 1
//      global quantile keys (exact key values, not bin edges)
//   3. splitters with an equal-keys bucket per hot quantile key (rsort_multi_splitters_make_hot), a
//      stable partition of the local keys into those buckets
//   4. all-gather of the bucket counts and capacities; the exchange plan (rsort_multi_exchange_plan)
//      -- identical on every rank, so a capacity error is returned by all ranks together before
//      any key moves
//   5. ONE exchange: the rank's own range by a device copy, every other message point to point
//      (each pair of GPUs on its own xGMI link), cut into equal rounds of <= 2^28 keys
//   6. local LSD sort of what arrived, in place.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "rsort.h"
#include "rsort_internal.hpp"

using namespace rsort;

namespace {

constexpr int kMaxRanks = RSORT_MAX_RANKS;
constexpr int kMaxBuckets = 2 * kMaxRanks;
// total sample budget over all ranks: quantile error ~ sqrt(1/4/2^20) of the keys (0.05 %)
constexpr int64_t kSampleBudget = (int64_t)1 << 20;
// keys per message of one exchange round (1 GiB): this RCCL (2.26, ROCm 7) leaves the second half
// of an all_to_all / send message of >= 2 GiB unwritten without an error (dev/a2a_lab.py); 1 GiB
// messages arrive whole
constexpr int64_t kMaxPiece = (int64_t)1 << 28;
std::atomic<int64_t> g_piece{kMaxPiece};  // rsort_set_exchange_piece (tests force several rounds)
std::atomic<int> g_multi_opts{0};         // rsort_set_multi_options
std::atomic<int> g_multi_prof{0};         // rsort_multi_set_profiling
std::atomic<int> g_fail_rank{-1}, g_fail_stage{0}, g_fail_status{0};  // rsort_multi_inject_failure (tests)
int injected(int rank, int stage) {
    return (g_fail_rank.load() == rank && g_fail_stage.load() == stage) ? g_fail_status.load() : RSORT_OK;
}
// the calling thread's last profiled multi-GPU sort (the loopback tests run one rank per thread)
thread_local rsort_multi_stats t_stats;
thread_local bool t_stats_valid = false;

// hipEvents at the phase boundaries of one multi-GPU sort, on the caller's stream (profiling only)
struct MultiTimer {
    enum { kStart, kPlan, kPartition, kExchange, kEnd, kMarks };
    bool on = false;
    hipStream_t s;
    hipEvent_t ev[kMarks] = {};
    bool marked[kMarks] = {};
    MultiTimer(bool enable, hipStream_t stream) : s(stream) {
        if (!enable) return;
        on = true;
        for (auto &e : ev)
            if (hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                on = false;
            }
    }
    ~MultiTimer() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int i) {
        if (on && hipEventRecord(ev[i], s) == hipSuccess) marked[i] = true;
    }
    double ms(int a, int b) const {
        float t = 0.f;
        if (!marked[a] || !marked[b] || hipEventElapsedTime(&t, ev[a], ev[b]) != hipSuccess) return 0.0;
        return t;
    }
    // waits for the sort to finish (profiling makes the call synchronous) and keeps the record
    int finish(rsort_multi_stats &st) {
        if (!on) return RSORT_OK;
        mark(kEnd);
        if (hipEventSynchronize(ev[kEnd]) != hipSuccess) return RSORT_ERR_HIP;
        // phases without a mark of their own (the direct world-1 sort) take the time up to the next
        int prev = kStart;
        double *out[kMarks] = {nullptr, &st.ms_plan, &st.ms_partition, &st.ms_exchange, &st.ms_local_sort};
        for (int i = kPlan; i < kMarks; ++i) {
            if (!marked[i]) continue;
            *out[i] = ms(prev, i);
            prev = i;
        }
        st.ms_total = ms(kStart, kEnd);
        t_stats = st;
        t_stats_valid = true;
        return RSORT_OK;
    }
};

// step 1's all-gathered words per rank: key count, values flags, local status
constexpr size_t kNWords = 3, kNStatusWord = 2;
// step 4's: the bucket counts in [0, buckets), then the capacity and the local status at fixed words
constexpr size_t kRowWords = kMaxBuckets + 2, kCapWord = kMaxBuckets, kStatusWord = kMaxBuckets + 1;

// the local sorts of one call: one per half (the direct sort takes the first slot)
constexpr int kCheckSlots = 2;

struct MultiCarve {
    uint32_t *part_k, *part_v;
    uint64_t *n_send, *n_all;      // [kNWords], [world][kNWords]
    uint64_t *c_send, *c_all;      // [kRowWords], [world][kRowWords]: counts, capacity, status
    uint32_t *starts;              // [kMaxBuckets + 1]
    uint32_t *checks;              // [kCheckSlots]: every local sort's check word, copied behind that sort
    uint32_t *samp_send, *samp_all;  // [kSampleBudget + 1], [world][...]: the sample row + the status
    size_t control_bytes;          // the buffers above part_k
    void *sub;                     // partition, sample sort and local sort, in turn
    size_t sub_bytes;
};

size_t sub_bytes(int64_t n, int64_t cap, int k, int pairs, int world) {
    size_t a = rsort_partition_workspace_size(n, kMaxSplitters + 1, pairs);  // (any bucket count: overlap mode)
    // the gathered sample: world rows of at most kSampleBudget samples
    size_t b = rsort_workspace_size(world * kSampleBudget, 8, 0) + ((size_t)4 << 8 << 12);
    // the received count is only known later; a smaller n can pick a geometry with a larger
    // chunk table (<= 2^k x 4096 entries), or a digit-group plan where cap's is not, so leave room
    // for both
    size_t c = rsort_workspace_size(std::max<int64_t>(cap, 1), k, pairs) + ((size_t)4 << k << 12) +
               (k == kJointBits ? kJointExtraBytes : 0);
    return std::max(a, std::max(b, c));
}

// The layout: one Bump walk (rsort_internal.hpp), like the sort's carve; returns its bytes. base == nullptr: sizing.
size_t multi_bytes(int64_t n, int64_t cap, int k, int pairs, int world, MultiCarve *mc, void *base) {
    Bump b(base);
    MultiCarve m{};
    // the collectives' small buffers first: a rank whose workspace is too small for the rest still
    // takes part in them (with its error status, so every rank returns it together)
    m.n_send = (uint64_t *)b.take(kNWords * 8);
    m.n_all = (uint64_t *)b.take((size_t)kMaxRanks * kNWords * 8);
    m.c_send = (uint64_t *)b.take(kRowWords * 8);
    m.c_all = (uint64_t *)b.take((size_t)kMaxRanks * kRowWords * 8);
    m.starts = b.take((size_t)(kMaxBuckets + 1) * 4);
    m.checks = b.take((size_t)kCheckSlots * 4);
    m.samp_send = b.take((size_t)(kSampleBudget + 1) * 4);
    m.samp_all = b.take((size_t)world * (kSampleBudget + 1) * 4);
    m.control_bytes = b.off;
    m.part_k = b.take((size_t)n * 4);
    m.part_v = pairs ? b.take((size_t)n * 4) : nullptr;
    m.sub_bytes = sub_bytes(n, cap, k, pairs, world);
    m.sub = b.take(m.sub_bytes);
    if (mc) *mc = m;
    return b.off;
}

// A second stream per device (with its two events) for work that overlaps the exchange: created on
// first use, kept for the process. Concurrent multi-GPU sorts on one device (the loopback tests'
// ranks) each take their own from a small pool.
struct SideStream {
    int device;
    bool busy;
    hipStream_t s;
    hipEvent_t ready, done;
};
std::mutex g_side_mu;
std::vector<SideStream *> g_side;

SideStream *side_stream() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(g_side_mu);
    for (SideStream *x : g_side)
        if (x->device == dev && !x->busy) {
            x->busy = true;
            return x;
        }
    SideStream *x = new (std::nothrow) SideStream{dev, true, nullptr, nullptr, nullptr};
    if (!x) return nullptr;
    if (hipStreamCreateWithFlags(&x->s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x->ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x->done, hipEventDisableTiming) != hipSuccess) {
        delete x;  // (a partly created stream/event leaks: a HIP failure this early is terminal anyway)
        return nullptr;
    }
    g_side.push_back(x);
    return x;
}

// One sort's use of a side stream beside its own stream `s`, and the only place that touches the two events. Its rule:
// on EVERY way out of the scope while the side stream holds work (an own-range copy, the lower half's sort) `s` first
// waits for it, so a caller that synchronises `s` after an error never frees buffers a side-stream kernel still
// writes; only then does the stream go back to the pool (a later user enqueues behind the work anyway).
struct SideScope {
    SideStream *x;
    hipStream_t s;
    bool pending = false;  // the side stream holds work `s` must wait for
    explicit SideScope(hipStream_t stream) : x(side_stream()), s(stream) {}
    ~SideScope() {
        (void)join();
        std::lock_guard<std::mutex> g(g_side_mu);
        if (x) x->busy = false;
    }
    // where work that may run beside `s` goes: the side stream, behind everything enqueued on `s` so far -- or `s`
    // itself when there is no side stream or it still holds work; mark() after enqueueing on the side stream
    hipStream_t fork() {
        const bool forked = x && !pending && hipEventRecord(x->ready, s) == hipSuccess &&
                            hipStreamWaitEvent(x->s, x->ready, 0) == hipSuccess;
        return forked ? x->s : s;
    }
    int mark() {
        if (hipEventRecord(x->done, x->s) != hipSuccess) return RSORT_ERR_HIP;
        pending = true;
        return RSORT_OK;
    }
    // `s` waits for the side stream's work (a failed wait leaves it pending: the destructor tries again)
    int join() {
        if (pending && hipStreamWaitEvent(s, x->done, 0) != hipSuccess) return RSORT_ERR_HIP;
        pending = false;
        return RSORT_OK;
    }
};

// ------------------------------------------------------------------------------ RCCL transport
// Every RCCL step is bounded: RCCL itself never times out, so a peer that died or
// never joined would leave this rank's kernels spinning and its host waiting forever. Each step's
// calls are completed (a non-blocking communicator returns ncclInProgress until they are), then the
// step's stream work is polled to completion; past the deadline, or on an asynchronous RCCL error,
// the communicator is aborted (ncclCommAbort also stops its kernels) and RSORT_ERR_COMM returned.
std::atomic<int> g_comm_timeout_ms{300000};  // rsort_set_comm_timeout
std::mutex g_aborted_mu;
// communicators a timeout aborted and nobody has released yet: rsort_u32_multi refuses them and
// rsort_rccl_comm_destroy only forgets them (ncclCommAbort freed them). An address leaves the list when
// destroy is called for it and when rsort_rccl_comm_init hands it out again for a new, live communicator
// (freed communicators' addresses are reused, so a stale entry would refuse a live one)
std::vector<void *> g_aborted;

void comm_forget(ncclComm_t c) {
    std::lock_guard<std::mutex> g(g_aborted_mu);
    g_aborted.erase(std::remove(g_aborted.begin(), g_aborted.end(), (void *)c), g_aborted.end());
}

bool comm_aborted(ncclComm_t c) {
    std::lock_guard<std::mutex> g(g_aborted_mu);
    return std::find(g_aborted.begin(), g_aborted.end(), (void *)c) != g_aborted.end();
}

int comm_abort(ncclComm_t c) {
    {
        std::lock_guard<std::mutex> g(g_aborted_mu);
        if (std::find(g_aborted.begin(), g_aborted.end(), (void *)c) != g_aborted.end()) return RSORT_ERR_COMM;
        g_aborted.push_back((void *)c);
    }
    (void)ncclCommAbort(c);
    return RSORT_ERR_COMM;
}

using Clock = std::chrono::steady_clock;

// r == ncclInProgress (a non-blocking communicator): poll until the call has completed
ncclResult_t nb_complete(ncclComm_t c, ncclResult_t r, Clock::time_point deadline) {
    while (r == ncclInProgress) {
        if (Clock::now() > deadline) return ncclInProgress;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (ncclCommGetAsyncError(c, &r) != ncclSuccess) return ncclInternalError;
    }
    return r;
}

// the step's calls returned `r`; now wait (bounded) for its work on `s`
int rccl_finish(ncclComm_t c, ncclResult_t r, hipStream_t s, Clock::time_point deadline) {
    r = nb_complete(c, r, deadline);
    if (r != ncclSuccess) return comm_abort(c);
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return RSORT_ERR_HIP;
    int st = hipEventRecord(ev, s) == hipSuccess ? RSORT_OK : RSORT_ERR_HIP;
    for (int spin = 0; st == RSORT_OK; ++spin) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) {
            st = RSORT_ERR_HIP;
            break;
        }
        ncclResult_t ae = ncclSuccess;
        if (ncclCommGetAsyncError(c, &ae) != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress) ||
            Clock::now() > deadline) {
            st = comm_abort(c);
            break;
        }
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    (void)hipEventDestroy(ev);
    return st;
}

Clock::time_point comm_deadline() { return Clock::now() + std::chrono::milliseconds(g_comm_timeout_ms.load()); }

struct RcclCtx {
    ncclComm_t comm;
};

int rccl_allgather(void *ctx, const void *d_send, void *d_recv, size_t bytes, void *stream) {
    ncclComm_t comm = static_cast<RcclCtx *>(ctx)->comm;
    const Clock::time_point dl = comm_deadline();
    return rccl_finish(comm, ncclAllGather(d_send, d_recv, bytes, ncclUint8, comm, (hipStream_t)stream),
                       (hipStream_t)stream, dl);
}

int rccl_exchange(void *ctx, void *const *d_send, const size_t *send_bytes, void *const *d_recv,
                  const size_t *recv_bytes, void *stream) {
    ncclComm_t comm = static_cast<RcclCtx *>(ctx)->comm;
    int world = 0, me = 0;
    if (ncclCommCount(comm, &world) != ncclSuccess || ncclCommUserRank(comm, &me) != ncclSuccess) return RSORT_ERR_COMM;
    hipStream_t s = (hipStream_t)stream;
    const Clock::time_point dl = comm_deadline();
    // every call inside the group is checked; the group is always closed (an open group would
    // leave the communicator unusable), and the first failure is returned
    ncclResult_t first = ncclGroupStart();
    if (first != ncclSuccess) return comm_abort(comm);
    for (int p = 0; p < world; ++p) {
        if (p == me) continue;
        if (send_bytes[p]) {
            const ncclResult_t r = ncclSend(d_send[p], send_bytes[p], ncclUint8, p, comm, s);
            if (first == ncclSuccess) first = r;
        }
        if (recv_bytes[p]) {
            const ncclResult_t r = ncclRecv(d_recv[p], recv_bytes[p], ncclUint8, p, comm, s);
            if (first == ncclSuccess) first = r;
        }
    }
    const ncclResult_t e = ncclGroupEnd();
    if (first == ncclSuccess || first == ncclInProgress) first = e;
    return rccl_finish(comm, first, s, dl);
}

// ------------------------------------------------------------------------------ loopback transport
// World of `world` ranks in one process (one thread per rank, any devices with peer access, or one
// device): collectives through a host rendezvous and device-to-device copies. Test transport for
// the multi-GPU path on a one-GPU box (RCCL refuses two ranks on one device: "Duplicate GPU
// detected"); every wait is bounded so a protocol bug ends in RSORT_ERR_COMM, not a hang.
struct LoopbackGroup;
struct LoopbackCtx {
    LoopbackGroup *g;
    int rank;
};

struct LoopbackGroup {
    int world;
    LoopbackCtx ctx[kMaxRanks];
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    bool broken = false;
    // posted by each rank between two barriers
    const void *ag_src[kMaxRanks];
    size_t ag_bytes[kMaxRanks];
    void *const *ex_send[kMaxRanks];
    const size_t *ex_send_bytes[kMaxRanks];

    // returns false on timeout (and marks the group broken so every rank fails fast)
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const uint64_t gen = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
            return true;
        }
        const bool ok = cv.wait_for(lk, std::chrono::seconds(120), [&] { return generation != gen || broken; });
        if (!ok || broken) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
};

int lb_allgather(void *ctx, const void *d_send, void *d_recv, size_t bytes, void *stream) {
    LoopbackCtx *c = static_cast<LoopbackCtx *>(ctx);
    LoopbackGroup *g = c->g;
    hipStream_t s = (hipStream_t)stream;
    if (hipStreamSynchronize(s) != hipSuccess) return RSORT_ERR_HIP;  // d_send is ready
    g->ag_src[c->rank] = d_send;
    g->ag_bytes[c->rank] = bytes;
    if (!g->barrier()) return RSORT_ERR_COMM;
    int st = RSORT_OK;
    for (int r = 0; r < g->world && !st; ++r) {
        if (g->ag_bytes[r] != bytes) st = RSORT_ERR_COMM;
        else if (bytes && hipMemcpyAsync((char *)d_recv + (size_t)r * bytes, g->ag_src[r], bytes,
                                         hipMemcpyDeviceToDevice, s) != hipSuccess)
            st = RSORT_ERR_HIP;
    }
    if (!st && hipStreamSynchronize(s) != hipSuccess) st = RSORT_ERR_HIP;
    if (!g->barrier()) return RSORT_ERR_COMM;  // nobody reuses its send buffer before all have copied
    return st;
}

int lb_exchange(void *ctx, void *const *d_send, const size_t *send_bytes, void *const *d_recv,
                const size_t *recv_bytes, void *stream) {
    LoopbackCtx *c = static_cast<LoopbackCtx *>(ctx);
    LoopbackGroup *g = c->g;
    hipStream_t s = (hipStream_t)stream;
    if (hipStreamSynchronize(s) != hipSuccess) return RSORT_ERR_HIP;
    g->ex_send[c->rank] = d_send;
    g->ex_send_bytes[c->rank] = send_bytes;
    if (!g->barrier()) return RSORT_ERR_COMM;
    int st = RSORT_OK;
    for (int p = 0; p < g->world && !st; ++p) {
        if (p == c->rank) continue;
        // what p sends to me must be what I expect to receive from p
        if (g->ex_send_bytes[p][c->rank] != recv_bytes[p]) st = RSORT_ERR_COMM;
        else if (recv_bytes[p] && hipMemcpyAsync(d_recv[p], g->ex_send[p][c->rank], recv_bytes[p],
                                                 hipMemcpyDeviceToDevice, s) != hipSuccess)
            st = RSORT_ERR_HIP;
    }
    if (!st && hipStreamSynchronize(s) != hipSuccess) st = RSORT_ERR_HIP;
    if (!g->barrier()) return RSORT_ERR_COMM;
    return st;
}

// ------------------------------------------------------------------------------ host transport
// rsort_host_transport_wrap: device bytes staged through host buffers for a host-memory transport
struct HostCtx {
    rsort_host_transport host;
    std::vector<char> send, recv;
};

int host_allgather(void *ctx, const void *d_send, void *d_recv, size_t bytes, void *stream) {
    HostCtx *c = static_cast<HostCtx *>(ctx);
    hipStream_t s = (hipStream_t)stream;
    const size_t world = (size_t)c->host.world;
    c->send.resize(std::max<size_t>(bytes, 1));
    c->recv.resize(std::max<size_t>(world * bytes, 1));
    if (bytes && hipMemcpyAsync(c->send.data(), d_send, bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
        return RSORT_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return RSORT_ERR_HIP;
    const int st = c->host.allgather(c->host.ctx, c->send.data(), c->recv.data(), bytes);
    if (st) return st;
    if (bytes && hipMemcpyAsync(d_recv, c->recv.data(), world * bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return RSORT_ERR_HIP;
    return hip_status(hipStreamSynchronize(s));
}

int host_exchange(void *ctx, void *const *d_send, const size_t *send_bytes, void *const *d_recv,
                  const size_t *recv_bytes, void *stream) {
    HostCtx *c = static_cast<HostCtx *>(ctx);
    hipStream_t s = (hipStream_t)stream;
    const int world = c->host.world;
    size_t so[kMaxRanks + 1] = {0}, ro[kMaxRanks + 1] = {0};
    for (int p = 0; p < world; ++p) {
        so[p + 1] = so[p] + send_bytes[p];
        ro[p + 1] = ro[p] + recv_bytes[p];
    }
    c->send.resize(std::max<size_t>(so[world], 1));
    c->recv.resize(std::max<size_t>(ro[world], 1));
    void *hs[kMaxRanks], *hr[kMaxRanks];
    for (int p = 0; p < world; ++p) {
        hs[p] = c->send.data() + so[p];
        hr[p] = c->recv.data() + ro[p];
        if (send_bytes[p] && hipMemcpyAsync(hs[p], d_send[p], send_bytes[p], hipMemcpyDeviceToHost, s) != hipSuccess)
            return RSORT_ERR_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess) return RSORT_ERR_HIP;
    const int st = c->host.exchange(c->host.ctx, hs, send_bytes, hr, recv_bytes);
    if (st) return st;
    for (int p = 0; p < world; ++p)
        if (recv_bytes[p] && hipMemcpyAsync(d_recv[p], hr[p], recv_bytes[p], hipMemcpyHostToDevice, s) != hipSuccess)
            return RSORT_ERR_HIP;
    return hip_status(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------ the sort
// One call's state: the caller's arguments and what the steps below share.
struct MultiCall {
    const uint32_t *keys, *vals;
    int64_t n;  // (0 once the rank has failed its checks: nothing reads the keys of a failed rank)
    uint32_t *keys_out, *vals_out;
    int64_t capacity, *out_n, *out_offset;
    int k_bits, world, me, pairs;
    const rsort_transport *tr;
    hipStream_t s;
    MultiTimer timer;
    // halves per rank, and virtual ranks: world * H (the planning functions run for V ranks; multi_sort)
    int H = 1, V = 1;
    MultiCarve m{};
    // The running local status: every local failure but a missing transport or control buffer is carried to the
    // peers in the next all-gather (a status word per rank) and returned by every rank together -- the lowest rank's
    // first -- instead of leaving the peers waiting in a collective this rank never joins (a rank that dies instead
    // is caught by the RCCL transport's bounded waits: rccl_finish).
    int local = RSORT_OK;
    rsort_multi_stats stats{};
};

// One status-carrying all-gather of rows of `row` words. The last `up` words of this rank's row come from `host`
// (the whole row, or only the status word of a row the device filled); every rank's row is read back into `all`
// -- all == nullptr: only its status word, the one at `at` -- and the lowest rank's non-zero status is returned.
template <class W>
int gather_status(MultiCall &c, const W *host, size_t up, W *d_send, W *d_all, size_t row, size_t at, W *all) {
    if (hipMemcpyAsync(d_send + (row - up), host, up * sizeof(W), hipMemcpyHostToDevice, c.s) != hipSuccess)
        return RSORT_ERR_HIP;
    int st;
    if ((st = c.tr->allgather(c.tr->ctx, d_send, d_all, row * sizeof(W), c.s))) return st;
    W status[kMaxRanks];
    if (all) {
        if ((st = read_bytes(all, d_all, (size_t)c.world * row * sizeof(W), c.s))) return st;
        for (int r = 0; r < c.world; ++r) status[r] = all[r * row + at];
    } else {
        for (int r = 0; r < c.world; ++r)
            if (hip_status(hipMemcpyAsync(&status[r], d_all + r * row + at, sizeof(W), hipMemcpyDeviceToHost, c.s)))
                return RSORT_ERR_HIP;
        if (hipStreamSynchronize(c.s) != hipSuccess) return RSORT_ERR_HIP;
    }
    for (int r = 0; r < c.world; ++r)
        if (status[r] != 0) return (int)status[r];
    return RSORT_OK;
}

// The argument checks past the transport's. A workspace without room for the control buffers is returned at once (the
// rank cannot even tell its peers it failed); everything else becomes the local status.
int check_args(MultiCall &c, void *ws, size_t workspace_bytes) {
    const bool sizes_ok = key_count_ok(c.n) && key_count_ok(c.capacity);
    const int64_t n = sizes_ok ? c.n : 0, cap = sizes_ok ? c.capacity : 0;
    const size_t need = multi_bytes(n, cap, c.k_bits, c.pairs, c.world, &c.m, ws);
    if (workspace_bytes < c.m.control_bytes) return RSORT_ERR_WORKSPACE;
    if (c.k_bits < kMinBits || c.k_bits > kMaxBits) c.local = RSORT_ERR_BITS;
    else if (!sizes_ok) c.local = RSORT_ERR_SIZE;
    else if (!c.out_n || !c.out_offset || (c.n > 0 && !c.keys) || (c.capacity > 0 && !c.keys_out))
        c.local = RSORT_ERR_ARG;
    else if (workspace_bytes < need) c.local = RSORT_ERR_WORKSPACE;
    if (c.local != RSORT_OK) c.n = 0;
    return RSORT_OK;
}

// The local sorts' self-checks. The halves sort one after the other in the same workspace (m.sub), and pass 0 of a
// sort clears the check word the sort before it set: each sort's word is copied into its slot of the control area
// right behind it, on its stream, and the slots are read once when all have run.
int clear_checks(MultiCall &c) { return hip_status(hipMemsetAsync(c.m.checks, 0, (size_t)kCheckSlots * 4, c.s)); }
int keep_check(MultiCall &c, const rsort_plan &p, int slot, hipStream_t ss) {
    return hip_status(hipMemcpyAsync(c.m.checks + slot, sort_check_word(p, c.m.sub), 4, hipMemcpyDeviceToDevice, ss));
}
// waits for the local sorts (the call's last synchronisation of `s`): RSORT_ERR_CHECK when any of them failed
int read_checks(MultiCall &c) {
    uint32_t h[kCheckSlots] = {0};
    int st;
    if ((st = read_words(h, c.m.checks, kCheckSlots, c.s))) return st;
    for (uint32_t w : h)
        if (w & (kCheckTable | kCheckRankOrder)) return RSORT_ERR_CHECK;
    return RSORT_OK;
}

// One rank without RSORT_MULTI_FULL: the partition would be one bucket (a copy) and the exchange a self copy, so the
// keys go straight through the local sort (same output, no peers to agree with).
int sort_direct(MultiCall &c) {
    if (c.local != RSORT_OK) return c.local;
    if (c.n > c.capacity) return RSORT_ERR_CAPACITY;
    c.timer.mark(MultiTimer::kExchange);  // (nothing exchanged: the whole time is the local sort)
    int st;
    rsort_plan p;
    if ((st = clear_checks(c))) return st;
    // (the multi-GPU path's local sorts never take the hybrid route: said here, not left to its gate)
    if (c.n > 0 && ((st = rsort_plan_make(c.n, c.k_bits, c.pairs, 0, &p)) ||
                    (st = rsort_sort_planned_ex(&p, c.keys, c.vals, c.keys_out, c.vals_out, c.m.sub, c.m.sub_bytes, c.s,
                                                RSORT_SORT_NO_HYBRID)) ||
                    (st = keep_check(c, p, 0, c.s))))
        return st;
    if ((st = read_checks(c))) return st;
    *c.out_n = c.n;
    *c.out_offset = 0;
    c.stats.direct = c.stats.halves = 1;
    c.stats.n_out = c.stats.send_keys[0] = c.stats.recv_keys[0] = c.n;
    return c.timer.finish(c.stats);
}

// 1. key counts, value flags and statuses -> the sampling plan. A rank sorts pairs when it passes values or a values
//    output (one with no keys may pass an empty, NULL values input); a mismatch between the ranks is an argument
//    error on every rank (all see the same flags).
int gather_counts(MultiCall &c, rsort_sample_plan *sp) {
    const uint64_t mine[kNWords] = {(uint64_t)c.n, (uint64_t)(c.pairs | (c.vals ? 2 : 0) | (c.vals_out ? 4 : 0)),
                                    (uint64_t)c.local};
    uint64_t nf[kNWords * kMaxRanks];
    int st;
    if ((st = gather_status(c, mine, kNWords, c.m.n_send, c.m.n_all, kNWords, kNStatusWord, nf))) return st;
    int64_t n_all[kMaxRanks] = {0};  // per virtual rank: rank r's keys at r * H, none at the others
    bool any_pairs = false, bad = false;
    for (int r = 0; r < c.world; ++r) {
        n_all[r * c.H] = (int64_t)nf[kNWords * r];
        any_pairs |= (nf[kNWords * r + 1] & 1) != 0;
    }
    for (int r = 0; r < c.world && any_pairs; ++r)
        bad |= !(nf[kNWords * r + 1] & 4) || ((int64_t)nf[kNWords * r] > 0 && !(nf[kNWords * r + 1] & 2));
    if (bad) return RSORT_ERR_ARG;
    if ((st = rsort_multi_sample_plan(c.V, n_all, std::max<int64_t>(1, kSampleBudget / c.V), sp))) return st;
    return sp->row_len > kSampleBudget ? RSORT_ERR_ARG : RSORT_OK;  // (cannot happen: budget / V per virtual rank)
}

// 2. sample (+ this rank's status in the row's last word), gather, sort on the device, read the V - 1 quantile keys
//    and whether each is hot. A failure after the gather stays in c.local (plan_splitters).
int sample_quantiles(MultiCall &c, const rsort_sample_plan &sp, uint32_t *q, int *hot) {
    const MultiCarve &m = c.m;
    const size_t row = (size_t)sp.row_len + 1;
    if (launch_sample(c.keys, (uint64_t)c.n, (uint64_t)sp.stride, (uint64_t)sp.count[c.me * c.H], (uint64_t)sp.row_len,
                      m.samp_send, c.s) != hipSuccess)
        c.local = RSORT_ERR_HIP;
    const uint32_t lst = (uint32_t)c.local;
    int st;
    if ((st = gather_status<uint32_t>(c, &lst, 1, m.samp_send, m.samp_all, row, row - 1, nullptr))) return st;
    if (c.V == 1 || sp.total <= 0) return RSORT_OK;
    // the rows (each followed by its status word) sorted as one array: the status words are 0 and sort first, so
    // the quantile positions move up by world (and the rows' padding, 0xFFFFFFFF, sorts after the sp.total samples)
    const int64_t ns = (int64_t)c.world * (int64_t)row;
    profile_pause(1);  // (its passes are part of the plan phase, not the measured local sort)
    c.local = rsort_u32_device(m.samp_all, m.samp_all, ns, 8, m.sub, m.sub_bytes, c.s);
    profile_pause(-1);
    // its self-check, read with the quantile keys below (an unstable sample sort gives unsorted quantiles)
    uint32_t check = 0;
    rsort_plan sort_plan;
    if (!c.local) c.local = rsort_plan_make(ns, 8, 0, 0, &sort_plan);  // (rsort_u32_device's plan)
    if (!c.local && hipMemcpyAsync(&check, sort_check_word(sort_plan, m.sub), 4, hipMemcpyDeviceToHost, c.s) != hipSuccess)
        c.local = RSORT_ERR_HIP;
    // each quantile key and the samples hot_reach away on both sides: the key is hot (its own equal-keys bucket,
    // rsort_multi_splitters_make_hot) when either is the same key
    const int64_t L = std::max<int64_t>(1, sp.total / ((int64_t)c.V * 128));
    uint32_t nb[kMaxRanks][2];
    for (int i = 1; i < c.V && !c.local; ++i) {
        const int64_t qi = rsort_multi_quantile_index(&sp, i);
        const int64_t at[3] = {qi, qi - L, qi + L};
        uint32_t *dst[3] = {&q[i - 1], &nb[i - 1][0], &nb[i - 1][1]};
        nb[i - 1][0] = nb[i - 1][1] = 0;
        for (int j = 0; j < 3 && !c.local; ++j) {
            if (at[j] < 0 || at[j] >= sp.total) continue;  // (a neighbour outside the samples: not hot there)
            if (hipMemcpyAsync(dst[j], m.samp_all + c.world + at[j], 4, hipMemcpyDeviceToHost, c.s) != hipSuccess)
                c.local = RSORT_ERR_HIP;
        }
    }
    if (!c.local && hipStreamSynchronize(c.s) != hipSuccess) c.local = RSORT_ERR_HIP;
    if (!c.local && (check & (kCheckTable | kCheckRankOrder))) c.local = RSORT_ERR_CHECK;
    for (int i = 1; i < c.V && !c.local; ++i) {
        const int64_t qi = rsort_multi_quantile_index(&sp, i);
        hot[i - 1] = (qi - L >= 0 && nb[i - 1][0] == q[i - 1]) || (qi + L < sp.total && nb[i - 1][1] == q[i - 1]);
    }
    if (!c.local) c.local = injected(c.me, 1);
    return RSORT_OK;
}

// 3. the splitters. A rank that failed since the last status exchange (the sample sort, a quantile copy) still joins
//    the next all-gather with a row of its peers' size and its status in it: it plans on placeholder quantiles (all 0,
//    monotone) instead of its partial ones, and a failure of the pure planning is carried the same way, not returned.
void plan_splitters(MultiCall &c, uint32_t *q, int *hot, rsort_multi_splitters *spl) {
    if (c.local) {
        memset(q, 0, kMaxRanks * sizeof(*q));
        memset(hot, 0, kMaxRanks * sizeof(*hot));
    }
    const int st = rsort_multi_splitters_make_hot(c.V, q, hot, spl);  // pure, identical on every healthy rank
    if (st) {
        if (!c.local) c.local = st;
        memset(spl, 0, sizeof(*spl));
        spl->world = c.V;
    }
    c.timer.mark(MultiTimer::kPlan);
}

// 3-4. stable partition into the splitters' buckets; then count matrix + capacities + statuses -> every virtual rank's
//      exchange plan, xv[V] (the same on every rank: a capacity error comes back from all of them before any key moves)
int partition_and_plan(MultiCall &c, const rsort_multi_splitters &spl, rsort_exchange_plan *xv) {
    const MultiCarve &m = c.m;
    const int world = c.world, H = c.H, buckets = std::min(spl.nsplit + 1, kMaxSplitters + 1);
    int &local = c.local;
    if (spl.nsplit + 1 > kMaxSplitters + 1 && !local) local = RSORT_ERR_ARG;  // (pure: every rank alike)
    uint32_t starts[kMaxBuckets + 1] = {0};
    if (!local) local = injected(c.me, 2);
    if (!local)
        local = rsort_partition_device(c.keys, c.vals, m.part_k, m.part_v, c.n, spl.split, buckets, m.starts, m.sub,
                                       m.sub_bytes, c.s);
    if (!local) local = read_words(starts, m.starts, (size_t)(buckets + 1), c.s);
    if (!local) {  // the partition's self-check (its scatter's rank check): a failure stops every rank below
        int pf = 0;
        local = rsort_partition_check(c.n, buckets, c.vals != nullptr ? 1 : 0, m.sub, &pf, c.s);
        if (!local && pf) local = RSORT_ERR_CHECK;
    }
    // (a row of fixed size whatever this rank's bucket count -- a failed rank's may differ: the all-gather matches)
    uint64_t rowc[kRowWords] = {0}, all[kMaxRanks * kRowWords];
    for (int b = 0; b < buckets && !local; ++b) rowc[b] = (uint64_t)(starts[b + 1] - starts[b]);
    rowc[kCapWord] = (uint64_t)c.capacity;
    rowc[kStatusWord] = (uint64_t)local;
    int st;
    if ((st = gather_status(c, rowc, kRowWords, m.c_send, m.c_all, kRowWords, kStatusWord, all))) return st;
    int64_t counts[kMaxRanks * kMaxBuckets] = {0}, caps[kMaxRanks], cap_of[kMaxRanks];
    for (int r = 0; r < world; ++r) {
        for (int b = 0; b < buckets; ++b) counts[r * H * buckets + b] = (int64_t)all[r * kRowWords + b];
        cap_of[r] = (int64_t)all[r * kRowWords + kCapWord];
        for (int h = 0; h < H; ++h) caps[r * H + h] = cap_of[r];  // (the halves' sum is checked below)
    }
    for (int v = 0; v < c.V; ++v) {
        st = rsort_multi_exchange_plan(c.V, v, buckets, counts, &spl, caps, &xv[v]);
        if (st != RSORT_OK && st != RSORT_ERR_CAPACITY) return st;
    }
    for (int r = 0; r < world; ++r) {  // the capacity check is on each rank's total
        int64_t tot = 0;
        for (int h = 0; h < H; ++h) tot += xv[r * H + h].n_recv;
        if (tot > cap_of[r]) return RSORT_ERR_CAPACITY;
    }
    return RSORT_OK;
}

// 5. half h's exchange into ok / ov: the own range by a device copy beside the messages (on the side stream where it
//    is free), every other message through the transport on `s`, in equal rounds of <= the piece limit
int exchange_half(MultiCall &c, SideScope &side, const rsort_exchange_plan &xs, const rsort_exchange_plan &xd, int h,
                  uint32_t *ok, uint32_t *ov, int64_t rounds, int64_t piece) {
    const MultiCarve &m = c.m;
    const int me = c.me, H = c.H, own_dst = me * H + h, own_src = me * H;
    if (xs.send_cnt[own_dst] != xd.recv_cnt[own_src]) return RSORT_ERR_ARG;
    int st;
    const int64_t own = xs.send_cnt[own_dst], from = xs.send_off[own_dst], to = xd.recv_off[own_src];
    if (own > 0) {
        const hipStream_t cs = side.fork();
        for (int arr = 0; arr < (c.pairs ? 2 : 1); ++arr)
            if (hipMemcpyAsync((arr ? ov : ok) + to, (arr ? m.part_v : m.part_k) + from, (size_t)own * 4,
                               hipMemcpyDeviceToDevice, cs) != hipSuccess)
                return RSORT_ERR_HIP;
        if (cs != c.s && (st = side.mark())) return st;
    }
    for (int64_t rd = 0; rd < rounds; ++rd) {
        for (int arr = 0; arr < (c.pairs ? 2 : 1); ++arr) {
            uint32_t *src = arr ? m.part_v : m.part_k, *dst = arr ? ov : ok;
            void *sp[kMaxRanks], *rp[kMaxRanks];
            size_t sb[kMaxRanks], rb[kMaxRanks];
            for (int p = 0; p < c.world; ++p) {
                const int dv = p * H + h, sv = p * H;  // virtual destination / source
                const int64_t a0 = std::min(xs.send_cnt[dv], rd * piece), a1 = std::min(xs.send_cnt[dv], (rd + 1) * piece);
                const int64_t b0 = std::min(xd.recv_cnt[sv], rd * piece), b1 = std::min(xd.recv_cnt[sv], (rd + 1) * piece);
                sp[p] = src + xs.send_off[dv] + a0;
                rp[p] = dst + xd.recv_off[sv] + b0;
                sb[p] = p == me ? 0 : (size_t)(a1 - a0) * 4;
                rb[p] = p == me ? 0 : (size_t)(b1 - b0) * 4;
            }
            if ((st = c.tr->exchange(c.tr->ctx, sp, sb, rp, rb, c.s))) return st;
        }
    }
    return RSORT_OK;
}

// 6. local sort of the n keys that arrived in ok / ov, in place; beside: on the side stream, while the next half is
//    exchanged on `s` (the side stream then holds work, so that half's own copy stays on `s`)
int sort_half(MultiCall &c, SideScope &side, int64_t n, uint32_t *ok, uint32_t *ov, int slot, bool beside) {
    if (n <= 0) return RSORT_OK;
    int st;
    rsort_plan p;
    if ((st = rsort_plan_make(n, c.k_bits, c.pairs, 0, &p))) return st;
    const hipStream_t ss = beside ? side.fork() : c.s;
    // (a rank's keys cover 1 / N of the key space: their (digit 3, digit 2) buckets would overflow)
    if ((st = rsort_sort_planned_ex(&p, ok, ov, ok, ov, c.m.sub, c.m.sub_bytes, ss, RSORT_SORT_NO_HYBRID))) return st;
    st = keep_check(c, p, slot, ss);
    if (ss != c.s) {  // (the side stream holds the sort whether or not the copy went in behind it)
        const int marked = side.mark();
        if (!st) st = marked;
    }
    return st;
}

// 5-6. per half: the exchange, then the local sort of what arrived (the first half's beside the second's exchange)
int exchange_and_sort(MultiCall &c, const rsort_exchange_plan *xv) {
    const int me = c.me, H = c.H;
    const rsort_exchange_plan &xs = xv[me * H];  // (this rank sends as virtual rank me * H, receives as me * H + h)
    int st;
    int64_t rounds = 0, piece = 0;
    if ((st = rsort_multi_exchange_rounds(xs.max_message, g_piece.load(), &rounds, &piece))) return st;
    c.timer.mark(MultiTimer::kPartition);
    c.stats.halves = H;
    c.stats.rounds = rounds;
    for (int p = 0; p < c.world; ++p)
        for (int h = 0; h < H; ++h) {
            c.stats.send_keys[p] += xs.send_cnt[p * H + h];
            c.stats.recv_keys[p] += xv[me * H + h].recv_cnt[p * H];
        }
    if ((st = clear_checks(c))) return st;
    SideScope side(c.s);  // (every return below leaves through its destructor)
    int64_t base = 0;
    for (int h = 0; h < H; ++h) {
        const rsort_exchange_plan &xd = xv[me * H + h];
        const bool last = h + 1 == H;
        uint32_t *ok = c.keys_out + base, *ov = c.pairs ? c.vals_out + base : nullptr;
        if ((st = exchange_half(c, side, xs, xd, h, ok, ov, rounds, piece))) return st;
        // this half has arrived (on `s`, and its own range on the side stream); under the overlap the exchange
        // phase ends with the last message, before waiting for the lower half's sort
        if (last && H > 1) c.timer.mark(MultiTimer::kExchange);
        if ((st = side.join())) return st;
        if (last && H == 1) c.timer.mark(MultiTimer::kExchange);
        if ((st = sort_half(c, side, xd.n_recv, ok, ov, h, !last))) return st;
        base += xd.n_recv;
    }
    if ((st = side.join())) return st;
    if ((st = read_checks(c))) return st;
    *c.out_n = c.stats.n_out = base;
    *c.out_offset = xs.offset;
    return c.timer.finish(c.stats);
}

int multi_sort(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n, uint32_t *d_keys_out, uint32_t *d_vals_out,
               int64_t capacity, int64_t *out_n, int64_t *out_offset, int k_bits, const rsort_transport *tr,
               void *d_workspace, size_t workspace_bytes, hipStream_t s) {
    // (without a transport, its place in it and the control buffers a rank cannot even tell its peers it failed)
    if (!tr || !tr->allgather || !tr->exchange || !d_workspace) return RSORT_ERR_ARG;
    const int world = tr->world, me = tr->rank, opts = g_multi_opts.load();
    if (world < 1 || world > kMaxRanks || me < 0 || me >= world) return RSORT_ERR_ARG;
    const int pairs = (d_vals != nullptr || d_vals_out != nullptr) ? 1 : 0;  // (the ranks agree on it in step 1)
    MultiCall c{d_keys, d_vals, n, d_keys_out, d_vals_out, capacity, out_n, out_offset, k_bits, world, me, pairs,
                tr, s, MultiTimer(g_multi_prof.load() != 0, s)};
    int st;
    if ((st = check_args(c, d_workspace, workspace_bytes))) return st;
    c.stats.world = world;
    c.stats.rank = me;
    c.stats.n_in = c.n;
    c.stats.bytes_per_key = pairs ? 8 : 4;
    c.timer.mark(MultiTimer::kStart);
    if (world == 1 && !(opts & RSORT_MULTI_FULL)) return sort_direct(c);
    // RSORT_MULTI_OVERLAP (automatic: 2 <= world <= RSORT_MULTI_AUTO_OVERLAP_MAX_WORLD, rsort.h and DESIGN §5): every
    // rank's key range is cut in two; the lower half is exchanged first and sorted while the upper half is exchanged
    const bool ov = (opts & RSORT_MULTI_OVERLAP) != 0 ||
                    (!(opts & RSORT_MULTI_NO_OVERLAP) && world <= RSORT_MULTI_AUTO_OVERLAP_MAX_WORLD);
    c.H = (ov && world >= 2 && 2 * world <= kMaxRanks) ? 2 : 1;
    c.V = world * c.H;
    rsort_sample_plan sp;
    uint32_t q[kMaxRanks] = {0};
    int hot[kMaxRanks] = {0};
    rsort_multi_splitters spl;
    rsort_exchange_plan xv[kMaxRanks];
    if ((st = gather_counts(c, &sp))) return st;               // 1
    if ((st = sample_quantiles(c, sp, q, hot))) return st;     // 2
    plan_splitters(c, q, hot, &spl);                           // 3
    if ((st = partition_and_plan(c, spl, xv))) return st;      // 3-4
    return exchange_and_sort(c, xv);                           // 5-6
}

}  // namespace

extern "C" {

size_t rsort_multi_workspace_size(int64_t n, int64_t capacity, int k_bits, int pairs, int world) {
    if (n < 0 || capacity < 0 || world < 1 || world > kMaxRanks) return 0;
    return multi_bytes(n, capacity, k_bits, pairs ? 1 : 0, world, nullptr, nullptr);
}

int rsort_u32_multi_transport(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n, uint32_t *d_keys_out,
                              uint32_t *d_vals_out, int64_t capacity, int64_t *out_n, int64_t *out_offset, int k_bits,
                              const rsort_transport *transport, void *d_workspace, size_t workspace_bytes,
                              void *stream) {
    return multi_sort(d_keys, d_vals, n, d_keys_out, d_vals_out, capacity, out_n, out_offset, k_bits, transport,
                      d_workspace, workspace_bytes, (hipStream_t)stream);
}

int rsort_u32_multi(const uint32_t *d_keys, const uint32_t *d_vals, int64_t n, uint32_t *d_keys_out,
                    uint32_t *d_vals_out, int64_t capacity, int64_t *out_n, int64_t *out_offset, int k_bits,
                    void *nccl_comm, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!nccl_comm) return RSORT_ERR_ARG;
    if (comm_aborted((ncclComm_t)nccl_comm)) return RSORT_ERR_COMM;  // (a timeout aborted it earlier)
    RcclCtx ctx{(ncclComm_t)nccl_comm};
    int world = 0, me = 0;
    if (ncclCommCount(ctx.comm, &world) != ncclSuccess || ncclCommUserRank(ctx.comm, &me) != ncclSuccess)
        return RSORT_ERR_COMM;
    rsort_transport tr{&ctx, world, me, rccl_allgather, rccl_exchange};
    return multi_sort(d_keys, d_vals, n, d_keys_out, d_vals_out, capacity, out_n, out_offset, k_bits, &tr,
                      d_workspace, workspace_bytes, (hipStream_t)stream);
}

int rsort_rccl_unique_id(void *id128) {
    if (!id128) return RSORT_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "NCCL_UNIQUE_ID_BYTES");
    return ncclGetUniqueId(static_cast<ncclUniqueId *>(id128)) == ncclSuccess ? RSORT_OK : RSORT_ERR_COMM;
}

int rsort_rccl_comm_init(void **comm, int world, int rank, const void *id128, int timeout_ms) {
    if (!comm || !id128 || world < 1 || rank < 0 || rank >= world) return RSORT_ERR_ARG;
    *comm = nullptr;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;  // returns at once; setup runs in the background and is polled below
    ncclComm_t c = nullptr;
    ncclResult_t r = ncclCommInitRankConfig(&c, world, id, rank, &cfg);
    if (c == nullptr) return RSORT_ERR_COMM;
    comm_forget(c);  // (a new communicator at the address of one aborted earlier: this one is live)
    const int ms = timeout_ms > 0 ? timeout_ms : g_comm_timeout_ms.load();
    r = nb_complete(c, r, Clock::now() + std::chrono::milliseconds(ms));
    if (r != ncclSuccess) return comm_abort(c);  // (a peer never joined, or setup failed)
    *comm = c;
    return RSORT_OK;
}

int rsort_rccl_comm_destroy(void *comm) {
    if (!comm) return RSORT_ERR_ARG;
    if (comm_aborted((ncclComm_t)comm)) {  // released by the abort: only forget it
        comm_forget((ncclComm_t)comm);
        return RSORT_OK;
    }
    return ncclCommDestroy((ncclComm_t)comm) == ncclSuccess ? RSORT_OK : RSORT_ERR_COMM;
}

int rsort_set_comm_timeout(int timeout_ms) {
    const int old = g_comm_timeout_ms.load();
    if (timeout_ms > 0) g_comm_timeout_ms.store(timeout_ms);
    return old;
}

int rsort_multi_inject_failure(int rank, int stage, int status) {
    if (rank < 0) {
        g_fail_rank.store(-1);
        g_fail_stage.store(0);
        return RSORT_OK;
    }
    if (stage < 1 || stage > 2 || status == RSORT_OK) return RSORT_ERR_ARG;
    g_fail_status.store(status);
    g_fail_stage.store(stage);
    g_fail_rank.store(rank);
    return RSORT_OK;
}

int rsort_multi_set_profiling(int enable) { return g_multi_prof.exchange(enable ? 1 : 0); }

int rsort_multi_last_stats(rsort_multi_stats *out) {
    if (!out || !t_stats_valid) return RSORT_ERR_ARG;
    *out = t_stats;
    return RSORT_OK;
}

int rsort_set_multi_options(int flags) {
    if ((flags & RSORT_MULTI_OVERLAP) && (flags & RSORT_MULTI_NO_OVERLAP)) return -RSORT_ERR_ARG;
    return g_multi_opts.exchange(flags & (RSORT_MULTI_OVERLAP | RSORT_MULTI_FULL | RSORT_MULTI_NO_OVERLAP));
}

int64_t rsort_set_exchange_piece(int64_t keys) {
    const int64_t old = g_piece.load();
    if (keys >= 64 && keys <= kMaxPiece) g_piece.store(keys);
    return old;
}

int rsort_host_transport_wrap(const rsort_host_transport *host, rsort_transport *out) {
    if (!host || !out || !host->allgather || !host->exchange || host->world < 1 || host->world > kMaxRanks ||
        host->rank < 0 || host->rank >= host->world)
        return RSORT_ERR_ARG;
    HostCtx *c = new (std::nothrow) HostCtx();
    if (!c) return RSORT_ERR_ALLOC;
    c->host = *host;
    *out = rsort_transport{c, host->world, host->rank, host_allgather, host_exchange};
    return RSORT_OK;
}

void rsort_host_transport_free(rsort_transport *wrapped) {
    if (!wrapped || wrapped->allgather != host_allgather) return;
    delete static_cast<HostCtx *>(wrapped->ctx);
    wrapped->ctx = nullptr;
}

int rsort_loopback_create(int world, void **group) {
    if (!group || world < 1 || world > kMaxRanks) return RSORT_ERR_ARG;
    LoopbackGroup *g = new (std::nothrow) LoopbackGroup();
    if (!g) return RSORT_ERR_ALLOC;
    g->world = world;
    for (int r = 0; r < world; ++r) g->ctx[r] = LoopbackCtx{g, r};
    *group = g;
    return RSORT_OK;
}

int rsort_loopback_transport(void *group, int rank, rsort_transport *out) {
    LoopbackGroup *g = static_cast<LoopbackGroup *>(group);
    if (!g || !out || rank < 0 || rank >= g->world) return RSORT_ERR_ARG;
    *out = rsort_transport{&g->ctx[rank], g->world, rank, lb_allgather, lb_exchange};
    return RSORT_OK;
}

void rsort_loopback_destroy(void *group) {
    delete static_cast<LoopbackGroup *>(group);
}

}  // extern "C"

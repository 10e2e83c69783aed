// gn_host.h -- internal header of the Gauss-Newton host driver: the per-call types (Layout, Plan,
// Staging, Ctx) and the functions that cross its translation units
//   gn_plan.hip     staging, workspace layout, pose-graph plan, elimination-plan and PCG policies
//   gn_enqueue.hip  the per-iteration enqueue functions
//   gn_driver.hip   setup, the iteration loop, the deferred timeout report
//   gn_api.hip      the C ABI (include/m3s_backend.h), debug extraction, bench profiling hooks
// An M3S_* switch read through env_int()/getenv() in a function body is read on every call of
// that function; one held in a function-local `static` is latched on first use for the process
// (INTEGRATION.md §7 lists which is which).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/m3s_backend.h"
#include "gn_kernels.h"
#include "m3s_common.h"
#include "sparse_plan.h"

namespace m3s {

int env_int(const char* name, int dflt);  // atoi(getenv(name)), or dflt when unset

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Optional phase timing with HIP events on the GN stream (bench.py roofline; gn_api.hip).
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> pool;
    std::vector<hipEvent_t> marks;  // per iteration: t0 accum t1 system t2 solve t3 retract t4
    hipEvent_t get();
    bool accum_only = false;  // record only the two events bracketing the accumulate kernel
    // (every timed event record is a queue marker; with a release to system scope it left ~5 us
    // of idle GPU each, so the timed bench region carries only the accumulate pair)
    std::vector<char> first;  // accum_only: per event pair, the launch built the packed records
    void mark(hipStream_t st, bool accum = false, bool first_pack = false);
};
extern Prof g_prof;

// the last call's diagnostics (M3S_GN_DEBUG_FLAGS; read by m3s_gn_debug_flags / _pcg_stats / _pcg_plan)
extern int g_dbg_flags[4];     // done, fail, packed, ray-constrained accumulate
extern int g_dbg_pcg[5];       // PCG solves, their CG steps, fallbacks, PCG planned, first PCG iteration
extern int g_dbg_pcg_plan[5];  // pcg_R, pcg_nwg, pcg_onex, pcg_lag, pcg_nitem (0 when none planned)

// Pinned host staging for the per-call plan transfers (D2H of ii/jj/K, H2D of the plan
// integers): one buffer per host thread, reused across calls.  The H2D copies of a call are
// asynchronous; the next call waits for them (an event) before overwriting the buffer.
struct Staging {
    char* buf = nullptr;
    char* dev = nullptr;  // buf's device address (the stage-copy kernel reads it directly)
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
    // no destructor: released by m3s_shutdown (m3s_common.h)
    static void release(void* p);
    // a buffer of >= bytes, free of in-flight copies
    char* get(size_t bytes);
    // H2D of [h, h + bytes) (inside buf) to dst, stream-ordered: by a kernel reading the pinned
    // buffer (default), or by hipMemcpyAsync (M3S_STAGE_DMA=1, or no device address)
    hipError_t upload(void* dst, const char* h, size_t bytes, hipStream_t st);
    // D2H of bytes from src (device) into [h, h + bytes) (inside buf), stream-ordered: by the
    // same copy kernel writing the pinned buffer through its device address (default; a DMA
    // transfer's queue handshake costs more than the copy at these sizes), or by
    // hipMemcpyAsync (M3S_STAGE_DMA=1, unaligned, or no device address)
    hipError_t download(char* h, const void* src, size_t bytes, hipStream_t st);
    hipError_t mark(hipStream_t st);
};
// Per host thread, created on first use and registered for m3s_shutdown (a thread that ends
// leaves its buffers to the shutdown).  The thread_local objects are plain pointers: nothing
// runs at thread or process exit.
struct Stagings {
    Staging in;   // D2H
    Staging out;  // H2D: the sparse solver's plan
    Staging ws;   // H2D: the workspace's plan (CSR lists, schedule)
    Staging tmo;  // D2H: the last call's timeout flag (deferred report, see take_deferred_timeout)
    int tmo_armed = 0;  // 0: nothing to report; 1: tmo holds an int flag; 2: a double (rank sum)
    static void release(void* p);
};
Stagings& stagings();

struct Layout {
    size_t partials, edgeblk, compact, x, flags, ii_loc, jj_loc, blk_ptr, blk_ent, blk_ref, grad_ptr,
        grad_ent, ecnt, cok, sorder, sched, pack, packx, pcnt, zs, twc_save, total;
    int nchunks, npad, nblk_max;
};
Layout make_layout(int mode, int64_t N, int64_t HW, int64_t E_total, int64_t E_local);
int chunk_points(int64_t HW, int nchunks);

// Host-side plan of the pose graph (identical on every rank: built from ALL edges).
struct Plan {
    int nblk = 0;
    std::vector<int> ii_loc, jj_loc;              // local edges: Twc/Xs rows
    std::vector<int> blk_ptr, blk_ent;            // CSR: slot -> (edge<<1 | neg)
    std::vector<int> blk_ref;                     // the same entries as (edge<<3 | type), gn_refacc.hip
    std::vector<int> grad_ptr, grad_ent;          // CSR: pose -> (edge<<1 | neg)
    std::vector<int> slotmap;                     // (npose x npose) -> slot or -1
    std::vector<std::pair<int, int>> pairs;      // slot nblk0.. -> unordered pose pair (a<b)
    float K[4] = {0, 0, 0, 0};
    // Edge-ordered exchange of a sharded call: the ranks' per-edge records are all-gathered into
    // nranks blocks of gchunk records (rank r's edges at r * gchunk), and the CSR lists cover ALL
    // edges in edge order by their gathered position -- every rank assembles exactly the sum one
    // GPU does, so the poses do not depend on the rank count
    bool gather = false;
    int grank = 0, granks = 1, gchunk = 0;
};

// the host plans, per thread across calls (Ctx below)
Plan& tls_plan();
SparsePlan& tls_sparse_plan();

struct Ctx {
    bool need_slotmap = false;  // dense solver / debug system: upload the slot table
    bool packed = false;  // per-call packed stream (gn_pack_kernel) feeds the accumulate
    bool compact = false;  // ... holding only the live points (gn_pack_compact_kernel)
    bool ref_order = false;  // M3S_GN_ORDER_REFERENCE: gn_refacc.hip accumulate + assembly
    bool pack_issued = false;  // prepare_iterations already enqueued (setup's early pack)
    bool acc_enqueued = false;  // iteration 0's accumulate enqueued before the planning
    bool gathered = false;      // ... and, edge-sharded, its records' all-gather too
    // the first accumulate of the call builds the packed records (no separate pack pass)
    bool first_pack = false;
    RefParams R;
    Layout L;
    // the host plans, per thread across calls: their lists keep their capacity (fresh
    // allocations of this size cost a page fault per 4 KiB on every call; sparse_plan.h)
    Plan& plan = tls_plan();
    SparsePlan& sp = tls_sparse_plan();
    AccParams P;
    EdgeSrc es{};
    bool vec;
    char* ws;
    hipStream_t st = nullptr;
    // dense solver / debug system: (npad+64) x npad f64 matrix (RHS as a border row), its 64x64
    // tile inverses and the (npose x npose) slot table, one stream-ordered allocation
    char* dyn = nullptr;
    size_t o_dense = 0, o_linv = 0, o_slot = 0;
    double* eall = nullptr;  // Plan::gather: every rank's edge records (granks x gchunk)
    // where this rank's accumulate writes its f64 edge records, and what the assembly reads
    double* eblk() const {
        return eall ? eall + (size_t)plan.grank * plan.gchunk * kEdgeBlk : at<double>(L.edgeblk);
    }
    const double* eblk_all() const { return eall ? eall : at<double>(L.edgeblk); }
    int chol_epoch = 0;  // dataflow factorisations enqueued in this call (chol_df.hip ready words)
    int pcg_launches = 0;  // PCG launches enqueued in this call (their exchange tags)
    // an M refresh enqueued on the side stream that the call's stream has not waited for yet
    bool inv_pending = false;
    hipEvent_t inv_done = nullptr;
    bool may_timeout = false;  // a solver with bounded device-side waits ran (kFlagTimeout)
    template <typename T>
    T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }
    template <typename T>
    T* dyn_at(size_t off) const { return reinterpret_cast<T*>(dyn + off); }
    int alloc_dense(int npad, int npose) {
        size_t off = 0;
        auto take = [&](size_t bytes) {
            size_t o = off;
            off = align_up(off + std::max<size_t>(bytes, 8), 256);
            return o;
        };
        o_dense = take(sizeof(double) * (size_t)(npad + kCholTile) * npad);
        o_linv = take(chol_linv_bytes(npad));
        o_slot = take(sizeof(int) * (size_t)npose * npose);
        M3S_HIP_CHECK(hipMallocAsync((void**)&dyn, off, st));
        M3S_HIP_CHECK(hipMemsetAsync(chol_ready_ptr(dyn_at<double>(o_linv), npad), 0, chol_ready_bytes(npad), st));
        return M3S_OK;
    }
    Ctx() { sp.reset(); }  // (no earlier call's plan survives into this one)
    Ctx(const Ctx&) = delete;
    Ctx& operator=(const Ctx&) = delete;
    // every return path of a call releases its per-call buffers (stream-ordered)
    ~Ctx() {
        // (an error path may leave an M refresh in flight on the side stream: it reads the plan
        // buffer, so the call's stream waits for it before the buffer is released)
        if (inv_pending && inv_done) (void)hipStreamWaitEvent(st, inv_done, 0);
        if (sp.dbuf) (void)hipFreeAsync(sp.dbuf, st);
        sp.dbuf = nullptr;
        if (dyn) (void)hipFreeAsync(dyn, st);
        if (eall) (void)hipFreeAsync(eall, st);
    }
};

// ---- gn_plan.hip ----
extern double g_plan_sync_us;  // M3S_PROF_HOST: build_plan's edge-list copies + stream sync
int gn_order(const m3s_gn_args& a);
int validate(const m3s_gn_args& a);
void build_schedule_order(const std::vector<int>& ii_loc, const std::vector<int>& jj_loc, int nkey, int* order,
                          SchedGroups& G);
int build_plan(const m3s_gn_args& a, hipStream_t st, Plan& plan, const std::function<int()>& before_wait = {});
void choose_sparse_plan(const Plan& plan, int npose, SparsePlan& sp);
void choose_pcg(const m3s_gn_args& a, const Ctx& c, const Plan& plan, int npose, SparsePlan& sp);
int upload_sparse_plan(SparsePlan& sp, int npose, hipStream_t st);
int plan_info(const int64_t* ii, const int64_t* jj, int64_t E, int64_t N, int32_t* info, int32_t* order,
              int32_t* round_ptr, int32_t round_cap);

// ---- gn_enqueue.hip ----
int prepare_iterations(const m3s_gn_args& a, Ctx& c);
int enqueue_system(const m3s_gn_args& a, Ctx& c);
int enqueue_accumulate(const m3s_gn_args& a, Ctx& c);
int enqueue_assembly(const m3s_gn_args& a, Ctx& c);
int enqueue_solve(const m3s_gn_args& a, Ctx& c, bool fallback = false);
int enqueue_inverse(const m3s_gn_args& a, Ctx& c, bool snapshot);
int enqueue_pcg(const m3s_gn_args& a, Ctx& c);

// ---- gn_driver.hip ----
int setup(const m3s_gn_args& a, Ctx& c, bool early_pack = false);
int run(const m3s_gn_args& a);
int take_deferred_timeout(const char* which);

}  // namespace m3s

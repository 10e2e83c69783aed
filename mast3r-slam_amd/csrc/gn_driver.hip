// gn_driver.hip -- one Gauss-Newton call on the host: setup, the iteration loop and the deferred
// timeout report (the C ABI that enters here: gn_api.hip; the types: gn_host.h).
//
// Replaces gauss_newton_{points,rays,calib}_cuda (reference gn_kernels.cu:725-811,
// 1140-1228, 1546-1637) and SparseBlock (:57-159).  Per call:
//   1. ONE host sync: copy ii/jj (and K) to the host, build the keyframe remap
//      (unique + searchsorted, :161-170), the block-sparse layout of the pose graph and
//      the deterministic CSR contribution lists; upload them into the workspace (gn_plan.hip).
//      Iteration 0's accumulate is enqueued before the host plans the elimination.
//   2. Enqueue max_iter iterations on the caller's stream with no host round trip
//      (gn_enqueue.hip): accumulate -> edge reduce -> block system [-> RCCL all-gather /
//      all-reduce] -> block-sparse f64 solve (elimination rounds, a dense core factored by the
//      dataflow Cholesky or in registers, back-substitution; from iteration 3 or 4 on a PCG
//      preconditioned with an earlier iteration's factor, the direct solve behind it as its
//      fallback) -> retraction.  The ||dx|| < delta_thresh early exit is a device flag that turns
//      the remaining iterations into no-ops (same result as the reference's host `break`).
//   3. A bounded device-side wait that gave up restores the call's poses on the device; the error
//      is reported by the next call or m3s_gn_check (take_deferred_timeout).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "gn_host.h"
#include "m3s_comm.h"

namespace m3s {

namespace {
// The per-call solver buffers come from the device's default stream-ordered pool
// (hipMallocAsync); its default release threshold (0) hands freed memory back to the driver at
// every synchronisation -- and the call synchronises once on its edge lists -- so every call
// mapped its buffers again (~10 MB with the PCG's M and factor copy).  M3S_POOL_KEEP_MB (default
// 1024): keep that much cached in the pool.  Once per device; the pool is the HIP runtime's (not
// torch's caching allocator).
void keep_pool() {
    static std::mutex mu;
    static bool done[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev]) return;
    done[dev] = true;
    const long mb = env_int("M3S_POOL_KEEP_MB", 1024);
    if (mb <= 0) return;
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess) return;
    uint64_t thr = (uint64_t)mb << 20;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
}
}  // namespace

// early_pack: launch the packed stream (prepare_iterations) as soon as the edge lists are on
// the device, before the host builds the accumulate schedule
int setup(const m3s_gn_args& a, Ctx& c, bool early_pack) {
    int rc = validate(a);
    if (rc) return rc;
    keep_pool();
    c.st = (hipStream_t)a.stream;
    c.ws = (char*)a.ws;
    c.L = make_layout(a.mode, a.N, a.HW, a.E_total, a.E_local);
    static const bool prof_host = env_int("M3S_PROF_HOST", 0) != 0;
    const auto s0 = std::chrono::steady_clock::now();
    const Layout& L = c.L;
    AccParams& P = c.P;
    P.s0_inv = 1.0f / a.sigma0;
    P.s1_inv = (a.mode == M3S_GN_POINTS) ? 0.0f : 1.0f / a.sigma1;
    P.C_thresh = a.C_thresh;
    P.Q_thresh = a.Q_thresh;
    P.pb_lo = (float)a.pixel_border;
    P.pb_hi_u = (float)(a.width - 1 - a.pixel_border);
    P.pb_hi_v = (float)(a.height - 1 - a.pixel_border);
    P.z_eps = a.z_eps;
    P.width = a.width > 0 ? a.width : 1;
    P.height = a.height;
    {   // Granlund-Montgomery: l = ceil(log2 W), m = ceil(2^(31+l) / W) < 2^32
        int l = 0;
        while ((1LL << l) < P.width) l++;
        const unsigned long long num = 1ULL << (31 + l);
        P.div_m = (unsigned)((num + (unsigned long long)P.width - 1) / (unsigned long long)P.width);
        P.div_sh = 31 + l;
    }
    P.HW = (int)a.HW;
    P.chunk = chunk_points(a.HW, L.nchunks);
    P.nchunks = L.nchunks;
    P.nkf = (int)a.N;
    auto al16 = [](const void* ptr) { return ((uintptr_t)ptr & 15) == 0; };
    const bool two = a.idx_b != nullptr;
    c.es.idx[0] = a.idx;
    c.es.valid[0] = a.valid;
    c.es.Q[0] = a.Q;
    c.es.idx[1] = two ? a.idx_b : a.idx;
    c.es.valid[1] = two ? a.valid_b : a.valid;
    c.es.Q[1] = two ? a.Q_b : a.Q;
    c.es.E_a = two ? (int)a.E_a : (int)a.E_local;
    c.vec = (a.HW % 4 == 0) && al16(a.Xs) && al16(a.Cs) && al16(a.idx) && al16(a.valid) &&
            al16(a.Q) && (!two || (al16(a.idx_b) && al16(a.valid_b) && al16(a.Q_b)));
    // M3S_GN_PACK: 0 never, 1 (default) when the call runs >= 3 iterations, 2 always
    const int pack_mode = env_int("M3S_GN_PACK", 1);
    c.packed = c.vec && a.E_local > 0 && (pack_mode == 2 || (pack_mode == 1 && a.max_iter >= 3)) &&
               a.HW <= kPackedMaxHW;  // (32-bit byte offsets within an image: gn_accum.hip)
    // M3S_GN_COMPACT=1: the packed stream holds only the live points (gn_accum.hip).  Off by
    // default: on the bench graphs 80-90 % of the points are live, the accumulate gains 3 %
    // (cfg3) / 13 % (cfg4), and the compacting pack (Xj copies, finiteness gathers) costs more
    // per call than the 10 iterations save
    c.compact = c.packed && env_int("M3S_GN_COMPACT", 0) != 0;
    // calib: the packed records carry the match as its pixel (v << 16 | u), decoded with a mask, a
    // bit-field extract and one 24-bit multiply-add instead of a 64-bit division by W per point
    if (a.mode == M3S_GN_CALIB && (a.width >= 65536 || a.height >= 32768)) c.packed = c.compact = false;
    P.pack_uv = c.packed && a.mode == M3S_GN_CALIB;
    // calib: the packed accumulate reads Xj as its 4-B depth when gn_depth_kernel finds every point
    // on its pixel's ray bit for bit (solve_GN_calib's constrain_points_to_ray; bitwise the same
    // result): 16 instead of 24 B per point-edge.  M3S_GN_RAYCHECK=0 keeps the positional path only.
    P.raycheck = c.packed && !c.compact && a.mode == M3S_GN_CALIB && env_int("M3S_GN_RAYCHECK", 1) != 0;

    c.ref_order = gn_order(a) == M3S_GN_ORDER_REFERENCE;
    if (c.ref_order) {
        c.packed = false;  // the reference-order kernel reads the reference's tensors
        RefParams& R = c.R;
        R.s0_inv = (float)(1.0 / (double)a.sigma0);  // `const float sigma_*_inv = 1.0/sigma_*`
        R.s1_inv = (a.mode == M3S_GN_POINTS) ? 0.0f : (float)(1.0 / (double)a.sigma1);
        R.C_thresh = a.C_thresh;
        R.Q_thresh = a.Q_thresh;
        R.z_eps = a.z_eps;
        R.width = a.width > 0 ? a.width : 1;
        R.height = a.height;
        R.pixel_border = a.pixel_border;
        R.HW = a.HW;
        R.variant = env_int("M3S_GN_REF_VARIANT", 0);  // diagnostics
        R.contract = a.contract;
    }
    // the per-call passes that need no edge lists (the keyframes' confidence pass, calib's depth
    // arrays) and the call's device flags are enqueued right after the edge-list copies: they run
    // while the host waits for the copies and plans (the lists upload below no longer carries
    // the flags / cok)
    int* dflags = c.at<int>(L.flags);
    int* dcok = c.at<int>(L.cok);
    auto pre_pass = [&]() -> int {
        M3S_HIP_CHECK(launch_gn_init(c.st, dflags, P.raycheck ? 0 : 1, dcok, a.N));
        if (c.packed)
            M3S_HIP_CHECK(launch_pack_pre(c.st, a.Xs, a.N, a.Cs, P, !c.compact ? dcok : nullptr,
                                          a.mode == M3S_GN_CALIB ? c.at<float>(L.zs) : nullptr, dflags,
                                          a.mode == M3S_GN_CALIB ? a.K : nullptr));
        return M3S_OK;
    };
    // M3S_PREPASS=0 (A/B): the passes after the host's stream wait instead (cfg3 +0.6 % with
    // them before it, two interleaved pairs on one box: profiles/r05_u_prepass/)
    static const bool prepass_early = env_int("M3S_PREPASS", 1) != 0;
    rc = build_plan(a, c.st, c.plan, prepass_early ? pre_pass : std::function<int()>());
    if (!rc && !prepass_early) rc = pre_pass();
    if (rc) return rc;
    if (c.plan.gather)
        M3S_HIP_CHECK(hipMallocAsync((void**)&c.eall,
                                     sizeof(double) * kEdgeBlk * (size_t)c.plan.granks * c.plan.gchunk, c.st));
    const auto s1 = std::chrono::steady_clock::now();
    const Plan& p = c.plan;
    P.fx = p.K[0];
    P.fy = p.K[1];
    P.cx = p.K[2];
    P.cy = p.K[3];
    if (c.ref_order) {
        c.R.fx = p.K[0];
        c.R.fy = p.K[1];
        c.R.cx = p.K[2];
        c.R.cy = p.K[3];
    }
    // the workspace's plan integers (ii_loc .. sched, one contiguous span of the layout) as an
    // image in pinned memory: the edge lists / CSR lists first (what the pack reads), then the
    // accumulate's task records (built while the GPU packs)
    const size_t ntask = (size_t)a.E_local * L.nchunks;
    const size_t lo = L.ii_loc, hi = L.sched;
    const size_t nslot = c.need_slotmap ? p.slotmap.size() : 0;
    if (c.need_slotmap) {
        rc = c.alloc_dense(L.npad, (int)std::max<int64_t>(a.N - 1, 0));
        if (rc) return rc;
    }
    char* h = stagings().ws.get(hi - lo + sizeof(int) * nslot);
    M3S_REQUIRE(h != nullptr, "gauss_newton: pinned host allocation failed");
    auto put = [&](size_t off, const std::vector<int>& v) {
        if (!v.empty()) std::memcpy(h + (off - lo), v.data(), sizeof(int) * v.size());
    };
    put(L.ii_loc, p.ii_loc);
    put(L.jj_loc, p.jj_loc);
    put(L.blk_ptr, p.blk_ptr);
    put(L.blk_ent, p.blk_ent);
    put(L.blk_ref, p.blk_ref);
    put(L.grad_ptr, p.grad_ptr);
    put(L.grad_ent, p.grad_ent);
    std::memset(h + (L.ecnt - lo), 0, sizeof(int) * (size_t)a.E_local);  // (the kernel re-zeroes them)
    SchedGroups G;
    build_schedule_order(p.ii_loc, p.jj_loc, (int)std::max<int64_t>(a.N, 1), reinterpret_cast<int*>(h + (L.sorder - lo)), G);
    M3S_HIP_CHECK(stagings().ws.upload(c.ws + lo, h, L.sched - lo, c.st));
    // the accumulate's task records carry the edge's keyframes: one load, not three levels
    M3S_HIP_CHECK(launch_sched_expand(c.st, c.at<int>(L.sorder), c.at<int>(L.ii_loc), c.at<int>(L.jj_loc), L.nchunks,
                                      G, (int64_t)ntask, c.at<int>(L.sched)));
    // M3S_GN_PACK_FIRST (default 1): a call's first accumulate builds the packed records
    // from the reference's inputs itself (gn_accum_packed_kernel<..., FIRST>): 13 B read + 8 B
    // written per point-edge inside the first iteration instead of a separate 21-B pack pass
    // followed by the first iteration's 8-B record reads (run() only: its early pack)
    c.first_pack = early_pack && c.packed && !c.compact && !c.ref_order && a.max_iter > 0 &&
                   env_int("M3S_GN_PACK_FIRST", 1) != 0;
    if (early_pack) {
        rc = prepare_iterations(a, c);
        if (rc) return rc;
        c.pack_issued = true;
    }
    const auto s2 = std::chrono::steady_clock::now();
    if (nslot) {  // the dense (npose x npose) slot table
        std::memcpy(h + (hi - lo), p.slotmap.data(), sizeof(int) * nslot);
        M3S_HIP_CHECK(hipMemcpyAsync(c.dyn + c.o_slot, h + (hi - lo), sizeof(int) * nslot,
                                     hipMemcpyHostToDevice, c.st));
    }
    M3S_HIP_CHECK(stagings().ws.mark(c.st));
    if (prof_host) {
        auto us = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
            return std::chrono::duration<double, std::micro>(y - x).count();
        };
        fprintf(stderr, "gn host: build_plan %.0f us (of which copies + sync %.0f us), params+lists+schedule+pack "
                "%.0f us, rest %.0f us\n", us(s0, s1), g_plan_sync_us, us(s1, s2), us(s2, std::chrono::steady_clock::now()));
    }
    return M3S_OK;
}

// The deferred timeout report of this thread's last gauss_newton call (waits for its flag copy):
// M3S_ERR_TIMEOUT once, then cleared.
int take_deferred_timeout(const char* which) {
    Stagings& sg = stagings();
    if (!sg.tmo_armed) return M3S_OK;
    const int kind = sg.tmo_armed;
    sg.tmo_armed = 0;
    const char* h = sg.tmo.get(64);  // waits for the copy (its event)
    const bool hit = kind == 2 ? *reinterpret_cast<const double*>(h) > 0.0 : *reinterpret_cast<const int*>(h) != 0;
    if (hit) {
        set_error("gauss_newton: %sa device-side wait of the factorisation timed out (the solve was "
                  "discarded; not a singular system)", which);
        return M3S_ERR_TIMEOUT;
    }
    return M3S_OK;
}

int run(const m3s_gn_args& a) {
    // M3S_PROF_HOST: host-side phase times of the call (stderr)
    static const bool prof_host = env_int("M3S_PROF_HOST", 0) != 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) {
        return std::chrono::duration<double, std::micro>(y - x).count();
    };
    const auto t0 = now();
    Ctx c;
    c.need_slotmap = env_int("M3S_SOLVER_DENSE", 0) != 0;
    // the packed stream is launched inside setup as soon as its inputs are on the device: the
    // GPU builds it while the host plans the accumulate schedule and the elimination
    int rc = setup(a, c, a.N > 1);
    if (rc) return rc;
    // an earlier call's timeout (its copy has landed: setup synchronised the stream)
    rc = take_deferred_timeout("an earlier call: ");
    if (rc) return rc;
    const auto t1 = now();
    const int npose = (int)(a.N - 1);
    if (npose <= 0) return M3S_OK;  // nothing to optimise (all poses pinned)
    const Layout& L = c.L;
    int* flags = c.at<int>(L.flags);
    std::chrono::steady_clock::time_point t2 = t1, t3 = t1;
    // M3S_EARLY_ACC (default 1): iteration 0's accumulate is enqueued before the host builds the
    // elimination plan (the GPU works while the host plans; the per-call pack alone no longer
    // covers the planning once the edges are sharded over several GPUs)
    if (!c.ref_order && a.max_iter > 0 && env_int("M3S_EARLY_ACC", 1) != 0) {
        g_prof.mark(c.st);
        rc = enqueue_accumulate(a, c);
        if (rc) return rc;
        c.acc_enqueued = true;
        // edge-sharded: the records' all-gather needs no plan either -- the ranks exchange (and
        // wait for the slowest rank's accumulate) while their hosts plan.  M3S_EARLY_GATHER: -1
        // (default) with RCCL only (a host-callback exchange would block this thread until every
        // rank's accumulate is done), 1 always (tests: the host exchange), 0 never
        static const int early_gather = env_int("M3S_EARLY_GATHER", -1);
        if (c.plan.gather && (early_gather > 0 || (early_gather < 0 && comm_is_async(a.comm)))) {
            rc = comm_allgather_f64(a.comm, c.eall, (size_t)c.plan.gchunk * kEdgeBlk, c.st);
            if (rc) return rc;
            c.gathered = true;
        }
    }
    const auto t1b = now();
    if (env_int("M3S_SOLVER_DENSE", 0) == 0 || c.ref_order) {
        choose_sparse_plan(c.plan, npose, c.sp);
        choose_pcg(a, c, c.plan, npose, c.sp);
        t2 = now();
        M3S_REQUIRE(c.sp.npad_tail <= kMaxNpad,
                    "gauss_newton: the dense core of the elimination (%d unknowns) exceeds the "
                    "dense solve limit (%d)", c.sp.npad_tail, kMaxNpad);
        rc = upload_sparse_plan(c.sp, npose, c.st);
        if (rc) return rc;
        t3 = now();
    }
    if (prof_host)
        fprintf(stderr, "gn host: setup %.0f us, early enqueue %.0f us, plan %.0f us, upload %.0f us\n", us(t0, t1),
                us(t1, t1b), us(t1b, t2), us(t2, t3));
    for (int itr = 0; itr < a.max_iter; itr++) {
        if (!c.acc_enqueued) g_prof.mark(c.st);  // (iteration 0's mark preceded its early accumulate)
        rc = enqueue_system(a, c);
        if (rc) return rc;
        g_prof.mark(c.st);
        // the poses the call started from, so that a timed-out call can restore them (below)
        if (itr == 0) M3S_HIP_CHECK(launch_twc_save(c.st, a.Twc, c.at<float>(L.twc_save), (int)(8 * a.N)));
        const int from = c.sp.pcg_from, lag = c.sp.pcg_lag;
        if (c.sp.pcg && itr >= from) {  // the direct solve below is its fallback
            if (c.inv_pending) {  // M's refresh (side stream) must be complete
                M3S_HIP_CHECK(hipStreamWaitEvent(c.st, c.inv_done, 0));
                c.inv_pending = false;
            }
            rc = enqueue_pcg(a, c);
            if (rc) return rc;
        }
        rc = enqueue_solve(a, c, c.sp.pcg && itr >= from);
        if (rc) return rc;
        g_prof.mark(c.st);
        if (!c.sp.fused && !c.sp.hybrid)  // gn_solve retracts inside its launch
            M3S_HIP_CHECK(launch_retract(c.st, a.Twc, c.at<double>(L.x), a.dx, (int)a.N,
                                         a.delta_thresh, flags, a.contract));
        // M from this iteration's factor: iteration M3S_PCG_FROM - M3S_PCG_LAG's (a copy of it
        // when the lag is 2 or more), then after every PCG that fell back to the direct solve
        // (sp_inverse_kernel returns at once when this iteration's PCG converged: M stays)
        if (c.sp.pcg && (itr == from - lag || itr >= from) && itr + 1 < a.max_iter) {
            rc = enqueue_inverse(a, c, itr < from - 1);
            if (rc) return rc;
        }
        g_prof.mark(c.st);
    }
    // (the per-call solver buffers are released by ~Ctx on this and every error path)
    if (c.may_timeout && a.max_iter > 0) {
        // A bounded device-side wait that gave up discarded that iteration's solve (dx = 0): an
        // error, not a singular system (the reference's host Eigen solve cannot time out).  The
        // call then restores the poses it started from, on the device (twc_guard_kernel), so a
        // timed-out call never commits poses -- whatever its caller does next -- and
        // every rank of a sharded call ends with the same Twc.  The flag leaves the device without
        // a host wait (the same kernel writes it to pinned memory): the error is reported by the
        // next GN call on this thread (once setup() has synchronised the stream) or by
        // m3s_gn_check, like an asynchronous kernel fault.  Waiting here instead left the GPU idle
        // between calls for the host's per-call work (cfg3: 694 vs 318 us call-to-call gap,
        // rocprofv3 trace).  M3S_GN_TIMEOUT_SYNC=1: report it from this call (one stream
        // synchronisation).
        Stagings& sg = stagings();
        char* h = sg.tmo.get(64);
        M3S_REQUIRE(h != nullptr, "gauss_newton: pinned host allocation failed");
        float* save = c.at<float>(L.twc_save);
        const int n8 = (int)(8 * a.N);
        if (a.comm) {
            // edge-sharded: every rank ran the same replicated solve, but the flag is rank-local --
            // OR it over the ranks (a sum of 0 / 1) so that all fail together instead of one rank
            // returning the error while the others go on to their next collective,
            // and all restore their poses
            double* dv = c.at<double>(L.x);  // the solution buffer is free once the call retracted
            M3S_HIP_CHECK(launch_flag_export(c.st, flags + kFlagTimeout, dv, 1));
            rc = comm_allreduce_sum_f64(a.comm, dv, 1, c.st);
            if (rc) return rc;
            M3S_HIP_CHECK(launch_twc_restore_on_flag(c.st, a.Twc, save, n8, dv, 1, sg.tmo.dev));
            if (!sg.tmo.dev) M3S_HIP_CHECK(hipMemcpyAsync(h, dv, sizeof(double), hipMemcpyDeviceToHost, c.st));
            sg.tmo_armed = 2;
        } else {
            M3S_HIP_CHECK(launch_twc_restore_on_flag(c.st, a.Twc, save, n8, flags + kFlagTimeout, 0, sg.tmo.dev));
            if (!sg.tmo.dev)
                M3S_HIP_CHECK(hipMemcpyAsync(h, flags + kFlagTimeout, sizeof(int), hipMemcpyDeviceToHost, c.st));
            sg.tmo_armed = 1;
        }
        M3S_HIP_CHECK(sg.tmo.mark(c.st));
        static const bool sync_report = env_int("M3S_GN_TIMEOUT_SYNC", 0) != 0;
        if (sync_report) {
            rc = take_deferred_timeout("");
            if (rc) return rc;
        }
    }
    if (const int dbg = env_int("M3S_GN_DEBUG_FLAGS", 0)) {  // diagnostics: the device flags after the call
        int hf[kNumFlags];
        M3S_HIP_CHECK(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, c.st));
        M3S_HIP_CHECK(hipStreamSynchronize(c.st));
        // m3s_gn_debug_flags: which accumulate path the call took (bench.py prices its bytes)
        g_dbg_flags[0] = hf[kFlagDone];
        g_dbg_flags[1] = (hf[kFlagFail] | hf[kFlagFailed]) != 0;  // (the retraction consumed kFlagFail)
        g_dbg_flags[2] = c.packed ? 1 : 0;
        g_dbg_flags[3] = (c.packed && c.P.raycheck && hf[kFlagNotRay] == 0) ? 1 : 0;
        g_dbg_pcg[0] = hf[kFlagPcgRuns];
        g_dbg_pcg[1] = hf[kFlagPcgSteps];
        g_dbg_pcg[2] = hf[kFlagPcgFall];
        g_dbg_pcg[3] = c.sp.pcg ? 1 : 0;
        g_dbg_pcg[4] = c.sp.pcg ? c.sp.pcg_from : 0;
        g_dbg_pcg_plan[0] = c.sp.pcg ? c.sp.pcg_R : 0;
        g_dbg_pcg_plan[1] = c.sp.pcg ? c.sp.pcg_nwg : 0;
        g_dbg_pcg_plan[2] = c.sp.pcg && c.sp.pcg_onex ? 1 : 0;
        g_dbg_pcg_plan[3] = c.sp.pcg ? c.sp.pcg_lag : 0;
        g_dbg_pcg_plan[4] = c.sp.pcg ? c.sp.pcg_nitem : 0;
        if (dbg != 2)
            fprintf(stderr, "gn flags: done %d fail %d not_ray %d timeout %d packed %d pcg runs %d steps %d fallbacks %d\n",
                    hf[kFlagDone], g_dbg_flags[1], hf[kFlagNotRay], hf[kFlagTimeout], (int)c.packed,
                    hf[kFlagPcgRuns], hf[kFlagPcgSteps], hf[kFlagPcgFall]);
    }
    return M3S_OK;
}

}  // namespace m3s

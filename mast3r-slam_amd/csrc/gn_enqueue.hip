// gn_enqueue.hip -- what the host enqueues per Gauss-Newton iteration (gn_host.h), with no host
// round trip: accumulate (+ edge reduce) -> assembly of the block system [-> all-gather of the edge
// records / all-reduce of the system] -> the step, by the block-sparse direct solve (elimination
// rounds, dense core, back-substitution) or, from a later iteration on, by the lagged-factor PCG
// with the direct solve behind it as its fallback -> retraction.  Replaces the iteration bodies
// of gauss_newton_{points,rays,calib}_cuda (reference gn_kernels.cu:725-811, 1140-1228,
// 1546-1637) and SparseBlock's update / solve (:57-159).  Also here: the once-per-call packed
// stream, the PCG's side stream and the solve / PCG debug readbacks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gn_host.h"
#include "m3s_comm.h"

namespace m3s {

namespace {
// The PCG's side stream (gn_pcg.hip): M's refresh (sp_inverse_kernel) runs there, beside the
// next iteration's accumulate on the call's stream; per host thread and device (the events must
// not be shared by concurrent calls), released by m3s_shutdown.
struct PcgSide {
    static constexpr int kMaxDev = 64;
    hipStream_t ss[kMaxDev] = {};
    hipEvent_t e1[kMaxDev] = {}, e2[kMaxDev] = {};
    static void release(void* p) {
        PcgSide* s = static_cast<PcgSide*>(p);
        for (int d = 0; d < kMaxDev; d++) {
            if (s->e1[d]) (void)hipEventDestroy(s->e1[d]);
            if (s->e2[d]) (void)hipEventDestroy(s->e2[d]);
            if (s->ss[d]) (void)hipStreamDestroy(s->ss[d]);
            s->e1[d] = s->e2[d] = nullptr;
            s->ss[d] = nullptr;
        }
    }
};
thread_local PcgSide* t_pcg_side = nullptr;
// this thread's side stream and its two events for the current device (created on first use)
int pcg_side(hipStream_t& ss, hipEvent_t& e1, hipEvent_t& e2) {
    if (!t_pcg_side) {
        t_pcg_side = new PcgSide;
        register_host_resource(t_pcg_side, &PcgSide::release);
    }
    int dev = 0;
    M3S_HIP_CHECK(hipGetDevice(&dev));
    M3S_REQUIRE(dev >= 0 && dev < PcgSide::kMaxDev, "gauss_newton: device %d out of range", dev);
    PcgSide& p = *t_pcg_side;
    if (!p.ss[dev]) {
        M3S_HIP_CHECK(hipStreamCreateWithFlags(&p.ss[dev], hipStreamNonBlocking));
        // (device-scope only: a default event's system-scope release / acquire writes back and
        // invalidates the caches on the call's stream at every record -- idle GPU, Prof above)
        M3S_HIP_CHECK(hipEventCreateWithFlags(&p.e1[dev], hipEventDisableTiming | hipEventDisableSystemFence));
        M3S_HIP_CHECK(hipEventCreateWithFlags(&p.e2[dev], hipEventDisableTiming | hipEventDisableSystemFence));
    }
    ss = p.ss[dev];
    e1 = p.e1[dev];
    e2 = p.e2[dev];
    return M3S_OK;
}
}  // namespace

// Once per call, before the iterations: the packed stream (and calib depth array).
int prepare_iterations(const m3s_gn_args& a, Ctx& c) {
    if (!c.packed) return M3S_OK;
    const Layout& L = c.L;
    M3S_HIP_CHECK(launch_pack(a.mode, c.st, (int)a.E_local, a.Xs, a.N, a.Cs, c.at<int>(L.ii_loc),
                              c.at<int>(L.jj_loc), c.es, c.P, c.at<int>(L.cok), c.at<int4>(L.pack),
                              c.compact ? c.at<float>(L.packx) : nullptr, c.at<int>(L.pcnt),
                              c.at<int>(L.flags), c.first_pack));
    return M3S_OK;
}

// accumulate + edge reduce + compact (+ all-reduce): the system of one iteration
int enqueue_system(const m3s_gn_args& a, Ctx& c) {
    const Layout& L = c.L;
    int* flags = c.at<int>(L.flags);
    const int npose_r = (int)(a.N - 1);
    if (c.ref_order) {
        // the reference kernels' order (gn_refacc.hip), then the block system from the lower
        // triangle of the reference's matrix (the sparse solvers' format)
        M3S_REQUIRE(c.sp.enabled, "gauss_newton: the reference order needs the block-sparse solver");
        g_prof.mark(c.st, true);
        M3S_HIP_CHECK(launch_accum_ref(a.mode, (int)a.E_local, c.st, a.Twc, a.Xs, a.Cs,
                                       c.at<int>(L.ii_loc), c.at<int>(L.jj_loc), c.es,
                                       c.R, c.at<float>(L.edgeblk), flags));
        g_prof.mark(c.st, true);
        SparsePlan& sp = c.sp;
        double* sys = sp.dptr<double>(sp.o_sys);
        M3S_HIP_CHECK(launch_assemble_ref(c.st, c.at<float>(L.edgeblk), c.at<int>(L.blk_ptr),
                                          c.at<int>(L.blk_ref), c.at<int>(L.grad_ptr),
                                          c.at<int>(L.grad_ent), c.plan.nblk, sp.nblocks, npose_r,
                                          sp.bpad, sys, flags));
        if (a.comm) {
            const size_t count = (size_t)sp.bpad + (size_t)c.plan.nblk * 49;
            int rc = comm_allreduce_sum_f64(a.comm, sys, count, c.st);
            if (rc) return rc;
        }
        return M3S_OK;
    }
    if (!c.acc_enqueued) {
        int rc = enqueue_accumulate(a, c);
        if (rc) return rc;
    }
    c.acc_enqueued = false;
    return enqueue_assembly(a, c);
}

// the accumulate (+ edge reduce) of one iteration: needs no elimination plan, so iteration 0's
// is enqueued before the host builds it
int enqueue_accumulate(const m3s_gn_args& a, Ctx& c) {
    const Layout& L = c.L;
    int* flags = c.at<int>(L.flags);
    if (a.E_local > 0) {
        g_prof.mark(c.st, true);
        const dim3 grid((unsigned)(L.nchunks * a.E_local));
        // M3S_GN_FUSE_REDUCE=1 (default): the packed accumulate's last workgroup per edge does
        // the edge reduce (no separate launch); 0: gn_edge_reduce_kernel
        const bool fuse_reduce = env_int("M3S_GN_FUSE_REDUCE", 1) != 0;
        const bool fused = c.packed && fuse_reduce;
        const bool was_first = c.packed && c.first_pack;
        if (c.packed) {
            M3S_HIP_CHECK(launch_accum_packed(a.mode, grid, c.st, a.Twc, a.Xs, c.at<float>(L.zs),
                                              c.at<int>(L.ii_loc), c.at<int>(L.jj_loc),
                                              c.at<int4>(L.pack), c.P, c.at<int4>(L.sched),
                                              c.at<float>(L.partials), flags,
                                              c.compact ? c.at<float>(L.packx) : nullptr,
                                              c.at<int>(L.pcnt), fused ? c.at<int>(L.ecnt) : nullptr,
                                              c.eblk(), c.first_pack ? &c.es : nullptr,
                                              a.Cs, c.at<int>(L.cok)));
            c.first_pack = false;  // the records exist from here on
        } else
            M3S_HIP_CHECK(launch_accum(a.mode, c.vec, grid, c.st, a.Twc, a.Xs, a.Cs,
                                       c.at<int>(L.ii_loc), c.at<int>(L.jj_loc), c.es, c.P,
                                       c.at<int4>(L.sched), c.at<float>(L.partials),
                                       flags));
        g_prof.mark(c.st, true, was_first);
        if (!fused)
            M3S_HIP_CHECK(launch_edge_reduce((int)a.E_local, c.st, c.at<float>(L.partials), L.nchunks,
                                             a.Twc, c.at<int>(L.ii_loc), c.eblk(), flags));
    }
    return M3S_OK;
}

// edge blocks -> the solver's system (+ the all-reduce)
int enqueue_assembly(const m3s_gn_args& a, Ctx& c) {
    const Layout& L = c.L;
    int* flags = c.at<int>(L.flags);
    const int npose = (int)(a.N - 1);
    if (c.plan.gather && !c.gathered) {
        // every rank's edge records, then the assembly of ALL edges in edge order (no all-reduce)
        int rc = comm_allgather_f64(a.comm, c.eall, (size_t)c.plan.gchunk * kEdgeBlk, c.st);
        if (rc) return rc;
    }
    c.gathered = false;
    const bool reduce = a.comm && !c.plan.gather;
    if (c.sp.enabled) {
        // block format for the sparse solves, in the solver's buffer
        SparsePlan& sp = c.sp;
        double* sys = sp.dptr<double>(sp.o_sys);
        M3S_HIP_CHECK(launch_assemble(c.st, c.eblk_all(), c.at<int>(L.blk_ptr),
                                      c.at<int>(L.blk_ent), c.at<int>(L.grad_ptr),
                                      c.at<int>(L.grad_ent), c.plan.nblk, sp.nblocks, npose, sp.bpad,
                                      sys, flags));
        if (reduce) {
            const size_t count = (size_t)sp.bpad + (size_t)c.plan.nblk * 49;
            int rc = comm_allreduce_sum_f64(a.comm, sys, count, c.st);
            if (rc) return rc;
        }
        return M3S_OK;
    }
    M3S_HIP_CHECK(launch_compact(c.st, c.eblk_all(), c.at<int>(L.blk_ptr),
                                 c.at<int>(L.blk_ent), c.at<int>(L.grad_ptr),
                                 c.at<int>(L.grad_ent), c.plan.nblk, npose,
                                 c.at<double>(L.compact), flags));
    if (reduce) {
        const size_t count = (size_t)c.plan.nblk * 28 + (size_t)npose * 7;
        int rc = comm_allreduce_sum_f64(a.comm, c.at<double>(L.compact), count, c.st);
        if (rc) return rc;
    }
    return M3S_OK;
}

namespace {
// M3S_SOLVE_DEBUG: gn_solve_kernel writes its phase clocks to a device buffer; the driver
// waits for the launch and prints them (debug runs only: the wait serialises the call)
constexpr int kSolveDbgWords = kSolveDbgCycles + 1;
unsigned long long* solve_dbg_buffer() {
    static unsigned long long* p = nullptr;
    if (p == nullptr && hipMalloc(&p, sizeof(unsigned long long) * kSolveDbgWords) != hipSuccess) p = nullptr;
    if (p != nullptr) (void)hipMemset(p, 0, sizeof(unsigned long long) * kSolveDbgWords);
    return p;
}
hipError_t launch_gn_solve_dbg(hipStream_t st, const SolveArgs& S) {
    hipError_t e = launch_gn_solve(st, S);
    if (e != hipSuccess || !S.debug || S.dbg == nullptr) return e;
    unsigned long long h[kSolveDbgWords];
    e = hipMemcpyAsync(h, S.dbg, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) print_solve_debug(h);
    return e;
}
}  // namespace

// fallback: the direct solve enqueued behind a PCG launch (it runs only when the PCG did not
// converge; otherwise each of its launches returns at once, ~4-5 us apiece)
int enqueue_solve(const m3s_gn_args& a, Ctx& c, bool fallback) {
    const Layout& L = c.L;
    const int npose = (int)(a.N - 1);
    int* flags = c.at<int>(L.flags);
    if (!c.sp.enabled) {
        c.may_timeout = true;  // dense factorisation: chol_df's ready waits
        M3S_HIP_CHECK(launch_solve(c.st, c.at<double>(L.compact), c.dyn_at<int>(c.o_slot), c.plan.nblk,
                                   npose, 7 * npose, L.npad, c.dyn_at<double>(c.o_dense),
                                   c.dyn_at<double>(c.o_linv), c.at<double>(L.x), flags, ++c.chol_epoch));
        return M3S_OK;
    }
    SparsePlan& sp = c.sp;
    SolveArgs S{};
    S.npose = npose;
    S.b = sp.dptr<double>(sp.o_sys);
    S.A = S.b + sp.bpad;
    S.y = sp.dptr<double>(sp.o_y);
    S.Lstore = sp.dptr<double>(sp.o_L);
    S.W = sp.dptr<double>(sp.o_W);
    S.Lg = sp.dptr<double>(sp.o_Lg);
    S.x = c.at<double>(L.x);
    S.meta = sp.iptr(0);
    S.nmeta = (int)sp.nints;
    S.meta_lds = solve_lds_bytes(S.nmeta) <= (size_t)kSolveMaxLds && env_int("M3S_SOLVE_META_LDS", 1);
    S.o_rounds = (int)sp.i_rounds;
    S.o_nodes = (int)sp.i_nodes;
    S.o_fptr = (int)sp.i_fptr;
    S.o_fronts = (int)sp.i_fronts;
    S.o_tg = (int)sp.i_tg;
    S.o_tc = (int)sp.i_tc;
    S.o_rtg = (int)sp.i_rtg;
    S.o_rc = (int)sp.i_rc;
    S.o_tail = (int)sp.i_tail;
    S.o_tmap = (int)sp.i_tmap;
    S.nrounds = (int)sp.rounds.size();
    S.zero_blk = sp.zero_blk;
    S.ntail = sp.ntail;
    S.Twc = a.Twc;
    S.dx = a.dx;
    S.N = (int)a.N;
    S.delta_thresh = a.delta_thresh;
    S.flags = flags;
    S.debug = env_int("M3S_SOLVE_DEBUG", 0);
    S.dbg = S.debug ? solve_dbg_buffer() : nullptr;
    S.contract = a.contract;
    if (S.debug) {
        static int printed = 0;
        if (printed++ == 0) {
            fprintf(stderr, "solve plan: npose %d nblocks %d (real %d) nW %d ntail %d nints %zu meta_lds %d fused %d\n",
                    npose, sp.nblocks, c.plan.nblk, sp.nW, sp.ntail, sp.nints, S.meta_lds, (int)sp.fused_tail);
            for (const SpRound& R : sp.rounds) {
                int ncontrib = 0, maxc = 0;
                for (int t = 0; t < R.nbt; t++) {
                    const int* T = sp.fused ? &sp.tg[3 * (R.tbeg + t)]
                                            : &sp.inl[(size_t)kSpRec * (R.tbeg + R.rbeg + t)];
                    const int k = T[2] - T[1];
                    ncontrib += k;
                    maxc = std::max(maxc, k);
                }
                int nf = 0;
                for (int q = R.node_begin; q < R.node_begin + R.nnodes; q++) nf += sp.fptr[q + 1] - sp.fptr[q];
                fprintf(stderr, "  round: nodes %d fronts %d block targets %d (contrib %d, max %d) rhs targets %d\n",
                        R.nnodes, nf, R.nbt, ncontrib, maxc, R.nrt);
            }
        }
    }
    if (sp.fused) {
        // one launch: rounds, in-register dense tail, back-substitution, retraction
        if (env_int("M3S_SOLVE_SPLIT", 1) && S.nrounds > 0) {
            // the rounds by a wider workgroup (memory latency overlapped across 8 waves), then
            // the in-register tail + back-substitution + retraction
            S.do_fwd = 1;
            S.do_tail = S.do_back = 0;
            M3S_HIP_CHECK(launch_gn_solve_dbg(c.st, S));
            S.do_fwd = 0;
            S.do_tail = S.do_back = 1;
            M3S_HIP_CHECK(launch_gn_solve_dbg(c.st, S));
            return M3S_OK;
        }
        S.do_fwd = S.do_tail = S.do_back = 1;
        M3S_HIP_CHECK(launch_gn_solve_dbg(c.st, S));
        return M3S_OK;
    }
    // multi-launch: one launch per round phase, the tail by the tiled dense Cholesky
    double* A = S.A;
    double* b = S.b;
    double* y = S.y;
    double* Ls = S.Lstore;
    double* W = S.W;
    double* x = S.x;
    // M3S_SOLVE_DF: 1 (default) = a PCG iteration's fallback runs its rounds (and the core's fill)
    // as ONE plain launch of ticketed targets (sp_rounds_df_kernel: no co-residency) -- slower
    // when it runs, but a converged PCG skips one launch instead of one per round (cfg3: 5 round
    // launches + the fill); 2 = every direct solve does; 0 = one launch per round everywhere
    static const int df_mode = env_int("M3S_SOLVE_DF", 1);
    // the rounds and the core fill ran as the single ticketed launch
    const bool df = df_mode == 2 || (df_mode == 1 && fallback);
    if (df) {
        c.may_timeout = true;  // the tickets' bounded waits
        SpRoundsArgs ca{};
        ca.inl = sp.iptr(sp.i_inl);
        ca.tc3 = sp.iptr(sp.i_tc3);
        ca.rc4 = sp.iptr(sp.i_rc4);
        ca.rounds = sp.iptr(sp.i_rounds);
        ca.tmap = sp.iptr(sp.i_tmap);
        ca.tail = sp.iptr(sp.i_tail);
        ca.A = A;
        ca.b = b;
        ca.Lstore = Ls;
        ca.W = W;
        ca.y = y;
        // (the ticketed launch fills the multi plan's core too: one launch less behind a PCG)
        ca.Hd = sp.ntail > 0 ? sp.dptr<double>(sp.o_dense) : nullptr;
        ca.flags = flags;
        ca.nrounds = (int)sp.rounds.size();
        ca.ntail = sp.ntail;
        ca.npad = sp.npad_tail;
        M3S_HIP_CHECK(launch_sp_rounds_df(c.st, ca, sp.dptr<int>(sp.o_dfcnt)));
    } else {
        for (const SpRound& R : sp.rounds)
            M3S_HIP_CHECK(launch_sp_round(c.st, sp.iptr(sp.i_inl), R.tbeg + R.rbeg, R.nbt, R.nrt,
                                          sp.iptr(sp.i_tc3), sp.iptr(sp.i_rc4), A, b, Ls, W, y, flags));
    }
    // M3S_HYB_CORE=1 (default): the hybrid's dense core (<= kHybDfTailMax = 64 poses, 36 by
    // default) is factored and solved by the dataflow launch (chol_df.hip: batch-cyclic tile
    // factor, ~100 ns per column on the pivot chain, back-substitution in the same launch)
    // instead of gn_solve's in-register pose steps (~330-430 ns per column); gn_solve then only
    // back-substitutes through the rounds and retracts.  0: the in-register core, <= 27 poses.
    // The planner read the switch (hyb_core_df) and sized the core for it: the plan carries the
    // choice.
    const bool core_df = sp.core_df;
    if (sp.hybrid && core_df && sp.ntail > 0) {
        c.may_timeout = true;  // chol_df's bounded waits
        if (!df)  // (the ticketed launch filled the core)
            M3S_HIP_CHECK(launch_sp_tail_fill(c.st, A, b, sp.iptr(sp.i_tmap), sp.iptr(sp.i_tail), sp.ntail,
                                              sp.npad_tail, sp.dptr<double>(sp.o_dense), flags));
        M3S_HIP_CHECK(launch_dense_factor_solve(c.st, sp.npad_tail, sp.dptr<double>(sp.o_dense),
                                                sp.dptr<double>(sp.o_linv), sp.dptr<double>(sp.o_xd), flags,
                                                ++c.chol_epoch));
        S.xd = sp.dptr<double>(sp.o_xd);  // gn_solve reads the core's x in its dense order
        S.Hd = nullptr;
        S.nmeta = (int)sp.nints_back;
        S.meta_lds = 1;
        S.do_fwd = 0;
        S.do_tail = 0;
        S.do_back = 1;
        S.x_tail_global = 1;
        M3S_HIP_CHECK(launch_gn_solve_dbg(c.st, S));
        return M3S_OK;
    }
    if (sp.hybrid) {
        M3S_REQUIRE(sp.fused_tail, "gauss_newton: a %d-pose hybrid core exceeds the in-register factorisation",
                    sp.ntail);
        // the <= 27-pose core in registers, the back-substitution through the rounds and the
        // retraction: one single-workgroup launch (gn_solve.hip) reading the plan prefix; the
        // core is first laid out densely by a many-workgroup fill (one CU gathering it block by
        // block took ~28 us) -- inside the ticketed launch, or its own launch
        if (!df)
            M3S_HIP_CHECK(launch_sp_tail_fill(c.st, A, b, sp.iptr(sp.i_tmap), sp.iptr(sp.i_tail),
                                              sp.ntail, sp.npad_tail, sp.dptr<double>(sp.o_dense), flags));
        S.Hd = sp.ntail > 0 ? sp.dptr<double>(sp.o_dense) : nullptr;
        S.npad_h = sp.npad_tail;
        S.nmeta = (int)sp.nints_back;
        S.meta_lds = 1;
        S.do_fwd = 0;
        S.do_tail = S.do_back = 1;
        M3S_HIP_CHECK(launch_gn_solve_dbg(c.st, S));
        return M3S_OK;
    }
    if (sp.ntail > 0) c.may_timeout = true;  // the core's dataflow factorisation (chol_df)
    M3S_HIP_CHECK(launch_sp_tail(c.st, A, b, sp.iptr(sp.i_tmap), sp.iptr(sp.i_tail), sp.ntail,
                                 sp.npad_tail, sp.dptr<double>(sp.o_dense), sp.dptr<double>(sp.o_linv),
                                 sp.dptr<double>(sp.o_xd), x, flags, ++c.chol_epoch, !df));
    for (auto it = sp.rounds.rbegin(); it != sp.rounds.rend(); ++it)
        M3S_HIP_CHECK(launch_sp_back(c.st, it->nnodes, sp.iptr(sp.i_nodes), sp.iptr(sp.i_fptr),
                                     sp.iptr(sp.i_fronts), it->node_begin, Ls, W, y, x, flags));
    return M3S_OK;
}

// snapshot: read a copy of the factor taken now (sp.o_snap), not the live one
int enqueue_inverse(const m3s_gn_args& a, Ctx& c, bool snapshot) {
    const SparsePlan& sp = c.sp;
    const size_t shift = snapshot ? sp.o_snap - sp.o_L : 0;
    if (snapshot) {
        M3S_REQUIRE(sp.snap_bytes > 0, "PCG: no factor snapshot buffer");
        M3S_HIP_CHECK(hipMemcpyAsync(sp.dbuf + sp.o_snap, sp.dbuf + sp.o_L, sp.snap_bytes, hipMemcpyDeviceToDevice, c.st));
    }
    InvArgs v{};
    v.n = 7 * (int)(a.N - 1);
    v.ldx = sp.pcg_ldx;
    v.nrounds = (int)sp.rounds.size();
    v.ntail = sp.ntail;
    v.npad = sp.npad_tail;
    v.rounds = sp.iptr(sp.i_rounds);
    v.nodes = sp.iptr(sp.i_nodes);
    v.fptr = sp.iptr(sp.i_fptr);
    v.fronts = sp.iptr(sp.i_fronts);
    v.inl = sp.iptr(sp.i_inl);
    v.rc4 = sp.iptr(sp.i_rc4);
    v.tail = sp.iptr(sp.i_tail);
    v.Lstore = sp.dptr<double>(sp.o_L + shift);
    v.W = sp.dptr<double>(sp.o_W + shift);
    v.Hd = sp.dptr<double>(sp.o_dense + shift);
    v.Linv = sp.dptr<double>(sp.o_linv + shift);
    v.X = sp.dptr<double>(sp.o_pcgx);
    v.Xt = sp.dptr<float>(sp.o_pcgxt);
    v.ldt = sp.pcg_ldt;
    v.flags = c.at<int>(c.L.flags);
    // M3S_PCG_SIDE (default 1): on the side stream, beside the next iteration's accumulate (it
    // reads the factor and the flags, writes X only; the next PCG launch waits for it); 0: on
    // the call's stream
    static const bool side = env_int("M3S_PCG_SIDE", 1) != 0;
    if (!side) {
        M3S_HIP_CHECK(launch_sp_inverse(c.st, v));
        return M3S_OK;
    }
    hipStream_t ss;
    hipEvent_t e1, e2;
    int rc = pcg_side(ss, e1, e2);
    if (rc) return rc;
    M3S_HIP_CHECK(hipEventRecord(e1, c.st));
    M3S_HIP_CHECK(hipStreamWaitEvent(ss, e1, 0));
    // M3S_PCG_DEBUG=1: the refresh's duration on the side stream (timing events; serialises)
    static const bool dbg = env_int("M3S_PCG_DEBUG", 0) != 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    static long long* ibuf = nullptr;
    if (dbg && !ibuf && hipMalloc(&ibuf, sizeof(long long) * 8) != hipSuccess) ibuf = nullptr;
    v.dbg = dbg ? ibuf : nullptr;
    if (dbg) {
        if (ibuf) M3S_HIP_CHECK(hipMemsetAsync(ibuf, 0, sizeof(long long) * 8, ss));
        M3S_HIP_CHECK(hipEventCreate(&t0));
        M3S_HIP_CHECK(hipEventCreate(&t1));
        M3S_HIP_CHECK(hipEventRecord(t0, ss));
    }
    M3S_HIP_CHECK(launch_sp_inverse(ss, v));
    if (dbg) {
        M3S_HIP_CHECK(hipEventRecord(t1, ss));
        M3S_HIP_CHECK(hipEventSynchronize(t1));
        float ms = 0.f;
        M3S_HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
        long long h[8] = {0};
        if (ibuf) M3S_HIP_CHECK(hipMemcpy(h, ibuf, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "pcg inverse (M refresh): %.1f us, %d workgroups; wg0: init %.1f fwd rounds %.1f core %.1f back rounds %.1f f32 copy %.1f us\n",
                ms * 1e3, (v.n + 15) / 16, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01, (h[3] - h[2]) * 0.01,
                (h[4] - h[3]) * 0.01, (h[5] - h[4]) * 0.01);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
    }
    M3S_HIP_CHECK(hipEventRecord(e2, ss));
    c.inv_pending = true;
    c.inv_done = e2;
    return M3S_OK;
}

int enqueue_pcg(const m3s_gn_args& a, Ctx& c) {
    const SparsePlan& sp = c.sp;
    PcgArgs g{};
    g.b = sp.dptr<double>(sp.o_sys);
    g.A = g.b + sp.bpad;
    g.adj_ptr = sp.iptr(sp.i_apt);
    g.adj = reinterpret_cast<const int2*>(sp.iptr(sp.i_adj));
    g.nitem = sp.pcg_nitem;
    g.R4 = pcg_r4(sp.pcg_R);
    g.Xt = sp.dptr<float>(sp.o_pcgxt);
    g.ldt = sp.pcg_ldt;
    g.n = 7 * (int)(a.N - 1);
    g.nv = sp.pcg_nv;
    g.onex = sp.pcg_onex ? 1 : 0;
    g.R = sp.pcg_R;
    g.nwg = sp.pcg_nwg;
    g.gran = reinterpret_cast<unsigned long long*>(sp.dbuf + sp.o_gran);
    // tags: unique within the call (the granules are zeroed per call), 2 kmax + 1 exchanges a launch
    static const int kmax = std::max(1, std::min(200, env_int("M3S_PCG_KMAX", 30)));
    static const double tol = [] {
        const char* e = getenv("M3S_PCG_TOL");
        return e ? atof(e) : 1e-6;
    }();
    g.kmax = kmax;
    g.tol2 = tol * tol;
    g.tag0 = 1u + (unsigned)c.pcg_launches * (unsigned)(2 * kmax + 2);
    c.pcg_launches++;
    const char* ft = getenv("M3S_TEST_FORCE_TIMEOUT");
    g.spin_limit = (ft && atoi(ft) != 0) ? 0 : (1 << 22);
    g.Twc = a.Twc;
    g.dx = a.dx;
    g.N = (int)a.N;
    g.delta_thresh = a.delta_thresh;
    g.contract = a.contract;
    g.flags = c.at<int>(c.L.flags);
    // M3S_PCG_DEBUG=1: workgroup 0's phase clocks, printed after the launch (the wait serialises
    // the call: diagnostics only)
    static const bool dbg = env_int("M3S_PCG_DEBUG", 0) != 0;
    static long long* dbuf = nullptr;
    if (dbg && !dbuf && hipMalloc(&dbuf, sizeof(long long) * kPcgDbgSlots) != hipSuccess) dbuf = nullptr;
    if (dbg && dbuf) M3S_HIP_CHECK(hipMemsetAsync(dbuf, 0, sizeof(long long) * kPcgDbgSlots, c.st));
    g.dbg = dbg ? dbuf : nullptr;
    M3S_HIP_CHECK(launch_pcg(c.st, g));
    if (g.dbg) {
        long long h[kPcgDbgSlots];
        M3S_HIP_CHECK(hipMemcpyAsync(h, dbuf, sizeof(h), hipMemcpyDeviceToHost, c.st));
        M3S_HIP_CHECK(hipStreamSynchronize(c.st));
        // s_memrealtime: 100 MHz
        fprintf(stderr, "pcg[%d] R %d nwg %d: stage %.2f us, z0 %.2f us;", c.pcg_launches - 1, g.R, g.nwg,
                (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01);
        long long prev = h[2];
        for (int st = 1; 3 * st + 2 < kPcgDbgSlots && h[3 * st + 2] != 0; st++) {
            fprintf(stderr, " [Ap %.2f pq %.2f z %.2f]", (h[3 * st] - prev) * 0.01, (h[3 * st + 1] - h[3 * st]) * 0.01,
                    (h[3 * st + 2] - h[3 * st + 1]) * 0.01);
            prev = h[3 * st + 2];
        }
        fprintf(stderr, "\n");
    }
    return M3S_OK;
}

}  // namespace m3s

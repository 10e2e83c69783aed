// gn_plan.hip -- what the host decides once per Gauss-Newton call (gn_host.h).
//
// Replaces the host side of SparseBlock (reference gn_kernels.cu:57-159) and the keyframe remap
// of gauss_newton_{points,rays,calib}_cuda (unique + searchsorted, :161-170):
//   - the pinned staging buffers of the per-call transfers;
//   - the accumulate's chunking, the workspace layout and the XCD-aware task order;
//   - build_plan: the ONE host sync of a call (ii/jj and K to the host), the block-sparse layout
//     of the pose graph and the deterministic CSR contribution lists;
//   - the elimination plan (sparse_plan.h) the solve runs: its round policies, the choice between
//     the single-workgroup, hybrid and multi-launch plans, the lagged-factor PCG's policy, and
//     the plan's upload;
//   - argument validation and the summation order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "gn_host.h"
#include "m3s_comm.h"

namespace m3s {

void Staging::release(void* p) {
    Staging* s = static_cast<Staging*>(p);
    if (s->pending) (void)hipEventSynchronize(s->done);
    if (s->done) (void)hipEventDestroy(s->done);
    if (s->buf) (void)hipHostFree(s->buf);
    s->buf = s->dev = nullptr;
    s->cap = 0;
    s->done = nullptr;
    s->pending = false;
}
char* Staging::get(size_t bytes) {
    if (pending) {
        (void)hipEventSynchronize(done);
        pending = false;
    }
    if (bytes > cap) {
        if (buf) (void)hipHostFree(buf);
        cap = align_up(std::max<size_t>(bytes, 1 << 16) * 2, 4096);
        if (hipHostMalloc((void**)&buf, cap, hipHostMallocDefault) != hipSuccess) {
            buf = nullptr;
            cap = 0;
        } else if (hipHostGetDevicePointer((void**)&dev, buf, 0) != hipSuccess) {
            dev = nullptr;
        }
    }
    return buf;
}
hipError_t Staging::upload(void* dst, const char* h, size_t bytes, hipStream_t st) {
    static const bool dma = [] {
        const char* e = getenv("M3S_STAGE_DMA");
        return e && atoi(e) != 0;
    }();
    if (!dma && dev && (bytes & 3) == 0 && ((uintptr_t)dst & 15) == 0 && ((h - buf) & 15) == 0)
        return launch_stage_copy(st, dst, dev + (h - buf), bytes);
    return hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st);
}
hipError_t Staging::download(char* h, const void* src, size_t bytes, hipStream_t st) {
    static const bool dma = [] {
        const char* e = getenv("M3S_STAGE_DMA");
        return e && atoi(e) != 0;
    }();
    if (!dma && dev && (bytes & 3) == 0 && ((uintptr_t)src & 15) == 0 && ((h - buf) & 15) == 0)
        return launch_stage_copy(st, dev + (h - buf), src, bytes);
    return hipMemcpyAsync(h, src, bytes, hipMemcpyDeviceToHost, st);
}
hipError_t Staging::mark(hipStream_t st) {
    if (!done) {
        hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipEventRecord(done, st);
    pending = e == hipSuccess;
    return e;
}
void Stagings::release(void* p) {
    Stagings* s = static_cast<Stagings*>(p);
    Staging::release(&s->in);
    Staging::release(&s->out);
    Staging::release(&s->ws);
    Staging::release(&s->tmo);
    s->tmo_armed = 0;
}
namespace {
thread_local Stagings* t_stagings = nullptr;
}  // namespace
Stagings& stagings() {
    if (!t_stagings) {
        t_stagings = new Stagings;
        register_host_resource(t_stagings, &Stagings::release);
    }
    return *t_stagings;
}

namespace {
// Points per accumulate task (edge x chunk).  16384 (round 3): the chunks amortise the task
// prologue (pose loads, the affine map) and the workgroup reduction over twice the points of the
// former 8192 -- cfg3 accumulate 0.342 -> 0.331 ms, cfg4 1.98 -> 1.94 ms; flat up to ~49k
// (profiles/r03_chunk_ab.txt)
int chunk_target() {
    static int t = [] {
        const char* e = getenv("M3S_ACC_CHUNK");
        return e ? std::max(1024, atoi(e)) : 16384;
    }();
    return t;
}

// Number of point chunks per directed edge: chunks of ~chunk_target() points (the per-XCD
// working set of a chunk-major schedule is ~16 keyframes x chunk x 16 B), and at least
// ~4096 workgroups overall when the edge count is small.
int choose_nchunks(int64_t HW, int64_t E_local) {
    int64_t nc = (HW + chunk_target() - 1) / chunk_target();
    const int64_t want = (4096 + std::max<int64_t>(E_local, 1) - 1) / std::max<int64_t>(E_local, 1);
    nc = std::max(nc, want);
    const int64_t max_nc = std::max<int64_t>(1, (HW + 1023) / 1024);
    nc = std::min(std::max<int64_t>(nc, 1), max_nc);
    int64_t chunk = align_up((size_t)((HW + nc - 1) / nc), 4);
    nc = (HW + chunk - 1) / chunk;
    return (int)std::max<int64_t>(nc, 1);
}
}  // namespace

int chunk_points(int64_t HW, int nchunks) {
    return (int)align_up((size_t)((HW + nchunks - 1) / nchunks), 4);
}

Layout make_layout(int mode, int64_t N, int64_t HW, int64_t E_total, int64_t E_local) {
    Layout L{};
    const int64_t npose = std::max<int64_t>(N - 1, 0);
    const int64_t n = 7 * npose;
    // from the TOTAL edge count: every rank of a sharded call then chunks its edges exactly as one
    // GPU would, so the per-edge f32 partial sums (and the poses, up to the f64 all-reduce order)
    // do not depend on the number of ranks
    L.nchunks = choose_nchunks(HW, E_total);
    L.npad = (int)std::max<int64_t>(kCholTile, align_up((size_t)n, kCholTile));
    L.nblk_max = (int)(npose + E_total);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + std::max<size_t>(bytes, 1), 256);
        return o;
    };
    L.partials = take(sizeof(float) * (size_t)E_local * L.nchunks * kNaccPad);
    // per-edge records: the fast path's f64 Hjj/vj (kEdgeBlk doubles), or the reference-order
    // path's f32 D/g (kRefStride floats)
    static_assert(sizeof(float) * kRefStride <= sizeof(double) * kEdgeBlk, "edge record");
    L.edgeblk = take(sizeof(double) * (size_t)E_local * kEdgeBlk);
    L.compact = take(sizeof(double) * ((size_t)L.nblk_max * 28 + (size_t)npose * 7));
    // (the dense f64 matrices -- the dense solver's / debug system's (npad+64) x npad, the sparse
    // solvers' core -- are sized by the solver actually used, in per-call stream-ordered
    // allocations: see Ctx::alloc_dense and upload_sparse_plan)
    L.x = take(sizeof(double) * (size_t)L.npad);
    L.flags = take(sizeof(int) * kNumFlags);
    L.cok = take(sizeof(int) * (size_t)std::max<int64_t>(N, 1));  // per keyframe: every c > C_thresh
    L.twc_save = take(sizeof(float) * 8 * (size_t)std::max<int64_t>(N, 1));  // Twc at the call's start
    L.ii_loc = take(sizeof(int) * (size_t)E_local);
    L.jj_loc = take(sizeof(int) * (size_t)E_local);
    L.blk_ptr = take(sizeof(int) * ((size_t)L.nblk_max + 1));
    // (the CSR lists span ALL edges when the ranks' records are gathered: Plan::gather)
    L.blk_ent = take(sizeof(int) * (size_t)std::max(E_local, E_total) * 4);
    L.blk_ref = take(sizeof(int) * (size_t)E_local * 4);  // reference-order assembly codes
    L.grad_ptr = take(sizeof(int) * ((size_t)npose + 1));
    L.grad_ent = take(sizeof(int) * (size_t)std::max(E_local, E_total) * 2);
    L.ecnt = take(sizeof(int) * (size_t)E_local);  // fused edge reduce: finished chunks per edge
    L.sorder = take(sizeof(int) * (size_t)E_local);  // the accumulate schedule's edge order
    L.sched = take(sizeof(int) * 4 * (size_t)E_local * L.nchunks);  // {edge, chunk, ix, jx} per task
    // iteration-invariant packed stream {code, sqrt q} per directed point-edge (8 B), and the
    // dense depth array of the keyframes (calib)
    if (env_int("M3S_GN_COMPACT", 0) != 0) {
        // compacted stream (opt-in): every (edge, chunk) region holds a whole chunk
        const size_t cap = (size_t)E_local * (size_t)L.nchunks * (size_t)chunk_points(HW, L.nchunks);
        L.pack = take(8 * std::max(cap, (size_t)E_local * (size_t)HW));
        L.packx = take(12 * cap);
        L.pcnt = take(sizeof(int) * (size_t)E_local * L.nchunks);
    } else {
        L.pack = take(8 * (size_t)E_local * (size_t)HW);
        L.packx = L.pcnt = L.pack;  // unused
    }
    // + the ray tables tu[W], tv[H] (gn_depth_kernel); HW floats is an upper bound for W + H
    // + the inverse depths IZs [N, HW] after the tables (gn_accum.hip inv_depths)
    L.zs = take(mode == M3S_GN_CALIB ? sizeof(float) * (2 * (size_t)N + 1) * (size_t)HW + 64 : 0);
    L.total = off;
    return L;
}

// XCD-aware order of the accumulate tasks (a performance heuristic only: results do not
// depend on it).  Local directed edges sorted by (jx, ix) are split into 8 contiguous
// groups, one per XCD (blocks b, b+8, ... share an XCD under round-robin dispatch); inside a
// group tasks run chunk-major, so the few keyframes of a group stay L2-resident while all
// of their edges stream the same point range.  The host orders the edges (two stable
// counting sorts, by ix then by jx: the stable (jx, ix) order, O(E + N)) and sizes the groups;
// the device expands the task records {e, c, ix, jx} (launch_sched_expand): group g's list is
// chunk-major (element k: edge order[lo_g + k % n_g], chunk k / n_g) and the groups are
// interleaved round-robin.  (Written record by record into pinned memory and read back over
// PCIe, the schedule cost ~0.1 ms of host time per cfg4 call.)
void build_schedule_order(const std::vector<int>& ii_loc, const std::vector<int>& jj_loc, int nkey, int* order,
                          SchedGroups& G) {
    const int E = (int)ii_loc.size();
    static const bool off = [] {
        const char* e = getenv("M3S_ACC_SCHED");
        return e && atoi(e) == 0;
    }();
    G = SchedGroups{};
    G.off = off ? 1 : 0;
    if (off || E == 0) return;
    static thread_local std::vector<int> tmp, cnt;
    tmp.resize(E);
    auto pass = [&](const std::vector<int>& key, const int* src, int* dst) {
        cnt.assign((size_t)nkey + 1, 0);
        for (int k = 0; k < E; k++) cnt[key[src ? src[k] : k] + 1]++;
        for (int v = 0; v < nkey; v++) cnt[v + 1] += cnt[v];
        for (int k = 0; k < E; k++) {
            const int e = src ? src[k] : k;
            dst[cnt[key[e]]++] = e;
        }
    };
    pass(ii_loc, nullptr, tmp.data());
    pass(jj_loc, tmp.data(), order);
    constexpr int NG = 8;
    G.q = E;
    for (int g = 0; g < NG; g++) {
        G.lo[g] = (int)((int64_t)E * g / NG);
        G.n[g] = (int)((int64_t)E * (g + 1) / NG) - G.lo[g];
        G.q = std::min(G.q, G.n[g]);
    }
    for (int g = 0; g < NG; g++)
        if (G.n[g] > G.q) G.big[G.nbig++] = g;
}

namespace {
// The pose graph's blocks from the edge lists (host copies): keyframe ids -> rows by
// unique(cat(ii, jj)) sorted + searchsorted (gn_kernels.cu:161-170), the first row pinned
// (num_fix = 1); diagonal blocks first (slot p <-> pose p), then the unordered pose pairs in order
// of first appearance over ALL edges; slotmap is the dense (npose x npose) slot table.
int plan_pairs(const int64_t* hii, const int64_t* hjj, int64_t E, int64_t N, Plan& plan, std::vector<int>& iopt,
               std::vector<int>& jopt) {
    const int npose = (int)(N - 1);
    iopt.resize(E);
    jopt.resize(E);
    // keyframe ids are small non-negative integers in practice: rank them through a dense
    // table (O(E + max id)); a comparison sort of the 2E ids took most of this function's
    // ~0.2 ms per cfg4 call.  Other ids: sort + binary search.
    int64_t lo = 0, hi = -1;
    for (int64_t e = 0; e < E; e++) {
        lo = std::min({lo, hii[e], hjj[e]});
        hi = std::max({hi, hii[e], hjj[e]});
    }
    size_t nuniq = 0;
    if (lo >= 0 && hi < std::max<int64_t>(1 << 16, 8 * (E + N))) {
        static thread_local std::vector<int> rank;
        rank.assign((size_t)hi + 1, 0);
        for (int64_t e = 0; e < E; e++) rank[hii[e]] = rank[hjj[e]] = 1;
        for (int64_t id = 0; id <= hi; id++)
            if (rank[id]) rank[id] = (int)nuniq++;
        if ((int64_t)nuniq <= N)
            for (int64_t e = 0; e < E; e++) {
                iopt[e] = rank[hii[e]] - 1;  // pin = num_fix = 1
                jopt[e] = rank[hjj[e]] - 1;
            }
    } else {
        std::vector<int64_t> u(hii, hii + E);
        u.insert(u.end(), hjj, hjj + E);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        nuniq = u.size();
        auto row_of = [&](int64_t id) { return (int)(std::lower_bound(u.begin(), u.end(), id) - u.begin()); };
        if ((int64_t)nuniq <= N)
            for (int64_t e = 0; e < E; e++) {
                iopt[e] = row_of(hii[e]) - 1;
                jopt[e] = row_of(hjj[e]) - 1;
            }
    }
    M3S_REQUIRE((int64_t)nuniq <= N,
                "gauss_newton: %lld unique keyframe ids in ii/jj but only %lld poses in Twc/Xs",
                (long long)nuniq, (long long)N);
    plan.slotmap.assign((size_t)std::max(npose, 0) * std::max(npose, 0), -1);
    for (int q = 0; q < npose; q++) plan.slotmap[(size_t)q * npose + q] = q;
    plan.nblk = npose;
    plan.pairs.clear();
    for (int64_t e = 0; e < E; e++) {
        const int i = iopt[e], j = jopt[e];
        if (i >= 0 && j >= 0 && i != j && plan.slotmap[(size_t)i * npose + j] < 0) {
            plan.slotmap[(size_t)i * npose + j] = plan.slotmap[(size_t)j * npose + i] = plan.nblk++;
            plan.pairs.push_back(std::make_pair(std::min(i, j), std::max(i, j)));
        }
    }
    return M3S_OK;
}
}  // namespace

double g_plan_sync_us = 0;  // M3S_PROF_HOST: build_plan's edge-list copies + stream sync

// before_wait: enqueued after the edge-list copies, before the host waits for them (work that
// needs no plan runs on the GPU while the host plans)
int build_plan(const m3s_gn_args& a, hipStream_t st, Plan& plan, const std::function<int()>& before_wait) {
    const int64_t E = a.E_total;
    // sharded call: gather the edge records (M3S_GN_GATHER=0: all-reduce the assembled system)
    int grank = 0, granks = 1;
    if (a.comm && gn_order(a) != M3S_GN_ORDER_REFERENCE && env_int("M3S_GN_GATHER", 1) != 0) {
        int rc = comm_rank_size(a.comm, &grank, &granks);
        if (rc) return rc;
    }
    const size_t hb_ranges = align_up(sizeof(int64_t) * 2 * (size_t)E + 64, 64);
    char* hb = stagings().in.get(hb_ranges + sizeof(double) * 2 * (size_t)granks);
    M3S_REQUIRE(hb != nullptr, "gauss_newton: pinned host allocation failed");
    int64_t* hii = reinterpret_cast<int64_t*>(hb);
    int64_t* hjj = hii + E;
    float* Kh = reinterpret_cast<float*>(hjj + E);
    double* hr = reinterpret_cast<double*>(hb + hb_ranges);  // every rank's (edge_offset, E_local)
    double* dr = nullptr;
    if (granks > 1) {
        // the ranks' edge ranges (once per call; exact in f64 below 2^53)
        hr[2 * grank] = (double)a.edge_offset;
        hr[2 * grank + 1] = (double)a.E_local;
        M3S_HIP_CHECK(hipMallocAsync((void**)&dr, sizeof(double) * 2 * (size_t)granks, st));
        Staging& in = stagings().in;
        M3S_HIP_CHECK(in.upload(dr + 2 * grank, reinterpret_cast<const char*>(hr + 2 * grank), sizeof(double) * 2, st));
        int rc = comm_allgather_f64(a.comm, dr, 2, st);
        if (rc) {
            (void)hipFreeAsync(dr, st);
            return rc;
        }
        M3S_HIP_CHECK(in.download(reinterpret_cast<char*>(hr), dr, sizeof(double) * 2 * (size_t)granks, st));
        M3S_HIP_CHECK(hipFreeAsync(dr, st));
    }
    const auto c0 = std::chrono::steady_clock::now();
    Staging& in = stagings().in;
    if (E > 0) {
        M3S_HIP_CHECK(in.download(reinterpret_cast<char*>(hii), a.ii, sizeof(int64_t) * E, st));
        M3S_HIP_CHECK(in.download(reinterpret_cast<char*>(hjj), a.jj, sizeof(int64_t) * E, st));
    }
    if (a.mode == M3S_GN_CALIB)
        M3S_HIP_CHECK(in.download(reinterpret_cast<char*>(Kh), a.K, sizeof(float) * 9, st));
    if (before_wait) {
        static thread_local hipEvent_t copied = nullptr;  // (no destructor: nothing at exit)
        if (!copied) M3S_HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        M3S_HIP_CHECK(hipEventRecord(copied, st));
        int rc = before_wait();
        if (rc) return rc;
        M3S_HIP_CHECK(hipEventSynchronize(copied));
    } else {
        M3S_HIP_CHECK(hipStreamSynchronize(st));
    }
    g_plan_sync_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
    // gathered position of every edge, when the ranks' ranges partition [0, E) (else: the
    // all-reduce of the assembled system, which sums whatever the ranks hold)
    std::vector<int> gpos;
    plan.gather = false;
    plan.grank = grank;
    plan.granks = granks;
    plan.gchunk = 0;
    if (granks > 1) {
        int64_t chunk = 0;
        std::vector<int> cover(E, 0);
        bool ok = true;
        gpos.assign(E, -1);
        for (int r = 0; r < granks && ok; r++) {
            const int64_t off = (int64_t)hr[2 * r], cnt = (int64_t)hr[2 * r + 1];
            ok = off >= 0 && cnt >= 0 && off + cnt <= E;
            chunk = std::max(chunk, cnt);
        }
        for (int r = 0; r < granks && ok; r++) {
            const int64_t off = (int64_t)hr[2 * r], cnt = (int64_t)hr[2 * r + 1];
            for (int64_t k = 0; k < cnt && ok; k++) {
                ok = cover[off + k]++ == 0;
                gpos[off + k] = (int)(r * chunk + k);
            }
        }
        for (int64_t e = 0; e < E && ok; e++) ok = cover[e] == 1;
        ok = ok && (int64_t)granks * chunk < (int64_t)(INT32_MAX >> 3);
        if (ok && chunk > 0) {
            plan.gather = true;
            plan.gchunk = (int)chunk;
        }
    }
    if (a.mode == M3S_GN_CALIB) {
        plan.K[0] = Kh[0];  // fx = K[0][0]
        plan.K[1] = Kh[4];  // fy = K[1][1]
        plan.K[2] = Kh[2];  // cx = K[0][2]
        plan.K[3] = Kh[5];  // cy = K[1][2]
    }

    const int npose = (int)(a.N - 1);
    std::vector<int> iopt, jopt;
    int rc = plan_pairs(hii, hjj, E, a.N, plan, iopt, jopt);
    if (rc) return rc;
    auto slot = [&](int r, int c) { return plan.slotmap[(size_t)r * npose + c]; };

    // contributions of the LOCAL edges as CSR lists (update_lhs order per edge:
    // (ii,ii,+) (ii,jj,-) (jj,ii,-) (jj,jj,+)), built by counting sort
    plan.ii_loc.resize(a.E_local);
    plan.jj_loc.resize(a.E_local);
    plan.blk_ptr.assign(plan.nblk + 1, 0);
    plan.grad_ptr.assign(std::max(npose, 0) + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        std::vector<int> bfill, gfill;
        if (pass == 1) {
            for (int k = 0; k < plan.nblk; k++) plan.blk_ptr[k + 1] += plan.blk_ptr[k];
            for (int k = 0; k < npose; k++) plan.grad_ptr[k + 1] += plan.grad_ptr[k];
            plan.blk_ent.assign(plan.blk_ptr[plan.nblk], 0);
            plan.blk_ref.assign(plan.gather ? 0 : plan.blk_ptr[plan.nblk], 0);
            plan.grad_ent.assign(plan.grad_ptr[npose], 0);
            bfill.assign(plan.blk_ptr.begin(), plan.blk_ptr.end() - 1);
            gfill.assign(plan.grad_ptr.begin(), plan.grad_ptr.end() - 1);
        }
        // the lists' edges: the local ones, or ALL (by gathered position) when gathering
        const int64_t nlist = plan.gather ? E : a.E_local;
        for (int64_t el = 0; el < nlist; el++) {
            const int64_t e = plan.gather ? el : a.edge_offset + el;
            const int64_t code = plan.gather ? gpos[e] : el;
            const int i = iopt[e], j = jopt[e];
            if (pass == 0 && !plan.gather) {
                plan.ii_loc[el] = i + 1;
                plan.jj_loc[el] = j + 1;
            }
            const int rr[4] = {i, i, j, j}, cc[4] = {i, j, i, j}, neg[4] = {0, 1, 1, 0};
            for (int b = 0; b < 4; b++) {
                if (rr[b] >= 0 && cc[b] >= 0 && rr[b] <= cc[b]) {
                    const int sl = slot(rr[b], cc[b]);
                    if (pass == 0) {
                        plan.blk_ptr[sl + 1]++;
                    } else {
                        // reference-order block types (gn_assemble_ref_kernel): Hs[0]/Hs[3] on
                        // the diagonal, Hs[1] at (ii, jj) when ii < jj, Hs[2] at (jj, ii) when
                        // jj < ii, a self-edge's Hs[1]/Hs[2] on its diagonal block
                        const int type = (b == 0 || b == 3) ? 0 : (i == j ? (b == 1 ? 3 : 4) : (b == 1 ? 2 : 1));
                        if (!plan.gather) plan.blk_ref[bfill[sl]] = (int)(el << 3) | type;
                        plan.blk_ent[bfill[sl]++] = (int)(code << 1) | neg[b];
                    }
                }
            }
            if (i >= 0) {  // vi = -vj
                if (pass == 0) plan.grad_ptr[i + 1]++;
                else plan.grad_ent[gfill[i]++] = (int)(code << 1) | 1;
            }
            if (j >= 0) {
                if (pass == 0) plan.grad_ptr[j + 1]++;
                else plan.grad_ent[gfill[j]++] = (int)(code << 1);
            }
        }
    }
    if (plan.gather) {
        for (int64_t el = 0; el < a.E_local; el++) {
            plan.ii_loc[el] = iopt[a.edge_offset + el] + 1;
            plan.jj_loc[el] = jopt[a.edge_offset + el] + 1;
        }
        plan.blk_ref.clear();  // (the reference order never gathers)
    }
    return M3S_OK;
}


// ---------------------------------------------------------------------------------
// Block-sparse elimination plan (sparse_plan.h builds it, gn_sparse.hip runs it): its round
// policies and the upload.
// ---------------------------------------------------------------------------------
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

namespace {
RoundPolicy fused_policy() {
    return {true, env_int("M3S_SPARSE_DCAP", 64), env_int("M3S_SPARSE_RMIN", 1),
            env_int("M3S_SPARSE_RMAX", 64),
            std::min(kTailPoseMax, env_int("M3S_SPARSE_TAILCAP", kTailPoseMax)),
            env_int("M3S_SPARSE_KMIN", 4), env_int("M3S_SPARSE_MMD", 1) != 0};
}
// multi: dcap 32 (round 5: cfg4 -- 255 free poses, 1007 pose pairs -- 4 rounds and a 125-pose
// core instead of 3 rounds and 141 poses; solve 0.307 -> 0.288 ms per iteration on one box, dcap
// 24 0.292, 64 0.301: profiles/r05_b_dcap*.json)
RoundPolicy multi_policy() {
    return {false, env_int("M3S_MULTI_DCAP", 32), env_int("M3S_MULTI_RMIN", 2),
            env_int("M3S_MULTI_RMAX", 64), 0, env_int("M3S_MULTI_KMIN", 4), env_int("M3S_MULTI_MMD", 0) != 0};
}
// hybrid: multi-launch rounds in minimum-degree order down to a dense core, then gn_solve
// back-substitutes and retracts.  The core is factored by the dataflow launch (M3S_HYB_CORE=1,
// default) -- then it is not bound by gn_solve's in-register factorisation (kTailPoseMax poses)
// and M3S_HYB_TAILCAP may move the rounds' stop point up to kHybDfTailMax poses -- or in
// registers (M3S_HYB_CORE=0: <= kTailPoseMax poses).
// Default stop point with the dataflow core: 36 poses (252 unknowns: still 4 tile columns), where
// a round must remove >= kmin poses to continue -- cfg3: 5 rounds and a 34-pose core instead of 8
// rounds and 26 poses, solve 0.1205 -> 0.1148 ms per iteration (two interleaved same-box rounds;
// caps 30 and 40 with kmin 6 -- 7 rounds / 28 poses, 4 rounds / 39 poses in 5 tiles -- were slower:
// profiles/r05_ap_hyb_tailcap/).
constexpr int kHybDfTailMax = 64;
constexpr int kHybDfTailDefault = 36;
// read by the planner per call and carried with the plan (SparsePlan::core_df), so that
// enqueue_solve factors the core the way the plan was sized for (a per-call read
// beside a per-process one could hand a 28-64-pose core to the in-register factorisation)
bool hyb_core_df() { return env_int("M3S_HYB_CORE", 1) != 0; }
RoundPolicy hybrid_policy() {
    const bool df = hyb_core_df();
    return {false, env_int("M3S_HYB_DCAP", 64), env_int("M3S_HYB_RMIN", 1),
            env_int("M3S_HYB_RMAX", 64),
            std::min(df ? kHybDfTailMax : kTailPoseMax, env_int("M3S_HYB_TAILCAP", df ? kHybDfTailDefault : kTailPoseMax)),
            env_int("M3S_HYB_KMIN", 4), env_int("M3S_HYB_MMD", 1) != 0};
}
// the hybrid plan's core fits its factorisation
bool hyb_core_fits(const SparsePlan& p) {
    return hyb_core_df() ? p.ntail <= kHybDfTailMax : p.fused_tail;
}
}  // namespace

int upload_sparse_plan(SparsePlan& sp, int npose, hipStream_t st) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + std::max<size_t>(bytes, 8), 256);
        return o;
    };
    sp.bpad = (int)align_up((size_t)npose * 7, 49);
    sp.o_sys = take(sizeof(double) * ((size_t)sp.bpad + 49 * (size_t)sp.nblocks));
    sp.o_y = take(sizeof(double) * 7 * (size_t)npose);
    sp.o_L = take(sizeof(double) * std::max(kLStoreRec, 49) * sp.nodes.size());
    sp.o_W = take(sizeof(double) * 49 * (size_t)sp.nW);
    sp.o_xd = take(sizeof(double) * (size_t)std::max(sp.npad_tail, 1));
    if (sp.npad_tail > 0) {
        sp.o_dense = take(sizeof(double) * (size_t)(sp.npad_tail + kCholTile) * sp.npad_tail);
        sp.o_linv = take(chol_linv_bytes(sp.npad_tail));
    }
    sp.o_Lg = take(sp.fused_tail ? sizeof(double) * 49 * (size_t)sp.ntail * sp.ntail : 0);
    sp.o_dfcnt = take(sizeof(int) * (size_t)sp_rounds_df_words((int)sp.rounds.size()));
    if (sp.pcg) {
        sp.snap_bytes = 0;
        if (sp.pcg_lag >= 2) {
            sp.snap_bytes = (sp.npad_tail > 0 ? sp.o_linv + chol_linv_bytes(sp.npad_tail) : sp.o_xd) - sp.o_L;
            sp.o_snap = take(sp.snap_bytes);
        }
        sp.o_pcgx = take(sizeof(double) * (size_t)npose * 7 * sp.pcg_ldx);
        sp.o_pcgxt = take(sizeof(float) * (size_t)npose * 7 * sp.pcg_ldt);
        sp.o_gran = take(16 * 4 * (size_t)sp.pcg_nv);
    }
    // the plan integers in one array (layout: SparsePlan), the rounds BEFORE tmap: a launch that
    // only back-substitutes stages [nodes fptr fronts tail rounds] and not the core map
    std::vector<const std::vector<int>*> parts = {&sp.nodes, &sp.fptr, &sp.fronts, &sp.tail,
                                                  &sp.tmap, &sp.tg, &sp.tc, &sp.rtg, &sp.rc,
                                                  &sp.tc3, &sp.rc4, &sp.inl, &sp.apt, &sp.adj};
    size_t* offs[] = {&sp.i_nodes, &sp.i_fptr, &sp.i_fronts, &sp.i_tail, &sp.i_tmap, &sp.i_tg,
                      &sp.i_tc, &sp.i_rtg, &sp.i_rc, &sp.i_tc3, &sp.i_rc4, &sp.i_inl, &sp.i_apt, &sp.i_adj};
    // (inl: its first ninl ints; SparsePlan::inl)
    auto len = [&](size_t k) { return parts[k] == &sp.inl ? sp.ninl : parts[k]->size(); };
    size_t n = 0;
    for (size_t k = 0; k < parts.size(); k++) {
        if (k == 4) {
            sp.i_rounds = n;
            n += 8 * sp.rounds.size();
        }
        if (parts[k] == &sp.inl) n = align_up(n, 4);  // 16-B records (int4 loads)
        if (parts[k] == &sp.adj) n = align_up(n, 2);  // int2 entries
        *offs[k] = n;
        n += len(k);
    }
    sp.o_int = take(sizeof(int) * std::max<size_t>(n, 1));
    M3S_HIP_CHECK(hipMallocAsync((void**)&sp.dbuf, off, st));
    M3S_HIP_CHECK(hipMemsetAsync(sp.dbuf + sp.o_dfcnt, 0, sizeof(int) * (size_t)sp_rounds_df_words((int)sp.rounds.size()), st));
    if (sp.npad_tail > 0)  // the dataflow factor's ready words start below every epoch
        M3S_HIP_CHECK(hipMemsetAsync(chol_ready_ptr(sp.dptr<double>(sp.o_linv), sp.npad_tail), 0,
                                     chol_ready_bytes(sp.npad_tail), st));
    if (sp.pcg)  // the exchange's tags start below every launch's
        M3S_HIP_CHECK(hipMemsetAsync(sp.dbuf + sp.o_gran, 0, 16 * 4 * (size_t)sp.pcg_nv, st));
    if (n > 0) {
        int* h = reinterpret_cast<int*>(stagings().out.get(sizeof(int) * n));
        M3S_REQUIRE(h != nullptr, "gauss_newton: pinned host allocation failed");
        for (size_t k = 0; k < parts.size(); k++)
            if (len(k) > 0) std::memcpy(h + *offs[k], parts[k]->data(), sizeof(int) * len(k));
        int* hr = h + sp.i_rounds;
        for (const SpRound& R : sp.rounds) {
            const int v[8] = {R.node_begin, R.nnodes, R.tbeg, R.nbt, R.rbeg, R.nrt, R.wbeg, R.wcount};
            std::memcpy(hr, v, sizeof(v));
            hr += 8;
        }
        M3S_HIP_CHECK(stagings().out.upload(sp.dbuf + sp.o_int, reinterpret_cast<const char*>(h), sizeof(int) * n, st));
        M3S_HIP_CHECK(stagings().out.mark(st));  // no host sync: the staging buffer outlives the copy
    }
    return M3S_OK;
}

// M3S_GN_ORDER_*: the args field, else env M3S_GN_ORDER=reference|fast, else fast
int gn_order(const m3s_gn_args& a) {
    if (a.order == M3S_GN_ORDER_FAST || a.order == M3S_GN_ORDER_REFERENCE) return a.order;
    static const int env = [] {
        const char* e = getenv("M3S_GN_ORDER");
        if (e && (!strcmp(e, "reference") || !strcmp(e, "ref") || !strcmp(e, "2"))) return (int)M3S_GN_ORDER_REFERENCE;
        return (int)M3S_GN_ORDER_FAST;
    }();
    return env;
}

int validate(const m3s_gn_args& a) {
    M3S_REQUIRE(a.order >= M3S_GN_ORDER_DEFAULT && a.order <= M3S_GN_ORDER_REFERENCE,
                "gauss_newton: bad summation order %d", a.order);
    M3S_REQUIRE(a.mode == M3S_GN_POINTS || a.mode == M3S_GN_RAYS || a.mode == M3S_GN_CALIB,
                "gauss_newton: bad mode %d", a.mode);
    M3S_REQUIRE(a.contract == M3S_CONTRACT_NVCC || a.contract == M3S_CONTRACT_OFF ||
                    a.contract == M3S_CONTRACT_NVCC_RIGHT,
                "gauss_newton: unknown contraction convention %d", a.contract);
    M3S_REQUIRE(a.N >= 1 && a.HW >= 1, "gauss_newton: need N >= 1 poses and HW >= 1 points");
    M3S_REQUIRE(a.E_total >= 0 && a.E_local >= 0 && a.edge_offset >= 0 &&
                    a.edge_offset + a.E_local <= a.E_total,
                "gauss_newton: bad edge range");
    M3S_REQUIRE(a.HW < ((int64_t)1 << 31) && a.E_local < (1 << 30),
                "gauss_newton: sizes exceed int32 indexing");
    // the dense solver (M3S_SOLVER_DENSE=1, diagnostics) factors the whole system; the sparse
    // solvers check their dense core against the same limit after planning (run())
    if (env_int("M3S_SOLVER_DENSE", 0) != 0 && a.order != M3S_GN_ORDER_REFERENCE)
        M3S_REQUIRE(7 * (a.N - 1) <= kMaxNpad,
                    "gauss_newton: %lld poses exceed the dense solve limit (%d unknowns)",
                    (long long)a.N, kMaxNpad);
    M3S_REQUIRE(a.mode != M3S_GN_CALIB || (a.K != nullptr && a.width > 0 && a.height > 0),
                "gauss_newton_calib: K / image size required");
    M3S_REQUIRE(a.Twc && a.Xs && a.Cs && a.dx, "gauss_newton: null pointer");
    if (a.E_total > 0) M3S_REQUIRE(a.ii && a.jj, "gauss_newton: null ii/jj");
    if (a.E_local > 0) M3S_REQUIRE(a.idx && a.valid && a.Q, "gauss_newton: null edge data");
    if (a.idx_b || a.valid_b || a.Q_b) {
        M3S_REQUIRE(a.idx_b && a.valid_b && a.Q_b, "gauss_newton: incomplete second edge half");
        M3S_REQUIRE(a.E_a >= 0 && a.E_a <= a.E_local, "gauss_newton: bad edge split E_a = %lld",
                    (long long)a.E_a);
    }
    const size_t need = make_layout(a.mode, a.N, a.HW, a.E_total, a.E_local).total;
    M3S_REQUIRE(a.ws != nullptr && a.ws_bytes >= need,
                "gauss_newton: workspace too small (%zu < %zu bytes)", a.ws_bytes, need);
    return M3S_OK;
}

Plan& tls_plan() {
    static thread_local Plan p;
    return p;
}
SparsePlan& tls_sparse_plan() {
    static thread_local SparsePlan sp;
    return sp;
}

// ---- the lagged-factor PCG (gn_pcg.hip) ----
// From iteration `from` on, the step may be solved by CG preconditioned with the inverse of
// iteration (from - lag)'s system, which that iteration's direct factorisation provides
// (sp_inverse_kernel); the direct solve stays enqueued behind every PCG launch as its fallback and
// returns at once when the PCG converged.  Plans whose factor the inverse reads: elimination
// rounds by sp_round_kernel and a chol_df core (the hybrid with M3S_HYB_CORE=1, the multi plan);
// not the single-workgroup solve, the reference-order mode or the dense solver.
//   from (M3S_PCG_FROM, default by the core's size): 3 when the direct solve's dense core has >= 8
//     tile columns -- its factorisation chain (~14 us per column on one CU) is what the iteration
//     waits for, and M = A_1^-1 takes 4 CG steps (cfg4: solve 0.27 -> 0.09 ms); 4 below that --
//     the direct solve is short (cfg3, 4 columns: 0.116 ms) and the 8 direct launches behind a
//     PCG (its fallback, ~4-5 us each even when they return at once) leave room only for M =
//     A_2^-1's 4 steps (0.077 ms), not A_1^-1's 6 (0.094 ms: no net gain).
//   lag (M3S_PCG_LAG, default 2): with lag 1 the inverse (~0.75 ms alone on cfg4, ~2.7 ms beside an
//     accumulate that fills the chip: rocprofv3 trace r06_l) runs over one accumulate and the
//     first PCG waits ~0.7 ms for it; with lag 2 it has an accumulate, a direct solve and
//     another accumulate, and reads a copy of that iteration's factor (the next direct solve
//     overwrites the live one).  Refreshes after a PCG that fell back use lag 1 (the next PCG
//     waits for them).
namespace {
int pcg_from_for(int tiles) {
    const int v = env_int("M3S_PCG_FROM", 0);
    return v > 0 ? v : (tiles >= 8 ? 3 : 4);
}
int pcg_lag_for(int from) { return std::max(1, std::min(from, env_int("M3S_PCG_LAG", 2))); }
}  // namespace
// M3S_GN_PCG: 0 off; 1 (default) on every plan above whose core has >= M3S_PCG_MIN_TILES (1) tile
// columns; 2 always.
void choose_pcg(const m3s_gn_args& a, const Ctx& c, const Plan& plan, int npose, SparsePlan& sp) {
    sp.pcg = false;
    const int n = 7 * npose;
    const int mode = env_int("M3S_GN_PCG", 1);
    const int min_tiles = env_int("M3S_PCG_MIN_TILES", 1);
    const int tiles = sp.npad_tail / kCholTile;
    sp.pcg_from = pcg_from_for(tiles);
    sp.pcg_lag = pcg_lag_for(sp.pcg_from);
    if (mode == 0 || (mode == 1 && tiles < min_tiles) || c.ref_order || !sp.enabled || sp.fused ||
        (sp.hybrid && !sp.core_df) || a.max_iter <= sp.pcg_from || n > kPcgMaxN || n < 7)
        return;
    // rows of M per workgroup: 12 or 24, the smaller one giving <= M3S_PCG_WG
    // workgroups (default 64) -- or the largest whose f32 rows fit the LDS beside the vector and
    // the product's lists; never more than 240 workgroups (all resident at once, at most one per CU)
    const int wg_cap = std::max(1, env_int("M3S_PCG_WG", 64));
    // the most (row, block) items of a workgroup's rows: R rows span <= R / 7 + 2 poses
    std::vector<int> deg((size_t)npose, 1);
    for (const auto& pr : plan.pairs) {
        deg[pr.first]++;
        deg[pr.second]++;
    }
    const int maxdeg = npose > 0 ? *std::max_element(deg.begin(), deg.end()) : 1;
    auto items = [&](int R) { return 7 * maxdeg * (R / 7 + 2); };
    // (R = threads / 64 or threads / 32: a row's threads stay within one wave, a power of two)
    // M3S_PCG_ONEX (default 0: two exchanges per CG step) = 1: one exchange per step (B = M A's
    // rows in LDS beside M's) where they fit (cfg3's 889 unknowns: yes; cfg4's 1785: no)
    auto pick = [&](bool ox) {
        int R = kPcgThreads / 64;
        auto fits = [&](int r) { return pcg_lds_bytes(n, r, items(r), ox) <= (size_t)kPcgMaxLds && (!ox || r <= kPcgMaxR); };
        if ((n + R - 1) / R > wg_cap && fits(2 * R)) R *= 2;
        return (n + R - 1) / R > 240 || !fits(R) ? 0 : R;
    };
    bool onex = env_int("M3S_PCG_ONEX", 0) != 0 && pick(true) > 0;
    const int R = pick(onex);
    if (R == 0) return;
    if (inverse_lds_bytes(sp.npad_tail) > (size_t)kPcgMaxLds) return;  // M's core rows in LDS
    sp.pcg_nitem = items(R);
    sp.pcg = true;
    sp.pcg_R = R;
    sp.pcg_onex = onex;
    sp.pcg_nwg = (n + R - 1) / R;
    sp.pcg_ldx = (int)align_up((size_t)n, 16);
    sp.pcg_ldt = (int)align_up((size_t)n, 4);
    sp.pcg_nv = pcg_nv(n);
    // the matrix-vector product's lists: per pose its diagonal block, then its pair blocks
    sp.apt.assign((size_t)npose + 1, 0);
    for (const auto& pr : plan.pairs) {
        sp.apt[pr.first + 1]++;
        sp.apt[pr.second + 1]++;
    }
    for (int v = 0; v < npose; v++) sp.apt[v + 1] += sp.apt[v] + 1;
    sp.adj.assign(2 * (size_t)sp.apt[npose], 0);
    std::vector<int> fill(sp.apt.begin(), sp.apt.end() - 1);
    for (int v = 0; v < npose; v++) {
        sp.adj[2 * (size_t)fill[v]] = v;  // (the diagonal block's slot is the pose)
        sp.adj[2 * (size_t)fill[v] + 1] = v;
        fill[v]++;
    }
    for (size_t k = 0; k < plan.pairs.size(); k++) {
        const int x = plan.pairs[k].first, y = plan.pairs[k].second, slot = npose + (int)k;
        sp.adj[2 * (size_t)fill[x]] = slot;
        sp.adj[2 * (size_t)fill[x]++ + 1] = y;
        sp.adj[2 * (size_t)fill[y]] = slot;
        sp.adj[2 * (size_t)fill[y]++ + 1] = x;
    }
}

// The elimination plan the solve runs for this pose graph (M3S_SOLVER pins
// one).  Default: the hybrid (multi-launch rounds + gn_solve's back-substitution) when its core
// fits, else the multi-launch plan; the single-workgroup solve when the plan needs few rounds.
void choose_sparse_plan(const Plan& plan, int npose, SparsePlan& sp) {
    // M3S_SOLVER: 1 = single-workgroup (gn_solve), 2 = multi-launch, 0 (default) = the
    // single-workgroup solve when its plan needs few rounds, else multi-launch
    const int choice = env_int("M3S_SOLVER", 0);
    const int max_fused_rounds = env_int("M3S_FUSED_MAX_ROUNDS", 3);
    const bool hybrid_on = env_int("M3S_HYBRID", 1) != 0;
    // Default choice: the hybrid plan first.  The fused policy is the hybrid's plus a cap on
    // the poses per round (LDS staging), so it never needs fewer rounds; when the hybrid
    // plan already needs more than max_fused_rounds, the fused solve would be rejected and
    // building its plan (~0.23 ms of host time on cfg3, exposed once the per-call pack is
    // short, e.g. edge-sharded over several GPUs) is skipped.
    bool planned = false;
    if (choice == 0 && hybrid_on) {
        // the hybrid's rounds and core decided symbolically first (no lists): on a graph
        // whose core does not fit the in-register factorisation (cfg4) building the hybrid's
        // lists only to replace them by the multi plan cost ~1.5 ms of host time per call,
        // exposed once the edges are sharded (the first accumulate no longer covers it)
        static thread_local SparsePlan probe;
        build_sparse_plan(plan.pairs, plan.nblk, npose, hybrid_policy(), probe, true);
        if ((int)probe.rounds.size() > max_fused_rounds) {
            const bool hyb = hyb_core_fits(probe) && npose <= solve_max_poses() &&
                             solve_lds_bytes((int)probe.nints_back) <= (size_t)kSolveMaxLds;
            build_sparse_plan(plan.pairs, plan.nblk, npose, hyb ? hybrid_policy() : multi_policy(), sp);
            sp.hybrid = hyb;
            planned = true;
        }
    }
    bool fused_ok = false, meta_fits = false;
    if (!planned) {
        build_sparse_plan(plan.pairs, plan.nblk, npose, fused_policy(), sp);
        meta_fits = solve_lds_bytes((int)sp.nints) <= (size_t)kSolveMaxLds;
        fused_ok = sp.fused && meta_fits && npose <= solve_max_poses() &&
                   (choice == 1 || (choice == 0 && (int)sp.rounds.size() <= max_fused_rounds));
    }
    if (env_int("M3S_SOLVE_DEBUG", 0) && !fused_ok && !planned)
        fprintf(stderr, "fused solve rejected: fused_tail %d (ntail %d) rounds %zu nints %zu meta_fits %d\n",
                (int)sp.fused, sp.ntail, sp.rounds.size(), sp.nints, (int)meta_fits);
    if (!fused_ok && !planned) {
        // M3S_SOLVER=3 / default: multi-launch rounds + the in-register core when it fits
        bool hyb = false;
        if (choice == 3 || (choice == 0 && hybrid_on)) {
            build_sparse_plan(plan.pairs, plan.nblk, npose, hybrid_policy(), sp);
            hyb = hyb_core_fits(sp) && npose <= solve_max_poses() &&
                  solve_lds_bytes((int)sp.nints_back) <= (size_t)kSolveMaxLds;
        }
        if (!hyb) build_sparse_plan(plan.pairs, plan.nblk, npose, multi_policy(), sp);
        sp.hybrid = hyb;
    }
    sp.core_df = hyb_core_df();
}

// m3s_gn_plan_info (include/m3s_backend.h): the plan choose_sparse_plan makes, from host lists
int plan_info(const int64_t* ii, const int64_t* jj, int64_t E, int64_t N, int32_t* info, int32_t* order,
              int32_t* round_ptr, int32_t round_cap) {
    M3S_REQUIRE(info != nullptr && N >= 1 && E >= 0 && (E == 0 || (ii != nullptr && jj != nullptr)),
                "gn_plan_info: bad arguments");
    // the op's per-thread plan objects (no call is in flight on this thread here)
    Plan& plan = tls_plan();
    std::vector<int> iopt, jopt;
    int rc = plan_pairs(ii, jj, E, N, plan, iopt, jopt);
    if (rc) return rc;
    const int npose = (int)(N - 1);
    SparsePlan& sp = tls_sparse_plan();
    sp.reset();
    if (npose > 0) choose_sparse_plan(plan, npose, sp);
    info[0] = npose <= 0 ? -1 : sp.fused ? 0 : sp.hybrid ? 1 : 2;
    info[1] = (int32_t)sp.rounds.size();
    info[2] = (int32_t)sp.nodes.size();
    info[3] = sp.ntail;
    info[4] = sp.npad_tail;
    info[5] = (int32_t)plan.pairs.size();
    info[6] = (int32_t)sp.nints;
    info[7] = sp.npad_tail <= kMaxNpad ? 1 : 0;
    if (order) {
        std::copy(sp.nodes.begin(), sp.nodes.end(), order);
        std::copy(sp.tail.begin(), sp.tail.end(), order + sp.nodes.size());
    }
    if (round_ptr && round_cap >= (int32_t)sp.rounds.size() + 1) {
        for (size_t k = 0; k < sp.rounds.size(); k++) round_ptr[k] = sp.rounds[k].node_begin;
        round_ptr[sp.rounds.size()] = (int32_t)sp.nodes.size();
    }
    return M3S_OK;
}

}  // namespace m3s

// gn_api.hip -- the C ABI of the Gauss-Newton ops (include/m3s_backend.h) over the host driver
// (gn_host.h): the entries that replace gauss_newton_{points,rays,calib}_cuda (reference
// gn_kernels.cu:725-811, 1140-1228, 1546-1637), the thread's error string, the host-resource
// registry behind m3s_shutdown, the debug extraction of the per-edge Hessians and the assembled
// system (the reference's Hs/gs and SparseBlock::update_lhs/update_rhs, :71-113), and the bench
// profiling hooks (m3s_prof_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "gn_host.h"

namespace m3s {

namespace {
thread_local std::string g_err;
}  // namespace

// the last call's diagnostics (gn_host.h; written by run() under M3S_GN_DEBUG_FLAGS)
int g_dbg_flags[4] = {0, 0, 0, 0};
int g_dbg_pcg[5] = {0, 0, 0, 0, 0};
int g_dbg_pcg_plan[5] = {0, 0, 0, 0, 0};

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

const char* get_error() { return g_err.c_str(); }

namespace {
struct HostResources {
    std::mutex mu;
    std::vector<std::pair<void*, void (*)(void*)>> items;
    bool shut = false;
};
HostResources& host_resources() {
    static HostResources* r = new HostResources;  // never destroyed (used from atexit)
    return *r;
}
}  // namespace

void register_host_resource(void* obj, void (*release)(void*)) {
    HostResources& r = host_resources();
    std::lock_guard<std::mutex> lk(r.mu);
    r.items.emplace_back(obj, release);
}

// ---- profiling state (the m3s_prof_* hooks are at the end of the file) ----
hipEvent_t Prof::get() {
    if (pool.empty()) {
        // timing-only events: no system-scope release / acquire when recorded (a default
        // event record writes back and invalidates the caches -- idle GPU between the
        // kernels it separates); M3S_PROF_SYSFENCE=1: default events
        static const bool sysfence = env_int("M3S_PROF_SYSFENCE", 0) != 0;
        hipEvent_t e;
        if (sysfence || hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) {
            (void)hipGetLastError();
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
        }
        return e;
    }
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
}

void Prof::mark(hipStream_t st, bool accum, bool first_pack) {
    if (!on || (accum_only && !accum)) return;
    hipEvent_t e = get();
    if (e && hipEventRecord(e, st) == hipSuccess) {
        marks.push_back(e);
        if (accum_only && marks.size() % 2 == 0) first.push_back(first_pack);
    }
}

Prof g_prof;
namespace {
std::vector<double> g_prof_launch_ms;  // the last accumulate-only session: the iteration kernel's per-launch ms
std::vector<double> g_prof_solve_ms;   // the last phase session: each iteration's solve ms
}  // namespace

}  // namespace m3s

using namespace m3s;

extern "C" const char* m3s_last_error(void) { return m3s::get_error(); }

extern "C" int m3s_gn_check(void* stream) {
    const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        set_error("gn_check: %s", hipGetErrorString(e));
        return M3S_ERR_HIP;
    }
    return m3s::take_deferred_timeout("");
}

extern "C" void m3s_gn_debug_flags(int* out4) {
    for (int k = 0; k < 4; k++) out4[k] = m3s::g_dbg_flags[k];
}

extern "C" void m3s_gn_pcg_stats(int* out5) {
    for (int k = 0; k < 5; k++) out5[k] = m3s::g_dbg_pcg[k];
}

extern "C" void m3s_gn_pcg_plan(int* out5) {
    for (int k = 0; k < 5; k++) out5[k] = m3s::g_dbg_pcg_plan[k];
}

extern "C" const char* m3s_version(void) { return "m3s 0.1.0 gfx950"; }

extern "C" void m3s_shutdown(void) {
    HostResources& r = host_resources();
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.shut) return;
    r.shut = true;
    for (auto& it : r.items) it.second(it.first);
    r.items.clear();
}

namespace {
// Registered when the library is loaded: after the HIP runtime's own exit-time teardown (and a
// profiler's) was registered, so m3s_shutdown runs before them.
__attribute__((constructor)) void m3s_register_shutdown() { std::atexit(m3s_shutdown); }
}  // namespace

extern "C" size_t m3s_gn_workspace_bytes(int mode, int64_t N, int64_t HW, int64_t E_total,
                                         int64_t E_local) {
    if (N < 1 || HW < 1 || E_total < 0 || E_local < 0) return 0;
    return make_layout(mode, N, HW, E_total, E_local).total;
}

extern "C" int m3s_gn_plan_info(const int64_t* ii, const int64_t* jj, int64_t E, int64_t N, int32_t* info,
                                int32_t* order, int32_t* round_ptr, int32_t round_cap) {
    return m3s::plan_info(ii, jj, E, N, info, order, round_ptr, round_cap);
}

extern "C" int m3s_gauss_newton(const m3s_gn_args* args) {
    if (!args) {
        set_error("gauss_newton: null args");
        return M3S_ERR_INVALID;
    }
    return run(*args);
}

namespace {
// Reference-order per-edge records (kRefStride floats: D[7][7], g[7]) of ONE accumulate pass,
// copied to the host.
int ref_edge_records(const m3s_gn_args& a0, Ctx& c, std::vector<float>& rec) {
    m3s_gn_args a = a0;
    a.order = M3S_GN_ORDER_REFERENCE;
    int rc = setup(a, c);
    if (rc) return rc;
    rec.assign((size_t)a.E_local * kRefStride, 0.0f);
    if (a.E_local == 0) return M3S_OK;
    const Layout& L = c.L;
    M3S_HIP_CHECK(launch_accum_ref(a.mode, (int)a.E_local, c.st, a.Twc, a.Xs, a.Cs, c.at<int>(L.ii_loc),
                                   c.at<int>(L.jj_loc), c.es, c.R, c.at<float>(L.edgeblk),
                                   c.at<int>(L.flags)));
    M3S_HIP_CHECK(hipMemcpyAsync(rec.data(), c.at<float>(L.edgeblk), sizeof(float) * rec.size(),
                                 hipMemcpyDeviceToHost, c.st));
    M3S_HIP_CHECK(hipStreamSynchronize(c.st));
    return M3S_OK;
}

// The reference's four blocks of one edge from its record (see gn_refacc.hip):
// Hs[0] = Hs[3] = lower(D) mirrored, Hs[1] = -D^T, Hs[2] = -D.
double ref_block(const float* D, int blk, int r, int cc) {
    switch (blk) {
        case 0:
        case 3: return (double)D[std::max(r, cc) * 7 + std::min(r, cc)];
        case 1: return -(double)D[cc * 7 + r];
        default: return -(double)D[r * 7 + cc];
    }
}
}  // namespace

extern "C" int m3s_gn_edge_hessians(const m3s_gn_args* args, float* Hs_host, float* gs_host) {
    if (!args || !Hs_host || !gs_host) {
        set_error("gn_edge_hessians: null argument");
        return M3S_ERR_INVALID;
    }
    Ctx c;
    std::vector<float> rec;
    int rc = ref_edge_records(*args, c, rec);
    if (rc) return rc;
    const int64_t E = args->E_local;
    for (int64_t e = 0; e < E; e++) {
        const float* D = rec.data() + e * kRefStride;
        for (int blk = 0; blk < 4; blk++)
            for (int r = 0; r < 7; r++)
                for (int q = 0; q < 7; q++)
                    Hs_host[((blk * E + e) * 7 + r) * 7 + q] = (float)ref_block(D, blk, r, q);
        for (int q = 0; q < 7; q++) {
            gs_host[(0 * E + e) * 7 + q] = -D[49 + q];
            gs_host[(1 * E + e) * 7 + q] = D[49 + q];
        }
    }
    return M3S_OK;
}

extern "C" int m3s_gn_build_system(const m3s_gn_args* args, double* H_host, double* b_host) {
    if (!args) {
        set_error("gn_build_system: null args");
        return M3S_ERR_INVALID;
    }
    const m3s_gn_args& a = *args;
    if (gn_order(a) == M3S_GN_ORDER_REFERENCE) {
        // the full (not exactly symmetric) matrix SparseBlock::update_lhs/update_rhs builds
        // from the reference-order Hs/gs (gn_kernels.cu:71-113)
        Ctx c;
        std::vector<float> rec;
        int rc = ref_edge_records(a, c, rec);
        if (rc) return rc;
        const int64_t n = 7 * (a.N - 1);
        std::fill(H_host, H_host + n * n, 0.0);
        std::fill(b_host, b_host + n, 0.0);
        for (int64_t el = 0; el < a.E_local; el++) {
            const float* D = rec.data() + el * kRefStride;
            const int i = c.plan.ii_loc[el] - 1, j = c.plan.jj_loc[el] - 1;
            const int rr[4] = {i, i, j, j}, cc[4] = {i, j, i, j};
            for (int blk = 0; blk < 4; blk++) {
                if (rr[blk] < 0 || cc[blk] < 0) continue;
                for (int r = 0; r < 7; r++)
                    for (int q = 0; q < 7; q++)
                        H_host[(7 * rr[blk] + r) * n + 7 * cc[blk] + q] += ref_block(D, blk, r, q);
            }
            for (int q = 0; q < 7; q++) {
                if (i >= 0) b_host[7 * i + q] -= (double)D[49 + q];
                if (j >= 0) b_host[7 * j + q] += (double)D[49 + q];
            }
        }
        return M3S_OK;
    }
    Ctx c;
    c.need_slotmap = true;
    int rc = setup(a, c);
    if (rc) return rc;
    const int npose = (int)(a.N - 1);
    const int n = 7 * npose;
    if (npose <= 0) return M3S_OK;
    rc = prepare_iterations(a, c);
    if (rc) return rc;
    rc = enqueue_system(a, c);
    if (rc) return rc;
    const Layout& L = c.L;
    M3S_HIP_CHECK(launch_fill_only(c.st, c.at<double>(L.compact), c.dyn_at<int>(c.o_slot), c.plan.nblk,
                                   npose, n, L.npad, c.dyn_at<double>(c.o_dense), c.at<int>(L.flags)));
    M3S_HIP_CHECK(hipMemcpy2DAsync(H_host, sizeof(double) * n, c.dyn_at<double>(c.o_dense),
                                   sizeof(double) * L.npad, sizeof(double) * n, n,
                                   hipMemcpyDeviceToHost, c.st));
    M3S_HIP_CHECK(hipMemcpyAsync(b_host, c.dyn_at<double>(c.o_dense) + (size_t)L.npad * L.npad,
                                 sizeof(double) * n, hipMemcpyDeviceToHost, c.st));
    M3S_HIP_CHECK(hipStreamSynchronize(c.st));
    return M3S_OK;
}

namespace {
m3s_gn_args base_args(int mode, float* Twc, const float* Xs, const float* Cs, const int64_t* ii,
                      const int64_t* jj, const int64_t* idx, const uint8_t* valid, const float* Q,
                      int64_t N, int64_t HW, int64_t E, int max_iter, float delta_thresh,
                      float* dx, void* ws, size_t ws_bytes, void* stream) {
    m3s_gn_args a;
    std::memset(&a, 0, sizeof(a));
    a.mode = mode;
    a.Twc = Twc; a.Xs = Xs; a.Cs = Cs; a.ii = ii; a.jj = jj;
    a.idx = idx; a.valid = valid; a.Q = Q;
    a.N = N; a.HW = HW; a.E_total = E; a.E_local = E; a.edge_offset = 0;
    a.max_iter = max_iter; a.delta_thresh = delta_thresh;
    a.dx = dx; a.ws = ws; a.ws_bytes = ws_bytes; a.stream = stream;
    return a;
}
}  // namespace

extern "C" int m3s_gauss_newton_points(float* Twc, const float* Xs, const float* Cs,
                                       const int64_t* ii, const int64_t* jj, const int64_t* idx,
                                       const uint8_t* valid, const float* Q, int64_t N, int64_t HW,
                                       int64_t E, float sigma_point, float C_thresh,
                                       float Q_thresh, int max_iter, float delta_thresh,
                                       float* dx, void* ws, size_t ws_bytes, void* stream) {
    m3s_gn_args a = base_args(M3S_GN_POINTS, Twc, Xs, Cs, ii, jj, idx, valid, Q, N, HW, E,
                              max_iter, delta_thresh, dx, ws, ws_bytes, stream);
    a.sigma0 = sigma_point;
    a.C_thresh = C_thresh;
    a.Q_thresh = Q_thresh;
    return run(a);
}

extern "C" int m3s_gauss_newton_rays(float* Twc, const float* Xs, const float* Cs,
                                     const int64_t* ii, const int64_t* jj, const int64_t* idx,
                                     const uint8_t* valid, const float* Q, int64_t N, int64_t HW,
                                     int64_t E, float sigma_ray, float sigma_dist, float C_thresh,
                                     float Q_thresh, int max_iter, float delta_thresh, float* dx,
                                     void* ws, size_t ws_bytes, void* stream) {
    m3s_gn_args a = base_args(M3S_GN_RAYS, Twc, Xs, Cs, ii, jj, idx, valid, Q, N, HW, E, max_iter,
                              delta_thresh, dx, ws, ws_bytes, stream);
    a.sigma0 = sigma_ray;
    a.sigma1 = sigma_dist;
    a.C_thresh = C_thresh;
    a.Q_thresh = Q_thresh;
    return run(a);
}

extern "C" int m3s_gauss_newton_calib(float* Twc, const float* Xs, const float* Cs, const float* K,
                                      const int64_t* ii, const int64_t* jj, const int64_t* idx,
                                      const uint8_t* valid, const float* Q, int64_t N, int64_t HW,
                                      int64_t E, int height, int width, int pixel_border,
                                      float z_eps, float sigma_pixel, float sigma_depth,
                                      float C_thresh, float Q_thresh, int max_iter,
                                      float delta_thresh, float* dx, void* ws, size_t ws_bytes,
                                      void* stream) {
    m3s_gn_args a = base_args(M3S_GN_CALIB, Twc, Xs, Cs, ii, jj, idx, valid, Q, N, HW, E,
                              max_iter, delta_thresh, dx, ws, ws_bytes, stream);
    a.K = K;
    a.height = height;
    a.width = width;
    a.pixel_border = pixel_border;
    a.z_eps = z_eps;
    a.sigma0 = sigma_pixel;
    a.sigma1 = sigma_depth;
    a.C_thresh = C_thresh;
    a.Q_thresh = Q_thresh;
    return run(a);
}

// ---- profiling (bench.py): phase times from HIP events on the GN stream ----
extern "C" int m3s_prof_begin(void) {
    for (hipEvent_t e : g_prof.marks) g_prof.pool.push_back(e);
    g_prof.marks.clear();
    g_prof.first.clear();
    g_prof.accum_only = false;
    g_prof.on = true;
    return M3S_OK;
}

extern "C" int m3s_prof_begin_accum(void) {
    int rc = m3s_prof_begin();
    g_prof.accum_only = true;
    return rc;
}

// out[0] accumulate-kernel ms, out[1] edge-reduce/compact/all-reduce ms, out[2] solve ms,
// out[3] retract ms (sums over iterations); *n_iter = iterations recorded.
extern "C" int m3s_prof_end(double* out, int* n_iter) {
    g_prof.on = false;
    double acc[4] = {0, 0, 0, 0};
    int n = 0;
    if (g_prof.accum_only) {  // a0 a1 per iteration
        // out[0] / *n_iter: the iteration kernel (records already packed); out[1] / out[2]: the
        // launches that built the records themselves (a call's first, M3S_GN_PACK_FIRST) and
        // their count
        g_prof.accum_only = false;
        g_prof_launch_ms.clear();
        for (size_t k = 0; k + 2 <= g_prof.marks.size(); k += 2) {
            float ms = 0.f;
            M3S_HIP_CHECK(hipEventSynchronize(g_prof.marks[k + 1]));
            M3S_HIP_CHECK(hipEventElapsedTime(&ms, g_prof.marks[k], g_prof.marks[k + 1]));
            if (k / 2 < g_prof.first.size() && g_prof.first[k / 2]) {
                acc[1] += ms;
                acc[2] += 1;
            } else {
                acc[0] += ms;
                n++;
                g_prof_launch_ms.push_back(ms);
            }
        }
        for (int q = 0; q < 4; q++) out[q] = acc[q];
        *n_iter = n;
        for (hipEvent_t e : g_prof.marks) g_prof.pool.push_back(e);
        g_prof.marks.clear();
        return M3S_OK;
    }
    const size_t per = 6;  // t0 [a0 a1] t1 t2 t3 (a0/a1 bracket the accumulate kernel)
    g_prof_solve_ms.clear();
    for (size_t k = 0; k + per <= g_prof.marks.size(); k += per) {
        hipEvent_t* m = &g_prof.marks[k];
        float ms[5];
        for (int q = 0; q < 5; q++) {
            M3S_HIP_CHECK(hipEventSynchronize(m[q + 1]));
            M3S_HIP_CHECK(hipEventElapsedTime(&ms[q], m[q], m[q + 1]));
        }
        acc[0] += ms[1];
        acc[1] += ms[0] + ms[2];
        acc[2] += ms[3];
        acc[3] += ms[4];
        g_prof_solve_ms.push_back(ms[3]);
        n++;
    }
    for (int q = 0; q < 4; q++) out[q] = acc[q];
    *n_iter = n;
    for (hipEvent_t e : g_prof.marks) g_prof.pool.push_back(e);
    g_prof.marks.clear();
    return M3S_OK;
}

// the per-launch durations (ms) of the iteration kernel from the last m3s_prof_begin_accum ..
// m3s_prof_end session (bench.py: the spread of the accumulate over the timed steps); returns the
// number of launches recorded, copies at most cap of them
extern "C" int m3s_prof_launch_ms(double* out, int cap) {
    const int n = (int)g_prof_launch_ms.size();
    for (int k = 0; k < n && k < cap; k++) out[k] = g_prof_launch_ms[k];
    return n;
}

// each iteration's solve ms from the last m3s_prof_begin .. m3s_prof_end session (bench.py: the
// direct iterations apart from the PCG ones); returns the count, copies at most cap
extern "C" int m3s_prof_solve_ms(double* out, int cap) {
    const int n = (int)g_prof_solve_ms.size();
    for (int k = 0; k < n && k < cap; k++) out[k] = g_prof_solve_ms[k];
    return n;
}

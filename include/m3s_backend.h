/*
 * m3s_backend.h -- C ABI of the MI355X-native MASt3R-SLAM backend
 * (dense iterative-projection matching + Sim3 Gauss-Newton).
 *
 * This is the drop-in boundary that the Python module `mast3r_slam_backends`
 * (mast3r-slam_amd/mast3r_slam_backends) binds with ctypes.  Each entry point
 * replaces one pybind11 op of the reference module
 * (/root/reference/mast3r_slam/backend/src/gn.cpp:116-123; prototypes gn.h:22-117).
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer to contiguous memory (torch.Tensor.data_ptr()).
 *     bool tensors are passed as uint8_t (0/1), fp16 as uint16_t bit patterns.
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); all work
 *     is enqueued on it.  Matching ops are fully asynchronous.  The GN ops perform
 *     one host synchronisation per call (to plan the sparse system from ii/jj),
 *     then enqueue all iterations without further host round trips.
 *   - Return value: M3S_OK (0) or an error code; m3s_last_error() gives a
 *     thread-local message.  The Python layer raises RuntimeError with it, as the
 *     reference's TORCH_CHECK does.
 */
#ifndef M3S_BACKEND_H
#define M3S_BACKEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    M3S_OK = 0,
    M3S_ERR_INVALID = 1, /* bad shape / argument */
    M3S_ERR_HIP = 2,     /* HIP runtime error */
    M3S_ERR_WORKSPACE = 3,
    M3S_ERR_COMM = 4,
    M3S_ERR_TIMEOUT = 5  /* a bounded device-side wait (dataflow factorisation / grid barrier)
                            gave up: the solve's result was discarded -- not a singular system */
};

const char* m3s_last_error(void);
/* Library build identifier ("m3s <version> gfx950"). */
const char* m3s_version(void);
/* Releases the library's cached host resources (pinned staging buffers, events).  Registered
 * with atexit when the library is loaded (and called by the Python module's atexit hook), so no
 * HIP call runs from a static or thread-local destructor during exit().  Idempotent; no other
 * entry point may be called afterwards. */
void m3s_shutdown(void);

/*
 * FMA-contraction convention of the reference build's float arithmetic.  The reference is built
 * by nvcc -O3 (setup.py:29-37: --fmad=true), which fuses a multiply into the add that consumes it;
 * for `a*b + c*d` the left product is fused (LLVM / NVPTX combine order).  The parity paths
 * (iter_proj, refine_matches f32/f64, the reference-order GN accumulate and the retraction)
 * restate that explicitly (mast3r-slam_amd/csrc/contract.h); OFF and NVCC_RIGHT are variants for
 * measuring the convention's effect.
 */
enum {
    M3S_CONTRACT_NVCC = 0,       /* nvcc --fmad=true, left product of a two-product sum fused */
    M3S_CONTRACT_OFF = 1,        /* IEEE multiply, then add (no fusion) */
    M3S_CONTRACT_NVCC_RIGHT = 2, /* the same as NVCC, right product fused */
    M3S_CONTRACT_DEFAULT = M3S_CONTRACT_NVCC  /* 0: a zero-initialised argument is the default */
};

/*
 * iter_proj -- replaces iter_proj (gn.cpp:84-99 -> matching_kernels.cu:279-316).
 *   rays      [B,H,W,9] f32  (ray, d/du, d/dv), H,W >= 3
 *   pts       [B,N,3]   f32  normalised target rays
 *   p_init    [B,N,2]   f32  initial (u,v) in image 1
 *   p_new     [B,N,2]   f32  out
 *   converged [B,N]     u8   out
 */
int m3s_iter_proj(const float* rays, const float* pts, const float* p_init,
                  float* p_new, uint8_t* converged,
                  int64_t B, int64_t H, int64_t W, int64_t N,
                  int max_iter, float lambda_init, float cost_thresh, void* stream);
/* The same with an explicit contraction convention (M3S_CONTRACT_*); m3s_iter_proj uses
 * M3S_CONTRACT_DEFAULT. */
int m3s_iter_proj_ex(const float* rays, const float* pts, const float* p_init,
                     float* p_new, uint8_t* converged,
                     int64_t B, int64_t H, int64_t W, int64_t N,
                     int max_iter, float lambda_init, float cost_thresh, int contract, void* stream);

/*
 * refine_matches -- replaces refine_matches (gn.cpp:101-114 -> matching_kernels.cu:84-116).
 *   D11 [B,H,W,F], D21 [B,N,F]  (fp16 bit patterns, f32 or f64: the reference's
 *   AT_DISPATCH_FLOATING_TYPES_AND_HALF, matching_kernels.cu:103)
 *   p1  [B,N,2] i64 (u,v) -> p1_new [B,N,2] i64
 */
int m3s_refine_matches_f16(const uint16_t* D11, const uint16_t* D21,
                           const int64_t* p1, int64_t* p1_new,
                           int64_t B, int64_t H, int64_t W, int64_t N, int64_t F,
                           int radius, int dilation_max, void* stream);
int m3s_refine_matches_f32(const float* D11, const float* D21,
                           const int64_t* p1, int64_t* p1_new,
                           int64_t B, int64_t H, int64_t W, int64_t N, int64_t F,
                           int radius, int dilation_max, void* stream);
int m3s_refine_matches_f64(const double* D11, const double* D21,
                           const int64_t* p1, int64_t* p1_new,
                           int64_t B, int64_t H, int64_t W, int64_t N, int64_t F,
                           int radius, int dilation_max, void* stream);

/*
 * match_iterative_proj -- the whole matching pipeline of the reference's Python caller
 * (matching.py:52-90: prep_for_iter_proj, iter_proj, p.long(), the occlusion test, refine on
 * .half() descriptors, pixel_to_lin) in five launches.  `contract`: iter_proj's M3S_CONTRACT_*.
 *   X11, X21  [B,H,W,3] f32      D11, D21 [B,H,W,F] f32
 *   idx_init  [B,H*W]   i64 or NULL (identity start)
 *   idx_out   [B,H*W]   i64 out  (u + W v)      valid_out [B,H*W] u8 out (bool)
 *   ws        device workspace of >= m3s_match_workspace_bytes(B, H, W, F) bytes
 */
size_t m3s_match_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t F);
int m3s_match_iterative_proj(const float* X11, const float* X21, const float* D11, const float* D21,
                             const int64_t* idx_init, int64_t B, int64_t H, int64_t W, int64_t F,
                             int max_iter, float lambda_init, float cost_thresh, float dist_thresh,
                             int radius, int dilation_max, int contract, int64_t* idx_out,
                             uint8_t* valid_out, void* ws, size_t ws_bytes, void* stream);

/* The measured-slower refine_matches variants (LDS tile, MFMA correlation, dot2) are not part of
 * this boundary: include/m3s_variants.h, lib/libm3s_variants.so. */

/* ---------------- Gauss-Newton ---------------- */

/* Diagnostics: with env M3S_GN_DEBUG_FLAGS set (2: silently), a GN call reads back its device
 * flags at the end (one extra synchronisation); out4 = {early exit, pivot failure (in any
 * iteration), packed stream, ray-constrained calib accumulate (Xj read as its depth)} of the last
 * such call. */
void m3s_gn_debug_flags(int* out4);
/* The same call's lagged-factor PCG: out5 = {PCG solves, their CG steps in all,
 * PCG solves that fell back to the direct factorisation, 1 if the call planned PCG iterations,
 * the first PCG iteration (0 if none planned)}. */
void m3s_gn_pcg_stats(int* out5);
/* The same call's PCG plan (host plan fields, no synchronisation of their own): out5 = {rows of M
 * per workgroup (12 or 24), workgroups, 1 if B = M A is staged for one exchange per CG step
 * (M3S_PCG_ONEX), the lag of M behind the first PCG iteration, the LDS item capacity of a
 * workgroup's rows of A}; all 0 when the call planned no PCG. */
void m3s_gn_pcg_plan(int* out5);

/* Deferred error report.  A GN call whose solver has bounded device-side waits (the dataflow
 * factorisation) exports its timeout flag without a host wait.  A call whose wait timed out
 * restores Twc to the poses it started from on the device (its result is discarded; every rank of
 * a sharded call restores), so it never commits poses.  M3S_ERR_TIMEOUT for it is returned by this
 * function, which synchronises `stream` (hipStream_t) first, or else by the next
 * m3s_gauss_newton_* call on the same host thread: that call checks the flag once its per-call
 * setup has synchronised the stream -- after the setup's own work (the edge-range exchange of a
 * sharded call, the plan uploads, the workspace allocation), before its first GN iteration -- and
 * returns without running an iteration.  m3s_gn_build_system and m3s_gn_edge_hessians do not
 * check it.  Env M3S_GN_TIMEOUT_SYNC=1 reports it from the call itself.  Returns M3S_OK,
 * M3S_ERR_TIMEOUT (then cleared) or M3S_ERR_HIP. */
int m3s_gn_check(void* stream);

enum { M3S_GN_POINTS = 0, M3S_GN_RAYS = 1, M3S_GN_CALIB = 2 };

/*
 * Common arguments of gauss_newton_{points,rays,calib} (gn.h:22-117).
 *   Twc   [N,8]  f32  poses [t(3), q(4, xyzw), s], UPDATED IN PLACE (pose 0 pinned)
 *   Xs    [N,HW,3] f32, Cs [N,HW] f32 (rows ordered by sorted unique keyframe id)
 *   ii,jj [E_total] i64 GLOBAL keyframe ids of the directed edges
 *   idx   [E_local,HW] i64, valid [E_local,HW] u8, Q [E_local,HW] f32 for the
 *         directed edges edge_offset .. edge_offset+E_local-1 (single GPU:
 *         edge_offset = 0, E_local = E_total)
 *   dx    [N-1,7] f32 out: the last iteration's update (the op's return value)
 *   ws    device workspace of >= m3s_gn_workspace_bytes(...) bytes
 *   comm  NULL, or an m3s communicator: the per-iteration compact Hessian is
 *         summed over ranks (RCCL all-reduce) before the replicated solve.
 */
typedef struct m3s_gn_args {
    int mode;
    float* Twc;
    const float* Xs;
    const float* Cs;
    const int64_t* ii;
    const int64_t* jj;
    const int64_t* idx;
    const uint8_t* valid;
    const float* Q;
    int64_t N, HW, E_total, E_local, edge_offset;
    /* residual parameters */
    float sigma0;           /* sigma_point | sigma_ray | sigma_pixel */
    float sigma1;           /* -           | sigma_dist | sigma_depth */
    float C_thresh, Q_thresh;
    const float* K;         /* calib: device [3,3] f32; fx,fy,cx,cy = K[0][0],K[1][1],K[0][2],K[1][2] */
    int height, width, pixel_border;
    float z_eps;
    int max_iter;
    float delta_thresh;
    float* dx;
    void* ws;
    size_t ws_bytes;
    void* comm;
    void* stream;
    /* summation order of the per-edge normal equations (M3S_GN_ORDER_*); 0 = the
     * default, overridable by the environment variable M3S_GN_ORDER=reference|fast */
    int order;
    /* Optional second half of the local edges' idx / valid / Q (NULL = one contiguous
     * tensor, the reference's layout): local directed edges 0 .. E_a-1 are rows of idx / valid
     * / Q, edges E_a .. E_local-1 are rows 0 .. E_local-E_a-1 of idx_b / valid_b / Q_b.  A
     * two-way edge store (forward edges, then the same pairs backward) is passed as its two
     * halves instead of the per-call concatenation of prep_two_way_edges
     * (global_opt.py:104-110). */
    const int64_t* idx_b;
    const uint8_t* valid_b;
    const float* Q_b;
    int64_t E_a;
    /* FMA-contraction convention (M3S_CONTRACT_*; 0 = the reference build's) of the
     * reference-order accumulate and of the retraction (the fast path's reformulated sums have
     * none to follow) */
    int contract;
} m3s_gn_args;
enum {
    M3S_GN_ORDER_DEFAULT = 0,
    /* packed stream, pre-adjoint rows, f32 lane chains of <= 32 points + f64 chunk sums
     * (gn_accum.hip): the fast path */
    M3S_GN_ORDER_FAST = 1,
    /* the reference kernels' own order and formulas (gn_refacc.hip): one 256-thread
     * workgroup per edge, 768-long fp32 chains per thread, blockReduce tree, per-point
     * apply_Sim3_adj_inv; the system read from its lower triangle like SimplicialLLT */
    M3S_GN_ORDER_REFERENCE = 2
};

size_t m3s_gn_workspace_bytes(int mode, int64_t N, int64_t HW, int64_t E_total, int64_t E_local);

/* Generic entry: replaces gauss_newton_{points,rays,calib}_cuda
 * (gn_kernels.cu:725-811, 1140-1228, 1546-1637). */
int m3s_gauss_newton(const m3s_gn_args* args);

/* Thin positional wrappers with the reference's argument order (gn.h). */
int m3s_gauss_newton_points(float* Twc, const float* Xs, const float* Cs,
                            const int64_t* ii, const int64_t* jj, const int64_t* idx,
                            const uint8_t* valid, const float* Q,
                            int64_t N, int64_t HW, int64_t E,
                            float sigma_point, float C_thresh, float Q_thresh,
                            int max_iter, float delta_thresh,
                            float* dx, void* ws, size_t ws_bytes, void* stream);
int m3s_gauss_newton_rays(float* Twc, const float* Xs, const float* Cs,
                          const int64_t* ii, const int64_t* jj, const int64_t* idx,
                          const uint8_t* valid, const float* Q,
                          int64_t N, int64_t HW, int64_t E,
                          float sigma_ray, float sigma_dist, float C_thresh, float Q_thresh,
                          int max_iter, float delta_thresh,
                          float* dx, void* ws, size_t ws_bytes, void* stream);
int m3s_gauss_newton_calib(float* Twc, const float* Xs, const float* Cs, const float* K,
                           const int64_t* ii, const int64_t* jj, const int64_t* idx,
                           const uint8_t* valid, const float* Q,
                           int64_t N, int64_t HW, int64_t E,
                           int height, int width, int pixel_border, float z_eps,
                           float sigma_pixel, float sigma_depth, float C_thresh, float Q_thresh,
                           int max_iter, float delta_thresh,
                           float* dx, void* ws, size_t ws_bytes, void* stream);

/*
 * Debug / test entry: run ONE accumulate + assemble pass with the current Twc and
 * write the dense normal equations H [n,n] and b [n] (n = 7(N-1), f64, host
 * pointers), i.e. the system SparseBlock builds (gn_kernels.cu:71-113).
 */
int m3s_gn_build_system(const m3s_gn_args* args, double* H_host, double* b_host);
/*
 * Debug / test entry: ONE reference-order accumulate pass (gn_refacc.hip) with the current
 * Twc, returning exactly the tensors the reference's align kernels write
 * (gn_kernels.cu:1096-1137): Hs [4, E_local, 7, 7] f32 and gs [2, E_local, 7] f32 (host).
 */
int m3s_gn_edge_hessians(const m3s_gn_args* args, float* Hs_host, float* gs_host);

/*
 * Diagnostic (host only, no GPU): the elimination plan m3s_gauss_newton would build for this
 * pose graph -- the step the reference leaves to Eigen's SimplicialLLT symbolic analysis on every
 * solve (gn_kernels.cu:132-153).  ii, jj [E] host i64 global keyframe ids (as the op's), N
 * poses (the first pinned).  info[8]: [0] solver (0 single-workgroup fused, 1 hybrid, 2
 * multi-launch, -1 nothing to solve), [1] elimination rounds, [2] poses eliminated by the
 * rounds, [3] poses in the dense core, [4] the core's padded unknowns, [5] pose pairs (graph
 * blocks off the diagonal), [6] plan integers uploaded per call, [7] 1 if the core fits the
 * dense solve limit.  order (optional, N-1 ints): the poses (0-based rows after the pinned one)
 * round by round, each round ascending, then the core's.  round_ptr (optional, round_cap ints):
 * where each round starts in order, then the core's start -- written when round_cap >=
 * rounds + 1.  Environment knobs as for the op.
 */
int m3s_gn_plan_info(const int64_t* ii, const int64_t* jj, int64_t E, int64_t N, int32_t* info,
                     int32_t* order, int32_t* round_ptr, int32_t round_cap);

/*
 * Phase timing (bench.py): between m3s_prof_begin() and m3s_prof_end() every GN
 * iteration records HIP events on its stream.  out[0] = accumulate kernel ms,
 * out[1] = edge reduce + compact (+ all-reduce) ms, out[2] = solve ms, out[3] = retract
 * ms, summed over the *n_iter recorded iterations.  Not thread-safe; test/bench only.
 */
int m3s_prof_begin(void);
/* The same, recording only the two events around each accumulate launch (every timed event
 * record idles the GPU ~5 us): m3s_prof_end then fills out[0] and *n_iter with the iteration
 * kernel's launches, out[1] / out[2] with the ms and count of the launches that also built the
 * packed records (a calib call's first accumulate, M3S_GN_PACK_FIRST), out[3] = 0. */
int m3s_prof_begin_accum(void);
int m3s_prof_end(double* out /* [4] */, int* n_iter);
/* After an m3s_prof_begin_accum() .. m3s_prof_end() session: the iteration kernel's per-launch
 * ms (out[0 .. min(n, cap) - 1]); returns n, the number of launches recorded (bench.py reports
 * their min / median / max: the accumulate's spread within one run). */
int m3s_prof_launch_ms(double* out, int cap);
/* After an m3s_prof_begin() .. m3s_prof_end() session: each recorded iteration's solve ms
 * (out[0 .. min(n, cap) - 1], call after call); returns n. */
int m3s_prof_solve_ms(double* out, int cap);

/* ---------------- frame tracking (single-pair Sim3 GN) ---------------- */

/*
 * track_sim3 -- replaces the torch loop of FrameTracker.opt_pose_ray_dist_sim3 /
 * opt_pose_calib_sim3 (/root/reference/mast3r_slam/tracker.py:173-266) with its solve
 * (:156-171), huber (nonlinear_optimizer.py:28-33), check_convergence (:5-25) and the
 * residual models point_to_ray_dist / act_Sim3 / project_calib (geometry.py:17-104).
 * The reference has no native op for this (it is torch + lietorch); this entry is an
 * extension of the drop-in module (mast3r_slam_backends.track_sim3).
 *   mode      M3S_GN_RAYS (ray + distance residual, 4 rows) or M3S_GN_CALIB (pixel +
 *             log-depth, 3 rows)
 *   Xf        [HW,3] f32  frame points already gathered by the match (Xf[idx_f2k])
 *   Xk        [HW,3] f32  keyframe points (rays mode; unused by calib)
 *   Qk        [HW]   f32  match confidence sqrt(Qff[idx] * Qkf)
 *   valid     [HW]   u8   valid_opt
 *   meas_k    [HW,3] f32  calib: (u, v, log z) of the keyframe pixel (0 where invalid)
 *   valid_meas[HW]   u8   calib: z_k > depth_eps
 *   K         [3,3]  f32  calib intrinsics (device)
 *   T_WCf, T_WCk [8] f32  lietorch Sim3 data (t, q xyzw, s) (device)
 *   T_WCf_out, T_CkCf_out [8] f32 (device, out)
 *   info      [4] i32 (device, out): iterations run, converged, cholesky failed, 0
 *   cost      [1] f64 (device, out): cost of the last linearisation
 * The python-float parameters (sigmas, huber k, thresholds) are passed as double and
 * rounded where torch rounds them.  One host synchronisation per `check_every`
 * iterations (the reference syncs on every iteration's `.item()`).  A non-positive (or
 * NaN) Cholesky pivot stops the loop and sets info[2] -- the caller raises, as
 * torch.linalg.cholesky does (tracker.py:91).
 */
typedef struct m3s_track_args {
    int mode;
    const float* Xf;
    const float* Xk;
    const float* Qk;
    const uint8_t* valid;
    const float* meas_k;
    const uint8_t* valid_meas;
    const float* K;
    const float* T_WCf;
    const float* T_WCk;
    int64_t HW;
    int height, width, pixel_border;
    double z_eps;
    double sigma0;          /* sigma_ray   | sigma_pixel */
    double sigma1;          /* sigma_dist  | sigma_depth */
    double huber_k;
    int max_iters;
    double rel_error, delta_norm;
    int check_every;        /* iterations between host checks of the convergence flag */
    float* T_WCf_out;
    float* T_CkCf_out;
    int* info;
    double* cost;
    void* ws;
    size_t ws_bytes;
    void* stream;
} m3s_track_args;

size_t m3s_track_workspace_bytes(int64_t HW);
/* Where m3s_track_sim3 keeps its per-workgroup partial sums inside the workspace (host only, no
 * device call): *partials_offset = byte offset of a value-major [36][*ld] f32 table of which
 * columns 0 .. *nblk - 1 are written (one per workgroup; the padding columns are never written
 * nor summed).  Rows: H's upper triangle row-major (28), g (7), sum of b^2 (1).  After a call the
 * table holds the last live iteration's partials.  M3S_ERR_INVALID (nothing written) for a null pointer or an HW
 * that m3s_track_sim3 rejects (HW < 1, HW >= 2^31). */
int m3s_track_workspace_layout(int64_t HW, size_t* partials_offset, int* nblk, int* ld);
int m3s_track_sim3(const m3s_track_args* args);
/* The last m3s_track_sim3 call's result on this host thread, on the host: info4 = {iterations,
 * converged, cholesky failed, 0}, *cost (the same values as the call's device `info` / `cost`).
 * Free of a device round trip when the call returned on a host check that saw its done flag
 * (converged before max_iters); otherwise it synchronises the call's stream once.  That call's
 * workspace must still be allocated at the first read after the call, which drops the reference
 * to it: later reads (same thread, no new call) return the same host copy without touching device
 * memory.  Per host thread: another thread's calls are not seen.  Extension (the reference's
 * tracker reads them with .item()). */
int m3s_track_last_result(int32_t* info4, double* cost);

/* ---------------- edge construction after matching ---------------- */

/*
 * edge_confidence -- the per-pixel glue of FactorGraph.add_factors (global_opt.py:53-67) in one
 * pass over B keyframe pairs:
 *   Qj = sqrt(Qii[b, idx_i2j] * Qji), Qi = sqrt(Qjj[b, idx_j2i] * Qij)     [B,HW] f32 out
 *   counts[b] = (#(valid_match_j & Qj > Q_conf), #(valid_match_i & Qi > Q_conf))  [B,2] i32 out
 *   idx_* [B,HW] i64, valid_match_* [B,HW] u8, Q* [B,HW] f32.  Bit-exact (same f32 ops: the
 *   product, a correctly rounded sqrt, an f32 compare; a NaN Q is not counted).
 * An index outside [0, HW-1] is clamped to 0 or HW-1 of the pair's own row (the reference would
 * read out of range): nothing outside Qii[b] / Qjj[b] is read.  counts is zeroed by every call;
 * B == 0 returns at once, HW == 0 zeroes counts and needs no other pointer.
 */
int m3s_edge_confidence(const int64_t* idx_i2j, const int64_t* idx_j2i,
                        const uint8_t* valid_match_j, const uint8_t* valid_match_i,
                        const float* Qii, const float* Qjj, const float* Qji, const float* Qij,
                        float Q_conf, int64_t B, int64_t HW, float* Qj, float* Qi, int* counts,
                        void* stream);

/* ---------------- keyframe point-map fusion ---------------- */

enum { M3S_FILTER_WEIGHTED_POINTMAP = 0, M3S_FILTER_INDEP_CONF = 1, M3S_FILTER_RECENT = 2 };

/*
 * pointmap_update -- replaces Frame.update_pointmap (frame.py:41-105) for the per-point
 * filtering modes (weighted_pointmap :74-77, indep_conf :69-73, recent :58-61), fused with
 * the transform of the new observation the tracker applies first (tracker.py:98-99).
 *   T      [8] f32 Sim3 data applied to X_new (lietorch act), or NULL for none
 *   X_new  [HW,3], C_new [HW] f32; X [HW,3], C [HW] f32 updated in place
 * The update is bit-exact against the torch expressions on the same (transformed) inputs: every
 * product, sum and quotient rounded to f32, the divide correctly rounded, subnormals kept;
 * indep_conf replaces where C_new > C strictly (a NaN replaces nothing).  The transform is
 * act_so3 (the rotation, at the default contraction convention M3S_CONTRACT_NVCC: its sums of
 * products fused) followed by an unfused s * r + t; it is within 8 * 2^-24 * (5 |s| |p| + max|t|)
 * of the exact s R(q) p + t at every point (tests/keyframe_model.py act_bound), and a mode with T
 * is bit for bit that mode on the output of "recent" with T.  HW == 0 returns without a launch.
 */
int m3s_pointmap_update(int mode, const float* T, const float* X_new, const float* C_new,
                        float* X, float* C, int64_t HW, void* stream);

/* ---------------- map export ---------------- */

/*
 * The confidence-filtered world point cloud of N keyframes as the body of a binary little-endian
 * PLY file (replaces save_reconstruction, evaluate.py:47-106; extension op -- the reference builds
 * the cloud on the host).  For k = 0..N-1, n = 0..HW-1, in that order:
 *   kept    C[k,n] / n_obs[k] > thresh       (f32 divide and compare; NaN is not kept)
 *   point   p = X[k,n]; with K, p = z ((u - cx) / fx, (v - cy) / fy, 1), z = X[k,n,2],
 *           u = n % width, v = n / width  (geometry.py:37-42, f32 subtract / divide / multiply);
 *           pW = s R(q) p + t of T_WC[k]  (the act of m3s_pointmap_update, bit for bit)
 *   record  <f4 x, f4 y, f4 z, u1 r, u1 g, u1 b>: 15 bytes, packed, little-endian
 * count: counts [N] i64 = kept points per keyframe, total [1] i64 = their sum (both device); leaves
 *   the tile offsets in ws.  emit: follows a count with the same args and ws on the same stream;
 *   writes the first min(total, capacity) records to out and nothing past 15 * capacity bytes.
 * Neither call synchronises the host.  N == 0 or HW == 0: M3S_OK, total 0.  Two runs give the
 * same bytes.  A tile (m3s_recon_tile_points points) never spans two keyframes.
 */
typedef struct m3s_recon_args {
  const float* X;      /* [N,HW,3] */
  const float* C;      /* [N,HW] */
  const float* n_obs;  /* [N] */
  const float* T_WC;   /* [N,8] */
  const uint8_t* rgb;  /* [N,HW,3] or NULL (records get 0,0,0) */
  const float* K;      /* [3,3] device or NULL */
  int64_t N, HW;
  int height, width;   /* height*width == HW, used only with K */
  float thresh;
  void* ws;
  size_t ws_bytes;
  void* stream;
} m3s_recon_args;
size_t m3s_recon_workspace_bytes(int64_t N, int64_t HW);
int64_t m3s_recon_tile_points(void);
int m3s_recon_count(const m3s_recon_args* args, int64_t* counts /* [N] dev */,
                    int64_t* total /* [1] dev */);
int m3s_recon_emit(const m3s_recon_args* args, void* out /* dev, 15*capacity B */, int64_t capacity);

/* ---------------- head finish: raw MASt3R head outputs -> X, C, D, Q ---------------- */

/*
 * One streaming pass from the raw tensors of a MASt3R head to the X, C, D, Q that matching, the
 * tracker and the edge construction consume.  Replaces the torch chain of
 * Cat_MLP_LocalFeatures_DPT_Pts3d.forward after the two sub-heads (catmlp_dpt_head.py:83-95:
 * transpose, view, pixel_shuffle, cat, postprocess), reg_dense_depth / reg_dense_conf
 * (dust3r/heads/postprocess.py:22-58), reg_desc (catmlp_dpt_head.py:17-22) and downsample
 * (mast3r_utils.py:43-52).  Extension op.  All tensors f32 on the device; batch strides in elements
 * (a [:, :4] view of a larger tensor is accepted), every other dimension contiguous.
 *   pts   [B,4,H,W] channel-planar: the DPT output (x, y, z, confidence logit)
 *   feat  NULL (no descriptor work: D and Q must be NULL too), or
 *         TOKENS [B,S,(F+1) p^2], S = (H/p)(W/p), p = patch = 16: the MLP output before the
 *                transpose and pixel_shuffle; pixel (v,u), channel c is at token (v/p)(W/p) + u/p,
 *                offset c p^2 + (v%p) p + (u%p); needs H % p == 0 and W % p == 0
 *         PLANAR [B,F+1,H,W]: channels 4.. of the head's raw output (any H, W)
 *         channels 0..F-1 the descriptor, channel F the descriptor-confidence logit; 1 <= F <= 32
 *   outputs, h = ceil(H/ds), w = ceil(W/ds), pixel (v ds, u ds) of the input (Python's [::ds]):
 *         X [B,h,w,3], C [B,h,w], D [B,h,w,F], Q [B,h,w], contiguous
 * f32 arithmetic, uncontracted, correctly rounded sqrt and divide, in this order:
 *   s = (x x + y y) + z z;  d = sqrt(s);  m = d < 1e-8f ? 1e-8f : d   (a NaN d stays NaN)
 *   X_c = (x_c / m) expm1f(d)
 *   C   = conf_vmin + min'(expf(a), conf_vmax - conf_vmin)            (min' keeps a NaN, as clip)
 *   n   = sqrt(((f_0 f_0 + f_1 f_1) + f_2 f_2) + ... + f_{F-1} f_{F-1});  D_c = f_c / n  (n = 0: NaN)
 *   Q   = dconf_vmin + min'(expf(q), dconf_vmax - dconf_vmin)
 * so D is a function of the inputs alone, bit for bit; X, C, Q carry the device library's expm1f /
 * expf.  Only the checkpoint's modes exist (depth exp unbounded, conf exp, desc norm, two
 * confidences): the mode fields must be 0.  Enqueues on `stream`, never synchronises, uses no
 * workspace; two runs give the same bytes.  B H W == 0: M3S_OK.
 */
enum { M3S_HEAD_TOKENS = 0, M3S_HEAD_PLANAR = 1 };
enum { M3S_HEAD_DEPTH_EXP = 0, M3S_HEAD_DEPTH_LINEAR = 1, M3S_HEAD_DEPTH_SQUARE = 2 };
enum { M3S_HEAD_CONF_EXP = 0, M3S_HEAD_CONF_SIGMOID = 1 };
enum { M3S_HEAD_DESC_NORM = 0 };
typedef struct m3s_head_args {
  const float* pts;
  const float* feat;   /* or NULL */
  int64_t pts_bstride, feat_bstride; /* elements between batch items */
  int64_t B, H, W, F;
  int layout;          /* M3S_HEAD_TOKENS / M3S_HEAD_PLANAR */
  int patch;           /* 16 */
  int downsample;      /* ds >= 1 */
  int depth_mode, conf_mode, desc_mode, single_conf; /* all 0: the checkpoint's */
  float conf_vmin, conf_vmax, dconf_vmin, dconf_vmax;
  float* X;
  float* C;
  float* D;            /* D and Q: both given or both NULL */
  float* Q;
  void* stream;
} m3s_head_args;
int m3s_head_finish(const m3s_head_args* args);

/* ---------------- RoPE2D: the attention's rotary position embedding, in place ---------------- */

/*
 * CroCo's curope kernel (thirdparty/mast3r/dust3r/croco/models/curope/kernels.cu,
 * rope_2d_cuda_kernel; torch fallback pos_embed.py:112-159) as one streaming pass.  tokens
 * [B,N,H,D], f32 or f16 on the device, updated in place; B and N strides in elements, the H stride
 * is D and the D stride 1 (a qkv[:, :, i] view of a [B,N,3,H,D] buffer is accepted).  pos [B,N,2]
 * int64, contiguous: (y, x) of every token.  With Q = D/4 a head's D values are
 * [u_Y (Q) | v_Y (Q) | u_X (Q) | v_X (Q)], and for axis A in {Y, X}, i in [0, Q):
 *   theta = (float)pos[b,n,A] * inv_freq_i,   inv_freq_i = (float)(f0 / base^(i/Q))  (host, f64)
 *   u' = u cos(theta) - v sin(theta);   v' = v cos(theta) + u sin(theta)
 * f32 arithmetic, uncontracted, the accurate sincosf; one rounding to the token dtype.  Only the
 * H D run of each addressed token is read or written.  D % 4 == 0, 4 <= D <= 256.  Enqueues on
 * `stream`, never synchronises, allocates nothing; B N == 0: M3S_OK and no launch.
 *
 * m3s_rope2d rotates `tokens` by `pos` (the k fields are ignored).  m3s_rope2d_pair rotates q by
 * qpos and k by kpos in ONE launch: Nq != Nk is allowed, B, H, D and the dtype are shared, qpos
 * and kpos may be one pointer; the bytes are those of two m3s_rope2d calls.
 */
enum { M3S_ROPE_F32 = 0, M3S_ROPE_F16 = 1 };
typedef struct m3s_rope_args {
  void* tokens;          /* q */
  const int64_t* pos;    /* qpos */
  int64_t N;             /* Nq */
  int64_t bstride, nstride; /* elements */
  void* k_tokens;        /* pair only */
  const int64_t* k_pos;
  int64_t k_N;
  int64_t k_bstride, k_nstride;
  int64_t B, H, D;
  float base, f0;
  int dtype;             /* M3S_ROPE_F32 / M3S_ROPE_F16 */
  void* stream;
} m3s_rope_args;
int m3s_rope2d(const m3s_rope_args* args);
int m3s_rope2d_pair(const m3s_rope_args* args);

/* ---------------- loop-closure retrieval (ASMK) ---------------- */

/*
 * RetrievalDatabase.update after the retrieval network (retrieval_database.py:43-166 with
 * asmk/kernel.py:26-68, inverted_file.py:56-108, functional.py:11-15, hamming.pyx): binary kernel,
 * no idf.  All on `stream`; a database is used from one stream at a time.  Extension ops (the
 * reference runs this in torch, numpy and Cython on the host).
 *
 * create: centroids [K,D] f32 on the device, BORROWED (they must outlive the database);
 *   1 <= D <= 4096, ma_build <= ma_query <= 8, K >= ma_query, max_feat * ma_query <= 4096.  |c|^2 is
 *   computed here.  table_or_null: NULL for the library's term table (m3s_retrieval_term_table),
 *   or [32 W + 1] f32 (host or device), W = ceil(D/32), the caller's own T[h] -- e.g. a host's
 *   np.power values, to reproduce that host's scores bit for bit.
 */
int m3s_retrieval_create(const float* centroids, int64_t K, int64_t D, int ma_build, int ma_query,
                         float alpha, float sim_thresh, const float* table_or_null,
                         int64_t max_feat, void** db);
int m3s_retrieval_destroy(void* db);
int m3s_retrieval_size(void* db, int64_t* n_images);
/* Host only (no GPU): T[h], h = 0..32W, the score term of a word pair at Hamming distance h:
 * nh = (float)h / (float)(32 W); sim = -2 nh + 1 (f32); T = 0 where sim < sim_thresh, else the
 * f32 rounding of pow((double)sim, (double)alpha).  table_out: host [32 W + 1]. */
int m3s_retrieval_term_table(int64_t D, float alpha, float sim_thresh, float* table_out);
/* ids_out [n,ma] i32: per feature the ma centroids of least |q|^2 + |c|^2 - 2 q.c (f32, the dot
 * product on the f32-input MFMA), ascending; equal distances by the lower index.  1 <= ma <= 8. */
int m3s_retrieval_quantize(void* db, const float* feat, int64_t n, int ma, int32_t* ids_out,
                           void* stream);
/* ids [n,ma] -> words_out [n*ma] i32 (the first *n_words_out ascending), codes_out [n*ma, W] u32
 * (sign bits of the per-word f32 residual sums, MSB first), n_words_out [1] i32, all device. */
int m3s_retrieval_aggregate(void* db, const float* feat, const int32_t* ids, int64_t n, int ma,
                            int32_t* words_out, uint32_t* codes_out, int32_t* n_words_out,
                            void* stream);
/* Quantise (ma_query), aggregate and score against every stored image: scores_out [n_images] f64
 * on the device (unused when the database is empty).  Keeps the query's nearest words for a
 * following add of the same `feat`.  No host synchronisation. */
int m3s_retrieval_query(void* db, const float* feat, int64_t n, double* scores_out, void* stream);
/* Append the image: its ma_build nearest words per feature (those of the preceding
 * m3s_retrieval_query of the same feat, n when reuse_last_query; else quantised here). */
int m3s_retrieval_add(void* db, const float* feat, int64_t n, int reuse_last_query, void* stream);
/* Read-back of stored image m (test / inspection): words_out [max_feat*ma_build] i32, codes_out
 * [max_feat*ma_build, W] u32, n_words_out [1] i32, all device. */
int m3s_retrieval_image(void* db, int64_t m, int32_t* words_out, uint32_t* codes_out,
                        int32_t* n_words_out, void* stream);

/* ---------------- multi-GPU (RCCL over xGMI) ---------------- */

/*
 * Communicator of the edge-sharded GN op (m3s_gn_args.comm): every iteration the compact
 * block-sparse system (f64) is sum-all-reduced in place before the replicated solve.  The
 * reference is single-GPU (its solve runs in Eigen on the host, gn_kernels.cu:1201-1209);
 * this is the seam SURVEY.md section 8(e) adds.
 */
#define M3S_COMM_ID_BYTES 128
/* RCCL over xGMI (production).  Rank 0 creates the id, the caller broadcasts it (e.g.
 * torch.distributed), every rank calls m3s_comm_init. */
int m3s_comm_get_unique_id(void* id_out /* M3S_COMM_ID_BYTES */);
int m3s_comm_init(const void* id, int nranks, int rank, void** comm_out);
/* Host-callback collective (test hook): the library drains the stream, stages the `count`
 * doubles in pinned host memory and calls fn(user, buf, count), which must replace buf with
 * the element-wise sum over ranks (e.g. a torch.distributed gloo all_reduce) and return 0. */
typedef int (*m3s_host_allreduce_fn)(void* user, double* buf, size_t count);
int m3s_comm_init_host(m3s_host_allreduce_fn fn, void* user, int nranks, int rank, void** comm_out);
int m3s_comm_destroy(void* comm);
/* The number of ranks the communicator spans, as its transport reports it (RCCL:
 * ncclCommCount; host callback: the count it was created with). */
int m3s_comm_size(void* comm, int* nranks_out);

#ifdef __cplusplus
}
#endif
#endif

// recon.hip -- map export: the confidence-filtered world point cloud of every keyframe as the
// body of a binary little-endian PLY file (gfx950).
//
// Replaces save_reconstruction (reference mast3r_slam/evaluate.py:47-106), which walks the
// keyframes on the host: per keyframe a D2H copy of the points, the confidences and the image, a
// boolean gather, and one concatenate at the end.  Here X, C, n_obs and T_WC are device-resident in
// one layout (KeyframeStore) and one streaming pass produces the file body:
//   kept    C[k,n] / n_obs[k] > thresh          (f32 divide, f32 compare; NaN is not kept)
//   point   p = X[k,n], or with K  z ((u - cx) / fx, (v - cy) / fy, 1)  (geometry.py:37-42)
//           pW = s R(q) p + t  of T_WC[k]       (the act of keyframe.hip, uncontracted)
//   record  <f4 x, f4 y, f4 z, u1 r, u1 g, u1 b>, 15 bytes, packed, in (k, n) order
//
// Three plain launches, none of which waits on another workgroup:
//   count  one workgroup per tile of kTile points of one keyframe -> tile_cnt[t]
//   scan   one workgroup: exclusive scan of tile_cnt -> tile_off[t] (i64), counts[k], total
//   emit   one workgroup per tile: re-evaluates the selection, ranks the kept points (ballot +
//          mbcnt inside a wave, LDS across the waves), stages their records in LDS at the byte
//          phase of the tile's output run, and writes the run as dword stores; only the first and
//          the last dword of a run can be partial, and those go out as byte stores (the neighbour
//          tiles own the other bytes of them).
// The order is fixed by the scan, so two runs give the same bytes.  All record and byte offsets
// are 64-bit (100 M points x 15 B > 2^31).
#include <hip/hip_runtime.h>

#include "../../include/m3s_backend.h"
#include "m3s_common.h"
#include "sim3.h"

#pragma clang fp contract(off)

namespace m3s {
namespace {

constexpr int kThreads = 256;                 // 4 waves of 64
constexpr int kWaves = kThreads / 64;
constexpr int kRounds = 4;                    // points per thread
constexpr int kTile = kThreads * kRounds;     // points per tile (m3s_recon_tile_points)
constexpr int kRec = 15;                      // bytes per record
constexpr int kStageWords = (kTile * kRec + 3 + 3) / 4;  // + up to 3 bytes of phase
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxGrid = 1 << 20;

struct Workspace {
    int64_t* tile_off;   // [ntiles + 1]
    uint32_t* tile_cnt;  // [ntiles]
};

__host__ __device__ inline int64_t tiles_per_keyframe(int64_t HW) { return (HW + kTile - 1) / kTile; }

inline size_t workspace_bytes(int64_t ntiles) {
    const size_t b = (size_t)(ntiles + 1) * sizeof(int64_t) + (size_t)ntiles * sizeof(uint32_t);
    return (b + 255) & ~(size_t)255;
}

inline Workspace carve(void* ws, int64_t ntiles) {
    Workspace w;
    w.tile_off = (int64_t*)ws;
    w.tile_cnt = (uint32_t*)(w.tile_off + ntiles + 1);
    return w;
}

// get_average_conf() > c_conf_threshold (evaluate.py:61-64); false for NaN
__device__ __forceinline__ bool kept(float c, float n_obs, float thresh) { return c / n_obs > thresh; }

// lanes below this one whose bit is set in `mask`
__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(kThreads) void recon_count_kernel(
    const float* __restrict__ C, const float* __restrict__ n_obs, int64_t HW, int64_t tpk,
    int64_t ntiles, float thresh, uint32_t* __restrict__ tile_cnt) {
    __shared__ int wave_cnt[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t k = t / tpk, n0 = (t - k * tpk) * kTile;
        const float nk = n_obs[k];
        const float* Ck = C + k * HW;
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
            const int64_t n = n0 + r * kThreads + threadIdx.x;
            const bool keep = n < HW && kept(Ck[n], nk, thresh);
            cnt += __popcll(__ballot(keep));
        }
        if (lane == 0) wave_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) s += wave_cnt[w];
            tile_cnt[t] = (uint32_t)s;
        }
        __syncthreads();
    }
}

// One workgroup: tile_off[t] = sum of tile_cnt[0..t), tile_off[ntiles] = total; then the kept
// points per keyframe from the offsets of its first tile and the next keyframe's.
__global__ __launch_bounds__(kScanThreads) void recon_scan_kernel(
    const uint32_t* __restrict__ tile_cnt, int64_t ntiles, int64_t tpk, int64_t N,
    int64_t* __restrict__ tile_off, int64_t* __restrict__ counts, int64_t* __restrict__ total) {
    __shared__ int64_t wave_sum[kScanThreads / 64];
    __shared__ int64_t carry_s;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < ntiles; base += kScanThreads) {
        const int64_t t = base + threadIdx.x;
        const int64_t v = t < ntiles ? (int64_t)tile_cnt[t] : 0;
        int64_t incl = v;  // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry_s;
        for (int w = 0; w < wave; w++) before += wave_sum[w];
        if (t < ntiles) tile_off[t] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tile_off[ntiles] = carry_s;
        total[0] = carry_s;
    }
    __threadfence_block();
    __syncthreads();
    for (int64_t k = threadIdx.x; k < N; k += kScanThreads)
        counts[k] = tile_off[(k + 1) * tpk] - tile_off[k * tpk];
}

__device__ __forceinline__ void stage_u32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

template <bool CALIB>
__global__ __launch_bounds__(kThreads) void recon_emit_kernel(
    const float* __restrict__ X, const float* __restrict__ C, const float* __restrict__ n_obs,
    const float* __restrict__ T_WC, const uint8_t* __restrict__ rgb, const float* __restrict__ K,
    int64_t HW, int width, int64_t tpk, int64_t ntiles, float thresh,
    const int64_t* __restrict__ tile_off, uint8_t* __restrict__ out, int64_t capacity) {
    __shared__ uint32_t stage_w[kStageWords];
    __shared__ int wave_cnt[kRounds * kWaves];
    uint8_t* stage = (uint8_t*)stage_w;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
    if constexpr (CALIB) { fx = K[0]; cx = K[2]; fy = K[4]; cy = K[5]; }

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t base = tile_off[t];                 // records before this tile
        const int64_t room = capacity - base;             // records this tile may still write
        if (room <= 0) continue;                          // uniform over the workgroup
        const int64_t k = t / tpk, n0 = (t - k * tpk) * kTile;
        const float nk = n_obs[k];
        const float* Ck = C + k * HW;

        bool keep[kRounds];
        int below[kRounds];
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
            const int64_t n = n0 + r * kThreads + threadIdx.x;
            keep[r] = n < HW && kept(Ck[n], nk, thresh);
            const uint64_t m = __ballot(keep[r]);
            below[r] = lanes_below(m);
            if (lane == 0) wave_cnt[r * kWaves + wave] = __popcll(m);
        }
        __syncthreads();
        // rank in the tile: points go round by round, wave by wave, lane by lane (= n order)
        int prefix[kRounds];
        int tile_cnt = 0;
#pragma unroll
        for (int r = 0; r < kRounds; r++)
#pragma unroll
            for (int w = 0; w < kWaves; w++) {
                if (w == wave) prefix[r] = tile_cnt;
                tile_cnt += wave_cnt[r * kWaves + w];
            }
        const int nrec = (int)((int64_t)tile_cnt < room ? (int64_t)tile_cnt : room);
        const int64_t byte0 = base * kRec;                 // first byte of the run in `out`
        const int phase = (int)(((uintptr_t)out + (uint64_t)byte0) & 3u);

        const float* Tk = T_WC + k * 8;
        const float tt[3] = {Tk[0], Tk[1], Tk[2]};
        const float q[4] = {Tk[3], Tk[4], Tk[5], Tk[6]};
        const float s = Tk[7];
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
            const int idx = prefix[r] + below[r];
            if (!keep[r] || idx >= nrec) continue;
            const int64_t n = n0 + r * kThreads + threadIdx.x;
            const int64_t g = k * HW + n;
            float p[3] = {X[3 * g], X[3 * g + 1], X[3 * g + 2]};
            if constexpr (CALIB) {  // constrain_points_to_ray: z * ((u - cx) / fx, (v - cy) / fy, 1)
                const uint32_t nn = (uint32_t)n;  // HW < 2^31 with K
                const float u = (float)(nn % (uint32_t)width), v = (float)(nn / (uint32_t)width);
                const float z = p[2];
                p[0] = z * ((u - cx) / fx);
                p[1] = z * ((v - cy) / fy);
            }
            float rr[3];
            act_so3(q, p, rr);  // lietorch act: s R(q) p + t, as pointmap_update_kernel
            const float w0 = s * rr[0] + tt[0];
            const float w1 = s * rr[1] + tt[1];
            const float w2 = s * rr[2] + tt[2];
            uint8_t* rec = stage + phase + idx * kRec;
            stage_u32(rec, __float_as_uint(w0));
            stage_u32(rec + 4, __float_as_uint(w1));
            stage_u32(rec + 8, __float_as_uint(w2));
            uint8_t c0 = 0, c1 = 0, c2 = 0;
            if (rgb) { c0 = rgb[3 * g]; c1 = rgb[3 * g + 1]; c2 = rgb[3 * g + 2]; }
            rec[12] = c0; rec[13] = c1; rec[14] = c2;
        }
        __syncthreads();
        // staged bytes [phase, end) <-> out bytes [byte0, byte0 + 15 nrec): dword j of the stage
        // is the aligned dword j of the run
        const int end = phase + nrec * kRec;
        const int ndw = (end + 3) >> 2;
        uint8_t* run = out + (byte0 - phase);              // 4-byte aligned
        for (int j = threadIdx.x; j < ndw; j += kThreads) {
            const int lo = 4 * j, hi = lo + 4;
            if (lo >= phase && hi <= end) {
                ((uint32_t*)run)[j] = stage_w[j];
            } else {  // head or tail dword: the bytes outside [phase, end) belong to other tiles
                const int b0 = lo > phase ? lo : phase, b1 = hi < end ? hi : end;
                for (int b = b0; b < b1; b++) run[b] = stage[b];
            }
        }
        __syncthreads();  // the stage is reused by the next tile
    }
}

hipError_t zero_results(int64_t* counts, int64_t N, int64_t* total, hipStream_t st) {
    if (N > 0) {
        hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * sizeof(int64_t), st);
        if (e != hipSuccess) return e;
    }
    return hipMemsetAsync(total, 0, sizeof(int64_t), st);
}

}  // namespace
}  // namespace m3s

#define M3S_RECON_REQUIRE_ARGS(a, what)                                                         \
    M3S_REQUIRE((a) != nullptr, what ": null args");                                            \
    M3S_REQUIRE((a)->N >= 0 && (a)->HW >= 0, what ": negative size");                           \
    M3S_REQUIRE((a)->HW <= ((int64_t)1 << 40) && (a)->N <= ((int64_t)1 << 31), what ": size too large")

extern "C" int64_t m3s_recon_tile_points(void) { return m3s::kTile; }

extern "C" size_t m3s_recon_workspace_bytes(int64_t N, int64_t HW) {
    if (N <= 0 || HW <= 0) return m3s::workspace_bytes(0);
    return m3s::workspace_bytes(N * m3s::tiles_per_keyframe(HW));
}

static int recon_check(const m3s_recon_args* a, const char* what, int64_t* ntiles_out) {
    const int64_t ntiles = a->N * m3s::tiles_per_keyframe(a->HW);
    M3S_REQUIRE(ntiles < ((int64_t)1 << 40), "%s: too many tiles", what);
    M3S_REQUIRE(a->X && a->C && a->n_obs && a->T_WC, "%s: null pointer", what);
    M3S_REQUIRE(a->ws && a->ws_bytes >= m3s::workspace_bytes(ntiles), "%s: workspace too small (%zu < %zu)",
                what, a->ws_bytes, m3s::workspace_bytes(ntiles));
    M3S_REQUIRE(((uintptr_t)a->ws & 7u) == 0, "%s: workspace must be 8-byte aligned", what);
    if (a->K)
        M3S_REQUIRE(a->height > 0 && a->width > 0 && (int64_t)a->height * a->width == a->HW &&
                        a->HW < ((int64_t)1 << 31),
                    "%s: height * width must equal HW (< 2^31) when K is given", what);
    *ntiles_out = ntiles;
    return M3S_OK;
}

extern "C" int m3s_recon_count(const m3s_recon_args* a, int64_t* counts, int64_t* total) {
    M3S_RECON_REQUIRE_ARGS(a, "recon_count");
    M3S_REQUIRE(total && (counts || a->N == 0), "recon_count: null output");
    hipStream_t st = (hipStream_t)a->stream;
    if (a->N == 0 || a->HW == 0) {
        M3S_HIP_CHECK(m3s::zero_results(counts, a->N, total, st));
        return M3S_OK;
    }
    int64_t ntiles = 0;
    if (int rc = recon_check(a, "recon_count", &ntiles)) return rc;
    const m3s::Workspace w = m3s::carve(a->ws, ntiles);
    const int64_t tpk = m3s::tiles_per_keyframe(a->HW);
    const int nb = (int)(ntiles < m3s::kMaxGrid ? ntiles : m3s::kMaxGrid);
    hipLaunchKernelGGL(m3s::recon_count_kernel, dim3(nb), dim3(m3s::kThreads), 0, st, a->C, a->n_obs,
                       a->HW, tpk, ntiles, a->thresh, w.tile_cnt);
    M3S_LAUNCH_CHECK();
    hipLaunchKernelGGL(m3s::recon_scan_kernel, dim3(1), dim3(m3s::kScanThreads), 0, st, w.tile_cnt,
                       ntiles, tpk, a->N, w.tile_off, counts, total);
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

extern "C" int m3s_recon_emit(const m3s_recon_args* a, void* out, int64_t capacity) {
    M3S_RECON_REQUIRE_ARGS(a, "recon_emit");
    M3S_REQUIRE(capacity >= 0, "recon_emit: negative capacity");
    if (a->N == 0 || a->HW == 0 || capacity == 0) return M3S_OK;
    M3S_REQUIRE(out != nullptr, "recon_emit: null output");
    int64_t ntiles = 0;
    if (int rc = recon_check(a, "recon_emit", &ntiles)) return rc;
    const m3s::Workspace w = m3s::carve(a->ws, ntiles);
    const int64_t tpk = m3s::tiles_per_keyframe(a->HW);
    const int nb = (int)(ntiles < m3s::kMaxGrid ? ntiles : m3s::kMaxGrid);
    hipStream_t st = (hipStream_t)a->stream;
    if (a->K)
        hipLaunchKernelGGL(m3s::recon_emit_kernel<true>, dim3(nb), dim3(m3s::kThreads), 0, st, a->X,
                           a->C, a->n_obs, a->T_WC, a->rgb, a->K, a->HW, a->width, tpk, ntiles,
                           a->thresh, w.tile_off, (uint8_t*)out, capacity);
    else
        hipLaunchKernelGGL(m3s::recon_emit_kernel<false>, dim3(nb), dim3(m3s::kThreads), 0, st, a->X,
                           a->C, a->n_obs, a->T_WC, a->rgb, a->K, a->HW, a->width, tpk, ntiles,
                           a->thresh, w.tile_off, (uint8_t*)out, capacity);
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

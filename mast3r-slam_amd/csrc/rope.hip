// rope.hip -- RoPE2D: the attention's rotary position embedding, in place, one pass (gfx950).
//
// CroCo's curope kernel (reference thirdparty/mast3r/dust3r/croco/models/curope/kernels.cu,
// rope_2d_cuda_kernel) for the MI355X; on ROCm the reference runs its torch fallback
// (croco/models/pos_embed.py:112-159: a host wait on positions.max() and about a dozen launches per
// call, two calls per attention).  The formula is stated in include/m3s_backend.h ("RoPE2D");
// nothing is contracted (-ffp-contract=off in the Makefile), so a token at position (0, 0) keeps
// its bits and the result does not depend on the head, the kernel variant or the launch shape.
//
// The pass is launch- and latency-bound (a token of 16 heads x 64 f32 is 4 KB, a call a few MB).
// D = 64 (the encoder's 1024/16 and the decoder's 768/12): one wave per token, 8 lanes per head,
// 8 heads per step.  A lane owns the 4-element runs u[4j..4j+3] and v[4j..4j+3] of one axis of one
// head (16-byte accesses for f32, 8-byte for f16), computes its four sincosf once per token and
// reuses them for every head step: no LDS, no cross-lane traffic.  Every other D, and a D = 64
// buffer without that alignment: one thread per (u, v) pair, scalar accesses.
// q and k of one attention go in one launch: the waves (threads) past q's tokens take k's.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>

#include "../../include/m3s_backend.h"
#include "m3s_common.h"

#pragma clang fp contract(off)

namespace m3s {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;  // tokens per workgroup of the D = 64 kernel
constexpr int kSpecD = 64;
constexpr int kMaxD = 256;
constexpr int kMaxQ = kMaxD / 4;

struct RopeSide {
    void* tok;
    const int64_t* pos;
    int64_t sB, sN;  // element strides of tok
    int64_t N;
};

struct RopeParams {
    RopeSide q, k;
    int64_t nq_tok;  // B * Nq: tokens [0, nq_tok) are q's, [nq_tok, total) k's
    int64_t total;   // B * (Nq + Nk)
    uint32_t H, D;
    float inv_freq[kMaxQ];
};

__device__ __forceinline__ void rotate(float u, float v, float c, float s, float& uo, float& vo) {
    uo = u * c - v * s;
    vo = v * c + u * s;
}

__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ void store1(float* p, float x) { *p = x; }
__device__ __forceinline__ void store1(__half* p, float x) { *p = __float2half_rn(x); }

__device__ __forceinline__ void load4(const float* p, float (&x)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
}
__device__ __forceinline__ void load4(const __half* p, float (&x)[4]) {
    union { uint2 raw; __half h[4]; } t;
    t.raw = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int e = 0; e < 4; e++) x[e] = __half2float(t.h[e]);
}
__device__ __forceinline__ void store4(float* p, const float (&x)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
}
__device__ __forceinline__ void store4(__half* p, const float (&x)[4]) {
    union { uint2 raw; __half h[4]; } t;
#pragma unroll
    for (int e = 0; e < 4; e++) t.h[e] = __float2half_rn(x[e]);
    *reinterpret_cast<uint2*>(p) = t.raw;
}

// token w of the launch -> its first element and its (y, x)
template <typename T>
__device__ __forceinline__ T* token_of(const RopeParams& p, int64_t w, const int64_t*& pos) {
    const bool isk = w >= p.nq_tok;
    if (isk) w -= p.nq_tok;
    const int64_t N = isk ? p.k.N : p.q.N;
    const int64_t b = w / N, n = w - b * N;
    pos = (isk ? p.k.pos : p.q.pos) + 2 * w;
    T* base = static_cast<T*>(isk ? p.k.tok : p.q.tok);
    return base + b * (isk ? p.k.sB : p.q.sB) + n * (isk ? p.k.sN : p.q.sN);
}

// D = 64: wave = token, lane = (head of the step, axis, 4-element run)
template <typename T>
__global__ __launch_bounds__(kThreads) void rope2d_d64_kernel(const RopeParams p) {
    constexpr uint32_t Q = kSpecD / 4;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (w >= p.total) return;
    const int64_t* pos;
    T* tok = token_of<T>(p, w, pos);

    const uint32_t hs = lane >> 3, axis = (lane >> 2) & 1u, j = lane & 3u;
    const float t = (float)pos[axis];
    float c[4], s[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float f = p.inv_freq[e];
#pragma unroll
        for (int jj = 1; jj < 4; jj++) f = j == (uint32_t)jj ? p.inv_freq[4 * jj + e] : f;
        sincosf(t * f, &s[e], &c[e]);
    }

    T* mine = tok + axis * (2 * Q) + 4 * j;  // u run; the v run is Q further
    for (uint32_t h0 = 0; h0 < p.H; h0 += 16) {
        // two head steps per trip, both loaded before either is stored
        const uint32_t ha = h0 + hs, hb = h0 + 8 + hs;
        const bool oka = ha < p.H, okb = hb < p.H;
        T* pa = mine + (int64_t)ha * kSpecD;
        T* pb = mine + (int64_t)hb * kSpecD;
        float ua[4], va[4], ub[4], vb[4];
        if (oka) { load4(pa, ua); load4(pa + Q, va); }
        if (okb) { load4(pb, ub); load4(pb + Q, vb); }
        if (oka) {
            float uo[4], vo[4];
#pragma unroll
            for (int e = 0; e < 4; e++) rotate(ua[e], va[e], c[e], s[e], uo[e], vo[e]);
            store4(pa, uo);
            store4(pa + Q, vo);
        }
        if (okb) {
            float uo[4], vo[4];
#pragma unroll
            for (int e = 0; e < 4; e++) rotate(ub[e], vb[e], c[e], s[e], uo[e], vo[e]);
            store4(pb, uo);
            store4(pb + Q, vo);
        }
    }
}

// any D: thread = one (u, v) pair
template <typename T>
__global__ __launch_bounds__(kThreads) void rope2d_generic_kernel(const RopeParams p, int64_t pairs) {
    __shared__ float inv_freq[kMaxQ];
    const uint32_t Q = p.D / 4;
    if (threadIdx.x < kMaxQ) {
        float f = 0.0f;
#pragma unroll
        for (int i = 0; i < kMaxQ; i++) f = threadIdx.x == (uint32_t)i ? p.inv_freq[i] : f;
        inv_freq[threadIdx.x] = f;
    }
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= pairs) return;
    const int64_t per_tok = (int64_t)p.H * (2 * Q);
    const int64_t w = g / per_tok;
    const uint32_t r = (uint32_t)(g - w * per_tok);  // < H * D / 2
    const uint32_t h = r / (2 * Q), ra = r - h * (2 * Q);
    const uint32_t axis = ra / Q, i = ra - axis * Q;
    const int64_t* pos;
    T* tok = token_of<T>(p, w, pos);
    float c, s;
    sincosf((float)pos[axis] * inv_freq[i], &s, &c);
    T* pu = tok + (int64_t)h * p.D + axis * (2 * Q) + i;
    float uo, vo;
    rotate(load1(pu), load1(pu + Q), c, s, uo, vo);
    store1(pu, uo);
    store1(pu + Q, vo);
}

template <typename T>
bool aligned4(const RopeSide& s) {
    const uintptr_t m = 4 * sizeof(T) - 1;
    return (((uintptr_t)s.tok | (uintptr_t)(s.sB * (int64_t)sizeof(T)) |
             (uintptr_t)(s.sN * (int64_t)sizeof(T))) & m) == 0;
}

template <typename T>
int launch(const RopeParams& p, hipStream_t st) {
    if (p.D == kSpecD && aligned4<T>(p.q) && (p.k.tok == nullptr || aligned4<T>(p.k))) {
        const int64_t blocks = (p.total + kWaves - 1) / kWaves;
        M3S_REQUIRE(blocks <= 0x7fffffff, "rope2d: too many tokens for one launch");
        hipLaunchKernelGGL((rope2d_d64_kernel<T>), dim3((uint32_t)blocks), dim3(kThreads), 0, st, p);
    } else {
        M3S_REQUIRE(p.total <= INT64_MAX / ((int64_t)p.H * (p.D / 2)), "rope2d: too many values");
        const int64_t pairs = p.total * p.H * (p.D / 2);
        const int64_t blocks = (pairs + kThreads - 1) / kThreads;
        M3S_REQUIRE(blocks <= 0x7fffffff, "rope2d: too many values for one launch");
        hipLaunchKernelGGL((rope2d_generic_kernel<T>), dim3((uint32_t)blocks), dim3(kThreads), 0, st,
                           p, pairs);
    }
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

int run(const m3s_rope_args* a, bool pair, const char* what) {
    M3S_REQUIRE(a != nullptr, "%s: null args", what);
    M3S_REQUIRE(a->dtype == M3S_ROPE_F32 || a->dtype == M3S_ROPE_F16, "%s: unknown dtype %d", what,
                a->dtype);
    M3S_REQUIRE(a->D % 4 == 0, "%s: token dim must be multiple of 4, got %lld", what, (long long)a->D);
    M3S_REQUIRE(a->D >= 4 && a->D <= kMaxD, "%s: token dim must be in 4..%d, got %lld", what, kMaxD,
                (long long)a->D);
    const int64_t Nk = pair ? a->k_N : 0;
    M3S_REQUIRE(a->B >= 0 && a->N >= 0 && Nk >= 0 && a->H >= 0, "%s: negative size", what);
    M3S_REQUIRE(a->B <= 0x7fffffff && a->N <= 0x7fffffff && Nk <= 0x7fffffff && a->H <= 0x7fffff,
                "%s: size too large", what);
    M3S_REQUIRE(a->base > 0.0f && std::isfinite(a->base) && std::isfinite(a->f0),
                "%s: base must be positive and finite, F0 finite", what);
    const int64_t nq = a->B * a->N, nk = a->B * Nk;
    if (nq + nk == 0 || a->H == 0) return M3S_OK;

    RopeParams p;
    p.q = RopeSide{a->tokens, a->pos, a->bstride, a->nstride, a->N};
    p.k = RopeSide{nullptr, nullptr, 0, 0, 1};
    if (nk) p.k = RopeSide{a->k_tokens, a->k_pos, a->k_bstride, a->k_nstride, Nk};
    if (nq == 0) {  // only k has tokens: it becomes the launch's first side
        p.q = p.k;
        p.k = RopeSide{nullptr, nullptr, 0, 0, 1};
    }
    p.nq_tok = nq ? nq : nk;
    p.total = nq + nk;
    M3S_REQUIRE(p.q.tok && p.q.pos && (p.total == p.nq_tok || (p.k.tok && p.k.pos)),
                "%s: null pointer", what);
    p.H = (uint32_t)a->H;
    p.D = (uint32_t)a->D;
    const int Q = (int)(a->D / 4);
    for (int i = 0; i < kMaxQ; i++)
        p.inv_freq[i] =
            i < Q ? (float)((double)a->f0 / std::pow((double)a->base, (double)i / (double)Q)) : 0.0f;

    hipStream_t st = (hipStream_t)a->stream;
    return a->dtype == M3S_ROPE_F32 ? launch<float>(p, st) : launch<__half>(p, st);
}

}  // namespace
}  // namespace m3s

extern "C" int m3s_rope2d(const m3s_rope_args* a) { return m3s::run(a, false, "rope2d"); }

extern "C" int m3s_rope2d_pair(const m3s_rope_args* a) { return m3s::run(a, true, "rope2d_pair"); }

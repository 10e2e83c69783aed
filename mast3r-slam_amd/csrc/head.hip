// head.hip -- head finish: the raw tensors of a MASt3R head to X, C, D, Q in one pass (gfx950).
//
// Replaces the torch chain between the network's two sub-heads and the matcher: transpose, view,
// pixel_shuffle, cat and postprocess of Cat_MLP_LocalFeatures_DPT_Pts3d.forward (reference
// thirdparty/mast3r/mast3r/catmlp_dpt_head.py:83-95, :17-39), reg_dense_depth / reg_dense_conf
// (dust3r/heads/postprocess.py:22-58) and downsample (mast3r_slam/mast3r_utils.py:43-52).  The
// arithmetic and its order are stated in include/m3s_backend.h ("head finish"); nothing is
// contracted (-ffp-contract=off in the Makefile) and sqrt / divide are correctly rounded, so D is
// a function of the inputs alone.
//
// One 256-thread workgroup per 16x16 patch, thread = pixel (i, j) of the patch.  The MLP's
// token-major output holds channel c of a patch as 256 contiguous floats in (i, j) order, so in
// the TOKENS layout every load of a wave is 256 contiguous bytes and the pixel shuffle is the load
// index; PLANAR reads 16 rows of 64 bytes per channel.  A thread keeps its pixel's F+1 values in
// registers.  The kept pixels of a patch ([::ds] in both directions) form nr x nc outputs; each of
// its output rows is one contiguous run of nc*F floats of D (nc*3 of X), so D and X are staged in
// LDS in output order and the runs go out as consecutive 16-byte (D, when F % 4 == 0) or 4-byte
// stores.  C and Q are 64-byte runs and are stored from registers.  No workgroup reads what
// another wrote: no atomics, no workspace, and the bytes do not depend on the schedule.
#include <hip/hip_runtime.h>

#include "../../include/m3s_backend.h"
#include "m3s_common.h"

#pragma clang fp contract(off)

namespace m3s {
namespace {

constexpr int kP = 16;                 // patch edge
constexpr int kThreads = kP * kP;      // one thread per pixel of a patch
constexpr int kMaxF = 32;              // largest descriptor width
constexpr int kSpecF = 24;             // the checkpoint's width: compile-time channel loops

struct HeadParams {
    const float* pts;
    const float* feat;
    float* X;
    float* C;
    float* D;
    float* Q;
    int64_t pts_bs, feat_bs;  // batch strides, elements
    int64_t HW;               // H * W
    uint32_t H, W, h, w;      // input and output image
    uint32_t gh, gw;          // patch grid
    uint32_t F, ds;
    float conf_vmin, conf_lim, dconf_vmin, dconf_lim;  // lim = vmax - vmin
};

// vmin + clip(exp(a), max = lim): a NaN stays NaN, as torch.clip does
__device__ __forceinline__ float conf_exp(float a, float vmin, float lim) {
    const float e = expf(a);
    return vmin + (e > lim ? lim : e);
}

// first kept output index and the count of kept indices of the input range [x0, x0 + kP) clipped
// to n outputs: kept inputs are the multiples of ds
__device__ __forceinline__ void kept_range(uint32_t x0, uint32_t ds, uint32_t n, uint32_t& first,
                                           uint32_t& count) {
    first = (x0 + ds - 1) / ds;
    uint32_t end = (x0 + kP + ds - 1) / ds;
    if (end > n) end = n;
    count = end - first;
}

// The nr x nc x K staged values go to rows of `nc * K` consecutive elements of type T, `pitch`
// elements of T apart, starting at dst.
template <typename T>
__device__ __forceinline__ void store_runs(const T* __restrict__ stage, T* __restrict__ dst,
                                           uint32_t nr, uint32_t run, int64_t pitch) {
    const uint32_t total = nr * run;
    for (uint32_t q = threadIdx.x; q < total; q += kThreads) {
        const uint32_t lr = q / run, rem = q - lr * run;
        dst[(int64_t)lr * pitch + rem] = stage[q];
    }
}

// FT: the descriptor width when known at compile time, 0 for the run-time p.F (<= kMaxF).
template <bool DESC, int FT, bool TOKENS, bool VEC4>
__global__ __launch_bounds__(kThreads) void head_finish_kernel(const HeadParams p) {
    constexpr int FCAP = FT ? FT : kMaxF;
    __shared__ __align__(16) float sD[DESC ? kThreads * FCAP : 4];
    __shared__ float sX[kThreads * 3];

    const uint32_t tid = threadIdx.x;
    const uint32_t F = FT ? (uint32_t)FT : p.F;
    uint32_t blk = blockIdx.x;
    const uint32_t tx = blk % p.gw;
    blk /= p.gw;
    const uint32_t ty = blk % p.gh;
    const int64_t b = blk / p.gh;

    const uint32_t v = ty * kP + (tid >> 4), u = tx * kP + (tid & 15u);
    const uint32_t vo = v / p.ds, uo = u / p.ds;
    const bool keep = v < p.H && u < p.W && vo * p.ds == v && uo * p.ds == u;
    uint32_t r0, nr, c0, nc;
    kept_range(ty * kP, p.ds, p.h, r0, nr);
    kept_range(tx * kP, p.ds, p.w, c0, nc);

    if (keep) {
        const uint32_t slot = (vo - r0) * nc + (uo - c0);  // < nr * nc <= kThreads
        const int64_t pix = (int64_t)v * p.W + u;
        const float* pp = p.pts + b * p.pts_bs + pix;
        const float x = pp[0], y = pp[p.HW], z = pp[2 * p.HW], a = pp[3 * p.HW];

        float f[FCAP + 1];
        if constexpr (DESC) {
            const float* fp;
            int64_t cs;  // channel stride
            if constexpr (TOKENS) {
                fp = p.feat + b * p.feat_bs + (int64_t)(ty * p.gw + tx) * ((F + 1) * kThreads) + tid;
                cs = kThreads;
            } else {
                fp = p.feat + b * p.feat_bs + pix;
                cs = p.HW;
            }
#pragma unroll
            for (int c = 0; c <= FCAP; c++) f[c] = (uint32_t)c <= F ? fp[c * cs] : 0.0f;
        }

        const float s = (x * x + y * y) + z * z;
        const float d = sqrtf(s);
        const float m = d < 1e-8f ? 1e-8f : d;  // clip(min): a NaN d stays NaN
        const float g = expm1f(d);
        sX[3 * slot + 0] = (x / m) * g;
        sX[3 * slot + 1] = (y / m) * g;
        sX[3 * slot + 2] = (z / m) * g;
        const int64_t o = (b * p.h + vo) * p.w + uo;
        p.C[o] = conf_exp(a, p.conf_vmin, p.conf_lim);

        if constexpr (DESC) {
            float acc = f[0] * f[0];
#pragma unroll
            for (int c = 1; c < FCAP; c++)
                if ((uint32_t)c < F) acc = acc + f[c] * f[c];
            const float n = sqrtf(acc);  // no guard: n = 0 gives NaN, as the reference does
            float q = f[FCAP];           // the logit is channel F
            if constexpr (FT == 0) {
#pragma unroll
                for (int c = 1; c < FCAP; c++)
                    if ((uint32_t)c == F) q = f[c];
            }
#pragma unroll
            for (int c = 0; c < FCAP; c++)
                if ((uint32_t)c < F) f[c] = f[c] / n;
            if constexpr (VEC4) {  // F % 4 == 0
                float4* row = reinterpret_cast<float4*>(sD) + slot * (F / 4);
#pragma unroll
                for (int k = 0; k < FCAP / 4; k++)
                    if ((uint32_t)(4 * k) < F)
                        row[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
            } else {
#pragma unroll
                for (int c = 0; c < FCAP; c++)
                    if ((uint32_t)c < F) sD[slot * F + c] = f[c];
            }
            p.Q[o] = conf_exp(q, p.dconf_vmin, p.dconf_lim);
        }
    }
    __syncthreads();

    // element offset of the patch's first output pixel; its rows are w pixels apart
    const int64_t o0 = (b * p.h + r0) * p.w + c0;
    store_runs<float>(sX, p.X + 3 * o0, nr, nc * 3, (int64_t)p.w * 3);
    if constexpr (DESC) {
        if constexpr (VEC4)  // D is 16-byte aligned and F % 4 == 0: every pixel starts a float4
            store_runs<float4>(reinterpret_cast<const float4*>(sD),
                               reinterpret_cast<float4*>(p.D) + o0 * (F / 4), nr, nc * (F / 4),
                               (int64_t)p.w * (F / 4));
        else
            store_runs<float>(sD, p.D + o0 * F, nr, nc * F, (int64_t)p.w * F);
    }
}

template <bool DESC, int FT, bool TOKENS, bool VEC4>
void launch(const HeadParams& p, int64_t nblocks, hipStream_t st) {
    hipLaunchKernelGGL((head_finish_kernel<DESC, FT, TOKENS, VEC4>), dim3((uint32_t)nblocks),
                       dim3(kThreads), 0, st, p);
}

template <int FT>
void launch_desc(const HeadParams& p, bool tokens, bool vec4, int64_t nblocks, hipStream_t st) {
    if (tokens) {
        if (vec4) launch<true, FT, true, true>(p, nblocks, st);
        else launch<true, FT, true, false>(p, nblocks, st);
    } else {
        if (vec4) launch<true, FT, false, true>(p, nblocks, st);
        else launch<true, FT, false, false>(p, nblocks, st);
    }
}

}  // namespace
}  // namespace m3s

extern "C" int m3s_head_finish(const m3s_head_args* a) {
    using namespace m3s;
    M3S_REQUIRE(a != nullptr, "head_finish: null args");
    M3S_REQUIRE(a->depth_mode == M3S_HEAD_DEPTH_EXP,
                "head_finish: only depth mode exp (unbounded) is built, got %d", a->depth_mode);
    M3S_REQUIRE(a->conf_mode == M3S_HEAD_CONF_EXP, "head_finish: only conf mode exp is built, got %d",
                a->conf_mode);
    M3S_REQUIRE(a->desc_mode == M3S_HEAD_DESC_NORM, "head_finish: only desc mode norm is built, got %d",
                a->desc_mode);
    M3S_REQUIRE(a->single_conf == 0, "head_finish: only two_confs=True is built");
    M3S_REQUIRE(a->layout == M3S_HEAD_TOKENS || a->layout == M3S_HEAD_PLANAR,
                "head_finish: unknown feat layout %d", a->layout);
    M3S_REQUIRE(a->patch == kP, "head_finish: patch must be %d, got %d", kP, a->patch);
    M3S_REQUIRE(a->downsample >= 1, "head_finish: downsample must be >= 1, got %d", a->downsample);
    M3S_REQUIRE(a->B >= 0 && a->H >= 0 && a->W >= 0, "head_finish: negative size");
    M3S_REQUIRE((a->D == nullptr) == (a->Q == nullptr), "head_finish: D and Q go together");
    const bool desc = a->D != nullptr;
    if (desc) {
        M3S_REQUIRE(a->F >= 1 && a->F <= kMaxF, "head_finish: F must be in 1..%d, got %lld", kMaxF,
                    (long long)a->F);
        if (a->layout == M3S_HEAD_TOKENS)
            M3S_REQUIRE(a->H % kP == 0 && a->W % kP == 0,
                        "head_finish: the tokens layout needs H and W to be multiples of %d, got %lldx%lld",
                        kP, (long long)a->H, (long long)a->W);
    }
    if (a->B == 0 || a->H == 0 || a->W == 0) return M3S_OK;
    M3S_REQUIRE(a->pts && a->X && a->C, "head_finish: null pointer");
    M3S_REQUIRE(!desc || a->feat, "head_finish: D and Q need feat");
    M3S_REQUIRE(a->pts_bstride >= 0 && (!desc || a->feat_bstride >= 0), "head_finish: negative batch stride");
    M3S_REQUIRE(a->H <= ((int64_t)1 << 30) && a->W <= ((int64_t)1 << 30), "head_finish: image too large");
    const int64_t gh = (a->H + kP - 1) / kP, gw = (a->W + kP - 1) / kP;
    M3S_REQUIRE(gh * gw <= 0x7fffffff && a->B <= 0x7fffffff / (gh * gw),
                "head_finish: too many patches for one launch");
    const int64_t nblocks = a->B * gh * gw;

    HeadParams p;
    p.pts = a->pts;
    p.feat = a->feat;
    p.X = a->X;
    p.C = a->C;
    p.D = a->D;
    p.Q = a->Q;
    p.pts_bs = a->pts_bstride;
    p.feat_bs = a->feat_bstride;
    p.HW = a->H * a->W;
    p.H = (uint32_t)a->H;
    p.W = (uint32_t)a->W;
    // a step past the image keeps pixel (0, 0) only
    p.ds = (uint32_t)(a->downsample < ((int64_t)1 << 30) ? a->downsample : ((int64_t)1 << 30));
    p.h = (p.H + p.ds - 1) / p.ds;
    p.w = (p.W + p.ds - 1) / p.ds;
    p.gh = (uint32_t)gh;
    p.gw = (uint32_t)gw;
    p.F = (uint32_t)(desc ? a->F : 0);
    p.conf_vmin = a->conf_vmin;
    p.conf_lim = a->conf_vmax - a->conf_vmin;
    p.dconf_vmin = a->dconf_vmin;
    p.dconf_lim = a->dconf_vmax - a->dconf_vmin;

    hipStream_t st = (hipStream_t)a->stream;
    if (!desc) {
        launch<false, 0, false, false>(p, nblocks, st);
    } else {
        const bool tokens = a->layout == M3S_HEAD_TOKENS;
        const bool vec4 = a->F % 4 == 0 && ((uintptr_t)a->D & 15u) == 0;
        if (a->F == kSpecF) launch_desc<kSpecF>(p, tokens, vec4, nblocks, st);
        else launch_desc<0>(p, tokens, vec4, nblocks, st);
    }
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

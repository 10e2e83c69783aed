// retrieval.hip -- ASMK loop-closure retrieval on the device (gfx950).
//
// Replaces RetrievalDatabase.update of the reference (mast3r_slam/retrieval_database.py:43-166)
// from the prepared local features on: quantise against the codebook, aggregate the residuals
// per visual word into binary codes, score every stored image, add the image to the store.
//
//   quantise   [n,D] x [D,K] on the f32-input MFMA (v_mfma_f32_32x32x2_f32) with a running
//              top-ma per feature in registers; the [n,K] distance matrix is never stored.  K is
//              split over workgroups, each writes its partial top-ma, a second launch merges.
//              Ties resolve by the lower centroid index.
//   aggregate  LDS bitonic sort of the (word, feature) pairs, unique words, then per word the
//              reference's f32 sum of (des - centroid) over ascending feature and the sign bits
//              packed MSB first.
//   score      forward file: one wave per stored image intersects its sorted words with the
//              query's, looks the term up in T[hamming] and adds in ascending word order (f64).
//
// Compiled with -ffp-contract=off: every f32 operation of aggregate and score is the reference's
// own, one rounding each; the only fused operations are the MFMA's k-ordered fma chain.
// Launches of one call are ordered by the caller's stream; nothing waits across workgroups.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/m3s_backend.h"
#include "m3s_common.h"

#pragma clang fp contract(off)

namespace m3s {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kQT = 128;        // centroids per tile and features per tile
constexpr int kQK = 32;         // D step of one LDS tile
constexpr int kQLD = kQT + 4;   // LDS row stride in floats
constexpr int kQThreads = 256;  // 4 waves: 2 (centroid halves) x 2 (feature halves)
constexpr int kMaMax = 8;       // largest multiple assignment
constexpr int kSplitMax = 1024;  // most K-splits of one quantise launch
constexpr int kSortMax = 4096;  // (word, feature) pairs one LDS sort holds (32 KiB of keys)
constexpr int kSortThreads = 1024;

// ------------------------------------------------------------------------------------------
// squared norms of rows: one wave per row
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ x, int64_t rows,
                                                       int D, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = x + r * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float v = p[k];
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[r] = s;
}

// ------------------------------------------------------------------------------------------
// quantise: MFMA distance tiles with a fused running top-MA
// ------------------------------------------------------------------------------------------

// Insert (d, c) into an ascending list; equal distances keep the earlier entry first.  The caller
// feeds one list ascending c, so this is the (distance, index) order.
template <int MA>
__device__ __forceinline__ void topk_insert(float (&td)[MA], int (&ti)[MA], float d, int c) {
    if (d < td[MA - 1]) {
        td[MA - 1] = d;
        ti[MA - 1] = c;
#pragma unroll
        for (int p = MA - 1; p >= 1; --p) {
            if (td[p] < td[p - 1]) {
                const float fd = td[p];
                td[p] = td[p - 1];
                td[p - 1] = fd;
                const int fi = ti[p];
                ti[p] = ti[p - 1];
                ti[p - 1] = fi;
            }
        }
    }
}

// The same for candidates in any order: (distance, index) lexicographic.
template <int MA>
__device__ __forceinline__ void topk_insert_lex(float (&td)[MA], int (&ti)[MA], float d, int c) {
    if (d < td[MA - 1] || (d == td[MA - 1] && c < ti[MA - 1])) {
        td[MA - 1] = d;
        ti[MA - 1] = c;
#pragma unroll
        for (int p = MA - 1; p >= 1; --p) {
            if (td[p] < td[p - 1] || (td[p] == td[p - 1] && ti[p] < ti[p - 1])) {
                const float fd = td[p];
                td[p] = td[p - 1];
                td[p - 1] = fd;
                const int fi = ti[p];
                ti[p] = ti[p - 1];
                ti[p - 1] = fi;
            }
        }
    }
}

// 16 floats of one [128 rows x 32 k] tile per thread, zero beyond `rows` and D.
template <bool VEC>
__device__ __forceinline__ void load_tile(const float* __restrict__ src, int64_t row0, int64_t rows,
                                          int D, int k0, int t, float (&r)[16]) {
    if (VEC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + kQThreads * q;
            const int row = e >> 3, k = k0 + (e & 7) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + row < rows && k < D)
                v = *reinterpret_cast<const float4*>(src + (row0 + row) * D + k);
            r[4 * q] = v.x;
            r[4 * q + 1] = v.y;
            r[4 * q + 2] = v.z;
            r[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = t + kQThreads * q;
            const int row = e >> 5, k = k0 + (e & 31);
            r[q] = (row0 + row < rows && k < D) ? src[(row0 + row) * D + k] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_tile(float* __restrict__ dst, int t, const float (&r)[16]) {
    if (VEC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + kQThreads * q;
            const int row = e >> 3, k = (e & 7) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(k + j) * kQLD + row] = r[4 * q + j];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = t + kQThreads * q;
            dst[(e & 31) * kQLD + (e >> 5)] = r[q];
        }
    }
}

// grid (nsplit, feature tiles).  Workgroup (s, y) scans centroid tiles [s*tps, (s+1)*tps) for
// features [128 y, 128 y + 128) and writes MA (distance, index) pairs per feature to
// part[(f * nsplit + s) * MA ..].  A = centroids (rows, in the accumulator's registers),
// B = features (columns, on the lanes): a lane's 16 results of one accumulator belong to ONE
// feature, so the running top-MA needs no cross-lane step until the end.
template <int MA, bool VEC>
__global__ __launch_bounds__(kQThreads, 2) void quantize_tile_kernel(
    const float* __restrict__ feat, const float* __restrict__ cent, const float* __restrict__ qn,
    const float* __restrict__ cn, int n, int64_t K, int D, int tiles_c, int tps, int nsplit,
    float* __restrict__ part_d, int* __restrict__ part_i) {
    __shared__ float smem[2 * kQK * kQLD + kQT];
    static_assert(2 * kQT * 4 * kMaMax <= 2 * kQK * kQLD, "candidate lists reuse the tile LDS");
    float* As = smem;
    float* Bs = smem + kQK * kQLD;
    float* cns = smem + 2 * kQK * kQLD;

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int split = blockIdx.x;
    const int64_t f0 = (int64_t)blockIdx.y * kQT;
    const int t0 = split * tps;
    const int t1 = t0 + tps < tiles_c ? t0 + tps : tiles_c;
    const int ksteps = (D + kQK - 1) / kQK;
    const int S = (t1 - t0) * ksteps;

    float td[2][MA];
    int ti[2][MA];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < MA; ++p) {
            td[j][p] = INFINITY;
            ti[j][p] = INT_MAX;
        }
    float qnv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t f = f0 + wn * 64 + j * 32 + li;
        qnv[j] = f < n ? qn[f] : 0.f;
    }

    f32x16 acc[2][2];
    float ra[16], rb[16];
    if (S > 0) {
        load_tile<VEC>(cent, (int64_t)t0 * kQT, K, D, 0, t, ra);
        load_tile<VEC>(feat, f0, n, D, 0, t, rb);
    }
    for (int s = 0; s < S; ++s) {
        const int tile = t0 + s / ksteps;
        const int kt = s - (s / ksteps) * ksteps;
        __syncthreads();
        store_tile<VEC>(As, t, ra);
        store_tile<VEC>(Bs, t, rb);
        if (kt == 0 && t < kQT) {
            const int64_t c = (int64_t)tile * kQT + t;
            cns[t] = c < K ? cn[c] : 0.f;
        }
        __syncthreads();
        if (s + 1 < S) {
            const int s1 = s + 1;
            const int tile1 = t0 + s1 / ksteps;
            const int kt1 = s1 - (s1 / ksteps) * ksteps;
            load_tile<VEC>(cent, (int64_t)tile1 * kQT, K, D, kt1 * kQK, t, ra);
            load_tile<VEC>(feat, f0, n, D, kt1 * kQK, t, rb);
        }
        if (kt == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < kQK / 2; ++kk) {
            const int k = 2 * kk + lh;
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[k * kQLD + wm * 64 + i * 32 + li];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[k * kQLD + wn * 64 + j * 32 + li];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt == ksteps - 1) {
            // accumulator register r of lane (li, lh): row (r&3) + 8 (r>>2) + 4 lh, column li
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int crow = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int64_t c = (int64_t)tile * kQT + crow;
                    const float cnv = cns[crow];
                    if (c < K) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            // the reference's expansion |q|^2 + |c|^2 - 2 q.c; NaN and +inf rank
                            // last among real candidates, by index
                            float d = (qnv[j] + cnv) - 2.f * acc[i][j][r];
                            d = fminf(d, FLT_MAX);
                            topk_insert<MA>(td[j], ti[j], d, (int)c);
                        }
                    }
                }
        }
    }

    // the 4 lists of one feature (2 centroid halves x 2 lane halves) -> one
    __syncthreads();
    float* cand_d = smem;
    int* cand_i = reinterpret_cast<int*>(smem + kQT * 4 * MA);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int fl = wn * 64 + j * 32 + li;
        const int slot = wm * 2 + lh;
#pragma unroll
        for (int p = 0; p < MA; ++p) {
            cand_d[(fl * 4 + slot) * MA + p] = td[j][p];
            cand_i[(fl * 4 + slot) * MA + p] = ti[j][p];
        }
    }
    __syncthreads();
    if (t < kQT && f0 + t < n) {
        float md[MA];
        int mi[MA];
#pragma unroll
        for (int p = 0; p < MA; ++p) {
            md[p] = INFINITY;
            mi[p] = INT_MAX;
        }
        for (int e = 0; e < 4 * MA; ++e)
            topk_insert_lex<MA>(md, mi, cand_d[t * 4 * MA + e], cand_i[t * 4 * MA + e]);
        const int64_t o = ((f0 + t) * nsplit + split) * MA;
#pragma unroll
        for (int p = 0; p < MA; ++p) {
            part_d[o + p] = md[p];
            part_i[o + p] = mi[p];
        }
    }
}

// One wave per feature merges its nsplit*MAs partial pairs: lane-local lists, then `ma` rounds
// of a wave-wide (distance, index) minimum.
__global__ __launch_bounds__(64) void quantize_merge_kernel(const float* __restrict__ part_d,
                                                            const int* __restrict__ part_i,
                                                            int ncand, int ma, int64_t K,
                                                            int* __restrict__ ids, int ids_stride) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    float md[kMaMax];
    int mi[kMaMax];
#pragma unroll
    for (int p = 0; p < kMaMax; ++p) {
        md[p] = INFINITY;
        mi[p] = INT_MAX;
    }
    for (int e = lane; e < ncand; e += 64)
        topk_insert_lex<kMaMax>(md, mi, part_d[f * ncand + e], part_i[f * ncand + e]);
    for (int r = 0; r < ma; ++r) {
        float bd = md[0];
        int bi = mi[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float od = __shfl_xor(bd, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) {
                bd = od;
                bi = oi;
            }
        }
        if (mi[0] == bi && bi != INT_MAX) {  // indices are unique: one lane pops
#pragma unroll
            for (int p = 0; p + 1 < kMaMax; ++p) {
                md[p] = md[p + 1];
                mi[p] = mi[p + 1];
            }
            md[kMaMax - 1] = INFINITY;
            mi[kMaMax - 1] = INT_MAX;
        }
        if (lane == 0) ids[f * ids_stride + r] = bi < K ? bi : (int)(K - 1);
    }
}

// ------------------------------------------------------------------------------------------
// aggregate
// ------------------------------------------------------------------------------------------

// One workgroup: sort the (word, feature) pairs of ids[:, :ma] (row stride ids_stride), find the
// unique words.  Out: words [<= n*ma] ascending, *count, seg [count+1] (each word's first sorted
// pair, then the number of valid pairs), sorted_f [n*ma] the pairs' features.
__global__ __launch_bounds__(kSortThreads) void aggregate_sort_kernel(
    const int* __restrict__ ids, int ids_stride, int n, int ma, int64_t K, int P,
    int* __restrict__ words, int* __restrict__ count, int* __restrict__ seg,
    int* __restrict__ sorted_f) {
    extern __shared__ unsigned long long keys[];
    __shared__ int sc[kSortThreads];
    const int t = threadIdx.x;
    const int npair = n * ma;
    const unsigned long long kInvalid = ~0ull;
    for (int i = t; i < P; i += kSortThreads) {
        unsigned long long key = kInvalid;
        if (i < npair) {
            const int f = i / ma, c = i - f * ma;
            const int id = ids[(int64_t)f * ids_stride + c];
            if (id >= 0 && id < K) key = ((unsigned long long)(unsigned)id << 32) | (unsigned)f;
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += kSortThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // each thread owns a contiguous run of the sorted pairs
    const int per = (P + kSortThreads - 1) / kSortThreads;
    const int i0 = t * per < P ? t * per : P;
    const int i1 = i0 + per < P ? i0 + per : P;
    int heads = 0;
    for (int i = i0; i < i1; ++i) {
        const unsigned long long key = keys[i];
        if (key != kInvalid && (i == 0 || (keys[i - 1] >> 32) != (key >> 32))) ++heads;
    }
    sc[t] = heads;
    __syncthreads();
    for (int off = 1; off < kSortThreads; off <<= 1) {
        const int v = t >= off ? sc[t - off] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    const int total = sc[kSortThreads - 1];
    int u = sc[t] - heads;
    for (int i = i0; i < i1; ++i) {
        const unsigned long long key = keys[i];
        if (key == kInvalid) continue;
        if (i == 0 || (keys[i - 1] >> 32) != (key >> 32)) {
            words[u] = (int)(key >> 32);
            seg[u] = i;
            ++u;
        }
        sorted_f[i] = (int)(key & 0xffffffffu);
        if (i + 1 == P || keys[i + 1] == kInvalid) seg[total] = i + 1;
    }
    if (t == 0) {
        *count = total;
        if (keys[0] == kInvalid) seg[0] = 0;
    }
}

// One workgroup per unique word, one wave per 64 components: the reference's f32 sum of
// (des[f] - centroid[w]) over ascending f, then sign bits packed MSB first.
__global__ __launch_bounds__(256) void aggregate_pack_kernel(
    const float* __restrict__ feat, const float* __restrict__ cent, int D, int W,
    const int* __restrict__ words, const int* __restrict__ count, const int* __restrict__ seg,
    const int* __restrict__ sorted_f, uint32_t* __restrict__ codes) {
    const int u = blockIdx.x;
    if (u >= *count) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t word = words[u];
    const int s0 = seg[u], s1 = seg[u + 1];
    for (int chunk = wave; chunk * 64 < D; chunk += nw) {
        const int comp = chunk * 64 + lane;
        const bool in = comp < D;
        const float cv = in ? cent[word * D + comp] : 0.f;
        float acc = 0.f;
        int prev = -1;
        for (int s = s0; s < s1; ++s) {
            const int f = sorted_f[s];
            if (f == prev) continue;  // a feature lists a word once
            const float v = (in ? feat[(int64_t)f * D + comp] : 0.f) - cv;
            acc = prev < 0 ? v : acc + v;
            prev = f;
        }
        const unsigned long long mask = __ballot(in && acc > 0.f);
        if (lane == 0) {
            codes[(int64_t)u * W + 2 * chunk] = __brev((unsigned)(mask & 0xffffffffu));
            if (2 * chunk + 1 < W) codes[(int64_t)u * W + 2 * chunk + 1] = __brev((unsigned)(mask >> 32));
        }
    }
}

// ------------------------------------------------------------------------------------------
// score
// ------------------------------------------------------------------------------------------

// One wave per stored image.  sqrt_d[c] = sqrt((double)c), sqrt_f[c] = (double)sqrtf((float)c),
// both from the host.
__global__ __launch_bounds__(64) void score_kernel(
    const int* __restrict__ q_words, const uint32_t* __restrict__ q_codes,
    const int* __restrict__ q_count, const int* __restrict__ db_words,
    const uint32_t* __restrict__ db_codes, const int* __restrict__ db_nwords, int row, int W,
    const float* __restrict__ table, const double* __restrict__ sqrt_d,
    const double* __restrict__ sqrt_f, double* __restrict__ scores) {
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x;
    const int nq = *q_count;
    const int nm = db_nwords[m];
    const int* mw = db_words + m * row;
    const uint32_t* mc = db_codes + m * (int64_t)row * W;
    const double norm = sqrt_d[nm];
    double sum = 0.0;
    for (int base = 0; base < nm; base += 64) {
        const int i = base + lane;
        float term = 0.f;
        bool hit = false;
        if (i < nm) {
            const int word = mw[i];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (q_words[mid] < word) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && q_words[lo] == word) {
                int h = 0;
                for (int j = 0; j < W; ++j)
                    h += __popc(q_codes[(int64_t)lo * W + j] ^ mc[(int64_t)i * W + j]);
                term = (float)((double)table[h] / norm);
                hit = true;
            }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {  // ascending word order
            const int l = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            sum += (double)__shfl(term, l, 64);
        }
    }
    if (lane == 0) scores[m] = sum / sqrt_f[nq];
}

// ------------------------------------------------------------------------------------------
// the database object
// ------------------------------------------------------------------------------------------

struct RetrievalDb {
    const float* cent = nullptr;  // [K,D], borrowed
    int64_t K = 0;
    int D = 0, W = 0;
    int ma_build = 1, ma_query = 5, ma_max = 5;
    int max_feat = 0;
    int row = 0;  // words one stored image can hold: max_feat * ma_build
    int device = 0;
    int ncu = 256;
    float* cn = nullptr;      // [K]
    float* qn = nullptr;      // [max_feat]
    float* part_d = nullptr;  // quantise partials
    int* part_i = nullptr;
    int64_t part_rows = 0;
    float* table = nullptr;   // [32W+1]
    double* sqrt_d = nullptr; // [max_feat*ma_max+1]
    double* sqrt_f = nullptr;
    int* q_ids = nullptr;     // [max_feat, ma_max]
    int* q_words = nullptr;   // [max_feat*ma_max]
    uint32_t* q_codes = nullptr;
    int* q_count = nullptr;
    int* seg = nullptr;       // [max_feat*ma_max+1]
    int* sorted_f = nullptr;  // [max_feat*ma_max]
    // forward file
    int64_t n_images = 0, cap = 0;
    int* db_words = nullptr;       // [cap, row]
    uint32_t* db_codes = nullptr;  // [cap, row, W]
    int* db_nwords = nullptr;      // [cap]
    // the last query's ids, for an add that reuses them
    int64_t last_n = -1;
    const float* last_feat = nullptr;
};

void free_db(RetrievalDb* db) {
    void* ptrs[] = {db->cn, db->qn, db->part_d, db->part_i, db->table, db->sqrt_d, db->sqrt_f,
                    db->q_ids, db->q_words, db->q_codes, db->q_count, db->seg, db->sorted_f,
                    db->db_words, db->db_codes, db->db_nwords};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete db;
}

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

int grow_store(RetrievalDb* db, int64_t want, hipStream_t st) {
    if (want <= db->cap) return M3S_OK;
    int64_t cap = db->cap > 0 ? db->cap : 16;
    while (cap < want) cap *= 2;
    const size_t wrow = (size_t)db->row, crow = (size_t)db->row * db->W;
    int* nw = nullptr;
    uint32_t* nc = nullptr;
    int* nn = nullptr;
    M3S_HIP_CHECK(hipMalloc(&nw, sizeof(int) * wrow * cap));
    M3S_HIP_CHECK(hipMalloc(&nc, sizeof(uint32_t) * crow * cap));
    M3S_HIP_CHECK(hipMalloc(&nn, sizeof(int) * cap));
    M3S_HIP_CHECK(hipMemsetAsync(nw, 0, sizeof(int) * wrow * cap, st));
    M3S_HIP_CHECK(hipMemsetAsync(nc, 0, sizeof(uint32_t) * crow * cap, st));
    M3S_HIP_CHECK(hipMemsetAsync(nn, 0, sizeof(int) * cap, st));
    if (db->n_images > 0) {
        const size_t k = (size_t)db->n_images;
        M3S_HIP_CHECK(hipMemcpyAsync(nw, db->db_words, sizeof(int) * wrow * k, hipMemcpyDeviceToDevice, st));
        M3S_HIP_CHECK(hipMemcpyAsync(nc, db->db_codes, sizeof(uint32_t) * crow * k, hipMemcpyDeviceToDevice, st));
        M3S_HIP_CHECK(hipMemcpyAsync(nn, db->db_nwords, sizeof(int) * k, hipMemcpyDeviceToDevice, st));
    }
    // the old buffers may still be read by work queued on the stream
    M3S_HIP_CHECK(hipStreamSynchronize(st));
    if (db->db_words) (void)hipFree(db->db_words);
    if (db->db_codes) (void)hipFree(db->db_codes);
    if (db->db_nwords) (void)hipFree(db->db_nwords);
    db->db_words = nw;
    db->db_codes = nc;
    db->db_nwords = nn;
    db->cap = cap;
    return M3S_OK;
}

template <int MA>
void launch_quantize_tiles(bool vec, dim3 grid, hipStream_t st, const float* feat, const float* cent,
                           const float* qn, const float* cn, int n, int64_t K, int D, int tiles_c,
                           int tps, int nsplit, float* pd, int* pi) {
    if (vec)
        hipLaunchKernelGGL((quantize_tile_kernel<MA, true>), grid, dim3(kQThreads), 0, st, feat, cent,
                           qn, cn, n, K, D, tiles_c, tps, nsplit, pd, pi);
    else
        hipLaunchKernelGGL((quantize_tile_kernel<MA, false>), grid, dim3(kQThreads), 0, st, feat, cent,
                           qn, cn, n, K, D, tiles_c, tps, nsplit, pd, pi);
}

int do_quantize(RetrievalDb* db, const float* feat, int n, int ma, int* ids, int ids_stride,
                hipStream_t st) {
    hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, feat,
                       (int64_t)n, db->D, db->qn);
    M3S_LAUNCH_CHECK();
    const int tiles_c = (int)((db->K + kQT - 1) / kQT);
    const int mtiles = (n + kQT - 1) / kQT;
    // Tiles per workgroup: the fewest tiles the busiest CU gets (the stage is MFMA-bound, so a
    // CU's time is its tile count), and among equals the larger run -- fewer partial lists.
    const int64_t cap_split = db->part_rows / n < kSplitMax ? db->part_rows / n : kSplitMax;
    int tps_min = (int)((tiles_c + cap_split - 1) / cap_split);
    int tps = tiles_c;
    int64_t best = INT64_MAX;
    for (int c = tps_min; c < tps_min + 16 && c <= tiles_c; ++c) {
        const int64_t wgs = (int64_t)((tiles_c + c - 1) / c) * mtiles;
        const int64_t span = (wgs + db->ncu - 1) / db->ncu * c;
        if (span <= best) {
            best = span;
            tps = c;
        }
    }
    const int nsplit = (tiles_c + tps - 1) / tps;
    const int MA = ma == 1 ? 1 : (ma <= 5 ? 5 : kMaMax);
    M3S_REQUIRE((int64_t)n * nsplit <= db->part_rows, "retrieval_quantize: partial buffer too small");
    const bool vec = db->D % 4 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(db->cent) & 15) == 0;
    const dim3 grid((unsigned)nsplit, (unsigned)mtiles);
    if (MA == 1)
        launch_quantize_tiles<1>(vec, grid, st, feat, db->cent, db->qn, db->cn, n, db->K, db->D,
                                 tiles_c, tps, nsplit, db->part_d, db->part_i);
    else if (MA == 5)
        launch_quantize_tiles<5>(vec, grid, st, feat, db->cent, db->qn, db->cn, n, db->K, db->D,
                                 tiles_c, tps, nsplit, db->part_d, db->part_i);
    else
        launch_quantize_tiles<kMaMax>(vec, grid, st, feat, db->cent, db->qn, db->cn, n, db->K, db->D,
                                      tiles_c, tps, nsplit, db->part_d, db->part_i);
    M3S_LAUNCH_CHECK();
    hipLaunchKernelGGL(quantize_merge_kernel, dim3((unsigned)n), dim3(64), 0, st, db->part_d,
                       db->part_i, nsplit * MA, ma, db->K, ids, ids_stride);
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

int do_aggregate(RetrievalDb* db, const float* feat, const int* ids, int ids_stride, int n, int ma,
                 int* words, uint32_t* codes, int* count, hipStream_t st) {
    const int npair = n * ma;
    int P = 2;
    while (P < npair) P <<= 1;
    M3S_REQUIRE(P <= kSortMax, "retrieval_aggregate: n*ma = %d exceeds the %d pairs of one sort",
                npair, kSortMax);
    hipLaunchKernelGGL(aggregate_sort_kernel, dim3(1), dim3(kSortThreads),
                       sizeof(unsigned long long) * (size_t)P, st, ids, ids_stride, n, ma, db->K, P,
                       words, count, db->seg, db->sorted_f);
    M3S_LAUNCH_CHECK();
    int nw = (db->D + 63) / 64;
    if (nw > 4) nw = 4;
    hipLaunchKernelGGL(aggregate_pack_kernel, dim3((unsigned)npair), dim3(64 * nw), 0, st, feat,
                       db->cent, db->D, db->W, words, count, db->seg, db->sorted_f, codes);
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

int check_feat(const char* what, RetrievalDb* db, const float* feat, int64_t n) {
    M3S_REQUIRE(db != nullptr, "%s: null database", what);
    M3S_REQUIRE(n >= 1 && n <= db->max_feat, "%s: n = %lld outside 1..max_feat = %d", what,
                (long long)n, db->max_feat);
    M3S_REQUIRE(feat != nullptr && is_device_ptr(feat), "%s: feat is not a device pointer", what);
    return M3S_OK;
}

}  // namespace
}  // namespace m3s

using m3s::RetrievalDb;

extern "C" int m3s_retrieval_term_table(int64_t D, float alpha, float sim_thresh, float* table_out) {
    // the reference's f32 steps up to sim (hamming.pyx:34-42, kernel.py:62-63, functional.py:13),
    // then the f32 rounding of the double power
    M3S_REQUIRE(D >= 1 && D <= 4096 && table_out, "retrieval_term_table: bad argument");
    const int nbits = 32 * (int)((D + 31) / 32);
    for (int h = 0; h <= nbits; ++h) {
        const float nh = (float)h / (float)nbits;
        const float sim = -2.f * nh + 1.f;
        table_out[h] = sim < sim_thresh ? 0.f : (float)std::pow((double)sim, (double)alpha);
    }
    return M3S_OK;
}

extern "C" int m3s_retrieval_create(const float* centroids, int64_t K, int64_t D, int ma_build,
                                    int ma_query, float alpha, float sim_thresh,
                                    const float* table_or_null, int64_t max_feat, void** db_out) {
    M3S_REQUIRE(db_out != nullptr, "retrieval_create: null output");
    *db_out = nullptr;
    M3S_REQUIRE(D >= 1 && D <= 4096, "retrieval_create: D = %lld outside 1..4096", (long long)D);
    M3S_REQUIRE(ma_build >= 1 && ma_query >= 1 && ma_build <= m3s::kMaMax && ma_query <= m3s::kMaMax,
                "retrieval_create: multiple assignment outside 1..%d", m3s::kMaMax);
    M3S_REQUIRE(ma_build <= ma_query,
                "retrieval_create: the build's multiple assignment must not exceed the query's");
    const int ma_max = ma_query;
    M3S_REQUIRE(K >= ma_max && K < ((int64_t)1 << 31) - m3s::kQT,
                "retrieval_create: K = %lld must be >= the multiple assignment (%d) and < 2^31",
                (long long)K, ma_max);
    M3S_REQUIRE(max_feat >= 1 && max_feat * ma_max <= m3s::kSortMax,
                "retrieval_create: max_feat * multiple assignment = %lld outside 1..%d",
                (long long)(max_feat * ma_max), m3s::kSortMax);
    M3S_REQUIRE(centroids != nullptr && m3s::is_device_ptr(centroids),
                "retrieval_create: centroids is not a device pointer");
    RetrievalDb* db = new RetrievalDb();
    db->cent = centroids;
    db->K = K;
    db->D = (int)D;
    db->W = (int)((D + 31) / 32);
    db->ma_build = ma_build;
    db->ma_query = ma_query;
    db->ma_max = ma_max;
    db->max_feat = (int)max_feat;
    db->row = (int)max_feat * ma_build;
    const int nbits = 32 * db->W;
    const size_t npair = (size_t)max_feat * ma_max;
    db->part_rows = (int64_t)m3s::kQT * m3s::kSplitMax + max_feat;
    // the term table T[h] unless the caller brings its own
    std::vector<float> T(nbits + 1);
    m3s_retrieval_term_table(D, alpha, sim_thresh, T.data());
    std::vector<double> sd(npair + 1), sf(npair + 1);
    for (size_t c = 0; c <= npair; ++c) {
        sd[c] = std::sqrt((double)c);
        sf[c] = (double)std::sqrt((float)c);
    }
#define M3S_DB_CHECK(expr)                                                                  \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            m3s::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                       \
            m3s::free_db(db);                                                               \
            return M3S_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)
    M3S_DB_CHECK(hipGetDevice(&db->device));
    M3S_DB_CHECK(hipDeviceGetAttribute(&db->ncu, hipDeviceAttributeMultiprocessorCount, db->device));
    if (db->ncu < 1) db->ncu = 1;
    M3S_DB_CHECK(hipMalloc(&db->cn, sizeof(float) * (size_t)K));
    M3S_DB_CHECK(hipMalloc(&db->qn, sizeof(float) * (size_t)max_feat));
    M3S_DB_CHECK(hipMalloc(&db->part_d, sizeof(float) * (size_t)db->part_rows * m3s::kMaMax));
    M3S_DB_CHECK(hipMalloc(&db->part_i, sizeof(int) * (size_t)db->part_rows * m3s::kMaMax));
    M3S_DB_CHECK(hipMalloc(&db->table, sizeof(float) * (nbits + 1)));
    M3S_DB_CHECK(hipMalloc(&db->sqrt_d, sizeof(double) * (npair + 1)));
    M3S_DB_CHECK(hipMalloc(&db->sqrt_f, sizeof(double) * (npair + 1)));
    M3S_DB_CHECK(hipMalloc(&db->q_ids, sizeof(int) * npair));
    M3S_DB_CHECK(hipMalloc(&db->q_words, sizeof(int) * npair));
    M3S_DB_CHECK(hipMalloc(&db->q_codes, sizeof(uint32_t) * npair * db->W));
    M3S_DB_CHECK(hipMalloc(&db->q_count, sizeof(int)));
    M3S_DB_CHECK(hipMalloc(&db->seg, sizeof(int) * (npair + 1)));
    M3S_DB_CHECK(hipMalloc(&db->sorted_f, sizeof(int) * npair));
    M3S_DB_CHECK(hipMemset(db->q_count, 0, sizeof(int)));
    if (table_or_null) {
        M3S_DB_CHECK(hipMemcpy(db->table, table_or_null, sizeof(float) * (nbits + 1), hipMemcpyDefault));
    } else {
        M3S_DB_CHECK(hipMemcpy(db->table, T.data(), sizeof(float) * (nbits + 1), hipMemcpyHostToDevice));
    }
    M3S_DB_CHECK(hipMemcpy(db->sqrt_d, sd.data(), sizeof(double) * (npair + 1), hipMemcpyHostToDevice));
    M3S_DB_CHECK(hipMemcpy(db->sqrt_f, sf.data(), sizeof(double) * (npair + 1), hipMemcpyHostToDevice));
    // |c|^2 once
    hipLaunchKernelGGL(m3s::row_norm_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, 0, centroids,
                       K, db->D, db->cn);
    M3S_DB_CHECK(hipGetLastError());
    M3S_DB_CHECK(hipStreamSynchronize(0));
#undef M3S_DB_CHECK
    *db_out = db;
    return M3S_OK;
}

extern "C" int m3s_retrieval_destroy(void* dbv) {
    if (!dbv) return M3S_OK;
    m3s::free_db(static_cast<RetrievalDb*>(dbv));
    return M3S_OK;
}

extern "C" int m3s_retrieval_size(void* dbv, int64_t* n_images) {
    M3S_REQUIRE(dbv && n_images, "retrieval_size: null argument");
    *n_images = static_cast<RetrievalDb*>(dbv)->n_images;
    return M3S_OK;
}

extern "C" int m3s_retrieval_quantize(void* dbv, const float* feat, int64_t n, int ma, int32_t* ids_out,
                                      void* stream) {
    RetrievalDb* db = static_cast<RetrievalDb*>(dbv);
    if (int rc = m3s::check_feat("retrieval_quantize", db, feat, n)) return rc;
    M3S_REQUIRE(ma >= 1 && ma <= m3s::kMaMax && ma <= db->K, "retrieval_quantize: ma = %d outside 1..%d",
                ma, m3s::kMaMax);
    M3S_REQUIRE(ids_out && m3s::is_device_ptr(ids_out), "retrieval_quantize: ids_out is not a device pointer");
    return m3s::do_quantize(db, feat, (int)n, ma, ids_out, ma, (hipStream_t)stream);
}

extern "C" int m3s_retrieval_aggregate(void* dbv, const float* feat, const int32_t* ids, int64_t n,
                                       int ma, int32_t* words_out, uint32_t* codes_out,
                                       int32_t* n_words_out, void* stream) {
    RetrievalDb* db = static_cast<RetrievalDb*>(dbv);
    if (int rc = m3s::check_feat("retrieval_aggregate", db, feat, n)) return rc;
    M3S_REQUIRE(ma >= 1 && ma <= db->ma_max, "retrieval_aggregate: ma = %d outside 1..%d", ma, db->ma_max);
    M3S_REQUIRE(ids && words_out && codes_out && n_words_out && m3s::is_device_ptr(ids) &&
                    m3s::is_device_ptr(words_out) && m3s::is_device_ptr(codes_out) &&
                    m3s::is_device_ptr(n_words_out),
                "retrieval_aggregate: ids / outputs must be device pointers");
    return m3s::do_aggregate(db, feat, ids, ma, (int)n, ma, words_out, codes_out, n_words_out,
                             (hipStream_t)stream);
}

extern "C" int m3s_retrieval_query(void* dbv, const float* feat, int64_t n, double* scores_out,
                                   void* stream) {
    RetrievalDb* db = static_cast<RetrievalDb*>(dbv);
    if (int rc = m3s::check_feat("retrieval_query", db, feat, n)) return rc;
    M3S_REQUIRE(db->n_images == 0 || (scores_out && m3s::is_device_ptr(scores_out)),
                "retrieval_query: scores_out is not a device pointer");
    hipStream_t st = (hipStream_t)stream;
    db->last_n = -1;
    if (int rc = m3s::do_quantize(db, feat, (int)n, db->ma_query, db->q_ids, db->ma_query, st)) return rc;
    if (int rc = m3s::do_aggregate(db, feat, db->q_ids, db->ma_query, (int)n, db->ma_query, db->q_words,
                                   db->q_codes, db->q_count, st))
        return rc;
    db->last_n = n;
    db->last_feat = feat;
    if (db->n_images == 0) return M3S_OK;
    hipLaunchKernelGGL(m3s::score_kernel, dim3((unsigned)db->n_images), dim3(64), 0, st, db->q_words,
                       db->q_codes, db->q_count, db->db_words, db->db_codes, db->db_nwords,
                       db->row, db->W, db->table, db->sqrt_d, db->sqrt_f, scores_out);
    M3S_LAUNCH_CHECK();
    return M3S_OK;
}

extern "C" int m3s_retrieval_add(void* dbv, const float* feat, int64_t n, int reuse_last_query,
                                 void* stream) {
    RetrievalDb* db = static_cast<RetrievalDb*>(dbv);
    if (int rc = m3s::check_feat("retrieval_add", db, feat, n)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int stride = db->ma_build;
    if (reuse_last_query) {
        M3S_REQUIRE(db->last_n == n && db->last_feat == feat,
                    "retrieval_add: reuse_last_query needs a preceding query of the same features");
        stride = db->ma_query;  // the nearest ma_build of the query's ids
    } else {
        db->last_n = -1;
        if (int rc = m3s::do_quantize(db, feat, (int)n, db->ma_build, db->q_ids, stride, st)) return rc;
    }
    if (int rc = m3s::grow_store(db, db->n_images + 1, st)) return rc;
    const int64_t m = db->n_images;
    if (int rc = m3s::do_aggregate(db, feat, db->q_ids, stride, (int)n, db->ma_build,
                                   db->db_words + m * db->row,
                                   db->db_codes + m * (int64_t)db->row * db->W, db->db_nwords + m, st))
        return rc;
    db->last_n = -1;
    db->n_images = m + 1;
    return M3S_OK;
}

extern "C" int m3s_retrieval_image(void* dbv, int64_t m, int32_t* words_out, uint32_t* codes_out,
                                   int32_t* n_words_out, void* stream) {
    RetrievalDb* db = static_cast<RetrievalDb*>(dbv);
    M3S_REQUIRE(db != nullptr, "retrieval_image: null database");
    M3S_REQUIRE(m >= 0 && m < db->n_images, "retrieval_image: image %lld outside 0..%lld", (long long)m,
                (long long)db->n_images - 1);
    M3S_REQUIRE(words_out && codes_out && n_words_out && m3s::is_device_ptr(words_out) &&
                    m3s::is_device_ptr(codes_out) && m3s::is_device_ptr(n_words_out),
                "retrieval_image: outputs must be device pointers");
    hipStream_t st = (hipStream_t)stream;
    const size_t wrow = (size_t)db->row, crow = (size_t)db->row * db->W;
    M3S_HIP_CHECK(hipMemcpyAsync(words_out, db->db_words + m * wrow, sizeof(int) * wrow,
                                 hipMemcpyDeviceToDevice, st));
    M3S_HIP_CHECK(hipMemcpyAsync(codes_out, db->db_codes + m * crow, sizeof(uint32_t) * crow,
                                 hipMemcpyDeviceToDevice, st));
    M3S_HIP_CHECK(hipMemcpyAsync(n_words_out, db->db_nwords + m, sizeof(int), hipMemcpyDeviceToDevice, st));
    return M3S_OK;
}

// RICE retrieval (ref:icv_src/utils/mm_topk_retriver.py: CLIP features -> faiss.IndexFlatIP.search): the exact flat inner-product
// search with the top-k fused into the tile loop, the row normalisation that feeds it, and CLIP's QuickGELU.
//
// licv_topk_ip.  Scores are exact fp32 (v_mfma_f32_32x32x2_f32: a chain of fp32 FMAs, one rounding per product).  The sum over d runs
// in ONE fixed order for every (query, index row) pair - groups of four in order, inside a group d0, d2, d1, d3 (the two halves of a
// wave feed the two k slots of the instruction) - and nothing else enters it, so a pair's score is the same bits wherever the index
// row sits and however Q and N are tiled.  A workgroup (4 waves) owns 128 queries x one chunk of index rows; wave w owns queries
// 32w..32w+31 and keeps, per query, a sorted list of the best 64 (key, index) entries in LDS.  A score reaches the list only when it
// is above the query's current k-th best (one v_cmp per score, a ballot per accumulator register); after the first few tiles
// almost none is.  Per (query, chunk) the k best entries go to the workspace; topk_merge_k merges the chunks in chunk order.
// Entries are ordered by one 64-bit key: (monotone image of the score) << 32 | (0xffffffff - index), larger = better, so equal scores
// resolve to the lowest index and the result does not depend on the order in which candidates arrive.  No atomics.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int TK_THREADS = 256;      // 4 waves
constexpr int TK_QT = 128;           // queries per workgroup (32 per wave)
constexpr int TK_NT = 128;           // index rows per tile (4 accumulators of 32 x 32 per wave)
constexpr int TK_DK = 32;            // d per LDS stage
constexpr int TK_LD = TK_DK + 2;     // LDS row stride in floats: 8-byte reads of 32 consecutive rows fall on distinct bank pairs
constexpr int TK_SLOTS = 64;         // list length kept per query (k <= 64)
constexpr int TK_CUS = 256;          // MI355X
constexpr int TK_MAX_CHUNKS = 128;

typedef unsigned long long u64;

// monotone 32-bit image of an fp32 score, larger = better: -0 counts as +0, NaN is below every number (below -inf)
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0u;
    const int32_t b = __float_as_int(s + 0.0f);
    return (uint32_t)(b ^ ((b >> 31) & 0x7fffffff)) ^ 0x80000000u;
}
__device__ __forceinline__ float key_score(uint32_t k) {
    if (k == 0u) return __int_as_float(0x7fc00000);
    const int32_t b = (int32_t)(k ^ 0x80000000u);
    return __int_as_float(b ^ ((b >> 31) & 0x7fffffff));
}
__device__ __forceinline__ u64 make_entry(float s, uint32_t idx) { return ((u64)score_key(s) << 32) | (u64)(0xffffffffu - idx); }

// lane l <- lane l - 1 over the whole wave (DPP wave_shr:1; lane 0 keeps its own value, which list_insert never uses)
__device__ __forceinline__ u64 shfl_up1(u64 v) {
    const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(uint32_t)(v >> 32), (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, false);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ u64 read_lane(u64 v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// One sorted list (descending) of 64 entries lives one entry per lane; empty slots are 0, below every real entry.  Returns the list
// with `cand` inserted (the last entry falls off); entries are distinct, so the result is independent of the insertion order.
__device__ __forceinline__ u64 list_insert(u64 mine, u64 cand, int lane) {
    const int pos = __popcll(__ballot(mine > cand));          // entries ahead of the candidate: a prefix of the lanes
    const u64 prev = shfl_up1(mine);
    return lane < pos ? mine : (lane == pos ? cand : prev);
}

struct TopkPlan { int64_t q_tiles, chunks, chunk_len; };

TopkPlan topk_plan(int64_t Q, int64_t N) {
    TopkPlan p;
    p.q_tiles = (Q + TK_QT - 1) / TK_QT;
    const int64_t n_tiles = (N + TK_NT - 1) / TK_NT;
    int64_t want = (3 * TK_CUS) / p.q_tiles;                  // about three workgroups per CU over the whole grid
    if (want < 1) want = 1;
    if (want > TK_MAX_CHUNKS) want = TK_MAX_CHUNKS;
    if (want > n_tiles) want = n_tiles;
    const int64_t tiles_per_chunk = (n_tiles + want - 1) / want;
    p.chunk_len = tiles_per_chunk * TK_NT;
    p.chunks = (N + p.chunk_len - 1) / p.chunk_len;
    return p;
}

__global__ __launch_bounds__(TK_THREADS)
void topk_ip_k(const float* __restrict__ qp, int64_t ldq, const float* __restrict__ xp, int64_t ldx, int Q, int N, int D, int k,
               int chunk_len, int chunks, u64* __restrict__ part) {
    __shared__ float As[TK_QT * TK_LD];
    __shared__ float Bs[TK_NT * TK_LD];
    __shared__ u64 lists[TK_QT * TK_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * TK_QT, chunk = blockIdx.y;
    const int n_begin = chunk * chunk_len, n_end = min(N, n_begin + chunk_len);
    const int li = lane & 31, lh = lane >> 5;

    u64* my_lists = lists + wave * 32 * TK_SLOTS;
    for (int i = lane; i < 32 * TK_SLOTS; i += 64) my_lists[i] = 0;      // each wave touches its own lists only: no barrier needed for them
    // k-th best score of the query behind accumulator register r: NaN until the list holds k entries; +inf for rows past Q, whose
    // zero scores then never qualify
    float thr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) thr[r] = q0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh < Q ? __int_as_float(0x7fc00000) : INFINITY;

    // staging: thread -> (row tid/8 + 32 j, float4 column tid%8) of a 128 x 32 stage
    const int s_row = tid >> 3, s_c4 = (tid & 7) * 4;

    for (int n0 = n_begin; n0 < n_end; n0 += TK_NT) {
        floatx16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

        float4 ra[4], rb[4];
        auto fetch = [&](int d0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = s_row + 32 * j, d = d0 + s_c4;
                const int qr = q0 + row, xr = n0 + row;
                ra[j] = (qr < Q && d < D) ? *reinterpret_cast<const float4*>(qp + (int64_t)qr * ldq + d) : float4{0.f, 0.f, 0.f, 0.f};
                rb[j] = (xr < n_end && d < D) ? *reinterpret_cast<const float4*>(xp + (int64_t)xr * ldx + d) : float4{0.f, 0.f, 0.f, 0.f};
            }
        };
        fetch(0);
        for (int d0 = 0; d0 < D; d0 += TK_DK) {
            __syncthreads();                                               // the previous stage has been consumed
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float* a = As + (s_row + 32 * j) * TK_LD + s_c4;
                float* b = Bs + (s_row + 32 * j) * TK_LD + s_c4;
                *reinterpret_cast<float2*>(a) = float2{ra[j].x, ra[j].y};
                *reinterpret_cast<float2*>(a + 2) = float2{ra[j].z, ra[j].w};
                *reinterpret_cast<float2*>(b) = float2{rb[j].x, rb[j].y};
                *reinterpret_cast<float2*>(b + 2) = float2{rb[j].z, rb[j].w};
            }
            __syncthreads();
            if (d0 + TK_DK < D) fetch(d0 + TK_DK);                         // next stage in flight behind this stage's MFMAs
            const int kmax = min(TK_DK, D - d0);                           // D % 4 == 0: whole groups of four
            const float* ar = As + (wave * 32 + li) * TK_LD + 2 * lh;
            const float* br = Bs + li * TK_LD + 2 * lh;
            for (int kk = 0; kk < kmax; kk += 4) {
                const float2 a2 = *reinterpret_cast<const float2*>(ar + kk);
                float2 b2[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) b2[t] = *reinterpret_cast<const float2*>(br + t * 32 * TK_LD + kk);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.x, b2[t].x, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2.y, b2[t].y, acc[t], 0, 0, 0);
            }
        }

        // running top-k: accumulator register r of lane l holds query (r&3) + 8 (r>>2) + 4 (l>>5) of this wave, index row n0 + 32 t + (l&31).
        // A score qualifies when it is ABOVE the query's k-th best before this tile: index rows arrive in ascending order, so an equal
        // score from a later row loses the tie to the entry it equals and can never be among the k.  NaN thresholds compare false.
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            u64 m[4], any = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                m[t] = __ballot(n0 + t * 32 + li < n_end && !(acc[t][r] <= thr[r]));
                any |= m[t];
            }
            if (any) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u64 half = h ? 0xffffffff00000000ull : 0x00000000ffffffffull;
                    if (any & half) {                                      // one query: its list stays in registers for the whole batch
                        u64* L = my_lists + ((r & 3) + 8 * (r >> 2) + 4 * h) * TK_SLOTS;
                        u64 mine = L[lane];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            u64 mm = m[t] & half;
                            if (mm) {
                                const u64 cand_all = make_entry(acc[t][r], (uint32_t)(n0 + t * 32 + li));
                                while (mm) {
                                    const int src = __ffsll((long long)mm) - 1;
                                    mm &= mm - 1;
                                    mine = list_insert(mine, read_lane(cand_all, src), lane);
                                }
                            }
                        }
                        L[lane] = mine;
                        // NaN while fewer than k entries (an empty slot's key reads as NaN) or a NaN in k-th place: everything qualifies
                        const float kth = key_score((uint32_t)(read_lane(mine, k - 1) >> 32));
                        if (lh == h) thr[r] = kth;
                    }
                }
            }
        }
    }

    // this chunk's k best of every query of the wave: part[(q * chunks + chunk) * k + j]
    for (int i = 0; i < 32; ++i) {
        const int q = q0 + wave * 32 + i;
        if (q < Q && lane < k) part[((int64_t)q * chunks + chunk) * k + lane] = my_lists[i * TK_SLOTS + lane];
    }
}

// one wave per query: the chunks' lists (each sorted) merged in chunk order
__global__ __launch_bounds__(64)
void topk_merge_k(const u64* __restrict__ part, int Q, int chunks, int k, int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const u64* p = part + (int64_t)q * chunks * k;
    u64 mine = lane < k ? p[lane] : 0;
    u64 next = (chunks > 1 && lane < k) ? p[k + lane] : 0;
    for (int c = 1; c < chunks; ++c) {
        const u64 theirs = next;
        next = (c + 1 < chunks && lane < k) ? p[(int64_t)(c + 1) * k + lane] : 0;      // in flight behind this chunk's inserts
        for (int j = 0; j < k; ++j) {
            const u64 cand = read_lane(theirs, j);
            if (cand <= read_lane(mine, k - 1)) break;                     // sorted: nothing further down this chunk's list can enter
            mine = list_insert(mine, cand, lane);
        }
    }
    if (lane < k) {
        out_idx[(int64_t)q * k + lane] = (int64_t)(0xffffffffu - (uint32_t)mine);
        out_score[(int64_t)q * k + lane] = key_score((uint32_t)(mine >> 32));
    }
}

int topk_check(int64_t Q, int64_t N, int64_t D, int64_t k) {
    LICV_CHECK_ARG(Q >= 1 && Q < (1LL << 31), "topk_ip: Q = %lld outside [1, 2^31)", (long long)Q);
    LICV_CHECK_ARG(N >= 1 && N < (1LL << 31) - TK_NT, "topk_ip: N = %lld outside [1, 2^31 - %d)", (long long)N, TK_NT);
    LICV_CHECK_ARG(k >= 1 && k <= TK_SLOTS, "topk_ip: k = %lld outside [1, %d]", (long long)k, TK_SLOTS);
    LICV_CHECK_ARG(k <= N, "topk_ip: k = %lld exceeds N = %lld", (long long)k, (long long)N);
    LICV_CHECK_ARG(D >= 4 && D <= 1024 && D % 4 == 0, "topk_ip: D = %lld must be a multiple of 4 in [4, 1024]", (long long)D);
    return LICV_OK;
}

// ------------------------------------------------------------------------------------------------ row kernels
// features / features.norm(dim=-1, keepdim=True): one wave per row; the sum of squares is taken in fp64 and the norm rounded to fp32
// once, then an IEEE fp32 division per element (two roundings against the exact quotient).
template <typename T>
__global__ __launch_bounds__(256)
void l2_normalize_k(const T* __restrict__ x, float* __restrict__ out, int64_t rows, int64_t dim) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T* xr = x + row * dim;
    double ss = 0.0;
    for (int64_t i = lane; i < dim; i += 64) {
        float v;
        if constexpr (sizeof(T) == 2) v = bf2f(xr[i]); else v = xr[i];
        ss += (double)v * (double)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float norm = (float)sqrt(ss);
    for (int64_t i = lane; i < dim; i += 64) {
        float v;
        if constexpr (sizeof(T) == 2) v = bf2f(xr[i]); else v = xr[i];
        out[row * dim + i] = v / norm;
    }
}

// hf:activations.py QuickGELUActivation on a bf16 tensor, as the unfused torch ops round: t = bf16(1.702 x), s = bf16(sigmoid(t)),
// y = bf16(x s).
__global__ __launch_bounds__(256)
void quick_gelu_k(bf16_t* __restrict__ x, int64_t rows, int64_t dim, int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * dim) return;
    bf16_t* p = x + (i / dim) * ld + (i % dim);
    const float v = bf2f(*p);
    const float t = rbf(1.702f * v);
    const float s = rbf(1.0f / (1.0f + expf(-t)));
    *p = f2bf(v * s);
}

}  // namespace

extern "C" int licv_topk_ip_workspace(int64_t Q, int64_t N, int64_t D, int64_t k, int64_t* bytes) {
    LICV_CHECK_ARG(bytes, "topk_ip_workspace: null pointer");
    if (int st = topk_check(Q, N, D, k)) return st;
    const TopkPlan p = topk_plan(Q, N);
    *bytes = Q * p.chunks * k * (int64_t)sizeof(u64);
    return LICV_OK;
}

extern "C" int licv_topk_ip(const float* queries, int64_t ldq, const float* index, int64_t ldx, int64_t Q, int64_t N, int64_t D, int64_t k,
                            int64_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int st = topk_check(Q, N, D, k)) return st;
    LICV_CHECK_ARG(ldq >= D && ldx >= D && ldq % 4 == 0 && ldx % 4 == 0, "topk_ip: ldq / ldx must be multiples of 4 and at least D");
    const TopkPlan p = topk_plan(Q, N);
    const int64_t need = Q * p.chunks * k * (int64_t)sizeof(u64);
    LICV_CHECK_ARG(workspace_bytes >= need, "topk_ip: workspace of %lld bytes, %lld needed (licv_topk_ip_workspace)", (long long)workspace_bytes,
                   (long long)need);
    LICV_CHECK_ARG(queries && index && out_idx && out_score && workspace, "topk_ip: null pointer");
    LICV_CHECK_ARG(((uintptr_t)queries | (uintptr_t)index) % 16 == 0 && (uintptr_t)workspace % 8 == 0,
                   "topk_ip: queries / index must be 16-byte aligned, the workspace 8-byte aligned");
    topk_ip_k<<<dim3((unsigned)p.q_tiles, (unsigned)p.chunks), dim3(TK_THREADS), 0, (hipStream_t)stream>>>(
        queries, ldq, index, ldx, (int)Q, (int)N, (int)D, (int)k, (int)p.chunk_len, (int)p.chunks, reinterpret_cast<u64*>(workspace));
    LICV_LAUNCH_CHECK();
    topk_merge_k<<<dim3((unsigned)Q), dim3(64), 0, (hipStream_t)stream>>>(reinterpret_cast<const u64*>(workspace), (int)Q, (int)p.chunks, (int)k,
                                                                         out_idx, out_score);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

extern "C" int licv_l2_normalize_rows(const void* x, int x_dtype, float* out, int64_t rows, int64_t dim, void* stream) {
    LICV_CHECK_ARG(x && out, "l2_normalize_rows: null pointer");
    LICV_CHECK_ARG(x_dtype == LICV_BF16 || x_dtype == LICV_F32, "l2_normalize_rows: dtype must be bf16 or fp32");
    LICV_CHECK_ARG(rows >= 1 && dim >= 1 && (rows + 3) / 4 <= INT_MAX, "l2_normalize_rows: bad shape %lld x %lld", (long long)rows, (long long)dim);
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (x_dtype == LICV_BF16) l2_normalize_k<bf16_t><<<grid, dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<const bf16_t*>(x), out, rows, dim);
    else l2_normalize_k<float><<<grid, dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<const float*>(x), out, rows, dim);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

extern "C" int licv_quick_gelu(void* x_bf16, int64_t rows, int64_t dim, int64_t ld, void* stream) {
    LICV_CHECK_ARG(x_bf16, "quick_gelu: null pointer");
    LICV_CHECK_ARG(rows >= 1 && dim >= 1 && ld >= dim && (rows * dim + 255) / 256 <= INT_MAX, "quick_gelu: bad shape %lld x %lld (ld %lld)",
                   (long long)rows, (long long)dim, (long long)ld);
    quick_gelu_k<<<dim3((unsigned)((rows * dim + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(reinterpret_cast<bf16_t*>(x_bf16), rows, dim, ld);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

// The CLIP text tower on PACKED tokens (hf:clip/modeling_clip.py CLIPTextTransformer, what ref:icv_src/utils/mm_topk_retriver.py
// encode_text runs): the tower is causal, so a token's state never depends on what follows it and the valid tokens of a right-padded
// batch, laid back to back, give exactly the padded tower's states.  Three kernels the rest of the library lacks: the token + position
// embedding on packed ids, causal self-attention over a ragged batch of short sequences, and a LayerNorm over selected rows (the final
// norm runs on the end-of-text rows only).
//
// licv_attn_varlen_causal.  One workgroup per (sequence, head); a sequence has at most 128 tokens and the head dimension is 64, so the
// whole K and V of the item sit in LDS (rows padded to 160 bytes: 2 x 128 x 160 = 40 KiB at most, sized by the longest sequence of
// the call) after ONE barrier, and the softmax of a 16-query sub-tile is one fp32 pass over its resident scores - no running max, no
// rescale.  The MFMA layouts are those of attention.hip (v_mfma_f32_16x16x32_bf16): S^T = K.Q^T keeps the query on lane & 15, so P^T is
// already the B operand of O^T = V^T.P^T and V^T comes through the transposing LDS read.  Sub-tile qs (queries 16 qs .. 16 qs + 15)
// needs key sub-tiles 0 .. qs only - everything above the diagonal is never multiplied - and only the diagonal sub-tile is masked.
// The workgroup has one wave per 16 tokens of the call's longest sequence (at most 4); wave w takes sub-tiles w, w + waves, ...
// Rounding points as licv_attn_fwd: exp2 of fp32 scores, bf16 probabilities into the PV MFMA, fp32 sums, one division, bf16 output.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 vbf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 vbf16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int vu32x4;

constexpr int VT_HD = 64;            // head dimension (every public CLIP text tower)
constexpr int VT_MAXLEN = 128;       // tokens per sequence
constexpr int VT_STR = 160;          // LDS row stride in bytes of a 64-column bf16 row (40 dwords = 8 mod 16: attention.hip's lds_stride(64))
constexpr int VT_MAXWAVES = 4;

__device__ __forceinline__ vbf16x4 vt_read_tr(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    s4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(p));
    return *reinterpret_cast<vbf16x4*>(&r);
}

// One 16-query sub-tile against key sub-tiles 0 .. NKT - 1 (NKT - 1 is the diagonal one).  Lane (g, ql) = (lane >> 4, lane & 15) holds
// query ql; s[st][r] is its score against key 16 st + 4 g + r.  V rows up to 32 * ceil(NKT / 2) are read: the staging zero-fills them.
template <int NKT>
__device__ __forceinline__ void vt_subtile(const char* sK, const char* sV, const vbf16x8 (&qf)[2], float sc, int g, int ql,
                                           floatx4 (&oacc)[VT_HD / 16], float& l_out) {
    constexpr int NP = (NKT + 1) / 2;                       // 32-key steps of the PV product
    floatx4 s[NKT];
#pragma unroll
    for (int st = 0; st < NKT; ++st) {
        s[st] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const vbf16x8 kf = *reinterpret_cast<const vbf16x8*>(sK + (st * 16 + ql) * VT_STR + (ks * 32 + g * 8) * 2);
            s[st] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[st], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (g * 4 + r > ql) s[NKT - 1][r] = -INFINITY;      // the diagonal sub-tile: key 16 (NKT-1) + 4 g + r <= query 16 (NKT-1) + ql
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < NKT; ++st) tmax = fmaxf(tmax, fmaxf(fmaxf(s[st][0], s[st][1]), fmaxf(s[st][2], s[st][3])));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));           // finite: key 16 (NKT-1) is allowed for every query of the sub-tile
    const float m = tmax * sc;
    float psum = 0.f;
    vbf16x8 pf[NP];
#pragma unroll
    for (int st = 0; st < 2 * NP; ++st)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = (st < NKT) ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[st < NKT ? st : 0][r], sc, -m)) : 0.f;
            psum += p;
            pf[st >> 1][(st & 1) * 4 + r] = (__bf16)p;
        }
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    l_out = psum;
#pragma unroll
    for (int dt = 0; dt < VT_HD / 16; ++dt) oacc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < NP; ++s2) {
#pragma unroll
        for (int dt = 0; dt < VT_HD / 16; ++dt) {
            const char* p0 = sV + ((2 * s2) * 16 + g * 4 + (ql >> 2)) * VT_STR + (dt * 16 + (ql & 3) * 4) * 2;
            const vbf16x4 lo = vt_read_tr(p0);
            const vbf16x4 hi = vt_read_tr(p0 + 16 * VT_STR);
            vbf16x8 vf;
            vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
            vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[s2], oacc[dt], 0, 0, 0);
        }
    }
}

// qkv: (total, ld) bf16 rows [Q | K | V], each E = n_heads * 64 wide; out: (total, E) dense.  alloc_rows = LDS rows per operand.
__global__ __launch_bounds__(64 * VT_MAXWAVES)
void attn_varlen_causal_k(const bf16_t* __restrict__ qkv, int64_t ld, const int32_t* __restrict__ cu, int n_heads, int total,
                          int alloc_rows, float sc, bf16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char vt_lds[];
    char* sK = vt_lds;
    char* sV = vt_lds + alloc_rows * VT_STR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int g = lane >> 4, ql = lane & 15;
    const int seq = blockIdx.x / n_heads, head = blockIdx.x % n_heads;
    const int start = cu[seq], L = cu[seq + 1] - start;
    const int rows = (L + 31) & ~31;                         // staged rows: the PV product walks keys in steps of 32
    // the host checked its own copy of cu_seqlens; a device copy that disagrees must not take the kernel out of the buffers or the LDS
    if (L < 1 || rows > alloc_rows || start < 0 || start + L > total) return;
    const int E = n_heads * VT_HD;
    const bf16_t* base = qkv + (int64_t)start * ld + head * VT_HD;

    for (int c = tid; c < rows * (VT_HD / 8); c += blockDim.x) {
        const int row = c >> 3, ch = c & 7;
        vu32x4 k = vu32x4{0u, 0u, 0u, 0u}, v = vu32x4{0u, 0u, 0u, 0u};
        if (row < L) {
            const bf16_t* p = base + (int64_t)row * ld + ch * 8;
            k = *reinterpret_cast<const vu32x4*>(p + E);
            v = *reinterpret_cast<const vu32x4*>(p + 2 * E);
        }
        *reinterpret_cast<vu32x4*>(sK + row * VT_STR + ch * 16) = k;
        *reinterpret_cast<vu32x4*>(sV + row * VT_STR + ch * 16) = v;
    }
    __syncthreads();

    const int nqt = (L + 15) >> 4;
    for (int qs = wave; qs < nqt; qs += nw) {
        const int qrow = qs * 16 + ql;
        vbf16x8 qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            vu32x4 r = vu32x4{0u, 0u, 0u, 0u};
            if (qrow < L) r = *reinterpret_cast<const vu32x4*>(base + (int64_t)qrow * ld + ks * 32 + g * 8);
            qf[ks] = *reinterpret_cast<vbf16x8*>(&r);
        }
        floatx4 oacc[VT_HD / 16];
        float l = 1.f;
        switch (qs) {
            case 0: vt_subtile<1>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 1: vt_subtile<2>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 2: vt_subtile<3>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 3: vt_subtile<4>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 4: vt_subtile<5>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 5: vt_subtile<6>(sK, sV, qf, sc, g, ql, oacc, l); break;
            case 6: vt_subtile<7>(sK, sV, qf, sc, g, ql, oacc, l); break;
            default: vt_subtile<8>(sK, sV, qf, sc, g, ql, oacc, l); break;
        }
        if (qrow < L) {
            const float inv = 1.0f / l;                      // l >= 1: the row's largest score contributes exp2(0)
            bf16_t* op = out + (int64_t)(start + qrow) * E + head * VT_HD;
#pragma unroll
            for (int dt = 0; dt < VT_HD / 16; ++dt) {
                uint2 u;
                u.x = (uint32_t)f2bf(oacc[dt][0] * inv) | ((uint32_t)f2bf(oacc[dt][1] * inv) << 16);
                u.y = (uint32_t)f2bf(oacc[dt][2] * inv) | ((uint32_t)f2bf(oacc[dt][3] * inv) << 16);
                *reinterpret_cast<uint2*>(op + dt * 16 + g * 4) = u;
            }
        }
    }
}

// hf:clip/modeling_clip.py CLIPTextEmbeddings on packed tokens: out[t] = bf16(tok[ids[t]] + pos[positions[t]]), the sum in fp32 and
// rounded once (torch's bf16 add).  One thread per 8 columns.  An id or position outside its table reads nothing and writes zeros.
__global__ __launch_bounds__(256)
void clip_text_embed_k(const int64_t* __restrict__ ids, const int32_t* __restrict__ positions, const bf16_t* __restrict__ tok,
                       const bf16_t* __restrict__ pos, bf16_t* __restrict__ out, int64_t total, int dim8, int64_t vocab, int n_pos) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total * dim8) return;
    const int64_t t = i / dim8;
    const int c = (int)(i % dim8) * 8;
    const int64_t id = ids[t];
    const int p = positions[t];
    const int64_t dim = (int64_t)dim8 * 8;
    vu32x4 o = vu32x4{0u, 0u, 0u, 0u};
    if (id >= 0 && id < vocab && p >= 0 && p < n_pos) {
        const vu32x4 a = *reinterpret_cast<const vu32x4*>(tok + id * dim + c);
        const vu32x4 b = *reinterpret_cast<const vu32x4*>(pos + (int64_t)p * dim + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = __uint_as_float(a[j] << 16) + __uint_as_float(b[j] << 16);
            const float hi = __uint_as_float(a[j] & 0xffff0000u) + __uint_as_float(b[j] & 0xffff0000u);
            o[j] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
        }
    }
    *reinterpret_cast<vu32x4*>(out + t * dim + c) = o;
}

// out[j] = LayerNorm(x[rows[j]]): one wave per output row, fp32 statistics (mean, then the centred sum of squares), one rounding - the
// arithmetic of layernorm_fwd_k.  A row index outside [0, n_src) reads nothing and writes zeros.
__global__ __launch_bounds__(256)
void layernorm_rows_k(const bf16_t* __restrict__ x, int64_t ld_x, int64_t n_src, const int32_t* __restrict__ rows, const bf16_t* __restrict__ w,
                      const bf16_t* __restrict__ b, bf16_t* __restrict__ out, int64_t n_rows, int dim, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_rows) return;
    const int64_t src = rows[j];
    bf16_t* o = out + j * dim;
    if (src < 0 || src >= n_src) {
        for (int i = lane; i < dim; i += 64) o[i] = 0;
        return;
    }
    const bf16_t* xr = x + src * ld_x;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) s += bf2f(xr[i]);
    const float mean = wave_sum(s) / (float)dim;
    float q = 0.f;
    for (int i = lane; i < dim; i += 64) { const float d = bf2f(xr[i]) - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)dim + eps);
    for (int i = lane; i < dim; i += 64) o[i] = f2bf((bf2f(xr[i]) - mean) * rstd * bf2f(w[i]) + bf2f(b[i]));
}

}  // namespace

extern "C" int licv_attn_varlen_causal(const void* qkv_bf16, int64_t ld_qkv, const int32_t* cu_seqlens_host, const int32_t* cu_seqlens_dev,
                                       int64_t n_seq, int64_t n_heads, int64_t head_dim, float scale, void* out_bf16, void* stream) {
    LICV_CHECK_ARG(qkv_bf16 && cu_seqlens_host && cu_seqlens_dev && out_bf16, "attn_varlen_causal: null pointer");
    LICV_CHECK_ARG(head_dim == VT_HD, "attn_varlen_causal: head_dim = %lld, only %d is supported", (long long)head_dim, VT_HD);
    LICV_CHECK_ARG(scale > 0.f && scale < INFINITY, "attn_varlen_causal: scale must be positive and finite");
    LICV_CHECK_ARG(n_seq >= 1 && n_heads >= 1 && n_heads <= 1024 && n_seq * n_heads <= INT_MAX, "attn_varlen_causal: bad n_seq = %lld / n_heads = %lld",
                   (long long)n_seq, (long long)n_heads);
    LICV_CHECK_ARG(cu_seqlens_host[0] == 0, "attn_varlen_causal: cu_seqlens[0] = %d, must be 0", (int)cu_seqlens_host[0]);
    int max_len = 0;
    for (int64_t i = 0; i < n_seq; ++i) {
        const int64_t len = (int64_t)cu_seqlens_host[i + 1] - (int64_t)cu_seqlens_host[i];
        LICV_CHECK_ARG(len >= 1 && len <= VT_MAXLEN, "attn_varlen_causal: sequence %lld has length %lld (cu_seqlens must ascend in steps of 1 to %d)",
                       (long long)i, (long long)len, VT_MAXLEN);
        if (len > max_len) max_len = (int)len;
    }
    const int64_t E = n_heads * VT_HD;
    LICV_CHECK_ARG(ld_qkv >= 3 * E && ld_qkv % 8 == 0, "attn_varlen_causal: ld_qkv = %lld must be a multiple of 8 and at least 3 * n_heads * head_dim",
                   (long long)ld_qkv);
    LICV_CHECK_ARG(((uintptr_t)qkv_bf16 | (uintptr_t)out_bf16) % 16 == 0, "attn_varlen_causal: qkv / out must be 16-byte aligned");
    const int total = cu_seqlens_host[n_seq];
    const int alloc_rows = (max_len + 31) & ~31;
    int waves = (max_len + 15) / 16;
    if (waves > VT_MAXWAVES) waves = VT_MAXWAVES;
    attn_varlen_causal_k<<<dim3((unsigned)(n_seq * n_heads)), dim3(64 * waves), (size_t)(2 * alloc_rows * VT_STR), (hipStream_t)stream>>>(
        reinterpret_cast<const bf16_t*>(qkv_bf16), ld_qkv, cu_seqlens_dev, (int)n_heads, total, alloc_rows, scale * 1.4426950408889634f,
        reinterpret_cast<bf16_t*>(out_bf16));
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

extern "C" int licv_clip_text_embed(const int64_t* ids, const int32_t* positions, const void* tok_bf16, const void* pos_bf16, void* out_bf16,
                                    int64_t total, int64_t dim, int64_t vocab, int64_t n_pos, void* stream) {
    LICV_CHECK_ARG(ids && positions && tok_bf16 && pos_bf16 && out_bf16, "clip_text_embed: null pointer");
    LICV_CHECK_ARG(total >= 1 && dim >= 8 && dim % 8 == 0 && dim <= (1 << 20) && vocab >= 1 && n_pos >= 1 && n_pos <= INT_MAX,
                   "clip_text_embed: bad shape (total %lld, dim %lld, vocab %lld, positions %lld; dim must be a multiple of 8)", (long long)total,
                   (long long)dim, (long long)vocab, (long long)n_pos);
    LICV_CHECK_ARG(((uintptr_t)tok_bf16 | (uintptr_t)pos_bf16 | (uintptr_t)out_bf16) % 16 == 0, "clip_text_embed: tables / out must be 16-byte aligned");
    const int64_t threads = total * (dim / 8);
    LICV_CHECK_ARG((threads + 255) / 256 <= INT_MAX, "clip_text_embed: too many elements");
    clip_text_embed_k<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        ids, positions, reinterpret_cast<const bf16_t*>(tok_bf16), reinterpret_cast<const bf16_t*>(pos_bf16), reinterpret_cast<bf16_t*>(out_bf16),
        total, (int)(dim / 8), vocab, (int)n_pos);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

extern "C" int licv_layernorm_rows_fwd(const void* x_bf16, int64_t ld_x, int64_t n_src_rows, const int32_t* rows, const void* w_bf16,
                                       const void* b_bf16, void* out_bf16, int64_t n_rows, int64_t dim, float eps, void* stream) {
    LICV_CHECK_ARG(x_bf16 && rows && w_bf16 && b_bf16 && out_bf16, "layernorm_rows_fwd: null pointer");
    LICV_CHECK_ARG(n_rows >= 1 && n_src_rows >= 1 && dim >= 1 && dim <= (1 << 20) && ld_x >= dim && (n_rows + 3) / 4 <= INT_MAX,
                   "layernorm_rows_fwd: bad shape (%lld of %lld rows, dim %lld, ld %lld)", (long long)n_rows, (long long)n_src_rows, (long long)dim,
                   (long long)ld_x);
    layernorm_rows_k<<<dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
        reinterpret_cast<const bf16_t*>(x_bf16), ld_x, n_src_rows, rows, reinterpret_cast<const bf16_t*>(w_bf16),
        reinterpret_cast<const bf16_t*>(b_bf16), reinterpret_cast<bf16_t*>(out_bf16), n_rows, (int)dim, eps);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

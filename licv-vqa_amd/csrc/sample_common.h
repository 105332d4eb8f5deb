// Device code shared by the sampling step (sample.hip) and the beam-search sampling step (beam.hip): Philox4x32-10, and the kept set
// of a row of processed scores under transformers' warpers (hf:generation/logits_process.py TopKLogitsWarper, TopPLogitsWarper,
// MinPLogitsWarper, applied in that order).  One 1024-lane workgroup owns a row; lane l holds the ids [l*npt, (l+1)*npt) as ordered
// 32-bit keys in registers (npt <= 64: V <= 65536).
//
// Every kept set is a prefix of one total order - key descending, then token id ascending - and is written (t, c): kept = key > t or
// (key == t and id <= c).  Selections are MSB-first radix selects over the keys (four passes of 256 bins) with counts or probability
// mass per bin.  Mass is exp(y - max) in 2^-40 fixed point, so a sum does not depend on its order: the kernel's parallel sums equal
// a sequential sum, and a restatement can evaluate every decision exactly.
#pragma once
#include "common.h"
#include <limits.h>

#define SAMPLE_THREADS 1024
#define SAMPLE_NPT 64                            // vocabulary entries per lane
#define SAMPLE_MAX_V (SAMPLE_THREADS * SAMPLE_NPT)

// Philox4x32-10 (Salmon et al., SC'11), first output word; key = 64-bit seed (low word first), counter = (c0, c1, c2, c3)
__device__ __forceinline__ uint32_t philox_x0(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// u = ((x >> 8) + 0.5) * 2^-24, exact in double, strictly inside (0, 1)
__device__ __forceinline__ double philox_uniform(uint32_t x) { return ((double)(x >> 8) + 0.5) * 5.9604644775390625e-8; }
// Gumbel noise -log(-log u), evaluated in double and rounded once to fp32
__device__ __forceinline__ float gumbel_noise(uint32_t x) { return (float)(-log(-log(philox_uniform(x)))); }

// order-preserving float <-> uint32 map; key 0 marks an empty slot (below every float but a negative NaN)
__device__ __forceinline__ uint32_t f2key(float f) { const uint32_t b = __float_as_uint(f); return b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu)); }
// probability mass relative to the row maximum in 2^-40 fixed point (w <= 1, so a row of 65536 sums below 2^57)
__device__ __forceinline__ uint64_t mass_fix(float y, float m) { return (uint64_t)((double)expf(y - m) * 1099511627776.0); }

struct KeptSet { uint32_t t; int c; };
__device__ __forceinline__ bool kept_in(uint32_t k, int id, KeptSet s) { return k > s.t || (k == s.t && id <= s.c); }

struct SampleSmem {
    uint32_t hc[256];
    unsigned long long hm[256];
    unsigned long long wu[SAMPLE_THREADS / 64];
    float wf[SAMPLE_THREADS / 64];
    uint32_t bt; unsigned long long bu; int bi;
};

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const int lo = __shfl_xor((int)(uint32_t)v, o, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int o) {
    const int lo = __shfl_up((int)(uint32_t)v, o, 64), hi = __shfl_up((int)(uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
// inclusive scan over the lanes of a wave
__device__ __forceinline__ unsigned long long wave_incl_u64(unsigned long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = shfl_up_u64(v, o); if (lane >= o) v += u; }
    return v;
}

__device__ __forceinline__ float sblk_max(float v, SampleSmem& s) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s.wf[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s.wf[0];
    for (int w = 1; w < SAMPLE_THREADS / 64; ++w) r = fmaxf(r, s.wf[w]);
    return r;
}
// exclusive scan over the lanes of the workgroup in lane order; *total = the sum
__device__ __forceinline__ unsigned long long sblk_excl(unsigned long long v, SampleSmem& s, unsigned long long* total) {
    const unsigned long long incl = wave_incl_u64(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 63) s.wu[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < SAMPLE_THREADS / 64; ++w) { if (w < wave) before += s.wu[w]; all += s.wu[w]; }
    *total = all;
    return before + incl - v;
}

// id of the rank-th (1-based) lowest id among the entries with key == t and id <= cap
template <int NPT>
__device__ int id_of_rank(const uint32_t (&kk)[NPT], int npt, int base, uint32_t t, int cap, unsigned long long rank, SampleSmem& s) {
    unsigned long long cnt = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) if (j < npt && kk[j] == t && base + j <= cap) ++cnt;
    unsigned long long tot;
    const unsigned long long ex = sblk_excl(cnt, s, &tot);
    if (ex < rank && rank <= ex + cnt) {
        unsigned long long run = ex;
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (j < npt && kk[j] == t && base + j <= cap) { if (++run == rank) { s.bi = base + j; break; } }
    }
    __syncthreads();
    return s.bi;
}

// the need-th entry (1-based) of the whole row in the total order: the kept set of the top `need` entries
template <int NPT>
__device__ KeptSet select_top(const uint32_t (&kk)[NPT], int npt, int base, unsigned long long need, SampleSmem& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t pre = 0, msk = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s.hc[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (j < npt && kk[j] != 0 && (kk[j] & msk) == pre) atomicAdd(&s.hc[(kk[j] >> shift) & 255], 1u);
        __syncthreads();
        if (wave == 0) {                                   // lane l: bins 255-4l .. 252-4l, from the top
            uint32_t h[4]; unsigned long long ls = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { h[q] = s.hc[255 - 4 * lane - q]; ls += h[q]; }
            const unsigned long long incl = wave_incl_u64(ls), ex = incl - ls;
            if (ex < need && need <= incl) {
                unsigned long long run = ex;
                for (int q = 0; q < 4; ++q) {
                    if (run + h[q] >= need) { s.bt = 255 - 4 * lane - q; s.bu = need - run; break; }
                    run += h[q];
                }
            }
        }
        __syncthreads();
        pre |= s.bt << shift; msk |= 0xffu << shift; need = s.bu;
    }
    return KeptSet{pre, id_of_rank(kk, npt, base, pre, INT_MAX, need, s)};
}

template <int NPT>
__device__ unsigned long long count_kept(const uint32_t (&kk)[NPT], int npt, int base, KeptSet S, SampleSmem& s) {
    unsigned long long n = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S)) ++n;
    unsigned long long tot;
    sblk_excl(n, s, &tot);
    return tot;
}

// top-p: remove kept entries in ascending order (key ascending, then id descending) while the removed mass stays <= bound
template <int NPT>
__device__ KeptSet top_p_select(const uint32_t (&kk)[NPT], int npt, int base, KeptSet S, float m, unsigned long long bound, SampleSmem& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t pre = 0, msk = 0;
    unsigned long long below = 0, cnt_t = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) { s.hc[tid] = 0; s.hm[tid] = 0; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S) && (kk[j] & msk) == pre) {
                const int d = (kk[j] >> shift) & 255;
                atomicAdd(&s.hc[d], 1u);
                atomicAdd(&s.hm[d], (unsigned long long)mass_fix(key2f(kk[j]), m));
            }
        __syncthreads();
        if (wave == 0) {                                   // lane l: bins 4l .. 4l+3, from the bottom
            unsigned long long h[4], ls = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { h[q] = s.hm[4 * lane + q]; ls += h[q]; }
            const unsigned long long incl = wave_incl_u64(ls), ex = incl - ls;
            if (below + ex <= bound && bound < below + incl) {
                unsigned long long run = below + ex;
                for (int q = 0; q < 4; ++q) {
                    if (run + h[q] > bound) { s.bt = 4 * lane + q; s.bu = run; s.bi = (int)s.hc[4 * lane + q]; break; }
                    run += h[q];
                }
            }
        }
        __syncthreads();
        pre |= s.bt << shift; msk |= 0xffu << shift; below = s.bu; cnt_t = (unsigned long long)s.bi;
        __syncthreads();
    }
    // the entries of key pre share one mass; the removable ones go highest id first
    const unsigned long long q_t = mass_fix(key2f(pre), m);
    const unsigned long long r = (bound - below) / q_t;
    const int cap = pre == S.t ? S.c : INT_MAX;
    return KeptSet{pre, id_of_rank(kk, npt, base, pre, cap, cnt_t - r, s)};
}

struct SampleFilter { float temperature; int64_t top_k; float top_p; float min_p; int mtk; };

// the kept set of a row of processed scores under top-k, top-p, min-p (each a no-op at its neutral value); *m_out = the row maximum
template <int NPT>
__device__ KeptSet row_filter(const uint32_t (&kk)[NPT], int npt, int base, int V, const SampleFilter& p, float* m_out, SampleSmem& s) {
    float ml = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPT; ++j) if (j < npt && kk[j] != 0) ml = fmaxf(ml, key2f(kk[j]));
    const float m = sblk_max(ml, s);
    *m_out = m;
    KeptSet S{0u, -1};                                     // every entry of the row (key 0 = no entry)
    if (p.top_k > 0) {                                     // TopKLogitsWarper: every score >= the k-th largest stays
        const int64_t k = p.top_k > p.mtk ? p.top_k : p.mtk;
        if (k < V) S = KeptSet{select_top(kk, npt, base, (unsigned long long)k, s).t, INT_MAX};
    }
    if (p.top_p < 1.0f) {                                  // TopPLogitsWarper on the top-k survivors
        unsigned long long z = 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S)) z += mass_fix(key2f(kk[j]), m);
        unsigned long long Z;
        sblk_excl(z, s, &Z);
        const float om = (float)(1.0 - (double)p.top_p);
        const unsigned long long bound = (unsigned long long)floor((double)om * (double)Z);
        S = top_p_select(kk, npt, base, S, m, bound, s);
        if (count_kept(kk, npt, base, S, s) < (unsigned long long)p.mtk) S = select_top(kk, npt, base, (unsigned long long)p.mtk, s);
    }
    if (p.min_p > 0.0f) {                                  // MinPLogitsWarper: p >= min_p * max p, i.e. exp(y - max) >= min_p
        uint32_t lo = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S) && expf(key2f(kk[j]) - m) >= p.min_p) lo = min(lo, kk[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s.wu[threadIdx.x >> 6] = lo;
        __syncthreads();
        uint32_t t_m = 0xffffffffu;
        for (int w = 0; w < SAMPLE_THREADS / 64; ++w) t_m = min(t_m, (uint32_t)s.wu[w]);
        if (t_m > S.t) S = KeptSet{t_m, INT_MAX};
        if (count_kept(kk, npt, base, S, s) < (unsigned long long)p.mtk) S = select_top(kk, npt, base, (unsigned long long)p.mtk, s);
    }
    return S;
}

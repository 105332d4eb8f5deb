// A continuation step's self-attention block - T new tokens per row, read through the KV cache's row table - as a single launch:
// the fused QKV projection's bf16 rows (row r*T + t = token t of row r) -> rotary on Q and K (hf:idefics/modeling_idefics.py:396-428,
// each bf16 op rounded) -> optionally K | V appended to cache[r, past : past+T] -> attention of query t over the history positions
// j < past (cache row kv_rows[r][j]) and over the new tokens u <= t of its OWN row -> O.  It generalises csrc/decode.hip (T = 1 with
// append = 1 gives that kernel's bits, output and cache) and keeps its arithmetic: scores in fp32 in the log2 domain, P rounded to
// bf16 before the P.V product with the sum taken over the unrounded P, 64-key sweeps that are online across sweeps, a history key's
// score as one lane's 128-term fma chain and a new key's score as the wave's butterfly sum over the lanes' two rotated columns.
//
// One 64-lane wave per (row, kv head) - per (row, kv head, slice of the group's query heads) only where the LDS budget below cannot hold
// the whole group.  The loop nest is the decode kernel's turned inside out: the SWEEP is the outer loop, so a lane requests the K row
// and the V row of its key ONCE (16-byte loads), holds K in registers and parks V in LDS, and the T queries of every query head of the
// group are served inside the sweep.  A chain of T decode steps fetches the same history T times.  What has to outlive a sweep lives
// in LDS: the rotated Q of every (head, token), the rotated K and the V of the T new tokens (they are keys past .. past+T-1 of the
// last sweeps and never make a round trip through memory, so append = 0 costs nothing extra), and each query's running maximum,
// running sum and fp32 output row.  A key that is masked or not yet visible to a query scores -inf: it adds exactly zero and never
// raises the running maximum; a sweep that lies wholly behind a query is skipped for it.  Nothing a query computes depends on T or on
// a later token, so padded tails and later tokens cannot change an earlier token's bits.
#include "common.h"
#include <limits.h>

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_a;
#define APP_VSTR 272                  // LDS stride of a V row (256 B + 16: conflict-free 16-byte row writes, 2-byte column reads)
#define APP_STATIC_LDS (64 * APP_VSTR + 2 * 64 * 4)
#define APP_LDS_SMALL (64 * 1024)     // what a launch gets without asking
#define APP_LDS_LARGE (152 * 1024)    // of the CU's 160 KiB, asked for through the function attribute

struct AppendP {
    const bf16_t* qkv; int64_t ldq;
    const bf16_t* cosT; const bf16_t* sinT; const int64_t* pos; int64_t n_pos;
    bf16_t* cache; int64_t max_len;
    const int32_t* kv_rows; int64_t ld_rows;
    const int32_t* key_valid;
    bf16_t* out;
    int M, T, Sk, past, nh, nkv, hd, hpb, append;     // hpb: query heads of the group served by one workgroup (divides nh / nkv)
    float scale;
};

// dynamic LDS of one workgroup: Q (hpb*T rows) | new K | new V (bf16), the fp32 output rows, running max / sum, positions, row table
static size_t append_lds_bytes(int hpb, int T, int hd, int Sk) {
    const size_t nq = (size_t)hpb * T;
    return (nq + 2 * (size_t)T) * hd * 2 + nq * hd * 4 + 2 * nq * 4 + (size_t)T * 4 + (size_t)Sk * 4;
}

__global__ __launch_bounds__(64)
void append_attn_k(AppendP a) {
    extern __shared__ __attribute__((aligned(16))) char app_smem[];
    __shared__ __attribute__((aligned(16))) char vt[64 * APP_VSTR];     // the sweep's V rows (bf16), one per key
    __shared__ float pch[2][64];                                         // a query's probabilities of the sweep (two buffers: one barrier per query)
    const int lane = threadIdx.x;
    const int hd = a.hd, half = hd >> 1, rep = a.nh / a.nkv, T = a.T, past = a.past, Sk = a.Sk, hpb = a.hpb;
    const int nsplit = rep / hpb;
    const int hs = blockIdx.x % nsplit, rg = blockIdx.x / nsplit;
    const int r = rg / a.nkv, g = rg % a.nkv;
    const int head0 = g * rep + hs * hpb;
    const int nq = hpb * T;
    const int64_t qd = (int64_t)a.nh * hd, kd = (int64_t)a.nkv * hd;
    const bool act = lane < half;
    const float sc = a.scale * 1.4426950408889634f;
    const int nch = hd >> 3;                            // 16-byte chunks per K / V row
    bf16_t* qs = reinterpret_cast<bf16_t*>(app_smem);  // [nq][hd] rotated Q, query qi = qh * T + t
    bf16_t* kn = qs + (size_t)nq * hd;                 // [T][hd] rotated K of the new tokens
    bf16_t* vn = kn + (size_t)T * hd;                  // [T][hd] their V
    float* ost = reinterpret_cast<float*>(vn + (size_t)T * hd);          // [nq][hd] un-normalised output rows
    float* mst = ost + (size_t)nq * hd;                // [nq] running maximum (log2 domain)
    float* lst = mst + nq;                             // [nq] running sum
    int* spos = reinterpret_cast<int*>(lst + nq);      // [T] clamped positions
    int* srow = spos + T;                              // [Sk] physical cache row of every key, -1 = masked
    const int32_t* rows_r = a.kv_rows ? a.kv_rows + (int64_t)r * a.ld_rows : nullptr;
    const int32_t* valid_r = a.key_valid ? a.key_valid + (int64_t)r * Sk : nullptr;
    // ---- memory round trip 1: positions, row table and mask
    if (lane < T) {
        int64_t p = a.pos[(int64_t)r * T + lane];
        p = p < 0 ? 0 : (p >= a.n_pos ? a.n_pos - 1 : p);
        spos[lane] = (int)p;
    }
    for (int j = lane; j < Sk; j += 64) {
        const int pr = (j < past && rows_r) ? rows_r[j] : r;              // a new token's K / V never come from the cache
        const bool ok = !valid_r || valid_r[j] != 0;
        srow[j] = ok ? pr : -1;
    }
    for (int i = lane; i < nq; i += 64) { mst[i] = -INFINITY; lst[i] = 0.f; }
    for (int i = lane; i < nq * hd; i += 64) ost[i] = 0.f;
    __syncthreads();
    // ---- round trip 2: cos / sin and the raw Q, K, V of every new token; rotary; the new K | V to LDS (and to the cache when appending)
    const bool writer = a.append && hs == 0;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
        if (act) {
            const int64_t p = spos[t];
            const bf16_t* row = a.qkv + ((int64_t)r * T + t) * a.ldq;
            const float c = bf2f(a.cosT[p * hd + lane]), s = bf2f(a.sinT[p * hd + lane]);
            const float klo = bf2f(row[qd + (int64_t)g * hd + lane]), khi = bf2f(row[qd + (int64_t)g * hd + lane + half]);
            const bf16_t v0 = row[qd + kd + (int64_t)g * hd + lane], v1 = row[qd + kd + (int64_t)g * hd + lane + half];
            const bf16_t k0 = f2bf(rbf(klo * c) + rbf(-khi * s));
            const bf16_t k1 = f2bf(rbf(khi * c) + rbf(klo * s));
            kn[t * hd + lane] = k0; kn[t * hd + lane + half] = k1;
            vn[t * hd + lane] = v0; vn[t * hd + lane + half] = v1;
            if (writer) {
                bf16_t* crow = a.cache + ((int64_t)r * a.max_len + past + t) * 2 * kd + (int64_t)g * hd;
                crow[lane] = k0; crow[lane + half] = k1;
                crow[kd + lane] = v0; crow[kd + lane + half] = v1;
            }
            for (int qh = 0; qh < hpb; ++qh) {
                const float lo = bf2f(row[(int64_t)(head0 + qh) * hd + lane]), hi = bf2f(row[(int64_t)(head0 + qh) * hd + lane + half]);
                bf16_t* qrow = qs + (size_t)(qh * T + t) * hd;
                qrow[lane] = f2bf(rbf(lo * c) + rbf(-hi * s));
                qrow[lane + half] = f2bf(rbf(hi * c) + rbf(lo * s));
            }
        }
    }
    // ---- 64 keys per sweep, ONE key per lane: K into registers and V into LDS once, then every query of the workgroup
    for (int j0 = 0; j0 < Sk; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < Sk;
        const int pr = in ? srow[j] : -1;
        const bool ok = pr >= 0;
        u32x4_a kv[16], vv[16];
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) { kv[ch] = u32x4_a{0u, 0u, 0u, 0u}; vv[ch] = u32x4_a{0u, 0u, 0u, 0u}; }
        __syncthreads();                                // the rotary's LDS writes are visible; the previous sweep's readers are done with vt
        if (ok && j < past) {                           // (a masked key is never fetched: its table entry need not name a real row)
            const bf16_t* rowp = a.cache + ((int64_t)pr * a.max_len + j) * 2 * kd + (int64_t)g * hd;
            const u32x4_a* kp = reinterpret_cast<const u32x4_a*>(rowp);
            const u32x4_a* vp = reinterpret_cast<const u32x4_a*>(rowp + kd);
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) if (ch < nch) kv[ch] = kp[ch];
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) if (ch < nch) vv[ch] = vp[ch];
        } else if (ok) {
            const u32x4_a* kp = reinterpret_cast<const u32x4_a*>(kn + (size_t)(j - past) * hd);
            const u32x4_a* vp = reinterpret_cast<const u32x4_a*>(vn + (size_t)(j - past) * hd);
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) if (ch < nch) { kv[ch] = kp[ch]; vv[ch] = vp[ch]; }
        }
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) if (ch < nch) *reinterpret_cast<u32x4_a*>(vt + lane * APP_VSTR + ch * 16) = vv[ch];
        const bool has_new = j0 + 64 > past;            // this sweep holds new tokens
        int pb = 0;
        for (int qh = 0; qh < hpb; ++qh) {
            for (int t = 0; t < T; ++t) {
                if (j0 > past + t) continue;            // the whole sweep lies behind this query
                const int qi = qh * T + t;
                const bf16_t* qrow = qs + (size_t)qi * hd;
                u32x4_a qreg[16];
#pragma unroll
                for (int ch = 0; ch < 16; ++ch) qreg[ch] = ch < nch ? reinterpret_cast<const u32x4_a*>(qrow)[ch] : u32x4_a{0u, 0u, 0u, 0u};
                float acc = 0.f;
#pragma unroll
                for (int ch = 0; ch < 16; ++ch)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc = __builtin_fmaf(__uint_as_float(kv[ch][e] << 16), __uint_as_float(qreg[ch][e] << 16), acc);
                        acc = __builtin_fmaf(__uint_as_float(kv[ch][e] & 0xffff0000u), __uint_as_float(qreg[ch][e] & 0xffff0000u), acc);
                    }
                float sj = acc;
                if (has_new) {                          // a new key's score: the decode kernel's sum over the lanes' two columns
                    const float q0 = act ? bf2f(qrow[lane]) : 0.f, q1 = act ? bf2f(qrow[lane + half]) : 0.f;
                    const int u_lo = max(0, j0 - past), u_hi = min(t, j0 + 63 - past);
                    for (int u = u_lo; u <= u_hi; ++u) {
                        const float k0 = act ? bf2f(kn[u * hd + lane]) : 0.f, k1 = act ? bf2f(kn[u * hd + lane + half]) : 0.f;
                        const float s_new = wave_sum(q0 * k0 + q1 * k1);
                        if (j == past + u) sj = s_new;
                    }
                }
                if (!(ok && j <= past + t)) sj = -INFINITY;               // masked, or not yet visible to this query
                const float m_run = mst[qi], l_run = lst[qi];
                const float cmax = wave_max(sj);
                const float m_new = fmaxf(m_run, cmax * sc);
                const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);            // m_run = -inf -> 0
                const float pj = __builtin_amdgcn_exp2f(__builtin_fmaf(sj, sc, -m_use));
                const float l_new = l_run * alpha + wave_sum(pj);
                pch[pb][lane] = rbf(pj);
                __syncthreads();                        // pch (and, for the sweep's first query, vt) written; everyone has read mst / lst
                if (lane == 0) { mst[qi] = m_new; lst[qi] = l_new; }
                if (act) {
                    float o0 = ost[(size_t)qi * hd + lane] * alpha, o1 = ost[(size_t)qi * hd + lane + half] * alpha;
                    const int nk = min(64, past + t + 1 - j0);            // keys behind the query's own hold p = 0
                    for (int jj = 0; jj < nk; ++jj) {
                        const float pv = pch[pb][jj];
                        const bf16_t* vr = reinterpret_cast<const bf16_t*>(vt + jj * APP_VSTR);
                        const bool live = pv != 0.f;                      // (a masked key contributes nothing, whatever its LDS row holds)
                        o0 = __builtin_fmaf(pv, live ? bf2f(vr[lane]) : 0.f, o0);
                        o1 = __builtin_fmaf(pv, live ? bf2f(vr[lane + half]) : 0.f, o1);
                    }
                    ost[(size_t)qi * hd + lane] = o0; ost[(size_t)qi * hd + lane + half] = o1;
                }
                pb ^= 1;
            }
        }
    }
    __syncthreads();
    if (act)
        for (int qh = 0; qh < hpb; ++qh)
            for (int t = 0; t < T; ++t) {
                const int qi = qh * T + t;
                const float l_run = lst[qi];
                const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
                bf16_t* op = a.out + ((int64_t)r * T + t) * qd + (int64_t)(head0 + qh) * hd;
                op[lane] = f2bf(ost[(size_t)qi * hd + lane] * inv); op[lane + half] = f2bf(ost[(size_t)qi * hd + lane + half] * inv);
            }
}

extern "C" int licv_append_attn(const licv_append_attn_args* x, void* stream) {
    LICV_CHECK_ARG(x && x->qkv_bf16 && x->cos && x->sin && x->position_ids && x->cache && x->out, "append_attn: null pointer");
    LICV_CHECK_ARG(x->T >= 1 && x->T <= LICV_APPEND_MAX_T, "append_attn: T = %lld new tokens per row (1 .. %d)", (long long)x->T, LICV_APPEND_MAX_T);
    LICV_CHECK_ARG(x->M > 0 && x->past >= 0 && x->past + x->T <= x->max_len, "append_attn: bad rows / past (%lld + %lld of %lld)",
                   (long long)x->past, (long long)x->T, (long long)x->max_len);
    LICV_CHECK_ARG(x->n_heads > 0 && x->n_kv_heads > 0 && x->n_heads % x->n_kv_heads == 0, "append_attn: n_heads must be a multiple of n_kv_heads");
    LICV_CHECK_ARG(x->head_dim >= 8 && x->head_dim <= 128 && x->head_dim % 8 == 0, "append_attn: head_dim %lld unsupported (multiple of 8, <= 128)", (long long)x->head_dim);
    LICV_CHECK_ARG(x->ldq >= (x->n_heads + 2 * x->n_kv_heads) * x->head_dim, "append_attn: ldq smaller than the fused row");
    LICV_CHECK_ARG(x->n_pos > 0 && x->n_pos <= INT_MAX, "append_attn: bad rotary table length %lld", (long long)x->n_pos);
    LICV_CHECK_ARG(((uintptr_t)x->cache & 15) == 0, "append_attn: the cache must be 16-byte aligned");
    LICV_CHECK_ARG(!x->kv_rows || x->ld_kv_rows >= x->past, "append_attn: kv_rows rows shorter than the history");
    LICV_CHECK_ARG(x->append == 0 || x->append == 1, "append_attn: append must be 0 or 1");
    AppendP p;
    p.qkv = (const bf16_t*)x->qkv_bf16; p.ldq = x->ldq;
    p.cosT = (const bf16_t*)x->cos; p.sinT = (const bf16_t*)x->sin; p.pos = x->position_ids; p.n_pos = x->n_pos;
    p.cache = (bf16_t*)x->cache; p.max_len = x->max_len; p.kv_rows = x->kv_rows; p.ld_rows = x->ld_kv_rows; p.key_valid = x->key_valid;
    p.out = (bf16_t*)x->out;
    LICV_CHECK_ARG((x->past + x->T) * (int64_t)sizeof(int) <= 40 * 1024, "append_attn: history of %lld keys exceeds the kernel's LDS budget", (long long)(x->past + x->T));
    p.M = (int)x->M; p.T = (int)x->T; p.Sk = (int)(x->past + x->T); p.past = (int)x->past; p.nh = (int)x->n_heads; p.nkv = (int)x->n_kv_heads;
    p.hd = (int)x->head_dim; p.append = x->append;
    p.scale = x->scale;
    // the whole query-head group in one workgroup where its state fits the CU's LDS, else the largest slice of it that does
    const int rep = p.nh / p.nkv;
    auto pick = [&](size_t budget) {
        for (int h = rep; h >= 1; --h)
            if (rep % h == 0 && APP_STATIC_LDS + append_lds_bytes(h, p.T, p.hd, p.Sk) <= budget) return h;
        return 0;
    };
    p.hpb = pick(APP_LDS_LARGE);
    LICV_CHECK_ARG(p.hpb > 0, "append_attn: T = %d tokens of head_dim %d over %d keys exceed the kernel's LDS budget", p.T, p.hd, p.Sk);
    if (APP_STATIC_LDS + append_lds_bytes(p.hpb, p.T, p.hd, p.Sk) > APP_LDS_SMALL) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(append_attn_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(APP_LDS_LARGE - APP_STATIC_LDS)) != hipSuccess) {
            (void)hipGetLastError();
            p.hpb = pick(APP_LDS_SMALL);                 // a runtime that will not grant more: smaller slices of the group
            LICV_CHECK_ARG(p.hpb > 0, "append_attn: T = %d tokens of head_dim %d over %d keys exceed the kernel's LDS budget", p.T, p.hd, p.Sk);
        }
    }
    const int64_t blocks = x->M * x->n_kv_heads * (rep / p.hpb);
    LICV_CHECK_ARG(blocks <= INT_MAX, "append_attn: %lld workgroups", (long long)blocks);
    const size_t lds = append_lds_bytes(p.hpb, p.T, p.hd, p.Sk);
    append_attn_k<<<dim3((unsigned)blocks), dim3(64), lds, (hipStream_t)stream>>>(p);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

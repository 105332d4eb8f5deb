// A decode step's self-attention block over a LONG history, as two launches: decode_attn_split_k cuts the key range of every
// (row, kv head) into splits of whole 64-key sweeps and leaves, per (row, query head, split), an un-normalised partial - the running
// max m (scaled, log2 domain; -inf where every key of the split is masked), the running sum l and head_dim fp32 output columns - in
// a workspace; decode_attn_merge_k combines the partials of a (row, query head) in split order and writes the bf16 row.  The
// arithmetic of a split is decode_attn_k's (csrc/decode.hip: same inputs, same rotary, one key per lane, the same 128-term fma
// chain, the same online softmax), so ONE split gives its bits; what differs is that nothing of the row table lives in LDS - a
// sweep's table entries and mask flags are read from memory when the sweep is requested (the NEXT sweep's are requested one sweep
// ahead, so they are no round trip of their own) - hence no limit on the history, and that a long history of few rows spreads over
// M * n_kv_heads * n_splits waves instead of M * n_kv_heads.
//
// Two launches on purpose: no workgroup waits for or signals another, no counters, no atomics, no fences; the result does not depend
// on how the workgroups were scheduled and an interrupted call leaves nothing behind that a later call could trip over.
//
// Workspace: float[M][n_heads][n_splits][head_dim + 2] = { m, l, o[0 .. head_dim) }.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_s;
#define DSP_VSTR 272                  // LDS stride of a V row (256 B + 16), as DEC_VSTR in decode.hip

struct DecodeSplitP {
    const float* ws; int splits; int64_t slice, stride;       // split-K slices of the QKV projection (ws == nullptr: qkv16)
    const bf16_t* qkv16; int64_t ldq;
    const bf16_t* cosT; const bf16_t* sinT; const int64_t* pos; int64_t n_pos;
    bf16_t* cache; int64_t max_len;
    const int32_t* kv_rows; int64_t ld_rows;
    const int32_t* key_valid;
    float* part;                                               // the partials (see above)
    bf16_t* out;
    int M, Sk, past, nh, nkv, hd;
    int n_splits, split_len;                                   // keys per split: a multiple of 64; n_splits * split_len >= Sk > (n_splits - 1) * split_len
    float scale;
};

// dec_in of decode.hip: one element of the fused QKV row, the bf16 value or bf16(slice 0 + slice 1 + ... in slice order)
__device__ __forceinline__ float dsp_in(const DecodeSplitP& a, int64_t row, int64_t col) {
    if (!a.ws) return bf2f(a.qkv16[row * a.ldq + col]);
    const float* p = a.ws + row * a.stride + col;
    float v = 0.f;
    for (int s0 = 0; s0 < a.splits; s0 += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(int64_t)min(s0 + u, a.splits - 1) * a.slice];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += (s0 + u < a.splits) ? t[u] : 0.f;
    }
    return rbf(v);
}

// physical cache row of key j of this row's history, -1 = masked or beyond the split (no memory is touched then)
__device__ __forceinline__ int dsp_entry(const int32_t* rows_r, const int32_t* valid_r, int r, int j, int j_end) {
    if (j >= j_end) return -1;
    const int pr = rows_r ? rows_r[j] : r;
    const int vd = valid_r ? valid_r[j] : 1;
    return vd != 0 ? pr : -1;
}

// One 64-lane wave per (row, kv head, split); the group's query heads one after the other, as decode_attn_k.
__global__ __launch_bounds__(64)
void decode_attn_split_k(DecodeSplitP a) {
    __shared__ __attribute__((aligned(16))) bf16_t qs[128];
    __shared__ __attribute__((aligned(16))) char vt[64 * DSP_VSTR];     // the sweep's V rows (bf16), one per key
    __shared__ float pch[64];                                            // ... and their probabilities
    const int lane = threadIdx.x;
    const int sp = blockIdx.x % a.n_splits;
    const int rg = blockIdx.x / a.n_splits;
    const int r = rg / a.nkv, g = rg % a.nkv;
    const int hd = a.hd, half = hd >> 1, rep = a.nh / a.nkv;
    const int64_t qd = (int64_t)a.nh * hd, kd = (int64_t)a.nkv * hd;
    const bool act = lane < half;
    const float sc = a.scale * 1.4426950408889634f;
    const int nch = hd >> 3;                            // 16-byte chunks per K / V row
    const int j_beg = sp * a.split_len, j_end = min(j_beg + a.split_len, a.Sk);
    const bool has_new = a.past >= j_beg && a.past < j_end;             // the split that holds the new token's own key
    const int32_t* rows_r = a.kv_rows ? a.kv_rows + (int64_t)r * a.ld_rows : nullptr;
    const int32_t* valid_r = a.key_valid ? a.key_valid + (int64_t)r * a.Sk : nullptr;
    // ---- memory round trip 1: the position, the first sweep's table entries, the raw elements of the first query head and - in the
    // split of the new token only - of K and V
    int64_t p = a.pos[r];
    const int e_first = dsp_entry(rows_r, valid_r, r, j_beg + lane, j_end);
    float klo = 0.f, khi = 0.f, v0 = 0.f, v1 = 0.f, qlo = 0.f, qhi = 0.f;
    if (act) {
        if (has_new) {
            klo = dsp_in(a, r, qd + (int64_t)g * hd + lane); khi = dsp_in(a, r, qd + (int64_t)g * hd + lane + half);
            v0 = dsp_in(a, r, qd + kd + (int64_t)g * hd + lane); v1 = dsp_in(a, r, qd + kd + (int64_t)g * hd + lane + half);
        }
        qlo = dsp_in(a, r, (int64_t)(g * rep) * hd + lane); qhi = dsp_in(a, r, (int64_t)(g * rep) * hd + lane + half);
    }
    // ---- round trip 2: cos / sin of the position
    p = p < 0 ? 0 : (p >= a.n_pos ? a.n_pos - 1 : p);
    const float c = act ? bf2f(a.cosT[p * hd + lane]) : 0.f, s = act ? bf2f(a.sinT[p * hd + lane]) : 0.f;
    // ---- the new token's K (rotated) and V of this kv head: written by ONE split, into the cache row of THIS beam row at position
    // `past`, and kept in registers (no split reads position `past` of any row from memory)
    float k0 = 0.f, k1 = 0.f;
    if (act && has_new) {
        bf16_t* crow = a.cache + ((int64_t)r * a.max_len + a.past) * 2 * kd + (int64_t)g * hd;
        k0 = rbf(rbf(klo * c) + rbf(-khi * s));
        k1 = rbf(rbf(khi * c) + rbf(klo * s));
        crow[lane] = f2bf(k0); crow[lane + half] = f2bf(k1);
        crow[kd + lane] = f2bf(v0); crow[kd + lane + half] = f2bf(v1);
    }
    for (int qh = 0; qh < rep; ++qh) {
        const int head = g * rep + qh;
        // ---- Q of this head, rotated; its score against the new key from registers
        float q0 = 0.f, q1 = 0.f;
        if (act) {
            const float lo = qh == 0 ? qlo : dsp_in(a, r, (int64_t)head * hd + lane), hi = qh == 0 ? qhi : dsp_in(a, r, (int64_t)head * hd + lane + half);
            q0 = rbf(rbf(lo * c) + rbf(-hi * s));
            q1 = rbf(rbf(hi * c) + rbf(lo * s));
            qs[lane] = f2bf(q0); qs[lane + half] = f2bf(q1);
        }
        const float s_new = wave_sum(q0 * k0 + q1 * k1);
        __syncthreads();
        u32x4_s qreg[16];
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) qreg[ch] = ch < nch ? reinterpret_cast<const u32x4_s*>(qs)[ch] : u32x4_s{0u, 0u, 0u, 0u};
        float m_run = -INFINITY, l_run = 0.f, o0 = 0.f, o1 = 0.f;
        int e_cur = qh == 0 ? e_first : dsp_entry(rows_r, valid_r, r, j_beg + lane, j_end);
        for (int j0 = j_beg; j0 < j_end; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < j_end;
            const int e_nxt = dsp_entry(rows_r, valid_r, r, j + 64, j_end);     // requested a sweep ahead of its use
            const int pr = e_cur;
            const bool ok = pr >= 0, own = in && j == a.past;
            u32x4_s kv[16], vv[16];
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) { kv[ch] = u32x4_s{0u, 0u, 0u, 0u}; vv[ch] = u32x4_s{0u, 0u, 0u, 0u}; }
            if (ok && !own) {       // a masked key fetches nothing (its score is -inf, its P is 0); the new token's key is in registers
                const bf16_t* rowp = a.cache + ((int64_t)pr * a.max_len + j) * 2 * kd + (int64_t)g * hd;
                const u32x4_s* kp = reinterpret_cast<const u32x4_s*>(rowp);
                const u32x4_s* vp = reinterpret_cast<const u32x4_s*>(rowp + kd);
#pragma unroll
                for (int ch = 0; ch < 16; ++ch) if (ch < nch) kv[ch] = kp[ch];
#pragma unroll
                for (int ch = 0; ch < 16; ++ch) if (ch < nch) vv[ch] = vp[ch];
            }
            float acc = 0.f;
#pragma unroll
            for (int ch = 0; ch < 16; ++ch)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc = __builtin_fmaf(__uint_as_float(kv[ch][e] << 16), __uint_as_float(qreg[ch][e] << 16), acc);
                    acc = __builtin_fmaf(__uint_as_float(kv[ch][e] & 0xffff0000u), __uint_as_float(qreg[ch][e] & 0xffff0000u), acc);
                }
            float sj = own ? s_new : acc;
            if (!ok) sj = -INFINITY;
            const float cmax = wave_max(sj);
            const float m_new = fmaxf(m_run, cmax * sc);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);            // m_run = -inf -> 0
            const float pj = __builtin_amdgcn_exp2f(__builtin_fmaf(sj, sc, -m_use));
            l_run = l_run * alpha + wave_sum(pj);
            m_run = m_new;
            __syncthreads();                                                      // the previous sweep's readers are done with vt / pch
            pch[lane] = rbf(pj);
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) if (ch < nch) *reinterpret_cast<u32x4_s*>(vt + lane * DSP_VSTR + ch * 16) = vv[ch];
            __syncthreads();
            o0 *= alpha; o1 *= alpha;
            if (act) {
                const int nk = min(64, j_end - j0);
                for (int jj = 0; jj < nk; ++jj) {
                    const float pv = pch[jj];
                    const bf16_t* vr = reinterpret_cast<const bf16_t*>(vt + jj * DSP_VSTR);
                    const bool ownj = (j0 + jj == a.past);                        // the new token's V comes from registers
                    const bool live = pv != 0.f;                                  // (a masked key contributes nothing, whatever its cache row holds)
                    o0 = __builtin_fmaf(pv, live ? (ownj ? v0 : bf2f(vr[lane])) : 0.f, o0);
                    o1 = __builtin_fmaf(pv, live ? (ownj ? v1 : bf2f(vr[lane + half])) : 0.f, o1);
                }
            }
            e_cur = e_nxt;
        }
        float* pp = a.part + (((int64_t)r * a.nh + head) * a.n_splits + sp) * (hd + 2);
        if (lane == 0) { pp[0] = m_run; pp[1] = l_run; }
        if (act) { pp[2 + lane] = o0; pp[2 + lane + half] = o1; }
        __syncthreads();                               // qs / vt / pch are rewritten by the next query head
    }
}

// One 64-lane wave per (row, query head): Mx = max m_s; w_s = exp2(m_s - Mx) (0 for a fully masked split); L = sum w_s l_s and
// O = sum w_s o_s in increasing s; out = bf16(O * (1 / L)), 0 where L is not positive.  One split: w = 1, so bf16(o * (1 / l)).
__global__ __launch_bounds__(64)
void decode_attn_merge_k(const float* __restrict__ part, bf16_t* __restrict__ out, int n_splits, int hd) {
    const int lane = threadIdx.x, half = hd >> 1;
    const float* pp = part + (int64_t)blockIdx.x * n_splits * (hd + 2);
    const bool act = lane < half;
    const int c0 = act ? lane : 0;
    float mx = -INFINITY;
    for (int s = 0; s < n_splits; ++s) mx = fmaxf(mx, pp[(int64_t)s * (hd + 2)]);
    float L = 0.f, o0 = 0.f, o1 = 0.f;
    for (int s = 0; s < n_splits; ++s) {
        const float* ps = pp + (int64_t)s * (hd + 2);
        const float m = ps[0];
        const float w = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - mx);
        const float wl = w * ps[1], w0 = w * ps[2 + c0], w1 = w * ps[2 + c0 + half];
        if (s == 0) { L = wl; o0 = w0; o1 = w1; }
        else { L += wl; o0 += w0; o1 += w1; }
    }
    if (act) {
        const float inv = L > 0.f ? 1.0f / L : 0.f;
        bf16_t* op = out + (int64_t)blockIdx.x * hd;
        op[lane] = f2bf(o0 * inv); op[lane + half] = f2bf(o1 * inv);
    }
}

static int64_t dsp_sweeps(int64_t Sk) { return (Sk + 63) / 64; }

// sweeps per split and the number of non-empty splits for a wish of n splits (1 <= n <= sweeps)
static void dsp_layout(int64_t sweeps, int64_t n, int64_t* per, int64_t* n_eff) {
    *per = (sweeps + n - 1) / n;
    *n_eff = (sweeps + *per - 1) / *per;
}

static int64_t dsp_plan(int64_t M, int64_t n_kv_heads, int64_t Sk) {
    // The split kernel runs one wave per (row, kv head, split), and 2048 of them are resident at once: 256 CUs x 8 workgroups
    // (17.5 KiB of LDS and 179 VGPRs each).  Measured (tools/decode_attn_bench.py): the time falls with the number of
    // splits until the waves fill that, stays flat beyond, and rises a little where they spill into a second, partly filled round -
    // so the largest n with M * n_kv_heads * n <= 2048.  A split may be as short as one sweep: its fixed cost (the QKV elements,
    // the rotary, the partial's store and the merge's load) stayed below what a second sweep in line costs.
    const int64_t sweeps = dsp_sweeps(Sk), waves = M * n_kv_heads;
    int64_t n = 2048 / waves;
    const int64_t cap = sweeps < LICV_DECODE_MAX_SPLITS ? sweeps : LICV_DECODE_MAX_SPLITS;
    if (n > cap) n = cap;
    if (n < 1) n = 1;
    int64_t per, n_eff;
    dsp_layout(sweeps, n, &per, &n_eff);
    return n_eff;
}

extern "C" int64_t licv_decode_attn_split_plan(int64_t M, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim, int64_t Sk, int* n_splits) {
    if (M <= 0 || n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || Sk <= 0) {
        if (n_splits) *n_splits = 0;
        return 0;
    }
    const int64_t n = dsp_plan(M, n_kv_heads, Sk);
    if (n_splits) *n_splits = (int)n;
    return M * n_heads * n * (head_dim + 2) * 4;
}

extern "C" int licv_decode_attn_split(const licv_decode_attn_args* x, int n_splits, void* workspace, int64_t workspace_bytes, void* stream) {
    LICV_CHECK_ARG(x && (x->qkv_ws || x->qkv_bf16) && x->cos && x->sin && x->position_ids && x->cache && x->out, "decode_attn_split: null pointer");
    LICV_CHECK_ARG(x->M > 0 && x->past >= 0 && x->past < x->max_len, "decode_attn_split: bad rows / past (%lld of %lld)", (long long)x->past, (long long)x->max_len);
    LICV_CHECK_ARG(x->past < INT32_MAX - 64, "decode_attn_split: past %lld does not fit the kernel's key index", (long long)x->past);
    LICV_CHECK_ARG(x->n_heads > 0 && x->n_kv_heads > 0 && x->n_heads % x->n_kv_heads == 0, "decode_attn_split: n_heads must be a multiple of n_kv_heads");
    LICV_CHECK_ARG(x->head_dim >= 16 && x->head_dim <= 128 && x->head_dim % 16 == 0, "decode_attn_split: head_dim %lld unsupported (multiple of 16, <= 128)", (long long)x->head_dim);
    LICV_CHECK_ARG(!x->qkv_ws || (x->splits >= 1 && x->slice_elems > 0 && x->row_stride > 0), "decode_attn_split: bad split-K workspace description");
    LICV_CHECK_ARG(x->qkv_ws || x->ldq >= (x->n_heads + 2 * x->n_kv_heads) * x->head_dim, "decode_attn_split: ldq smaller than the fused row");
    LICV_CHECK_ARG(((uintptr_t)x->cache & 15) == 0, "decode_attn_split: the cache must be 16-byte aligned");
    LICV_CHECK_ARG(!x->kv_rows || x->ld_kv_rows > x->past, "decode_attn_split: kv_rows rows shorter than the history");
    LICV_CHECK_ARG(n_splits <= LICV_DECODE_MAX_SPLITS, "decode_attn_split: n_splits %d above LICV_DECODE_MAX_SPLITS (%d)", n_splits, LICV_DECODE_MAX_SPLITS);
    const int64_t Sk = x->past + 1, sweeps = dsp_sweeps(Sk);
    int64_t n = n_splits <= 0 ? dsp_plan(x->M, x->n_kv_heads, Sk) : n_splits;
    if (n > sweeps) n = sweeps;
    const int64_t need = x->M * x->n_heads * n * (x->head_dim + 2) * 4;
    LICV_CHECK_ARG(workspace, "decode_attn_split: null workspace (%lld bytes needed for %lld splits)", (long long)need, (long long)n);
    LICV_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "decode_attn_split: the workspace must be 16-byte aligned");
    LICV_CHECK_ARG(workspace_bytes >= need, "decode_attn_split: workspace of %lld bytes, %lld needed for %lld splits", (long long)workspace_bytes,
                   (long long)need, (long long)n);
    int64_t per, n_eff;
    dsp_layout(sweeps, n, &per, &n_eff);               // no empty split: n_eff <= n, so the partials fit the checked size
    LICV_CHECK_ARG(x->M * x->n_kv_heads * n_eff <= INT32_MAX && x->M * x->n_heads <= INT32_MAX, "decode_attn_split: too many rows for one launch");
    DecodeSplitP p;
    p.ws = x->qkv_ws; p.splits = x->splits; p.slice = x->slice_elems; p.stride = x->row_stride;
    p.qkv16 = (const bf16_t*)x->qkv_bf16; p.ldq = x->ldq;
    p.cosT = (const bf16_t*)x->cos; p.sinT = (const bf16_t*)x->sin; p.pos = x->position_ids; p.n_pos = x->n_pos;
    p.cache = (bf16_t*)x->cache; p.max_len = x->max_len; p.kv_rows = x->kv_rows; p.ld_rows = x->ld_kv_rows; p.key_valid = x->key_valid;
    p.part = (float*)workspace; p.out = (bf16_t*)x->out;
    p.M = (int)x->M; p.Sk = (int)Sk; p.past = (int)x->past; p.nh = (int)x->n_heads; p.nkv = (int)x->n_kv_heads; p.hd = (int)x->head_dim;
    p.n_splits = (int)n_eff; p.split_len = (int)(per * 64);
    p.scale = x->scale;
    decode_attn_split_k<<<dim3((unsigned)(x->M * x->n_kv_heads * n_eff)), dim3(64), 0, (hipStream_t)stream>>>(p);
    LICV_LAUNCH_CHECK();
    decode_attn_merge_k<<<dim3((unsigned)(x->M * x->n_heads)), dim3(64), 0, (hipStream_t)stream>>>(p.part, p.out, (int)n_eff, p.hd);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

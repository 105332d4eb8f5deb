// One decode step of sampled generate without beams (ref:inference.py:300-321 -> transformers GenerationMixin._sample with
// do_sample=True, generation/utils.py:2794-2930) as ONE launch: per row (one 1024-lane workgroup) EOS suppression, temperature, the
// top-k / top-p / min-p kept set (sample_common.h), the inverse-CDF draw over the kept tokens in token-id order, the pad id for
// finished rows, the unfinished flags, and the loop's "continue" flag combined by the last workgroup.
#include "sample_common.h"

template <int NPT>
__global__ __launch_bounds__(SAMPLE_THREADS)
void sample_step_k(licv_sample_step_args a, licv_sample_params p) {
    __shared__ SampleSmem s;
    const int r = blockIdx.x, tid = threadIdx.x;
    const bool live = a.unfinished[r] != 0;
    int64_t tok = a.pad;
    if (live) {                                            // (uniform over the workgroup)
        const int V = (int)a.V, npt = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS, base = tid * npt;
        const int64_t row = (int64_t)r * a.ld;
        uint32_t kk[NPT];
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int i = base + j;
            uint32_t k = 0;
            if (j < npt && i < V) {
                float x = a.logits_dtype == LICV_F32 ? reinterpret_cast<const float*>(a.logits)[row + i]
                                                     : bf2f(reinterpret_cast<const bf16_t*>(a.logits)[row + i]);
                if (a.suppress_eos && i == a.eos) x = -INFINITY;
                k = f2key(x / p.temperature);
            }
            kk[j] = k;
        }
        const SampleFilter f{p.temperature, p.top_k, p.top_p, p.min_p, 1};
        float m;
        const KeptSet S = row_filter(kk, npt, base, V, f, &m, s);
        // inverse CDF in token-id order: the smallest id whose prefix mass exceeds floor(u * total)
        unsigned long long loc = 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S)) loc += mass_fix(key2f(kk[j]), m);
        unsigned long long Z;
        const unsigned long long ex = sblk_excl(loc, s, &Z);
        const double u = philox_uniform(philox_x0(p.seed, (uint32_t)(a.cur - a.P), (uint32_t)r, 0u, 0u));
        unsigned long long target = (unsigned long long)floor(u * (double)Z);
        if (target >= Z) target = Z - 1;
        if (ex <= target && target < ex + loc) {
            unsigned long long run = ex;
#pragma unroll
            for (int j = 0; j < NPT; ++j)
                if (j < npt && kk[j] != 0 && kept_in(kk[j], base + j, S)) {
                    run += mass_fix(key2f(kk[j]), m);
                    if (run > target) { s.bi = base + j; break; }
                }
        }
        __syncthreads();
        tok = s.bi;
    }
    if (tid == 0) {
        a.ids[(int64_t)r * a.ids_ld + a.cur] = tok;
        a.next_tokens[r] = tok;
        const bool unf = live && !(a.eos >= 0 && tok == a.eos);
        a.unfinished[r] = unf ? 1 : 0;
        if (unf) atomicAdd(&a.sync[1], 1);
        __threadfence();
        const int arrived = atomicAdd(&a.sync[0], 1);
        if (arrived == (int)gridDim.x - 1) {
            const int n_unf = atomicExch(&a.sync[1], 0);
            atomicExch(&a.sync[0], 0);
            a.flags[0] = (n_unf > 0 && a.cur + 1 < a.max_len) ? 1 : 0;
        }
    }
}

extern "C" int licv_sample_step(const licv_sample_step_args* x, const licv_sample_params* p, void* stream) {
    LICV_CHECK_ARG(x && p && x->logits && x->ids && x->unfinished && x->next_tokens && x->flags && x->sync, "sample_step: null pointer");
    LICV_CHECK_ARG(x->logits_dtype == LICV_BF16 || x->logits_dtype == LICV_F32, "sample_step: bad logits dtype");
    LICV_CHECK_ARG(x->B >= 1 && x->B <= INT_MAX && x->V >= 1 && x->V <= SAMPLE_MAX_V && x->ld >= x->V,
                   "sample_step: bad batch / vocabulary size (V %lld, at most %d)", (long long)x->V, SAMPLE_MAX_V);
    LICV_CHECK_ARG(x->cur >= x->P && x->cur < x->max_len && x->P >= 1 && x->ids_ld >= x->max_len,
                   "sample_step: position %lld outside [P, max_len)", (long long)x->cur);
    LICV_CHECK_ARG(p->temperature > 0.0f, "sample_step: temperature %g must be > 0", (double)p->temperature);
    LICV_CHECK_ARG(p->top_k >= 0, "sample_step: top_k %lld must be >= 0", (long long)p->top_k);
    LICV_CHECK_ARG(p->top_p > 0.0f && p->top_p <= 1.0f, "sample_step: top_p %g outside (0, 1]", (double)p->top_p);
    LICV_CHECK_ARG(p->min_p >= 0.0f && p->min_p <= 1.0f, "sample_step: min_p %g outside [0, 1]", (double)p->min_p);
    // vocabulary entries per lane in registers: 32 up to V = 32768, 64 above
    if (x->V <= SAMPLE_THREADS * 32) sample_step_k<32><<<dim3((unsigned)x->B), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream>>>(*x, *p);
    else sample_step_k<SAMPLE_NPT><<<dim3((unsigned)x->B), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream>>>(*x, *p);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

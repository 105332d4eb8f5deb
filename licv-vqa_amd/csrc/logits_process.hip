// The logits processors of hooked generate as ONE launch per decode step (licv_logits_process, include/licv_hip.h): transformers 5.x
// RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and
// SuppressTokensAtBeginLogitsProcessor (generation/logits_process.py) in _get_logits_processor's order, on the raw logits (_sample)
// or on their fp32 log-softmax (_beam_search).
//
// One 1024-lane workgroup per output row.  The row is read ONCE into registers (lane t holds tokens t, t + 1024, ...: coalesced);
// meanwhile two V-bit maps are built in LDS from the row's token history and the lists: `seen` (the tokens the penalty applies to:
// a token that occurs twice is penalised once, as hf's scatter writes the same value twice) and `ban`.  With normalize the
// workgroup reduces max and sum of exp over the registers.  Every output is then one IEEE operation on the mode's input value:
// -inf if banned, else s * t or s / t if seen, else s.  The work is small (R <= 64 rows of 32002 entries, a history of a few
// thousand tokens): the kernel is latency-bound, so it is one launch with no host sync rather than a bandwidth design.
#include "common.h"
#include <limits.h>

#define LP_THREADS 1024
#define LP_MAX_V 65536
#define LP_WORDS (LP_MAX_V / 32)

__device__ __forceinline__ void lp_mark(uint32_t* map, int64_t t, int V) {
    if (t >= 0 && t < V) atomicOr(&map[t >> 5], 1u << (t & 31));
}

template <int NPT>
__global__ __launch_bounds__(LP_THREADS)
void logits_process_k(licv_logits_process_args a) {
    __shared__ uint32_t s_ban[LP_WORDS], s_seen[LP_WORDS];
    __shared__ float red[LP_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = (int)a.V;
    const int64_t cur = a.cur;
    const int64_t row = ((int64_t)(r / a.nb) * a.q_stride_rows + (int64_t)(r % a.nb) * a.beam_stride_rows) * a.ld;
    float x[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int i = tid + j * LP_THREADS;
        x[j] = i >= V ? -INFINITY : a.logits_dtype == LICV_F32 ? reinterpret_cast<const float*>(a.logits)[row + i]
                                                               : bf2f(reinterpret_cast<const bf16_t*>(a.logits)[row + i]);
    }
    const int words = (V + 31) >> 5;
    for (int i = tid; i < words; i += LP_THREADS) { s_ban[i] = 0u; s_seen[i] = 0u; }
    __syncthreads();
    const int64_t* h = a.ids + (int64_t)r * a.ids_ld;
    const bool penal = a.repetition_penalty != 1.0f;
    if (penal) for (int64_t i = tid; i < cur; i += LP_THREADS) lp_mark(s_seen, h[i], V);
    const int64_t n = a.no_repeat_ngram_size;
    if (n > 0 && cur >= n) {                                    // windows [i, i + n) inside the history; the suffix is h[cur-n+1 .. cur-1]
        const int64_t* suf = h + (cur - n + 1);
        for (int64_t i = tid; i <= cur - n; i += LP_THREADS) {
            bool m = true;
            for (int64_t j = 0; j < n - 1 && m; ++j) m = h[i + j] == suf[j];
            if (m) lp_mark(s_ban, h[i + n - 1], V);
        }
    }
    for (int64_t w = tid; w < a.n_bad_words; w += LP_THREADS) {
        const int64_t o0 = a.bad_offsets[w], o1 = a.bad_offsets[w + 1], L = o1 - o0;
        if (o0 < 0 || L < 1 || o1 > a.bad_words_len) continue;  // (the host checked its copy of the offsets; never read past the list)
        bool m = L <= cur;                                      // hf ignores a word longer than the history
        if (L == 1) m = true;
        for (int64_t j = 0; j < L - 1 && m; ++j) m = h[cur - (L - 1) + j] == (int64_t)a.bad_words[o0 + j];
        if (m) lp_mark(s_ban, a.bad_words[o1 - 1], V);
    }
    for (int64_t i = tid; i < a.n_suppress; i += LP_THREADS) lp_mark(s_ban, a.suppress[i], V);
    if (cur == a.P) for (int64_t i = tid; i < a.n_begin_suppress; i += LP_THREADS) lp_mark(s_ban, a.begin_suppress[i], V);
    if (a.normalize) {                                          // fp32 log-softmax: (x - max) - log(sum exp(x - max))
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NPT; ++j) mx = fmaxf(mx, x[j]);
        mx = wave_max(mx);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
        for (int w = 1; w < LP_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < NPT; ++j) if (tid + j * LP_THREADS < V) z += expf(x[j] - mx);
        z = wave_sum(z);
        __syncthreads();
        if (lane == 0) red[wave] = z;
        __syncthreads();
        z = red[0];
        for (int w = 1; w < LP_THREADS / 64; ++w) z += red[w];
        const float lse = logf(z);
#pragma unroll
        for (int j = 0; j < NPT; ++j) x[j] = (x[j] - mx) - lse;
    }
    __syncthreads();                                            // the maps are complete
    float* o = a.out + (int64_t)r * a.out_ld;
    const float t = a.repetition_penalty;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int i = tid + j * LP_THREADS;
        if (i < V) {
            const uint32_t bit = 1u << (i & 31);
            float v = x[j];
            if (s_ban[i >> 5] & bit) v = -INFINITY;
            else if (penal && (s_seen[i >> 5] & bit)) v = v < 0.f ? v * t : v / t;
            o[i] = v;
        }
    }
}

extern "C" int licv_logits_process(const licv_logits_process_args* x, void* stream) {
    LICV_CHECK_ARG(x && x->logits && x->ids && x->out, "logits_process: null pointer");
    LICV_CHECK_ARG(x->logits_dtype == LICV_BF16 || x->logits_dtype == LICV_F32, "logits_process: bad logits dtype");
    LICV_CHECK_ARG(x->V >= 1 && x->V <= LP_MAX_V, "logits_process: vocabulary %lld outside 1..%d", (long long)x->V, LP_MAX_V);
    LICV_CHECK_ARG(x->B >= 1 && x->nb >= 1 && x->B * x->nb <= INT_MAX && x->ld >= x->V && x->out_ld >= x->V && x->q_stride_rows >= 0 &&
                   x->beam_stride_rows >= 0, "logits_process: bad batch size, row stride or row addressing");
    LICV_CHECK_ARG(x->P >= 0 && x->cur >= x->P && x->cur <= x->ids_ld, "logits_process: position %lld outside [P, ids_ld]", (long long)x->cur);
    LICV_CHECK_ARG(x->repetition_penalty > 0.0f, "logits_process: repetition_penalty %g must be > 0", (double)x->repetition_penalty);
    LICV_CHECK_ARG(x->no_repeat_ngram_size >= 0, "logits_process: no_repeat_ngram_size %lld must be >= 0", (long long)x->no_repeat_ngram_size);
    LICV_CHECK_ARG(x->n_bad_words >= 0 && x->bad_words_len >= 0 && x->n_suppress >= 0 && x->n_begin_suppress >= 0, "logits_process: negative list length");
    LICV_CHECK_ARG((x->n_bad_words == 0 || (x->bad_words && x->bad_offsets && x->bad_offsets_host)) && (x->n_suppress == 0 || x->suppress) &&
                   (x->n_begin_suppress == 0 || x->begin_suppress), "logits_process: a list has a length but no pointer");
    if (x->n_bad_words > 0) {
        LICV_CHECK_ARG(x->bad_offsets_host[0] == 0 && x->bad_offsets_host[x->n_bad_words] == x->bad_words_len,
                       "logits_process: bad-word offsets must start at 0 and end at bad_words_len");
        for (int64_t w = 0; w < x->n_bad_words; ++w)
            LICV_CHECK_ARG(x->bad_offsets_host[w + 1] > x->bad_offsets_host[w], "logits_process: bad-word offsets out of order at word %lld", (long long)w);
    }
    const dim3 grid((unsigned)(x->B * x->nb)), block(LP_THREADS);
    if (x->V <= LP_THREADS * 32) logits_process_k<32><<<grid, block, 0, (hipStream_t)stream>>>(*x);
    else logits_process_k<LP_MAX_V / LP_THREADS><<<grid, block, 0, (hipStream_t)stream>>>(*x);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

// Image resize on the device, bit-equal to Pillow's 8-bit resampler (Pillow src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc over the coefficients of precompute_coeffs + normalize_coeffs_8bpc), which is what transformers'
// PIL-backed image processors call (ref:icv_src/utils/mm_topk_retriver.py -> CLIPImageProcessor; ref:icv_src/icv_datamodule.py ->
// the Idefics processors).  The coefficients are fixed point with 22 fractional bits and come from the HOST (licv.frontend.resample_plan:
// a contracted FMA in the filter polynomial could move one by a unit); the passes are integer arithmetic and therefore exact here:
//     byte = clip8((2^21 + sum_k pixel[xmin + k] * coef[k]) >> 22)          int32 accumulator, arithmetic shift
// horizontal first, rounded to uint8, then vertical; each pass only where that axis changes size.
//   * resize_horizontal_k : the source rows the vertical pass will read, the columns the crop keeps -> uint8 workspace rows
//                           (16-byte aligned stride).  Pixels are 3 bytes and rows start anywhere: R row segments are staged in LDS
//                           with aligned 16-byte loads, one thread per output pixel reads its taps from there, and the finished rows
//                           leave as 16-byte stores.
//   * resize_vertical_k   : vertical pass over the workspace (or straight over the source where no horizontal pass ran), 4 bytes per
//                           thread, + crop + padding, then either uint8 HWC or the normalised bf16 CHW of image_preprocess_k (same
//                           table, image_table.h) + mask.
// No scratch, no atomics; images are independent (blockIdx.y = image), so a ragged batch is one pair of launches.
#include "common.h"
#include "image_table.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_BITS = 22;                      // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int RS_HALF = 1 << (RS_BITS - 1);
constexpr int RS_TABLE_BYTES = 3 * 256 * (int)sizeof(bf16_t);
constexpr int64_t RS_MAX_SIDE = 1 << 20;
constexpr int64_t RS_MAX_LDS = 64 * 1024;

__host__ __device__ __forceinline__ int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// clip8(acc >> 22) with the clamp in front of the shift (the shift is monotone, so the two orders agree).  Written this way on purpose:
// clamp(acc >> 22, 0, 255) packed two to a dword is selected as v_ashr_pk_u8_i32 on gfx950, which leaves the upper half of its
// destination as it was, and the bytes OR-ed in above it came out wrong on the device.
__device__ __forceinline__ int clip8(int acc) { return clampi(acc, 0, (256 << RS_BITS) - 1) >> RS_BITS; }

// The source rows [r0, r1) that the vertical pass reads for the crop's rows (all of them where the height does not change).  A plan's
// xmin and xmin + count never decrease, so the first and the last crop row bound the range.  Values are clamped to the image: a
// plan that is not one cannot send a load out of bounds.
__device__ __forceinline__ void rows_needed(const licv_resize_desc& d, const int32_t* __restrict__ plans, int& r0, int& r1) {
    const int h = (int)d.h, top = (int)d.top, ch = (int)d.ch;
    if (d.oh != d.h) {
        const int32_t* vxmin = plans + d.vplan_offset;
        const int32_t* vcount = vxmin + d.oh;
        r0 = clampi(vxmin[top], 0, h);
        r1 = clampi(vxmin[top + ch - 1] + vcount[top + ch - 1], r0, h);
    } else {
        r0 = top;
        r1 = top + ch;
    }
}

__global__ __launch_bounds__(RS_THREADS)
void resize_horizontal_k(const unsigned char* __restrict__ src, int64_t src_bytes, const licv_resize_desc* __restrict__ desc,
                         const int32_t* __restrict__ plans, unsigned char* __restrict__ ws, int R, int seg_stride, int out_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const licv_resize_desc d = desc[blockIdx.y];
    if (d.h <= 0 || d.w <= 0 || d.w == d.ow || d.ch <= 0 || d.cw <= 0) return;         // missing image / no horizontal pass: block-uniform
    const int tid = threadIdx.x;
    const int w = (int)d.w, ow = (int)d.ow, left = (int)d.left, cw = (int)d.cw, hk = (int)d.hplan_ksize;
    const int32_t* hxmin = plans + d.hplan_offset;
    const int32_t* hcount = hxmin + ow;
    const int32_t* hcoef = hcount + ow;
    int r0, r1;
    rows_needed(d, plans, r0, r1);
    const int c0 = clampi(hxmin[left], 0, w);                                           // source columns the kept output columns read
    const int c1 = clampi(hxmin[left + cw - 1] + hcount[left + cw - 1], c0, w);
    const int segbytes = 3 * (c1 - c0);
    const int tmp_ld = (int)align16(3 * (int64_t)cw);
    unsigned char* seg = sm;
    unsigned char* orow = sm + (int64_t)R * seg_stride;
    unsigned char* tmp = ws + d.ws_offset;
    const int64_t g0 = d.src_offset + d.x0_bytes + 3 * (int64_t)c0;

    for (int rb = r0 + (int)blockIdx.x * R; rb < r1; rb += (int)gridDim.x * R) {
        const int nr = min(R, r1 - rb);
        // (1) stage the row segments: 16-byte chunks at aligned addresses (the last chunk of the whole buffer byte by byte)
        for (int r = 0; r < nr; ++r) {
            const int64_t g = g0 + (int64_t)(rb + r) * d.src_ld_bytes;
            const int64_t ga = g & ~(int64_t)15;
            const int nchunk = (int)((g + segbytes - ga + 15) >> 4);
            for (int i = tid; i < nchunk; i += RS_THREADS) {
                const int64_t a = ga + 16 * (int64_t)i;
                uint4 v;
                if (a + 16 <= src_bytes) {
                    v = *reinterpret_cast<const uint4*>(src + a);
                } else {
                    uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (a + j < src_bytes) q[j >> 2] |= (uint32_t)src[a + j] << (8 * (j & 3));
                    v = make_uint4(q[0], q[1], q[2], q[3]);
                }
                *reinterpret_cast<uint4*>(seg + (int64_t)r * seg_stride + 16 * i) = v;
            }
        }
        __syncthreads();
        // (2) one output pixel per thread: its taps out of LDS, three accumulators
        for (int it = tid; it < nr * cw; it += RS_THREADS) {
            const int r = it / cw, x = it - r * cw, xo = left + x;
            const int xm = clampi(hxmin[xo], c0, c1);
            const int cnt = min(min(hcount[xo], hk), c1 - xm);
            const int32_t* kk = hcoef + (int64_t)xo * hk;
            const int shift = (int)((g0 + (int64_t)(rb + r) * d.src_ld_bytes) & 15);
            const unsigned char* p = seg + (int64_t)r * seg_stride + shift + 3 * (xm - c0);
            int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF;
            for (int k = 0; k < cnt; ++k) {
                const int c = kk[k];
                a0 += (int)p[3 * k] * c;
                a1 += (int)p[3 * k + 1] * c;
                a2 += (int)p[3 * k + 2] * c;
            }
            unsigned char* o = orow + (int64_t)r * out_stride + 3 * x;
            o[0] = (unsigned char)clip8(a0);
            o[1] = (unsigned char)clip8(a1);
            o[2] = (unsigned char)clip8(a2);
        }
        __syncthreads();
        // (3) the finished rows leave as 16-byte stores (the workspace's row stride is a multiple of 16; the pad bytes carry no meaning)
        const int nq = tmp_ld >> 4;
        for (int i = tid; i < nr * nq; i += RS_THREADS) {
            const int r = i / nq, q = i - r * nq;
            *reinterpret_cast<uint4*>(tmp + (int64_t)(rb + r) * tmp_ld + 16 * q) =
                *reinterpret_cast<const uint4*>(orow + (int64_t)r * out_stride + 16 * q);
        }
        // no third barrier: a thread reaches the next round's writes to `orow` only through the barrier after (1), i.e. after every
        // thread has left (3); and (1) writes `seg`, which nobody reads after the barrier in front of (3)
    }
}

// 4 bytes of a row at byte offset 4 j.  The workspace's rows are 16-byte aligned and padded, the source's are neither: there the load
// is unaligned and the last, partial dword of a row is read byte by byte (it may be the last of the buffer).
template <bool WS>
__device__ __forceinline__ uint32_t load4(const unsigned char* p, int remaining) {
    if (WS) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
    if (remaining >= 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int j = 0; j < remaining; ++j) v |= (uint32_t)p[j] << (8 * j);
    }
    return v;
}

template <bool WS>
__device__ __forceinline__ void vertical_row(const unsigned char* __restrict__ in, int64_t in_ld, int ym, int cnt, const int32_t* __restrict__ kk,
                                             bool vres, int rowbytes, unsigned char* __restrict__ row) {
    const int ndw = (rowbytes + 3) >> 2;
    for (int j = threadIdx.x; j < ndw; j += RS_THREADS) {
        const int remaining = rowbytes - 4 * j;
        const unsigned char* p = in + (int64_t)ym * in_ld + 4 * j;
        uint32_t res;
        if (vres) {
            int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF, a3 = RS_HALF;
            for (int k = 0; k < cnt; ++k) {
                const uint32_t v = load4<WS>(p + (int64_t)k * in_ld, remaining);
                const int c = kk[k];
                a0 += (int)(v & 255u) * c;
                a1 += (int)((v >> 8) & 255u) * c;
                a2 += (int)((v >> 16) & 255u) * c;
                a3 += (int)(v >> 24) * c;
            }
            res = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24);
        } else {
            res = load4<WS>(p, remaining);
        }
        *reinterpret_cast<uint32_t*>(row + 4 * j) = res;
    }
}

template <bool BF16>
__global__ __launch_bounds__(RS_THREADS)
void resize_vertical_k(const unsigned char* __restrict__ src, const licv_resize_desc* __restrict__ desc, const int32_t* __restrict__ plans,
                       const unsigned char* __restrict__ ws, void* __restrict__ out, unsigned char* __restrict__ mask, int H, int W,
                       ImageTable tb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    bf16_t* table = reinterpret_cast<bf16_t*>(sm);                                      // [3][256]
    unsigned char* row = sm + RS_TABLE_BYTES;                                           // one finished row of the crop, 3 * cw bytes
    const int tid = threadIdx.x;
    if (BF16) {
#pragma unroll
        for (int c = 0; c < 3; ++c) table[c * 256 + tid] = tb.v[c][tid];                // 256 threads: one byte value each
    }
    const int64_t img = blockIdx.y;
    const licv_resize_desc d = desc[img];
    const bool missing = d.h <= 0 || d.w <= 0;
    const int h = (int)d.h, top = (int)d.top, ch = missing ? 0 : (int)d.ch, cw = missing ? 0 : (int)d.cw;
    const bool hres = !missing && d.w != d.ow, vres = !missing && d.h != d.oh;
    const int vk = (int)d.vplan_ksize, oh = (int)d.oh;
    const int32_t* vxmin = plans + (vres ? d.vplan_offset : 0);
    const int32_t* vcount = vxmin + oh;
    const int32_t* vcoef = vcount + oh;
    const unsigned char* in = hres ? ws + d.ws_offset : src + d.src_offset + d.x0_bytes + 3 * d.left;
    const int64_t in_ld = hres ? align16(3 * (int64_t)cw) : d.src_ld_bytes;
    const int rowbytes = 3 * cw;
    const int64_t plane = (int64_t)H * W;
    __syncthreads();
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        if (y < ch) {                                                                    // block-uniform
            int ym = top + y, cnt = 1;
            const int32_t* kk = vcoef;
            if (vres) {
                ym = clampi(vxmin[top + y], 0, h);
                cnt = min(min(vcount[top + y], vk), h - ym);
                kk = vcoef + (int64_t)(top + y) * vk;
            }
            if (hres) vertical_row<true>(in, in_ld, ym, cnt, kk, vres, rowbytes, row);
            else vertical_row<false>(in, in_ld, ym, cnt, kk, vres, rowbytes, row);
        }
        __syncthreads();
        if (BF16) {
            bf16_t* dst = reinterpret_cast<bf16_t*>(out) + img * plane * 3 + (int64_t)y * W;
            for (int x = tid; x < W; x += RS_THREADS) {
                const bool real = y < ch && x < cw;
                bf16_t r = 0, g = 0, b = 0;
                if (real) {
                    r = table[row[3 * x]];
                    g = table[256 + row[3 * x + 1]];
                    b = table[512 + row[3 * x + 2]];
                }
                dst[x] = r;
                dst[plane + x] = g;
                dst[2 * plane + x] = b;
                if (mask) mask[img * plane + (int64_t)y * W + x] = real ? 1 : 0;
            }
        } else {
            unsigned char* dst = reinterpret_cast<unsigned char*>(out) + (img * H + y) * (int64_t)W * 3;
            const int valid = y < ch ? rowbytes : 0;
            if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {          // 3 W bytes per row: whole dwords
                for (int q = tid; q < (3 * W) >> 2; q += RS_THREADS) {
                    const int nv = clampi(valid - 4 * q, 0, 4);
                    uint32_t v = nv ? *reinterpret_cast<const uint32_t*>(row + 4 * q) : 0u;
                    if (nv < 4) v &= (1u << (8 * nv)) - 1u;
                    reinterpret_cast<uint32_t*>(dst)[q] = v;
                }
            } else {
                for (int j = tid; j < 3 * W; j += RS_THREADS) dst[j] = j < valid ? row[j] : (unsigned char)0;
            }
            if (mask)
                for (int x = tid; x < W; x += RS_THREADS) mask[img * plane + (int64_t)y * W + x] = (y < ch && x < cw) ? 1 : 0;
        }
        __syncthreads();
    }
}

struct ResizeLayout { int64_t ws_bytes, max_w, max_cw; bool any_h; };

// Argument checks shared by the size query and the call; fills the workspace layout (offset i = sum of the sizes before i).
int resize_check(const licv_resize_desc* d, int64_t n, int64_t H, int64_t W, bool geometry_only, int64_t src_bytes, int64_t plan_elems,
                 ResizeLayout* lay, licv_resize_desc* write_offsets) {
    LICV_CHECK_ARG(d, "resize_images: null descriptors");
    LICV_CHECK_ARG(n >= 0 && n <= 65535, "resize_images: %lld images (at most 65535 per call)", (long long)n);
    lay->ws_bytes = 0; lay->max_w = 0; lay->max_cw = 0; lay->any_h = false;
    for (int64_t i = 0; i < n; ++i) {
        const licv_resize_desc& e = d[i];
        LICV_CHECK_ARG(e.h >= 0 && e.w >= 0 && e.h <= RS_MAX_SIDE && e.w <= RS_MAX_SIDE, "resize_images: image %lld: bad size %lld x %lld",
                       (long long)i, (long long)e.h, (long long)e.w);
        if (write_offsets) write_offsets[i].ws_offset = lay->ws_bytes;
        else LICV_CHECK_ARG(e.ws_offset == lay->ws_bytes, "resize_images: image %lld: ws_offset %lld, %lld expected (licv_resize_images_workspace)",
                            (long long)i, (long long)e.ws_offset, (long long)lay->ws_bytes);
        if (e.h == 0 || e.w == 0) continue;                                               // a missing image: all padding
        LICV_CHECK_ARG(e.oh >= 1 && e.ow >= 1 && e.oh <= RS_MAX_SIDE && e.ow <= RS_MAX_SIDE, "resize_images: image %lld: bad resized size %lld x %lld",
                       (long long)i, (long long)e.oh, (long long)e.ow);
        LICV_CHECK_ARG(e.top >= 0 && e.left >= 0 && e.ch >= 0 && e.cw >= 0 && e.top + e.ch <= e.oh && e.left + e.cw <= e.ow,
                       "resize_images: image %lld: crop (top %lld, left %lld, %lld x %lld) outside the resized image %lld x %lld", (long long)i,
                       (long long)e.top, (long long)e.left, (long long)e.ch, (long long)e.cw, (long long)e.oh, (long long)e.ow);
        if (H >= 0)
            LICV_CHECK_ARG(e.ch <= H && e.cw <= W, "resize_images: image %lld: crop %lld x %lld larger than the frame %lld x %lld", (long long)i,
                           (long long)e.ch, (long long)e.cw, (long long)H, (long long)W);
        if (!geometry_only) {
            LICV_CHECK_ARG(e.src_offset >= 0 && e.x0_bytes >= 0 && e.src_ld_bytes >= e.x0_bytes + 3 * e.w &&
                           e.src_offset + (e.h - 1) * e.src_ld_bytes + e.x0_bytes + 3 * e.w <= src_bytes,
                           "resize_images: image %lld: offset %lld, row stride %lld, x0 %lld do not fit %lld x %lld in %lld bytes", (long long)i,
                           (long long)e.src_offset, (long long)e.src_ld_bytes, (long long)e.x0_bytes, (long long)e.h, (long long)e.w, (long long)src_bytes);
            if (e.w != e.ow)
                LICV_CHECK_ARG(e.hplan_ksize >= 1 && e.hplan_offset >= 0 && e.hplan_offset + e.ow * (2 + e.hplan_ksize) <= plan_elems,
                               "resize_images: image %lld: horizontal plan (offset %lld, ksize %lld) outside the %lld plan elements", (long long)i,
                               (long long)e.hplan_offset, (long long)e.hplan_ksize, (long long)plan_elems);
            if (e.h != e.oh)
                LICV_CHECK_ARG(e.vplan_ksize >= 1 && e.vplan_offset >= 0 && e.vplan_offset + e.oh * (2 + e.vplan_ksize) <= plan_elems,
                               "resize_images: image %lld: vertical plan (offset %lld, ksize %lld) outside the %lld plan elements", (long long)i,
                               (long long)e.vplan_offset, (long long)e.vplan_ksize, (long long)plan_elems);
        }
        if (e.w != e.ow && e.ch > 0 && e.cw > 0) {
            lay->any_h = true;
            lay->ws_bytes += e.h * align16(3 * e.cw);
            lay->max_w = e.w > lay->max_w ? e.w : lay->max_w;
            lay->max_cw = e.cw > lay->max_cw ? e.cw : lay->max_cw;
        }
    }
    return LICV_OK;
}

}  // namespace

extern "C" int licv_resize_images_workspace(licv_resize_desc* desc_host, int64_t n_images, int64_t* bytes) {
    LICV_CHECK_ARG(bytes, "resize_images_workspace: null pointer");
    ResizeLayout lay;
    if (int st = resize_check(desc_host, n_images, -1, -1, true, 0, 0, &lay, desc_host)) return st;
    *bytes = lay.ws_bytes;
    return LICV_OK;
}

extern "C" int licv_resize_images(const void* src_u8, int64_t src_bytes, const licv_resize_desc* desc_host, const licv_resize_desc* desc_dev,
                                  int64_t n_images, const int32_t* plans, int64_t plan_elems, int64_t H, int64_t W, void* out_u8, void* out_bf16,
                                  void* mask_u8, double rescale, const float* mean3, const float* std3, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    LICV_CHECK_ARG(H > 0 && W > 0 && H * W < (1ll << 31) && 3 * W + 16 + RS_TABLE_BYTES <= RS_MAX_LDS, "resize_images: bad frame %lld x %lld",
                   (long long)H, (long long)W);
    LICV_CHECK_ARG((out_u8 != nullptr) != (out_bf16 != nullptr), "resize_images: exactly one of out_u8 / out_bf16");
    ResizeLayout lay;
    if (int st = resize_check(desc_host, n_images, H, W, false, src_bytes, plan_elems, &lay, nullptr)) return st;
    if (n_images == 0) return LICV_OK;
    LICV_CHECK_ARG(desc_dev && (src_u8 || src_bytes == 0) && (plans || plan_elems == 0), "resize_images: null pointer");
    LICV_CHECK_ARG(((uintptr_t)src_u8 & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "resize_images: src / workspace must be 16-byte aligned");
    LICV_CHECK_ARG(workspace_bytes >= lay.ws_bytes && (workspace || lay.ws_bytes == 0),
                   "resize_images: workspace of %lld bytes, %lld needed (licv_resize_images_workspace)", (long long)workspace_bytes, (long long)lay.ws_bytes);
    ImageTable tb = {};
    if (out_bf16) {
        LICV_CHECK_ARG(mean3 && std3, "resize_images: null mean / std");
        LICV_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "resize_images: zero std");
        tb = build_image_table(rescale, mean3, std3);
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t per_image = 2048 / n_images > 1 ? 2048 / n_images : 1;                 // blocks per image: ~2048 in all, grid-stride the rest
    if (lay.any_h) {
        const int64_t seg_stride = align16(3 * lay.max_w + 32), out_stride = align16(3 * lay.max_cw);
        int R = 4;
        if (R * (seg_stride + out_stride) > RS_MAX_LDS / 2) R = 1;
        if (R * (seg_stride + out_stride) > RS_MAX_LDS)
            return licv_set_error(LICV_E_UNSUPPORTED, "resize_images: a source row of %lld pixels does not fit the LDS staging", (long long)lay.max_w);
        int64_t max_h = 0;
        for (int64_t i = 0; i < n_images; ++i) max_h = desc_host[i].h > max_h ? desc_host[i].h : max_h;
        int64_t bx = (max_h + R - 1) / R;
        bx = bx > per_image ? per_image : bx;
        resize_horizontal_k<<<dim3((unsigned)bx, (unsigned)n_images), RS_THREADS, (size_t)(R * (seg_stride + out_stride)), st>>>(
            (const unsigned char*)src_u8, src_bytes, desc_dev, plans, (unsigned char*)workspace, R, (int)seg_stride, (int)out_stride);
        LICV_LAUNCH_CHECK();
    }
    const int64_t by = H > per_image ? per_image : H;
    const size_t lds = (size_t)(RS_TABLE_BYTES + align16(3 * W) + 16);
    if (out_bf16)
        resize_vertical_k<true><<<dim3((unsigned)by, (unsigned)n_images), RS_THREADS, lds, st>>>(
            (const unsigned char*)src_u8, desc_dev, plans, (const unsigned char*)workspace, out_bf16, (unsigned char*)mask_u8, (int)H, (int)W, tb);
    else
        resize_vertical_k<false><<<dim3((unsigned)by, (unsigned)n_images), RS_THREADS, lds, st>>>(
            (const unsigned char*)src_u8, desc_dev, plans, (const unsigned char*)workspace, out_u8, (unsigned char*)mask_u8, (int)H, (int)W, tb);
    LICV_LAUNCH_CHECK();
    return LICV_OK;
}

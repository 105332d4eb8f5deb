// The 3 x 256 table of normalised bf16 values of a byte, shared by every kernel that turns uint8 pixels into pixel_values
// (frontend.hip image_preprocess_k, resize.hip): hf:image_transforms.py rescale :118-122 = f32(f64(u8) * f64 scale), normalize :437 =
// (x - f32 mean) / f32 std, computed on the HOST with exactly those IEEE operations and rounded once to bf16, handed to the kernel by
// value (1.5 KB of kernel arguments).
#pragma once
#include <cstring>
#include "common.h"

struct ImageTable { bf16_t v[3][256]; };

static inline ImageTable build_image_table(double rescale, const float* mean3, const float* std3) {
    ImageTable tb;
    for (int v = 0; v < 256; ++v) {
        const volatile float x = (float)((double)v * rescale);        // hf:image_transforms.py:118-122 (volatile: one rounding per step,
        for (int c = 0; c < 3; ++c) {                                 //  no wider intermediate, whatever the host compiler's flags)
            const volatile float d = x - mean3[c];
            const volatile float q = d / std3[c];                     // :437
            uint32_t u; float qf = q; memcpy(&u, &qf, 4);
            tb.v[c][v] = (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);      // round to nearest even (finite values only)
        }
    }
    return tb;
}

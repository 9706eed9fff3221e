// conv_i8.hpp — launch interface of the int8 matrix-pipe convolution (conv_i8.hip) of HP_DTYPE_I8 engines and of the
// calibration reduction.  Activations stay fp16 NHWC in HBM (conv_kernels.hpp); the kernel quantizes its input tile while it
// stages it, multiplies int8 x int8 on v_mfma_i32_32x32x32_i8 with exact int32 sums, and hands (float)acc * dq[c] to the fp16
// engine's epilogue (conv_epilogue.hpp), which adds the bias and does everything else exactly as for an fp16 layer.
#pragma once
#include "conv_kernels.hpp"

namespace hp {

struct conv_i8_params {
    conv_params c;      // the layer as the fp16 engine describes it (geometry, bias, activation, residual, outputs); c.w / ksplit unused
    const int8_t* w;    // q_w, rows [tap][c.Cout_pad][c.Cin] (zero rows / columns beyond Cout / the layer's real input channels)
    const float* dq;    // [c.Cout_pad] s_a * s_w[c], 0 beyond Cout
    float inv_a;        // 1 / s_a: q_x = clamp(rint(x * inv_a), -127, 127)
    const int8_t* w_direct; // conv_i8_direct_kernel's copy of q_w in MFMA-fragment order (conv_i8_direct_index), or nullptr
};

// the layers conv_i8_kernel is built for: 1 x 1 at stride 1 | 2, 3 x 3 at stride 1 | 2 and dilation 1 | 2, 7 x 7 at stride 1
bool conv_i8_ok(int kh, int kw, int stride, int dil);
// the layers conv_i8_direct_kernel takes (3 x 3 / 7 x 7, stride 1, dilation 1, whole 64-channel chunks, 128-row output tiles): the halo tile
// of a channel chunk is quantized into LDS once per block and re-used by every tap
bool conv_i8_direct_ok(const conv_params& p);
// byte of q_w[tap][m][c] in the direct form's weights: [tap][c / 64][(c % 64) / 32][m / 32][lane = (c % 32) / 16 * 32 + m % 32][c % 16]
inline size_t conv_i8_direct_index(int tap, int m, int c, int cin, int cout_pad)
{
    return (((((size_t)tap * (cin / 64) + c / 64) * 2 + (c % 64) / 32) * (cout_pad / 32) + m / 32) * 64 + (c % 32) / 16 * 32 + m % 32) * 16 + c % 16;
}
hipError_t launch_conv_i8(const conv_i8_params& p, hipStream_t s);
// profile tile code (hp_layer_time::tile): 8000000 + BM * 1000 + BK for conv_i8_kernel, 8900000 + K for conv_i8_direct_kernel
int conv_i8_tile(const conv_params& p);

// max |x| over the valid pixels of channels [0, C) of an fp16 view, frames [0, B), folded into *amax (the float's bits, unsigned max:
// every |x| is >= 0, so the order of the bit patterns is the order of the values)
hipError_t launch_absmax(const tview& t, int B, int H, int W, int C, unsigned* amax, hipStream_t s);

} // namespace hp

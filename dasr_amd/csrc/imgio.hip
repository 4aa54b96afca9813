// Input stage of the evaluation datasets on the device, gfx950 (reference: codes/SRN/data/util.py:78-96 read_img, :133-145 modcrop, :243-433 imresize_np as
// codes/SRN/data/LRHR_dataset.py:44-126 and LR_dataset.py use them in the val / test phase; host restatement: dasr_amd/data.py load_image, imresize_matlab):
//  * u8_to_planar: the decoded image as PIL hands it over (uint8, HWC, RGB) -> the top-left Hc x Wc window (modcrop) as planar fp32 in [0, 1]
//  * imresize_down: MATLAB-style antialiased bicubic down-sampling by an integer s, as two gather passes over per-axis tap tables (index and fp64 weight,
//    4 s + 2 taps per output sample) the host builds once per (length, s): rows first into an fp64 intermediate, then columns, ONE rounding to fp32 at the end
// Both are memory-bound (about 36 multiply-adds per output sample at s = 4 against 2 x 18 gathered reads), so the kernels are plain: one thread per output
// sample, the x index on the lanes so that loads and stores of a wave are contiguous (pass 2 reads with a stride of s samples inside one row of the
// intermediate, which the 18-tap overlap of neighbouring outputs keeps in cache), no LDS, no atomics.
//
// fp contraction is off for the whole file: every product is rounded to fp64 before it is added, in tap order, so the result does not depend on what the
// compiler fuses.  The file must not be built with fast-math or approximate-division flags: `u / 255.0f` is the correctly rounded fp32 division numpy does.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// one thread: one pixel of the window, three channels.  src [H][W][3] (row stride W * 3 bytes); dst [3][Hc][Wc]
__global__ __launch_bounds__(256) void u8_to_planar_kernel(const uint8_t* __restrict__ src, int W, int Hc, int Wc, float* __restrict__ dst) {
    const long long HWc = (long long)Hc * Wc;
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= HWc) return;
    const int y = (int)(gi / Wc), x = (int)(gi - (long long)y * Wc);
    const uint8_t* p = src + ((size_t)y * W + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * HWc + gi] = (float)p[c] / 255.0f;
}

// pass 1, along H: tmp[c][oy][x] = sum over t (in order) of wt[oy][t] * src[c][idx[oy][t]][x].  grid (ceil(W / 256), Ho, C); the taps of a row are
// uniform over the workgroup.  TAPS = 4 s + 2 is a template argument so that the gathers of one output are unrolled and in flight together.
template <int TAPS>
__global__ __launch_bounds__(256) void imresize_rows_kernel(const float* __restrict__ src, int H, int W, int Ho, const int32_t* __restrict__ idx,
                                                            const double* __restrict__ wt, double* __restrict__ tmp) {
    const int x = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, c = blockIdx.z;
    if (x >= W) return;
    const float* plane = src + (size_t)c * H * W;
    const int32_t* ji = idx + (size_t)oy * TAPS;
    const double* jw = wt + (size_t)oy * TAPS;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
        const int j = min(max(ji[t], 0), H - 1);   // (the host tables are mirrored into range already: a damaged table reads a wrong row, never outside the image)
        acc += jw[t] * (double)plane[(size_t)j * W + x];
    }
    tmp[((size_t)c * Ho + oy) * W + x] = acc;
}

// pass 2, along W: dst[c][oy][ox] = (float) sum over t (in order) of wt[ox][t] * tmp[c][oy][idx[ox][t]].  grid (ceil(Wo / 256), Ho, C)
template <int TAPS>
__global__ __launch_bounds__(256) void imresize_cols_kernel(const double* __restrict__ tmp, int W, int Ho, int Wo, const int32_t* __restrict__ idx,
                                                            const double* __restrict__ wt, float* __restrict__ dst) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, c = blockIdx.z;
    if (ox >= Wo) return;
    const double* row = tmp + ((size_t)c * Ho + oy) * W;
    const int32_t* ji = idx + (size_t)ox * TAPS;
    const double* jw = wt + (size_t)ox * TAPS;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
        const int j = min(max(ji[t], 0), W - 1);
        acc += jw[t] * row[j];
    }
    dst[((size_t)c * Ho + oy) * Wo + ox] = (float)acc;
}

template <int TAPS>
int imresize_launch(const float* src, int C, int H, int W, int s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, double* tmp,
                    float* dst, void* stream) {
    const int Ho = H / s, Wo = W / s;
    auto rows = imresize_rows_kernel<TAPS>;
    auto cols = imresize_cols_kernel<TAPS>;
    DASR_LAUNCH_TAG("imresize_rows_kernel", rows, dim3((W + 255) / 256, Ho, C), dim3(256), 0, as_stream(stream), src, H, W, Ho, idx_h, w_h, tmp);
    DASR_LAUNCH_TAG("imresize_cols_kernel", cols, dim3((Wo + 255) / 256, Ho, C), dim3(256), 0, as_stream(stream), (const double*)tmp, W, Ho, Wo, idx_w, w_w, dst);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dasr_u8_to_planar(const uint8_t* src, int32_t H, int32_t W, int32_t Hc, int32_t Wc, float* dst, void* stream) {
    if (!src || !dst || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0 || Hc > H || Wc > W || H > 65535 || W > 65535) return DASR_EINVAL;
    const long long total = (long long)Hc * Wc;
    DASR_LAUNCH(u8_to_planar_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), src, W, Hc, Wc, dst);
    return (int)hipGetLastError();
}

extern "C" int dasr_imresize_down(const float* src, int32_t C, int32_t H, int32_t W, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                                  const double* w_w, double* tmp, float* dst, void* stream) {
    if (!src || !idx_h || !w_h || !idx_w || !w_w || !tmp || !dst || C <= 0 || C > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return DASR_EINVAL;
    if (s < 2 || s > 4 || H % s || W % s) return DASR_EINVAL;
    return s == 2 ? imresize_launch<10>(src, C, H, W, s, idx_h, w_h, idx_w, w_w, tmp, dst, stream)
         : s == 3 ? imresize_launch<14>(src, C, H, W, s, idx_h, w_h, idx_w, w_w, tmp, dst, stream)
                  : imresize_launch<18>(src, C, H, W, s, idx_h, w_h, idx_w, w_w, tmp, dst, stream);
}

// Image-quality metrics of the SRN validation / evaluation drivers on the device, gfx950 (reference: codes/SRN/utils/util.py:180-204 tensor2img,
// :236-291 calculate_psnr / ssim / calculate_ssim, codes/SRN/data/util.py:169-190 bgr2ycbcr; host restatement: dasr_amd/util.py):
//  * tensor2img: fp32 NCHW image -> uint8, HWC BGR (what save_img takes) and / or planar CHW (what the metric kernels read); NaN -> 0, counted
//  * squared error over the cropped region: the integer sum over all channels (RGB PSNR) and the fp64 sum on the Y channel (PSNR_Y)
//  * SSIM (11 x 11 Gaussian window, sigma 1.5, 'valid' region of the cropped images), fp64, on the uint8 planes or on the Y channel
// and of the folder evaluator (reference: codes/DSN/evaluate.py:44-46; host side: dasr_amd/metrics.py pair_metrics_u8):
//  * SSIM in scikit-image's form (7 x 7 uniform window, sample covariance) from exact integer window sums, one fp64 evaluation per window
//  * the exact integer sum of the bytes of every channel (the mean colour of PSNR_col)
// Every sum over the grid is two launches: one partial per workgroup (plain stores into the caller's workspace), then one workgroup per image that adds
// the partials in index order.  The kernel boundary orders the two, so there is no in-launch hand-off and no floating-point atomic: the same inputs give
// the same bits run to run.  The work is small (two 8 MB images, under 3 GFLOP of fp64 at 1356 x 2040), so the kernels are plain: one LDS-staged tile
// per workgroup, 64-lane waves, no assembly.
//
// fp contraction is off for the whole file: the quantisation must round the product `q * 255.0f` before rint (as numpy does), and the Y channel is
// defined by the host's sequence of individually rounded fp64 operations.  The file must not be built with fast-math or approximate-division flags
// (the fp32 division of the quantisation is the correctly rounded one).
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SSIM_K = 11;          // window
constexpr int SSIM_TH = 16;         // output tile: 16 rows x 32 columns, two outputs per thread
constexpr int SSIM_TW = 32;
constexpr int SSIM_IH = SSIM_TH + SSIM_K - 1;   // 26 input rows
constexpr int SSIM_IW = SSIM_TW + SSIM_K - 1;   // 42 input columns
constexpr int SSE_MAX_BLOCKS = 512;             // row-interleaved workgroups per image of the squared-error kernel

struct ssim_window { double w[SSIM_K]; };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the 256 threads of the workgroup in a fixed order (xor butterfly inside a wave, the four waves in index order); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red4) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

__device__ __forceinline__ long long block_sum_i64(long long v, long long* red4) {
    v = wave_sum_i64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// the value test.py compares on the Y channel: bgr2ycbcr's float branch on u / 255 (float32(u / 255.) * 255.0f == u for all 256 values), then `* 255`
__device__ __forceinline__ double y_of(int r, int g, int b) {
    const double dot = (24.966 * (double)b + 128.553 * (double)g) + 65.481 * (double)r;
    return ((dot / 255.0 + 16.0) / 255.0) * 255.0;
}

// one thread: one pixel, all channels.  x [N][C][H][W] fp32; hwc [N][H][W][C] with the channel order reversed; planar [N][C][H][W]
__global__ void tensor2img_u8_kernel(const float* __restrict__ x, int C, long long HW, long long total, float lo, float hi, float range,
                                     uint8_t* __restrict__ hwc, uint8_t* __restrict__ planar, int* __restrict__ nan_count) {
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int nans = 0;
    if (gi < total) {
        const long long n = gi / HW, p = gi - n * HW;
        for (int c = 0; c < C; ++c) {
            const float v = x[(n * C + c) * HW + p];
            uint8_t u = 0;
            if (v != v) {
                ++nans;
            } else {
                const float q = (fminf(fmaxf(v, lo), hi) - lo) / range;
                u = (uint8_t)(int)rintf(q * 255.0f);   // round half to even, like numpy's .round()
            }
            if (planar) planar[(n * C + c) * HW + p] = u;
            if (hwc) hwc[gi * C + (C - 1 - c)] = u;
        }
    }
    if (nan_count) {   // integer atomics: the count does not depend on the order
        const int w = (int)wave_sum_i64(nans);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(nan_count, w);
    }
}

// Squared error of two planar uint8 images over rows [crop, H - crop) x columns [crop, W - crop): workgroup g of image n takes the cropped rows g, g + G, ...;
// a thread takes the columns t, t + 256, ... of each and all channels of a pixel.  part_i[n * G + g]: integer sum over all channels; part_y[n * G + g]: fp64 sum of the
// squared Y difference (C == 3 only).
__global__ void img_sse_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int C, int H, int W, int crop,
                               long long* __restrict__ part_i, double* __restrict__ part_y) {
    __shared__ double red_d[4];
    __shared__ long long red_i[4];
    const int n = blockIdx.y, G = gridDim.x;
    const int h = H - 2 * crop, w = W - 2 * crop;
    const size_t HW = (size_t)H * W;
    const uint8_t* pa = a + (size_t)n * C * HW;
    const uint8_t* pb = b + (size_t)n * C * HW;
    long long si = 0;
    double sy = 0.0;
    for (int r = blockIdx.x; r < h; r += G) {
        const size_t row = (size_t)(r + crop) * W + crop;
        for (int xx = threadIdx.x; xx < w; xx += 256) {
            int va[3] = {0, 0, 0}, vb[3] = {0, 0, 0};
            for (int c = 0; c < C; ++c) {
                va[c] = pa[c * HW + row + xx];
                vb[c] = pb[c * HW + row + xx];
                const int d = va[c] - vb[c];
                si += d * d;
            }
            if (part_y) {
                const double dy = y_of(va[0], va[1], va[2]) - y_of(vb[0], vb[1], vb[2]);
                sy += dy * dy;
            }
        }
    }
    const long long ti = block_sum_i64(si, red_i);
    if (threadIdx.x == 0) part_i[(size_t)n * G + blockIdx.x] = ti;
    if (part_y) {
        const double ty = block_sum_f64(sy, red_d);
        if (threadIdx.x == 0) part_y[(size_t)n * G + blockIdx.x] = ty;
    }
}

// second stage of every grid sum: one workgroup per image adds its G partials in a fixed order (thread t: t, t + 256, ...; then block_sum).
// out_d[n] = sum / div (div 1: the sum itself); either pair may be null.
__global__ void img_reduce_kernel(const long long* __restrict__ part_i, const double* __restrict__ part_d, int G, long long* __restrict__ out_i,
                                  double* __restrict__ out_d, double div) {
    __shared__ double red_d[4];
    __shared__ long long red_i[4];
    const int n = blockIdx.x;
    if (part_i) {
        long long s = 0;
        for (int i = threadIdx.x; i < G; i += 256) s += part_i[(size_t)n * G + i];
        s = block_sum_i64(s, red_i);
        if (threadIdx.x == 0) out_i[n] = s;
    }
    if (part_d) {
        double s = 0.0;
        for (int i = threadIdx.x; i < G; i += 256) s += part_d[(size_t)n * G + i];
        s = block_sum_f64(s, red_d);
        if (threadIdx.x == 0) out_d[n] = s / div;
    }
}

// SSIM map of one 16 x 32 tile of the valid region of one channel (YMODE: of the Y channel formed from the three planes), summed.
// grid (tiles_x * tiles_y, channels, N).  The 26 x 42 input patch of both images is staged in LDS as fp64 once; the window is applied separably (rows, then
// columns) to the five moment maps a, b, a^2, b^2, a b.  part[(n * channels + ch) * tiles + tile] = sum of the SSIM map over the tile's pixels inside the region.
template <bool YMODE>
__global__ __launch_bounds__(256) void img_ssim_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int C, int H, int W, int crop, int tiles_x,
                                                       ssim_window win, double* __restrict__ part) {
    __shared__ double sa[SSIM_IH][SSIM_IW + 1];
    __shared__ double sb[SSIM_IH][SSIM_IW + 1];
    __shared__ double hm[5][SSIM_IH][SSIM_TW];
    __shared__ double red_d[4];
    const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int h = H - 2 * crop, w = W - 2 * crop;          // cropped image
    const int hv = h - (SSIM_K - 1), wv = w - (SSIM_K - 1);   // valid region
    const int oy = (tile / tiles_x) * SSIM_TH, ox = (tile % tiles_x) * SSIM_TW;
    const size_t HW = (size_t)H * W;
    const uint8_t* pa = a + (size_t)n * C * HW;
    const uint8_t* pb = b + (size_t)n * C * HW;
    for (int i = threadIdx.x; i < SSIM_IH * SSIM_IW; i += 256) {
        const int r = i / SSIM_IW, c = i - r * SSIM_IW;
        const int iy = oy + r, ix = ox + c;
        double va = 0.0, vb = 0.0;   // outside the cropped image: feeds only outputs outside the valid region, which are not summed
        if (iy < h && ix < w) {
            const size_t p = (size_t)(iy + crop) * W + (ix + crop);
            if (YMODE) {
                va = y_of(pa[p], pa[HW + p], pa[2 * HW + p]);
                vb = y_of(pb[p], pb[HW + p], pb[2 * HW + p]);
            } else {
                va = (double)pa[ch * HW + p];
                vb = (double)pb[ch * HW + p];
            }
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SSIM_IH * SSIM_TW; i += 256) {
        const int r = i / SSIM_TW, c = i - r * SSIM_TW;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const double va = sa[r][c + k], vb = sb[r][c + k], wk = win.w[k];
            m[0] += wk * va;
            m[1] += wk * vb;
            m[2] += wk * (va * va);
            m[3] += wk * (vb * vb);
            m[4] += wk * (va * vb);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hm[q][r][c] = m[q];
    }
    __syncthreads();
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double s = 0.0;
    for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += 256) {
        const int r = i / SSIM_TW, c = i - r * SSIM_TW;
        if (oy + r >= hv || ox + c >= wv) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const double wk = win.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += wk * hm[q][r + k][c];
        }
        const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
        const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        s += ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
    }
    const double t = block_sum_f64(s, red_d);
    if (threadIdx.x == 0) part[((size_t)n * gridDim.y + ch) * gridDim.x + tile] = t;
}

constexpr int BOX_K = 7;            // window of the box SSIM
constexpr int BOX_TH = 32;          // output tile: 32 rows x 64 columns, eight outputs (one column, eight rows) per thread
constexpr int BOX_TW = 64;
constexpr int BOX_IH = BOX_TH + BOX_K - 1;   // 38 input rows: the tile and its 6-pixel apron
constexpr int BOX_IW = BOX_TW + BOX_K - 1;   // 70 input columns
constexpr int BOX_PITCH = 72;                // bytes per staged row

// SSIM of one 7 x 7 window from its five integer sums (skimage.measure.compare_ssim: uniform filter, use_sample_covariance, data_range 255).
// The integers are exact and fit 32 bits: Sx <= 49 * 255 = 12 495, Sxx <= 49 * 255^2 = 3 186 225, and the largest intermediate, 49 * Sxx or Sx^2, is
// 156 125 025 < 2^31.  The formula is evaluated once, in fp64, from them: the value does not depend on how the image was cut into tiles.
// With u = S / n and v = (n Sxx - Sx^2) / (n (n - 1)), S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) is evaluated with the first factor of
// numerator and denominator multiplied by n^2 and the second by n (n - 1): the integer parts enter exactly and ONE division is left (six otherwise).
__device__ __forceinline__ double box_ssim_of(int sx, int sy, int sxx, int syy, int sxy) {
    const double K1 = ((0.01 * 255) * (0.01 * 255)) * (49.0 * 49.0), K2 = ((0.03 * 255) * (0.03 * 255)) * (49.0 * 48.0);
    const double dx = (double)(49 * sxx - sx * sx), dy = (double)(49 * syy - sy * sy), dxy = (double)(49 * sxy - sx * sy);
    const double pxx = (double)(sx * sx), pyy = (double)(sy * sy), pxy = (double)(sx * sy);
    return ((2.0 * pxy + K1) * (2.0 * dxy + K2)) / ((pxx + pyy + K1) * (dx + dy + K2));
}

// Box SSIM map of one 32 x 64 tile of the window positions of one channel, summed.  grid (tiles_x * tiles_y, C, N).  The 38 x 70 bytes under the tile (with the
// 6-pixel apron) of both images are staged in LDS; row sums over 7 columns of a, b, a^2, b^2, a b are formed there as integers (a and b share a word: both are
// under 2^16, also after the column sum), then every thread walks 8 rows of one column with a running column sum (integers: adding a row and dropping one is exact).
// part[(n * C + ch) * tiles + tile] = sum of the map over the tile's window positions inside the cropped image.
__global__ __launch_bounds__(256) void img_ssim_box_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int C, int H, int W, int crop, int tiles_x,
                                                           double* __restrict__ part) {
    __shared__ uint8_t sa[BOX_IH][BOX_PITCH];
    __shared__ uint8_t sb[BOX_IH][BOX_PITCH];
    __shared__ int hs[4][BOX_IH][BOX_TW];   // row sums: a | b << 16, a^2, b^2, a b
    __shared__ double red_d[4];
    const int tile = blockIdx.x, ch = blockIdx.y, n = blockIdx.z;
    const int h = H - 2 * crop, w = W - 2 * crop;          // cropped image
    const int hv = h - (BOX_K - 1), wv = w - (BOX_K - 1);   // window positions
    const int oy = (tile / tiles_x) * BOX_TH, ox = (tile % tiles_x) * BOX_TW;
    const size_t HW = (size_t)H * W;
    const uint8_t* pa = a + ((size_t)n * C + ch) * HW;
    const uint8_t* pb = b + ((size_t)n * C + ch) * HW;
    for (int i = threadIdx.x; i < BOX_IH * BOX_IW; i += 256) {
        const int r = i / BOX_IW, c = i - r * BOX_IW;
        const int iy = oy + r, ix = ox + c;
        uint8_t va = 0, vb = 0;   // outside the cropped image: feeds only window positions outside it, which are not summed
        if (iy < h && ix < w) {
            const size_t p = (size_t)(iy + crop) * W + (ix + crop);
            va = pa[p];
            vb = pb[p];
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BOX_IH * BOX_TW; i += 256) {
        const int r = i / BOX_TW, c = i - r * BOX_TW;
        int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#pragma unroll
        for (int k = 0; k < BOX_K; ++k) {
            const int va = sa[r][c + k], vb = sb[r][c + k];
            m0 += va | (vb << 16);
            m1 += va * va;
            m2 += vb * vb;
            m3 += va * vb;
        }
        hs[0][r][c] = m0;
        hs[1][r][c] = m1;
        hs[2][r][c] = m2;
        hs[3][r][c] = m3;
    }
    __syncthreads();
    const int c = threadIdx.x & (BOX_TW - 1), r0 = (threadIdx.x >> 6) * 8;   // a wave: 64 columns of the same 8 rows
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#pragma unroll
    for (int k = 0; k < BOX_K - 1; ++k) {
        m0 += hs[0][r0 + k][c];
        m1 += hs[1][r0 + k][c];
        m2 += hs[2][r0 + k][c];
        m3 += hs[3][r0 + k][c];
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // window rows r0 + j .. r0 + j + 6 (at most row 37)
        m0 += hs[0][r0 + j + 6][c];
        m1 += hs[1][r0 + j + 6][c];
        m2 += hs[2][r0 + j + 6][c];
        m3 += hs[3][r0 + j + 6][c];
        if (oy + r0 + j < hv && ox + c < wv) s += box_ssim_of(m0 & 0xffff, m0 >> 16, m1, m2, m3);
        m0 -= hs[0][r0 + j][c];
        m1 -= hs[1][r0 + j][c];
        m2 -= hs[2][r0 + j][c];
        m3 -= hs[3][r0 + j][c];
    }
    const double t = block_sum_f64(s, red_d);
    if (threadIdx.x == 0) part[((size_t)n * gridDim.y + ch) * gridDim.x + tile] = t;
}

// Sum of the bytes of one plane (image n, channel c: blockIdx.x = n * C + c) over rows [crop, H - crop) x columns [crop, W - crop): workgroup g = blockIdx.y of
// the plane takes the cropped rows g, g + G, ...;  part[plane * G + g]
__global__ void img_channel_sums_kernel(const uint8_t* __restrict__ a, int H, int W, int crop, long long* __restrict__ part) {
    __shared__ long long red_i[4];
    const int G = gridDim.y;
    const int h = H - 2 * crop, w = W - 2 * crop;
    const uint8_t* p = a + (size_t)blockIdx.x * H * W;
    long long s = 0;
    for (int r = blockIdx.y; r < h; r += G) {
        const size_t row = (size_t)(r + crop) * W + crop;
        int rs = 0;   // a thread's share of a row: at most 128 bytes
        for (int xx = threadIdx.x; xx < w; xx += 256) rs += p[row + xx];
        s += rs;
    }
    const long long t = block_sum_i64(s, red_i);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * G + blockIdx.y] = t;
}

inline bool geometry_ok(int N, int C, int H, int W, int crop) {
    // (N rides in a grid's y / z dimension: <= 65535)
    return N > 0 && N <= 65535 && (C == 1 || C == 3) && crop >= 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && 2 * (long long)crop < H && 2 * (long long)crop < W;
}

inline int sse_blocks(int H, int crop) { const int h = H - 2 * crop; return h < SSE_MAX_BLOCKS ? h : SSE_MAX_BLOCKS; }

inline long long ssim_tiles(int H, int W, int crop, int* tiles_x) {
    const int hv = H - 2 * crop - (SSIM_K - 1), wv = W - 2 * crop - (SSIM_K - 1);
    if (hv < 1 || wv < 1) return 0;
    *tiles_x = (wv + SSIM_TW - 1) / SSIM_TW;
    return (long long)*tiles_x * ((hv + SSIM_TH - 1) / SSIM_TH);
}

inline long long box_tiles(int H, int W, int crop, int* tiles_x) {
    const int hv = H - 2 * crop - (BOX_K - 1), wv = W - 2 * crop - (BOX_K - 1);
    if (hv < 1 || wv < 1) return 0;
    *tiles_x = (wv + BOX_TW - 1) / BOX_TW;
    return (long long)*tiles_x * ((hv + BOX_TH - 1) / BOX_TH);
}

// bytes of workspace dasr_img_sse / dasr_img_ssim / dasr_img_ssim_box / dasr_img_channel_sums write their per-workgroup partials into (the largest of the four)
inline long long ws_bytes(int N, int C, int H, int W, int crop) {
    int tx = 0;
    const long long sse = (long long)N * sse_blocks(H, crop) * 16;
    const long long ssim = (long long)N * C * ssim_tiles(H, W, crop, &tx) * 8;
    const long long box = (long long)N * C * box_tiles(H, W, crop, &tx) * 8;
    const long long chan = (long long)N * C * sse_blocks(H, crop) * 8;
    const long long m1 = sse > ssim ? sse : ssim, m2 = box > chan ? box : chan;
    return m1 > m2 ? m1 : m2;
}

}  // namespace

extern "C" int dasr_img_ws_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop) {
    if (!geometry_ok(N, C, H, W, crop)) return DASR_EINVAL;
    const long long b = ws_bytes(N, C, H, W, crop);
    return b > 0x7fffffffLL ? DASR_EINVAL : (int)b;
}

extern "C" int dasr_tensor2img_u8(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, double lo, double hi, uint8_t* hwc_bgr, uint8_t* planar,
                                  int32_t* nan_count, void* stream) {
    if (!x || N <= 0 || C <= 0 || C > 4 || H <= 0 || W <= 0 || !(hi > lo) || (!hwc_bgr && !planar)) return DASR_EINVAL;
    const long long HW = (long long)H * W, total = (long long)N * HW;
    if ((total + 255) / 256 > 0x7fffffffLL) return DASR_EINVAL;
    if (nan_count) HIP_TRY(hipMemsetAsync(nan_count, 0, sizeof(int32_t), as_stream(stream)));
    // util.tensor2img: clamp_(lo, hi), `- lo`, `/ (hi - lo)` with the Python scalars rounded to fp32 (the difference is formed in double first)
    DASR_LAUNCH(tensor2img_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, C, HW, total, (float)lo, (float)hi,
                (float)(hi - lo), hwc_bgr, planar, nan_count);
    return (int)hipGetLastError();
}

extern "C" int dasr_img_sse(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int64_t* sse, double* sse_y,
                            void* ws, int64_t ws_size, void* stream) {
    if (!a || !b || !sse || !ws || !geometry_ok(N, C, H, W, crop) || (sse_y && C != 3)) return DASR_EINVAL;
    const int G = sse_blocks(H, crop);
    if (ws_size < (long long)N * G * 16) return DASR_EINVAL;
    long long* part_i = (long long*)ws;
    double* part_y = sse_y ? (double*)ws + (size_t)N * G : nullptr;
    DASR_LAUNCH(img_sse_kernel, dim3(G, N), dim3(256), 0, as_stream(stream), a, b, C, H, W, crop, part_i, part_y);
    DASR_LAUNCH(img_reduce_kernel, dim3(N), dim3(256), 0, as_stream(stream), (const long long*)part_i, (const double*)part_y, G, (long long*)sse, sse_y, 1.0);
    return (int)hipGetLastError();
}

extern "C" int dasr_img_ssim(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t y_channel, double* ssim,
                             void* ws, int64_t ws_size, void* stream) {
    if (!a || !b || !ssim || !ws || !geometry_ok(N, C, H, W, crop) || (y_channel != 0 && y_channel != 1) || (y_channel && C != 3)) return DASR_EINVAL;
    int tiles_x = 0;
    const long long tiles = ssim_tiles(H, W, crop, &tiles_x);
    if (tiles < 1) return DASR_EINVAL;   // a cropped side under 11 pixels: the valid region is empty
    const int ch = y_channel ? 1 : C;
    if (tiles * ch > 0x7fffffffLL || ws_size < (long long)N * ch * tiles * 8) return DASR_EINVAL;
    ssim_window win;   // util._gauss_window(11, 1.5): exp(-x^2 / (2 sigma^2)), normalised
    double sum = 0.0;
    for (int k = 0; k < SSIM_K; ++k) {
        const double ax = (double)k - (SSIM_K - 1) / 2.0;
        win.w[k] = exp(-(ax * ax) / (2.0 * 1.5 * 1.5));
        sum += win.w[k];
    }
    for (int k = 0; k < SSIM_K; ++k) win.w[k] /= sum;
    const double count = (double)ch * (double)(H - 2 * crop - (SSIM_K - 1)) * (double)(W - 2 * crop - (SSIM_K - 1));
    if (y_channel) {
        auto kfn = img_ssim_kernel<true>;
        DASR_LAUNCH_TAG("img_ssim_kernel<y>", kfn, dim3((unsigned)tiles, ch, N), dim3(256), 0, as_stream(stream), a, b, C, H, W, crop, tiles_x, win, (double*)ws);
    } else {
        auto kfn = img_ssim_kernel<false>;
        DASR_LAUNCH_TAG("img_ssim_kernel<u8>", kfn, dim3((unsigned)tiles, ch, N), dim3(256), 0, as_stream(stream), a, b, C, H, W, crop, tiles_x, win, (double*)ws);
    }
    DASR_LAUNCH(img_reduce_kernel, dim3(N), dim3(256), 0, as_stream(stream), (const long long*)nullptr, (const double*)ws, (int)(tiles * ch), (long long*)nullptr, ssim,
                count);
    return (int)hipGetLastError();
}

extern "C" int dasr_img_ssim_box(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, double* ssim, void* ws, int64_t ws_size,
                                 void* stream) {
    if (!a || !b || !ssim || !ws || !geometry_ok(N, C, H, W, crop)) return DASR_EINVAL;
    int tiles_x = 0;
    const long long tiles = box_tiles(H, W, crop, &tiles_x);
    if (tiles < 1) return DASR_EINVAL;   // a cropped side under 7 pixels: no window fits
    if (tiles * C > 0x7fffffffLL || ws_size < (long long)N * C * tiles * 8) return DASR_EINVAL;
    const double count = (double)C * (double)(H - 2 * crop - (BOX_K - 1)) * (double)(W - 2 * crop - (BOX_K - 1));
    DASR_LAUNCH(img_ssim_box_kernel, dim3((unsigned)tiles, C, N), dim3(256), 0, as_stream(stream), a, b, C, H, W, crop, tiles_x, (double*)ws);
    DASR_LAUNCH(img_reduce_kernel, dim3(N), dim3(256), 0, as_stream(stream), (const long long*)nullptr, (const double*)ws, (int)(tiles * C), (long long*)nullptr, ssim,
                count);
    return (int)hipGetLastError();
}

extern "C" int dasr_img_channel_sums(const uint8_t* a, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int64_t* sums, void* ws, int64_t ws_size, void* stream) {
    if (!a || !sums || !ws || !geometry_ok(N, C, H, W, crop)) return DASR_EINVAL;
    const int G = sse_blocks(H, crop);
    if (ws_size < (long long)N * C * G * 8) return DASR_EINVAL;
    DASR_LAUNCH(img_channel_sums_kernel, dim3(N * C, G), dim3(256), 0, as_stream(stream), a, H, W, crop, (long long*)ws);
    DASR_LAUNCH(img_reduce_kernel, dim3(N * C), dim3(256), 0, as_stream(stream), (const long long*)ws, (const double*)nullptr, G, (long long*)sums, (double*)nullptr, 1.0);
    return (int)hipGetLastError();
}

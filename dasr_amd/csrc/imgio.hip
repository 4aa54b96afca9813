// Input stage of the evaluation datasets on the device, gfx950 (reference: codes/SRN/data/util.py:78-96 read_img, :133-145 modcrop, :243-433 imresize_np as
// codes/SRN/data/LRHR_dataset.py:44-126 and LR_dataset.py use them in the val / test phase; host restatement: dasr_amd/data.py load_image, imresize_matlab):
//  * u8_to_planar: the decoded image as PIL hands it over (uint8, HWC, RGB) -> the top-left Hc x Wc window (modcrop) as planar fp32 in [0, 1]
//  * imresize_down: MATLAB-style antialiased bicubic down-sampling by an integer s, as two gather passes over per-axis tap tables (index and fp64 weight,
//    4 s + 2 taps per output sample) the host builds once per (length, s): rows first into an fp64 intermediate, then columns, ONE rounding to fp32 at the end
//  * gather_crops_u8 / crops_bicubic_down: batch assembly of the DSN trainer on resident 8-bit images (reference: codes/DSN/data_loader.py:12-59, utils.py:37-160; host
//    restatement: dasr_amd/dsn_data.py TrainDeresnetDataset).  The first cuts one transformed window per descriptor out of a decoded image and converts it, the second makes the
//    clamped bicubic x1/4 image of every crop of the batch in ONE launch, both passes through LDS (no fp64 intermediate in device memory).  A batch is a few MB: both are
//    bound by launch latency, so what counts is one launch per batch tensor and no host synchronisation, not bandwidth.
//  * gather_srn_u8 / crops_down4_u8: batch assembly of the SRN trainers on resident 8-bit images (`"resident_u8": true`; reference: codes/SRN/data/LRHR_dataset.py:44-126,
//    LRHR_wavelet_unpairEq_fake_w_dataset.py:50-166, data/util.py:116-128 augment; host side: dasr_amd/data.py).  The first writes every 3-channel tensor of a batch in one launch
//    (per-descriptor window size and destination), the second the augmented LR crops of an HR-only set: samples of the x1/4 image of the WHOLE image, made where a crop needs them.
//  * dihedral8 / dihedral8_mean: the geometry of the x8 self-ensemble (`"self_ensemble": true`; reference: codes/SRN/models/SR_model.py:102-140 test_x8): the eight flips /
//    transposes of the LR image in one launch, and the mean of the eight inverse-transformed SR images in one launch with a fixed order of the adds.
//  * bp_residual / bp_update: the two launches of one iteration of the back-projection of an SR image onto its LR input (`"back_projection"`), near the end of the file.
//  * windows_down_u8 / imresize_up: the bicubic LR and Bic images of windows of a resident 8-bit image (`python -m dasr_amd.prepare_data`) and the up-sampling of the
//    reverse filter, at the end of the file.
// The first two are memory-bound (about 36 multiply-adds per output sample at s = 4 against 2 x 18 gathered reads), so the kernels are plain: one thread per output
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

// one thread: one output pixel, three channels; ox on the lanes.  Output pixel (i, j) of the transformed crop (n = crop) comes from (k quarter-turns counter-clockwise undone
// first, then the horizontal, then the vertical flip): k = 1: (j, n-1-i), k = 2: (n-1-i, n-1-j), k = 3: (n-1-j, i).  For k odd a wave walks down a column of the source.
// Every source coordinate is clamped into the image: a damaged descriptor reads a wrong pixel, never outside the allocation.  grid (ceil(size^2 / 256), n)
__global__ __launch_bounds__(256) void gather_crops_u8_kernel(const dasr_crop_u8_desc* __restrict__ descs, int size, float* __restrict__ dst) {
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi >= size * size) return;
    const dasr_crop_u8_desc d = descs[blockIdx.y];
    const int oy = gi / size, ox = gi - oy * size;
    const int n1 = d.crop - 1, i = d.sub_y + oy, j = d.sub_x + ox, k = (d.flags >> 2) & 3;
    int r = k == 0 ? i : k == 1 ? j : k == 2 ? n1 - i : n1 - j;
    int c = k == 0 ? j : k == 1 ? n1 - i : k == 2 ? n1 - j : i;
    if (d.flags & 2) c = n1 - c;
    if (d.flags & 1) r = n1 - r;
    const int y = min(max(d.y0 + r, 0), max(d.H - 1, 0)), x = min(max(d.x0 + c, 0), max(d.W - 1, 0));
    const uint8_t* p = d.src + ((size_t)y * (size_t)max(d.W, 1) + x) * 3;
    float* o = dst + (size_t)blockIdx.y * 3 * size * size + gi;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[(size_t)ch * size * size] = d.src ? (float)p[ch] / 255.0f : 0.f;   // (a descriptor left zeroed: a black sample, no access)
}

// Both passes of the x1/4 resize of one plane's tile of BD_ROWS output rows in one workgroup.  Output row oy takes the 18 input rows 4 oy - 7 .. 4 oy + 10 (mirrored at the ends), so
// the tile needs the BD_IN = 4 BD_ROWS + 14 consecutive input rows from `base` on -- whole rows of a c-wide plane, ONE contiguous run of memory, staged with 16-byte loads.
//   LDS: in [BD_IN][c] fp32, then mid [BD_ROWS][4][c / 4 + 8] fp64 = c x 152 + 1024 bytes: 39 KB at c = 256 (four workgroups per CU), 153 KB at the largest c = 1024.
//   BD_ROWS = 4: a batch of 8 crops of 256 x 256 is 24 planes x 16 tiles = 384 workgroups for 256 CUs, and the staged rows overlap 30 / 16; 8 rows would halve the workgroups
//   (192 < 256 CUs) and no longer fit c = 1024.  The tile only groups outputs: every output sample is the same sequence of operations for any tile.
//   mid is stored de-interleaved by x mod 4 (row r, column x at [r][x & 3][x >> 2]): the column pass reads x = 4 ox - 7 + t, consecutive doubles over the lanes for a fixed tap.
// Arithmetic as in the two-pass kernels above: fp64 products and sums in tap order, the row-pass result kept in fp64, clamped in fp64 (a NaN stays a NaN), one rounding to fp32.
constexpr int BD_ROWS = 4, BD_TAPS = 18, BD_IN = 4 * BD_ROWS + 14;
__global__ __launch_bounds__(256) void crops_bicubic_down_kernel(const float* __restrict__ hr, int c, int tiles, const int32_t* __restrict__ idx, const double* __restrict__ wt,
                                                                 float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int co = c >> 2, qs = co + 8;
    const int nin = min(BD_IN, c);
    float* in = (float*)smem;
    double* mid = (double*)(smem + (size_t)BD_IN * c * sizeof(float));
    const int plane = blockIdx.x / tiles, oy0 = (blockIdx.x - plane * tiles) * BD_ROWS;
    const int base = min(max(4 * oy0 - 7, 0), c - nin);
    const float4* src = (const float4*)(hr + ((size_t)plane * c + base) * c);
    for (int e = threadIdx.x; e < nin * co; e += 256) ((float4*)in)[e] = src[e];
    __syncthreads();
    const int rows = min(BD_ROWS, co - oy0);
    for (int e = threadIdx.x; e < rows * c; e += 256) {
        const int r = e / c, x = e - r * c;
        const int32_t* ji = idx + (size_t)(oy0 + r) * BD_TAPS;
        const double* jw = wt + (size_t)(oy0 + r) * BD_TAPS;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < BD_TAPS; ++t) {
            const int j = min(max(ji[t] - base, 0), nin - 1);   // (a damaged table reads a wrong staged row, never outside the tile)
            acc += jw[t] * (double)in[j * c + x];
        }
        mid[(r * 4 + (x & 3)) * qs + (x >> 2)] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * co; e += 256) {
        const int r = e / co, ox = e - r * co;
        const int32_t* ji = idx + (size_t)ox * BD_TAPS;
        const double* jw = wt + (size_t)ox * BD_TAPS;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < BD_TAPS; ++t) {
            const int j = min(max(ji[t], 0), c - 1);
            acc += jw[t] * mid[(r * 4 + (j & 3)) * qs + (j >> 2)];
        }
        acc = acc < 0.0 ? 0.0 : acc > 1.0 ? 1.0 : acc;
        dst[((size_t)plane * co + oy0 + r) * co + ox] = (float)acc;
    }
}

// One launch for every 3-channel tensor of an SRN batch: descriptor blockIdx.y, one thread per output pixel (three channels), ox on the lanes.  The descriptors of one launch
// have different sizes (LR and HR windows): the grid covers max_size^2 pixels and a smaller window masks the rest.  Output pixel (y, x) comes from window pixel (ci, cj):
// the transpose was applied last, so it is undone first, then the vertical, then the horizontal flip (gather_crops_kernel of misc.hip).  For a transposed window a wave
// walks down a column of the source.  Every source coordinate is clamped into the image.  grid (ceil(max_size^2 / 256), n)
__global__ __launch_bounds__(256) void gather_srn_u8_kernel(const dasr_srn_u8_desc* __restrict__ descs, int max_size) {
    const dasr_srn_u8_desc d = descs[blockIdx.y];
    const int size = min(d.size, max_size);
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (!d.src || !d.dst || size <= 0 || gi >= size * size) return;   // (a descriptor left zeroed: nothing is read or written)
    const int y = gi / size, x = gi - y * size;
    int ci = y, cj = x;
    if (d.flags & 4) { ci = x; cj = y; }
    if (d.flags & 2) ci = size - 1 - ci;
    if (d.flags & 1) cj = size - 1 - cj;
    const int sy = min(max(d.y0 + ci, 0), max(d.H - 1, 0)), sx = min(max(d.x0 + cj, 0), max(d.W - 1, 0));
    const uint8_t* p = d.src + ((size_t)sy * (size_t)max(d.W, 1) + sx) * 3;
    float* o = d.dst + gi;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[(size_t)ch * size * size] = (float)p[ch] / 255.0f;
}

// The x1/4 image of the WHOLE 8-bit image, evaluated only where a crop needs it.  One workgroup: a D4_T x D4_T tile (before the flips) of the LR window of one descriptor,
// the three channels one after the other.
//   win: the D4_IN x D4_IN x 3 byte window of the image the tile's taps reach (rows 4 (y0 + oy0) - 7 on, columns likewise), loaded ONCE with the mirroring at the image's
//        borders folded into the load -- the passes index it without a test.  The mirror is bicubic_taps': j < 0 -> -j - 1, then j >= n -> 2 n - 1 - j, then a clamp.
//   lut: (double)((float)b / 255.0f) of the 256 byte values: the one correctly rounded fp32 division of dasr_u8_to_planar, made once per workgroup instead of once per tap.
//   mid: the row pass of one channel, [D4_T][D4_IN] fp64, column x of row r at [r][x & 3][x >> 2] so that the column pass reads consecutive doubles over the lanes.
//   LDS: 78 x 78 x 3 + 2 KB + 16 x 4 x 20 x 8 = 18256 + 2048 + 10240 = 30544 bytes: five workgroups on a CU (a 32 x 32 tile would need 60 KB for the bytes alone).
// Arithmetic: that of imresize_rows_kernel / imresize_cols_kernel on the planar fp32 image: fp64 products and sums in tap order from 0.0, the row result kept in fp64, NO
// clamp, one rounding to fp32.  The 18 weights are kernel arguments (the same for every output sample at scale 1 / 4).  grid (tiles^2, n), tiles = ceil(size / D4_T)
constexpr int D4_T = 16, D4_TAPS = 18, D4_IN = 4 * D4_T + 14, D4_Q = D4_IN / 4 + 1;
struct d4_weights { double w[D4_TAPS]; };

__device__ __forceinline__ int d4_mirror(int j, int n) {
    if (j < 0) j = -j - 1;
    if (j >= n) j = 2 * n - 1 - j;
    return min(max(j, 0), n - 1);
}

__global__ __launch_bounds__(256) void crops_down4_u8_kernel(const dasr_srn_u8_desc* __restrict__ descs, int size, int tiles, d4_weights wt) {
    __shared__ __attribute__((aligned(16))) uint8_t win[(D4_IN * D4_IN * 3 + 15) / 16 * 16];
    __shared__ double lut[256];
    __shared__ double mid[D4_T * 4 * D4_Q];
    const dasr_srn_u8_desc d = descs[blockIdx.y];
    if (!d.src || !d.dst || d.H < 1 || d.W < 1) return;   // (uniform over the workgroup: in front of every barrier)
    const int ty = blockIdx.x / tiles, oy0 = ty * D4_T, ox0 = (blockIdx.x - ty * tiles) * D4_T;
    const int rows = min(D4_T, size - oy0), cols = min(D4_T, size - ox0);
    const int nin_y = 4 * rows + 14, nin_x = 4 * cols + 14;
    const int base_y = 4 * (d.y0 + oy0) - 7, base_x = 4 * (d.x0 + ox0) - 7;
    lut[threadIdx.x] = (double)((float)threadIdx.x / 255.0f);
    for (int e = threadIdx.x; e < nin_y * nin_x; e += 256) {
        const int r = e / nin_x, x = e - r * nin_x;
        const uint8_t* p = d.src + ((size_t)d4_mirror(base_y + r, d.H) * (size_t)d.W + d4_mirror(base_x + x, d.W)) * 3;
        uint8_t* q = win + (r * D4_IN + x) * 3;
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
    __syncthreads();
    for (int ch = 0; ch < 3; ++ch) {
        for (int e = threadIdx.x; e < rows * nin_x; e += 256) {
            const int r = e / nin_x, x = e - r * nin_x;
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < D4_TAPS; ++t) acc += wt.w[t] * lut[win[((4 * r + t) * D4_IN + x) * 3 + ch]];
            mid[(r * 4 + (x & 3)) * D4_Q + (x >> 2)] = acc;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < rows * cols; e += 256) {
            const int r = e / cols, ox = e - r * cols;
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < D4_TAPS; ++t) {
                const int x = 4 * ox + t;
                acc += wt.w[t] * mid[(r * 4 + (x & 3)) * D4_Q + (x >> 2)];
            }
            const int ci = oy0 + r, cj = ox0 + ox;                 // position in the window before the flips -> position in the augmented crop
            const int a = (d.flags & 2) ? size - 1 - ci : ci, b = (d.flags & 1) ? size - 1 - cj : cj;
            const int y = (d.flags & 4) ? b : a, x = (d.flags & 4) ? a : b;
            d.dst[((size_t)ch * size + y) * size + x] = (float)acc;
        }
        __syncthreads();
    }
}

// ---- x8 geometric self-ensemble (reference: codes/SRN/models/SR_model.py:102-140 test_x8; host restatement: dasr_amd/util.py dihedral8_reference) ----------------------
// Member i of the ensemble: b0 = i & 1 flips along W, b1 = (i >> 1) & 1 flips along H, b2 = i >> 2 transposes (applied last).  Both kernels work on D8_T x D8_T tiles of
// the untransposed image, one workgroup per tile and channel, grid (ceil(W / D8_T), ceil(H / D8_T), C).  The four untransposed members never touch the LDS: a thread
// moves the samples it holds (a flip along W reverses them inside the 16-byte vector and mirrors the vector's position).  The four transposed members go through an LDS
// tile with a row stride of D8_T + 1 words, written along one axis and read along the other, so that BOTH global sides are contiguous over the lanes (256-byte runs).
// VW / VH: 16-byte global accesses along W (x, dst_a / sr_a, dst) and along H (dst_b / sr_b): the launcher sets them when the length is a multiple of 4 and the pointers are
// 16-byte aligned -- every row then starts aligned, a mirrored vector (W - 4 - q) is aligned too, and a vector is never cut by the image's edge.  Otherwise one sample per lane.
// Memory-bound (1 read + 8 writes of the image / 8 reads + 1 write), no arithmetic but the seven adds and the exact scaling by 1 / 8.
constexpr int D8_T = 64, D8_S = D8_T + 1;

__device__ __forceinline__ float4 d8_rev(float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

template <bool VW, bool VH>
__global__ __launch_bounds__(256) void dihedral8_kernel(const float* __restrict__ x, int H, int W, float* __restrict__ dst_a, float* __restrict__ dst_b) {
    __shared__ float tile[D8_T * D8_S];   // tile[r][q] of the source
    const int q0 = blockIdx.x * D8_T, r0 = blockIdx.y * D8_T;
    const size_t HW = (size_t)H * W, CHW = HW * gridDim.z;
    const float* xp = x + blockIdx.z * HW;
    float* a = dst_a + blockIdx.z * HW;
    float* b = dst_b + blockIdx.z * HW;
    if (VW) {
        for (int e = threadIdx.x; e < D8_T * D8_T / 4; e += 256) {
            const int rl = e >> 4, ql = (e & 15) * 4, r = r0 + rl, q = q0 + ql;
            if (r >= H || q >= W) continue;
            const size_t up = (size_t)r * W, dn = (size_t)(H - 1 - r) * W;
            const int qf = W - 4 - q;
            const float4 v = *(const float4*)(xp + up + q);
            float* t = tile + rl * D8_S + ql;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
            *(float4*)(a + up + q) = v;
            *(float4*)(a + CHW + up + qf) = d8_rev(v);
            *(float4*)(a + 2 * CHW + dn + q) = v;
            *(float4*)(a + 3 * CHW + dn + qf) = d8_rev(v);
        }
    } else {
        for (int e = threadIdx.x; e < D8_T * D8_T; e += 256) {
            const int rl = e >> 6, ql = e & 63, r = r0 + rl, q = q0 + ql;
            if (r >= H || q >= W) continue;
            const size_t up = (size_t)r * W, dn = (size_t)(H - 1 - r) * W;
            const int qf = W - 1 - q;
            const float v = xp[up + q];
            tile[rl * D8_S + ql] = v;
            a[up + q] = v;
            a[CHW + up + qf] = v;
            a[2 * CHW + dn + q] = v;
            a[3 * CHW + dn + qf] = v;
        }
    }
    __syncthreads();
    // transposed members: planes [W][H]; source (r, q) -> row q or W - 1 - q, column r or H - 1 - r.  The lanes run along r.
    if (VH) {
        for (int e = threadIdx.x; e < D8_T * D8_T / 4; e += 256) {
            const int rl = (e & 15) * 4, ql = e >> 4, r = r0 + rl, q = q0 + ql;
            if (r >= H || q >= W) continue;
            const size_t up = (size_t)q * H, dn = (size_t)(W - 1 - q) * H;
            const int rf = H - 4 - r;
            const float* t = tile + rl * D8_S + ql;
            const float4 v = make_float4(t[0], t[D8_S], t[2 * D8_S], t[3 * D8_S]);
            *(float4*)(b + up + r) = v;
            *(float4*)(b + CHW + dn + r) = v;
            *(float4*)(b + 2 * CHW + up + rf) = d8_rev(v);
            *(float4*)(b + 3 * CHW + dn + rf) = d8_rev(v);
        }
    } else {
        for (int e = threadIdx.x; e < D8_T * D8_T; e += 256) {
            const int rl = e & 63, ql = e >> 6, r = r0 + rl, q = q0 + ql;
            if (r >= H || q >= W) continue;
            const size_t up = (size_t)q * H, dn = (size_t)(W - 1 - q) * H;
            const int rf = H - 1 - r;
            const float v = tile[rl * D8_S + ql];
            b[up + r] = v;
            b[CHW + dn + r] = v;
            b[2 * CHW + up + rf] = v;
            b[3 * CHW + dn + rf] = v;
        }
    }
}

// dst[c][R][Q] = 0.125f * (((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7), s_i the sample of member i's SR image that lands on (R, Q) once its transform is undone.
// The transposed members (sr_b, planes [W][H]) are staged first: lds[m][Q - Q0][R - R0], read from memory with the lanes along R and from the LDS with the lanes along Q.
// LDS: 4 x D8_T x D8_S words = 66560 bytes (dynamic: above the 64 KB of a static array), two workgroups on a CU.
template <bool VW, bool VH>
__global__ __launch_bounds__(256) void dihedral8_mean_kernel(const float* __restrict__ sr_a, const float* __restrict__ sr_b, int H, int W, float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lds = (float*)smem;
    constexpr int M = D8_T * D8_S;
    const int Q0 = blockIdx.x * D8_T, R0 = blockIdx.y * D8_T;
    const size_t HW = (size_t)H * W, CHW = HW * gridDim.z;
    const float* ap = sr_a + blockIdx.z * HW;
    const float* bp = sr_b + blockIdx.z * HW;
    if (VH) {
        for (int e = threadIdx.x; e < D8_T * D8_T / 4; e += 256) {
            const int rl = (e & 15) * 4, ql = e >> 4, R = R0 + rl, Q = Q0 + ql;
            if (R >= H || Q >= W) continue;
            const size_t up = (size_t)Q * H, dn = (size_t)(W - 1 - Q) * H;
            const int rf = H - 4 - R;
            const float4 v4 = *(const float4*)(bp + up + R), v5 = *(const float4*)(bp + CHW + dn + R);
            const float4 v6 = d8_rev(*(const float4*)(bp + 2 * CHW + up + rf)), v7 = d8_rev(*(const float4*)(bp + 3 * CHW + dn + rf));
            float* t = lds + ql * D8_S + rl;
            t[0] = v4.x; t[1] = v4.y; t[2] = v4.z; t[3] = v4.w;
            t[M] = v5.x; t[M + 1] = v5.y; t[M + 2] = v5.z; t[M + 3] = v5.w;
            t[2 * M] = v6.x; t[2 * M + 1] = v6.y; t[2 * M + 2] = v6.z; t[2 * M + 3] = v6.w;
            t[3 * M] = v7.x; t[3 * M + 1] = v7.y; t[3 * M + 2] = v7.z; t[3 * M + 3] = v7.w;
        }
    } else {
        for (int e = threadIdx.x; e < D8_T * D8_T; e += 256) {
            const int rl = e & 63, ql = e >> 6, R = R0 + rl, Q = Q0 + ql;
            if (R >= H || Q >= W) continue;
            const size_t up = (size_t)Q * H, dn = (size_t)(W - 1 - Q) * H;
            const int rf = H - 1 - R;
            float* t = lds + ql * D8_S + rl;
            t[0] = bp[up + R];
            t[M] = bp[CHW + dn + R];
            t[2 * M] = bp[2 * CHW + up + rf];
            t[3 * M] = bp[3 * CHW + dn + rf];
        }
    }
    __syncthreads();
    float* o = dst + blockIdx.z * HW;
    if (VW) {
        for (int e = threadIdx.x; e < D8_T * D8_T / 4; e += 256) {
            const int rl = e >> 4, ql = (e & 15) * 4, R = R0 + rl, Q = Q0 + ql;
            if (R >= H || Q >= W) continue;
            const size_t up = (size_t)R * W, dn = (size_t)(H - 1 - R) * W;
            const int qf = W - 4 - Q;
            const float4 s0 = *(const float4*)(ap + up + Q), s1 = d8_rev(*(const float4*)(ap + CHW + up + qf));
            const float4 s2 = *(const float4*)(ap + 2 * CHW + dn + Q), s3 = d8_rev(*(const float4*)(ap + 3 * CHW + dn + qf));
            float acc[4] = {((s0.x + s1.x) + s2.x) + s3.x, ((s0.y + s1.y) + s2.y) + s3.y, ((s0.z + s1.z) + s2.z) + s3.z, ((s0.w + s1.w) + s2.w) + s3.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* t = lds + (ql + k) * D8_S + rl;
                acc[k] = 0.125f * ((((acc[k] + t[0]) + t[M]) + t[2 * M]) + t[3 * M]);
            }
            *(float4*)(o + up + Q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
    } else {
        for (int e = threadIdx.x; e < D8_T * D8_T; e += 256) {
            const int rl = e >> 6, ql = e & 63, R = R0 + rl, Q = Q0 + ql;
            if (R >= H || Q >= W) continue;
            const size_t up = (size_t)R * W, dn = (size_t)(H - 1 - R) * W;
            const int qf = W - 1 - Q;
            const float* t = lds + ql * D8_S + rl;
            const float acc = ((ap[up + Q] + ap[CHW + up + qf]) + ap[2 * CHW + dn + Q]) + ap[3 * CHW + dn + qf];
            o[up + Q] = 0.125f * ((((acc + t[0]) + t[M]) + t[2 * M]) + t[3 * M]);
        }
    }
}

inline bool d8_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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

extern "C" int dasr_gather_crops_u8(const dasr_crop_u8_desc* descs_dev, int32_t n, int32_t size, float* dst, void* stream) {
    if (!descs_dev || !dst || n <= 0 || n > 65535 || size <= 0 || size > 4096) return DASR_EINVAL;
    DASR_LAUNCH(gather_crops_u8_kernel, dim3((unsigned)((size * size + 255) / 256), (unsigned)n), dim3(256), 0, as_stream(stream), descs_dev, size, dst);
    return (int)hipGetLastError();
}

extern "C" int dasr_crops_bicubic_down(const float* hr, int32_t n, int32_t c, int32_t s, const int32_t* idx, const double* wt, float* dst, void* stream) {
    if (!hr || !idx || !wt || !dst || n <= 0 || n > 65535 || s != 4 || c < 4 || c > 1024 || c % 4 || ((uintptr_t)hr & 15)) return DASR_EINVAL;
    const int tiles = (c / 4 + BD_ROWS - 1) / BD_ROWS;
    const size_t lds = (size_t)BD_IN * c * sizeof(float) + (size_t)BD_ROWS * 4 * (c / 4 + 8) * sizeof(double);
    // per call: the attribute belongs to the current device, and the call is cheap next to a launch.  The largest c: 1024 x 152 + 1024 bytes of the 160 KB of a CU
    HIP_TRY(hipFuncSetAttribute((const void*)crops_bicubic_down_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BD_IN * 1024 * 4 + BD_ROWS * 4 * (256 + 8) * 8));
    DASR_LAUNCH(crops_bicubic_down_kernel, dim3((unsigned)(3 * n * tiles)), dim3(256), lds, as_stream(stream), hr, (int)c, tiles, idx, wt, dst);
    return (int)hipGetLastError();
}

extern "C" int dasr_gather_srn_u8(const dasr_srn_u8_desc* descs_dev, int32_t n, int32_t max_size, void* stream) {
    if (!descs_dev || n <= 0 || n > 65535 || max_size <= 0 || max_size > 4096) return DASR_EINVAL;
    DASR_LAUNCH(gather_srn_u8_kernel, dim3((unsigned)((max_size * max_size + 255) / 256), (unsigned)n), dim3(256), 0, as_stream(stream), descs_dev, (int)max_size);
    return (int)hipGetLastError();
}

extern "C" int dasr_crops_down4_u8(const dasr_srn_u8_desc* descs_dev, const dasr_srn_u8_desc* descs_host, int32_t n, int32_t size, const double* w18, void* stream) {
    if (!descs_dev || !descs_host || !w18 || n <= 0 || n > 65535 || size <= 0 || size > 128) return DASR_EINVAL;
    for (int k = 0; k < n; ++k) {
        const dasr_srn_u8_desc& d = descs_host[k];
        if (!d.src || !d.dst || d.H <= 0 || d.W <= 0 || d.H % 4 || d.W % 4 || d.size != size) return DASR_EINVAL;
        if (d.y0 < 0 || d.x0 < 0 || d.y0 > d.H / 4 - size || d.x0 > d.W / 4 - size) return DASR_EINVAL;
    }
    d4_weights wt;
    for (int t = 0; t < D4_TAPS; ++t) wt.w[t] = w18[t];
    const int tiles = (size + D4_T - 1) / D4_T;
    DASR_LAUNCH(crops_down4_u8_kernel, dim3((unsigned)(tiles * tiles), (unsigned)n), dim3(256), 0, as_stream(stream), descs_dev, (int)size, tiles, wt);
    return (int)hipGetLastError();
}

extern "C" int dasr_dihedral8(const float* x, int32_t C, int32_t H, int32_t W, float* dst_a, float* dst_b, void* stream) {
    if (!x || !dst_a || !dst_b || C <= 0 || C > 65535 || H <= 0 || W <= 0 || dst_a == x || dst_b == x || dst_a == dst_b) return DASR_EINVAL;
    const dim3 grid((unsigned)((W + D8_T - 1) / D8_T), (unsigned)((H + D8_T - 1) / D8_T), (unsigned)C);
    if (grid.y > 65535) return DASR_EINVAL;
    const bool vw = W % 4 == 0 && d8_al16(x) && d8_al16(dst_a), vh = H % 4 == 0 && d8_al16(dst_b);
    auto k = vw ? (vh ? dihedral8_kernel<true, true> : dihedral8_kernel<true, false>) : (vh ? dihedral8_kernel<false, true> : dihedral8_kernel<false, false>);
    DASR_LAUNCH_TAG("dihedral8_kernel", k, grid, dim3(256), 0, as_stream(stream), x, (int)H, (int)W, dst_a, dst_b);
    return (int)hipGetLastError();
}

extern "C" int dasr_dihedral8_mean(const float* sr_a, const float* sr_b, int32_t C, int32_t H, int32_t W, float* dst, void* stream) {
    if (!sr_a || !sr_b || !dst || C <= 0 || C > 65535 || H <= 0 || W <= 0 || dst == sr_a || dst == sr_b) return DASR_EINVAL;
    const dim3 grid((unsigned)((W + D8_T - 1) / D8_T), (unsigned)((H + D8_T - 1) / D8_T), (unsigned)C);
    if (grid.y > 65535) return DASR_EINVAL;
    const bool vw = W % 4 == 0 && d8_al16(sr_a) && d8_al16(dst), vh = H % 4 == 0 && d8_al16(sr_b);
    auto k = vw ? (vh ? dihedral8_mean_kernel<true, true> : dihedral8_mean_kernel<true, false>)
                : (vh ? dihedral8_mean_kernel<false, true> : dihedral8_mean_kernel<false, false>);
    const int lds = 4 * D8_T * D8_S * (int)sizeof(float);
    HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds));   // (per call: the attribute belongs to the current device)
    DASR_LAUNCH_TAG("dihedral8_mean_kernel", k, grid, dim3(256), (size_t)lds, as_stream(stream), sr_a, sr_b, (int)H, (int)W, dst);
    return (int)hipGetLastError();
}

// ---- iterative back-projection (`"back_projection"`; reference: codes/SRN/scripts/back_projection/backprojection.m:1-20, main_bp.m; host side: dasr_amd/backproject.py) ------
// One iteration is   d = LR - imresize(SR, 1 / s);   SR += conv2(imresize(d, s), p, 'same')   with p the squared,
// renormalised 5 x 5 Gaussian of sigma 1 -- the outer product of u_i = exp(-i^2) / sum_j exp(-j^2), i = -2 .. 2.  Two launches:
//  * bp_residual_kernel: d = lr - (float)down(sr), `down` bit for bit dasr_imresize_down above: the same tap tables, rows first, fp64 products rounded before
//    they are added in tap order, one rounding to fp32 -- but both passes through LDS (the scheme of crops_bicubic_down_kernel): a workgroup stages the HR window its
//    BP_RT x BP_CT tile of LR outputs reaches once and no fp64 intermediate goes to device memory.
//  * bp_update_kernel: sr += G(U), U = imresize(d, s) (bicubic, NOT antialiased: 6-entry tap tables of imgio.bicubic_taps(n, s), rows first), G the separable 5-tap pass
//    in both directions.  Per BP_UY x BP_UX tile of SR samples, all in LDS: the d window, the row pass V, U with a halo of 2, the horizontal 5-tap pass T, then the vertical
//    5-tap pass added to the thread's own sr sample and rounded to fp32 ONCE.  In place: a thread reads sr only where it writes.
//    Two halo rules meet here and are kept apart: the up-sampling mirrors at the IMAGE border (the tables carry the mirrored indices, which point back into the staged
//    window); the 5 x 5 pass sees zeros beyond the IMAGE border (conv2 'same') but the real neighbours beyond a TILE border (U is evaluated on the halo).
// Both are memory / LDS work with a few dozen fp64 operations per sample; the tiles only group outputs: every output sample is the same sequence of operations for any tile.
// Table indices are clamped into the staged window: a damaged table reads a wrong staged sample, never outside the window or the image.
//
// (fp contraction is off for the whole file: every product is rounded to fp64 before it is added, in a fixed order.)
namespace {

constexpr int BP_RT = DASR_BP_RES_TILE_H, BP_CT = DASR_BP_RES_TILE_W;   // LR outputs per workgroup of the residual kernel
constexpr int BP_UY = DASR_BP_UPD_TILE_H, BP_UX = DASR_BP_UPD_TILE_W;   // SR samples per workgroup of the update kernel

// Output sample o of imresize(., 1 / S) takes the 4 S + 2 source samples from S o - OFF on (before mirroring), OFF = S + 1 + S / 2 (4, 5, 7 for S = 2, 3, 4:
// bicubic_taps' floor(u - 2 S) at u = (o + 1) S + (1 - S) / 2).  The window is taken ONE sample wider on both sides, so it does not hinge on how that floor rounded.
//   LDS at S = 4: in [48][144] fp32 + mid [8][4][37] fp64 + the tile's taps ([18][32] column, [8][18] row; int32 + fp64) = 27648 + 9472 + 6912 + 1728 = 45760 bytes, three workgroups on a CU.
//   mid is stored de-interleaved by x mod S (row r, window column x at [r][x % S][x / S]): the column pass reads columns S ox + const, consecutive doubles over the lanes.
//   Latency: a workgroup is a chain of dependent steps (stage, row pass, column pass), and with three or four workgroups on a CU nothing hides a trip to memory inside one.
//   So EVERYTHING the workgroup reads from memory is requested before the first barrier, each thread's loads all in flight together: the window (a compile-time number of
//   masked loads per thread into registers, then the LDS stores), the tile's rows of both tap tables (the column taps transposed to [tap][column]: read from memory in the
//   column pass they are a stride of 4 S + 2 entries between the lanes) and the thread's own lr sample.  After the barrier the kernel touches only LDS, until its one store.
template <int S>
__global__ __launch_bounds__(256) void bp_residual_kernel(const float* __restrict__ sr, const float* __restrict__ lr, int H, int W, const int32_t* __restrict__ idx_h,
                                                          const double* __restrict__ w_h, const int32_t* __restrict__ idx_w, const double* __restrict__ w_w,
                                                          float* __restrict__ d) {
    constexpr int TAPS = 4 * S + 2, OFF = S + 1 + S / 2;
    constexpr int WIN_H = S * BP_RT + 3 * S + 4, WIN_W = S * BP_CT + 3 * S + 4, QS = (WIN_W + S - 1) / S + 1;
    constexpr int NLD = (WIN_H * WIN_W + 255) / 256, NROW = (BP_RT * WIN_W + 255) / 256;
    static_assert(BP_RT * BP_CT == 256 && BP_RT * TAPS <= 256, "one output per thread in the column pass; the row taps are staged in one step");
    __shared__ float in[WIN_H * WIN_W];
    __shared__ double mid[BP_RT * S * QS];
    __shared__ double tw[TAPS * BP_CT], rw[BP_RT * TAPS];
    __shared__ int32_t tj[TAPS * BP_CT], rj[BP_RT * TAPS];
    const int tid = threadIdx.x;
    const int h = H / S, w = W / S;
    const int ox0 = blockIdx.x * BP_CT, oy0 = blockIdx.y * BP_RT;
    const int rows = min(BP_RT, h - oy0), cols = min(BP_CT, w - ox0);
    const int by = max(S * oy0 - OFF - 1, 0), bx = max(S * ox0 - OFF - 1, 0);
    const int nh = min(min(S * (oy0 + rows - 1) - OFF + TAPS, H - 1) - by + 1, WIN_H), nw = min(min(S * (ox0 + cols - 1) - OFF + TAPS, W - 1) - bx + 1, WIN_W);
#pragma unroll
    for (int e = tid; e < BP_CT * TAPS; e += 256) {   // (rows ox0 .. ox0 + cols - 1 of the column table: one contiguous run; kept as window columns)
        const int ox = e / TAPS, t = e - ox * TAPS;
        if (ox < cols) {
            tj[t * BP_CT + ox] = min(max(idx_w[(size_t)ox0 * TAPS + e] - bx, 0), nw - 1);
            tw[t * BP_CT + ox] = w_w[(size_t)ox0 * TAPS + e];
        }
    }
    if (tid < rows * TAPS) {                           // (rows oy0 .. oy0 + rows - 1 of the row table, kept as offsets of window rows)
        rj[tid] = min(max(idx_h[(size_t)oy0 * TAPS + tid] - by, 0), nh - 1) * WIN_W;
        rw[tid] = w_h[(size_t)oy0 * TAPS + tid];
    }
    const int orow = tid / BP_CT, ox = tid % BP_CT;
    const bool live = orow < rows && ox < cols;
    const size_t o = ((size_t)blockIdx.z * h + oy0 + min(orow, rows - 1)) * w + ox0 + min(ox, cols - 1);
    const float lrv = lr[o];
    const float* plane = sr + (size_t)blockIdx.z * H * W + (size_t)by * W + bx;
    float v[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int e = tid + 256 * k, r = e / WIN_W, x = e - r * WIN_W;
        v[k] = (r < nh && x < nw) ? plane[(size_t)r * W + x] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k)
        if (tid + 256 * k < WIN_H * WIN_W) in[tid + 256 * k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NROW; ++k) {
        const int e = tid + 256 * k, r = e / WIN_W, x = e - r * WIN_W;
        if (r < rows && x < nw) {
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) acc += rw[r * TAPS + t] * (double)in[rj[r * TAPS + t] + x];
            mid[(r * S + x % S) * QS + x / S] = acc;
        }
    }
    __syncthreads();
    if (live) {
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int j = tj[t * BP_CT + ox];
            acc += tw[t * BP_CT + ox] * mid[(orow * S + j % S) * QS + j / S];
        }
        d[o] = lrv - (float)acc;
    }
}

// floor((2 Y + 1 - S) / (2 S)): the LR sample at or below SR position Y (the centre of SR sample Y sits at (Y + 0.5) / S - 0.5 in LR coordinates)
template <int S>
__device__ __forceinline__ int bp_lr_floor(int Y) {
    const int a = 2 * Y + 1 - S;
    return a >= 0 ? a / (2 * S) : -((-a + 2 * S - 1) / (2 * S));
}

struct bp_u5 { double u[5]; };

// SR sample Y of imresize(., S) takes the LR samples bp_lr_floor(Y) - 2 .. + 3 (6 table entries, the outer ones with weight 0 or mirrored).  The staged d window is that
// range for the tile and its halo of 2, one sample wider on both sides, cut at the image: at most ceil((T + 3) / S) + 8 samples along an axis with T tile samples.
//   LDS at S = 2 (the largest): dwin [18][42] fp32 + V [20][42] + U [20][68] + T [20][64] fp64 + the taps ([6][68] column, [20][6] row; int32 + fp64)
//   = 3024 + 6720 + 10880 + 10240 + 4896 + 1440 = 37200 bytes, four workgroups on a CU.
//   As in bp_residual_kernel everything read from memory is requested before the first barrier: the d window, the tile's rows of both tap tables (clamped into the
//   window; the column taps transposed to [tap][column]) and the thread's own four sr samples, which wait in registers for the last step.
// grid (ceil(W / BP_UX), ceil(H / BP_UY), C), H = S h, W = S w
template <int S>
__global__ __launch_bounds__(256) void bp_update_kernel(float* __restrict__ sr, const float* __restrict__ d, int h, int w, const int32_t* __restrict__ idx_h,
                                                        const double* __restrict__ w_h, const int32_t* __restrict__ idx_w, const double* __restrict__ w_w, bp_u5 g) {
    constexpr int HY = BP_UY + 4, HX = BP_UX + 4;
    constexpr int DH = (HY - 1 + S - 1) / S + 8, DW = (HX - 1 + S - 1) / S + 8;
    constexpr int NLD = (DH * DW + 255) / 256, NOUT = BP_UY * BP_UX / 256;
    static_assert(BP_UY * BP_UX % 256 == 0 && HY * 6 <= 256, "whole steps of 256 outputs; the row taps are staged in one step");
    __shared__ float dwin[DH * DW];
    __shared__ double V[HY * DW];
    __shared__ double U[HY * HX];
    __shared__ double T[HY * BP_UX];
    __shared__ double cw[6 * HX], rw[HY * 6];
    __shared__ int32_t cj[6 * HX], rj[HY * 6];
    const int tid = threadIdx.x;
    const int H = S * h, W = S * w;
    const int X0 = blockIdx.x * BP_UX, Y0 = blockIdx.y * BP_UY;
    const int ya = max(Y0 - 2, 0), yb = min(Y0 + BP_UY + 1, H - 1), xa = max(X0 - 2, 0), xb = min(X0 + BP_UX + 1, W - 1);
    const int ly0 = max(bp_lr_floor<S>(ya) - 3, 0), lx0 = max(bp_lr_floor<S>(xa) - 3, 0);
    const int nh = min(min(bp_lr_floor<S>(yb) + 4, h - 1) - ly0 + 1, DH), nw = min(min(bp_lr_floor<S>(xb) + 4, w - 1) - lx0 + 1, DW);
#pragma unroll
    for (int e = tid; e < 6 * HX; e += 256) {   // (the table rows of SR columns X0 - 2 .. X0 + BP_UX + 1 inside the image: one contiguous run)
        const int Xl = e / 6, t = e - Xl * 6, X = X0 - 2 + Xl;
        if (X >= 0 && X < W) {
            cj[t * HX + Xl] = min(max(idx_w[(size_t)X * 6 + t] - lx0, 0), nw - 1);
            cw[t * HX + Xl] = w_w[(size_t)X * 6 + t];
        }
    }
    if (tid < HY * 6) {
        const int Y = Y0 - 2 + tid / 6;
        if (Y >= 0 && Y < H) {
            rj[tid] = min(max(idx_h[(size_t)Y * 6 + tid % 6] - ly0, 0), nh - 1) * DW;
            rw[tid] = w_h[(size_t)Y * 6 + tid % 6];
        }
    }
    float* sp = sr + (size_t)blockIdx.z * H * W;
    float own[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int e = tid + 256 * k, Y = Y0 + e / BP_UX, X = X0 + e % BP_UX;
        own[k] = (Y < H && X < W) ? sp[(size_t)Y * W + X] : 0.f;
    }
    const float* dp = d + (size_t)blockIdx.z * h * w + (size_t)ly0 * w + lx0;
    float v[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int e = tid + 256 * k, r = e / DW, x = e - r * DW;
        v[k] = (r < nh && x < nw) ? dp[(size_t)r * w + x] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k)
        if (tid + 256 * k < DH * DW) dwin[tid + 256 * k] = v[k];
    __syncthreads();
    // row pass of the up-sampling: V[Yl][x] for SR row Y = Y0 - 2 + Yl inside the image, window column x
#pragma unroll
    for (int e = tid; e < HY * DW; e += 256) {
        const int Yl = e / DW, x = e - Yl * DW, Y = Y0 - 2 + Yl;
        if (Y < 0 || Y >= H || x >= nw) continue;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 6; ++t) acc += rw[Yl * 6 + t] * (double)dwin[rj[Yl * 6 + t] + x];
        V[e] = acc;
    }
    __syncthreads();
    // column pass: U on the tile and its halo; zero beyond the IMAGE (conv2 'same'), the real up-sampled value beyond the tile
#pragma unroll
    for (int e = tid; e < HY * HX; e += 256) {
        const int Yl = e / HX, Xl = e - Yl * HX, Y = Y0 - 2 + Yl, X = X0 - 2 + Xl;
        double acc = 0.0;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
#pragma unroll
            for (int t = 0; t < 6; ++t) acc += cw[t * HX + Xl] * V[Yl * DW + cj[t * HX + Xl]];
        }
        U[e] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int e = tid; e < HY * BP_UX; e += 256) {
        const int Yl = e / BP_UX, xl = e - Yl * BP_UX;
        const double* up = U + Yl * HX + xl;
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 5; ++b) acc += g.u[b] * up[b];
        T[e] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int e = tid + 256 * k, yl = e / BP_UX, xl = e % BP_UX, Y = Y0 + yl, X = X0 + xl;
        if (Y >= H || X >= W) continue;
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 5; ++a) acc += g.u[a] * T[(yl + a) * BP_UX + xl];
        sp[(size_t)Y * W + X] = (float)((double)own[k] + acc);
    }
}

template <int S>
int bp_residual_launch(const float* sr, const float* lr, int C, int H, int W, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, float* d,
                       void* stream) {
    const dim3 grid((unsigned)((W / S + BP_CT - 1) / BP_CT), (unsigned)((H / S + BP_RT - 1) / BP_RT), (unsigned)C);
    auto k = bp_residual_kernel<S>;
    DASR_LAUNCH_TAG("bp_residual_kernel", k, grid, dim3(256), 0, as_stream(stream), sr, lr, H, W, idx_h, w_h, idx_w, w_w, d);
    return (int)hipGetLastError();
}

template <int S>
int bp_update_launch(float* sr, const float* d, int C, int h, int w, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, const bp_u5& g,
                     void* stream) {
    const dim3 grid((unsigned)((S * w + BP_UX - 1) / BP_UX), (unsigned)((S * h + BP_UY - 1) / BP_UY), (unsigned)C);
    auto k = bp_update_kernel<S>;
    DASR_LAUNCH_TAG("bp_update_kernel", k, grid, dim3(256), 0, as_stream(stream), sr, d, h, w, idx_h, w_h, idx_w, w_w, g);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dasr_bp_residual(const float* sr, const float* lr, int32_t C, int32_t H, int32_t W, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                                const double* w_w, float* d, void* stream) {
    if (!sr || !lr || !idx_h || !w_h || !idx_w || !w_w || !d || C <= 0 || C > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return DASR_EINVAL;
    if (s < 2 || s > 4 || H % s || W % s) return DASR_EINVAL;
    return s == 2 ? bp_residual_launch<2>(sr, lr, C, H, W, idx_h, w_h, idx_w, w_w, d, stream)
         : s == 3 ? bp_residual_launch<3>(sr, lr, C, H, W, idx_h, w_h, idx_w, w_w, d, stream)
                  : bp_residual_launch<4>(sr, lr, C, H, W, idx_h, w_h, idx_w, w_w, d, stream);
}

extern "C" int dasr_bp_update(float* sr, const float* d, int32_t C, int32_t h, int32_t w, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                              const double* w_w, const double* u5, void* stream) {
    if (!sr || !d || !idx_h || !w_h || !idx_w || !w_w || !u5 || C <= 0 || C > 65535 || h <= 0 || w <= 0 || s < 2 || s > 4) return DASR_EINVAL;
    if (h > 65535 / s || w > 65535 / s) return DASR_EINVAL;
    bp_u5 g;
    for (int i = 0; i < 5; ++i) g.u[i] = u5[i];
    return s == 2 ? bp_update_launch<2>(sr, d, C, h, w, idx_h, w_h, idx_w, w_w, g, stream)
         : s == 3 ? bp_update_launch<3>(sr, d, C, h, w, idx_h, w_h, idx_w, w_w, g, stream)
                  : bp_update_launch<4>(sr, d, C, h, w, idx_h, w_h, idx_w, w_w, g, stream);
}

// ---- dataset preparation (`python -m dasr_amd.prepare_data`; reference: codes/SRN/scripts/generate_mod_LR_bic.m:50-64, back_projection/main_reverse_filter.m:18-22; host side:
// dasr_amd/bicubic.py, backproject.reverse_filter) ----------------------------------------------------------------------------------------------------------------------
//  * windows_down_u8_kernel: L = imresize(window / 255.0, 1 / s) of n windows of one resident 8-bit image, the scheme of bp_residual_kernel (the window a tile of LR outputs
//    reaches is staged once, both passes in LDS, everything read from memory requested before the first barrier) with three differences.  The tap tables are those of the
//    WINDOW (hh x ww), so the mirror edge is the window's edge.  The staged samples are the interleaved BYTES as they lie in memory, all three channels of a pixel in one
//    workgroup: a window row is one run of 3 nw bytes, fetched as the aligned 4-byte words that cover it (rows of 3 W bytes start at any of the four byte phases, so the
//    phase of each staged row is kept with its row offset) -- a word that would end beyond the image, or any word of an image whose pointer is not 4-byte aligned, is put
//    together from single bytes.  im2double is a 256-entry table of (double)b / 255.0 in LDS, filled by the workgroup's 256 threads: one correctly rounded division per
//    thread instead of one per tap.
//      LDS at S = 4: bytes [48][436] + lut [256] fp64 + mid [3][8][4][37] fp64 + the tile's taps (6912 + 1728) = 20928 + 2048 + 28416 + 8640 = 60032 bytes, two workgroups on a CU.
//  * imresize_up_kernel: the up-sampling stage of bp_update_kernel on its own (no halo, no 5 x 5 pass), for fp32 or fp64 planes, writing fp32 (plain or accumulated onto
//    dst with one rounding) or interleaved bytes.  With byte output a workgroup walks the C channels of its tile one after the other, so the C bytes of a pixel are written
//    by one workgroup within a few hundred cycles and meet in the cache; the planar modes take one plane per workgroup.
namespace {

constexpr int WD_RT = DASR_WD_TILE_H, WD_CT = DASR_WD_TILE_W;   // LR outputs per workgroup of the window kernel
constexpr int UP_TY = DASR_UP_TILE_H, UP_TX = DASR_UP_TILE_W;   // output samples per workgroup of the up-sampling kernel

// MATLAB's im2uint8 of a double: min(255, max(0, floor(x * 255 + 0.5))), every step rounded to fp64 (contraction is off)
__device__ __forceinline__ uint8_t quant_u8(double x) {
    return (uint8_t)(int)fmin(255.0, fmax(0.0, floor(x * 255.0 + 0.5)));
}

// grid (ceil(ww / S / WD_CT), ceil(hh / S / WD_RT), n)
template <int S>
__global__ __launch_bounds__(256) void windows_down_u8_kernel(const uint8_t* __restrict__ src, int H, int W, int wide, const dasr_window_desc* __restrict__ wins, int hh, int ww,
                                                              const int32_t* __restrict__ idx_h, const double* __restrict__ w_h, const int32_t* __restrict__ idx_w,
                                                              const double* __restrict__ w_w, uint8_t* __restrict__ lr_u8, double* __restrict__ lr_f64) {
    constexpr int TAPS = 4 * S + 2, OFF = S + 1 + S / 2;
    constexpr int WIN_H = S * WD_RT + 3 * S + 4, WIN_W = S * WD_CT + 3 * S + 4, QS = (WIN_W + S - 1) / S + 1;
    constexpr int ROWD = (3 * WIN_W + 3 + 3) / 4, ROWB = 4 * ROWD;   // words / bytes of a staged row: 3 WIN_W bytes behind a phase of up to 3
    constexpr int NLD = (WIN_H * ROWD + 255) / 256, NROW = (WD_RT * 3 * WIN_W + 255) / 256;
    static_assert(WD_RT * WD_CT == 256 && WD_RT * TAPS <= 256, "one output pixel per thread in the column pass; the row taps are staged in one step");
    __shared__ uint32_t in32[WIN_H * ROWD];
    __shared__ double lut[256];
    __shared__ double mid[3 * WD_RT * S * QS];
    __shared__ double tw[TAPS * WD_CT], rw[WD_RT * TAPS];
    __shared__ int32_t tj[TAPS * WD_CT], rj[WD_RT * TAPS];
    const int tid = threadIdx.x;
    const int h = hh / S, w = ww / S;
    const int ox0 = blockIdx.x * WD_CT, oy0 = blockIdx.y * WD_RT;
    const int rows = min(WD_RT, h - oy0), cols = min(WD_CT, w - ox0);
    // (the host checked the corners; clamped all the same: a damaged descriptor reads a wrong window, never outside the image)
    const int y0 = min(max(wins[blockIdx.z].y0, 0), H - hh), x0 = min(max(wins[blockIdx.z].x0, 0), W - ww);
    const int by = max(S * oy0 - OFF - 1, 0), bx = max(S * ox0 - OFF - 1, 0);   // window coordinates: the window is the image of bp_residual_kernel
    const int nh = min(min(S * (oy0 + rows - 1) - OFF + TAPS, hh - 1) - by + 1, WIN_H), nw = min(min(S * (ox0 + cols - 1) - OFF + TAPS, ww - 1) - bx + 1, WIN_W);
    const size_t total = (size_t)H * W * 3, pitch = (size_t)W * 3;
    const size_t g0 = ((size_t)(y0 + by) * W + x0 + bx) * 3;                     // byte offset of staged sample (0, 0), channel 0
    lut[tid] = (double)tid / 255.0;
#pragma unroll
    for (int e = tid; e < WD_CT * TAPS; e += 256) {
        const int ox = e / TAPS, t = e - ox * TAPS;
        if (ox < cols) {
            tj[t * WD_CT + ox] = min(max(idx_w[(size_t)ox0 * TAPS + e] - bx, 0), nw - 1);
            tw[t * WD_CT + ox] = w_w[(size_t)ox0 * TAPS + e];
        }
    }
    if (tid < rows * TAPS) {   // (kept as the byte offset of the staged row's first sample: row offset plus the row's phase)
        const int r = min(max(idx_h[(size_t)oy0 * TAPS + tid] - by, 0), nh - 1);
        rj[tid] = r * ROWB + (int)((g0 + (size_t)r * pitch) & 3);
        rw[tid] = w_h[(size_t)oy0 * TAPS + tid];
    }
    uint32_t v[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int e = tid + 256 * k, r = e / ROWD, q = e - r * ROWD;
        const size_t g = g0 + (size_t)r * pitch, a = (g & ~(size_t)3) + 4 * (size_t)q;   // the q-th aligned word of staged row r
        v[k] = 0u;
        if (r < nh && a < g + 3 * (size_t)nw) {
            if (wide && a + 4 <= total) {
                v[k] = *reinterpret_cast<const uint32_t*>(src + a);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (a + b < total) v[k] |= (uint32_t)src[a + b] << (8 * b);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k)
        if (tid + 256 * k < WIN_H * ROWD) in32[tid + 256 * k] = v[k];
    __syncthreads();
    const uint8_t* inb = reinterpret_cast<const uint8_t*>(in32);
#pragma unroll
    for (int k = 0; k < NROW; ++k) {
        const int e = tid + 256 * k, r = e / (3 * WIN_W), xb = e - r * (3 * WIN_W);
        if (r < rows && xb < 3 * nw) {
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) acc += rw[r * TAPS + t] * lut[inb[rj[r * TAPS + t] + xb]];
            const int x = xb / 3, c = xb - 3 * x;
            mid[((c * WD_RT + r) * S + x % S) * QS + x / S] = acc;
        }
    }
    __syncthreads();
    const int orow = tid / WD_CT, ox = tid % WD_CT;
    if (orow < rows && ox < cols) {
        const size_t o = ((size_t)blockIdx.z * h + oy0 + orow) * w + ox0 + ox;   // pixel index in [n][h][w]
        const size_t plane = (size_t)h * w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int j = tj[t * WD_CT + ox];
                acc += tw[t * WD_CT + ox] * mid[((c * WD_RT + orow) * S + j % S) * QS + j / S];
            }
            if (lr_f64) lr_f64[((size_t)blockIdx.z * 3 + c) * plane + (size_t)(oy0 + orow) * w + ox0 + ox] = acc;
            if (lr_u8) lr_u8[o * 3 + c] = quant_u8(acc);
        }
    }
}

// grid (ceil(W / UP_TX), ceil(H / UP_TY), MODE == DASR_UP_U8 ? N : N C), H = S h, W = S w.  The staged window is the LR range bp_lr_floor(Y) - 2 .. + 3 of the tile's
// rows and columns, one sample wider on both sides, cut at the image (bp_update_kernel's, without the halo): at most ceil((T - 1) / S) + 8 samples along an axis.
//   LDS at S = 2 (the largest): window [16][40] + V [16][40] fp64 + the taps ([6][64] column, [16][6] row; int32 + fp64) = 5120 + 5120 + 4608 + 1152 = 16000 bytes.
template <int S, typename TIn, int MODE>
__global__ __launch_bounds__(256) void imresize_up_kernel(const TIn* __restrict__ x, int C, int h, int w, const int32_t* __restrict__ idx_h, const double* __restrict__ w_h,
                                                          const int32_t* __restrict__ idx_w, const double* __restrict__ w_w, void* __restrict__ dst) {
    constexpr int DH = (UP_TY - 1 + S - 1) / S + 8, DW = (UP_TX - 1 + S - 1) / S + 8;
    constexpr int NLD = (DH * DW + 255) / 256, NOUT = UP_TY * UP_TX / 256;
    static_assert(UP_TY * UP_TX % 256 == 0 && UP_TY * 6 <= 256, "whole steps of 256 outputs; the row taps are staged in one step");
    __shared__ double dwin[DH * DW];
    __shared__ double V[UP_TY * DW];
    __shared__ double cw[6 * UP_TX], rw[UP_TY * 6];
    __shared__ int32_t cj[6 * UP_TX], rj[UP_TY * 6];
    const int tid = threadIdx.x;
    const int H = S * h, W = S * w;
    const int X0 = blockIdx.x * UP_TX, Y0 = blockIdx.y * UP_TY;
    const int yb = min(Y0 + UP_TY - 1, H - 1), xb = min(X0 + UP_TX - 1, W - 1);
    const int ly0 = max(bp_lr_floor<S>(Y0) - 3, 0), lx0 = max(bp_lr_floor<S>(X0) - 3, 0);
    const int nh = min(min(bp_lr_floor<S>(yb) + 4, h - 1) - ly0 + 1, DH), nw = min(min(bp_lr_floor<S>(xb) + 4, w - 1) - lx0 + 1, DW);
#pragma unroll
    for (int e = tid; e < 6 * UP_TX; e += 256) {
        const int Xl = e / 6, t = e - Xl * 6, X = X0 + Xl;
        if (X < W) {
            cj[t * UP_TX + Xl] = min(max(idx_w[(size_t)X * 6 + t] - lx0, 0), nw - 1);
            cw[t * UP_TX + Xl] = w_w[(size_t)X * 6 + t];
        }
    }
    if (tid < UP_TY * 6) {
        const int Y = Y0 + tid / 6;
        if (Y < H) {
            rj[tid] = min(max(idx_h[(size_t)Y * 6 + tid % 6] - ly0, 0), nh - 1) * DW;
            rw[tid] = w_h[(size_t)Y * 6 + tid % 6];
        }
    }
    const int np = MODE == DASR_UP_U8 ? C : 1;   // planes this workgroup walks
    for (int p = 0; p < np; ++p) {
        const size_t plane = (size_t)blockIdx.z * np + p;
        float own[NOUT];
        if (MODE == DASR_UP_F32_ACC) {
            const float* sp = static_cast<const float*>(dst) + plane * H * W;
#pragma unroll
            for (int k = 0; k < NOUT; ++k) {
                const int e = tid + 256 * k, Y = Y0 + e / UP_TX, X = X0 + e % UP_TX;
                own[k] = (Y < H && X < W) ? sp[(size_t)Y * W + X] : 0.f;
            }
        }
        const TIn* dp = x + plane * h * w + (size_t)ly0 * w + lx0;
        TIn v[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int e = tid + 256 * k, r = e / DW, c = e - r * DW;
            v[k] = (r < nh && c < nw) ? dp[(size_t)r * w + c] : (TIn)0;
        }
        // (a second plane overwrites dwin only after every thread has passed the barrier behind the row pass that read it, and V only after the barrier below, which a
        // thread reaches with its column pass over the previous plane done)
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (tid + 256 * k < DH * DW) dwin[tid + 256 * k] = (double)v[k];
        __syncthreads();
#pragma unroll
        for (int e = tid; e < UP_TY * DW; e += 256) {
            const int Yl = e / DW, c = e - Yl * DW;
            if (Y0 + Yl >= H || c >= nw) continue;
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) acc += rw[Yl * 6 + t] * dwin[rj[Yl * 6 + t] + c];
            V[e] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int e = tid + 256 * k, Yl = e / UP_TX, Xl = e % UP_TX, Y = Y0 + Yl, X = X0 + Xl;
            if (Y >= H || X >= W) continue;
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) acc += cw[t * UP_TX + Xl] * V[Yl * DW + cj[t * UP_TX + Xl]];
            if (MODE == DASR_UP_U8)
                static_cast<uint8_t*>(dst)[(((size_t)blockIdx.z * H + Y) * W + X) * C + p] = quant_u8(acc);
            else if (MODE == DASR_UP_F32_ACC)
                static_cast<float*>(dst)[(plane * H + Y) * W + X] = (float)((double)own[k] + acc);
            else
                static_cast<float*>(dst)[(plane * H + Y) * W + X] = (float)acc;
        }
    }
}

template <int S>
int windows_down_launch(const uint8_t* src, int H, int W, const dasr_window_desc* wins, int n, int hh, int ww, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                        const double* w_w, uint8_t* lr_u8, double* lr_f64, void* stream) {
    const dim3 grid((unsigned)((ww / S + WD_CT - 1) / WD_CT), (unsigned)((hh / S + WD_RT - 1) / WD_RT), (unsigned)n);
    const int wide = ((uintptr_t)src & 3) == 0;
    auto k = windows_down_u8_kernel<S>;
    DASR_LAUNCH_TAG("windows_down_u8_kernel", k, grid, dim3(256), 0, as_stream(stream), src, H, W, wide, wins, hh, ww, idx_h, w_h, idx_w, w_w, lr_u8, lr_f64);
    return (int)hipGetLastError();
}

template <int S, typename TIn, int MODE>
int imresize_up_launch(const void* x, int N, int C, int h, int w, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, void* dst, void* stream) {
    const dim3 grid((unsigned)((S * w + UP_TX - 1) / UP_TX), (unsigned)((S * h + UP_TY - 1) / UP_TY), (unsigned)(MODE == DASR_UP_U8 ? N : N * C));
    auto k = imresize_up_kernel<S, TIn, MODE>;
    DASR_LAUNCH_TAG("imresize_up_kernel", k, grid, dim3(256), 0, as_stream(stream), static_cast<const TIn*>(x), C, h, w, idx_h, w_h, idx_w, w_w, dst);
    return (int)hipGetLastError();
}

template <int S, typename TIn>
int imresize_up_mode(int mode, const void* x, int N, int C, int h, int w, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, void* dst,
                     void* stream) {
    return mode == DASR_UP_F32     ? imresize_up_launch<S, TIn, DASR_UP_F32>(x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream)
         : mode == DASR_UP_F32_ACC ? imresize_up_launch<S, TIn, DASR_UP_F32_ACC>(x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream)
                                   : imresize_up_launch<S, TIn, DASR_UP_U8>(x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream);
}

template <int S>
int imresize_up_type(int x_f64, int mode, const void* x, int N, int C, int h, int w, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, void* dst,
                     void* stream) {
    return x_f64 ? imresize_up_mode<S, double>(mode, x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream)
                 : imresize_up_mode<S, float>(mode, x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream);
}

}  // namespace

extern "C" int dasr_windows_down_u8(const uint8_t* src, int32_t H, int32_t W, const dasr_window_desc* wins_dev, const dasr_window_desc* wins_host, int32_t n, int32_t hh,
                                    int32_t ww, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, uint8_t* lr_u8, double* lr_f64,
                                    void* stream) {
    if (!src || !wins_dev || !wins_host || !idx_h || !w_h || !idx_w || !w_w || (!lr_u8 && !lr_f64)) return DASR_EINVAL;
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || n <= 0 || n > 65535 || s < 2 || s > 4) return DASR_EINVAL;
    if (hh <= 0 || ww <= 0 || hh % s || ww % s || hh > H || ww > W) return DASR_EINVAL;
    for (int k = 0; k < n; ++k)
        if (wins_host[k].y0 < 0 || wins_host[k].x0 < 0 || wins_host[k].y0 > H - hh || wins_host[k].x0 > W - ww) return DASR_EINVAL;
    return s == 2 ? windows_down_launch<2>(src, H, W, wins_dev, n, hh, ww, idx_h, w_h, idx_w, w_w, lr_u8, lr_f64, stream)
         : s == 3 ? windows_down_launch<3>(src, H, W, wins_dev, n, hh, ww, idx_h, w_h, idx_w, w_w, lr_u8, lr_f64, stream)
                  : windows_down_launch<4>(src, H, W, wins_dev, n, hh, ww, idx_h, w_h, idx_w, w_w, lr_u8, lr_f64, stream);
}

extern "C" int dasr_imresize_up(const void* x, int32_t x_f64, int32_t N, int32_t C, int32_t h, int32_t w, int32_t s, const int32_t* idx_h, const double* w_h,
                                const int32_t* idx_w, const double* w_w, void* dst, int32_t mode, void* stream) {
    if (!x || !dst || !idx_h || !w_h || !idx_w || !w_w || x == dst || (x_f64 != 0 && x_f64 != 1)) return DASR_EINVAL;
    if (N <= 0 || C <= 0 || N > 65535 || C > 65535 || (long long)N * C > 65535 || h <= 0 || w <= 0 || s < 2 || s > 4) return DASR_EINVAL;
    if (h > 65535 / s || w > 65535 / s) return DASR_EINVAL;
    if (mode != DASR_UP_F32 && mode != DASR_UP_F32_ACC && mode != DASR_UP_U8) return DASR_EINVAL;
    return s == 2 ? imresize_up_type<2>(x_f64, mode, x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream)
         : s == 3 ? imresize_up_type<3>(x_f64, mode, x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream)
                  : imresize_up_type<4>(x_f64, mode, x, N, C, h, w, idx_h, w_h, idx_w, w_w, dst, stream);
}

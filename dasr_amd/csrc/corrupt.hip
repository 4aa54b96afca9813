// The corruptions of codes/DSN/add_corruptions.py on 8-bit RGB images resident in device memory (dasr_amd/corrupt.py states the same arithmetic in numpy):
//  * jpeg_blocks_kernel + jpeg_merge_kernel: the round trip through a baseline 4:2:0 JPEG file as libjpeg-turbo writes and reads it for PIL, without the entropy coder
//    (the file is decoded right after it is encoded, so the coder is a lossless no-op).  Integer arithmetic only, int32 throughout as in libjpeg.
//  * noise_u8_kernel: clip(img + rint(std z)), z from Philox4x32-10 and Box-Muller in fp64, a function of (seed, image index, element index) only.
#include "common.h"

namespace {

// ---- 8-point passes of libjpeg's slow-integer DCT (jfdctint.c / jidctint.c: Loeffler-Ligtenberg-Moschytz, CONST_BITS 13, PASS1_BITS 2) ----------------------------
constexpr int CB = 13, P1 = 2;
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int N = FIRST ? CB - P1 : CB + P1;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * (1 << P1) : descale(t10 + t11, P1);
    d[4] = FIRST ? (t10 - t11) * (1 << P1) : descale(t10 - t11, P1);
    int z1 = (t12 + t13) * F_0_541;
    d[2] = descale(z1 + t13 * F_0_765, N);
    d[6] = descale(z1 - t12 * F_1_847, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175;
    t4 *= F_0_298; t5 *= F_2_053; t6 *= F_3_072; t7 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562;
    z3 = z3 * -F_1_961 + z5;
    z4 = z4 * -F_0_390 + z5;
    d[7] = descale(t4 + z1 + z3, N);
    d[5] = descale(t5 + z2 + z4, N);
    d[3] = descale(t6 + z2 + z3, N);
    d[1] = descale(t7 + z1 + z4, N);
}

template <bool FIRST>
__device__ __forceinline__ void idct8(int (&c)[8]) {
    constexpr int N = FIRST ? CB - P1 : CB + P1 + 3;
    int z1 = (c[2] + c[6]) * F_0_541;
    int t2 = z1 - c[6] * F_1_847, t3 = z1 + c[2] * F_0_765;
    int t0 = (c[0] + c[4]) * (1 << CB), t1 = (c[0] - c[4]) * (1 << CB);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = c[7]; t1 = c[5]; t2 = c[3]; t3 = c[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * F_1_175;
    t0 *= F_0_298; t1 *= F_2_053; t2 *= F_3_072; t3 *= F_1_501;
    z1 *= -F_0_899; z2 *= -F_2_562;
    z3 = z3 * -F_1_961 + z5;
    z4 = z4 * -F_0_390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    c[0] = descale(t10 + t3, N); c[7] = descale(t10 - t3, N);
    c[1] = descale(t11 + t2, N); c[6] = descale(t11 - t2, N);
    c[2] = descale(t12 + t1, N); c[5] = descale(t12 - t1, N);
    c[3] = descale(t13 + t0, N); c[4] = descale(t13 - t0, N);
}

// Annex K base tables in natural order: luminance, chrominance
__device__ const uint8_t jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ __forceinline__ int byte_of(const uint32_t* w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// NPX pixels of one image row from pixel x0 on, as the 3 NPX / 4 words of their bytes.  g_row: byte offset of the row in `src`.  A run that lies inside the row of an
// image whose pointer is 4-byte aligned is fetched as the aligned words that cover it (rows of 3 W bytes start at any of the four byte phases) and shifted into place;
// a word that would end beyond the tensor is put together from bytes.  Any other run is read pixel by pixel with the last column repeated.
template <int NPX>
__device__ __forceinline__ void load_run(const uint8_t* __restrict__ src, size_t total, int wide, size_t g_row, int x0, int W, uint32_t (&out)[NPX * 3 / 4]) {
    constexpr int NW = NPX * 3 / 4;
    if (wide && x0 + NPX <= W) {
        const size_t g = g_row + 3 * (size_t)x0, a = g & ~(size_t)3;
        const unsigned sh = 8u * (unsigned)(g & 3);
        uint32_t w[NW + 1];
#pragma unroll
        for (int i = 0; i <= NW; ++i) {
            const size_t aa = a + 4 * (size_t)i;
            if (aa + 4 <= total) {
                w[i] = *reinterpret_cast<const uint32_t*>(src + aa);
            } else {
                w[i] = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (aa + b < total) w[i] |= (uint32_t)src[aa + b] << (8 * b);
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) out[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> sh);
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) out[i] = 0u;
#pragma unroll
        for (int p = 0; p < NPX; ++p) {
            const uint8_t* q = src + g_row + 3 * (size_t)min(x0 + p, W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(3 * p + c) >> 2] |= (uint32_t)q[c] << (8 * ((3 * p + c) & 3));
        }
    }
}

__device__ __forceinline__ int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

constexpr int JB_TASKS = 32;          // 8 x 8 blocks per workgroup: 8 lanes each, one row or column per lane
constexpr int JB_STRIDE = 8 * 9 + 1;  // ints of LDS per block: rows padded to 9

struct jpeg_geom {
    int bwY, bhY, bwC, bhC, hc, wc;    // blocks across / down of the Y and the chroma planes; real chroma rows / columns
    size_t y_bytes, c_bytes;           // bytes of the Y plane and of one chroma plane
};

inline jpeg_geom jpeg_geometry(int H, int W) {
    jpeg_geom g;
    g.hc = (H + 1) / 2; g.wc = (W + 1) / 2;
    g.bwY = (W + 7) / 8; g.bhY = (H + 7) / 8; g.bwC = (W + 15) / 16; g.bhC = (g.hc + 7) / 8;
    g.y_bytes = (size_t)g.bwY * g.bhY * 64; g.c_bytes = (size_t)g.bwC * g.bhC * 64;
    return g;
}

// grid (ceil(Y blocks / 32) + ceil(chroma blocks / 32), N): the first workgroups take the Y blocks of image blockIdx.y, the others its chroma blocks (Cb, then Cr of the
// same pixels).  Colour conversion and the 2 x 2 chroma average feed the row pass in registers; row pass -> LDS -> column pass, quantise, dequantise, the column pass of
// the inverse (it works on the column the lane already holds) -> LDS -> row pass, + 128, clamp, 8 bytes stored.  Coefficients never leave registers / LDS.
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ src, int N, int H, int W, int wide, int scale, jpeg_geom G, uint8_t* __restrict__ planes) {
    __shared__ int tile[JB_TASKS * JB_STRIDE];
    __shared__ int qt[64];
    const int tid = threadIdx.x, t = tid >> 3, l = tid & 7, n = blockIdx.y;
    const int nY = G.bwY * G.bhY, nC = G.bwC * G.bhC, gY = (nY + JB_TASKS - 1) / JB_TASKS;
    const bool chroma = (int)blockIdx.x >= gY;   // uniform over the workgroup
    const int count = chroma ? nC : nY, bw = chroma ? G.bwC : G.bwY;
    const int task_raw = ((int)blockIdx.x - (chroma ? gY : 0)) * JB_TASKS + t;
    const bool valid = task_raw < count;
    const int task = min(task_raw, count - 1), by = task / bw, bx = task - by * bw;
    if (tid < 64) qt[tid] = min(max((jpeg_base[chroma ? 1 : 0][tid] * scale + 50) / 100, 1), 255);
    const size_t total = (size_t)N * H * W * 3, pitch = (size_t)W * 3, img0 = (size_t)n * H * pitch;
    int s[2][8];
    if (!chroma) {
        uint32_t px[6];
        load_run<8>(src, total, wide, img0 + (size_t)min(by * 8 + l, H - 1) * pitch, bx * 8, W, px);   // the Y plane repeats its last row
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s[0][k] = rgb_y(byte_of(px, 3 * k), byte_of(px, 3 * k + 1), byte_of(px, 3 * k + 2)) - 128;
            s[1][k] = 0;
        }
    } else {
        // rows below the last AVERAGED row repeat it; the full-resolution planes get at most one repeated row (odd H)
        const int rc = min(by * 8 + l, G.hc - 1);
        uint32_t pa[12], pb[12];
        load_run<16>(src, total, wide, img0 + (size_t)(2 * rc) * pitch, bx * 16, W, pa);
        load_run<16>(src, total, wide, img0 + (size_t)min(2 * rc + 1, H - 1) * pitch, bx * 16, W, pb);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int cb = 1 + (k & 1), cr = 1 + (k & 1);   // the bias 1, 2, 1, 2, ... along the output columns
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int o = 3 * (2 * k + e);
                const int r0 = byte_of(pa, o), g0 = byte_of(pa, o + 1), b0 = byte_of(pa, o + 2), r1 = byte_of(pb, o), g1 = byte_of(pb, o + 1), b1 = byte_of(pb, o + 2);
                cb += rgb_cb(r0, g0, b0) + rgb_cb(r1, g1, b1);
                cr += rgb_cr(r0, g0, b0) + rgb_cr(r1, g1, b1);
            }
            s[0][k] = (cb >> 2) - 128;
            s[1][k] = (cr >> 2) - 128;
        }
    }
    int* my = tile + t * JB_STRIDE;
    const size_t wp = (size_t)bw * 8;   // padded width of the plane
    uint8_t* out = planes + (size_t)n * (G.y_bytes + 2 * G.c_bytes) + (chroma ? G.y_bytes : 0) + ((size_t)by * 8 + l) * wp + (size_t)bx * 8;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !chroma) break;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = s[pass][k];
        fdct8<true>(d);                      // row l
#pragma unroll
        for (int k = 0; k < 8; ++k) my[l * 9 + k] = d[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = my[k * 9 + l];
        fdct8<false>(d);                     // column l: 8 x the DCT
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = qt[k * 8 + l], a = (int)((unsigned)(abs(d[k]) + ((8 * q) >> 1)) / (unsigned)(8 * q)) * q;
            d[k] = d[k] < 0 ? -a : a;
        }
        idct8<true>(d);                      // jidctint.c works on the columns first
#pragma unroll
        for (int k = 0; k < 8; ++k) my[k * 9 + l] = d[k];   // (the column this lane read: nobody else touches it)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = my[l * 9 + k];
        idct8<false>(d);                     // row l
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(max(d[k] + 128, 0), 255) << (8 * k);
            hi |= (uint32_t)min(max(d[k + 4] + 128, 0), 255) << (8 * k);
        }
        if (valid) *reinterpret_cast<uint2*>(out + (size_t)pass * G.c_bytes) = make_uint2(lo, hi);   // (the next pass writes row l of the tile, which only this lane has read)
    }
}

constexpr int JM_TX = 64, JM_TY = 4;

// grid (ceil(ceil(wc / 2) / 64), ceil(hc / 4), N), block (64, 4): one thread per chroma row and PAIR of chroma columns = 2 rows of 4 pixels.  The triangle filter of
// h2v2_fancy_upsample (3/4 this + 1/4 neighbour, rows first on 3 this + neighbour, then columns with + 8 / + 7 and >> 4) with the neighbour of an edge sample the sample
// itself (4 this + 8, 4 this + 7 at the two ends of a row); plain replication when the chroma plane is at most 2 wide, as jdsample.c chooses.
__global__ __launch_bounds__(256) void jpeg_merge_kernel(const uint8_t* __restrict__ planes, int H, int W, int wide, jpeg_geom G, uint8_t* __restrict__ dst) {
    const int jj = blockIdx.x * JM_TX + threadIdx.x, r = blockIdx.y * JM_TY + threadIdx.y, n = blockIdx.z;
    const int j0 = 2 * jj;
    if (r >= G.hc || j0 >= G.wc) return;
    const size_t wy = (size_t)G.bwY * 8, wcp = (size_t)G.bwC * 8;
    const uint8_t* yp = planes + (size_t)n * (G.y_bytes + 2 * G.c_bytes);
    const uint8_t* cp = yp + G.y_bytes;
    const int rows[3] = {max(r - 1, 0), r, min(r + 1, G.hc - 1)};
    int col[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) col[c] = min(max(j0 - 1 + c, 0), G.wc - 1);
    int up[2][2][4];   // [row of the pair][Cb, Cr][pixel]
    if (G.wc > 2) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint8_t* pl = cp + (size_t)p * G.c_bytes;
            int v[2][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int a = pl[rows[0] * wcp + col[c]], b = pl[rows[1] * wcp + col[c]], d = pl[rows[2] * wcp + col[c]];
                v[0][c] = 3 * b + a;
                v[1][c] = 3 * b + d;
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                up[e][p][0] = (3 * v[e][1] + v[e][0] + 8) >> 4;
                up[e][p][1] = (3 * v[e][1] + v[e][2] + 7) >> 4;
                up[e][p][2] = (3 * v[e][2] + v[e][1] + 8) >> 4;
                up[e][p][3] = (3 * v[e][2] + v[e][3] + 7) >> 4;
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int a = cp[(size_t)p * G.c_bytes + r * wcp + col[1]], b = cp[(size_t)p * G.c_bytes + r * wcp + col[2]];
#pragma unroll
            for (int e = 0; e < 2; ++e) { up[e][p][0] = up[e][p][1] = a; up[e][p][2] = up[e][p][3] = b; }
        }
    }
    const int x0 = 4 * jj;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int y = 2 * r + e;
        if (y >= H) break;
        const uint32_t yw = *reinterpret_cast<const uint32_t*>(yp + y * wy + x0);   // (x0 + 4 <= the padded width: it is a multiple of 8 above x0)
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int Y = (int)((yw >> (8 * k)) & 255u), cb = up[e][0][k] - 128, cr = up[e][1][k] - 128;
            const int rgb[3] = {Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)};
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(3 * k + c) >> 2] |= (uint32_t)min(max(rgb[c], 0), 255) << (8 * ((3 * k + c) & 3));
        }
        const size_t g = (((size_t)n * H + y) * W + x0) * 3;
        if (wide && x0 + 4 <= W && (g & 3) == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) reinterpret_cast<uint32_t*>(dst + g)[i] = o[i];
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (x0 + b / 3 < W) dst[g + b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// ---- noise ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// grid (ceil(ceil(per / 4) / 256), N): one thread per group of four consecutive elements of image blockIdx.y (counter: group lo, group hi, index0 + image, 0; key: seed).
// The four outputs are two Box-Muller pairs in fp64: u1 = (x + 1) 2^-32, u2 = x 2^-32, sqrt(-2 ln u1) (cos, sin)(2 pi u2).
__global__ __launch_bounds__(256) void noise_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t per, int wide, double std, uint32_t k0, uint32_t k1,
                                                       uint32_t index0) {
    const uint64_t grp = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const int64_t e0 = (int64_t)(4 * grp);
    if (e0 >= per) return;
    uint32_t c[4] = {(uint32_t)grp, (uint32_t)(grp >> 32), index0 + blockIdx.y, 0u};
    philox4x32_10(c, k0, k1);
    double z[4];
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const double u1 = ((double)c[k] + 1.0) * 0x1p-32, u2 = (double)c[k + 1] * 0x1p-32;
        const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * 3.141592653589793 * u2;
        z[k] = rad * cos(ang);
        z[k + 1] = rad * sin(ang);
    }
    const size_t g = (size_t)blockIdx.y * (size_t)per + (size_t)e0;
    const int cnt = (int)min((int64_t)4, per - e0);
    const bool word = wide && cnt == 4 && (g & 3) == 0;
    uint32_t in = 0u, o = 0u;
    if (word) {
        in = *reinterpret_cast<const uint32_t*>(src + g);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) in |= (uint32_t)src[g + k] << (8 * k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v = (double)((in >> (8 * k)) & 255u) + rint(std * z[k]);
        o |= (uint32_t)fmin(fmax(v, 0.0), 255.0) << (8 * k);
    }
    if (word) {
        *reinterpret_cast<uint32_t*>(dst + g) = o;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) dst[g + k] = (uint8_t)(o >> (8 * k));
    }
}

bool jpeg_args_ok(const void* a, const void* b, int N, int H, int W) { return a && b && a != b && N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }

}  // namespace

extern "C" int dasr_jpeg_blocks(const uint8_t* src, int32_t N, int32_t H, int32_t W, int32_t quality, uint8_t* planes, void* stream) {
    if (!jpeg_args_ok(src, planes, N, H, W) || quality < 1 || quality > 100 || ((uintptr_t)planes & 7)) return DASR_EINVAL;
    const jpeg_geom G = jpeg_geometry(H, W);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const unsigned gx = (unsigned)((G.bwY * G.bhY + JB_TASKS - 1) / JB_TASKS + (G.bwC * G.bhC + JB_TASKS - 1) / JB_TASKS);
    DASR_LAUNCH(jpeg_blocks_kernel, dim3(gx, (unsigned)N), dim3(256), 0, as_stream(stream), src, N, H, W, (int)(((uintptr_t)src & 3) == 0), scale, G, planes);
    return (int)hipGetLastError();
}

extern "C" int dasr_jpeg_merge(const uint8_t* planes, int32_t N, int32_t H, int32_t W, uint8_t* dst, void* stream) {
    if (!jpeg_args_ok(planes, dst, N, H, W) || ((uintptr_t)planes & 7)) return DASR_EINVAL;
    const jpeg_geom G = jpeg_geometry(H, W);
    const dim3 grid((unsigned)(((G.wc + 1) / 2 + JM_TX - 1) / JM_TX), (unsigned)((G.hc + JM_TY - 1) / JM_TY), (unsigned)N);
    DASR_LAUNCH(jpeg_merge_kernel, grid, dim3(JM_TX, JM_TY), 0, as_stream(stream), planes, H, W, (int)(((uintptr_t)dst & 3) == 0), G, dst);
    return (int)hipGetLastError();
}

extern "C" int dasr_noise_u8(const uint8_t* src, uint8_t* dst, int32_t N, int64_t per, double std, int64_t seed, int64_t index0, void* stream) {
    if (!src || !dst || N < 1 || N > 65535 || per < 1 || per > ((int64_t)1 << 36) || !(std >= 0.0) || std > 1.0e300 || index0 < 0 || index0 + N > ((int64_t)1 << 32))
        return DASR_EINVAL;
    const unsigned gx = (unsigned)(((per + 3) / 4 + 255) / 256);
    const int wide = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    DASR_LAUNCH(noise_u8_kernel, dim3(gx, (unsigned)N), dim3(256), 0, as_stream(stream), src, dst, per, wide, std, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32),
                (uint32_t)index0);
    return (int)hipGetLastError();
}

// Fused residual block of SRResNet (dasr_resblock, include/dasr_hip.h; reference: ResNetBlock, codes/SRN/models/modules/block.py:221-251).
//
// One workgroup = one 16 x 16 output tile of one image, 8 waves, ONE workgroup per CU (129.5 KB of LDS):
//   input window  20 x 20 pixels x 64 channels bf16   51 200 B   [chunk][pixel][32 B]
//   h window      18 x 18 pixels x 64 channels bf16   41 472 B   [chunk][pixel][32 B]
//   weights       2 x one 16-channel chunk of a conv  36 864 B   (the packed chunk image of dasr_pack_weights, mt 2: [tap][m-tile][lane][16 B])
// Both convs' whole weights (147 KB) do not fit beside the two windows, so the eight (conv, chunk) steps stream through two chunk buffers:
// the chunk of step t + 1 is fetched into registers while step t multiplies, then written to the other buffer in front of the step's barrier.
// conv0 runs over the 324 h pixels as 11 groups of 32 (the MFMA N dimension; lanes of the last group past pixel 323 compute a discarded copy
// of pixel 0): wave w owns groups w and w + 8.  conv1 runs over the 256 output pixels as 8 groups of 32 (two tile rows each): wave w owns group w.
// Every wave multiplies both 32-channel m-tiles of its groups.
//
// Bit-identity with dasr_conv (conv_glds_kernel, csrc/conv.hip): every accumulator sees the same sequence of v_mfma_f32_32x32x16_bf16 --
// chunks in order, inside a chunk the taps in the order kx-major / ky-minor, A = packed weight fragment, B = activation fragment (lane (nn, kh2):
// pixel nn, channels 8 kh2 .. 8 kh2 + 7) -- from the same initial value (0 for conv0; x32 / res_scale for conv1, the R1_PRE form of the conv5-class
// epilogue), and the same epilogue arithmetic (conv0: v + b0, fmaxf(v, 0) + slope * fminf(v, 0), bf16; conv1: v + b1, * res_scale when != 1).
#include "common.h"

namespace {

constexpr int RB_TH = 16, RB_TW = 16;                        // output tile
constexpr int RB_HH = RB_TH + 2, RB_HW = RB_TW + 2;          // h window (one-pixel halo)
constexpr int RB_XH = RB_TH + 4, RB_XW = RB_TW + 4;          // input window (two-pixel halo)
constexpr int RB_XPIX = RB_XH * RB_XW, RB_HPIX = RB_HH * RB_HW;
constexpr int RB_XCK = RB_XPIX * 32, RB_HCK = RB_HPIX * 32;  // bytes of one 16-channel chunk of a window
constexpr int RB_X_BYTES = 4 * RB_XCK, RB_H_BYTES = 4 * RB_HCK;
constexpr int RB_W_BYTES = 9 * 2 * 1024;                     // one chunk of packed weights, 64 output channels (mt 2)
constexpr int RB_LDS = RB_X_BYTES + RB_H_BYTES + 2 * RB_W_BYTES;
constexpr int RB_NTH = 512;
constexpr int RB_G0 = (RB_HPIX + 31) / 32;                   // conv0 pixel groups (11)
constexpr int RB_WPIECES = RB_W_BYTES / 16;
constexpr int RB_WR = (RB_WPIECES + RB_NTH - 1) / RB_NTH;
static_assert(RB_LDS <= 160 * 1024, "LDS per CU");
static_assert(RB_TH * RB_TW == 8 * 32, "conv1: one group of 32 output pixels per wave");
static_assert(RB_G0 <= 16, "conv0: at most two groups per wave");

template <bool TRAIN>
__global__ __launch_bounds__(RB_NTH, 2) void resblock_kernel(const dasr_resblock_params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const xs = smem;
    char* const hs = smem + RB_X_BYTES;
    char* const wsb = hs + RB_H_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nn = lane & 31, kh2 = lane >> 5;
    const int H = p.H, W = p.W;
    const int tiles_x = (W + RB_TW - 1) / RB_TW, tiles_y = (H + RB_TH - 1) / RB_TH;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int oy0 = ty * RB_TH, ox0 = tx * RB_TW;

    // ---- weights of step t (t < 4: conv0 chunk t, else conv1 chunk t - 4), staged through registers
    u32x4 wreg[RB_WR];
    auto wload = [&](int t) {
        const u32x4* src = (const u32x4*)((const char*)(t < 4 ? p.w0 : p.w1) + (size_t)(t & 3) * RB_W_BYTES);
#pragma unroll
        for (int r = 0; r < RB_WR; ++r) {
            const int q = tid + r * RB_NTH;
            if (q < RB_WPIECES) wreg[r] = src[q];
        }
    };
    auto wstore = [&](int t) {
        u32x4* dst = (u32x4*)(wsb + (t & 1) * RB_W_BYTES);
#pragma unroll
        for (int r = 0; r < RB_WR; ++r) {
            const int q = tid + r * RB_NTH;
            if (q < RB_WPIECES) dst[q] = wreg[r];
        }
    };
    wload(0);

    // ---- input window: 20 x 20 pixels around the tile, zero outside the image (conv0's zero padding)
    {
        const bf16_t* x16 = (const bf16_t*)p.x16.p + (size_t)n * p.x16.n_stride;
        for (int q = tid; q < 4 * RB_XPIX * 2; q += RB_NTH) {
            const int half = q & 1, pc = q >> 1;
            const int ck = pc / RB_XPIX, pix = pc - ck * RB_XPIX;
            const int iy = pix / RB_XW, ix = pix - iy * RB_XW;
            const int gy = oy0 - 2 + iy, gx = ox0 - 2 + ix;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const u32x4*)(x16 + (size_t)ck * p.x16.cb_stride + ((size_t)gy * W + gx) * 16 + 8 * half);
            *(u32x4*)(xs + ck * RB_XCK + pix * 32 + half * 16) = v;
        }
    }
    wstore(0);
    __syncthreads();

    // ---- conv0 groups of this wave: h pixel q = group * 32 + nn (clamped to pixel 0 past the window), input pixel of tap (0, 0)
    const bool two = wave + 8 < RB_G0;
    int pb0[2];
#pragma unroll
    for (int gs = 0; gs < 2; ++gs) {
        const int q = (wave + 8 * gs) * 32 + nn;
        const int qq = q < RB_HPIX ? q : 0;
        const int hr = qq / RB_HW, hc = qq - hr * RB_HW;
        pb0[gs] = hr * RB_XW + hc;
    }
    // conv1 group of this wave: output pixel (r, c) of the tile, h pixel of tap (0, 0)
    const int r1 = 2 * wave + (nn >> 4), c1 = nn & 15;
    const int pb1 = r1 * RB_HW + c1;
    const int oy = oy0 + r1, ox = ox0 + c1;
    const bool out_ok = oy < H && ox < W;

    f32x16 acc0[2][2], acc1[2];
#pragma unroll
    for (int gs = 0; gs < 2; ++gs)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc0[gs][mi][j] = 0.f;

    for (int t = 0; t < 8; ++t) {
        if (t + 1 < 8) wload(t + 1);
        const char* wb = wsb + (t & 1) * RB_W_BYTES + lane * 16;
        const int ck = t & 3;
        if (t < 4) {
            const char* xb = xs + ck * RB_XCK + kh2 * 16;
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const int kx = s / 3, ky = s - kx * 3, tap = ky * 3 + kx;
                const bf16x8 a0 = *(const bf16x8*)(wb + (tap * 2 + 0) * 1024);
                const bf16x8 a1 = *(const bf16x8*)(wb + (tap * 2 + 1) * 1024);
                const bf16x8 b0 = *(const bf16x8*)(xb + (pb0[0] + ky * RB_XW + kx) * 32);
                acc0[0][0] = mfma16<false>(a0, b0, acc0[0][0]);
                acc0[0][1] = mfma16<false>(a1, b0, acc0[0][1]);
                if (two) {
                    const bf16x8 b1 = *(const bf16x8*)(xb + (pb0[1] + ky * RB_XW + kx) * 32);
                    acc0[1][0] = mfma16<false>(a0, b1, acc0[1][0]);
                    acc0[1][1] = mfma16<false>(a1, b1, acc0[1][1]);
                }
            }
        } else {
            const char* hb = hs + ck * RB_HCK + kh2 * 16;
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const int kx = s / 3, ky = s - kx * 3, tap = ky * 3 + kx;
                const bf16x8 a0 = *(const bf16x8*)(wb + (tap * 2 + 0) * 1024);
                const bf16x8 a1 = *(const bf16x8*)(wb + (tap * 2 + 1) * 1024);
                const bf16x8 b = *(const bf16x8*)(hb + (pb1 + ky * RB_HW + kx) * 32);
                acc1[0] = mfma16<false>(a0, b, acc1[0]);
                acc1[1] = mfma16<false>(a1, b, acc1[1]);
            }
        }
        if (t == 3) {
            // ---- conv0 epilogue: h = bf16(act(acc + b0)) into the h window (zero outside the image); training: the tile's interior to p.h
            const float slope = p.slope;
            bf16_t* hg = TRAIN ? (bf16_t*)p.h.p + (size_t)n * p.h.n_stride : nullptr;
#pragma unroll
            for (int gs = 0; gs < 2; ++gs) {
                if (gs == 1 && !two) continue;
                const int q = (wave + 8 * gs) * 32 + nn;
                if (q >= RB_HPIX) continue;
                const int hr = q / RB_HW, hc = q - hr * RB_HW;
                const int gy = oy0 - 1 + hr, gx = ox0 - 1 + hc;
                const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                const bool interior = inside && hr >= 1 && hr <= RB_TH && hc >= 1 && hc <= RB_TW;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int oc = mi * 32 + 8 * g + 4 * kh2;
                        bf16x4 o;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float v = acc0[gs][mi][4 * g + j] + p.b0[oc + j];
                            v = fmaxf(v, 0.f) + slope * fminf(v, 0.f);
                            o[j] = inside ? (bf16_t)v : (bf16_t)0.f;
                        }
                        const u32x2 ov = __builtin_bit_cast(u32x2, o);
                        *(u32x2*)(hs + (oc >> 4) * RB_HCK + q * 32 + (oc & 15) * 2) = ov;
                        if (TRAIN && interior) *(u32x2*)(hg + (size_t)(oc >> 4) * p.h.cb_stride + ((size_t)gy * W + gx) * 16 + (oc & 15)) = ov;
                    }
            }
            // ---- conv1 accumulators start from x32 / res_scale (the skip, folded in front of the MFMAs as dasr_conv's conv5-class epilogue does)
            const float* x32 = (const float*)p.x32.p + (size_t)n * p.x32.n_stride;
            const float c1s = 1.f / p.res_scale;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int oc = mi * 32 + 8 * g + 4 * kh2;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (out_ok) v = *(const f32x4*)(x32 + (size_t)(oc >> 4) * p.x32.cb_stride + ((size_t)oy * W + ox) * 16 + (oc & 15));
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc1[mi][4 * g + j] = v[j] * c1s;
                }
        }
        if (t + 1 < 8) wstore(t + 1);
        __syncthreads();
    }

    // ---- conv1 epilogue: y = (acc + b1) * res_scale -> fp32 stream and bf16 shadow
    if (!out_ok) return;
    float* y32 = (float*)p.y32.p + (size_t)n * p.y32.n_stride;
    bf16_t* y16 = (bf16_t*)p.y16.p + (size_t)n * p.y16.n_stride;
    const bool scaled = p.res_scale != 1.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int oc = mi * 32 + 8 * g + 4 * kh2;
            f32x4 v;
            bf16x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float u = acc1[mi][4 * g + j] + p.b1[oc + j];
                if (scaled) u *= p.res_scale;
                v[j] = u;
                o[j] = (bf16_t)u;
            }
            const size_t pix = ((size_t)oy * W + ox) * 16 + (oc & 15);
            *(f32x4*)(y32 + (size_t)(oc >> 4) * p.y32.cb_stride + pix) = v;
            *(u32x2*)(y16 + (size_t)(oc >> 4) * p.y16.cb_stride + pix) = __builtin_bit_cast(u32x2, o);
        }
}

template <bool TRAIN>
int launch_resblock(const dasr_resblock_params& p, hipStream_t s) {
    static bool attr_set = false;
    auto kfn = resblock_kernel<TRAIN>;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, RB_LDS));
        attr_set = true;
    }
    const long long grid = (long long)p.N * ((p.H + RB_TH - 1) / RB_TH) * ((p.W + RB_TW - 1) / RB_TW);
    if (grid <= 0 || grid >= (1LL << 31)) return DASR_EINVAL;
    DASR_LAUNCH(kfn, dim3((unsigned)grid), dim3(RB_NTH), RB_LDS, s, p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dasr_resblock(const dasr_resblock_params* pp, void* stream) {
    if (!pp) return DASR_EINVAL;
    const dasr_resblock_params& p = *pp;
    if (!p.x16.p || !p.x32.p || !p.w0 || !p.w1 || !p.b0 || !p.b1 || !p.y32.p || !p.y16.p) return DASR_EINVAL;
    if (p.N <= 0 || p.H <= 0 || p.W <= 0 || !(p.res_scale != 0.f)) return DASR_EINVAL;
    // 64 channels = 4 planes per tensor: every plane stride must leave room for a whole H x W plane, every image for four of them
    const long long plane = (long long)p.H * p.W * 16;
    const dasr_tensor* ts[5] = {&p.x16, &p.x32, &p.y32, &p.y16, &p.h};
    for (int i = 0; i < 5; ++i) {
        if (!ts[i]->p) continue;
        if (ts[i]->cb_stride < plane || ts[i]->n_stride < 4 * ts[i]->cb_stride) return DASR_EINVAL;
        if (((uintptr_t)ts[i]->p & 15) != 0) return DASR_EINVAL;
    }
    // a tile reads its neighbours' input halo while they write their outputs: no output may overlap an input or another output (byte ranges)
    const int esz[5] = {2, 4, 4, 2, 2};
    uintptr_t lo[5], hi[5];
    for (int i = 0; i < 5; ++i) {
        lo[i] = (uintptr_t)ts[i]->p;
        hi[i] = ts[i]->p ? lo[i] + (uintptr_t)(((long long)(p.N - 1) * ts[i]->n_stride + 3 * ts[i]->cb_stride + plane) * esz[i]) : lo[i];
    }
    for (int o = 2; o < 5; ++o)
        for (int i = 0; i < 5; ++i)
            if (i != o && ts[o]->p && ts[i]->p && lo[o] < hi[i] && lo[i] < hi[o]) return DASR_EINVAL;
    hipStream_t s = as_stream(stream);
    return p.h.p ? launch_resblock<true>(p, s) : launch_resblock<false>(p, s);
}

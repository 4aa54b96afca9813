// Weight-gradient kernels for gfx950.
//
// dW[oc][c][tap] = sum_{n,y,x} G[n][oc][y][x] * X[n][c][y*S+ky-P][x*S+kx-P]
// GEMM view per tap: D[oc][c] = sum_k A[oc][k] * B[k][c], k = output pixel.  Both operands are stored
// pixel-major ([pixel][16 channels]) so the MFMA fragments (8 consecutive k per lane) are gathered with
// the LDS transpose read ds_read_b64_tr_b16 (4 pixels x 16 channels per 16-lane group).
// One workgroup (4 waves) = one "part" (32 oc x up to 64 cin x all taps of one conv) x one pixel split.
// wave w: cin tile = w & 1, tap group = w >> 1.  Partial sums -> workspace; wgrad_reduce sums the splits
// in a fixed order (deterministic) and scatters into the reference layout [cout][cin][kh][kw].
#include "common.h"
#include <type_traits>

namespace {

template <int KH, int STRIDE>
struct WCfg {
    static constexpr int NTAPS = KH * KH;
    static constexpr int TAPS_PER_PART = NTAPS <= 16 ? NTAPS : 10;  // 5x5: three parts of 10 / 10 / 5 taps
    static constexpr int TPG = (TAPS_PER_PART + 1) / 2;             // taps per wave
    static constexpr int PH = STRIDE == 2 ? 2 : ((KH == 3 || KH == 1) ? 8 : 4), PW = 16;  // output-pixel tile (PH k-steps of 16 pixels)
    static constexpr int IH = (PH - 1) * STRIDE + KH;
    static constexpr int IW = (PW - 1) * STRIDE + KH;
    static constexpr int GPLANE = PH * PW * 32 + 128;  // bytes; stride = 128 (mod 256): the two planes of a
    static constexpr int IPLANE_RAW = IH * IW * 32;    // 32-lane half hit disjoint bank halves
    static constexpr int IPLANE = IPLANE_RAW + ((IPLANE_RAW % 256) == 128 ? 0 : ((128 - (IPLANE_RAW % 256) + 256) % 256));
    static constexpr int G_BYTES = 2 * GPLANE;
    static constexpr int I_BYTES = 4 * IPLANE;
    static constexpr int LDS_BYTES = G_BYTES + I_BYTES;
};

template <bool F16>
__device__ __forceinline__ float frag_f32(bf16x8 a, int j) {
    if constexpr (F16) return (float)__builtin_bit_cast(f16x8, a)[j];
    else return (float)a[j];
}

__device__ __forceinline__ bf16x8 frag_tr(const char* base, int off0, int off1) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((DASR_LDS bf16x4*)(base + off0));
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((DASR_LDS bf16x4*)(base + off1));
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Staging helpers: one "piece" = 16 B of LDS payload (8 bf16 channels of one pixel).  For f32 sources a piece is
// assembled from two 16 B global loads (8 floats) and rounded to bf16 on the way.
template <bool F32>
struct StageReg {
    u32x4 a, b;  // b only used when F32
};

// branch-free staging loads: an out-of-range buffer offset reads as zero (halo / partial tiles / missing planes)
constexpr unsigned OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7fffffff, 0x00020000);
}

template <bool F32>
__device__ __forceinline__ void stage_load(StageReg<F32>& r, __amdgpu_buffer_rsrc_t rs, unsigned eoff, bool ok) {
    if constexpr (F32) {
        const unsigned o = ok ? eoff * 4u : OOB;
        r.a = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
        r.b = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 16, 0);
    } else {
        r.a = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? eoff * 2u : OOB, 0, 0);
    }
}

// F16: the f32 values are multiplied by `scale` (a power of two) and rounded to f16 instead of bf16
template <bool F32, bool F16 = false>
__device__ __forceinline__ void stage_store(const StageReg<F32>& r, char* dst, float scale = 1.f) {
    if constexpr (F32 && F16) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = (f16_t)(__uint_as_float(r.a[j]) * scale);
            o[4 + j] = (f16_t)(__uint_as_float(r.b[j]) * scale);
        }
        *(f16x8*)dst = o;
    } else if constexpr (F32) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = (bf16_t)__uint_as_float(r.a[j]);
            o[4 + j] = (bf16_t)__uint_as_float(r.b[j]);
        }
        *(bf16x8*)dst = o;
    } else {
        *(u32x4*)dst = r.a;
    }
}

// (4x4 kernels: 8 accumulator tiles per wave + the staging registers of an f32 source need ~290 registers: one workgroup per CU instead of
// scratch spills inside the MFMA loop -- VERDICT r02 item 10)
template <int KH, int STRIDE, bool USE_TR, bool F32, bool F16 = false>
__global__ __launch_bounds__(256, KH == 4 ? 1 : 2) void wgrad_kernel(const dasr_wgrad_part* __restrict__ parts, int nparts, int nsplit,
                                                       float* __restrict__ ws) {
    static_assert(!F16 || F32, "f16 staging converts f32 tensors");
    using C = WCfg<KH, STRIDE>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* gl = smem;
    char* il = smem + C::G_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int part_id = blockIdx.x / nsplit, split = blockIdx.x - part_id * nsplit;
    const dasr_wgrad_part P = parts[part_id];
    const int ct = wave & 1, tg = wave >> 1;
    const bool active = ct < P.n_ctiles;
    const int tiles_x = (P.Wout + C::PW - 1) / C::PW, tiles_y = (P.Hout + C::PH - 1) / C::PH;
    const int ntiles = tiles_x * tiles_y * P.N;
    const int HL = P.ups ? 2 * P.Hin : P.Hin, WL = P.ups ? 2 * P.Win : P.Win;
    constexpr int ESZ = F32 ? 4 : 2;
    constexpr int GPIX = C::PH * C::PW, IPIX = C::IH * C::IW;
    constexpr int GPIECES = 2 * GPIX * 2;          // 2 planes x pixels x 2 halves (8 channels each)
    constexpr int GR = (GPIECES + 255) / 256;
    constexpr int IPIECES_MAX = 4 * IPIX * 2;
    constexpr int IR = (IPIECES_MAX + 255) / 256;
    const int ipieces = 2 * P.n_ctiles * IPIX * 2;
    const float gsc = (F16 && P.g_scale != 0.f) ? P.g_scale : 1.f;

    f32x16 acc[C::TPG];
#pragma unroll
    for (int t = 0; t < C::TPG; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
    float bsum = 0.f;
    const int gg = lane >> 4, li = lane & 15;
    const int fplane = gg & 1, khalf = gg >> 1;

    StageReg<F32> greg[GR], ireg[IR];

    auto prefetch = [&](int tile) {
        int t2 = tile;
        const int tx = t2 % tiles_x;
        t2 /= tiles_x;
        const int ty = t2 % tiles_y;
        const int n = t2 / tiles_y;
        const int oy0 = ty * C::PH, ox0 = tx * C::PW;
        const int iy0 = oy0 * STRIDE - P.pad, ix0 = ox0 * STRIDE - P.pad;
        const __amdgpu_buffer_rsrc_t gb = make_rsrc((const char*)P.g.p + (size_t)n * P.g.n_stride * ESZ);
        const __amdgpu_buffer_rsrc_t ib = make_rsrc((const char*)P.in.p + (size_t)n * P.in.n_stride * ESZ);
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            const int q = tid + r * 256;
            const int half = q & 1, pix = (q >> 1) % GPIX, pl = (q >> 1) / GPIX;
            const int py = pix / C::PW, px = pix - py * C::PW;
            const int oy = oy0 + py, ox = ox0 + px;
            const bool ok = q < GPIECES && oy < P.Hout && ox < P.Wout && pl < P.g_planes;
            stage_load<F32>(greg[r], gb, (unsigned)(pl * (int)P.g.cb_stride + (oy * P.Wout + ox) * 16 + half * 8), ok);
        }
#pragma unroll
        for (int r = 0; r < IR; ++r) {
            const int q = tid + r * 256;
            const int half = q & 1, pix = (q >> 1) % IPIX, pl = (q >> 1) / IPIX;
            const int iy = pix / C::IW, ix = pix - iy * C::IW;
            const int gy = iy0 + iy, gx = ix0 + ix;
            const bool ok = q < ipieces && gy >= 0 && gy < HL && gx >= 0 && gx < WL && pl < P.in_planes;
            const int sy = P.ups ? gy >> 1 : gy, sx = P.ups ? gx >> 1 : gx;
            stage_load<F32>(ireg[r], ib, (unsigned)(pl * (int)P.in.cb_stride + (sy * P.Win + sx) * 16 + half * 8), ok);
        }
    };
    char* const dummy = smem + C::LDS_BYTES;  // 16 B slot that swallows the tail threads' stores (no divergent branch)
    // f32 gradients: the bias gradient (sum over pixels, heavy cancellation) is accumulated from the UNROUNDED values
    // while staging; thread t always stages the same 8 channels (plane, half) in round r.
    float bacc[GR][8];
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j) bacc[r][j] = 0.f;
    auto commit = [&]() {
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            const int q = tid + r * 256;
            const int half = q & 1, pix = (q >> 1) % GPIX, pl = (q >> 1) / GPIX;
            stage_store<F32, F16>(greg[r], q < GPIECES ? gl + pl * C::GPLANE + pix * 32 + half * 16 : dummy, gsc);
            if constexpr (F32) {   // (scaled like the staged values: the caller's reduce scale undoes g_scale for weights and bias alike)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bacc[r][j] += __uint_as_float(greg[r].a[j]) * gsc;
                    bacc[r][4 + j] += __uint_as_float(greg[r].b[j]) * gsc;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < IR; ++r) {
            const int q = tid + r * 256;
            const int half = q & 1, pix = (q >> 1) % IPIX, pl = (q >> 1) / IPIX;
            stage_store<F32, F16>(ireg[r], q < ipieces ? il + pl * C::IPLANE + pix * 32 + half * 16 : dummy);
        }
    };

    if (split < ntiles) prefetch(split);
    for (int tile = split; tile < ntiles; tile += nsplit) {
        __syncthreads();  // previous tile's LDS reads are done
        commit();
        __syncthreads();
        if (tile + nsplit < ntiles) prefetch(tile + nsplit);  // global loads fly under the MFMAs below
        if (!active) continue;
#pragma unroll 2
        for (int r = 0; r < C::PH; ++r) {
            bf16x8 a;
            if constexpr (USE_TR) {
                const int o0 = fplane * C::GPLANE + (r * C::PW + 8 * khalf + (li >> 2)) * 32 + (li & 3) * 8;
                a = frag_tr(gl, o0, o0 + 4 * 32);
            } else {
                const char* b0 = gl + fplane * C::GPLANE + (r * C::PW + 8 * khalf) * 32 + li * 2;
#pragma unroll
                for (int j = 0; j < 8; ++j) a[j] = *(const bf16_t*)(b0 + j * 32);
            }
            if constexpr (!F32) {
                if (P.want_bias && tg == 0 && ct == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) bsum += (float)a[j];
                }
            }
#pragma unroll
            for (int t = 0; t < C::TPG; ++t) {
                const int tl = tg * C::TPG + t;
                const int tap = P.tap0 + tl;
                if (tl < C::TAPS_PER_PART && tap < C::NTAPS) {  // uniform per wave
                    const int ky = tap / KH, kx = tap - ky * KH;
                    bf16x8 b;
                    const int prow = (r * STRIDE + ky) * C::IW + kx;
                    if constexpr (USE_TR) {
                        const int o0 = (ct * 2 + fplane) * C::IPLANE + (prow + (8 * khalf + (li >> 2)) * STRIDE) * 32 + (li & 3) * 8;
                        b = frag_tr(il, o0, o0 + 4 * STRIDE * 32);
                    } else {
                        const char* b0 = il + (ct * 2 + fplane) * C::IPLANE + (prow + 8 * khalf * STRIDE) * 32 + li * 2;
#pragma unroll
                        for (int j = 0; j < 8; ++j) b[j] = *(const bf16_t*)(b0 + j * STRIDE * 32);
                    }
                    acc[t] = mfma16<F16>(a, b, acc[t]);
                }
            }
        }
    }

    // ---- write partials: ws[part][split][tap][oc 32][cin 64] ----
    if (active) {
        float* w = ws + P.ws_off + (size_t)split * C::TAPS_PER_PART * 32 * 64;
        const int cin = ct * 32 + (lane & 31), h = lane >> 5;
#pragma unroll
        for (int t = 0; t < C::TPG; ++t) {
            const int tl = tg * C::TPG + t;
            if (tl < C::TAPS_PER_PART && P.tap0 + tl < C::NTAPS) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int oc = (j & 3) + 8 * (j >> 2) + 4 * h;
                    w[((size_t)tl * 32 + oc) * 64 + cin] = acc[t][j];
                }
            }
        }
        if constexpr (!F32) {
            if (P.want_bias && tg == 0 && ct == 0) {
                const float tot = bsum + __shfl_xor(bsum, 32, 64);
                if (lane < 32) ws[P.ws_bias_off + (size_t)split * 32 + lane] = tot;
            }
        }
    }
    if constexpr (F32) {
        if (P.want_bias) {  // uniform: deterministic fixed-order reduction of the per-thread fp32 partials through LDS
            __syncthreads();
            float* red = (float*)smem;  // [256][GR*8]
#pragma unroll
            for (int r = 0; r < GR; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) red[tid * (GR * 8) + r * 8 + j] = (tid + r * 256 < GPIECES) ? bacc[r][j] : 0.f;
            __syncthreads();
            if (tid < 32) {
                const int pl = tid >> 4, half = (tid >> 3) & 1, j = tid & 7;
                float tot = 0.f;
                for (int t = 0; t < 256; ++t) {
#pragma unroll
                    for (int r = 0; r < GR; ++r) {
                        const int q = t + r * 256;
                        if (q < GPIECES && (q & 1) == half && (q >> 1) / GPIX == pl) tot += red[t * (GR * 8) + r * 8 + j];
                    }
                }
                ws[P.ws_bias_off + (size_t)split * 32 + tid] = tot;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad v3 (3x3, stride 1): one part = one 64-channel INPUT block x up to three 32-oc tiles of the gradient slab x all 9 taps.
// Compared with the 4-wave kernel above this halves the bytes staged per MFMA (the input block is shared by three oc tiles instead of
// one): the dense-block wgrad is bound by L2/HBM traffic, not by MFMA issue.
// workspace per part: [split][tap][ot 3][oc 32][cin 64]; bias: [split][96]
// ---------------------------------------------------------------------------------------------------------------
// workgroup -> (part, pixel split).  nsplit_flags: bits 0-15 nsplit, bits 16-23 ppu.
// ppu = 0: block = part * nsplit + split; with nsplit a multiple of 8 every part's workgroup of one pixel split runs on XCD split % 8
// (workgroup b -> XCD b % 8) and the G / X tiles the parts share are fetched into ONE L2.
// ppu > 0 (grouped launches of many RDBs with few splits, nsplit not a multiple of 8): the parts come in units of ppu consecutive parts that
// read the same slab pair (one RDB); unit u = (rdb, split) is placed on XCD u % 8 as a whole: block b -> xcd = b % 8, slot = b / 8,
// unit = (slot / ppu) * 8 + xcd, part = rdb * ppu + slot % ppu.  The host only sets ppu when (nparts / ppu) * nsplit is a multiple of 8.
__device__ __forceinline__ void w3_block_map(int nsplit_flags, int& part_id, int& split) {
    const int nsplit = nsplit_flags & 0xffff, ppu = (nsplit_flags >> 16) & 0xff;
    const int b = blockIdx.x;
    if (ppu == 0) {
        part_id = b / nsplit;
        split = b - part_id * nsplit;
    } else {
        const int xcd = b & 7, slot = b >> 3;
        const int su = slot / ppu, pin = slot - su * ppu;
        const int unit = su * 8 + xcd;
        const int rdb = unit / nsplit;
        split = unit - rdb * nsplit;
        part_id = rdb * ppu + pin;
    }
}

// One LDS-DMA instruction (64 lanes x 16 bytes -> 1 KiB of LDS at `lds_addr`, lane l at +16 l) issued through inline assembly.
// Why not __builtin_amdgcn_raw_ptr_buffer_load_lds here: hipcc (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of every ds_read_b64_tr_b16 that
// follows a pending LDS-DMA in program order (the transpose-read intrinsic carries no memory operand, so the waitcnt pass must assume it reads
// what the DMA writes) -- with the DMA of the NEXT tile issued between the fragment reads of the current one, every k-step then waited for a full
// global round trip (3.4 ms per launch instead of 2.2 in the first build that did).  Issued from assembly WITHOUT a "memory" clobber (with one, the waitcnt
// pass treats the statement itself as a pending vector-memory access and waits just the same) the compiler does not see the DMA at all; its
// completion is awaited by the explicit `s_waitcnt vmcnt(0)` + barrier that ends every tile, which volatile asm cannot cross.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned lds_addr, unsigned voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc) : "m0");
}

// the LDS image of one pixel tile: 48 one-KiB DMA instructions (6 G planes x 4, 4 X planes x 6); each lane's source address is tile origin + a
// per-lane constant
struct W3G {
    static constexpr int PH = 8, PW = 16, IH = 10, IW = 18, GPIX = PH * PW, IPIX = IH * IW;
    static constexpr int GPLANE = GPIX * 32 + 128;           // 4 DMA instructions per plane
    static constexpr int IPLANE = 6 * 1024 + 128;            // 6 DMA instructions per plane (180 pixels = 5.6 KiB), = 128 (mod 256)
    static constexpr int G_BYTES = 6 * GPLANE, I_BYTES = 4 * IPLANE;
    static constexpr int BUF_BYTES = G_BYTES + I_BYTES;
};

struct W3GTile {
    __amdgpu_buffer_rsrc_t gb, ib;
    int oy0, ox0;
};

__device__ __forceinline__ W3GTile w3g_tile(const dasr_wgrad_part& P, int tile, int tiles_x, int tiles_y) {
    W3GTile T;
    int t2 = tile;
    const int tx = t2 % tiles_x;
    t2 /= tiles_x;
    const int ty = t2 % tiles_y;
    const int n = t2 / tiles_y;
    T.oy0 = ty * W3G::PH;
    T.ox0 = tx * W3G::PW;
    T.gb = make_rsrc((const bf16_t*)P.g.p + (size_t)n * P.g.n_stride);
    T.ib = make_rsrc((const bf16_t*)P.in.p + (size_t)n * P.in.n_stride);
    return T;
}

// ---------------------------------------------------------------------------------------------------------------
// wgrad3 with LOADER WAVES (round 3): 12 compute waves (oc tile x cin tile x tap half, 5 accumulators, transposed LDS reads, an LDS image filled
// by LDS-DMA) plus FOUR waves, one per SIMD, that do nothing but issue the 48 DMA
// instructions of the next pixel tile and wait for them.  The round-3 ablations (profiles/r03_wgrad_ablation.txt) showed that the weight gradient
// pays the SUM of its MFMA time and of its L2 -> LDS transfer time: a wave that issues a load into a busy memory pipe stalls, and its MFMAs with
// it.  Here the compute waves never touch vector memory inside the tile loop; the loaders stall instead, and a stalled loader costs no MFMA slot.
// 16 waves x 128 registers: the compute side fits because nothing is staged through registers.
// (The 4-wave register-window kernel and the 12-wave forms that stage from the compute waves measured slower: profiles/r03_wgrad_ablation.txt.)
// ---------------------------------------------------------------------------------------------------------------
struct W3L {
    static constexpr int NT = 1024, NLD = 4, NDMA = 12;   // 12 compute waves + 4 loaders; 48 DMA instructions per tile, 12 per loader
    static constexpr int NBUF = 3;                        // ring of three tile images (151 KB): the loaders run one tile ahead of the wait
    static constexpr int LDS_BYTES = NBUF * W3G::BUF_BYTES;
};

// The k-steps of one pixel tile for one compute wave, REGISTER-WINDOW form (round 6).  The 12-wave decomposition of round 3 read 6 fragments per
// k-step (5 X + 1 G) for 5 (th = 0) or 4 (th = 1) MFMAs: 576 KB of transposed LDS reads per tile and CU + 47 KB of LDS-DMA writes = 4 870 cycles of the
// LDS port (128 B / clk) against 3 840 cycles of MFMA -- the kernel sat at 71 % MFMA busy because the LDS port, not the matrix pipe, bounded it
// (profiles/r03_wgrad_ablation.txt: MFMA + fragment reads alone 1 686 us against 1 275 us MFMA-bound; profiles/r06f_pmc_mfma_busy.txt).
// Here a wave owns taps that share a COLUMN of the 3 x 3 stencil, so that the X fragment of halo row r + dy is the same registers for every (r, dy)
// with the same sum: th = 0: (dy 0..2, dx 0) + (dy 0..1, dx 1); th = 1: (dy 0..2, dx 2) + (2, 1).  Per k-step: ONE new fragment per column + the G
// fragment = 3 reads for 5 / 4 MFMAs (312 KB per tile and CU).  A fragment is reloaded IN PLACE right behind the last MFMA that reads it (dy = 0) and is
// next needed as dy = 2 (dy = 1 for the two-row column) of the following k-step: 28 fragment registers instead of 36.
struct W3Win {
    bf16x8 xa[3], xb[2], g[2];   // column A: halo rows r, r + 1, r + 2 (ring of three); column B: two rows (th 0) / one row, double-buffered (th 1); G row r, r + 1
};
template <int TH>
__device__ __forceinline__ bf16x8 w3_win_x(const char* buf, int ibase, int R, int dx) {
    const int o = ibase + (R * W3G::IW + dx) * 32;
    return frag_tr(buf, o, o + 4 * 32);
}
__device__ __forceinline__ bf16x8 w3_win_g(const char* buf, int gbase, int r) {
    const int o = gbase + r * W3G::PW * 32;
    return frag_tr(buf, o, o + 4 * 32);
}
// the fragments k-step 0 of a tile starts from (the first tile of a workgroup; later tiles get them in place during the previous tile's last k-step)
template <int TH>
__device__ __forceinline__ void w3_win_prologue(const char* buf, int gbase, int ibase, W3Win& w) {
    constexpr int DXA = TH ? 2 : 0;
    w.g[0] = w3_win_g(buf, gbase, 0);
    w.xa[0] = w3_win_x<TH>(buf, ibase, 0, DXA);
    w.xb[0] = w3_win_x<TH>(buf, ibase, TH ? 2 : 0, 1);
    w.xa[1] = w3_win_x<TH>(buf, ibase, 1, DXA);
    if constexpr (TH == 0) w.xb[1] = w3_win_x<TH>(buf, ibase, 1, 1);
    w.xa[2] = w3_win_x<TH>(buf, ibase, 2, DXA);
}
// k-steps 0 .. 6 of a tile
template <bool F16, int TH>
__device__ __forceinline__ void w3_win_steps(const char* buf, int gbase, int ibase, W3Win& w, f32x16 (&acc)[5], float& bsum, bool want_bias) {
    constexpr int DXA = TH ? 2 : 0;
#pragma unroll
    for (int r = 0; r < W3G::PH - 1; ++r) {
        w.g[(r + 1) & 1] = w3_win_g(buf, gbase, r + 1);
        if constexpr (TH == 1) w.xb[(r + 1) & 1] = w3_win_x<TH>(buf, ibase, r + 3, 1);
        __builtin_amdgcn_sched_barrier(0);
        acc[0] = mfma16<F16>(w.g[r & 1], w.xa[r % 3], acc[0]);                       // (0, DXA)
        __builtin_amdgcn_sched_barrier(0);
        w.xa[r % 3] = w3_win_x<TH>(buf, ibase, r + 3, DXA);        // -> (2, DXA) of k-step r + 1
        __builtin_amdgcn_sched_barrier(0);
        acc[3] = mfma16<F16>(w.g[r & 1], w.xb[r & 1], acc[3]);                       // th 0: (0, 1); th 1: (2, 1)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (TH == 0) {
            w.xb[r & 1] = w3_win_x<TH>(buf, ibase, r + 2, 1);                        // -> (1, 1) of k-step r + 1
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[1] = mfma16<F16>(w.g[r & 1], w.xa[(r + 1) % 3], acc[1]);                 // (1, DXA)
        if constexpr (TH == 0) {
            acc[4] = mfma16<F16>(w.g[r & 1], w.xb[(r + 1) & 1], acc[4]);             // (1, 1)
            if (want_bias) {
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum += frag_f32<F16>(w.g[r & 1], j);
            }
        }
        acc[2] = mfma16<F16>(w.g[r & 1], w.xa[(r + 2) % 3], acc[2]);                 // (2, DXA)
        __builtin_amdgcn_sched_barrier(0);
    }
}
// k-step 7 of a tile: nothing is read from the tile's own image any more; every fragment register is re-filled IN PLACE, right behind its last MFMA, with
// what k-step 0 of the NEXT tile starts from (`nbuf`: landed -- the barrier in front of this k-step is the loaders' "tile t + 1 is in LDS"; behind the last tile
// of the workgroup the reads fetch a stale image and nobody uses them).  So a tile starts without a burst of prologue reads behind its barrier.
template <bool F16, int TH>
__device__ __forceinline__ void w3_win_last(const char* nbuf, int gbase, int ibase, W3Win& w, f32x16 (&acc)[5], float& bsum, bool want_bias) {
    constexpr int DXA = TH ? 2 : 0, r = W3G::PH - 1;
    static_assert(r == 7, "ring indices below are those of k-step 7");
    w.g[0] = w3_win_g(nbuf, gbase, 0);
    if constexpr (TH == 1) w.xb[0] = w3_win_x<TH>(nbuf, ibase, 2, 1);
    __builtin_amdgcn_sched_barrier(0);
    acc[2] = mfma16<F16>(w.g[1], w.xa[0], acc[2]);                                   // (2, DXA): halo row 9
    __builtin_amdgcn_sched_barrier(0);
    w.xa[0] = w3_win_x<TH>(nbuf, ibase, 0, DXA);
    __builtin_amdgcn_sched_barrier(0);
    acc[0] = mfma16<F16>(w.g[1], w.xa[1], acc[0]);                                   // (0, DXA): halo row 7
    __builtin_amdgcn_sched_barrier(0);
    w.xa[1] = w3_win_x<TH>(nbuf, ibase, 1, DXA);
    __builtin_amdgcn_sched_barrier(0);
    acc[1] = mfma16<F16>(w.g[1], w.xa[2], acc[1]);                                   // (1, DXA): halo row 8
    __builtin_amdgcn_sched_barrier(0);
    w.xa[2] = w3_win_x<TH>(nbuf, ibase, 2, DXA);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (TH == 0) {
        acc[4] = mfma16<F16>(w.g[1], w.xb[0], acc[4]);                               // (1, 1): halo row 8
        __builtin_amdgcn_sched_barrier(0);
        w.xb[0] = w3_win_x<TH>(nbuf, ibase, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (want_bias) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bsum += frag_f32<F16>(w.g[1], j);
        }
        acc[3] = mfma16<F16>(w.g[1], w.xb[1], acc[3]);                               // (0, 1): halo row 7
        __builtin_amdgcn_sched_barrier(0);
        w.xb[1] = w3_win_x<TH>(nbuf, ibase, 1, 1);
    } else {
        acc[3] = mfma16<F16>(w.g[1], w.xb[1], acc[3]);                               // (2, 1): halo row 9
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <bool F16>
__device__ __forceinline__ void wgrad3_ld_body(const dasr_wgrad_part* __restrict__ parts, int nparts, int nsplit_flags, float* __restrict__ ws) {
    using C = W3G;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nsplit = nsplit_flags & 0xffff;
    int part_id, split;
    w3_block_map(nsplit_flags, part_id, split);
    const dasr_wgrad_part P = parts[part_id];
    const int tiles_x = (P.Wout + C::PW - 1) / C::PW, tiles_y = (P.Hout + C::PH - 1) / C::PH;
    const int ntiles = tiles_x * tiles_y * P.N;
    const unsigned lds0 = (unsigned)(size_t)(DASR_LDS char*)smem;
    if (wave >= 12) {
        // ---- loader wave lw: quarter lw (32 pixels) of each of the 6 G planes, and the 6 sixths of X plane lw
        const int lw = wave - 12;
        const int HL = P.ups ? 2 * P.Hin : P.Hin, WL = P.ups ? 2 * P.Win : P.Win;
        const int half8 = (lane & 1) * 8;
        int pos_g, pos_x[6];
        {
            const int pix = (lw * 64 + lane) >> 1;
            pos_g = (pix >> 4) | ((pix & 15) << 16);
        }
        const bool x_plane_ok = (lw < P.in_planes) & (lw < 2 * P.n_ctiles);
#pragma unroll
        for (int sub = 0; sub < 6; ++sub) {
            const int pix = (sub * 64 + lane) >> 1, iy = pix / C::IW;
            pos_x[sub] = (((pix < C::IPIX) & x_plane_ok) ? iy : 0x7fff) | ((pix - iy * C::IW) << 16);
        }
        const int rel_x = lw * (int)P.in.cb_stride + half8;
        auto fill = [&](int tile, unsigned buf) {
            const W3GTile T = w3g_tile(P, tile, tiles_x, tiles_y);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int oy = T.oy0 + (pos_g & 0xffff), ox = T.ox0 + (pos_g >> 16);
                const bool ok = (oy < P.Hout) & (ox < P.Wout) & (k < P.g_planes);
                const unsigned off = ok ? (unsigned)((k * (int)P.g.cb_stride + half8 + (oy * P.Wout + ox) * 16) * 2) : OOB;
                lds_dma16(T.gb, buf + k * C::GPLANE + lw * 1024, off);
            }
#pragma unroll
            for (int sub = 0; sub < 6; ++sub) {
                const int gy = T.oy0 - P.pad + (pos_x[sub] & 0xffff), gx = T.ox0 - P.pad + (pos_x[sub] >> 16);
                const bool ok = (gy >= 0) & (gy < HL) & (gx >= 0) & (gx < WL);
                const int sy = P.ups ? gy >> 1 : gy, sx = P.ups ? gx >> 1 : gx;
                const unsigned off = ok ? (unsigned)((rel_x + (sy * P.Win + sx) * 16) * 2) : OOB;
                lds_dma16(T.ib, buf + C::G_BYTES + lw * C::IPLANE + sub * 1024, off);
            }
        };
        // ring of three: during tile t the loaders request tile t + 2 (into the slot tile t - 1 was read from) and wait only for tile t + 1,
        // requested a whole tile earlier: the barrier that ends a tile never waits for a load in flight
        if (split < ntiles) fill(split, lds0);
        if (split + nsplit < ntiles) {
            fill(split + nsplit, lds0 + C::BUF_BYTES);
            asm volatile("s_waitcnt vmcnt(12)");
        } else {
            asm volatile("s_waitcnt vmcnt(0)");
        }
        __syncthreads();
        int cur = 0;
        for (int tile = split; tile < ntiles; tile += nsplit) {
            const int slot2 = cur == 0 ? 2 : cur - 1;
            const bool more = tile + 2 * nsplit < ntiles;
            if (more) {
                fill(tile + 2 * nsplit, lds0 + slot2 * C::BUF_BYTES);
                asm volatile("s_waitcnt vmcnt(12)");   // tile t + 1 has landed (this loader's share), tile t + 2 may fly ...
            } else {
                asm volatile("s_waitcnt vmcnt(0)");
            }
            __syncthreads();                           // ... everybody's; and the compute waves are done with the current slot
            cur = cur == 2 ? 0 : cur + 1;
        }
        return;
    }
    // ---- compute wave: pair = wave % 6 -> (oc tile, cin tile); taps 0..4 (wave < 6) or 5..8
    const int pair = wave % 6, th = wave / 6;
    const int ot = pair >> 1, ct = pair & 1;
    const int n_ot = (P.g_planes + 1) >> 1;
    const bool active = ct < P.n_ctiles && ot < n_ot;
    f32x16 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
    float bsum = 0.f;
    const int gg = lane >> 4, li = lane & 15;
    const int fplane = gg & 1, khalf = gg >> 1;
    const int gbase = (ot * 2 + fplane) * C::GPLANE + (8 * khalf + (li >> 2)) * 32 + (li & 3) * 8;
    const int ibase = C::G_BYTES + (ct * 2 + fplane) * C::IPLANE + (8 * khalf + (li >> 2)) * 32 + (li & 3) * 8;
    const bool want_bias = P.want_bias && ct == 0 && th == 0;
    __syncthreads();   // tile 0 is in LDS
    int cur = 0;
    // ONE barrier per tile, in front of its LAST k-step: for the loaders it is "tile t + 1 has landed, and nobody requests anything from tile t's image
    // any more" (k-step 7 reads registers only; its in-place reloads go to tile t + 1's image).  One loop per tap set: the wave-uniform choice is made
    // once; every wave, active or not, meets the same barriers.
    auto run = [&](auto th_c) {
        constexpr int TH = decltype(th_c)::value;
        W3Win w;
        if (active) w3_win_prologue<TH>(smem, gbase, ibase, w);
        for (int tile = split; tile < ntiles; tile += nsplit) {
            const char* buf = smem + cur * C::BUF_BYTES;
            cur = cur == 2 ? 0 : cur + 1;
            if (active) w3_win_steps<F16, TH>(buf, gbase, ibase, w, acc, bsum, want_bias);
            __syncthreads();
            if (active) w3_win_last<F16, TH>(smem + cur * C::BUF_BYTES, gbase, ibase, w, acc, bsum, want_bias);
        }
    };
    if (th == 0) run(std::integral_constant<int, 0>{});
    else run(std::integral_constant<int, 1>{});
    if (active) {
        float* w = ws + P.ws_off + (size_t)split * 9 * 3 * 2048 + (size_t)ot * 2048;
        const int cin = ct * 32 + (lane & 31), h = lane >> 5;
        const int na = th ? 4 : 5;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            if (t < na) {
                const int tap = th ? (t == 0 ? 2 : t == 1 ? 5 : t == 2 ? 8 : 7) : (t == 0 ? 0 : t == 1 ? 3 : t == 2 ? 6 : t == 3 ? 1 : 4);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int oc = (j & 3) + 8 * (j >> 2) + 4 * h;
                    w[(size_t)tap * 3 * 2048 + oc * 64 + cin] = acc[t][j];
                }
            }
        }
        if (want_bias) {
            const float tot = bsum + __shfl_xor(bsum, 32, 64);
            if (lane < 32) ws[P.ws_bias_off + (size_t)split * 96 + ot * 32 + lane] = tot;
        }
    }
}

template <bool F16>
__global__ __launch_bounds__(1024, 1) void wgrad3_ld_kernel(const dasr_wgrad_part* __restrict__ parts, int nparts, int nsplit_flags, float* __restrict__ ws) {
    wgrad3_ld_body<F16>(parts, nparts, nsplit_flags, ws);
}
// deterministic split reduction.  One workgroup = one output channel x 16 input channels of one part; thread (split lane sl = t >> 4, cin =
// t & 15) sums splits sl, sl + 16, ... of every tap (two accumulators, fixed order), the 16 lane sums meet in LDS and are added in a fixed
// tree, and the reference layout [cout][cin][kh][kw] is written as ONE contiguous run of 16 * ntaps floats per workgroup (the first version
// stored 4 bytes per lane 36 bytes apart: 8x write amplification, ~1 TB/s, 8 % of the DSN iteration).  128 workgroups per part: enough
// parallelism both for the many-parts / 16-splits launches of the RRDB trunk and the 2-parts / 128-splits launches of the DSN generator.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const dasr_wgrad_reduce_part* __restrict__ parts, int nparts,
                                                           const float* __restrict__ ws, float* __restrict__ grad, float scale) {
    __shared__ float red[16 * 16 * 17];
    const dasr_wgrad_reduce_part P = parts[blockIdx.y];
    // gridDim.x == 32 (the launcher's `few_splits`): every part takes the few-splits path below, which needs ONE workgroup per output channel -- the three
    // of four workgroups that only returned cost more than the work (7680 workgroups per launch of the grouped trunk gradients: 55 us for 18 MB, dispatch-bound)
    const bool per_oc = gridDim.x == 32;
    const int oc = per_oc ? blockIdx.x : blockIdx.x >> 2, cg = per_oc ? 0 : blockIdx.x & 3, goc = P.oc0 + oc;
    if (goc >= P.cout) return;   // uniform per block
    const int per = P.ntaps * 32 * 64;
    const long long sstride = P.split_stride > 0 ? P.split_stride : per, tstride = P.tap_stride > 0 ? P.tap_stride : 2048;
    const long long bstride = P.bias_stride > 0 ? P.bias_stride : 32;
    const int NT = P.ntaps_total > 0 ? P.ntaps_total : P.ntaps;
    const int ntaps = min(P.ntaps, NT - P.tap0);                        // taps of this part that exist in the kernel window
    const int n_c = min(min(32 * P.n_ctiles, P.cin - P.c0), 64) - cg * 16;   // valid input channels of this 16-channel group (may be <= 0)
    const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    if (P.nsplit <= 4 && ntaps <= 16) {
        // few splits (the grouped dense-block launches of the RRDB trunk: 60 parts x 4 pixel splits): the 16 split lanes would be three quarters
        // idle and a workgroup would move 2.3 KB.  Instead ONE workgroup per output channel covers all four 16-channel groups: lane group
        // sl = 4 * (channel group) + split, nine independent loads per thread, one contiguous run of 64 * ntaps floats out.  Same summation
        // order as the general path ((s0 + s1) + (s2 + s3)): bit-identical results.
        if (cg != 0) return;   // (uniform per block)
        const int n_all = min(min(32 * P.n_ctiles, P.cin - P.c0), 64);
        const int cgi = sl >> 2, sp = sl & 3, c = cgi * 16 + cl;
        if (c < n_all && sp < P.nsplit) {
            const float* src = ws + P.ws_off + (size_t)sp * sstride + oc * 64 + c;
            float q[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) q[t] = t < ntaps ? src[(long long)t * tstride] : 0.f;
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (t < ntaps) red[(sl * 16 + cl) * 17 + t] = q[t];
        } else if (c < n_all) {
            for (int t = 0; t < ntaps; ++t) red[(sl * 16 + cl) * 17 + t] = 0.f;
        }
        __syncthreads();
        float* dst = grad + P.dst_w_off + ((long long)goc * P.cin + P.c0) * NT + P.tap0;
        const int nvalid = n_all * ntaps;
        for (int o = threadIdx.x; o < nvalid; o += 256) {
            const int cc = o / ntaps, tap = o - cc * ntaps;
            const float* r = red + (((cc >> 4) * 4) * 16 + (cc & 15)) * 17 + tap;
            const float tot = (r[0] + r[16 * 17]) + (r[2 * 16 * 17] + r[3 * 16 * 17]);
            dst[ntaps == NT ? (long long)o : (long long)cc * NT + tap] = tot * scale;
        }
        if (P.dst_b_off >= 0 && threadIdx.x < 64) {
            float b = threadIdx.x < (P.bias_nsplit > 0 ? P.bias_nsplit : P.nsplit) ? ws[P.ws_bias_off + (size_t)threadIdx.x * bstride + oc] : 0.f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
            if (threadIdx.x == 0) grad[P.dst_b_off + goc] = b * scale;
        }
        return;
    }
    if (n_c > 0) {
        const float* src = ws + P.ws_off + oc * 64 + cg * 16 + cl;
        for (int tap0 = 0; tap0 < ntaps; tap0 += 3) {      // three taps x eight splits = 24 independent loads in flight per thread: the
            float a[3] = {0.f, 0.f, 0.f};                    // few-parts / many-splits launches (DSN: 2 parts x 128 splits) are latency-bound
            if (cl < n_c) {
                for (int sp = sl; sp < P.nsplit; sp += 16 * 8) {
                    float q[3][8];
#pragma unroll
                    for (int t = 0; t < 3; ++t)
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            q[t][k] = (tap0 + t < ntaps && sp + 16 * k < P.nsplit) ? src[(size_t)(sp + 16 * k) * sstride + (long long)(tap0 + t) * tstride] : 0.f;
#pragma unroll
                    for (int t = 0; t < 3; ++t)
#pragma unroll
                        for (int k = 0; k < 8; ++k) a[t] += q[t][k];   // ascending split order, whatever the unrolling
                }
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (tap0 + t < ntaps) red[(sl * 16 + cl) * 17 + tap0 + t] = a[t];
        }
    }
    __syncthreads();
    if (n_c > 0) {
        float* dst = grad + P.dst_w_off + ((long long)goc * P.cin + P.c0 + cg * 16) * NT + P.tap0;
        const int nvalid = (n_c < 16 ? n_c : 16) * ntaps;
        for (int o = threadIdx.x; o < nvalid; o += 256) {
            const int c = o / ntaps, tap = o - c * ntaps;
            const float* r = red + c * 17 + tap;
            float q[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) q[k] = r[k * 16 * 17];
            const float tot = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) +
                              (((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15])));
            // the whole kernel window: [cin][tap] is contiguous in the destination; a tap range of a larger window (5x5 in parts of 10 taps): runs
            dst[ntaps == NT ? (long long)o : (long long)c * NT + tap] = tot * scale;
        }
    }
    if (cg == 0 && P.dst_b_off >= 0 && threadIdx.x < 64) {   // bias of this output channel: lane l sums splits l, l + 64, ...; fixed xor tree
        float b = 0.f;
        const int nb_ = P.bias_nsplit > 0 ? P.bias_nsplit : P.nsplit;
        for (int sp = threadIdx.x; sp < nb_; sp += 64) b += ws[P.ws_bias_off + (size_t)sp * bstride + oc];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
        if (threadIdx.x == 0) grad[P.dst_b_off + goc] = b * scale;
    }
}

__global__ void probe_tr16_kernel(int* result) {
    __shared__ __attribute__((aligned(16))) short lds[4 * 64];
    const int l = threadIdx.x;
    // 4 groups, each a 4 x 16 row-major matrix M[row][col] = 1000*group + 16*row + col
    for (int i = l; i < 256; i += 64) lds[i] = (short)(1000 * (i >> 6) + (i & 63));
    __syncthreads();
    const int gg = l >> 4, li = l & 15;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DASR_LDS s16x4*)((char*)lds + gg * 128 + (li >> 2) * 32 + (li & 3) * 8));
    int ok = 1;
    for (int j = 0; j < 4; ++j) ok &= (v[j] == (short)(1000 * gg + 16 * j + li));
    const unsigned long long m = __ballot(ok);
    if (l == 0) *result = (m == ~0ull) ? 1 : 0;
}

template <int KH, int STRIDE, bool USE_TR, bool F32, bool F16 = false>
int launch_wgrad(const dasr_wgrad_part* parts, int nparts, int nsplit, float* ws, hipStream_t s) {
    using C = WCfg<KH, STRIDE>;
    auto kfn = wgrad_kernel<KH, STRIDE, USE_TR, F32, F16>;
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES + 16));
        attr_set = true;
    }
    DASR_LAUNCH_TAG(__PRETTY_FUNCTION__, kfn, dim3(nparts * nsplit), dim3(256), C::LDS_BYTES + 16, s, parts, nparts, nsplit, ws);
    return (int)hipGetLastError();
}

template <bool F16>
int launch_wgrad3_ld(const dasr_wgrad_part* parts, int nparts, int nsplit, float* ws, hipStream_t s) {
    auto kfn = wgrad3_ld_kernel<F16>;
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, W3L::LDS_BYTES));
        attr_set = true;
    }
    DASR_LAUNCH_TAG(__PRETTY_FUNCTION__, kfn, dim3(nparts * (nsplit & 0xffff)), dim3(W3L::NT), W3L::LDS_BYTES, s, parts, nparts, nsplit, ws);
    return (int)hipGetLastError();
}

int g_use_tr = -1;  // -1 unknown, 0 gather fallback, 1 transpose reads

}  // namespace

extern "C" int dasr_probe_tr16(void* stream) {
    int* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(int)));
    DASR_LAUNCH(probe_tr16_kernel, dim3(1), dim3(64), 0, as_stream(stream), d);
    int h = -1;
    hipError_t e = hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(d);
    if (e != hipSuccess) return -(int)e;
    g_use_tr = h;
    return h;
}

extern "C" int dasr_wgrad_set_mode(int use_tr) {
    if (use_tr & ~1) return DASR_EINVAL;   // bit 0 only: transpose reads on / off
    g_use_tr = use_tr & 1;
    return 0;
}

namespace {
template <int KH, int STRIDE>
int dispatch_wgrad(const dasr_wgrad_part* parts, int nparts, int nsplit, bool tr, int f32, float* ws, hipStream_t s) {
    if (f32 & 2) {   // f32 tensors rounded to f16 (pre-scaled gradient), f16 MFMA
        if (tr) return launch_wgrad<KH, STRIDE, true, true, true>(parts, nparts, nsplit, ws, s);
        return launch_wgrad<KH, STRIDE, false, true, true>(parts, nparts, nsplit, ws, s);
    }
    if (tr) return f32 ? launch_wgrad<KH, STRIDE, true, true>(parts, nparts, nsplit, ws, s) : launch_wgrad<KH, STRIDE, true, false>(parts, nparts, nsplit, ws, s);
    return f32 ? launch_wgrad<KH, STRIDE, false, true>(parts, nparts, nsplit, ws, s) : launch_wgrad<KH, STRIDE, false, false>(parts, nparts, nsplit, ws, s);
}
}  // namespace

extern "C" int dasr_wgrad(const dasr_wgrad_part* parts_dev, int32_t nparts, int32_t nsplit, int32_t kh, int32_t stride, int32_t f32,
                          float* ws, void* stream) {
    hipStream_t s = as_stream(stream);
    if (nparts <= 0 || nsplit <= 0) return DASR_EINVAL;
    if (kh != 33 && (nsplit >> 16)) return DASR_EINVAL;   // the unit placement bits exist for the 12-wave 3x3 kernel only
    if (kh == 33) {
        const int ns = nsplit & 0xffff, ppu = (nsplit >> 16) & 0xff;
        if (ns <= 0 || (nsplit >> 24) || (ppu && ((nparts % ppu) || (((long long)(nparts / ppu) * ns) & 7)))) return DASR_EINVAL;
    }
    if (g_use_tr < 0) return DASR_EINVAL;  // dasr_probe_tr16 must run once per process (outside graph capture)
    const bool tr = g_use_tr == 1;
    if (kh == 33) {  // 3x3 stride 1 on 16-bit tensors: one part = 64 input channels x up to three 32-oc tiles; wgrad3_ld_kernel (12 compute + 4 loader waves)
        if (!tr || f32 == 1) return DASR_EINVAL;   // gfx950 has ds_read_b64_tr_b16 (dasr_probe_tr16 confirms it); the grouped 3x3 form exists for 16-bit tensors only
        return f32 == 2 ? launch_wgrad3_ld<true>(parts_dev, nparts, nsplit, ws, s) : launch_wgrad3_ld<false>(parts_dev, nparts, nsplit, ws, s);
    }
    if (kh == 3 && stride == 1) return dispatch_wgrad<3, 1>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    if (kh == 4 && stride == 1) return dispatch_wgrad<4, 1>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    if (kh == 4 && stride == 2) return dispatch_wgrad<4, 2>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    if (kh == 5 && stride == 1) return dispatch_wgrad<5, 1>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    if (kh == 1 && stride == 1) return dispatch_wgrad<1, 1>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    if (kh == 3 && stride == 2) return dispatch_wgrad<3, 2>(parts_dev, nparts, nsplit, tr, f32, ws, s);
    return DASR_EINVAL;
}

extern "C" int dasr_wgrad_reduce(const dasr_wgrad_reduce_part* parts_dev, int32_t nparts, const float* ws, float* grad_flat,
                                 float scale, int32_t few_splits, void* stream) {
    if (nparts <= 0) return DASR_EINVAL;
    DASR_LAUNCH(wgrad_reduce_kernel, dim3(few_splits ? 32 : 128, nparts), dim3(256), 0, as_stream(stream), parts_dev, nparts, ws, grad_flat, scale);
    return (int)hipGetLastError();
}

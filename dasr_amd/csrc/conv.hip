// Implicit-GEMM convolution (forward / data-gradient) for gfx950.
//
// GEMM view: D[oc][pixel] = sum_{tap, c} W[oc][tap][c] * X[pixel + tap][c]
//   A operand = packed weights (32 oc x 16 c per MFMA), B operand = activations (16 c x 32 pixels),
//   v_mfma_f32_32x32x16_bf16, fp32 accumulate.  The output fragment then holds, per lane, one pixel
//   and 4x4 consecutive output channels -> vector stores into the NC16HW16 layout.
// Workgroup = 4 waves; spatial tile TH x TW output pixels; each wave owns NT n-tiles (32 pixels each)
// and MT m-tiles (32 output channels each).  Input channels are consumed in chunks of 16 (one MFMA
// k-step per tap): the (TH-1)*S+KH by (TW-1)*S+KH input halo tile of the chunk and the chunk's
// weights are staged in LDS (im2col-free: the taps are just shifted LDS reads with immediate offsets).
// prec 3 ("split bf16"): x = hi + lo with hi = bf16(x), lo = bf16(x - hi); hi*hi + hi*lo + lo*hi
// gives ~2^-17 relative operand error with three bf16 MFMAs (16x faster than the f32 MFMA).
#include "common.h"

namespace {

template <int PREC, bool IN_F32, int MT, int KH, int STRIDE, int NT_, int KS = 1>
struct Cfg {
    static constexpr int NT = NT_;
    static constexpr int RPT = STRIDE == 1 ? 1 : 2;    // output rows per n-tile
    static constexpr int CPT = STRIDE == 1 ? 32 : 16;  // output cols per n-tile
    static constexpr int TH = 4 * NT * RPT;
    static constexpr int TW = CPT;
    static constexpr int IH = (TH - 1) * STRIDE + KH;
    static constexpr int IW = (TW - 1) * STRIDE + KH;
    static constexpr int NTAPS = KH * KH;
    static constexpr int PIXB = KS == 1 ? 48 : 80;  // 32*KS B of bf16 + 16 B pad: conflict-free ds_read_b128 (3 or 5 slots/pixel)
    static constexpr int ACT_BYTES = IH * IW * PIXB;
    static constexpr int W_BYTES = KS * NTAPS * MT * 1024;
    static constexpr int NARR = PREC >= 3 ? 2 : 1;
    static constexpr int LDS_BYTES = NARR * (ACT_BYTES + W_BYTES);
    // staging pieces (16 B of global memory each)
    static constexpr int PPP16 = IN_F32 ? 4 : 2;  // pieces per pixel per 16-channel plane
    static constexpr int PPP = PPP16 * KS;        // pieces per pixel
    static constexpr int NPIECE = IH * IW * PPP;
    static constexpr int AR = (NPIECE + 255) / 256;
    static constexpr int WPIECE = KS * NTAPS * MT * 64;
    static constexpr int WR = (WPIECE + 255) / 256;
};

// All global traffic goes through raw buffer loads/stores: an out-of-range offset (OOB) reads as zero / drops the
// store, so halo padding, partial tiles and padded channels need no divergent branches (exec-masked branches around
// loads make hipcc drain vmcnt and serialise the pipeline).
constexpr unsigned OOB = 0x80000000u;
constexpr int RSRC_FLAGS = 0x00020000;
constexpr int RSRC_RANGE = 0x7fffffff;

#ifdef DASR_TRACE
__device__ unsigned long long* g_trace = nullptr;  // [grid][16]: s_memrealtime at entry, then s_memtime stamps
#define TRACE_STAMP(k)                                                                         \
    do {                                                                                       \
        if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 16 + (k)] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define TRACE_STAMP(k) do {} while (0)
#endif

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, RSRC_RANGE, RSRC_FLAGS);
}

// ---------------------------------------------------------------------------------------------------
// Epilogue shared by the conv kernels: acc (MFMA D layout: lane -> pixel nn = lane & 31 of an n-tile row, channels
// 8g + 4*(lane >> 5) + j of the m-tile) -> bias / activation / mask / scaled residual adds -> fp32 and/or bf16 stores.
// ---------------------------------------------------------------------------------------------------
// mask planes of a workgroup's output tile fetched during the LAST chunk of the main loop (dgrad convs whose only epilogue input is the
// LeakyReLU' mask): no LDS-DMA is in flight then (nothing left to prefetch), so the loads neither queue behind nor delay a chunk, and the
// round trip (2-4 us under load, the whole difference between the dgrad and the forward launch) overlaps the last 36 MFMAs per wave.
template <int NG>
struct MaskPre {
    u32x4 v[NG][2];
};

template <int MT, int NT>
__device__ __forceinline__ void mask_prefetch(const dasr_conv_params& p, MaskPre<NT * MT>& m, int tid, int mg, int n, int oy0, int ox0) {
    const int lane = tid & 63, wave = tid >> 6, nn = lane & 31, kh2 = lane >> 5;
    const int ostr = p.out_stride > 1 ? p.out_stride : 1, owid = p.out_W > 0 ? p.out_W : p.Wout;
    const __amdgpu_buffer_rsrc_t rmask = make_rsrc((const char*)p.mask.p + (size_t)n * p.mask.n_stride * 2);
    const unsigned mask_cb = (unsigned)p.mask.cb_stride;
#pragma unroll
    for (int gi = 0; gi < NT * MT; ++gi) {
        const int nt = gi / MT, mi = gi - nt * MT;
        const int oy = oy0 + wave * NT + nt, ox = ox0 + nn;
        const unsigned oob = ((oy < p.Hout) & (ox < p.Wout)) ? 0u : OOB;   // arithmetic, not a branch: the loads stay unconditional
        const unsigned pixel = (unsigned)((oy * ostr + p.out_oy) * owid + ox * ostr + p.out_ox) * 16u;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const int oc = (mg * MT + mi) * 32 + 16 * pr;
            const unsigned mo = (((unsigned)(oc >> 4) * mask_cb + pixel + 8u * kh2) * 2u) | oob;
            m.v[gi][pr] = __builtin_amdgcn_raw_buffer_load_b128(rmask, mo, 0, 0);
        }
    }
}

// 16-byte epilogue store.  SC1 (compile time: the bf16 dense-block convs with Cout = 32, forward and data gradient): `sc1` = written through, the
// line leaves the XCD's L2.  With plain stores the 8-16 MB a launch writes stay dirty in the L2 until the end-of-kernel release writes them back
// (+ dirty bytes / 6 TB/s on every kernel boundary, MI355X_MICROARCH.md price list); measured in round 3 with a run-time switch, three A/B
// rounds on one box: plain 32.92-33.02 ms / step, sc1 32.28-32.50, `sc0 sc1` the same, `nt` flat; on the 64-channel conv5, the f16 HR tail and
// the f32-tensor convs sc1 measured flat or worse (DSN iteration +10 %), so they keep plain stores (profiles/r03_conv_ablation.txt section 5)
template <bool SC1>
__device__ __forceinline__ void st128(u32x4 v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    if constexpr (SC1) __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 16);
    else __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 0);
}

// F16OUT: -1 = the 16-bit output format is a run-time (wave-uniform) choice; 0 / 1 = bf16 / f16 fixed at compile time (the dense-block LDS-DMA
// kernels: the run-time form converted every element to BOTH formats and selected: 224 of the 628 VALU instructions of the Cout=32 epilogue)
// BIAS_STAGED: the caller has already put the m-group's bias into LDS at `smem` and synchronised (conv_chain_kernel V2: staged in front of the last chunk
// barrier of the main loop, in a region no DMA touches) -- no hand-over barrier here
// CONST_SLOPE: the caller guarantees p.slope_ptr == nullptr (the chained launches validate it): without it hipcc turns `slope_ptr ? *slope_ptr : slope` into an
// unconditional vector load from a selected address, and its `s_waitcnt vmcnt(0)` drains every LDS-DMA request in flight (rdb_is_kernel: the weights of the next three steps)
template <bool IN_F32, int MT, int NT, int STRIDE, int EPI, int F16OUT = -1, bool PRE = false, bool FSC1 = false, bool BIAS_STAGED = false, bool CONST_SLOPE = false,
          bool PACC = false>
__device__ __forceinline__ void conv_epilogue(const dasr_conv_params& p, f32x16 (&acc)[MT][NT], char* smem, float bias_reg, int tid, int mg, int n,
                                              int oy0, int ox0, const MaskPre<NT * MT>* pre = nullptr) {
    const int lane = tid & 63, wave = tid >> 6, nn = lane & 31, kh2 = lane >> 5;
    (void)lane;
    // ---- epilogue.  EPI != 0: the set of optional terms is a compile-time constant (the hot dense-block cases, chosen by
    // the host from the call's arguments), the code is straight-line; EPI == 0: every term is selected by a wave-uniform
    // branch on a kernel argument.  Only per-lane conditions (partial tiles) use out-of-range offsets.  The bias of the
    // m-group was fetched by the first 32*MT threads at kernel start and is handed round through LDS (free after the loop).
    constexpr bool G = EPI == 0;
    const bool has_bias = G ? p.bias != nullptr : bool(EPI & 1);
    const bool act_lrelu = G ? p.act == 1 : bool(EPI & 2);
    const bool act_sigmoid = G ? p.act == 2 : false;
    const bool has_mask = G ? p.mask.p != nullptr : bool(EPI & 4);
    const bool has_r1 = G ? p.res1.p != nullptr : bool(EPI & 8);
    const bool has_r2 = G ? p.res2.p != nullptr : bool(EPI & 16);
    const bool has_f32 = G ? p.out_f32.p != nullptr : bool(EPI & 32);
    const bool has_bf16 = G ? p.out_bf16.p != nullptr : bool(EPI & 64);
    const bool scaled = G ? true : bool(EPI & 128);   // alpha / gamma may differ from 1
    const bool f16out = F16OUT < 0 ? p.out16_f16 != 0 : F16OUT != 0;   // the 16-bit output tensor holds f16 (HR tail, f16 storage) instead of bf16: wave-uniform
    const bool chan_tail = G ? true : false;          // cout not a multiple of 32 (specialised variants require it)
    const int ostr = p.out_stride > 1 ? p.out_stride : 1, owid = p.out_W > 0 ? p.out_W : p.Wout;  // strided sub-grid output (stride-2 dgrad)
    constexpr int MSZ = IN_F32 ? 4 : 2;
    const float slope = (!CONST_SLOPE && p.slope_ptr) ? *p.slope_ptr : p.slope;  // PReLU: the (learned) slope lives in the parameter buffer (round 5: also in the specialised variants)
    // dL/dslope of nn.PReLU() (ONE shared slope; codes/DSN/model.py:29,215) from the data-gradient epilogue that already holds both operands (round 6): the conv result v in
    // front of the mask factor is dL/dh, the mask tensor is h = PReLU(z), and dL/da = sum_{h <= 0} dL/dh * z = sum v * h / a.  The 64-channel mask-only epilogue of the
    // LDS-DMA kernel (EPI 68, MT 2: the residual blocks of the DSN generator; a 16-bit mask in the format of the 16-bit output) accumulates slope * v * h per lane and
    // writes ONE partial per workgroup to p.prelu_part[blockIdx.x]; dasr_prelu_final sums them in a fixed order and divides by a^2 (the layout of dasr_prelu_grad's
    // partials, whose two passes over h and dL/dz this replaces).  PACC: the caller (conv_glds_kernel) instantiates the epilogue twice and takes this one when
    // p.prelu_part is set -- the HR-tail launches of the same kernel run the plain code.
    constexpr bool PACC_OK = PACC && EPI == 68 && MT == 2 && !IN_F32 && !FSC1 && !PRE;
    static_assert(!PACC || PACC_OK, "the slope-gradient partials exist for the 64-channel mask-only epilogue of the LDS-DMA kernel");
    constexpr bool pacc_on = PACC_OK;
    float pacc = 0.f;
    const __amdgpu_buffer_rsrc_t rmask = make_rsrc((const char*)p.mask.p + (size_t)n * p.mask.n_stride * MSZ);
    const __amdgpu_buffer_rsrc_t rr1 = make_rsrc((const char*)p.res1.p + (size_t)n * p.res1.n_stride * ((G && p.res1_lo) ? 2 : 4));
    const __amdgpu_buffer_rsrc_t rr2 = make_rsrc((const float*)p.res2.p + (size_t)n * p.res2.n_stride);
    const __amdgpu_buffer_rsrc_t rof = make_rsrc((float*)p.out_f32.p + (size_t)n * p.out_f32.n_stride);
    const __amdgpu_buffer_rsrc_t rob = make_rsrc((bf16_t*)p.out_bf16.p + (size_t)n * p.out_bf16.n_stride);
    const unsigned mask_cb = (unsigned)p.mask.cb_stride, r1_cb = (unsigned)p.res1.cb_stride, r2_cb = (unsigned)p.res2.cb_stride;
    const unsigned of_cb = (unsigned)p.out_f32.cb_stride, ob_cb = (unsigned)p.out_bf16.cb_stride;
    constexpr bool SC1 = FSC1 || (MT == 1 && !IN_F32 && F16OUT == 0);   // bf16 dense-block convs with Cout = 32 (st128); FSC1: every store of a chained layer (conv_chain_kernel)
    // split 16-bit output: the remainder goes lo_pl planes further (wave-uniform; 0 = plain).  The specialised bf16 epilogues (dense blocks) do not
    // carry the branch: classify_epi sends a bf16 split output to the generic epilogue
    const unsigned lo_pl = (G || F16OUT != 0) ? (unsigned)p.out16_lo : 0u;
    f32x4 bia[MT][4];
    if (has_bias) {
        float* bl = (float*)smem;
        if constexpr (!BIAS_STAGED) {
            if (tid < 32 * MT) bl[tid] = bias_reg;
            __syncthreads();
        }
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) bia[mi][g] = *(const f32x4*)(bl + mi * 32 + 8 * g + 4 * kh2);
    }
    TRACE_STAMP(5);
    // groups (nt, mi) of 32 pixels x 32 channels.  With a compile-time term set the optional-tensor loads of group g+1 are issued
    // before the arithmetic and stores of group g (two register sets), so only the first group's load latency is exposed;
    // the 64-channel kernel with two residuals has no registers left for that and loads just in time.
    constexpr int NG = NT * MT;
    // bf16 tensors of the specialised variants move 16 bytes per lane (v_permlane32_swap pairs the two half-waves' 4-channel groups):
    // half the VMEM instructions of the epilogue, each covering one contiguous KiB (the store tail is issue-bound, not bandwidth-bound)
    constexpr bool WIDE16 = !G && !IN_F32;
    // f32 tensors of the specialised variants: in the MFMA D layout one 16-byte access per lane touches HALF of 32 different 64-byte lines (a pixel's
    // 16-channel plane is one line; a lane holds 4 of its channels, its partner lane kh2 the next 4) -- the vector L1 moves whole lines, so the
    // fp32 residual loads / stores of conv5 ran at half its rate and the epilogue took 20 k cycles (18 % of the workgroup).  v_permlane16_swap
    // exchanges the 16-lane rows of the register sets g = 2 pr and 2 pr + 1: set A then holds all four channel quarters of pixels 0-15, set B of
    // pixels 16-31 -- every instruction covers 16 complete lines.
    constexpr bool WIDE32 = !G && STRIDE == 1;
    constexpr bool PIPE_EPI = !G && !(MT == 2 && (EPI & 16) && (EPI & 8)) && (EPI & (4 | 8 | 16));   // (the 64-channel kernel with BOTH residuals in the epilogue has no registers for it)
    u32x4 mk[2][4], r1v[2][4], r2v[2][4];
    auto group_addr = [&](int gi, unsigned (&eo)[4], unsigned (&cbv)[4]) {
        const int nt = gi / MT, mi = gi - nt * MT;
        int r, c;
        if constexpr (STRIDE == 1) {
            r = wave * NT + nt;
            c = nn;
        } else {
            r = (wave * NT + nt) * 2 + (nn >> 4);
            c = nn & 15;
        }
        const int oy = oy0 + r, ox = ox0 + c;
        const bool pv = (oy < p.Hout) & (ox < p.Wout);
        const unsigned pixel = (unsigned)((oy * ostr + p.out_oy) * owid + ox * ostr + p.out_ox) * 16u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int oc = (mg * MT + mi) * 32 + 8 * g + 4 * kh2;
            const bool cv = chan_tail ? (pv & (oc < ((p.cout + 15) & ~15))) : pv;
            cbv[g] = (unsigned)(oc >> 4);
            eo[g] = cv ? pixel + (unsigned)(oc & 15) : OOB;
        }
    };
    // WIDE32 addressing of group gi: element offset (within a plane) of this lane's 4 channels in register set A / B
    auto group_addr32 = [&](int gi, unsigned (&e32)[2]) {
        const int nt = gi / MT;
        const int oy = oy0 + wave * NT + nt;
        const unsigned q4 = 4u * (2u * (unsigned)(nn >> 4) + (unsigned)kh2);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int ox = ox0 + (nn & 15) + 16 * st;
            const bool pv = (oy < p.Hout) & (ox < p.Wout);
            e32[st] = pv ? (unsigned)((oy * ostr + p.out_oy) * owid + ox * ostr + p.out_ox) * 16u + q4 : OOB;
        }
    };
    auto issue_loads = [&](int gi, int slot) {
        unsigned eo[4], cbv[4];
        group_addr(gi, eo, cbv);
        unsigned e32[2];
        if constexpr (WIDE32) group_addr32(gi, e32);
        if (has_mask && !PRE) {
            if constexpr (WIDE16) {
                // one 16-byte load per lane and 16-channel plane: lanes 0-31 fetch channels 0-7, lanes 32-63 channels 8-15 of their pixel
                // (a fully contiguous KiB per instruction); the half-wave exchange back to the MFMA D layout happens after the wait
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const unsigned mo = eo[2 * pr] != OOB ? (cbv[2 * pr] * mask_cb + eo[2 * pr] + 4u * kh2) * 2u : OOB;
                    mk[slot][2 * pr] = __builtin_amdgcn_raw_buffer_load_b128(rmask, mo, 0, 0);
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned mo = eo[g] != OOB ? (cbv[g] * mask_cb + eo[g]) * MSZ : OOB;
                    if constexpr (IN_F32) {
                        mk[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rmask, mo, 0, 0);
                    } else {
                        const u32x2 t2 = __builtin_amdgcn_raw_buffer_load_b64(rmask, mo, 0, 0);
                        mk[slot][g] = u32x4{t2[0], t2[1], 0u, 0u};  // unpacked after the wait
                    }
                }
            }
        }
        if (G && has_r1 && p.res1_lo) {   // split 16-bit residual (hi planes + remainder planes, dasr_conv_params::res1_lo): two 8-byte loads per group
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x2 hi = __builtin_amdgcn_raw_buffer_load_b64(rr1, eo[g] != OOB ? (cbv[g] * r1_cb + eo[g]) * 2u : OOB, 0, 0);
                const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(rr1, eo[g] != OOB ? ((cbv[g] + (unsigned)p.res1_lo) * r1_cb + eo[g]) * 2u : OOB, 0, 0);
                r1v[slot][g] = u32x4{hi[0], hi[1], lo[0], lo[1]};
            }
        } else if (has_r1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if constexpr (WIDE32) r1v[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rr1, e32[g & 1] != OOB ? (cbv[g] * r1_cb + e32[g & 1]) * 4u : OOB, 0, 0);
                else r1v[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rr1, eo[g] != OOB ? (cbv[g] * r1_cb + eo[g]) * 4u : OOB, 0, 0);
            }
        }
        if (has_r2) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if constexpr (WIDE32) r2v[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rr2, e32[g & 1] != OOB ? (cbv[g] * r2_cb + e32[g & 1]) * 4u : OOB, 0, 0);
                else r2v[slot][g] = __builtin_amdgcn_raw_buffer_load_b128(rr2, eo[g] != OOB ? (cbv[g] * r2_cb + eo[g]) * 4u : OOB, 0, 0);
            }
        }
    };
    auto rows_swap = [&](u32x4& a, u32x4& b) {   // sets (2 pr, 2 pr + 1) <-> (A, B): an involution
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const auto r = __builtin_amdgcn_permlane16_swap(a[j], b[j], false, false);
            a[j] = r[0];
            b[j] = r[1];
        }
    };
    if constexpr (PIPE_EPI) issue_loads(0, 0);
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        const int nt = gi / MT, mi = gi - nt * MT;
        const int slot = PIPE_EPI ? (gi & 1) : 0;
        if constexpr (PIPE_EPI) {
            if (gi + 1 < NG) issue_loads(gi + 1, (gi + 1) & 1);
        } else {
            issue_loads(gi, 0);
        }
        {
            unsigned eo[4], cbv[4];
            group_addr(gi, eo, cbv);
            // arithmetic in passes: the VALU work of an absent term is skipped, not multiplied by a neutral coefficient
            // (64 outputs per lane: every op per element is 64 VALU instructions per wave; exp/rcp are quarter rate)
            float v[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[g][j] = acc[mi][nt][4 * g + j];
            if (has_bias) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] += bia[mi][g][j];
            }
            if (act_lrelu && !G && !CONST_SLOPE && p.slope_ptr) {   // specialised variants with a learned PReLU slope (any sign / size): select, three VALU ops per element
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] = v[g][j] > 0.f ? v[g][j] : slope * v[g][j];
            } else if (act_lrelu && !G) {   // specialised variants (classify_epi: slope in [0, 1]): LeakyReLU = max(v, slope * v), two VALU ops per element, not three
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] = fmaxf(v[g][j], slope * v[g][j]);
            } else if (act_lrelu) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] = fmaxf(v[g][j], 0.f) + slope * fminf(v[g][j], 0.f);
            } else if (act_sigmoid) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] = __frcp_rn(1.f + __expf(-v[g][j]));
            }
            if (has_mask) {
                if constexpr (WIDE16) {   // wide piece {w0 w1 | w2 w3} -> this lane's two 4-channel groups of the plane
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        u32x4 w = mk[slot][2 * pr];
                        if constexpr (PRE) w = pre->v[gi][pr];
                        const auto r0 = __builtin_amdgcn_permlane32_swap(w[0], w[2], false, false);
                        const auto r1 = __builtin_amdgcn_permlane32_swap(w[1], w[3], false, false);
                        mk[slot][2 * pr] = u32x4{r0[0], r1[0], 0u, 0u};
                        mk[slot][2 * pr + 1] = u32x4{r0[1], r1[1], 0u, 0u};
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (IN_F32) {
                            v[g][j] *= __uint_as_float(mk[slot][g][j]) > 0.f ? 1.f : slope;
                        } else {
                            // 16-bit mask (bf16 or f16 forward activation): positive <=> its bit pattern is a positive int16 (no unpacking to f32);
                            // select between v and slope * v (packed multiply): 2.5 VALU ops per element instead of 3.5
                            const unsigned wd = mk[slot][g][j >> 1];
                            const short hbits = (j & 1) ? (short)(wd >> 16) : (short)(wd & 0xffffu);
                            if constexpr (PACC_OK) {
                                if (pacc_on) {
                                    const unsigned short hb = (unsigned short)hbits;
                                    const float hv = f16out ? (float)__builtin_bit_cast(f16_t, hb) : (float)__builtin_bit_cast(bf16_t, hb);
                                    pacc += hbits > 0 ? 0.f : v[g][j] * hv;
                                }
                            }
                            v[g][j] = hbits > 0 ? v[g][j] : slope * v[g][j];
                        }
                    }
            }
            if (scaled && p.alpha != 1.f) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] *= p.alpha;
            }
            if (G && has_r1 && p.res1_lo) {   // value = hi + lo (f16 or bf16 pairs, the 16-bit format of the output tensor)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const u32x4 w = r1v[slot][g];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned short hb = (unsigned short)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
                        const unsigned short lb = (unsigned short)((j & 1) ? (w[2 + (j >> 1)] >> 16) : (w[2 + (j >> 1)] & 0xffffu));
                        const float r = f16out ? (float)__builtin_bit_cast(f16_t, hb) + (float)__builtin_bit_cast(f16_t, lb)
                                               : (float)__builtin_bit_cast(bf16_t, hb) + (float)__builtin_bit_cast(bf16_t, lb);
                        v[g][j] += p.beta1 * r;
                    }
                }
            } else if (has_r1) {
                if constexpr (WIDE32) {
                    rows_swap(r1v[slot][0], r1v[slot][1]);
                    rows_swap(r1v[slot][2], r1v[slot][3]);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] += p.beta1 * __uint_as_float(r1v[slot][g][j]);
            }
            if (has_r2) {
                if constexpr (WIDE32) {
                    rows_swap(r2v[slot][0], r2v[slot][1]);
                    rows_swap(r2v[slot][2], r2v[slot][3]);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[g][j] += p.beta2 * __uint_as_float(r2v[slot][g][j]);
            }
            if (chan_tail && (mg * MT + mi) * 32 + 32 > p.cout) {  // last, partial m-tile: padded channels of the last plane stay zero
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((mg * MT + mi) * 32 + 8 * g + 4 * kh2 + j >= p.cout) v[g][j] = 0.f;
            }
            if (has_f32 && WIDE32) {
                unsigned e32[2];
                group_addr32(gi, e32);
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    u32x4 oa = {__float_as_uint(v[2 * pr][0]), __float_as_uint(v[2 * pr][1]), __float_as_uint(v[2 * pr][2]), __float_as_uint(v[2 * pr][3])};
                    u32x4 ob = {__float_as_uint(v[2 * pr + 1][0]), __float_as_uint(v[2 * pr + 1][1]), __float_as_uint(v[2 * pr + 1][2]), __float_as_uint(v[2 * pr + 1][3])};
                    rows_swap(oa, ob);
                    st128<SC1>(oa, rof, e32[0] != OOB ? (cbv[2 * pr] * of_cb + e32[0]) * 4u : OOB);
                    st128<SC1>(ob, rof, e32[1] != OOB ? (cbv[2 * pr] * of_cb + e32[1]) * 4u : OOB);
                }
            } else if (has_f32) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const u32x4 o = {__float_as_uint(v[g][0]), __float_as_uint(v[g][1]), __float_as_uint(v[g][2]), __float_as_uint(v[g][3])};
                    st128<SC1>(o, rof, eo[g] != OOB ? (cbv[g] * of_cb + eo[g]) * 4u : OOB);
                }
            }
            if (has_bf16 && WIDE16) {
                const bool gm = scaled && p.gamma != 1.f;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    bf16x4 oa, ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float va = gm ? v[2 * pr][j] * p.gamma : v[2 * pr][j], vb = gm ? v[2 * pr + 1][j] * p.gamma : v[2 * pr + 1][j];
                        oa[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)va) : (bf16_t)va;
                        ob[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)vb) : (bf16_t)vb;
                    }
                    const u32x2 a = __builtin_bit_cast(u32x2, oa), b = __builtin_bit_cast(u32x2, ob);
                    const auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
                    const auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
                    const u32x4 o = {r0[0], r1[0], r0[1], r1[1]};   // lanes 0-31: channels 0-7 of the plane, lanes 32-63: channels 8-15
                    st128<SC1>(o, rob, eo[2 * pr] != OOB ? (cbv[2 * pr] * ob_cb + eo[2 * pr] + 4u * kh2) * 2u : OOB);
                    if (lo_pl) {   // remainder plane: lo = round16(value - hi)
                        bf16x4 la, lb;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float va = gm ? v[2 * pr][j] * p.gamma : v[2 * pr][j], vb = gm ? v[2 * pr + 1][j] * p.gamma : v[2 * pr + 1][j];
                            const float ha = f16out ? (float)(f16_t)va : (float)(bf16_t)va, hb = f16out ? (float)(f16_t)vb : (float)(bf16_t)vb;   // (re-rounded, not read back from the packed vector)
                            la[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)(va - ha)) : (bf16_t)(va - ha);
                            lb[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)(vb - hb)) : (bf16_t)(vb - hb);
                        }
                        const u32x2 a2 = __builtin_bit_cast(u32x2, la), b2 = __builtin_bit_cast(u32x2, lb);
                        const auto q0 = __builtin_amdgcn_permlane32_swap(a2[0], b2[0], false, false);
                        const auto q1 = __builtin_amdgcn_permlane32_swap(a2[1], b2[1], false, false);
                        const u32x4 o2 = {q0[0], q1[0], q0[1], q1[1]};
                        st128<SC1>(o2, rob, eo[2 * pr] != OOB ? ((cbv[2 * pr] + lo_pl) * ob_cb + eo[2 * pr] + 4u * kh2) * 2u : OOB);
                    }
                }
            } else if (has_bf16) {
                const bool gm = scaled && p.gamma != 1.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float vv = gm ? v[g][j] * p.gamma : v[g][j];
                        ob[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)vv) : (bf16_t)vv;
                    }
#ifdef DASR_TRACE
                    if (p.xcd_remap & 2) {  // timing experiment only: lane-linear (fully contiguous) store addresses, wrong layout
                        const unsigned lin = ((((unsigned)blockIdx.x * 4 + wave) * NT + nt) * 4 + g) * 512u + (unsigned)lane * 8u;
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ob), make_rsrc(p.out_bf16.p), lin, 0, 0);
                        continue;
                    }
#endif
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ob), rob, eo[g] != OOB ? (cbv[g] * ob_cb + eo[g]) * 2u : OOB, 0, 0);
                    if (lo_pl) {
                        bf16x4 lb;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float vv = gm ? v[g][j] * p.gamma : v[g][j];
                            const float hh = f16out ? (float)(f16_t)vv : (float)(bf16_t)vv;
                            lb[j] = f16out ? __builtin_bit_cast(bf16_t, (f16_t)(vv - hh)) : (bf16_t)(vv - hh);
                        }
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lb), rob, eo[g] != OOB ? ((cbv[g] + lo_pl) * ob_cb + eo[g]) * 2u : OOB, 0, 0);
                    }
                }
            }
        }
    }
    if constexpr (PACC_OK) {
        if (pacc_on) {   // one partial per workgroup, fixed order: lanes (DPP tree), then the waves in order
            const float t = wave_sum(pacc);
            __syncthreads();   // (every wave is done with the LDS image of the main loop)
            if (lane == 0) ((float*)smem)[wave] = t;
            __syncthreads();
            if (tid == 0) {
                float tot = 0.f;
                for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += ((const float*)smem)[w];
                p.prelu_part[blockIdx.x] = tot * slope;
            }
        }
    }
}

template <int PREC, bool IN_F32, int MT, int KH, int STRIDE, int NT, int KS, bool DBUF, int MODE, int EPI>
__global__ __launch_bounds__(256, 2) void conv_kernel(const dasr_conv_params p) {
    using C = Cfg<PREC, IN_F32, MT, KH, STRIDE, NT, KS>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [act_hi | act_lo (prec 3) | w_hi | w_lo (prec 3)]; one 16 B dummy slot behind
    constexpr int ACT_LO = C::ACT_BYTES, W_HI = C::NARR * C::ACT_BYTES, W_LO = W_HI + C::W_BYTES;
    constexpr int DUMMY = C::LDS_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef DASR_TRACE
    if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
    TRACE_STAMP(0);
    const int cout_tiles = (p.cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (p.Wout + C::TW - 1) / C::TW, tiles_y = (p.Hout + C::TH - 1) / C::TH;
    int bid = blockIdx.x;
    {   // XCD-aware remap: workgroup b runs on XCD b % 8 (private L2).  Give each XCD a contiguous range of tiles so
        // that neighbouring tiles (which share halo rows/columns) hit the same L2.  Bijective when the grid is a
        // multiple of 8; otherwise keep the natural order.
        const int total = gridDim.x;
        if ((p.xcd_remap & 1) && (total & 7) == 0) bid = (bid & 7) * (total >> 3) + (bid >> 3);
    }
    const int mg = bid % MG;
    bid /= MG;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;
    const int iy0 = oy0 * STRIDE - p.pad, ix0 = ox0 * STRIDE - (p.pad_x >= 0 ? p.pad_x : p.pad);
    const int HL = p.ups ? 2 * p.Hin : p.Hin, WL = p.ups ? 2 * p.Win : p.Win;
    const int nchunks = p.cin / (16 * KS);
    constexpr int ESZ = IN_F32 ? 4 : 2;
    static_assert(PREC != 2 || IN_F32, "prec 2 (f16 operands) converts an f32 input while staging");
    const float in_sc = ((PREC == 2 || PREC == 4) && p.in_scale != 0.f) ? p.in_scale : 1.f;
    // bias of this m-group: one value per thread of the first 32*MT, consumed in the epilogue (latency hidden by the main loop)
    float bias_reg = 0.f;
    {
        const int oc = mg * MT * 32 + tid;
        const unsigned bo = ((p.bias != nullptr) & (tid < 32 * MT) & (oc < p.cout)) ? (unsigned)oc * 4u : OOB;
        bias_reg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(p.bias), bo, 0, 0));
    }

    // ---- per-thread staging offsets (independent of the chunk) ----
    unsigned goff[C::AR];  // byte offset inside the image, OOB: zero fill
    int loff[C::AR];       // LDS byte offset (dummy slot for the tail)
#pragma unroll
    for (int r = 0; r < C::AR; ++r) {
        const int q = tid + r * 256;
        const int pix = q / C::PPP, piece = q - pix * C::PPP;
        const int iy = pix / C::IW, ix = pix - iy * C::IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const bool ok = (q < C::NPIECE) & (gy >= 0) & (gy < HL) & (gx >= 0) & (gx < WL);  // bitwise: keeps the prologue one basic block
        const int sy = p.ups ? (gy >> 1) : gy, sx = p.ups ? (gx >> 1) : gx;
        const int pl = piece / C::PPP16, pp = piece - pl * C::PPP16;
        const int spix = p.in_stride > 1 ? (sy * p.in_stride + p.in_oy) * p.in_W + sx * p.in_stride + p.in_ox : sy * p.Win + sx;
        goff[r] = ok ? (unsigned)((pl * (int)p.in.cb_stride + spix * 16 + pp * (IN_F32 ? 4 : 8)) * ESZ) : OOB;
        loff[r] = q < C::NPIECE ? pix * C::PIXB + piece * (IN_F32 ? 8 : 16) : DUMMY;
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc((const char*)p.in.p + (size_t)n * p.in.n_stride * ESZ);
    const unsigned in_chunk_bytes = (unsigned)(p.in.cb_stride * KS * ESZ);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc((const bf16_t*)p.w + (size_t)mg * nchunks * KS * C::NTAPS * MT * 512);
    const unsigned w_chunk_bytes = KS * C::NTAPS * MT * 1024;
    const unsigned w_lo_bytes = (unsigned)(p.w_lo_off * 2);
    unsigned woff[C::WR];
    int wloff[C::WR];
#pragma unroll
    for (int r = 0; r < C::WR; ++r) {
        const int q = tid + r * 256;
        woff[r] = q < C::WPIECE ? (unsigned)q * 16u : OOB;
        wloff[r] = q < C::WPIECE ? q * 16 : DUMMY - W_HI;
    }

    u32x4 areg[C::AR];
    u32x4 wreg[C::WR * C::NARR];
    auto load_chunk = [&](int ck) {
        const unsigned so = (unsigned)ck * in_chunk_bytes;
#pragma unroll
        for (int r = 0; r < C::AR; ++r) areg[r] = __builtin_amdgcn_raw_buffer_load_b128(rin, goff[r], so, 0);
        const unsigned wo = (unsigned)ck * w_chunk_bytes;
#pragma unroll
        for (int r = 0; r < C::WR; ++r) {
            wreg[r] = __builtin_amdgcn_raw_buffer_load_b128(rw, woff[r], wo, 0);
            if constexpr (PREC >= 3) wreg[C::WR + r] = __builtin_amdgcn_raw_buffer_load_b128(rw, woff[r], wo + w_lo_bytes, 0);
        }
    };
    auto store_chunk = [&](char* buf) {
#pragma unroll
        for (int r = 0; r < C::AR; ++r) {
            if constexpr (!IN_F32) {
                *(u32x4*)(buf + loff[r]) = areg[r];
            } else {
                bf16x4 hi, lo;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bf16_t h, l;
                    if constexpr (PREC == 2) {   // one rounding to f16 (11-bit mantissa) of the pre-scaled value
                        h = __builtin_bit_cast(bf16_t, (f16_t)(__uint_as_float(areg[r][j]) * in_sc));
                        l = h;
                    } else if constexpr (PREC == 4) {   // f16 hi + lo of the pre-scaled value (22 mantissa bits)
                        split_f16(__uint_as_float(areg[r][j]) * in_sc, h, l);
                    } else {
                        split_bf16(__uint_as_float(areg[r][j]), h, l);
                    }
                    hi[j] = h;
                    lo[j] = l;
                }
                *(bf16x4*)(buf + loff[r]) = hi;
                if constexpr (PREC >= 3) *(bf16x4*)(buf + (loff[r] == DUMMY ? DUMMY : ACT_LO + loff[r])) = lo;
            }
        }
#pragma unroll
        for (int r = 0; r < C::WR; ++r) {
            *(u32x4*)(buf + W_HI + wloff[r]) = wreg[r];
            if constexpr (PREC >= 3) *(u32x4*)(buf + (wloff[r] == DUMMY - W_HI ? DUMMY : W_LO + wloff[r])) = wreg[C::WR + r];
        }
    };

    // ---- per-lane fragment addresses ----
    const int nn = lane & 31, kh2 = lane >> 5;
    int boff[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        int r, c;
        if constexpr (STRIDE == 1) {
            r = (wave * NT + nt);
            c = nn;
        } else {
            r = (wave * NT + nt) * 2 + (nn >> 4);
            c = nn & 15;
        }
        boff[nt] = ((r * STRIDE) * C::IW + c * STRIDE) * C::PIXB + kh2 * 16;
    }
    const int aoff = lane * 16;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[mi][nt][j] = 0.f;

    auto compute = [&](const char* buf) {
        const char* act_hi = buf;
        const char* act_lo = buf + ACT_LO;
        const char* w_hi = buf + W_HI;
        const char* w_lo = buf + W_LO;
        if constexpr ((PREC == 1 && !IN_F32) || (PREC == 2 && MT == 1)) {
            // software pipeline over taps: the fragments of tap t+1 are requested from LDS before the MFMAs of tap t are issued
            // (two register sets), so an MFMA never waits on a ds_read issued just ahead of it (hipcc's own schedule reads
            // just-in-time: lgkmcnt(1) before every MFMA pair, ~130 cycles per MFMA instead of 32)
            constexpr int TOT = KS * C::NTAPS;
            bf16x8 fa[2][MT], fb[2][NT];
            auto ldfrag = [&](int idx, int set) {
                const int ks = idx / C::NTAPS, t = idx - ks * C::NTAPS;
                const int ky = t / KH, kx = t - ky * KH;
                const int toff = (ky * C::IW + kx) * C::PIXB + ks * 32;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) fa[set][mi] = *(const bf16x8*)(w_hi + ((ks * C::NTAPS + t) * MT + mi) * 1024 + aoff);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) fb[set][nt] = *(const bf16x8*)(act_hi + boff[nt] + toff);
            };
            ldfrag(0, 0);
#pragma unroll
            for (int idx = 0; idx < TOT; ++idx) {
                if (idx + 1 < TOT) ldfrag(idx + 1, (idx + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(fa[idx & 1][mi], fb[idx & 1][nt], acc[mi][nt]);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
        if constexpr (PREC >= 3 && NT <= 2) {
            // same tap-level pipeline for the split-bf16 path where the register budget allows two fragment sets (8x32 tiles)
            constexpr int TOT = KS * C::NTAPS;
            bf16x8 fa[2][MT], fal[2][MT], fb[2][NT], fbl[2][NT];
            auto ldfrag = [&](int idx, int set) {
                const int ks = idx / C::NTAPS, t = idx - ks * C::NTAPS;
                const int ky = t / KH, kx = t - ky * KH;
                const int toff = (ky * C::IW + kx) * C::PIXB + ks * 32;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    fa[set][mi] = *(const bf16x8*)(w_hi + ((ks * C::NTAPS + t) * MT + mi) * 1024 + aoff);
                    fal[set][mi] = *(const bf16x8*)(w_lo + ((ks * C::NTAPS + t) * MT + mi) * 1024 + aoff);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    fb[set][nt] = *(const bf16x8*)(act_hi + boff[nt] + toff);
                    fbl[set][nt] = *(const bf16x8*)(act_lo + boff[nt] + toff);
                }
            };
            ldfrag(0, 0);
#pragma unroll
            for (int idx = 0; idx < TOT; ++idx) {
                if (idx + 1 < TOT) ldfrag(idx + 1, (idx + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(fal[idx & 1][mi], fb[idx & 1][nt], acc[mi][nt]);
                        acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(fa[idx & 1][mi], fbl[idx & 1][nt], acc[mi][nt]);
                        acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(fa[idx & 1][mi], fb[idx & 1][nt], acc[mi][nt]);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int t = 0; t < C::NTAPS; ++t) {
                const int ky = t / KH, kx = t - ky * KH;
                const int toff = (ky * C::IW + kx) * C::PIXB + ks * 32;
                bf16x8 a[MT], al[MT], b[NT], bl[NT];
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    a[mi] = *(const bf16x8*)(w_hi + ((ks * C::NTAPS + t) * MT + mi) * 1024 + aoff);
                    if constexpr (PREC >= 3) al[mi] = *(const bf16x8*)(w_lo + ((ks * C::NTAPS + t) * MT + mi) * 1024 + aoff);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    b[nt] = *(const bf16x8*)(act_hi + boff[nt] + toff);
                    if constexpr (PREC >= 3) bl[nt] = *(const bf16x8*)(act_lo + boff[nt] + toff);
                }
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if constexpr (PREC >= 3) {
                            acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(al[mi], b[nt], acc[mi][nt]);
                            acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(a[mi], bl[nt], acc[mi][nt]);
                        }
                        acc[mi][nt] = mfma16<PREC == 2 || PREC == 4>(a[mi], b[nt], acc[mi][nt]);
                    }
            }
        }
    };

    load_chunk(0);
    TRACE_STAMP(1);
    for (int ck = 0; ck < nchunks; ++ck) {
        if (ck == 2) TRACE_STAMP(8);
        store_chunk(smem);
        if (ck == 2) TRACE_STAMP(9);
        __syncthreads();
        if (ck == 0) TRACE_STAMP(2);
        if (ck == 2) TRACE_STAMP(10);
        if (ck + 1 < nchunks) load_chunk(ck + 1);
        if (ck == 2) TRACE_STAMP(11);
        compute(smem);
        if (ck == 0) TRACE_STAMP(3);
        if (ck == 2) TRACE_STAMP(12);
        __syncthreads();
        if (ck == 2) TRACE_STAMP(13);
    }
    TRACE_STAMP(4);
    if constexpr (PREC == 2 || PREC == 4) {
        if (in_sc != 1.f) {   // undo the operand pre-scaling (exact: power of two)
            const float inv = 1.f / in_sc;
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mi][nt] *= inv;
        }
    }

    conv_epilogue<IN_F32, MT, NT, STRIDE, EPI>(p, acc, smem, bias_reg, tid, mg, n, oy0, ox0);
    TRACE_STAMP(6);  // all stores issued
#ifdef DASR_TRACE
    __builtin_amdgcn_s_waitcnt(0);  // stamp 7 = all stores retired (vmcnt/expcnt/lgkmcnt 0)
#endif
    TRACE_STAMP(7);
#ifdef DASR_TRACE
    if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 16 + 14] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---------------------------------------------------------------------------------------------------
// Dense-block convolution, second generation ("glds"): 3x3 / stride 1 / pad 1, bf16 activations and weights, Cout tiles of 32*MT.
// Differences from conv_kernel:
//  * global -> LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`): no staging registers, no ds_write, no VGPR round trip; the chunk
//    k+1 lands in the other LDS buffer while chunk k is multiplied; one barrier per chunk.
//  * DMA writes 64 lanes x 16 B contiguously, so pixels cannot be padded apart; instead the two 16-byte halves (channels 0-7 /
//    8-15) of pixel p are stored at 16-byte slot 2p + (h ^ bit3(p)): a ds_read_b128 lane group then covers 16 distinct slots of
//    the 256-byte bank row for any tile offset (pixels p and p+8 / p+24 share bank positions and differ in bit 3).  Each lane
//    chooses WHICH global 16 bytes it fetches so that the linear DMA placement realises that layout.
//  * B fragments are reused across the three ky taps (a wave's 4 output rows need 6 input rows per kx): 18 + 9*MT ds_read_b128
//    per chunk instead of 36 + 9*MT, prefetched one (kx, ky) step ahead of the MFMAs.
// Tile 16 x 32 output pixels, 4 waves, wave w owns rows 4w..4w+3 (4 n-tiles of 32 pixels) x MT m-tiles.
// ---------------------------------------------------------------------------------------------------
template <int MT, int NW = 4>
struct GCfg {
    static constexpr int NT = 4, NTH = NW * 64, TH = 4 * NW, TW = 32, IH = TH + 2, IW = 34, NPIX = IH * IW;
    static constexpr int AR = (NPIX * 2 + NTH - 1) / NTH;      // activation DMA pieces per thread (16 B each)
    static constexpr int ACT_BYTES = AR * NTH * 16;            // >= NPIX * 32
    static constexpr int WPIECE = 9 * MT * 64;                 // 16-byte pieces of a chunk's weights
    static constexpr int WR = (WPIECE + NTH - 1) / NTH;
    static constexpr int W_BYTES = WPIECE * 16;
    static constexpr int BUF_BYTES = ACT_BYTES + W_BYTES;
    static constexpr int LDS_BYTES = 2 * BUF_BYTES;
};

// one 16-byte-per-lane DMA piece of chunk ck: piece i < AR activations, else weights; the LDS base is wave-uniform.
// (A free function, not a lambda: hipcc drops the host-side kernel handle when this builtin sits in a lambda of a __global__ template.)
template <int MT, int NW>
__device__ __forceinline__ void glds_dma_piece(int i, int ck, char* buf, __amdgpu_buffer_rsrc_t rin, __amdgpu_buffer_rsrc_t rw, const unsigned* goff,
                                               unsigned in_chunk_bytes, int wave, int tid, int ckp) {
    using C = GCfg<MT, NW>;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    // (cache policy `nt` on these loads, measured in round 3: activations flat, weights +4 % step time -- default policy kept)
    if (i < C::AR) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_ptr)(buf + (i * C::NTH + wave * 64) * 16), 16, goff[i], (unsigned)ckp * in_chunk_bytes, 0, 0);
    } else {
        const int r = i - C::AR;
        if (r * C::NTH + wave * 64 < C::WPIECE)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(buf + C::ACT_BYTES + (r * C::NTH + wave * 64) * 16), 16, (unsigned)(tid + r * C::NTH) * 16u,
                                                     (unsigned)ck * (9u * MT * 1024u), 0, 0);
    }
}

// F16: the 16-bit activations and packed weights are f16 (HR tail of the generator in f16 storage): v_mfma_f32_32x32x16_f16.
// p.ups: nearest x2 up-sampling folded into the DMA source addresses (upconv_blcok, block.py:854-861): each lane fetches the 16 bytes of
// low-resolution pixel (y >> 1, x >> 1); the four duplicates come from L2.
// ABL, RING: always 0 (launch_glds pins them; they stay in the signature because the kernel's printed name keys profiles/pmc_*.json).
template <int MT, int EPI, int NW, int ABL = 0, bool F16 = false, int RING = 0>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void conv_glds_kernel(const dasr_conv_params p) {
    using C = GCfg<MT, NW>;
    constexpr int NT = C::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef DASR_TRACE
    if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 16 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
    TRACE_STAMP(0);
    // every kernel argument the prologue needs, fetched in ONE scalar-memory batch (hipcc otherwise sinks each s_load next to its first
    // use: three dependent ~0.4 us round trips before the first DMA could be issued); the empty asm pins the batch here
    int a_cout = p.cout, a_Wout = p.Wout, a_Hout = p.Hout, a_remap = p.xcd_remap, a_ups = p.ups, a_cin = p.cin, a_Hin = p.Hin, a_Win = p.Win;
    const void* a_bias = p.bias;
    const void* a_in = p.in.p;
    const void* a_w = p.w;
    long long a_nstr = p.in.n_stride, a_cbstr = p.in.cb_stride;
    int a_wrap = p.in_wrap;
    // (the plain "s" inputs: what the EPILOGUE reads from the parameter block rides in the same batch -- its own scalar-memory round trip in front
    // of the stores otherwise; ONE asm statement, or hipcc forms a second batch behind the first wait)
    asm volatile("" : "+s"(a_cout), "+s"(a_Wout), "+s"(a_Hout), "+s"(a_remap), "+s"(a_cin), "+s"(a_Hin), "+s"(a_Win), "+s"(a_bias), "+s"(a_in), "+s"(a_w),
                 "+s"(a_nstr), "+s"(a_cbstr), "+s"(a_wrap), "+s"(a_ups)
                 : "s"(p.slope), "s"(p.out_stride), "s"(p.out_oy), "s"(p.out_ox), "s"(p.out_W), "s"(p.alpha), "s"(p.gamma), "s"(p.out16_lo), "s"(p.N));
    // (p.N is not needed: it keeps the fourth register of the {cout, Hout, Wout, N} load from being re-used by a later load of the batch, whose
    // write-after-write hazard would bring the first wait back)
    a_remap |= a_ups << 8;   // (no arithmetic on a loaded value IN FRONT of the asm: its wait would split the batch)
    const int cout_tiles = (a_cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (a_Wout + C::TW - 1) / C::TW, tiles_y = (a_Hout + C::TH - 1) / C::TH;
    int bid = blockIdx.x;
    {   // XCD-aware tile order as a select, not a branch: the whole prologue stays ONE basic block, so hipcc batches every kernel-argument
        // load into a single scalar-memory round trip at the top (three serialised round trips of ~0.4 us each before)
        const int total = (int)((unsigned)a_remap >> 12);   // grid size from the launcher (gridDim.x is a hidden kernel argument: a second scalar-memory round trip)
        const int remapped = (bid & 7) * (total >> 3) + (bid >> 3);
        bid = ((a_remap & 1) && (total & 7) == 0) ? remapped : bid;
    }
    const int mg = bid % MG;
    bid /= MG;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    const int nchunks = a_cin >> 4;
    const int in_wrap = a_wrap > 0 ? a_wrap : 0x7fffffff;   // split 16-bit input: chunks >= in_wrap read the hi planes a second time
    constexpr int rot = 0;   // (per-workgroup chunk-order rotation was tried against L2 hot-spotting of the shared weight blocks: no effect)
    float bias_reg = 0.f;
    {
        const int oc = mg * MT * 32 + tid;
        const unsigned bo = ((a_bias != nullptr) & (tid < 32 * MT) & (oc < a_cout)) ? (unsigned)oc * 4u : OOB;
        bias_reg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(a_bias), bo, 0, 0));
    }
    // ---- DMA source offsets: piece q = tid + 256 r -> LDS slot q -> pixel p = q >> 1, stored half hs = q & 1 holds channel half hs ^ bit3(p)
    unsigned goff[C::AR];
#pragma unroll
    for (int r = 0; r < C::AR; ++r) {
        const int q = tid + r * C::NTH;
        const int pp = q >> 1, h = (q & 1) ^ ((pp >> 3) & 1);
        const int iy = pp / C::IW, ix = pp - iy * C::IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const int us = (a_remap >> 8) & 1;   // nearest x2: the conv runs on the (2 Hin) x (2 Win) grid, the source pixel is (gy >> 1, gx >> 1)
        const bool ok = (pp < C::NPIX) & (gy >= 0) & (gy < (a_Hin << us)) & (gx >= 0) & (gx < (a_Win << us));  // bitwise: keeps the prologue one basic block
        goff[r] = ok ? (unsigned)((((gy >> us) * a_Win + (gx >> us)) * 16 + 8 * h) * 2) : OOB;
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc((const bf16_t*)a_in + (size_t)n * a_nstr);
    const unsigned in_chunk_bytes = (unsigned)(a_cbstr * 2);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc((const bf16_t*)a_w + (size_t)mg * nchunks * 9 * MT * 512);
    constexpr int NP = C::AR + C::WR;
    // chunk 0 is requested before the fragment addresses and accumulators are set up: the DMA round trip overlaps that ALU work
#pragma unroll
    for (int i = 0; i < NP; ++i) glds_dma_piece<MT, NW>(i, rot, smem, rin, rw, goff, in_chunk_bytes, wave, tid, rot);
    TRACE_STAMP(1);
    // ---- fragment read addresses: row rr (0..5) of this wave's 6 input rows, column shift kx; lane (nn, kh2)
    const int nn = lane & 31, kh2 = lane >> 5;
    int baddr[6][3];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int pp = (wave * NT + rr) * C::IW + nn + kx;
            baddr[rr][kx] = ((pp << 1) + (kh2 ^ ((pp >> 3) & 1))) << 4;
        }
    const int aoff = lane * 16;   // relative to the chunk's weight image

    f32x16 acc[MT][NT];
    // R1_PRE (conv5 of a dense block: alpha * conv + beta1 * x -> fp32 stream): the epilogue's residual fetch kept ONE group of four 1-KiB loads
    // per wave in flight (32 KB per CU against ~2 us of loaded latency: ~15 B/clk) and took 20 k cycles = 18 % of the workgroup
    // (profiles/r03_conv_ablation.txt).  The residual is fetched HERE instead, straight into the accumulator registers -- all 32 loads of a wave
    // (128 KB per workgroup) in flight behind the DMA of chunk 0 -- and the MFMAs accumulate on top of (beta1 / alpha) * x; the epilogue only
    // scales by alpha and stores.  fp32 throughout: alpha * ((beta1 / alpha) x + conv) differs from alpha * conv + beta1 * x by ~1e-7 relative.
    constexpr bool R1_PRE = MT == 2 && EPI != 0 && (EPI & 8);
    if constexpr (R1_PRE) {
        const __amdgpu_buffer_rsrc_t rr1 = make_rsrc((const float*)p.res1.p + (size_t)n * p.res1.n_stride);
        const unsigned r1_cb = (unsigned)p.res1.cb_stride;
        const int nn_ = lane & 31, kh_ = lane >> 5;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int oy = oy0 + wave * NT + nt, ox = ox0 + nn_;
            const bool pv = (oy < a_Hout) & (ox < a_Wout);
            const unsigned pixel = (unsigned)((oy + p.out_oy) * (p.out_W > 0 ? p.out_W : a_Wout) + ox + p.out_ox) * 16u;   // (as conv_epilogue::group_addr with out_stride 1)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int oc = (mg * MT + mi) * 32 + 8 * g + 4 * kh_;
                    const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rr1, pv ? ((unsigned)(oc >> 4) * r1_cb + pixel + (unsigned)(oc & 15)) * 4u : OOB, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][nt][4 * g + j] = __uint_as_float(t[j]);
                }
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[mi][nt][j] = 0.f;
    }

    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's DMA pieces have landed
    __syncthreads();
    if constexpr (R1_PRE) {
        const float c1 = p.beta1 / p.alpha;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mi][nt] *= c1;
    }
    TRACE_STAMP(2);

    constexpr bool PRE = EPI == 68 && MT == 1;
    MaskPre<NT * MT> mpre;
    bf16x8 fb[2][6], fa[2][MT];
    for (int ck = 0; ck < nchunks; ++ck) {
        const char* buf = smem + (ck & 1) * C::BUF_BYTES;   // activation image
        const char* wbuf = buf + C::ACT_BYTES;              // weight image
        char* nbuf = smem + ((ck + 1) & 1) * C::BUF_BYTES;
        const bool more = ck + 1 < nchunks;
        if constexpr (PRE) {
            if (!more) mask_prefetch<MT, NT>(p, mpre, tid, mg, n, oy0, ox0);   // last chunk: the memory pipe is idle, the epilogue finds the mask in registers
        }
        const int ckn = ck + 1 + rot < nchunks ? ck + 1 + rot : ck + 1 + rot - nchunks;  // global index of the next chunk
        const int ckp = ckn >= in_wrap ? ckn - in_wrap : ckn;                            // ... and the input plane group it reads
        if (ck == 2) TRACE_STAMP(8);
        // step s = kx * 3 + ky; B rows of phase kx live in fb[kx & 1], A of step s in fa[s & 1]
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) fb[0][rr] = *(const bf16x8*)(buf + baddr[rr][0]);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) fa[0][mi] = *(const bf16x8*)(wbuf + aoff + (0 * MT + mi) * 1024);
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int kx = s / 3, ky = s - kx * 3;
            if (s + 1 < 9) {
                const int kx1 = (s + 1) / 3, ky1 = (s + 1) - kx1 * 3;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) fa[(s + 1) & 1][mi] = *(const bf16x8*)(wbuf + aoff + ((ky1 * 3 + kx1) * MT + mi) * 1024);
                if (ky == 1 && kx < 2) {  // rows of the next phase, requested one step before they are needed
#pragma unroll
                    for (int rr = 0; rr < 6; ++rr) fb[(kx + 1) & 1][rr] = *(const bf16x8*)(buf + baddr[rr][kx + 1]);
                }
            }
            if (more && s < 4) {  // all pieces of the next chunk are requested in the first steps: they have the rest of the chunk to land
#pragma unroll
                for (int i = s * NP / 4; i < (s + 1) * NP / 4; ++i) glds_dma_piece<MT, NW>(i, ckn, nbuf, rin, rw, goff, in_chunk_bytes, wave, tid, ckp);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mi][nt] = mfma16<F16>(fa[s & 1][mi], fb[kx & 1][nt + ky], acc[mi][nt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ck == 2) TRACE_STAMP(9);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        if (ck == 2) TRACE_STAMP(10);
        __syncthreads();
        if (ck == 2) TRACE_STAMP(11);
    }
    TRACE_STAMP(4);
    if constexpr (EPI == 68 && MT == 2 && !PRE) {   // (the DSN generator's data-gradient convs also leave the PReLU-slope partials: dasr_conv_params::prelu_part)
        if (p.prelu_part) conv_epilogue<false, MT, NT, 1, EPI, F16 ? 1 : 0, false, false, false, false, true>(p, acc, smem, bias_reg, tid, mg, n, oy0, ox0, &mpre);
        else conv_epilogue<false, MT, NT, 1, EPI, F16 ? 1 : 0, PRE>(p, acc, smem, bias_reg, tid, mg, n, oy0, ox0, &mpre);
    } else {
        conv_epilogue<false, MT, NT, 1, R1_PRE ? (EPI & ~8) : EPI, F16 ? 1 : 0, PRE>(p, acc, smem, bias_reg, tid, mg, n, oy0, ox0, &mpre);
    }
    TRACE_STAMP(6);
#ifdef DASR_TRACE
    __builtin_amdgcn_s_waitcnt(0);
#endif
    TRACE_STAMP(7);
#ifdef DASR_TRACE
    if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 16 + 14] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---------------------------------------------------------------------------------------------------
// conv_subpix_dgrad_kernel: data gradient of nearest-x2 + 3x3 (upconv_blcok, block.py:854-861) in its sub-pixel form on f16 tensors
// (dasr_conv_params::ups == 2).  The input is the gradient g on the (2 Hout) x (2 Wout) grid, the output lives on the Hout x Wout grid:
//   out[m][n] = sum over the four parities (py, px) and the taps (a, b) of a 2x2 kernel  Wp[py][px][a][b] . g[2 (m - py + a) + py][2 (n - px + b) + px]
// where Wp are the 16 tap sums of the transposed 3x3 weights (PackRegistry tapmasks, rounded to f16 once): 16 MFMA steps per 16-channel
// chunk into ONE accumulator set instead of 36 on four times the pixels, no gradient tensor at the high resolution and no 2x2 sum behind it.
// A pipeline stage is one (chunk, parity) pair: the DMA de-interleaves that parity's sub-grid of the tile -- 17 x 33 pixels for a tile of
// 16 x 32 outputs -- into the LDS image layout of conv_glds_kernel (every lane chooses which global 16 bytes it fetches), so the fragment
// addressing carries over; the two x-parities of a row are consecutive stages and share their 64-byte runs in the L2.  Per stage 20 KB of
// activations + 4 MT KB of weights, double-buffered: 56 KB at MT 2, two workgroups per CU.  Zero padding of g is the buffer's range check.
// ---------------------------------------------------------------------------------------------------
template <int MT>
struct SCfg {
    static constexpr int NT = 4, NTH = 256, TH = 16, TW = 32, IH = TH + 1, IW = TW + 1, NPIX = IH * IW;
    static constexpr int AR = (NPIX * 2 + NTH - 1) / NTH;      // activation DMA pieces per thread (16 B each)
    static constexpr int ACT_BYTES = AR * NTH * 16;            // >= NPIX * 32
    static constexpr int WPIECE = 4 * MT * 64;                 // 16-byte pieces of a stage's weights (2x2 taps)
    static constexpr int WR = (WPIECE + NTH - 1) / NTH;
    static constexpr int W_BYTES = WPIECE * 16;
    static constexpr int BUF_BYTES = ACT_BYTES + W_BYTES;
    static constexpr int LDS_BYTES = 2 * BUF_BYTES;
};

// one 16-byte-per-lane DMA piece of stage sk = 4 * chunk + parity: piece i < AR activations of plane ckp, else weights
template <int MT>
__device__ __forceinline__ void subpix_dma_piece(int i, int sk, char* buf, __amdgpu_buffer_rsrc_t rin, __amdgpu_buffer_rsrc_t rw, const unsigned* gbase,
                                                 const unsigned* vbits, unsigned par_delta, unsigned in_chunk_bytes, int wave, int tid) {
    using C = SCfg<MT>;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    if (i < C::AR) {
        const unsigned off = ((vbits[i] >> (sk & 3)) & 1u) ? gbase[i] - par_delta : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_ptr)(buf + (i * C::NTH + wave * 64) * 16), 16, off, (unsigned)(sk >> 2) * in_chunk_bytes, 0, 0);
    } else {
        const int r = i - C::AR;
        if (r * C::NTH + wave * 64 < C::WPIECE)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(buf + C::ACT_BYTES + (r * C::NTH + wave * 64) * 16), 16, (unsigned)(tid + r * C::NTH) * 16u,
                                                     (unsigned)sk * (4u * MT * 1024u), 0, 0);
    }
}

template <int MT, int EPI>
__global__ __launch_bounds__(256, 2) void conv_subpix_dgrad_kernel(const dasr_conv_params p) {
    using C = SCfg<MT>;
    constexpr int NT = C::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cout_tiles = (p.cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (p.Wout + C::TW - 1) / C::TW, tiles_y = (p.Hout + C::TH - 1) / C::TH;
    int bid = blockIdx.x;
    {   // XCD-aware tile order (as conv_glds_kernel): neighbouring tiles, which share halo lines, on one XCD
        const int total = (int)gridDim.x;
        const int remapped = (bid & 7) * (total >> 3) + (bid >> 3);
        bid = ((p.xcd_remap & 1) && (total & 7) == 0) ? remapped : bid;
    }
    const int mg = bid % MG;
    bid /= MG;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;
    const int nstages = (p.cin >> 4) * 4;
    float bias_reg = 0.f;
    {
        const int oc = mg * MT * 32 + tid;
        const unsigned bo = ((p.bias != nullptr) & (tid < 32 * MT) & (oc < p.cout)) ? (unsigned)oc * 4u : OOB;
        bias_reg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(p.bias), bo, 0, 0));
    }
    // ---- DMA source offsets: piece q = tid + 256 r -> LDS slot q -> sub-image pixel pp = q >> 1 = (iy, ix), stored half q & 1 holds channel half
    // (q & 1) ^ bit3(pp).  Parity (py, px) reads sub-grid pixel (oy0 + iy - py, ox0 + ix - px), i.e. pixel (2 (oy0 + iy) - py, 2 (ox0 + ix) - px) of g:
    // gbase is the byte offset at parity (0, 0), the parity shifts it by (py Win + px) pixels; vbits bit (2 py + px): inside the sub-grid
    unsigned gbase[C::AR], vbits[C::AR];
#pragma unroll
    for (int r = 0; r < C::AR; ++r) {
        const int q = tid + r * C::NTH;
        const int pp = q >> 1, h = (q & 1) ^ ((pp >> 3) & 1);
        const int iy = pp / C::IW, ix = pp - iy * C::IW;
        const int sy = oy0 + iy, sx = ox0 + ix;
        const bool in = pp < C::NPIX;
        const bool y0 = sy < p.Hout, y1 = (sy >= 1) & (sy <= p.Hout), x0 = sx < p.Wout, x1 = (sx >= 1) & (sx <= p.Wout);
        vbits[r] = in ? ((unsigned)(y0 & x0) | ((unsigned)(y0 & x1) << 1) | ((unsigned)(y1 & x0) << 2) | ((unsigned)(y1 & x1) << 3)) : 0u;
        // (unsigned arithmetic: slots of a partial tile beyond the image may wrap, they are never used -- vbits selects the out-of-range offset)
        gbase[r] = ((2u * (unsigned)sy * (unsigned)p.Win + 2u * (unsigned)sx) * 16u + 8u * (unsigned)h) * 2u;
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc((const bf16_t*)p.in.p + (size_t)n * p.in.n_stride);
    const unsigned in_chunk_bytes = (unsigned)(p.in.cb_stride * 2);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc((const bf16_t*)p.w + (size_t)mg * nstages * 4 * MT * 512);
    const unsigned row_bytes = (unsigned)p.Win * 32u;
    constexpr int NP = C::AR + C::WR;
#pragma unroll
    for (int i = 0; i < NP; ++i) subpix_dma_piece<MT>(i, 0, smem, rin, rw, gbase, vbits, 0u, in_chunk_bytes, wave, tid);
    // ---- fragment read addresses: row rr (0..4) of this wave's 5 sub-image rows, column shift b; lane (nn, kh2)
    const int nn = lane & 31, kh2 = lane >> 5;
    int baddr[5][2];
#pragma unroll
    for (int rr = 0; rr < 5; ++rr)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int pp = (wave * NT + rr) * C::IW + nn + b;
            baddr[rr][b] = ((pp << 1) + (kh2 ^ ((pp >> 3) & 1))) << 4;
        }
    const int aoff = lane * 16;   // relative to the stage's weight image

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[mi][nt][j] = 0.f;

    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's DMA pieces have landed
    __syncthreads();

    bf16x8 fb[2][5], fa[2][MT];
    for (int sk = 0; sk < nstages; ++sk) {
        const char* buf = smem + (sk & 1) * C::BUF_BYTES;   // activation image of this (chunk, parity)
        const char* wbuf = buf + C::ACT_BYTES;              // its 2x2 taps
        char* nbuf = smem + ((sk + 1) & 1) * C::BUF_BYTES;
        const bool more = sk + 1 < nstages;
        const unsigned ndelta = (((sk + 1) >> 1) & 1) * row_bytes + ((sk + 1) & 1) * 32u;   // parity of the next stage: py = bit 1, px = bit 0
        // step s = b * 2 + a (tap row a, tap column b; packed tap a * 2 + b); B rows of column shift b live in fb[b], A of step s in fa[s & 1]
#pragma unroll
        for (int rr = 0; rr < 5; ++rr) fb[0][rr] = *(const bf16x8*)(buf + baddr[rr][0]);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) fa[0][mi] = *(const bf16x8*)(wbuf + aoff + (0 * MT + mi) * 1024);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int b = s >> 1, a = s & 1;
            if (s + 1 < 4) {
                const int b1 = (s + 1) >> 1, a1 = (s + 1) & 1;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) fa[(s + 1) & 1][mi] = *(const bf16x8*)(wbuf + aoff + ((a1 * 2 + b1) * MT + mi) * 1024);
                if (s == 0) {   // rows of the second column shift, requested one step before they are needed
#pragma unroll
                    for (int rr = 0; rr < 5; ++rr) fb[1][rr] = *(const bf16x8*)(buf + baddr[rr][1]);
                }
            }
            if (more && s < 2) {   // the next stage is requested in the first steps: it has the rest of this one to land
#pragma unroll
                for (int i = s * NP / 2; i < (s + 1) * NP / 2; ++i) subpix_dma_piece<MT>(i, sk + 1, nbuf, rin, rw, gbase, vbits, ndelta, in_chunk_bytes, wave, tid);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mi][nt] = mfma16<true>(fa[s & 1][mi], fb[b][nt + a], acc[mi][nt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
    }
    conv_epilogue<false, MT, NT, 1, EPI, 1, false>(p, acc, smem, bias_reg, tid, mg, n, oy0, ox0, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// conv_chain_kernel (round 4): a CHAIN of dense-block convs in ONE persistent launch -- the forward trunk of the generator
// (conv1-4 + conv5 of every RDB, 5 x 3 x nb layers of the same geometry) without a kernel boundary between layers.
//
// What a boundary costs per layer (profiles/r04_kernel_budget.txt: ~10 us of non-MFMA time in a 20 us Cout-32 launch): kernel end / start
// (1.7 us), workgroup ramp (1.5 us), the argument round trip and the first DMA round trip (2 us), all of it with the matrix cores idle.
// Round 2 measured that replacing the boundary by neighbour flags costs the same ~3 us per stage WHEN THE WAIT IS EXPOSED
// (profiles/r02i_micro_sync.txt).  In a dense block it need not be: layer L reads planes [0, cin/16) of the slab, of which only the LAST
// cout(L-1)/16 planes come from layer L-1 -- everything before is at least two layers old and final.  A workgroup therefore starts layer L
// immediately on the old planes and looks at its neighbours' flags only before it requests the first chunk that holds layer L-1's output
// (dep_chunk): 2-8 chunks = 5-20 us after it published its own flag.  Only conv1 of an RDB (all 64 input channels come from the previous
// conv5) waits up front.
//
// Coherence.  All tiles of image n are given to workgroups that RUN on XCD n % 8 (every workgroup reads HW_REG_XCC_ID and draws its tile from that XCD's
// ticket counter, see the kernel), so every halo a tile reads was written by a CU of its own XCD and the XCD's L2 is the coherence point (the per-XCD L2s are not
// coherent with each other without agent-scope fences that cost 30-70 us per use).  Data stores and the flag store are write-through (sc1: with
// plain stores a few lines per 10^4 were not yet in the L2 when vmcnt(0) returned); flag polls bypass the vector L1 (sc0 sc1); halo data is
// first touched after the flag (the L1 was invalidated at kernel start, a 128-byte L1 line never spans two tiles: tiles are 32 pixels = 1 KiB
// wide per plane row).
// Co-residency: every workgroup of the launch must be resident (a waiting tile spins) and every XCD must host exactly its share: grid == 2 workgroups x
// 256 CUs, checked by the launcher; a spin gives up after ~1 s and sets err bit 1 (the results are then wrong, the launch still ends).
// ---------------------------------------------------------------------------------------------------
#ifdef DASR_TRACE
// per-workgroup accumulators of the chained launches: g_trace[2^20 + block * 64 + type * 8 + phase] (behind the per-launch stamps of the other kernels) (type 0 conv1 of a dense block, 1 conv2-4, 2 conv5-class;
// phase 0 entry (flag wait + chunk-0 request), 1 chunk 0 landed, 2 main loop, 3 (inside 2) flag poll, 4 epilogue issue, 5 publish, 6 items, 7 chunks)
#define CH_T() (g_trace && threadIdx.x == 0 ? (unsigned long long)__builtin_readcyclecounter() : 0ull)
#define CH_ACC(type, phase, val)                                                                           \
    do {                                                                                                   \
        if (g_trace && threadIdx.x == 0) g_trace[(size_t)(1 << 20) + (size_t)blockIdx.x * 64 + (type) * 8 + (phase)] += (val); \
    } while (0)
#else
#define CH_T() 0ull
#define CH_ACC(type, phase, val) do {} while (0)
#endif

#ifdef DASR_TRACE
// where a workgroup of a chained launch ran: g_trace[2^20 + block * 64 + 56 ...] = HW_ID register, ticket, XCC id
#define CH_WHERE(ticket, xcc)                                                                  \
    do {                                                                                       \
        if (g_trace && threadIdx.x == 0) {                                                     \
            unsigned hw;                                                                       \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                   \
            g_trace[(size_t)(1 << 20) + (size_t)blockIdx.x * 64 + 56] = hw;                    \
            g_trace[(size_t)(1 << 20) + (size_t)blockIdx.x * 64 + 57] = (unsigned)(ticket);    \
            g_trace[(size_t)(1 << 20) + (size_t)blockIdx.x * 64 + 58] = (unsigned)(xcc);       \
        }                                                                                      \
    } while (0)
#else
#define CH_WHERE(ticket, xcc) do {} while (0)
#endif

struct ChainSync {
    __amdgpu_buffer_rsrc_t rflags;
    int* err;
    unsigned f0;          // this launch's stage base: flag value every tile of the launch starts with
    int base, ty, tx, tiles_y, tiles_x;

    // layer `layer` may read the outputs of layer - 1 in the halo: the eight neighbours have published f0 + layer
    __device__ __forceinline__ void wait(int layer, int tid) const {
        if (layer > 0) {
            if (tid < 9 && tid != 4) {
                const int y = ty + tid / 3 - 1, x = tx + tid % 3 - 1;
                if ((y >= 0) & (y < tiles_y) & (x >= 0) & (x < tiles_x)) {
                    const unsigned off = (unsigned)(base + y * tiles_x + x) * 4u, target = f0 + (unsigned)layer;
                    int spins = 0;
                    while ((int)(__builtin_amdgcn_raw_buffer_load_b32(rflags, off, 0, 17) - target) < 0) {
                        __builtin_amdgcn_s_sleep(2);
                        ++spins;
                        // give up after ~1 s -- or at once when another wait of this launch has given up already (the launch is lost either way:
                        // ONE timeout per launch, not one per layer, when the placement assumption is broken, e.g. by a second process on the device)
                        if (spins > (1 << 21) || ((spins & 1023) == 0 && __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(err), 0, 0, 17) != 0)) {
                            atomicOr(err, 2);
                            break;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // every store of this tile's layer has been acknowledged; then the flag
    __device__ __forceinline__ void publish(int layer, int tid) const {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (tid == 0) __builtin_amdgcn_raw_buffer_store_b32(f0 + (unsigned)layer + 1u, rflags, (unsigned)(base + ty * tiles_x + tx) * 4u, 0, 16);
    }
};

template <int MT, int EPI, bool F16>
__device__ __forceinline__ void chain_layer(const dasr_conv_params& p, char* smem, const int tid, const int n, const int oy0, const int ox0,
                                            const unsigned (&goff)[GCfg<1, 4>::AR], const int dep_chunk, const ChainSync& cs, const int layer) {
    using C = GCfg<MT, 4>;
    constexpr int NT = C::NT, NW = 4;
    static_assert(GCfg<1, 4>::AR == GCfg<2, 4>::AR, "the activation pieces do not depend on MT");
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nchunks = p.cin >> 4;
    const int ttype = MT == 2 ? 2 : (dep_chunk <= 1 ? 0 : 1);
    (void)ttype;
    const unsigned long long t_a = CH_T();
    float bias_reg;
    {
        const unsigned bo = ((p.bias != nullptr) & (tid < 32 * MT)) ? (unsigned)tid * 4u : OOB;
        bias_reg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(make_rsrc(p.bias), bo, 0, 0));
    }
    const __amdgpu_buffer_rsrc_t rin = make_rsrc((const bf16_t*)p.in.p + (size_t)n * p.in.n_stride);
    const unsigned in_chunk_bytes = (unsigned)(p.in.cb_stride * 2);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.w);
    constexpr int NP = C::AR + C::WR;
    if (dep_chunk <= 0) cs.wait(layer, tid);   // every input plane comes from the previous layer (conv1 of an RDB reads the previous conv5's shadow)
#pragma unroll
    for (int i = 0; i < NP; ++i) glds_dma_piece<MT, NW>(i, 0, smem, rin, rw, goff, in_chunk_bytes, wave, tid, 0);
    const unsigned long long t_b = CH_T();
    const int nn = lane & 31, kh2 = lane >> 5;
    int baddr[6][3];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int pp = (wave * NT + rr) * C::IW + nn + kx;
            baddr[rr][kx] = ((pp << 1) + (kh2 ^ ((pp >> 3) & 1))) << 4;
        }
    const int aoff = lane * 16;
    f32x16 acc[MT][NT];
    constexpr bool R1_PRE = MT == 2 && (EPI & 8);   // conv5: the fp32 residual lands in the accumulators behind chunk 0's DMA (see conv_glds_kernel)
    if constexpr (R1_PRE) {
        const __amdgpu_buffer_rsrc_t rr1 = make_rsrc((const float*)p.res1.p + (size_t)n * p.res1.n_stride);
        const unsigned r1_cb = (unsigned)p.res1.cb_stride;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int oy = oy0 + wave * NT + nt, ox = ox0 + nn;
            const bool pv = (oy < p.Hout) & (ox < p.Wout);
            const unsigned pixel = (unsigned)(oy * p.Wout + ox) * 16u;
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int oc = mi * 32 + 8 * g + 4 * kh2;
                    const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rr1, pv ? ((unsigned)(oc >> 4) * r1_cb + pixel + (unsigned)(oc & 15)) * 4u : OOB, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mi][nt][4 * g + j] = __uint_as_float(t[j]);
                }
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[mi][nt][j] = 0.f;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    if constexpr (R1_PRE) {
        const float c1 = p.beta1 / p.alpha;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mi][nt] *= c1;
    }
    constexpr bool PRE = EPI == 68 && MT == 1;   // data gradient of conv1-4: the LeakyReLU' mask of the output tile is fetched during the last chunk (see conv_glds_kernel)
    MaskPre<NT * MT> mpre;
    bf16x8 fb[2][6];
    const unsigned long long t_c = CH_T();
    unsigned long long t_poll = 0;
    (void)t_poll;
    for (int ck = 0; ck < nchunks; ++ck) {
        const char* buf = smem + (ck & 1) * C::BUF_BYTES;
        const char* wbuf = buf + C::ACT_BYTES;
        char* nbuf = smem + ((ck + 1) & 1) * C::BUF_BYTES;
        const bool more = ck + 1 < nchunks;
        if (ck + 1 == dep_chunk) {   // the next chunk is the first that holds the previous layer's output: the neighbours must have published it
            const unsigned long long t0 = CH_T();
            cs.wait(layer, tid);
            t_poll += CH_T() - t0;
        }
        if constexpr (PRE) {
            if (!more) mask_prefetch<MT, NT>(p, mpre, tid, 0, n, oy0, ox0);
        }
        // (Measured in round 5 and not kept, profiles/r05_chain_variants.txt: other spreads of the DMA pieces over the steps, weight fragments read two
        // steps ahead, no sched_barrier; conv5 storing and publishing its 16-bit shadow in front of the fp32 stream; plain stores for that stream.)
        // Only fa[0] / fa[1] are used.  The third set exists to steer the compiler: with fa[2][MT] hipcc schedules and allocates this loop differently,
        // so the size is kept at 3 to preserve the code object that was measured (profiles/r05_chain_trace.txt).  Do not shrink it without re-measuring.
        bf16x8 fa[3][MT];
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) fb[0][rr] = *(const bf16x8*)(buf + baddr[rr][0]);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) fa[0][mi] = *(const bf16x8*)(wbuf + aoff + (0 * MT + mi) * 1024);
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int kx = s / 3, ky = s - kx * 3;
            if (s + 1 < 9) {
                const int kx1 = (s + 1) / 3, ky1 = (s + 1) - kx1 * 3;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) fa[(s + 1) & 1][mi] = *(const bf16x8*)(wbuf + aoff + ((ky1 * 3 + kx1) * MT + mi) * 1024);
                if (ky == 1 && kx < 2) {
#pragma unroll
                    for (int rr = 0; rr < 6; ++rr) fb[(kx + 1) & 1][rr] = *(const bf16x8*)(buf + baddr[rr][kx + 1]);
                }
            }
            if (more && s < 4) {
#pragma unroll
                for (int i = s * NP / 4; i < (s + 1) * NP / 4; ++i) glds_dma_piece<MT, NW>(i, ck + 1, nbuf, rin, rw, goff, in_chunk_bytes, wave, tid, ck + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mi][nt] = mfma16<F16>(fa[s & 1][mi], fb[kx & 1][nt + ky], acc[mi][nt]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
    }
    const unsigned long long t_d = CH_T();
    conv_epilogue<false, MT, NT, 1, R1_PRE ? (EPI & ~8) : EPI, F16 ? 1 : 0, PRE, true>(p, acc, smem, bias_reg, tid, 0, n, oy0, ox0, &mpre);
    const unsigned long long t_e = CH_T();
    cs.publish(layer, tid);
    const unsigned long long t_f = CH_T();
    CH_ACC(ttype, 0, t_b - t_a);
    CH_ACC(ttype, 1, t_c - t_b);
    CH_ACC(ttype, 2, t_d - t_c);
    CH_ACC(ttype, 3, t_poll);
    CH_ACC(ttype, 4, t_e - t_d);
    CH_ACC(ttype, 5, t_f - t_e);
    CH_ACC(ttype, 6, 1ull);
    CH_ACC(ttype, 7, (unsigned long long)nchunks);
    (void)t_a; (void)t_b; (void)t_c; (void)t_d; (void)t_e; (void)t_f;
}

template <bool F16, bool BWD>
__global__ __launch_bounds__(256, 2) void conv_chain_kernel(const dasr_conv_params* __restrict__ layers, const int* __restrict__ dep_chunk, int nlayers,
                                                           int tiles_y, int tiles_x, unsigned* flags, unsigned* tickets, int* err) {
    using C = GCfg<1, 4>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int T = tiles_y * tiles_x;
    // Which tile this workgroup owns follows from WHERE IT RUNS, not from its index: the dispatcher's round-robin over the XCDs (workgroup b -> XCD
    // b % 8) holds for a kernel that has the chip to itself and fewer workgroups than slots, but not for the 512-workgroup launch that fills every
    // slot (measured: workgroups land off their index once XCDs fill up).  Every workgroup reads its XCC id and draws a ticket from that XCD's
    // counter (an atomic in the XCD's own L2: only its CUs touch the word): ticket -> (image of this XCD, tile).  The launch fills the chip exactly
    // (grid = 512 = 2 workgroups x 256 CUs, all resident, checked by the launcher), so every XCD hosts exactly grid / 8 workgroups and the tickets
    // of an XCD cover its images' tiles exactly once; the counters run on from launch to launch (ticket % quota).
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const int xcd = (int)(xcc & 7u);
    const int quota = (int)(gridDim.x >> 3);
    int* tk = (int*)smem;
    if (tid == 0) tk[0] = (int)(atomicAdd(tickets + xcd, 1u) % (unsigned)quota);
    __syncthreads();
    const int j = __builtin_amdgcn_readfirstlane(tk[0]);
    __syncthreads();
    const int img = j / T, tile = j - img * T;
    const int n = xcd + 8 * img;                        // all tiles of image n on XCD n % 8
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    CH_WHERE(j, xcc);
    ChainSync cs;
    cs.rflags = make_rsrc(flags);
    cs.err = err;
    cs.base = n * T;
    cs.ty = ty, cs.tx = tx, cs.tiles_y = tiles_y, cs.tiles_x = tiles_x;
    cs.f0 = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_raw_buffer_load_b32(cs.rflags, (unsigned)(cs.base + tile) * 4u, 0, 17));
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    const int Hin = layers[0].Hin, Win = layers[0].Win;
    unsigned goff[C::AR];
#pragma unroll
    for (int r = 0; r < C::AR; ++r) {
        const int q = tid + r * C::NTH;
        const int pp = q >> 1, h = (q & 1) ^ ((pp >> 3) & 1);
        const int iy = pp / C::IW, ix = pp - iy * C::IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const bool ok = (pp < C::NPIX) & (gy >= 0) & (gy < Hin) & (gx >= 0) & (gx < Win);
        goff[r] = ok ? (unsigned)(((gy * Win + gx) * 16 + 8 * h) * 2) : OOB;
    }
    for (int L = 0; L < nlayers; ++L) {
        const dasr_conv_params& p = layers[L];
        const int dep = dep_chunk[L];
        if constexpr (BWD) {   // data-gradient chain: mask -> 16-bit planes; alpha, one / two fp32 residuals -> fp32 + 16-bit (no bias)
            if (p.mt == 1) chain_layer<1, 68, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
            else if (p.res2.p != nullptr) chain_layer<2, 248, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
            else chain_layer<2, 232, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
        } else {
            if (p.mt == 1) chain_layer<1, 67, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
            else if (p.res2.p != nullptr) chain_layer<2, 249, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
            else chain_layer<2, 233, F16>(p, smem, tid, n, oy0, ox0, goff, dep, cs, L);
        }
    }
}

template <int MT, int EPI = 0, int NW = 4, int ABL = 0, bool F16 = false, int RING = 0>
int launch_glds(const dasr_conv_params& p, hipStream_t s) {
    // ABL / RING stay in the signature only because bench.py and profiles/pmc_*.json key on the printed name (conv_glds_kernel<2, 0, 4, 0, true, 0>)
    static_assert(ABL == 0 && RING == 0, "one dense-block conv kernel");
    using C = GCfg<MT, NW>;
    static bool attr_set = false;
    auto kfn = conv_glds_kernel<MT, EPI, NW, ABL, F16, RING>;
    if ((p.cin & 15) || p.kh != 3 || p.stride != 1 || p.pad != 1 || p.in_f32 || p.prec != (F16 ? 2 : 1) || (p.pad_x >= 0 && p.pad_x != 1) || p.in_stride > 1)
        return DASR_EINVAL;
    if (p.out_bf16.p && (p.out16_f16 != 0) != F16) return DASR_EINVAL;   // the 16-bit output format of this kernel is its operand format (compile time)
    if (p.prelu_part && !(EPI == 68 && MT == 2)) return DASR_EINVAL;   // the slope-gradient partials exist in the 64-channel mask-only epilogue alone
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
        attr_set = true;
    }
    const int cout_tiles = (p.cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (p.Wout + C::TW - 1) / C::TW, tiles_y = (p.Hout + C::TH - 1) / C::TH;
    const long long grid = (long long)MG * tiles_x * tiles_y * p.N;
    if (grid <= 0 || grid >= (1LL << 20)) return DASR_EINVAL;
    dasr_conv_params q = p;
    q.xcd_remap = (p.xcd_remap & 0xfff) | (int)((unsigned)grid << 12);   // bits 12-31: the grid size (conv_glds_kernel reads it instead of gridDim.x)
    DASR_LAUNCH_TAG(__PRETTY_FUNCTION__, kfn, dim3((unsigned)grid), dim3(C::NTH), C::LDS_BYTES, s, q);
    return (int)hipGetLastError();
}

// dasr_conv_params::ups == 2: the sub-pixel data gradient of nearest-x2 + 3x3 on f16 tensors (conv_subpix_dgrad_kernel)
template <int MT, int EPI>
int launch_subpix_dgrad(const dasr_conv_params& p, hipStream_t s) {
    using C = SCfg<MT>;
    static bool attr_set = false;
    auto kfn = conv_subpix_dgrad_kernel<MT, EPI>;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
        attr_set = true;
    }
    const int cout_tiles = (p.cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (p.Wout + C::TW - 1) / C::TW, tiles_y = (p.Hout + C::TH - 1) / C::TH;
    const long long grid = (long long)MG * tiles_x * tiles_y * p.N;
    if (grid <= 0 || grid >= (1LL << 31)) return DASR_EINVAL;
    DASR_LAUNCH_TAG(__PRETTY_FUNCTION__, kfn, dim3((unsigned)grid), dim3(C::NTH), C::LDS_BYTES, s, p);
    return (int)hipGetLastError();
}

int classify_epi(const dasr_conv_params& p);

int subpix_dgrad(const dasr_conv_params& p, hipStream_t s) {
    if (p.in_f32 || p.prec != 2 || p.kh != 3 || p.stride != 1 || p.pad != 1 || (p.pad_x >= 0 && p.pad_x != 1) || p.in_stride > 1 || p.out_stride > 1) return DASR_EINVAL;
    if (p.Hout <= 0 || p.Wout <= 0 || p.N <= 0 || p.Hin != 2 * p.Hout || p.Win != 2 * p.Wout) return DASR_EINVAL;
    if (p.in_wrap || p.out16_lo || p.res1_lo || p.prelu_part) return DASR_EINVAL;
    if (p.mt != 1 && p.mt != 2) return DASR_EINVAL;
    // epilogue terms of a data gradient, and no others: LeakyReLU' mask (constant slope), alpha / gamma, fp32 and / or f16 output on the dense low-resolution grid
    if (p.bias || p.act || p.res1.p || p.res2.p || p.slope_ptr || p.out_oy || p.out_ox || p.out_W) return DASR_EINVAL;
    if (!p.out_f32.p && !p.out_bf16.p) return DASR_EINVAL;
    if (p.out_bf16.p && !p.out16_f16) return DASR_EINVAL;   // the 16-bit output format of this kernel is f16, its operand format
    // 32-bit byte offsets inside one image: a plane of g, and the planes of one image together
    if ((long long)(p.Hin + 1) * p.Win * 32 > 0x7fffffffLL || (long long)(p.cin >> 4) * p.in.cb_stride * 2 > 0xffffffffLL) return DASR_EINVAL;
    const int e = classify_epi(p);
    if (p.mt == 2) {
        switch (e) {
            case 68: return launch_subpix_dgrad<2, 68>(p, s);     // LeakyReLU' mask -> f16 gradient (upconv2)
            case 160: return launch_subpix_dgrad<2, 160>(p, s);   // alpha -> fp32 gradient of the trunk output (upconv1)
            default: return launch_subpix_dgrad<2, 0>(p, s);
        }
    }
    return launch_subpix_dgrad<1, 0>(p, s);
}

template <int PREC, bool IN_F32, int MT, int KH, int STRIDE, int NT, int KS = 1, bool DBUF = false, int MODE = 0, int EPI = 0>
int launch(const dasr_conv_params& p, hipStream_t s) {
    // KS / DBUF / MODE stay in the signature only because bench.py and profiles/pmc_*.json key on the printed name (conv_kernel<3, true, 1, 3, 1, 4, 1, false, 0, 0>)
    static_assert(KS == 1 && !DBUF && MODE == 0, "one staging form of the register-staged kernel");
    using C = Cfg<PREC, IN_F32, MT, KH, STRIDE, NT, KS>;
    static bool attr_set = false;
    auto kfn = conv_kernel<PREC, IN_F32, MT, KH, STRIDE, NT, KS, DBUF, MODE, EPI>;
    if (p.cin % (16 * KS)) return DASR_EINVAL;
    if (p.prelu_part) return DASR_EINVAL;   // (dasr_conv_params::prelu_part: the LDS-DMA kernel's 64-channel mask-only epilogue only -- never silently dropped)
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES + 16));
        attr_set = true;
    }
    const int cout_tiles = (p.cout + 31) >> 5;
    const int MG = (cout_tiles + MT - 1) / MT;
    const int tiles_x = (p.Wout + C::TW - 1) / C::TW, tiles_y = (p.Hout + C::TH - 1) / C::TH;
    const long long grid = (long long)MG * tiles_x * tiles_y * p.N;
    if (grid <= 0 || grid > 0x7fffffffLL) return DASR_EINVAL;
    DASR_LAUNCH_TAG(__PRETTY_FUNCTION__, kfn, dim3((unsigned)grid), dim3(256), C::LDS_BYTES + 16, s, p);
    return (int)hipGetLastError();
}

// naive cross-check: one thread per (n, oc, oy, ox); fp32 direct convolution from the reference weight layout
__global__ void conv_naive_kernel(const dasr_conv_params p, const float* w) {
    const long long total = (long long)p.N * p.cout * p.Hout * p.Wout;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = i % p.Wout;
    long long t = i / p.Wout;
    const int oy = t % p.Hout;
    t /= p.Hout;
    const int oc = t % p.cout;
    const int n = t / p.cout;
    const int HL = p.ups ? 2 * p.Hin : p.Hin, WL = p.ups ? 2 * p.Win : p.Win;
    float acc = 0.f;
    for (int c = 0; c < p.cin; ++c)
        for (int ky = 0; ky < p.kh; ++ky)
            for (int kx = 0; kx < p.kh; ++kx) {
                const int gy = oy * p.stride - p.pad + ky, gx = ox * p.stride - (p.pad_x >= 0 ? p.pad_x : p.pad) + kx;
                if (gy < 0 || gy >= HL || gx < 0 || gx >= WL) continue;
                const int sy = p.ups ? gy >> 1 : gy, sx = p.ups ? gx >> 1 : gx;
                const size_t spix = p.in_stride > 1 ? ((size_t)sy * p.in_stride + p.in_oy) * p.in_W + (size_t)sx * p.in_stride + p.in_ox : (size_t)sy * p.Win + sx;
                const size_t o = (size_t)n * p.in.n_stride + (size_t)(c >> 4) * p.in.cb_stride + spix * 16 + (c & 15);
                const float x = p.in_f32 ? ((const float*)p.in.p)[o] : (float)((const bf16_t*)p.in.p)[o];
                acc += x * w[(((size_t)oc * p.cin + c) * p.kh + ky) * p.kh + kx];
            }
    if (p.bias) acc += p.bias[oc];
    const float nslope = p.slope_ptr ? *p.slope_ptr : p.slope;
    if (p.act == 1) acc = acc > 0.f ? acc : acc * nslope;
    if (p.act == 2) acc = 1.f / (1.f + expf(-acc));
    const size_t po = ((size_t)oy * p.Wout + ox) * 16 + (oc & 15);
    if (p.mask.p) {
        const size_t mo = (size_t)n * p.mask.n_stride + (size_t)(oc >> 4) * p.mask.cb_stride + po;
        const float m = p.mask_f32 ? ((const float*)p.mask.p)[mo] : (float)((const bf16_t*)p.mask.p)[mo];
        acc = m > 0.f ? acc : acc * nslope;
    }
    acc *= p.alpha;
    if (p.res1.p) acc += p.beta1 * ((const float*)p.res1.p)[(size_t)n * p.res1.n_stride + (size_t)(oc >> 4) * p.res1.cb_stride + po];
    if (p.res2.p) acc += p.beta2 * ((const float*)p.res2.p)[(size_t)n * p.res2.n_stride + (size_t)(oc >> 4) * p.res2.cb_stride + po];
    if (p.out_f32.p) ((float*)p.out_f32.p)[(size_t)n * p.out_f32.n_stride + (size_t)(oc >> 4) * p.out_f32.cb_stride + po] = acc;
    if (p.out_bf16.p)
        ((bf16_t*)p.out_bf16.p)[(size_t)n * p.out_bf16.n_stride + (size_t)(oc >> 4) * p.out_bf16.cb_stride + po] = (bf16_t)(acc * p.gamma);
}

// compile-time epilogue variant of the hot dense-block cases (bit set: see conv_kernel's epilogue); 0 = generic
int classify_epi(const dasr_conv_params& p) {
    if ((p.cout & 31) || p.act == 2 || p.out_stride > 1 || p.res1_lo || (p.out16_lo && !p.out16_f16)) return 0;
    if (p.act == 1 && !p.slope_ptr && !(p.slope >= 0.f && p.slope <= 1.f)) return 0;   // the specialised epilogues use max(v, slope * v) for a constant slope, a select for a learned one (slope_ptr)
    int e = (p.bias ? 1 : 0) | (p.act == 1 ? 2 : 0) | (p.mask.p ? 4 : 0) | (p.res1.p ? 8 : 0) | (p.res2.p ? 16 : 0) | (p.out_f32.p ? 32 : 0) |
            (p.out_bf16.p ? 64 : 0);
    if (p.res1.p || p.alpha != 1.f || p.gamma != 1.f) e |= 128;
    return e;
}

// workgroup-shape rule of the Cout = 64 dense-block convs (dasr_set_tuning key 2): 13 = the 8-wave form for launches of <= 256 four-wave workgroups
// (worth 1-2 % of the step under two sub-batch streams), 12 = always 4 waves
int g_tune_rdb64 = 13;

#include "rdb_is.h"

}  // namespace

#ifdef DASR_TRACE
extern "C" int dasr_debug_set_trace(void* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf));
}
#endif

extern "C" int dasr_set_tuning(int32_t key, int32_t value) {
    // one dense-block conv kernel: the only live choice is the workgroup-shape rule of the Cout = 64 launches (key 2); keys 1 / 3-6 accept the one
    // value the library is built for
    if (key == 2 && (value == 12 || value == 13)) { g_tune_rdb64 = value; return 0; }
    if ((key == 1 && value == 12) || (key == 3 && value == 0) || (key == 4 && value == 1) || (key == 5 && value == 1) || (key == 6 && value == 0)) return 0;
    return DASR_EINVAL;
}

// host_layers: the same nlayers parameter blocks the device array holds (the launcher validates them; the kernel reads the device copy)
extern "C" int dasr_conv_chain(const dasr_conv_params* dev_layers, const dasr_conv_params* host_layers, const int32_t* dev_dep_chunk, int32_t nlayers,
                               uint32_t* dev_flags, int32_t* dev_err, void* stream) {
    using C = GCfg<2, 4>;
    if (!dev_layers || !host_layers || !dev_dep_chunk || nlayers <= 0 || !dev_flags || !dev_err) return DASR_EINVAL;
    const dasr_conv_params& p0 = host_layers[0];
    const bool f16 = p0.prec == 2;
    const bool bwd = classify_epi(p0) == 68 || classify_epi(p0) == 232 || classify_epi(p0) == 248;
    for (int i = 0; i < nlayers; ++i) {
        const dasr_conv_params& p = host_layers[i];
        // one geometry for the whole chain: dense 3x3 / stride 1 / pad 1 on 16-bit tensors, every layer one m-group of its workgroup shape
        if (p.kh != 3 || p.stride != 1 || p.pad != 1 || p.in_f32 || p.prec != p0.prec || (p.cin & 15) || p.cin <= 0 || p.ups || p.in_wrap || p.out16_lo || p.res1_lo) return DASR_EINVAL;
        if (p.Hin != p0.Hin || p.Win != p0.Win || p.Hout != p0.Hin || p.Wout != p0.Win || p.N != p0.N || p.out_stride > 1 || p.in_stride > 1 || p.out_W || p.out_oy || p.out_ox) return DASR_EINVAL;
        if (!(p.mt == 1 || p.mt == 2) || p.cout != 32 * p.mt || !p.w || !p.in.p || p.slope_ptr || p.mask_f32 || p.prelu_part) return DASR_EINVAL;
        if ((p.out16_f16 != 0) != f16 || (p.prec != 1 && p.prec != 2)) return DASR_EINVAL;
        const int epi = classify_epi(p);
        // forward: conv1-4 bias + LeakyReLU -> 16-bit planes (67), conv5 bias, alpha, one / two fp32 residuals -> fp32 + 16-bit (233 / 249);
        // data gradient: LeakyReLU' mask -> 16-bit planes (68), alpha, one / two fp32 residuals -> fp32 + 16-bit (232 / 248)
        const bool ok = bwd ? (p.mt == 1 ? epi == 68 : (epi == 232 || epi == 248)) : (p.mt == 1 ? epi == 67 : (epi == 233 || epi == 249));
        if (!ok) return DASR_EINVAL;
    }
    const int tiles_x = (p0.Wout + C::TW - 1) / C::TW, tiles_y = (p0.Hout + C::TH - 1) / C::TH;
    const long long ntiles = (long long)tiles_x * tiles_y * p0.N;
    const long long grid = 512;   // the launch fills the chip exactly (2 workgroups x 256 CUs, all resident): see the ticket comment in the kernels
    // whole images per XCD, one tile per workgroup (a multi-tile form measured slower than one launch per conv: profiles/r05_chain_trace.txt)
    if ((p0.N & 7) || ntiles != grid) return DASR_EINVAL;
    {
        static int n_cu = -1;   // (a partitioned device -- CPX / DPX -- exposes fewer CUs per logical GPU: the launch would not be resident as a whole)
        if (n_cu < 0) {
            int dev = 0;
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDevice(&dev));
            HIP_TRY(hipGetDeviceProperties(&prop, dev));
            n_cu = prop.multiProcessorCount;
        }
        if (n_cu != 256) return DASR_EINVAL;
    }
    hipStream_t s = as_stream(stream);
    static bool attr_set[4] = {false, false, false, false};
    const int v = (f16 ? 1 : 0) | (bwd ? 2 : 0);
// (NAME: the kernel's name as rocprofv3 prints it -- <F16, BWD> -- so that bench.py finds its PMC traffic entry)
#define DASR_CHAIN_LAUNCH(F16_, BWD_, NAME)                                                                                                              \
    {                                                                                                                                                    \
        auto kfn = conv_chain_kernel<F16_, BWD_>;                                                                                                        \
        if (!attr_set[v]) {                                                                                                                              \
            HIP_TRY(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));                                    \
            attr_set[v] = true;                                                                                                                          \
        }                                                                                                                                                \
        DASR_LAUNCH_TAG(NAME, kfn, dim3((unsigned)grid), dim3(256), C::LDS_BYTES, s, dev_layers, (const int*)dev_dep_chunk, (int)nlayers, tiles_y, tiles_x, \
                        dev_flags, dev_flags + grid, dev_err);                                                                                           \
    }
    if (v == 0) DASR_CHAIN_LAUNCH(false, false, "conv_chain_kernel<false, false>")
    else if (v == 1) DASR_CHAIN_LAUNCH(true, false, "conv_chain_kernel<true, false>")
    else if (v == 2) DASR_CHAIN_LAUNCH(false, true, "conv_chain_kernel<false, true>")
    else DASR_CHAIN_LAUNCH(true, true, "conv_chain_kernel<true, true>")
#undef DASR_CHAIN_LAUNCH
    return (int)hipGetLastError();
}

// The chained trunk launch, input-stationary form (rdb_is.h): nlayers = 5 x (dense blocks), layers[5 b + k] = conv k + 1 of block b as dasr_conv would run it.
extern "C" int dasr_rdb_chain(const dasr_conv_params* dev_layers, const dasr_conv_params* host_layers, int32_t nlayers, uint32_t* dev_flags, int32_t* dev_err, void* stream) {
    if (!dev_layers || !host_layers || nlayers <= 0 || nlayers % 5 || !dev_flags || !dev_err) return DASR_EINVAL;
    const dasr_conv_params& p0 = host_layers[0];
    if (p0.prec != 1) return DASR_EINVAL;   // bf16 storage (the f16 dense blocks keep the per-layer launches)
    const int e0 = classify_epi(p0);
    const bool bwd = e0 == 68;
    if (!bwd && e0 != 67) return DASR_EINVAL;
    for (int i = 0; i < nlayers; ++i) {
        const dasr_conv_params& p = host_layers[i];
        const dasr_conv_params& pb = host_layers[i - i % 5];
        const int k = i % 5;
        if (p.kh != 3 || p.stride != 1 || p.pad != 1 || p.in_f32 || p.prec != 1 || p.ups || p.in_wrap || p.out16_lo || p.res1_lo || p.out16_f16) return DASR_EINVAL;
        if (p.Hin != p0.Hin || p.Win != p0.Win || p.Hout != p0.Hin || p.Wout != p0.Win || p.N != p0.N || p.out_stride > 1 || p.in_stride > 1 || p.out_W || p.out_oy || p.out_ox) return DASR_EINVAL;
        if (p.cin != 64 + 32 * k || p.mt != (k == 4 ? 2 : 1) || p.cout != 32 * p.mt || !p.w || !p.in.p || p.slope_ptr || p.mask_f32 || p.prelu_part) return DASR_EINVAL;
        if (p.in.p != pb.in.p || p.in.n_stride != pb.in.n_stride || p.in.cb_stride != pb.in.cb_stride) return DASR_EINVAL;   // one slab per dense block
        const int epi = classify_epi(p);
        // forward: conv1-4 bias + LeakyReLU -> 16-bit planes (67), conv5 bias, alpha, one / two fp32 residuals -> fp32 (+ 16-bit) (233 / 249, 169 / 185);
        // data gradient: LeakyReLU' mask -> 16-bit planes (68), alpha, one / two fp32 residuals -> fp32 (+ 16-bit) (232 / 248, 168 / 184)
        const bool ok = k < 4 ? epi == (bwd ? 68 : 67) : ((epi & ~(16 | 64)) == (bwd ? 168 : 169) && p.res1.p && p.alpha != 0.f);
        if (!ok) return DASR_EINVAL;
    }
    // Geometry: whole images per XCD (N % 8 == 0: image n lives on XCD n % 8), q workgroups per XCD (one per CU, q <= 32), each owning tpw = (tiles per XCD) / q <= 8 tiles --
    // and every tile of an image must be worked on AT THE SAME TIME (a tile waits for its neighbours inside a dense block): the q workgroups of an XCD hold whole images,
    // q % T == 0.  The largest such q is taken: 16 x 128^2 -> q 32, 2 tiles each.  Tile heights 16 (8 waves x 2 rows), 8 (8 x 1), 4 (4 x 1) rows of 32 pixels:
    // a chained launch is a fixed sequence of 34 steps per dense block and tile whatever the tile's height, and its steps get shorter with the tile only down to the latency
    // of the neighbour synchronisation -- so the height is chosen by (tiles a workgroup owns) x (measured chain time of one tile at that height), see below: small images
    // are spread over more CUs (the reference's shipped 16 crops of 32 x 32: 128 workgroups of 4-row tiles), but never at the price of more tiles per workgroup.
    // Measured (profiles/r06_is_chain.txt): 16 x 32 x 32: 8.8 / 6.6 / 6.0 ms per SR step with 16- / 8- / 4-row tiles -- and 6.4 ms with 2-row tiles (2 waves, 256
    // workgroups; built, bit-identical, dropped): below 4 rows the launch is bound by the latency chain store -> flag -> poll -> halo DMA between neighbouring tiles, which
    // more workgroups do not shorten.
    if (p0.N & 7) return DASR_EINVAL;
    const int tiles_x = (p0.Wout + ISC::TW - 1) / ISC::TW;
    auto geometry = [&](int th, int& q_out, int& tpw_out) -> bool {   // workgroups per XCD / tiles per workgroup for tiles of th rows
        const int T = tiles_x * ((p0.Hout + th - 1) / th);
        if (T <= 0 || T > 32) return false;
        const long long per_xcd = (long long)T * p0.N / 8;
        for (int c = 32 - 32 % T; c >= T; c -= T)
            if (per_xcd % c == 0 && per_xcd / c <= ISC::MAX_TPW) {
                q_out = c, tpw_out = (int)(per_xcd / c);
                return true;
            }
        return false;
    };
    // the height that minimises (tiles per workgroup) x (time of one tile's chain at that height: 4.3 / 3.0 / 2.4 ms per 69 dense blocks for 16 / 8 / 4 rows, measured)
    int th = 0, q = 0, tpw = 0, best = 1 << 30;
    for (int cand = 16; cand >= 4; cand >>= 1) {
        int qc = 0, tc = 0;
        if (!geometry(cand, qc, tc)) continue;
        const int cost = tc * (cand == 16 ? 43 : cand == 8 ? 30 : 24);
        if (cost < best) best = cost, th = cand, q = qc, tpw = tc;
    }
    if (!th) return DASR_EINVAL;
    const int grid = 8 * q;
    const int tiles_y = (p0.Hout + th - 1) / th;
    {
        static int n_cu = -1;
        if (n_cu < 0) {
            int dev = 0;
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDevice(&dev));
            HIP_TRY(hipGetDeviceProperties(&prop, dev));
            n_cu = prop.multiProcessorCount;
        }
        if (n_cu != 256) return DASR_EINVAL;
    }
    // (the ticket counters sit behind the flag words of the LARGEST tile count a caller may have to provide for: N x ceil(H / 4) x ceil(W / 32))
    unsigned* tickets = dev_flags + (long long)tiles_x * ((p0.Hout + 3) / 4) * p0.N;
    const int nrdb = nlayers / 5;
    hipStream_t st = as_stream(stream);
#define IS_GO(NTv, NWv)                                                                                                                                              \
    return bwd ? launch_rdb_is<false, true, NTv, NWv>(dev_layers, nrdb, tiles_y, tiles_x, tpw, dev_flags, tickets, dev_err, st, "rdb_is_kernel<false, true, " #NTv ", " #NWv ">", grid) \
               : launch_rdb_is<false, false, NTv, NWv>(dev_layers, nrdb, tiles_y, tiles_x, tpw, dev_flags, tickets, dev_err, st, "rdb_is_kernel<false, false, " #NTv ", " #NWv ">", grid)
    if (th == 16) { IS_GO(2, 8); }
    if (th == 8) { IS_GO(1, 8); }
    IS_GO(1, 4);
#undef IS_GO
}

extern "C" int dasr_conv(const dasr_conv_params* pp, void* stream) {
    dasr_conv_params p = *pp;
    p.xcd_remap = 1;  // bit 0: XCD-aware tile order (bit 1, trace builds only: the contiguous-store timing experiment of conv_epilogue)
    if (p.pad_x == 0 && p.out_stride == 0 && p.kh != 2 && p.kh != 1) p.pad_x = -1;  // zero-initialised extension fields = "same as pad"
    hipStream_t s = as_stream(stream);
    if (p.cin <= 0 || (p.cin & 15) || p.cout <= 0 || !p.w || !p.in.p) return DASR_EINVAL;
    if (!(p.mt == 1 || p.mt == 2) || !(p.prec >= 1 && p.prec <= 4)) return DASR_EINVAL;
    if (p.prec == 4 && (!p.in_f32 || p.mt != 1)) return DASR_EINVAL;   // split-f16: f32 tensors, 32-oc workgroups
    if (p.prec == 2 && !p.in_f32 && (p.kh != 3 || p.stride != 1)) return DASR_EINVAL;   // f16 tensors: dense 3x3 kernel only
    int kcode = 0;
    if (p.kh == 4) kcode = p.stride == 2 ? 2 : 1;
    else if (p.kh == 2) kcode = 3;
    else if (p.kh == 5) kcode = 4;
    else if (p.kh == 1) kcode = 5;
    else if (p.kh == 3 && p.stride == 2) kcode = 6;
    const int key = (p.prec == 4 ? 3000 : p.prec == 3 ? 1000 : p.prec == 2 ? 2000 : 0) + (p.in_f32 ? 100 : 0) + p.mt * 10 + kcode;
    // 3x3: pad 1; the register-staged f32-tensor stride-1 kernel also runs pad 0 / 2 (LPIPS conv1 on the space-to-depth grid and its adjoint)
    if (p.kh == 3 && ((p.stride != 1 && p.stride != 2) || (p.pad != 1 && !(p.pad >= 0 && p.pad <= 2 && p.stride == 1 && p.in_f32)))) return DASR_EINVAL;
    if (p.kh == 5 && (p.stride != 1 || p.pad != 2)) return DASR_EINVAL;
    if (p.kh == 1 && (p.stride != 1 || p.pad != 0)) return DASR_EINVAL;
    if (p.kh == 4 && ((p.stride != 1 && p.stride != 2) || p.pad < 0 || p.pad > 3)) return DASR_EINVAL;
    if (p.kh == 2 && (p.stride != 1 || p.pad < 0 || p.pad > 1)) return DASR_EINVAL;
    if (p.kh < 1 || p.kh > 5) return DASR_EINVAL;
    if (p.mask.p && (p.mask_f32 != 0) != (p.in_f32 != 0)) return DASR_EINVAL;  // mask dtype is tied to the input dtype
    if (p.ups && !p.in_f32 && p.prec != 2) return DASR_EINVAL;
    if (p.ups == 2) return subpix_dgrad(p, s);
    if (p.in_wrap < 0 || p.out16_lo < 0 || p.res1_lo < 0) return DASR_EINVAL;
    if (p.in_wrap || p.out16_lo || p.res1_lo) {   // split 16-bit tensors: the LDS-DMA kernel only (a 16-bit input, 3x3 / stride 1 / pad 1, one-pass precisions)
        if (p.in_f32 || p.kh != 3 || p.stride != 1 || p.pad != 1 || !(p.prec == 1 || p.prec == 2) || p.ups || p.out_stride > 1) return DASR_EINVAL;
        if (p.in_wrap && (p.cin >> 4) * 2 != p.in_wrap * 3) return DASR_EINVAL;   // cin = 3 * 16K virtual channels, in_wrap = 2K
        if (p.out16_lo && !p.out_bf16.p) return DASR_EINVAL;
        if (p.res1_lo < 0 || (p.res1_lo && !p.res1.p)) return DASR_EINVAL;
    }
    switch (key) {
        // prec 1, bf16 input (RDB dense-block convs, fwd and dgrad)
        case 10:
            switch (classify_epi(p)) {
                case 67: return launch_glds<1, 67>(p, s);   // bias + LeakyReLU -> bf16 slab planes (forward conv1-4)
                case 68: return launch_glds<1, 68>(p, s);   // LeakyReLU' mask -> bf16 gslab planes (data gradient)
                default: return launch_glds<1, 0>(p, s);
            }
        case 20:
            // one kernel, two workgroup shapes: 13 (default) = the 8-wave form when the 4-wave grid would not exceed one workgroup per CU
            // (sub-batch launches), else 4 waves; 12 = always 4 waves
            if (g_tune_rdb64 == 12 || (long long)p.N * ((p.Hout + 15) / 16) * ((p.Wout + 31) / 32) * ((p.cout + 63) / 64) > 256) {
                switch (classify_epi(p)) {
                    case 233: return launch_glds<2, 233>(p, s);   // conv5: bias, alpha, one residual -> fp32 stream + bf16 shadow
                    case 249: return launch_glds<2, 249>(p, s);   // conv5 of RDB3: two residuals (RRDB skip fused)
                    case 232: return launch_glds<2, 232>(p, s);   // data gradient w.r.t. the RDB input
                    case 248: return launch_glds<2, 248>(p, s);
                    default: return launch_glds<2, 0>(p, s);
                }
            }
            switch (classify_epi(p)) {
                case 233: return launch_glds<2, 233, 8>(p, s);
                case 249: return launch_glds<2, 249, 8>(p, s);
                case 232: return launch_glds<2, 232, 8>(p, s);
                case 248: return launch_glds<2, 248, 8>(p, s);
                default: return launch_glds<2, 0, 8>(p, s);
            }
        // prec 1, f32 input (VGG perceptual branch)
        case 110: return launch<1, true, 1, 3, 1, 4>(p, s);
        case 120: return launch<1, true, 2, 3, 1, 4>(p, s);
        // prec 3, f32 input (residual-stream convs of the generator, discriminator)
        case 1110: return launch<3, true, 1, 3, 1, 4>(p, s);
        case 1111: return launch<3, true, 1, 4, 1, 2>(p, s);
        case 1112: return launch<3, true, 1, 4, 2, 1>(p, s);
        case 1113: return launch<3, true, 1, 2, 1, 4>(p, s);  // 2x2 parity sub-convs of the stride-2 data-gradient
        case 1114: return launch<3, true, 1, 5, 1, 2>(p, s);  // DSN FSD discriminator 5x5
        case 1115: return launch<3, true, 1, 1, 1, 4>(p, s);  // 1x1 head
        case 1116: return launch<3, true, 1, 3, 2, 1>(p, s);  // De_resnet down-sampling convs
        // prec 2 on f16 TENSORS (HR tail in f16 storage): the LDS-DMA dense-conv kernel with the f16 MFMA
        case 2010:
            switch (classify_epi(p)) {
                case 67: return launch_glds<1, 67, 4, 0, true>(p, s);
                case 68: return launch_glds<1, 68, 4, 0, true>(p, s);
                case 64: return launch_glds<1, 64, 4, 0, true>(p, s);
                default: return launch_glds<1, 0, 4, 0, true>(p, s);
            }
        case 2020:
            // conv5-class epilogues (alpha, residuals -> fp32 stream + 16-bit shadow): the dense blocks in f16 storage (DASR_RDB_PREC=2, rrdbnet.py);
            // same workgroup-shape rule as the bf16 launches
            if (p.res1.p) {
                const bool four = g_tune_rdb64 == 12 || (long long)p.N * ((p.Hout + 15) / 16) * ((p.Wout + 31) / 32) * ((p.cout + 63) / 64) > 256;
                switch (classify_epi(p)) {
                    case 233: return four ? launch_glds<2, 233, 4, 0, true>(p, s) : launch_glds<2, 233, 8, 0, true>(p, s);
                    case 249: return four ? launch_glds<2, 249, 4, 0, true>(p, s) : launch_glds<2, 249, 8, 0, true>(p, s);
                    case 232: return four ? launch_glds<2, 232, 4, 0, true>(p, s) : launch_glds<2, 232, 8, 0, true>(p, s);
                    case 248: return four ? launch_glds<2, 248, 4, 0, true>(p, s) : launch_glds<2, 248, 8, 0, true>(p, s);
                    default: return launch_glds<2, 0, 4, 0, true>(p, s);
                }
            }
            switch (classify_epi(p)) {
                case 67: return launch_glds<2, 67, 4, 0, true>(p, s);
                case 68: return launch_glds<2, 68, 4, 0, true>(p, s);
                case 64: return launch_glds<2, 64, 4, 0, true>(p, s);
                default: return launch_glds<2, 0, 4, 0, true>(p, s);
            }
        // prec 4: split-f16 (hi*hi + hi*lo + lo*hi on f16 pairs, 22-bit operands): the BatchNorm discriminator, where 16 bits are not enough
        case 3110: return launch<4, true, 1, 3, 1, 4>(p, s);
        case 3111: return launch<4, true, 1, 4, 1, 2>(p, s);
        case 3112: return launch<4, true, 1, 4, 2, 1>(p, s);
        case 3113: return launch<4, true, 1, 2, 1, 4>(p, s);
        case 3114: return launch<4, true, 1, 5, 1, 2>(p, s);
        case 3115: return launch<4, true, 1, 1, 1, 4>(p, s);
        case 3116: return launch<4, true, 1, 3, 2, 1>(p, s);
        // prec 2: f16 operands, ONE MFMA pass on f32 activations (HR tail of the generator; VGG / discriminators / DSN when selected)
        case 2110: return launch<2, true, 1, 3, 1, 4>(p, s);
        case 2120: return launch<2, true, 2, 3, 1, 4>(p, s);
        case 2111: return launch<2, true, 1, 4, 1, 2>(p, s);
        case 2112: return launch<2, true, 1, 4, 2, 1>(p, s);
        case 2113: return launch<2, true, 1, 2, 1, 4>(p, s);
        case 2123: return launch<2, true, 2, 2, 1, 4>(p, s);
        case 2114: return launch<2, true, 1, 5, 1, 2>(p, s);
        case 2115: return launch<2, true, 1, 1, 1, 4>(p, s);
        case 2116: return launch<2, true, 1, 3, 2, 1>(p, s);
        default: return DASR_EINVAL;
    }
}

extern "C" int dasr_conv_naive(const dasr_conv_params* pp, const float* w_ref, void* stream) {
    const dasr_conv_params& p = *pp;
    const long long total = (long long)p.N * p.cout * p.Hout * p.Wout;
    if (total <= 0) return DASR_EINVAL;
    DASR_LAUNCH(conv_naive_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), p, w_ref);
    return (int)hipGetLastError();
}

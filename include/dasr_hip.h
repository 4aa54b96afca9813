/*
 * dasr_hip.h -- C ABI of libdasr_hip.so, the MI355X (gfx950) kernels behind the DASR SRN
 * training step (ShuhangGu/DASR, codes/SRN).  Plain pointers and sizes only; no torch types.
 *
 * The reference has NO native/FFI layer: every op below replaces a stock
 * PyTorch op that the reference reaches through nn.Module graphs.  The citation on each entry
 * point names the reference construct whose arithmetic it takes over.
 *
 * Activation layout ("NC16HW16"): T[n][cb][y][x][16], 16 channels innermost, bf16 or f32.
 * A dasr_tensor is a view: base pointer of plane cb=0 of the slice, element strides between
 * images and between 16-channel planes.  H, W travel in the op parameters.
 *
 * All launchers are asynchronous on `stream` (a hipStream_t passed as void*), own no memory,
 * and return 0 on success or a hipError_t / negative DASR_E* code.
 */
#ifndef DASR_HIP_H
#define DASR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DASR_ABI_VERSION 22
#define DASR_EINVAL (-22)
#define DASR_ECAPTURE (-16)   /* a launch needed a device allocation (the scratch row of a deterministic grid sum, first use per accumulator and stream) while its stream was being captured */

typedef struct {
    void*   p;          /* base of plane 0 (device pointer) */
    int64_t n_stride;   /* elements between images */
    int64_t cb_stride;  /* elements between 16-channel planes */
} dasr_tensor;

/* ---- implicit-GEMM convolution, forward and data-gradient ------------------------------------
 * Replaces nn.Conv2d fwd (+bias, +LeakyReLU/ReLU, + residual scale-add) of conv_block
 * (codes/SRN/models/modules/block.py:130-156), the torch.cat of ResidualDenseBlock_5C
 * (block.py:280-286: input = first cin/16 planes of a dense slab, output written into its own
 * planes), nn.Upsample(nearest,2) of upconv_blcok (block.py:854-861, `ups` = 1; its data gradient, `ups` = 2), the 4x4 convs of
 * NLayerDiscriminator (architecture.py:983-1024) and VGG19 convs (architecture.py:1060-1088).
 * The data-gradient of a stride-1 conv is the same op on flipped/transposed packed weights
 * with `mask` = forward activation (LeakyReLU'/ReLU').
 *   v = acc + bias[oc]; if act: v = v>0 ? v : slope*v; if mask.p: v *= (mask>0 ? 1 : slope)
 *   v = alpha*v + beta1*res1 + beta2*res2;  out_f32 = v;  out_bf16 = bf16(gamma*v)
 * Corners (held by tests/test_gpu_conv.py): the mask test is `mask > 0`, so +0 and -0 both take `slope`.  Whole 16-channel planes are written up to
 * ceil(cout/16): the padding channels of the last plane are written as exact zeros whatever bias, mask, res1 and res2 hold at those channels (they
 * are read, never used); input padding channels must hold zeros.  With out_stride = 2 only the addressed parity of the output tensor is written.
 * The conv5-class launches of the LDS-DMA kernel (64 output channels per workgroup, res1 given) evaluate alpha*((beta1/alpha)*res1 + acc): the same
 * value to fp32 rounding, alpha must not be 0 there.
 */
typedef struct {
    dasr_tensor in;  int32_t in_f32;  int32_t Hin, Win;  int32_t ups;  int32_t cin; /* cin % 16 == 0 */
    /* ups: 0 plain conv; 1 the input is nearest-x2 up-sampled on the fly (Hout x Wout = (2 Hin) x (2 Win));
     * 2: the DATA GRADIENT of nearest-x2 + 3x3 (upconv_blcok, block.py:854-861) in its sub-pixel form, one launch: `in` is the f16 gradient on the
     * Hin x Win = (2 Hout) x (2 Wout) grid, the output (and the mask) live on the Hout x Wout grid of the conv's low-resolution input;
     * out[m][n] = sum over parities (py, px) and 2x2 taps (a, b) of Wp[2 py + px][2 a + b] . in[2 (m - py + a) + py][2 (n - px + b) + px], zero outside.
     * `w`: 16 packed taps, 4 (2 py + px) + 2 a + b, each the sum of the transposed 3x3 taps that meet the same gradient pixel (dasr_pack_desc::tapmask).
     * f16 tensors only (in_f32 0, prec 2, kh 3 / stride 1 / pad 1, a 16-bit output is f16, no split tensors).  Epilogue terms: `mask` with the constant
     * `slope`, alpha / gamma, out_f32 and / or the f16 out_bf16 on the dense grid; bias, act, res1 / res2, slope_ptr, prelu_part and a strided output
     * (out_stride, out_oy, out_ox, out_W) are DASR_EINVAL.  (A value of an existing field: the struct and DASR_ABI_VERSION are unchanged.) */
    const void* w;   int64_t w_lo_off;      /* packed bf16 weights (dasr_pack_weights); lo plane offset (elements) for prec 3 */
    const float* bias;                      /* [cout] or NULL */
    int32_t cout, Hout, Wout, N;
    int32_t kh, stride, pad;                /* 3/1/1 or 4/2/1 or 4/1/1; the f32-tensor 3x3 stride-1 conv also takes pad 0 / 2 (LPIPS conv1 and its adjoint) */
    int32_t prec;                           /* 1: bf16 operands; 2: f16 operands, one MFMA pass (f32 input, see in_scale); 3: split-bf16 (hi*hi+hi*lo+lo*hi), ~fp32;
                                             * 4: split-f16 (same three passes on f16 hi/lo pairs of the in_scale'd f32 input: 22-bit operands) */
    int32_t mt;                             /* 32-oc tiles per workgroup (1 or 2); must match the packing */
    int32_t act;  float slope;
    dasr_tensor mask;  int32_t mask_f32;
    float alpha;  dasr_tensor res1;  float beta1;  dasr_tensor res2;  float beta2;
    dasr_tensor out_f32;  dasr_tensor out_bf16;  float gamma;
    int32_t xcd_remap;                      /* set by the library (XCD-aware tile order); callers leave it 0 */
    /* extensions used by the stride-2 data-gradient (four 2x2 parity sub-convolutions writing interleaved sub-grids):
     * pad_x < 0: same as pad; out_stride 0/1: dense output, 2: output pixel (oy,ox) lands at (2*oy+out_oy, 2*ox+out_ox)
     * of a tensor of width out_W (mask / res / out tensors are all indexed at that full-resolution position). */
    int32_t pad_x, out_stride, out_oy, out_ox, out_W;
    /* act: 0 none, 1 (Leaky/P)ReLU with `slope`, 2 sigmoid.  slope_ptr != NULL: slope read from device memory
     * (nn.PReLU's learned parameter, codes/DSN/model.py:29,215), used for `act` and for the `mask` derivative. */
    const float* slope_ptr;
    /* strided INPUT view (sub-pixel data-gradient of nearest-x2 + 3x3: the parity sub-grids of the gradient are read in place):
     * in_stride 0/1: dense; 2: input pixel (y,x) of the Hin x Win grid lives at (2*y+in_oy, 2*x+in_ox) of a tensor of width in_W.
     * conv_kernel variants only (not the LDS-DMA dense-block kernel). */
    int32_t in_stride, in_oy, in_ox, in_W;
    /* prec 2: the f32 input is multiplied by in_scale (a power of two; 0 = 1) before it is rounded to f16, and the accumulator by
     * 1/in_scale before the epilogue: keeps tiny loss gradients (1e-8..1e-5) inside f16's normal range, exact otherwise. */
    float in_scale;
    /* non-zero: the 16-bit output tensor (`out_bf16`) is written as f16 instead of bf16 (activations of the generator's HR tail are
     * kept in f16: 11-bit mantissa, one MFMA pass in the consuming conv, prec 2 with in_f32 = 0) */
    int32_t out16_f16;
    /* SPLIT 16-BIT TENSORS (round 3): a tensor of C channels held as 2K planes of 16-bit elements (K = ceil(C/16)): planes [0, K) the rounded
     * value `hi`, planes [K, 2K) the remainder lo = round16(v - hi) -- 22 (f16) or 16 (bf16) mantissa bits in the same 4 bytes per element as
     * f32, but in the layout the LDS-DMA dense-conv kernel streams.  The split-precision product hi*hi + lo*hi + hi*lo (prec 3 / 4 on f32
     * tensors: three MFMA passes over operands split on the fly) then is ONE launch of that kernel over 3K "virtual" chunks:
     *   in_wrap = 2K, cin = 3 * 16K: chunk c reads plane (c < in_wrap ? c : c - in_wrap) of `in`, i.e. hi, lo, hi again; the weights are
     *   packed as [hi | hi | lo] (dasr_pack_weights fmt 3 / 4).  0: plain tensor.
     *   out16_lo = K' > 0: the 16-bit output is written split: hi into plane cb, lo = round16(gamma * v - hi) into plane cb + K'.
     *   res1_lo = K' > 0: `res1` is a split 16-bit tensor (same element format as the 16-bit output), read as hi + lo.
     * LDS-DMA kernel only (16-bit input, 3x3 / stride 1 / pad 1, prec 1 or 2). */
    int32_t in_wrap, out16_lo, res1_lo;
    /* (ABI 20) non-NULL, 64-channel mask-only data-gradient convs of the LDS-DMA kernel (16-bit input, `mask` a 16-bit tensor in the format of the 16-bit output, no other
     * epilogue term): every workgroup also writes prelu_part[workgroup] = slope * sum over its outputs with mask <= 0 of (conv result * mask) -- the per-workgroup partials
     * of dL/dslope of the nn.PReLU() (one shared slope, codes/DSN/model.py:29,215) whose output the mask is.  The buffer holds >= N * ceil(H/4) * ceil(W/16) floats (one per workgroup of any tile shape the launcher may choose), zero at
     * allocation (entries no workgroup owns stay zero); dasr_prelu_final finishes the sum.  Elsewhere the field must be NULL. */
    float* prelu_part;
} dasr_conv_params;

int dasr_conv(const dasr_conv_params* p, void* stream);
/* A chain of dense-block convs in ONE persistent launch (round 4; replaces the per-layer launches of ResidualDenseBlock_5C / RRDB forward,
 * codes/SRN/models/modules/block.py:254-309, for the trunk of RRDBNet, architecture.py:174-205).  Layer L is dasr_conv(layers[L]) -- same arithmetic,
 * bit-identical results -- but a tile of the image goes from layer to layer inside the launch and waits for its eight neighbour tiles (flags in
 * `flags`, one word per tile, zero at allocation) only before it reads the first input chunk that holds layer L-1's output (dep_chunk[L], in
 * 16-channel chunks; <= 0: every chunk).  Constraints (DASR_EINVAL otherwise): 3x3 / stride 1 / pad 1 on 16-bit tensors of ONE geometry,
 * cout == 32 * mt, the term sets of the dense-block forward (bias + LeakyReLU -> 16-bit planes; bias, alpha, one or two fp32 residuals -> fp32 +
 * 16-bit), N a multiple of 8 (whole images per XCD) and N * tiles == 512 (the launch fills the chip exactly: every workgroup resident, every XCD
 * hosts the tiles of its own images).
 * `flags`: N * tiles + 8 words (the last eight: per-XCD ticket counters).  `err` (device word, zero at allocation): bit 1 a neighbour wait gave
 * up -- the results are then not valid (pass the word to dasr_adam as gate_flag: such a step then never reaches the weights).
 * What the kernels rely on in `flags` (both forms; held by tests/test_gpu_chain.py), beyond "zero at allocation":
 *   - The words COUNT ON from launch to launch: a launch of nlayers layers leaves every tile word it owns nlayers higher (layer L of a tile publishes
 *     start + L + 1) and every ticket word higher by the launch's workgroups per XCD (64 here, q in the input-stationary form); nothing is reset, and the
 *     caller never writes the buffer between launches.  Every comparison is a signed difference, (int)(word - target) < 0: the tile words may wrap 2^32.
 *   - ALL TILE WORDS A LAUNCH USES ARE EQUAL WHEN IT STARTS (the first N * tiles words of the buffer).  A tile reads its own word as its start value and compares its eight neighbours' words with targets
 *     counted from that value, never from theirs: a neighbour whose word starts higher looks finished before it has begun (its halo is read too early), one
 *     that starts lower is waited for until the wait gives up.
 *   - A workgroup takes tile (ticket % workgroups per XCD) of its XCD: within a launch the tickets of an XCD must be that many CONSECUTIVE integers.  Counters
 *     that only launches of one geometry have advanced are a multiple of that number and are never touched by two launches at a time; where the number is not a
 *     power of two (input-stationary form, q = 18, 27, ...) a counter must not pass 2^32 (2^32 / 32 launches of one buffer at the least).
 *   - So a flag buffer belongs to the launches of ONE geometry (N, H, W and form: another one owns another set of tile words, which the first has left
 *     unequal to the rest, and keeps its ticket words elsewhere -- behind 512 tile words here, behind N * ceil(H / 4) * ceil(W / 32) in the input-stationary
 *     form), one launch at a time.  engine.ConvChain allocates one buffer per chain (rrdbnet.py: every forward and data-gradient chain of a plan its own).
 * OPERATIONAL CONTRACT: the launch needs the device to itself -- a whole 256-CU MI355X (no CPX / DPX partition), no other process on it, and no
 * other kernel of this process in flight on another stream (a collective's kernels on a communication stream included) while it runs: all 512
 * workgroups must be resident at once, 64 per XCD.  See INTEGRATION.md "Chained launches: operational contract".
 * dev_layers / dev_dep_chunk: device copies the kernel reads; host_layers: the same blocks in host memory (validated by the launcher). */
int dasr_conv_chain(const dasr_conv_params* dev_layers, const dasr_conv_params* host_layers, const int32_t* dev_dep_chunk, int32_t nlayers,
                    uint32_t* dev_flags, int32_t* dev_err, void* stream);
/* The same chain, INPUT-STATIONARY form (round 6; replaces ResidualDenseBlock_5C.forward, codes/SRN/models/modules/block.py:280-286, and its data
 * gradient, for the whole trunk of RRDBNet, architecture.py:174-205, in one launch).  layers[5 b + k], k = 0..4, are the five convs of dense block b
 * exactly as dasr_conv would run them (cin = 64 + 32 k on ONE slab, cout 32 / 32 / 32 / 32 / 64; forward: bias + LeakyReLU -> 16-bit planes, conv5 bias,
 * alpha, one or two fp32 residuals -> fp32 stream (+ 16-bit planes of the next slab, may be absent on the last block); data gradient: LeakyReLU' mask ->
 * 16-bit planes, alpha, residuals -> fp32 (+ 16-bit)) -- bit-identical results -- but every 16-channel chunk of the slab is staged in LDS ONCE and
 * multiplied into the accumulators of every conv of the block that consumes it (12 chunks per block and tile instead of 40), one workgroup of 8 waves per
 * CU.  Geometry: tiles of 16, 8 or 4 rows x 32 pixels (8 waves x 2 rows, 8 x 1, 4 x 1), T per image; image n on XCD n % 8; q workgroups per XCD (the largest multiple of
 * T that is <= 32, divides the N T / 8 tiles of an XCD and leaves at most 8 tiles per workgroup), i.e. a launch of 8 q <= 256 workgroups (csrc/rdb_is.h); the launcher takes
 * the height that minimises (tiles per workgroup) x (measured chain time of one tile at that height).  Constraints (DASR_EINVAL otherwise): bf16 storage, nlayers a multiple
 * of 5, N a multiple of 8, T <= 32 and such a q exists for one of the heights (16 x 128^2: 16 rows, q 32, two tiles each; 8 x 128^2: 16 rows, one tile; 16 crops of
 * 32 x 32: 4 rows, q 16).  flags: N * ceil(H / 4) * ceil(W / 32) + 8 words, zero at allocation (sized for the finest tiles whichever height runs; the last eight: per-XCD
 * ticket counters; a launch leaves the words of the tiles of the height that ran 5 higher per dense block, the words behind them as they were, the tickets q higher: see
 * dasr_conv_chain for what the kernel relies on); err / operational contract: as dasr_conv_chain (the launch needs all 256 CUs of the device to itself: up to 256 workgroups with 160 KB of LDS each, all
 * resident). */
int dasr_rdb_chain(const dasr_conv_params* dev_layers, const dasr_conv_params* host_layers, int32_t nlayers, uint32_t* dev_flags, int32_t* dev_err,
                   void* stream);
/* ---- fused residual block (ABI 21, csrc/resblock.hip) -----------------------------------------------
 * Replaces ResNetBlock in mode CNA (codes/SRN/models/modules/block.py:221-251: conv0 -> ReLU -> conv1, x + res_scale * res) of SRResNet
 * (architecture.py:18-48) in ONE launch: y = x + res_scale * (conv1(act(conv0(x) + b0)) + b1) for nf = 64, 3x3, stride 1, zero padding.
 * Operands are the bf16 shadow x16 (MFMA operands) and the fp32 stream x32 (the skip); the outputs are the fp32 stream y32 and its bf16 shadow
 * y16; w0 / w1 are packed as the forward dasr_conv of the same conv (dasr_pack_weights: cout 64, cin 64, 9 taps, mt 2, prec 1).  A workgroup
 * computes h = bf16(act(conv0 + b0)) for its 16 x 16 output tile plus a one-pixel halo into LDS (halo pixels outside the image are ZERO: conv1's
 * zero padding of h), then conv1 from there.  The MFMA shape and k order are those of dasr_conv, so h, y32 and y16 are bit-identical to the
 * two-launch composition dasr_conv(act = 1, slope) -> h, dasr_conv(res1 = x32, alpha = res_scale, beta1 = 1) -> y32 / y16.
 * h.p != NULL (training): the interior of h (bf16, 64 channels) is also stored -- the ReLU mask of conv0's data gradient and the input of
 * conv1's weight gradient; NULL (inference): not.  act: `slope` as dasr_conv's act = 1 (0: ReLU).  All tensors NC16HW16, 64 channels, N x H x W. */
typedef struct {
    dasr_tensor x16;  dasr_tensor x32;      /* block input: bf16 shadow, fp32 stream */
    const void* w0;  const float* b0;       /* conv0 (res.0): packed bf16 weights, bias [64] */
    const void* w1;  const float* b1;       /* conv1 (res.2) */
    dasr_tensor y32;  dasr_tensor y16;      /* block output: fp32 stream, bf16 shadow.  y32, y16 and h must not overlap each other or an input
                                             * (a tile reads its neighbours' input halo): DASR_EINVAL */
    dasr_tensor h;                          /* bf16 h = act(conv0(x) + b0), training only (p == NULL: not stored) */
    int32_t N, H, W;
    float res_scale, slope;
} dasr_resblock_params;
int dasr_resblock(const dasr_resblock_params* p, void* stream);

/* kernel-variant knob (bench.py --sweep / --tune).  key 2: workgroup shape of the Cout = 64 dense-block convs: 13 (default) = the 8-wave 32x32-tile
 * form when the 4-wave grid has <= 256 workgroups, else 4 waves; 12 = always 4 waves.  Keys 1 / 3 / 4 / 5 / 6 accept only their fixed values 12 / 0 / 1 / 1 / 0
 * (one dense-block conv kernel, one stream conv, XCD-aware tile order, compile-time specialised epilogues, no chunk-order rotation); anything else: DASR_EINVAL.
 * (round 3: the Cout-32 dense-block convs store their output `sc1`, written through -- measured with a run-time switch, now compile time.) */
int dasr_set_tuning(int32_t key, int32_t value);

/* ---- weight gradient ---------------------------------------------------------------------------
 * Replaces autograd's convolution_backward (weight, bias) for the convs above.  One launch covers
 * a list of `parts` (each: one 32-oc tile x up to two 32-cin tiles x all taps of one conv) times
 * `nsplit` pixel splits; partial sums go to a workspace, dasr_wgrad_reduce sums them
 * deterministically into the flat gradient buffer in the reference layout [cout][cin][kh][kw].
 */
typedef struct {
    dasr_tensor g;   int32_t g_f32;         /* output-gradient, planes starting at this part's oc tile */
    dasr_tensor in;  int32_t in_f32;        /* layer input, planes starting at this part's first cin tile */
    int32_t ups;                            /* input is nearest-x2 upsampled on the fly */
    int32_t n_ctiles;                       /* 1 or 2 valid 32-cin tiles */
    int32_t g_planes, in_planes;            /* 16-ch planes that really exist (g: 1..2, in: 1..4); the rest reads as zero */
    int32_t Hin, Win, Hout, Wout, N;
    int32_t kh, stride, pad;
    int32_t want_bias;                      /* this part also accumulates sum_p g[oc] */
    int64_t ws_off;                         /* float offset into workspace: [nsplit][taps of the part][32][64] (+ bias [nsplit][32]) */
    int64_t ws_bias_off;
    int32_t tap0;                           /* first tap of this part (5x5 kernels are split into parts of <= 10 taps) */
    float g_scale;                          /* f16 staging (f32 & 2): g is multiplied by g_scale (power of two, 0 = 1) before rounding; the caller folds
                                             * 1/g_scale into dasr_wgrad_reduce's scale */
} dasr_wgrad_part;

/* f32 bit 0: g and in tensors of ALL parts are f32 (rounded while staging) instead of bf16; bit 1: ... rounded to f16 (11-bit mantissa,
 * g pre-scaled by part.g_scale) and multiplied with v_mfma_f32_32x32x16_f16 instead of bf16.
 * kh = 33 selects the 6-wave 3x3 kernel: a part is one 64-channel input block x up to three 32-oc tiles
 * (g_planes = 2/4/6), workspace [split][tap][3][32][64], bias [split][96]. */
int dasr_wgrad(const dasr_wgrad_part* parts_dev, int32_t nparts, int32_t nsplit, int32_t kh, int32_t stride, int32_t f32,
               float* ws, void* stream);
/* bit 0: 1 = ds_read_b64_tr_b16 gathers, 0 = scalar LDS gathers (dasr_probe_tr16 sets it from the device); any other bit: DASR_EINVAL. */
int dasr_wgrad_set_mode(int32_t use_tr);

typedef struct {
    int64_t ws_off;  int64_t ws_bias_off;  int32_t nsplit;  int32_t ntaps;
    int32_t oc0, c0;                        /* tile origin inside the conv */
    int32_t cout, cin, n_ctiles;            /* real (unpadded) sizes of the conv */
    int64_t dst_w_off;  int64_t dst_b_off;  /* float offsets into the flat grad buffer; dst_b_off < 0: no bias */
    int32_t flip_io;                        /* reserved */
    /* workspace strides (floats); 0 = the 4-wave layout [split][tap][32][64] / bias [split][32] */
    int64_t split_stride, tap_stride, bias_stride;
    int32_t tap0, ntaps_total;              /* part covers taps [tap0, tap0+ntaps) of a kernel with ntaps_total taps (0: = ntaps) */
    int32_t bias_nsplit, reserved_;         /* splits that carry a bias partial (0: = nsplit).  Split-operand weight gradients (three wgrad parts
                                             * g.x, g.x_lo, g_lo.x laid out as 3 * nsplit consecutive splits) sum the bias over the first nsplit only */
} dasr_wgrad_reduce_part;

/* few_splits != 0 (ABI 17): the caller guarantees nsplit <= 4 and ntaps <= 16 for EVERY part (the grouped dense-block launches): one workgroup per
 * output channel is launched instead of four (same results; the other three only returned). */
int dasr_wgrad_reduce(const dasr_wgrad_reduce_part* parts_dev, int32_t nparts, const float* ws, float* grad_flat,
                      float scale, int32_t few_splits, void* stream);

/* ---- weight packing ------------------------------------------------------------------------------
 * fp32 master weights (reference layout [cout][cin][kh][kw], nn.Conv2d) -> bf16 MFMA-fragment order
 * [mgroup][chunk][tap][mt][lane][8] (+ lo plane for prec 3).  A packed conv is assembled from up to
 * 5 source segments so that the dense-block data-gradient (transposed, tap-flipped, concatenated
 * over the later convs of the block) is just another packed conv.
 */
typedef struct {
    int64_t src_off;      /* float offset of the source conv weight in the flat param buffer */
    int32_t src_cout, src_cin;
    int32_t cin_start, cin_len;   /* range of packed input channels fed by this segment */
    int32_t src_c0;       /* fwd: source cin offset; bwd: source cin (= packed oc) offset */
    int32_t transpose;    /* 0: W[oc][src_c0+ci][tapmap[t]];  1: W[ci][src_c0+oc][tapmap[t]] */
} dasr_pack_seg;

typedef struct {
    int64_t dst_off;      /* bf16 element offset of the hi plane; lo plane at dst_off + lo_off */
    int64_t lo_off;       /* 0 when prec 1 */
    int32_t cout, cin_pad, ntaps, mt, nseg;
    int32_t src_ntaps;    /* taps of the source weight (kh*kw of the nn.Conv2d) */
    int32_t fmt;          /* 0: bf16 (hi plane, + lo plane when lo_off != 0); 1: f16 (prec 2 convs); 2: f16 hi + f16 lo planes (prec 4);
                           * 3 (f16) / 4 (bf16): cin_pad = 3 * 16K virtual channels [hi | hi | lo] of 16K real ones, one plane (split 16-bit tensors,
                           * dasr_conv_params::in_wrap; segments address the real channels) */
    int8_t  tapmap[32];   /* packed tap -> source tap (identity: forward; reversed: stride-1 dgrad; parity subset: stride-2 dgrad) */
    uint16_t tapmask[16]; /* non-zero: packed tap t (< 16) = SUM of the source taps whose bits are set (sub-pixel form of nearest-x2 + 3x3) */
    dasr_pack_seg seg[5];
} dasr_pack_desc;

/* piece_prefix_dev[ndesc+1]: cumulative count of 16-byte output pieces (= mgroups*chunks*ntaps*mt*64 per desc) */
int dasr_pack_weights(const dasr_pack_desc* descs_dev, int32_t ndesc, int64_t total_pieces, const int64_t* piece_prefix_dev,
                      const float* params_flat, void* packed, void* stream);

/* ---- elementwise / reductions --------------------------------------------------------------------*/
/* NCHW f32 [N][C][H][W] (reference tensor layout at the trainer boundary) <-> NC16HW16 f32 (+ optional bf16 copy) */
int dasr_nchw_to_blocked(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor dst_f32,
                         dasr_tensor dst_bf16, void* stream);
int dasr_blocked_to_nchw(dasr_tensor src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, void* stream);

/* L1 pixel loss of SRModel (codes/SRN/models/SR_model.py:80) / DASR_Model (DASR_model.py:212-222):
 *   loss_acc[0] += coef * sum wm*|sr - hr|,   grad (blocked f32, zero beyond C) (+)= coef * wm * sign(sr - hr)
 * coef = weight / element count is computed by the caller; `weight_map` (NCHW [N][1][H][W]) is the optional
 * domain-distance map of the multiweights pixel loss (DASR_model.py:213-215).
 * accumulate bit 0: grad += instead of grad =; bit 1: squared error (nn.MSELoss, pixel_criterion 'l2', SR_model.py:33-36):
 * loss_acc[0] += coef * sum wm*(sr - hr)^2, grad (+)= 2 coef wm (sr - hr);
 * bit 2 (round 6; not with bit 0): `grad` is an f16 tensor and receives f16(grad_scale * g) -- the generator's f16 HR tail takes dL/dSR in that form (a power-of-two
 * pre-scale keeps it inside f16's range); only the 4-channel groups that hold a real channel are written.  grad_scale 0 = 1. */
int dasr_l1_loss(dasr_tensor sr, const float* hr_nchw, const float* weight_map, int32_t N, int32_t C, int32_t H, int32_t W,
                 float coef, float* loss_acc, dasr_tensor grad, int32_t accumulate, float grad_scale, void* stream);

/* backward of nn.Upsample(nearest,2) (block.py:857): dst[y][x] = sum of the 2x2 block of src (Hs=2H, Ws=2W);
 * optional LeakyReLU' mask (mask>0 ? 1 : slope) from the forward activation at the low resolution. */
int dasr_downsum2x(dasr_tensor src, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor mask, int32_t mask_f32,
                   float slope, dasr_tensor dst_f32, dasr_tensor dst_bf16, void* stream);

/* f16 storage of the generator's HR tail: y (f16, blocked) = f16(scale * x) of a blocked f32 tensor (dL/dSR -> pre-scaled f16 gradient), and
 * the backward of nn.Upsample(nearest,2) on f16 tensors: dst = out_scale * mask' * (2x2 block sum of src); dst_f32 and/or dst_f16 */
int dasr_cvt_f16(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, float scale, dasr_tensor y, void* stream);
/* split 16-bit copy (dasr_conv_params::in_wrap): y planes [0, K) = round16(scale * x), planes [K, 2K) = round16(scale * x - hi); f16 != 0: IEEE half, else bfloat16 */
int dasr_cvt_split16(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, float scale, dasr_tensor y, int32_t f16, void* stream);
/* y (f32) = x - f16(scale * x) / scale on a blocked f32 tensor: the part of x an f16 operand rounding drops.  Used to run the weight gradients of
 * the BatchNorm discriminators (Discriminator_VGG_128 architecture.py:442-495, FSD-Batch codes/DSN/model.py:176-189) with 22-bit operands on the
 * f16 MFMA: dW = g.x + g.x_lo + g_lo.x as three parts of one dasr_wgrad launch (their D gradients were 1.3e-2 off an fp64 run). */
int dasr_f16_residual(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, float scale, dasr_tensor y, void* stream);
int dasr_downsum2x_f16(dasr_tensor src, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor mask /* f16, optional */, float slope,
                       float out_scale, dasr_tensor dst_f32, dasr_tensor dst_f16, void* stream);

/* nn.PixelShuffle(2) of pixelshuffle_block (codes/SRN/models/modules/block.py:838-851) on f16 blocked tensors: src has C4 = 4 C channels at H x W,
 * dst C channels at 2H x 2W, dst[c][2y+dy][2x+dx] = src[4c+2dy+dx][y][x]; and its adjoint with the LeakyReLU' of the (activated) src as mask */
int dasr_pixel_shuffle_f16(dasr_tensor src, int32_t N, int32_t C4, int32_t H, int32_t W, dasr_tensor dst, void* stream);
int dasr_pixel_unshuffle_f16(dasr_tensor gsrc, dasr_tensor mask /* f16 [C4 @ HxW], optional */, float slope, int32_t N, int32_t C4, int32_t H,
                             int32_t W, dasr_tensor gdst, void* stream);

/* out = a*x + b*z (z optional) over blocked f32 tensors, optional bf16 copy scaled by gamma
 * (ShortcutBlock / RRDB residual bookkeeping, block.py:97-105,305-309).  Like the two down-sums, it works on whole 16-channel planes:
 * the padding channels of the last plane are computed like real ones (zero in, zero out). */
int dasr_axpby(dasr_tensor x, float a, dasr_tensor z, float b, int32_t N, int32_t C, int32_t H, int32_t W,
               dasr_tensor out_f32, dasr_tensor out_bf16, float gamma, dasr_tensor mask /* optional (P)ReLU' mask, f32 */, float slope,
               const float* slope_ptr, void* stream);

/* torch.optim.Adam step (DASR_model.py:129-143; SR_model.py:50-51) on flat fp32 buffers:
 * g += wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * nonfinite_flag (optional, device int): bit 0 is OR-ed in when any gradient element is inf / NaN (the update itself is what torch would do);
 * the trainers read it with their lazily synchronised log and raise -- e.g. an overflow of the f16-stored HR-tail gradients (DASR_HR_PREC=3
 * keeps that tail in split-bf16 on f32 tensors).
 * gate_flag (optional, device int; ABI 17): when the word is non-zero the launch changes NOTHING (weights and moments untouched).  The trainers pass the
 * error word of the generator's chained trunk launches (dasr_conv_chain `err`): gradients computed behind a broken neighbour wait never reach the
 * weights; the host raises at its next synchronisation point (log interval, checkpoint). */
int dasr_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int32_t step, int32_t* nonfinite_flag, const int32_t* gate_flag, void* stream);

int dasr_fill_f32(float* p, int64_t n, float value, void* stream);
/* y += x over flat fp32 buffers (sum of the gradient buffers of concurrently processed sub-batches) */
int dasr_add_flat(float* y, const float* x, int64_t n, void* stream);


/* ---- GAN-step kernels (csrc/gan.hip) ---------------------------------------------------------------------*/
/* nn.InstanceNorm2d(affine=False, eps) + LeakyReLU of NLayerDiscriminator (architecture.py:1003-1015), fused;
 * stats[N][Cpad][2] = (mean, rstd).  Backward takes the saved forward output a and dL/da, returns dL/dx.
 * Contracts of the InstanceNorm group (these two, dasr_inorm_lrelu_jvp, dasr_inorm_second):
 *  - padding channels: whole 16-channel planes are processed, the padding channels of the last plane like real ones -- zero in, zero out: with zeros
 *    in the padding channels of every input tensor (and of `out` when accumulating) every output holds exact zeros there; stats holds (0, 1/sqrt(eps)).
 *  - the three kernels that read the saved output recover xhat = a > 0 ? a : a / slope and LeakyReLU' = a > 0 ? 1 : slope: at a == +0 and a == -0 the
 *    slope branch (xhat = 0, derivative `slope`, as autograd has it).  They divide by slope: slope <= 0 is DASR_EINVAL (the forward takes any slope).
 *  - stats of the forward may be null (not written); every other pointer and tensor is required.
 *  - DASR_EINVAL, nothing launched: N, C, H or W <= 0; a required tensor or pointer null; slope <= 0 (bwd / jvp / second). */
int dasr_inorm_lrelu_fwd(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, float eps, float slope, dasr_tensor y,
                         float* stats, void* stream);
int dasr_inorm_lrelu_bwd(dasr_tensor a, dasr_tensor ga, int32_t N, int32_t C, int32_t H, int32_t W, float slope,
                         const float* stats, dasr_tensor gx, void* stream);
/* Second-order pieces for the DSN's --wgan gradient penalty (codes/DSN/train.py:231-236: torch.autograd.grad(..., create_graph=True) through the
 * discriminator and the backward of that).  InstanceNorm's Jacobian is symmetric, J t = rstd (t - mean t - xhat mean(xhat t)):
 * dasr_inorm_lrelu_jvp: forward-mode tangent  out = lrelu'(a) * J t  (a = saved forward output, t = tangent of the conv output);
 * dasr_inorm_second: adjoint of z -> J(z) t for fixed t, upstream w = lrelu'(a) * ga:
 *   out (+)= -rstd^2 [ xhat (mean(w t) - mean w mean t - 3 mean(w xhat) mean(xhat t)) + mean(xhat t) (w - mean w) + mean(w xhat) (t - mean t) ];
 * dasr_grad_penalty: nrm = ||g||_2 over the C (<= 16) real channels of ALL images, out3 (FOUR floats) = {nrm, weight (nrm - 1)^2, 2 weight (nrm - 1) / nrm, -},
 *   loss_acc[0] += the penalty; part256 = 256 floats of scratch (deterministic two-stage sum).  stage 0 / world 1: all of it.  Data parallel (the
 *   reference's norm is over the global batch): stage 1 leaves the local sum of squares in out3[3], the caller SUM-all-reduces that word, stage 2 finishes
 *   with nrm^2 = out3[3] / world^2 and out3[2] scaled by 1 / world (the reverse pass's weight-gradient reductions carry the other 1 / world; the ranks' gradients are summed);
 * dasr_fill_scaled: x = factor * scalar[0] on the C real channels (a constant upstream gradient whose value was computed on the device). */
int dasr_inorm_lrelu_jvp(dasr_tensor a, dasr_tensor t, int32_t N, int32_t C, int32_t H, int32_t W, float slope, const float* stats, dasr_tensor out, void* stream);
int dasr_inorm_second(dasr_tensor a, dasr_tensor t, dasr_tensor ga, int32_t N, int32_t C, int32_t H, int32_t W, float slope, const float* stats,
                      dasr_tensor out, int32_t accumulate, void* stream);
int dasr_grad_penalty(dasr_tensor g, int32_t N, int32_t C, int32_t H, int32_t W, float weight, float* part256, float* out3, float* loss_acc, int32_t stage,
                      int32_t world, void* stream);
int dasr_fill_scaled(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, const float* scalar, float factor, void* stream);
/* nn.BatchNorm2d in TRAINING mode (batch statistics, affine gamma / beta) + LeakyReLU of Discriminator_VGG_128 (architecture.py:442-495), fused.
 * The N images are normalised in groups of `group` consecutive images with their own statistics (the reference runs the discriminator on the
 * fake and the real half in separate calls, DASR_model.py:251,288-289).  stats[N/group][Cpad][3] = (mean, rstd, biased variance).
 * Backward recomputes xhat / z from the saved conv output x: gx per group; dgamma / dbeta (optional, both or none) = pscale * sums over all groups.
 * dasr_bnorm_running: running_mean / running_var (unbiased, `count` = elements per channel of the group; count 1: the biased value) / num_batches_tracked
 * (optional; += 1) after one forward on group g (row g of stats).
 * Contracts of the BatchNorm group (the forward, the backward, dasr_bnorm_lrelu_jvp, dasr_bnorm_second):
 *  - groups: N need not be a multiple of `group`; the last group then holds the N % group remaining images, with statistics (and counts) of its own:
 *    stats has ceil(N / group) rows of Cpad entries, row g for the images [g * group, min(N, (g + 1) * group)).
 *  - padding channels: gamma, beta, dgamma and dbeta hold C entries; the kernels mask per channel (c < C), read gamma / beta below C only and take
 *    them as 0 from C on.  The padding channels of the inputs may hold any values for which xhat = (x - mean) rstd and the group sums stay finite in
 *    fp32 (an overflow there would meet the 0 of gamma as inf * 0): the outputs then hold zeros there (accumulating: what they held),
 *    dgamma / dbeta are not written from C on; the padding entries of a stats row are written by the forward and carry no meaning.
 *  - LeakyReLU' is read from the sign of z = gamma xhat + beta, recomputed in fp32 from the saved x and the stats row: z <= 0 (both zeros) is the
 *    slope branch.  Any slope is accepted (nothing divides by it).
 *  - optional pointers: dgamma and dbeta of the backward (both or none), dgamma of dasr_bnorm_second, num_batches_tracked; everything else is required.
 *  - DASR_EINVAL, nothing launched: N, C, H, W or group <= 0; a required tensor or pointer null; only one of dgamma / dbeta given; dasr_bnorm_running:
 *    g < 0, C <= 0 or count <= 0. */
int dasr_bnorm_lrelu_fwd(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t group, float eps, float slope, const float* gamma,
                         const float* beta, dasr_tensor y, float* stats, void* stream);
int dasr_bnorm_lrelu_bwd(dasr_tensor x, dasr_tensor ga, int32_t N, int32_t C, int32_t H, int32_t W, int32_t group, float slope, const float* gamma,
                         const float* beta, const float* stats, dasr_tensor gx, float* dgamma, float* dbeta, float pscale, void* stream);
/* Second-order pieces of BatchNorm2d (training mode) + LeakyReLU for `--wgan` with `--norm_layer Batch` (ABI 19; codes/DSN/train.py:231-236 through
 * model.py:136-160,176-189): the InstanceNorm pair above with group means, gamma behind the normalisation and lrelu' read from y = gamma xhat + beta
 * (x = saved conv output).  dasr_bnorm_lrelu_jvp: out = lrelu'(y) gamma r (t - mean t - xhat mean(xhat t)).  dasr_bnorm_second (u = lrelu'(y) ga, w = gamma u):
 * out (+)= -r^2 [xhat (mean(w t) - mean w mean t - 3 mean(w xhat) mean(xhat t)) + mean(xhat t) (w - mean w) + mean(w xhat) (t - mean t)];
 * dgamma (optional; += when `accumulate`) = pscale * sum u xhat_dot -- the tangent output is linear in gamma; beta has no term. */
int dasr_bnorm_lrelu_jvp(dasr_tensor x, dasr_tensor t, int32_t N, int32_t C, int32_t H, int32_t W, int32_t group, float slope, const float* gamma,
                         const float* beta, const float* stats, dasr_tensor out, void* stream);
int dasr_bnorm_second(dasr_tensor x, dasr_tensor t, dasr_tensor ga, int32_t N, int32_t C, int32_t H, int32_t W, int32_t group, float slope,
                      const float* gamma, const float* beta, const float* stats, dasr_tensor out, int32_t accumulate, float* dgamma, float pscale,
                      void* stream);
int dasr_bnorm_running(const float* stats, int32_t g, int32_t C, int32_t count, float momentum, float* running_mean, float* running_var,
                       float* num_batches_tracked, void* stream);
/* GANLoss('vanilla') = BCEWithLogitsLoss vs a constant target (loss.py:8-40): loss_acc += coef*sum(bce),
 * score_acc += score_coef*sum(x) (the disc_Score log), grad = gcoef*(sigmoid(x)-target) on the C (1..16) real channels of plane 0, zero on the
 * others (the padding channels of x are never read).  loss_acc, score_acc and grad are optional, each on its own.  DASR_EINVAL: N * H * W <= 0,
 * C outside 1..16, x null, (dasr_gan_loss) gan_type outside 0..2. */
int dasr_bce_logits(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, float target, float coef, float gcoef,
                    float* loss_acc, float* score_acc, float score_coef, dasr_tensor grad, void* stream);
/* GANLoss(gan_type) (loss.py:8-40; DASR_model.py:35): gan_type 0 'vanilla' (= dasr_bce_logits), 1 'lsgan' (MSELoss: (x-target)^2, grad
 * gcoef*2(x-target)), 2 'wgan-gp' (-x when target is the real label (> 0.5), +x otherwise; the reference builds but never applies its
 * gradient penalty, DASR_model.py:114-118).  Accumulators and grad as in dasr_bce_logits. */
int dasr_gan_loss(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t gan_type, float target, float coef, float gcoef,
                  float* loss_acc, float* score_acc, float score_coef, dasr_tensor grad, void* stream);
/* relativistic average GAN loss (`ragan: true`, DASR_model.py:240-244,273-275): a, b = logit maps [N][1][H][W] of the two halves,
 *   L = coef * sum_{n,p} [ bce(a - mean_n(b), ta) + bce(b - mean_n(a), tb) ],  means per pixel over the GLOBAL batch (n_glob >= N samples).
 * Three stages so that data-parallel ranks can all-reduce (SUM) the two tiny per-pixel buffers in between (2*H*W floats each):
 *   stage 0: sums = [sum_n a ; sum_n b];   stage 1: loss_acc += coef * local loss, score_a/b += score_coef * sum a / b,
 *   part = [sum_n (sigmoid(za) - ta) ; sum_n (sigmoid(zb) - tb)];   stage 2: ga / gb (optional) = gcoef * d(sum)/da, /db incl. the mean terms
 * form 0: the SRN form above (score = mean logit); form 2 / 3: the same with the GANLoss('lsgan') / ('wgan-gp') term instead of bce.  form 1: the DSN's `--ragan` (codes/DSN/train.py:221-223, model.py:98-106, loss.py:11-41):
 *   term(z, t) = -log(sigmoid(z) + eps) for t > 0.5, -log(1 - sigmoid(z) + eps) for 0 <= t <= 0.5, absent for t < 0; score = mean sigmoid(z). */
int dasr_ragan(dasr_tensor a, dasr_tensor b, int32_t N, int32_t H, int32_t W, int32_t stage, int32_t n_glob, int32_t form, float ta, float tb,
               float coef, float gcoef, float eps, float* sums, float* part, float* loss_acc, float* score_a, float* score_b, float score_coef,
               dasr_tensor ga, dasr_tensor gb, void* stream);
/* Haar DWT level 1 as used by DASR_Model.wavelet_s (DASR_model.py:442-452) on C (1..5) channels of plane 0 of x ([N][C][2 H2][2 W2] fp32; H2, W2 =
 * output size): over each block [[a, b], [c, d]]  LL = (a+b+c+d)/2 -> ll (C channels), LH = (a+b-c-d)/2, HL = (a-b+c-d)/2, HH = (a-b-c+d)/2 -> hc
 * ([LH | HL | HH], 3C channels).  norm bits: bit 0: LL * 0.5, bands * 0.5 + 0.5; bit 1: the 'sum' format of the DSN discriminator
 * (codes/DSN/model.py:113-114), hc = (LH + HL + HH) / 3 in C channels (taken after bit 0); bit 2: the linear part only (bit 0 without its + 0.5: the
 * tangent of the normalised bands).  ll or hc may be null (not computed), not both.  Every output given is written on all 16 channels of plane 0:
 * zero from channel C on (ll) / from channel 3C on, C with bit 1 (hc); channels of x from C on are never read; no other plane is touched.
 * dasr_dwt_bwd is the adjoint of the linear part: gx (+)= DWT^T (gll, ghc), with the same norm bits (bit 2 changes nothing); gll or ghc may be null
 * (taken as zero), not both.  accumulate 0: plane 0 of gx is written on all 16 channels, zero from channel C on; accumulate != 0: channels below C
 * are added to, the others keep their bits.
 * DASR_EINVAL: N * H2 * W2 <= 0, C outside 1..5, x / gx null, both outputs / both inputs null. */
int dasr_dwt_fwd(dasr_tensor x, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t norm, dasr_tensor ll, dasr_tensor hc, void* stream);
int dasr_dwt_bwd(dasr_tensor gll, dasr_tensor ghc, int32_t N, int32_t C, int32_t H2, int32_t W2, int32_t norm, dasr_tensor gx,
                 int32_t accumulate, void* stream);
/* depthwise k x k low-pass (GaussianFilter / AvgPool2d of FilterLow/FilterHigh, architecture.py:1177-1243) on C (1..4) channels of plane 0, k odd,
 * w = [k][k] fp32 on the device: cross-correlation with zero padding r = (k - 1) / 2, low(x)[y][x] = sum w[ky][kx] * x[y + ky - r][x + kx - r].
 * mode bit 1 set: normalise by the in-image fraction of the window (count of in-image taps / k^2: with w = 1 / k^2 this is
 * AvgPool2d(count_include_pad=False), model.py:69-74); the window may be larger than the image.
 * mode bit 0 clear (forward): out_low = low(x), out_high = a_h*(x - low(x)) + b_h; either output may be null, not both; x2 and accumulate are not
 * read.  Each output given is written on all 16 channels of plane 0, zero from channel C on.
 * mode bit 0 set (adjoint): out_low (+)= low(x) + a_h*(x2 - low(x2)) with x = dL/dlow, x2 = dL/dhigh (either may be null, not both); out_high and
 * b_h are not read.  With mode bit 1 the normaliser is the one of the forward op's OUTPUT pixel.  The kernel correlates with w itself where the
 * adjoint correlates with the flipped w: this form is the adjoint only for a SYMMETRIC w (w[ky][kx] == w[k-1-ky][k-1-kx]: every gaussian and box
 * kernel of the trainers); the caller keeps that contract.  accumulate 0: all 16 channels written, zero from channel C on; accumulate != 0: channels
 * below C are added to, the others keep their bits.
 * DASR_EINVAL: N * H * W <= 0, C outside 1..4, k <= 0 or even, w null; forward: x null or both outputs null; adjoint: out_low null or both inputs null. */
int dasr_lowpass(dasr_tensor x, dasr_tensor x2, const float* w, int32_t k, int32_t N, int32_t C, int32_t H, int32_t W,
                 int32_t mode, float a_h, float b_h, dasr_tensor out_low, dasr_tensor out_high, int32_t accumulate, void* stream);
/* nn.MaxPool2d(2,2) of the VGG19 feature stack, forward and backward (Ho, Wo = pooled size; Win = width of the INPUT: 2 Wo or 2 Wo + 1 --
 * an odd input drops its last row / column as nn.MaxPool2d's floor does; 0 = 2 Wo.  Round 3: before, odd inputs were mis-addressed); is_f32: 0 bf16, 1 f32, 2 f16 tensors; 3 / 4: split f16 / bf16 tensors (C channels in 2 * ceil(C/16) planes: hi planes, then lo planes);
 * backward only: 5 = split f16 activations x, plain f16 gradients.  Whole 16-channel planes are pooled, padding channels included (zero in, zero out);
 * of tied maxima the first in scan order wins (ATen); split tensors compare hi + lo and move the (hi, lo) pair unchanged. */
int dasr_maxpool2(dasr_tensor x, int32_t is_f32, int32_t N, int32_t C, int32_t Ho, int32_t Wo, dasr_tensor y, int32_t Win, void* stream);
/* relu_mask: also zero the gradient where the pooled maximum is <= 0 (the ReLU' of the conv feeding the pool).  Every element of every 2x2 window of gx is
 * written (the gradient or zero).  The last row / column of gx that an odd input size leaves outside every window is NOT written: the trainers rely on
 * zero at allocation there. */
int dasr_maxpool2_bwd(dasr_tensor x, dasr_tensor gy, int32_t is_f32, int32_t N, int32_t C, int32_t Ho, int32_t Wo, dasr_tensor gx,
                      int32_t relu_mask, int32_t Win, void* stream);
/* L1 between two blocked tensors (feature loss DASR_model.py:224-229; LL loss :220-222): loss_acc += coef*sum|a-b|,
 * ga = gcoef*sign(a-b).  is_f32 bit 1 set: squared form (MSE of the DSN VGG16 perceptual loss, loss.py:119-130). */
int dasr_l1_diff(dasr_tensor a, dasr_tensor b, int32_t is_f32, int32_t N, int32_t C, int32_t H, int32_t W, float coef, float gcoef,
                 float* loss_acc, dasr_tensor ga, void* stream);
/* per-channel affine on <=4 channels (VGG input normalisation architecture.py:1086-1087 and its adjoint); y_f32: 0 bf16, 1 f32, 2 f16 output, 3 split f16 (hi in plane 0, remainder in plane 1; no accumulate).
 * accumulate 0: all 16 channels of plane 0 of y are written (both planes of the split form), zero from channel C on; accumulate != 0: y[c] += for c < C, the
 * channels from C on keep what they held.  Planes of y past those are never touched.  scale4 / shift4: HOST pointers (read by the launcher). */
int dasr_affine4(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, const float* scale4, const float* shift4, dasr_tensor y,
                 int32_t y_f32, int32_t accumulate, void* stream);
/* F.interpolate(bilinear, align_corners=False) of the domain-distance map (DASR_model.py:173-174) by the integer `factor`: src NCHW [N][1][h][w] ->
 * dst [N][1][h * factor][w * factor], plain fp32 device buffers (h or w may be 1).  DASR_EINVAL: N * h * w <= 0, factor <= 0, src / dst null. */
int dasr_bilinear_up(const float* src, int32_t N, int32_t h, int32_t w, int32_t factor, float* dst, void* stream);

/* ---- LPIPS(alex) perceptual loss (csrc/lpips.hip) ----------------------------------------------------------------------
 * feature_criterion "LPIPS" of the shipped DASR configs: PerceptualLossLPIPS codes/SRN/models/modules/loss.py:66-72 -> PNetLin.forward
 * codes/PerceptualSimilarity/models/networks_basic.py:64-92 on the AlexNet slices of pretrained_networks.py:57-95.  The convs run on
 * dasr_conv (prec 3); these are the layers around them, all on blocked f32 tensors. */
/* mode 0: ScalingLayer (networks_basic.py:94-101, with the 2x-1 of models/util.py:36-38 folded into scale4/shift4) + 4x4 space-to-depth of
 * the 3-channel image (plane 0 of x) zero-padded by 2: y[c][Y][X][4*by+bx] = scale4[c]*x[c][4Y+by-2][4X+bx-2] + shift4[c], 3 planes of
 * (H+4)/4 x (W+4)/4 -- the 11x11/s4/p2 conv becomes 3x3/s1/p0 on 48 channels.  mode 1: adjoint, ACCUMULATED into channels 0..2 of x.
 * mode bits 4-6 (DSN --lpips_rot_flip, PerceptualLoss.forward codes/DSN/loss.py:155-168: torch.rot90 / torch.flip of both images in front of
 * LPIPS): the network sees T(x), T(x)[i][j] = x[u][v], (u, v) = (i, j) swapped if bit 4, u -> H-1-u if bit 5, v -> W-1-v if bit 6; mode 1 routes
 * the gradient back through the same map.  Transposing forms need H == W.
 * Contracts (tests/test_gpu_lpips_prelu.py):
 *  - mode 0 reads channels 0..2 of plane 0 of x (channels 3..15 and other planes are never read) and writes all 16 slots of exactly 3 planes of y; where the
 *    padded grid lies outside the image y holds +0 bit for bit (the zero padding is applied to the SCALED image: a border pixel is 0, not shift4[c]).
 *  - mode 1 adds scale4[c] * (the slot pixel (u, v) of x went to) into channels 0..2 of plane 0 of x; channels 3..15 and every other plane keep their bits; y is
 *    read only.  With a symmetry the gradient of T(x)[i][j] returns to x[u][v]: the INVERSE of the index map mode 0 reads through (the two differ for the quarter turns).
 *  - scale4 / shift4: HOST pointers to 4 floats (3 used), read by the launcher.
 *  - DASR_EINVAL, nothing launched or dereferenced: N, H or W <= 0; H or W not a multiple of 4; (mode & 15) outside {0, 1}; a transposing code with H != W; x, y,
 *    scale4 or shift4 null. */
int dasr_lpips_s2d(dasr_tensor x, int32_t N, int32_t H, int32_t W, const float* scale4, const float* shift4, dasr_tensor y, int32_t mode,
                   void* stream);
/* The forward input stage of dasr_lpips_s2d mode 0 (no symmetry, no adjoint) for ANY image size H, W >= 31 (the folder evaluator, dasr_amd/dsn_evaluate.py: result
 * images and border crops have arbitrary sizes).  Per axis the 11 / stride 4 / pad 2 conv has Ho = (H - 7) / 4 + 1 outputs (integer division) and the grid has
 * Hs = Ho + 2 block rows; y[c][Y][X][4*by+bx] = scale4[c]*x[c][4Y+by-2][4X+bx-2] + shift4[c] inside the image, 3 planes of Hs x Ws.
 * Contracts (tests/test_gpu_evaluate.py):
 *  - reads channels 0..2 of plane 0 of x; writes all 16 slots of exactly 3 planes of y; where the grid lies outside the image, on ANY side, y holds +0 bit for
 *    bit.  (Rows and columns of the image past the last window of the conv are written too: they meet the zero taps of the re-indexed weights.)
 *  - at multiples of 4, Hs = H / 4 + 1 and every byte equals what dasr_lpips_s2d mode 0 writes (the same kernel); callers keep using that entry point there.
 *  - scale4 / shift4: HOST pointers to 4 floats (3 used), read by the launcher.
 *  - DASR_EINVAL, nothing launched or dereferenced: N <= 0; H or W < 31 (below that the network's second pool has no output); x, y, scale4 or shift4 null. */
int dasr_lpips_s2d_any(dasr_tensor x, int32_t N, int32_t H, int32_t W, const float* scale4, const float* shift4, dasr_tensor y, void* stream);
/* nn.MaxPool2d(3, 2) of torchvision alexnet.features[2] / [5] on H x W inputs (output (H-3)/2+1), and its backward: gather form, first
 * maximum in scan order wins (ATen); relu_mask: zero where x <= 0; accumulate: gx += (the head gradient of that layer is already there).
 * Contracts (tests/test_gpu_lpips_prelu.py):
 *  - whole 16-channel planes are processed, the padding channels of the last plane like real ones -- zero in, zero out.
 *  - inputs are finite and above -3.4e38 (the running maximum starts there); the forward moves the maximum (equal to MaxPool2d by value).
 *  - ties: the FIRST maximum of a window in scan order (rows, then columns) receives that window's gradient; a pixel receives the gradients of those of its (at most
 *    2 x 2) windows whose first maximum it is, added in window order (rows, then columns).
 *  - relu_mask != 0: a pixel with x <= 0 (+0 and -0 included) receives nothing -- gx is exact zero there, or keeps its value when accumulating; the windows that
 *    are all zero hand nothing on.  relu_mask == 0: no mask.
 *  - the backward writes EVERY pixel of the C planes of gx: a row / column no window covers (even H or W) gets exact +0, or keeps its value when accumulating.
 *  - DASR_EINVAL, nothing launched: N or C <= 0; H or W < 3; x, y (forward), x, gy or gx (backward) null. */
int dasr_maxpool3s2(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor y, void* stream);
int dasr_maxpool3s2_bwd(dasr_tensor x, dasr_tensor gy, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor gx, int32_t relu_mask,
                        int32_t accumulate, void* stream);
/* one LPIPS layer: images n < N of f are compared with images n + pair_off; u = f0/(|f0|_2+eps), v likewise (normalize_tensor),
 * loss_acc += coef * sum_pixels sum_c lin[c] (u_c-v_c)^2;  g0 (optional) = gcoef * d(sum)/df0, zeroed where f0 <= 0 when relu_mask.
 * Contracts (tests/test_gpu_lpips_prelu.py):
 *  - only images [0, N) and [pair_off, pair_off + N) of f are read (pair_off need not be N); features of either sign are accepted; lin: C floats on the device.
 *  - g0 null: the loss alone; otherwise all C channels of N images of g0 are written.  relu_mask != 0: g0 is exact zero where f0 <= 0 (+0 and -0 included), whatever f1 holds.
 *  - a pixel whose f0 is all zero: u = 0 and the derivative of the norm is taken as 0 at the origin (k2 = 0), so g0_c = gcoef 2 lin[c] (0 - v_c) / eps there: large
 *    (eps = 1e-10) but finite, and zero when f1 is all zero too (such a pixel adds nothing to the loss).
 *  - loss_acc is added to (whatever it holds) through a fixed-order sum over the grid: the same inputs give the same bits in loss_acc and g0 on every run.
 *    loss_acc may be null (the gradient alone).
 *  - DASR_EINVAL, nothing launched: N, C, H or W <= 0; C not a multiple of 16; f or lin null. */
int dasr_lpips_head(dasr_tensor f, int64_t pair_off, int32_t N, int32_t C, int32_t H, int32_t W, const float* lin, float eps, float coef,
                    float gcoef, float* loss_acc, dasr_tensor g0, int32_t relu_mask, void* stream);

/* ---- DSN (codes/DSN) kernels ---------------------------------------------------------------------------------*/
/* domain-distance map for any discriminator conv table (receptive_cal.py:34-60, create_dataset_modified.py:14-24,119-126): D output value
 * (i, j) spread over its receptive-field window (jump / rf / start of the walk over the conv table), divided by the coverage count; d =
 * [N][1][n_h][n_w] D output, out = [N][1][H][W] map (channel 0 of 16-channel fp32 planes: only channel 0 of d is read, channels 1..15 of plane 0 of
 * out are written zero).  (jump, rf, start) of the walk over the WIDTH serve both axes.  FSD uses the equivalent 17 x 17 box of dasr_lowpass. */
int dasr_ddm_spread(dasr_tensor d, int32_t N, int32_t n_h, int32_t n_w, int32_t H, int32_t W, int32_t jump, int32_t rf, float start,
                    dasr_tensor out, void* stream);
/* -log losses of codes/DSN/loss.py:11-41 on p = sigmoid(logit) (model.py:104-105), logit = channel 0 of plane 0 of x: mode 0: -log(p+eps), mode 1:
 * -log(1-p+eps); loss_acc += coef*sum, score_acc += score_coef*sum(p) (either or both may be null), grad (+)= gcoef * d/dlogit (may be null).
 * accumulate 0: plane 0 of grad is written on all 16 channels, zero from channel 1 on; accumulate != 0: channel 0 is added to, the others keep their
 * bits.  Saturated logits give finite values: the loss stays within [-log(1+eps), -log(eps)], the gradient goes to (signed) zero.
 * DASR_EINVAL: N * H * W <= 0, x null, mode outside {0, 1}. */
int dasr_logloss(dasr_tensor x, int32_t N, int32_t H, int32_t W, int32_t mode, float eps, float coef, float gcoef, float* loss_acc,
                 float* score_acc, float score_coef, dasr_tensor grad, int32_t accumulate, void* stream);
/* backward of the generator's output sigmoid (model.py:55): gz = g * y * (1 - y) on C (<= 4) channels of plane 0; gz is written on all 16 channels
 * of plane 0, zero from channel C on; no other plane is touched.  DASR_EINVAL: N * H * W <= 0, C > 4, y / g / gz null. */
int dasr_sigmoid_bwd(dasr_tensor y, dasr_tensor g, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor gz, void* stream);
/* y = sigmoid(x) on C (<= 4) channels of plane 0: the discriminator's output map at inference (codes/DSN/model.py:104-106,
 * consumed by create_dataset_modified.py:14-24) */
int dasr_sigmoid_fwd(dasr_tensor x, int32_t N, int32_t C, int32_t H, int32_t W, dasr_tensor y, void* stream);
/* gradient of nn.PReLU()'s single slope (model.py:29,215) from the layer output y and dL/dx; deterministic two-stage sum;
 * scratch256: 1024 floats (one partial per workgroup of the first stage; the name is historical).
 * Contracts of the three slope-gradient entry points (tests/test_gpu_lpips_prelu.py):
 *  - *dst = scale * sum_{y <= 0} gx * y / a^2, a = *slope, over whole 16-channel planes (padding channels: zero in y and gx).  At y == +0 and -0 the term is an exact
 *    zero: the entry points are indifferent to `y <= 0` versus `y < 0` for finite gx, and no test tells the two apart.
 *  - every term is rounded to fp32 once (exact for f16 inputs), both stages sum per thread in double in a fixed order and finish with a fixed tree: deterministic, and
 *    accurate relative to sum |terms| (the total is a small difference of large sums).
 *  - the first stage runs min(1024, ceil(vector loads / 256)) workgroups (a grid-stride loop beyond that) and writes that many words of scratch256; the rest is not touched.
 *  - DASR_EINVAL, nothing launched: N, C, H or W <= 0; y, gx, slope, scratch256 or dst null. */
int dasr_prelu_grad(dasr_tensor y, dasr_tensor gx, int32_t N, int32_t C, int32_t H, int32_t W, const float* slope, float* scratch256,
                    float* dst, float scale, void* stream);
/* the same on f16 tensors (the DSN generator's 16-bit backward: y = f16 shadow of the layer output, gx = power-of-two pre-scaled f16 gradient;
 * the caller folds 1 / pre-scale into `scale`) */
int dasr_prelu_grad_f16(dasr_tensor y, dasr_tensor gx, int32_t N, int32_t C, int32_t H, int32_t W, const float* slope, float* scratch256,
                        float* dst, float scale, void* stream);
/* (ABI 20) the second stage alone for `count` slopes in one launch: workgroup k sums partial[k * stride .. + nblocks) in a fixed order and writes
 * *dsts[k] = scale * sum / (*slopes[k])^2.  The partials are those the data-gradient conv epilogues leave in dasr_conv_params::prelu_part (slope * dL/dh * h per
 * workgroup): the DSN generator's residual blocks no longer read h and dL/dz a second time (dasr_prelu_grad_f16 did). slopes / dsts: DEVICE arrays of device pointers.
 * Only partial[k * stride + i], i < nblocks, is read: the gaps of a stride > nblocks layout are not.  DASR_EINVAL, nothing launched: nblocks <= 0, stride < nblocks,
 * count <= 0, partial, slopes or dsts null. */
int dasr_prelu_final(const float* partial, int32_t nblocks, int64_t stride, int32_t count, const float* const* slopes, float* const* dsts, float scale, void* stream);
/* un-padded low-pass of the colour loss (FilterLow(padding=False), loss.py:52-56) on C (<= 4) channels of plane 0, w = [k][k] fp32 on the device
 * (any w: nothing relies on symmetry here).  H, W are the size of the IMAGE in both modes.  mode 0 forward: out[y][x] = sum w[ky][kx] * x[y+ky][x+kx],
 * x H x W -> out (H-k+1) x (W-k+1).  mode 1: its adjoint, x = gradient (H-k+1) x (W-k+1) -> out H x W, out[y+ky][x+kx] (+)= w[ky][kx] * x[y][x].
 * accumulate 0: plane 0 of out is written on all 16 channels, zero from channel C on; accumulate != 0: channels below C are added to, the others
 * keep their bits.  DASR_EINVAL: k <= 0, H < k, W < k, C > 4, mode outside {0, 1}, x / out / w null, N <= 0. */
int dasr_lowpass_valid(dasr_tensor x, const float* w, int32_t k, int32_t N, int32_t C, int32_t H, int32_t W, int32_t mode,
                       dasr_tensor out, int32_t accumulate, void* stream);

/* ---- device-side input pipeline -----------------------------------------------------
 * Batch assembly of codes/SRN/data/LRHR_wavelet_unpairEq_fake_w_dataset.py:50-166 + data/util.py:116-128 on resident images:
 * sample k of the batch = size x size crop at (y0, x0) of image `src` (CHW fp32, RGB) -- first resized bilinearly to vH x vW when
 * that differs from H x W (cv2.resize(..., INTER_LINEAR) of the domain-distance map to the LR size) -- then horizontal flip,
 * vertical flip, transpose, in that order (util.augment).  dst is [n][C][size][size] fp32.
 * Contracts (tests/test_gpu_lpips_prelu.py):
 *  - every element of dst is written.  A sample without a resize is a copy, bit for bit.  Channels c >= desc.C are zero (descriptors of different channel counts may
 *    share a launch).  Where the window leaves the (resized) view -- y0 + i or x0 + j outside [0, vH) x [0, vW) -- dst is zero and nothing is read.
 *  - the resize follows cv2.INTER_LINEAR: source coordinate (v + 0.5) * H / vH - 0.5 (half-pixel centres), both neighbours clamped to the image (edge clamp); it is
 *    taken whenever vH != H or vW != W (an axis of equal size then has integer coordinates and weight 0).
 *  - descriptors are device memory and are NOT validated: src must hold C * H * W floats.
 *  - DASR_EINVAL, nothing launched: n, C or size <= 0; descs_dev or dst null. */
typedef struct {
    const float* src;
    int32_t C, H, W;      /* source image */
    int32_t vH, vW;       /* size it is resized to before cropping (== H, W: no resize) */
    int32_t y0, x0;       /* crop origin */
    int32_t flags;        /* bit 0 hflip, bit 1 vflip, bit 2 transpose */
} dasr_crop_desc;
int dasr_gather_crops(const dasr_crop_desc* descs_dev, int32_t n, int32_t C, int32_t size, float* dst, void* stream);

/* ---- executor: run a recorded list of ops in one call (keeps the host out of the step) ----------*/
/* Which slot of dasr_op carries which argument of an op kind: the dasr_run_ops switch (csrc/misc.hip), mirrored by the table OP_ARGS of
 * dasr_amd/_lib.py (tests/test_host.py checks the two against each other and against the parameter names below). */
enum { DASR_OP_CONV = 1, DASR_OP_WGRAD = 2, DASR_OP_WGRAD_REDUCE = 3, DASR_OP_PACK = 4, DASR_OP_DOWNSUM = 5,
       DASR_OP_AXPBY = 6, DASR_OP_FILL = 7, DASR_OP_L1LOSS = 8, DASR_OP_NCHW2B = 9, DASR_OP_B2NCHW = 10,
       DASR_OP_INORM_FWD = 11, DASR_OP_INORM_BWD = 12, DASR_OP_BCE = 13, DASR_OP_DWT_FWD = 14, DASR_OP_DWT_BWD = 15,
       DASR_OP_LOWPASS = 16, DASR_OP_MAXPOOL = 17, DASR_OP_MAXPOOL_BWD = 18, DASR_OP_L1DIFF = 19, DASR_OP_AFFINE4 = 20,
       DASR_OP_BILINEAR = 21, DASR_OP_LOGLOSS = 22, DASR_OP_SIGMOID_BWD = 23, DASR_OP_PRELU_GRAD = 24, DASR_OP_LOWPASS_VALID = 25,
       DASR_OP_ADD_FLAT = 26, DASR_OP_SIGMOID_FWD = 27,
       /* scheduling ops: an event from dasr_event_create / a hipStream_t (NULL: back to the stream dasr_run_ops was called with) */
       DASR_OP_EVENT_RECORD = 28, DASR_OP_STREAM_WAIT = 29, DASR_OP_SET_STREAM = 30,
       DASR_OP_CVT_F16 = 31, DASR_OP_DOWNSUM_F16 = 32, DASR_OP_PIXSHUF = 33, DASR_OP_PIXUNSHUF = 34,
       DASR_OP_LPIPS_S2D = 35, DASR_OP_MAXPOOL3 = 36, DASR_OP_MAXPOOL3_BWD = 37, DASR_OP_LPIPS_HEAD = 38, DASR_OP_RAGAN = 39,
       DASR_OP_BNORM_FWD = 40, DASR_OP_BNORM_BWD = 41, DASR_OP_BNORM_RUNNING = 42, DASR_OP_DDM_SPREAD = 43,
       /* --wgan gradient penalty (round 4) */
       DASR_OP_INORM_JVP = 44, DASR_OP_INORM_SECOND = 45, DASR_OP_GRAD_PENALTY = 46, DASR_OP_FILL_SCALED = 47,
       DASR_OP_CONV_CHAIN = 48,  /* dasr_conv_chain */
       DASR_OP_RDB_CHAIN = 49,   /* dasr_rdb_chain */
       /* --wgan with BatchNorm discriminators (round 6): dasr_bnorm_lrelu_jvp, dasr_bnorm_second */
       DASR_OP_BNORM_JVP = 50, DASR_OP_BNORM_SECOND = 51,
       DASR_OP_PRELU_FINAL = 52,  /* dasr_prelu_final */
       DASR_OP_RESBLOCK = 53,     /* dasr_resblock (host dasr_resblock_params, kept alive by the plan) */
       DASR_OP_LPIPS_S2D_ANY = 54 /* dasr_lpips_s2d_any */ };

typedef struct {
    int32_t op;  int32_t i[8];  float f[4];  int64_t l[4];  void* p[4];  dasr_tensor t[5];
    dasr_conv_params conv;
    double flops, bytes;   /* algorithmic work of the op (set by the plan builder; only read by the profiling session below) */
} dasr_op;

int dasr_run_ops(const dasr_op* ops, int32_t n, void* stream);
/* Enqueue `nlists` independent op lists, list i on streams[i], each from its own host thread (list 0 on the caller, a persistent pool for
 * the rest, bound to the caller's device); returns when every list has been enqueued.  For the sub-batch replica streams of a training step
 * (dasr_amd/models.py: three or four replicas are 5 000+ launches per step -- more than one enqueue thread feeds).  nlists <= 8.  On failure
 * dasr_last_failed_op() = op index | (list index << 24).  Replaces nothing in the reference (its step is one autograd graph on one stream,
 * codes/SRN/models/SR_model.py:77-85). */
int dasr_run_ops_mt(const dasr_op* const* lists, const int32_t* counts, void* const* streams, int32_t nlists);
/* events for the scheduling ops (hipEventDisableTiming); independent work of one list can be moved to a second stream this way
 * (the dense-block weight gradients are not on the data-gradient chain's critical path) */
void* dasr_event_create(void);
int dasr_event_destroy(void* ev);
int dasr_last_failed_op(void);   /* index of the op that made dasr_run_ops return non-zero */

/* ---- RCCL gradient exchange (csrc/rccl.hip) ------------------------------------------------------------------------------
 * Replaces the single-process nn.DataParallel of the reference (codes/SRN/models/networks.py:144-146,192-193): one process per GPU,
 * replicated weights, SUM all-reduce of the flat fp32 gradient buffer over xGMI (the 1/world factor is folded into dasr_wgrad_reduce).
 * Rank 0 creates a 128-byte id (dasr_rccl_unique_id) and hands it to the other ranks through any side channel; every rank then calls
 * dasr_rccl_init (collective).  dasr_allreduce / dasr_broadcast are in place, asynchronous on `stream`; return an ncclResult_t. */
int dasr_rccl_unique_id(void* id128);
int dasr_rccl_init(const void* id128, int32_t rank, int32_t world, void** comm_out);
int dasr_allreduce(void* comm, float* buf, int64_t count, void* stream);
int dasr_broadcast(void* comm, float* buf, int64_t count, int32_t root, void* stream);
int dasr_rccl_destroy(void* comm);

/* ---- image-quality metrics of the validation / evaluation drivers (csrc/metrics.hip, ABI 22) -------------------------------------
 * Replaces the host numpy of codes/SRN/utils/util.py:180-204 (tensor2img), :236-291 (calculate_psnr / ssim / calculate_ssim) and
 * data/util.py:169-190 (bgr2ycbcr, Y only) on what the trainers hold after test(): contiguous fp32 NCHW device images, C = 3 or 1.
 *
 * dasr_tensor2img_u8: u = rint(((clamp(x, lo, hi) - lo) / (hi - lo)) * 255.0f) in fp32, in tensor2img's order of operations, round half to even,
 * as uint8 -- byte for byte the host function.  Two outputs, either may be NULL (not both): hwc_bgr [N][H][W][C] with the channel order reversed
 * (what save_img takes; C = 1: [N][H][W]) and planar [N][C][H][W] in the input's channel order (what the two entry points below read).  A NaN
 * becomes 0 and is counted in *nan_count (device int32, may be NULL; set to zero by the call).
 *
 * dasr_img_sse: over rows [crop, H - crop) x columns [crop, W - crop) of two planar uint8 images, per image n: sse[n] = the INTEGER sum of the squared
 * differences over all channels (PSNR = 20 log10(255 / sqrt(sse / count)) is left to the caller); sse_y[n] (may be NULL; C = 3 only) = the fp64 sum
 * of the squared difference of y = (((24.966 B + 128.553 G + 65.481 R) / 255 + 16) / 255) * 255 (bgr2ycbcr's float branch and the `* 255` of the
 * call site, unrounded), planes in R, G, B order.
 *
 * dasr_img_ssim: ssim[n] = mean over every channel and every pixel of the 'valid' region of the cropped images of the SSIM map: window 11 x 11,
 * sigma 1.5, normalised, applied separably, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, fp64 throughout.  y_channel 1 (C = 3 only): on y as above.
 * A cropped side under 11 pixels has no valid region: DASR_EINVAL.
 *
 * The grid sums are per-workgroup partials in `ws` (device, ws_size bytes >= dasr_img_ws_bytes(N, C, H, W, crop), 8-byte aligned) added in index order
 * by a second launch: no floating-point atomics, the same bits run to run.  Calls that share `ws` must be ordered by their stream.  sse, sse_y, ssim,
 * nan_count: device memory; nothing is synchronised.  Null pointers, N <= 0, C not 1 or 3, 2 crop >= H or W: DASR_EINVAL, nothing is launched.
 *
 * The two entry points of the folder evaluator (codes/DSN/evaluate.py:44-46; dasr_amd/metrics.py pair_metrics_u8), additive under ABI 22, on the same planar
 * uint8 images, crop and workspace -- dasr_img_ws_bytes covers both:
 *
 * dasr_img_ssim_box: ssim[n] = mean over every channel and every 7 x 7 window that lies wholly inside the cropped image of the SSIM of that window in the form of
 * skimage.measure.compare_ssim(X, Y, multichannel=True) on uint8 (uniform filter, use_sample_covariance=True, data_range 255): with the window sums Sx, Sy,
 * Sxx, Syy, Sxy over n = 49 pixels, ux = Sx / n, vx = (n Sxx - Sx^2) / (n (n - 1)) (vy, vxy likewise), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 * S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)).  The five sums are formed as exact 32-bit integers and S is evaluated once per window in
 * fp64 from them, so the map does not depend on the tiling; identical images give exactly 1.  A cropped side under 7 pixels: DASR_EINVAL.
 *
 * dasr_img_channel_sums: sums[n * C + c] = the exact integer sum of the bytes of channel c of image n over the cropped region (the mean colour of PSNR_col).
 *
 * Both: per-workgroup partials in ws, added in index order by a second launch (no atomics, the same bits run to run); ssim / sums: device memory.  Null pointers,
 * N <= 0, C not 1 or 3, 2 crop >= H or W, ws_size under what the call needs: DASR_EINVAL, nothing is launched. */
int dasr_img_ws_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop);   /* bytes, or DASR_EINVAL */
int dasr_tensor2img_u8(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, double lo, double hi, uint8_t* hwc_bgr, uint8_t* planar,
                       int32_t* nan_count, void* stream);
int dasr_img_sse(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int64_t* sse, double* sse_y,
                 void* ws, int64_t ws_size, void* stream);
int dasr_img_ssim(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t y_channel, double* ssim,
                  void* ws, int64_t ws_size, void* stream);
int dasr_img_ssim_box(const uint8_t* a, const uint8_t* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, double* ssim, void* ws, int64_t ws_size,
                      void* stream);
int dasr_img_channel_sums(const uint8_t* a, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int64_t* sums, void* ws, int64_t ws_size, void* stream);

/* ---- input stage of the evaluation datasets (csrc/imgio.hip) ---------------------------------------------------------------------
 * What data.EvalFolderDataset runs per image file in place of the host's read_img / modcrop / imresize_np (codes/SRN/data/util.py:78-96, :133-145,
 * :243-433).  Plain vector loads and stores, no atomics, asynchronous on `stream`.
 *
 * dasr_u8_to_planar: src = a decoded image, uint8 [H][W][3] (interleaved, any channel order); dst = its top-left Hc x Wc window as planar fp32
 * [3][Hc][Wc], dst[c][y][x] = (float)src[y][x][c] / 255.0f with the correctly rounded fp32 division -- bit for bit numpy's
 * `asarray(img, float32) / 255.0` followed by modcrop (Hc = H - H % scale, Wc = W - W % scale).  Hc > H, Wc > W, a side over 65535: DASR_EINVAL.
 *
 * dasr_imresize_down: src planar fp32 [C][H][W] -> dst [C][H / s][W / s], MATLAB's imresize(., 1 / s) (bicubic, antialiased) for s in {2, 3, 4}.
 * The caller supplies the per-axis tap tables of data.bicubic_taps(n, 1 / s): idx_* [n / s][4 s + 2] int32 (0-based source index, already mirrored
 * into [0, n)), w_* [n / s][4 s + 2] fp64 (normalised per output sample), in device memory; the same pair may serve both axes when H == W.
 * Pass 1 (along H) writes tmp (device, C * (H / s) * W doubles); pass 2 (along W) reads it.  Products and sums are fp64, in tap order, the products
 * rounded before they are added; the result is rounded to fp32 once.  Same inputs, same bits.  H or W not a multiple of s, s outside {2, 3, 4},
 * a null pointer, a side or C over 65535: DASR_EINVAL, nothing is launched. */
int dasr_u8_to_planar(const uint8_t* src, int32_t H, int32_t W, int32_t Hc, int32_t Wc, float* dst, void* stream);
int dasr_imresize_down(const float* src, int32_t C, int32_t H, int32_t W, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                       const double* w_w, double* tmp, float* dst, void* stream);

/* ---- batch assembly of the DSN trainer on resident 8-bit images (csrc/imgio.hip) ---------------------------------------------------
 * What dsn_data.DeviceTrainDeresnet / DeviceValDeresnet run per batch in place of the host's decode, crop, flips, rotation, to_tensor and imresize
 * (codes/DSN/data_loader.py:12-59, :157-190, utils.py:37-160).  Asynchronous on `stream`, nothing is synchronised, same inputs give the same bits.
 *
 * dasr_gather_crops_u8: sample k of dst [n][3][size][size] fp32 = the size x size window at (sub_y, sub_x) of the TRANSFORMED crop x crop window at (y0, x0) of
 * image `src` (uint8 [H][W][3], as PIL decodes it): vertical flip (flags bit 0), then horizontal flip (bit 1), then k = bits 2-3 quarter-turns counter-clockwise
 * (torch.rot90(., k, (1, 2))), in that order; every sample is (float)byte / 255.0f, the correctly rounded fp32 division.  The clean crop has size == crop and
 * sub_y == sub_x == 0, the source-domain crop size == crop / 4.  The descriptors are device memory and are not validated: the caller guarantees
 * y0 + crop <= H, x0 + crop <= W, sub + size <= crop; the kernel clamps every source coordinate into the image, so a damaged descriptor reads a wrong pixel
 * and never outside the allocation.  A null pointer, n <= 0, n > 65535, size <= 0, size > 4096: DASR_EINVAL, nothing is launched.
 *
 * dasr_crops_bicubic_down: hr [n][3][c][c] fp32 -> dst [n][3][c / s][c / s], MATLAB's imresize(., 1 / s) (bicubic, antialiased), rows first, then columns,
 * clamped to [0, 1], for the whole batch in one launch and without an intermediate in device memory.  idx / wt [c / s][4 s + 2]: the tap table of
 * data.bicubic_taps(c, 1 / s) (int32 0-based source index mirrored into [0, c), fp64 weight), one table for both axes and all 3 n planes.  fp64 products and
 * sums in tap order, the clamp in fp64, one rounding to fp32.  s != 4, c not a multiple of 4 in [4, 1024], n <= 0, n > 65535, a null pointer, hr not 16-byte
 * aligned: DASR_EINVAL, nothing is launched. */
typedef struct {
    const uint8_t* src;
    int32_t H, W;           /* source image */
    int32_t y0, x0, crop;   /* crop x crop window of the source */
    int32_t flags;          /* bit 0 vertical flip, bit 1 horizontal flip, bits 2-3 quarter-turns */
    int32_t sub_y, sub_x;   /* origin of the size x size output window inside the transformed crop */
} dasr_crop_u8_desc;
int dasr_gather_crops_u8(const dasr_crop_u8_desc* descs_dev, int32_t n, int32_t size, float* dst, void* stream);
int dasr_crops_bicubic_down(const float* hr, int32_t n, int32_t c, int32_t s, const int32_t* idx, const double* wt, float* dst, void* stream);

/* ---- batch assembly of the SRN trainers on resident 8-bit images (csrc/imgio.hip) ---------------------------------------------------
 * What data.DeviceUnpairedDataset / DevicePairedDataset run per batch under `"resident_u8": true` (codes/SRN/data/LRHR_wavelet_unpairEq_fake_w_dataset.py:50-166,
 * LRHR_dataset.py:44-126, data/util.py:116-128 augment).  Asynchronous on `stream`, nothing is synchronised, same inputs give the same bits.
 *
 * dasr_gather_srn_u8: ONE launch writes every 3-channel tensor of a batch.  Descriptor k: the size x size window at (y0, x0) of image `src` (uint8 [H][W][3], RGB, as
 * PIL decodes it), then horizontal flip (flags bit 0), vertical flip (bit 1), transpose (bit 2), in that order -- dasr_crop_desc's flags -- written to `dst` as planar fp32
 * [3][size][size]; every sample is (float)byte / 255.0f, the correctly rounded fp32 division.  The sizes of the descriptors of one launch may differ (LR and HR windows):
 * the grid is sized by max_size, a descriptor with size > max_size is cut off at max_size^2 samples, smaller windows are masked.  A descriptor with a null src or
 * dst or size <= 0 writes nothing.  The descriptors are device memory and are not validated: the caller guarantees y0 + size <= H, x0 + size <= W; the kernel clamps every
 * source coordinate into the image, so a damaged descriptor reads a wrong pixel and never outside the image.  A null pointer, n <= 0, n > 65535, max_size <= 0,
 * max_size > 4096: DASR_EINVAL, nothing is launched.
 *
 * dasr_crops_down4_u8: the augmented LR crops of `mode: "LRHR"` without LR files, straight from the resident HR bytes, one launch per batch, no intermediate in device
 * memory.  Descriptor k: `src` the HR image (H and W multiples of 4), (y0, x0) the origin of the size x size window in the LR image, flags and dst as above.  Before the
 * flips, output pixel (oy, ox) is pixel (y0 + oy, x0 + ox) of MATLAB's imresize(image / 255, 1 / 4) of the WHOLE image: the 18 rows 4 (y0 + oy) - 7 ... + 10, mirrored at the
 * image's own borders (j < 0 -> -j - 1, j >= H -> 2 H - 1 - j), with the weights w18[0 .. 17] (the one row of data.bicubic_taps(n, 0.25)[1]: at scale 1 / 4 every output
 * sample has the same weights), then the 18 columns likewise.  fp64 products, each rounded before it is added, sums in tap order, no clamp, one rounding to fp32: bit for
 * bit dasr_imresize_down of dasr_u8_to_planar of the image, cropped and augmented.  w18 is HOST memory (18 doubles, passed to the kernel by value).  descs_host is a host
 * copy of the n descriptors (the staging buffer they were uploaded from) and is what is validated: a null pointer, n <= 0, n > 65535, size <= 0, size > 128, a descriptor
 * with a null src or dst, H or W not a positive multiple of 4, size different from `size`, or a window outside the LR image: DASR_EINVAL, nothing is launched. */
typedef struct {
    const uint8_t* src;
    int32_t H, W;           /* source image */
    int32_t y0, x0, size;   /* size x size window at (y0, x0) */
    int32_t flags;          /* bit 0 hflip, bit 1 vflip, bit 2 transpose */
    float* dst;             /* [3][size][size] */
} dasr_srn_u8_desc;
int dasr_gather_srn_u8(const dasr_srn_u8_desc* descs_dev, int32_t n, int32_t max_size, void* stream);
int dasr_crops_down4_u8(const dasr_srn_u8_desc* descs_dev, const dasr_srn_u8_desc* descs_host, int32_t n, int32_t size, const double* w18, void* stream);

/* ---- x8 geometric self-ensemble (csrc/imgio.hip) --------------------------------------------------------------------------------------
 * The geometry of BaseModel.test_x8 (codes/SRN/models/SR_model.py:102-140): super-resolve the eight flips / transposes of the LR image, undo each transform on its SR
 * image, average.  Member i = 0..7 as the reference's list construction numbers them: b0 = i & 1 flips along W, b1 = (i >> 1) & 1 flips along H, b2 = i >> 2 transposes
 * (applied last).  Both calls are ONE launch, asynchronous on `stream`, planar fp32 images, any H, W >= 1 (16-byte accesses when the length along the contiguous axis is a
 * multiple of 4 and the pointers are 16-byte aligned, one sample per lane otherwise; the transposed half goes through LDS tiles, never a strided global access).
 *
 * dasr_dihedral8: x [C][H][W] -> dst_a [4][C][H][W] (members 0..3): dst_a[i][c][r][q] = x[c][b1 ? H-1-r : r][b0 ? W-1-q : q], and dst_b [4][C][W][H] (members 4..7):
 * dst_b[i-4][c][a][b] = x[c][b1 ? H-1-b : b][b0 ? W-1-a : a].  Exact copies.
 *
 * dasr_dihedral8_mean: H, W are the size of the OUTPUT; sr_a [4][C][H][W] and sr_b [4][C][W][H] are the generator's outputs for dst_a and dst_b.
 * dst[c][R][Q] = 0.125f * (((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7) in fp32, in exactly that order (no contraction, no fast-math: the same inputs give the same
 * bits), with Rh = b1 ? H-1-R : R, Qv = b0 ? W-1-Q : Q, s_i = sr_a[i][c][Rh][Qv] for i < 4 and s_i = sr_b[i-4][c][Qv][Rh] for i >= 4.
 *
 * A null pointer, C, H or W <= 0, C > 65535, H > 65535 * 64, or a destination equal to a source (or dst_a == dst_b): DASR_EINVAL, nothing is launched.  The buffers must
 * not overlap in any other way either (not checked). */
int dasr_dihedral8(const float* x, int32_t C, int32_t H, int32_t W, float* dst_a, float* dst_b, void* stream);
int dasr_dihedral8_mean(const float* sr_a, const float* sr_b, int32_t C, int32_t H, int32_t W, float* dst, void* stream);

/* ---- iterative back-projection of an SR image onto its LR input (csrc/imgio.hip) -----------------------------------------------------
 * One iteration of codes/SRN/scripts/back_projection/backprojection.m:12-19 as two launches (dasr_amd/backproject.py back_project):
 * d = LR - imresize(SR, 1 / s), then SR += conv2(imresize(d, s), p, 'same').  Planar fp32 images, s in {2, 3, 4}, any LR size h, w >= 1 and C >= 1, asynchronous on
 * `stream`, no atomics, nothing is synchronised, same inputs give the same bits.  All tables are device memory.
 *
 * dasr_bp_residual: sr [C][H][W], lr and d [C][H / s][W / s].  d[c][y][x] = lr[c][y][x] - (float)down(sr)[c][y][x], the subtraction in fp32, `down` bit for bit what
 * dasr_imresize_down writes: the tap tables of data.bicubic_taps(n, 1 / s) (idx_* [n / s][4 s + 2] int32 mirrored into [0, n), w_* fp64), rows first, fp64 products
 * rounded before they are added in tap order, one rounding to fp32.  Both passes run in LDS on the HR window a DASR_BP_RES_TILE_H x DASR_BP_RES_TILE_W tile of LR
 * outputs reaches; there is no intermediate in device memory.  d must not overlap sr or lr.
 *
 * dasr_bp_update: IN PLACE on sr [C][s h][s w]; d [C][h][w].  sr[c][y][x] = (float)((double)sr[c][y][x] + sum over a, b = -2 .. 2 of u5[a + 2] * u5[b + 2] * U[c][y + a][x + b]),
 * U = 0 outside the image and U = imresize(d, s) inside (bicubic, not antialiased): the tables of data.bicubic_taps(n, s), idx_* [s n][6] int32 mirrored into [0, n),
 * w_* [s n][6] fp64, rows first, then columns.  The 5-tap pass runs along x first (b in order), then along y (a in order); every product and sum is fp64, the result
 * is rounded to fp32 once.  u5 is HOST memory: 5 doubles, passed to the kernel by value (u_i = exp(-i^2) / sum_j exp(-j^2): the 2-D kernel of backprojection.m:6-8
 * is their outer product).  One launch per call, DASR_BP_UPD_TILE_H x DASR_BP_UPD_TILE_W samples of sr per workgroup.  d must not overlap sr.
 *
 * A null pointer, s outside {2, 3, 4}, H or W not a multiple of s, C or a side of the HR image over 65535: DASR_EINVAL, nothing is launched. */
#define DASR_BP_RES_TILE_H 8
#define DASR_BP_RES_TILE_W 32
#define DASR_BP_UPD_TILE_H 16
#define DASR_BP_UPD_TILE_W 64
int dasr_bp_residual(const float* sr, const float* lr, int32_t C, int32_t H, int32_t W, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                     const double* w_w, float* d, void* stream);
int dasr_bp_update(float* sr, const float* d, int32_t C, int32_t h, int32_t w, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                   const double* w_w, const double* u5, void* stream);

/* ---- dataset preparation: bicubic LR and Bic images of windows of a resident 8-bit image (csrc/imgio.hip) ---------------------------
 * codes/SRN/scripts/generate_mod_LR_bic.m:50-64 on the device (dasr_amd/bicubic.py, `python -m dasr_amd.prepare_data`), and the up-sampling half of
 * back_projection/main_reverse_filter.m:18-22 (backproject.reverse_filter).  Plain vector loads and stores, no atomics, asynchronous on `stream`, nothing is
 * synchronised, same inputs give the same bits.  Every product and sum is fp64, in tap order, the product rounded before it is added (the convention of
 * dasr_imresize_down); rows first, then columns.  All tables are device memory.
 * q(x) = min(255, max(0, floor(x * 255 + 0.5))) evaluated in fp64: MATLAB's imwrite of a double image (im2uint8).
 *
 * dasr_windows_down_u8: src = a decoded image, uint8 [H][W][3] interleaved; n windows of hh x ww pixels (multiples of s) with their top-left corners in wins_dev[k]
 * (device memory; wins_host is the same array in HOST memory, read before the launch for the bounds check only).  Per window
 * L = imresize(window / 255.0, 1 / s) with the tables of data.bicubic_taps(hh, 1 / s) and (ww, 1 / s) (idx_* [hh / s][4 s + 2] int32 mirrored into [0, hh), w_* fp64):
 * the mirror edge is the WINDOW's edge, a window never reads its neighbours' pixels.  Both passes run in LDS on the window bytes a DASR_WD_TILE_H x DASR_WD_TILE_W
 * tile of LR outputs reaches; there is no intermediate in device memory.  lr_u8 [n][hh / s][ww / s][3] = q(L), lr_f64 [n][3][hh / s][ww / s] = L; either may be
 * null, not both.  Rows of 3 W bytes are read as aligned 4-byte words where src is 4-byte aligned and the word lies inside the image, byte by byte elsewhere.
 *
 * dasr_imresize_up: MATLAB's imresize(x, s) (bicubic, not antialiased, symmetric edge) of planes x [N][C][h][w], fp32 (x_f64 = 0) or fp64 (x_f64 = 1), any h, w >= 1:
 * the tables of data.bicubic_taps(n, s), idx_* [s n][6] int32 mirrored into [0, n), w_* [s n][6] fp64 (what dasr_bp_update reads).  mode DASR_UP_F32: dst fp32
 * [N][C][s h][s w] = (float)up(x); DASR_UP_F32_ACC: dst = (float)((double)dst + up(x)), one rounding; DASR_UP_U8: dst uint8 [N][s h][s w][C] = q(up(x)), interleaved.
 * DASR_UP_TILE_H x DASR_UP_TILE_W output samples per workgroup.  dst must not overlap x.
 *
 * A null pointer, s outside {2, 3, 4}, hh or ww not a multiple of s, a side of an image or window, n, N or N C over 65535, a window that does not lie inside the image,
 * an unknown mode: DASR_EINVAL, nothing is launched. */
#define DASR_WD_TILE_H 8
#define DASR_WD_TILE_W 32
#define DASR_UP_TILE_H 16
#define DASR_UP_TILE_W 64
#define DASR_UP_F32 0
#define DASR_UP_F32_ACC 1
#define DASR_UP_U8 2
typedef struct {
    int32_t y0, x0;   /* top-left corner of the window in the image */
} dasr_window_desc;
int dasr_windows_down_u8(const uint8_t* src, int32_t H, int32_t W, const dasr_window_desc* wins_dev, const dasr_window_desc* wins_host, int32_t n, int32_t hh, int32_t ww,
                         int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w, const double* w_w, uint8_t* lr_u8, double* lr_f64, void* stream);
int dasr_imresize_up(const void* x, int32_t x_f64, int32_t N, int32_t C, int32_t h, int32_t w, int32_t s, const int32_t* idx_h, const double* w_h, const int32_t* idx_w,
                     const double* w_w, void* dst, int32_t mode, void* stream);

/* ---- dataset corruption: JPEG round trip and rounded Gaussian noise on resident 8-bit images (csrc/corrupt.hip) -------------------------
 * codes/DSN/add_corruptions.py on the device (dasr_amd/corrupt.py, `python -m dasr_amd.add_corruptions`).  Images are uint8 [N][H][W][3] interleaved RGB, any H, W >= 1.
 * Integer arithmetic (int32) and plain vector loads and stores, no atomics, asynchronous on `stream`, nothing is synchronised, same inputs give the same bits.
 *
 * dasr_jpeg_blocks + dasr_jpeg_merge: what Image.save(f, 'JPEG', quality=q) followed by Image.open gives back with libjpeg-turbo, bit for bit, without the entropy
 * coder: baseline, 4:2:0, the slow-integer DCT (jfdctint.c / jidctint.c), Annex K tables scaled as jpeg_set_quality does, h2v2 "fancy" up-sampling (plain replication
 * when the chroma plane is at most 2 samples wide).  corrupt.jpeg_roundtrip_ref states every step.
 * dasr_jpeg_blocks writes the DECODED planes of every image into `planes` (8-byte aligned), per image DASR_JPEG_PLANE_BYTES(H, W) bytes: Y [ceil8(H)][ceil8(W)], then
 * Cb and Cr [ceil8(ceil(H / 2))][ceil16(W) / 2].  One 8 x 8 block per 8 lanes (DASR_JPEG_BLOCKS_PER_WG blocks per workgroup): RGB bytes -> YCbCr -> 2 x 2 chroma average
 * -> forward DCT, quantise, dequantise, inverse DCT; coefficients stay in registers and LDS.  Edges: columns repeat the last column up to a multiple of 16 before the
 * average; rows get at most one repeated row (odd H) before it, and the averaged chroma plane repeats its last row down to a multiple of 8; Y repeats its last row.
 * Rows of 3 W bytes are read as aligned 4-byte words where src is 4-byte aligned and the run lies inside the row, byte by byte elsewhere.
 * dasr_jpeg_merge reads those planes: chroma up-sampling, YCbCr -> RGB, clamp, interleaved bytes to dst [N][H][W][3].
 *
 * dasr_noise_u8: dst[n][e] = clip(src[n][e] + rint(std z), 0, 255), e < per (= H W 3), rint to nearest even.  z: Philox4x32-10 with key `seed` (low word, high word) and
 * counter (g lo, g hi, index0 + n, 0) for the group g = e / 4; its outputs x0 .. x3 give z of e = 4 g .. 4 g + 3 as two Box-Muller pairs in fp64: u1 = (x0 + 1) 2^-32,
 * u2 = x1 2^-32, sqrt(-2 ln u1) cos(2 pi u2) and ... sin(2 pi u2); x2, x3 likewise.  dst may be src.
 *
 * A null pointer, N outside 1 .. 65535, a side outside 1 .. 65535, quality outside 1 .. 100, planes not 8-byte aligned, planes equal to src / dst, per < 1 or above
 * 2^36, std negative or not finite, index0 < 0 or index0 + N > 2^32: DASR_EINVAL, nothing is launched. */
#define DASR_JPEG_BLOCKS_PER_WG 32
#define DASR_JPEG_CEIL(v, m) (((v) + (m) - 1) / (m) * (m))
#define DASR_JPEG_PLANE_BYTES(H, W) \
    ((int64_t)DASR_JPEG_CEIL(H, 8) * DASR_JPEG_CEIL(W, 8) + 2 * (int64_t)DASR_JPEG_CEIL(((H) + 1) / 2, 8) * (DASR_JPEG_CEIL(W, 16) / 2))
int dasr_jpeg_blocks(const uint8_t* src, int32_t N, int32_t H, int32_t W, int32_t quality, uint8_t* planes, void* stream);
int dasr_jpeg_merge(const uint8_t* planes, int32_t N, int32_t H, int32_t W, uint8_t* dst, void* stream);
int dasr_noise_u8(const uint8_t* src, uint8_t* dst, int32_t N, int64_t per, double std, int64_t seed, int64_t index0, void* stream);

/* ---- PNG files from resident 8-bit images (csrc/png.hip) ----------------------------------------------------------------------------
 * `python -m dasr_amd.prepare_data --device_png`, `add_corruptions --device_png` (dasr_amd/png.py states the stream in numpy and pure Python).  The deflate stream of an
 * image is the concatenation of independently coded STRIPS of whole rows (at most 65 535 filtered bytes each), without LZ77: per strip one dynamic-Huffman block (BFINAL 0)
 * followed by an empty stored block that byte-aligns it (zlib's Z_SYNC_FLUSH), or one stored block where that is smaller.  The host adds 78 01 in front, 03 00 (an empty
 * final fixed-Huffman block) and the Adler-32 behind, and the PNG container.  A batch of images is one call per stage.  Asynchronous on `stream`, nothing is synchronised,
 * plain loads and stores and LDS atomics only, same inputs give the same bits.
 *
 * Tables: images [n_images] and strips [n_strips] in device memory, and the same arrays in HOST memory (the staging buffer they were uploaded from), which is what every
 * call validates before it launches.  An image is interleaved RGB bytes, `pitch` bytes from row to row (a window of a larger image: src points at its first pixel); its
 * strips are strips[first_strip .. first_strip + n_strips).  Strip s covers rows [row0, row0 + rows) of image `image`; n = rows (1 + 3 W) is its count of filtered bytes;
 * they stand at filt + filt_off (a multiple of 16; the strip owns n rounded up to 16 bytes there) and its coded bytes at slots + slot_off (a multiple of 4; the slot is
 * DASR_PNG_SLOT_BYTES(n) = n + 16 rounded up to 4 bytes).
 *
 * dasr_png_filter: per row the five PNG filter types with bpp 3 (None, Sub, Up, Average with floor((left + up) / 2), Paeth with tie order a, b, c; the row above an
 * image's first row is zeros, the row above a strip's first row is the row above it in the image); cost of a type = sum of min(b, 256 - b) over the row's 3 W filtered
 * bytes, the smallest wins, ties to the lowest type; the row is written as type byte + filtered bytes.  hist [n_strips][257]: counts of the strip's byte values (type
 * bytes included) and end-of-block = 1.  adler [n_strips][2]: s1 = sum b_i mod 65521, s2 = sum (n - i) b_i mod 65521 over the strip's bytes b_0 .. b_(n-1) (Adler-32
 * run from s1 = s2 = 0; the stream's checksum follows from (1, 0) by s2 += n s1 + strip.s2, s1 += strip.s1).
 *
 * dasr_png_codes: hist [n][257] (sum below 2^32; below 2^28 for hdr[1]) -> lens [n][257] (<= 15; 0 for an unused symbol), codes [n][257] (canonical, RFC 1951
 * 3.2.2, as numbers: deflate packs them starting from the most significant bit) and hdr [n][DASR_PNG_HDR_WORDS]: [0] bits of the block header, [1] bits of the coded
 * symbols sum hist lens, [2] HLIT | HDIST << 8 | HCLEN << 16 (0, 1, number of code-length codes - 4), [3] 0, [4 ..] the header's bits, LSB first: BFINAL 0, BTYPE 10,
 * HLIT, HDIST, HCLEN, the lengths (<= 7) of the code-length code in the order 16, 17, 18, 0, 8, ..., then the 257 lengths and the two distance lengths (1, 1: what zlib's
 * Z_HUFFMAN_ONLY streams declare) one by one in that code (no run symbols 16 - 18).  The code is complete (Kraft sum 1).  It is a Huffman code (two-queue construction on
 * the symbols sorted by (count, symbol)) where that tree is no deeper than 15; a deeper tree has its counts per length repaired (one code leaves length 15, one moves a
 * level down, until the Kraft sum is 1) and the lengths handed out again by count.  Fewer than two used symbols: two codes of one bit.
 *
 * dasr_png_emit: one workgroup per strip writes its block into its slot and its size into sizes [n_strips]: the header, the codes bit-reversed and LSB first at the bit
 * offsets an exclusive scan of the code lengths gives, end-of-block, three zero bits, padding to a byte, 00 00 FF FF; a strip that would take more than n + 5 bytes is
 * 00, LEN, ~LEN and its n bytes.  Bits are put together in LDS and stored as whole words; a word outside the slot is not stored and sets bit 0 of *status (device
 * memory, 8 bytes, zeroed by the caller; meta[0] of dasr_png_pack).  lens above 15 are read as 15.
 *
 * dasr_png_pack: an exclusive scan of the sizes (ws: n_strips x 8 bytes of scratch), the strips gathered in order into out (4-byte aligned, out_bytes: the sum of the
 * slots always suffices), and meta [n_images + 3]: [0] status (bit 1: a size above its slot, bit 2: a strip beyond out_bytes; such strips are left out), [1] total
 * bytes, [2 + i] offset of image i's first strip, [2 + n_images] the total again.  Two launches, no host loop.
 *
 * DASR_EINVAL, nothing launched: a null pointer, n_images or n_strips < 1, an image with H or W < 1, W > 21 844 (a row above 65 535 filtered bytes) or pitch < 3 W, a
 * strip outside its image, with n != rows (1 + 3 W) or n > 65 535, with a misaligned offset or beyond filt_bytes / slots_bytes, a misaligned buffer. */
#define DASR_PNG_HDR_WORDS 64
#define DASR_PNG_SLOT_BYTES(n) (((n) + 16 + 3) / 4 * 4)
typedef struct {
    const uint8_t* src;
    int64_t pitch;                   /* bytes from row to row */
    int32_t H, W;
    int32_t first_strip, n_strips;
} dasr_png_image;
typedef struct {
    int32_t image, row0, rows, n;    /* n = rows (1 + 3 W) filtered bytes */
    int64_t filt_off, slot_off;
} dasr_png_strip;
int dasr_png_filter(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                    const dasr_png_strip* strips_host, int32_t n_strips, uint8_t* filt, int64_t filt_bytes, uint32_t* hist, uint32_t* adler, void* stream);
int dasr_png_codes(const uint32_t* hist, int32_t n, uint8_t* lens, uint16_t* codes, uint32_t* hdr, void* stream);
int dasr_png_emit(const dasr_png_strip* strips_dev, const dasr_png_strip* strips_host, int32_t n_strips, const uint8_t* filt, int64_t filt_bytes, const uint8_t* lens,
                  const uint16_t* codes, const uint32_t* hdr, uint8_t* slots, int64_t slots_bytes, uint32_t* sizes, uint64_t* status, void* stream);
int dasr_png_pack(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                  const dasr_png_strip* strips_host, int32_t n_strips, const uint32_t* sizes, const uint8_t* slots, int64_t slots_bytes, uint64_t* ws, uint8_t* out,
                  int64_t out_bytes, uint64_t* meta, void* stream);
/* The same two stages for the other pixel layouts the drivers hold (`"device_png": true` of the SRN option files, `back_projection --device_png`,
 * `dsn_create_dataset --device_png`); one batch has one fmt, with bpp bytes per pixel in source and file:
 *   DASR_PNG_RGB  interleaved RGB, bpp 3: the bits of dasr_png_filter / dasr_png_pack.
 *   DASR_PNG_BGR  interleaved BGR (util.tensor2img's order), bpp 3: byte j of a PNG row is source byte 3 (j / 3) + 2 - j % 3, its left and upper-left neighbours the same
 *                 channel of the pixel to the left: the output of DASR_PNG_RGB on the channel-reversed image (the file is colour type 2, RGB).
 *   DASR_PNG_GREY one channel [H, W], bpp 1, PNG colour type 0: a row has W bytes, the left neighbour is the byte before.
 * Everything above holds with bpp in place of 3: n = rows (1 + bpp W), pitch >= bpp W, W <= (65 535 - 1) / bpp (21 844 or 65 534).  Any other fmt is DASR_EINVAL.
 * dasr_png_codes and dasr_png_emit see filtered bytes and strip sizes only and serve every fmt. */
#define DASR_PNG_RGB 0
#define DASR_PNG_BGR 1
#define DASR_PNG_GREY 2
int dasr_png_filter_fmt(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                        const dasr_png_strip* strips_host, int32_t n_strips, uint8_t* filt, int64_t filt_bytes, uint32_t* hist, uint32_t* adler, int32_t fmt, void* stream);
int dasr_png_pack_fmt(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                      const dasr_png_strip* strips_host, int32_t n_strips, const uint32_t* sizes, const uint8_t* slots, int64_t slots_bytes, uint64_t* ws, uint8_t* out,
                      int64_t out_bytes, uint64_t* meta, int32_t fmt, void* stream);

/* ---- profiling session (bench.py `roofline`) -----------------------------------------------------------
 * Between dasr_prof_begin and dasr_prof_end every kernel launch of the library (up to `capacity`) carries its own start/stop
 * events on its launch stream (hipExtLaunchKernel: the dispatch's begin/end timestamps, what rocprofv3 --kernel-trace prints).
 * dasr_prof_end synchronises the device and returns, per launch in issue order: duration in microseconds, the algorithmic
 * flops / bytes of the op it belongs to (dasr_op.flops / .bytes, attributed to the op's first launch), the op kind (bits 0-7; bits 8-15: the
 * plan builder's time-bucket tag dasr_op.i[7], which no kernel reads) and a
 * static string naming the kernel variant.  Returns the number of records written (<= max_out) or a negative error.
 * A launch made outside dasr_run_ops (a plain entry point: dasr_adam, dasr_fill_f32, dasr_add_flat, ...) records kind 0, bucket 0, no flops and no
 * bytes, whatever list ran before it on the thread.  `capacity` is that of the session it opens, whatever earlier sessions asked for; <= 0: DASR_EINVAL. */
int dasr_prof_begin(int32_t capacity);
int dasr_prof_end(int32_t max_out, float* us_out, double* flops_out, double* bytes_out, int32_t* op_out, const char** tag_out);
/* Restricts the NEXT profiling sessions to launches whose tag (kernel name / launcher signature) contains `substr` (NULL or "": every launch again).  A session over
 * one kernel family costs two events per matching launch and nothing else: bench.py times the dominant kernel this way over ordinary steps (round 6: a step in which
 * EVERY launch carries events runs ~6 % slower and over-reported the chained launches by 7-11 %).  DASR_EINVAL while a session is open. */
int dasr_prof_filter(const char* substr);

/* ---- diagnostics ----------------------------------------------------------------------------------*/
int dasr_abi_version(void);
/* Frees the scratch rows of the deterministic grid sums (one per (device, loss accumulator, stream), allocated on first use and otherwise kept for the life of the
 * process).  The caller guarantees that no launch of this library is in flight.  Returns 0. */
int dasr_red_release(void);
/* 1 if ds_read_b64_tr_b16 has the lane mapping the wgrad kernel assumes on this device, 0 if not, <0 on error.
 * Must be called once per process before dasr_wgrad (it also selects the wgrad gather mode). */
int dasr_probe_tr16(void* stream);
/* naive fp32 direct convolution (one thread per output), used by tests as an on-device cross-check */
int dasr_conv_naive(const dasr_conv_params* p, const float* w_ref /* [cout][cin][kh][kw] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif

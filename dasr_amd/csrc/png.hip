// PNG encoding of 8-bit images resident in device memory (interleaved RGB, interleaved BGR written as RGB, or one grey channel), without LZ77 (dasr_amd/png.py states the
// same stream in numpy and pure Python):
//  * png_filter_kernel: per row the PNG filter type with the smallest sum of min(b, 256 - b), the filtered bytes, and per strip of rows the histogram and the Adler-32 partials.
//  * png_codes_kernel: per strip a length-limited Huffman code for its 257 symbols, the canonical codes and the bits of the dynamic block's header.
//  * png_emit_kernel: per strip the deflate block (or a stored block where that is smaller) and the empty stored block that byte-aligns it, into the strip's slot.
//  * png_scan_kernel + png_gather_kernel: exclusive scan of the strip sizes, the strips of all images gathered into one buffer, the per-image offsets.
// A batch is described by dasr_png_image / dasr_png_strip tables; the launchers validate the HOST copies of the tables, so a kernel never indexes outside a buffer the
// caller sized as the header says.  Plain loads and stores and LDS atomics only; nothing is synchronised.
#include "common.h"

namespace {

constexpr int SYMS = 257;             // byte values and end-of-block
constexpr int MAX_STRIP = 65535;
constexpr int max_w(int bpp) { return (MAX_STRIP - 1) / bpp; }   // 1 + bpp W <= 65 535: 21 844 for three bytes per pixel, 65 534 for one
constexpr int ADLER_MOD = 65521;
constexpr int HDR_WORDS = DASR_PNG_HDR_WORDS;

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- 1. filter ------------------------------------------------------------------------------------------------------------------------
// grid (n_strips), 256 threads: wave w takes rows w, w + 4, ... of the strip, one byte per lane and step.  First sweep: the five costs of the row; second sweep: the bytes of the
// winning type, the histogram (one copy per wave in LDS) and the two Adler sums (64-bit per lane: (n - i) b < 2^24 per byte, < 2^40 per strip).
// BPP: bytes per pixel of source and file (3: colour type 2, 1: colour type 0).  REV (BPP 3): the source is BGR, byte j of a PNG row is source byte 3 (j / 3) + 2 - j % 3; its
// left neighbour is the same channel of the pixel to the left, BPP source bytes back, so the output is that of the channel-reversed image.
template <int BPP, bool REV>
__device__ __forceinline__ int src_index(int j) {
    if constexpr (REV) return j + 2 - 2 * (j % 3);
    else return j;
}

template <int BPP, bool REV>
__global__ __launch_bounds__(256) void png_filter_kernel(const dasr_png_image* __restrict__ images, const dasr_png_strip* __restrict__ strips, uint8_t* __restrict__ filt,
                                                         uint32_t* __restrict__ hist, uint32_t* __restrict__ adler) {
    __shared__ uint32_t h[4][SYMS];
    __shared__ unsigned long long red[4][2];
    const dasr_png_strip S = strips[blockIdx.x];
    const dasr_png_image I = images[S.image];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 4 * SYMS; i += 256) (&h[0][0])[i] = 0u;
    __syncthreads();
    const int rb = BPP * I.W, stride = rb + 1, n = S.rows * stride;
    uint8_t* out = filt + S.filt_off;
    unsigned long long s1 = 0, s2 = 0;
    for (int r = wave; r < S.rows; r += 4) {
        const int y = S.row0 + r;
        const uint8_t* cur = I.src + (int64_t)y * I.pitch;
        const uint8_t* up = cur - I.pitch;   // (read only where y > 0)
        const bool has_up = y > 0;
        uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
        for (int j = lane; j < rb; j += 64) {
            const int q = src_index<BPP, REV>(j);
            const int x = cur[q], a = j >= BPP ? cur[q - BPP] : 0, b = has_up ? up[q] : 0, c = (has_up && j >= BPP) ? up[q - BPP] : 0;
            const int v[5] = {x, (x - a) & 255, (x - b) & 255, (x - ((a + b) >> 1)) & 255, (x - paeth(a, b, c)) & 255};
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += (uint32_t)min(v[t], 256 - v[t]);
        }
        int best = 0;
        uint32_t best_cost = 0u;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            uint32_t cst = cost[t];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cst += __shfl_xor(cst, o, 64);
            if (t == 0 || cst < best_cost) { best = t; best_cost = cst; }   // ties: the lowest type
        }
        const int pos0 = r * stride;
        if (lane == 0) {
            out[pos0] = (uint8_t)best;
            atomicAdd(&h[wave][best], 1u);
            s1 += (unsigned)best;
            s2 += (unsigned long long)(n - pos0) * (unsigned)best;
        }
        for (int j = lane; j < rb; j += 64) {
            const int q = src_index<BPP, REV>(j);
            const int x = cur[q], a = j >= BPP ? cur[q - BPP] : 0, b = has_up ? up[q] : 0, c = (has_up && j >= BPP) ? up[q - BPP] : 0;
            const int pred = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : paeth(a, b, c);
            const int v = (x - pred) & 255, pos = pos0 + 1 + j;
            out[pos] = (uint8_t)v;
            atomicAdd(&h[wave][v], 1u);
            s1 += (unsigned)v;
            s2 += (unsigned long long)(n - pos) * (unsigned)v;
        }
    }
    s1 = wave_sum_u64(s1);
    s2 = wave_sum_u64(s2);
    if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
    __syncthreads();
    for (int i = tid; i < SYMS; i += 256) hist[(size_t)blockIdx.x * SYMS + i] = h[0][i] + h[1][i] + h[2][i] + h[3][i] + (i == 256 ? 1u : 0u);
    if (tid == 0) {
        adler[2 * (size_t)blockIdx.x] = (uint32_t)((red[0][0] + red[1][0] + red[2][0] + red[3][0]) % ADLER_MOD);
        adler[2 * (size_t)blockIdx.x + 1] = (uint32_t)((red[0][1] + red[1][1] + red[2][1] + red[3][1]) % ADLER_MOD);
    }
}

// ---- 2. codes -------------------------------------------------------------------------------------------------------------------------
constexpr int HUFF_MAXN = 288;
struct huff_ws {
    uint32_t w[2 * HUFF_MAXN];     // weights: the used symbols in ascending (frequency, symbol) order, then the internal nodes in the order they are made
    uint16_t par[2 * HUFF_MAXN];   // parent of every node (always a higher index)
    uint16_t sym[HUFF_MAXN];       // symbol of every leaf
    uint32_t num[32];              // codes per length
    uint32_t next[16];             // first code of every length
    int n_used;
};

// Code lengths (<= maxlen <= 15) of a complete prefix code for the symbols with freq > 0, by the 64 lanes of a one-wave workgroup (every lane calls it; freq, lens and ws are
// LDS).  Rank sort in parallel, the two-queue Huffman construction on lane 0 (the heads of both queues kept in registers: one LDS read per node taken), the leaf depths in
// parallel by walking up the parents.  The counts per length of a tree deeper than maxlen are repaired as miniz does it: one code leaves the longest length and one moves a level
// down until the Kraft sum is 1.  The lengths are then handed out by frequency, the most frequent symbol first: for a tree within maxlen this has the cost of the Huffman tree
// (equal counts per length, the same order by frequency).  Fewer than two used symbols: two codes of one bit, as zlib pads a tree.  Needs sum freq < 2^32.
__device__ void build_lengths(const uint32_t* freq, int nsym, int maxlen, uint8_t* lens, huff_ws& ws) {
    const int lane = threadIdx.x;
    if (lane == 0) ws.n_used = 0;
    if (lane < 32) ws.num[lane] = 0u;
    __syncthreads();
    for (int s = lane; s < nsym; s += 64) {
        lens[s] = 0;
        const uint32_t f = freq[s];
        if (f) {
            int r = 0;
            for (int t = 0; t < nsym; ++t) {
                const uint32_t g = freq[t];
                r += (g && (g < f || (g == f && t < s))) ? 1 : 0;
            }
            ws.sym[r] = (uint16_t)s;
            ws.w[r] = f;
            atomicAdd(&ws.n_used, 1);
        }
    }
    __syncthreads();
    const int n = ws.n_used;
    if (n < 2) {
        if (lane == 0) {
            const int s = n ? ws.sym[0] : 0;
            lens[s] = 1;
            lens[s == 0 ? 1 : 0] = 1;
        }
        __syncthreads();
        return;
    }
    if (lane == 0) {
        // leaves [li, n) and internal nodes [qi, qe), both in ascending weight; wl / wq: the weights at their heads (all ones: that queue is empty); a leaf wins a tie
        // (the shallower tree)
        constexpr unsigned long long EMPTY = ~0ull;
        int li = 0, qi = n, qe = n;
        unsigned long long wl = ws.w[0], wq = EMPTY;
        for (int k = 0; k < n - 1; ++k) {
            uint32_t sum = 0u;
#pragma unroll
            for (int pick = 0; pick < 2; ++pick) {
                if (wl <= wq) {
                    sum += (uint32_t)wl;
                    ws.par[li++] = (uint16_t)qe;
                    wl = li < n ? (unsigned long long)ws.w[li] : EMPTY;
                } else {
                    sum += (uint32_t)wq;
                    ws.par[qi++] = (uint16_t)qe;
                    wq = qi < qe ? (unsigned long long)ws.w[qi] : EMPTY;
                }
            }
            ws.w[qe] = sum;
            if (qi == qe) wq = sum;   // (the queue of internal nodes was empty: the new node is its head)
            ++qe;
        }
    }
    __syncthreads();
    const int root = 2 * n - 2;
    for (int r = lane; r < n; r += 64) {
        int d = 0;
        for (int p = r; p != root && d < 2 * HUFF_MAXN; ++d) p = ws.par[p];
        atomicAdd(&ws.num[min(d, maxlen)], 1u);
    }
    __syncthreads();
    if (lane == 0) {
        uint32_t total = 0u;
        for (int i = maxlen; i >= 1; --i) total += ws.num[i] << (maxlen - i);
        for (int guard = 0; total > (1u << maxlen) && ws.num[maxlen] > 0u && guard < (1 << 16); ++guard) {
            ws.num[maxlen]--;
            for (int i = maxlen - 1; i > 0; --i)
                if (ws.num[i]) { ws.num[i]--; ws.num[i + 1] += 2u; break; }
            --total;
        }
    }
    __syncthreads();
    for (int r = lane; r < n; r += 64) {
        const uint32_t t = (uint32_t)(n - 1 - r);   // rank from the most frequent symbol
        int L = 1;
        uint32_t cum = ws.num[1];
        while (cum <= t && L < maxlen) { ++L; cum += ws.num[L]; }
        lens[ws.sym[r]] = (uint8_t)L;
    }
    __syncthreads();
}

// RFC 1951 3.2.2 by the 64 lanes (lens <= 15, codes and ws LDS): the counts per length, the first code of every length on lane 0, then for every symbol the first code of its
// length plus the number of lower symbols of the same length
__device__ void canonical_codes(const uint8_t* lens, int nsym, uint16_t* codes, huff_ws& ws) {
    const int lane = threadIdx.x;
    if (lane < 32) ws.num[lane] = 0u;
    __syncthreads();
    for (int s = lane; s < nsym; s += 64)
        if (lens[s]) atomicAdd(&ws.num[lens[s] & 15], 1u);
    __syncthreads();
    if (lane == 0) {
        uint32_t code = 0u;
        ws.next[0] = 0u;
        for (int b = 1; b <= 15; ++b) { code = (code + ws.num[b - 1]) << 1; ws.next[b] = code; }
    }
    __syncthreads();
    for (int s = lane; s < nsym; s += 64) {
        const int L = lens[s] & 15;
        uint32_t below = 0u;
        for (int t = 0; t < s; ++t) below += lens[t] == L ? 1u : 0u;
        codes[s] = L ? (uint16_t)(ws.next[L] + below) : (uint16_t)0;
    }
    __syncthreads();
}

// value (nbits <= 16 bits) OR-ed into a zeroed LDS bit string at bit position pos, LSB first
__device__ __forceinline__ void or_bits(uint32_t* words, uint32_t pos, uint32_t value, uint32_t nbits) {
    const uint32_t w = pos >> 5, sh = pos & 31u;
    if (nbits) atomicOr(&words[w], value << sh);
    if (sh + nbits > 32u) atomicOr(&words[w + 1], value >> (32u - sh));
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t code, int len) { return len ? __brev(code) >> (32 - len) : 0u; }

__device__ const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

constexpr int HDR_PER = 5;   // code lengths per lane in the header: 64 x 5 >= 257 + 2

// grid (n), 64 threads: one strip per one-wave workgroup
__global__ __launch_bounds__(64) void png_codes_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ lens_out, uint16_t* __restrict__ codes_out,
                                                       uint32_t* __restrict__ hdr_out) {
    __shared__ uint32_t freq[SYMS], clfreq[19], hdr[HDR_WORDS];
    __shared__ uint8_t lens[SYMS], cllens[19];
    __shared__ uint16_t codes[SYMS], clcodes[19];
    __shared__ huff_ws ws;
    __shared__ uint32_t fixed_bits;
    const int lane = threadIdx.x;
    const size_t k = blockIdx.x;
    for (int s = lane; s < SYMS; s += 64) freq[s] = hist[k * SYMS + s];
    if (lane < 19) clfreq[lane] = 0u;
    hdr[lane] = 0u;
    __syncthreads();
    build_lengths(freq, SYMS, 15, lens, ws);
    canonical_codes(lens, SYMS, codes, ws);
    for (int s = lane; s < SYMS; s += 64) atomicAdd(&clfreq[lens[s]], 1u);
    __syncthreads();
    if (lane == 0) clfreq[1] += 2u;   // the two distance codes of one bit
    __syncthreads();
    build_lengths(clfreq, 19, 7, cllens, ws);
    canonical_codes(cllens, 19, clcodes, ws);
    uint32_t* bits = hdr + 4;
    if (lane == 0) {
        int ncl = 4;
        for (int i = 0; i < 19; ++i)
            if (cllens[cl_order[i]]) ncl = max(ncl, i + 1);
        // BFINAL 0, BTYPE 10, HLIT 0 (257 codes), HDIST 1 (2 codes), HCLEN: 17 bits, then the lengths of the code-length code
        or_bits(bits, 0u, ((2u << 1) | (1u << 8) | ((uint32_t)(ncl - 4) << 13)) & 0xFFFFu, 16);
        or_bits(bits, 16u, (uint32_t)(ncl - 4) >> 3, 1);
        for (int i = 0; i < ncl; ++i) or_bits(bits, 17u + 3u * i, cllens[cl_order[i]], 3);
        fixed_bits = 17u + 3u * ncl;
        hdr[2] = 0u | (1u << 8) | ((uint32_t)(ncl - 4) << 16);
    }
    __syncthreads();
    // the 257 + 2 code lengths in the code-length code: HDR_PER per lane, placed by a scan over the wave; the coded size of the symbols by a sum over the wave
    uint32_t mine = 0u, body = 0u;
#pragma unroll
    for (int j = 0; j < HDR_PER; ++j) {
        const int e = lane * HDR_PER + j;
        if (e < SYMS + 2) mine += cllens[e < SYMS ? lens[e] : 1];
        if (e < SYMS) body += freq[e] * lens[e];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) body += __shfl_xor(body, o, 64);
    uint32_t pos = fixed_bits + incl - mine;
#pragma unroll
    for (int j = 0; j < HDR_PER; ++j) {
        const int e = lane * HDR_PER + j;
        if (e < SYMS + 2) {
            const int l = e < SYMS ? lens[e] : 1;
            or_bits(bits, pos, rev_bits(clcodes[l], cllens[l]), cllens[l]);
            pos += cllens[l];
        }
    }
    if (lane == 63) {
        hdr[0] = fixed_bits + incl;   // at most 3 + 14 + 19 * 3 + 259 * 7 = 1887 bits = 59 words
        hdr[1] = body;
    }
    __syncthreads();
    for (int s = lane; s < SYMS; s += 64) {
        lens_out[k * SYMS + s] = lens[s];
        codes_out[k * SYMS + s] = codes[s];
    }
    hdr_out[k * HDR_WORDS + lane] = hdr[lane];
}

// ---- 3. emit --------------------------------------------------------------------------------------------------------------------------
constexpr int EM_PER = 16;                 // symbols per thread and tile: one 16-byte load
constexpr int EM_TILE = 256 * EM_PER;      // symbols per tile
constexpr int EM_WORDS = 2048;             // words of the tile's bit buffer: 31 carried bits + 4096 x 15 bits = 1922 words at most

__device__ __forceinline__ int strip_cap(int n) { return (n + 16 + 3) & ~3; }

// one guarded word store into a strip's slot: an index outside the slot sets bit 0 of the status word and stores nothing
__device__ __forceinline__ void slot_store(uint32_t* slot32, int cap, uint32_t w, uint32_t v, unsigned long long* status) {
    if (4ull * (w + 1ull) <= (unsigned long long)cap) slot32[w] = v;
    else atomicOr(status, 1ull);
}

// grid (n_strips), 256 threads.  Tile by tile: every thread loads 16 consecutive symbols (the end-of-block symbol follows the strip's last byte), an exclusive scan of the
// threads' bit counts places them, the codes are OR-ed into the tile's bit buffer in LDS (word 0 starts with the bits carried over from the tile before), the whole words go to
// the slot with plain coalesced stores and the last partial word is carried on.
__global__ __launch_bounds__(256) void png_emit_kernel(const dasr_png_strip* __restrict__ strips, const uint8_t* __restrict__ filt, const uint8_t* __restrict__ lens,
                                                       const uint16_t* __restrict__ codes, const uint32_t* __restrict__ hdr, uint8_t* __restrict__ slots,
                                                       uint32_t* __restrict__ sizes, unsigned long long* __restrict__ status) {
    __shared__ uint32_t table[SYMS];   // bit-reversed code | length << 16
    __shared__ uint32_t buf[EM_WORDS];
    __shared__ uint32_t wave_tot[4];
    const dasr_png_strip S = strips[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S.n, cap = strip_cap(n);
    const uint32_t* H = hdr + (size_t)blockIdx.x * HDR_WORDS;
    const uint32_t hb = H[0], body = H[1];
    uint8_t* slot = slots + S.slot_off;
    uint32_t* slot32 = reinterpret_cast<uint32_t*>(slot);
    const uint8_t* src = filt + S.filt_off;
    const bool hdr_ok = hb >= 17u && hb <= 32u * (HDR_WORDS - 4) - 32u;
    const unsigned long long coded = ((unsigned long long)hb + body + 3ull + 7ull) / 8ull + 4ull;
    if (!hdr_ok || coded > (unsigned long long)n + 5ull) {   // one stored block: 00, LEN, ~LEN, the bytes
        if (tid < 5) {
            const uint32_t len = (uint32_t)n, nlen = ~len & 0xFFFFu;
            slot[tid] = tid == 0 ? 0 : tid == 1 ? (uint8_t)len : tid == 2 ? (uint8_t)(len >> 8) : tid == 3 ? (uint8_t)nlen : (uint8_t)(nlen >> 8);
        }
        for (int i = tid; i < n; i += 256) slot[5 + i] = src[i];   // (5 + n <= cap)
        if (tid == 0) sizes[blockIdx.x] = (uint32_t)(n + 5);
        return;
    }
    for (int s = tid; s < SYMS; s += 256) {
        const int L = min((int)lens[(size_t)blockIdx.x * SYMS + s], 15);   // (a length above 15 would overrun the bit buffer)
        table[s] = rev_bits(codes[(size_t)blockIdx.x * SYMS + s] & ((1u << L) - 1u), L) | ((uint32_t)L << 16);
    }
    const uint32_t hfull = hb >> 5;
    for (uint32_t w = tid; w < hfull; w += 256) slot_store(slot32, cap, w, H[4 + w], status);
    uint32_t carry = (hb & 31u) ? (H[4 + hfull] & ((1u << (hb & 31u)) - 1u)) : 0u;
    unsigned long long bitpos = hb;   // (the same in every thread)
    for (int e0 = 0; e0 <= n; e0 += EM_TILE) {
        for (int i = tid; i < EM_WORDS; i += 256) buf[i] = i == 0 ? carry : 0u;
        __syncthreads();   // (also: the table is complete)
        const int e = e0 + tid * EM_PER;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (e < n) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + e);   // (16-byte aligned; the strip's filtered bytes are padded to a multiple of 16)
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        }
        uint32_t t[EM_PER], mine = 0u;
#pragma unroll
        for (int k = 0; k < EM_PER; ++k) {
            const int idx = e + k;
            const uint32_t sym = idx < n ? ((v[k >> 2] >> (8 * (k & 3))) & 255u) : 256u;
            t[k] = idx <= n ? table[sym] : 0u;
            mine += t[k] >> 16;
        }
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, tile_bits = 0u;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_tot[w];
            tile_bits += wave_tot[w];
        }
        const uint32_t first = (uint32_t)(bitpos & 31ull);
        uint32_t start = first + before + incl - mine;
        uint32_t w = start >> 5, nb = start & 31u;
        unsigned long long acc = 0ull;
#pragma unroll
        for (int k = 0; k < EM_PER; ++k) {
            acc |= (unsigned long long)(t[k] & 0xFFFFu) << nb;
            nb += t[k] >> 16;
            if (nb >= 32u) {
                atomicOr(&buf[w], (uint32_t)acc);
                ++w;
                acc >>= 32;
                nb -= 32u;
            }
        }
        if (nb) atomicOr(&buf[w], (uint32_t)acc);
        __syncthreads();
        const uint32_t tot = first + tile_bits, nw = tot >> 5;
        const uint32_t gw = (uint32_t)(bitpos >> 5);
        for (uint32_t i = tid; i < nw; i += 256) slot_store(slot32, cap, gw + i, buf[i], status);
        carry = (tot & 31u) ? buf[nw] : 0u;
        bitpos += tile_bits;
        __syncthreads();   // (buf and wave_tot are rewritten by the next tile)
    }
    if (tid == 0) {
        // three zero bits of the empty stored block, padding to a byte, 00 00 FF FF
        const unsigned long long p = (bitpos + 3ull + 7ull) >> 3;   // byte index of LEN
        const unsigned long long size = p + 4ull;
        const uint32_t w0 = (uint32_t)(bitpos >> 5), w1 = (uint32_t)((size - 1ull) >> 2);
        for (uint32_t w = w0; w <= w1; ++w) {
            uint32_t val = w == w0 ? carry : 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned long long byte = 4ull * w + b;
                if (byte == p + 2ull || byte == p + 3ull) val |= 0xFFu << (8 * b);
            }
            slot_store(slot32, cap, w, val, status);
        }
        sizes[blockIdx.x] = size <= (unsigned long long)cap ? (uint32_t)size : 0u;
    }
}

// ---- 4. pack --------------------------------------------------------------------------------------------------------------------------
// one workgroup of 1024 threads: thread t sums a run of consecutive strips, an exclusive scan over the threads, then the offsets of its strips.  A size above its slot counts as 0
// and sets bit 1 of the status word.  meta: [0] status, [1] total bytes, [2 .. 2 + n_images] the offset of every image's first strip and the total again.
__global__ __launch_bounds__(1024) void png_scan_kernel(const dasr_png_image* __restrict__ images, int n_images, const dasr_png_strip* __restrict__ strips, int n_strips,
                                                        const uint32_t* __restrict__ sizes, unsigned long long* __restrict__ strip_dst, unsigned long long* __restrict__ meta) {
    __shared__ unsigned long long wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (n_strips + 1023) / 1024, s0 = min(tid * per, n_strips), s1 = min(s0 + per, n_strips);
    unsigned long long mine = 0ull;
    for (int s = s0; s < s1; ++s) {
        const uint32_t sz = sizes[s];
        if (sz > (uint32_t)strip_cap(strips[s].n)) atomicOr(meta, 2ull);
        else mine += sz;
    }
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long run = incl - mine, total = 0ull;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) run += wave_tot[w];
        total += wave_tot[w];
    }
    for (int s = s0; s < s1; ++s) {
        const uint32_t sz = sizes[s];
        strip_dst[s] = run;
        if (sz <= (uint32_t)strip_cap(strips[s].n)) run += sz;
    }
    __syncthreads();   // (the offsets written above are read below by other threads of this workgroup)
    for (int i = tid; i < n_images; i += 1024) meta[2 + i] = strip_dst[images[i].first_strip];
    if (tid == 0) { meta[1] = total; meta[2 + n_images] = total; }
}

// grid (n_strips), 256 threads: the strip's bytes from its (4-byte aligned) slot to out + strip_dst, as aligned words of the destination put together from two words of the slot;
// the bytes before the first and after the last whole word one by one.
__global__ __launch_bounds__(256) void png_gather_kernel(const dasr_png_strip* __restrict__ strips, const uint32_t* __restrict__ sizes, const uint8_t* __restrict__ slots,
                                                         const unsigned long long* __restrict__ strip_dst, uint8_t* __restrict__ out, unsigned long long out_bytes,
                                                         unsigned long long* __restrict__ status) {
    const dasr_png_strip S = strips[blockIdx.x];
    const int tid = threadIdx.x, cap = strip_cap(S.n);
    const uint32_t size = sizes[blockIdx.x];
    const unsigned long long d0 = strip_dst[blockIdx.x];
    if (size > (uint32_t)cap || d0 + size > out_bytes) {
        if (tid == 0) atomicOr(status, 4ull);
        return;
    }
    const uint8_t* src = slots + S.slot_off;
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);
    uint8_t* dst = out + d0;
    const uint32_t head = min((uint32_t)((4ull - (d0 & 3ull)) & 3ull), size);   // (out is 4-byte aligned)
    if ((uint32_t)tid < head) dst[tid] = src[tid];
    const uint32_t nwords = (size - head) >> 2, sh = 8u * head, capw = (uint32_t)cap >> 2;
    uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t j = tid; j < nwords; j += 256) {
        const uint32_t lo = src32[j], hi = (head && j + 1u < capw) ? src32[j + 1u] : 0u;   // (j + 1 words lie inside the slot: 4 j + head + 4 <= size <= cap)
        dst32[j] = head ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
    const uint32_t done = head + 4u * nwords;
    if ((uint32_t)tid < size - done) dst[done + tid] = src[done + tid];
}

// ---- validation of the host copies of the tables ---------------------------------------------------------------------------------------
bool images_ok(const dasr_png_image* im, int n_images, int n_strips, int bpp = 3) {
    if (!im || n_images < 1) return false;
    for (int i = 0; i < n_images; ++i) {
        const dasr_png_image& I = im[i];
        if (!I.src || I.H < 1 || I.W < 1 || I.W > max_w(bpp) || (I.H > 1 && I.pitch < bpp * (int64_t)I.W)) return false;
        if (I.first_strip < 0 || I.n_strips < 1 || (int64_t)I.first_strip + I.n_strips > n_strips) return false;
    }
    return true;
}

// filt_bytes / slots_bytes < 0: that buffer is not used by the call
bool strips_ok(const dasr_png_strip* st, int n_strips, const dasr_png_image* im, int n_images, int64_t filt_bytes, int64_t slots_bytes, int bpp = 3) {
    if (!st || n_strips < 1) return false;
    for (int s = 0; s < n_strips; ++s) {
        const dasr_png_strip& S = st[s];
        if (S.rows < 1 || S.row0 < 0 || S.n < 1 || S.n > MAX_STRIP) return false;
        if (im) {
            if (S.image < 0 || S.image >= n_images) return false;
            const dasr_png_image& I = im[S.image];
            if ((int64_t)S.row0 + S.rows > I.H || (int64_t)S.rows * (1 + bpp * (int64_t)I.W) != S.n) return false;
        }
        if (filt_bytes >= 0 && (S.filt_off < 0 || (S.filt_off & 15) || S.filt_off + ((S.n + 15) & ~15) > filt_bytes)) return false;
        if (slots_bytes >= 0 && (S.slot_off < 0 || (S.slot_off & 3) || S.slot_off + ((S.n + 16 + 3) & ~3) > slots_bytes)) return false;
    }
    return true;
}

// fmt of the _fmt entry points: 0 interleaved RGB, 1 interleaved BGR, 2 one channel; bytes per pixel, 0 for any other value
int fmt_bpp(int32_t fmt) { return fmt == 0 || fmt == 1 ? 3 : fmt == 2 ? 1 : 0; }

}  // namespace

extern "C" int dasr_png_filter_fmt(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                                   const dasr_png_strip* strips_host, int32_t n_strips, uint8_t* filt, int64_t filt_bytes, uint32_t* hist, uint32_t* adler, int32_t fmt,
                                   void* stream) {
    const int bpp = fmt_bpp(fmt);
    if (!bpp || !images_dev || !strips_dev || !filt || !hist || !adler || filt_bytes < 0 || ((uintptr_t)filt & 15)) return DASR_EINVAL;
    if (!images_ok(images_host, n_images, n_strips, bpp) || !strips_ok(strips_host, n_strips, images_host, n_images, filt_bytes, -1, bpp)) return DASR_EINVAL;
    const dim3 grid((unsigned)n_strips), block(256);
    if (fmt == 0) { DASR_LAUNCH_TAG("png_filter_kernel", (png_filter_kernel<3, false>), grid, block, 0, as_stream(stream), images_dev, strips_dev, filt, hist, adler); }
    else if (fmt == 1) { DASR_LAUNCH_TAG("png_filter_kernel<bgr>", (png_filter_kernel<3, true>), grid, block, 0, as_stream(stream), images_dev, strips_dev, filt, hist, adler); }
    else { DASR_LAUNCH_TAG("png_filter_kernel<grey>", (png_filter_kernel<1, false>), grid, block, 0, as_stream(stream), images_dev, strips_dev, filt, hist, adler); }
    return (int)hipGetLastError();
}

extern "C" int dasr_png_filter(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                               const dasr_png_strip* strips_host, int32_t n_strips, uint8_t* filt, int64_t filt_bytes, uint32_t* hist, uint32_t* adler, void* stream) {
    return dasr_png_filter_fmt(images_dev, images_host, n_images, strips_dev, strips_host, n_strips, filt, filt_bytes, hist, adler, 0, stream);
}

extern "C" int dasr_png_codes(const uint32_t* hist, int32_t n, uint8_t* lens, uint16_t* codes, uint32_t* hdr, void* stream) {
    if (!hist || !lens || !codes || !hdr || n < 1 || ((uintptr_t)codes & 1) || ((uintptr_t)hdr & 3) || ((uintptr_t)hist & 3)) return DASR_EINVAL;
    DASR_LAUNCH(png_codes_kernel, dim3((unsigned)n), dim3(64), 0, as_stream(stream), hist, lens, codes, hdr);
    return (int)hipGetLastError();
}

extern "C" int dasr_png_emit(const dasr_png_strip* strips_dev, const dasr_png_strip* strips_host, int32_t n_strips, const uint8_t* filt, int64_t filt_bytes, const uint8_t* lens,
                             const uint16_t* codes, const uint32_t* hdr, uint8_t* slots, int64_t slots_bytes, uint32_t* sizes, uint64_t* status, void* stream) {
    if (!strips_dev || !filt || !lens || !codes || !hdr || !slots || !sizes || !status || filt_bytes < 0 || slots_bytes < 0) return DASR_EINVAL;
    if (((uintptr_t)filt & 15) || ((uintptr_t)slots & 3) || ((uintptr_t)codes & 1) || ((uintptr_t)hdr & 3) || ((uintptr_t)status & 7)) return DASR_EINVAL;
    if (!strips_ok(strips_host, n_strips, nullptr, 0, filt_bytes, slots_bytes)) return DASR_EINVAL;
    DASR_LAUNCH(png_emit_kernel, dim3((unsigned)n_strips), dim3(256), 0, as_stream(stream), strips_dev, filt, lens, codes, hdr, slots, sizes,
                reinterpret_cast<unsigned long long*>(status));
    return (int)hipGetLastError();
}

extern "C" int dasr_png_pack_fmt(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                                 const dasr_png_strip* strips_host, int32_t n_strips, const uint32_t* sizes, const uint8_t* slots, int64_t slots_bytes, uint64_t* ws,
                                 uint8_t* out, int64_t out_bytes, uint64_t* meta, int32_t fmt, void* stream) {
    const int bpp = fmt_bpp(fmt);
    if (!bpp) return DASR_EINVAL;
    if (!images_dev || !strips_dev || !sizes || !slots || !ws || !out || !meta || slots_bytes < 0 || out_bytes < 0) return DASR_EINVAL;
    if (((uintptr_t)slots & 3) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)meta & 7)) return DASR_EINVAL;
    if (!images_ok(images_host, n_images, n_strips, bpp) || !strips_ok(strips_host, n_strips, images_host, n_images, -1, slots_bytes, bpp)) return DASR_EINVAL;
    DASR_LAUNCH(png_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), images_dev, n_images, strips_dev, n_strips, sizes, reinterpret_cast<unsigned long long*>(ws),
                reinterpret_cast<unsigned long long*>(meta));
    DASR_LAUNCH(png_gather_kernel, dim3((unsigned)n_strips), dim3(256), 0, as_stream(stream), strips_dev, sizes, slots, reinterpret_cast<const unsigned long long*>(ws), out,
                (unsigned long long)out_bytes, reinterpret_cast<unsigned long long*>(meta));
    return (int)hipGetLastError();
}

extern "C" int dasr_png_pack(const dasr_png_image* images_dev, const dasr_png_image* images_host, int32_t n_images, const dasr_png_strip* strips_dev,
                             const dasr_png_strip* strips_host, int32_t n_strips, const uint32_t* sizes, const uint8_t* slots, int64_t slots_bytes, uint64_t* ws, uint8_t* out,
                             int64_t out_bytes, uint64_t* meta, void* stream) {
    return dasr_png_pack_fmt(images_dev, images_host, n_images, strips_dev, strips_host, n_strips, sizes, slots, slots_bytes, ws, out, out_bytes, meta, 0, stream);
}

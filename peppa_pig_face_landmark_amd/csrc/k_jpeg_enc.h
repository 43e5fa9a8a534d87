// Baseline JPEG encoder (pf_encode_jpeg, jpeg_enc.inl): n packed BGR images of one size -> n complete JFIF files, every byte what
// libjpeg(-turbo) writes for the same quality and sampling with one restart interval per MCU row (specification: INTEGRATION.md 4g,
// numpy restatement: tests/jpeg_enc_ref.py).  The forward twin of k_jpeg.h.  Integers only.
//
//   jpeg_enc_blocks    one workgroup owns a strip of 128 pixel columns of one MCU row: BGR rows into LDS as the 32-bit words that
//                      hold them in global memory (redact_kernel's staging), colour conversion with the edge replication of the
//                      specification, chroma down-sampling, the "islow" forward DCT (8 threads per block: a row each, then a column
//                      each) and quantisation.  Output: one record of 64 int16 in zigzag order per block, in scan order, blocks that
//                      do not exist included (all AC zero, the DC of the block coded before them).  No plane goes to HBM.
//   jpeg_enc_entropy   one workgroup per restart interval (= MCU row), one block per thread and round of 256 blocks, the round's
//                      records staged in LDS: the block's bit length (its DC difference read from the neighbouring record), a
//                      prefix sum over the workgroup for the bit offsets, then every block deposits its bits in the interval's
//                      slice of the bit scratch: whole 32-bit words it owns are stored, its first and last word are ADDED (the
//                      bits of neighbours are disjoint, so the sum is the union; the emulator has no atomicOr).  Then the pad
//                      bits, the 0xFF bytes counted, and the interval's raw and stuffed byte lengths.  No device-wide fence: the
//                      slice is the workgroup's own until the kernel ends, barriers order its stores and adds (with fences the
//                      stage took 4.6 times as long: profiles/jpeg_encode_bench.json).
//   jpeg_enc_pack      one workgroup per interval: the sum of the stuffed lengths in front of it and of the whole image, the verdict
//                      against `capacity`, the header (first interval), the interval's bytes with 0x00 behind every 0xFF (positions
//                      from a prefix sum over the 0xFF counts), RSTm or EOI, sizes[i].
//
// Bounds: a block's code is at most PF_JPEG_ENC_BLOCK_BITS bits (bit sizes are clamped to those of 8-bit baseline, which they never
// exceed), an interval's slice of the bit scratch holds that many bits for every block and every word index is checked against the
// slice; the pack kernel writes at byte offsets below min(capacity, file length) of its own slot only.
#pragma once
#include <vector>

#include "k_jpeg.h"

// longest code of one block: DC 11 bits + 11 value bits (chroma table), 63 x (16 bits + 10 value bits), no end-of-block behind a last
// non-zero coefficient
#define PF_JPEG_ENC_BLOCK_BITS (22 + 63 * 26)
#define PF_JPEG_ENC_HEADER_MAX 640     // the header is 629 bytes
#define PF_JPEG_ENC_STRIP 128          // pixel columns of a jpeg_enc_blocks workgroup
#define PF_JPEG_ENC_MAXBLK 48          // blocks of a strip: 8 MCUs x 6 (4:2:0), 8 x 4 (4:2:2), 16 x 3 (4:4:4)

// The tables of one (height, width, quality, subsampling), built on the host and kept in device memory
struct JpegEncTables {
    unsigned short qdiv[2][64];        // 8 x quantiser, natural order
    unsigned dc[2][16];                // code << 5 | length, by bit size
    unsigned ac[2][256];               // by run << 4 | size
    unsigned char header[PF_JPEG_ENC_HEADER_MAX];
    int header_len;
};

struct JpegEncState {
    JpegEncTables* d_tab = nullptr; size_t tab_bytes = 0;
    short* d_coef = nullptr; size_t coef_bytes = 0;            // [images of a chunk][blocks][64]
    unsigned* d_bits = nullptr; size_t bits_bytes = 0;         // [intervals][words of an interval]
    int* d_len = nullptr; size_t len_bytes = 0;                // [intervals][2]: raw bytes, stuffed bytes
    unsigned char* d_in = nullptr; size_t in_bytes = 0;        // host images
    unsigned char* d_out = nullptr; size_t out_bytes = 0;      // host output
    int* d_sizes = nullptr; size_t sizes_bytes = 0;
    JpegEncTables h_tab;
    int key[4] = {0, 0, 0, 0};         // what h_tab / d_tab were built for
    void release() {
        void* ptrs[] = {d_tab, d_coef, d_bits, d_len, d_in, d_out, d_sizes};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = JpegEncState();
    }
};

struct JpegEncArgs {
    const unsigned char* images;       // image i of the chunk at images + i * img_stride
    long long img_stride;
    int row_stride;
    int n;                             // images of the chunk
    int H, W;
    int hs, vs;                        // luma sampling factors = chroma down-sampling
    int mcus_x, mcus_y;                // mcus_y = restart intervals of an image
    int bpm;                           // blocks per MCU: hs * vs + 2
    int strips, G;                     // strips of an MCU row, MCUs per strip
    int wb, hb;                        // luma blocks that exist
    int ch;                            // chroma rows that exist
    const JpegEncTables* tab;
    short* coef;
    unsigned* bits;
    unsigned words;                    // words of an interval's slice of `bits`
    int* len;
    unsigned char* out;                // slot i of the chunk at out + i * capacity
    size_t capacity;
    int* sizes;
};

__device__ __forceinline__ int pf_jpeg_enc_zigzag_pos(int natural) {      // natural (row-major) index -> zigzag position
    constexpr unsigned char t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                     41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                     46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[natural];
}

// One pass of the "islow" forward DCT, the forward twin of pf_jpeg_idct_1d: FIRST is the row pass (outputs scaled by 4), the
// column pass removes that scale and leaves the factor 8 the quantiser divides out.
template <bool FIRST>
__device__ __forceinline__ void pf_jpeg_fdct_1d(const int (&d)[8], int (&o)[8]) {
    constexpr int SH = FIRST ? 11 : 15, RND = 1 << (SH - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { o[0] = (t10 + t11) * 4; o[4] = (t10 - t11) * 4; }
    else { o[0] = (t10 + t11 + 2) >> 2; o[4] = (t10 - t11 + 2) >> 2; }
    const int ze = (t12 + t13) * 4433;
    o[2] = (ze + t13 * 6270 + RND) >> SH;
    o[6] = (ze - t12 * 15137 + RND) >> SH;
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    o[7] = (t4 * 2446 + z1 + z3 + RND) >> SH;
    o[5] = (t5 * 16819 + z2 + z4 + RND) >> SH;
    o[3] = (t6 * 25172 + z2 + z3 + RND) >> SH;
    o[1] = (t7 * 12299 + z1 + z4 + RND) >> SH;
}

// sign(c) * ((|c| + (d >> 1)) / d)
__device__ __forceinline__ int pf_jpeg_enc_quant(int c, int d) {
    const int a = c < 0 ? -c : c;
    const int q = (int)((unsigned)(a + (d >> 1)) / (unsigned)d);
    return c < 0 ? -q : q;
}

// Exclusive prefix sum of v over the 256 threads of a workgroup; *total is the sum.  s_w: 4 words of LDS.  Two barriers.
__device__ __forceinline__ unsigned pf_jpeg_enc_scan256(unsigned v, unsigned* s_w, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl(inc, max(lane - d, 0), 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                   // the previous use of s_w has been read
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned x = s_w[w];
        if (w < wave) before += x;
        all += x;
    }
    *total = all;
    return before + inc - v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// No byte outside [row start, row start + 3 W) of an input row is read: word loads only where all four bytes lie inside.
__global__ __launch_bounds__(256) void jpeg_enc_blocks(JpegEncArgs a) {
    constexpr int SW = PF_JPEG_ENC_STRIP;
    constexpr int WORDS = ((3 + SW * 3 + 3) / 4) | 1;
    __shared__ __attribute__((aligned(16))) unsigned s_raw[16 * WORDS];
    __shared__ __attribute__((aligned(16))) unsigned char s_ycc[3][16][SW];
    __shared__ int s_ws[PF_JPEG_ENC_MAXBLK * 65];
    __shared__ __attribute__((aligned(16))) short s_rec[PF_JPEG_ENC_MAXBLK * 64];
    const int t = threadIdx.x;
    int bid = blockIdx.x;
    const int strip = bid % a.strips; bid /= a.strips;
    const int my = bid % a.mcus_y, img = bid / a.mcus_y;
    const int H = a.H, W = a.W, hs = a.hs, vs = a.vs;
    const int x0 = strip * SW, y0 = my * 8 * vs;            // x0 < W and y0 < H: the strip holds a pixel
    const int rows = 8 * vs, vrows = min(rows, H - y0), vcols = min(SW, W - x0);
    const unsigned char* base = a.images + (size_t)img * a.img_stride;
    // ---- 1. the pixels that exist, as words ----
    const bool rows_aligned = (a.row_stride & 3) == 0;
    const int shift = rows_aligned ? (int)(((size_t)base + (size_t)x0 * 3) & 3) : 0;
    const int words = (shift + vcols * 3 + 3) / 4;          // <= WORDS
    const int row_bytes = W * 3;
    for (int i = t; i < vrows * words; i += 256) {
        const int r = i / words, wd = i - r * words;
        const unsigned char* row = base + (size_t)(y0 + r) * a.row_stride;
        const int bx = x0 * 3 - shift + 4 * wd;
        unsigned v = 0u;
        if (rows_aligned && bx >= 0 && bx + 4 <= row_bytes) {
            v = *reinterpret_cast<const unsigned*>(row + bx);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (bx + k >= 0 && bx + k < row_bytes) v |= (unsigned)row[bx + k] << (8 * k);
        }
        s_raw[r * WORDS + wd] = v;
    }
    __syncthreads();
    // ---- 2. colour; the last column and the last row repeat ----
    for (int i = t; i < rows * SW; i += 256) {
        const int r = i / SW, c = i - r * SW;
        const unsigned char* px = reinterpret_cast<const unsigned char*>(s_raw) + (size_t)min(r, vrows - 1) * WORDS * 4 + shift + min(c, vcols - 1) * 3;
        const int B = px[0], Gr = px[1], R = px[2];
        s_ycc[0][r][c] = (unsigned char)((19595 * R + 38470 * Gr + 7471 * B + 32768) >> 16);
        s_ycc[1][r][c] = (unsigned char)((-11059 * R - 21709 * Gr + 32768 * B + (128 << 16) + 32767) >> 16);
        s_ycc[2][r][c] = (unsigned char)((32768 * R - 27439 * Gr - 5329 * B + (128 << 16) + 32767) >> 16);
    }
    __syncthreads();
    // ---- 3. forward DCT: 8 threads per block ----
    const int G = min(a.G, a.mcus_x - strip * a.G), nblk = G * a.bpm, ny = hs * vs;
    for (int i = t; i < nblk * 8; i += 256) {               // row r of block b
        const int b = i >> 3, r = i & 7, m = b / a.bpm, k = b - m * a.bpm;
        int d[8], o[8];
        if (k < ny) {
            const int bx = m * hs + k % hs, by = k / hs;
            if (strip * a.G * hs + bx >= a.wb || my * vs + by >= a.hb) continue;      // a block that does not exist
            const unsigned char* p = &s_ycc[0][by * 8 + r][bx * 8];
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = (int)p[c] - 128;
        } else {
            const int comp = 1 + k - ny;
            const int rr = min(my * 8 + r, a.ch - 1) - my * 8;                         // the last down-sampled row repeats
            const unsigned char* p0 = &s_ycc[comp][rr * vs][m * 8 * hs];
            if (hs == 1) {
#pragma unroll
                for (int c = 0; c < 8; ++c) d[c] = (int)p0[c] - 128;
            } else if (vs == 1) {
#pragma unroll
                for (int c = 0; c < 8; ++c) d[c] = (((int)p0[2 * c] + (int)p0[2 * c + 1] + (c & 1)) >> 1) - 128;
            } else {
                const unsigned char* p1 = p0 + SW;
#pragma unroll
                for (int c = 0; c < 8; ++c) d[c] = (((int)p0[2 * c] + (int)p0[2 * c + 1] + (int)p1[2 * c] + (int)p1[2 * c + 1] + 1 + (c & 1)) >> 2) - 128;
            }
        }
        pf_jpeg_fdct_1d<true>(d, o);
#pragma unroll
        for (int c = 0; c < 8; ++c) s_ws[b * 65 + r * 8 + c] = o[c];
    }
    __syncthreads();
    for (int i = t; i < nblk * 8; i += 256) {               // column c of block b
        const int b = i >> 3, c = i & 7, m = b / a.bpm, k = b - m * a.bpm;
        if (k < ny) {
            const int bx = m * hs + k % hs, by = k / hs;
            if (strip * a.G * hs + bx >= a.wb || my * vs + by >= a.hb) continue;
        }
        const unsigned short* q = a.tab->qdiv[k < ny ? 0 : 1];
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = s_ws[b * 65 + r * 8 + c];
        pf_jpeg_fdct_1d<false>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_rec[b * 64 + pf_jpeg_enc_zigzag_pos(r * 8 + c)] = (short)pf_jpeg_enc_quant(o[r], (int)q[r * 8 + c]);
    }
    __syncthreads();
    // ---- 4. blocks that do not exist: the DC of the last block of the MCU that does, no AC ----
    for (int i = t; i < nblk * 8; i += 256) {
        const int b = i >> 3, part = i & 7, m = b / a.bpm, k = b - m * a.bpm;
        if (k == 0 || k >= ny) continue;
        const int bx = m * hs + k % hs, by = k / hs;
        if (strip * a.G * hs + bx < a.wb && my * vs + by < a.hb) continue;
        int src = k - 1;                                    // block 0 of an MCU always exists
        while (src > 0 && (strip * a.G * hs + m * hs + src % hs >= a.wb || my * vs + src / hs >= a.hb)) --src;
#pragma unroll
        for (int e = 0; e < 8; ++e) s_rec[b * 64 + part * 8 + e] = (short)0;
        if (part == 0) s_rec[b * 64] = s_rec[(b - k + src) * 64];
    }
    __syncthreads();
    // ---- 5. the strip's records are contiguous in scan order ----
    const size_t first = (((size_t)img * a.mcus_y + my) * a.mcus_x + (size_t)strip * a.G) * a.bpm;
    uint4* dst = reinterpret_cast<uint4*>(a.coef + first * 64);
    for (int i = t; i < nblk * 8; i += 256) dst[i] = reinterpret_cast<const uint4*>(s_rec)[i];
}

// ------------------------------------------------------------------------------------------------------------------------------
// bit size of a coefficient or DC difference, clamped to what baseline allows (which the arithmetic never exceeds)
__device__ __forceinline__ int pf_jpeg_enc_size(int v, int cap) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? min(32 - __builtin_clz(a), cap) : 0;
}

// the record whose DC predicts block b of an interval (b >= bpm, or k > 0 for luma; else the prediction is 0)
__device__ __forceinline__ int pf_jpeg_enc_pred(const short* rec, int b, int k, int ny, int bpm) {
    if (k < ny) {
        if (k > 0) return rec[(size_t)(b - 1) * 64];
        return b ? rec[(size_t)(b - bpm + ny - 1) * 64] : 0;
    }
    return b >= bpm ? rec[(size_t)(b - bpm) * 64] : 0;
}

struct PfJpegBitWriter {
    unsigned* base;
    unsigned words, w;
    unsigned long long acc;
    int n;
    bool first;
    __device__ __forceinline__ void open(unsigned* slice, unsigned slice_words, unsigned bit) {
        base = slice; words = slice_words; w = bit >> 5; n = (int)(bit & 31u); acc = 0ull; first = true;
    }
    __device__ __forceinline__ void put(unsigned bits, int len) {      // len <= 27
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            n -= 32;
            const unsigned word = (unsigned)(acc >> n);
            if (w < words) {
                if (first) atomicAdd(&base[w], word);       // shared with the blocks in front
                else base[w] = word;                        // owned
            }
            first = false;
            ++w;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void close() {               // shared with the blocks behind
        if (n > 0 && w < words) atomicAdd(&base[w], (unsigned)(acc << (32 - n)));
    }
};

// bytes 0 .. nbytes-1 of a big-endian bit stream held in words: how many of the 4 bytes of word i exist, how many are 0xFF
__device__ __forceinline__ int pf_jpeg_enc_ff(unsigned word, int valid) {
    int ff = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < valid && ((word >> (24 - 8 * k)) & 255u) == 255u) ++ff;
    return ff;
}

// A round: 256 consecutive blocks.  Their records are contiguous, so they come into LDS with coalesced 16-byte loads (pitch 33 words:
// thread t walks record t, and 33 t + j / 2 puts the 64 lanes on 64 banks); a thread collects the bit mask of its record's non-zero
// coefficients and walks those twice, for the length and for the bits, from LDS.  The words a round's bits reach are zeroed in that round: from the first word that begins inside the round's
// bit range (the word in front is shared with the previous round, which zeroed it) to the word its last bit falls in.
__global__ __launch_bounds__(256) void jpeg_enc_entropy(JpegEncArgs a) {
    __shared__ unsigned s_dc[2][16], s_ac[2][256];
    __shared__ unsigned s_rec[256 * 33];
    __shared__ unsigned s_w[4];
    __shared__ unsigned s_ff;
    const int t = threadIdx.x;
    const int interval = blockIdx.x;                        // image of the chunk * mcus_y + MCU row
    const int nb = a.mcus_x * a.bpm, ny = a.hs * a.vs;
    const short* rec = a.coef + (size_t)interval * nb * 64;
    unsigned* slice = a.bits + (size_t)interval * a.words;
    for (int i = t; i < 512; i += 256) s_ac[i >> 8][i & 255] = a.tab->ac[i >> 8][i & 255];
    if (t < 32) s_dc[t >> 4][t & 15] = a.tab->dc[t >> 4][t & 15];
    if (t == 0) s_ff = 0u;
    unsigned run_bits = 0u;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int nt = min(256, nb - b0);
        __syncthreads();                                    // the tables are there; the previous round's records have been read
        const uint4* src = reinterpret_cast<const uint4*>(rec + (size_t)b0 * 64);
        for (int i = t; i < nt * 8; i += 256) {
            const uint4 v = src[i];
            unsigned* d = &s_rec[(i >> 3) * 33 + (i & 7) * 4];
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
        // ---- 1, 2. bit lengths and bit offsets ----
        const int b = b0 + t;
        const short* r = reinterpret_cast<const short*>(&s_rec[t * 33]);
        const int k = b % a.bpm, tb = k < ny ? 0 : 1;
        int diff = 0, s = 0;
        unsigned len = 0u;
        unsigned long long nz = 0ull;
        if (b < nb) {
            diff = (int)r[0] - pf_jpeg_enc_pred(rec, b, k, ny, a.bpm);
            s = pf_jpeg_enc_size(diff, 11);
            len = (s_dc[tb][s] & 31u) + (unsigned)s;
            // bit j: coefficient j is not zero; both walks visit those only (a photograph's block has a handful)
            const unsigned* rw = &s_rec[t * 33];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const unsigned w = rw[i];
                if (w & 0xFFFFu) nz |= 1ull << (2 * i);
                if (w >> 16) nz |= 2ull << (2 * i);
            }
            nz &= ~1ull;
            int prev = 0;
            for (unsigned long long m = nz; m; m &= m - 1ull) {
                const int j = __builtin_ctzll(m), zr = j - prev - 1;
                prev = j;
                len += (unsigned)(zr >> 4) * (s_ac[tb][0xF0] & 31u);
                const int sz = pf_jpeg_enc_size((int)r[j], 10);
                len += (s_ac[tb][((zr & 15) << 4) | sz] & 31u) + (unsigned)sz;
            }
            if (prev != 63) len += s_ac[tb][0] & 31u;
        }
        unsigned total;
        const unsigned ex = pf_jpeg_enc_scan256(len, s_w, &total);
        const unsigned z0 = (run_bits + 31u) >> 5, z1 = min((run_bits + total + 31u) >> 5, a.words);
        for (unsigned i = z0 + t; i < z1; i += 256) slice[i] = 0u;
        __syncthreads();                                    // the zeroes are written before any lane adds into them (one workgroup, one L2)
        // ---- 3. every block deposits its bits ----
        if (b < nb) {
            PfJpegBitWriter wr;
            wr.open(slice, a.words, run_bits + ex);
            const unsigned dcode = s_dc[tb][s];
            wr.put(dcode >> 5, (int)(dcode & 31u));
            if (s) wr.put((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
            int prev = 0;
            for (unsigned long long m = nz; m; m &= m - 1ull) {
                const int j = __builtin_ctzll(m);
                int zr = j - prev - 1;
                prev = j;
                for (; zr > 15; zr -= 16) wr.put(s_ac[tb][0xF0] >> 5, (int)(s_ac[tb][0xF0] & 31u));
                const int v = r[j], sz = pf_jpeg_enc_size(v, 10);
                const unsigned code = s_ac[tb][(zr << 4) | sz];
                wr.put(((code >> 5) << sz) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u)), (int)(code & 31u) + sz);
            }
            if (prev != 63) wr.put(s_ac[tb][0] >> 5, (int)(s_ac[tb][0] & 31u));
            wr.close();
        }
        run_bits += total;
    }
    // ---- 5a. the last byte is filled with ones ----
    const unsigned nbytes = (run_bits + 7u) >> 3, nwords = min((nbytes + 3u) >> 2, a.words);
    if (t == 0 && (run_bits & 7u)) {
        const unsigned pad = 8u - (run_bits & 7u), w = run_bits >> 5;
        if (w < a.words) atomicAdd(&slice[w], ((1u << pad) - 1u) << (32u - (run_bits & 31u) - pad));
    }
    __syncthreads();
    // ---- 4, 5b. the bytes that need stuffing, the interval's lengths.  The words are read where the adds went, in L2 (an add of 0):
    // a plain load may be served by a line the first-level cache kept from before the adds.  No device-wide fence anywhere: the
    // slice belongs to this workgroup until the kernel ends.
    unsigned ff = 0u;
    for (unsigned i = t; i < nwords; i += 256) ff += (unsigned)pf_jpeg_enc_ff(atomicAdd(&slice[i], 0u), (int)min(nbytes - 4u * i, 4u));
    if (ff) atomicAdd(&s_ff, ff);
    __syncthreads();
    if (t == 0) {
        const unsigned have = min(nbytes, a.words * 4u);    // equal: the slice holds every block at its longest
        a.len[2 * interval] = (int)have;
        a.len[2 * interval + 1] = (int)(have + s_ff);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Every store goes to out + img * capacity + p with p < min(capacity, file length).
__global__ __launch_bounds__(256) void jpeg_enc_pack(JpegEncArgs a) {
    __shared__ unsigned s_w[4];
    __shared__ unsigned long long s_sum[2];
    const int t = threadIdx.x;
    const int interval = blockIdx.x, img = interval / a.mcus_y, my = interval - img * a.mcus_y;
    const int* len = a.len + (size_t)img * a.mcus_y * 2;
    if (t < 2) s_sum[t] = 0ull;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
    for (int j = t; j < a.mcus_y; j += 256) {
        const unsigned long long l = (unsigned long long)len[2 * j + 1] + 2ull;      // + RSTm or EOI
        all += l;
        if (j < my) before += l;
    }
    if (before) atomicAdd(&s_sum[0], before);
    if (all) atomicAdd(&s_sum[1], all);
    __syncthreads();
    const int hl = a.tab->header_len;
    const unsigned long long file = (unsigned long long)hl + s_sum[1];                // < 2^31: pf_encode_jpeg_bound is
    const bool fits = file <= (unsigned long long)a.capacity;
    if (my == 0 && t == 0) a.sizes[img] = fits ? (int)file : -(int)file;
    if (!fits) return;                                      // uniform
    unsigned char* out = a.out + (size_t)img * a.capacity;
    const size_t limit = (size_t)file;                      // <= capacity
    if (my == 0)
        for (int i = t; i < hl; i += 256)
            if ((size_t)i < limit) out[i] = a.tab->header[i];
    const unsigned* slice = a.bits + (size_t)interval * a.words;
    const unsigned nbytes = (unsigned)len[2 * my];
    size_t pos = (size_t)hl + (size_t)s_sum[0];
    for (unsigned i0 = 0; i0 * 4u < nbytes; i0 += 256) {
        const unsigned i = i0 + t;
        const int valid = i * 4u < nbytes ? (int)min(nbytes - 4u * i, 4u) : 0;
        const unsigned word = valid ? slice[i] : 0u;
        unsigned total;
        const unsigned ex = pf_jpeg_enc_scan256((unsigned)pf_jpeg_enc_ff(word, valid), s_w, &total);
        size_t p = pos + 4u * (size_t)(i - i0) + ex;
        for (int k = 0; k < valid; ++k) {
            const unsigned char v = (unsigned char)(word >> (24 - 8 * k));
            if (p < limit) out[p] = v;
            ++p;
            if (v == 255) { if (p < limit) out[p] = 0; ++p; }
        }
        pos += (size_t)min(nbytes - 4u * i0, 1024u) + total;
    }
    if (t == 0) {
        if (pos < limit) out[pos] = 255;
        if (pos + 1 < limit) out[pos + 1] = (unsigned char)(my + 1 == a.mcus_y ? 0xD9 : 0xD0 + (my & 7));
    }
}

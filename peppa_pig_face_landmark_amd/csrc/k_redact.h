// Face redaction (pf_redact_faces / pf_face_redact, redact.inl): every frame byte is written once, the pixels the label maps of
// k_mask.h select are filled, pixelated or box-blurred, all others are their input.  The first kernel here that writes pixels.
//
//   redact_kernel<RMAX>   output-stationary: one workgroup owns one 128 x 16 tile of one output frame (the tiling of mask_fill_kernel,
//                         so a tile's labels are 2 KB and mosaic cells of 4, 8 and 16 never straddle tiles)
//
// The arithmetic is the specification and is restated in numpy by tests/redact_ref.py: integers only, the source
// of every sum is the input frame, so every byte is reproducible and independent of the tile order.
//
// A tile without a selected pixel -- the great majority -- copies its 16 row segments and touches no LDS.  Any other tile
//   1. stages its source footprint (the tile; for the blur the tile plus a halo of r, clipped to the frame) in LDS as the 32-bit
//      words that hold it in global memory: a row's first word starts 4-byte aligned and the shift is kept, as align_warp_kernel does;
//   2. sums it vertically: a thread owns one word column and carries the four byte sums as two packed pairs of 16-bit lanes (65 x 255
//      fits), sliding down the 16 rows of the tile, into s_v;
//   3. sums s_v horizontally: a thread owns four consecutive pixels of rows r and r + 8 and slides along them, only where one of the
//      four is selected; the 12 output bytes leave as three 32-bit words where the address allows it.
// A box sum is exact, so the separable evaluation gives the bytes of the specification.  LDS (source + sums + 4.3 KB of box list):
// RMAX 0: 22.4 KB, 8: 31.5 KB, 16: 42.1 KB, 32: 67.7 KB (two workgroups per CU); the launcher takes the smallest instance that holds
// the radius, and fill and mosaic take RMAX 0.
#pragma once
#include <vector>

#include "k_mask.h"

// modes and mask bits: PF_REDACT_FILL / _MOSAIC / _BLUR and PF_REDACT_BOX of include/peppa_hip.h
#define PF_REDACT_SHIFT 34            // (num * ceil(2^34 / n)) >> 34 == num / n for num < 2^21, n < 2^13 (see pf_redact_div)

// Host side of a handle: the label maps the redaction reads and the staging of host outputs
struct RedactState {
    unsigned char* d_labels = nullptr; size_t labels_bytes = 0;
    unsigned char* d_owners = nullptr; size_t owners_bytes = 0;
    int* d_valid = nullptr; size_t valid_bytes = 0;
    int* d_select = nullptr; size_t select_bytes = 0;
    AlignFrame* d_table = nullptr; size_t table_bytes = 0;
    unsigned char* d_out = nullptr; size_t out_bytes = 0;
    std::vector<int> h_valid;
    std::vector<AlignFrame> h_table;
    int stage_all = 0;                // measurement tool's build only: every tile goes through LDS, none is copied
    void release() {
        void* ptrs[] = {d_labels, d_owners, d_valid, d_select, d_table, d_out};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = RedactState();
    }
};

struct RedactArgs {
    const AlignFrame* frames;         // [images]: where output frame i reads its input
    const int* rec;                   // [n][PF_MASK_REC] of mask_edges_kernel: valid flag and clipped box
    const unsigned char* labels;      // [images][H][W]
    const unsigned char* owners;      // like labels; read only when select is given
    const int* select;                // optional [n]
    unsigned char* out;               // [images][H][W][3]
    int n, per;                       // slots, slots per image
    int H, W, tiles_x, tiles;
    int mode, label_mask, strength, pad;
    unsigned colour;
    unsigned n_in;                    // pixel count of an interior window / cell
    unsigned long long recip;         // ceil(2^PF_REDACT_SHIFT / n_in)
    int stage_all;                    // RedactState::stage_all
};

// floor(num / n), exact: num < 2^21 and n < 2^13.  With M = ceil(2^34 / n) and e = M n - 2^34 in [0, n), num M / 2^34 = num / n +
// num e / (n 2^34), and num e < 2^34 keeps the second term below 1 / n, so the floor is that of num / n.  Every other n (windows and
// cells the frame's border clips) takes the hardware's division sequence.
__device__ __forceinline__ unsigned pf_redact_div(unsigned num, unsigned n, unsigned n_in, unsigned long long recip) {
    return n == n_in ? (unsigned)(((unsigned long long)num * recip) >> PF_REDACT_SHIFT) : num / n;
}

// `lanes` threads copy n bytes: 16-byte vectors where both addresses allow them, else 32-bit words behind a common byte head, else bytes
__device__ __forceinline__ void pf_redact_copy(unsigned char* d, const unsigned char* s, int n, int lane, int lanes) {
    if ((((size_t)d | (size_t)s) & 15) == 0) {
        const int nv = n >> 4;
        for (int i = lane; i < nv; i += lanes) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        for (int i = (nv << 4) + lane; i < n; i += lanes) d[i] = s[i];
    } else if ((((size_t)d ^ (size_t)s) & 3) == 0) {
        const int head = min((int)((4 - ((size_t)s & 3)) & 3), n), nw = (n - head) >> 2;
        for (int i = lane; i < head; i += lanes) d[i] = s[i];
        for (int i = lane; i < nw; i += lanes) reinterpret_cast<unsigned*>(d + head)[i] = reinterpret_cast<const unsigned*>(s + head)[i];
        for (int i = head + (nw << 2) + lane; i < n; i += lanes) d[i] = s[i];
    } else {
        for (int i = lane; i < n; i += lanes) d[i] = s[i];
    }
}

// the rows (columns) summed for output row (column) v of a frame of `size`: the blur's window, the mosaic's cell, clipped
__device__ __forceinline__ void pf_redact_range(int mode, int strength, int v, int size, int* lo, int* hi) {
    if (mode == PF_REDACT_BLUR) { *lo = max(v - strength, 0); *hi = min(v + strength, size - 1); }
    else { *lo = v & ~(strength - 1); *hi = min(*lo + strength - 1, size - 1); }
}

// No byte outside [row start, row start + 3 W) of an input row is read and no byte outside `out` is written: word accesses are made
// only where all four bytes lie inside.  Every branch around a barrier depends on the arguments or on s_any and is uniform.
template <int RMAX>
__global__ __launch_bounds__(256) void redact_kernel(RedactArgs a) {
    constexpr int FW = PF_MASK_TW + 2 * RMAX, FH = PF_MASK_TH + 2 * RMAX;
    constexpr int WORDS = ((3 + FW * 3 + 3) / 4) | 1;            // odd pitch: the rows of the footprint start on different banks
    __shared__ __attribute__((aligned(16))) unsigned s_src[FH * WORDS];
    __shared__ __attribute__((aligned(16))) unsigned s_v[PF_MASK_TH][WORDS][2];      // [0]: sums of bytes 0 | 2 of the word column, [1]: 1 | 3
    __shared__ int s_box[256][4];
    __shared__ unsigned char s_hit[256];
    __shared__ int s_nbox, s_any;
    const int t = threadIdx.x;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
    const int tx0 = tile_x * PF_MASK_TW, ty0 = tile_y * PF_MASK_TH;
    const int H = a.H, W = a.W;
    const int slot0 = img * a.per, slot1 = min(slot0 + a.per, a.n);
    const int qx = (t & 31) * 4, ry = t >> 5;                    // this thread's pixels: columns qx .. qx + 3 of rows ry and ry + 8
    const int x = tx0 + qx, npx = min(4, W - x);                 // npx <= 0: no pixel
    if (t == 0) s_any = 0;
    __syncthreads();
    unsigned sel[2] = {0u, 0u};                                  // bit k: pixel x + k of that row is selected
    for (int p = 0; p < 2; ++p) {
        const int y = ty0 + ry + 8 * p;
        if (y >= H || npx <= 0) continue;
        const size_t o = ((size_t)img * H + y) * W + x;
        unsigned lab = 0u, own = 0u;
        if (npx == 4 && ((size_t)(a.labels + o) & 3) == 0) {
            lab = *reinterpret_cast<const unsigned*>(a.labels + o);
            if (a.select && lab) own = *reinterpret_cast<const unsigned*>(a.owners + o);      // maps of one allocation size: aligned alike
        } else {
            for (int k = 0; k < npx; ++k) {
                lab |= (unsigned)a.labels[o + k] << (8 * k);
                if (a.select) own |= (unsigned)a.owners[o + k] << (8 * k);
            }
        }
        for (int k = 0; k < npx; ++k) {
            const unsigned L = (lab >> (8 * k)) & 255u, ow = (own >> (8 * k)) & 255u;
            bool ok = ((a.label_mask >> L) & 1) != 0;
            if (ok && L && a.select) ok = a.select[slot0 + (int)ow - 1] != 0;
            if (ok) sel[p] |= 1u << k;
        }
    }
    if (a.label_mask & PF_REDACT_BOX) {
        for (int c0 = slot0; c0 < slot1; c0 += 256) {            // 256 slots at a time: the padded boxes that meet the tile, compacted
            const int slot = c0 + t;
            int hit = 0;
            if (slot < slot1) {
                const int* rec = a.rec + (size_t)slot * PF_MASK_REC;
                if (rec[0] && (!a.select || a.select[slot] != 0) && rec[3] > rec[1] && rec[4] > rec[2]) {
                    const int bx0 = rec[1] - a.pad, by0 = rec[2] - a.pad, bx1 = rec[3] + a.pad, by1 = rec[4] + a.pad;
                    if (bx0 < tx0 + PF_MASK_TW && bx1 > tx0 && by0 < ty0 + PF_MASK_TH && by1 > ty0) {
                        hit = 1;
                        s_box[t][0] = bx0; s_box[t][1] = by0; s_box[t][2] = bx1; s_box[t][3] = by1;
                    }
                }
            }
            s_hit[t] = (unsigned char)hit;
            __syncthreads();
            if (t == 0) {
                int n = 0;
                for (int i = 0; i < 256; ++i) {
                    if (!s_hit[i]) continue;
                    for (int k = 0; k < 4; ++k) s_box[n][k] = s_box[i][k];      // n <= i: only entries already read are overwritten
                    ++n;
                }
                s_nbox = n;
            }
            __syncthreads();
            const int nbox = s_nbox;
            for (int p = 0; p < 2; ++p) {
                const int y = ty0 + ry + 8 * p;
                if (y >= H) continue;
                for (int i = 0; i < nbox; ++i) {
                    if (y < s_box[i][1] || y >= s_box[i][3]) continue;
                    for (int k = 0; k < npx; ++k)
                        if (x + k >= s_box[i][0] && x + k < s_box[i][2]) sel[p] |= 1u << k;
                }
            }
            __syncthreads();                                     // the list has been read
        }
    }
    if (sel[0] | sel[1]) s_any = 1;
    __syncthreads();
    const AlignFrame f = a.frames[img];
    unsigned char* const out = a.out + (size_t)img * H * W * 3;
    if (!s_any && !a.stage_all) {                                // 16 threads per row segment of at most 384 bytes
        const int r = t >> 4, y = ty0 + r;
        if (y < H)
            pf_redact_copy(out + ((size_t)y * W + tx0) * 3, f.base + (size_t)y * f.row_stride + (size_t)tx0 * 3, min(PF_MASK_TW, W - tx0) * 3,
                           t & 15, 16);
        return;
    }
    // ---- 1. the footprint ----
    const int R = a.mode == PF_REDACT_BLUR ? a.strength : 0;     // <= RMAX
    const int fx0 = max(tx0 - R, 0), fx1 = min(tx0 + PF_MASK_TW + R, W), fy0 = max(ty0 - R, 0), fy1 = min(ty0 + PF_MASK_TH + R, H);
    const int fh = fy1 - fy0;
    const bool rows_aligned = (f.row_stride & 3) == 0;
    const int shift = rows_aligned ? (int)(((size_t)f.base + (size_t)fx0 * 3) & 3) : 0;
    const int words = (shift + (fx1 - fx0) * 3 + 3) / 4;         // <= WORDS
    const int row_bytes = W * 3;
    for (int i = t; i < fh * words; i += 256) {
        const int r = i / words, wd = i - r * words;
        const unsigned char* row = f.base + (size_t)(fy0 + r) * f.row_stride;
        const int bx = fx0 * 3 - shift + 4 * wd;                 // byte offset inside the frame row
        unsigned v = 0u;
        if (rows_aligned && bx >= 0 && bx + 4 <= row_bytes) {
            v = *reinterpret_cast<const unsigned*>(row + bx);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (bx + k >= 0 && bx + k < row_bytes) v |= (unsigned)row[bx + k] << (8 * k);
        }
        s_src[r * WORDS + wd] = v;
    }
    __syncthreads();
    // ---- 2. vertical sums ----
    if (a.mode != PF_REDACT_FILL && t < words) {
        unsigned acc0 = 0u, acc1 = 0u;
        int plo = 0, phi = -1;
        for (int j = 0; j < PF_MASK_TH && ty0 + j < H; ++j) {
            int lo, hi;
            pf_redact_range(a.mode, a.strength, ty0 + j, H, &lo, &hi);
            int add0 = phi + 1;
            if (lo > phi) { acc0 = acc1 = 0u; add0 = lo; }
            for (int yy = add0; yy <= hi; ++yy) {                // the additions first: no lane ever borrows
                const unsigned w = s_src[(yy - fy0) * WORDS + t];
                acc0 += w & 0x00FF00FFu; acc1 += (w >> 8) & 0x00FF00FFu;
            }
            if (lo <= phi)
                for (int yy = plo; yy < lo; ++yy) {
                    const unsigned w = s_src[(yy - fy0) * WORDS + t];
                    acc0 -= w & 0x00FF00FFu; acc1 -= (w >> 8) & 0x00FF00FFu;
                }
            s_v[j][t][0] = acc0; s_v[j][t][1] = acc1;
            plo = lo; phi = hi;
        }
    }
    __syncthreads();
    // ---- 3. horizontal sums and the output ----
    for (int p = 0; p < 2; ++p) {
        const int j = ry + 8 * p, y = ty0 + j;
        if (y >= H || npx <= 0) continue;
        const unsigned char* srow = reinterpret_cast<const unsigned char*>(s_src) + (size_t)(y - fy0) * WORDS * 4 + shift + (x - fx0) * 3;
        unsigned char o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = k < npx * 3 ? srow[k] : (unsigned char)0;
        if (sel[p] && a.mode == PF_REDACT_FILL) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((sel[p] >> k) & 1u) { o[3 * k] = (unsigned char)a.colour; o[3 * k + 1] = (unsigned char)(a.colour >> 8); o[3 * k + 2] = (unsigned char)(a.colour >> 16); }
        } else if (sel[p]) {
            int ylo, yhi;
            pf_redact_range(a.mode, a.strength, y, H, &ylo, &yhi);
            const unsigned ny = (unsigned)(yhi - ylo + 1);
            const unsigned short* vrow = reinterpret_cast<const unsigned short*>(&s_v[j][0][0]);
            unsigned s[3] = {0u, 0u, 0u};
            int plo = 0, phi = -1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= npx) break;
                int lo, hi;
                pf_redact_range(a.mode, a.strength, x + k, W, &lo, &hi);
                int add0 = phi + 1;
                if (lo > phi) { s[0] = s[1] = s[2] = 0u; add0 = lo; }
                for (int xx = add0; xx <= hi; ++xx) {
                    const int b = shift + (xx - fx0) * 3;        // byte b + c of the footprint row: word (b + c) / 4, lane order 0, 2, 1, 3
#pragma unroll
                    for (int c = 0; c < 3; ++c) s[c] += vrow[((b + c) & ~3) + (((b + c) & 1) << 1) + (((b + c) >> 1) & 1)];
                }
                if (lo <= phi)
                    for (int xx = plo; xx < lo; ++xx) {
                        const int b = shift + (xx - fx0) * 3;
#pragma unroll
                        for (int c = 0; c < 3; ++c) s[c] -= vrow[((b + c) & ~3) + (((b + c) & 1) << 1) + (((b + c) >> 1) & 1)];
                    }
                plo = lo; phi = hi;
                if ((sel[p] >> k) & 1u) {
                    const unsigned n = (unsigned)(hi - lo + 1) * ny;
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[3 * k + c] = (unsigned char)pf_redact_div(s[c] + (n >> 1), n, a.n_in, a.recip);
                }
            }
        }
        unsigned char* d = out + ((size_t)y * W + x) * 3;
        if (npx == 4 && ((size_t)d & 3) == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w)
                reinterpret_cast<unsigned*>(d)[w] = (unsigned)o[4 * w] | ((unsigned)o[4 * w + 1] << 8) | ((unsigned)o[4 * w + 2] << 16) | ((unsigned)o[4 * w + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < npx * 3) d[k] = o[k];
        }
    }
}

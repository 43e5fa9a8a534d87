// Aligned face chips from the 98 WFLW landmarks (pf_align_faces / pf_face_chips, align.inl): the similarity warp of a face onto the
// public ArcFace five-point template, the normalised image recognition / liveness networks take.
//
//   align_fit_kernel    five points of a face (eye-contour means, nose tip, mouth corners) -> least-squares similarity without
//                       reflection, closed form, float64; its inverse; a valid flag
//   align_warp_kernel   one 16 x 16 chip tile per workgroup: source footprint through LDS, Q10 bilinear taps in integers
//
// The arithmetic is the specification and is restated in numpy by tests/align_ref.py.  Every float64 operation
// is individually rounded -- `#pragma clang fp contract(off)` in each function that computes one -- so that the Q10 coordinates,
// and with them every chip byte, are reproducible on any IEEE-754 machine.
#pragma once
#include <vector>

#include "pf_common.h"

#define PF_ALIGN_TILE 16
#define PF_ALIGN_LDS_BYTES 16384      // source footprint of a tile that still goes through LDS
#define PF_ALIGN_REC 4                // doubles per slot the warp reads: the inverse map ia, ib, itx, ity

// where a slot's pixels come from: one table entry per slot, so batches, the resident frame and the stream slots share one kernel
struct AlignFrame {
    const unsigned char* base;    // packed BGR rows, row_stride bytes apart
    int H, W, row_stride, pad_;
};

// Host side of a handle: scratch of the two kernels (what the handle's last call left for pf_face_chips is FaceRows, face_rows.h)
struct AlignState {
    AlignFrame* d_table = nullptr; size_t table_bytes = 0;
    std::vector<AlignFrame> h_table;
    double* d_rec = nullptr; size_t rec_bytes = 0;
    int* d_valid = nullptr; size_t valid_bytes = 0;
    unsigned char* d_chips = nullptr; size_t chips_bytes = 0;        // host outputs are produced here first
    double* d_mats = nullptr; size_t mats_bytes = 0;
    std::vector<int> h_valid;
    int lds_budget = PF_ALIGN_LDS_BYTES;
    void release() {
        void* ptrs[] = {d_table, d_rec, d_valid, d_chips, d_mats};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = AlignState();
    }
};

struct AlignFitArgs {
    const void* kps;          // [n][98][2] float32 or float64
    int kps_f64;
    int n, per_frame, S;
    const int* counts;        // optional [n / per_frame]: slot k of a frame is live iff k < counts[frame]
    const int* valid_in;      // optional per-slot flags, valid_stride ints apart (the crop parameters of pf_landmarks)
    int valid_stride;
    double* rec;              // [n][PF_ALIGN_REC]
    int* valid;               // [n]
    double* mats_out;         // optional [n][2][3]: rows of valid slots only
    int* valid_out;           // optional [n]: every slot
};

__device__ __forceinline__ double pf_align_kp(const void* kps, int kps_f64, int slot, int point, int xy) {
    const size_t i = ((size_t)slot * 98 + point) * 2 + xy;
    return kps_f64 ? reinterpret_cast<const double*>(kps)[i] : (double)reinterpret_cast<const float*>(kps)[i];
}

__device__ __forceinline__ bool pf_align_finite(double v) { return v - v == 0.0; }      // false for NaN and +-inf

// m <- M row-major, inv <- ia, ib, itx, ity; returns the valid flag.  p: the five points (x, y).
__device__ inline int pf_align_fit(const double (*p)[2], int S, double* m, double* inv) {
#pragma clang fp contract(off)
    const double q112[5][2] = {{38.2946, 51.6963}, {73.5318, 51.5014}, {56.0252, 71.7366}, {41.5493, 92.3655}, {70.7299, 92.2041}};
    const double k = (double)S / 112.0;
    double q[5][2];
    for (int i = 0; i < 5; ++i) { q[i][0] = q112[i][0] * k; q[i][1] = q112[i][1] * k; }
    double mpx = 0.0, mpy = 0.0, mqx = 0.0, mqy = 0.0;
    for (int i = 0; i < 5; ++i) { mpx += p[i][0]; mpy += p[i][1]; mqx += q[i][0]; mqy += q[i][1]; }
    mpx /= 5.0; mpy /= 5.0; mqx /= 5.0; mqy /= 5.0;
    double den = 0.0, na = 0.0, nb = 0.0;
    for (int i = 0; i < 5; ++i) {
        const double dpx = p[i][0] - mpx, dpy = p[i][1] - mpy, dqx = q[i][0] - mqx, dqy = q[i][1] - mqy;
        den += dpx * dpx + dpy * dpy;
        na += dpx * dqx + dpy * dqy;
        nb += dpx * dqy - dpy * dqx;
    }
    if (!(den > 0.0)) return 0;
    const double a = na / den, b = nb / den;
    const double tx = mqx - (a * mpx - b * mpy), ty = mqy - (b * mpx + a * mpy);
    const double det = a * a + b * b;
    if (!(pf_align_finite(a) && pf_align_finite(b) && pf_align_finite(tx) && pf_align_finite(ty))) return 0;
    if (!(det >= 0.000244140625 && det <= 4096.0)) return 0;       // scale in [1/64, 64]: every later integer stays in 32 bits
    const double ia = a / det, ib = b / det;
    m[0] = a; m[1] = -b; m[2] = tx; m[3] = b; m[4] = a; m[5] = ty;
    inv[0] = ia; inv[1] = ib;
    inv[2] = -(ia * tx + ib * ty);
    inv[3] = -(ia * ty - ib * tx);
    return 1;
}

// the five points of slot `slot` (also read by mask_edges_kernel, k_mask.h: chip-space masks use the chips' matrix)
__device__ inline void pf_align_points(const void* kps, int kps_f64, int slot, double (*p)[2]) {
#pragma clang fp contract(off)
    for (int xy = 0; xy < 2; ++xy) {
        double e0 = 0.0, e1 = 0.0;
        for (int k = 0; k < 8; ++k) { e0 += pf_align_kp(kps, kps_f64, slot, 60 + k, xy); e1 += pf_align_kp(kps, kps_f64, slot, 68 + k, xy); }
        p[0][xy] = e0 / 8.0;                                    // eye contours, not the pupils 96 / 97: those follow the gaze
        p[1][xy] = e1 / 8.0;
        p[2][xy] = pf_align_kp(kps, kps_f64, slot, 54, xy);     // nose tip
        p[3][xy] = pf_align_kp(kps, kps_f64, slot, 76, xy);     // mouth corners
        p[4][xy] = pf_align_kp(kps, kps_f64, slot, 82, xy);
    }
}

__global__ __launch_bounds__(64) void align_fit_kernel(AlignFitArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    int ok = 1;
    if (a.counts && (i % a.per_frame) >= a.counts[i / a.per_frame]) ok = 0;
    if (ok && a.valid_in && a.valid_in[(size_t)i * a.valid_stride] == 0) ok = 0;
    double m[6], inv[PF_ALIGN_REC];
    if (ok) {
        double p[5][2];
        pf_align_points(a.kps, a.kps_f64, i, p);
        ok = pf_align_fit(p, a.S, m, inv);
    }
    a.valid[i] = ok;
    if (a.valid_out) a.valid_out[i] = ok;
    if (!ok) return;
    for (int k = 0; k < PF_ALIGN_REC; ++k) a.rec[(size_t)i * PF_ALIGN_REC + k] = inv[k];
    if (a.mats_out)
        for (int k = 0; k < 6; ++k) a.mats_out[(size_t)i * 6 + k] = m[k];
}

// --------------------------------------------------------------------------------------------
struct AlignWarpArgs {
    const AlignFrame* frames;     // [n]
    const double* rec;            // [n][PF_ALIGN_REC]
    const int* valid;             // [n]
    unsigned char* chips;         // [n][S][S][3]
    int n, S;
    int lds_budget;               // PF_ALIGN_LDS_BYTES (the measurement tool's build can force the direct path with 0)
    int out_aligned;              // chips is 4-byte aligned: tiles leave as 32-bit words
};

// Q10 source coordinate of chip pixel (x, y): U = round(1024 u), V = round(1024 v), u / v clamped two pixels outside the frame (every
// tap there is border, so the clamp changes no result and keeps the integers small)
__device__ __forceinline__ void pf_align_coord(const double* rec, int x, int y, int H, int W, int* U, int* V) {
#pragma clang fp contract(off)
    const double ia = rec[0], ib = rec[1], itx = rec[2], ity = rec[3];
    const double dx = (double)x, dy = (double)y;
    double u = (ia * dx + ib * dy) + itx;
    double v = (ia * dy - ib * dx) + ity;
    const double umax = (double)(W + 1), vmax = (double)(H + 1);
    u = u < -2.0 ? -2.0 : (u > umax ? umax : u);
    v = v < -2.0 ? -2.0 : (v > vmax ? vmax : v);
    *U = (int)floor(u * 1024.0 + 0.5);
    *V = (int)floor(v * 1024.0 + 0.5);
}

__device__ __forceinline__ unsigned pf_align_blend(unsigned p00, unsigned p10, unsigned p01, unsigned p11, unsigned fx, unsigned fy) {
    return (p00 * (1024u - fx) * (1024u - fy) + p10 * fx * (1024u - fy) + p01 * (1024u - fx) * fy + p11 * fx * fy + (1u << 19)) >> 20;
}

__device__ __forceinline__ unsigned pf_align_px(const AlignFrame& f, int y, int x, int c) {      // constant border 0
    if ((unsigned)y >= (unsigned)f.H || (unsigned)x >= (unsigned)f.W) return 0u;
    return f.base[(size_t)y * f.row_stride + (size_t)x * 3 + c];
}

// One workgroup = one 16 x 16 tile of one chip (square, because the footprint is rotated: its source bounding box stays near
// (16 (|cos| + |sin|) / s + 2)^2 pixels at any roll).  The box is fetched ONCE as aligned 32-bit words, the zero border materialised,
// into LDS and the taps read it there; a box beyond the LDS budget (a very large face) makes this workgroup's pixels read the frame
// directly, byte by byte.  Both paths evaluate the same U, V and the same integer blend.  The finished 16 x 48-byte tile is assembled
// in LDS and leaves as aligned 32-bit words.
__global__ __launch_bounds__(256) void align_warp_kernel(AlignWarpArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned s_src[PF_ALIGN_LDS_BYTES / 4];
    __shared__ __attribute__((aligned(16))) unsigned char s_out[PF_ALIGN_TILE * PF_ALIGN_TILE * 3];
    __shared__ int s_corner[4][2];
    const int t = threadIdx.x;
    const int slot = blockIdx.y;
    if (!a.valid[slot]) return;                        // dead or degenerate slot: its chip is left untouched
    const int S = a.S, tiles = S / PF_ALIGN_TILE;
    const int tile_y = blockIdx.x / tiles, tile_x = blockIdx.x - tile_y * tiles;
    const int lx = t & 15, ly = t >> 4;
    const AlignFrame f = a.frames[slot];
    const double* rec = a.rec + (size_t)slot * PF_ALIGN_REC;
    int U, V;
    pf_align_coord(rec, tile_x * PF_ALIGN_TILE + lx, tile_y * PF_ALIGN_TILE + ly, f.H, f.W, &U, &V);
    // the map is monotone in x and in y (each rounded operation is), so the tile's extreme coordinates are those of its corners
    if ((lx == 0 || lx == 15) && (ly == 0 || ly == 15)) {
        const int c = (lx ? 1 : 0) + (ly ? 2 : 0);
        s_corner[c][0] = U >> 10; s_corner[c][1] = V >> 10;
    }
    __syncthreads();
    const int bx0 = min(min(s_corner[0][0], s_corner[1][0]), min(s_corner[2][0], s_corner[3][0]));
    const int bx1 = max(max(s_corner[0][0], s_corner[1][0]), max(s_corner[2][0], s_corner[3][0])) + 1;
    const int by0 = min(min(s_corner[0][1], s_corner[1][1]), min(s_corner[2][1], s_corner[3][1]));
    const int by1 = max(max(s_corner[0][1], s_corner[1][1]), max(s_corner[2][1], s_corner[3][1])) + 1;
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    // box byte b of a row lives at LDS byte shift + b of that row: the row's first word starts 4-byte aligned in global memory
    const bool rows_aligned = (f.row_stride & 3) == 0;
    const long long fx0 = (long long)bx0 * 3;          // first box byte inside a frame row (may be negative)
    const int shift = rows_aligned ? (int)((((long long)(size_t)f.base + fx0) % 4 + 4) % 4) : 0;
    const int words = ((shift + bw * 3 + 3) / 4) | 1;  // odd row pitch: rows of the box start on different banks
    const int x0 = U >> 10, y0 = V >> 10;
    const unsigned fx = (unsigned)(U & 1023), fy = (unsigned)(V & 1023);
    unsigned char* o = s_out + (size_t)t * 3;
    if ((long long)bh * words * 4 > (long long)a.lds_budget) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[c] = (unsigned char)pf_align_blend(pf_align_px(f, y0, x0, c), pf_align_px(f, y0, x0 + 1, c), pf_align_px(f, y0 + 1, x0, c),
                                                 pf_align_px(f, y0 + 1, x0 + 1, c), fx, fy);
    } else {
        const long long row_bytes = (long long)f.W * 3;
        for (int i = t; i < bh * words; i += 256) {
            const int r = i / words, wd = i - r * words;
            const int gy = by0 + r;
            const long long bx = fx0 - shift + 4LL * wd;       // byte offset inside the frame row
            unsigned v = 0u;
            if ((unsigned)gy < (unsigned)f.H) {
                const unsigned char* row = f.base + (size_t)gy * f.row_stride;
                if (rows_aligned && bx >= 0 && bx + 4 <= row_bytes) {
                    v = *reinterpret_cast<const unsigned*>(row + bx);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const long long b = bx + k;
                        if (b >= 0 && b < row_bytes) v |= (unsigned)row[b] << (8 * k);
                    }
                }
            }
            s_src[i] = v;
        }
        __syncthreads();
        const unsigned char* q0 = reinterpret_cast<const unsigned char*>(s_src) + (size_t)(y0 - by0) * words * 4 + shift + (x0 - bx0) * 3;
        const unsigned char* q1 = q0 + (size_t)words * 4;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)pf_align_blend(q0[c], q0[3 + c], q1[c], q1[3 + c], fx, fy);
    }
    __syncthreads();
    unsigned char* out = a.chips + (((size_t)slot * S + (size_t)tile_y * PF_ALIGN_TILE) * S + (size_t)tile_x * PF_ALIGN_TILE) * 3;
    if (a.out_aligned) {          // S * 3 and the tile's 48-byte rows are multiples of 4
        if (t < PF_ALIGN_TILE * 12) {
            const int r = t / 12, w = t - r * 12;
            reinterpret_cast<unsigned*>(out + (size_t)r * S * 3)[w] = reinterpret_cast<const unsigned*>(s_out)[t];
        }
    } else {
        for (int i = t; i < PF_ALIGN_TILE * 48; i += 256) {
            const int r = i / 48;
            out[(size_t)r * S * 3 + (i - r * 48)] = s_out[i];
        }
    }
}

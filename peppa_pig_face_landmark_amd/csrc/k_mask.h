// Face-region label maps from the 98 WFLW landmarks (pf_mask_faces / pf_face_masks, mask.inl): which pixels are face, and which part
// of the face, scan-converted on the device from the landmarks alone -- no frame is read.
//
//   mask_edges_kernel   per slot: validity, the 96 used vertices in Q4 (through the chips' matrix in chip space), the clipped box
//   mask_fill_kernel    output-stationary even-odd polygon fill: one workgroup owns one 128 x 16 tile of one output image and writes
//                       every byte of it once, background and all faces in one pass
//
// The arithmetic is the specification and is restated in numpy by tests/mask_ref.py: everything after the Q4
// conversion is integer, so every byte is reproducible.
//
// Tile: 128 wide x 16 high, 256 threads, a thread owns four consecutive pixels of rows r and r + 8.  A wave therefore stores two
// 512-byte row segments as 32-bit words (one byte per pixel: a narrower tile would leave stores of under 256 bytes per row), and a
// slot costs 16 x 103 = 1648 (row, edge) threshold evaluations, 6.4 per thread, each with one emulated 64-bit division; a taller tile
// would raise that in proportion while most of its rows lie outside the face.  LDS: 1648 B of edges + 1664 B of thresholds + 256 B
// of list lengths and parities = 3568 B, so LDS never limits occupancy.
#pragma once
#include <vector>

#include "k_align.h"

#define PF_MASK_TW 128
#define PF_MASK_TH 16
#define PF_MASK_EDGES 103             // 43 + 9 + 9 + 8 + 8 + 6 + 12 + 8
#define PF_MASK_REGIONS 8
#define PF_MASK_VERTS 96              // landmarks 0..95; the pupils 96 / 97 are not used
#define PF_MASK_REC 200               // ints per slot: valid, box x0 y0 x1 y1, 3 unused, then X, Y of vertices 0..95 in Q4
#define PF_MASK_FLIP 255              // threshold code of an edge that crosses the row right of the tile: the whole row flips

// Host side of a handle: scratch of the two kernels; host outputs are produced here first
struct MaskState {
    int* d_rec = nullptr; size_t rec_bytes = 0;
    unsigned char* d_labels = nullptr; size_t labels_bytes = 0;
    unsigned char* d_owners = nullptr; size_t owners_bytes = 0;
    int* d_boxes = nullptr; size_t boxes_bytes = 0;
    int* d_valid = nullptr; size_t valid_bytes = 0;
    std::vector<int> h_valid;
    int no_cull = 0;                  // measurement tool's build only: every slot of the image in every tile, no parity folding
    void release() {
        void* ptrs[] = {d_rec, d_labels, d_owners, d_boxes, d_valid};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = MaskState();
    }
};

// Regions 0..7 carry labels 1..8: face, left brow, right brow, left eye, right eye, nose, lips, inner mouth.  Region g owns edges
// [pf_mask_edge0(g), pf_mask_edge0(g + 1)); edge j of a region joins its vertices j and j + 1 (the last one closes the polygon).
__device__ __forceinline__ int pf_mask_edge0(int g) {
    const int e0[PF_MASK_REGIONS + 1] = {0, 43, 52, 61, 69, 77, 83, 95, 103};
    return e0[g];
}

__device__ __forceinline__ int pf_mask_vertex(int g, int j) {
    if (g == 0) return j < 33 ? j : (j < 38 ? 79 - j : 75 - j);      // jaw 0..32, then 46..42, then 37..33: the upper brow lines backwards
    if (g == 5) return j == 0 ? 51 : 54 + j;                         // nose: 51, 55..59
    const int base[PF_MASK_REGIONS] = {0, 33, 42, 60, 68, 0, 76, 88};
    return base[g] + j;
}

// Q4 of a coordinate: clamped to [-65536, 65536] (a NaN, which only an overflow of the chip-space transform can produce, takes the
// lower bound), then floor(16 v + 0.5)
__device__ __forceinline__ int pf_mask_q4(double v) {
#pragma clang fp contract(off)
    v = !(v >= -65536.0) ? -65536.0 : (v > 65536.0 ? 65536.0 : v);
    return (int)floor(v * 16.0 + 0.5);
}

__device__ __forceinline__ int pf_mask_ceil16(int v) { return (v + 15) >> 4; }       // ceil(v / 16), also for negative v

// ceil(n / d) for d > 0 and |n| < 2^53: the 64-bit division is emulated on this hardware, so the quotient comes from one float64
// division (both operands exact; the rounded quotient, below 2^40, is within one of the integer quotient) and the exact int64
// remainder corrects it
__device__ __forceinline__ long long pf_mask_ceil_div(long long n, long long d) {
    long long q = (long long)((double)n / (double)d);
    long long r = n - q * d;
    if (r < 0) { q -= 1; r += d; }
    else if (r >= d) { q += 1; r -= d; }
    return q + (r > 0 ? 1 : 0);
}

// What mask_edges_kernel and draw_prims_kernel (k_draw.h) share, so that a slot is live and boxed alike for the maps and the overlay.
// A slot is live iff it lies below its frame's count and its flag of the last call, where either is given.
__device__ __forceinline__ int pf_mask_live(const int* counts, int per_frame, const int* valid_in, int valid_stride, int slot) {
    if (counts && (slot % per_frame) >= counts[slot / per_frame]) return 0;
    if (valid_in && valid_in[(size_t)slot * valid_stride] == 0) return 0;
    return 1;
}

// the clipped box of a slot from the Q4 extremes of its vertices 0..95: pixels x0 <= x < x1, y0 <= y < y1 inside [0, W] x [0, H]
__device__ __forceinline__ void pf_mask_box(int X0, int Y0, int X1, int Y1, int W, int H, int* box) {
    box[0] = min(max(pf_mask_ceil16(X0), 0), W); box[1] = min(max(pf_mask_ceil16(Y0), 0), H);
    box[2] = min(max(pf_mask_ceil16(X1), 0), W); box[3] = min(max(pf_mask_ceil16(Y1), 0), H);
}

struct MaskEdgesArgs {
    const void* kps;          // [n][98][2] float32 or float64
    int kps_f64;
    int n, per_frame;
    int S;                    // 0: frame space; else chip space, the vertices go through the chips' matrix for chip size S
    int H, W;                 // the box is clipped to [0, W] x [0, H] (S x S in chip space)
    const int* counts;        // optional [n / per_frame]: slot k of a frame is live iff k < counts[frame]
    const int* valid_in;      // optional per-slot flags, valid_stride ints apart (the crop parameters of pf_landmarks)
    int valid_stride;
    int* rec;                 // [n][PF_MASK_REC]
    int* boxes_out;           // optional [n][4]: rows of valid slots only
    int* valid_out;           // optional [n]: every slot
};

// One wave per slot: lane t converts vertices t and t + 64.
__global__ __launch_bounds__(64) void mask_edges_kernel(MaskEdgesArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_xy[PF_MASK_VERTS][2];
    __shared__ int s_fin[64];
    __shared__ double s_m[6];
    __shared__ int s_ok;
    const int t = threadIdx.x, slot = blockIdx.x;
    int* rec = a.rec + (size_t)slot * PF_MASK_REC;
    const int live = pf_mask_live(a.counts, a.per_frame, a.valid_in, a.valid_stride, slot);      // the same in every lane
    double x[2] = {0.0, 0.0}, y[2] = {0.0, 0.0};
    int fin = 1;
    if (live) {
        for (int k = 0; k < 2; ++k) {
            const int v = t + 64 * k;
            if (v >= PF_MASK_VERTS) break;
            x[k] = pf_align_kp(a.kps, a.kps_f64, slot, v, 0);
            y[k] = pf_align_kp(a.kps, a.kps_f64, slot, v, 1);
            if (!(pf_align_finite(x[k]) && pf_align_finite(y[k]))) fin = 0;
        }
    }
    s_fin[t] = fin;
    __syncthreads();
    if (t == 0) {
        int ok = live;
        for (int i = 0; i < 64; ++i) ok &= s_fin[i];
        if (ok && a.S) {                                         // the same function as align_fit_kernel: the chips' bits
            double p[5][2], m[6], inv[PF_ALIGN_REC];
            pf_align_points(a.kps, a.kps_f64, slot, p);
            ok = pf_align_fit(p, a.S, m, inv);
            if (ok) for (int i = 0; i < 6; ++i) s_m[i] = m[i];
        }
        s_ok = ok;
        if (!ok) {                                               // boxes_out keeps its row
            rec[0] = 0;
            if (a.valid_out) a.valid_out[slot] = 0;
        }
    }
    __syncthreads();
    if (!s_ok) return;
    for (int k = 0; k < 2; ++k) {
        const int v = t + 64 * k;
        if (v >= PF_MASK_VERTS) break;
        double vx = x[k], vy = y[k];
        if (a.S) {
            const double ca = s_m[0], cb = s_m[3], tx = s_m[2], ty = s_m[5];
            vx = (ca * x[k] - cb * y[k]) + tx;
            vy = (cb * x[k] + ca * y[k]) + ty;
        }
        const int X = pf_mask_q4(vx), Y = pf_mask_q4(vy);
        s_xy[v][0] = X; s_xy[v][1] = Y;
        rec[8 + 2 * v] = X; rec[9 + 2 * v] = Y;
    }
    __syncthreads();
    if (t == 0) {
        int x0 = s_xy[0][0], x1 = x0, y0 = s_xy[0][1], y1 = y0;
        for (int v = 1; v < PF_MASK_VERTS; ++v) {
            x0 = min(x0, s_xy[v][0]); x1 = max(x1, s_xy[v][0]);
            y0 = min(y0, s_xy[v][1]); y1 = max(y1, s_xy[v][1]);
        }
        int box[4];
        pf_mask_box(x0, y0, x1, y1, a.W, a.H, box);
        rec[0] = 1;
        for (int i = 0; i < 4; ++i) {
            rec[1 + i] = box[i];
            if (a.boxes_out) a.boxes_out[(size_t)slot * 4 + i] = box[i];
        }
        if (a.valid_out) a.valid_out[slot] = 1;
    }
}

// --------------------------------------------------------------------------------------------
struct MaskFillArgs {
    const int* rec;               // [n][PF_MASK_REC]
    unsigned char* labels;        // [images][H][W]
    unsigned char* owners;        // optional, like labels: slot within the image + 1
    int n;                        // slots
    int per;                      // slots per image: per_frame in frame space, 1 in chip space
    int H, W;                     // image size (S x S in chip space)
    int tiles_x, tiles;           // tiles per image row, per image
    int chip;                     // chip space: the map of an invalid slot is left untouched
    int no_cull;                  // MaskState::no_cull
};

// bytes of x that are not zero -> 0xFF (bytes of x at most 0x80)
__device__ __forceinline__ unsigned pf_mask_nonzero_bytes(unsigned x) { return (((x + 0x7F7F7F7Fu) & 0x80808080u) >> 7) * 0xFFu; }

// four pixels: one 32-bit store where the address is 4-byte aligned and all four lie in the row, byte stores otherwise
__device__ __forceinline__ void pf_mask_store4(unsigned char* p, unsigned v, int room) {
    if (room >= 4 && ((size_t)p & 3) == 0) { *reinterpret_cast<unsigned*>(p) = v; return; }
    for (int k = 0; k < 4 && k < room; ++k) p[k] = (unsigned char)(v >> (8 * k));
}

// The workgroup walks its image's slots in slot order and skips those whose box misses the tile.  For a slot that touches it:
//   1. the 103 edges, endpoints ordered by Y, go to LDS;
//   2. every (tile row, edge) pair gets its threshold T relative to the tile's left column -- 0 where the edge is not active on the
//      row or T lies left of the tile (it contributes nothing), PF_MASK_FLIP where T lies right of it (every pixel of the row is
//      left of the crossing);
//   3. one thread per (row, region) compacts the region's thresholds in place into a list and folds the flips into a parity bit; the
//      list's room is the region's edge count, so nothing can overflow;
//   4. a thread's pixels count the list entries right of them, highest region first.  No pixel evaluates an edge equation.
// A pixel keeps the label of the first slot that gives it one, so the overlap rule and the background need no second pass, no clear
// and no atomics.  Every branch around a barrier depends on the record alone and is uniform.
__global__ __launch_bounds__(256) void mask_fill_kernel(MaskFillArgs a) {
    __shared__ int s_edge[PF_MASK_EDGES][4];                     // Xa, Ya, Xb, Yb with Ya <= Yb
    __shared__ unsigned char s_T[PF_MASK_TH][PF_MASK_EDGES + 1];
    __shared__ unsigned char s_cnt[PF_MASK_TH][PF_MASK_REGIONS];
    __shared__ unsigned char s_par[PF_MASK_TH][PF_MASK_REGIONS];
    const int t = threadIdx.x;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
    const int tx0 = tile_x * PF_MASK_TW, ty0 = tile_y * PF_MASK_TH;
    const int slot0 = img * a.per, slot1 = min(slot0 + a.per, a.n);
    if (a.chip && !a.rec[(size_t)slot0 * PF_MASK_REC]) return;
    const int qx = (t & 31) * 4, ry = t >> 5;                    // this thread's pixels: columns qx .. qx + 3 of rows ry and ry + 8
    unsigned lab[2] = {0u, 0u}, own[2] = {0u, 0u};               // four bytes each, pixel qx in the low byte
    for (int slot = slot0; slot < slot1; ++slot) {
        const int* rec = a.rec + (size_t)slot * PF_MASK_REC;
        if (!rec[0]) continue;
        const int bx0 = rec[1], by0 = rec[2], bx1 = rec[3], by1 = rec[4];
        if (!a.no_cull && (bx0 >= bx1 || by0 >= by1 || bx0 >= tx0 + PF_MASK_TW || bx1 <= tx0 || by0 >= ty0 + PF_MASK_TH || by1 <= ty0)) continue;
        __syncthreads();                                         // the previous slot's lists have been read
        if (t < PF_MASK_EDGES) {
            int g = 0;
            while (t >= pf_mask_edge0(g + 1)) ++g;
            const int j = t - pf_mask_edge0(g), nv = pf_mask_edge0(g + 1) - pf_mask_edge0(g);
            const int va = pf_mask_vertex(g, j), vb = pf_mask_vertex(g, j + 1 == nv ? 0 : j + 1);
            const int Xa = rec[8 + 2 * va], Ya = rec[9 + 2 * va], Xb = rec[8 + 2 * vb], Yb = rec[9 + 2 * vb];
            const bool up = Ya <= Yb;
            s_edge[t][0] = up ? Xa : Xb; s_edge[t][1] = up ? Ya : Yb;
            s_edge[t][2] = up ? Xb : Xa; s_edge[t][3] = up ? Yb : Ya;
        }
        __syncthreads();
        // the row is the fast thread index: the 16 lanes of an edge read one s_edge entry (broadcast) and write bytes 104 apart, i.e.
        // dwords 26 r, which fall on 16 different banks; the two edges of a 32-lane group share dwords, not more
        for (int i = t; i < PF_MASK_TH * PF_MASK_EDGES; i += 256) {
            const int e = i / PF_MASK_TH, r = i - e * PF_MASK_TH;
            const int Y = 16 * (ty0 + r);
            const int Xa = s_edge[e][0], Ya = s_edge[e][1], Xb = s_edge[e][2], Yb = s_edge[e][3];
            int code = 0;
            if (Ya <= Y && Y < Yb) {                             // half-open; a horizontal edge is never active
                const long long dy = Yb - Ya;
                const long long T = pf_mask_ceil_div((long long)Xa * dy + (long long)(Xb - Xa) * (Y - Ya), 16 * dy);
                const long long rel = T - tx0;
                if (rel >= PF_MASK_TW) code = a.no_cull ? PF_MASK_TW : PF_MASK_FLIP;
                else if (rel > 0) code = (int)rel;
            }
            s_T[r][e] = (unsigned char)code;
        }
        __syncthreads();
        if (t < PF_MASK_TH * PF_MASK_REGIONS) {
            const int r = t / PF_MASK_REGIONS, g = t - r * PF_MASK_REGIONS;
            const int e0 = pf_mask_edge0(g), e1 = pf_mask_edge0(g + 1);
            int n = 0, par = 0;
            for (int e = e0; e < e1; ++e) {
                const int c = s_T[r][e];
                if (c == PF_MASK_FLIP) par ^= 1;
                else if (c) s_T[r][e0 + n++] = (unsigned char)c;      // n <= e - e0: only entries already read are overwritten
            }
            s_cnt[r][g] = (unsigned char)n; s_par[r][g] = (unsigned char)par;
        }
        __syncthreads();
        for (int p = 0; p < 2; ++p) {
            const int r = ry + 8 * p;
            unsigned face = 0u;                                  // this slot's labels of the four pixels
            for (int g = PF_MASK_REGIONS - 1; g >= 0; --g) {
                unsigned in = s_par[r][g] ? 0xFFFFFFFFu : 0u;
                const unsigned char* list = &s_T[r][pf_mask_edge0(g)];
                const int n = s_cnt[r][g];
                for (int i = 0; i < n; ++i) {
                    const int T = list[i];
                    in ^= (qx < T ? 0xFFu : 0u) | (qx + 1 < T ? 0xFF00u : 0u) | (qx + 2 < T ? 0xFF0000u : 0u) | (qx + 3 < T ? 0xFF000000u : 0u);
                }
                face |= in & ~pf_mask_nonzero_bytes(face) & ((unsigned)(g + 1) * 0x01010101u);
            }
            const unsigned take = pf_mask_nonzero_bytes(face) & ~pf_mask_nonzero_bytes(lab[p]);
            lab[p] |= face & take;
            if (a.owners) own[p] |= take & ((unsigned)(slot - slot0 + 1) * 0x01010101u);
        }
    }
    for (int p = 0; p < 2; ++p) {
        const int y = ty0 + ry + 8 * p, x = tx0 + qx;
        if (y >= a.H || x >= a.W) continue;
        const size_t o = ((size_t)img * a.H + y) * a.W + x;
        pf_mask_store4(a.labels + o, lab[p], a.W - x);
        if (a.owners) pf_mask_store4(a.owners + o, own[p], a.W - x);
    }
}

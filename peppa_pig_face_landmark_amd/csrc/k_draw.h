// Face overlay (pf_draw_faces / pf_face_draw, draw.inl): the 98 landmarks as discs, the 103 contour edges of the label maps' regions
// as round-capped thick lines and the clipped box as an outline, blended once onto a copy of the frame.  Every output byte is
// written; an uncovered pixel is its input.
//
//   draw_prims_kernel   one wave per slot: validity and the clipped box (the functions of mask_edges_kernel, k_mask.h), then the slot's
//                       PF_DRAW_PRIMS = 205 primitives in priority order -- points 97 .. 0, the 103 edges, the four bars of the box
//                       outline -- each with its own pixel bounds, and the slot's draw rectangle, the union of those bounds
//   draw_kernel         output-stationary, the 128 x 16 tile of mask_fill_kernel and redact_kernel: a workgroup writes every byte of
//                       its tile once
//
// The arithmetic is the specification and is restated in numpy by tests/draw_ref.py: after the Q4 conversion
// everything is integer (the one square root is corrected to the exact integer root), so every byte is reproducible and independent
// of the tile order.
//
// A tile first asks all slots of its image at once -- thread t reads the rectangle of slot c0 + t, 256 slots a pass, no load depends
// on another -- and compacts those that meet it, in slot order (wave ballots, no serial scan).  A tile that none meets, the great
// majority, copies its 16 row segments with pf_redact_copy and touches no other LDS.  Any other tile walks the primitives of its
// slots 256 candidates a round: thread t reads the packed bounds of candidate k0 + t (8 bytes, consecutive over the threads) and,
// where they meet the tile, copies the 64-byte primitive into the LDS list at its compacted position, which keeps the priority
// order; then every thread walks the list for its eight pixels (four consecutive ones of rows r and r + 8) and stops at the first
// hit of each.  A tile whose rounds list nothing copies as well.
// HOW MANY PRIMITIVES A TILE MAY HOLD: any number.  The list holds 256 (a round's candidates, so it cannot overflow) and the rounds
// repeat until the slots' primitives are through; nothing is dropped, a pixel decided in an earlier round skips the later ones.
// LDS: 16 KB of list + 6.1 KB of staged pixels + 1 KB of slots = 23.2 KB, six workgroups of four waves per CU of 160 KB -- the
// occupancy of redact_kernel<0> (22.4 KB); a list of 512 would drop it to four for rounds that eight faces a frame never need.
// No atomics, no fences; every branch around a barrier depends on the arguments or on LDS all threads read alike and is uniform.
#pragma once
#include <vector>

#include "k_mask.h"
#include "k_redact.h"

// what bits: PF_DRAW_POINTS / _CONTOURS / _BOX of include/peppa_hip.h
#define PF_DRAW_NPOINTS 98
#define PF_DRAW_PRIMS (PF_DRAW_NPOINTS + PF_MASK_EDGES + 4)      // 205
#define PF_DRAW_HEAD 8                // ints per slot: valid, the draw rectangle x0 y0 x1 y1, 3 unused
#define PF_DRAW_DISC 0
#define PF_DRAW_EDGE 1
#define PF_DRAW_BAR 2

// One primitive.  Bounds are pixels, half-open and clipped to the frame; bx0 >= bx1 or by0 >= by1: not drawn.  A disc covers
// |P - A|^2 <= r2; an edge the discs about A and A + d and, with q = P - A, 0 <= q.d <= len2 and |q x d| <= bound; a bar its bounds.
struct __attribute__((aligned(16))) DrawPrim {
    int bx0, by0, bx1, by1;
    int ax, ay, dx, dy;               // Q4
    long long len2, bound;            // d.d and isqrt(64 w^2 len2)
    int r2;                           // (16 r)^2 of a point, (8 w)^2 of an edge's caps
    int kind;                         // PF_DRAW_DISC / _EDGE / _BAR | colour index << 4 (0 hi, 1 lo, 2 contour, 3 box)
    int pad_[2];
};
static_assert(sizeof(DrawPrim) == 64, "a primitive is four 16-byte vectors");

// Host side of a handle: scratch of the two kernels and the staging of host outputs
struct DrawState {
    int* d_head = nullptr; size_t head_bytes = 0;
    DrawPrim* d_prims = nullptr; size_t prims_bytes = 0;
    unsigned long long* d_bounds = nullptr; size_t bounds_bytes = 0;
    float* d_scores = nullptr; size_t scores_bytes = 0;
    int* d_valid = nullptr; size_t valid_bytes = 0;
    AlignFrame* d_table = nullptr; size_t table_bytes = 0;
    unsigned char* d_out = nullptr; size_t out_bytes = 0;
    std::vector<int> h_valid;
    std::vector<AlignFrame> h_table;
    int no_cull = 0;                  // measurement tool's build only: every tile stages, every primitive of the image is listed
    void release() {
        void* ptrs[] = {d_head, d_prims, d_bounds, d_scores, d_valid, d_table, d_out};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = DrawState();
    }
};

struct DrawPrimsArgs {
    const void* kps;          // [n][98][2] float32 or float64
    int kps_f64;
    int n, per_frame;
    int H, W;
    const int* counts;        // as MaskEdgesArgs
    const int* valid_in;
    int valid_stride;
    const float* scores;      // optional [n][98]
    float score_thres;
    int what, r, w;
    int* head;                // [n][PF_DRAW_HEAD]
    DrawPrim* prims;          // [n][PF_DRAW_PRIMS]
    unsigned long long* bounds;      // [n][PF_DRAW_PRIMS]: the primitives' bounds again, packed (pf_draw_pack)
    int* valid_out;           // optional [n]
};

// floor(sqrt(v)), exact, 0 <= v < 2^58: the float64 root is within one of it
__device__ __forceinline__ long long pf_draw_isqrt(long long v) {
    long long r = (long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// A primitive's bounds in 8 bytes, x0 | x1 << 16 | y0 << 32 | y1 << 48 (a frame is at most 32768 wide and high): what a tile reads of
// every candidate, 1.6 KB per slot next to the 13 KB of its primitives
__device__ __forceinline__ unsigned long long pf_draw_pack(int x0, int y0, int x1, int y1) {
    return (unsigned long long)x0 | ((unsigned long long)x1 << 16) | ((unsigned long long)y0 << 32) | ((unsigned long long)y1 << 48);
}

// the pixels whose centres 16 p lie in [lo, hi] (Q4), clipped to [0, size): first and one past the last
__device__ __forceinline__ void pf_draw_span(int lo, int hi, int size, int* p0, int* p1) {
    *p0 = min(max(pf_mask_ceil16(lo), 0), size);
    *p1 = min(max((hi >> 4) + 1, 0), size);
}

// One wave per slot: lane t converts landmarks t and t + 64, then builds primitives t, t + 64, ...
__global__ __launch_bounds__(64) void draw_prims_kernel(DrawPrimsArgs a) {
    __shared__ int s_xy[PF_DRAW_NPOINTS][2];
    __shared__ int s_drawn[PF_DRAW_NPOINTS];
    __shared__ int s_fin[64];
    __shared__ int s_rect[64][4];
    __shared__ int s_box[4];
    __shared__ int s_ok;
    const int t = threadIdx.x, slot = blockIdx.x;
    int* head = a.head + (size_t)slot * PF_DRAW_HEAD;
    const int live = pf_mask_live(a.counts, a.per_frame, a.valid_in, a.valid_stride, slot);      // the same in every lane
    int fin = 1;
    if (live) {
        for (int k = 0; k < 2; ++k) {
            const int v = t + 64 * k;
            if (v >= PF_DRAW_NPOINTS) break;
            const double x = pf_align_kp(a.kps, a.kps_f64, slot, v, 0), y = pf_align_kp(a.kps, a.kps_f64, slot, v, 1);
            const int f = pf_align_finite(x) && pf_align_finite(y);
            if (v < PF_MASK_VERTS && !f) fin = 0;                // a pupil that is not finite is not drawn, the slot is
            s_xy[v][0] = pf_mask_q4(x); s_xy[v][1] = pf_mask_q4(y);
            s_drawn[v] = f;
        }
    }
    s_fin[t] = fin;
    __syncthreads();
    if (t == 0) {
        int ok = live;
        for (int i = 0; i < 64; ++i) ok &= s_fin[i];
        s_ok = ok;
        if (ok) {
            int x0 = s_xy[0][0], x1 = x0, y0 = s_xy[0][1], y1 = y0;
            for (int v = 1; v < PF_MASK_VERTS; ++v) {
                x0 = min(x0, s_xy[v][0]); x1 = max(x1, s_xy[v][0]);
                y0 = min(y0, s_xy[v][1]); y1 = max(y1, s_xy[v][1]);
            }
            pf_mask_box(x0, y0, x1, y1, a.W, a.H, s_box);
        } else {
            for (int i = 0; i < PF_DRAW_HEAD; ++i) head[i] = 0;
        }
        if (a.valid_out) a.valid_out[slot] = ok;
    }
    __syncthreads();
    if (!s_ok) return;
    int rect[4] = {a.W, a.H, 0, 0};
    for (int p = t; p < PF_DRAW_PRIMS; p += 64) {
        DrawPrim q{};
        int on = 0;
        if (p < PF_DRAW_NPOINTS) {                               // the highest index first: it wins among points
            const int v = PF_DRAW_NPOINTS - 1 - p, R = 16 * a.r;
            on = (a.what & PF_DRAW_POINTS) && s_drawn[v];
            const bool hi = !a.scores || a.scores[(size_t)slot * PF_DRAW_NPOINTS + v] > a.score_thres;      // NaN: lo
            q.ax = s_xy[v][0]; q.ay = s_xy[v][1];
            q.r2 = R * R;
            q.kind = PF_DRAW_DISC | ((hi ? 0 : 1) << 4);
            pf_draw_span(q.ax - R, q.ax + R, a.W, &q.bx0, &q.bx1);
            pf_draw_span(q.ay - R, q.ay + R, a.H, &q.by0, &q.by1);
        } else if (p < PF_DRAW_NPOINTS + PF_MASK_EDGES) {
            const int e = p - PF_DRAW_NPOINTS, R = 8 * a.w;
            int g = 0;
            while (e >= pf_mask_edge0(g + 1)) ++g;
            const int j = e - pf_mask_edge0(g), nv = pf_mask_edge0(g + 1) - pf_mask_edge0(g);
            const int va = pf_mask_vertex(g, j), vb = pf_mask_vertex(g, j + 1 == nv ? 0 : j + 1);
            on = (a.what & PF_DRAW_CONTOURS) != 0;
            q.ax = s_xy[va][0]; q.ay = s_xy[va][1];
            q.dx = s_xy[vb][0] - q.ax; q.dy = s_xy[vb][1] - q.ay;
            q.len2 = (long long)q.dx * q.dx + (long long)q.dy * q.dy;
            q.bound = pf_draw_isqrt(64LL * a.w * a.w * q.len2);
            q.r2 = R * R;
            q.kind = PF_DRAW_EDGE | (2 << 4);
            pf_draw_span(min(q.ax, q.ax + q.dx) - R, max(q.ax, q.ax + q.dx) + R, a.W, &q.bx0, &q.bx1);
            pf_draw_span(min(q.ay, q.ay + q.dy) - R, max(q.ay, q.ay + q.dy) + R, a.H, &q.by0, &q.by1);
        } else {                                                 // top, bottom, left, right: the outline lies outside the box
            const int i = p - PF_DRAW_NPOINTS - PF_MASK_EDGES, w = a.w;
            const int x0 = s_box[0], y0 = s_box[1], x1 = s_box[2], y1 = s_box[3];
            on = (a.what & PF_DRAW_BOX) && x1 > x0 && y1 > y0;
            q.kind = PF_DRAW_BAR | (3 << 4);
            q.bx0 = i == 3 ? x1 : x0 - w; q.bx1 = i == 2 ? x0 : x1 + w;
            q.by0 = i == 0 ? y0 - w : (i == 1 ? y1 : y0); q.by1 = i == 0 ? y0 : (i == 1 ? y1 + w : y1);
            q.bx0 = min(max(q.bx0, 0), a.W); q.bx1 = min(max(q.bx1, 0), a.W);
            q.by0 = min(max(q.by0, 0), a.H); q.by1 = min(max(q.by1, 0), a.H);
        }
        if (!on || q.bx0 >= q.bx1 || q.by0 >= q.by1) {
            q.bx0 = q.by0 = q.bx1 = q.by1 = 0;
        } else {
            rect[0] = min(rect[0], q.bx0); rect[1] = min(rect[1], q.by0);
            rect[2] = max(rect[2], q.bx1); rect[3] = max(rect[3], q.by1);
        }
        a.prims[(size_t)slot * PF_DRAW_PRIMS + p] = q;
        a.bounds[(size_t)slot * PF_DRAW_PRIMS + p] = pf_draw_pack(q.bx0, q.by0, q.bx1, q.by1);
    }
    for (int i = 0; i < 4; ++i) s_rect[t][i] = rect[i];
    __syncthreads();
    if (t == 0) {
        for (int l = 1; l < 64; ++l) {
            rect[0] = min(rect[0], s_rect[l][0]); rect[1] = min(rect[1], s_rect[l][1]);
            rect[2] = max(rect[2], s_rect[l][2]); rect[3] = max(rect[3], s_rect[l][3]);
        }
        head[0] = 1;
        for (int i = 0; i < 4; ++i) head[1 + i] = rect[i];       // nothing drawn: x0 = W > x1 = 0, which meets no tile
        head[5] = head[6] = head[7] = 0;
    }
}

// --------------------------------------------------------------------------------------------
struct DrawArgs {
    const AlignFrame* frames;         // [images]: where output frame i reads its input
    const int* head;                  // [n][PF_DRAW_HEAD]
    const DrawPrim* prims;            // [n][PF_DRAW_PRIMS]
    const unsigned long long* bounds; // [n][PF_DRAW_PRIMS]
    unsigned char* out;               // [images][H][W][3]
    int n, per;                       // slots, slots per image
    int H, W, tiles_x, tiles;
    int alpha;                        // 1 .. 256
    unsigned colour[4];               // hi, lo, contour, box; the low byte is channel 0
    int no_cull;                      // DrawState::no_cull
};

// does primitive q cover the pixel whose centre is (16 px, 16 py)?  The pixel lies inside q's bounds.
__device__ __forceinline__ bool pf_draw_covers(const DrawPrim& q, int px, int py) {
    const int kind = q.kind & 15;
    if (kind == PF_DRAW_BAR) return true;
    const int qx = 16 * px - q.ax, qy = 16 * py - q.ay;          // below 2^21: every product below fits 64 bits with room
    if ((long long)qx * qx + (long long)qy * qy <= (long long)q.r2) return true;
    if (kind == PF_DRAW_DISC) return false;
    const int ex = qx - q.dx, ey = qy - q.dy;
    if ((long long)ex * ex + (long long)ey * ey <= (long long)q.r2) return true;
    if (q.len2 <= 0) return false;
    const long long dot = (long long)qx * q.dx + (long long)qy * q.dy;
    if (dot < 0 || dot > q.len2) return false;
    const long long cr = (long long)qx * q.dy - (long long)qy * q.dx;
    return (cr < 0 ? -cr : cr) <= q.bound;
}

// Positions of the threads with `hit` among all 256, in thread order, and their number; two barriers, so that s_wcnt can be used again
__device__ __forceinline__ int pf_draw_compact(int hit, int t, int* s_wcnt, int* total) {
    const unsigned long long m = __ballot(hit);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, sum = 0;
    for (int i = 0; i < 4; ++i) { if (i < wave) base += s_wcnt[i]; sum += s_wcnt[i]; }
    __syncthreads();
    *total = sum;
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// No byte outside [row start, row start + 3 W) of an input row is read and no byte outside `out` is written: word accesses are made
// only where all four bytes lie inside, whatever the alignment of the pointers, of 3 W and of the row stride.
__global__ __launch_bounds__(256) void draw_kernel(DrawArgs a) {
    constexpr int WORDS = ((3 + PF_MASK_TW * 3 + 3) / 4) | 1;    // odd pitch: the rows start on different banks
    __shared__ __attribute__((aligned(16))) unsigned s_src[PF_MASK_TH * WORDS];
    __shared__ DrawPrim s_list[256];
    __shared__ int s_slots[256];
    __shared__ int s_wcnt[4];
    const int t = threadIdx.x;
    const int img = blockIdx.x / a.tiles, tile = blockIdx.x - img * a.tiles;
    const int tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
    const int tx0 = tile_x * PF_MASK_TW, ty0 = tile_y * PF_MASK_TH;
    const int H = a.H, W = a.W;
    const int slot0 = img * a.per, slot1 = min(slot0 + a.per, a.n);
    const int qx = (t & 31) * 4, ry = t >> 5;                    // this thread's pixels: columns qx .. qx + 3 of rows ry and ry + 8
    const int x = tx0 + qx, npx = min(4, W - x);                 // npx <= 0: no pixel
    unsigned col[2] = {0u, 0u};                                  // byte k: colour index + 1 of pixel x + k, 0 = not covered
    unsigned und[2];                                             // bit k: pixel x + k is not decided yet
    for (int p = 0; p < 2; ++p) und[p] = (ty0 + ry + 8 * p < H && npx > 0) ? (1u << npx) - 1u : 0u;
    int listed = 0;                                              // primitives listed so far: the same in every thread
    for (int c0 = slot0; c0 < slot1; c0 += 256) {                // 256 slots a pass: the rectangles that meet the tile, in slot order
        const int slot = c0 + t;
        int hit = 0;
        if (slot < slot1) {
            const int* hd = a.head + (size_t)slot * PF_DRAW_HEAD;
            if (hd[0]) hit = a.no_cull || (hd[1] < tx0 + PF_MASK_TW && hd[3] > tx0 && hd[2] < ty0 + PF_MASK_TH && hd[4] > ty0);
        }
        int ns;
        const int spos = pf_draw_compact(hit, t, s_wcnt, &ns);
        if (ns == 0) continue;
        if (hit) s_slots[spos] = slot;
        __syncthreads();
        const int ncand = ns * PF_DRAW_PRIMS;
        for (int k0 = 0; k0 < ncand; k0 += 256) {                // a round: 256 candidates in priority order
            const int c = k0 + t;
            const DrawPrim* pr = nullptr;
            int take = 0;
            if (c < ncand) {
                const int j = c / PF_DRAW_PRIMS;
                const size_t at = (size_t)s_slots[j] * PF_DRAW_PRIMS + (c - j * PF_DRAW_PRIMS);
                pr = a.prims + at;
                const unsigned long long b = a.bounds[at];       // consecutive threads, consecutive 8 bytes
                const int bx0 = (int)(b & 0xFFFFu), bx1 = (int)((b >> 16) & 0xFFFFu), by0 = (int)((b >> 32) & 0xFFFFu), by1 = (int)(b >> 48);
                take = bx0 < bx1 && by0 < by1 && (a.no_cull || (bx0 < tx0 + PF_MASK_TW && bx1 > tx0 && by0 < ty0 + PF_MASK_TH && by1 > ty0));
            }
            int np;
            const int pos = pf_draw_compact(take, t, s_wcnt, &np);
            if (np == 0) continue;
            listed += np;
            if (take) {
                const uint4* s = reinterpret_cast<const uint4*>(pr);
                uint4* d = reinterpret_cast<uint4*>(&s_list[pos]);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = s[i];
            }
            __syncthreads();
            for (int i = 0; i < np && (und[0] | und[1]); ++i) {
                const DrawPrim& q = s_list[i];                   // every thread reads the same entry: a broadcast
                const unsigned code = (unsigned)(q.kind >> 4) + 1u;
                for (int p = 0; p < 2; ++p) {
                    const int y = ty0 + ry + 8 * p;
                    if (!und[p] || y < q.by0 || y >= q.by1) continue;
                    for (int k = 0; k < 4; ++k) {
                        if (!((und[p] >> k) & 1u) || x + k < q.bx0 || x + k >= q.bx1) continue;
                        if (pf_draw_covers(q, x + k, y)) { col[p] |= code << (8 * k); und[p] &= ~(1u << k); }
                    }
                }
            }
            __syncthreads();                                     // the list has been read
        }
    }
    const AlignFrame f = a.frames[img];
    unsigned char* const out = a.out + (size_t)img * H * W * 3;
    if (!listed && !a.no_cull) {                                 // 16 threads per row segment of at most 384 bytes
        const int r = t >> 4, y = ty0 + r;
        if (y < H)
            pf_redact_copy(out + ((size_t)y * W + tx0) * 3, f.base + (size_t)y * f.row_stride + (size_t)tx0 * 3, min(PF_MASK_TW, W - tx0) * 3,
                           t & 15, 16);
        return;
    }
    // ---- the tile's pixels, as the aligned 32-bit words that hold them ----
    const int fx1 = min(tx0 + PF_MASK_TW, W), fh = min(ty0 + PF_MASK_TH, H) - ty0;
    const bool rows_aligned = (f.row_stride & 3) == 0;
    const int shift = rows_aligned ? (int)(((size_t)f.base + (size_t)tx0 * 3) & 3) : 0;
    const int words = (shift + (fx1 - tx0) * 3 + 3) / 4;         // <= WORDS
    const int row_bytes = W * 3;
    for (int i = t; i < fh * words; i += 256) {
        const int r = i / words, wd = i - r * words;
        const unsigned char* row = f.base + (size_t)(ty0 + r) * f.row_stride;
        const int bx = tx0 * 3 - shift + 4 * wd;                 // byte offset inside the frame row
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
    // ---- the output: one colour, applied once ----
    const unsigned na = 256u - (unsigned)a.alpha, al = (unsigned)a.alpha;
    for (int p = 0; p < 2; ++p) {
        const int j = ry + 8 * p, y = ty0 + j;
        if (y >= H || npx <= 0) continue;
        const unsigned char* srow = reinterpret_cast<const unsigned char*>(s_src) + (size_t)j * WORDS * 4 + shift + qx * 3;
        unsigned char o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = k < npx * 3 ? srow[k] : (unsigned char)0;
        if (col[p]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned code = (col[p] >> (8 * k)) & 255u;
                if (!code) continue;
                const unsigned c = code == 1u ? a.colour[0] : (code == 2u ? a.colour[1] : (code == 3u ? a.colour[2] : a.colour[3]));
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    o[3 * k + ch] = (unsigned char)(((unsigned)o[3 * k + ch] * na + ((c >> (8 * ch)) & 255u) * al + 128u) >> 8);
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

// Per-face region statistics (pf_measure_faces / pf_face_stats, stats.inl): for every slot k and label L in 1..8, nine exact integer
// sums over the frame pixels with owner == k + 1 and label == L of the maps of k_mask.h -- n, the three channel sums, the sums of the
// luma Y and of Y^2, the sum of the squared 4-neighbour Laplacian of Y, and the numbers of dark and bright pixels.  The first kernel
// here that turns a face into numbers; nothing is stored per pixel.
//
//   face_stats_zero_kernel    the 72 values of every VALID slot become 0; rows of invalid slots are never touched
//   face_stats_kernel         segmented reduction: workgroup (slot, band) walks its share of the rows of the slot's clipped box, a
//                             thread per pixel, every value read from global memory, one 64-bit LDS atomic per (label, field) and
//                             pixel, and adds its 72 sums to the slot's row
//   face_stats_staged_kernel  the same grid walking the rows in pieces of the maps' tile size (128 x 16) staged in LDS, with
//                             per-thread registers and a shuffle reduction; measurement tool's build only (StatsState::staged)
//
// The arithmetic is the specification and is restated in numpy by tests/stats_ref.py: integers only, so every
// value is reproducible whatever the order of addition.
//
// A slot's work is its box, not the frame: invalid slots, empty boxes and bands past the box's last row return at once.
// Which form ships was decided by measurement (tools/bench_face_stats.py, profiles/face_stats_bench.json; both give identical
// values): the staged form was written first, as the one that reads every frame byte once and keeps the additions in registers, and
// the direct form as the straightforward yardstick.  On MI355X the direct form is the faster of the two -- level with the staged one
// on 200 x 260 faces and about 2.5 x faster on 100 x 130 faces, where a workgroup of the staged form walks one or two pieces and then
// pays three barriers per piece and a 72-value shuffle reduction -- so it ships.  A face's pixels are read by one workgroup while
// they are hot in cache (the five luma reads of a pixel hit lines its neighbours fetched), and an LDS atomic needs no flush.
// Width discipline of the direct form: there is no 32-bit partial anywhere.  Every addend of every pixel goes straight into a 64-bit
// LDS total, the totals leave as 64-bit atomics, and a pixel index inside a band is at most 1024 rows x 32768 columns < 2^31.
//
// The staged form, per piece:
//   1. the piece plus a ring of one pixel, clipped to the frame, is staged in LDS as the 32-bit words that hold it in global memory
//      (a row's first word starts 4-byte aligned and the shift is kept, as redact_kernel does);
//   2. Y is computed once per staged pixel into LDS;
//   3. a thread owns four consecutive pixels of rows r and r + 8, reads their labels and owners as one word each where the address
//      allows it, takes the Laplacian from LDS with the neighbour coordinates clamped to the FRAME (the clamped coordinate always
//      lies inside the staged footprint), and adds into 8 x 5 32-bit registers, statically indexed by label.
// Width discipline of the staged form: a thread adds at most 8 pixels per piece and its registers are flushed after at most PF_STATS_FLUSH = 32 pieces,
// i.e. 256 pixels.  The nine partial sums of a label share five registers (72 separate ones cost 238 VGPRs and half the occupancy):
//   n | dark << 10 | bright << 20    each count <= 256 < 2^10
//   sum c0 | sum c1 << 16            each <= 256 x 255 = 65 280 < 2^16; likewise sum c2 | sum Y << 16
//   sum Y^2                          <= 256 x 65 025 < 2^24
//   sum Lap^2                        <= 256 x 1020^2 = 266 342 400 < 2^32
// A flush unpacks them; the wave's shuffles run in 32 bits for the eight fields whose sum over 64 lanes fits (the largest, Y^2:
// 64 x 256 x 65 025 < 2^30) and in 64 bits for sum Lap^2, which does not; from there on -- across the waves through LDS, the
// workgroup's running totals, the output -- everything is 64-bit.  The bound holds for every frame size the maps accept because it
// counts pieces, not rows.
// Output across bands, either form: 72 integer atomicAdds per workgroup into the row face_stats_zero_kernel cleared, not a partials buffer with a
// second pass.  The sums are integers, so the order of the additions cannot change a bit (unlike the floats of face_attrs_kernel);
// contention is at most the band count (<= 32) per address; and a partials buffer would be slots x bands x 576 bytes, 19 GB at the
// 2^20 slots the entry points accept.  LDS: 576 bytes of totals (direct); 7.1 KB of words + 2.4 KB of Y + 2.3 KB of wave sums (staged).
#pragma once
#include "k_mask.h"

#define PF_STATS_LABELS 8
#define PF_STATS_FIELDS 9
#define PF_STATS_ROW (PF_STATS_LABELS * PF_STATS_FIELDS)
#define PF_STATS_MAX_BANDS 32
#define PF_STATS_REGS 5               // 32-bit registers per label: n | dark | bright, c0 | c1, c2 | Y, Y^2, Lap^2
#define PF_STATS_FLUSH 32             // pieces between two flushes of the 32-bit registers (see the header)
#define PF_STATS_FW (PF_MASK_TW + 2)  // staged columns and rows: the piece and its ring
#define PF_STATS_FH (PF_MASK_TH + 2)
#define PF_STATS_WORDS 99             // (3 + 130 * 3 + 3) / 4 = 99, odd: the rows of the footprint start on different banks

// Host side of a handle: the label maps the reduction reads and the staging of host outputs
struct StatsState {
    unsigned char* d_labels = nullptr; size_t labels_bytes = 0;
    unsigned char* d_owners = nullptr; size_t owners_bytes = 0;
    int* d_valid = nullptr; size_t valid_bytes = 0;
    AlignFrame* d_table = nullptr; size_t table_bytes = 0;
    unsigned long long* d_out = nullptr; size_t out_bytes = 0;
    std::vector<int> h_valid;
    std::vector<AlignFrame> h_table;
    int staged = 0;                   // measurement tool's build only: face_stats_staged_kernel in place of face_stats_kernel
    void release() {
        void* ptrs[] = {d_labels, d_owners, d_valid, d_table, d_out};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = StatsState();
    }
};

struct StatsArgs {
    const AlignFrame* frames;         // [images]: where the slots of image i read their pixels
    const int* rec;                   // [n][PF_MASK_REC] of mask_edges_kernel: valid flag and clipped box
    const unsigned char* labels;      // [images][H][W]
    const unsigned char* owners;      // like labels: slot within the image + 1
    unsigned long long* out;          // [n][8][9]
    int n, per;                       // slots, slots per image
    int H, W;
    int bands;                        // workgroups per slot
    int dark, bright;
};

__device__ __forceinline__ int pf_stats_luma(unsigned c0, unsigned c1, unsigned c2) { return (int)((29u * c0 + 150u * c1 + 77u * c2 + 128u) >> 8); }

// the rows [*y0, *y1) of the box rows [by0, by1) that band `band` of `bands` walks: whole pieces of PF_MASK_TH rows, dealt out in runs
__device__ __forceinline__ void pf_stats_band_rows(int by0, int by1, int band, int bands, int* y0, int* y1) {
    const int pieces = (by1 - by0 + PF_MASK_TH - 1) / PF_MASK_TH, per = (pieces + bands - 1) / bands;
    *y0 = min(by0 + band * per * PF_MASK_TH, by1);
    *y1 = min(*y0 + per * PF_MASK_TH, by1);
}

__global__ __launch_bounds__(256) void face_stats_zero_kernel(StatsArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.n * PF_STATS_ROW) return;
    if (a.rec[(size_t)(i / PF_STATS_ROW) * PF_MASK_REC]) a.out[i] = 0ull;
}

template <typename T>
__device__ __forceinline__ T pf_stats_wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// The registers of the four waves, unpacked and summed: per wave by shuffle -- in 32 bits where 64 lanes x 256 pixels fit (sum Y^2:
// 64 x 256 x 65 025 < 2^30), sum Lap^2 in 64 -- then across the waves through LDS in 64 bits into `tot` of the threads t < 72; the
// registers restart at zero.  Every thread of the workgroup calls it.
__device__ __forceinline__ void pf_stats_flush(unsigned (&acc)[PF_STATS_LABELS][PF_STATS_REGS], unsigned long long (*s_red)[PF_STATS_ROW],
                                               unsigned long long& tot, int t) {
#pragma unroll
    for (int L = 0; L < PF_STATS_LABELS; ++L) {
        const unsigned a0 = acc[L][0], a1 = acc[L][1], a2 = acc[L][2];
        unsigned v[PF_STATS_FIELDS];
        v[0] = a0 & 1023u; v[7] = (a0 >> 10) & 1023u; v[8] = a0 >> 20;
        v[1] = a1 & 0xFFFFu; v[2] = a1 >> 16; v[3] = a2 & 0xFFFFu; v[4] = a2 >> 16;
        v[5] = acc[L][3]; v[6] = 0u;
        const unsigned long long lap = pf_stats_wave_sum((unsigned long long)acc[L][4]);
#pragma unroll
        for (int r = 0; r < PF_STATS_REGS; ++r) acc[L][r] = 0u;
#pragma unroll
        for (int f = 0; f < PF_STATS_FIELDS; ++f) {
            if (f != 6) v[f] = pf_stats_wave_sum(v[f]);
            if ((t & 63) == 0) s_red[t >> 6][L * PF_STATS_FIELDS + f] = f == 6 ? lap : (unsigned long long)v[f];
        }
    }
    __syncthreads();
    if (t < PF_STATS_ROW) tot += s_red[0][t] + s_red[1][t] + s_red[2][t] + s_red[3][t];
    __syncthreads();                                             // s_red is free again
}

// No byte outside [row start, row start + 3 W) of a frame row and no byte outside the maps is read: word accesses are made only where
// all four bytes lie inside.  Every branch around a barrier or a shuffle depends on the arguments and the record alone and is uniform.
__global__ __launch_bounds__(256) void face_stats_staged_kernel(StatsArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned s_src[PF_STATS_FH * PF_STATS_WORDS];
    __shared__ unsigned char s_y[PF_STATS_FH][PF_STATS_FW + 2];
    __shared__ unsigned long long s_red[4][PF_STATS_ROW];
    const int t = threadIdx.x;
    const int slot = blockIdx.x / a.bands, band = blockIdx.x - slot * a.bands;
    const int* rec = a.rec + (size_t)slot * PF_MASK_REC;
    if (!rec[0]) return;
    const int bx0 = rec[1], by0 = rec[2], bx1 = rec[3], by1 = rec[4];
    if (bx0 >= bx1 || by0 >= by1) return;
    int ry0, ry1;
    pf_stats_band_rows(by0, by1, band, a.bands, &ry0, &ry1);
    if (ry0 >= ry1) return;
    const int H = a.H, W = a.W;
    const int img = slot / a.per;
    const unsigned me = (unsigned)(slot - img * a.per + 1);       // this slot in the owners
    const AlignFrame f = a.frames[img];
    const bool rows_aligned = (f.row_stride & 3) == 0;
    const int row_bytes = W * 3;
    const unsigned char* const labels = a.labels + (size_t)img * H * W;
    const unsigned char* const owners = a.owners + (size_t)img * H * W;
    const int qx = (t & 31) * 4, ry = t >> 5;                    // this thread's pixels: columns qx .. qx + 3 of rows ry and ry + 8
    const int bxa = bx0 & ~3;                                    // >= 0; the pixels left of the box belong to nobody
    unsigned acc[PF_STATS_LABELS][PF_STATS_REGS];
#pragma unroll
    for (int L = 0; L < PF_STATS_LABELS; ++L)
#pragma unroll
        for (int k = 0; k < PF_STATS_REGS; ++k) acc[L][k] = 0u;
    unsigned long long tot = 0ull;
    int since = 0;                                               // pieces in the registers
    for (int py0 = ry0; py0 < ry1; py0 += PF_MASK_TH) {
        const int py1 = min(py0 + PF_MASK_TH, ry1);
        for (int px0 = bxa; px0 < bx1; px0 += PF_MASK_TW) {
            const int px1 = min(px0 + PF_MASK_TW, bx1);
            // ---- 1. the footprint ----
            const int fx0 = max(px0 - 1, 0), fx1 = min(px1 + 1, W), fy0 = max(py0 - 1, 0), fy1 = min(py1 + 1, H);
            const int fw = fx1 - fx0, fh = fy1 - fy0;            // <= 130, <= 18
            const int shift = rows_aligned ? (int)(((size_t)f.base + (size_t)fx0 * 3) & 3) : 0;
            const int words = (shift + fw * 3 + 3) / 4;          // <= 99
            if (since) __syncthreads();                          // the previous piece has been read
            for (int r = t >> 7; r < fh; r += 2) {
                const int wd = t & 127;
                if (wd >= words) continue;
                const unsigned char* row = f.base + (size_t)(fy0 + r) * f.row_stride;
                const int bx = fx0 * 3 - shift + 4 * wd;         // byte offset inside the frame row
                unsigned v = 0u;
                if (rows_aligned && bx >= 0 && bx + 4 <= row_bytes) {
                    v = *reinterpret_cast<const unsigned*>(row + bx);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bx + k >= 0 && bx + k < row_bytes) v |= (unsigned)row[bx + k] << (8 * k);
                }
                s_src[r * PF_STATS_WORDS + wd] = v;
            }
            __syncthreads();
            // ---- 2. the luma ----
            for (int r = t >> 7; r < fh; r += 2)
                for (int c = t & 127; c < fw; c += 128) {
                    const unsigned char* p = reinterpret_cast<const unsigned char*>(s_src) + (size_t)r * PF_STATS_WORDS * 4 + shift + c * 3;
                    s_y[r][c] = (unsigned char)pf_stats_luma(p[0], p[1], p[2]);
                }
            __syncthreads();
            // ---- 3. this thread's pixels ----
            const int x = px0 + qx, npx = min(4, px1 - x);       // npx <= 0: no pixel
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int y = py0 + ry + 8 * p;
                if (y >= py1 || npx <= 0) continue;
                const size_t o = (size_t)y * W + x;
                unsigned lab = 0u, own = 0u;
                if (npx == 4 && ((size_t)(labels + o) & 3) == 0) {
                    lab = *reinterpret_cast<const unsigned*>(labels + o);
                    if (lab) own = *reinterpret_cast<const unsigned*>(owners + o);      // maps of one allocation size: aligned alike
                } else {
                    for (int k = 0; k < npx; ++k) {
                        lab |= (unsigned)labels[o + k] << (8 * k);
                        own |= (unsigned)owners[o + k] << (8 * k);
                    }
                }
                if (!lab) continue;
                const unsigned char* srow = reinterpret_cast<const unsigned char*>(s_src) + (size_t)(y - fy0) * PF_STATS_WORDS * 4 + shift + (x - fx0) * 3;
                const unsigned char* yc = &s_y[y - fy0][0];
                const unsigned char* yu = &s_y[max(y - 1, 0) - fy0][0];
                const unsigned char* yd = &s_y[min(y + 1, H - 1) - fy0][0];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned L = (lab >> (8 * k)) & 255u;
                    if (k >= npx || L == 0u || ((own >> (8 * k)) & 255u) != me) continue;
                    const int xc = x + k - fx0, xl = max(x + k - 1, 0) - fx0, xr = min(x + k + 1, W - 1) - fx0;
                    const unsigned c0 = srow[3 * k], c1 = srow[3 * k + 1], c2 = srow[3 * k + 2];
                    const int Y = yc[xc];
                    const int lap = 4 * Y - yc[xl] - yc[xr] - yu[xc] - yd[xc];
                    const unsigned yy = (unsigned)(Y * Y), ll = (unsigned)(lap * lap);
                    const unsigned v0 = 1u | (Y <= a.dark ? 1u << 10 : 0u) | (Y >= a.bright ? 1u << 20 : 0u);
                    const unsigned v1 = c0 | (c1 << 16), v2 = c2 | ((unsigned)Y << 16);
#pragma unroll
                    for (int g = 0; g < PF_STATS_LABELS; ++g)    // static register indices: the label picks by comparison
                        if (L == (unsigned)(g + 1)) { acc[g][0] += v0; acc[g][1] += v1; acc[g][2] += v2; acc[g][3] += yy; acc[g][4] += ll; }
                }
            }
            if (++since == PF_STATS_FLUSH) {
                pf_stats_flush(acc, s_red, tot, t);
                since = 0;
            }
        }
    }
    if (since) pf_stats_flush(acc, s_red, tot, t);
    if (t < PF_STATS_ROW && tot) atomicAdd(a.out + (size_t)slot * PF_STATS_ROW + t, tot);
}

// The direct form, which ships: a thread per pixel of the band's share of the box, the pixel and its four neighbours read from global
// memory (no byte outside a frame row or the maps: every coordinate is clamped to the frame), one 64-bit LDS atomic per field.
__global__ __launch_bounds__(256) void face_stats_kernel(StatsArgs a) {
    __shared__ unsigned long long s_tot[PF_STATS_ROW];
    const int t = threadIdx.x;
    const int slot = blockIdx.x / a.bands, band = blockIdx.x - slot * a.bands;
    const int* rec = a.rec + (size_t)slot * PF_MASK_REC;
    if (!rec[0]) return;
    const int bx0 = rec[1], by0 = rec[2], bx1 = rec[3], by1 = rec[4];
    if (bx0 >= bx1 || by0 >= by1) return;
    int ry0, ry1;
    pf_stats_band_rows(by0, by1, band, a.bands, &ry0, &ry1);
    if (ry0 >= ry1) return;
    const int H = a.H, W = a.W, bw = bx1 - bx0;
    const int img = slot / a.per;
    const unsigned me = (unsigned)(slot - img * a.per + 1);
    const AlignFrame f = a.frames[img];
    const unsigned char* const labels = a.labels + (size_t)img * H * W;
    const unsigned char* const owners = a.owners + (size_t)img * H * W;
    if (t < PF_STATS_ROW) s_tot[t] = 0ull;
    __syncthreads();
    const unsigned count = (unsigned)(ry1 - ry0) * (unsigned)bw;      // a band has at most 1024 rows of at most 32768 columns
    for (unsigned i = t; i < count; i += 256u) {
        const int y = ry0 + (int)(i / (unsigned)bw), x = bx0 + (int)(i % (unsigned)bw);
        const size_t o = (size_t)y * W + x;
        const unsigned L = labels[o];
        if (L == 0u || L > (unsigned)PF_STATS_LABELS || owners[o] != me) continue;
        int Y[5];
        const int nx[5] = {x, max(x - 1, 0), min(x + 1, W - 1), x, x}, ny[5] = {y, y, y, max(y - 1, 0), min(y + 1, H - 1)};
        unsigned c[3] = {0u, 0u, 0u};
        for (int k = 0; k < 5; ++k) {
            const unsigned char* p = f.base + (size_t)ny[k] * f.row_stride + (size_t)nx[k] * 3;
            Y[k] = pf_stats_luma(p[0], p[1], p[2]);
            if (k == 0) { c[0] = p[0]; c[1] = p[1]; c[2] = p[2]; }
        }
        const int lap = 4 * Y[0] - Y[1] - Y[2] - Y[3] - Y[4];
        unsigned long long* row = s_tot + (L - 1u) * PF_STATS_FIELDS;
        atomicAdd(row + 0, 1ull); atomicAdd(row + 1, (unsigned long long)c[0]); atomicAdd(row + 2, (unsigned long long)c[1]);
        atomicAdd(row + 3, (unsigned long long)c[2]); atomicAdd(row + 4, (unsigned long long)Y[0]);
        atomicAdd(row + 5, (unsigned long long)(Y[0] * Y[0])); atomicAdd(row + 6, (unsigned long long)(lap * lap));
        if (Y[0] <= a.dark) atomicAdd(row + 7, 1ull);
        if (Y[0] >= a.bright) atomicAdd(row + 8, 1ull);
    }
    __syncthreads();
    if (t < PF_STATS_ROW && s_tot[t]) atomicAdd(a.out + (size_t)slot * PF_STATS_ROW + t, s_tot[t]);
}

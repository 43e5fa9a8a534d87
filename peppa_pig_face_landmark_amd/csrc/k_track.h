// Tracking state of one video stream on the device.
//
// FaceAna.run() keeps three pieces of state between frames (Skps/core/api/facer.py:40-42, core/smoother/lk.py:8-9):
// the boxes of the previous frame (track_box), the previous landmark sets and their last displacement.  Between the
// detector and the landmark regressor it matches boxes by IoU and smooths them (judge_boxs :144-189), keeps the top-k by
// area (sort_and_filter :120-142); after the regressor it smooths the landmarks with a One-Euro filter against the
// previous set (GroupTrack.calculate, lk.py:19-56,117-149) and derives the next track boxes from their hulls (:70-81).
// On the host that costs a device->host->device trip of the boxes between the two networks on every frame.  The
// kernels below keep all of it in HBM, for one stream (pf_track_frame) or for the N streams of a pf_track_streams call
// (the state of each in its slot of a TrackPool): one small workgroup per frame -- a stream has at most top_k faces --
// so the arithmetic of every stream is the same code whatever the number of streams in the call.
//
// Values are STORED as float64, but the arithmetic follows the dtype numpy would be working in (round 3): detector rows and
// network landmarks are float32, `landmarks / [w, h]` (lk.py:39-41) promotes a smoothed landmark set -- and from there the
// hull boxes, the EMA-smoothed track boxes and the next frame's crop arithmetic -- to float64, and np.array([...]) of mixed
// rows is float64 as soon as one row is.  So a frame's boxes are float32 on a detector frame with nothing to smooth against
// and float64 once the stream is running; IoU, EMA, areas and FaceLandmark.preprocess round differently in the two (a crop
// edge lands on the other side of an integer), hence three dtype flags travel with the state: track boxes, current boxes,
// landmark sets.  A float32 value is exactly representable in its float64 slot, so only the operations need the flag.
#pragma once
#include <vector>

#include "pf_common.h"

const int kTrackMaxNow = 1024;   // rows NMS can keep per frame (judge_boxs input)

// One frame of a tracking call (pf_track_frame: one; pf_track_streams: one per listed stream), built on the host after the
// gate and uploaded once per call.  Every track kernel below has the frame index i as a grid dimension and finds its
// stream's state through `slot`: state of slot s persists across calls, scratch of frame i lives only for the call.
struct TrackFrameDesc {
    int slot;        // stream slot of the pool
    int cur;         // which ping-pong half of the slot holds the PREVIOUS landmark sets (the new ones go to cur ^ 1)
    int has_track;   // track_box is not None
    int lm_valid;    // trace.previous_landmarks_set is not None (0 on a detector frame, facer.py:60)
    int det;         // index of this frame among the call's detector frames (its NMS rows), -1: the gate skipped the detector
    int cmp;         // track_gate_kernel: the slot holds a previous frame of the same size
};

// Device arrays of a slot pool (pointers only, passed by value to the kernels).
struct TrackPoolView {
    // ---- state of slot s
    double* track_box;   // [S][kTrackMaxNow][4] boxes of the previous frame (FaceAna.track_box)
    int* n_track;        // [S] rows of it
    double* lm;          // [S][2][K][98][2] previous / new landmark sets (ping-pong)
    double* dx;          // [S][2][K][98][2] previous_dx
    int* n_lm;           // [S][2] rows of each
    // dtype flags (1 = float32, 0 = float64), on the device because they depend on which rows matched:
    // [s][0] track_box  [s][1] judge_boxs output of a detector frame  [s][2], [s][3] landmark sets (ping-pong, like lm)
    int* f32;            // [S][4]
    // ---- scratch of frame i of a call (capacity K rows per frame, the call's rows at stride top_k)
    double* judged;      // [S][kTrackMaxNow][4] judge_boxs(track_box, detector boxes)
    int* n_judged;       // [S]
    double* sel;         // [S][K][4] sort_and_filter output == boxes_return, fed to the landmark stage
    int* n_sel;          // [S] (doubles as the per-frame count of the landmark stage)
    int* sel_f32;        // [S] dtype flag of sel (per-frame flag of crop_params_kernel)
    double* hull;        // [S][K][4] hull boxes of the new landmark sets (tmp_box)
    float* scores;       // [S][K][98] scores of the valid faces, compacted like the landmarks
    int* out_count;      // [S] results of frame i, gathered from its slot (track_gather_kernel)
    double* out_box;     // [S][K][4]
    double* out_lm;      // [S][K][98][2]
    const TrackFrameDesc* desc;   // [S], the first n used
    int K;               // faces per slot the pool was allocated for
    int top_k;           // faces per frame of this call (<= K)
    __device__ double* slot_lm(double* base, int slot, int half) const { return base + ((size_t)slot * 2 + half) * K * 196; }
};

// Host side of a pool: the device arrays plus each slot's host-known state.  pf_track_frame owns a pool of one slot,
// pf_track_streams one of max_streams slots (track.inl).
struct TrackSlot {
    int cur = 0;                // ping-pong half holding the previous sets
    bool has_track = false;     // track_box is not None
    bool lm_valid = false;      // trace.previous_landmarks_set is not None
    bool have_prev = false;     // pf_track_streams: the slot's frame buffer holds the stream's previous frame ...
    int prev_h = 0, prev_w = 0; // ... of this size
};

struct TrackPool {
    TrackPoolView v{};
    TrackFrameDesc* d_desc = nullptr;
    int S = 0, K = 0;
    std::vector<TrackSlot> slots;
    std::vector<TrackFrameDesc> h_desc;   // staging of the descriptor upload: lives until the call's final synchronisation
    // pf_track_streams only: previous frame of every slot ([S][frame_slot_bytes]) and the gate's sums
    unsigned char* d_frames = nullptr; size_t frame_slot_bytes = 0;
    unsigned long long* d_sums = nullptr;
    int* d_det_idx = nullptr;              // [S] call indices of the detector frames (letterbox_kernel frame_idx)
    std::vector<int> h_det_idx;
    std::vector<unsigned long long> h_sums;
    std::vector<double> h_box, h_lm;       // pf_track_frame: host staging of the results (trimmed to the count after the sync)
    std::vector<float> h_scores;
    void release() {
        void* ptrs[] = {v.track_box, v.n_track, v.lm, v.dx, v.n_lm, v.f32, v.judged, v.n_judged, v.sel, v.n_sel, v.sel_f32,
                        v.hull, v.scores, v.out_count, v.out_box, v.out_lm, d_desc, d_frames, d_sums, d_det_idx};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = TrackPool();
    }
};

__device__ __forceinline__ double pf_box_iou_f64(const double* a, const double* b) {   // facer.py:152-172, lk.py:58-80
    const double s1 = (a[2] - a[0]) * (a[3] - a[1]);
    const double s2 = (b[2] - b[0]) * (b[3] - b[1]);
    const double x1 = fmax(a[0], b[0]), y1 = fmax(a[1], b[1]);
    const double x2 = fmin(a[2], b[2]), y2 = fmin(a[3], b[3]);
    const double inter = fmax(0.0, x2 - x1) * fmax(0.0, y2 - y1);
    return inter / (s1 + s2 - inter);
}
// the same on float32 scalars (both boxes float32: numpy keeps float32 scalar arithmetic in float32); no FMA contraction
__device__ __forceinline__ double pf_box_iou_f32(const double* a, const double* b) {
    const float a0 = (float)a[0], a1 = (float)a[1], a2 = (float)a[2], a3 = (float)a[3];
    const float b0 = (float)b[0], b1 = (float)b[1], b2 = (float)b[2], b3 = (float)b[3];
    const float s1 = __fmul_rn(__fsub_rn(a2, a0), __fsub_rn(a3, a1));
    const float s2 = __fmul_rn(__fsub_rn(b2, b0), __fsub_rn(b3, b1));
    const float x1 = fmaxf(a0, b0), y1 = fmaxf(a1, b1), x2 = fminf(a2, b2), y2 = fminf(a3, b3);
    const float inter = __fmul_rn(fmaxf(0.f, __fsub_rn(x2, x1)), fmaxf(0.f, __fsub_rn(y2, y1)));   // max(0, f32) stays f32
    return (double)__fdiv_rn(inter, __fsub_rn(__fadd_rn(s1, s2), inter));
}
__device__ __forceinline__ double pf_box_iou(const double* a, int a32, const double* b, int b32) {
    return (a32 && b32) ? pf_box_iou_f32(a, b) : pf_box_iou_f64(a, b);
}
// exponential_smoothing(alpha, x, x_prev) = alpha * x + (1 - alpha) * x_prev on ARRAYS (lk.py:96-97): a python float times a
// float32 array is a float32 product, the sum is float32 only if both terms are
__device__ __forceinline__ double pf_ema(double alpha, double x, int x32, double p, int p32) {
    const double om = 1.0 - alpha;
    if (x32 && p32) return (double)__fadd_rn(__fmul_rn((float)alpha, (float)x), __fmul_rn((float)om, (float)p));
    const double t1 = x32 ? (double)__fmul_rn((float)alpha, (float)x) : alpha * x;
    const double t2 = p32 ? (double)__fmul_rn((float)om, (float)p) : om * p;
    return t1 + t2;
}

// judge_boxs (facer.py:144-189): every current box is matched against the FIRST previous box with IoU > thres and
// EMA-smoothed with it (alpha * now + (1 - alpha) * previous), or passed through.  The result array is float32 only if
// the current rows are and no float64 previous row was mixed in.  One workgroup per frame f of the call, two stages:
//   TRACK_JUDGE_DETECTIONS  track_box vs the frame's NMS rows -> judged (detector frames only)     facer.py:58-59
//   TRACK_JUDGE_HULLS       boxes_return vs the hull boxes    -> track_box (every frame)          facer.py:70-81
enum { TRACK_JUDGE_DETECTIONS = 0, TRACK_JUDGE_HULLS = 1 };
struct JudgeArgs {      // the operands of one frame
    const double* prev; const int* n_prev; int has_prev;      // has_prev == 0: previous is None -> pass through
    const int* prev_f32;                                      // dtype flag of prev (device), nullptr = float64
    const float* now_f32; int now_stride;                     // detector rows (float32, stride 16) ...
    const double* now_f64;                                    // ... or rows of 4 stored as float64,
    const int* now_f32_flag;                                  //     whose dtype flag is here (nullptr = float64)
    const int* n_now;
    double* out; int* n_out;
    int* out_f32;                                             // dtype flag of the result
    double iou_thres, alpha;
    int max_now;
};

struct JudgeStageArgs {
    TrackPoolView v;
    int stage;
    const float* det_rows; const int* det_count; int det_stride;   // NMS output: [D][det_stride][16] rows, [D] counts
    double iou_thres, alpha;
};

__global__ __launch_bounds__(256) void track_judge_kernel(JudgeStageArgs g) {
    __shared__ int s_mixed;                                   // some row was smoothed against a float64 previous row
    const int f = blockIdx.x;
    const TrackFrameDesc d = g.v.desc[f];
    const int s = d.slot, nxt = d.cur ^ 1;
    JudgeArgs a{};
    a.iou_thres = g.iou_thres; a.alpha = g.alpha;
    if (g.stage == TRACK_JUDGE_DETECTIONS) {
        if (d.det < 0) return;                                // uniform per workgroup: the gate skipped the detector
        a.prev = g.v.track_box + (size_t)s * kTrackMaxNow * 4; a.n_prev = g.v.n_track + s; a.has_prev = d.has_track;
        a.prev_f32 = g.v.f32 + (size_t)s * 4 + 0;
        a.now_f32 = g.det_rows + (size_t)d.det * g.det_stride * 16; a.now_stride = 16; a.now_f64 = nullptr; a.now_f32_flag = nullptr;
        a.n_now = g.det_count + d.det;
        a.out = g.v.judged + (size_t)f * kTrackMaxNow * 4; a.n_out = g.v.n_judged + f; a.out_f32 = g.v.f32 + (size_t)s * 4 + 1;
        a.max_now = kTrackMaxNow;
    } else {
        a.prev = g.v.sel + (size_t)f * g.v.top_k * 4; a.n_prev = g.v.n_sel + f; a.has_prev = 1; a.prev_f32 = g.v.sel_f32 + f;
        a.now_f32 = nullptr; a.now_stride = 4; a.now_f64 = g.v.hull + (size_t)f * g.v.top_k * 4;
        a.now_f32_flag = g.v.f32 + (size_t)s * 4 + 2 + nxt; a.n_now = g.v.n_lm + (size_t)s * 2 + nxt;
        a.out = g.v.track_box + (size_t)s * kTrackMaxNow * 4; a.n_out = g.v.n_track + s; a.out_f32 = g.v.f32 + (size_t)s * 4 + 0;
        a.max_now = g.v.top_k;
    }
    if (threadIdx.x == 0) s_mixed = 0;
    __syncthreads();
    const int n = min(*a.n_now, a.max_now);
    const int np = a.has_prev ? *a.n_prev : 0;
    const int n32 = a.now_f64 ? (a.now_f32_flag ? *a.now_f32_flag : 0) : 1;
    const int p32 = a.prev_f32 ? *a.prev_f32 : 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        double b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = a.now_f64 ? a.now_f64[(size_t)i * 4 + c] : (double)a.now_f32[(size_t)i * a.now_stride + c];
        for (int j = 0; j < np; ++j) {
            const double* p = a.prev + (size_t)j * 4;
            if (pf_box_iou(b, n32, p, p32) > a.iou_thres) {
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = pf_ema(a.alpha, b[c], n32, p[c], p32);
                if (!p32) s_mixed = 1;
                break;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) a.out[(size_t)i * 4 + c] = b[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) { *a.n_out = n; *a.out_f32 = (n32 && !s_mixed) ? 1 : 0; }
}

// sort_and_filter (facer.py:120-142): drop area <= min_face, keep the top_k largest (descending; equal areas: the
// later row first, the reversed ascending argsort of the reference).  Input: the judged rows on a detector frame, the
// slot's track_box otherwise; output: frame i's boxes_return and its dtype flag.
struct SelectArgs {
    TrackPoolView v;
    double min_face;
};

__device__ __forceinline__ double pf_box_area(const double* b, int f32) {
    return f32 ? (double)__fmul_rn(__fsub_rn((float)b[2], (float)b[0]), __fsub_rn((float)b[3], (float)b[1])) : (b[2] - b[0]) * (b[3] - b[1]);
}

__global__ __launch_bounds__(64) void track_select_kernel(SelectArgs g) {
    if (threadIdx.x != 0) return;
    const int i = blockIdx.x;
    const TrackFrameDesc d = g.v.desc[i];
    struct { const double* boxes; double* out; double min_face; int top_k; } a;
    const bool det = d.det >= 0;
    a.boxes = det ? g.v.judged + (size_t)i * kTrackMaxNow * 4 : g.v.track_box + (size_t)d.slot * kTrackMaxNow * 4;
    a.out = g.v.sel + (size_t)i * g.v.top_k * 4; a.min_face = g.min_face; a.top_k = g.v.top_k;
    const int n = det ? g.v.n_judged[i] : g.v.n_track[d.slot];
    const int f32 = g.v.f32[(size_t)d.slot * 4 + (det ? 1 : 0)];
    g.v.sel_f32[i] = f32;
    int npass = 0;
    for (int k = 0; k < n; ++k) npass += pf_box_area(a.boxes + (size_t)k * 4, f32) > a.min_face ? 1 : 0;
    int nsel = 0;
    if (npass <= a.top_k) {
        for (int k = 0; k < n; ++k) {
            const double* b = a.boxes + (size_t)k * 4;
            if (pf_box_area(b, f32) > a.min_face) {
                for (int c = 0; c < 4; ++c) a.out[nsel * 4 + c] = b[c];
                nsel++;
            }
        }
    } else {
        double last_area = 1.0e300;
        int last_k = -1;
        for (int s = 0; s < a.top_k; ++s) {
            double best = -1.0;
            int bk = -1;
            for (int k = n - 1; k >= 0; --k) {
                const double* b = a.boxes + (size_t)k * 4;
                const double ar = pf_box_area(b, f32);
                if (!(ar > a.min_face)) continue;
                if (ar > last_area || (ar == last_area && k >= last_k)) continue;
                if (ar > best) { best = ar; bk = k; }
            }
            if (bk < 0) break;
            for (int c = 0; c < 4; ++c) a.out[nsel * 4 + c] = a.boxes[(size_t)bk * 4 + c];
            nsel++;
            last_area = best;
            last_k = bk;
        }
    }
    g.v.n_sel[i] = nsel;
}

// GroupTrack.calculate (lk.py:19-56) + OneEuroFilter.__call__ (lk.py:117-149) + the hull boxes of facer.py:70-74.
// One workgroup per face slot (x) and frame (y); faces the crop stage rejected (params[slot][0] == 0) are dropped and the
// survivors compacted, like `landmarks[valid]` on the host.
struct GroupStageArgs {
    TrackPoolView v;
    const float* kps;         // [n][top_k][98][2] float32 landmarks of the call (frame coordinates)
    const float* scores_in;   // [n][top_k][98]
    const int* crop_params;   // [n][top_k][8]
    double iou_thres, scale_w, scale_h;
    double min_cutoff, beta, d_cutoff;
    const float* attrs_in;    // [n][top_k][16] face-attribute records of the landmark program (face_attrs=True), or nullptr
    float* attrs_out;         // [n][top_k][16] the records of the valid faces, compacted like the scores
};
struct GroupTrackArgs {       // the operands of one frame
    const float* kps;         // [top_k][98][2] float32 landmarks of this frame (frame coordinates)
    const float* scores_in;   // [top_k][98]
    const int* crop_params;   // [top_k][8], [0] = valid
    const int* n_sel;         // face slots in use this frame
    const double* prev_lm; const double* prev_dx; const int* n_prev; int prev_valid;
    const int* prev_f32;      // dtype flag of the previous landmark sets
    int* out_f32;             // dtype flag of the new sets: set to 1 before the launch, cleared by any face that was smoothed
    double* out_lm; double* out_dx; int* n_out;
    double* hull;             // [top_k][4]
    float* scores_out;        // [top_k][98]
    double iou_thres, scale_w, scale_h;
    double min_cutoff, beta, d_cutoff;
};

__device__ __forceinline__ void pf_hull_98(const double* pts, int tid, double* s_red, double* box) {
    // min / max over 98 points by the first 128 threads (s_red: 4 x 128 doubles)
    double mnx = 1.0e300, mny = 1.0e300, mxx = -1.0e300, mxy = -1.0e300;
    if (tid < 98) { mnx = mxx = pts[2 * tid]; mny = mxy = pts[2 * tid + 1]; }
    if (tid < 128) { s_red[tid] = mnx; s_red[128 + tid] = mny; s_red[256 + tid] = mxx; s_red[384 + tid] = mxy; }
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (tid < s) {
            s_red[tid] = fmin(s_red[tid], s_red[tid + s]);
            s_red[128 + tid] = fmin(s_red[128 + tid], s_red[128 + tid + s]);
            s_red[256 + tid] = fmax(s_red[256 + tid], s_red[256 + tid + s]);
            s_red[384 + tid] = fmax(s_red[384 + tid], s_red[384 + tid + s]);
        }
        __syncthreads();
    }
    box[0] = s_red[0]; box[1] = s_red[128]; box[2] = s_red[256]; box[3] = s_red[384];
    __syncthreads();
}

__global__ __launch_bounds__(128) void track_group_kernel(GroupStageArgs g) {
    __shared__ double s_red[512];
    __shared__ double s_now[196];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int i = blockIdx.y, K = g.v.top_k;
    const TrackFrameDesc d = g.v.desc[i];
    const int st = d.slot, nxt = d.cur ^ 1;
    GroupTrackArgs a{};
    a.kps = g.kps + (size_t)i * K * 196; a.scores_in = g.scores_in + (size_t)i * K * 98; a.crop_params = g.crop_params + (size_t)i * K * 8;
    a.n_sel = g.v.n_sel + i;
    a.prev_lm = g.v.slot_lm(g.v.lm, st, d.cur); a.prev_dx = g.v.slot_lm(g.v.dx, st, d.cur); a.n_prev = g.v.n_lm + (size_t)st * 2 + d.cur;
    a.prev_valid = d.lm_valid; a.prev_f32 = g.v.f32 + (size_t)st * 4 + 2 + d.cur; a.out_f32 = g.v.f32 + (size_t)st * 4 + 2 + nxt;
    a.out_lm = g.v.slot_lm(g.v.lm, st, nxt); a.out_dx = g.v.slot_lm(g.v.dx, st, nxt); a.n_out = g.v.n_lm + (size_t)st * 2 + nxt;
    a.hull = g.v.hull + (size_t)i * K * 4; a.scores_out = g.v.scores + (size_t)i * K * 98;
    a.iou_thres = g.iou_thres; a.scale_w = g.scale_w; a.scale_h = g.scale_h;
    a.min_cutoff = g.min_cutoff; a.beta = g.beta; a.d_cutoff = g.d_cutoff;
    const int nsel = *a.n_sel;
    if (slot >= nsel || a.crop_params[(size_t)slot * 8] == 0) return;      // uniform per workgroup
    int oi = 0;                                                            // output row = valid slots before this one
    for (int k = 0; k < slot; ++k) oi += a.crop_params[(size_t)k * 8] != 0 ? 1 : 0;
    for (int i = tid; i < 196; i += 128) s_now[i] = (double)a.kps[(size_t)slot * 196 + i];
    __syncthreads();
    double nbox[4];
    pf_hull_98(s_now, tid, s_red, nbox);
    int match = -1;
    if (a.prev_valid) {
        const int np = *a.n_prev;
        const int p32 = *a.prev_f32;
        for (int j = 0; j < np && match < 0; ++j) {
            double pbox[4];
            pf_hull_98(a.prev_lm + (size_t)j * 196, tid, s_red, pbox);
            if (pf_box_iou(nbox, 1, pbox, p32) > a.iou_thres) match = j;      // this frame's landmarks are float32
        }
    }
    if (match >= 0 && tid == 0) *a.out_f32 = 0;                 // `/ scale` made this set float64, hence the whole array
    const double two_pi = 2.0 * 3.141592653589793;
    if (tid < 98) {
        double rx = s_now[2 * tid], ry = s_now[2 * tid + 1], ddx = 0.0, ddy = 0.0;
        if (match >= 0) {
            const double* pl = a.prev_lm + (size_t)match * 196 + 2 * tid;
            const double* pd = a.prev_dx + (size_t)match * 196 + 2 * tid;
            const double x0 = rx / a.scale_w, x1 = ry / a.scale_h;               // now / scale
            const double p0 = pl[0] / a.scale_w, p1 = pl[1] / a.scale_h;         // previous / scale
            const double q0 = pd[0] / a.scale_w, q1 = pd[1] / a.scale_h;         // previous_dx / scale
            const double a_d = (two_pi * a.d_cutoff) / (two_pi * a.d_cutoff + 1.0);
            const double dx = sqrt((x0 - p0) * (x0 - p0) + (x1 - p1) * (x1 - p1));
            const double dxp = sqrt(q0 * q0 + q1 * q1);
            const double dx_hat = a_d * dx + (1.0 - a_d) * dxp;
            const double cutoff = a.min_cutoff + a.beta * fabs(dx_hat);
            double al = (two_pi * cutoff) / (two_pi * cutoff + 1.0);
            if (dx < 0.002) al = 0.01;
            const double f0 = (al * x0 + (1.0 - al) * p0) * a.scale_w;
            const double f1 = (al * x1 + (1.0 - al) * p1) * a.scale_h;
            ddx = pl[0] - f0; ddy = pl[1] - f1;                                  // previous - filtered (lk.py:45)
            rx = f0; ry = f1;
        }
        a.out_lm[(size_t)oi * 196 + 2 * tid] = rx;
        a.out_lm[(size_t)oi * 196 + 2 * tid + 1] = ry;
        a.out_dx[(size_t)oi * 196 + 2 * tid] = ddx;
        a.out_dx[(size_t)oi * 196 + 2 * tid + 1] = ddy;
        a.scores_out[(size_t)oi * 98 + tid] = a.scores_in[(size_t)slot * 98 + tid];
        if (g.attrs_in && tid < 16)
            g.attrs_out[((size_t)i * K + oi) * 16 + tid] = g.attrs_in[((size_t)i * K + slot) * 16 + tid];
        s_now[2 * tid] = rx;
        s_now[2 * tid + 1] = ry;
    }
    __syncthreads();
    double hb[4];
    pf_hull_98(s_now, tid, s_red, hb);
    if (tid < 4) a.hull[(size_t)oi * 4 + tid] = hb[tid];
}

// rows of the new landmark set = face slots the crop stage accepted; the new set's dtype flag starts at float32 (the
// network's landmarks) and track_group_kernel clears it when a face is smoothed against the previous ones.  One
// workgroup per frame, launched before track_group_kernel.
__global__ void track_count_kernel(TrackPoolView v, const int* crop_params) {
    if (threadIdx.x != 0) return;
    const int i = blockIdx.x;
    const TrackFrameDesc d = v.desc[i];
    const int nxt = d.cur ^ 1;
    int nv = 0;
    const int n = v.n_sel[i];
    for (int k = 0; k < n; ++k) nv += crop_params[((size_t)i * v.top_k + k) * 8] != 0 ? 1 : 0;
    v.n_lm[(size_t)d.slot * 2 + nxt] = nv;
    v.f32[(size_t)d.slot * 4 + 2 + nxt] = 1;
}

// results of frame i, gathered from its slot into call order: the count (<= top_k), the new track boxes and the new
// landmark sets (rows beyond the count are left as they are)
__global__ __launch_bounds__(256) void track_gather_kernel(TrackPoolView v) {
    const int i = blockIdx.x, K = v.top_k;
    const TrackFrameDesc d = v.desc[i];
    if (threadIdx.x == 0) v.out_count[i] = min(v.n_track[d.slot], K);
    const double* tb = v.track_box + (size_t)d.slot * kTrackMaxNow * 4;
    for (int k = threadIdx.x; k < K * 4; k += 256) v.out_box[(size_t)i * K * 4 + k] = tb[k];
    const double* lm = v.slot_lm(v.lm, d.slot, d.cur ^ 1);
    for (int k = threadIdx.x; k < K * 196; k += 256) v.out_lm[(size_t)i * K * 196 + k] = lm[k];
}

// Frame-difference gate of a pf_track_streams call, fused with the store of the frame (facer.py:98-118): workgroup row y =
// frame i.  Every 16-byte word of the current frame is read, compared with the slot's previous frame when that one is
// comparable (desc.cmp), and then written over it, so the slot holds this frame for the next call.  Each word is read
// before the same lane overwrites it, and the frames of one call go to distinct slots.  The sum of |cur - prev| is exact:
// a lane adds at most 16 * 255 per word over at most PF_GATE_MAX_WORDS words (the host sizes the grid for that), the
// workgroup adds its 256 lane sums in 64 bits and one 64-bit atomic per workgroup folds them into sums[i].
#define PF_GATE_MAX_WORDS 65536      // words per lane: 65536 * 16 * 255 < 2^32
struct GateArgs {
    const unsigned char* cur;    // [n][bytes] frames of the call
    unsigned char* prev;         // [S][slot_bytes] previous frame of every slot
    size_t bytes, slot_bytes;
    const TrackFrameDesc* desc;  // [n]
    unsigned long long* sums;    // [n], zeroed before the launch
    int vec;                     // 1: bytes, both bases and slot_bytes are multiples of 16 (uint4 path)
};

__global__ __launch_bounds__(256) void track_gate_kernel(GateArgs a) {
    __shared__ unsigned long long s_part[256];
    const int i = blockIdx.y;
    const TrackFrameDesc d = a.desc[i];
    const unsigned char* c = a.cur + (size_t)i * a.bytes;
    unsigned char* p = a.prev + (size_t)d.slot * a.slot_bytes;
    const bool cmp = d.cmp != 0;
    const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int acc = 0;
    size_t done = 0;
    if (a.vec) {
        const size_t nvec = a.bytes / 16;
        for (size_t k = t0; k < nvec; k += stride) {
            const uint4 x = *reinterpret_cast<const uint4*>(c + k * 16);
            if (cmp) {
                const uint4 y = *reinterpret_cast<const uint4*>(p + k * 16);
                const unsigned int xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int df = (int)((xs[w] >> (8 * b)) & 0xFF) - (int)((ys[w] >> (8 * b)) & 0xFF);
                        acc += (unsigned int)(df < 0 ? -df : df);
                    }
            }
            *reinterpret_cast<uint4*>(p + k * 16) = x;
        }
        done = nvec * 16;
    }
    for (size_t k = done + t0; k < a.bytes; k += stride) {      // byte path: unaligned frames, or none at all of it
        const unsigned char x = c[k];
        if (cmp) { const int df = (int)x - (int)p[k]; acc += (unsigned int)(df < 0 ? -df : df); }
        p[k] = x;
    }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) s_part[threadIdx.x] += s_part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0 && cmp && s_part[0]) atomicAdd(a.sums + i, s_part[0]);
}

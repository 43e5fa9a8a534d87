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
const int kTrackMaxLost = 64;    // entries of a stream's lost list (persistent ids); also the most faces per frame ids are kept for

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
    // ---- persistent face ids (pf_track_ids_config; the rule: include/peppa_hip.h).  State of slot s, rows at stride K:
    int* id;             // [S][K] id of row r of track_box (0 = no id)
    int* age;            // [S][K] frames that id has been seen
    int* next_id;        // [S] ids handed out so far: the next fresh id is next_id + 1, never reused while the pool lives
    int* lost_n;         // [S] entries of the lost list, in insertion order:
    int* lost_id;        // [S][kTrackMaxLost]
    int* lost_age;       // [S][kTrackMaxLost]
    int* lost_gone;      // [S][kTrackMaxLost] frames the id has been absent
    double* lost_box;    // [S][kTrackMaxLost][4] its last track box
    // scratch of frame i: the provenance the stages record (written only while ids are on) and the ids in call order
    int* match_j;        // [S][kTrackMaxNow] previous row a judged row was smoothed with, -1: none (track_judge_kernel)
    double* match_w;     // [S][kTrackMaxNow] the IoU of that match
    int* sel_src;        // [S][K] judged row (detector frame) or track row (gated frame) of every selected row (track_select_kernel)
    double* prev_box;    // [S][K][4] track_box as it was before this frame, captured by track_select_kernel
    int* prev_n;         // [S] rows of it (0 without a track)
    int* out_id;         // [S][K] ids of frame i's rows at stride top_k, 0 beyond its count
    int* out_age;        // [S][K]
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
    std::vector<int> h_ids;                // host copies of out_id / out_age of the last call (pf_track_ids)
    void release() {
        void* ptrs[] = {v.track_box, v.n_track, v.lm, v.dx, v.n_lm, v.f32, v.judged, v.n_judged, v.sel, v.n_sel, v.sel_f32,
                        v.hull, v.scores, v.out_count, v.out_box, v.out_lm, d_desc, d_frames, d_sums, d_det_idx,
                        v.id, v.age, v.next_id, v.lost_n, v.lost_id, v.lost_age, v.lost_gone, v.lost_box, v.match_j, v.match_w,
                        v.sel_src, v.prev_box, v.prev_n, v.out_id, v.out_age};
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
    int* match_j; double* match_w;     // persistent ids on, detections stage: TrackPoolView::match_j / match_w; nullptr otherwise
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
        int mj = -1;
        double mw = 0.0;
        for (int j = 0; j < np; ++j) {
            const double* p = a.prev + (size_t)j * 4;
            const double iou = pf_box_iou(b, n32, p, p32);
            if (iou > a.iou_thres) {
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = pf_ema(a.alpha, b[c], n32, p[c], p32);
                if (!p32) s_mixed = 1;
                mj = j; mw = iou;
                break;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) a.out[(size_t)i * 4 + c] = b[c];
        if (g.match_j) { g.match_j[(size_t)f * kTrackMaxNow + i] = mj; g.match_w[(size_t)f * kTrackMaxNow + i] = mw; }
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
    int ids;             // persistent ids on: record TrackPoolView::sel_src and capture prev_box / prev_n
};

__device__ __forceinline__ double pf_box_area(const double* b, int f32) {
    return f32 ? (double)__fmul_rn(__fsub_rn((float)b[2], (float)b[0]), __fsub_rn((float)b[3], (float)b[1])) : (b[2] - b[0]) * (b[3] - b[1]);
}

__global__ __launch_bounds__(64) void track_select_kernel(SelectArgs g) {
    const int i = blockIdx.x;
    const TrackFrameDesc d = g.v.desc[i];
    if (g.ids) {         // the previous track boxes, before the hull judge of this frame overwrites them (track_ident_kernel)
        const int np = d.has_track ? min(g.v.n_track[d.slot], g.v.K) : 0;
        const double* tb = g.v.track_box + (size_t)d.slot * kTrackMaxNow * 4;
        for (int k = threadIdx.x; k < np * 4; k += 64) g.v.prev_box[(size_t)i * g.v.K * 4 + k] = tb[k];
        if (threadIdx.x == 0) g.v.prev_n[i] = np;
    }
    if (threadIdx.x != 0) return;
    int* src = g.ids ? g.v.sel_src + (size_t)i * g.v.top_k : nullptr;
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
                if (src) src[nsel] = k;
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
            if (src) src[nsel] = bk;
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

// pf_box_iou_f64 with contraction switched off in the source: the lost-list comparison of the identity rule is restated in numpy
// (core/smoother/ident.py), which never fuses a multiply into an add
__device__ __forceinline__ double pf_box_iou_f64_strict(const double* a, const double* b) {
#pragma clang fp contract(off)
    const double s1 = (a[2] - a[0]) * (a[3] - a[1]);
    const double s2 = (b[2] - b[0]) * (b[3] - b[1]);
    const double x1 = fmax(a[0], b[0]), y1 = fmax(a[1], b[1]);
    const double x2 = fmin(a[2], b[2]), y2 = fmin(a[3], b[3]);
    const double inter = fmax(0.0, x2 - x1) * fmax(0.0, y2 - y1);
    const double sum = s1 + s2;
    return inter / (sum - inter);
}

// Persistent face ids: steps 1-6 of the identity rule (include/peppa_hip.h, "Persistent face ids") for frame i = blockIdx.x of the
// call, one workgroup per frame like its neighbours.  ORDERING: one launch, BEHIND the hull judge, because step 5 compares the NEW
// track boxes with the lost list; the PREVIOUS boxes that step 6 appends for rows that lose their id were captured in front of that
// launch by track_select_kernel (prev_box / prev_n), together with the provenance of the selected rows (sel_src) and, on a detector
// frame, of the judged rows (match_j / match_w, track_judge_kernel).  Everything is staged into LDS by all lanes, the IoU matrix
// output rows x lost entries is filled by all lanes, then lane 0 resolves the conflicts, the claims and the list serially (at most
// kTrackMaxLost rows against at most kTrackMaxLost entries, all in LDS) and all lanes write the state and the call-order ids back.
// No atomics, no global scratch beyond the pool's arrays.  A slot without a track (first frame, after a reset) starts with no rows
// and an empty list, which is how the resets forget ids without touching the device; next_id is left alone by them.
struct IdentArgs {
    TrackPoolView v;
    const int* crop_params;   // [n][top_k][8], [0] = the landmark stage accepted the selected row
    double iou_thres;
    int keep_lost;            // 0 .. 255
};

__global__ __launch_bounds__(256) void track_ident_kernel(IdentArgs g) {
    const int L = kTrackMaxLost;
    __shared__ double s_iou[L * L];            // [output row][lost entry]
    __shared__ double s_nbox[L * 4];           // new track boxes
    __shared__ double s_lbox[2 * L * 4];       // lost boxes; the second half takes this frame's appends before the list is cut to L
    __shared__ double s_w[L];
    __shared__ int s_src[L], s_keeper[L], s_pid[L], s_page[L], s_id[L], s_age[L], s_claimed[L];
    __shared__ int s_lid[2 * L], s_lage[2 * L], s_lgone[2 * L];
    __shared__ int s_nl;
    const int i = blockIdx.x, tid = threadIdx.x, K = g.v.top_k, KP = g.v.K;
    const TrackFrameDesc d = g.v.desc[i];
    const int s = d.slot;
    const bool det = d.det >= 0;
    const int n_prev = d.has_track ? min(g.v.prev_n[i], L) : 0;
    const int n_lost = (d.has_track && g.keep_lost > 0) ? min(g.v.lost_n[s], L) : 0;
    const int n_sel = min(g.v.n_sel[i], min(K, L));
    const int n_out = min(min(g.v.n_track[s], K), L);          // rows of the new track_box == output rows
    const double* tb = g.v.track_box + (size_t)s * kTrackMaxNow * 4;
    // ---- stage: previous ids, the lost list, the new boxes, source and weight of every output row (steps 1, 2)
    if (tid < L) {
        s_pid[tid] = tid < n_prev ? g.v.id[(size_t)s * KP + tid] : 0;
        s_page[tid] = tid < n_prev ? g.v.age[(size_t)s * KP + tid] : 0;
        s_claimed[tid] = 0;
        s_src[tid] = -1;
        s_w[tid] = 0.0;
        if (tid < n_lost) {
            s_lid[tid] = g.v.lost_id[(size_t)s * L + tid];
            s_lage[tid] = g.v.lost_age[(size_t)s * L + tid];
            s_lgone[tid] = g.v.lost_gone[(size_t)s * L + tid];
        }
    }
    for (int k = tid; k < n_lost * 4; k += 256) s_lbox[k] = g.v.lost_box[(size_t)s * L * 4 + k];
    for (int k = tid; k < n_out * 4; k += 256) s_nbox[k] = tb[k];
    __syncthreads();
    if (tid < n_sel && g.crop_params[((size_t)i * K + tid) * 8] != 0) {
        int o = 0;                                              // output row = accepted selected rows before this one
        for (int k = 0; k < tid; ++k) o += g.crop_params[((size_t)i * K + k) * 8] != 0 ? 1 : 0;
        const int r = g.v.sel_src[(size_t)i * K + tid];
        int j = det ? g.v.match_j[(size_t)i * kTrackMaxNow + r] : r;
        const double w = det ? g.v.match_w[(size_t)i * kTrackMaxNow + r] : 0.0;
        if (j >= n_prev || (j >= 0 && s_pid[j] == 0)) j = -1;   // a row without an id passes on no source
        if (o < L) { s_src[o] = j; s_w[o] = j >= 0 ? w : 0.0; }
    }
    // ---- IoU of every output row with every lost entry
    for (int k = tid; k < n_out * n_lost; k += 256) {
        const int o = k / n_lost, e = k - o * n_lost;
        s_iou[o * L + e] = pf_box_iou_f64_strict(s_nbox + o * 4, s_lbox + e * 4);
    }
    __syncthreads();
    if (tid == 0) {
        // step 3: the greatest weight keeps a contested source, the lowest output row on equal weights
        for (int j = 0; j < n_prev; ++j) s_keeper[j] = -1;
        for (int o = 0; o < n_out; ++o) {
            const int j = s_src[o];
            if (j >= 0 && (s_keeper[j] < 0 || s_w[o] > s_w[s_keeper[j]])) s_keeper[j] = o;
        }
        // steps 4, 5
        int next = g.v.next_id[s];
        for (int o = 0; o < n_out; ++o) {
            const int j = s_src[o];
            if (j >= 0 && s_keeper[j] == o) { s_id[o] = s_pid[j]; s_age[o] = s_page[j] + 1; continue; }
            int best = -1;
            double bw = g.iou_thres;
            for (int e = 0; e < n_lost; ++e)
                if (!s_claimed[e] && s_iou[o * L + e] > bw) { best = e; bw = s_iou[o * L + e]; }
            if (best >= 0) { s_id[o] = s_lid[best]; s_age[o] = s_lage[best] + 1; s_claimed[best] = 1; }
            else { s_id[o] = ++next; s_age[o] = 1; }
        }
        g.v.next_id[s] = next;
        // step 6
        int m = 0;
        for (int e = 0; e < n_lost; ++e) {
            if (s_claimed[e] || s_lgone[e] + 1 > g.keep_lost) continue;
            s_lid[m] = s_lid[e]; s_lage[m] = s_lage[e]; s_lgone[m] = s_lgone[e] + 1;
            for (int c = 0; c < 4; ++c) s_lbox[m * 4 + c] = s_lbox[e * 4 + c];
            ++m;
        }
        if (g.keep_lost > 0)
            for (int j = 0; j < n_prev; ++j) {
                if (s_pid[j] == 0 || s_keeper[j] >= 0) continue;
                s_lid[m] = s_pid[j]; s_lage[m] = s_page[j]; s_lgone[m] = 1;
                for (int c = 0; c < 4; ++c) s_lbox[m * 4 + c] = g.v.prev_box[((size_t)i * KP + j) * 4 + c];
                ++m;
            }
        while (m > L) {                                         // the longest gone goes, the earliest inserted among equals
            int worst = 0;
            for (int e = 1; e < m; ++e) if (s_lgone[e] > s_lgone[worst]) worst = e;
            for (int e = worst; e + 1 < m; ++e) {
                s_lid[e] = s_lid[e + 1]; s_lage[e] = s_lage[e + 1]; s_lgone[e] = s_lgone[e + 1];
                for (int c = 0; c < 4; ++c) s_lbox[e * 4 + c] = s_lbox[(e + 1) * 4 + c];
            }
            --m;
        }
        s_nl = m;
    }
    __syncthreads();
    // ---- the slot's state and the ids of frame i in call order
    const int m = s_nl;
    if (tid == 0) g.v.lost_n[s] = m;
    if (tid < m) {
        g.v.lost_id[(size_t)s * L + tid] = s_lid[tid];
        g.v.lost_age[(size_t)s * L + tid] = s_lage[tid];
        g.v.lost_gone[(size_t)s * L + tid] = s_lgone[tid];
    }
    for (int k = tid; k < m * 4; k += 256) g.v.lost_box[(size_t)s * L * 4 + k] = s_lbox[k];
    for (int k = tid; k < KP; k += 256) {
        g.v.id[(size_t)s * KP + k] = k < n_out ? s_id[k] : 0;
        g.v.age[(size_t)s * KP + k] = k < n_out ? s_age[k] : 0;
    }
    for (int k = tid; k < K; k += 256) {
        g.v.out_id[(size_t)i * K + k] = k < n_out ? s_id[k] : 0;
        g.v.out_age[(size_t)i * K + k] = k < n_out ? s_age[k] : 0;
    }
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

// What a handle's last call left on the device for the stages behind the landmarks: ONE record (pf_handle::last), read by pf_face_chips,
// pf_face_masks, pf_face_masks_shape, pf_face_redact, pf_face_stats (the rows with their frames; checked reader: last_face_rows, face_rows.inl) and by
// pf_face_attrs (the attribute rows), and written through its own functions and nowhere else:
//   forget()          everything the record points at is about to be replaced: the pipeline and tracking calls on entry,
//                     pf_load_program of the landmark slot, every lane of a pf_batch_run_frames
//   forget_frames()   the frame, landmarks or crop parameters of the rows are about to be overwritten, the attribute records are not
//   note_frameless()  pf_landmark_forward: rows without a frame (the accessors say so); its attribute rows follow
//   note_frames()     rows [F][per_frame] and the frame each group of per_frame rows is read from, ready-made
//   note_attrs()      attribute rows of kind 1, 2 or 3 (below)
//   note_ids()        persistent ids and ages of the rows (the tracking calls while pf_track_ids_config has them on; pf_track_ids)
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "k_align.h"

struct FaceRows {
    // kind 0 = the last call left no rows, 1 = rows 0 .. rows-1, row r in frame r / per_frame, 2 = rows without a frame (pf_landmark_forward)
    int kind = 0, rows = 0, per_frame = 1, kps_f64 = 0, valid_stride = 0;
    const void* kps = nullptr;
    const int* counts = nullptr;
    const int* valid = nullptr;
    std::vector<AlignFrame> frames;
    // rows of face-attribute records the last landmark-running call left (pf_face_attrs): attr_kind 0 = none, 1 = rows 0 .. attr_rows-1 of
    // the landmark program's out_buf2 as they are (pf_landmark_forward, pf_run_frames*), 2 = the same with the valid flags of
    // pf_landmarks (snapshot in h_attr_valid / d_attr_valid, taken by that call: face_rows_snapshot_valid), 3 = rows of attr_src (the
    // tracking calls: records compacted like their scores by track_group_kernel into d_track_attrs)
    int attr_kind = 0, attr_rows = 0;
    const float* attr_src = nullptr;
    std::vector<int> h_attr_valid;
    int* d_attr_valid = nullptr; size_t attr_valid_bytes = 0;
    // persistent ids / ages of the rows (the tracker pool's out_id / out_age and the host copies the call brought back), or nullptr
    const int* ids = nullptr; const int* ages = nullptr;
    const int* h_ids = nullptr; const int* h_ages = nullptr;

    void forget() { kind = 0; attr_kind = 0; ids = ages = h_ids = h_ages = nullptr; }
    void forget_frames() { kind = 0; ids = ages = h_ids = h_ages = nullptr; }
    void note_frameless() { kind = 2; attr_kind = 0; }
    void note_frames(std::vector<AlignFrame> table, int n_rows, int rows_per_frame, const void* d_kps, int f64, const int* d_counts,
                     const int* d_valid = nullptr, int stride = 0) {
        frames = std::move(table);
        kind = 1; rows = n_rows; per_frame = std::max(rows_per_frame, 1); kps = d_kps; kps_f64 = f64;
        counts = d_counts; valid = d_valid; valid_stride = stride;
    }
    void note_attrs(int k, int n_rows, const float* src = nullptr) { attr_kind = k; attr_rows = n_rows; attr_src = src; }
    void note_ids(const int* d_ids, const int* d_ages, const int* host_ids, const int* host_ages) {
        ids = d_ids; ages = d_ages; h_ids = host_ids; h_ages = host_ages;
    }
    void release() {
        if (d_attr_valid) (void)hipFree(d_attr_valid);
        *this = FaceRows();
    }
};

// F frames of one size, `frame_stride` bytes apart (0: every group of rows reads the same frame)
inline std::vector<AlignFrame> face_frames(const unsigned char* base, size_t frame_stride, int F, int H, int W, int row_stride) {
    std::vector<AlignFrame> t(F);
    for (int f = 0; f < F; ++f) t[f] = AlignFrame{base + (size_t)f * frame_stride, H, W, row_stride, 0};
    return t;
}

// host frames / landmarks / counts of the stage-level entry points, uploaded by stage_faces
struct StageUpload {
    unsigned char* d_frames = nullptr; size_t frames_bytes = 0;
    char* d_kps = nullptr; size_t kps_bytes = 0;
    int* d_counts = nullptr; size_t counts_bytes = 0;
    void release() {
        void* ptrs[] = {d_frames, d_kps, d_counts};
        for (void* p : ptrs) if (p) (void)hipFree(p);
        *this = StageUpload();
    }
};

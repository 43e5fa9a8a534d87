// What align.inl, mask.inl and redact.inl share, next to the record of the last call (FaceRows, face_rows.h): the allocator of their
// scratch, the record's checked reader, the prologue of the stage-level entry points and the copy of valid rows to the host.
namespace {

// scratch of the stages behind the landmarks only: never referenced by a captured graph, so the graph cache is not told
template <typename T>
int scratch_ensure(pf_handle* h, T*& ptr, size_t& have_bytes, size_t need_bytes) {
    if (need_bytes <= have_bytes && ptr) return 0;
    if (ptr) { (void)hipStreamSynchronize(h->stream); (void)hipFree(ptr); }
    ptr = nullptr; have_bytes = 0;
    PF_HIP(h, hipMalloc((void**)&ptr, need_bytes));
    have_bytes = need_bytes;
    return 0;
}

bool face_out_mem_ok(int m) { return m == PF_MEM_HOST || m == PF_MEM_DEVICE || m == PF_MEM_HOST_PINNED; }

// pf_landmarks: the valid flags of THIS call (word 0 of each row's `stride` ints), kept apart from the crop-parameter scratch the
// next call overwrites.  Tells the graph cache when it grows, like the pipeline scratch it is taken from (by hand: ensure_dev, which
// does both, is defined behind this file, in pipeline.inl).
int face_rows_snapshot_valid(pf_handle* h, const int* flags, int stride, int n) {
    FaceRows& s = h->last;
    s.h_attr_valid.resize(n);
    for (int i = 0; i < n; ++i) s.h_attr_valid[i] = flags[(size_t)i * stride] != 0;
    const size_t need = (size_t)n * sizeof(int);
    if ((need > s.attr_valid_bytes || !s.d_attr_valid) && h->graphs.note_realloc(h->err)) return 1;
    if (scratch_ensure(h, s.d_attr_valid, s.attr_valid_bytes, need)) return 1;
    PF_HIP(h, hipMemcpy(s.d_attr_valid, s.h_attr_valid.data(), need, hipMemcpyHostToDevice));
    return 0;
}

// The record of the last call for an accessor that needs `rows` rows AND their frames, or its refusal.  `no_frame` is the clause
// that differs: what the accessor would have done with the frame pf_landmark_forward does not have.
int last_face_rows(pf_handle* h, const char* who, const char* no_frame, int rows, const FaceRows** out) {
    const FaceRows& s = h->last;
    if (s.kind == 2) PF_FAIL(h, "%s: the handle's last call was pf_landmark_forward, which has %s", who, no_frame);
    if (s.kind == 0)
        PF_FAIL(h, "%s: the handle's last call left no face rows (pf_landmarks*, pf_run_frames*, pf_track_frame* and pf_track_streams do)", who);
    if (rows > s.rows) PF_FAIL(h, "%s: %d rows asked, the last call left %d", who, rows, s.rows);
    *out = &s;
    return 0;
}

// what stage_faces yields: device pointers, the rows, and the frame each group of top_k rows reads (empty without frames)
struct StageFaces {
    int rows = 0;
    const void* d_kps = nullptr;
    const int* d_counts = nullptr;
    std::vector<AlignFrame> frames;
};

// The prologue of pf_align_faces / pf_mask_faces / pf_redact_faces, behind the checks that belong to one stage: shared argument checks
// (`out`: the stage's one mandatory output), the 2^20-slot limit, PF_MEM_RESIDENT, upload of host frames, landmarks and counts, the
// frame table.  want_frames = false (pf_mask_faces reads no pixel): frames, mem, height and width are not looked at.
int stage_faces(pf_handle* h, const char* who, bool want_frames, const uint8_t* frames, int mem, int n_frames, int height, int width,
                const void* kps, int kps_f64, int kps_mem, const int* counts, int top_k, const void* out, int out_mem, StageFaces* st) {
    if (n_frames < 1 || top_k < 1 || !kps || !out || (kps_mem != PF_MEM_HOST && kps_mem != PF_MEM_DEVICE) || !face_out_mem_ok(out_mem) ||
        (want_frames && (height < 1 || width < 1 || height > 32768 || width > 32768 || (!frames && mem != PF_MEM_RESIDENT) ||
                         (mem != PF_MEM_HOST && mem != PF_MEM_DEVICE && mem != PF_MEM_RESIDENT))))
        PF_FAIL(h, "%s: bad arguments", who);
    if ((long long)n_frames * top_k > (1 << 20)) PF_FAIL(h, "%s: %d x %d face slots are too many", who, n_frames, top_k);
    StageUpload& s = h->upload;
    const size_t frame_bytes = (size_t)height * width * 3;
    const unsigned char* d_frames = frames;
    if (want_frames && mem == PF_MEM_RESIDENT) {
        if (n_frames != 1) PF_FAIL(h, "%s: PF_MEM_RESIDENT is one frame, n_frames = %d", who, n_frames);
        if (!h->pipe.have_cur || h->pipe.cur_h != height || h->pipe.cur_w != width)
            PF_FAIL(h, "%s: no resident frame of this size (call pf_set_frame first)", who);
        d_frames = h->pipe.d_cur;
    }
    PF_HIP(h, hipSetDevice(h->device));
    st->rows = n_frames * top_k;
    if (want_frames && mem == PF_MEM_HOST) {
        if (scratch_ensure(h, s.d_frames, s.frames_bytes, (size_t)n_frames * frame_bytes)) return 1;
        PF_HIP(h, hipMemcpyAsync(s.d_frames, frames, (size_t)n_frames * frame_bytes, hipMemcpyHostToDevice, h->stream));
        d_frames = s.d_frames;
    }
    st->d_kps = kps;
    st->d_counts = counts;
    if (kps_mem == PF_MEM_HOST) {
        const size_t kb = (size_t)st->rows * 196 * (kps_f64 ? sizeof(double) : sizeof(float));
        if (scratch_ensure(h, s.d_kps, s.kps_bytes, kb)) return 1;
        PF_HIP(h, hipMemcpyAsync(s.d_kps, kps, kb, hipMemcpyHostToDevice, h->stream));
        st->d_kps = s.d_kps;
        if (counts) {
            if (scratch_ensure(h, s.d_counts, s.counts_bytes, (size_t)n_frames * sizeof(int))) return 1;
            PF_HIP(h, hipMemcpyAsync(s.d_counts, counts, (size_t)n_frames * sizeof(int), hipMemcpyHostToDevice, h->stream));
            st->d_counts = s.d_counts;
        }
    }
    if (want_frames) st->frames = face_frames(d_frames, frame_bytes, n_frames, height, width, width * 3);
    return 0;
}

// Host outputs whose rows of invalid slots stay untouched: runs of valid rows come over in one copy each, straight into the
// caller's arrays, for up to two arrays (dst == nullptr: none); one synchronisation behind them.
struct RowCopy { void* dst; const void* src; size_t row_bytes; };
int copy_valid_runs(pf_handle* h, const std::vector<int>& h_valid, int rows, RowCopy a, RowCopy b = RowCopy{nullptr, nullptr, 0}) {
    for (int r = 0; r < rows;) {
        if (!h_valid[r]) { ++r; continue; }
        int e = r + 1;
        while (e < rows && h_valid[e]) ++e;
        for (const RowCopy& c : {a, b})
            if (c.dst) PF_HIP(h, hipMemcpyAsync((char*)c.dst + (size_t)r * c.row_bytes, (const char*)c.src + (size_t)r * c.row_bytes,
                                                (size_t)(e - r) * c.row_bytes, hipMemcpyDeviceToHost, h->stream));
        r = e;
    }
    PF_HIP(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

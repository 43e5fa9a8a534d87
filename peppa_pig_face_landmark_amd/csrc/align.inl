// Aligned face chips (included at the end of engine.cpp; kernels in k_align.h):
//   pf_align_faces        stage-level: the caller supplies frames and landmarks
//   pf_face_chips         the faces of the handle's last pipeline call, from the frame(s) and landmarks it left on the device
//   pf_batch_face_chips   the same over the lanes of a pf_batch
// Every pipeline entry point records what it left with chips_note_* (next to its attr_kind bookkeeping).
namespace {

// scratch of this file only: never referenced by a captured graph, so the graph cache is not told
template <typename T>
int align_ensure(pf_handle* h, T*& ptr, size_t& have_bytes, size_t need_bytes) {
    if (need_bytes <= have_bytes && ptr) return 0;
    if (ptr) { (void)hipStreamSynchronize(h->stream); (void)hipFree(ptr); }
    ptr = nullptr; have_bytes = 0;
    PF_HIP(h, hipMalloc((void**)&ptr, need_bytes));
    have_bytes = need_bytes;
    return 0;
}

const char* align_check_size(int S) {
    return (S < 32 || S > 256 || (S % 16) != 0) ? "chip_size must be a multiple of 16 in [32, 256]" : nullptr;
}

bool align_out_mem_ok(int m) { return m == PF_MEM_HOST || m == PF_MEM_DEVICE || m == PF_MEM_HOST_PINNED; }

// Fit + warp of `rows` slots; row r reads frame groups[r / per_frame].  d_kps / d_counts / d_valid_in are device pointers.  Outputs in
// device memory are written by the kernels themselves (dead and degenerate slots untouched); host outputs are produced in the
// handle's scratch, copied, synchronised and the rows of valid slots handed over.
int align_run(pf_handle* h, int rows, int S, const AlignFrame* groups, int per_frame, const void* d_kps, int kps_f64,
              const int* d_counts, const int* d_valid_in, int valid_stride, uint8_t* chips, double* mats, int* valid, int out_mem) {
    AlignState& s = h->align;
    const size_t chip_bytes = (size_t)S * S * 3;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    if (align_ensure(h, s.d_table, s.table_bytes, (size_t)rows * sizeof(AlignFrame))) return 1;
    if (align_ensure(h, s.d_rec, s.rec_bytes, (size_t)rows * PF_ALIGN_REC * sizeof(double))) return 1;
    if (align_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
    if (!to_device) {
        if (align_ensure(h, s.d_chips, s.chips_bytes, (size_t)rows * chip_bytes)) return 1;
        if (mats && align_ensure(h, s.d_mats, s.mats_bytes, (size_t)rows * 6 * sizeof(double))) return 1;
    }
    s.h_table.resize(rows);
    for (int r = 0; r < rows; ++r) s.h_table[r] = groups[r / per_frame];
    PF_HIP(h, hipMemcpyAsync(s.d_table, s.h_table.data(), (size_t)rows * sizeof(AlignFrame), hipMemcpyHostToDevice, h->stream));
    AlignFitArgs fa{};
    fa.kps = d_kps; fa.kps_f64 = kps_f64; fa.n = rows; fa.per_frame = per_frame; fa.S = S;
    fa.counts = d_counts; fa.valid_in = d_valid_in; fa.valid_stride = valid_stride;
    fa.rec = s.d_rec; fa.valid = s.d_valid;
    fa.mats_out = to_device ? mats : (mats ? s.d_mats : nullptr);
    fa.valid_out = to_device ? valid : nullptr;
    {
        ProfScope ps(h, "align_fit");
        PF_LAUNCH(align_fit_kernel, dim3(pf_div_up(rows, 64)), dim3(64), h->stream, fa);
    }
    AlignWarpArgs wa{};
    wa.frames = s.d_table; wa.rec = s.d_rec; wa.valid = s.d_valid;
    wa.chips = to_device ? chips : s.d_chips;
    wa.n = rows; wa.S = S;
    wa.lds_budget = std::min(std::max(s.lds_budget, 0), PF_ALIGN_LDS_BYTES);
    wa.out_aligned = ((size_t)wa.chips & 3) == 0 ? 1 : 0;
    {
        ProfScope ps(h, "align_warp");
        PF_LAUNCH(align_warp_kernel, dim3((S / PF_ALIGN_TILE) * (S / PF_ALIGN_TILE), rows), dim3(256), h->stream, wa);
    }
    PF_HIP(h, hipGetLastError());
    if (to_device) return 0;
    s.h_valid.resize(rows);
    PF_HIP(h, hipMemcpyAsync(s.h_valid.data(), s.d_valid, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipStreamSynchronize(h->stream));
    // runs of valid rows come over in one copy each, straight into the caller's arrays
    for (int r = 0; r < rows;) {
        if (!s.h_valid[r]) { ++r; continue; }
        int e = r + 1;
        while (e < rows && s.h_valid[e]) ++e;
        PF_HIP(h, hipMemcpyAsync(chips + (size_t)r * chip_bytes, s.d_chips + (size_t)r * chip_bytes, (size_t)(e - r) * chip_bytes,
                                 hipMemcpyDeviceToHost, h->stream));
        if (mats) PF_HIP(h, hipMemcpyAsync(mats + (size_t)r * 6, s.d_mats + (size_t)r * 6, (size_t)(e - r) * 6 * sizeof(double),
                                           hipMemcpyDeviceToHost, h->stream));
        r = e;
    }
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

}  // namespace

// what a pipeline call left for pf_face_chips: F frames of one size `frame_stride` bytes apart, rows [F][per_frame]
static void chips_note_frames(pf_handle* h, const unsigned char* base, size_t frame_stride, int F, int H, int W, int row_stride,
                              int rows, int per_frame, const void* d_kps, int kps_f64, const int* d_counts,
                              const int* d_valid = nullptr, int valid_stride = 0) {
    AlignState& s = h->align;
    s.frames.resize(F);
    for (int f = 0; f < F; ++f) s.frames[f] = AlignFrame{base + (size_t)f * frame_stride, H, W, row_stride, 0};
    s.kind = 1; s.rows = rows; s.per_frame = std::max(per_frame, 1); s.kps = d_kps; s.kps_f64 = kps_f64;
    s.counts = d_counts; s.valid = d_valid; s.valid_stride = valid_stride;
}

extern "C" {

int pf_align_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                   const void* kps, int kps_f64, int kps_mem, const int* counts, int top_k, int chip_size,
                   uint8_t* chips, double* mats, int* valid, int out_mem) {
    if (!h) return 1;
    if (const char* why = align_check_size(chip_size)) PF_FAIL(h, "pf_align_faces: %s (got %d)", why, chip_size);
    if (n_frames < 1 || height < 1 || width < 1 || height > 32768 || width > 32768 || top_k < 1 || !kps || !chips ||
        (mem != PF_MEM_HOST && mem != PF_MEM_DEVICE && mem != PF_MEM_RESIDENT) || (kps_mem != PF_MEM_HOST && kps_mem != PF_MEM_DEVICE) ||
        !align_out_mem_ok(out_mem) || (!frames && mem != PF_MEM_RESIDENT))
        PF_FAIL(h, "pf_align_faces: bad arguments");
    if ((long long)n_frames * top_k > (1 << 20)) PF_FAIL(h, "pf_align_faces: %d x %d face slots are too many", n_frames, top_k);
    AlignState& s = h->align;
    const size_t frame_bytes = (size_t)height * width * 3;
    const unsigned char* d_frames = frames;
    if (mem == PF_MEM_RESIDENT) {
        if (n_frames != 1) PF_FAIL(h, "pf_align_faces: PF_MEM_RESIDENT is one frame, n_frames = %d", n_frames);
        if (!h->pipe.have_cur || h->pipe.cur_h != height || h->pipe.cur_w != width)
            PF_FAIL(h, "pf_align_faces: no resident frame of this size (call pf_set_frame first)");
        d_frames = h->pipe.d_cur;
    }
    PF_HIP(h, hipSetDevice(h->device));
    const int rows = n_frames * top_k;
    if (mem == PF_MEM_HOST) {
        if (align_ensure(h, s.d_frames, s.frames_bytes, (size_t)n_frames * frame_bytes)) return 1;
        PF_HIP(h, hipMemcpyAsync(s.d_frames, frames, (size_t)n_frames * frame_bytes, hipMemcpyHostToDevice, h->stream));
        d_frames = s.d_frames;
    }
    const void* d_kps = kps;
    const int* d_counts = counts;
    if (kps_mem == PF_MEM_HOST) {
        const size_t kb = (size_t)rows * 196 * (kps_f64 ? sizeof(double) : sizeof(float));
        if (align_ensure(h, s.d_kps, s.kps_bytes, kb)) return 1;
        PF_HIP(h, hipMemcpyAsync(s.d_kps, kps, kb, hipMemcpyHostToDevice, h->stream));
        d_kps = s.d_kps;
        if (counts) {
            if (align_ensure(h, s.d_counts, s.counts_bytes, (size_t)n_frames * sizeof(int))) return 1;
            PF_HIP(h, hipMemcpyAsync(s.d_counts, counts, (size_t)n_frames * sizeof(int), hipMemcpyHostToDevice, h->stream));
            d_counts = s.d_counts;
        }
    }
    std::vector<AlignFrame> groups(n_frames);
    for (int f = 0; f < n_frames; ++f) groups[f] = AlignFrame{d_frames + (size_t)f * frame_bytes, height, width, width * 3, 0};
    return align_run(h, rows, chip_size, groups.data(), top_k, d_kps, kps_f64 ? 1 : 0, d_counts, nullptr, 0, chips, mats, valid, out_mem);
}

int pf_face_chips(pf_handle* h, int rows, int chip_size, uint8_t* chips, double* mats, int* valid, int out_mem) {
    if (!h) return 1;
    if (const char* why = align_check_size(chip_size)) PF_FAIL(h, "pf_face_chips: %s (got %d)", why, chip_size);
    if (!chips || rows < 0 || !align_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_chips: bad arguments");
    const AlignState& s = h->align;
    if (s.kind == 2) PF_FAIL(h, "pf_face_chips: the handle's last call was pf_landmark_forward, which has no frame to cut chips from");
    if (s.kind == 0) PF_FAIL(h, "pf_face_chips: the handle's last call left no face rows (pf_landmarks*, pf_run_frames*, pf_track_frame* "
                                "and pf_track_streams do)");
    if (rows > s.rows) PF_FAIL(h, "pf_face_chips: %d rows asked, the last call left %d", rows, s.rows);
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    const std::vector<AlignFrame> groups = s.frames;      // align_run grows the scratch next to it
    return align_run(h, rows, chip_size, groups.data(), s.per_frame, s.kps, s.kps_f64, s.counts, s.valid, s.valid_stride, chips, mats, valid,
                     out_mem);
}

}  // extern "C"

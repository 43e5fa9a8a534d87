// Aligned face chips (included at the end of engine.cpp; kernels in k_align.h):
//   pf_align_faces        stage-level: the caller supplies frames and landmarks (prologue: stage_faces, face_rows.inl)
//   pf_face_chips         the faces of the handle's last pipeline call, from the frame(s) and landmarks it left on the device
//   pf_batch_face_chips   the same over the lanes of a pf_batch (batch.inl)
// What the last call left is pf_handle::last (face_rows.h); this file only reads it, through last_face_rows.
namespace {

const char* align_check_size(int S) {
    return (S < 32 || S > 256 || (S % 16) != 0) ? "chip_size must be a multiple of 16 in [32, 256]" : nullptr;
}

// Fit + warp of `rows` slots; row r reads frame groups[r / per_frame].  d_kps / d_counts / d_valid_in are device pointers.  Outputs in
// device memory are written by the kernels themselves (dead and degenerate slots untouched); host outputs are produced in the
// handle's scratch, copied, synchronised and the rows of valid slots handed over.
int align_run(pf_handle* h, int rows, int S, const AlignFrame* groups, int per_frame, const void* d_kps, int kps_f64,
              const int* d_counts, const int* d_valid_in, int valid_stride, uint8_t* chips, double* mats, int* valid, int out_mem) {
    AlignState& s = h->align;
    const size_t chip_bytes = (size_t)S * S * 3;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    if (scratch_ensure(h, s.d_table, s.table_bytes, (size_t)rows * sizeof(AlignFrame))) return 1;
    if (scratch_ensure(h, s.d_rec, s.rec_bytes, (size_t)rows * PF_ALIGN_REC * sizeof(double))) return 1;
    if (scratch_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
    if (!to_device) {
        if (scratch_ensure(h, s.d_chips, s.chips_bytes, (size_t)rows * chip_bytes)) return 1;
        if (mats && scratch_ensure(h, s.d_mats, s.mats_bytes, (size_t)rows * 6 * sizeof(double))) return 1;
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
    if (copy_valid_runs(h, s.h_valid, rows, RowCopy{chips, s.d_chips, chip_bytes}, RowCopy{mats, s.d_mats, 6 * sizeof(double)})) return 1;
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

}  // namespace

extern "C" {

int pf_align_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                   const void* kps, int kps_f64, int kps_mem, const int* counts, int top_k, int chip_size,
                   uint8_t* chips, double* mats, int* valid, int out_mem) {
    if (!h) return 1;
    if (const char* why = align_check_size(chip_size)) PF_FAIL(h, "pf_align_faces: %s (got %d)", why, chip_size);
    StageFaces st;
    if (stage_faces(h, "pf_align_faces", true, frames, mem, n_frames, height, width, kps, kps_f64, kps_mem, counts, top_k, chips, out_mem, &st)) return 1;
    return align_run(h, st.rows, chip_size, st.frames.data(), top_k, st.d_kps, kps_f64 ? 1 : 0, st.d_counts, nullptr, 0, chips, mats, valid, out_mem);
}

int pf_face_chips(pf_handle* h, int rows, int chip_size, uint8_t* chips, double* mats, int* valid, int out_mem) {
    if (!h) return 1;
    if (const char* why = align_check_size(chip_size)) PF_FAIL(h, "pf_face_chips: %s (got %d)", why, chip_size);
    if (!chips || rows < 0 || !face_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_chips: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_chips", "no frame to cut chips from", rows, &s)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    return align_run(h, rows, chip_size, s->frames.data(), s->per_frame, s->kps, s->kps_f64, s->counts, s->valid, s->valid_stride, chips, mats,
                     valid, out_mem);
}

}  // extern "C"

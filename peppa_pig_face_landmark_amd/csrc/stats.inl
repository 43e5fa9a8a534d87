// Per-face region statistics (included after redact.inl; kernels in k_stats.h):
//   pf_measure_faces      stage-level: the caller supplies frames and landmarks (prologue: stage_faces, face_rows.inl)
//   pf_face_stats         the frames and faces of the handle's last pipeline call, from the record it left (pf_handle::last, face_rows.h)
//   pf_batch_face_stats   the same over the lanes of a pf_batch (batch.inl)
// The label maps and owners are filled into the handle's scratch by mask_run's device-output path and read by face_stats_kernel.
namespace {

// refusals every entry point shares; nullptr when the request is fine
const char* stats_check(int dark, int bright, int per_frame, const void* stats, int out_mem, char* buf, size_t cap) {
    if (dark < 0 || bright > 255 || dark >= bright) {
        snprintf(buf, cap, "0 <= dark < bright <= 255 is needed (got dark %d, bright %d)", dark, bright);
        return buf;
    }
    if (!stats) return "stats must not be NULL";
    if (per_frame > 255) {
        snprintf(buf, cap, "owners are bytes (slot + 1): top_k <= 255 is needed, after pf_landmarks* at most 255 boxes (got %d slots per frame)", per_frame);
        return buf;
    }
    if (!face_out_mem_ok(out_mem)) { snprintf(buf, cap, "bad out_mem %d", out_mem); return buf; }
    if (out_mem == PF_MEM_DEVICE && ((size_t)stats & 7)) return "stats in device memory must be 8-byte aligned";
    return nullptr;
}

// Label maps + statistics of `rows` slots; the slots of frame i read groups[i].  d_kps / d_counts / d_valid_in are device pointers.
// Device output is written by the kernels themselves; host output is produced in the handle's scratch, copied in the call's own
// batch of copies and synchronised once (rows of invalid slots stay untouched either way).
int stats_run(pf_handle* h, const char* who, int rows, int per_frame, int H, int W, const AlignFrame* groups, const void* d_kps, int kps_f64,
              const int* d_counts, const int* d_valid_in, int valid_stride, int dark, int bright, unsigned long long* stats, int* valid,
              int out_mem) {
    StatsState& s = h->stats;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    const int images = pf_div_up(rows, per_frame);
    const size_t map_bytes = (size_t)H * W, row_bytes = PF_STATS_ROW * sizeof(unsigned long long);
    if ((long long)pf_div_up(W, PF_MASK_TW) * pf_div_up(H, PF_MASK_TH) * images > 0x7fffffffLL)
        PF_FAIL(h, "%s: %d frames of %d x %d are too many", who, images, H, W);
    if (scratch_ensure(h, s.d_labels, s.labels_bytes, (size_t)images * map_bytes)) return 1;
    if (scratch_ensure(h, s.d_owners, s.owners_bytes, (size_t)images * map_bytes)) return 1;
    if (scratch_ensure(h, s.d_table, s.table_bytes, (size_t)images * sizeof(AlignFrame))) return 1;
    if (!to_device) {
        if (scratch_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
        if (scratch_ensure(h, s.d_out, s.out_bytes, (size_t)rows * row_bytes)) return 1;
    }
    s.h_table.assign(groups, groups + images);
    PF_HIP(h, hipMemcpyAsync(s.d_table, s.h_table.data(), (size_t)images * sizeof(AlignFrame), hipMemcpyHostToDevice, h->stream));
    if (mask_run(h, rows, per_frame, H, W, 0, d_kps, kps_f64, d_counts, d_valid_in, valid_stride, s.d_labels, s.d_owners, nullptr,
                 to_device ? valid : s.d_valid, PF_MEM_DEVICE))
        return 1;
    StatsArgs sa{};
    sa.frames = s.d_table; sa.rec = h->mask.d_rec; sa.labels = s.d_labels; sa.owners = s.d_owners;
    sa.out = to_device ? stats : s.d_out;
    sa.n = rows; sa.per = per_frame; sa.H = H; sa.W = W;
    sa.bands = std::min(pf_div_up(H, 4 * PF_MASK_TH), PF_STATS_MAX_BANDS);      // four pieces of rows per band when the box is the frame
    sa.dark = dark; sa.bright = bright;
    {
        ProfScope ps(h, "face_stats");
        PF_LAUNCH(face_stats_zero_kernel, dim3((unsigned)pf_div_up(rows * PF_STATS_ROW, 256)), dim3(256), h->stream, sa);
        const dim3 grid((unsigned)(rows * sa.bands));            // rows <= 2^20 (stage_faces, the programs' max_batch), bands <= 32
        if (s.staged) PF_LAUNCH(face_stats_staged_kernel, grid, dim3(256), h->stream, sa);
        else PF_LAUNCH(face_stats_kernel, grid, dim3(256), h->stream, sa);
    }
    PF_HIP(h, hipGetLastError());
    if (to_device) return 0;
    s.h_valid.resize(rows);
    PF_HIP(h, hipMemcpyAsync(s.h_valid.data(), s.d_valid, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (copy_valid_runs(h, s.h_valid, rows, RowCopy{stats, s.d_out, row_bytes})) return 1;
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

}  // namespace

extern "C" {

int pf_measure_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width, const void* kps, int kps_f64,
                     int kps_mem, const int* counts, int top_k, int dark, int bright, uint64_t* stats, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = stats_check(dark, bright, top_k, stats, out_mem, buf, sizeof(buf))) PF_FAIL(h, "pf_measure_faces: %s", why);
    StageFaces st;
    if (stage_faces(h, "pf_measure_faces", true, frames, mem, n_frames, height, width, kps, kps_f64, kps_mem, counts, top_k, stats, out_mem, &st)) return 1;
    return stats_run(h, "pf_measure_faces", st.rows, top_k, height, width, st.frames.data(), st.d_kps, kps_f64 ? 1 : 0, st.d_counts, nullptr, 0,
                     dark, bright, reinterpret_cast<unsigned long long*>(stats), valid, out_mem);
}

int pf_face_stats(pf_handle* h, int rows, int dark, int bright, uint64_t* stats, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = stats_check(dark, bright, h->last.kind == 1 ? h->last.per_frame : 0, stats, out_mem, buf, sizeof(buf)))
        PF_FAIL(h, "pf_face_stats: %s", why);
    if (rows < 0) PF_FAIL(h, "pf_face_stats: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_stats", kNoFrameForMaps, rows, &s)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    if ((size_t)pf_div_up(rows, s->per_frame) > s->frames.size()) PF_FAIL(h, "pf_face_stats: the last call left %d frames", (int)s->frames.size());
    return stats_run(h, "pf_face_stats", rows, s->per_frame, s->frames[0].H, s->frames[0].W, s->frames.data(), s->kps, s->kps_f64, s->counts,
                     s->valid, s->valid_stride, dark, bright, reinterpret_cast<unsigned long long*>(stats), valid, out_mem);
}

}  // extern "C"

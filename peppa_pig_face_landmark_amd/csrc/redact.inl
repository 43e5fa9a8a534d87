// Face redaction (included after mask.inl; kernel in k_redact.h):
//   pf_redact_faces        stage-level: the caller supplies frames and landmarks (prologue: stage_faces, face_rows.inl)
//   pf_face_redact         the frames and faces of the handle's last pipeline call, from the record it left (pf_handle::last, face_rows.h)
//   pf_batch_face_redact   the same over the lanes of a pf_batch (batch.inl)
// The label maps are filled into the handle's scratch by mask_run's device-output path and read by redact_kernel.
namespace {

// refusals every entry point shares; nullptr when the request is fine
const char* redact_check(int mode, int label_mask, int strength, int pad, const void* select, int per_frame, const void* out, char* buf, size_t cap) {
    if (mode != PF_REDACT_FILL && mode != PF_REDACT_MOSAIC && mode != PF_REDACT_BLUR) {
        snprintf(buf, cap, "mode must be PF_REDACT_FILL (0), PF_REDACT_MOSAIC (1) or PF_REDACT_BLUR (2) (got %d)", mode);
        return buf;
    }
    if (label_mask == 0 || (label_mask & ~0x3FF)) {
        snprintf(buf, cap, "label_mask must have a bit of 0x3FF set and none above (got 0x%x)", (unsigned)label_mask);
        return buf;
    }
    if (mode == PF_REDACT_MOSAIC && strength != 4 && strength != 8 && strength != 16) {
        snprintf(buf, cap, "strength of PF_REDACT_MOSAIC is the cell size: 4, 8 or 16 (got %d)", strength);
        return buf;
    }
    if (mode == PF_REDACT_BLUR && (strength < 1 || strength > 32)) {
        snprintf(buf, cap, "strength of PF_REDACT_BLUR is the radius: 1 .. 32 (got %d)", strength);
        return buf;
    }
    if (pad < 0 || pad > 4096) { snprintf(buf, cap, "pad must lie in [0, 4096] (got %d)", pad); return buf; }
    if (select && per_frame > 255) {
        snprintf(buf, cap, "select needs owners, which are bytes (slot + 1): top_k <= 255 is needed, after pf_landmarks* at most 255 boxes (got %d slots per frame)", per_frame);
        return buf;
    }
    if (!out) return "out must not be NULL";
    return nullptr;
}

// Label maps + redaction of ceil(rows / per_frame) frames; frame i reads groups[i].  d_kps / d_counts / d_valid_in / d_select are
// device pointers.  Device output is written by the kernel itself; host output is produced in the handle's scratch, copied and
// synchronised.
int redact_run(pf_handle* h, const char* who, int rows, int per_frame, int H, int W, const AlignFrame* groups, const void* d_kps, int kps_f64,
               const int* d_counts, const int* d_valid_in, int valid_stride, const int* d_select, int mode, int label_mask, int strength,
               int pad, unsigned colour, uint8_t* out, int* valid, int out_mem) {
    RedactState& s = h->redact;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    const int images = pf_div_up(rows, per_frame);
    const size_t map_bytes = (size_t)H * W;
    const int tiles_x = pf_div_up(W, PF_MASK_TW), tiles = tiles_x * pf_div_up(H, PF_MASK_TH);
    if ((long long)tiles * images > 0x7fffffffLL) PF_FAIL(h, "%s: %d frames of %d x %d are too many", who, images, H, W);
    if (scratch_ensure(h, s.d_labels, s.labels_bytes, (size_t)images * map_bytes)) return 1;
    if (d_select && scratch_ensure(h, s.d_owners, s.owners_bytes, (size_t)images * map_bytes)) return 1;
    if (scratch_ensure(h, s.d_table, s.table_bytes, (size_t)images * sizeof(AlignFrame))) return 1;
    if (!to_device) {
        if (scratch_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
        if (scratch_ensure(h, s.d_out, s.out_bytes, (size_t)images * map_bytes * 3)) return 1;
    }
    s.h_table.assign(groups, groups + images);
    PF_HIP(h, hipMemcpyAsync(s.d_table, s.h_table.data(), (size_t)images * sizeof(AlignFrame), hipMemcpyHostToDevice, h->stream));
    if (mask_run(h, rows, per_frame, H, W, 0, d_kps, kps_f64, d_counts, d_valid_in, valid_stride, s.d_labels, d_select ? s.d_owners : nullptr,
                 nullptr, to_device ? valid : s.d_valid, PF_MEM_DEVICE))
        return 1;
    RedactArgs ra{};
    ra.frames = s.d_table; ra.rec = h->mask.d_rec; ra.labels = s.d_labels; ra.owners = d_select ? s.d_owners : nullptr; ra.select = d_select;
    ra.out = to_device ? out : s.d_out;
    ra.n = rows; ra.per = per_frame; ra.H = H; ra.W = W; ra.tiles_x = tiles_x; ra.tiles = tiles;
    ra.mode = mode; ra.label_mask = label_mask; ra.strength = strength; ra.pad = pad; ra.colour = colour;
    ra.n_in = mode == PF_REDACT_BLUR ? (unsigned)((2 * strength + 1) * (2 * strength + 1)) : (mode == PF_REDACT_MOSAIC ? (unsigned)(strength * strength) : 1u);
    ra.recip = ((1ULL << PF_REDACT_SHIFT) + ra.n_in - 1) / ra.n_in;
    ra.stage_all = s.stage_all;
    {
        ProfScope ps(h, "redact");
        const dim3 grid((unsigned)(tiles * images));
        const int r = mode == PF_REDACT_BLUR ? strength : 0;       // the smallest instance whose LDS holds the halo
        if (r == 0) PF_LAUNCH(redact_kernel<0>, grid, dim3(256), h->stream, ra);
        else if (r <= 8) PF_LAUNCH(redact_kernel<8>, grid, dim3(256), h->stream, ra);
        else if (r <= 16) PF_LAUNCH(redact_kernel<16>, grid, dim3(256), h->stream, ra);
        else PF_LAUNCH(redact_kernel<32>, grid, dim3(256), h->stream, ra);
    }
    PF_HIP(h, hipGetLastError());
    if (to_device) return 0;
    s.h_valid.resize(rows);
    PF_HIP(h, hipMemcpyAsync(s.h_valid.data(), s.d_valid, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipMemcpyAsync(out, s.d_out, (size_t)images * map_bytes * 3, hipMemcpyDeviceToHost, h->stream));      // every byte is written
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

// `select` of `n` ints from host memory into the handle's scratch
int redact_upload_select(pf_handle* h, const int* select, int n, const int** d_select) {
    RedactState& s = h->redact;
    *d_select = nullptr;
    if (!select) return 0;
    if (scratch_ensure(h, s.d_select, s.select_bytes, (size_t)n * sizeof(int))) return 1;
    PF_HIP(h, hipMemcpyAsync(s.d_select, select, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    *d_select = s.d_select;
    return 0;
}

}  // namespace

extern "C" {

int pf_redact_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width, const void* kps, int kps_f64,
                    int kps_mem, const int* counts, const int* select, int top_k, int mode, int label_mask, int strength, int pad,
                    unsigned colour, uint8_t* out, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = redact_check(mode, label_mask, strength, pad, select, top_k, out, buf, sizeof(buf))) PF_FAIL(h, "pf_redact_faces: %s", why);
    StageFaces st;
    if (stage_faces(h, "pf_redact_faces", true, frames, mem, n_frames, height, width, kps, kps_f64, kps_mem, counts, top_k, out, out_mem, &st)) return 1;
    const int* d_select = select;       // lives where the landmarks live
    if (kps_mem == PF_MEM_HOST && redact_upload_select(h, select, st.rows, &d_select)) return 1;
    return redact_run(h, "pf_redact_faces", st.rows, top_k, height, width, st.frames.data(), st.d_kps, kps_f64 ? 1 : 0, st.d_counts, nullptr, 0,
                      d_select, mode, label_mask, strength, pad, colour, out, valid, out_mem);
}

int pf_face_redact(pf_handle* h, int rows, const int* select, int mode, int label_mask, int strength, int pad, unsigned colour, uint8_t* out,
                   int* valid, int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = redact_check(mode, label_mask, strength, pad, select, h->last.kind == 1 ? h->last.per_frame : 0, out, buf, sizeof(buf)))
        PF_FAIL(h, "pf_face_redact: %s", why);
    if (rows < 0 || !face_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_redact: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_redact", kNoFrameForMaps, rows, &s)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    const int* d_select = nullptr;
    if (redact_upload_select(h, select, rows, &d_select)) return 1;
    if ((size_t)pf_div_up(rows, s->per_frame) > s->frames.size()) PF_FAIL(h, "pf_face_redact: the last call left %d frames", (int)s->frames.size());
    return redact_run(h, "pf_face_redact", rows, s->per_frame, s->frames[0].H, s->frames[0].W, s->frames.data(), s->kps, s->kps_f64, s->counts,
                      s->valid, s->valid_stride, d_select, mode, label_mask, strength, pad, colour, out, valid, out_mem);
}

}  // extern "C"

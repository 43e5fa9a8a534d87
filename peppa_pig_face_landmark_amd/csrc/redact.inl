// Face redaction (included after mask.inl; kernel in k_redact.h):
//   pf_redact_faces        stage-level: the caller supplies frames and landmarks
//   pf_face_redact         the frames and faces of the handle's last pipeline call, from the record chips_note_* keeps for pf_face_chips
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
    if (align_ensure(h, s.d_labels, s.labels_bytes, (size_t)images * map_bytes)) return 1;
    if (d_select && align_ensure(h, s.d_owners, s.owners_bytes, (size_t)images * map_bytes)) return 1;
    if (align_ensure(h, s.d_table, s.table_bytes, (size_t)images * sizeof(AlignFrame))) return 1;
    if (!to_device) {
        if (align_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
        if (align_ensure(h, s.d_out, s.out_bytes, (size_t)images * map_bytes * 3)) return 1;
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
    if (align_ensure(h, s.d_select, s.select_bytes, (size_t)n * sizeof(int))) return 1;
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
    if (n_frames < 1 || height < 1 || width < 1 || height > 32768 || width > 32768 || top_k < 1 || !kps ||
        (mem != PF_MEM_HOST && mem != PF_MEM_DEVICE && mem != PF_MEM_RESIDENT) || (kps_mem != PF_MEM_HOST && kps_mem != PF_MEM_DEVICE) ||
        !align_out_mem_ok(out_mem) || (!frames && mem != PF_MEM_RESIDENT))
        PF_FAIL(h, "pf_redact_faces: bad arguments");
    if ((long long)n_frames * top_k > (1 << 20)) PF_FAIL(h, "pf_redact_faces: %d x %d face slots are too many", n_frames, top_k);
    AlignState& s = h->align;       // the upload scratch of pf_align_faces serves here too
    const size_t frame_bytes = (size_t)height * width * 3;
    const unsigned char* d_frames = frames;
    if (mem == PF_MEM_RESIDENT) {
        if (n_frames != 1) PF_FAIL(h, "pf_redact_faces: PF_MEM_RESIDENT is one frame, n_frames = %d", n_frames);
        if (!h->pipe.have_cur || h->pipe.cur_h != height || h->pipe.cur_w != width)
            PF_FAIL(h, "pf_redact_faces: no resident frame of this size (call pf_set_frame first)");
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
    const int* d_select = select;
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
        if (redact_upload_select(h, select, rows, &d_select)) return 1;
    }
    std::vector<AlignFrame> groups(n_frames);
    for (int f = 0; f < n_frames; ++f) groups[f] = AlignFrame{d_frames + (size_t)f * frame_bytes, height, width, width * 3, 0};
    return redact_run(h, "pf_redact_faces", rows, top_k, height, width, groups.data(), d_kps, kps_f64 ? 1 : 0, d_counts, nullptr, 0, d_select, mode,
                      label_mask, strength, pad, colour, out, valid, out_mem);
}

int pf_face_redact(pf_handle* h, int rows, const int* select, int mode, int label_mask, int strength, int pad, unsigned colour, uint8_t* out,
                   int* valid, int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = redact_check(mode, label_mask, strength, pad, select, h->align.kind == 1 ? h->align.per_frame : 0, out, buf, sizeof(buf)))
        PF_FAIL(h, "pf_face_redact: %s", why);
    if (rows < 0 || !align_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_redact: bad arguments");
    int H = 0, W = 0;
    if (mask_last_call(h, "pf_face_redact", rows, &H, &W)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    const AlignState& s = h->align;
    const int* d_select = nullptr;
    if (redact_upload_select(h, select, rows, &d_select)) return 1;
    const std::vector<AlignFrame> groups = s.frames;
    if ((size_t)pf_div_up(rows, s.per_frame) > groups.size()) PF_FAIL(h, "pf_face_redact: the last call left %d frames", (int)groups.size());
    return redact_run(h, "pf_face_redact", rows, s.per_frame, H, W, groups.data(), s.kps, s.kps_f64, s.counts, s.valid, s.valid_stride, d_select, mode,
                      label_mask, strength, pad, colour, out, valid, out_mem);
}

}  // extern "C"

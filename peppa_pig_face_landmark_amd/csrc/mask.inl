// Face-region label maps (included after align.inl; kernels in k_mask.h):
//   pf_mask_faces         stage-level: the caller supplies landmarks and the frame's size
//   pf_face_masks         the faces of the handle's last pipeline call, from the record chips_note_* keeps for pf_face_chips
//   pf_batch_face_masks   the same over the lanes of a pf_batch (batch.inl)
// A mask reads the landmarks and the frame's size, never a pixel.
namespace {

// Edges + fill of `rows` slots.  chip_size = 0: frame space, ceil(rows / per_frame) maps of H x W; else one S x S map per slot.
// d_kps / d_counts / d_valid_in are device pointers.  Device outputs are written by the kernels themselves; host outputs are
// produced in the handle's scratch, copied and synchronised (maps of invalid chip-space slots and box rows of invalid slots stay
// untouched either way).
int mask_run(pf_handle* h, int rows, int per_frame, int H, int W, int S, const void* d_kps, int kps_f64, const int* d_counts,
             const int* d_valid_in, int valid_stride, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem) {
    MaskState& s = h->mask;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    const int images = S ? rows : pf_div_up(rows, per_frame);
    const int mh = S ? S : H, mw = S ? S : W;
    const size_t map_bytes = (size_t)mh * mw;
    const int tiles_x = pf_div_up(mw, PF_MASK_TW), tiles = tiles_x * pf_div_up(mh, PF_MASK_TH);
    if ((long long)tiles * images > 0x7fffffffLL) PF_FAIL(h, "pf_mask_faces: %d maps of %d x %d are too many", images, mh, mw);
    if (align_ensure(h, s.d_rec, s.rec_bytes, (size_t)rows * PF_MASK_REC * sizeof(int))) return 1;
    if (!to_device) {
        if (align_ensure(h, s.d_labels, s.labels_bytes, (size_t)images * map_bytes)) return 1;
        if (owners && align_ensure(h, s.d_owners, s.owners_bytes, (size_t)images * map_bytes)) return 1;
        if (boxes && align_ensure(h, s.d_boxes, s.boxes_bytes, (size_t)rows * 4 * sizeof(int))) return 1;
        if (align_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
    }
    MaskEdgesArgs ea{};
    ea.kps = d_kps; ea.kps_f64 = kps_f64; ea.n = rows; ea.per_frame = per_frame; ea.S = S; ea.H = mh; ea.W = mw;
    ea.counts = d_counts; ea.valid_in = d_valid_in; ea.valid_stride = valid_stride;
    ea.rec = s.d_rec;
    ea.boxes_out = to_device ? boxes : (boxes ? s.d_boxes : nullptr);
    ea.valid_out = to_device ? valid : s.d_valid;
    {
        ProfScope ps(h, "mask_edges");
        PF_LAUNCH(mask_edges_kernel, dim3(rows), dim3(64), h->stream, ea);
    }
    MaskFillArgs fa{};
    fa.rec = s.d_rec;
    fa.labels = to_device ? labels : s.d_labels;
    fa.owners = owners ? (to_device ? owners : s.d_owners) : nullptr;
    fa.n = rows; fa.per = S ? 1 : per_frame; fa.H = mh; fa.W = mw; fa.tiles_x = tiles_x; fa.tiles = tiles;
    fa.chip = S ? 1 : 0; fa.no_cull = s.no_cull;
    {
        ProfScope ps(h, "mask_fill");
        PF_LAUNCH(mask_fill_kernel, dim3((unsigned)(tiles * images)), dim3(256), h->stream, fa);
    }
    PF_HIP(h, hipGetLastError());
    if (to_device) return 0;
    s.h_valid.resize(rows);
    PF_HIP(h, hipMemcpyAsync(s.h_valid.data(), s.d_valid, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (!S) {       // every byte of a frame's maps is written
        PF_HIP(h, hipMemcpyAsync(labels, s.d_labels, (size_t)images * map_bytes, hipMemcpyDeviceToHost, h->stream));
        if (owners) PF_HIP(h, hipMemcpyAsync(owners, s.d_owners, (size_t)images * map_bytes, hipMemcpyDeviceToHost, h->stream));
    }
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (S || boxes) {
        for (int r = 0; r < rows;) {       // runs of valid rows come over in one copy each
            if (!s.h_valid[r]) { ++r; continue; }
            int e = r + 1;
            while (e < rows && s.h_valid[e]) ++e;
            if (S) PF_HIP(h, hipMemcpyAsync(labels + (size_t)r * map_bytes, s.d_labels + (size_t)r * map_bytes, (size_t)(e - r) * map_bytes,
                                            hipMemcpyDeviceToHost, h->stream));
            if (boxes) PF_HIP(h, hipMemcpyAsync(boxes + (size_t)r * 4, s.d_boxes + (size_t)r * 4, (size_t)(e - r) * 4 * sizeof(int),
                                                hipMemcpyDeviceToHost, h->stream));
            r = e;
        }
        PF_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

// refusals every entry point shares; nullptr when the request is fine
const char* mask_check(int chip_size, int per_frame, const void* owners, const void* boxes, char* buf, size_t cap) {
    if (chip_size != 0) {
        if (const char* why = align_check_size(chip_size)) { snprintf(buf, cap, "%s, or 0 for frame space (got %d)", why, chip_size); return buf; }
        if (owners || boxes) return "owners and boxes must be NULL in chip space (chip_size != 0): a chip map holds one face";
    } else if (owners && per_frame > 255) {
        snprintf(buf, cap, "owners are bytes (slot + 1): top_k <= 255 is needed, after pf_landmarks* at most 255 boxes (got %d slots per frame)", per_frame);
        return buf;
    }
    return nullptr;
}

// the record of the last pipeline call, as pf_face_chips judges it; on success the frame size the maps take
int mask_last_call(pf_handle* h, const char* who, int rows, int* H, int* W) {
    const AlignState& s = h->align;
    if (s.kind == 2) PF_FAIL(h, "%s: the handle's last call was pf_landmark_forward, which has no frame to lay the maps over", who);
    if (s.kind == 0)
        PF_FAIL(h, "%s: the handle's last call left no face rows (pf_landmarks*, pf_run_frames*, pf_track_frame* and pf_track_streams do)", who);
    if (rows > s.rows) PF_FAIL(h, "%s: %d rows asked, the last call left %d", who, rows, s.rows);
    *H = s.frames[0].H; *W = s.frames[0].W;
    return 0;
}

}  // namespace

extern "C" {

int pf_mask_faces(pf_handle* h, int n_frames, int height, int width, const void* kps, int kps_f64, int kps_mem, const int* counts,
                  int top_k, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[160];
    if (const char* why = mask_check(chip_size, top_k, owners, boxes, buf, sizeof(buf))) PF_FAIL(h, "pf_mask_faces: %s", why);
    if (n_frames < 1 || top_k < 1 || !kps || !labels || (kps_mem != PF_MEM_HOST && kps_mem != PF_MEM_DEVICE) || !align_out_mem_ok(out_mem) ||
        (chip_size == 0 && (height < 1 || width < 1 || height > 32768 || width > 32768)))
        PF_FAIL(h, "pf_mask_faces: bad arguments");
    if ((long long)n_frames * top_k > (1 << 20)) PF_FAIL(h, "pf_mask_faces: %d x %d face slots are too many", n_frames, top_k);
    PF_HIP(h, hipSetDevice(h->device));
    AlignState& s = h->align;       // the upload scratch of pf_align_faces serves here too
    const int rows = n_frames * top_k;
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
    return mask_run(h, rows, top_k, height, width, chip_size, d_kps, kps_f64 ? 1 : 0, d_counts, nullptr, 0, labels, owners, boxes, valid, out_mem);
}

int pf_face_masks(pf_handle* h, int rows, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[160];
    if (const char* why = mask_check(chip_size, h->align.kind == 1 ? h->align.per_frame : 0, owners, boxes, buf, sizeof(buf)))
        PF_FAIL(h, "pf_face_masks: %s", why);
    if (!labels || rows < 0 || !align_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_masks: bad arguments");
    int H = 0, W = 0;
    if (mask_last_call(h, "pf_face_masks", rows, &H, &W)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    const AlignState& s = h->align;
    return mask_run(h, rows, s.per_frame, H, W, chip_size, s.kps, s.kps_f64, s.counts, s.valid, s.valid_stride, labels, owners, boxes, valid,
                    out_mem);
}

int pf_face_masks_shape(pf_handle* h, int rows, int* n_frames, int* height, int* width) {
    if (!h) return 1;
    if (rows < 0 || !n_frames || !height || !width) PF_FAIL(h, "pf_face_masks_shape: bad arguments");
    if (mask_last_call(h, "pf_face_masks_shape", rows, height, width)) return 1;
    *n_frames = pf_div_up(rows, h->align.per_frame);
    return 0;
}

}  // extern "C"

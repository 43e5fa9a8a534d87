// Face-region label maps (included after align.inl; kernels in k_mask.h):
//   pf_mask_faces         stage-level: the caller supplies landmarks and the frame's size (prologue: stage_faces without frames)
//   pf_face_masks         the faces of the handle's last pipeline call, from the record it left (pf_handle::last, face_rows.h)
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
    if (scratch_ensure(h, s.d_rec, s.rec_bytes, (size_t)rows * PF_MASK_REC * sizeof(int))) return 1;
    if (!to_device) {
        if (scratch_ensure(h, s.d_labels, s.labels_bytes, (size_t)images * map_bytes)) return 1;
        if (owners && scratch_ensure(h, s.d_owners, s.owners_bytes, (size_t)images * map_bytes)) return 1;
        if (boxes && scratch_ensure(h, s.d_boxes, s.boxes_bytes, (size_t)rows * 4 * sizeof(int))) return 1;
        if (scratch_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
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
    if ((S || boxes) && copy_valid_runs(h, s.h_valid, rows, RowCopy{S ? labels : nullptr, s.d_labels, map_bytes},
                                        RowCopy{boxes, s.d_boxes, 4 * sizeof(int)}))
        return 1;
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

// last_face_rows for an accessor that lays maps over the frames of the last call (their size: frames[0].H x frames[0].W)
const char* const kNoFrameForMaps = "no frame to lay the maps over";

}  // namespace

extern "C" {

int pf_mask_faces(pf_handle* h, int n_frames, int height, int width, const void* kps, int kps_f64, int kps_mem, const int* counts,
                  int top_k, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[160];
    if (const char* why = mask_check(chip_size, top_k, owners, boxes, buf, sizeof(buf))) PF_FAIL(h, "pf_mask_faces: %s", why);
    // the frame's size matters in frame space only; the same refusal as the shared checks of stage_faces, which looks at neither
    if (chip_size == 0 && (height < 1 || width < 1 || height > 32768 || width > 32768)) PF_FAIL(h, "pf_mask_faces: bad arguments");
    StageFaces st;
    if (stage_faces(h, "pf_mask_faces", false, nullptr, 0, n_frames, height, width, kps, kps_f64, kps_mem, counts, top_k, labels, out_mem, &st)) return 1;
    return mask_run(h, st.rows, top_k, height, width, chip_size, st.d_kps, kps_f64 ? 1 : 0, st.d_counts, nullptr, 0, labels, owners, boxes, valid,
                    out_mem);
}

int pf_face_masks(pf_handle* h, int rows, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem) {
    if (!h) return 1;
    char buf[160];
    if (const char* why = mask_check(chip_size, h->last.kind == 1 ? h->last.per_frame : 0, owners, boxes, buf, sizeof(buf)))
        PF_FAIL(h, "pf_face_masks: %s", why);
    if (!labels || rows < 0 || !face_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_masks: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_masks", kNoFrameForMaps, rows, &s)) return 1;
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    return mask_run(h, rows, s->per_frame, s->frames[0].H, s->frames[0].W, chip_size, s->kps, s->kps_f64, s->counts, s->valid, s->valid_stride,
                    labels, owners, boxes, valid, out_mem);
}

int pf_face_masks_shape(pf_handle* h, int rows, int* n_frames, int* height, int* width) {
    if (!h) return 1;
    if (rows < 0 || !n_frames || !height || !width) PF_FAIL(h, "pf_face_masks_shape: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_masks_shape", kNoFrameForMaps, rows, &s)) return 1;
    *n_frames = pf_div_up(rows, s->per_frame);
    *height = s->frames[0].H; *width = s->frames[0].W;
    return 0;
}

}  // extern "C"

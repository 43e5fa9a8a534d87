// Face overlay (included after redact.inl; kernels in k_draw.h):
//   pf_draw_faces        stage-level: the caller supplies frames, landmarks and scores (prologue: stage_faces, face_rows.inl)
//   pf_face_draw         the frames and faces of the handle's last pipeline call, from the record it left (pf_handle::last, face_rows.h),
//                        or `base` frames of the same shape in their place
//   pf_batch_face_draw   the same over the lanes of a pf_batch (batch.inl)
// The calls read the record and leave it alone; nothing here is captured into a graph.
namespace {

// refusals every entry point shares; nullptr when the request is fine
const char* draw_check(const pf_draw_style* style, const void* out, char* buf, size_t cap) {
    if (!style) return "style must not be NULL";
    if (style->what == 0 || (style->what & ~7)) {
        snprintf(buf, cap, "what must have a bit of PF_DRAW_POINTS | PF_DRAW_CONTOURS | PF_DRAW_BOX (7) set and none above (got 0x%x)", (unsigned)style->what);
        return buf;
    }
    if (style->point_radius < 1 || style->point_radius > 16) { snprintf(buf, cap, "point_radius must lie in [1, 16] (got %d)", style->point_radius); return buf; }
    if (style->line_width < 1 || style->line_width > 16) { snprintf(buf, cap, "line_width must lie in [1, 16] (got %d)", style->line_width); return buf; }
    if (style->alpha < 1 || style->alpha > 256) { snprintf(buf, cap, "alpha must lie in [1, 256] (got %d)", style->alpha); return buf; }
    if (!out) return "out must not be NULL";
    return nullptr;
}

// Primitives + overlay of ceil(rows / per_frame) frames; frame i reads groups[i].  d_kps / d_counts / d_valid_in / d_scores are device
// pointers.  Device output is written by the kernel itself; host output is produced in the handle's scratch, copied and synchronised.
int draw_run(pf_handle* h, const char* who, int rows, int per_frame, int H, int W, const AlignFrame* groups, const void* d_kps, int kps_f64,
             const int* d_counts, const int* d_valid_in, int valid_stride, const float* d_scores, const pf_draw_style& st, uint8_t* out,
             int* valid, int out_mem) {
    DrawState& s = h->draw;
    const bool to_device = out_mem == PF_MEM_DEVICE;
    const int images = pf_div_up(rows, per_frame);
    const size_t frame_bytes = (size_t)H * W * 3;
    const int tiles_x = pf_div_up(W, PF_MASK_TW), tiles = tiles_x * pf_div_up(H, PF_MASK_TH);
    if ((long long)tiles * images > 0x7fffffffLL) PF_FAIL(h, "%s: %d frames of %d x %d are too many", who, images, H, W);
    if (scratch_ensure(h, s.d_head, s.head_bytes, (size_t)rows * PF_DRAW_HEAD * sizeof(int))) return 1;
    if (scratch_ensure(h, s.d_prims, s.prims_bytes, (size_t)rows * PF_DRAW_PRIMS * sizeof(DrawPrim))) return 1;
    if (scratch_ensure(h, s.d_bounds, s.bounds_bytes, (size_t)rows * PF_DRAW_PRIMS * sizeof(unsigned long long))) return 1;
    if (scratch_ensure(h, s.d_table, s.table_bytes, (size_t)images * sizeof(AlignFrame))) return 1;
    if (!to_device) {
        if (scratch_ensure(h, s.d_valid, s.valid_bytes, (size_t)rows * sizeof(int))) return 1;
        if (scratch_ensure(h, s.d_out, s.out_bytes, (size_t)images * frame_bytes)) return 1;
    }
    s.h_table.assign(groups, groups + images);
    PF_HIP(h, hipMemcpyAsync(s.d_table, s.h_table.data(), (size_t)images * sizeof(AlignFrame), hipMemcpyHostToDevice, h->stream));
    DrawPrimsArgs pa{};
    pa.kps = d_kps; pa.kps_f64 = kps_f64; pa.n = rows; pa.per_frame = per_frame; pa.H = H; pa.W = W;
    pa.counts = d_counts; pa.valid_in = d_valid_in; pa.valid_stride = valid_stride;
    pa.scores = d_scores; pa.score_thres = st.score_thres; pa.what = st.what; pa.r = st.point_radius; pa.w = st.line_width;
    pa.head = s.d_head; pa.prims = s.d_prims; pa.bounds = s.d_bounds; pa.valid_out = to_device ? valid : s.d_valid;
    {
        ProfScope ps(h, "draw_prims");
        PF_LAUNCH(draw_prims_kernel, dim3(rows), dim3(64), h->stream, pa);
    }
    DrawArgs da{};
    da.frames = s.d_table; da.head = s.d_head; da.prims = s.d_prims; da.bounds = s.d_bounds; da.out = to_device ? out : s.d_out;
    da.n = rows; da.per = per_frame; da.H = H; da.W = W; da.tiles_x = tiles_x; da.tiles = tiles;
    da.alpha = st.alpha;
    da.colour[0] = st.colour_hi; da.colour[1] = st.colour_lo; da.colour[2] = st.colour_contour; da.colour[3] = st.colour_box;
    da.no_cull = s.no_cull;
    {
        ProfScope ps(h, "draw");
        PF_LAUNCH(draw_kernel, dim3((unsigned)(tiles * images)), dim3(256), h->stream, da);
    }
    PF_HIP(h, hipGetLastError());
    if (to_device) return 0;
    s.h_valid.resize(rows);
    PF_HIP(h, hipMemcpyAsync(s.h_valid.data(), s.d_valid, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipMemcpyAsync(out, s.d_out, (size_t)images * frame_bytes, hipMemcpyDeviceToHost, h->stream));      // every byte is written
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (valid) memcpy(valid, s.h_valid.data(), (size_t)rows * sizeof(int));
    return 0;
}

// `scores` of `rows` x 98 floats from host memory into the handle's scratch
int draw_upload_scores(pf_handle* h, const float* scores, int rows, const float** d_scores) {
    DrawState& s = h->draw;
    *d_scores = nullptr;
    if (!scores) return 0;
    const size_t nb = (size_t)rows * PF_DRAW_NPOINTS * sizeof(float);
    if (scratch_ensure(h, s.d_scores, s.scores_bytes, nb)) return 1;
    PF_HIP(h, hipMemcpyAsync(s.d_scores, scores, nb, hipMemcpyHostToDevice, h->stream));
    *d_scores = s.d_scores;
    return 0;
}

bool draw_overlap(const void* a, const void* b, size_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + n && y < x + n;
}

}  // namespace

extern "C" {

int pf_draw_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width, const void* kps, int kps_f64,
                  int kps_mem, const int* counts, const float* scores, int top_k, const pf_draw_style* style, uint8_t* out, int* valid,
                  int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = draw_check(style, out, buf, sizeof(buf))) PF_FAIL(h, "pf_draw_faces: %s", why);
    StageFaces st;
    if (stage_faces(h, "pf_draw_faces", true, frames, mem, n_frames, height, width, kps, kps_f64, kps_mem, counts, top_k, out, out_mem, &st)) return 1;
    const float* d_scores = scores;       // lives where the landmarks live
    if (kps_mem == PF_MEM_HOST && draw_upload_scores(h, scores, st.rows, &d_scores)) return 1;
    return draw_run(h, "pf_draw_faces", st.rows, top_k, height, width, st.frames.data(), st.d_kps, kps_f64 ? 1 : 0, st.d_counts, nullptr, 0,
                    d_scores, *style, out, valid, out_mem);
}

int pf_face_draw(pf_handle* h, int rows, const float* scores, const pf_draw_style* style, const uint8_t* base, uint8_t* out, int* valid,
                 int out_mem) {
    if (!h) return 1;
    char buf[200];
    if (const char* why = draw_check(style, out, buf, sizeof(buf))) PF_FAIL(h, "pf_face_draw: %s", why);
    if (rows < 0 || !face_out_mem_ok(out_mem)) PF_FAIL(h, "pf_face_draw: bad arguments");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_face_draw", "no frame to draw on", rows, &s)) return 1;
    if (rows == 0) return 0;
    const int images = pf_div_up(rows, s->per_frame);
    if ((size_t)images > s->frames.size()) PF_FAIL(h, "pf_face_draw: the last call left %d frames", (int)s->frames.size());
    const int H = s->frames[0].H, W = s->frames[0].W;
    const size_t frame_bytes = (size_t)H * W * 3;
    if (base && out_mem == PF_MEM_DEVICE && draw_overlap(base, out, (size_t)images * frame_bytes)) PF_FAIL(h, "pf_face_draw: base must not alias out");
    PF_HIP(h, hipSetDevice(h->device));
    const float* d_scores = nullptr;
    if (draw_upload_scores(h, scores, rows, &d_scores)) return 1;
    std::vector<AlignFrame> over;
    if (base) over = face_frames(base, frame_bytes, images, H, W, W * 3);
    return draw_run(h, "pf_face_draw", rows, s->per_frame, H, W, base ? over.data() : s->frames.data(), s->kps, s->kps_f64, s->counts, s->valid,
                    s->valid_stride, d_scores, *style, out, valid, out_mem);
}

}  // extern "C"

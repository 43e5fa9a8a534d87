// pf_track_frame / pf_track_reset: FaceAna.run() / reset() for one video stream with the tracking state on the device;
// pf_track_streams*: the same for N streams on one handle, one call advancing any subset of them by one frame each
// (included at the end of engine.cpp; kernels in k_track.h).  Both run the same stream-batched kernels (track_enqueue).
namespace {

// Identity state of every slot of a pool back to "no ids, empty lost lists, counters at 0" (a new pool, pf_track_ids_config); the
// tracking state is left alone: rows whose id is 0 pass on no source and get fresh ids (rule step 1).  Ordered on the handle's stream.
int track_ids_forget(pf_handle* h, TrackPool& P) {
    if (!P.v.id) return 0;
    const size_t s = (size_t)P.S, k = (size_t)P.K;
    PF_HIP(h, hipMemsetAsync(P.v.id, 0, s * k * sizeof(int), h->stream));
    PF_HIP(h, hipMemsetAsync(P.v.age, 0, s * k * sizeof(int), h->stream));
    PF_HIP(h, hipMemsetAsync(P.v.next_id, 0, s * sizeof(int), h->stream));
    PF_HIP(h, hipMemsetAsync(P.v.lost_n, 0, s * sizeof(int), h->stream));
    return 0;
}

// Persistent ids are kept for at most kTrackMaxLost faces per frame.  Ids on and a pool of more faces never meet: whichever is asked
// for second is refused here, by the entry point that asks, before it changes anything.
int track_ids_fit(pf_handle* h, const char* who, int ids_on, int top_k) {
    if (ids_on && top_k > kTrackMaxLost)
        PF_FAIL(h, "%s: persistent ids are kept for at most %d faces per frame, top_k is %d", who, kTrackMaxLost, top_k);
    return 0;
}

// (Re)allocate a pool of S slots for up to K faces each; every slot forgets its stream.
int track_pool_alloc(pf_handle* h, TrackPool& P, int S, int K) {
    PF_HIP(h, hipStreamSynchronize(h->stream));
    P.release();
    TrackPoolView& v = P.v;
    const size_t s = (size_t)S, k = (size_t)K;
    PF_HIP(h, hipMalloc((void**)&v.track_box, s * kTrackMaxNow * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.judged, s * kTrackMaxNow * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.lm, s * 2 * k * 196 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.dx, s * 2 * k * 196 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.sel, s * k * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.hull, s * k * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.out_box, s * k * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.out_lm, s * k * 196 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.scores, s * k * 98 * sizeof(float)));
    PF_HIP(h, hipMalloc((void**)&v.n_track, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.n_lm, s * 2 * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.f32, s * 4 * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.n_judged, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.n_sel, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.sel_f32, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.out_count, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&P.d_desc, s * sizeof(TrackFrameDesc)));
    // persistent ids (small next to the landmark sets, so allocated whether or not pf_track_ids_config switches them on)
    PF_HIP(h, hipMalloc((void**)&v.id, s * k * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.age, s * k * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.next_id, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.lost_n, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.lost_id, s * kTrackMaxLost * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.lost_age, s * kTrackMaxLost * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.lost_gone, s * kTrackMaxLost * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.lost_box, s * kTrackMaxLost * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.match_j, s * kTrackMaxNow * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.match_w, s * kTrackMaxNow * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.sel_src, s * k * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.prev_box, s * k * 4 * sizeof(double)));
    PF_HIP(h, hipMalloc((void**)&v.prev_n, s * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.out_id, s * k * sizeof(int)));
    PF_HIP(h, hipMalloc((void**)&v.out_age, s * k * sizeof(int)));
    PF_HIP(h, hipMemset(v.f32, 0, s * 4 * sizeof(int)));
    PF_HIP(h, hipMemset(v.n_track, 0, s * sizeof(int)));
    PF_HIP(h, hipMemset(v.n_lm, 0, s * 2 * sizeof(int)));
    v.desc = P.d_desc;
    v.K = v.top_k = K;
    P.S = S;
    P.K = K;
    P.slots.assign(S, TrackSlot());
    P.h_desc.assign(S, TrackFrameDesc{});
    return track_ids_forget(h, P);        // a new pool counts its ids from 1
}

// pf_track_frame's pool: one slot, reallocated (and the stream forgotten) only when a call asks for more faces
int ensure_track(pf_handle* h, int top_k) {
    if (h->track.K >= top_k && h->track.v.track_box) return 0;
    return track_pool_alloc(h, h->track, 1, top_k);
}

// Steps 3-6 of FaceAna.run() for the n frames of a call whose gate has been evaluated (facer.py:55-81).  P.h_desc[0, n)
// holds each frame's slot / ping-pong half / flags and its index among the n_det detector frames (or -1); h_det_idx[j] is
// the call index of detector frame j and d_det_idx its device copy (nullptr when the detector frames are all n frames in
// order).  planted: host rows [n][planted_rows][16] that replace the detector's own rows.  Everything is enqueued; the
// results of frame i are in P.v.out_count / out_box / out_lm / scores [i] after the caller's synchronisation.
int track_enqueue(pf_handle* h, TrackPool& P, int n, int top_k, const unsigned char* d_frames, int H, int W, int n_det,
                  const int* h_det_idx, const int* d_det_idx, const float* planted, int planted_rows,
                  float score_thres, float nms_iou_thres, float min_face, float track_iou_thres, float smooth_box) {
    Program& det = h->prog[PF_NET_DETECTOR];
    Program& lm = h->prog[PF_NET_LANDMARK];
    const int rows = det.bufs[det.hdr.out_buf0].elems_per_item / 16;
    if (planted && n_det > 0 && planted_rows != rows) PF_FAIL(h, "pf_track: %d planted rows, the detector produces %d", planted_rows, rows);
    if (ensure_pipeline(h, std::max(n_det, 1), n * top_k, top_k, rows)) return 1;
    const bool ids = h->track_ids != 0;      // no pool has more than kTrackMaxLost faces per frame then (track_ids_fit)
    TrackPoolView v = P.v;
    v.top_k = top_k;
    PF_HIP(h, hipMemcpyAsync(P.d_desc, P.h_desc.data(), (size_t)n * sizeof(TrackFrameDesc), hipMemcpyHostToDevice, h->stream));
    // 1. detector + NMS on the frames whose gate opened, then judge_boxs against each stream's track boxes
    if (n_det > 0) {
        const LetterboxGeom g = letterbox_geom(H, W, det.hdr.in_h, det.hdr.in_w);
        if (run_detector_stage(h, d_frames, n_det, H, W, W * 3, g, d_det_idx)) return 1;
        const float* d_rows = (const float*)det.buf_ptr(det.hdr.out_buf0);
        if (planted) {   // planted-candidate protocol: the network ran, its rows are replaced
            const size_t fb = (size_t)rows * 16;
            if (ensure_dev(h, h->pipe.d_rows_planted, h->pipe.rows_planted_bytes, (size_t)n_det * fb * sizeof(float))) return 1;
            for (int j = 0; j < n_det;) {     // one copy per run of consecutive call indices
                int e = j + 1;
                while (e < n_det && h_det_idx[e] == h_det_idx[e - 1] + 1) ++e;
                PF_HIP(h, hipMemcpyAsync(h->pipe.d_rows_planted + (size_t)j * fb, planted + (size_t)h_det_idx[j] * fb,
                                         (size_t)(e - j) * fb * sizeof(float), hipMemcpyHostToDevice, h->stream));
                j = e;
            }
            d_rows = h->pipe.d_rows_planted;
        }
        if (run_nms_stage(h, d_rows, rows, n_det, g, score_thres, nms_iou_thres, 0.f, 1, false)) return 1;
        JudgeStageArgs ja{};
        ja.v = v; ja.stage = TRACK_JUDGE_DETECTIONS;
        ja.det_rows = h->pipe.d_keep_rows; ja.det_count = h->pipe.d_keep_count; ja.det_stride = kMaxKeep;
        ja.iou_thres = track_iou_thres; ja.alpha = smooth_box;
        if (ids) { ja.match_j = v.match_j; ja.match_w = v.match_w; }      // which previous row each detection was smoothed with
        PF_LAUNCH(track_judge_kernel, dim3(n), dim3(256), h->stream, ja);
    }
    // 2. sort_and_filter -> boxes_return (float64 rows, stay on the device)
    SelectArgs sa{};
    sa.v = v; sa.min_face = min_face; sa.ids = ids ? 1 : 0;
    PF_LAUNCH(track_select_kernel, dim3(n), dim3(64), h->stream, sa);
    // 3. landmark stage on the selected boxes: n x top_k slots, the per-frame counts read on the device
    if (run_landmark_stage(h, d_frames, H, W, W * 3, h->pipe.d_sel_boxes, v.n_sel, n * top_k, top_k, v.sel, nullptr, v.sel_f32)) return 1;
    // 4. One-Euro smoothing against the previous sets + hull boxes
    PF_LAUNCH(track_count_kernel, dim3(n), dim3(64), h->stream, v, (const int*)h->pipe.d_crop_params);
    GroupStageArgs ga{};
    ga.v = v;
    ga.kps = h->pipe.d_kps; ga.scores_in = (const float*)lm.buf_ptr(lm.hdr.out_buf1); ga.crop_params = h->pipe.d_crop_params;
    ga.iou_thres = track_iou_thres; ga.scale_w = (double)W; ga.scale_h = (double)H;
    ga.min_cutoff = 0.15; ga.beta = 0.8; ga.d_cutoff = 1.0;          // OneEuroFilter defaults, lk.py:100-101
    if (lm.hdr.out_buf2 >= 0) {      // face-attribute records follow the compaction of the scores (pf_face_attrs)
        if (ensure_dev(h, h->d_track_attrs, h->track_attrs_bytes, (size_t)n * top_k * PF_FACE_ATTR_REC * sizeof(float))) return 1;
        ga.attrs_in = (const float*)lm.buf_ptr(lm.hdr.out_buf2); ga.attrs_out = h->d_track_attrs;
    }
    PF_LAUNCH(track_group_kernel, dim3(top_k, n), dim3(128), h->stream, ga);
    // 5. track_box = judge_boxs(boxes_return, hull boxes) (facer.py:70-81)
    JudgeStageArgs jb{};
    jb.v = v; jb.stage = TRACK_JUDGE_HULLS;
    jb.iou_thres = track_iou_thres; jb.alpha = smooth_box;
    PF_LAUNCH(track_judge_kernel, dim3(n), dim3(256), h->stream, jb);
    // 5b. persistent ids of the new rows (off unless pf_track_ids_config asked): one launch, behind the hull judge
    if (ids) {
        IdentArgs ia{};
        ia.v = v; ia.crop_params = h->pipe.d_crop_params; ia.iou_thres = track_iou_thres; ia.keep_lost = h->track_keep_lost;
        ProfScope ps(h, "track_ident");
        PF_LAUNCH(track_ident_kernel, dim3(n), dim3(256), h->stream, ia);
    }
    // 6. results in call order
    PF_LAUNCH(track_gather_kernel, dim3(n), dim3(256), h->stream, v);
    for (int i = 0; i < n; ++i) {
        TrackSlot& t = P.slots[P.h_desc[i].slot];
        t.cur ^= 1;
        t.lm_valid = true;
        t.has_track = true;
    }
    return 0;
}

// previous-frame storage of a pf_track_streams pool, grown to frames of `bytes`; the frames it holds move with it
int ensure_stream_frames(pf_handle* h, TrackPool& P, size_t bytes) {
    if (bytes <= P.frame_slot_bytes && P.d_frames) return 0;
    const size_t stride = (bytes + 255) / 256 * 256;
    unsigned char* nf = nullptr;
    PF_HIP(h, hipMalloc((void**)&nf, (size_t)P.S * stride));
    if (P.d_frames) {
        for (int s = 0; s < P.S; ++s) {
            const TrackSlot& t = P.slots[s];
            if (t.have_prev)
                PF_HIP(h, hipMemcpyAsync(nf + (size_t)s * stride, P.d_frames + (size_t)s * P.frame_slot_bytes,
                                         (size_t)t.prev_h * t.prev_w * 3, hipMemcpyDeviceToDevice, h->stream));
        }
        PF_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(P.d_frames);
    }
    P.d_frames = nf;
    P.frame_slot_bytes = stride;
    return 0;
}

}  // namespace

extern "C" {

int pf_track_reset(pf_handle* h) {
    if (!h) return 1;
    for (TrackSlot& t : h->track.slots) t.has_track = t.lm_valid = false;
    return pf_forget_frames(h);
}

static int track_frame_impl(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                            const float* planted_rows, int planted_n,
                            float score_thres, float nms_iou_thres, float min_face, int top_k,
                            float track_iou_thres, float smooth_box, float diff_thres,
                            int* n_out, double* boxes, double* kps, float* scores, int* detector_ran);

int pf_track_frame(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                   float score_thres, float nms_iou_thres, float min_face, int top_k,
                   float track_iou_thres, float smooth_box, float diff_thres, int reserved,
                   int* n_out, double* boxes, double* kps, float* scores, int* detector_ran) {
    (void)reserved;
    return track_frame_impl(h, bgr, mem, height, width, row_stride, nullptr, 0, score_thres, nms_iou_thres, min_face, top_k,
                            track_iou_thres, smooth_box, diff_thres, n_out, boxes, kps, scores, detector_ran);
}

int pf_track_frame_planted(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                           const float* det_rows, int rows, float score_thres, float nms_iou_thres, float min_face, int top_k,
                           float track_iou_thres, float smooth_box, float diff_thres,
                           int* n_out, double* boxes, double* kps, float* scores, int* detector_ran) {
    if (!det_rows || rows < 1) { if (h) h->err = "pf_track_frame_planted: no rows"; return 1; }
    return track_frame_impl(h, bgr, mem, height, width, row_stride, det_rows, rows, score_thres, nms_iou_thres, min_face, top_k,
                            track_iou_thres, smooth_box, diff_thres, n_out, boxes, kps, scores, detector_ran);
}

static int track_frame_impl(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                            const float* planted_rows, int planted_n,
                            float score_thres, float nms_iou_thres, float min_face, int top_k,
                            float track_iou_thres, float smooth_box, float diff_thres,
                            int* n_out, double* boxes, double* kps, float* scores, int* detector_ran) {
    if (!h) return 1;
    h->last.forget();
    Program& det = h->prog[PF_NET_DETECTOR];
    Program& lm = h->prog[PF_NET_LANDMARK];
    if (!det.loaded || !lm.loaded) PF_FAIL(h, "pf_track_frame: detector and landmark programs must be loaded");
    if (track_ids_fit(h, "pf_track_frame", h->track_ids, top_k)) return 1;
    if (!bgr || !n_out || top_k < 1 || top_k > lm.max_batch) PF_FAIL(h, "pf_track_frame: bad arguments (top_k %d, landmark max_batch %d)", top_k, lm.max_batch);
    PF_HIP(h, hipSetDevice(h->device));
    if (ensure_track(h, top_k)) return 1;
    TrackPool& P = h->track;
    TrackSlot& t = P.slots[0];
    // 1. frame upload + frame-difference gate (facer.py:55-63,98-118): one 8-byte read-back decides whether the detector runs
    unsigned long long diff_sum = 0;
    int has_prev = 0;
    if (pf_set_frame(h, bgr, mem, height, width, row_stride, &diff_sum, &has_prev)) return 1;
    const double diff = has_prev ? (double)diff_sum / (double)height / (double)width / 3.0 : 0.0;
    const bool run_det = !has_prev || !t.has_track || diff > (double)diff_thres;
    if (detector_ran) *detector_ran = run_det ? 1 : 0;
    TrackFrameDesc& d = P.h_desc[0];
    d.slot = 0; d.cur = t.cur; d.has_track = t.has_track ? 1 : 0;
    d.lm_valid = (t.lm_valid && !run_det) ? 1 : 0;     // a detector frame drops the smoothing history (facer.py:60)
    d.det = run_det ? 0 : -1; d.cmp = 0;
    begin_call(h);
    static const int det_idx0 = 0;
    // 2.-5. the stream-batched track path with one stream (frame: the resident one pf_set_frame stored)
    if (track_enqueue(h, P, 1, top_k, h->pipe.d_cur, height, width, run_det ? 1 : 0, &det_idx0, nullptr,
                      planted_rows, planted_n, score_thres, nms_iou_thres, min_face, track_iou_thres, smooth_box)) return 1;
    // 6. results of this frame: the only device->host traffic of the call besides the 8-byte gate
    int n = 0;
    std::vector<double>& hb = P.h_box;
    std::vector<double>& hk = P.h_lm;
    std::vector<float>& hs = P.h_scores;
    hb.resize((size_t)top_k * 4); hk.resize((size_t)top_k * 196); hs.resize((size_t)top_k * 98);
    PF_HIP(h, hipMemcpyAsync(&n, P.v.out_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipMemcpyAsync(hb.data(), P.v.out_box, hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipMemcpyAsync(hk.data(), P.v.out_lm, hk.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipMemcpyAsync(hs.data(), P.v.scores, hs.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (h->track_ids) {      // ids and ages of the rows ride in the same batch of copies ([0, top_k) ids, [top_k, 2 top_k) ages)
        P.h_ids.resize((size_t)2 * top_k);
        PF_HIP(h, hipMemcpyAsync(P.h_ids.data(), P.v.out_id, (size_t)top_k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        PF_HIP(h, hipMemcpyAsync(P.h_ids.data() + top_k, P.v.out_age, (size_t)top_k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (check_numerics(h)) {
        // The range guard poisoned this frame's outputs with NaN, and steps 4-5 above have already folded them into the
        // stream's state (track boxes, landmark sets, One-Euro filters).  Drop all of it: the caller reloads the network as
        // exact f32 and sends the frame again, and that call must find a stream with no track and no previous frame -- so
        // the detector runs -- instead of a zero frame difference over NaN track boxes.
        const std::string why = h->err;
        (void)pf_track_reset(h);
        h->err = why;
        return 1;
    }
    n = std::min(n, top_k);
    *n_out = n;
    if (lm.hdr.out_buf2 >= 0) h->last.note_attrs(3, n, h->d_track_attrs);   // rows [n], like kps
    // pf_face_chips: the n compacted faces, their smoothed float64 landmarks, the resident frame
    h->last.note_frames(face_frames(h->pipe.d_cur, 0, 1, height, width, width * 3), n, top_k, P.v.out_lm, 1, nullptr);
    if (h->track_ids) h->last.note_ids(P.v.out_id, P.v.out_age, P.h_ids.data(), P.h_ids.data() + top_k);
    if (n > 0) {
        if (boxes) memcpy(boxes, hb.data(), (size_t)n * 4 * sizeof(double));
        if (kps) memcpy(kps, hk.data(), (size_t)n * 196 * sizeof(double));
        if (scores) memcpy(scores, hs.data(), (size_t)n * 98 * sizeof(float));
    }
    return 0;
}

// ---- N video streams on one handle (pf_track_streams*) -----------------------------------------------------------------

int pf_track_streams_config(pf_handle* h, int max_streams, int top_k) {
    if (!h) return 1;
    if (max_streams < 1 || top_k < 1) PF_FAIL(h, "pf_track_streams_config: bad arguments (max_streams %d, top_k %d)", max_streams, top_k);
    if (track_ids_fit(h, "pf_track_streams_config", h->track_ids, top_k)) return 1;
    PF_HIP(h, hipSetDevice(h->device));
    TrackPool& P = h->streams;
    h->last.forget_frames();      // the pool's frame slots and landmarks, which the rows of a pf_track_streams call point at, are replaced
    if (track_pool_alloc(h, P, max_streams, top_k)) return 1;
    PF_HIP(h, hipMalloc((void**)&P.d_sums, (size_t)max_streams * sizeof(unsigned long long)));
    PF_HIP(h, hipMalloc((void**)&P.d_det_idx, (size_t)max_streams * sizeof(int)));
    P.h_sums.assign(max_streams, 0);
    P.h_det_idx.assign(max_streams, 0);
    return 0;
}

int pf_track_ids_config(pf_handle* h, int enable, int keep_lost) {
    if (!h) return 1;
    if (keep_lost < 0 || keep_lost > 255) PF_FAIL(h, "pf_track_ids_config: keep_lost %d outside [0, 255]", keep_lost);
    const int on = enable ? 1 : 0;
    if (track_ids_fit(h, "pf_track_ids_config", on, std::max(h->track.K, h->streams.K))) return 1;
    if (on == h->track_ids && keep_lost == h->track_keep_lost) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    if (track_ids_forget(h, h->track) || track_ids_forget(h, h->streams)) return 1;
    h->track_ids = on;
    h->track_keep_lost = keep_lost;
    h->last.note_ids(nullptr, nullptr, nullptr, nullptr);      // ids of an earlier call belong to the state just forgotten
    return 0;
}

int pf_track_ids(pf_handle* h, int rows, int* ids, int* ages, int out_mem) {
    if (!h) return 1;
    if (rows < 0 || (out_mem != PF_MEM_HOST && out_mem != PF_MEM_DEVICE)) PF_FAIL(h, "pf_track_ids: bad arguments");
    if (!h->track_ids) PF_FAIL(h, "pf_track_ids: persistent ids are off (pf_track_ids_config switches them on)");
    const FaceRows* s = nullptr;
    if (last_face_rows(h, "pf_track_ids", "no tracker and so no ids", rows, &s)) return 1;
    if (!s->ids) PF_FAIL(h, "pf_track_ids: the handle's last call was not a tracking call (pf_track_frame* and pf_track_streams leave ids)");
    if (rows == 0) return 0;
    const size_t bytes = (size_t)rows * sizeof(int);
    if (out_mem == PF_MEM_HOST) {            // the copies the tracking call itself brought back: no device traffic, no synchronisation
        if (ids) memcpy(ids, s->h_ids, bytes);
        if (ages) memcpy(ages, s->h_ages, bytes);
        return 0;
    }
    PF_HIP(h, hipSetDevice(h->device));
    if (ids) PF_HIP(h, hipMemcpyAsync(ids, s->ids, bytes, hipMemcpyDeviceToDevice, h->stream));
    if (ages) PF_HIP(h, hipMemcpyAsync(ages, s->ages, bytes, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int pf_track_streams_reset(pf_handle* h, int stream_id) {
    if (!h) return 1;
    TrackPool& P = h->streams;
    if (P.S == 0) PF_FAIL(h, "pf_track_streams_reset: no stream pool (call pf_track_streams_config first)");
    if (stream_id < -1 || stream_id >= P.S) PF_FAIL(h, "pf_track_streams_reset: stream %d outside [-1, %d)", stream_id, P.S);
    for (int s = 0; s < P.S; ++s)
        if (stream_id < 0 || s == stream_id) { TrackSlot& t = P.slots[s]; t.has_track = t.lm_valid = t.have_prev = false; }
    return 0;
}

int pf_track_streams(pf_handle* h, int n, const int* stream_ids, const uint8_t* frames, int mem, int height, int width,
                     const float* det_rows, int rows, float score_thres, float nms_iou_thres, float min_face,
                     float track_iou_thres, float smooth_box, float diff_thres,
                     int* counts, double* boxes, double* kps, float* scores, int* detector_ran) {
    if (!h) return 1;
    h->last.forget();
    TrackPool& P = h->streams;
    // every check before anything changes: a rejected call leaves every stream as it was
    if (P.S == 0) PF_FAIL(h, "pf_track_streams: no stream pool (call pf_track_streams_config first)");
    Program& det = h->prog[PF_NET_DETECTOR];
    Program& lm = h->prog[PF_NET_LANDMARK];
    if (!det.loaded || !lm.loaded) PF_FAIL(h, "pf_track_streams: detector and landmark programs must be loaded");
    if (n < 1 || !stream_ids || !frames || !counts || height < 1 || width < 1 || (mem != PF_MEM_HOST && mem != PF_MEM_DEVICE))
        PF_FAIL(h, "pf_track_streams: bad arguments");
    if (n > P.S) PF_FAIL(h, "pf_track_streams: %d frames exceed max_streams %d", n, P.S);
    const int K = P.K;
    if (n * K > lm.max_batch) PF_FAIL(h, "pf_track_streams: %d frames x top_k %d exceed the landmark program's max_batch %d", n, K, lm.max_batch);
    if (n > det.max_batch) PF_FAIL(h, "pf_track_streams: %d frames exceed the detector program's max_batch %d", n, det.max_batch);
    const int det_nrows = det.bufs[det.hdr.out_buf0].elems_per_item / 16;
    if (det_rows && rows != det_nrows) PF_FAIL(h, "pf_track_streams: %d planted rows, the detector produces %d", rows, det_nrows);
    {
        std::vector<char> seen(P.S, 0);
        for (int i = 0; i < n; ++i) {
            const int s = stream_ids[i];
            if (s < 0 || s >= P.S) PF_FAIL(h, "pf_track_streams: stream id %d outside [0, %d)", s, P.S);
            if (seen[s]) PF_FAIL(h, "pf_track_streams: stream id %d listed twice", s);
            seen[s] = 1;
        }
    }
    const size_t bytes = (size_t)height * width * 3;
    PF_HIP(h, hipSetDevice(h->device));
    if (ensure_stream_frames(h, P, bytes)) return 1;
    if (ensure_pipeline(h, n, n * K, K, det_nrows)) return 1;
    const unsigned char* d_frames = nullptr;
    if (stage_frames(h, frames, mem, (size_t)n * bytes, &d_frames)) return 1;
    // 1. gate fused with the store of the frames into their slots; one read-back of the n sums
    for (int i = 0; i < n; ++i) {
        const TrackSlot& t = P.slots[stream_ids[i]];
        TrackFrameDesc& d = P.h_desc[i];
        d.slot = stream_ids[i]; d.cur = t.cur; d.has_track = t.has_track ? 1 : 0; d.lm_valid = t.lm_valid ? 1 : 0;
        d.det = -1; d.cmp = (t.have_prev && t.prev_h == height && t.prev_w == width) ? 1 : 0;
    }
    PF_HIP(h, hipMemcpyAsync(P.d_desc, P.h_desc.data(), (size_t)n * sizeof(TrackFrameDesc), hipMemcpyHostToDevice, h->stream));
    PF_HIP(h, hipMemsetAsync(P.d_sums, 0, (size_t)n * sizeof(unsigned long long), h->stream));
    GateArgs ga{};
    ga.cur = d_frames; ga.prev = P.d_frames; ga.bytes = bytes; ga.slot_bytes = P.frame_slot_bytes; ga.desc = P.d_desc; ga.sums = P.d_sums;
    ga.vec = (bytes % 16 == 0 && ((uintptr_t)d_frames % 16) == 0 && P.frame_slot_bytes % 16 == 0) ? 1 : 0;
    const size_t words = ga.vec ? bytes / 16 : bytes;
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(4096, (words + 256 * 16 - 1) / (256 * 16)));
    if ((words + (size_t)blocks * 256 - 1) / ((size_t)blocks * 256) > PF_GATE_MAX_WORDS) PF_FAIL(h, "pf_track_streams: frame of %zu bytes too large for the gate", bytes);
    {
        ProfScope ps(h, "track_gate");
        PF_LAUNCH(track_gate_kernel, dim3(blocks, n), dim3(256), h->stream, ga);
    }
    PF_HIP(h, hipMemcpyAsync(P.h_sums.data(), P.d_sums, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipStreamSynchronize(h->stream));
    // 2. the reference's rule per stream (facer.py:55-63); the slots now hold this call's frames
    int n_det = 0;
    for (int i = 0; i < n; ++i) {
        TrackFrameDesc& d = P.h_desc[i];
        TrackSlot& t = P.slots[d.slot];
        const double diff = d.cmp ? (double)P.h_sums[i] / (double)height / (double)width / 3.0 : 0.0;
        const bool run_det = !d.cmp || !t.has_track || diff > (double)diff_thres;
        if (detector_ran) detector_ran[i] = run_det ? 1 : 0;
        if (run_det) { P.h_det_idx[n_det] = i; d.det = n_det++; d.lm_valid = 0; }
        t.have_prev = true; t.prev_h = height; t.prev_w = width;
    }
    const int* d_det_idx = nullptr;                   // identity when every frame runs the detector
    if (n_det > 0 && n_det < n) {
        PF_HIP(h, hipMemcpyAsync(P.d_det_idx, P.h_det_idx.data(), (size_t)n_det * sizeof(int), hipMemcpyHostToDevice, h->stream));
        d_det_idx = P.d_det_idx;
    }
    begin_call(h);
    // 3.-5. detector on the detector frames only, track kernels and landmark stage over all n streams
    if (track_enqueue(h, P, n, K, d_frames, height, width, n_det, P.h_det_idx.data(), d_det_idx, det_rows, rows,
                      score_thres, nms_iou_thres, min_face, track_iou_thres, smooth_box)) return 1;
    // 6. results: one batch of copies, one synchronisation
    PF_HIP(h, hipMemcpyAsync(counts, P.v.out_count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (boxes) PF_HIP(h, hipMemcpyAsync(boxes, P.v.out_box, (size_t)n * K * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (kps) PF_HIP(h, hipMemcpyAsync(kps, P.v.out_lm, (size_t)n * K * 196 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (scores) PF_HIP(h, hipMemcpyAsync(scores, P.v.scores, (size_t)n * K * 98 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (h->track_ids) {      // the same batch of copies: [0, n K) ids, [n K, 2 n K) ages
        P.h_ids.resize((size_t)2 * n * K);
        PF_HIP(h, hipMemcpyAsync(P.h_ids.data(), P.v.out_id, (size_t)n * K * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        PF_HIP(h, hipMemcpyAsync(P.h_ids.data() + (size_t)n * K, P.v.out_age, (size_t)n * K * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (check_numerics(h)) {
        // as in track_frame_impl: the poisoned outputs are already in the state of every stream of this call; those streams
        // start afresh (no track, no previous frame), the others keep theirs.  The error still names the program slot.
        const std::string why = h->err;
        for (int i = 0; i < n; ++i) { TrackSlot& t = P.slots[stream_ids[i]]; t.has_track = t.lm_valid = t.have_prev = false; }
        h->err = why;
        return 1;
    }
    if (lm.hdr.out_buf2 >= 0) h->last.note_attrs(3, n * K, h->d_track_attrs);   // rows [n][K], like kps
    // pf_face_chips: rows [n][K]; frame i is read from its stream's slot, where the gate stored it
    std::vector<AlignFrame> slots(n);
    for (int i = 0; i < n; ++i) slots[i] = AlignFrame{P.d_frames + (size_t)stream_ids[i] * P.frame_slot_bytes, height, width, width * 3, 0};
    h->last.note_frames(std::move(slots), n * K, K, P.v.out_lm, 1, P.v.out_count);
    if (h->track_ids) h->last.note_ids(P.v.out_id, P.v.out_age, P.h_ids.data(), P.h_ids.data() + (size_t)n * K);
    return 0;
}

}  // extern "C"

/* peppa_hip.h -- C ABI of the MI355X-native FaceAna hot path (libpeppa_hip.so).
 *
 * Drop-in boundary for the compute the reference delegates to onnxruntime / OpenCV / numpy
 * (paths relative to the reference checkout 610265158/Peppa_Pig_Face_Landmark):
 *
 *   reference seam                                              entry point here
 *   ----------------------------------------------------------  -------------------------------
 *   ONNXEngine.__init__(onnx_f)      onnx_model_base.py:7-14     pf_create + pf_load_program
 *   ONNXEngine.__call__(data) kps    onnx_model_base.py:17-27,   pf_landmark_forward
 *                                    face_landmark.py:48
 *   ONNXEngine.__call__(data) det    face_detector.py:29-31      pf_detector_forward
 *   FaceDetector.__call__(image)     face_detector.py:23-42      pf_detect
 *   FaceLandmark.__call__(img,boxes) face_landmark.py:33-64      pf_landmarks
 *   FaceAna.run per frame (no track) facer.py:52-85, demo.py:83-86  pf_run_frames
 *
 * Conventions: every entry returns 0 on success, non-zero on failure (message via
 * pf_last_error).  Plain pointers and sizes only.  `mem` says where caller buffers live:
 * PF_MEM_HOST (numpy / malloc) or PF_MEM_DEVICE (HBM of the handle's device).  One handle = one
 * device + one HIP stream; calls on a handle are serialised by the caller; handles on different
 * devices are independent.  The library never falls back to the CPU.
 */
#ifndef PEPPA_HIP_H
#define PEPPA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_handle pf_handle;

enum { PF_MEM_HOST = 0, PF_MEM_DEVICE = 1, PF_MEM_RESIDENT = 2,     /* 2: the frame stored by pf_set_frame (bgr may be NULL) */
       PF_MEM_HOST_PINNED = 3 };  /* out_mem of pf_run_frames* only: page-locked host result buffers (pf_host_alloc); the call
                                   * returns after enqueueing the device->host copies, results are complete after pf_sync() */
/* pf_run_frames_planted only: OR into `mem` when the frames are in host memory but the planted detector rows
 * (a test / benchmark instrument, 968 KB per frame) already live on the device */
enum { PF_MEM_ROWS_DEVICE = 0x100 };
enum { PF_NET_LANDMARK = 0, PF_NET_DETECTOR = 1, PF_NET_SLOTS = 4 };
enum { PF_INPUT_U8_NHWC = 0, PF_INPUT_F32_NCHW = 1 };
enum { PF_DTYPE_F16 = 0, PF_DTYPE_F32 = 1, PF_DTYPE_F32_SPLIT = 2 };  /* 2: f32 tensors, 3 x f16-MFMA split-precision convs */

/* library / build identification: "peppa-hip <version> gfx950" (or "... simt-emu" for the
 * CPU test build of the same sources, which only tests/ may load) */
const char* pf_version(void);

/* Create an engine bound to HIP device `device_id` (one stream, no networks loaded yet). */
int pf_create(int device_id, pf_handle** out);
void pf_destroy(pf_handle* h);
/* Last error message of the handle (or of pf_create when h == NULL). */
const char* pf_last_error(pf_handle* h);
/* Block until all work queued on the handle's stream has finished. */
int pf_sync(pf_handle* h);

/* Load a packed network program (built by peppa_pig_face_landmark_amd.graph) into `slot`
 * and size its activation arena for up to `max_batch` items.  Replaces
 * rt.InferenceSession(onnx_f) -- onnx_model_base.py:14. */
int pf_load_program(pf_handle* h, int slot, const void* blob, size_t bytes, int max_batch);

/* Landmark regressor forward == session.run of kps_student.onnx (face_landmark.py:48):
 * input  B crops, either uint8 NHWC [B][S][S][3] (channel order as given by the caller) or
 *        float32 NCHW [B][3][S][S] already divided by 255 (face_landmark.py:44-47);
 * output loc_fix [B][196] (x0,y0,...,x97,y97 normalised to the crop, model.py:549-552) and
 *        score [B][98] (raw heat-map maximum, model.py:522). */
int pf_landmark_forward(pf_handle* h, const void* input, int input_kind, int mem, int batch,
                        float* loc_fix, float* score, int out_mem);

/* Face attributes of the landmark network's fc head (Net.fc, model.py:269,286-293), for landmark programs built with
 * face_attrs=True: copies `rows` rows [rows][7] left by the handle's last pf_landmark_forward (rows = batch),
 * pf_landmarks* (box order; rows whose valid flag is 0 are left untouched), pf_run_frames* ([F][top_k], like kps),
 * pf_track_frame* (the n_out tracked faces, compacted like kps) or pf_track_streams ([n][top_k], compacted like kps).
 * raw = 1: Net.forward's x (x[0:3] head pose / 90, x[3:7] face-state logits); raw = 0: pose in degrees (90 x[0:3], about
 * x, y, z as cv2.decomposeProjectionMatrix returns them) then sigmoid(x[3:7]) = P(eye of points 60-67 closed), P(eye of
 * points 68-75 closed), P(mouth closed), P(mouth wide open).  Enqueued on the handle's stream (out_mem = PF_MEM_DEVICE)
 * or copied and synchronised (host memory).  Fails with a message when the program has no head, when the handle's last
 * call left no rows or when more rows are asked than it left. */
int pf_face_attrs(pf_handle* h, int rows, float* out, int raw, int out_mem);

/* Aligned face chips: the similarity warp of a face onto the public ArcFace five-point template, the normalised image that
 * recognition / liveness / attribute networks take, cut on the device from the frame and the 98 landmarks.  Arithmetic (the
 * specification, restated in numpy by tests/align_ref.py): five points in float64 -- the means of landmarks
 * 60..67 and 68..75 (the eye contours; not the pupils 96 / 97, which follow the gaze), 54 (nose tip), 76 and 82 (mouth corners) --
 * fitted to the template scaled by chip_size / 112 as a least-squares similarity without reflection, in closed form:
 * M = [[a, -b, tx], [b, a, ty]] maps frame to chip.  A slot is valid iff the fit is finite and a^2 + b^2 lies in [2^-12, 2^12].
 * Every chip pixel is the bilinear sample at M^-1 (x, y), the coordinate rounded to 1/1024 pixel and the blend done in integers
 * ((sum of tap * weight + 2^19) >> 20), taps outside the frame reading 0; channel order untouched.  No float64 operation is
 * contracted into an fma, so the bytes are the same on every machine.  LIMIT: there is no anti-alias pre-filter -- a face much
 * larger than the chip aliases exactly as cv2.warpAffine(INTER_LINEAR) would.  chip_size: a multiple of 16 in [32, 256].
 *
 * pf_align_faces is the stage-level entry (like pf_crop_faces): frames [F][H][W][3] packed (mem = PF_MEM_HOST, PF_MEM_DEVICE or
 * PF_MEM_RESIDENT -- then n_frames must be 1 and frames may be NULL); kps [F][top_k][98][2] float32 (kps_f64 = 0) or float64,
 * in host or device memory (kps_mem); counts [F] in the same memory as kps, slot k of frame f being live iff k < counts[f]
 * (NULL: all top_k slots).  Outputs in host or device memory (out_mem): chips [F][top_k][S][S][3], mats [F][top_k][2][3]
 * float64, valid [F][top_k] (0 for dead or degenerate slots, whose chip and matrix rows are left untouched, like the kps of
 * pf_landmarks); mats and valid may be NULL.  Device outputs are enqueued on the handle's stream, host outputs are copied and
 * synchronised. */
int pf_align_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                   const void* kps, int kps_f64, int kps_mem, const int* counts, int top_k, int chip_size,
                   uint8_t* chips, double* mats, int* valid, int out_mem);
/* The chips of the faces of the handle's last pipeline call, cut from the frame(s) and landmarks that call left on the device;
 * row semantics exactly those of pf_face_attrs: after pf_landmarks* box order (rows whose valid flag is 0 are dead), after
 * pf_run_frames* [F][top_k] with the device counts, after pf_track_frame* the n_out tracked faces with their smoothed float64
 * landmarks, after pf_track_streams [n][top_k] with out_lm / the counts, the frames read from the stream slots.  FRAME LIFETIME:
 * frames the call was given with mem = PF_MEM_DEVICE are read again here and must still be alive and unchanged; frames given from
 * host memory are read from the handle's staging copy, which the next call that stages a frame overwrites (that call then leaves
 * no rows).  Fails with a message after pf_landmark_forward (no frame), when the last call left no rows and when more rows are
 * asked than it left. */
int pf_face_chips(pf_handle* h, int rows, int chip_size, uint8_t* chips, double* mats, int* valid, int out_mem);

/* Face-region label maps: which pixels are face, and which part of the face, scan-converted on the device from the 98 landmarks
 * alone (no frame is read).  Arithmetic (the specification, restated in numpy by tests/mask_ref.py): eight
 * closed polygons over WFLW indices -- 1 face (0..32, 46..42, 37..33: jaw, then the upper brow lines backwards), 2 left brow
 * (33..41), 3 right brow (42..50), 4 left eye (60..67), 5 right eye (68..75), 6 nose (51, 55..59), 7 lips (76..87), 8 inner mouth
 * (88..95); a pixel's label is the highest-numbered region containing it, 0 where none does.  A slot is valid iff it is live (as for
 * the chips) and landmarks 0..95 are finite; the pupils 96 / 97 are not used.  Each coordinate is taken as float64, clamped to
 * [-65536, 65536] and rounded to 1/16 pixel, X = floor(16 x + 0.5); everything after is integer.  Even-odd rule, pixel centres at
 * integer coordinates, half-open edges: an edge (Xa, Ya)-(Xb, Yb) with Ya < Yb is active on row py iff Ya <= 16 py < Yb, its
 * threshold there is T = ceil((Xa (Yb - Ya) + (Xb - Xa)(16 py - Ya)) / (16 (Yb - Ya))), and (px, py) is inside a polygon iff the
 * number of its active edges with px < T is odd.  An axis-aligned rectangle with integer corners fills exactly x0 <= px < x1,
 * y0 <= py < y1; abutting polygons share no pixel; self-intersecting polygons are well defined.  LIMITS: hard edges, no feathering;
 * the face polygon stops at the upper brow line, so the forehead is not covered.
 *
 * chip_size = 0, frame space: labels [F][H][W] uint8, every byte written (background 0).  Where faces of a frame overlap, the
 * lowest valid slot that gives the pixel a non-zero label owns it.  owners (optional) [F][H][W] uint8: slot + 1, 0 for background;
 * needs top_k <= 255.  boxes (optional) [F][top_k][4] int32 x0, y0, x1, y1 = ceil(min X / 16), ceil(min Y / 16), ceil(max X / 16),
 * ceil(max Y / 16) over the 96 vertices, clipped to the frame: every pixel a face can own lies in x0 <= px < x1, y0 <= py < y1.
 * Box rows of invalid slots are left untouched.  valid (optional) [F][top_k], every slot.
 * chip_size = S (a multiple of 16 in [32, 256]), chip space: labels [F][top_k][S][S], one map per slot in the coordinates of that
 * face's chip -- each vertex goes through the matrix pf_align_faces computes for the same landmarks (the same function, the same
 * bits), ((a x - b y) + tx, (b x + a y) + ty) in float64 without fma contraction, before the clamp.  A slot is valid iff the
 * landmarks are finite and the fit is valid; maps of invalid slots are left untouched.  owners and boxes must be NULL; height and
 * width are ignored.
 *
 * pf_mask_faces is the stage-level entry: kps, kps_f64, kps_mem, counts and top_k as for pf_align_faces.  Device outputs
 * (out_mem = PF_MEM_DEVICE) are enqueued on the handle's stream without a read-back; host outputs are produced in the handle's
 * scratch, copied and synchronised. */
int pf_mask_faces(pf_handle* h, int n_frames, int height, int width, const void* kps, int kps_f64, int kps_mem, const int* counts,
                  int top_k, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem);
/* The maps of the faces of the handle's last pipeline call; row semantics and refusals exactly those of pf_face_chips.  In frame
 * space the maps cover ceil(rows / per_frame) frames of that call's frame size, per_frame being the call's top_k (after
 * pf_landmarks* its box count: one frame).  It reads the landmarks, counts and live flags the call left in the handle's own
 * buffers and NEVER a frame, so -- unlike pf_face_chips -- it also works after device frames the CALLER owns are gone.  The record
 * itself is dropped by the same calls that drop it for the chips (pf_set_frame, a call that stages new frames, pf_load_program of the
 * landmark slot): after those it fails like pf_face_chips.
 * pf_face_masks_shape is part of the feature: the frame-space maps take the frame size and per-frame slot count of the LAST CALL,
 * which pf_face_masks does not take as arguments, so a caller that sizes labels / owners from its own bookkeeping and gets it wrong
 * is written past the end.  It reports labels (and owners) [n_frames][height][width] for `rows` rows, with the refusals of
 * pf_face_masks (same record, same messages), and writes nothing else. */
int pf_face_masks(pf_handle* h, int rows, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem);
int pf_face_masks_shape(pf_handle* h, int rows, int* n_frames, int* height, int* width);

/* Face redaction (kernel redact_kernel, csrc/k_redact.h): out [F][H][W][3] packed BGR, EVERY byte written -- the
 * pixels the label maps above select are filled, pixelated or box-blurred, every other pixel is its input byte for byte.  The
 * arithmetic is specified exactly and is integer throughout, so every byte is reproducible.
 * Selection.  The frame-space labels, owners, boxes and valid of pf_mask_faces are computed from the same landmarks, counts and live
 * flags over ALL valid slots.  select (optional) [F][top_k] ints; NULL selects every slot.  Pixel (x, y) with label L and owner o is
 * selected iff (a) bit L of label_mask is set and (L == 0 or select == NULL or select[o - 1] != 0), or (b) label_mask has
 * PF_REDACT_BOX and some valid, selected slot with a clipped box x1 > x0, y1 > y0 has x0 - pad <= x < x1 + pad and
 * y0 - pad <= y < y1 + pad.  Bit 0 is the background, bits 1..8 the labels of pf_mask_faces.  An unselected face that owns a
 * pixel protects it from (a).
 * Value of a selected pixel, per channel, always from the INPUT frame (never from an already redacted pixel):
 *   PF_REDACT_FILL    byte c of colour (the low byte is channel 0); strength is ignored
 *   PF_REDACT_MOSAIC  strength = cell size 4, 8 or 16; cells are aligned to the frame origin; with n the in-frame pixels of the
 *                     pixel's cell (selected or not) and S their sum: (S + (n >> 1)) / n, integer division
 *   PF_REDACT_BLUR    strength = radius r in [1, 32]; the window [x - r, x + r] x [y - r, y + r] clipped to the frame, n its
 *                     pixel count, S its sum: (S + (n >> 1)) / n
 * frames, mem (host, device, or PF_MEM_RESIDENT with one frame), kps, kps_f64, kps_mem, counts and top_k as for pf_align_faces;
 * select lives in the memory of kps; valid (optional) [F][top_k] as for pf_mask_faces; pad in [0, 4096]; select needs top_k <= 255
 * (owners are bytes).  out must not alias the frames.  Device output (out_mem = PF_MEM_DEVICE) is enqueued on the handle's stream
 * without a read-back; host output is produced in the handle's scratch, copied and synchronised.  LIMITS: out of place only; no
 * cells of 32, no radius above 32, no Gaussian or iterated blur, hard edges; the forehead and hair only as far as PF_REDACT_BOX
 * with pad reaches. */
enum { PF_REDACT_FILL = 0, PF_REDACT_MOSAIC = 1, PF_REDACT_BLUR = 2 };
enum { PF_REDACT_BACKGROUND = 0x001, PF_REDACT_FACE_ALL = 0x1FE, PF_REDACT_BOX = 0x200 };
int pf_redact_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                    const void* kps, int kps_f64, int kps_mem, const int* counts, const int* select, int top_k,
                    int mode, int label_mask, int strength, int pad, unsigned colour,
                    uint8_t* out, int* valid, int out_mem);
/* The frames of the handle's last pipeline call, redacted: rows, refusals and messages exactly those of pf_face_chips (the per-stream
 * frame slots after pf_track_streams and a row stride other than 3 W included).  out is [ceil(rows / per_frame)][H][W][3], the shape
 * pf_face_masks_shape reports; select is [rows] in HOST memory.  It reads the frames again: device frames the CALLER owns must
 * still be alive and unchanged, as for pf_face_chips.  rows == 0 succeeds and writes nothing. */
int pf_face_redact(pf_handle* h, int rows, const int* select, int mode, int label_mask, int strength, int pad, unsigned colour,
                   uint8_t* out, int* valid, int out_mem);

/* Face overlay (kernels draw_prims_kernel / draw_kernel, csrc/k_draw.h): out [F][H][W][3] packed BGR, EVERY byte
 * written -- a disc on each of the 98 landmarks, the 103 contour edges of the label maps' regions as round-capped lines and the
 * outline of the clipped box, blended once onto a copy of the frame; every uncovered pixel is its input byte for byte.  The rule is
 * exact and integer on the Q4 vertices of pf_mask_faces (all 98 landmarks; a pupil that is not finite is not drawn), with
 * P = (16 px, 16 py) the centre of pixel (px, py):
 *   disc (C, R)       covers P iff |P - C|^2 <= R^2
 *   PF_DRAW_POINTS    landmark i: the disc of R = 16 point_radius; colour_hi iff scores == NULL or scores[i] > score_thres in float32
 *                     (NaN and equality are lo), else colour_lo
 *   PF_DRAW_CONTOURS  edge A -> B of the region table, d = B - A, q = P - A, w = line_width: covered iff d.d > 0 and 0 <= q.d <= d.d and
 *                     (q x d)^2 <= 64 w^2 d.d, or a disc of R = 8 w about A or B covers P
 *   PF_DRAW_BOX       the clipped box (x0, y0, x1, y1) of pf_mask_faces, if x1 > x0 and y1 > y0: x0 - w <= px < x1 + w and
 *                     y0 - w <= py < y1 + w and not inside the box
 * Among the primitives that cover a pixel the lowest valid slot wins, within it points beat contours beat the box, among points the
 * highest index.  Exactly one colour c is applied, once: (in (256 - alpha) + c alpha + 128) >> 8 per channel (low byte of a colour =
 * channel 0).  frames, mem, kps, kps_f64, kps_mem, counts, top_k, valid and out_mem as for pf_redact_faces; scores (optional)
 * [F][top_k][98] float32 in the memory of kps.  out must not alias the frames.  LIMITS: out of place only, hard edges, no text. */
#define PF_DRAW_POINTS   1
#define PF_DRAW_CONTOURS 2
#define PF_DRAW_BOX      4
typedef struct pf_draw_style {
    int what;              /* bits above, at least one */
    int point_radius;      /* r, 1..16 pixels */
    int line_width;        /* w, 1..16 pixels: contours and box */
    int alpha;             /* a, 1..256; 256 = opaque */
    float score_thres;     /* a point is "hi" iff scores given and score > score_thres; scores NULL: all hi */
    unsigned colour_hi, colour_lo, colour_contour, colour_box;   /* low byte = channel 0, as pf_redact_faces */
} pf_draw_style;
int pf_draw_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                  const void* kps, int kps_f64, int kps_mem, const int* counts, const float* scores, int top_k,
                  const pf_draw_style* style, uint8_t* out, int* valid, int out_mem);
/* The frames of the handle's last pipeline call with its faces drawn: rows, refusals and messages those of pf_face_redact.  scores
 * (optional) is [rows][98] in HOST memory.  base (optional) is a DEVICE pointer to [ceil(rows / per_frame)][H][W][3] packed frames
 * drawn on in place of the frames of the last call (pf_face_redact to the device, then this); it must not alias out.  rows == 0
 * succeeds and writes nothing.  The record of the last call is left alone. */
int pf_face_draw(pf_handle* h, int rows, const float* scores, const pf_draw_style* style,
                 const uint8_t* base, uint8_t* out, int* valid, int out_mem);

/* Per-face region statistics (kernel face_stats_kernel, csrc/k_stats.h): a face turned into numbers about its
 * pixels.  Everything is an exact integer sum, so every value is reproducible whatever the order of addition.
 * The frame-space labels, owners, boxes and valid of pf_mask_faces are computed from the same landmarks, counts and live flags over
 * ALL valid slots.  For frame pixel (x, y) with bytes c0, c1, c2 (BGR: channel 0 = B):
 *   luma        Y = (29 c0 + 150 c1 + 77 c2 + 128) >> 8, in 0..255; a grey pixel of value v has Y = v
 *   Laplacian   Lap = 4 Y(x, y) - Y(x-1, y) - Y(x+1, y) - Y(x, y-1) - Y(x, y+1); neighbour coordinates are clamped to the FRAME (edge
 *               replication) and neighbours are read from the frame whatever their label or owner
 *   dark iff Y <= dark, bright iff Y >= bright, with 0 <= dark < bright <= 255
 * For slot k and label L in 1..8, over the pixels with owner == k + 1 and label == L, PF_STATS_FIELDS = 9 unsigned 64-bit values:
 *   0 n   1 sum c0   2 sum c1   3 sum c2   4 sum Y   5 sum Y^2   6 sum Lap^2   7 number of dark pixels   8 number of bright pixels
 * stats [F][top_k][8][9] uint64 (row L - 1 is label L); valid (optional) [F][top_k] as for pf_mask_faces.  Rows of invalid slots are
 * left untouched, as for the chips; a valid slot that owns no pixel gets 72 zeros.  Owners are bytes, so top_k <= 255 (after
 * pf_landmarks* at most 255 boxes) is required and refused otherwise.  frames, mem (host, device, or PF_MEM_RESIDENT with one frame),
 * kps, kps_f64, kps_mem, counts and top_k as for pf_redact_faces.  Device output (out_mem = PF_MEM_DEVICE, stats 8-byte aligned) is
 * enqueued on the handle's stream without a read-back; host output is produced in the handle's scratch, copied and synchronised.
 * LIMITS: frame space only, no statistics of the chip; the maps are computed again when masks or a redaction are asked in the same
 * step; sum Lap^2 / n is per FRAME pixel and therefore falls as a face grows; the face polygon stops at the upper brow line (no
 * forehead); hard edges. */
#define PF_STATS_FIELDS 9
int pf_measure_faces(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                     const void* kps, int kps_f64, int kps_mem, const int* counts, int top_k, int dark, int bright,
                     uint64_t* stats, int* valid, int out_mem);
/* The faces and frames of the handle's last pipeline call, measured: rows, refusals and messages those of pf_face_redact (the
 * per-stream frame slots after pf_track_streams and a row stride other than 3 W included).  stats is [rows][8][9], valid [rows].  It
 * reads the frames again: device frames the CALLER owns must still be alive and unchanged.  rows == 0 succeeds and writes nothing.
 * The record of the last call is left alone. */
int pf_face_stats(pf_handle* h, int rows, int dark, int bright, uint64_t* stats, int* valid, int out_mem);

/* Detector forward == session.run of yolov5n-0.5.onnx (face_detector.py:29-31):
 * input float32 NCHW [1][3][384][640] RGB/255 or uint8 NHWC letterboxed RGB;
 * output [rows][16] decoded rows (cx,cy,w,h,obj,10 landmark coords,cls), rows = 15120 at 384x640. */
int pf_detector_forward(pf_handle* h, const void* input, int input_kind, int mem, int batch,
                        float* rows_out, int out_mem);

/* Debug / parity tap: copy activation tensor `tensor_id` of the program in `slot` (as left by
 * the last forward of `batch` items) to host float32 NHWC [batch][H][W][C]. */
int pf_read_tensor(pf_handle* h, int slot, int tensor_id, int batch, float* out_host, size_t out_elems);

/* FaceDetector.__call__ (face_detector.py:23-42): BGR uint8 frame -> kept detections
 * [n][16] in frame coordinates (cols 0:4 xyxy, col 4 score), at most max_n rows, in keep order. */
int pf_detect(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
              float score_thres, float iou_thres, float* boxes, int max_n, int* n_out);

/* FaceLandmark.__call__ (face_landmark.py:33-64): for each of n boxes (xyxy, float32 [n][4])
 * crop (zero pad, square 1.4*w box), resize to the network size, run the regressor, map the
 * landmarks back to frame coordinates.  kps [n][98][2], scores [n][98], valid[n] = 0 for boxes
 * the reference rejects (w or h <= 20 px, face_landmark.py:76-77) -- those rows are left untouched. */
int pf_landmarks(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                 const float* boxes, int n, float* kps, float* scores, int* valid);
/* Same for float64 box rows.  On tracked video frames FaceAna hands FaceLandmark a float64 array (track_box comes out of
 * the float64 EMA / One-Euro arithmetic, facer.py:66-81, lk.py:19-56), and then every step of preprocess
 * (face_landmark.py:74-93: widths, `bbox += add`, `// 2`, the store-back, astype(int32)) is float64 arithmetic: rounding
 * the boxes to float32 first can move a floor division across an integer and shift the crop by one pixel. */
int pf_landmarks_f64(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                     const double* boxes, int n, float* kps, float* scores, int* valid);

/* Batched FaceAna.run()+reset() (facer.py:52-85 without tracking, demo.py:83-86) over F frames
 * of identical size resident in `frames` ([F][H][W][3] BGR): detect -> NMS -> drop area <=
 * min_face, keep top_k by area (facer.py:120-142) -> landmarks.  Outputs (host or device per
 * out_mem): counts[F], boxes [F][top_k][4], kps [F][top_k][98][2], scores [F][top_k][98]. */
int pf_run_frames(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                  float score_thres, float iou_thres, float min_face, int top_k,
                  int* counts, float* boxes, float* kps, float* scores, int out_mem);

/* Same stages as pf_run_frames but detections are supplied by the caller (planted-candidate
 * protocol): det_rows is the decoded detector output [F][rows][16] in letterboxed
 * coordinates; everything downstream (xywh2xyxy, NMS, un-letterbox, top-k, landmarks) runs on
 * the device.  det_rows lives where `frames` lives (host or device, per `mem`).  When a detector program
 * is loaded, letterbox + detector network + decode still run (their cost stays in the call) and only their
 * output is replaced by det_rows.  det_rows == NULL means "use the detector's own rows" (== pf_run_frames).
 * Device-side outputs (out_mem == PF_MEM_DEVICE) are complete after pf_sync(). */
int pf_run_frames_planted(pf_handle* h, const uint8_t* frames, int mem, int n_frames, int height, int width,
                          const float* det_rows, int rows, float score_thres, float iou_thres,
                          float min_face, int top_k,
                          int* counts, float* boxes, float* kps, float* scores, int out_mem);

/* Stage-level entry points (each is one reference function on its own; the parity tests check
 * them bit-for-bit against the numpy/OpenCV restatement):
 *  pf_letterbox   == FaceDetector.preprocess up to the float conversion (face_detector.py:45-63):
 *                    BGR frame -> RGB uint8 [out_h][out_w][3] letterboxed with 114; info = scale,left,top
 *  pf_nms_rows    == xywh2xyxy + py_nms + scale_coords (face_detector.py:31-37,73-136) on decoded
 *                    rows [R][16] (host); kept rows (xyxy in frame coords) in keep order
 *  pf_crop_faces  == FaceLandmark.preprocess (face_landmark.py:66-104): crops uint8 [n][S][S][3] and
 *                    params [n][8] = valid, add, x0, y0, xs, ys, w_crop, h_crop */
int pf_letterbox(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                 int out_h, int out_w, uint8_t* out_host, float* info3);
/* cv2.resize(img, (out_w, out_h)) with the default INTER_LINEAR on a uint8 HxWx3 image (channel order untouched), the same
 * fixed-point arithmetic as the letterbox / crop kernels.  Used by the WFLW evaluation harness (tools/eval_wflw.py), whose
 * reference counterpart resizes an aspect-changing crop (TRAIN/face_landmark/tools/eval_WFLW.py:123). */
int pf_resize(pf_handle* h, const uint8_t* img, int mem, int height, int width, int row_stride,
              int out_h, int out_w, uint8_t* out_host);
int pf_nms_rows(pf_handle* h, const float* rows_host, int n_rows, float scale, float left, float top,
                float score_thres, float iou_thres, float* kept, int max_n, int* n_out);
int pf_crop_faces(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                  const float* boxes, int n, int out_size, uint8_t* crops_host, int* params_host);
int pf_crop_faces_f64(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                      const double* boxes, int n, int out_size, uint8_t* crops_host, int* params_host);   /* float64 rows, see pf_landmarks_f64 */

/* Video mode (FaceAna.run on a stream, facer.py:52-85): upload the frame ONCE, keep it resident for the
 * following pf_detect / pf_landmarks calls (pass mem = PF_MEM_RESIDENT), and evaluate the frame-difference
 * gate of FaceAna.diff_frames (facer.py:98-118) on the device against the previous resident frame:
 * *abs_diff_sum = sum |prev - cur| over all H*W*3 bytes (the caller divides by H*W*3 and compares with 5),
 * *has_prev = 0 when there is no previous frame of the same shape.  row_stride must equal 3*width.
 * pf_forget_frames == FaceAna.reset() for the resident frames (facer.py:200-208). */
int pf_set_frame(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                 unsigned long long* abs_diff_sum, int* has_prev);
int pf_forget_frames(pf_handle* h);

/* Frame ingest: cv2.imread(path) for JPEG files (demo.py:76) without the host-side decode and the
 * upload of a 6 MB frame.  Single-scan baseline files -- what cameras and cv2.imwrite produce -- are entropy-decoded on the
 * DEVICE: the host strips the byte stuffing, the Huffman stream (~0.1 byte per pixel) crosses PCIe and is decoded as
 * self-synchronising 1024-bit sub-sequences (or one thread per restart interval when the file carries restart markers, see
 * below).  Other files (several scans, table ids above 1, tiny images) are Huffman-decoded on the host and their 16-bit
 * coefficient records go up through page-locked memory.  Dequantisation, inverse DCT, chroma upsampling and YCbCr->BGR run as
 * kernels either way, bit-identical with libjpeg(-turbo)'s default decoder (JDCT_ISLOW, fancy upsampling), i.e. with what
 * cv2.imread returns.  A stream whose sub-sequences do not settle within the queued rounds is decoded again on the host.  The frame (packed BGR, 3*width bytes per row) stays in device memory owned by the handle until
 * the decode after the next one; *d_bgr is that pointer -- hand it to pf_set_frame / pf_detect / pf_landmarks / pf_run_frames /
 * pf_track_frame with mem = PF_MEM_DEVICE.  bgr_host (may be NULL): host copy for drawing, height*width*3 bytes (sizes from
 * pf_jpeg_info).  Supported: 8-bit baseline / extended-sequential Huffman JPEG, greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
 * restart markers; progressive, arithmetic-coded, 12-bit, CMYK / Adobe-RGB files and other sampling grids are refused with an
 * error (decode those with the host library).  subsampling: 0 grey, 444, 422 or 420. */
int pf_jpeg_info(const uint8_t* jpeg, size_t bytes, int* height, int* width, int* components, int* subsampling);
int pf_decode_jpeg(pf_handle* h, const uint8_t* jpeg, size_t bytes, int* height, int* width, const uint8_t** d_bgr,
                   uint8_t* bgr_host);
/* n files of one size and sampling -> [n][height][width][3] in device memory (*d_frames, same ownership), ready for
 * pf_run_frames(mem = PF_MEM_DEVICE): the files' Huffman streams are decoded on `threads` host threads (one file per task), the
 * device stages run once over the whole batch.  Files that carry restart markers (one interleaved scan, table ids 0 / 1) in batches
 * of >= 4096 restart intervals skip the host Huffman loop: one device thread per interval decodes the stream, and only the
 * compressed scan crosses PCIe; files WITHOUT restart markers always take the device's sub-sequence decoder
 * (pf_set_option(PF_OPT_JPEG_ENTROPY, 1 | 2) overrides either choice).  If that decoder does not settle, this asynchronous call cannot decode
 * again by itself: the next synchronising call on the handle fails with "did not synchronise" and the batch has to be resubmitted
 * after pf_set_option(PF_OPT_JPEG_ENTROPY, 1) -- the Python shim's Engine.run_jpeg_files() does that and repeats the pipeline
 * call that consumed the frames (ordinary photographs settle in the first rounds; PF_OPT_JPEG_SYNC_ROUNDS queues fewer
 * rounds than the default 10 -- that can only make the decoder give up sooner, i.e. fall back or report, never return different
 * pixels).  Asynchronous like pf_run_frames: the frames are valid in the order of the
 * handle's stream (pf_run_frames on the same handle just works; pf_sync before another stream reads them).  Two buffer sets
 * alternate, so the pointer of call k stays valid until call k + 2 and the host work of call k + 1 overlaps the pipeline still
 * running on the frames of call k. */
int pf_decode_jpeg_batch(pf_handle* h, int n, const uint8_t* const* jpegs, const size_t* sizes, int threads, int* height,
                         int* width, const uint8_t** d_frames);

/* The forward direction: n packed BGR images of one size -> n complete baseline JFIF files, written by device kernels
 * (csrc/k_jpeg_enc.h).  Every byte is what libjpeg(-turbo) writes for the same quality and sampling without its optimisation
 * pass and with one restart interval per MCU row (Pillow: save(quality=q, subsampling=s, restart_marker_rows=1)); the numpy
 * restatement is tests/jpeg_enc_ref.py, the prose INTEGRATION.md 4g.  Integers throughout:
 *   colour     F(x) = int(x 65536 + .5): Y = (F(.299) R + F(.587) G + F(.114) B + 32768) >> 16,
 *              Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16,
 *              Cr = (F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16 (arithmetic shifts; byte 0 of a pixel is B)
 *   planes     luma is sampled 1x1 (444), 2x1 (422) or 2x2 (420) against chroma.  The converted plane repeats its last column and
 *              its last row up to the component's blocks; chroma is then averaged, 2x2: (a + b + c + d + bias) >> 2 with bias
 *              1, 2, 1, 2 .. along the output columns, 2x1: (a + b + bias) >> 1 with bias 0, 1, 0, 1 ..; then the last down-sampled
 *              row repeats to a multiple of 8 rows
 *   DCT        libjpeg's "islow" forward DCT on sample - 128 (13-bit constants, row pass scaled by 4, column pass descaled), the
 *              forward twin of the decoder's
 *   quantiser  ITU T.81 K.1 / K.2 scaled as libjpeg scales them (s = 5000 / q below 50, else 200 - 2 q; (base s + 50) / 100 clamped
 *              to 1 .. 255); with d = 8 Q the coefficient is sign(c) ((|c| + (d >> 1)) / d)
 *   blocks     a luma block an MCU needs beyond the image's blocks has no AC and the DC of the block coded before it in the MCU
 *   entropy    one interleaved scan (ids 1, 2, 3), the standard Huffman tables K.3 - K.6, restart interval = one MCU row: at its
 *              end the bits are padded with ones, RSTm follows (m counts modulo 8; EOI behind the last), DC predictions return to 0
 *   file       SOI, APP0 (JFIF 1.1, density 1 x 1), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, DRI, SOS, the scan, EOI
 * So the rows of MCUs are independent on the device, and pf_decode_jpeg* takes the files on its restart-interval path.
 *
 * Image i starts at images + i * height * row_stride, row_stride >= 3 * width with any alignment; mem = PF_MEM_HOST, PF_MEM_DEVICE
 * or PF_MEM_RESIDENT (then n = 1 and images may be NULL).  quality 1 .. 100, subsampling 444, 422 or 420 (the values pf_jpeg_info
 * reports), height and width 1 .. 65535.  File i goes to out + i * capacity and sizes[i] is its length.  A file that does not fit
 * its slot leaves sizes[i] = -(bytes needed); the call still succeeds, the content of that slot is unspecified, no byte outside the
 * slot is touched and no other image is affected.  Where it fits, exactly sizes[i] bytes are written and the rest of the slot is
 * untouched.  out_mem = PF_MEM_DEVICE: out and sizes are device memory and everything is enqueued on the handle's stream without
 * a read-back; PF_MEM_HOST: the files are copied and the call synchronises.  The call is never captured into a graph and leaves the
 * record of the handle's last call alone, so pf_face_chips / pf_face_redact (out_mem = PF_MEM_DEVICE) followed by pf_encode_jpeg
 * (mem = PF_MEM_DEVICE) on the same handle compose without a synchronisation.
 *
 * Scratch (coefficients: 128 bytes per block; the bit stream at its longest: about 208 bytes per block; the intervals' lengths)
 * belongs to the handle.  Calls run in internal chunks of images whose scratch stays below PF_JPEG_ENC_SCRATCH = 256 MiB, except that
 * one image always runs whole (4:2:0: about 8 bytes per pixel, 4:4:4: about 16).  Images whose pf_encode_jpeg_bound exceeds 2^31 - 1
 * (about 220 megapixels in 4:2:0, 110 in 4:4:4) are refused.
 *
 * pf_encode_jpeg_bound: a capacity no image of that shape can exceed, 0 for arguments pf_encode_jpeg refuses.  Derivation: a block is
 * at most 22 + 63 * 26 = 1660 bits (longest DC code 11 bits + 11 value bits; 63 coefficients of the longest AC code, 16 bits, + 10
 * value bits); an interval is its blocks (MCUs of a row x (hs vs + 2)), padded to a byte, every byte stuffed (x 2), + 2 bytes of RSTm
 * or EOI; the header is 629 bytes.  Generous by a factor of tens for photographs: allocate 3 * height * width and call again with
 * the bound only where a size comes back negative. */
int pf_encode_jpeg(pf_handle* h, const uint8_t* images, int mem, int n, int height, int width, int row_stride, int quality,
                   int subsampling, uint8_t* out, size_t capacity, int* sizes, int out_mem);
size_t pf_encode_jpeg_bound(int height, int width, int subsampling);
/* Device memory on the handle's device for callers without a HIP runtime of their own (the Python classes keep the device outputs of
 * pf_face_redact / pf_face_chips in it, which pf_encode_jpeg then reads).  pf_device_free synchronises the handle's stream first. */
int pf_device_alloc(pf_handle* h, size_t bytes, void** out);
int pf_device_free(pf_handle* h, void* p);

/* FaceAna.run(image) / reset() for ONE video stream with the tracking state on the device.  The
 * reference keeps track_box, the previous landmark sets and their displacement on the host and walks the boxes through
 * numpy between the two networks (judge_boxs facer.py:144-189, sort_and_filter :120-142, GroupTrack.calculate + the
 * One-Euro filter core/smoother/lk.py:19-56,117-149, hull boxes facer.py:70-81).  Here all of it is device kernels over
 * device state (float64, as the reference computes it under its pinned numpy): per frame the host reads back 8 bytes (the
 * frame-difference sum that gates the detector, facer.py:98-118) and the results.  One handle = one stream; shard streams,
 * never one stream, across handles / GPUs (several streams on one handle: pf_track_streams below).  Outputs: *n_out faces (<= top_k); boxes [n][4] = the new track boxes, kps
 * [n][98][2] = the smoothed landmarks (both float64), scores [n][98]; *detector_ran says whether the gate ran the detector.
 * track_iou_thres / smooth_box = Skps.yml Trace.iou_thres / Trace.smooth_box, diff_thres = 5 in the reference. */
int pf_track_frame(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                   float score_thres, float nms_iou_thres, float min_face, int top_k,
                   float track_iou_thres, float smooth_box, float diff_thres, int reserved,
                   int* n_out, double* boxes, double* kps, float* scores, int* detector_ran);
int pf_track_reset(pf_handle* h);
/* Same with the decoded detector rows supplied by the caller whenever the gate runs the detector (planted-candidate
 * protocol of pf_run_frames_planted: the network still runs, its output is replaced).  Test / benchmark instrument. */
int pf_track_frame_planted(pf_handle* h, const uint8_t* bgr, int mem, int height, int width, int row_stride,
                           const float* det_rows, int rows, float score_thres, float nms_iou_thres, float min_face, int top_k,
                           float track_iou_thres, float smooth_box, float diff_thres,
                           int* n_out, double* boxes, double* kps, float* scores, int* detector_ran);

/* N independent video streams on one handle (one camera feed = one stream): state of stream s lives in slot s
 * (0 <= s < max_streams), each slot holding the tracking state of pf_track_frame plus the stream's previous frame.
 * (Re)allocates the pool and forgets every stream.  Independent of pf_track_frame's own stream on the same handle. */
int pf_track_streams_config(pf_handle* h, int max_streams, int top_k);
/* One FaceAna.run() per listed stream: frames [n][height][width][3] packed BGR (mem = PF_MEM_HOST or PF_MEM_DEVICE),
 * frame i belongs to stream stream_ids[i] (distinct within a call; a stream absent from a call keeps its state and its
 * previous frame).  Per stream the semantics are those of pf_track_frame on its own handle, including a frame whose size
 * differs from the stream's previous frame counting as "no previous frame"; all frames of one call share one size.
 * det_rows: NULL = the detector's own rows, else planted decoded rows [n][rows][16], used only for the frames whose gate
 * runs the detector (test / benchmark instrument, as in pf_run_frames_planted).  The gate of all n frames is one kernel
 * and one read-back; the detector runs once on the frames whose gate opened, the landmark stage once on n x top_k slots.
 * Needs n <= max_streams, n <= the detector program's max_batch and n * top_k <= the landmark program's max_batch.
 * Outputs (host): counts[n], boxes [n][top_k][4] f64, kps [n][top_k][98][2] f64, scores [n][top_k][98] f32 (rows
 * beyond counts[i] are undefined), detector_ran[n]; boxes / kps / scores / detector_ran may be NULL.  A rejected call
 * (bad ids, sizes, no pool) changes no stream.  If the range guard fails the call, every stream of the call is reset
 * (the others keep their state) and the error names the program slot.  Never captured into a hipGraph. */
int pf_track_streams(pf_handle* h, int n, const int* stream_ids, const uint8_t* frames, int mem, int height, int width,
                     const float* det_rows, int rows, float score_thres, float nms_iou_thres, float min_face,
                     float track_iou_thres, float smooth_box, float diff_thres,
                     int* counts, double* boxes, double* kps, float* scores, int* detector_ran);
/* FaceAna.reset() of one stream (stream_id >= 0) or of all (-1). */
int pf_track_streams_reset(pf_handle* h, int stream_id);

/* Persistent face ids (kernel track_ident_kernel, csrc/k_track.h): which row of frame t is which row of frame
 * t - 1, as an integer id per output row of pf_track_frame* / pf_track_streams.  Off unless pf_track_ids_config switches it on; the
 * results of the tracking calls are bit-identical either way and the calls gain no synchronisation.  The rule is exact and integer.
 * State per stream, on the device: id[r] and age[r] for the rows r of the track boxes (row r of the previous call's output is row r
 * of the track boxes); a counter next_id (the first id is 1, 0 means "no id"); a lost list of at most 64 entries in insertion order,
 * each (id, age, box[4] float64, gone).  Per frame of a stream, with keep_lost in [0, 255]:
 *   1. Source of a selected row.  On a detector frame the source of selected row q is the previous row j that judge_boxs smoothed
 *      its detection with: the first j with IoU > track_iou_thres; no source if there was no match or no track.  The weight w of the
 *      claim is that IoU, as the judge computed it in that frame's dtype, held as a double.  On a gated (non-detector) frame selected
 *      row q is row k of the track boxes: its source is k, and no two rows can share it.  A previous row whose id is 0 passes on no
 *      source.
 *   2. Output rows are the selected rows the landmark stage accepted, compacted in order.
 *   3. Conflicts.  If several output rows have the same source j, the one with the greatest w keeps it; on equal w the lowest output
 *      row keeps it.  The others have no source.
 *   4. A row with source j gets id = id_prev[j] and age = age_prev[j] + 1.
 *   5. Rows without a source, in ascending output-row order.  If keep_lost > 0, the row's new track box (its row of the track boxes
 *      after this frame's hull judge, stored as float64) is compared with the box of every lost entry no earlier row has claimed: the
 *      IoU of judge_boxs in float64 with no FMA contraction.  The entry with the greatest IoU > track_iou_thres is taken, ties go to
 *      the lowest entry index; the row gets that entry's id and age + 1, and the entry is removed.  With no such entry, or with
 *      keep_lost == 0, the row gets id = next_id++ and age = 1.
 *   6. Lost list update, in this order: claimed entries are removed, compacting stably; every remaining entry gets gone += 1; entries
 *      with gone > keep_lost are dropped; every previous row with id != 0 that no output row kept is appended with its previous track
 *      box and gone = 1, in ascending previous-row order (rows unmatched on a detector frame, filtered by min_face or top_k, rejected
 *      by the crop stage, or the loser's source in step 3); while more than 64 entries remain, the entry with the greatest gone is
 *      dropped, ties drop the earliest inserted.  With keep_lost == 0 the list stays empty.
 * So a face absent from up to keep_lost consecutive frames comes back with its id.
 * Lifetime.  pf_track_reset, pf_track_streams_reset and the range-guard reset of a failed call forget id, age and the lost list of
 * the streams they reset and leave next_id alone: an id is never reused within the lifetime of a pool.  Reallocating a pool
 * (pf_track_streams_config, pf_track_frame growing top_k) restarts its counters at 1.  Ids are per stream: unique across streams is
 * (stream, id).
 * LIMITS: geometric identity only (IoU, no appearance): two people who swap places behind an occlusion swap ids; 64 lost entries;
 * ids for at most 64 faces per frame: with ids on, pf_track_frame* and pf_track_streams_config refuse a top_k above 64, and
 * pf_track_ids_config refuses to switch ids on while a pool has one; each refuses before it changes anything.
 *
 * pf_track_ids_config: both pools of the handle (pf_track_frame's and pf_track_streams'); enabling, disabling or changing keep_lost
 * forgets the identity state of both (ids restart at 1) and leaves the tracking state alone; keep_lost outside [0, 255] is refused.
 * pf_track_ids: ids and ages of the rows of the handle's last tracking call, counted as pf_face_chips counts them ([n] after
 * pf_track_frame, [n][top_k] after pf_track_streams; rows beyond a frame's count are 0); out_mem PF_MEM_HOST (the copies the call
 * itself brought back: no device traffic) or PF_MEM_DEVICE (enqueued on the handle's stream); either pointer may be NULL.  Refused
 * when the last call left no rows or was not a tracking call, when ids are off, or when rows exceeds what the call left. */
int pf_track_ids_config(pf_handle* h, int enable, int keep_lost);
int pf_track_ids(pf_handle* h, int rows, int* ids, int* ages, int out_mem);

/* Frame ingest (replaces the pageable numpy arrays cv2.imread / VideoCapture.read hand to
 * FaceAna.run, demo.py:13-17,76): page-locked host memory for frame batches (decode straight into it) and for
 * results.  Frames passed with mem = PF_MEM_HOST from such a buffer are copied host->device asynchronously on the
 * handle's stream, so with two handles (two streams) one batch's PCIe transfer overlaps the other batch's kernels;
 * from pageable memory the same call still works but the copy serialises.  Not tied to a handle. */
int pf_host_alloc(size_t bytes, void** out);
int pf_host_free(void* p);

/* Multi-GPU: frames shard across ranks -- frame f is processed by rank f mod R, each rank owning one GPU
 * and one handle -- and nothing on the data path crosses GPUs.  The one exchange is the start-up broadcast of the packed
 * network programs from rank 0 over RCCL / xGMI (the reference has no inference-side parallelism at all,
 * face_landmark.py:40-48; its only collectives are the DDP training all-reduces, net_work.py:30,131-137).
 *  pf_comm_unique_id     rank 0: a fresh 128-byte RCCL unique id (ncclGetUniqueId); the caller hands it to the
 *                        other ranks by whatever side channel launched them (env, file, torch.distributed store)
 *  pf_broadcast_weights  collective over all `world` ranks: creates the communicator on first use
 *                        (ncclCommInitRank on the handle's device), broadcasts rank 0's `blob` (*bytes long; other
 *                        ranks pass a buffer of `capacity` bytes and get the size back in *bytes) HBM-to-HBM with
 *                        ncclBroadcast on the handle's stream, then loads it into `slot` exactly like
 *                        pf_load_program on every rank.  *bcast_ms = device time of the payload broadcast.
 *                        world == 1 is valid (degenerates to pf_load_program through the same code path).
 * librccl is bound at the first call (dlopen); a missing library fails that call, not the engine. */
#define PF_COMM_ID_BYTES 128
int pf_comm_unique_id(void* id_out, size_t id_bytes);
int pf_rccl_version(int* version);
int pf_broadcast_weights(pf_handle* h, const void* rccl_unique_id, int rank, int world, int slot,
                         void* blob, size_t capacity, size_t* bytes, int max_batch, float* bcast_ms);
int pf_comm_destroy(pf_handle* h);

/* ---- multi-lane batch runner ---------------------------------------------------------------------------------------------
 * FaceAna.run() is a per-frame call (Skps/core/api/facer.py:52-85) and the reference never wrote a batch path
 * (face_landmark.py:119).  A pf_batch owns `lanes` engines -- one HIP stream, one activation arena and one graph cache
 * each -- on ONE device and hands every call's frames to them as contiguous slices (lane i: frames [i * ceil(F / lanes), ...)),
 * so the small kernels of one lane's detector overlap the large landmark kernels of the others.  This is the configuration
 * bench.py measures (three lanes of 32 frames).  Semantics and argument meaning of pf_batch_run_frames are those of
 * pf_run_frames_planted (det_rows == NULL: the detector's own rows); outputs cover all n_frames in frame order.  With
 * out_mem == PF_MEM_DEVICE / PF_MEM_HOST_PINNED the call returns after enqueueing (results complete after pf_batch_sync);
 * with PF_MEM_HOST it synchronises.  pf_batch_lane() exposes a lane's handle (owned by the batch) for pf_profile_* and
 * the stage-level entry points; max_batch_per_lane of pf_batch_load_program bounds the frames (detector slot) / faces
 * (landmark slot) of ONE lane's slice; the front engine's detector copy is sized for lanes x that many frames. */
typedef struct pf_batch pf_batch;
int pf_batch_create(int device_id, int lanes, pf_batch** out);
void pf_batch_destroy(pf_batch* b);
const char* pf_batch_last_error(pf_batch* b);
int pf_batch_lanes(pf_batch* b);
pf_handle* pf_batch_lane(pf_batch* b, int lane);
/* the engine that runs the detector + NMS half of a call for all lanes (PF_OPT_BATCH_FRONT; owned by the batch) -- for pf_profile_* */
pf_handle* pf_batch_front(pf_batch* b);
int pf_batch_load_program(pf_batch* b, int slot, const void* blob, size_t bytes, int max_batch_per_lane);
int pf_batch_set_option(pf_batch* b, int option, int value);
int pf_batch_sync(pf_batch* b);
int pf_batch_run_frames(pf_batch* b, const uint8_t* frames, int mem, int n_frames, int height, int width,
                        const float* det_rows, int rows, float score_thres, float iou_thres, float min_face, int top_k,
                        int* counts, float* boxes, float* kps, float* scores, int out_mem);

/* pf_face_attrs of the lanes, gathered: the [n_frames][top_k][7] attribute rows of the last pf_batch_run_frames (front mode
 * on or off), laid out like its kps.  Device output is enqueued on the lanes' streams. */
int pf_batch_face_attrs(pf_batch* b, int rows, float* out, int raw, int out_mem);
/* pf_face_chips of the lanes, gathered the same way: chips [n_frames][top_k][S][S][3] (mats, valid alike) of the last
 * pf_batch_run_frames, front mode on or off.  Device-resident frames of that call must still be alive. */
int pf_batch_face_chips(pf_batch* b, int rows, int chip_size, uint8_t* chips, double* mats, int* valid, int out_mem);
/* pf_face_masks of the lanes, gathered the same way: in frame space labels (owners) [n_frames][H][W] of the last
 * pf_batch_run_frames, each lane filling the maps of its own frames; boxes, valid and the chip-space maps laid out like its kps. */
int pf_batch_face_masks(pf_batch* b, int rows, int chip_size, uint8_t* labels, uint8_t* owners, int* boxes, int* valid, int out_mem);
/* the shape query of pf_face_masks_shape for the lanes' gathered maps */
int pf_batch_face_masks_shape(pf_batch* b, int rows, int* n_frames, int* height, int* width);
/* pf_face_redact of the lanes, gathered the same way: out [n_frames][H][W][3] of the last pf_batch_run_frames (the shape
 * pf_batch_face_masks_shape reports), each lane writing the frames it ran, front mode on or off; select [rows] in host memory, valid
 * laid out like its kps.  Device-resident frames of that call must still be alive. */
int pf_batch_face_redact(pf_batch* b, int rows, const int* select, int mode, int label_mask, int strength, int pad, unsigned colour,
                         uint8_t* out, int* valid, int out_mem);
/* pf_face_draw of the lanes, gathered the same way: each lane draws the frames it ran, front mode on or off; scores [rows][98] in host
 * memory; base (optional, device) and out are [n_frames][H][W][3] and offset per lane. */
int pf_batch_face_draw(pf_batch* b, int rows, const float* scores, const pf_draw_style* style,
                       const uint8_t* base, uint8_t* out, int* valid, int out_mem);
/* pf_face_stats of the lanes, gathered the same way: stats [rows][8][9] and valid [rows] of the last pf_batch_run_frames, each lane
 * measuring the rows of the frames it ran, front mode on or off.  Device-resident frames of that call must still be alive. */
int pf_batch_face_stats(pf_batch* b, int rows, int dark, int bright, uint64_t* stats, int* valid, int out_mem);

/* Engine options.  PF_OPT_HIP_GRAPH = 1: pf_run_frames* calls whose buffers all live on the device are captured
 * into a hipGraph per distinct (pointers, shapes, thresholds) and replayed (launch-latency bound small batches). */
enum { PF_OPT_HIP_GRAPH = 1,
       /* Range guard of the f32s (split-precision) programs.  Their convolutions write each f32 activation as f16 hi + f16 lo:
        * |x| >= 65504 overflows, and a tensor whose largest magnitude is below 2^-10 loses its low halves to f16 subnormals.
        * On EVERY forward call (value != 0, the default; 0 switches the guard off) each kernel that splits keeps max |x| of
        * what it splits and a one-workgroup kernel at the end of the forward judges the maxima -- part of the captured graphs
        * too.  A tensor outside [2^-10, 6e4] (or holding a NaN) sets that call's outputs to NaN and makes the next
        * synchronising entry point (pf_sync, any call with host outputs) fail with a message naming the op -- never silent
        * inf or garbage.  The remedy is to load the program with PF_DTYPE_F32 (exact f32 MFMA), which the Python facade does
        * on its own. */
       PF_OPT_RANGE_CHECK = 2,
       /* Where pf_decode_jpeg* decodes the Huffman stream: 0 = automatic (device for files without restart markers and for
        * batches that offer >= 4096 restart intervals, host threads otherwise), 1 = host, 2 = device. */
       PF_OPT_JPEG_ENTROPY = 3,
       /* Synchronisation rounds queued by the self-synchronising sub-sequence decoder (1 .. 10; 0 = all 10).  Fewer rounds save
        * empty launches on ordinary photographs; a stream that needs more is decoded again on the host (synchronous call) or
        * reported at the next synchronisation (pf_decode_jpeg_batch) -- never passed on. */
       PF_OPT_JPEG_SYNC_ROUNDS = 4,
       /* pf_batch_set_option only.  1 (default): a pf_batch_run_frames call on device-resident frames runs letterbox + detector +
        * NMS / top-k ONCE, on all of its frames, on the batch's front engine, and the lanes run crop + landmarks of their slices
        * behind it (the detector's launches are latency-bound: 96 frames cost 2.3 x what 32 do).  0: every lane detects its own
        * slice (the only path for host-resident frames). */
       PF_OPT_BATCH_FRONT = 5,
       /* Testing and tuning switch, per handle.  0 (default): the engine chooses the TH x TW output tile of every workgroup-level
        * detector launch (det_unit_kernel, det_c3_kernel) from the map, the batch and the device's compute units.  th << 16 | tw
        * forces that tile (cut to the map where the map is smaller) for all of them.  A tile whose input region does not fit the
        * LDS rows of a kernel the program launches makes the forward call fail with a message before anything is launched: it
        * never falls back to another tile.  Results do not depend on the tile; speed does.  Captured graphs are dropped on a
        * change. */
       PF_OPT_DET_TILE = 6 };
int pf_set_option(pf_handle* h, int option, int value);

/* Per-kernel device time of the last call, accumulated with HIP events on the handle's stream
 * when profiling is enabled.  names: '\n'-separated kernel tags; ms: same order. */
int pf_profile_enable(pf_handle* h, int on);
int pf_profile_fetch(pf_handle* h, char* names, size_t names_cap, float* ms, int* counts, int cap, int* n_out);
/* Kernels launched by the engine since profiling was enabled (nothing is recorded while it is off), in launch order: '\n'-separated
 * names as the launch sites spell them, template arguments included, e.g. "(conv3x3_halo_split_kernel<48, 8, 1, 256>)".  The
 * det_unit_kernel / det_c3_kernel entries are followed by their run-time tile, tiles per frame and grid: " tile=6x5 tpf=40 grid=80".
 * For tests of the dispatch.  At most names_cap - 1 bytes are written; *bytes_needed is the size that holds everything, *n_out the number
 * of launches (the log keeps the first 65536).  pf_profile_enable clears it. */
int pf_launch_log(pf_handle* h, char* names, size_t names_cap, int* n_out, size_t* bytes_needed);

#ifdef __cplusplus
}
#endif
#endif /* PEPPA_HIP_H */

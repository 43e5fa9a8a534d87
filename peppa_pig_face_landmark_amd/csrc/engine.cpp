// peppa-hip engine: program executor + C ABI (include/peppa_hip.h).
//
// One pf_handle = one HIP device + one stream + up to PF_NET_SLOTS loaded network programs.
// A program (pf_program.h) is executed as a straight-line sequence of fused-layer kernel launches
// over a static activation arena; nothing is allocated on the hot path.
#include "../../include/peppa_hip.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "k_conv_gemm.h"
#include "k_conv_split.h"
#include "k_expdw.h"
#include "k_halo.h"
#include "k_sepup_patch.h"
#include "k_layers.h"
#include "k_mbconv.h"
#include "k_chain.h"
#include "k_det.h"
#include "k_front.h"
#include "k_front2.h"
#include "k_hrb.h"
#include "k_hero.h"
#include "k_sepup.h"
#include "k_pwhead.h"
#include "k_mbx_args.h"
#include "k_jpeg.h"
#include "k_jpeg_enc.h"
#include "k_prepost.h"
#include "k_track.h"
#include "k_align.h"
#include "k_mask.h"
#include "k_redact.h"
#include "k_stats.h"
#include "k_draw.h"
#include "face_rows.h"
#include "pf_program.h"


namespace {

// Compute units of a handle's device: 256 on MI355X (8 XCDs x 32 CUs), queried at pf_create and kept WITH THE HANDLE (pf_handle::num_cus;
// a process-wide variable would follow whichever handle was created last).  Persistent kernels size their grids with it and the tile
// pickers count rounds of workgroups over the chip with it; correctness never depends on it (tiles are strided over gridDim).  The
// blockIdx & 7 == XCD affinity of the sepup kernels is an MI355X speed assumption only.
constexpr int kDefaultCUs = 256;
// workgroups per CU x CUs of the tile-walking kernels (k_det.h det_stem_kernel, k_front.h): the CPU emulator flavour caps the grid
// at 5 workgroups so that its small test images still make every workgroup walk several tiles
#ifdef PF_SIMT_EMULATION
inline int persistent_grid_n(int tiles, int, int) { return std::min(tiles, 5); }
#else
inline int persistent_grid_n(int tiles, int per_cu, int num_cus) { return std::min(tiles, per_cu * num_cus); }
#endif
#define persistent_grid(tiles, per_cu) persistent_grid_n((tiles), (per_cu), h->num_cus)      /* `h` is in scope at every launch site */

struct Program {
    bool loaded = false;
    PfHeader hdr{};
    std::vector<PfBufRec> bufs;
    std::vector<PfTensorRec> tens;
    std::vector<PfOpRec> ops;
    char* d_const = nullptr;
    char* d_arena = nullptr;
    unsigned* d_range = nullptr;     // f32s range guard: one slot per op (k_layers.h range_verdict_kernel)
    size_t arena_bytes = 0;
    int max_batch = 0;
    int esize = 2;

    char* buf_ptr(int b) const { return d_arena + (size_t)bufs[b].offset_units * 256 * (size_t)max_batch; }
    size_t buf_item_bytes(int b) const {
        const int e = bufs[b].etype;
        const size_t es = e == PF_ELEM_ACT ? (size_t)esize : (e == PF_ELEM_U8 ? 1 : 4);
        return (size_t)bufs[b].elems_per_item * es;
    }
    char* tensor_ptr(int t) const { return buf_ptr(tens[t].buf) + (size_t)tens[t].coff * esize; }
    const void* cptr(int off) const { return off < 0 ? nullptr : (const void*)(d_const + off); }
    // optional operands of an op (index < 0 = absent): pointer or nullptr, row stride or 0
    char* opt_tensor(int t) const { return t < 0 ? nullptr : tensor_ptr(t); }
    int opt_ld(int t) const { return t < 0 ? 0 : tens[t].ld; }
    char* opt_buf(int b) const { return b < 0 ? nullptr : buf_ptr(b); }
};

struct ProfEntry { double ms = 0; int count = 0; };

}  // namespace

#include "graph_cache.inl"

struct pf_handle {
    int device = 0;
    int num_cus = kDefaultCUs;      // compute units of `device`
    hipStream_t stream = nullptr;
    Program prog[PF_NET_SLOTS];
    std::string err;
    // staging for host-side inputs / outputs
    char* d_stage = nullptr;
    size_t stage_bytes = 0;
    // pipeline scratch (k_prepost)
    PipelineScratch pipe;
    GraphCache graphs;       // hipGraph replay of pf_run_frames* and of a pf_batch's halves (graph_cache.inl)
    unsigned long long* d_dbg = nullptr;   // PF_ACC_CYCLES / PF_ACC_DET_CYCLES: the cycle counters (PF_CYC_* regions, pf_ablate.h; ensure_cycle_counters)
    int dbg = 0;             // PEPPA_DBG: the PF_ABL_ / PF_SEL_ / PF_ACC_ bits of pf_ablate.h, never set in production
    // tracking state of the handle's video stream (pf_track_frame: one slot) and of its pf_track_streams pool (k_track.h)
    TrackPool track;
    TrackPool streams;
    int track_ids = 0, track_keep_lost = 0;   // pf_track_ids_config: persistent ids of both pools on / off, frames a lost id is kept
    JpegState jpeg;          // pf_decode_jpeg (jpeg.inl)
    JpegEncState jpeg_enc;   // pf_encode_jpeg (jpeg_enc.inl): tables and scratch of its three kernels
    // f32s range guard (pf_common.h pf_amax, k_layers.h range_verdict_kernel): on for every forward unless switched off with
    // PF_OPT_RANGE_CHECK = 0; the slots live with each program
    int range_every = 1;
    int jpeg_entropy = 0;               // PF_OPT_JPEG_ENTROPY: 0 automatic, 1 host, 2 device (jpeg.inl)
    int jpeg_rounds = 0;                // PF_OPT_JPEG_SYNC_ROUNDS: 0 = all PF_JPEG_SYNC_ROUNDS
    int det_tile = 0;                   // PF_OPT_DET_TILE: 0 = det_pick_tile chooses, th << 16 | tw = that tile for the det_unit / det_c3 launches
    unsigned long long n_calls = 0;
    int* h_status = nullptr;            // page-locked, device-visible: {code, op, value bits, program slot}
    // RCCL communicator for pf_broadcast_weights (comm.inl); created lazily, one per handle
    void* comm = nullptr;
    unsigned char comm_id[128] = {0};
    int comm_rank = -1, comm_world = 0;
    // what the handle's last call left for the stages behind the landmarks (face_rows.h): the rows with their frames, landmarks and
    // live flags (pf_face_chips, pf_face_masks*, pf_face_redact, pf_face_stats) and the attribute rows (pf_face_attrs); written by its own functions only
    FaceRows last;
    float* d_track_attrs = nullptr; size_t track_attrs_bytes = 0;      // attribute records of the tracking calls (FaceRows::attr_src)
    StageUpload upload;      // host frames / landmarks / counts of pf_align_faces, pf_mask_faces, pf_redact_faces, pf_measure_faces (stage_faces, face_rows.inl)
    AlignState align;        // aligned face chips (align.inl): scratch of its two kernels
    MaskState mask;          // face-region label maps (mask.inl): scratch of its two kernels
    // face redaction (redact.inl): the label maps it reads and the staging of host outputs
    RedactState redact;
    StatsState stats;        // per-face region statistics (stats.inl): the label maps and owners it reads and the staging of host outputs
    DrawState draw;         // face overlay (draw.inl): the primitives of its two kernels and the staging of host outputs
    // profiling
    bool profiling = false;
    std::map<std::string, ProfEntry> prof;
    std::vector<std::string> prof_order;
    std::vector<std::string> launch_log;      // spelled-out kernel of every PF_LAUNCH made while profiling is on, + its PF_LAUNCH_NOTE (pf_launch_log)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static std::string g_create_error;

static inline int host_dbg(const pf_handle* h) { return PF_ABLATE ? h->dbg : 0; }   // see pf_ablate.h: constant 0 in the production library

namespace { void comm_release(pf_handle* h); }   // comm.inl

#define PF_FAIL(h, ...)                                   \
    do {                                                  \
        char _b[512];                                     \
        snprintf(_b, sizeof(_b), __VA_ARGS__);            \
        (h)->err = _b;                                    \
        return 1;                                         \
    } while (0)

// Launch log (pf_launch_log): while profiling is on, every PF_LAUNCH leaves the kernel as it is spelled at the launch site, template
// arguments included ("(conv3x3_halo_split_kernel<48, 8, 1, 256>)"), so that a test of the dispatch knows which instance ran.
// Off otherwise: one predictable branch per launch.  mbx_launch.cpp (its own translation unit) is not logged.  PF_LAUNCH_NOTE, right
// behind a PF_LAUNCH, appends run-time facts of that launch to its entry (" tile=6x5 tpf=40 grid=80" of the det_* kernels).
constexpr size_t PF_LAUNCH_LOG_CAP = 1 << 16;

// every kernel launch is checked where it is made: a bad launch configuration (too much LDS, too many
// registers for the block size) must not surface one call later.  `h` is in scope at every launch site.
#undef PF_LAUNCH
#define PF_LAUNCH(kernel, grid, block, stream, ...)                                                          \
    do {                                                                                                     \
        if (h->profiling && h->launch_log.size() < PF_LAUNCH_LOG_CAP) h->launch_log.push_back(#kernel);      \
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                                     \
        const hipError_t _le = hipGetLastError();                                                            \
        if (_le != hipSuccess) PF_FAIL(h, "launch of %s failed: %s (%s:%d)", #kernel, hipGetErrorString(_le), __FILE__, __LINE__); \
    } while (0)

#define PF_LAUNCH_NOTE(...)                                                                                  \
    do {                                                                                                     \
        if (h->profiling && !h->launch_log.empty() && h->launch_log.size() < PF_LAUNCH_LOG_CAP) {            \
            char _n[96];                                                                                     \
            snprintf(_n, sizeof(_n), __VA_ARGS__);                                                           \
            h->launch_log.back() += _n;                                                                      \
        }                                                                                                    \
    } while (0)

#define PF_HIP(h, call)                                                                        \
    do {                                                                                       \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) PF_FAIL(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// ---------------------------------------------------------------------------------------------
// profiling helper: wraps one launch in an event pair when enabled; the tag is a printf format, filled in only then
struct ProfScope {
    pf_handle* h;
    std::string tag;
    __attribute__((format(printf, 3, 4))) ProfScope(pf_handle* h_, const char* fmt, ...) : h(h_) {
        if (!h->profiling) return;
        char buf[96]; va_list ap;
        va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
        tag = buf;
        (void)hipEventRecord(h->ev0, h->stream);
    }
    ~ProfScope() {
        if (!h->profiling) return;
        (void)hipEventRecord(h->ev1, h->stream);
        (void)hipEventSynchronize(h->ev1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
        auto it = h->prof.find(tag);
        if (it == h->prof.end()) { h->prof_order.push_back(tag); it = h->prof.emplace(tag, ProfEntry()).first; }
        it->second.ms += ms;
        it->second.count += 1;
    }
};

// ---------------------------------------------------------------------------------------------
// Output tile of a workgroup-level detector kernel (k_det.h): the largest-benefit TH x TW whose input region
// ((TH-1)*S+3) x ((TW-1)*S+3) fits the kernel's MAXR LDS rows.  Cost model: launches of these kernels are chains of a few
// phases (~3 us of fixed latency = ~768 rows' worth of work), so fewer rounds of workgroups over the chip come first, then
// the smaller tile; the halo rows every extra tile re-computes count with the chip's width.
static int g_det_tile_th = 0, g_det_tile_tw = 0;     // ablation build only: PEPPA_DET_TILE=th,tw forces the tile wherever it fits (tile sweeps)
static void det_pick_tile(int num_cus, int outH, int outW, int S, int max_rows, int B, int wg_per_cu, int* TH, int* TW) {
    double best = 1e30;
    *TH = 1; *TW = 1;
    if (PF_ABLATE != 0 && g_det_tile_th > 0 && ((g_det_tile_th - 1) * S + 3) * ((g_det_tile_tw - 1) * S + 3) <= max_rows) {
        *TH = std::min(g_det_tile_th, outH); *TW = std::min(g_det_tile_tw, outW);
        return;
    }
    for (int div = 1; div <= 16; ++div) {
        const int tw = (outW + div - 1) / div;
        if (div > 1 && tw == (outW + div - 2) / (div - 1)) continue;
        const int rw = (tw - 1) * S + 3;
        for (int th = 1; th <= outH; ++th) {
            const int rows = ((th - 1) * S + 3) * rw;
            if (rows > max_rows) break;
            const long long wgs = (long long)B * ((outH + th - 1) / th) * ((outW + tw - 1) / tw);
            const long long rounds = (wgs + (long long)num_cus * wg_per_cu - 1) / ((long long)num_cus * wg_per_cu);
            const double cost = (double)rounds * (768.0 + rows) + 0.5 * (double)wgs * rows / num_cus;
            if (cost < best) { best = cost; *TH = th; *TW = tw; }
        }
    }
}

// pf_div_small (pf_common.h) is exact for 0 <= x < min(4096, 2^20 / d): launch sites whose kernels divide a staging index by a tile-derived
// row length check the largest index they will produce against that domain instead of trusting the hard-coded tile
static inline bool pf_div_small_domain_ok(int max_x_exclusive, int d) {
    return d > 0 && max_x_exclusive <= 4096 && (long long)max_x_exclusive <= (1ll << 20) / d;
}

// Persistent kernels whose work units are faces: cost, in face times, of cutting each of B faces into `ns` units for a grid of
// `slots` workgroups -- rounds of the grid, the last one counted whole, and 2 % per extra unit for what every unit of a face
// fetches again.  384 faces on 256 slots are two rounds of faces (the second half empty) but three rounds of half faces.
static inline double last_round_cost(int B, int ns, int slots) { return (double)pf_div_up(B * ns, slots) / ns + 0.02 * (ns - 1); }

// cycle counters of the ablation build (pf_ablate.h: PF_ACC_* bits, PF_CYC_* regions of pf_handle::d_dbg)
static int ensure_cycle_counters(pf_handle* h) {
    if (h->d_dbg) return 0;
    PF_HIP(h, hipMalloc((void**)&h->d_dbg, PF_CYC_WORDS * sizeof(unsigned long long)));
    PF_HIP(h, hipMemset(h->d_dbg, 0, PF_CYC_WORDS * sizeof(unsigned long long)));
    return 0;
}

static void print_cycle_counters(const pf_handle* h) {      // at pf_destroy
    std::vector<unsigned long long> w(PF_CYC_WORDS);
    if (hipMemcpy(w.data(), h->d_dbg, w.size() * sizeof(w[0]), hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int k = 0; k < PF_CYC_DETUNIT.entries; ++k) {
        const unsigned long long* q = &w[PF_CYC_DETUNIT.at(k)];
        if (!q[4]) continue;
        const double n = (double)q[4];
        fprintf(stderr, "[det_unit C=%d S=%d] per workgroup (cycles): input+split %.0f | gemm1 %.0f | depthwise %.0f | gemm2+store %.0f  (%.0f workgroups)\n",
                k % 3 == 0 ? 32 : (k % 3 == 1 ? 64 : 128), k / 3 + 1, q[0] / n, q[1] / n, q[2] / n, q[3] / n, n);
    }
    for (int k = 0; k < PF_CYC_HRB.entries; ++k) {
        const unsigned long long* q = &w[PF_CYC_HRB.at(k)];
        if (!q[3]) continue;
        const double n = (double)q[3];
        fprintf(stderr, "[det_hr_bottleneck CIN=%d] per workgroup (cycles): conv1 %.0f | conv2 %.0f | conv3+store %.0f  (%.0f workgroups)\n", k ? 256 : 64,
                q[0] / n, q[1] / n, q[2] / n, n);
    }
    for (int k = 0; k < PF_CYC_MBX.entries; ++k) {
        const unsigned long long* q = &w[PF_CYC_MBX.at(k)];
        if (!q[7]) continue;
        static const char* shp[4] = {"KS3 k3", "KS4 k3", "KS4 k5", "KS5 k5d2"};
        const double n = (double)q[7];
        fprintf(stderr, "[det_mbx %s mode %d] per wave and launch-face (cycles): prologue+expand0 %.0f | project %.0f | wait a %.0f | depthwise %.0f | expand %.0f | wait b %.0f | epilogue %.0f  (%.0f waves)\n",
                shp[k / 4], k % 4, q[0] / n, q[1] / n, q[2] / n, q[3] / n, q[4] / n, q[5] / n, q[6] / n, n);
    }
    for (int k = 0; k < PF_CYC_SEPUP.entries; ++k) {
        const unsigned long long* q = &w[PF_CYC_SEPUP.at(k)];
        if (!q[2]) continue;
        const double steps = (double)q[3] / (double)q[2];          // K steps per wave
        fprintf(stderr, "[sepup_pipe BN=%d] per wave and K step (cycles): producer dma %.0f work %.0f wait %.0f | consumer dma %.0f mfma %.0f epilogue %.0f wait %.0f  (%.0f steps/wave)\n",
                k ? 256 : 128, q[9] / (double)q[2] / steps, q[0] / (double)q[2] / steps, q[1] / (double)q[2] / steps, q[4] / (double)q[8] / steps, q[5] / (double)q[8] / steps,
                q[6] / (double)q[8] / steps, q[7] / (double)q[8] / steps, steps);
    }
}

#include "launch_layers.inl"
#include "launch_landmark.inl"
#include "launch_teacher.inl"
#include "launch_det.inl"

// One launcher per op (launch_*.inl); an op that exists for f32 tensors or for split-precision programs only is refused here.
template <typename T, bool SPLIT>
static int run_program_t(pf_handle* h, int slot, const void* d_input, int input_kind, int B) {
    Program& p = h->prog[slot];
    constexpr bool F32 = std::is_same<T, float>::value;
    const bool guard = SPLIT && h->range_every > 0 && p.d_range != nullptr;     // every call, graph-captured ones included
    if (SPLIT && h->det_tile && det_forced_tile_fits(h, p)) return 1;           // PF_OPT_DET_TILE: refused before the first launch
    for (size_t oi = 0; oi < p.ops.size(); ++oi) {
        const PfOpRec& op = p.ops[oi];
        unsigned* const rs = guard ? p.d_range + oi * PF_RANGE_OP_WORDS : nullptr;
        int rc = 0;
        switch (op.code) {
            case PF_OP_STEM: rc = launch_stem<T>(h, p, op.as<PfStemOp>(), d_input, input_kind, SPLIT, B, rs); break;
            case PF_OP_CONV: rc = launch_conv<T, SPLIT>(h, p, op.as<PfConvOp>(), B, rs); break;
            case PF_OP_DW: rc = launch_dw<T>(h, p, op.as<PfDwOp>(), B); break;
            case PF_OP_UPCAT: rc = launch_upcat<T>(h, p, op.as<PfUpcatOp>(), B); break;
            case PF_OP_GAP: rc = launch_gap<T>(h, p, op.as<PfGapOp>(), B); break;
            case PF_OP_FC: rc = launch_fc(h, p, op.as<PfFcOp>(), B); break;
            case PF_OP_FC2: rc = launch_fc2(h, p, op.as<PfFc2Op>(), B); break;
            case PF_OP_SCSE: rc = launch_scse<T>(h, p, op.as<PfScseOp>(), B); break;
            case PF_OP_FACEATTR: rc = launch_faceattr(h, p, op.as<PfFaceattrOp>(), B); break;
            case PF_OP_HMDEC: rc = launch_hmdec<T>(h, p, op.as<PfHmdecOp>(), B); break;
            case PF_OP_ADDUP: rc = launch_addup<T>(h, p, op.as<PfAddupOp>(), B); break;
            case PF_OP_MAXPOOL: rc = launch_maxpool<T>(h, p, op.as<PfMaxpoolOp>(), B); break;
            case PF_OP_COPY: rc = launch_copy<T>(h, p, op.as<PfCopyOp>(), B); break;
            case PF_OP_DETDEC: rc = launch_detdec<T>(h, p, op.as<PfDetdecOp>(), B); break;
            case PF_OP_MBCONV:
                if (!F32) PF_FAIL(h, "fused inverted-residual op needs f32 tensors (f32 / f32s program)");
                rc = launch_mbconv(h, p, op.as<PfMbconvOp>(), SPLIT, B, rs);
                break;
            case PF_OP_FUSEUP:
                if (!F32) PF_FAIL(h, "fused HRNet fuse sum needs f32 tensors");
                rc = launch_fuseup(h, p, op.as<PfFuseupOp>(), B);
                break;
            case PF_OP_SEPUP:
                if (!SPLIT) PF_FAIL(h, "fused upsample+depthwise+pointwise op needs a split-precision (f32s) program");
                rc = launch_sepup(h, p, op.as<PfSepupOp>(), B, rs);
                break;
            case PF_OP_EXPDW:
                if (!SPLIT) PF_FAIL(h, "fused expand+depthwise op needs a split-precision (f32s) program");
                rc = launch_expdw(h, p, op.as<PfExpdwOp>(), B, rs);
                break;
            case PF_OP_MBX:
                if (!SPLIT) PF_FAIL(h, "fused inverted-residual op needs a split-precision (f32s) program");
                rc = launch_mbx(h, p, op.as<PfMbxOp>(), B, rs);
                break;
            case PF_OP_FRONT2:
                if (!SPLIT) PF_FAIL(h, "fused stem + first block op needs a split-precision (f32s) program");
                rc = launch_front2(h, p, op.as<PfFront2Op>(), d_input, input_kind, B, rs);
                break;
            case PF_OP_CHAIN:
                if (!SPLIT) PF_FAIL(h, "BasicBlock chain op needs a split-precision (f32s) program");
                rc = launch_chain(h, p, op.as<PfChainOp>(), B, rs);
                break;
            case PF_OP_BLOCK:
                if (!SPLIT) PF_FAIL(h, "BasicBlock op needs a split-precision (f32s) program");
                rc = launch_block(h, p, op.as<PfBlockOp>(), B, rs);
                break;
            case PF_OP_HRB:
                if (!SPLIT) PF_FAIL(h, "fused Bottleneck op needs a split-precision (f32s) program");
                rc = launch_hrb(h, p, op.as<PfHrbOp>(), B, rs);
                break;
            case PF_OP_DETUNIT:
                if (!SPLIT) PF_FAIL(h, "fused ShuffleV2Block op needs a split-precision (f32s) program");
                rc = launch_detunit(h, p, op.as<PfDetunitOp>(), B, rs);
                break;
            case PF_OP_DETC3:
                if (!SPLIT) PF_FAIL(h, "fused C3 op needs a split-precision (f32s) program");
                rc = launch_detc3(h, p, op.as<PfDetc3Op>(), B, rs);
                break;
            case PF_OP_DETSTEM:
                if (!SPLIT) PF_FAIL(h, "fused StemBlock op needs a split-precision (f32s) program");
                rc = launch_detstem(h, p, op.as<PfDetstemOp>(), d_input, input_kind, B, rs);
                break;
            default:
                PF_FAIL(h, "unknown op code %d at op %zu", op.code, oi);
        }
        if (rc) return rc;
    }
    if (guard) {
        RangeVerdictArgs v{};
        v.slots = p.d_range; v.n_ops = (int)p.ops.size();
        v.lo = 0.0009765625f;            // 2^-10: below this a tensor's low halves sit in the f16 subnormal range
        v.hi = 6.0e4f;                   // f16 overflows at 65504
        v.status = h->h_status; v.prog_slot = slot;
        v.poison0 = (float*)p.buf_ptr(p.hdr.out_buf0); v.n0 = (long long)B * p.bufs[p.hdr.out_buf0].elems_per_item;
        if (p.hdr.out_buf1 >= 0 && p.hdr.out_buf1 != p.hdr.out_buf0) { v.poison1 = (float*)p.buf_ptr(p.hdr.out_buf1); v.n1 = (long long)B * p.bufs[p.hdr.out_buf1].elems_per_item; }
        if (h->pipe.d_kps_for_decode) { v.poison2 = h->pipe.d_kps_for_decode; v.n2 = (long long)B * 98 * 2; }
        if (p.hdr.out_buf2 >= 0) { v.poison3 = (float*)p.buf_ptr(p.hdr.out_buf2); v.n3 = (long long)B * p.bufs[p.hdr.out_buf2].elems_per_item; }
        PF_LAUNCH(range_verdict_kernel, dim3(v.n_ops), dim3(64), h->stream, v);
    }
    PF_HIP(h, hipGetLastError());
    return 0;
}

// Start of every forward-running entry point
static void begin_call(pf_handle* h) { h->n_calls++; }

// After a stream synchronisation: did a range-checked forward find a tensor the f32s kernels cannot represent?
static int check_numerics(pf_handle* h) {
    if (!h->h_status || h->h_status[0] == 0) return 0;
    const int code = h->h_status[0], op = h->h_status[1], slot = h->h_status[3];
    float v;
    memcpy(&v, &h->h_status[2], 4);
    h->h_status[0] = 0;
    if (code == 3)
        PF_FAIL(h, "pf_decode_jpeg_batch: the parallel entropy decoder did not synchronise (%d sub-sequence records still changing "
                   "after the last round): the frames of that batch are invalid; decode it again with pf_set_option(PF_OPT_JPEG_ENTROPY, 1)", op);
    PF_FAIL(h, "activation range check failed: input of op %d of program %d has max |x| = %g, %s the range [9.8e-4, 6e4] the "
               "split-precision (f32s) convolutions can represent (outputs were set to NaN); rebuild the program with dtype 'f32'",
            op, slot, (double)v, code == 1 ? "above" : "below");
}

static int run_program(pf_handle* h, int slot, const void* d_input, int input_kind, int B) {
    Program& p = h->prog[slot];
    if (!p.loaded) PF_FAIL(h, "no program loaded in slot %d", slot);
    if (B < 1 || B > p.max_batch) PF_FAIL(h, "batch %d outside [1, %d]", B, p.max_batch);
    if (p.hdr.dtype == PF_DTYPE_F16) return run_program_t<pf_half, false>(h, slot, d_input, input_kind, B);
    if (p.hdr.dtype == PF_DTYPE_F32_SPLIT) return run_program_t<float, true>(h, slot, d_input, input_kind, B);
    return run_program_t<float, false>(h, slot, d_input, input_kind, B);
}

static int ensure_stage(pf_handle* h, size_t bytes) {
    if (bytes <= h->stage_bytes) return 0;
    if (h->d_stage) (void)hipFree(h->d_stage);
    h->d_stage = nullptr;
    h->stage_bytes = 0;
    PF_HIP(h, hipMalloc((void**)&h->d_stage, bytes));
    h->stage_bytes = bytes;
    return 0;
}

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* pf_version(void) { return "peppa-hip 0.1 " PF_BUILD_TAG; }

int pf_create(int device_id, pf_handle** out) {
    if (!out) return 1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_create_error = "no HIP device visible (the engine has no CPU fallback)"; return 1; }
    if (device_id < 0 || device_id >= n) { g_create_error = "device id out of range"; return 1; }
    if (hipSetDevice(device_id) != hipSuccess) { g_create_error = "hipSetDevice failed"; return 1; }
    pf_handle* h = new pf_handle();
    h->device = device_id;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus >= 8) h->num_cus = cus;
    }
    if constexpr (PF_ABLATE != 0) {      // ablation build only (libpeppa_hip_ablate.so): ablated kernels compute garbage, so the guard is off
        if (const char* v = getenv("PEPPA_DBG")) { h->dbg = atoi(v); if (h->dbg & PF_DBG_GUARD_OFF_MASK) h->range_every = 0; }   // which bits leave results right: pf_ablate.h
        if (const char* v = getenv("PEPPA_ALIGN_LDS")) h->align.lds_budget = atoi(v);     // 0: every align_warp tile takes the direct path (tools/bench_face_chips.py)
        if (const char* v = getenv("PEPPA_MASK_NOCULL")) h->mask.no_cull = atoi(v) ? 1 : 0;       // 1: mask_fill evaluates every slot in every tile, no parity folding (tools/bench_face_masks.py)
        if (const char* v = getenv("PEPPA_REDACT_STAGE_ALL")) h->redact.stage_all = atoi(v) ? 1 : 0;       // 1: redact_kernel stages every tile through LDS, none is copied (tools/bench_face_redact.py)
        if (const char* v = getenv("PEPPA_STATS_STAGED")) h->stats.staged = atoi(v) ? 1 : 0;       // 1: face_stats_staged_kernel, LDS-staged pieces and register partials, in place of face_stats_kernel (tools/bench_face_stats.py)
        if (const char* v = getenv("PEPPA_DRAW_NOCULL")) h->draw.no_cull = atoi(v) ? 1 : 0;       // 1: draw_kernel stages every tile and lists every primitive of the image in it (tools/bench_face_draw.py)
        if (const char* v = getenv("PEPPA_DET_TILE")) { if (sscanf(v, "%d,%d", &g_det_tile_th, &g_det_tile_tw) != 2) g_det_tile_th = g_det_tile_tw = 0; }
    }
    bool masked = false;
    if constexpr (PF_ABLATE != 0) {      // experiment: every handle of the process on its own share of the CUs (PEPPA_CU_PARTITION=parts,mode)
        static int s_lane = 0;
        int parts = 0, mode = 1;
        if (const char* v = getenv("PEPPA_CU_PARTITION")) (void)sscanf(v, "%d,%d", &parts, &mode);
        if (parts > 1) {
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int lane = s_lane++ % parts, per = h->num_cus / parts;
            for (int c = 0; c < h->num_cus; ++c)
                if ((mode == 1 && c % parts == lane) || (mode == 2 && c / per == lane) || (mode == 3 && (c / 8) % parts == lane)) mask[c >> 5] |= 1u << (c & 31);
            masked = hipExtStreamCreateWithCUMask(&h->stream, 8, mask) == hipSuccess;
            fprintf(stderr, "[peppa-hip] handle %d: CU partition %d/%d mode %d: %s\n", s_lane - 1, lane, parts, mode, masked ? "ok" : "FAILED");
        }
    }
    if ((!masked && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        g_create_error = "stream/event creation failed";
        delete h;
        return 1;
    }
    if (hipHostMalloc((void**)&h->h_status, 4 * sizeof(int), hipHostMallocPortable) != hipSuccess) {
        g_create_error = "hipHostMalloc(status) failed";
        delete h;
        return 1;
    }
    memset(h->h_status, 0, 4 * sizeof(int));
    *out = h;
    return 0;
}

void pf_destroy(pf_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->graphs.destroy_all();
    comm_release(h);
    for (auto& p : h->prog) {
        if (p.d_const) (void)hipFree(p.d_const);
        if (p.d_arena) (void)hipFree(p.d_arena);
        if (p.d_range) (void)hipFree(p.d_range);
    }
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->d_track_attrs) (void)hipFree(h->d_track_attrs);
    if (h->d_dbg) { print_cycle_counters(h); (void)hipFree(h->d_dbg); }
    if (h->h_status) (void)hipHostFree(h->h_status);
    h->pipe.release();
    h->last.release();
    h->upload.release();
    h->align.release();
    h->mask.release();
    h->redact.release();
    h->stats.release();
    h->draw.release();
    h->track.release();
    h->streams.release();
    h->jpeg.release();
    h->jpeg_enc.release();
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* pf_last_error(pf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pf_sync(pf_handle* h) {
    if (!h) return 1;
    PF_HIP(h, hipStreamSynchronize(h->stream));
    return check_numerics(h);
}

int pf_load_program(pf_handle* h, int slot, const void* blob, size_t bytes, int max_batch) {
    if (!h) return 1;
    if (slot < 0 || slot >= PF_NET_SLOTS) PF_FAIL(h, "slot %d out of range", slot);
    if (slot == PF_NET_LANDMARK) h->last.forget();      // the records of the previous program are gone with its arena
    if (!blob || bytes < sizeof(PfHeader)) PF_FAIL(h, "program blob too small");
    if (max_batch < 1) PF_FAIL(h, "max_batch must be >= 1");
    PF_HIP(h, hipSetDevice(h->device));
    PfHeader hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != PF_PROGRAM_MAGIC) PF_FAIL(h, "bad program magic 0x%08x", hd.magic);
    if (hd.version != PF_PROGRAM_VERSION) PF_FAIL(h, "program version %d, engine expects %d", hd.version, PF_PROGRAM_VERSION);
    if (hd.dtype != PF_DTYPE_F16 && hd.dtype != PF_DTYPE_F32 && hd.dtype != PF_DTYPE_F32_SPLIT) PF_FAIL(h, "bad dtype %d", hd.dtype);
    size_t off = sizeof(PfHeader);
    const size_t need = off + (size_t)hd.n_bufs * sizeof(PfBufRec) + (size_t)hd.n_tensors * sizeof(PfTensorRec) +
                        (size_t)hd.n_ops * sizeof(PfOpRec);
    if (bytes < need) PF_FAIL(h, "program blob truncated (tables)");
    Program& p = h->prog[slot];
    PF_HIP(h, hipStreamSynchronize(h->stream));
    if (h->graphs.note_realloc(h->err)) return 1;      // graphs captured over the old arena / constants must not be replayed
    if (p.d_const) { (void)hipFree(p.d_const); p.d_const = nullptr; }
    if (p.d_arena) { (void)hipFree(p.d_arena); p.d_arena = nullptr; }
    if (p.d_range) { (void)hipFree(p.d_range); p.d_range = nullptr; }
    p.loaded = false;
    p.hdr = hd;
    p.esize = hd.dtype == PF_DTYPE_F16 ? 2 : 4;
    const char* src = (const char*)blob;
    p.bufs.resize(hd.n_bufs);
    memcpy(p.bufs.data(), src + off, (size_t)hd.n_bufs * sizeof(PfBufRec)); off += (size_t)hd.n_bufs * sizeof(PfBufRec);
    p.tens.resize(hd.n_tensors);
    memcpy(p.tens.data(), src + off, (size_t)hd.n_tensors * sizeof(PfTensorRec)); off += (size_t)hd.n_tensors * sizeof(PfTensorRec);
    p.ops.resize(hd.n_ops);
    memcpy(p.ops.data(), src + off, (size_t)hd.n_ops * sizeof(PfOpRec)); off += (size_t)hd.n_ops * sizeof(PfOpRec);
    off = (off + 255) / 256 * 256;
    if (bytes < off + (size_t)hd.const_bytes) PF_FAIL(h, "program blob truncated (constants)");
    // validate indices once so the hot path can trust them
    for (const auto& t : p.tens)
        if (t.buf < 0 || t.buf >= hd.n_bufs) PF_FAIL(h, "tensor references buffer %d", t.buf);
    for (int b = 0; b < hd.n_bufs; ++b) {
        const size_t units = (p.buf_item_bytes(b) + 255) / 256;
        if ((size_t)p.bufs[b].offset_units + units > (size_t)hd.arena_units_per_item) PF_FAIL(h, "buffer %d outside the arena", b);
    }
    PF_HIP(h, hipMalloc((void**)&p.d_const, std::max<size_t>(hd.const_bytes, 256)));
    PF_HIP(h, hipMemcpy(p.d_const, src + off, hd.const_bytes, hipMemcpyHostToDevice));
    p.max_batch = max_batch;
    p.arena_bytes = (size_t)hd.arena_units_per_item * 256 * (size_t)max_batch;
    PF_HIP(h, hipMalloc((void**)&p.d_arena, p.arena_bytes + 256));          // + slack: masked pixel-operand units may read up to 124 bytes behind a tensor
    PF_HIP(h, hipMemset(p.d_arena, 0, p.arena_bytes + 256));
    if (hd.dtype == PF_DTYPE_F32_SPLIT) {
        const size_t rb = std::max<size_t>(hd.n_ops, 1) * PF_RANGE_OP_WORDS * sizeof(unsigned);
        PF_HIP(h, hipMalloc((void**)&p.d_range, rb + PF_RANGE_TAIL_WORDS * sizeof(unsigned)));
        PF_HIP(h, hipMemset(p.d_range, 0, rb + PF_RANGE_TAIL_WORDS * sizeof(unsigned)));
        PF_HIP(h, hipMemset((char*)p.d_range + rb, 0xFF, 8));       // the verdict key: all ones = no violation (range_verdict_kernel)
    }
    p.loaded = true;
    return 0;
}

static int net_forward_common(pf_handle* h, int slot, const void* input, int input_kind, int mem, int batch,
                              size_t in_item_bytes) {
    PF_HIP(h, hipSetDevice(h->device));
    const void* d_in = input;
    if (mem == PF_MEM_HOST) {
        if (ensure_stage(h, in_item_bytes * batch)) return 1;
        PF_HIP(h, hipMemcpyAsync(h->d_stage, input, in_item_bytes * batch, hipMemcpyHostToDevice, h->stream));
        d_in = h->d_stage;
    } else if ((size_t)input & 3) {
        // the staged-image kernels (k_det.h det_stem_kernel, k_front.h) fetch the uint8 image as 32-bit words: a device pointer that is
        // not 4-byte aligned (a view into somebody else's buffer) goes through the aligned staging buffer first
        if (ensure_stage(h, in_item_bytes * batch)) return 1;
        PF_HIP(h, hipMemcpyAsync(h->d_stage, input, in_item_bytes * batch, hipMemcpyDeviceToDevice, h->stream));
        d_in = h->d_stage;
    }
    return run_program(h, slot, d_in, input_kind, batch);
}

static int copy_out(pf_handle* h, const void* d_src, void* dst, size_t bytes, int out_mem) {
    if (!dst) return 0;
    PF_HIP(h, hipMemcpyAsync(dst, d_src, bytes, out_mem == PF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int pf_landmark_forward(pf_handle* h, const void* input, int input_kind, int mem, int batch,
                        float* loc_fix, float* score, int out_mem) {
    if (!h) return 1;
    Program& p = h->prog[PF_NET_LANDMARK];
    if (!p.loaded) PF_FAIL(h, "landmark program not loaded");
    const size_t px = (size_t)p.hdr.in_h * p.hdr.in_w * 3;
    h->pipe.d_crop_for_decode = nullptr;
    h->pipe.d_kps_for_decode = nullptr;
    begin_call(h);
    h->last.note_frameless();     // rows without a frame (pf_face_chips)
    if (net_forward_common(h, PF_NET_LANDMARK, input, input_kind, mem, batch, input_kind == PF_INPUT_U8_NHWC ? px : px * 4)) return 1;
    h->last.note_attrs(1, batch);
    if (copy_out(h, p.buf_ptr(p.hdr.out_buf0), loc_fix, (size_t)batch * p.buf_item_bytes(p.hdr.out_buf0), out_mem)) return 1;
    if (copy_out(h, p.buf_ptr(p.hdr.out_buf1), score, (size_t)batch * p.buf_item_bytes(p.hdr.out_buf1), out_mem)) return 1;
    if (out_mem == PF_MEM_HOST) {
        PF_HIP(h, hipStreamSynchronize(h->stream));
        return check_numerics(h);
    }
    return 0;
}

int pf_detector_forward(pf_handle* h, const void* input, int input_kind, int mem, int batch, float* rows_out, int out_mem) {
    if (!h) return 1;
    Program& p = h->prog[PF_NET_DETECTOR];
    if (!p.loaded) PF_FAIL(h, "detector program not loaded");
    const size_t px = (size_t)p.hdr.in_h * p.hdr.in_w * 3;
    begin_call(h);
    if (net_forward_common(h, PF_NET_DETECTOR, input, input_kind, mem, batch, input_kind == PF_INPUT_U8_NHWC ? px : px * 4)) return 1;
    if (copy_out(h, p.buf_ptr(p.hdr.out_buf0), rows_out, (size_t)batch * p.buf_item_bytes(p.hdr.out_buf0), out_mem)) return 1;
    if (out_mem == PF_MEM_HOST) {
        PF_HIP(h, hipStreamSynchronize(h->stream));
        return check_numerics(h);
    }
    return 0;
}

int pf_face_attrs(pf_handle* h, int rows, float* out, int raw, int out_mem) {
    if (!h) return 1;
    Program& p = h->prog[PF_NET_LANDMARK];
    if (!p.loaded) PF_FAIL(h, "pf_face_attrs: landmark program not loaded");
    if (p.hdr.out_buf2 < 0)
        PF_FAIL(h, "pf_face_attrs: the loaded landmark program has no face-attribute head (build it with face_attrs=True)");
    if (!out || rows < 0 || (out_mem != PF_MEM_HOST && out_mem != PF_MEM_DEVICE && out_mem != PF_MEM_HOST_PINNED))
        PF_FAIL(h, "pf_face_attrs: bad arguments");
    const FaceRows& s = h->last;        // its attribute half
    if (s.attr_kind == 0) PF_FAIL(h, "pf_face_attrs: the handle's last call left no face-attribute rows (pf_landmark_forward, "
                                     "pf_landmarks*, pf_run_frames*, pf_track_frame* and pf_track_streams do)");
    if (rows > s.attr_rows) PF_FAIL(h, "pf_face_attrs: %d rows asked, the last call left %d", rows, s.attr_rows);
    if (rows == 0) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    FaceAttrsPickArgs a{};
    a.rec = s.attr_kind == 3 ? s.attr_src : (const float*)p.buf_ptr(p.hdr.out_buf2);
    a.col0 = raw ? PF_FACE_ATTR_RAW : PF_FACE_ATTR_COOKED;
    a.valid = s.attr_kind == 2 ? s.d_attr_valid : nullptr; a.rows = rows;
    if (out_mem == PF_MEM_DEVICE) {
        a.out = out;
        PF_LAUNCH(face_attrs_pick_kernel, dim3(pf_div_up(rows * 7, 256)), dim3(256), h->stream, a);
        PF_HIP(h, hipGetLastError());
        return 0;
    }
    // host memory: the records come over, the picked rows are written on the host (rows whose pf_landmarks valid flag is 0 are left
    // as they were, like the kps of pf_landmarks)
    std::vector<float> rec((size_t)rows * PF_FACE_ATTR_REC);
    PF_HIP(h, hipMemcpyAsync(rec.data(), a.rec, rec.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    PF_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < rows; ++i) {
        if (s.attr_kind == 2 && !s.h_attr_valid[i]) continue;
        memcpy(out + (size_t)i * 7, rec.data() + (size_t)i * PF_FACE_ATTR_REC + a.col0, 7 * sizeof(float));
    }
    return 0;
}

int pf_read_tensor(pf_handle* h, int slot, int tensor_id, int batch, float* out_host, size_t out_elems) {
    if (!h) return 1;
    if (slot < 0 || slot >= PF_NET_SLOTS || !h->prog[slot].loaded) PF_FAIL(h, "slot %d not loaded", slot);
    Program& p = h->prog[slot];
    if (tensor_id < 0 || tensor_id >= (int)p.tens.size()) PF_FAIL(h, "tensor id %d out of range", tensor_id);
    const PfTensorRec& t = p.tens[tensor_id];
    const size_t n = (size_t)batch * t.H * t.W * t.C;
    if (out_elems < n) PF_FAIL(h, "output too small: %zu < %zu", out_elems, n);
    PF_HIP(h, hipStreamSynchronize(h->stream));
    const size_t item_elems = (size_t)t.H * t.W * t.ld;
    std::vector<char> tmp(item_elems * p.esize * batch);
    PF_HIP(h, hipMemcpy(tmp.data(), p.tensor_ptr(tensor_id) - (size_t)t.coff * p.esize, tmp.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)
        for (size_t px = 0; px < (size_t)t.H * t.W; ++px)
            for (int c = 0; c < t.C; ++c) {
                const size_t si = (size_t)b * item_elems + px * t.ld + t.coff + c;
                float v;
                if (p.esize == 2) v = (float)((const pf_half*)tmp.data())[si];
                else v = ((const float*)tmp.data())[si];
                out_host[((size_t)b * t.H * t.W + px) * t.C + c] = v;
            }
    return 0;
}

int pf_profile_enable(pf_handle* h, int on) {
    if (!h) return 1;
    h->profiling = on != 0;
    h->prof.clear();
    h->prof_order.clear();
    h->launch_log.clear();
    return 0;
}

int pf_launch_log(pf_handle* h, char* names, size_t names_cap, int* n_out, size_t* bytes_needed) {
    if (!h) return 1;
    std::string joined;
    for (const std::string& k : h->launch_log) {
        joined += k;
        joined += '\n';
    }
    if (names && names_cap) {
        const size_t c = std::min(names_cap - 1, joined.size());
        memcpy(names, joined.data(), c);
        names[c] = 0;
    }
    if (n_out) *n_out = (int)h->launch_log.size();
    if (bytes_needed) *bytes_needed = joined.size() + 1;
    return 0;
}

int pf_profile_fetch(pf_handle* h, char* names, size_t names_cap, float* ms, int* counts, int cap, int* n_out) {
    if (!h) return 1;
    std::string joined;
    int n = 0;
    for (const auto& tag : h->prof_order) {
        if (n >= cap) break;
        const ProfEntry& e = h->prof[tag];
        if (ms) ms[n] = (float)e.ms;
        if (counts) counts[n] = e.count;
        joined += tag;
        joined += '\n';
        ++n;
    }
    if (names && names_cap) {
        const size_t c = std::min(names_cap - 1, joined.size());
        memcpy(names, joined.data(), c);
        names[c] = 0;
    }
    if (n_out) *n_out = n;
    return 0;
}

}  // extern "C"

#include "face_rows.inl"
#include "align.inl"
#include "mask.inl"
#include "redact.inl"
#include "stats.inl"
#include "draw.inl"
#include "pipeline.inl"
#include "comm.inl"
#include "track.inl"
#include "jpeg.inl"
#include "jpeg_enc.inl"
#include "batch.inl"

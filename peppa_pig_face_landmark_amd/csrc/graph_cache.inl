// hipGraph cache of a handle (PF_OPT_HIP_GRAPH; included by engine.cpp in front of pf_handle, which holds one GraphCache).  A device-
// resident call is launched eagerly the first time its key is seen (which also performs every lazy allocation and constant upload),
// captured into a hipGraph the second time and replayed from then on: one graph launch instead of ~170 kernel launches (single-frame
// latency is launch bound).  A key names everything the captured launches take from the call; the cache's epoch stands for every device
// allocation they may point at: whoever frees or replaces one calls note_realloc() first (stale graphs are destroyed before the next lookup, never replayed).
#include <tuple>

// PF_HIP (engine.cpp) for the cache, which reports into a std::string `err`
#define PF_GRAPH_HIP(call)                                                                                                           \
    do {                                                                                                                             \
        const hipError_t _e = (call);                                                                                                \
        if (_e != hipSuccess) { char _b[512]; snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); err = _b; return 1; } \
    } while (0)

namespace {

enum GraphKind : int { GRAPH_WHOLE_CALL, GRAPH_FRONT, GRAPH_LANE_TAIL };      // pf_run_frames*; the two halves of a pf_batch call (batch.inl)

struct GraphKey {
    GraphKind kind = GRAPH_WHOLE_CALL;
    const void *frames = nullptr, *det_rows = nullptr, *sel_boxes = nullptr, *sel_count = nullptr;      // what the call reads ...
    const void *counts = nullptr, *boxes = nullptr, *kps = nullptr, *scores = nullptr;                  // ... and writes
    int n_frames = 0, height = 0, width = 0, rows = 0, top_k = 0, out_mem = 0;
    float score_thres = 0.f, iou_thres = 0.f, min_face = 0.f;
    unsigned long long epoch = 0;       // GraphCache::epoch at the lookup (set by GraphCache::run)

    // One builder per kind; the fields a kind does not use stay zero.
    static GraphKey front(const void* frames, const void* det_rows, int n_frames, int height, int width, int rows, float score_thres,
                          float iou_thres, float min_face, int top_k, const void* sel_boxes, const void* sel_count) {
        GraphKey k;
        k.kind = GRAPH_FRONT; k.frames = frames; k.det_rows = det_rows; k.sel_boxes = sel_boxes; k.sel_count = sel_count;
        k.n_frames = n_frames; k.height = height; k.width = width; k.rows = rows; k.top_k = top_k;
        k.score_thres = score_thres; k.iou_thres = iou_thres; k.min_face = min_face;
        return k;
    }
    static GraphKey lane_tail(const void* frames, int n_frames, int height, int width, const void* sel_boxes, const void* sel_count,
                              int top_k, const void* counts, const void* boxes, const void* kps, const void* scores, int out_mem) {
        GraphKey k;
        k.kind = GRAPH_LANE_TAIL; k.frames = frames; k.sel_boxes = sel_boxes; k.sel_count = sel_count;
        k.counts = counts; k.boxes = boxes; k.kps = kps; k.scores = scores; k.out_mem = out_mem;
        k.n_frames = n_frames; k.height = height; k.width = width; k.top_k = top_k;
        return k;
    }
    static GraphKey whole_call(const void* frames, const void* det_rows, int n_frames, int height, int width, int rows, float score_thres, float iou_thres,
                               float min_face, int top_k, const void* counts, const void* boxes, const void* kps, const void* scores, int out_mem) {
        GraphKey k = front(frames, det_rows, n_frames, height, width, rows, score_thres, iou_thres, min_face, top_k, nullptr, nullptr);      // front + tail on one handle
        k.kind = GRAPH_WHOLE_CALL; k.counts = counts; k.boxes = boxes; k.kps = kps; k.scores = scores; k.out_mem = out_mem;
        return k;
    }
    auto members() const { return std::tie(kind, frames, det_rows, sel_boxes, sel_count, counts, boxes, kps, scores, n_frames, height, width,
                                           rows, top_k, out_mem, score_thres, iou_thres, min_face, epoch); }
    // (thresholds compare as floats: a NaN threshold never matches, so such a call runs eagerly every time; -0 matches +0, which NMS cannot tell apart)
    bool operator==(const GraphKey& o) const { return members() == o.members(); }
};

struct GraphEntry { GraphKey key; hipGraphExec_t exec; };      // exec == nullptr: seen once, not captured yet
constexpr size_t kGraphCacheCapacity = 16;      // keys a handle keeps; one more drops them all

struct GraphCache {
    bool enabled = false;               // PF_OPT_HIP_GRAPH
    bool capturing = false;             // inside run()'s stream capture
    unsigned long long epoch = 0;       // generation of the device allocations captured graphs may reference
    std::vector<GraphEntry> entries;

    void destroy_all() {
        for (auto& g : entries) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        entries.clear();
    }
    // THE invalidation entry point: called in front of every free or replacement of device memory a captured graph may reference
    // (scratch growth, program (re)load, a pf_batch's selected-box buffers, a decoded-frame buffer) and when an option changes what a
    // call launches.  Refused inside a capture: the graph being recorded would be stale before it exists.
    int note_realloc(std::string& err) {
        if (capturing) { err = "internal: device scratch would be reallocated inside a graph capture"; return 1; }
        epoch++;
        return 0;
    }
    // `enqueue` through the cache when graphs are on and the caller finds the call capturable (no profiling, everything device
    // resident), eagerly otherwise
    template <typename Enqueue>
    int run(bool capturable, hipStream_t stream, std::string& err, GraphKey key, Enqueue&& enqueue) {
        if (!enabled || !capturable) return enqueue();
        auto failed = [&err](const char* what, hipError_t e) { err = std::string(what) + " failed: " + hipGetErrorString(e); return 1; };
        if (!entries.empty() && entries.front().key.epoch != epoch) destroy_all();
        key.epoch = epoch;
        GraphEntry* e = nullptr;
        for (auto& g : entries)
            if (g.key == key) { e = &g; break; }
        if (!e) {   // first sighting: run eagerly
            if (entries.size() >= kGraphCacheCapacity) destroy_all();
            const int rc = enqueue();
            if (epoch != key.epoch) destroy_all();      // this eager run (re)allocated scratch: older graphs are stale, this entry is not
            key.epoch = epoch;
            if (!rc) entries.push_back(GraphEntry{key, nullptr});
            return rc;
        }
        if (!e->exec) {
            PF_GRAPH_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            capturing = true;
            const int rc = enqueue();
            capturing = false;
            hipGraph_t graph = nullptr;
            hipError_t he = hipStreamEndCapture(stream, &graph);
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
            if (he != hipSuccess || !graph) return failed("hipStreamEndCapture", he);
            he = hipGraphInstantiate(&e->exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (he != hipSuccess) { e->exec = nullptr; return failed("hipGraphInstantiate", he); }
        }
        PF_GRAPH_HIP(hipGraphLaunch(e->exec, stream));
        return 0;
    }
};

}  // namespace
#undef PF_GRAPH_HIP

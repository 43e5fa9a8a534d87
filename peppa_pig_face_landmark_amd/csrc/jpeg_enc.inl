// Baseline JPEG encoder, host side (kernels in k_jpeg_enc.h):
//   pf_encode_jpeg         n packed BGR images of one size -> n JFIF files
//   pf_encode_jpeg_bound   a capacity no image of a shape can exceed
//   pf_device_alloc / pf_device_free   device memory for callers without a HIP runtime of their own
// The header and the tables are the same for every image of a call: built here, kept with the handle per (height, width, quality,
// subsampling).  The call leaves the record of the last call (pf_handle::last) alone and is never captured into a graph.
namespace {

// ITU T.81 K.1 / K.2 in natural order, K.3 - K.6 as code counts per length and symbols
const unsigned char kJpegEncQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const unsigned char kJpegEncDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char kJpegEncAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const unsigned char kJpegEncAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr int kJpegEncHeaderLen = 20 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14;      // 629

// what the shape decides; ok = false: a shape pf_encode_jpeg refuses
struct JpegEncGeom {
    bool ok = false;
    int hs = 1, vs = 1, mcus_x = 0, mcus_y = 0, bpm = 3, nb = 0;      // nb: blocks of an interval
    unsigned words = 0;               // words of an interval's slice of the bit scratch: every block at its longest
    unsigned long long bound = 0;     // pf_encode_jpeg_bound
};

JpegEncGeom jpeg_enc_geom(int height, int width, int subsampling) {
    JpegEncGeom g;
    if (height < 1 || width < 1 || height > 65535 || width > 65535) return g;
    if (subsampling == 444) { g.hs = 1; g.vs = 1; }
    else if (subsampling == 422) { g.hs = 2; g.vs = 1; }
    else if (subsampling == 420) { g.hs = 2; g.vs = 2; }
    else return g;
    g.mcus_x = pf_div_up(width, 8 * g.hs); g.mcus_y = pf_div_up(height, 8 * g.vs);
    g.bpm = g.hs * g.vs + 2; g.nb = g.mcus_x * g.bpm;
    const unsigned long long bits = (unsigned long long)g.nb * PF_JPEG_ENC_BLOCK_BITS;
    g.words = (unsigned)((bits + 31) / 32 + 1);
    // header + per interval: every block at its longest, padded to a byte, every byte 0xFF and stuffed, RSTm (EOI behind the last)
    g.bound = (unsigned long long)kJpegEncHeaderLen + (unsigned long long)g.mcus_y * (2 * ((bits + 7) / 8) + 2);
    g.ok = g.bound <= 0x7fffffffull;  // sizes[] are ints
    return g;
}

void jpeg_enc_huff(const unsigned char* bits, const unsigned char* vals, unsigned* table) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = code++ << 5 | (unsigned)len;
        code <<= 1;
    }
}

void jpeg_enc_tables(JpegEncTables& t, int height, int width, int quality, const JpegEncGeom& g) {
    memset(&t, 0, sizeof(t));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    unsigned char q[2][64];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            q[c][i] = (unsigned char)std::min(std::max((kJpegEncQ[c][i] * scale + 50) / 100, 1), 255);
            t.qdiv[c][i] = (unsigned short)(8 * q[c][i]);
        }
    unsigned char dc_vals[12];
    for (int i = 0; i < 12; ++i) dc_vals[i] = (unsigned char)i;
    for (int c = 0; c < 2; ++c) {
        jpeg_enc_huff(kJpegEncDcBits[c], dc_vals, t.dc[c]);
        jpeg_enc_huff(kJpegEncAcBits[c], kJpegEncAcVals[c], t.ac[c]);
    }
    unsigned char* p = t.header;
    auto put = [&p](std::initializer_list<int> v) { for (int x : v) *p++ = (unsigned char)x; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int k = 0; k < 64; ++k) *p++ = q[c][kZigzag[k]];
    }
    put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, g.hs << 4 | g.vs, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xC4, 0, 19 + 12, c});
        for (int i = 0; i < 16; ++i) *p++ = kJpegEncDcBits[c][i];
        for (int i = 0; i < 12; ++i) *p++ = dc_vals[i];
        put({0xFF, 0xC4, 0, 19 + 162, 0x10 | c});
        for (int i = 0; i < 16; ++i) *p++ = kJpegEncAcBits[c][i];
        for (int i = 0; i < 162; ++i) *p++ = kJpegEncAcVals[c][i];
    }
    put({0xFF, 0xDD, 0, 4, g.mcus_x >> 8, g.mcus_x & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    t.header_len = (int)(p - t.header);      // kJpegEncHeaderLen
}

constexpr size_t kJpegEncScratch = (size_t)256 << 20;      // PF_JPEG_ENC_SCRATCH of the header

}  // namespace

extern "C" {

int pf_device_alloc(pf_handle* h, size_t bytes, void** out) {
    if (!h) return 1;
    if (!out || bytes == 0) PF_FAIL(h, "pf_device_alloc: bad arguments");
    *out = nullptr;
    PF_HIP(h, hipSetDevice(h->device));
    PF_HIP(h, hipMalloc(out, bytes));
    return 0;
}

int pf_device_free(pf_handle* h, void* p) {
    if (!h) return 1;
    if (!p) return 0;
    PF_HIP(h, hipSetDevice(h->device));
    PF_HIP(h, hipStreamSynchronize(h->stream));      // work in flight may still read or write it
    PF_HIP(h, hipFree(p));
    return 0;
}

size_t pf_encode_jpeg_bound(int height, int width, int subsampling) {
    const JpegEncGeom g = jpeg_enc_geom(height, width, subsampling);
    return g.ok ? (size_t)g.bound : 0;
}

int pf_encode_jpeg(pf_handle* h, const uint8_t* images, int mem, int n, int height, int width, int row_stride, int quality,
                   int subsampling, uint8_t* out, size_t capacity, int* sizes, int out_mem) {
    if (!h) return 1;
    if (quality < 1 || quality > 100) PF_FAIL(h, "pf_encode_jpeg: quality must lie in [1, 100] (got %d)", quality);
    if (subsampling != 444 && subsampling != 422 && subsampling != 420)
        PF_FAIL(h, "pf_encode_jpeg: subsampling must be 444, 422 or 420 (got %d)", subsampling);
    if (height < 1 || width < 1 || height > 65535 || width > 65535)
        PF_FAIL(h, "pf_encode_jpeg: height and width must lie in [1, 65535] (got %d x %d)", height, width);
    const JpegEncGeom g = jpeg_enc_geom(height, width, subsampling);
    if (!g.ok) PF_FAIL(h, "pf_encode_jpeg: %d x %d is too large: the bound of a file's length must fit an int", height, width);
    if (mem != PF_MEM_HOST && mem != PF_MEM_DEVICE && mem != PF_MEM_RESIDENT)
        PF_FAIL(h, "pf_encode_jpeg: mem must be PF_MEM_HOST, PF_MEM_DEVICE or PF_MEM_RESIDENT (got %d)", mem);
    if (out_mem != PF_MEM_HOST && out_mem != PF_MEM_DEVICE) PF_FAIL(h, "pf_encode_jpeg: out_mem must be PF_MEM_HOST or PF_MEM_DEVICE (got %d)", out_mem);
    if (n < 1) PF_FAIL(h, "pf_encode_jpeg: n must be at least 1 (got %d)", n);
    if (!out || !sizes) PF_FAIL(h, "pf_encode_jpeg: out and sizes must not be NULL");
    if (!images && mem != PF_MEM_RESIDENT) PF_FAIL(h, "pf_encode_jpeg: images must not be NULL");
    if (row_stride < 3 * width) PF_FAIL(h, "pf_encode_jpeg: row_stride %d is below 3 * width = %d", row_stride, 3 * width);
    if (capacity < (size_t)kJpegEncHeaderLen) PF_FAIL(h, "pf_encode_jpeg: capacity %zu is below the header's %d bytes", capacity, kJpegEncHeaderLen);
    if (mem == PF_MEM_RESIDENT) {
        if (n != 1) PF_FAIL(h, "pf_encode_jpeg: PF_MEM_RESIDENT is one frame, n = %d", n);
        if (!h->pipe.have_cur || h->pipe.cur_h != height || h->pipe.cur_w != width)
            PF_FAIL(h, "pf_encode_jpeg: no resident frame of this size (call pf_set_frame first)");
        images = h->pipe.d_cur;
        row_stride = 3 * width;
    }
    PF_HIP(h, hipSetDevice(h->device));
    JpegEncState& s = h->jpeg_enc;
    const int key[4] = {height, width, quality, subsampling};
    if (!s.d_tab || memcmp(key, s.key, sizeof(key)) != 0) {
        if (scratch_ensure(h, s.d_tab, s.tab_bytes, sizeof(JpegEncTables))) return 1;
        PF_HIP(h, hipStreamSynchronize(h->stream));          // calls in flight read the tables that are replaced
        jpeg_enc_tables(s.h_tab, height, width, quality, g);
        PF_HIP(h, hipMemcpy(s.d_tab, &s.h_tab, sizeof(JpegEncTables), hipMemcpyHostToDevice));
        memcpy(s.key, key, sizeof(key));
    }
    // chunks of images: the scratch of a chunk stays below kJpegEncScratch wherever one image does
    const size_t blocks = (size_t)g.nb * g.mcus_y;
    const size_t per_image = blocks * 128 + (size_t)g.mcus_y * ((size_t)g.words * 4 + 8);
    const size_t img_stride = (size_t)height * row_stride;
    const int strips = pf_div_up(g.mcus_x * 8 * g.hs, PF_JPEG_ENC_STRIP);
    size_t chunk = std::max<size_t>(1, kJpegEncScratch / per_image);
    chunk = std::min(chunk, (size_t)0x7fffffff / ((size_t)g.mcus_y * strips));
    if (out_mem == PF_MEM_HOST) chunk = std::min(chunk, std::max<size_t>(1, kJpegEncScratch / capacity));
    chunk = std::min(chunk, (size_t)n);
    if (chunk < 1) PF_FAIL(h, "pf_encode_jpeg: %d x %d has too many MCUs for one launch", height, width);
    if (scratch_ensure(h, s.d_coef, s.coef_bytes, chunk * blocks * 128)) return 1;
    if (scratch_ensure(h, s.d_bits, s.bits_bytes, chunk * g.mcus_y * (size_t)g.words * 4)) return 1;
    if (scratch_ensure(h, s.d_len, s.len_bytes, chunk * g.mcus_y * 8)) return 1;
    if (mem == PF_MEM_HOST && scratch_ensure(h, s.d_in, s.in_bytes, chunk * img_stride)) return 1;
    if (out_mem == PF_MEM_HOST) {
        if (scratch_ensure(h, s.d_out, s.out_bytes, chunk * capacity)) return 1;
        if (scratch_ensure(h, s.d_sizes, s.sizes_bytes, chunk * sizeof(int))) return 1;
    }
    JpegEncArgs a{};
    a.img_stride = (long long)img_stride; a.row_stride = row_stride; a.H = height; a.W = width; a.hs = g.hs; a.vs = g.vs;
    a.mcus_x = g.mcus_x; a.mcus_y = g.mcus_y; a.bpm = g.bpm; a.strips = strips; a.G = PF_JPEG_ENC_STRIP / (8 * g.hs);
    a.wb = pf_div_up(width, 8); a.hb = pf_div_up(height, 8); a.ch = pf_div_up(height, g.vs);
    a.tab = s.d_tab; a.coef = s.d_coef; a.bits = s.d_bits; a.words = g.words; a.len = s.d_len; a.capacity = capacity;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += chunk) {
        const int c = (int)std::min(chunk, (size_t)n - i0);
        a.n = c;
        a.images = images + i0 * img_stride;
        if (mem == PF_MEM_HOST) {                               // the last row of the last image ends at 3 * width
            PF_HIP(h, hipMemcpyAsync(s.d_in, a.images, (size_t)c * img_stride - (size_t)(row_stride - 3 * width), hipMemcpyHostToDevice, h->stream));
            a.images = s.d_in;
        }
        a.out = out_mem == PF_MEM_HOST ? s.d_out : out + i0 * capacity;
        a.sizes = out_mem == PF_MEM_HOST ? s.d_sizes : sizes + i0;
        {
            ProfScope ps(h, "jpeg_enc_blocks");
            PF_LAUNCH(jpeg_enc_blocks, dim3((unsigned)(c * g.mcus_y * strips)), dim3(256), h->stream, a);
        }
        {
            ProfScope ps(h, "jpeg_enc_entropy");
            PF_LAUNCH(jpeg_enc_entropy, dim3((unsigned)(c * g.mcus_y)), dim3(256), h->stream, a);
        }
        {
            ProfScope ps(h, "jpeg_enc_pack");
            PF_LAUNCH(jpeg_enc_pack, dim3((unsigned)(c * g.mcus_y)), dim3(256), h->stream, a);
        }
        PF_HIP(h, hipGetLastError());
        if (out_mem != PF_MEM_HOST) continue;
        PF_HIP(h, hipMemcpyAsync(sizes + i0, s.d_sizes, (size_t)c * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        PF_HIP(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < c; ++i)                             // the files only; a slot whose file does not fit is left alone
            if (sizes[i0 + i] > 0)
                PF_HIP(h, hipMemcpyAsync(out + (i0 + i) * capacity, s.d_out + (size_t)i * capacity, (size_t)sizes[i0 + i], hipMemcpyDeviceToHost, h->stream));
        PF_HIP(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

}  // extern "C"

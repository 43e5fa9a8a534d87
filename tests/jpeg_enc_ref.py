"""Numpy restatement of the baseline JPEG encoder of pf_encode_jpeg (csrc/k_jpeg_enc.h): integers only, the whole
file.  It is libjpeg(-turbo)'s default encoder (JDCT_ISLOW, standard Huffman tables, no optimisation pass) with one restart interval
per MCU row; tests/test_jpeg_encode.py pins it to Pillow byte for byte.  Colour, padding, down-sampling, DCT and quantisation are
vectorised over blocks; the entropy coder walks the blocks."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
# ITU T.81 K.1 / K.2, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                     99, 99] + [99] * 32)
# K.3 - K.6: code counts per length 1 .. 16, then the symbols
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
    "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
SAMPLING = {444: (1, 1), 422: (2, 1), 420: (2, 2)}


def _fix(x):
    return int(x * 65536 + 0.5)


def quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((b * s + 50) // 100, 1, 255).astype(np.int64) for b in (Q_LUMA, Q_CHROMA)]


def huff_codes(bits, vals):
    """symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def header(height, width, quality, subsampling):
    hs, vs = SAMPLING[subsampling]
    q = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([height >> 8, height & 255, width >> 8, width & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x10, AC_BITS[0], AC_VALS[0]), (0x01, DC_BITS[1], DC_VALS[1]),
                            (0x11, AC_BITS[1], AC_VALS[1])):
        n = 19 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, cls]) + bytes(bits) + bytes(vals)
    dri = -(-width // (8 * hs))
    out += b"\xff\xdd\x00\x04" + bytes([dri >> 8, dri & 255])
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def ycc(bgr):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def component_plane(p, hs, vs):
    """The padded, down-sampled plane of one component (hs, vs: its down-sampling factors), hb * 8 x wb * 8, and (hb, wb)."""
    H, W = p.shape
    cw, ch = -(-W // hs), -(-H // vs)
    wb, hb = -(-cw // 8), -(-ch // 8)
    p = np.concatenate([p, np.repeat(p[:, -1:], wb * 8 * hs - W, axis=1)], axis=1)
    p = np.concatenate([p, np.repeat(p[-1:], ch * vs - H, axis=0)], axis=0)
    if (hs, vs) == (2, 2):
        bias = 1 + (np.arange(wb * 8) & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif (hs, vs) == (2, 1):
        bias = np.arange(wb * 8) & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    p = np.concatenate([p, np.repeat(p[-1:], hb * 8 - ch, axis=0)], axis=0)
    return p, hb, wb


def _fdct_1d(d, first):
    """d [..., 8] along the last axis; the row pass (first) or the column pass of jfdctint"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15
    rnd = 1 << (sh - 1)
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    out[..., 2] = (z1 + t13 * 6270 + rnd) >> sh
    out[..., 6] = (z1 - t12 * 15137 + rnd) >> sh
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = (t4 + z1 + z3 + rnd) >> sh
    out[..., 5] = (t5 + z2 + z4 + rnd) >> sh
    out[..., 3] = (t6 + z2 + z3 + rnd) >> sh
    out[..., 1] = (t7 + z1 + z4 + rnd) >> sh
    return out


def quantised_blocks(plane, q):
    """plane [hb * 8][wb * 8] -> [hb][wb][64] quantised coefficients in zigzag order"""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _fdct_1d(d, True)
    d = _fdct_1d(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2).reshape(hb, wb, 64)
    div = 8 * q
    c = np.sign(d) * ((np.abs(d) + (div >> 1)) // div)
    return c[..., ZIGZAG]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _code_block(w, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    s = abs(diff).bit_length()
    w.put(*dc[s])
    if s:
        w.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        w.put(*ac[run << 4 | s])
        w.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        run = 0
    if run:
        w.put(*ac[0])
    return int(blk[0])


def scan_blocks(bgr, quality, subsampling):
    """The blocks of the scan in coding order, [mcu rows][blocks of the row][64] (zigzag), dummy blocks included, and the component of
    every block of a row."""
    hs, vs = SAMPLING[subsampling]
    H, W = bgr.shape[:2]
    q = quant_tables(quality)
    y, cb, cr = ycc(bgr)
    py, hby, wby = component_plane(y, 1, 1)
    by = quantised_blocks(py, q[0])
    bc = [quantised_blocks(component_plane(p, hs, vs)[0], q[1]) for p in (cb, cr)]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    rows, comps = [], []
    for r in range(my):
        row = []
        for m in range(mx):
            last = None
            for j in range(vs):
                for i in range(hs):
                    yy, xx = r * vs + j, m * hs + i
                    if yy < hby and xx < wby:
                        last = by[yy, xx]
                    else:                       # a block that does not exist: the DC of the block coded just before it, no AC
                        last = np.concatenate([last[:1], np.zeros(63, np.int64)])
                    row.append(last)
            row += [bc[0][r, m], bc[1][r, m]]
        rows.append(np.stack(row))
    comps = ([0] * (hs * vs) + [1, 2]) * mx
    return np.stack(rows), comps


def encode(bgr, quality=90, subsampling=420):
    """bgr [H][W][3] uint8 -> the JFIF file pf_encode_jpeg writes"""
    bgr = np.asarray(bgr)
    H, W = bgr.shape[:2]
    rows, comps = scan_blocks(bgr, quality, subsampling)
    dc = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
    ac = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]
    out = bytearray(header(H, W, quality, subsampling))
    for r in range(len(rows)):
        w = _Bits()
        pred = [0, 0, 0]
        for blk, c in zip(rows[r], comps):
            t = 1 if c else 0
            pred[c] = _code_block(w, blk, pred[c], dc[t], ac[t])
        w.flush()
        out += w.out
        out += b"\xff" + bytes([0xD0 + (r & 7)]) if r + 1 < len(rows) else b"\xff\xd9"
    return bytes(out)

"""Rules E1-E9 of include/mvs.h (the baseline JPEG encoder) restated in numpy and plain Python, operation for operation, and the
restatement of ``mvs_depth_preview``.  ``encode`` returns the stream; ``encode_all`` also the quantised coefficient blocks and the counters
the fixture-set test reads (stuffed FF bytes, ZRL symbols, dummy blocks, padded and byte-aligned interval ends); ``encode_coef`` is E6-E9
alone, on coefficients its caller chose, and also returns the bytes of every interval before stuffing.  The round trip of
``mvs_jpeg_roundtrip`` is ``ref_jpeg.decode(encode(x))``."""
import numpy as np

from tests.ref_jpeg import ZIGZAG                # the one statement of the zigzag order

ROW = 65536                                   # restart_interval: one MCU row per interval (MVS_JPEG_RESTART_ROW)
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = ([1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
            114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86,
            87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138,
            146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
            194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233,
            234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250],
           [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
            209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
            86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
            137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
            185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
            233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
SAMPLING = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}


def codes(bits, vals):
    """BITS / HUFFVAL -> {symbol: (code, length)} (T.81 C.2)"""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


DC_CODES = [codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
AC_CODES = [codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def quant_table(base, quality):
    """E5 -> 64 entries in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(255, max(1, (b * scale + 50) // 100)) for b in base]


def colour(rgb):
    """E2: [h, w, 3] R G B -> Y, Cb, Cr as int32 planes"""
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    """the plane extended by repeating its last column, then its last row"""
    p = np.concatenate([p] + [p[:, -1:]] * (cols - p.shape[1]), axis=1) if cols > p.shape[1] else p
    return np.concatenate([p] + [p[-1:]] * (rows - p.shape[0]), axis=0) if rows > p.shape[0] else p


def component_plane(full, hr, vr, hmax, vmax):
    """E3: a full-resolution plane -> the component's plane, whole MCUs wide and high (hr, vr: 2 where the component is halved)"""
    H, W = full.shape
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    p = _extend(full, -(-H // vmax) * vmax, mcux * 8 * hmax)
    if hr == 2 and vr == 1:
        bias = np.arange(p.shape[1] // 2, dtype=np.int32) & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif hr == 2 and vr == 2:
        bias = 1 + (np.arange(p.shape[1] // 2, dtype=np.int32) & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _extend(p, mcuy * 8 * vmax // vr, p.shape[1])


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """E4: jfdctint's butterfly on the last axis of d (int64 here; the values fit int32)"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 11 if first else 15
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2], out[..., 6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7], out[..., 5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    out[..., 3], out[..., 1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out


def blocks_of(plane, table):
    """E4, E5: a component plane [8 bh, 8 bw] -> quantised coefficients [bh, bw, 64] int16, natural order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _fdct_1d(d, True)                                            # rows
    d = _fdct_1d(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    c = d.reshape(bh, bw, 64)
    e = np.asarray(table, np.int64)
    q = (np.abs(c) + 4 * e) // (8 * e)
    return np.where(c < 0, -q, q).astype(np.int16)


class Writer:
    """E7: bits MSB first, FF followed by 00"""

    def __init__(self):
        self.out, self.raw, self.acc, self.n, self.stuffed, self.bits = bytearray(), bytearray(), 0, 0, 0, 0   # raw: the bytes before stuffing

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        self.bits += length
        while self.n >= 8:
            self.n -= 8
            self._byte((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def _byte(self, b):
        self.out.append(b)
        self.raw.append(b)
        if b == 255:
            self.out.append(0)
            self.stuffed += 1

    def flush(self):
        """fills the last byte with 1 bits -> whether it had to"""
        if self.n == 0:
            return False
        self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return True


def _size(v):
    return int(abs(int(v))).bit_length()


def encode_block(w, blk, pred, dc, ac, count, seen=None):
    """E7: one block of 64 coefficients in natural order (None: a dummy block) -> the new predictor.  seen (optional): dict(dc, ac: sets
    that receive (symbol, value > 0) of every symbol of a real block, (symbol, None) where no value follows; bits: the longest real block)"""
    if blk is None:
        w.put(*dc[0])
        w.put(*ac[0])
        return pred
    start = w.bits
    d = int(blk[0]) - pred
    s = _size(d)
    w.put(*dc[s])
    if s:
        w.put((d if d >= 0 else d - 1) & ((1 << s) - 1), s)
    if seen is not None:
        seen["dc"].add((s, d > 0 if s else None))
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            count["zrl"] += 1
            run -= 16
            if seen is not None:
                seen["ac"].add((0xF0, None))
        s = _size(v)
        w.put(*ac[(run << 4) | s])
        w.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        if seen is not None:
            seen["ac"].add(((run << 4) | s, v > 0))
        run = 0
    if run:
        w.put(*ac[0])
    if seen is not None:
        if run:
            seen["ac"].add((0, None))
        seen["bits"] = max(seen["bits"], w.bits - start)
    return int(blk[0])


def header(W, H, mode, quality, restart):
    """E8: everything in front of the scan"""
    grey = mode == "grey"
    hmax, vmax = SAMPLING[mode]
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    tables = [quant_table(K1, quality)] + ([] if grey else [quant_table(K2, quality)])
    for t, q in enumerate(tables):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(q[ZIGZAG[k]] for k in range(64))
    nc = 1 if grey else 3
    out += b"\xff\xc0" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    out += bytes([1, (hmax << 4) | vmax, 0])
    if not grey:
        out += bytes([2, 0x11, 1, 3, 0x11, 1])
    for t in range(1 if grey else 2):
        for cls, bits, vals in ((0, DC_BITS[t], DC_VALS[t]), (1, AC_BITS[t], AC_VALS[t])):
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(cls << 4) | t]) + bytes(bits) + bytes(vals)
    if restart:
        out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * nc).to_bytes(2, "big") + bytes([nc, 1, 0x00])
    if not grey:
        out += bytes([2, 0x11, 3, 0x11])
    return bytes(out + b"\x00\x3f\x00")


def encode_all(img, mode="420", quality=95, restart_interval=0, order="RGB"):
    """img: [h, w, 3] uint8 in ``order``, or [h, w] with mode "grey" -> (stream, coefficient arrays per component [bh, bw, 64] with the
    dummy blocks zero, counters)"""
    img = np.asarray(img)
    grey = mode == "grey"
    assert img.dtype == np.uint8 and img.ndim == (2 if grey else 3)
    H, W = img.shape[:2]
    hmax, vmax = SAMPLING[mode]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    if grey:
        comps = [(img.astype(np.int32), 1, 1, 0)]
    else:
        y, cb, cr = colour(img if order == "RGB" else img[..., ::-1])
        comps = [(y, 1, 1, 0), (cb, hmax, vmax, 1), (cr, hmax, vmax, 1)]
    tables = [quant_table(K1, quality), quant_table(K2, quality)]
    coef, real = [], []
    for full, hr, vr, t in comps:
        c = blocks_of(component_plane(full, hr, vr, hmax, vmax), tables[t])
        cw, ch = -(-W // hr), -(-H // vr)
        rb = (-(-ch // 8), -(-cw // 8))                              # E6: the real blocks
        c[rb[0]:] = 0
        c[:, rb[1]:] = 0
        coef.append(c)
        real.append(rb)
    stream, _, count = encode_coef(coef, W, H, mode, quality, restart_interval)
    return stream, coef, count


def encode_coef(coef, W, H, mode, quality, restart_interval, seen=None):
    """E6-E9 on given coefficients: per component an int16 array [bh, bw, 64] over the padded plane, natural order inside a block; what
    stands at a dummy block is ignored -> (stream, the unstuffed bytes of every restart interval, counters).  seen (optional): per table
    (0 luma, 1 chroma) what ``encode_block`` records"""
    grey = mode == "grey"
    hmax, vmax = SAMPLING[mode]
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    comps = [(1, 1, 0)] if grey else [(1, 1, 0), (hmax, vmax, 1), (hmax, vmax, 1)]
    assert len(coef) == len(comps)
    real = []
    for c, (hr, vr, _) in zip(coef, comps):
        assert c.shape == (mcuy * vmax // vr, mcux * hmax // hr, 64) and c.dtype == np.int16
        real.append((-(-(-(-H // vr)) // 8), -(-(-(-W // hr)) // 8)))   # E6: the real blocks
    restart = mcux if restart_interval == ROW else restart_interval
    per = restart if restart else mcux * mcuy
    count = dict(stuffed=0, zrl=0, dummy_col=0, dummy_row=0, padded_end=0, aligned_end=0)
    out = bytearray(header(W, H, mode, quality, restart))
    raws = []
    n_int = -(-mcux * mcuy // per)
    for t in range(n_int):
        w, pred = Writer(), [0, 0, 0]
        for m in range(t * per, min((t + 1) * per, mcux * mcuy)):
            my, mx = divmod(m, mcux)
            for ci, (hr, vr, tab) in enumerate(comps):
                hs, vs = (hmax // hr, vmax // vr) if not grey else (1, 1)
                for j in range(vs):
                    for i in range(hs):
                        by, bx = my * vs + j, mx * hs + i
                        dummy = by >= real[ci][0] or bx >= real[ci][1]
                        if dummy:
                            count["dummy_row" if by >= real[ci][0] else "dummy_col"] += 1
                        pred[ci] = encode_block(w, None if dummy else coef[ci][by, bx], pred[ci], DC_CODES[tab], AC_CODES[tab], count,
                                                 None if seen is None else seen[tab])
        count["padded_end" if w.flush() else "aligned_end"] += 1
        count["stuffed"] += w.stuffed
        out += w.out
        raws.append(bytes(w.raw))
        if t + 1 < n_int:
            out += bytes([0xFF, 0xD0 + (t & 7)])
    return bytes(out + b"\xff\xd9"), raws, count


def encode(img, mode="420", quality=95, restart_interval=0, order="RGB"):
    return encode_all(img, mode, quality, restart_interval, order)[0]


def depth_preview(d):
    """``mvs_depth_preview`` for one raster [h, w] float32 -> uint8 [h, w]"""
    d = np.asarray(d, np.float32)
    valid = (d >= 0) & (d < np.inf)                                  # NaN is not; +inf counts as invalid too
    out = np.full(d.shape, 255, np.uint8)
    if not valid.any():
        return out
    lo, hi = np.float64(d[valid].min()), np.float64(d[valid].max())
    if hi == lo:
        out[valid] = 0
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        v = 255.0 * (d.astype(np.float64) - lo) / (hi - lo)
    out[valid] = np.trunc(v[valid]).astype(np.uint8)
    return out

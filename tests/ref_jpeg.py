"""Numpy restatement of rules J1-J7 of include/mvs.h (the baseline JPEG decoder; csrc/jpeg_rules.h is the C++ body, csrc/jpeg.hip the
kernels).  Operation for operation: the header walk and the segment table (J2), the serial entropy decode of every segment (J3), the
dequantisation and jidctint in wrapping int32 (J4), fancy chroma upsampling on the real samples (J5), the colour conversion (J6) and the
channel order (J7).  ``decode`` raises JpegError where the library returns MVS_E_IO; its text names the feature.

The oracle of the rules is libjpeg-turbo's default decompressor as Pillow runs it (tests/golden/jpeg, tests/make_jpeg_golden.py)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
E_BITS, E_CODE, E_RUN, E_SIZE = 1, 2, 3, 4            # the error word of a segment (J3)
ERR_TEXT = {E_BITS: "scan: out of bits", E_CODE: "scan: a code that is not in its table", E_RUN: "scan: a run past coefficient 63",
            E_SIZE: "scan: size category above 15"}


class JpegError(Exception):
    pass


class Huff:
    """canonical codes from BITS / HUFFVAL: the 8-bit look-ahead table and the maxcode / valoff fall-back"""

    def __init__(self, bits, vals):
        self.look_n = np.zeros(256, np.int32)
        self.look_v = np.zeros(256, np.int32)
        self.maxcode = np.full(17, -1, np.int64)
        self.valoff = np.zeros(17, np.int64)
        self.vals = list(vals)
        code, p = 0, 0
        for l in range(1, 17):
            if bits[l - 1]:
                self.valoff[l] = p - code
                for _ in range(bits[l - 1]):
                    if code >= 1 << l:
                        raise JpegError("Huffman table: code lengths overflow")
                    if l <= 8:
                        lo = code << (8 - l)
                        self.look_n[lo:lo + (1 << (8 - l))] = l
                        self.look_v[lo:lo + (1 << (8 - l))] = vals[p]
                    code += 1
                    p += 1
                self.maxcode[l] = code - 1
            code <<= 1


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """J1, J2: -> dict(w, h, ncomp, sof, restart, comps [(h, v, tq, td, ta)], quant {id: int32[64] natural order}, huff {(class, id): Huff},
    segments [(first, end, mcu0, nmcu)], mcux, mcuy)"""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise JpegError("not a JPEG stream (no SOI)")
    p = 2
    quant, huff = {}, {}
    frame = None
    restart = 0
    adobe = None
    while True:
        if p + 4 > n:
            raise JpegError("header: truncated")
        if d[p] != 0xFF:
            raise JpegError("header: marker expected")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        if m == 0xD8 or (0xD0 <= m <= 0xD7) or m == 0x01:
            continue
        if m == 0xD9:
            raise JpegError("header: EOI before a scan")
        ln = _u16(d, p)
        if ln < 2 or p + ln > n:
            raise JpegError("header: truncated")
        s, e = p + 2, p + ln
        if m == 0xC0 or m == 0xC1:
            if frame is not None:
                raise JpegError("more than one frame")
            if e - s < 6:
                raise JpegError("header: truncated")
            prec, h, w, nc = d[s], _u16(d, s + 1), _u16(d, s + 3), d[s + 5]
            if prec != 8:
                raise JpegError("12-bit samples")
            if nc != 1 and nc != 3:
                raise JpegError("%d components" % nc)
            if e - s != 6 + 3 * nc:
                raise JpegError("header: bad SOF length")
            if w == 0 or h == 0:
                raise JpegError("header: empty frame")
            comps = [[d[s + 6 + 3 * i], d[s + 7 + 3 * i] >> 4, d[s + 7 + 3 * i] & 15, d[s + 8 + 3 * i]] for i in range(nc)]
            frame = dict(w=w, h=h, ncomp=nc, sof=m - 0xC0, ids=[c[0] for c in comps], samp=[(c[1], c[2]) for c in comps], tq=[c[3] for c in comps])
        elif m == 0xC2:
            raise JpegError("progressive")
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise JpegError("arithmetic coding")
        elif m in (0xC3, 0xC5, 0xC6, 0xC7):
            raise JpegError("lossless or hierarchical")
        elif m == 0xCC:
            raise JpegError("arithmetic coding")
        elif m == 0xDB:
            while s < e:
                pq, tq = d[s] >> 4, d[s] & 15
                if pq > 1 or tq > 3 or s + 1 + 64 * (pq + 1) > e:
                    raise JpegError("header: bad DQT")
                q = np.zeros(64, np.int32)
                for k in range(64):
                    q[ZIGZAG[k]] = _u16(d, s + 1 + 2 * k) if pq else d[s + 1 + k]
                quant[tq] = q
                s += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            while s < e:
                tc, th = d[s] >> 4, d[s] & 15
                if tc > 1 or th > 3 or s + 17 > e:
                    raise JpegError("header: bad DHT")
                bits = list(d[s + 1:s + 17])
                cnt = sum(bits)
                if cnt > 256 or s + 17 + cnt > e:
                    raise JpegError("header: bad DHT")
                huff[(tc, th)] = Huff(bits, list(d[s + 17:s + 17 + cnt]))
                s += 17 + cnt
        elif m == 0xDD:
            if ln != 4:
                raise JpegError("header: bad DRI")
            restart = _u16(d, s)
        elif m == 0xEE:
            if ln >= 14 and d[s:s + 5] == b"Adobe":
                adobe = d[s + 11]
        elif m == 0xDA:
            if frame is None:
                raise JpegError("header: SOS before SOF")
            ns = d[s] if e > s else 0
            if ns != frame["ncomp"]:
                raise JpegError("non-interleaved or multi-scan")
            if e - s != 4 + 2 * ns:
                raise JpegError("header: bad SOS length")
            td, ta = [], []
            for i in range(ns):
                if d[s + 1 + 2 * i] != frame["ids"][i]:
                    raise JpegError("non-interleaved or multi-scan")
                td.append(d[s + 2 + 2 * i] >> 4)
                ta.append(d[s + 2 + 2 * i] & 15)
            p = e
            break
        p = e
    nc = frame["ncomp"]
    if nc == 3 and adobe == 0:
        raise JpegError("Adobe transform 0")
    samp = frame["samp"]
    if nc == 1:
        samp = [(1, 1)]
    else:
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise JpegError("sampling factors")
    for i in range(nc):
        if frame["tq"][i] > 3 or frame["tq"][i] not in quant:
            raise JpegError("header: missing quantisation table")
        if td[i] > 3 or ta[i] > 3 or (0, td[i]) not in huff or (1, ta[i]) not in huff:
            raise JpegError("header: missing Huffman table")
    hmax, vmax = samp[0]
    mcux = -(-frame["w"] // (8 * hmax))
    mcuy = -(-frame["h"] // (8 * vmax))
    total = mcux * mcuy
    per = restart if restart else total
    want = -(-total // per)
    segs = []
    first = p
    while True:
        q, marker = first, 0                                  # marker 0: the data ended inside the scan
        while q < n:
            if d[q] == 0xFF and q + 1 < n and d[q + 1] != 0 and d[q + 1] != 0xFF:
                marker = d[q + 1]
                break
            q += 1
        if len(segs) == want:
            raise JpegError("scan: more restart intervals than the frame has")
        segs.append((first, q, len(segs) * per, min(per, total - len(segs) * per)))
        if not (0xD0 <= marker <= 0xD7):
            break
        first = q + 2
    if len(segs) != want:
        raise JpegError("scan: %d of %d restart intervals" % (len(segs), want))
    if marker != 0 and marker != 0xD9:
        raise JpegError("non-interleaved or multi-scan")
    return dict(w=frame["w"], h=frame["h"], ncomp=nc, sof=frame["sof"], restart=restart, samp=samp, quant=[quant[frame["tq"][i]] for i in range(nc)],
                dc=[huff[(0, td[i])] for i in range(nc)], ac=[huff[(1, ta[i])] for i in range(nc)], segments=segs, mcux=mcux, mcuy=mcuy)


def info(data):
    h = parse(data)
    return dict(w=h["w"], h=h["h"], components=h["ncomp"], h_samp=h["samp"][0][0], v_samp=h["samp"][0][1], restart_interval=h["restart"],
                n_segments=len(h["segments"]), sof=h["sof"])


class Bits:
    """J3's bit reader over one segment: it never reads outside [first, end)"""

    def __init__(self, d, first, end):
        self.d, self.pos, self.end, self.acc, self.n = d, first, end, 0, 0

    def fill(self):
        while self.n <= 24 and self.pos < self.end:
            b = self.d[self.pos]
            self.pos += 1
            if b == 0xFF:
                if self.pos < self.end and self.d[self.pos] == 0:
                    self.pos += 1
                else:
                    self.pos = self.end
                    break
            self.acc = ((self.acc << 8) | b) & 0xFFFFFFFF
            self.n += 8

    def peek16(self):
        self.fill()
        return (self.acc >> (self.n - 16)) & 0xFFFF if self.n >= 16 else (self.acc << (16 - self.n)) & 0xFFFF

    def skip(self, l):
        if l > self.n:
            return False
        self.n -= l
        return True

    def get(self, s):
        self.fill()
        if s > self.n:
            return -1
        self.n -= s
        return (self.acc >> self.n) & ((1 << s) - 1)


def _symbol(b, t):
    """-> (symbol, 0) or (0, error)"""
    pk = b.peek16()
    l = int(t.look_n[pk >> 8])
    if l:
        v = int(t.look_v[pk >> 8])
    else:
        l = 9
        while l <= 16 and (pk >> (16 - l)) > t.maxcode[l]:
            l += 1
        if l > 16:
            return 0, E_CODE
        at = (pk >> (16 - l)) + int(t.valoff[l])
        if at < 0 or at >= len(t.vals):
            return 0, E_CODE
        v = t.vals[at]
    if not b.skip(l):
        return 0, E_BITS
    return v, 0


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _i16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def decode_block(b, dc, ac, pred, out):
    """one block into out[64] (zero on entry, natural order) -> (pred, error)"""
    s, err = _symbol(b, dc)
    if err:
        return pred, err
    if s > 15:
        return pred, E_SIZE
    if s:
        v = b.get(s)
        if v < 0:
            return pred, E_BITS
        pred = _i32(pred + _extend(v, s))
    out[0] = _i16(pred)
    k = 1
    while k < 64:
        rs, err = _symbol(b, ac)
        if err:
            return pred, err
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 64:
                return pred, E_RUN
            continue
        k += r
        if k > 63:
            return pred, E_RUN
        v = b.get(s)
        if v < 0:
            return pred, E_BITS
        out[ZIGZAG[k]] = _i16(_extend(v, s))
        k += 1
    return pred, 0


def layout(h):
    """per component: blocks per row / column of the padded plane, real samples per row / column"""
    hmax, vmax = h["samp"][0]
    out = []
    for (hs, vs) in h["samp"]:
        out.append(dict(bw=h["mcux"] * hs, bh=h["mcuy"] * vs, cw=-(-h["w"] * hs // hmax), ch=-(-h["h"] * vs // vmax), hs=hs, vs=vs))
    return out


def entropy(data, h):
    """J3 -> (coefficients per component int16 [bh * bw, 64], error word)"""
    d = bytes(data)
    lay = layout(h)
    coef = [np.zeros((l["bh"] * l["bw"], 64), np.int16) for l in lay]
    error = 0
    for (first, end, mcu0, nmcu) in h["segments"]:
        b = Bits(d, first, end)
        pred = [0] * h["ncomp"]
        err = 0
        for m in range(mcu0, mcu0 + nmcu):
            my, mx = divmod(m, h["mcux"])
            for c, l in enumerate(lay):
                for j in range(l["vs"]):
                    for i in range(l["hs"]):
                        if err:
                            continue
                        blk = coef[c][(my * l["vs"] + j) * l["bw"] + mx * l["hs"] + i]
                        pred[c], err = decode_block(b, h["dc"][c], h["ac"][c], pred[c], blk)
                        if err:
                            blk[:] = 0                    # the block that failed is written as zeros, like those behind it
        if err and not error:
            error = err
    return coef, error


def _descale(x, n):
    return (x + np.int32(1 << (n - 1))) >> np.int32(n)


def _idct_1d(x, shift, first):
    """jidctint's butterfly along axis 1 of x [N, 8, 8] int32 (wrapping)"""
    i = np.int32
    z2, z3 = x[:, 2], x[:, 6]
    z1 = (z2 + z3) * i(4433)
    tmp2 = z1 - z3 * i(15137)
    tmp3 = z1 + z2 * i(6270)
    z2, z3 = x[:, 0], x[:, 4]
    tmp0 = (z2 + z3) << i(13)
    tmp1 = (z2 - z3) << i(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[:, 7], x[:, 5], x[:, 3], x[:, 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * i(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * i(2446), tmp1 * i(16819), tmp2 * i(25172), tmp3 * i(12299)
    z1, z2, z3, z4 = z1 * i(-7373), z2 * i(-20995), z3 * i(-16069) + z5, z4 * i(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([_descale(tmp10 + tmp3, shift), _descale(tmp11 + tmp2, shift), _descale(tmp12 + tmp1, shift), _descale(tmp13 + tmp0, shift),
                     _descale(tmp13 - tmp0, shift), _descale(tmp12 - tmp1, shift), _descale(tmp11 - tmp2, shift), _descale(tmp10 - tmp3, shift)], axis=1)


def idct(coef, quant):
    """J4: int16 [N, 64] -> uint8 [N, 8, 8]"""
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * quant.astype(np.int32)[None, :]).reshape(-1, 8, 8)
        ws = _idct_1d(x, 11, True)                                      # columns: axis 1 is the row index v, the transform runs down it
        px = _idct_1d(ws.transpose(0, 2, 1), 18, False).transpose(0, 2, 1)   # rows
        return np.clip(px + np.int32(128), 0, 255).astype(np.uint8)


def planes(h, coef):
    """J4 for every component -> padded planes uint8 [bh * 8, bw * 8]"""
    out = []
    for c, l in enumerate(layout(h)):
        b = idct(coef[c], h["quant"][c]).reshape(l["bh"], l["bw"], 8, 8)
        out.append(np.ascontiguousarray(b.transpose(0, 2, 1, 3).reshape(l["bh"] * 8, l["bw"] * 8)))
    return out


def _h2(p, three, lo_add, hi_add, shift):
    """the horizontal half of J5 on rows p [rows, cw] int32: out[2i] from the left neighbour, out[2i+1] from the right"""
    rows, cw = p.shape
    out = np.zeros((rows, 2 * cw), np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out[:, 0::2] = (three * p + left + lo_add) >> shift
    out[:, 1::2] = (three * p + right + hi_add) >> shift
    return out


def upsample(plane, l, hmax, vmax, W, H):
    """J5: the real cw x ch samples of a padded plane -> [H, W] int32"""
    p = plane[:l["ch"], :l["cw"]].astype(np.int32)
    hr, vr = hmax // l["hs"], vmax // l["vs"]
    if hr == 1 and vr == 1:
        return p[:H, :W]
    if l["cw"] <= 2:                                          # a plane this narrow is replicated in both directions
        return np.repeat(np.repeat(p, vr, axis=0), hr, axis=1)[:H, :W]
    if vr == 1:
        out = _h2(p, 3, 1, 2, 2)
        out[:, 0] = p[:, 0]
        out[:, 2 * l["cw"] - 1] = p[:, -1]
        return out[:H, :W]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    dn = np.concatenate([p[1:], p[-1:]], axis=0)
    s = np.zeros((2 * l["ch"], l["cw"]), np.int32)
    s[0::2] = 3 * p + up
    s[1::2] = 3 * p + dn
    out = _h2(s, 3, 8, 7, 4)
    out[:, 0] = (4 * s[:, 0] + 8) >> 4
    out[:, 2 * l["cw"] - 1] = (4 * s[:, -1] + 7) >> 4
    return out[:H, :W]


def colour(y, cb, cr):
    """J6 on int32 rasters -> r, g, b uint8"""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return [np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b)]


def pixels(h, pl, order="RGB"):
    """J5-J7 -> [H, W, 3] uint8"""
    lay = layout(h)
    W, H = h["w"], h["h"]
    hmax, vmax = h["samp"][0]
    if h["ncomp"] == 1:
        y = pl[0][:H, :W]
        return np.stack([y, y, y], axis=2)
    ch = [upsample(pl[c], lay[c], hmax, vmax, W, H) for c in range(3)]
    r, g, b = colour(*ch)
    return np.stack([r, g, b] if order == "RGB" else [b, g, r], axis=2)


def decode_all(data, order="RGB"):
    """-> (header, coefficients, planes, pixels); JpegError where the library fails with MVS_E_IO"""
    h = parse(data)
    coef, err = entropy(data, h)
    if err:
        raise JpegError(ERR_TEXT[err])
    pl = planes(h, coef)
    return h, coef, pl, pixels(h, pl, order)


def decode(data, order="RGB"):
    return decode_all(data, order)[3]

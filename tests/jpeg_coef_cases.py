"""Coefficient blocks chosen to reach what pixels cannot: the inputs of ``mvs_test_jpeg_encode_coef`` (include/mvs_test.h) and, through
the streams ``ref_jpeg_enc.encode_coef`` writes from them, of the decoder.  Shared by tests/test_jpeg_coef_host.py (no GPU) and
tests/test_gpu_jpeg_coef.py.  Every case is seeded by its name; a case is a list of int16 arrays [bh, bw, 64], one per component over
its padded plane, natural order inside a block.  The dummy blocks (E6) hold 32767 everywhere, which nothing may read.

    ff     every block has 1023 at zigzag 16, 32 and 48 and DC 0: ``1111111111111110 1111111111`` three times per luma block
    sym    every (run 0..15, size 1..10) AC symbol of the component's table in both signs, packed greedily into blocks, and a block that is
           three ZRLs and one coefficient; the DCs cycle through -1024, 1023, 0, 0, 1, -1, 511, -512
    zrl    blocks whose only nonzeros stand at zigzag {63}, {17}, {33}, {49}, {62}, {1, 63}, {16, 32, 48}, {17, 34, 51}, and all-zero blocks
    rand   half the ACs nonzero, sizes uniform in 1..10, random signs, DC uniform in -1024..1023
    long   rand at density 0.6 on 75x100 4:4:4 without restart markers: one segment of about 27 KB
    max    all 63 ACs alternating +-1023, DC alternating -1024 / 1023: the longest blocks of the standard tables

``measure()`` reads, from the restatement's unstuffed bytes alone, the figures tests/test_jpeg_coef_host.py asserts, so that the cases cannot
quietly stop reaching the paths they were made for."""
import zlib

import numpy as np

from tests import ref_jpeg_enc as E
from tests.ref_jpeg import ZIGZAG

ROW = E.ROW
MODES = ("grey", "444", "422", "420")
SIZES = {"8x8": (8, 8), "17x23": (17, 23), "33x50": (33, 50), "75x100": (75, 100)}       # h x w
CHUNK = 1024                                                       # the stuffing chunk of csrc/jpeg_enc.hip in unstuffed bytes
RING = 2048                                                        # the decoder's byte ring of csrc/jpeg.hip
DUMMY = 32767                                                      # at the dummy blocks: a value E7 has no code for
ZRL_SETS = ((63,), (17,), (33,), (49,), (62,), (1, 63), (16, 32, 48), (17, 34, 51), ())
DC_CYCLE = (-1024, 1023, 0, 0, 1, -1, 511, -512)


def _cases():
    """-> {name: dict(kind, h, w, mode, restart, quality, golden)}: every mode with every kind, every restart form with ff and rand, every
    size; golden: Pillow decodes the stream to the restatement's pixels and tests/golden/jpeg_coef holds them"""
    out = {}

    def add(kind, size, mode, restart=0, quality=100, golden=False):
        r = {0: "", ROW: "_rstrow"}.get(restart, f"_rst{restart}")
        q = "" if quality == 100 else f"_q{quality}"
        h, w = SIZES[size]
        out[f"{kind}_{size}_{mode}{r}{q}"] = dict(kind=kind, h=h, w=w, mode=mode, restart=restart, quality=quality, golden=golden)

    for mode in MODES:
        add("ff", "33x50", mode, golden=True)
        add("sym", "75x100", mode, golden=True)
        add("zrl", "33x50", mode, golden=True)
        add("rand", "17x23", mode, golden=True)
        add("rand", "33x50", mode)
        add("max", "17x23", mode)
    add("long", "75x100", "444", golden=True)
    for k, restart in enumerate((1, 2, ROW)):                        # every restart form with ff and rand, the modes rotating
        for j, kind in enumerate(("ff", "rand")):
            add(kind, "33x50", MODES[(k + 2 * j) % 4], restart)
            add(kind, "17x23", MODES[(k + 2 * j + 1) % 4], restart)
    add("rand", "33x50", "grey", 2)
    add("max", "17x23", "grey", 1)
    add("max", "33x50", "444", 2)
    for k, kind in enumerate(("ff", "sym", "zrl", "rand", "max")):   # one block, and the sizes with dummy blocks
        add(kind, "8x8", MODES[k % 4])
        add(kind, "8x8", MODES[(k + 1) % 4], 1)
    for kind in ("ff", "sym", "zrl"):
        add(kind, "17x23", "422")
        add(kind, "17x23", "420", ROW)
    add("rand", "17x23", "420", quality=50)                          # other quantisers change the header and the pixels only
    add("rand", "33x50", "422", 1, quality=95)
    return out


CASES = _cases()
GOLDEN = sorted(k for k, v in CASES.items() if v["golden"])


def geometry(h, w, mode):
    """-> per component (blocks per column and row of the padded plane, real blocks per column and row)"""
    hmax, vmax = E.SAMPLING[mode]
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    comps = [(1, 1)] if mode == "grey" else [(1, 1), (hmax, vmax), (hmax, vmax)]
    return [((mcuy * vmax // vr, mcux * hmax // hr), (-(-(-(-h // vr)) // 8), -(-(-(-w // hr)) // 8))) for hr, vr in comps]


def _value(rng, size, positive):
    m = int(rng.integers(1 << (size - 1), 1 << size))
    return m if positive else -m


def _sym_blocks(rng):
    blocks, cur, k = [], np.zeros(64, np.int16), 1
    for variant in (0, 1):
        for run in range(16):
            for size in range(1, 11):
                if k + run > 63:
                    blocks.append(cur)
                    cur, k = np.zeros(64, np.int16), 1
                cur[ZIGZAG[k + run]] = _value(rng, size, (run + size + variant) % 2 == 0)
                k += run + 1
    blocks.append(cur)
    cur = np.zeros(64, np.int16)
    cur[ZIGZAG[63]] = -1                                             # ZRL ZRL ZRL (14, 1)
    blocks.append(cur)
    return blocks


def _zrl_blocks(rng):
    blocks = []
    for rep in range(3):
        for at in ZRL_SETS:
            b = np.zeros(64, np.int16)
            for k in at:
                b[ZIGZAG[k]] = _value(rng, (1, 10, int(rng.integers(1, 11)))[rep], bool(rng.integers(2)))
            b[0] = (0, 0, int(rng.integers(-64, 64)))[rep]
            blocks.append(b)
    return blocks


def _rand_block(rng, density):
    b = np.zeros(64, np.int16)
    for k in range(1, 64):
        if rng.random() < density:
            b[ZIGZAG[k]] = _value(rng, int(rng.integers(1, 11)), bool(rng.integers(2)))
    b[0] = int(rng.integers(-1024, 1024))
    return b


def make(kind, h, w, mode, seed, dc0=0):
    """the coefficient arrays of one image; dc0: the DC of the very first block of an ``ff`` image (shifts every bit behind it)"""
    rng = np.random.default_rng(seed)
    geo = geometry(h, w, mode)
    out = [np.full((bh, bw, 64), DUMMY, np.int16) for (bh, bw), _ in geo]
    lists = [_sym_blocks(rng), _sym_blocks(rng)] if kind == "sym" else [_zrl_blocks(rng)] * 2 if kind == "zrl" else None
    at = [0, 0]                                                      # blocks handed out per table
    for c, (_, (rh, rw)) in enumerate(geo):
        t = 1 if c else 0
        for by in range(rh):
            for bx in range(rw):
                i = at[t]
                at[t] += 1
                if kind == "ff":
                    b = np.zeros(64, np.int16)
                    b[ZIGZAG[[16, 32, 48]]] = 1023
                elif kind in ("sym", "zrl"):
                    b = lists[t][i % len(lists[t])].copy()
                    if kind == "sym":
                        b[0] = DC_CYCLE[(by * rw + bx) % len(DC_CYCLE)]
                elif kind in ("rand", "long"):
                    b = _rand_block(rng, 0.6 if kind == "long" else 0.5)
                else:
                    assert kind == "max"
                    b = np.zeros(64, np.int16)
                    b[ZIGZAG[1::2]], b[ZIGZAG[2::2]] = 1023, -1023
                    b[0] = -1024 if (by * rw + bx) % 2 == 0 else 1023
                out[c][by, bx] = b
    if kind == "ff":
        out[0][0, 0, 0] = dc0
    return out


_MADE, _ENCODED = {}, {}


def coef(name):
    """the arrays of case ``name``, made once; nobody writes to them"""
    if name not in _MADE:
        c = CASES[name]
        _MADE[name] = make(c["kind"], c["h"], c["w"], c["mode"], zlib.crc32(name.encode()))
        for a in _MADE[name]:
            a.flags.writeable = False
    return _MADE[name]


def flat(arrays):
    """component by component, blocks row-major, natural order inside a block: what mvs_test_jpeg_encode_coef takes for one image"""
    return np.concatenate([a.reshape(-1) for a in arrays])


def new_seen():
    return [dict(dc=set(), ac=set(), bits=0) for _ in range(2)]


def encoded(name):
    """the restatement on case ``name``, computed once -> (stream, unstuffed bytes per interval, counters, seen)"""
    if name not in _ENCODED:
        c, seen = CASES[name], new_seen()
        _ENCODED[name] = E.encode_coef(coef(name), c["w"], c["h"], c["mode"], c["quality"], c["restart"], seen) + (seen,)
    return _ENCODED[name]


_DECODED = {}


def decoded(name):
    """the decoder's restatement on the stream of case ``name``, computed once -> ref_jpeg.decode_all's (header, coefficients, planes,
    R G B pixels); B G R is the last axis reversed"""
    if name not in _DECODED:
        from tests import ref_jpeg as R
        _DECODED[name] = R.decode_all(encoded(name)[0], "RGB")
        _DECODED[name][3].flags.writeable = False
    return _DECODED[name]


# The call that puts FF on both sides of a chunk boundary of the call-wide unstuffed buffer and an FF into its last partial dword: images
# of ``ff`` 33x50 4:4:4 whose first DC differs, which shifts every later bit of the image.  The DCs were searched once (boundary_search)
BOUNDARY_DC0 = (0, 64, 256)


def boundary_call(dc0=None):
    """-> (arrays per image, the unstuffed bytes of the whole call)"""
    dc0 = BOUNDARY_DC0 if dc0 is None else dc0
    imgs = [make("ff", 33, 50, "444", 0, d) for d in dc0]
    raw = b"".join(b"".join(E.encode_coef(a, 50, 33, "444", 100, 0)[1]) for a in imgs)
    return imgs, raw


def boundary_figures(raw):
    """-> (chunk boundaries with FF on both sides, whether an FF lies in the last partial dword)"""
    both = [p for p in range(CHUNK, len(raw), CHUNK) if raw[p - 1] == 255 and raw[p] == 255]
    return both, len(raw) % 4 != 0 and 255 in raw[len(raw) // 4 * 4:]


def boundary_search():
    """the first (count, DCs) in a fixed order for which both figures hold"""
    import itertools
    dcs = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1023, -1, -2, -4)
    for n in (3, 4):
        for dc0 in itertools.product(dcs, repeat=n):
            both, tail = boundary_figures(boundary_call(dc0)[1])
            if both and tail:
                return dc0
    return None


def _ff_run(raw):
    best = cur = 0
    for b in raw:
        cur = cur + 1 if b == 255 else 0
        best = max(best, cur)
    return best


def measure(names=None):
    """-> (per case: dict of figures, the set of conditions it carries); everything from the restatement's unstuffed bytes and counters"""
    out = {}
    for name in names or CASES:
        c = CASES[name]
        stream, raws, count, seen = encoded(name)
        raw = b"".join(raws)
        starts = np.cumsum([0] + [len(r) for r in raws])
        share = raw.count(255) / len(raw)
        carries = set()
        if share >= 0.5:
            carries.add("half_ff")
        run = _ff_run(raw)
        if run >= 3:
            carries.add("ff_run3")
        if any(r[-1] == 255 for r in raws[:-1]):
            carries.add("ff_before_rst")
        if raws[-1][-1] == 255:
            carries.add("ff_before_eoi")
        if any(int(starts[i + 1] - 1) // CHUNK - int(starts[i]) // CHUNK >= 2 for i in range(len(raws))):
            carries.add("interval_spans_3_chunks")
        for k in range(0, len(raw), CHUNK):                          # a chunk that holds more than one whole interval
            if np.count_nonzero((starts[:-1] >= k) & (starts[1:] <= k + CHUNK)) > 1:
                carries.add("chunk_holds_intervals")
                break
        seg = max(len(r) + r.count(255) for r in raws)               # the segment as the decoder reads it, stuffing included
        if seg > 8 * RING:
            carries.add("segment_over_8_rings")
        elif seg > 2 * RING:
            carries.add("segment_over_2_rings")
        if seen[0]["bits"] == 1658:
            carries.add("block_1658_bits")
        if count["zrl"]:
            carries.add("zrl")
        out[name] = dict(bytes=len(stream), raw=len(raw), share=share, run=run, segment=seg, intervals=len(raws), carries=carries,
                         bits=max(s["bits"] for s in seen))
    return out


def coverage(names=None):
    """-> per table (0 luma, 1 chroma): the (symbol, sign) pairs of the AC symbols and of the DC categories all cases produce together"""
    ac, dc = [set(), set()], [set(), set()]
    for name in names or CASES:
        seen = encoded(name)[3]
        for t in range(2):
            ac[t] |= seen[t]["ac"]
            dc[t] |= seen[t]["dc"]
    return ac, dc

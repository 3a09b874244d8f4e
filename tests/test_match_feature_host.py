"""Host side of mvs_sift_match, mvs_sift_match_lists(_dev) (include/mvs.h): the argument checks, which answer before any device is
needed; the numpy restatement of the rules (tests/ref_match.py) against plain loops; and the scenarios of
tests/test_gpu_match_feature.py, checked here to hold what they are there for.  The GPU comparison is exact equality; what allows
that although the GPU's double acos may differ from numpy's by a few ulp is a condition on the INPUTS, asserted here for every
scenario: no threshold decision of the restatement is closer than 1e-9 to its threshold."""
import ctypes as C
import functools

import numpy as np

from multiviewstitch_amd import _lib
from tests import ref_match as RM

E_INVALID = -1
MARGIN = 1e-9


# ------------------------------------------------------------------ generators ----
def sift_like(rng, n):
    """random non-negative vectors, unit norm, clamped at 0.2, renormalised (SIFT's own normalisation)"""
    d = rng.gamma(0.6, 1.0, (n, 128))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.minimum(d, 0.2)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.astype(np.float32)


def noisy(rng, d, sigma):
    e = np.maximum(d + rng.normal(scale=sigma, size=d.shape), 0)
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def random_keys(rng, n, w=640, h=480):
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(1, 8, n), rng.uniform(-3.2, 3.2, n)], 1).astype(np.float32)


# -------------------------------------------------------------------- 1. tails ----
TAIL_VIEWS = 3
TAIL_LENGTHS1 = (0, 1, 15, 16, 17, 63, 64, 65, 130)
TAIL_LENGTHS2 = (64, 17, 130, 0, 65, 1, 16, 63, 15)
TAIL_FAR_FRAME = 1                                          # the frame of sequence 2 whose lists hold distractors only


@functools.lru_cache(maxsize=1)
def tails():
    """3 frames x 3 views per side; list l of sequence 1 = the first TAIL_LENGTHS1[l] descriptors of one pool (noisy); a list of
    sequence 2 holds noisy copies of a permuted part of the pool in its first ~60 % and distractors behind them — except the lists of
    frame TAIL_FAR_FRAME, which hold distractors only.  -> dict(keys1, descs1, keys2, descs2, truth); truth[(l1, l2)] = the set of
    (i, j) with j a copy of i."""
    rng = np.random.default_rng(21)
    pool = sift_like(rng, 130)
    keys1 = [random_keys(rng, n) for n in TAIL_LENGTHS1]
    descs1 = [noisy(rng, pool[:n], 0.012) for n in TAIL_LENGTHS1]
    keys2, descs2, src = [], [], []
    for l2, n in enumerate(TAIL_LENGTHS2):
        ncopy = 0 if l2 // TAIL_VIEWS == TAIL_FAR_FRAME else (n * 3 + 4) // 5
        which = rng.permutation(n)[:ncopy]                   # copies of pool[which], in this order
        d = np.concatenate([noisy(rng, pool[which], 0.1), sift_like(rng, n - ncopy)]) if n else np.zeros((0, 128), np.float32)
        keys2.append(random_keys(rng, n))
        descs2.append(d)
        src.append(which)
    truth = {(l1, l2): {(int(i), j) for j, i in enumerate(src[l2]) if i < n1} for l1, n1 in enumerate(TAIL_LENGTHS1) for l2 in range(9)}
    return dict(keys1=keys1, descs1=descs1, keys2=keys2, descs2=descs2, truth=truth)


@functools.lru_cache(maxsize=1)
def tails_expected():
    q = tails()
    return RM.match_feature(q["keys1"], q["descs1"], q["keys2"], q["descs2"], TAIL_VIEWS)


def test_tails_scenario():
    q = tails()
    raw, counts = tails_expected()
    ncopied = found = 0
    for (l1, l2), t in q["truth"].items():
        m = RM.match_pair(q["descs1"][l1], q["descs2"][l2])
        ncopied += len(t)
        found += len(t & {(int(i), int(j)) for i, j in m})
    sizes = np.array([[len(b) for b in row] for row in raw])
    print("tails: copied", ncopied, "matched", found, "bucket sizes", sizes.tolist(), "list pairs with matches", int((counts > 0).sum()))
    assert 0.3 * ncopied <= found <= 0.9 * ncopied
    assert (sizes == 0).any() and (sizes > 50).any()
    assert sorted(TAIL_LENGTHS1) == sorted(TAIL_LENGTHS2) == [0, 1, 15, 16, 17, 63, 64, 65, 130]
    assert counts.sum() == sizes.sum() and counts[TAIL_LENGTHS1.index(0)].sum() == 0


# ----------------------------------------------------------------- 2. unsigned ----
@functools.lru_cache(maxsize=1)
def unsigned():
    """70 x 90 descriptors built from bytes: six components of 150..230 in most of them (above 127, where a signed byte turns
    negative), the rest small; list 2 = permuted copies of list 1's bytes with +-3 noise, plus distractors.  Some descriptors then
    carry a 0.6 (quantises above 255: saturates), a negative value and a NaN (both give 0)."""
    rng = np.random.default_rng(22)

    def make(n):
        q = rng.integers(0, 24, (n, 128))
        for r in range(n):
            if r % 7 != 6:                                   # most descriptors
                q[r, rng.choice(128, 6, replace=False)] = rng.integers(150, 231, 6)
        return q
    q1 = make(70)
    perm = rng.permutation(70)[:60]
    q2 = np.concatenate([np.clip(q1[perm] + rng.integers(-3, 4, (60, 128)), 0, 255), make(30)])
    d1, d2 = (q1 / 512.0).astype(np.float32), (q2 / 512.0).astype(np.float32)
    for d in (d1, d2):
        small = np.argsort(d, axis=1)[:, :3]                 # three of each row's smallest components
        for r in range(0, len(d), 9):
            d[r, small[r, 0]] = 0.6
            d[r, small[r, 1]] = -0.25
            d[r, small[r, 2]] = np.nan
    return d1, d2, perm


def test_unsigned_scenario():
    d1, d2, perm = unsigned()
    q1, q2 = RM.quantise(d1), RM.quantise(d2)
    assert ((q1 > 127).any(axis=1).mean() > 0.8) and ((q2 > 127).any(axis=1).mean() > 0.8)
    assert (q1 == 255).sum() == len(range(0, 70, 9)) and np.isnan(d1).sum() == 8 and (d1 < 0).sum() == 8
    assert q1[np.isnan(d1)].max() == 0 and q1[d1 < 0].max() == 0 and (q1[d1 == np.float32(0.6)] == 255).all()
    m = RM.match_pair(d1, d2)
    wrong = RM.match_pair(d1, d2, signed_bytes=True)
    print("unsigned: matches", len(m), "with signed bytes", len(wrong))
    assert len(m) >= 40 and not np.array_equal(m, wrong)
    assert all(perm[j] == i for i, j in m if j < 60)


# ------------------------------------------------------------------ 3. k-order ----
@functools.lru_cache(maxsize=1)
def k_order():
    i, j, c = np.arange(33)[:, None], np.arange(47)[:, None], np.arange(128)[None, :]
    q1, q2 = (7 * i + 13 * c) % 251, (11 * j + c * c) % 253
    return (q1 / 512.0).astype(np.float32), (q2 / 512.0).astype(np.float32)


def test_k_order_scenario():
    """the patterns are asymmetric in i, j and c: a transposed write or a permuted k changes best / bestidx / second"""
    d1, d2 = k_order()
    q1, q2 = RM.quantise(d1), RM.quantise(d2)
    i, j, c = np.arange(33)[:, None], np.arange(47)[:, None], np.arange(128)[None, :]
    assert np.array_equal(q1, (7 * i + 13 * c) % 251) and np.array_equal(q2, (11 * j + c * c) % 253)
    want = RM.direction(RM.scores(q1, q2))
    for name, perm in (("halves", np.r_[64:128, 0:64]), ("16-byte groups", np.arange(128).reshape(8, 16)[[1, 0, 3, 2, 5, 4, 7, 6]].ravel()),
                       ("dwords", np.arange(128).reshape(32, 4)[:, ::-1].ravel())):
        got = RM.direction(RM.scores(q1[:, perm], q2))
        assert any(not np.array_equal(a, b) for a, b in zip(want, got)), name
    s = RM.scores(q1, q2)
    assert not np.array_equal(s[:33, :33], s[:33, :33].T)
    assert (q1 > 127).any() and (q2 > 127).any() and s.max() > 2 ** 21


# --------------------------------------------------------------------- 4. ties ----
TIE_PAIRS = ((3, 4), (10, 26), (20, 84), (40, 41 + 64), (70, 7))      # (j, its duplicate): neighbours, one lane, two tiles ...


@functools.lru_cache(maxsize=1)
def ties():
    """list 1: 60 descriptors; list 2: 150, of which 60 are noisy copies of list 1 at scattered places and TIE_PAIRS lists
    (j, j') where j' is made an exact duplicate of j.  -> (descs1, descs2, partner [60] = the place of i's copy)"""
    rng = np.random.default_rng(24)
    d1 = sift_like(rng, 60)
    d2 = sift_like(rng, 150)
    place = rng.permutation(150)[:60]
    forced = [a for a, _ in TIE_PAIRS]
    place[:len(forced)] = forced                             # queries 0..4 have their copy at the first member of a duplicated pair
    rest = [p for p in rng.permutation(150) if p not in forced and p not in [b for _, b in TIE_PAIRS]]
    place[len(forced):] = rest[:60 - len(forced)]
    d2[place] = noisy(rng, d1, 0.02)
    for a, b in TIE_PAIRS:
        d2[b] = d2[a]
    return d1, d2, place


def test_ties_scenario():
    d1, d2, place = ties()
    best, idx, second = RM.direction(RM.scores(RM.quantise(d1), RM.quantise(d2)))
    tied = np.arange(len(TIE_PAIRS))
    assert (best[tied] == second[tied]).all() and (best[5:] > second[5:]).all()
    assert [int(k) for k in idx[tied]] == [min(p) for p in TIE_PAIRS]                        # the lowest index
    loose = {(int(i), int(j)) for i, j in RM.match_pair(d1, d2, 0.7, 1.5)}
    strict = {(int(i), int(j)) for i, j in RM.match_pair(d1, d2, 0.7, 0.8)}
    print("ties: matches at ratiomax 1.5:", len(loose), "at 0.8:", len(strict))
    for i, p in enumerate(TIE_PAIRS):
        assert (i, min(p)) in loose and (i, max(p)) not in loose
        assert not any(a == i for a, _ in strict)
    assert len(strict) >= 40


# ---------------------------------------------------------------------- 5. cap ----
@functools.lru_cache(maxsize=1)
def cap_small():
    """40 x 50 at max_sift = 32: list 2's descriptor j is a copy of list 1's descriptor 39 - j (j < 40): the partners of j < 8 sit at
    39 - j >= 32, behind the cap"""
    rng = np.random.default_rng(25)
    d1 = sift_like(rng, 40)
    d2 = np.concatenate([noisy(rng, d1[::-1], 0.02), sift_like(rng, 10)])
    return d1, d2


@functools.lru_cache(maxsize=1)
def cap_large():
    """4100 x 64 at the default 4096: list 2's descriptors 0..3 are copies of list 1's 4096..4099, the others of 0..59"""
    rng = np.random.default_rng(26)
    d1 = sift_like(rng, 4100)
    d2 = noisy(rng, np.concatenate([d1[4096:], d1[:60]]), 0.02)
    return d1, d2


def test_cap_scenario():
    d1, d2 = cap_small()
    capped, free = RM.match_pair(d1, d2, max_sift=32), RM.match_pair(d1, d2, max_sift=4096)
    print("cap 32:", len(capped), "uncapped:", len(free))
    assert not np.array_equal(capped, free) and capped.max() < 32 and {39 - j for j in range(8)} <= set(free[:, 0].tolist())
    assert len(capped) >= 15
    d1, d2 = cap_large()
    capped, free = RM.match_pair(d1, d2), RM.match_pair(d1, d2, max_sift=5000)
    print("cap 4096:", len(capped), "uncapped:", len(free))
    assert not np.array_equal(capped, free) and capped[:, 0].max() < 4096 and free[:, 0].max() >= 4096 and len(capped) >= 40


# -------------------------------------------------------------------- 7. chain ----
CHAIN_PER_BUCKET = 60
CHAIN_MATCH = dict(distmax=0.7, ratiomax=0.8, max_sift=4096)


@functools.lru_cache(maxsize=1)
def chain():
    """the three sequences of tests/test_gpu_match_pairs.py's chain scenario; the first CHAIN_PER_BUCKET ground-truth correspondences
    of every frame pair become one key in the list of each endpoint's (frame, view), at the pixel plus a fraction below one half, with
    descriptors made of a shared vector plus noise.  -> (sequences with keys / descs and no raw, the restatement's raw per pair,
    the truth rows per pair)"""
    from tests.test_gpu_match_pairs import VIEWS, chain_scenario
    seqs = chain_scenario()[0]
    rng = np.random.default_rng(27)
    lists = [[([], []) for _ in range(len(q["cameras"]) * VIEWS)] for q in seqs]
    truth = []
    for k in range(len(seqs) - 1):
        a, b = seqs[k], seqs[k + 1]
        rows = []
        for i in range(len(a["cameras"])):
            rows.append([])
            for j in range(len(b["cameras"])):
                m = np.unique(a["raw"][i][j][:CHAIN_PER_BUCKET], axis=0)
                rows[-1].append(m)
                base = sift_like(rng, len(m))
                for r, d in zip(m, base):
                    for seq, frame, off in ((k, i, 0), (k + 1, j, 3)):
                        keys, descs = lists[seq][frame * VIEWS + int(r[off])]
                        keys.append([r[off + 1] + rng.uniform(-0.4, 0.4), r[off + 2] + rng.uniform(-0.4, 0.4), rng.uniform(1, 8), rng.uniform(-3, 3)])
                        descs.append(noisy(rng, d[None], 0.02)[0])
        truth.append(rows)
    out = []
    for q, ls in zip(seqs, lists):
        e = {key: q[key] for key in ("cameras", "depths", "tex", "imgs")}
        e["keys"] = [np.array(kk, np.float32).reshape(-1, 4) for kk, _ in ls]
        e["descs"] = [np.array(dd, np.float32).reshape(-1, 128) for _, dd in ls]
        out.append(e)
    raws = [RM.match_feature(out[k]["keys"], out[k]["descs"], out[k + 1]["keys"], out[k + 1]["descs"], VIEWS, **CHAIN_MATCH)[0]
            for k in range(len(out) - 1)]
    return out, raws, truth


def test_chain_scenario():
    _, raws, truth = chain()
    for raw, rows in zip(raws, truth):
        for i, row in enumerate(rows):
            for j, t in enumerate(row):
                got = {tuple(r) for r in raw[i][j].tolist()}
                want = {tuple(r) for r in t.tolist()}
                print("chain bucket", i, j, "truth", len(want), "matched", len(got), "of the truth", len(got & want))
                assert len(got & want) >= 0.7 * len(want) and len(got - want) <= 0.1 * len(got) and len(got) >= 30


# ------------------------------------------------------- the decision margins ----
def test_no_decision_sits_on_a_threshold():
    cases = []
    q = tails()
    cases += [("tails", q["descs1"][a], q["descs2"][b], {}) for a in range(9) for b in range(9)]
    cases += [("unsigned", *unsigned()[:2], {})]
    cases += [("ties", *ties()[:2], dict(ratiomax=r)) for r in (1.5, 0.8)]
    cases += [("cap 32", *cap_small(), dict(max_sift=32)), ("cap 4096", *cap_large(), {})]
    seqs = chain()[0]
    cases += [("chain", a, b, dict(CHAIN_MATCH)) for k in range(len(seqs) - 1) for a in seqs[k]["descs"] for b in seqs[k + 1]["descs"]]
    worst = {}
    for name, d1, d2, kw in cases:
        a, b = RM.margins(d1, d2, **kw)
        w = worst.setdefault(name, [np.inf, np.inf])
        w[0], w[1] = min(w[0], a), min(w[1], b)
    for name, (a, b) in worst.items():
        print(f"margins {name}: |dist - distmax| >= {a:.3e}, |dist - ratiomax dist2| >= {b:.3e}")
        assert a > MARGIN and b > MARGIN, name


# ------------------------------------------------- restatement against loops ----
def test_the_restatement_equals_plain_loops():
    rng = np.random.default_rng(5)
    d1, d2 = sift_like(rng, 5), np.concatenate([noisy(rng, sift_like(rng, 5), 0.0), sift_like(rng, 2)])
    d2[:4] = noisy(rng, d1[[3, 0, 4, 1]], 0.02)
    d2[5] = d2[1]                                            # a tie
    d1[2, 5], d1[2, 6], d1[2, 7], d2[6, 0] = 0.6, -1.0, np.nan, np.inf
    assert RM.quantise(d1).tolist() == RM.loops_quantise(d1) and RM.quantise(d2).tolist() == RM.loops_quantise(d2)
    q1, q2 = RM.quantise(d1), RM.quantise(d2)
    for a, b in ((q1, q2), (q2, q1), (q1, q2[:1]), (q1, q2[:0])):
        want = RM.loops_direction(a.tolist(), b.tolist())
        got = RM.direction(RM.scores(a, b))
        assert [tuple(int(x[k]) for x in got) for k in range(len(a))] == want
    for kw in (dict(distmax=0.7, ratiomax=0.8, max_sift=4096), dict(distmax=0.7, ratiomax=1.5, max_sift=4096), dict(distmax=0.7, ratiomax=0.8, max_sift=3),
               dict(distmax=0.2, ratiomax=0.8, max_sift=4096)):
        got = RM.match_pair(d1, d2, **kw)
        assert [tuple(r) for r in got.tolist()] == RM.loops_match_pair(d1, d2, **kw), kw
    assert len(RM.match_pair(d1, d2)) >= 3
    keys1, keys2 = [random_keys(rng, 5)], [random_keys(rng, 7)]
    keys1[0][0, 0], keys1[0][3, 1], keys2[0][1, 0] = 10.5, np.nan, 3e9
    raw, counts = RM.match_feature(keys1, [d1], keys2, [d2], 1)
    m = RM.match_pair(d1, d2)
    assert counts.tolist() == [[len(m)]] and len(raw[0][0]) == len(m)
    for (i, j), row in zip(m, raw[0][0]):
        assert row[0] == 0 and row[3] == 0
        for v, want in zip(row[[1, 2, 4, 5]], (keys1[0][i, 0], keys1[0][i, 1], keys2[0][j, 0], keys2[0][j, 1])):
            w = float(want) + 0.5
            assert v == (int(w) if np.isfinite(w) and abs(w) < 2 ** 31 else RM.INT_MIN)


# ------------------------------------------------------------- argument checks ----
def test_the_symbols_are_exported():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mvs_sift_match", "mvs_sift_match_lists", "mvs_sift_match_lists_dev", "mvs_test_sift_scores"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert C.sizeof(_lib.CSiftMatchParams) == 24 and lib.mvs_abi_version() == 4


def _prm(vc=2, max_sift=4096):
    return _lib.CSiftMatchParams(vc, max_sift, 0.7, 0.8)


def _lists_call(dev, **kw):
    a = dict(n1=1, n2=2, prm=_prm(), off1=np.array([0, 2, 3], np.int64), keys1=np.ones((3, 4), np.float32), descs1=np.zeros((3, 128), np.float32),
             off2=np.array([0, 1, 1, 4, 5], np.int64), keys2=np.ones((5, 4), np.float32), descs2=np.zeros((5, 128), np.float32),
             roff=np.zeros(3, np.int64), raw=np.zeros((16, 6), np.int32), cap=16, counts=np.zeros(8, np.int64))
    a.update(kw)
    P = _lib.ptr
    prm = C.byref(a["prm"]) if a["prm"] is not None else None
    common = (a["n1"], a["n2"], prm, P(a["off1"]), P(a["keys1"]), P(a["descs1"]), P(a["off2"]), P(a["keys2"]), P(a["descs2"]), P(a["roff"]),
              P(a["raw"]), a["cap"], P(a["counts"]))
    L = _lib.lib()
    return L.mvs_sift_match_lists_dev(*common, None) if dev else L.mvs_sift_match_lists(*common)


def test_match_lists_rejects_bad_arguments_without_a_device():
    cases = [dict(n1=0), dict(n2=0), dict(n1=-1), dict(prm=None), dict(prm=_prm(vc=0)), dict(prm=_prm(max_sift=0)), dict(prm=_prm(max_sift=-5)),
             dict(off1=None), dict(off2=None), dict(off1=np.array([1, 2, 3], np.int64)), dict(off2=np.array([0, 2, 1, 4, 5], np.int64)),
             dict(keys1=None), dict(descs1=None), dict(keys2=None), dict(descs2=None), dict(roff=None), dict(cap=-1),
             dict(n1=1001, n2=1000, off1=np.zeros(2003, np.int64), off2=np.zeros(2001, np.int64), roff=np.zeros(1001001, np.int64), counts=None)]
    for dev in (False, True):
        for kw in cases:
            assert _lists_call(dev, **kw) == E_INVALID, (dev, kw)
            assert _lib.lib().mvs_last_error()
        for kw in (dict(), dict(raw=None, cap=0), dict(counts=None)):                            # the optional ones
            assert _lists_call(dev, **kw) != E_INVALID, (dev, kw)


def test_match_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    d1, d2 = np.zeros((3, 128), np.float32), np.zeros((4, 128), np.float32)
    buf, n = np.zeros((3, 2), np.int32), C.c_int64()
    P = _lib.ptr
    ok = (3, P(d1), 4, P(d2), C.byref(_prm()), P(buf), C.byref(n))
    for k, v in ((0, -1), (1, None), (2, -1), (3, None), (4, None), (4, C.byref(_prm(max_sift=0))), (5, None), (6, None)):
        args = list(ok)
        args[k] = v
        assert L.mvs_sift_match(*args) == E_INVALID, k
    assert L.mvs_sift_match(*ok) != E_INVALID
    outs = [np.zeros(4, np.int32) for _ in range(6)]
    assert L.mvs_test_sift_scores(3, P(d1), 4, P(d2), 0, *[P(o) for o in outs]) == E_INVALID
    assert L.mvs_test_sift_scores(3, P(d1), 4, P(d2), 4096, *[P(o) for o in outs[:5]], None) == E_INVALID

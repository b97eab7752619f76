"""The statement of include/ldweaver_amd.h (24) in plain numpy: what tests/test_segmap_*.py compare the device and the package with — both entries and the
two-word split of the sums.  Nothing here imports the package."""
import numpy as np

from decay_ref import circ_len, pair_mask
from snpsum_ref import f64_key, same_bits  # noqa: F401  (same_bits: for the tests)

FRAC = 40
LO_BITS = 24
V_LIMIT = 4.0
NO_PAIR = np.uint64(0xFFFFFFFFFFFFFFFF)
INTS = ("n", "nge", "sum_lo", "sum_hi")


def q_split(v):
    """(lo, hi, refused) of the values: q = rint(v 2^40) — an exact scaling, then numpy's round-half-to-even —, 0 and refused for a value that is not finite
    or has |v| >= 4; lo = q & (2^24 - 1), hi = q >> 24 (arithmetic), so that q = hi 2^24 + lo."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(v) < V_LIMIT                       # False for NaN
    q = np.rint(np.where(ok, v, 0.0) * 2.0 ** FRAC).astype(np.int64)
    return q & np.int64((1 << LO_BITS) - 1), q >> np.int64(LO_BITS), ~ok


def key_f64(k):
    """The value of a key (csrc/ldw_dev.h key_f64)."""
    k = np.asarray(k, dtype=np.uint64)
    top = np.uint64(1 << 63)
    return np.where(k & top, k & ~top, ~k).astype(np.uint64).view(np.float64)


def values(mi, w_f=None, w_t=None):
    """v = mi, or mi - w_f[a] w_t[b]: the product, then the difference (csrc/ldw_score.h)."""
    mi = np.asarray(mi, dtype=np.float64)
    if w_f is None:
        return mi
    with np.errstate(invalid="ignore"):
        p = np.asarray(w_f, dtype=np.float64)[:, None] * np.asarray(w_t, dtype=np.float64)[None, :]
        return mi - p


def active_pairs(nf, nt, diag, pos_f, pos_t, g, seg_f, seg_t, sr_dist, cls_mask):
    """The pairs of the block that take part: a > b of a diagonal block, a != b of any other; both segments >= 0; the class inside the mask."""
    seg_f, seg_t = np.asarray(seg_f, dtype=np.int64), np.asarray(seg_t, dtype=np.int64)
    m = pair_mask(nf, nt, diag) & (seg_f[:, None] >= 0) & (seg_t[None, :] >= 0)
    if cls_mask != 3:
        ln = circ_len(np.asarray(pos_t, dtype=np.float64)[None, :], np.asarray(pos_f, dtype=np.float64)[:, None], g)
        m &= (np.where(ln <= sr_dist, 1, 2) & cls_mask) != 0
    return m


def cells(seg_f, seg_t, S):
    """The flat cell min(s, t) S + max(s, t) of every (row, column)."""
    s, t = np.asarray(seg_f, dtype=np.int64)[:, None], np.asarray(seg_t, dtype=np.int64)[None, :]
    return np.minimum(s, t) * S + np.maximum(s, t)


def empty_map(S):
    return dict(n=np.zeros((S, S), np.int64), nge=np.zeros((S, S), np.int64), sum_lo=np.zeros((S, S), np.int64), sum_hi=np.zeros((S, S), np.int64),
                key=np.zeros((S, S), np.uint64), npairs=0, refused=0, nan=0)


def add_block(tot, mi, pos_f, pos_t, g, diag, seg_f, seg_t, sr_dist, cls_mask, w_f=None, w_t=None, thr=np.inf):
    """One block of (nf, nt) values into the running map ``tot`` (empty_map): integers add, maxima by key."""
    S = tot["n"].shape[0]
    v = values(mi, w_f, w_t)
    nf, nt = v.shape
    m = active_pairs(nf, nt, diag, pos_f, pos_t, g, seg_f, seg_t, sr_dist, cls_mask)
    cell = cells(seg_f, seg_t, S)[m]
    vv = v[m]
    lo, hi, ref = q_split(vv)
    with np.errstate(invalid="ignore"):
        ge = vv >= thr
    nan = np.isnan(vv)
    np.add.at(tot["n"].reshape(-1), cell, 1)
    np.add.at(tot["nge"].reshape(-1), cell, ge.astype(np.int64))
    np.add.at(tot["sum_lo"].reshape(-1), cell, lo)
    np.add.at(tot["sum_hi"].reshape(-1), cell, hi)
    np.maximum.at(tot["key"].reshape(-1), cell, np.where(nan, np.uint64(0), f64_key(vv)))
    tot["npairs"] += int(m.sum())
    tot["refused"] += int(ref.sum())
    tot["nan"] += int(nan.sum())
    return tot


def finish(tot):
    """The map with ``max`` from the keys: NaN where a cell holds no value that is a number."""
    out = dict(tot)
    out["max"] = np.where(tot["key"] != 0, key_f64(np.where(tot["key"] != 0, tot["key"], np.uint64(1 << 63))), np.nan)
    return out


def segment_map(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr_dist, cls_mask, w_f=None, w_t=None, thr=np.inf):
    """ldw_debug_segment_map of one block."""
    return finish(add_block(empty_map(S), mi, pos_f, pos_t, g, diag, seg_f, seg_t, sr_dist, cls_mask, w_f, w_t, thr))


def best_block(pair, max_in, mi, pos_f, pos_t, g, diag, seg_f, seg_t, sr_dist, cls_mask, id_f, id_t, w_f=None, w_t=None):
    """One block into the running best pairs ``pair`` (S, S) uint64, all-ones at the start: per cell the smallest packed pair whose value has the bits of
    max_in[cell]."""
    S = pair.shape[0]
    v = values(mi, w_f, w_t)
    nf, nt = v.shape
    m = active_pairs(nf, nt, diag, pos_f, pos_t, g, seg_f, seg_t, sr_dist, cls_mask)
    cell = cells(seg_f, seg_t, S)
    mx = np.asarray(max_in, dtype=np.float64).reshape(-1)[cell]
    m &= ~np.isnan(v) & ~np.isnan(mx) & (v.view(np.int64) == mx.view(np.int64))
    a, b = np.asarray(id_f, dtype=np.uint64)[:, None], np.asarray(id_t, dtype=np.uint64)[None, :]
    packed = (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)
    np.minimum.at(pair.reshape(-1), cell[m], packed[m])
    return pair


def segment_best(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr_dist, cls_mask, id_f, id_t, max_in, w_f=None, w_t=None):
    """ldw_debug_segment_best of one block."""
    return best_block(np.full((S, S), NO_PAIR, dtype=np.uint64), max_in, mi, pos_f, pos_t, g, diag, seg_f, seg_t, sr_dist, cls_mask, id_f, id_t, w_f, w_t)


def same_map(got, ref):
    """Integers exactly, maxima bit for bit."""
    return all(np.array_equal(got[k], ref[k]) for k in INTS) and same_bits(got["max"], ref["max"]) and int(got["npairs"]) == int(ref["npairs"])


def exact(m):
    """The exact sums of a map as Python integers."""
    return m["sum_hi"].astype(object) * (1 << LO_BITS) + m["sum_lo"].astype(object)


def planted_genes():
    """The planted example of the gene map: 200 sequences, 120 SNPs in 12 segments of 10; every cell a minor state with probability 0.15; 40 lineage markers
    (one half / half split of the sequences, 2 % of the entries flipped) fill four segments (1, 4, 7, 10); five SNPs of segment 2 are each a random balanced
    column, and five SNPs of segment 8 their copies with 10 % flipped.  POS = 1000 i + 1 on a genome of 10^6 with sr_dist 500: every pair is long range.
    Returns (states (120, 200) uint8, POS int32, g, sr_dist, seg int32, marker segments, planted cell (2, 8), planted pairs [(a, b)] with a < b)."""
    rng = np.random.default_rng(11)
    L, N = 120, 200
    st = (rng.random((L, N)) < 0.15).astype(np.uint8)
    seg = (np.arange(L) // 10).astype(np.int32)
    marker_segs = (1, 4, 7, 10)
    split = np.zeros(N, dtype=np.uint8)
    split[rng.permutation(N)[:N // 2]] = 1
    for s in marker_segs:
        for i in range(10 * s, 10 * s + 10):
            st[i] = split ^ (rng.random(N) < 0.02)
    pairs = []
    for k in range(5):
        a, b = 20 + 2 * k, 80 + 2 * k
        base = np.zeros(N, dtype=np.uint8)
        base[rng.permutation(N)[:N // 2]] = 1
        st[a] = base
        st[b] = base ^ (rng.random(N) < 0.10)
        pairs.append((a, b))
    pos = (1000 * np.arange(L) + 1).astype(np.int32)
    return np.ascontiguousarray(st), pos, 1e6, 500.0, seg, marker_segs, (2, 8), pairs

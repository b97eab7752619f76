"""The statement of include/ldweaver_amd.h (20) and of the host rules of ldweaver_amd/decay.py in plain numpy: what tests/test_decay_*.py compare
the device and the package with.  Nothing here imports the package."""
import math

import numpy as np

NBINS = 4096
BUCKET_OFF = (1023 - 20) << 7


def mi_bucket(mi):
    """The engine's MI bucket from the float64 bits: (u >> 45) - ((1023 - 20) << 7) clamped to 0..4095, and 0 for u <= 0 (negatives, -0, +0)."""
    u = np.ascontiguousarray(mi, dtype=np.float64).view(np.int64)
    b = np.clip((u >> 45) - BUCKET_OFF, 0, NBINS - 1)
    return np.where(u <= 0, 0, b).astype(np.int64)


def bucket_lo(B):
    return ((np.asarray(B, dtype=np.int64) + BUCKET_OFF) << 45).view(np.float64)


def below(x):
    """The double just below x > 0."""
    return np.nextafter(np.asarray(x, dtype=np.float64), -np.inf)


def circ_len(pos1, pos2, g):
    d = np.mod(np.asarray(pos1, dtype=np.float64) - np.asarray(pos2, dtype=np.float64), float(g))
    return 0.5 * g - np.abs(d - 0.5 * g)


def pair_mask(nf, nt, diag):
    a, b = np.arange(nf)[:, None], np.arange(nt)[None, :]
    return a > b if diag else a != b


def profile_hist(mi, pos_f, pos_t, g, diag, cuts, mi_shift):
    """(hist uint64 (n_cut + 1, NB), max (n_cut + 1,) with NaN for an empty bin, n_pairs) of the (nf, nt) values ``mi``: the pairs a > b of a diagonal
    block, a != b of any other; distance bin = the number of cuts strictly below len(pos_t[b], pos_f[a]); MI bin = mi_bucket >> mi_shift."""
    mi = np.asarray(mi, dtype=np.float64)
    nf, nt = mi.shape
    cuts = np.asarray(cuts if cuts is not None else [], dtype=np.float64)
    nb = NBINS >> mi_shift
    m = pair_mask(nf, nt, diag)
    ln = circ_len(np.asarray(pos_t, dtype=np.float64)[None, :], np.asarray(pos_f, dtype=np.float64)[:, None], g)
    db = np.searchsorted(cuts, ln[m], side="left")        # cuts strictly below len
    v = mi[m]
    mb = mi_bucket(v) >> mi_shift
    hist = np.bincount(db * nb + mb, minlength=(len(cuts) + 1) * nb).reshape(len(cuts) + 1, nb).astype(np.uint64)
    mx = np.full(len(cuts) + 1, np.nan)
    u = np.ascontiguousarray(v).view(np.uint64)
    key = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))          # the order of the values with -0 below +0, as the device orders them
    for k in np.unique(db):
        sel = np.flatnonzero(db == k)
        mx[k] = v[sel[np.argmax(key[sel])]]
    return hist, mx, int(m.sum())


def same_max(a, b):
    """Bit for bit, NaN (an empty bin) matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


# ---- the host rules of LDDecay ----
def bin_edges(mi_shift):
    nb = NBINS >> mi_shift
    e = bucket_lo(np.arange(nb + 1, dtype=np.int64) << mi_shift)
    lo, hi = e[:-1].copy(), e[1:].copy()
    lo[0], hi[-1] = 0.0, np.inf
    return lo, hi


def quantile_bin(counts, q):
    """The bin holding rank ceil(q n) (1-based, at least 1) of the counted values, by a plain loop; -1 for none."""
    n = int(np.asarray(counts, dtype=np.int64).sum())
    if n == 0:
        return -1
    rank, c = min(max(math.ceil(q * n), 1), n), 0
    for j, k in enumerate(counts):
        c += int(k)
        if c >= rank:
            return j
    raise AssertionError


def quantile(hist, mi_shift, q):
    lo, hi = bin_edges(mi_shift)
    out = np.full((len(hist), 2), np.nan)
    for k, row in enumerate(hist):
        j = quantile_bin(row, q)
        if j >= 0:
            out[k] = lo[j], hi[j]
    return out[:, 0], out[:, 1]


def planted_alignment():
    """The planted example: 200 sequences, 50 groups of 8 consecutive SNPs, each group a random binary row copied with 5 % of the entries flipped
    independently; POS = 100 i + 1, g = 120 000, unit weights.  Returns (states (400, 200) uint8, POS int32, g, cuts)."""
    rng = np.random.default_rng(7)
    base = np.repeat(rng.integers(0, 2, (50, 200)), 8, axis=0)            # the 50 rows first, then every flip
    st = np.ascontiguousarray(base ^ (rng.random(base.shape) < 0.05), dtype=np.uint8)
    pos = (100 * np.arange(len(st)) + 1).astype(np.int32)
    cuts = np.array(list(range(100, 2001, 100)) + [5000, 10000, 20000, 40000], dtype=np.float64)
    return st, pos, 120000.0, cuts

"""The statement of include/ldweaver_amd.h (21) in plain numpy: what tests/test_snpsum_*.py and tests/test_background_host.py compare the device and the
package with.  Nothing here imports the package."""
import numpy as np

from decay_ref import circ_len, pair_mask

FRAC = 40
Q_LIMIT = 2.0 ** 22


def q_fixed(mi):
    """(q int64, refused bool) of the values: q = rint(mi 2^40) — an exact scaling, then numpy's round-half-to-even — and 0, refused, for a value that is
    not finite or has |mi| >= 2^22."""
    mi = np.asarray(mi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(mi) < Q_LIMIT                      # False for NaN
    return np.rint(np.where(ok, mi, 0.0) * 2.0 ** FRAC).astype(np.int64), ~ok


def f64_key(v):
    """The order of the values by their IEEE bits, -0 below +0 (csrc/ldw_dev.h f64_key)."""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def _max_by_key(v, hit, axis):
    """Per row (axis 1) or column (axis 0) of the (nf, nt) values the one with the largest key among ``hit``; NaN where none."""
    key = np.where(hit, f64_key(v), np.uint64(0))
    k = np.argmax(key, axis=axis)
    picked = np.take_along_axis(v, np.expand_dims(k, axis), axis).squeeze(axis)
    return np.where(hit.any(axis=axis), picked, np.nan)


def snp_summary(mi, pos_f, pos_t, g, diag, sr_dist, thr):
    """The two sides of one block of (nf, nt) values ``mi``: the pairs a > b of a diagonal block, a != b of any other; class 0 where
    circ_len(pos_t[b], pos_f[a]) <= sr_dist, else 1.  Returns (rows, cols, npairs, refused): rows / cols dicts of n, sumq, nge int64 and max float64,
    shaped (2, nf) / (2, nt) — what the pairs add to their from-SNPs / to-SNPs; npairs (2,); refused the pairs whose value q refuses."""
    mi = np.asarray(mi, dtype=np.float64)
    nf, nt = mi.shape
    m = pair_mask(nf, nt, diag)
    ln = circ_len(np.asarray(pos_t, dtype=np.float64)[None, :], np.asarray(pos_f, dtype=np.float64)[:, None], g)
    cls = np.where(ln <= sr_dist, 0, 1)
    q, ref = q_fixed(mi)
    rows = dict(n=np.zeros((2, nf), np.int64), sumq=np.zeros((2, nf), np.int64), max=np.full((2, nf), np.nan), nge=np.zeros((2, nf), np.int64))
    cols = dict(n=np.zeros((2, nt), np.int64), sumq=np.zeros((2, nt), np.int64), max=np.full((2, nt), np.nan), nge=np.zeros((2, nt), np.int64))
    npairs = np.zeros(2, np.int64)
    for c in (0, 1):
        hit = m & (cls == c)
        with np.errstate(invalid="ignore"):
            ge = hit & (mi >= thr[c])
        for side, axis in ((rows, 1), (cols, 0)):
            side["n"][c] = hit.sum(axis=axis)
            side["sumq"][c] = np.where(hit, q, 0).sum(axis=axis)
            side["nge"][c] = ge.sum(axis=axis)
            side["max"][c] = _max_by_key(mi, hit, axis)
        npairs[c] = hit.sum()
    return rows, cols, npairs, int((m & ref).sum())


def fold(total, side, idx):
    """Add one side of a block (its local SNPs are the global SNPs ``idx``, distinct) into the per-SNP totals (2, L): integers add, maxima by key."""
    for k in ("n", "sumq", "nge"):
        total[k][:, idx] += side[k]
    old, new = total["max"][:, idx], side["max"]
    take = ~np.isnan(new) & (np.isnan(old) | (f64_key(new) > f64_key(old)))
    total["max"][:, idx] = np.where(take, new, old)


def empty_total(L):
    return dict(n=np.zeros((2, L), np.int64), sumq=np.zeros((2, L), np.int64), max=np.full((2, L), np.nan), nge=np.zeros((2, L), np.int64))


def same_bits(a, b):
    """Bit for bit, NaN (no partner) matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def same_side(got, ref):
    return all(np.array_equal(got[k], ref[k]) for k in ("n", "sumq", "nge")) and same_bits(got["max"], ref["max"])


def planted_apc():
    """The planted example of the average product correction: 200 sequences, 120 SNPs; every cell a minor state with probability 0.15; 40 random columns are
    lineage markers (one half / half split of the sequences, 2 % of the entries flipped); two other columns are a random balanced column and its copy with
    10 % flipped.  POS = 1000 i + 1 on a genome of 10^6 with sr_dist 500: every pair is long range.  Returns (states (120, 200) uint8, POS int32, g,
    sr_dist, markers, planted (a, b))."""
    rng = np.random.default_rng(7)
    L, N = 120, 200
    st = (rng.random((L, N)) < 0.15).astype(np.uint8)
    cols = rng.permutation(L)
    markers, (pa, pb) = np.sort(cols[:40]), cols[40:42]
    split = np.zeros(N, dtype=np.uint8)
    split[rng.permutation(N)[:N // 2]] = 1
    for m in markers:
        st[m] = split ^ (rng.random(N) < 0.02)
    base = np.zeros(N, dtype=np.uint8)
    base[rng.permutation(N)[:N // 2]] = 1
    st[pa] = base
    st[pb] = base ^ (rng.random(N) < 0.10)
    pos = (1000 * np.arange(L) + 1).astype(np.int32)
    return np.ascontiguousarray(st), pos, 1e6, 500.0, markers, (int(pa), int(pb))

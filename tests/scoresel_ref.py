"""The statement of include/ldweaver_amd.h (22) and the threshold rule of ldweaver_amd/background.py in plain numpy: what tests/test_scoresel_*.py and
tests/test_apc_links_host.py compare the device and the package with.  Nothing here imports the package."""
import numpy as np

from decay_ref import BUCKET_OFF, NBINS, circ_len, mi_bucket, pair_mask  # noqa: F401  (mi_bucket: the long-range selection's rule, re-exported)
from snpsum_ref import f64_key, same_bits  # noqa: F401


def score(mi, wa, wb):
    """s = mi - wa wb on float64 arrays: numpy rounds the product, then the difference (it does not fuse them)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = np.asarray(wa, dtype=np.float64) * np.asarray(wb, dtype=np.float64)
        return np.asarray(mi, dtype=np.float64) - p


def block(mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, w_f, w_t):
    """(s, part) of one block of (nf, nt) values: the scores, and the pairs that take part — a > b of a diagonal block, a != b of any other, with the class
    (1 where circ_len(pos_t[b], pos_f[a]) <= sr_dist, else 2) inside the mask."""
    mi = np.asarray(mi, dtype=np.float64)
    nf, nt = mi.shape
    with np.errstate(invalid="ignore", over="ignore"):
        s = score(mi, np.asarray(w_f, dtype=np.float64)[:, None], np.asarray(w_t, dtype=np.float64)[None, :])
    ln = circ_len(np.asarray(pos_t, dtype=np.float64)[None, :], np.asarray(pos_f, dtype=np.float64)[:, None], g)
    cls = np.where(ln <= sr_dist, 1, 2)
    return s, pair_mask(nf, nt, diag) & ((cls & cls_mask) != 0)


def _best(s, ok, axis):
    key = np.where(ok, f64_key(s), np.uint64(0))
    k = np.argmax(key, axis=axis)
    picked = np.take_along_axis(s, np.expand_dims(k, axis), axis).squeeze(axis)
    return np.where(ok.any(axis=axis), picked, np.nan)


def scan(mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, w_f, w_t):
    """The scan of one block, the sides apart: dict of hist uint64 (4096,), best_f (nf,), best_t (nt,) — the largest score by f64_key over the partners whose
    score is a number, NaN where none —, npairs (inside the mask) and nan (the NaN scores among them)."""
    s, part = block(mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, w_f, w_t)
    ok = part & ~np.isnan(s)
    hist = np.bincount(mi_bucket(s[ok]), minlength=NBINS).astype(np.uint64)
    return dict(hist=hist, best_f=_best(s, ok, 1), best_t=_best(s, ok, 0), npairs=int(part.sum()), nan=int((part & np.isnan(s)).sum()))


def links(mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, id_f, id_t, w_f, w_t, thr, best_f=None, best_t=None):
    """The links of one block: (set of (id_f[a], id_t[b], bits of mi, bits of s) over the pairs that take part with s >= thr, partner_f, partner_t): per row
    the smallest id_t among its partners with f64_key(s) == f64_key(best_f[row]), -1 where best_f is NaN or nothing matches; per column likewise with id_f."""
    mi = np.asarray(mi, dtype=np.float64)
    s, part = block(mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, w_f, w_t)
    id_f, id_t = np.asarray(id_f, dtype=np.int64), np.asarray(id_t, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        hit = part & (s >= thr)
    a, b = np.nonzero(hit)
    out = set(zip(id_f[a].tolist(), id_t[b].tolist(), mi[a, b].view(np.int64).tolist(), s[a, b].view(np.int64).tolist()))
    assert len(out) == len(a)
    if best_f is None:
        return out, None, None
    ok = part & ~np.isnan(s)
    big = np.int64(1) << 40
    bf, bt = np.asarray(best_f, dtype=np.float64), np.asarray(best_t, dtype=np.float64)
    mf = ok & (f64_key(s) == f64_key(bf)[:, None]) & ~np.isnan(bf)[:, None]
    mt = ok & (f64_key(s) == f64_key(bt)[None, :]) & ~np.isnan(bt)[None, :]
    pf = np.where(mf, id_t[None, :], big).min(axis=1)
    pt = np.where(mt, id_f[:, None], big).min(axis=0)
    return out, np.where(pf == big, -1, pf).astype(np.int32), np.where(pt == big, -1, pt).astype(np.int32)


def empty_total(L):
    return dict(hist=np.zeros(NBINS, np.uint64), best=np.full(L, np.nan), npairs=0, nan=0)


def fold(total, sc, fi, ti):
    """Add the scan of one block (its rows are the global SNPs ``fi``, its columns ``ti``, each distinct) into the totals: counts add, bests by key."""
    total["hist"] += sc["hist"]
    total["npairs"] += sc["npairs"]
    total["nan"] += sc["nan"]
    for new, idx in ((sc["best_f"], fi), (sc["best_t"], ti)):
        old = total["best"][idx]
        take = ~np.isnan(new) & (np.isnan(old) | (f64_key(new) > f64_key(old)))
        total["best"][idx] = np.where(take, new, old)


def fold_partner(total, part, idx):
    """Fold one side's partner minima (-1: none) of a block into the per-SNP minima."""
    old = total[idx]
    total[idx] = np.where(part < 0, old, np.where(old < 0, part, np.minimum(old, part)))


def pick_threshold(hist, top):
    """(thr, cap): B* the largest B >= 1 whose buckets B.. hold at least ``top`` pairs, else 1; thr its lower edge; cap the pairs in the buckets B*.., by a
    plain loop over Python integers."""
    h = [int(x) for x in hist]
    assert len(h) == NBINS
    B, c, cum = 1, 0, [0] * (NBINS + 1)
    for k in range(NBINS - 1, 0, -1):
        c += h[k]
        cum[k] = c
    for k in range(NBINS - 1, 0, -1):
        if cum[k] >= top:
            B = k
            break
    bits = (B + ((1023 - 20) << 7)) << 45
    return float(np.array([bits], dtype=np.int64).view(np.float64)[0]), cum[B]

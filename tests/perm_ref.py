"""numpy restatement of the permutation test for links: the replicate orders and, per pair and replicate, the joint table and the
weighted MI.  The kernels (csrc/ldw_perm.hip), this file and the tests follow include/ldweaver_amd.h (19)."""
from __future__ import annotations

import numpy as np

import lineage_ref

M64 = (1 << 64) - 1
_C = tuple(np.uint64(v) for v in (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB))


def hash40(seed: int, r, s) -> np.ndarray:
    """h(seed, r, s), 40 bits, for arrays (or scalars) of replicate and sequence indices: uint64, all arithmetic mod 2^64."""
    r, s = np.asarray(r, dtype=np.uint64), np.asarray(s, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & M64) + _C[0] * (r + np.uint64(1)) + _C[1] * (s + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _C[2]
        z = (z ^ (z >> np.uint64(27))) * _C[3]
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(24)


def hash40_int(seed: int, r: int, s: int) -> int:
    """The same on Python integers: the statement, word for word."""
    z = (seed + 0x9E3779B97F4A7C15 * (r + 1) + 0xD1B54A32D192ED03 * (s + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 24


def order0(labels) -> np.ndarray:
    """int32 [P]: the labelled sequences sorted by (label, sequence index)."""
    labels = np.asarray(labels, dtype=np.int64)
    seq = np.nonzero(labels >= 0)[0]
    return seq[np.argsort(labels[seq], kind="stable")].astype(np.int32)


def orders(labels, B: int, seed: int) -> np.ndarray:
    """int32 (B, P): row r the labelled sequences stably sorted by (label << 40) | h(seed, r, s), equal keys in ascending sequence index."""
    labels = np.asarray(labels, dtype=np.int64)
    seq = np.nonzero(labels >= 0)[0]                            # ascending: a stable sort keeps that order among equal keys
    top = labels[seq].astype(np.uint64) << np.uint64(40)
    out = np.empty((int(B), len(seq)), dtype=np.int32)
    for r in range(int(B)):
        key = top | hash40(seed, r, seq)
        out[r] = seq[np.argsort(key, kind="stable")]
    return out


def links_permuted(states, hdw, pair_a, pair_b, labels, C: int, B: int, seed: int):
    """dict of mi_obs (K,), n_ge int32 (K,), null_max (K,), null (K, B), fixed int64 (K, B, 5, 5), fixed_obs int64 (K, 5, 5), orders int32 (B, P), P,
    frac_bits: what ldw_links_permuted returns.  The weight and SNP a's state stay with the sequence at order0[p]; SNP b's state is the one of the
    sequence at order_r[p]."""
    states = np.asarray(states)
    hdw = np.asarray(hdw, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    assert labels.min() >= -1 and labels.max() < int(C)
    a, b = np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    K, B = len(a), int(B)
    V, F = lineage_ref.quantise(hdw)
    o0 = order0(labels)
    ords = orders(labels, B, seed)
    neff = float(np.sum(hdw[labels >= 0].astype(np.longdouble)))
    w = V[o0].astype(np.float64)                                   # (every sum < 2^52: exact)
    sa, sb = np.minimum(states[a], 4).astype(np.int64), np.minimum(states[b], 4).astype(np.int64)

    def table(k, order):
        code = sa[k, o0] * 5 + sb[k, order]
        return np.bincount(code, minlength=25), np.rint(np.bincount(code, weights=w, minlength=25)).astype(np.int64)

    mi_obs, fixed_obs = np.zeros(K), np.zeros((K, 25), dtype=np.int64)
    null, fixed = np.zeros((K, B)), np.zeros((K, B, 25), dtype=np.int64)
    for k in range(K):
        cnt, fixed_obs[k] = table(k, o0)
        mi_obs[k] = lineage_ref.mi_from_tables(cnt, fixed_obs[k], F, neff)
        for r in range(B):
            cnt, fixed[k, r] = table(k, ords[r])
            null[k, r] = lineage_ref.mi_from_tables(cnt, fixed[k, r], F, neff)
    return dict(mi_obs=mi_obs, n_ge=(null >= mi_obs[:, None]).sum(axis=1).astype(np.int32), null_max=null.max(axis=1), null=null,
                fixed=fixed.reshape(K, B, 5, 5), fixed_obs=fixed_obs.reshape(K, 5, 5), orders=ords, P=len(o0), frac_bits=F)

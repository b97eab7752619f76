"""Bootstrap support of the neighbour-joining tree as DESIGN.md 26 states it, in numpy: the reference of tests/test_nj_bootstrap_host.py and
tests/test_nj_bootstrap_gpu.py.  The weighted distance by its definition, the Hamming stage's column rule and the diagonal identity the device uses, the
splits of a parent array as exact tip sets, and the support of a reference tree over replicate trees."""
import numpy as np


def weighted_distance(states: np.ndarray, m) -> np.ndarray:
    """d_m(i, j) = the sum of m[a] over the columns a with state(a, i) != state(a, j): int64 [N, N] of ``states`` uint8 [L, N]."""
    st = np.asarray(states)
    m = np.asarray(m, dtype=np.int64)
    N = st.shape[1]
    d = np.zeros((N, N), dtype=np.int64)
    for a in np.nonzero(m)[0]:
        d += m[a] * (st[a][:, None] != st[a][None, :])
    return d


def hamming_columns(states: np.ndarray):
    """The bit columns of csrc/ldw_hamming.hip (k_ham_ncols, k_ham_fill): (B uint8 [K, N], dig int64 [K], snp int64 [K]).  Per SNP with d its most
    frequent state (the lowest of equally frequent ones): no column when one state is present; the minor state's column with digit 2 when two are;
    otherwise one column per minor state and the column [x != d], digit 1 each."""
    st = np.asarray(states)
    cols, dig, snp = [], [], []
    for a in range(st.shape[0]):
        cnt = np.bincount(st[a], minlength=5)[:5]
        present = [x for x in range(5) if cnt[x] > 0]
        if len(present) <= 1:
            continue
        drop = max(present, key=lambda x: (cnt[x], -x))
        minors = [x for x in present if x != drop]
        for x in minors:
            cols.append(st[a] == x)
            dig.append(2 if len(minors) == 1 else 1)
            snp.append(a)
        if len(minors) > 1:
            cols.append(st[a] != drop)
            dig.append(1)
            snp.append(a)
    N = st.shape[1]
    return (np.asarray(cols, dtype=np.uint8).reshape(-1, N), np.asarray(dig, dtype=np.int64), np.asarray(snp, dtype=np.int64))


def identity_distance(states: np.ndarray, m) -> np.ndarray:
    """d_m by the device's route: G_m = sum_k dig[k] m[snp(k)] B_ki B_kj, d_m(i, j) = (G_m(i, i) + G_m(j, j)) / 2 - G_m(i, j)."""
    B, dig, snp = hamming_columns(states)
    w = dig * np.asarray(m, dtype=np.int64)[snp] if len(dig) else dig
    Bi = B.astype(np.int64)
    G = (Bi * w[:, None]).T @ Bi
    g = np.diag(G)
    assert not (g & 1).any()
    d = (g[:, None] + g[None, :]) // 2 - G
    return d


def splits(parent) -> dict:
    """{the side of the split that does not hold tip 0, as a frozenset of tips: the join node} for the join nodes N .. 2N-4 of a parent array."""
    par = np.asarray(parent).tolist()
    N = (len(par) + 2) // 2
    below = [frozenset([v]) if v < N else frozenset() for v in range(2 * N - 2)]
    for v in range(2 * N - 3):            # a parent has the larger id
        below[par[v]] = below[par[v]] | below[v]
    everything = frozenset(range(N))
    return {(everything - below[u] if 0 in below[u] else below[u]): u for u in range(N, 2 * N - 3)}


def support(ref_parent, rep_parents) -> np.ndarray:
    """int32 [2N-2]: per join node of the reference tree the number of replicate trees that have its split; -1 at the tips and the root."""
    ref = splits(ref_parent)
    out = np.full(len(ref_parent), -1, dtype=np.int32)
    out[list(ref.values())] = 0
    for p in rep_parents:
        theirs = splits(p)
        for s, u in ref.items():
            out[u] += s in theirs
    return out


def five_state_alignment(L: int, N: int, seed: int) -> np.ndarray:
    """uint8 [L, N]: monomorphic, biallelic and multi-allelic columns in turn, groups of sequences sharing their states so that a tree has clades."""
    rng = np.random.default_rng(seed)
    st = np.zeros((L, N), dtype=np.uint8)
    group = rng.integers(0, max(2, N // 3), size=N)
    for a in range(L):
        kind = a % 4
        if kind == 0:
            st[a] = rng.integers(0, 5)
        elif kind == 1:
            x, y = rng.choice(5, 2, replace=False)
            st[a] = np.where(rng.random(N) < 0.3, x, y)
        elif kind == 2:
            st[a] = rng.integers(0, 5, size=N)
        else:
            st[a] = rng.integers(0, 5, size=group.max() + 1)[group]
    return st

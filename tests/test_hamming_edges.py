"""The Hamming-weight stage (csrc/ldw_hamming.hip: the device-built column list, the column bits, the ballot transpose, the masked popcount, the
lower-triangular gemm_bits_kernel<1> with the COLUMN count as K, k_hdw and the strip form k_hdw_strip) against the oracle at its structural
edges.  Every comparison is on integers or on the bits of 1 / (count + 1): no tolerance anywhere in this file.

Why alignments of their own: on the synthetic and bundled alignments hardly any pair of sequences lies within a few SNPs of the threshold, so
hdw = 1 / (n + 1) does not move when a shared count is off by a few.  ``planted`` builds alignments whose within-group distances are a_i + a_j with
a_k in {h - 1, h, h + 1}, h = thresh // 2 — clustered on thresh - 2 .. thresh + 2 — with exact duplicates, with one SNP of every class the column
builder distinguishes (0 columns: monomorphic, all-gap; 1 column: biallelic, a singleton minor state; p columns: 3, 4 and 5 states; two- and three-way
ties for the most frequent state) and with the sequences permuted, so that the groups straddle the 64-sequence words and the 128-sequence tiles.
``columns_case`` builds alignments with an exact column count KR (the GEMM's K here): 0, the transpose's padding edges 64 / 128 and the edges of the K
loop's 1024-position chunks.  ``test_generated_cases_meet_their_conditions`` (no GPU) proves with the oracle alone that every case has what it was built
for, so that no GPU test can pass vacuously; a case that lacks a property FAILS there.

Where a condition cannot apply it is not asked: fewer than 63 sequences (N = 1, 2: only the planted SNP rows matter) carry no distance conditions; one
tile (N <= 128) has no pair across tiles; a world whose strips leave one non-empty strip has no pair across strips.

The constants the cases sit on, restated as plain numbers (a change there: revisit the cases):
  128    ldw_internal.h TILE / KSTEP: sequences per row tile of the comparison, padding of N; the launch skips tiles above the diagonal from N = 129 on
  64     one word of sequences (k_hamming_cols, k_bits_transpose) and the from-side tile of the GEMM
  1024   ldw_gemm_tile.h BW_CHUNK * 64: positions of K per chunk of the GEMM's loop (word pairs: K is padded to a multiple of 128, at least 128)
"""
import functools

import numpy as np
import pytest

import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd.dist import hamming_tile_strips

TILE = 128
WORLDS = (1, 2, 3, 4, 8)
CLASSES = ("mono", "allgap", "biallelic", "three", "four", "five", "tie2", "tie3", "singleton")


# ------------------------------------------------------------------------------------------------
# the column rule (ldw_hamming_stats) and the neighbour rule, in numpy
# ------------------------------------------------------------------------------------------------
def n_present(st):
    """Present states per SNP."""
    return sum(((st == x).any(axis=1)).astype(np.int64) for x in range(5))


def n_columns(st):
    """Columns of the Hamming GEMM: a SNP with p present states gives 0 columns for p <= 1, 1 for p = 2, p for p >= 3."""
    p = n_present(st)
    return int(np.where(p <= 1, 0, np.where(p == 2, 1, p)).sum())


def k_padded(kr):
    return max(128, -(-kr // 128) * 128)


def hdw_of(dist, thresh):
    """R/performPopulationStuctureCorrection.R:76 with an explicit integer threshold: strict <."""
    return 1.0 / ((dist < thresh).sum(axis=0) + 1.0)


def strip_counts(dist, thresh, t0, t1):
    """cnt[j] = sum over rows t of the strip and f >= t of A[t, f] ([j == t] + [j == f and f != t]), A = dist < thresh: every unordered pair once, in the
    strip that holds its smaller index."""
    N = len(dist)
    U = np.triu(dist < thresh).astype(np.int64)
    U[:t0 * TILE] = 0
    U[min(t1 * TILE, N):] = 0
    return U.sum(axis=1) + (U - np.diag(np.diag(U))).sum(axis=0)


def thresholds(Ls):
    t = int(0.1 * Ls)
    return sorted({0, 1, max(t - 1, 0), t, t + 1, t + 2, Ls, Ls + 1})


# ------------------------------------------------------------------------------------------------
# alignments with planted distances
# ------------------------------------------------------------------------------------------------
def _blocks_row(N, states, sizes, lead=None):
    """A SNP whose sequences (in the order before the final permutation) carry states[k] on a run of sizes[k]; what is left over goes to the LAST state, and
    `lead` = (state, count) puts a further state on the first sequences (the remainder of a tie)."""
    row = np.full(N, states[-1], dtype=np.uint8)
    o = 0
    if lead is not None:
        row[:lead[1]] = lead[0]
        o = lead[1]
    for s, n in zip(states[:-1], sizes[:-1]):
        row[o:o + n] = s
        o += n
    return row


def _planted_rows(N, g):
    """One SNP of every class of the column builder.  Every row is constant on the last third of the sequences (where the duplicates and their sources lie), and
    the cuts of the rows without a tie are rounded to group boundaries where there are enough groups, so that few groups see a distance other than a_i + a_j."""
    def cuts(fr):
        n = [max(1, int(round(f * N))) for f in fr]
        if N >= 12 * g:
            n = [max(g, x // g * g) for x in n]
        return n
    h2, h3 = N // 2, N // 3
    rows = {
        "mono": np.full(N, 1, dtype=np.uint8),
        "allgap": np.full(N, 4, dtype=np.uint8),
        "biallelic": _blocks_row(N, (2, 0), cuts((0.3, 0.7))),
        "three": _blocks_row(N, (4, 0, 3), cuts((0.2, 0.3, 0.5))),
        "four": _blocks_row(N, (3, 1, 0, 2), cuts((0.1, 0.2, 0.3, 0.4))),
        "five": _blocks_row(N, (2, 4, 3, 0, 1), cuts((0.08, 0.12, 0.2, 0.25, 0.35))),
        # ties for the most frequent state: exact halves / thirds; a remainder carries one more state (fewer sequences than the tied ones).  The tied states
        # come in descending order of their index: the builder drops the FIRST maximum, which is then not the first it meets along the sequences.
        "tie2": _blocks_row(N, (3, 1), (h2, h2), lead=(0, N - 2 * h2) if N % 2 else None),
        "tie3": _blocks_row(N, (4, 2, 0), (h3, h3, h3), lead=(3, N - 3 * h3) if N % 3 else None),
        "singleton": _blocks_row(N, (0, 2), (1, N - 1)),
    }
    return rows


def planted(Ls, N, thresh, group, seed):
    """(Ls, N) uint8 states.  Sequences come in groups of `group` round a centre (the centre is the group's first sequence); member k differs from the centre
    at a_k in {h - 1, h, h + 1} positions (h = thresh // 2) of its own part of the group's permutation of the positions, each with another state than the
    centre's, so two members lie a_i + a_j apart and a member a_k from its centre.  Centres: the first one with half of the positions re-drawn.  What N leaves
    over (at least one sequence) are exact duplicates.  Nine planted SNP rows (``CLASSES``) at random positions; the sequences permuted at the end."""
    rng = np.random.default_rng(seed)
    h = thresh // 2
    Lc = Ls - len(CLASSES)
    ngroups = (N - 1) // group if N >= 2 * group else 0
    assert ngroups == 0 or ((group - 1) * (h + 1) <= Lc and h >= 2), (Ls, N, thresh, group)
    core = np.empty((Lc, N), dtype=np.uint8)
    c0 = rng.integers(0, 4, Lc).astype(np.uint8)
    c0[rng.random(Lc) < 0.03] = 4
    for gi in range(ngroups):
        c = c0.copy()
        redraw = rng.permutation(Lc)[:Lc // 2]
        c[redraw] = rng.integers(0, 4, len(redraw))
        perm = rng.permutation(Lc)
        o = 0
        core[:, gi * group] = c
        for k in range(1, group):
            a = int(rng.integers(h - 1, h + 2))
            pos = perm[o:o + a]
            o += a
            m = c.copy()
            m[pos] = (c[pos].astype(np.int64) + 1 + rng.integers(0, 4, a)) % 5    # another state than the centre's, gaps included
            core[:, gi * group + k] = m
    n_own = ngroups * group
    if ngroups == 0:
        core[:] = rng.integers(0, 5, (Lc, N))
        n_own = N
    rows = _planted_rows(N, group)
    st = np.empty((Ls, N), dtype=np.uint8)
    where = np.sort(rng.choice(Ls, len(CLASSES), replace=False))
    st[np.setdiff1d(np.arange(Ls), where)] = core
    for w, name in zip(where, CLASSES):
        st[w] = rows[name]
    # duplicates: copies of sequences of the last third, on which every planted row is constant (so the ties stay exact)
    lo = N - N // 3
    for d in range(n_own, N):
        st[:, d] = st[:, int(rng.integers(lo, n_own))] if lo < n_own else st[:, n_own - 1]
    return np.ascontiguousarray(st[:, rng.permutation(N)]), {name: int(w) for w, name in zip(where, CLASSES)}


def columns_case(N, KR, seed, Ls=None):
    """An alignment of N sequences whose Hamming GEMM has exactly KR columns: SNPs of 3, 4 and 5 present states in turn (12 columns per round), topped up with
    biallelic SNPs one column at a time, one monomorphic (or all-gap) SNP after every six others, in random order.  The sequences are noisy copies of six
    centres with per-sequence rates between 2 % and 8 %, so distances within a cluster spread round a tenth of the SNPs.  KR = 0: Ls SNPs, all monomorphic
    or all-gap."""
    rng = np.random.default_rng(seed)
    ps, left = [], KR
    while left >= 12:
        ps += [3, 4, 5]
        left -= 12
    ps += [2] * left
    ps += [1] * (Ls if KR == 0 else len(ps) // 6 + 9)
    ps = np.array(ps)[rng.permutation(len(ps))]
    clusters = rng.integers(0, 6, N)
    clusters[:6] = np.arange(6)[:N]
    rate = rng.uniform(0.02, 0.08, N)
    st = np.empty((len(ps), N), dtype=np.uint8)
    for a, p in enumerate(ps):
        while True:
            if p == 1:
                st[a] = 4 if rng.random() < 0.3 else rng.integers(0, 4)
                break
            present = rng.permutation(5)[:p]
            centre = np.concatenate([np.arange(p), rng.integers(0, p, 6)])[:6][rng.permutation(6)]   # every state on some centre
            idx = centre[clusters]
            idx = np.where(rng.random(N) < rate, (idx + 1 + rng.integers(0, p - 1, N)) % p, idx)       # a mutation takes another of the SNP's states
            st[a] = present[idx]
            if len(np.unique(st[a])) == p:
                break
    assert n_columns(st) == KR
    return st


# ------------------------------------------------------------------------------------------------
# the cases, built once and shared
# ------------------------------------------------------------------------------------------------
#           N: (Ls, group, seed)
_PLANTED = {1: (300, 8, 1), 2: (300, 8, 2), 63: (600, 16, 3), 64: (600, 16, 21), 65: (600, 16, 5), 127: (800, 16, 6), 128: (800, 16, 7),
            129: (1000, 16, 8), 192: (700, 16, 9), 193: (500, 16, 10), 255: (900, 16, 11), 256: (640, 16, 12), 257: (1000, 16, 13),
            385: (1000, 16, 14)}
_KR_N = (70, 200)
_KR = (1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1151, 1152, 1153, 2047, 2048, 2049)
_KR0_L = (1, 5, 300)


class _Case:
    def __init__(self, name, st, thresh, kr=None, where=None):
        self.name, self.st, self.thresh, self.kr, self.where = name, st, thresh, kr, where
        self.Ls, self.N = st.shape

    @functools.cached_property
    def shared(self):
        return orc.shared_counts(self.st)

    @functools.cached_property
    def dist(self):
        return self.Ls - self.shared


@functools.lru_cache(maxsize=None)
def planted_case(N):
    Ls, group, seed = _PLANTED[N]
    thresh = int(0.1 * Ls)
    st, where = planted(Ls, N, thresh, group, seed)
    return _Case(f"planted N={N} L={Ls}", st, thresh, where=where)


@functools.lru_cache(maxsize=None)
def kr_case(N, KR, Ls=None):
    st = columns_case(N, KR, seed=1000 * N + KR + (Ls or 0), Ls=Ls)
    return _Case(f"columns N={N} KR={KR} L={len(st)}", st, int(0.1 * len(st)), kr=KR)


def kr_cases():
    for N in _KR_N:
        for Ls in _KR0_L:
            yield kr_case(N, 0, Ls)
        for KR in _KR:
            yield kr_case(N, KR)


# ------------------------------------------------------------------------------------------------
# 1. the generator has what the GPU tests rely on (oracle alone, no GPU)
# ------------------------------------------------------------------------------------------------
def test_generated_cases_meet_their_conditions(capsys):
    """Conditions, not measurements: every planted case of at least 63 sequences has >= 50 ordered off-diagonal pairs at each of the distances thresh - 1 and
    thresh, >= 1 at each of thresh - 2 and thresh + 1, >= 4 distinct neighbour counts, exact duplicates, every planted SNP class with its number of present
    states and its ties; from two tiles on, a pair at thresh - 1 or thresh across two 128-sequence tiles and, for every world of WORLDS that has two
    non-empty strips, across two strips.  Every columns case has the column count it was built for, SNPs of 1 to 5 present states (KR >= 63) and monomorphic
    SNPs in front of others, so that SNP index and column index differ.  Prints one line per case."""
    lines = []
    for N in _PLANTED:
        c = planted_case(N)
        st, t = c.st, c.thresh
        assert st.shape == (c.Ls, N) and st.max() <= 4
        p = n_present(st)
        w = c.where
        if N >= 63:
            assert [int(p[w[k]]) for k in CLASSES] == [1, 1, 2, 3, 4, 5, 2 + N % 2, 3 + (N % 3 > 0), 2], c.name
            assert (st[w["allgap"]] == 4).all()
            cnt = lambda k: np.bincount(st[w[k]], minlength=5)  # noqa: E731
            assert np.sort(cnt("tie2"))[-2:].tolist() == [N // 2, N // 2] and np.sort(cnt("tie3"))[-3:].tolist() == [N // 3] * 3, c.name
            assert np.sort(cnt("singleton"))[-2:].tolist() == [1, N - 1], c.name
            for k in ("biallelic", "three", "four", "five"):   # no tie where none is meant
                assert np.sort(cnt(k))[-1] > np.sort(cnt(k))[-2], (c.name, k)
        off = ~np.eye(N, dtype=bool)
        at = {d: int(((c.dist == t + d) & off).sum()) for d in (-2, -1, 0, 1)}
        ncnt = len(np.unique((c.dist < t).sum(axis=0)))
        lines.append(f"{c.name:24s} thresh={t:3d} KR={n_columns(st):5d} pairs at t-2,t-1,t,t+1 = {at[-2]:4d} {at[-1]:4d} {at[0]:4d} {at[1]:4d}  "
                     f"distinct neighbour counts = {ncnt}")
        if N < 63:
            continue
        assert at[-1] >= 50 and at[0] >= 50 and at[-2] >= 1 and at[1] >= 1, lines[-1]
        assert ncnt >= 4, lines[-1]
        assert int(((c.dist == 0) & off).sum()) >= 2, c.name                       # exact duplicates
        flip = ((c.dist == t - 1) | (c.dist == t)) & off
        if N > TILE:
            ti, tj = (x // TILE for x in np.nonzero(flip))
            assert (ti != tj).any(), c.name
            for world in WORLDS:
                strips = [s for s in hamming_tile_strips(N, world) if s[1] > s[0]]
                if len(strips) < 2:
                    continue
                owner = np.zeros((N + TILE - 1) // TILE, dtype=np.int64)
                for k, (t0, t1) in enumerate(strips):
                    owner[t0:t1] = k
                assert (owner[ti] != owner[tj]).any(), (c.name, world)
    for c in kr_cases():
        kr = n_columns(c.st)
        assert kr == c.kr, c.name
        p = n_present(c.st)
        assert (p <= 1).any() and (c.kr == 0 or (p[:np.nonzero(p > 1)[0][-1]] <= 1).any()), c.name
        if c.kr >= 63:
            assert set(np.unique(p).tolist()) >= ({1, 2, 3, 4, 5} if c.kr % 12 else {1, 3, 4, 5}), c.name
        if c.kr == 0:
            assert (c.dist == 0).all(), c.name
        off = ~np.eye(c.N, dtype=bool)
        t = c.thresh
        at = {d: int(((c.dist == t + d) & off).sum()) for d in (-2, -1, 0, 1)}
        lines.append(f"{c.name:24s} thresh={t:3d} KR={kr:5d} pairs at t-2,t-1,t,t+1 = {at[-2]:4d} {at[-1]:4d} {at[0]:4d} {at[1]:4d}  "
                     f"distinct neighbour counts = {len(np.unique((c.dist < t).sum(axis=0)))}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------
# the device against the oracle
# ------------------------------------------------------------------------------------------------
def _check_full(eng, c, tag=None):
    """shared == the oracle's (and symmetric, diagonal L); hdw == 1 / (count + 1), bit for bit, at every threshold of ``thresholds``."""
    tag = tag or c.name
    eng.set_alignment(c.st)
    hdw, shared = eng.hamming_weights(c.thresh, want_shared=True)
    assert np.array_equal(shared, c.shared), (tag, int((shared != c.shared).sum()))
    assert np.array_equal(shared, shared.T) and (np.diag(shared) == c.Ls).all(), tag
    assert np.array_equal(hdw, hdw_of(c.dist, c.thresh)), tag
    for t in thresholds(c.Ls):
        assert np.array_equal(eng.hamming_weights(t), hdw_of(c.dist, t)), (tag, t)
    return hdw


@pytest.mark.gpu
def test_shared_counts_and_weights_at_the_sequence_count_edges(engine):
    import c_oracle
    for N in _PLANTED:
        c = planted_case(N)
        _check_full(engine, c)
        # thresh = 1: exactly the duplicates are neighbours; thresh = L + 1: everyone is
        assert np.array_equal(engine.hamming_weights(1), 1.0 / ((c.dist == 0).sum(axis=0) + 1.0)), c.name
        assert np.array_equal(engine.hamming_weights(c.Ls + 1), np.full(N, 1.0 / (N + 1.0))), c.name
        if N in (65, 129, 257):   # a second opinion: the C oracle's pairwise loop
            h2, s2 = c_oracle.hamming_weights(c.st, c.thresh, want_shared=True)
            hdw, shared = engine.hamming_weights(c.thresh, want_shared=True)
            assert np.array_equal(shared, s2) and np.array_equal(hdw, h2), c.name


@pytest.mark.gpu
def test_column_count_at_the_chunk_edges(engine):
    for c in kr_cases():
        _check_full(engine, c)
        stats = engine.hamming_stats()
        assert stats["columns"] == n_columns(c.st) == c.kr, (c.name, stats["columns"])
        assert stats["k_padded"] == k_padded(c.kr), (c.name, stats["k_padded"])
        if c.kr == 0:
            _, shared = engine.hamming_weights(c.thresh, want_shared=True)
            assert (shared == c.Ls).all(), c.name
            assert np.array_equal(engine.hamming_weights(0), np.ones(c.N)), c.name
            for t in (1, 2, c.Ls, c.Ls + 1):
                assert np.array_equal(engine.hamming_weights(t), np.full(c.N, 1.0 / (c.N + 1.0))), (c.name, t)


@pytest.mark.gpu
def test_every_strip_counts_each_unordered_pair_once(engine):
    from ldweaver_amd.engine import Engine
    for N in (129, 257, 385):
        c = planted_case(N)
        ntiles = (N + TILE - 1) // TILE
        engine.set_alignment(c.st)
        for t in (c.thresh, c.thresh + 1):
            hdw = engine.hamming_weights(t)
            assert np.array_equal(hdw, hdw_of(c.dist, t)), (c.name, t)
            for k in range(ntiles):
                assert np.array_equal(engine.hamming_counts(t, k, k + 1), strip_counts(c.dist, t, k, k + 1)), (c.name, t, k)
            for world in WORLDS:
                strips = hamming_tile_strips(N, world)
                assert strips[0][0] == 0 and strips[-1][1] == ntiles and all(a[1] == b[0] for a, b in zip(strips, strips[1:])), (N, world)
                tot = np.zeros(N, dtype=np.int64)
                for t0, t1 in strips:
                    if t1 > t0:   # (more ranks than tiles: empty strips are skipped, as dist.hamming_weights_sharded does)
                        got = engine.hamming_counts(t, t0, t1)
                        assert np.array_equal(got, strip_counts(c.dist, t, t0, t1)), (c.name, t, world, t0, t1)
                        tot += got
                assert np.array_equal(1.0 / (tot + 1.0), hdw), (c.name, t, world)
        out = np.zeros(N, dtype=np.int64)
        lib = L.lib()
        for t0, t1 in ((1, 1), (2, 1), (0, ntiles + 1), (ntiles, ntiles + 1)):
            assert lib.ldw_hamming_counts(engine._ctx, c.thresh, t0, t1, L.ptr(out)) == L.LDW_ERR_ARG, (c.name, t0, t1)
    # several contexts of the one GPU: the strips of ldw_hamming_weights_multi
    c = planted_case(385)
    engs = [Engine(0) for _ in range(3)]
    try:
        for e in engs:
            e.set_alignment(c.st)
        for t in (c.thresh, c.thresh + 1):
            for n in (1, 2, 3):
                assert np.array_equal(Engine.hamming_weights_multi(engs[:n], t), hdw_of(c.dist, t)), (t, n)
    finally:
        for e in engs:
            e.close()


@pytest.mark.gpu
def test_the_context_carries_nothing_over(engine):
    """large -> KR = 0 -> small on ONE engine (the stage takes its buffers from a re-use pool per call and clears neither the transposed bits nor G), each
    against the oracle and against a fresh context."""
    from ldweaver_amd.engine import Engine
    for c in (planted_case(385), kr_case(200, 2049), kr_case(70, 0, 300), kr_case(70, 0, 1), planted_case(63), kr_case(70, 65)):
        _check_full(engine, c)
        hdw, shared = engine.hamming_weights(c.thresh, want_shared=True)
        with Engine(0) as fresh:
            fresh.set_alignment(c.st)
            h2, s2 = fresh.hamming_weights(c.thresh, want_shared=True)
        assert np.array_equal(shared, s2) and np.array_equal(hdw, h2), c.name

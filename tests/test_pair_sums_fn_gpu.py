"""The exact pair-sum kernels as functions (ldw_debug_pair_sums), against plain integer sums, over turns, shards and row lengths.

Every long-range MI of the default path is computed from the sums of k_pair_sums_q (a quarter-wave per pair, persistent waves), k_pair_sums (a wave per
pair, segment tables in LDS or in global memory) or k_pair_sums_bits (the bit walk), all in ldw_pairs.hip.  End to end they are only reached through whole
passes, where a block's lists fill one turn of the persistent grid, at most two.  Here the hook runs the sum kernels alone, through the launch code of the
default path, on caller-made lists and with a forced grid, and the whole sums buffer is compared with == :

  want[j * 4 + i] = sum over the sequences s of V_s [st[a, s] == state of a's row i] [st[b, s] == state of b's row j]        (numpy int64)

with V from debug_apx_params and the rows from debug_rows.  Paths 0..3 must write exactly the CA x CB entries k_pair_mi reads, path 4 all sixteen (0 where a
row is absent); every other int64 of the buffer — the other entries of paths 0..3, every slot at or past min(count, cap) — must still hold the fill pattern.

The case table is at module level; tests/test_pair_sums_cases_host.py checks, without a GPU, that it meets the conditions it is there for (a wave with three
turns, last turns of 1, 2 and 3 live rows, groups of four pairs over two and three shards, ...).  The issue's totals 0, 1, 3, 4, 5, 15, 16, 17, 33, 64, 67 hold
no total of 2 modulo 4, so 2 and 18 were added for the last turn with two live rows.

Sequence counts (words = 32-bit words of a bit row, Npad = N rounded up to 128; a lane l of a 16-lane row holds the words 32 k + 2 l, 32 k + 2 l + 1 of step k,
five steps from registers, the rest through the table):
  33     4 words: lanes 0, 1 busy          1 000   32 words: one step          5 000   160 words: all five register steps, no tail
  5 121  164 words: the first tail step with lanes 0, 1 busy          6 200   196 words: a whole tail step and a second one for lanes 0, 1 (and the tail of
  k_pair_sums, which keeps 192 words in registers)
The segment count the engine reports (apx_info) must equal the count derived here from the sorted weights, which pins the words and the classes.
"""
import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd.engine import Engine
from test_pair_sums_quarter import _alignment, _hand_weights
from test_sequence_count_edges import _dyadic

# ------------------------------------------------------------------------------------------------
# the case table (read by tests/test_pair_sums_cases_host.py)
# ------------------------------------------------------------------------------------------------
LS_FN = 600                      # SNPs of the alignments
CAP = 80                         # capacity of a list
PATHS, SHARDS = 5, 8
TOTALS = (0, 1, 3, 4, 5, 15, 16, 17, 33, 64, 67, 2, 18)      # entries of a path, split over its shards
SPLITS = ("shard 0", "shard 7", "even", "ragged", "clamped")
GRIDS = (1, 2, 5, 0)             # grid_wgs of the hook; 0: the default path's grid
PATH_SHAPES = ((1, 1), (2, 1), (1, 2), (2, 2))               # (rows of a, rows of b) of the lists of paths 0..3
GEN_SHAPES = ((1, 1), (3, 1), (1, 3), (2, 4), (4, 4), (3, 2))   # path 4: entry k of shard s has shape (k + s) mod 6
SEQ_WORDS = {33: 4, 1000: 32, 5000: 160, 5121: 164, 6200: 196}
REG_STEPS = 5                    # steps of 32 words whose segments a lane keeps in registers (PQ_KQ)
# (weighting, sequences): forms 1, 2 (and 0 -> 1) on the few-class weightings, forms 3, 4 (and 0 -> 4) on the distinct ones; every other form that can run, too
CASES = [("hamming", 33), ("hamming", 1000), ("hamming", 5000), ("hamming", 5121), ("hamming", 6200),
         ("hand", 1000), ("hand", 5000), ("hand tail", 6200),
         ("ones32", 1000), ("ones32", 5121),
         ("distinct", 1000), ("distinct", 5121), ("distinct", 6200)]


def words_of(N):
    return -(-N // 128) * 128 // 32


def shard_counts(total, split):
    """The eight counts of a path as the hook gets them (one may exceed CAP: the kernels clamp)."""
    c = [0] * SHARDS
    if split == "shard 0":
        c[0] = total
    elif split == "shard 7":
        c[7] = total
    elif split == "even":
        c = [total // SHARDS + (1 if s < total % SHARDS else 0) for s in range(SHARDS)]
    elif split == "ragged":                  # 1, 0, 0, 5, 0, 2, 0, rest
        left = total
        for s, n in ((0, 1), (3, 5), (5, 2)):
            c[s] = min(n, left)
            left -= c[s]
        c[7] = left
    elif split == "clamped":                 # shard 2 overflowed; the total goes in front of it and behind it
        c[0], c[2], c[3] = total // 2, CAP + 9, total - total // 2
    else:
        raise ValueError(split)
    return c


def live_counts(counts):
    return [min(n, CAP) for n in counts]


def entry_shape(path, shard, k):
    return PATH_SHAPES[path] if path < 4 else GEN_SHAPES[(k + shard) % len(GEN_SHAPES)]


POOL = 7                         # SNPs of each row count in the lists (a prime)


def entry_snps(sub, k):
    """Entry k of list sub: which SNP of the pool of its row count stands on the a side and on the b side."""
    return (3 * k + sub) % POOL, (k // POOL + 5 * k + 2 * sub + 1) % POOL


def index_space(live):
    """(shard, slot) of every pair of a path in the order the quarter-wave kernel walks them: the shards one after the other."""
    return [(s, k) for s in range(SHARDS) for k in range(live[s])]


def wave_turns(n_pairs, grid):
    """Wave w of `grid` workgroups takes the groups of four pairs w, w + 4 grid, ...: {wave: [group, ...]} of the waves that have any."""
    groups = -(-n_pairs // 4)
    return {w: list(range(w, groups, 4 * grid)) for w in range(min(4 * grid, groups))}


def busy_tail_lanes(words, step):
    """Lanes of a 16-lane row that hold words in tail step `step` (0: the first past the register steps)."""
    return [l for l in range(16) if 2 * (16 * (REG_STEPS + step) + l) < words]


# ------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------
FILL = Engine.PAIR_SUMS_FILL
_ALN = {}


def _aln(N):
    if N not in _ALN:
        seed = 700 + N
        syn = _alignment(N, seed, Ls=LS_FN)
        # every 13th SNP holds its major base and, planted, the three others: a gap in one sequence outside the planted groups (the group draw of
        # _alignment) makes five states, four indicator rows, at any sequence count
        grp = np.random.default_rng(seed + 1).integers(0, 12, N)
        col = int(np.flatnonzero((grp % 4 == 0) & (np.arange(N) > 0))[0])
        syn["states"][::13, col] = 4
        _ALN[N] = (syn, syn["states"].cpu().numpy())
    return _ALN[N]


def _hand_weights_tail(N):
    """_hand_weights with a second run of classes of 1, 2, 3 sequences ABOVE the large classes: the positions ascend in weight, so these share the last words."""
    sizes = [1, 2, 3] * 8
    rest = N - 2 * sum(sizes)
    big = [rest // 12] * 12
    big[-1] += rest - sum(big)
    sizes = sizes + big + [1, 2, 3] * 8
    k = (1 << 16) + 4099 * np.arange(len(sizes))
    w = np.repeat(np.ldexp(k.astype(np.float64), -22), sizes)
    return np.random.default_rng(N).permutation(w)


def _ones32_weights(N):
    """Four dyadic classes whose fixed-point values have all-ones low 32 bits (F = 38: the largest is 2^38 + 2^32 - 1, at the top of the 5-limb range)."""
    vals = np.array([(1 << 32) - 1, (1 << 33) - 1, (1 << 37) + (1 << 32) - 1, (1 << 38) + (1 << 32) - 1], dtype=np.int64)
    w = np.ldexp(vals.astype(np.float64), -38)[np.arange(N) % 4]
    return np.random.default_rng(N + 1).permutation(w)


def _segments_per_word(V):
    """(word, weight class) intersections per 32-bit word of a bit row: the positions ascend in weight, a class is a run of equal non-zero weights."""
    N = len(V)
    nw = -(-N // 32)
    vs = np.zeros(nw * 32, dtype=np.int64)
    vs[:N] = np.sort(V)
    vs = vs.reshape(nw, 32)
    return (vs[:, 0] > 0).astype(int) + ((vs[:, 1:] != vs[:, :-1]) & (vs[:, 1:] > 0)).sum(axis=1)


def _setup(eng, kind, N):
    """Loads the alignment and the weighting; returns the lists' SNPs, the expected sums of every slot and what the form choice depends on."""
    syn, st = _aln(N)
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(syn["states"])
    uqe = (eng.state_counts() > 0).T.astype(np.float64)
    if kind == "hamming":
        hdw = eng.hamming_weights(int(LS_FN * 0.1))
    elif kind == "hand":
        hdw = _hand_weights(N)
    elif kind == "hand tail":
        hdw = _hand_weights_tail(N)
    elif kind == "ones32":
        hdw = _ones32_weights(N)
    else:
        hdw = _dyadic(N, 900 + N)
    eng.set_weights(hdw)
    eng.set_snp_meta(uqe.sum(axis=1), uqe, syn["POS"], syn["paint"], float(syn["g"]))
    par, V, _ = eng.debug_apx_params()
    P = dict(zip(Engine.APX_PARAM_NAMES, par))
    info = eng.apx_info()
    words = words_of(N)
    segw = _segments_per_word(V)
    assert int(info["segments"]) == int(segw.sum()), (info, int(segw.sum()))
    if N in SEQ_WORDS:
        assert words == SEQ_WORDS[N]
    if kind == "ones32":
        assert int(P["F"]) == 38 and np.all((V & 0xFFFFFFFF) == 0xFFFFFFFF) and V.max() == (1 << 38) + (1 << 32) - 1 and len(np.unique(V)) == 4, (P["F"], np.unique(V))
    if kind in ("hand", "hand tail"):
        assert segw[:2].max() > 2, segw[:4]                      # more than two segments in a word: the table path of a lane's word
    if kind == "hand tail":
        assert segw[32 * REG_STEPS:].max() > 2, segw[32 * REG_STEPS:]   # ... and in a word of the tail
    if kind == "distinct":
        assert int(info["classes"]) == N and int(info["segments"]) == N, info

    row0, meta = eng.debug_rows()
    nrows = (meta & 7).astype(int)
    assert np.array_equal(nrows, np.diff(row0))
    pool = {n: np.flatnonzero(nrows == n)[:POOL] for n in (1, 2, 3, 4)}
    assert all(len(pool[n]) == POOL for n in pool), {n: len(p) for n, p in pool.items()}
    snps = np.concatenate([pool[n] for n in (1, 2, 3, 4)])
    at = {int(s): k for k, s in enumerate(snps)}
    # bits[k, i] = the sequences in which SNP snps[k] is in the state of its row i (nothing for an absent row), and their exact integer sums
    bits = np.zeros((len(snps), 4, N), dtype=np.int64)
    for k, s in enumerate(snps):
        m = int(meta[s])
        for i in range(m & 7):
            bits[k, i] = st[s] == ((m >> (8 + 3 * i)) & 7)
    flat = bits.reshape(-1, N)
    G = (flat * V[None, :]) @ flat.T                              # int64, exact: the engine keeps every sum below 2^52
    G = G.reshape(len(snps), 4, len(snps), 4)                     # [a, i, b, j]
    assert G.dtype == np.int64 and G.max() > 0

    a = np.zeros((PATHS * SHARDS, CAP), dtype=np.int32)
    b = np.zeros_like(a)
    want = np.full((PATHS * SHARDS, CAP, 16), FILL, dtype=np.int64)
    for sub in range(PATHS * SHARDS):
        path, shard = divmod(sub, SHARDS)
        for k in range(CAP):
            na, nb = entry_shape(path, shard, k)
            # (a, b) of slot k has period POOL^2 = 49 in k: no two turns of a wave (16, 32 or 80 slots apart) and no two rows of a wave hold the same pair,
            # so the sums of a stale or a neighbouring pair never pass for the right ones
            ia, ib = entry_snps(sub, k)
            sa, sb = int(pool[na][ia]), int(pool[nb][ib])
            a[sub, k], b[sub, k] = sa, sb
            ca, cb = (na, nb) if path < 4 else (4, 4)
            for j in range(cb):
                want[sub, k, 4 * j: 4 * j + ca] = G[at[sa], :ca, at[sb], j]
    lds = ((words + 4) * 4 + 15) // 16 * 16 + int(info["segments"]) * 16
    fits = lds <= 60000
    bits_can = 32 * (-(-words // 32) * 32) * 8 <= 160 * 1024
    many = (not fits) or int(info["segments"]) >= 8 * words
    auto = 4 if (many and bits_can) else (1 if fits else 3)      # what launch_pairs_exact documents
    return dict(a=a, b=b, want=want, fits=fits, bits_can=bits_can, auto=auto, words=words, info=info, pool=pool, nrows=nrows)


def _explain(got, want, what):
    bad = np.argwhere(got != want)
    l, k, e = (int(x) for x in bad[0])
    kind = "must keep the fill pattern" if want[l, k, e] == FILL else "a sum"
    return (f"{what}: {len(bad)} int64 differ, first at list {l} (path {l // SHARDS}, shard {l % SHARDS}) slot {k} entry {e} (j {e // 4}, i {e % 4}): "
            f"got {got[l, k, e]}, want {want[l, k, e]} ({kind})")


def _run_table(eng, S, form, expect):
    """Every total in every path, every split, every grid: the whole buffer == the expected one."""
    slot = np.arange(CAP)[None, :, None]
    calls = 0
    for rot in range(len(TOTALS)):
        totals = [TOTALS[(rot + p) % len(TOTALS)] for p in range(PATHS)]
        for split in SPLITS:
            counts = np.array([shard_counts(t, split) for t in totals], dtype=np.uint32).reshape(-1)
            live = np.minimum(counts, CAP)
            want = np.where(slot < live[:, None, None], S["want"], FILL)
            for grid in GRIDS:
                got, ran = eng.debug_pair_sums(counts, S["a"], S["b"], form=form, grid_wgs=grid)
                assert ran == expect, (form, ran, expect)
                if not np.array_equal(got, want):
                    raise AssertionError(_explain(got, want, f"form {form} grid {grid} split {split!r} totals {totals}"))
                calls += 1
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N", CASES)
def test_pair_sums_equal_the_integer_sums(engine, kind, N):
    S = _setup(engine, kind, N)
    few = kind != "distinct"
    assert S["bits_can"]
    if N >= 1000:
        assert S["auto"] == (1 if few else 4), S     # few classes: the quarter-wave kernel; N classes: the bit walk (up to Npad 20 480)
    if few or N == 1000:
        assert S["fits"]
    else:
        assert not S["fits"]                          # N x 16 B of segment records exceed the LDS: forms 1, 2 cannot run
    f0, k0 = engine.form_report(), engine.pair_kernel_report()
    calls = 0
    for form in (1, 2):
        if not S["fits"]:
            with pytest.raises(L.LdwError) as err:
                engine.debug_pair_sums(np.ones(PATHS * SHARDS, dtype=np.uint32), S["a"], S["b"], form=form, grid_wgs=1)
            assert err.value.code == L.LDW_ERR_STATE, err.value
    for form in (0, 1, 2, 3, 4):
        if form in (1, 2) and not S["fits"]:
            continue
        calls += _run_table(engine, S, form, S["auto"] if form == 0 else form)
    assert engine.form_report() == f0 and engine.pair_kernel_report() == k0     # the hook counts nothing
    print(f"{kind} N {N}: {S['words']} words, {int(S['info']['classes'])} classes, {int(S['info']['segments'])} segments, form 0 -> {S['auto']}, {calls} launches equal")


@pytest.mark.gpu
def test_bit_walk_refused_beyond_160_kb(engine):
    """Npad 20 608: the per-position table of the bit walk needs 164 864 B: form 4 answers LDW_ERR_STATE, the others run and agree."""
    N = 20500
    S = _setup(engine, "hand", N)
    assert not S["bits_can"] and S["fits"] and S["auto"] == 1, S
    counts = np.array([shard_counts(17, "ragged")] * PATHS, dtype=np.uint32).reshape(-1)
    want = np.where(np.arange(CAP)[None, :, None] < np.minimum(counts, CAP)[:, None, None], S["want"], FILL)
    with pytest.raises(L.LdwError) as err:
        engine.debug_pair_sums(counts, S["a"], S["b"], form=4, grid_wgs=1)
    assert err.value.code == L.LDW_ERR_STATE, err.value
    for form, grid in ((0, 0), (1, 1), (2, 1), (3, 2)):
        got, ran = engine.debug_pair_sums(counts, S["a"], S["b"], form=form, grid_wgs=grid)
        assert ran == (form or 1)
        assert np.array_equal(got, want), _explain(got, want, f"form {form} grid {grid}")


@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(engine):
    S = _setup(engine, "hamming", 1000)
    counts = np.zeros(PATHS * SHARDS, dtype=np.uint32)
    counts[0], counts[4 * SHARDS + 1] = 2, 3
    want = np.where(np.arange(CAP)[None, :, None] < counts[:, None, None].astype(np.int64), S["want"], FILL)

    def good():
        got, ran = engine.debug_pair_sums(counts, S["a"], S["b"], form=1, grid_wgs=1)
        assert ran == 1 and np.array_equal(got, want), _explain(got, want, "after a refusal")

    def refused(code, a=None, b=None, **kw):
        with pytest.raises(L.LdwError) as err:
            engine.debug_pair_sums(kw.pop("counts", counts), S["a"] if a is None else a, S["b"] if b is None else b, **kw)
        assert err.value.code == code, err.value
        good()

    good()
    for bad in (-1, LS_FN):                                       # an SNP out of range, either side
        a = S["a"].copy()
        a[0, 1] = bad
        refused(L.LDW_ERR_ARG, a=a)
        b = S["b"].copy()
        b[4 * SHARDS + 1, 2] = bad
        refused(L.LDW_ERR_ARG, b=b)
    a = S["a"].copy()
    a[0, 0] = S["pool"][2][0]                                     # 2 x 1 rows in the list of 1 x 1
    refused(L.LDW_ERR_ARG, a=a)
    none = np.flatnonzero(S["nrows"] == 0)
    if len(none):                                                 # a SNP without an indicator row has no place in any list
        b = S["b"].copy()
        b[4 * SHARDS + 1, 0] = none[0]
        refused(L.LDW_ERR_ARG, b=b)
    refused(L.LDW_ERR_ARG, a=np.zeros((PATHS * SHARDS, 0), dtype=np.int32), b=np.zeros((PATHS * SHARDS, 0), dtype=np.int32))   # cap 0
    refused(L.LDW_ERR_ARG, form=5)
    refused(L.LDW_ERR_ARG, grid_wgs=-1)
    a = S["a"].copy()
    a[0, 2:] = -1                                                 # slots past the count are not entries: never read
    got, _ = engine.debug_pair_sums(counts, a, S["b"], form=1, grid_wgs=1)
    assert np.array_equal(got, want)
    with Engine(0) as fresh:                                      # no weights: no tables
        fresh.set_alignment(_aln(1000)[0]["states"])
        with pytest.raises(L.LdwError) as err:
            fresh.debug_pair_sums(counts, S["a"], S["b"])
        assert err.value.code == L.LDW_ERR_STATE, err.value

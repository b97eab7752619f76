"""The case table of tests/test_apx_fused_gpu.py holds the situations it was made for, and the model it is judged by gives hand-worked answers (no GPU).

With unit weights the accumulators of the fused approximate GEMM are the exact co-occurrence counts bits[rows_t] @ bits[rows_f].T (e_last = 0: nothing is
truncated), so everything the launches must write follows from the inputs here, through tests/apx_fused_ref.py.  These are conditions on the inputs, not
measurements; the GPU test checks the same conditions on the accumulators it really gets."""
import numpy as np
import pytest

import apx_fused_cases as CS
import apx_fused_ref as REF
from ldweaver_amd.synth import synth_alignment

U, I = REF.UNWRITTEN, REF.INT_MAX


def indicator_bits(states):
    """One row per (SNP, state but the most common one): enough to draw co-occurrence counts from; not the engine's own row order."""
    rows = []
    for col in np.asarray(states):
        vals, counts = np.unique(col, return_counts=True)
        rows += [col == v for v in vals[np.argsort(-counts, kind="stable")][1:]]
    return np.array(rows, dtype=np.int64)


@pytest.fixture(scope="module", params=[(200, 11), (700, 12)], ids=["N200", "N700"])
def table(request):
    N, seed = request.param
    bits = indicator_bits(synth_alignment(500, N, seed=seed)["states"])
    cases = CS.make_cases(len(bits), lambda rt, rf: bits[rt] @ bits[rf].T, seed)
    return cases, [CS.situations(c) for c in cases]


def test_every_required_situation_is_in_the_table(table):
    cases, held = table
    seen = set().union(*held)
    for name in CS.REQUIRED:
        assert name in seen, f"no case holds: {name}"
    assert seen <= set(CS.REQUIRED), seen - set(CS.REQUIRED)


def test_the_table_covers_every_shape_and_scenario(table):
    cases, held = table
    shapes = {(c["nrt"], c["nrf"]) for c in cases}
    assert shapes == {(a, b) for a in CS.NRT for b in CS.NRF}
    names = {c["name"] for c in cases}
    assert names == {"epi", "epi_nomaybe", "epi_cap", "epi_lower", "rule_a", "rule_b", "flat"}
    assert sorted({-(-a // 128) * -(-b // 128) * 2 for a, b in shapes}) == [2, 4, 6, 8, 12, 16]      # wave tiles of the padded launches
    for c in cases:
        assert (c["rflag_t"] is None) == (c["rflag_f"] is None)
        assert all(b < 64 or b == 255 for b in c["bin_t"]) and all(b < 64 or b == 255 for b in c["bin_f"])
        if c["name"] == "epi_cap":
            assert 0 < c["maybe_cap"] < CS.expect(c, False).maybe_n, "the capacity is not below the total"
        if c["name"] == "epi_nomaybe":
            assert c["maybe_cap"] == -1 and CS.expect(c, False).maybe_n == 0 and not CS.expect(c, False).maybe


def test_fail_counts_are_products_whatever_the_data(table):
    """|A| |B| (+ 1): the same counts from any accumulators, except where bin 3 meets bin 3."""
    cases, _ = table
    for c in cases:
        if not c["name"].startswith("epi"):
            continue
        pbt, pbf = c["pad"][0], c["pad"][1]
        other = CS.REF.model(np.full_like(c["acc"], 7), pbt, pbf, c["tab"], sr_mask=c["sr_mask"], lower_only=c["lower_only"], maybe=c["maybe_cap"] > 0, maybe_max=CS.MAYBE_MAX)
        for (g, x), fails in CS.expect(c, False).fails.items():
            a = sum(pbt[32 * g:32 * g + 32] == 1) * sum(pbf[64 * x:64 * x + 64] == 1) + sum(pbt[32 * g:32 * g + 32] == 2) * sum(pbf[64 * x:64 * x + 64] == 2)
            n33 = sum(pbt[32 * g:32 * g + 32] == 3) * sum(pbf[64 * x:64 * x + 64] == 3)
            assert a <= len(fails) <= a + n33, (c["name"], g, x)
            if n33 == 0:
                assert len(other.fails[g, x]) == a


# ------------------------------------------------------------------------------------------------
# the model against answers worked out by hand: 128 x 128 accumulators = one tile row of two tiles, four regions each
# ------------------------------------------------------------------------------------------------
def _flat_inputs(rows=128):
    acc = np.full((rows, 128), 5, dtype=np.int64)
    tab = np.empty((64, 64, 2), dtype=np.int64)
    tab[:, :] = (-1, I)
    return acc, np.zeros(rows, dtype=np.int64), np.zeros(128, dtype=np.int64), tab


def test_model_by_hand_strict_thresholds_and_the_list():
    acc, bt, bf, tab = _flat_inputs()
    tab[0, 0] = (4, 6)                       # 4 < 5 < 6: every entry passes
    E = REF.model(acc, bt, bf, tab)
    assert E.clean.tolist() == [[1, 1], [1, 1], [1, 1], [1, 1]] and not E.stored.any() and E.maybe == [] and E.live == {(0, 0), (0, 1)}
    acc[33, 70] = 6                          # Hq itself: fails; row 33 is in region 1, column 70 in tile 1
    acc[127, 0] = 4                          # Lq itself: fails; region 3 of tile 0
    E = REF.model(acc, bt, bf, tab)
    assert E.clean.tolist() == [[1, 1], [1, 1], [1, 1], [1, 1]] and not E.stored.any()
    assert E.maybe == [(33, 70, 6), (127, 0, 4)] and E.maybe_n == 2
    E = REF.model(acc, bt, bf, tab, maybe=False)
    assert E.clean.tolist() == [[1, 1], [1, 0], [1, 1], [0, 1]] and E.stored.tolist() == [[False, False], [False, True], [False, False], [True, False]] and E.maybe_n == 0
    tab[0, 0] = (5, 6)                       # 5 is not above Lq = 5: 2048 fails per region, more than any list takes
    E = REF.model(acc, bt, bf, tab)
    assert E.clean.tolist() == [[0, 0]] * 4 and E.stored.all() and E.maybe == []
    acc[:] = 5
    acc[0, :64], acc[1, :33] = 9, 9          # 97 fails in region 0 of tile 0: one too many; 96 after the next line
    tab[0, 0] = (4, 6)
    assert REF.model(acc, bt, bf, tab).clean.tolist() == [[0, 1], [1, 1], [1, 1], [1, 1]]
    acc[1, 32] = 5
    E = REF.model(acc, bt, bf, tab)
    assert E.clean.tolist() == [[1, 1]] * 4 and E.maybe_n == 96 and E.maybe[0] == (0, 0, 9) and E.maybe[-1] == (1, 31, 9)


def test_model_by_hand_bins_and_the_mask():
    acc, bt, bf, tab = _flat_inputs()
    bt[40] = 255                             # region 1 of both tiles holds a row without a bin
    bf[127] = 255                            # every region of tile 1 holds a column without one
    E = REF.model(acc, bt, bf, tab)
    assert E.clean.tolist() == [[1, 0], [0, 0], [1, 0], [1, 0]] and (E.stored == (E.clean == 0)).all()
    mask = np.array([[3, 0]], dtype=np.uint8)
    E = REF.model(acc, bt, bf, tab, sr_mask=mask)
    assert E.clean.tolist() == [[0, 0]] * 4 and E.stored.all() and E.live == {(0, 0), (0, 1)}


def test_model_by_hand_pruning():
    acc, bt, bf, tab = _flat_inputs(256)     # two tile rows
    E = REF.model(acc, bt, bf, tab, prune=True)
    assert E.live == set() and E.pruned == 4 and E.clean.tolist() == [[1, 1]] * 8 and not E.stored.any()
    E = REF.model(acc, bt, bf, tab, prune=True, lower_only=True)          # tile row 1: columns 0..127 all lie below row 128
    assert E.pruned == 2 and E.clean.tolist() == [[1, 1]] * 4 + [[U, U]] * 4 and E.live == set()
    E = REF.model(acc, bt, bf, tab, prune=False, lower_only=True)
    assert E.live == {(0, 0), (0, 1)} and E.clean.tolist() == [[1, 1]] * 4 + [[U, U]] * 4
    bt[:128] = np.arange(128) % 8 + 10       # to-bins 10..17
    bf[:64] = np.arange(64) % 8 + 20         # 8 x 8 = 64 entries: pruned
    bf[64:] = np.arange(64) % 9 + 20         # 8 x 9 = 72: computed, and clean
    E = REF.model(acc, bt, bf, tab, prune=True)
    assert E.live == {(0, 1)} and E.pruned == 3 and E.rule[0, 0] == "a" and E.clean.tolist() == [[1, 1]] * 8
    tab[17, 27] = (-1, I - 1)                # passes everything, but is not the unconditional entry
    E = REF.model(acc, bt, bf, tab, prune=True)
    assert E.live == {(0, 0), (0, 1)} and E.pruned == 2
    # rule (b): to-rows of kind 3 (no bins), dead versus kind 2; from-rows of kind 2
    ft, ff = np.full(256, 3 | 4), np.full(128, 2)
    bt[:] = 255
    E = REF.model(acc, bt, bf, tab, rflag_t=ft, rflag_f=ff, prune=True)
    assert E.pruned == 4 and E.pruned_b == 4 and (E.clean == U).all() and E.live == set()
    ft[5] = 3                                # one to-row of tile row 0 is not dead
    E = REF.model(acc, bt, bf, tab, rflag_t=ft, rflag_f=ff, prune=True)
    assert E.live == {(0, 0), (0, 1)} and E.pruned == 2 and E.clean.tolist() == [[0, 0]] * 4 + [[U, U]] * 4
    ff[:64] = 2 | 8                          # ... but the from-rows of tile 0 are dead versus kind 3
    E = REF.model(acc, bt, bf, tab, rflag_t=ft, rflag_f=ff, prune=True)
    assert E.live == {(0, 1)} and E.detail[0, 0] == ("b", False, 3, 2, False, True)
    ff[3] = 3 | 8                            # a from-row of the other kind: no rule (b) for column block 0, not even under the dead to-rows of tile row 1
    assert REF.model(acc, bt, bf, tab, rflag_t=ft, rflag_f=ff, prune=True).live == {(0, 0), (0, 1), (1, 0)}

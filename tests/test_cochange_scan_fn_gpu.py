"""GPU: the pair kernel of the co-change scan as a function (ldw_debug_cochange_scan, ldw_debug_cochange_links; pytest -m gpu) against the numpy
statement tests/cochange_scan_ref.py.  Everything compared is an integer and every comparison is array_equal; lists are compared after a lexsort."""
import ctypes as C

import numpy as np
import pytest

import cochange_scan_ref as CR
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

SLOTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 321)      # both tile edges (256 on the I side, 64 on the J side), a diagonal tile, ragged last tiles
WORDS = (1, 7, 8, 9, 17, 33)


def problem(rng, M, words, density, all_ones=0):
    """M slots of ``words`` words: random bits of the given density with bit 0 of word 0 (the root, which no tree sets) clear; the first ``all_ones`` rows
    have every bit of every word set."""
    nodes = 32 * words
    change = rng.random((M, nodes)) < density
    change[:, 0] = False
    change[:all_ones] = True
    idx = np.sort(rng.choice(4 * M + 8, size=M, replace=False)).astype(np.int32)
    pos = rng.integers(1, 5000, size=M).astype(np.int32)
    return dict(change=change, bits=CR.pack_bits(change), changes=change.sum(axis=1).astype(np.int32), idx=idx, pos=pos, g=5000.0, B=nodes - 1)


def check(engine, pr, min_co=0, min_lift=0, min_len=-1.0, tag=None):
    """Scan and links on the device against the reference; returns the reference's scan."""
    kw = dict(min_co=min_co, min_lift=min_lift, min_len=min_len, pos=pr["pos"], g=pr["g"])
    want = CR.scan(pr["change"], pr["changes"], pr["B"], min_co, min_lift, min_len, pr["pos"], pr["g"])
    got = engine.debug_cochange_scan(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)
    for k in ("hist", "best", "nge"):
        assert np.array_equal(got[k], want[k]), (tag, k)
    assert (got["npairs"], got["n_qualifying"]) == (want["npairs"], want["n_qualifying"]), tag
    assert int(got["hist"].sum()) == got["n_qualifying"], tag
    ref = CR.links(pr["change"], pr["changes"], pr["idx"], pr["B"], min_co, min_lift, min_len, pr["pos"], pr["g"], want["best"])
    n = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)             # cap = 0 with null lists: a pure count
    assert n["count"] == ref["count"] and n["a"] is None and n["partner"] is None, tag
    lk = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], cap=ref["count"], best_in=got["best"], **kw)
    assert lk["count"] == ref["count"], tag
    if ref["count"]:
        assert all(np.array_equal(x, y) for x, y in zip(CR.sorted_links(lk), CR.sorted_links(ref))), (tag, "lists")
        assert np.all(lk["a"] < lk["b"]), tag
    assert np.array_equal(lk["partner"], ref["partner"]), (tag, "partner")
    return want


@pytest.mark.parametrize("M", SLOTS)
def test_slot_counts_on_both_sides_of_the_tile_edges(engine, M):
    rng = np.random.default_rng(M)
    for words, density in ((1, 0.5), (9, 0.02), (9, 0.5)):
        pr = problem(rng, M, words, density)
        check(engine, pr, tag=(M, words, density, "all"))
        check(engine, pr, min_co=2, min_lift=1, tag=(M, words, density, "lift 1"))
        check(engine, pr, min_co=1, min_lift=2, min_len=700.0, tag=(M, words, density, "lift 2, len"))


@pytest.mark.parametrize("words", WORDS)
def test_word_counts_and_densities_with_rows_of_all_ones(engine, words):
    rng = np.random.default_rng(words)
    for density in (0.02, 0.5):
        pr = problem(rng, 130, words, density, all_ones=3)
        want = check(engine, pr, min_co=3, tag=(words, density))
        assert want["best"][0] == 32 * words                           # two rows of all ones share every branch
        check(engine, pr, min_co=1, min_lift=1, min_len=100.0, tag=(words, density, "filters"))


def test_co_above_1023_and_exactly_1023_share_the_last_bin(engine):
    """33 words: two all-ones rows give co = 1056, a row of 1023 bits gives exactly 1023 with each of them."""
    rng = np.random.default_rng(33)
    pr = problem(rng, 70, 33, 0.5, all_ones=2)
    pr["change"][2] = False
    pr["change"][2, 1:1024] = True
    pr["bits"], pr["changes"] = CR.pack_bits(pr["change"]), pr["change"].sum(axis=1).astype(np.int32)
    want = check(engine, pr, min_co=1000, tag="cap")
    co = want["co"]
    assert co[0, 1] == 1056 and co[0, 2] == 1023 and co[1, 2] == 1023
    assert want["hist"][1023] >= 3 and int(((co > 1023) & want["q"]).sum()) >= 1 and int(((co == 1023) & want["q"]).sum()) >= 2
    got = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], min_co=1024, cap=8)
    assert got["count"] == 1 and got["co"].tolist() == [1056]          # the list keeps the count the histogram caps


def test_the_lift_at_equality(engine):
    """B = 24, changes 4 and 3, co = 2: 2 x 24 = 48 = 4 x 4 x 3 qualifies at min_lift 4 and not at 5."""
    change = np.zeros((2, 25), dtype=bool)
    change[0, [1, 2, 3, 4]] = True
    change[1, [3, 4, 5]] = True
    pr = dict(change=change, bits=CR.pack_bits(change), changes=np.array([4, 3], dtype=np.int32), idx=np.array([10, 20], dtype=np.int32),
              pos=np.array([1, 2], dtype=np.int32), g=100.0, B=24)
    at4, at5 = check(engine, pr, min_lift=4, tag="lift 4"), check(engine, pr, min_lift=5, tag="lift 5")
    assert (at4["n_qualifying"], at5["n_qualifying"], at4["npairs"], at5["npairs"]) == (1, 0, 1, 1)
    assert at4["best"].tolist() == [2, 2] and at5["best"].tolist() == [-1, -1] and at4["hist"][2] == 1
    top = check(engine, dict(pr, changes=np.array([2 ** 21 - 1, 2 ** 21 - 1], dtype=np.int32), B=2 ** 21 - 1), min_lift=2 ** 20, tag="int64")
    assert top["n_qualifying"] == 0                                    # 2^20 (2^21 - 1)^2 stays inside int64


def test_min_len_on_a_circle(engine):
    """g = 1000, min_len = 100: the pair at exactly 100 (40, 140) is out, the one at 101 (60, 161) is in; of the two whose short way round crosses the origin
    (950, 40) at 90 is out and (950, 60) at 110 is in."""
    pos = np.array([40, 60, 140, 161, 950], dtype=np.int32)
    rng = np.random.default_rng(5)
    change = rng.random((5, 40)) < 0.5
    change[:, 0] = False
    pr = dict(change=change, bits=CR.pack_bits(change), changes=change.sum(axis=1).astype(np.int32), idx=np.arange(5, dtype=np.int32), pos=pos, g=1000.0, B=39)
    want = check(engine, pr, min_len=100.0, tag="circle")
    in_p, _ = CR.pair_sets(want["co"], pr["changes"], 39, 0, 100.0, pos, 1000.0)
    assert np.argwhere(in_p).tolist() == [[0, 3], [1, 3], [1, 4], [2, 4], [3, 4]]
    lk = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], 39, min_len=100.0, pos=pos, g=1000.0, cap=10)
    assert sorted(zip(lk["a"].tolist(), lk["b"].tolist())) == [(0, 3), (1, 3), (1, 4), (2, 4), (3, 4)]
    assert check(engine, pr, min_len=0.0, tag="zero")["npairs"] == 10 and check(engine, pr, min_len=500.0, tag="half")["npairs"] == 0


def raw_links(engine, pr, min_co, cap, room):
    """ldw_debug_cochange_links straight through ctypes, the three lists ``room`` entries long and filled with a guard value."""
    lists = [np.full(room, -7, dtype=np.int32) for _ in range(3)]
    n = C.c_int64(-1)
    ch, ix = pr["changes"], pr["idx"]
    rc = L.lib().ldw_debug_cochange_links(engine._ctx, L.ptr(pr["bits"]), pr["bits"].shape[0], pr["bits"].shape[1], L.ptr(ch), L.ptr(ix), None, 0.0, pr["B"], min_co, 0, -1.0,
                                          None, cap, *[L.ptr(x) for x in lists], C.byref(n), None)
    return rc, int(n.value), lists


def test_cap_below_at_and_above_the_count_and_cap_zero(engine):
    rng = np.random.default_rng(21)
    pr = problem(rng, 257, 7, 0.3)
    ref = CR.links(pr["change"], pr["changes"], pr["idx"], pr["B"], min_co=32)
    count = ref["count"]
    assert 20 < count < 3000
    for cap in (count, count + 5):
        rc, n, lists = raw_links(engine, pr, 32, cap, count + 9)
        assert rc == L.LDW_OK and n == count
        assert all(np.array_equal(x, y) for x, y in zip(CR.sorted_links(dict(a=lists[0][:n], b=lists[1][:n], co=lists[2][:n])), CR.sorted_links(ref)))
        assert all(np.all(x[n:] == -7) for x in lists)
    rc, n, lists = raw_links(engine, pr, 32, count - 3, count + 9)
    assert rc == L.LDW_ERR_SIZE and n == count and all(np.all(x[count - 3:] == -7) for x in lists)      # nothing past cap
    assert b"ldw_debug_cochange_links" in L.lib().ldw_last_error()
    with pytest.raises(L.LdwError) as e:
        engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], min_co=32, cap=1)
    assert e.value.code == L.LDW_ERR_SIZE and e.value.count == count
    assert engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], min_co=32)["count"] == count
    n = C.c_int64(0)
    one = np.zeros(1, dtype=np.int32)
    rc = L.lib().ldw_debug_cochange_links(engine._ctx, L.ptr(pr["bits"]), 7, 257, L.ptr(pr["changes"]), L.ptr(pr["idx"]), None, 0.0, pr["B"], 32, 0, -1.0, None, 4, L.ptr(one),
                                          None, L.ptr(one), C.byref(n), None)
    assert rc == L.LDW_ERR_ARG and b"cap 4 needs the three lists" in L.lib().ldw_last_error()


def test_a_tie_on_co_between_two_partners_goes_to_the_smaller_snp(engine):
    """Slot 0 shares two branches with slot 70 and two with slot 300 (another wave, another tile): its partner is the smaller SNP; slots 70 and 300 share none."""
    M = 321
    change = np.zeros((M, 64), dtype=bool)
    change[0, [1, 2, 3, 4]] = True
    change[70, [1, 2]] = True
    change[300, [3, 4]] = True
    idx = (np.arange(M, dtype=np.int32) * 3 + 1)
    pr = dict(change=change, bits=CR.pack_bits(change), changes=np.maximum(change.sum(axis=1), 1).astype(np.int32), idx=idx, pos=np.arange(M, dtype=np.int32), g=1000.0,
              B=63)
    want = check(engine, pr, min_co=1, tag="tie")
    assert want["best"][0] == 2 and want["best"][70] == 2 and want["best"][300] == 2
    lk = engine.debug_cochange_links(pr["bits"], pr["changes"], idx, 63, min_co=1, cap=4, best_in=want["best"])
    assert lk["partner"][0] == idx[70] and lk["partner"][70] == idx[0] and lk["partner"][300] == idx[0]
    assert lk["partner"][1] == idx[0] and lk["partner"][5] == idx[0] and want["best"][1] == 0          # co = 0 is a best too: the smallest partner of all
    none = engine.debug_cochange_links(pr["bits"], pr["changes"], idx, 63, min_co=1, cap=4, best_in=np.full(M, -1, dtype=np.int32))
    assert np.all(none["partner"] == -1) and none["count"] == 2


@pytest.mark.parametrize("rows", ("1", "2"))
def test_forced_launch_bands_give_the_results_of_one_launch(engine, monkeypatch, rows):
    rng = np.random.default_rng(31)
    pr = problem(rng, 700, 5, 0.3)                                     # three tile rows
    monkeypatch.delenv("LDW_COSCAN_ROWS", raising=False)
    kw = dict(min_co=24, min_lift=1, min_len=300.0, pos=pr["pos"], g=pr["g"])
    want = engine.debug_cochange_scan(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)
    n = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)["count"]
    want_l = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], cap=n, best_in=want["best"], **kw)
    assert n > 10
    monkeypatch.setenv("LDW_COSCAN_ROWS", rows)
    check(engine, pr, min_co=24, min_lift=1, min_len=300.0, tag=("bands", rows))
    got = engine.debug_cochange_scan(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)
    got_l = engine.debug_cochange_links(pr["bits"], pr["changes"], pr["idx"], pr["B"], cap=n, best_in=got["best"], **kw)
    assert all(np.array_equal(got[k], want[k]) for k in ("hist", "best", "nge")) and got["npairs"] == want["npairs"]
    assert all(np.array_equal(x, y) for x, y in zip(CR.sorted_links(got_l), CR.sorted_links(want_l))) and np.array_equal(got_l["partner"], want_l["partner"])


def test_refusals_leave_the_context_usable(engine):
    rng = np.random.default_rng(41)
    pr = problem(rng, 20, 2, 0.5)
    bad = [
        (dict(min_co=-1), "min_co -1"), (dict(min_lift=-1), "min_lift -1"), (dict(min_lift=2 ** 20 + 1), "min_lift 1048577"), (dict(min_len=np.nan), "min_len is NaN"),
        (dict(min_len=5.0), "needs pos"), (dict(min_len=5.0, pos=pr["pos"], g=0.0), "positive g"),
    ]
    for kw, msg in bad:
        for call in (engine.debug_cochange_scan, engine.debug_cochange_links):
            with pytest.raises(L.LdwError, match=msg) as e:
                call(pr["bits"], pr["changes"], pr["idx"], pr["B"], **kw)
            assert e.value.code == L.LDW_ERR_ARG, msg
        check(engine, pr, tag=("after", msg))
    for change_ in (dict(idx=pr["idx"][::-1].copy()), dict(changes=np.full(20, -1, dtype=np.int32)), dict(B=0), dict(B=2 ** 21)):
        p2 = dict(pr, **change_)
        with pytest.raises(L.LdwError) as e:
            engine.debug_cochange_scan(p2["bits"], p2["changes"], p2["idx"], p2["B"])
        assert e.value.code == L.LDW_ERR_ARG
    n = C.c_int64(0)
    part = np.zeros(20, dtype=np.int32)
    rc = L.lib().ldw_debug_cochange_links(engine._ctx, L.ptr(pr["bits"]), 2, 20, L.ptr(pr["changes"]), L.ptr(pr["idx"]), None, 0.0, pr["B"], 0, 0, -1.0, None, 0, None, None, None,
                                          C.byref(n), L.ptr(part))
    assert rc == L.LDW_ERR_ARG and b"partner_out needs best_in" in L.lib().ldw_last_error()
    check(engine, pr, tag="after all")

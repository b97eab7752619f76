"""The case table of tests/test_pair_sums_fn_gpu.py meets the conditions it was made for (no GPU).

From the mapping in k_pair_sums_q's comment (ldw_pairs.hip): the eight shards of a path are one index space (the clamped counts one after the other), a group
is four consecutive pairs of it — one per 16-lane row of a wave —, and wave w of g workgroups takes the groups w, w + 4 g, ...  These are conditions on the
inputs, not measurements."""
import itertools

import test_pair_sums_fn_gpu as T


def _groups(live):
    sp = T.index_space(live)
    return [sp[k:k + 4] for k in range(0, len(sp), 4)]


def _all_lists():
    for total, split in itertools.product(T.TOTALS, T.SPLITS):
        yield total, split, T.live_counts(T.shard_counts(total, split))


def test_the_splits_hold_their_totals():
    for total, split, live in _all_lists():
        counts = T.shard_counts(total, split)
        assert len(counts) == T.SHARDS and all(n >= 0 for n in counts)
        if split == "clamped":
            assert counts[2] == T.CAP + 9 and live[2] == T.CAP and sum(live) == total + T.CAP
        else:
            assert counts == live and sum(live) == total, (total, split, counts)
    assert T.shard_counts(67, "ragged") == [1, 0, 0, 5, 0, 2, 0, 59]
    assert T.shard_counts(3, "ragged") == [1, 0, 0, 2, 0, 0, 0, 0]
    assert T.shard_counts(17, "even") == [3, 2, 2, 2, 2, 2, 2, 2]


def test_turns_of_the_persistent_loop():
    turns = {}
    for total, split, live in _all_lists():
        for grid in T.GRIDS:
            if grid:
                turns[total, split, grid] = T.wave_turns(sum(live), grid)
    # with one workgroup a turn is 16 pairs: one, two, three and five turns, full and partial last turns
    assert [len(T.wave_turns(t, 1).get(0, [])) for t in (16, 17, 33, 64, 67)] == [1, 2, 3, 4, 5]
    assert max(len(g) for w in turns.values() for g in w.values()) >= 3
    # a partial last turn: some waves of a workgroup have a next group, others do not (has_nx differs between the waves)
    assert any(len({len(g) for g in w.values()}) > 1 for w in turns.values())
    # at two workgroups some waves turn once more than others, and both take more than one turn
    assert any(grid == 2 and {len(g) for g in w.values()} >= {2, 3} for (_, _, grid), w in turns.items())
    # more workgroups than groups: the surplus leaves unstaged
    assert any(grid == 5 and 0 < sum(live) <= 16 * 4 for total, split, live in _all_lists() for grid in T.GRIDS)
    # the last group of a path holds 1, 2 and 3 live rows (and 4)
    assert {sum(live) % 4 for _, _, live in _all_lists() if sum(live)} == {0, 1, 2, 3}
    assert {t % 4 for t in T.TOTALS if t} == {0, 1, 2, 3}


def test_groups_against_the_shard_borders():
    spans, border_starts, empties = set(), 0, 0
    for total, split, live in _all_lists():
        for t, g in enumerate(_groups(live)):
            spans.add(len({s for s, _ in g}))
            border_starts += t > 0 and g[0][1] == 0  # a later group that starts exactly where a shard starts
        empties += any(live[s] == 0 and any(live[s + 1:]) for s in range(T.SHARDS))   # an empty shard in front of entries
    assert {2, 3} <= spans, spans                    # a group of four over two shards, and over three
    assert border_starts > 0 and empties > 0
    # the clamped shard is followed by a non-empty one
    for total in T.TOTALS:
        if total:
            live = T.live_counts(T.shard_counts(total, "clamped"))
            assert live[2] == T.CAP and live[3] > 0
    # every total that is no multiple of 4 or 16 is there, and 0
    assert 0 in T.TOTALS and any(t % 16 == 0 and t for t in T.TOTALS) and any(t % 4 == 0 and t % 16 for t in T.TOTALS)


def test_shapes_of_the_lists():
    assert T.PATH_SHAPES == ((1, 1), (2, 1), (1, 2), (2, 2))
    assert set(T.GEN_SHAPES) == {(1, 1), (3, 1), (1, 3), (2, 4), (4, 4), (3, 2)}
    for shard in range(T.SHARDS):
        for k in range(T.CAP - 1):
            assert T.entry_shape(4, shard, k) != T.entry_shape(4, shard, k + 1)      # consecutive entries differ in (na, nb)
        for path in range(4):
            assert T.entry_shape(path, shard, 5) == T.PATH_SHAPES[path]
    # one wave of the predicated list holds namax = 4 beside a row of na = 1 (and nbmax = 4 beside nb = 1), in every group of some list
    mixed_a = mixed_b = 0
    for total, split, live in _all_lists():
        for g in _groups(live):
            na = [T.entry_shape(4, s, k)[0] for s, k in g]
            nb = [T.entry_shape(4, s, k)[1] for s, k in g]
            mixed_a += max(na) == 4 and min(na) == 1
            mixed_b += max(nb) == 4 and min(nb) == 1
            if len(g) == 4:
                assert len({T.entry_shape(4, s, k) for s, k in g}) >= 2
    assert mixed_a > 0 and mixed_b > 0


def test_no_wave_meets_the_same_pair_twice():
    """The sums of a stale pair (an entry or rows not rotated between turns) or of a neighbouring row must not pass for the right ones: within a path, the
    four pairs of a group are different (shape, SNP of the pool, SNP of the pool), and so are the pairs a row of a wave takes in consecutive turns within
    a shard; from one shard to another they may meet again, rarely."""
    def ident(path, s, k):
        return T.entry_shape(path, s, k) + T.entry_snps(path * T.SHARDS + s, k)

    checked = across = same_across = 0
    for total, split, live in _all_lists():
        groups = _groups(live)
        for path in range(T.PATHS):
            for g in groups:
                assert len({ident(path, s, k) for s, k in g}) == len(g), (total, split, path, g)
            for grid in T.GRIDS:
                if not grid:
                    continue
                for turns in T.wave_turns(sum(live), grid).values():
                    for t0, t1 in zip(turns, turns[1:]):
                        for (s0, k0), (s1, k1) in zip(groups[t0], groups[t1]):       # the same row of the wave, one turn apart
                            checked += 1
                            if s0 == s1:
                                assert ident(path, s0, k0) != ident(path, s1, k1), (total, split, path, grid, (s0, k0), (s1, k1))
                            else:                    # 49 pairs of a shape over 8 x 80 slots: from one shard to another a few must meet again
                                across += 1
                                same_across += ident(path, s0, k0) == ident(path, s1, k1)
    assert checked > 10000 and across > 1000 and same_across < 0.03 * across, (checked, across, same_across)


def test_sequence_counts_sit_at_the_word_edges():
    for N, words in T.SEQ_WORDS.items():
        assert T.words_of(N) == words
    assert [busy for busy in (T.busy_tail_lanes(T.SEQ_WORDS[N], 0) for N in (33, 1000, 5000))] == [[], [], []]     # no tail up to 160 words
    assert [l for l in range(16) if 2 * l < T.SEQ_WORDS[33]] == [0, 1]                                            # 33: two busy lanes
    assert T.SEQ_WORDS[1000] == 32 and T.SEQ_WORDS[5000] == 32 * T.REG_STEPS                                       # one step; all five, exactly
    assert T.busy_tail_lanes(T.SEQ_WORDS[5121], 0) == [0, 1] and T.busy_tail_lanes(T.SEQ_WORDS[5121], 1) == []     # the first tail step, two lanes
    assert T.busy_tail_lanes(T.SEQ_WORDS[6200], 0) == list(range(16)) and T.busy_tail_lanes(T.SEQ_WORDS[6200], 1) == [0, 1]
    assert T.SEQ_WORDS[6200] > 192                                                                                 # and past the 3 x 64 words k_pair_sums keeps
    assert {N for _, N in T.CASES} == set(T.SEQ_WORDS)
    kinds = {k for k, _ in T.CASES}
    assert kinds == {"hamming", "hand", "hand tail", "ones32", "distinct"} and ("hand tail", 6200) in T.CASES

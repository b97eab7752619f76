"""A plain model of what the FUSED approximate GEMM does with the values it accumulates (no GPU): the live-tile pass k_apx_live_tiles and the table test
of apx_gemm_epilogue, written from their contract — ApxGemmArgs in csrc/ldw_apx.h, the comment above k_apx_live_tiles, BOUNDS.md 5 and 6 — tile by tile and
region by region with loops over rows and columns.  Nothing here knows which lane of a wave holds which entry.

  tile (ty, tx)    128 to-rows x 64 from-rows; valid unless lower_only and tx * 64 + 63 < ty * 128; masked when sr_mask[ty][tx] != 0
  region           32 to-rows x 64 from-rows: four per tile, flag clean[(32-row group)][tx]
  pruning          only with prune, only valid unmasked tiles.  Rule (b), with row flags: the 128 to-rows share one kind in {2, 3}, the 64 from-rows too, and
                   every to-row is dead versus the from kind or every from-row dead versus the to kind.  Rule (a): every row of both sides binned, the bin
                   rectangle holds at most 64 entries, all of them (< 0, INT_MAX).  A pruned tile with every row binned writes flag 1 four times, another
                   pruned tile writes nothing; nothing of a pruned or invalid tile is computed
  live tile        every region's flag is written: eligible (no 255 among its 32 + 64 bins, tile not masked) and no entry fails Lq < acc < Hq -> 1, not
                   stored; eligible, fails, a maybe list and at most `maybe_max` of them -> 1, not stored, the fails listed with n = acc; else 0, stored
"""
import numpy as np

INT_MAX = 2147483647
PF_KIND, PF_DEAD2, PF_DEAD3 = 3, 4, 8
UNWRITTEN = -1          # in Expect.clean: the flag no kernel writes


def padded(nrt, nrf, bin_t, bin_f, rflag_t=None, rflag_f=None):
    """The hook's padding of the per-row inputs to RTpad / RFpad rows: bin 255 and flag 0."""
    RTpad, RFpad = -(-nrt // 128) * 128, -(-nrf // 128) * 128
    bt = np.full(RTpad, 255, dtype=np.int64)
    bf = np.full(RFpad, 255, dtype=np.int64)
    bt[:nrt], bf[:nrf] = bin_t, bin_f
    ft = ff = None
    if rflag_t is not None:
        ft, ff = np.zeros(RTpad, dtype=np.int64), np.zeros(RFpad, dtype=np.int64)
        ft[:nrt], ff[:nrf] = rflag_t, rflag_f
    return bt, bf, ft, ff


class Expect:
    """clean [RTpad / 32][RFpad / 64]: 0, 1 or UNWRITTEN; stored: bool per region; live: set of (ty, tx); pruned: tiles the live-tile pass counts;
    pruned_b: those of them that rule (b) took; maybe: sorted list of (trow, fcol, n); maybe_n; fails: {(region row, tx): [(trow, fcol)]} of the eligible regions."""


def prune_rule(bt, bf, ft, ff, tab):
    """Which rule prunes a valid, unmasked tile with these 128 to-bins, 64 from-bins and (or None) flags: None, ("a", all_binned) or
    ("b", all_binned, kt, kf, to side dead, from side dead)."""
    all_binned = all(b < 64 for b in bt) and all(b < 64 for b in bf)
    if ft is not None:
        kinds_t, kinds_f = {int(f) & PF_KIND for f in ft}, {int(f) & PF_KIND for f in ff}
        if len(kinds_t) == 1 and len(kinds_f) == 1 and min(kinds_t) in (2, 3) and min(kinds_f) in (2, 3):
            kt, kf = min(kinds_t), min(kinds_f)
            dead_vs = {2: PF_DEAD2, 3: PF_DEAD3}
            to_dead, from_dead = all(int(f) & dead_vs[kf] for f in ft), all(int(f) & dead_vs[kt] for f in ff)
            if to_dead or from_dead:
                return ("b", all_binned, kt, kf, to_dead, from_dead)
    if all_binned:
        t0, t1, f0, f1 = int(min(bt)), int(max(bt)), int(min(bf)), int(max(bf))
        if (t1 - t0 + 1) * (f1 - f0 + 1) <= 64 and all(tab[a][b][0] < 0 and tab[a][b][1] == INT_MAX for a in range(t0, t1 + 1) for b in range(f0, f1 + 1)):
            return ("a", True)
    return None


def model(acc, bin_t, bin_f, tab, rflag_t=None, rflag_f=None, sr_mask=None, lower_only=False, prune=False, maybe=True, maybe_max=96):
    """acc [RTpad][RFpad]: the accumulators; bin_t / bin_f / rflag_t / rflag_f: per padded row (see padded()); tab [64][64][2]."""
    RTpad, RFpad = acc.shape
    assert RTpad % 128 == 0 and RFpad % 128 == 0 and len(bin_t) == RTpad and len(bin_f) == RFpad
    nty, ntx = RTpad // 128, RFpad // 64
    acc, tab = np.asarray(acc, dtype=np.int64), np.asarray(tab, dtype=np.int64)
    bin_t, bin_f = np.asarray(bin_t, dtype=np.int64), np.asarray(bin_f, dtype=np.int64)
    E = Expect()
    E.clean = np.full((RTpad // 32, ntx), UNWRITTEN, dtype=np.int64)
    E.stored = np.zeros((RTpad // 32, ntx), dtype=bool)
    E.live, E.pruned, E.pruned_b, E.maybe, E.maybe_n, E.fails = set(), 0, 0, [], 0, {}
    E.rule, E.detail = {}, {}         # (ty, tx) -> "invalid", "a", "b", "live"; what prune_rule said of a pruned tile
    for ty in range(nty):
        for tx in range(ntx):
            if lower_only and tx * 64 + 63 < ty * 128:
                E.rule[ty, tx] = "invalid"
                continue
            masked = sr_mask is not None and sr_mask[ty][tx] != 0
            bt, bf = bin_t[ty * 128:ty * 128 + 128], bin_f[tx * 64:tx * 64 + 64]
            if prune and not masked:
                ft = None if rflag_t is None else rflag_t[ty * 128:ty * 128 + 128]
                ff = None if rflag_t is None else rflag_f[tx * 64:tx * 64 + 64]
                why = prune_rule(bt, bf, ft, ff, tab)
                if why is not None:
                    E.pruned += 1
                    E.pruned_b += why[0] == "b"
                    E.rule[ty, tx] = why[0]
                    E.detail[ty, tx] = why
                    if why[1]:       # every row binned: the four regions are flagged clean
                        for i in range(4):
                            E.clean[ty * 4 + i][tx] = 1
                    continue
            E.live.add((ty, tx))
            E.rule[ty, tx] = "live"
            for i in range(4):
                g = ty * 4 + i
                r0, c0 = ty * 128 + 32 * i, tx * 64
                rows, cols = slice(r0, r0 + 32), slice(c0, c0 + 64)
                eligible = not masked and all(bin_t[rows] != 255) and all(bin_f[cols] != 255)
                clean = False
                if eligible:
                    entry = tab[bin_t[rows]][:, bin_f[cols]]                    # [32][64][2]: every pair's own (Lq, Hq)
                    a = acc[rows, cols]
                    passes = (entry[:, :, 0] < a) & (a < entry[:, :, 1])         # strict on both sides
                    fails = [(r0 + int(r), c0 + int(c)) for r, c in zip(*np.nonzero(~passes))]
                    E.fails[g, tx] = fails
                    if not fails:
                        clean = True
                    elif maybe and len(fails) <= maybe_max:
                        clean = True
                        E.maybe += [(r, c, int(acc[r][c])) for r, c in fails]
                        E.maybe_n += len(fails)
                E.clean[g][tx] = 1 if clean else 0
                E.stored[g][tx] = not clean
    E.maybe.sort()
    return E


def stored_entries(E, shape):
    """bool [RTpad][RFpad]: the entries of G the launches write."""
    return np.kron(E.stored.astype(np.uint8), np.ones((32, 64), dtype=np.uint8)).astype(bool).reshape(shape)

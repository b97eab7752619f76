"""The cases of tests/test_apx_fused_gpu.py, made by ONE function from an accumulator source, and the situations they must hold (no GPU).

make_cases(n_rows, acc_of, seed) draws the row lists of every shape, asks acc_of(rows_t, rows_f) for the accumulators of that launch — on the CPU the exact
co-occurrence counts of unit weights, on the GPU the kernel's own no-table launch — and lays bins, flags, table, mask and list capacity over them.  Fail
counts do not depend on the data: rows of bin 1 x columns of bin 1 meet an entry nothing passes (NEVER1), the one row and the one column of bin 2 a second
one (NEVER2), every other entry touched passes everything; |A| |B| (+ 1) entries of a region fail.  Only the entry [3][3] is fitted to the values present.
situations(case) names what a case holds, by the model alone; REQUIRED lists what the whole table must hold (tests/test_apx_fused_cases_host.py)."""
import numpy as np

import apx_fused_ref as REF
from ldweaver_amd.engine import Engine

NRT, NRF = (100, 128, 129, 384, 512), (40, 64, 65, 192, 256)
MAYBE_MAX = Engine.APX_MAYBE_MAX
INT_MAX = REF.INT_MAX
UNC, NEVER1, NEVER2 = (-1, INT_MAX), (INT_MAX, INT_MAX), (0, 0)
BIG_CAP = 8192          # >= 64 regions x MAYBE_MAX: never the limit

# per 32-row group of the to side / per 64-column block of the from side (epilogue scenarios)
GROUPS = ("none", "one2", "a12", "a12+2", "all1", "x255lo", "x255hi", "val3", "one2")
BLOCKS = ("b8+2", "none", "all1", "val3", "x255a", "b8+2", "x255b")
# rule (a): bin ranges per 128-row band / 64-column block
BANDS_A = {"t8": (10, 17), "t5": (10, 14), "t8c": (30, 37), "t1": (12, 12)}
BLOCKS_A = {"f8": (20, 27), "f13": (20, 32), "f8c": (40, 47), "f1": (22, 22)}
# rule (b): (kind, flag bits of every row, the odd row's flag or None) per band / block
SIDES_B = ((2, 2 | 4, None), (2, 2 | 8, None), (3, 3 | 4, None), (3, 3 | 8, None), (2, 2, None), (3, 3 | 4 | 8, None), (2, 2 | 4 | 8, 3 | 4 | 8), (3, 3 | 4 | 8, 3),
           (2, 2 | 4 | 8, None), (3, 3, None), (2, 2 | 4 | 8, 2))


def _spread(rng, n, lo, hi):
    """n bins covering lo..hi, both ends present."""
    b = rng.integers(lo, hi + 1, n)
    if n >= 2:
        i, j = rng.choice(n, 2, replace=False)
        b[i], b[j] = lo, hi
    return b


def _epi_bins(rng, k, nrt, nrf, acc):
    bt, bf = np.zeros(nrt, dtype=np.int64), np.zeros(nrf, dtype=np.int64)
    for g in range(-(-nrt // 32)):
        n = min(32, nrt - 32 * g)
        what = GROUPS[(g + k) % len(GROUPS)]
        pos = rng.permutation(n)
        b = np.zeros(n, dtype=np.int64)
        if what in ("a12", "a12+2", "x255lo", "x255hi"):
            b[pos[:12]] = 1
        if what == "all1":
            b[:] = 1
        if what in ("one2", "a12+2") and n > 12:
            b[pos[12]] = 2
        if what == "val3" and n > 13:
            # the row of bin 3: the one of the group's rows without another role that meets the most values in the columns of bin 3 (x3, below)
            x3 = [x for x in range(nrf // 64) if BLOCKS[(x + 2 * k) % len(BLOCKS)] == "val3"]
            variety = [len(set(acc[32 * g + o, 64 * x3[0]:64 * x3[0] + 64])) if x3 else 0 for o in pos[13:]]
            b[pos[13 + int(np.argmax(variety))]] = 3
        if what in ("x255lo", "x255hi"):
            half = what == "x255hi"
            b[([o for o in pos if (o % 8 >= 4) == half] + [pos[-1]])[0]] = 255
        bt[32 * g:32 * g + n] = b
    for x in range(-(-nrf // 64)):
        n = min(64, nrf - 64 * x)
        what = BLOCKS[(x + 2 * k) % len(BLOCKS)]
        pos = rng.permutation(n)
        b = np.zeros(n, dtype=np.int64)
        if what in ("b8+2", "x255a", "x255b"):
            b[pos[:8]] = 1
            if n > 8:
                b[pos[8]] = 2
        if what == "all1":
            b[:] = 1
        if what == "val3":
            b[:] = 3
        if what in ("x255a", "x255b"):
            half = what == "x255b"
            b[[o for o in pos if (o >= 32) == half][0] if n == 64 else pos[-1]] = 255
        bf[64 * x:64 * x + n] = b
    return bt, bf


def _fit_entry33(acc, bt, bf):
    """(Lq, Hq) for the pairs of bin 3 x bin 3, from the values of the first region that holds some: Lq and Hq are values present there (both fail), a
    present value between them passes — Lq + 1 and Hq - 1 themselves where the region holds them."""
    for g in range(len(bt) // 32):
        rows = [r for r in range(32 * g, 32 * g + 32) if bt[r] == 3]
        for x in range(len(bf) // 64):
            cols = [c for c in range(64 * x, 64 * x + 64) if bf[c] == 3]
            if not rows or not cols or 255 in bt[32 * g:32 * g + 32] or 255 in bf[64 * x:64 * x + 64]:
                continue
            d = sorted({int(v) for v in acc[np.ix_(rows, cols)].ravel()})
            if len(d) < 3:
                continue
            lq = next((v for v in d[:-2] if v + 1 in d), d[0])
            hq = next((v for v in reversed(d) if v - 1 in d and v - 1 > lq), d[-1])
            if hq - 1 == lq or hq <= lq:
                hq = d[-1]
            return lq, hq
    return UNC


def _case(name, shape, rows, acc, bt, bf, tab, ft=None, ff=None, mask=None, lower_only=False, maybe_cap=BIG_CAP):
    nrt, nrf = shape
    c = dict(name=name, nrt=nrt, nrf=nrf, rows_t=rows[0], rows_f=rows[1], acc=acc, bin_t=bt.astype(np.uint8), bin_f=bf.astype(np.uint8),
             rflag_t=None if ft is None else ft.astype(np.uint8), rflag_f=None if ff is None else ff.astype(np.uint8), tab=tab.astype(np.int32), sr_mask=mask,
             lower_only=lower_only, maybe_cap=maybe_cap)
    c["pad"] = REF.padded(nrt, nrf, c["bin_t"], c["bin_f"], c["rflag_t"], c["rflag_f"])
    c["expect"] = {}
    return c


def expect(c, prune, mask=True):
    """The model's expectation of the case with or without the live-tile pass (kept with the case: it does not depend on the launch form)."""
    key = (bool(prune), mask)
    if key not in c["expect"]:
        pbt, pbf, pft, pff = c["pad"]
        c["expect"][key] = REF.model(c["acc"], pbt, pbf, c["tab"], pft if prune else None, pff if prune else None, c["sr_mask"] if mask else None, c["lower_only"], prune,
                                     maybe=c["maybe_cap"] > 0, maybe_max=MAYBE_MAX)
    return c["expect"][key]


def make_cases(n_rows, acc_of, seed):
    """n_rows: indicator rows 0..n_rows-1 to draw from (with replacement); acc_of(rows_t, rows_f) -> int [nrt][nrf].  Returns the list of cases."""
    rng = np.random.default_rng(seed)
    cases = []
    for it, nrt in enumerate(NRT):
        for jf, nrf in enumerate(NRF):
            k, shape = it * len(NRF) + jf, (nrt, nrf)
            RTpad, RFpad = -(-nrt // 128) * 128, -(-nrf // 128) * 128
            nty, ntx = RTpad // 128, RFpad // 64
            rows = (rng.integers(0, n_rows, nrt).astype(np.int32), rng.integers(0, n_rows, nrf).astype(np.int32))
            acc = np.zeros((RTpad, RFpad), dtype=np.int64)      # (the padding rows hold no sequence)
            acc[:nrt, :nrf] = acc_of(*rows)
            # -- the epilogue's regions: the product construction, one value-fitted entry, a masked tile
            bt, bf = _epi_bins(rng, k, nrt, nrf, acc)
            tab = np.empty((64, 64, 2), dtype=np.int64)
            tab[:, :] = UNC
            tab[1, 1], tab[2, 2] = NEVER1, NEVER2
            pbt, pbf, _, _ = REF.padded(nrt, nrf, bt, bf)
            tab[3, 3] = _fit_entry33(acc, pbt, pbf)
            mask = None
            if nty * ntx >= 2 and k % 2 == 0:
                mask = np.zeros((nty, ntx), dtype=np.uint8)
                quiet = [x for x in range(nrf // 64) if BLOCKS[(x + 2 * k) % len(BLOCKS)] == "none"]      # a column block without a failing entry
                mask[(k // 2) % nty, quiet[0] if quiet else (k // 2) % ntx] = 1 + k % 3
            epi = _case("epi", shape, rows, acc, bt, bf, tab, mask=mask)
            cases.append(epi)
            cases.append(_case("epi_nomaybe", shape, rows, acc, bt, bf, tab, mask=mask, maybe_cap=-1))
            total = expect(epi, False).maybe_n
            if total >= 2:
                cases.append(_case("epi_cap", shape, rows, acc, bt, bf, tab, mask=mask, maybe_cap=max(1, total // 3)))
            if nty >= 2:
                cases.append(_case("epi_lower", shape, rows, acc, bt, bf, tab, lower_only=True))
            # -- rule (a): bin rectangles of 64 and 65 entries, a corner entry that is not unconditional
            bt, bf = np.zeros(nrt, dtype=np.int64), np.zeros(nrf, dtype=np.int64)
            for y in range(nty):
                n = min(128, nrt - 128 * y)
                bt[128 * y:128 * y + n] = _spread(rng, n, *BANDS_A[list(BANDS_A)[(y + jf) % 4]])
            for x in range(-(-nrf // 64)):
                n = min(64, nrf - 64 * x)
                bf[64 * x:64 * x + n] = _spread(rng, n, *BLOCKS_A[list(BLOCKS_A)[(x + it) % 4]])
            tab = np.empty((64, 64, 2), dtype=np.int64)
            tab[:, :] = UNC
            tab[5, 40:48] = (-7, INT_MAX)                       # (any negative Lq is unconditional)
            tab[37, 47] = (-1, INT_MAX - 1) if k % 2 else (0, INT_MAX)
            cases.append(_case("rule_a", shape, rows, acc, bt, bf, tab, lower_only=bool(nty >= 2 and jf % 2)))
            # -- rule (b): kinds and dead bits per band and block; kind 2 rows are binned, kind 3 rows are not
            ft, ff = np.zeros(nrt, dtype=np.int64), np.zeros(nrf, dtype=np.int64)
            for flags, n_all, width, a, b, d in ((ft, nrt, 128, 1, 2, 4), (ff, nrf, 64, 2, 4, 0)):      # (coefficients that spread the eleven recipes over the shapes)
                for y in range(-(-n_all // width)):
                    n = min(width, n_all - width * y)
                    kind, flag, odd = SIDES_B[(a * y + b * jf + d * it) % len(SIDES_B)]
                    flags[width * y:width * y + n] = flag
                    if odd is not None:
                        flags[width * y + int(rng.integers(n))] = odd
            bt = np.where((ft & 3) == 2, rng.integers(0, 3, nrt), 255)
            bf = np.where((ff & 3) == 2, rng.integers(0, 3, nrf), 255)
            tab = np.empty((64, 64, 2), dtype=np.int64)
            tab[:, :] = UNC
            tab[1, 1], tab[2, 2] = NEVER1, NEVER2
            cases.append(_case("rule_b", shape, rows, acc, bt, bf, tab, ft=ft, ff=ff))
            # -- one bin, an unconditional table: every tile without a padding row is pruned
            tab = np.empty((64, 64, 2), dtype=np.int64)
            tab[:, :] = UNC
            cases.append(_case("flat", shape, rows, acc, np.full(nrt, 5), np.full(nrf, 5), tab))
    return cases


# ------------------------------------------------------------------------------------------------
# what a case holds
# ------------------------------------------------------------------------------------------------
REQUIRED = (
    # regions
    "0 fails, list on", "1 fail, list on", "96 fails, list on: listed", "97 fails, list on: stored", "2048 fails, list on", "96 fails, list off: stored",
    "97 fails, list off: stored", "a listed fail in a row of lane half 0", "a listed fail in a row of lane half 1", "a listed fail in columns 0..31",
    "a listed fail in columns 32..63", "Lq equals a present value", "Hq equals a present value", "a present value between Lq and Hq passes", "Lq + 1 present and passes",
    "Hq - 1 present and passes", "a single 255 in a to-row of lane half 0", "a single 255 in a to-row of lane half 1", "a single 255 in columns 0..31",
    "a single 255 in columns 32..63", "ineligible by padding rows alone", "a masked tile whose regions would be clean", "a clean region in an unmasked neighbour",
    "capacity below the total", "live tiles for runs of two to four", "the bands of a run differ in bins and outcome",
    # tiles
    "rectangle of 64 pruned", "rectangle of 65 (5 x 13) computed", "rectangle with one conditional corner computed", "b(2,2) dead to side", "b(2,2) dead from side",
    "b(2,3) dead to side", "b(2,3) dead from side", "b(3,2) dead to side", "b(3,2) dead from side", "b(3,3) dead to side", "b(3,3) dead from side",
    "near miss of b: one row of the other kind", "near miss of b: one row not dead", "near miss of b: a padding row", "b-pruned, unbinned: no flag", "b-pruned, binned: flags 1",
    "lower_only: a tile above the diagonal left alone", "lower_only: a straddling tile computed", "every tile pruned", "no tile pruned",
)


def situations(c):
    """The names of REQUIRED this case holds, judged by the model."""
    S = set()
    nrt, nrf, cap = c["nrt"], c["nrf"], c["maybe_cap"]
    pbt, pbf, pft, pff = c["pad"]
    tab, acc = c["tab"], c["acc"]
    nty, ntx = len(pbt) // 128, len(pbf) // 64
    E0, E1 = expect(c, False), expect(c, True)
    on = "on" if cap > 0 else "off"
    for (g, x), fails in E0.fails.items():
        n = len(fails)
        listed = cap > 0 and 0 < n <= MAYBE_MAX
        assert E0.stored[g][x] == (n > 0 and not listed) and E0.clean[g][x] == (0 if E0.stored[g][x] else 1)
        if n in (0, 1, 2048) and cap > 0:
            S.add(f"{n} fail{'' if n == 1 else 's'}, list {on}")
        if n in (96, 97):
            S.add(f"{n} fails, list {on}: {'listed' if listed else 'stored'}")
        if listed:
            for r, col in fails:
                S.add(f"a listed fail in a row of lane half {int(r % 8 >= 4)}")
                S.add("a listed fail in columns 32..63" if col % 64 >= 32 else "a listed fail in columns 0..31")
        rows3 = [r for r in range(32 * g, 32 * g + 32) if pbt[r] == 3]
        cols3 = [q for q in range(64 * x, 64 * x + 64) if pbf[q] == 3]
        if rows3 and cols3 and tuple(tab[3, 3]) != UNC:
            lq, hq = (int(v) for v in tab[3, 3])
            V = {int(v) for v in acc[np.ix_(rows3, cols3)].ravel()}
            failing = {int(acc[r][q]) for r, q in fails if pbt[r] == 3 and pbf[q] == 3}
            if lq in V and lq in failing:
                S.add("Lq equals a present value")
            if hq in V and hq in failing:
                S.add("Hq equals a present value")
            if any(lq < v < hq for v in V):
                S.add("a present value between Lq and Hq passes")
            if lq + 1 in V and lq + 1 < hq and lq + 1 not in failing:
                S.add("Lq + 1 present and passes")
            if hq - 1 in V and hq - 1 > lq and hq - 1 not in failing:
                S.add("Hq - 1 present and passes")
    masked = (lambda y, x: c["sr_mask"] is not None and c["sr_mask"][y][x] != 0)
    for (y, x) in E0.live:
        for i in range(4):
            g = 4 * y + i
            if masked(y, x):
                continue
            t255 = [r for r in range(32 * g, 32 * g + 32) if pbt[r] == 255]
            f255 = [q for q in range(64 * x, 64 * x + 64) if pbf[q] == 255]
            if len(t255) + len(f255) == 1:
                assert E0.clean[g][x] == 0 and E0.stored[g][x]
                if t255:
                    S.add(f"a single 255 in a to-row of lane half {int(t255[0] % 8 >= 4)}")
                else:
                    S.add("a single 255 in columns 32..63" if f255[0] % 64 >= 32 else "a single 255 in columns 0..31")
            if t255 and not f255 and min(t255) >= nrt and 32 * g < nrt:
                S.add("ineligible by padding rows alone")
    if c["sr_mask"] is not None:
        free = expect(c, False, mask=False)
        for y in range(nty):
            for x in range(ntx):
                if masked(y, x) and all(free.clean[4 * y + i][x] == 1 for i in range(4)):
                    assert all(E0.clean[4 * y + i][x] == 0 and E0.stored[4 * y + i][x] for i in range(4))
                    S.add("a masked tile whose regions would be clean")
                    for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                        if 0 <= yy < nty and 0 <= xx < ntx and not masked(yy, xx) and any(E0.clean[4 * yy + i][xx] == 1 for i in range(4)):
                            S.add("a clean region in an unmasked neighbour")
    if 0 < cap < E0.maybe_n:
        S.add("capacity below the total")
    # tiles
    if 9 <= len(E1.live) <= 16:
        S.add("live tiles for runs of two to four")
        bands = [tuple(pbt[128 * y:128 * y + 128]) for y in range(nty)]
        outcome = [tuple(E1.clean[4 * y:4 * y + 4].ravel()) for y in range(nty)]
        if len(set(bands)) == nty and len(set(outcome)) == nty:
            S.add("the bands of a run differ in bins and outcome")
    for y in range(nty):
        for x in range(ntx):
            rule = E1.rule[y, x]
            bt, bf = pbt[128 * y:128 * y + 128], pbf[64 * x:64 * x + 64]
            region_flags = [int(E1.clean[4 * y + i][x]) for i in range(4)]
            if rule == "invalid":
                assert region_flags == [REF.UNWRITTEN] * 4 and not any(E1.stored[4 * y + i][x] for i in range(4)) and (y, x) not in E1.live
                S.add("lower_only: a tile above the diagonal left alone")
                continue
            if c["lower_only"] and rule == "live" and x * 64 < y * 128 + 127 and x * 64 + 63 >= y * 128:
                S.add("lower_only: a straddling tile computed")
            if masked(y, x):
                continue
            binned = all(b < 64 for b in bt) and all(b < 64 for b in bf)
            if binned:
                t0, t1, f0, f1 = int(min(bt)), int(max(bt)), int(min(bf)), int(max(bf))
                area = (t1 - t0 + 1) * (f1 - f0 + 1)
                cond = [(a, b) for a in range(t0, t1 + 1) for b in range(f0, f1 + 1) if not (tab[a][b][0] < 0 and tab[a][b][1] == INT_MAX)]
                if rule == "a" and area == 64:
                    S.add("rectangle of 64 pruned")
                if rule == "live" and pft is None and area == 65 and (t1 - t0 + 1, f1 - f0 + 1) == (5, 13) and not cond:
                    S.add("rectangle of 65 (5 x 13) computed")
                if rule == "live" and pft is None and area <= 64 and len(cond) == 1 and cond[0][0] in (t0, t1) and cond[0][1] in (f0, f1):
                    S.add("rectangle with one conditional corner computed")
            if rule == "b":
                _, all_binned, kt, kf, to_dead, from_dead = E1.detail[y, x]
                if to_dead != from_dead:
                    S.add(f"b({kt},{kf}) dead {'to' if to_dead else 'from'} side")
                if all_binned:
                    assert region_flags == [1] * 4
                    S.add("b-pruned, binned: flags 1")
                else:
                    assert region_flags == [REF.UNWRITTEN] * 4
                    S.add("b-pruned, unbinned: no flag")
            if rule == "live" and pft is not None and REF.prune_rule(bt, bf, None, None, tab) is None:
                ft, ff = pft[128 * y:128 * y + 128].copy(), pff[64 * x:64 * x + 64].copy()
                for side, n_real, base in ((ft, nrt, 128 * y), (ff, nrf, 64 * x)):
                    vals, counts = np.unique(side, return_counts=True)
                    if len(vals) != 2 or counts.min() != 1 and not (vals[0] == 0 and base + len(side) > n_real):
                        continue
                    odd, rest = (vals[0], vals[1]) if counts[0] <= counts[1] else (vals[1], vals[0])
                    if vals[0] == 0 and base + len(side) > n_real:
                        odd, rest = 0, vals[1]
                    mended = np.where(side == odd, rest, side)
                    why = REF.prune_rule(bt, bf, mended if side is ft else ft, mended if side is ff else ff, tab)
                    if why is None or why[0] != "b":
                        continue
                    if odd == 0:
                        S.add("near miss of b: a padding row")
                    elif (odd & 3) != (rest & 3):
                        S.add("near miss of b: one row of the other kind")
                    else:
                        S.add("near miss of b: one row not dead")
    tiles_valid = sum(1 for r in E1.rule.values() if r != "invalid")
    if tiles_valid and not E1.live:
        assert E1.pruned == tiles_valid
        S.add("every tile pruned")
    if len(E1.live) >= 2 and E1.pruned == 0:
        S.add("no tile pruned")
    return S

"""GPU: the exact co-occurrence GEMMs as functions (ldw_debug_limb_gemm, ldw_debug_lo_units), against plain integer sums, at K and tile edges (pytest -m gpu).

Every MI the engine emits is computed from the exact joint sums of gemm_bits_kernel<J> (block-wide, every launch form), gemm_lo_units_kernel (the gathered
low limbs of the mixed path; the same K loop, ldw_gemm_kloop.inc) or k_cooc_popc (the popcount engine).  Here the hooks run the launch code of the product
on caller-chosen indicator rows and caller-made unit lists, into buffers pre-filled with a pattern, and EVERY stored integer is compared with == :

  want[t][f] = sum over the sequences s of V_part(s) bits[t][s] bits[f][s],   V_part = sum_j d_(limb0 + j) 256^j

with the bit rows rebuilt from the states and debug_rows, V from debug_apx_params (checked against rint(ldexp(sqrt(w)^2, F))) and the balanced base-256 digits d
made here by the rule of ldw_set_weights.  An entry the launch must leave alone must still hold the fill.  There is no tolerance anywhere.

Sequence counts (the K loop stages 1024 sequences = 16 words per LDS chunk in two buffers; k_cooc_popc stages 32 words of 32 bits):
  100    KW 2: one macro step          1000  KW 16: exactly one chunk          1100  KW 18: a second chunk of one macro step
  2048   KW 32: two full chunks        2200  KW 36: three chunks, buffer 0 reused, the last one partial            (32-bit words: 4, 32, 35, 64, 69)
Weights: unit (one limb, F = 0); five distinct values whose classes end inside 32-bit words and span whole ones; uniform(1/64, 1) with w[0] = 1 and two
planted weights whose digits are 127 / -128 in every limb below the top one, for 2..6 limbs (six limbs run as 3 + 3 with a shift and an accumulate).

The sensitivity controls recompute the reference with one deliberate error each (the sequences of the last partial chunk dropped, the top limb dropped, the
carry of a -128 digit dropped, lower_only one tile off, the 33rd chunk of a tile dropped) and assert that it differs from what the kernel stored: the inputs
would show each of these errors."""
import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

LS = 400
SEQ_KW = {100: 2, 1000: 16, 1100: 18, 2048: 32, 2200: 36}
SEQ_WORDS32 = {100: 4, 1000: 32, 1100: 35, 2048: 64, 2200: 69}
NRT, NRF = (100, 128, 129, 300), (40, 64, 65, 200)
REDUCED = ((129, 65), (300, 200))
FILL = Engine.LIMB_GEMM_FILL
FILL32 = Engine.LO_UNITS_FILL
PLANT_3ROWS, PLANT_4ROWS = range(10, 20), range(20, 30)      # SNPs made to hold 4 and 5 states

_ALN = {}


def test_the_sequence_counts_are_the_edges_of_both_k_loops():
    for N, kw in SEQ_KW.items():
        assert -(-N // 128) * 2 == kw and -(-N // 32) == SEQ_WORDS32[N]
    chunks = {N: -(-kw // 16) for N, kw in SEQ_KW.items()}
    assert chunks == {100: 1, 1000: 1, 1100: 2, 2048: 2, 2200: 3}
    assert SEQ_KW[1100] - 16 == 2 and 0 < SEQ_KW[2200] - 32 < 16      # a second chunk of ONE macro step; a partial third chunk
    assert sorted({(-(-a // 128), 2 * -(-b // 128)) for a in NRT for b in NRF}) == [(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 4)]


# ------------------------------------------------------------------------------------------------
# inputs and references
# ------------------------------------------------------------------------------------------------
def _aln(N):
    """400 SNPs x N sequences; SNPs 10..19 / 20..29 get every base / every base and the gap, so that 3 and 4 indicator rows occur at any N."""
    if N not in _ALN:
        syn = synth_alignment(LS, N, seed=4100 + N)
        st = np.array(syn["states"], dtype=np.uint8)
        for a in list(PLANT_3ROWS) + list(PLANT_4ROWS):
            k = 5 if a in PLANT_4ROWS else 4
            st[a] = np.where(st[a] == 4, st[a, 0], st[a])               # no gap unless planted
            for s in range(k):
                st[a, 1 + s + 7 * (a % 5): N - 1: 9 + s] = s            # state s in every (9 + s)-th sequence from there
        syn["states"] = st
        _ALN[N] = syn
    return _ALN[N]


def _digits(V, J):
    """The balanced base-256 digits of ldw_set_weights: d in [-128, 127], the remainder carried to the next limb."""
    d = np.zeros((J, len(V)), dtype=np.int64)
    rem = V.astype(np.int64).copy()
    for j in range(J):
        d[j] = ((rem + 128) & 255) - 128
        rem = (rem - d[j]) // 256
    assert np.all(rem == 0)
    return d


def _vpart(d, limb0, n):
    return sum(d[limb0 + j] * (1 << (8 * j)) for j in range(n))


def _gram(bits_f, vpart):
    """G[t][f] over ALL rows (the padding row R included), exact: float64 products of integers whose absolute sum is below 2^53."""
    assert float(np.abs(vpart).sum()) < 2.0 ** 53
    G = (bits_f * vpart.astype(np.float64)[None, :]) @ bits_f.T
    Gi = np.rint(G).astype(np.int64)
    assert np.array_equal(Gi.astype(np.float64), G)
    return Gi


class Ctx:
    """An alignment and a weighting loaded into the engine, with everything the references need."""

    def __init__(self, eng, N, w, J):
        syn = _aln(N)
        self.N, self.J, self.eng = N, J, eng
        st = syn["states"]
        eng.set_engine(L.ENGINE_MFMA)
        eng.set_alignment(st)
        uqe = (eng.state_counts() > 0).T.astype(np.float64)
        eng.set_weights(w, J)
        eng.set_snp_meta(uqe.sum(axis=1), uqe, syn["POS"], syn["paint"], float(syn["g"]))
        self.reload(w)
        row0, meta = eng.debug_rows()
        self.row0, self.nrows = row0.astype(np.int64), (meta & 7).astype(int)
        assert np.array_equal(self.nrows, np.diff(row0))
        self.R = R = int(row0[-1])
        assert R >= 300
        bits = np.zeros((R + 1, N), dtype=bool)
        for a in range(LS):
            m = int(meta[a])
            for i in range(m & 7):
                bits[int(row0[a]) + i] = st[a] == ((m >> (8 + 3 * i)) & 7)
        assert not bits[R].any() and bits[:R].any(axis=1).all()
        self.bits = bits.astype(np.float64)
        self._grams = {}

    def reload(self, w):
        """After (another) set_weights: F, V checked independently of the engine, and the digits."""
        par, V, _ = self.eng.debug_apx_params()
        P = dict(zip(Engine.APX_PARAM_NAMES, par))
        self.F = int(P["F"])
        assert int(P["nlimbs"]) == self.J
        assert np.array_equal(V, np.rint(np.ldexp(np.sqrt(w) ** 2, self.F)).astype(np.int64))
        self.V = V
        self.d = _digits(V, self.J)
        self._grams = {}

    def set_weights(self, w):
        self.eng.set_weights(w, self.J)
        self.reload(w)

    def vpart(self, limb0=0, n=None):
        return _vpart(self.d, limb0, self.J - limb0 if n is None else n)

    def gram(self, limb0=0, n=None):
        key = (limb0, self.J - limb0 if n is None else n)
        if key not in self._grams:
            self._grams[key] = _gram(self.bits, self.vpart(*key))
        return self._grams[key]

    def rows(self, rng, nrt, nrf):
        """Random rows, the padding row R as the last entry of both lists."""
        rt = np.append(rng.choice(self.R, nrt - 1, replace=False), self.R).astype(np.int32)
        rf = np.append(rng.choice(self.R, nrf - 1, replace=False), self.R).astype(np.int32)
        return rt, rf


def _unit(N):
    return np.ones(N)


def _five_values(N):
    """Five classes of 13, 70, 5, N - 95, 7 sequences (ascending weight = ascending position): the first ends inside word 0, the second covers word 1 whole
    and ends inside word 2, the third lies inside word 2, ...: segments with a partial mask and with the full one."""
    sizes = [13, 70, 5, N - 95, 7]
    assert min(sizes) >= 1
    w = np.repeat(np.array([0.0703125 + 2.0 ** -19, 0.31, 0.5 + 2.0 ** -20, 0.83, 1.0]), sizes)
    return np.random.default_rng(N).permutation(w), sizes


def _check_five_values(cx, sizes):
    vs = np.sort(cx.V)
    assert len(np.unique(vs)) == 5 and np.array_equal(np.diff(np.flatnonzero(np.diff(vs)), prepend=-1), sizes[:-1])
    nw = len(vs) // 32
    words = vs[: nw * 32].reshape(nw, 32)
    uniform = (words == words[:, :1]).all(axis=1)
    assert uniform.any() and not uniform.all()                       # both segment branches of k_cooc_popc


def _generic(eng, N, J, seed):
    """uniform(1/64, 1) with w[0] = 1, then two weights replaced by V_t 2^-F: one with digit 127, one with digit -128 in every limb below the top one."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(1.0 / 64, 1.0, N)
    w[0] = 1.0
    cx = Ctx(eng, N, w, J)
    F = cx.F
    top = (1 << F) >> (8 * (J - 1))                                   # 2^F in units of the top limb
    assert top >= 2
    dA = max(1, top // 2)
    low = sum(1 << (8 * j) for j in range(J - 1))
    VA, VB = dA * (1 << (8 * (J - 1))) + 127 * low, (dA + 1) * (1 << (8 * (J - 1))) - 128 * low
    assert 0 < VA <= 1 << F and 0 < VB <= 1 << F
    pa, pb = N // 3, (2 * N) // 3
    w[pa], w[pb] = np.ldexp(float(VA), -F), np.ldexp(float(VB), -F)
    cx.set_weights(w)
    assert cx.F == F and cx.V[pa] == VA and cx.V[pb] == VB, (F, cx.F)
    for j in range(J - 1):
        assert cx.d[j].min() == -128 and cx.d[j].max() == 127, (j, cx.d[j].min(), cx.d[j].max())
    assert np.all(cx.d[:J - 1, pa] == 127) and np.all(cx.d[:J - 1, pb] == -128)
    return cx


def _tile_of(nrt, nrf, th=128, tw=64):
    by = (np.arange(nrt) // th)[:, None] + np.zeros(nrf, dtype=int)[None, :]
    bx = np.zeros(nrt, dtype=int)[:, None] + (np.arange(nrf) // tw)[None, :]
    return by, bx


def _kept_lower(nrt, nrf, th=128, tw=64, shift=0):
    """Entries in the tiles a lower_only launch keeps (it leaves out bx * tw + tw - 1 < by * th).  shift: the rule moved by that many tile columns (controls)."""
    by, bx = _tile_of(nrt, nrf, th, tw)
    return ~((bx + shift) * tw + tw - 1 < by * th)


def _explain(got, want, what):
    bad = np.argwhere(got != want)
    t, f = (int(x) for x in bad[0])
    kind = "must keep the fill pattern" if want[t, f] == FILL else ("a sum, the fill is there" if got[t, f] == FILL else "a sum")
    return f"{what}: {len(bad)} of {got.size} int64 differ, first at [{t}][{f}] (tile {t // 128}, {f // 64}): got {got[t, f]}, want {want[t, f]} ({kind})"


def _same(got, want, what):
    assert got.dtype == np.int64 and want.dtype == np.int64
    if not np.array_equal(got, want):
        raise AssertionError(_explain(got, want, what))


def _positions_of_last_partial_chunk(cx, chunk_seqs):
    """The sequences whose bit positions (ascending fixed-point weight, ties by sequence: ldw_set_weights) lie in the last, partial chunk of the K loop."""
    order = np.argsort(cx.V, kind="stable")
    first = (cx.N - 1) // chunk_seqs * chunk_seqs
    return order[first:]


# ------------------------------------------------------------------------------------------------
# the limb GEMM and the popcount kernel: shapes, sequence counts, limbs
# ------------------------------------------------------------------------------------------------
def _check_selection(cx, rng, shapes, limb0, n, popc=False, tag=""):
    eng, G = cx.eng, cx.gram(limb0, n)
    for nrt, nrf in shapes:
        rt, rf = cx.rows(rng, nrt, nrf)
        want = G[np.ix_(rt, rf)]
        got = eng.debug_limb_gemm(rt, rf, limb0=limb0, nlimbs=n)
        _same(got, want, f"{tag} N {cx.N} limbs {limb0}+{n} of {cx.J} shape {nrt} x {nrf}")
        assert np.all(got[-1] == 0) and np.all(got[:, -1] == 0)       # the padding row
        if popc:
            assert limb0 == 0 and n == cx.J
            gp = eng.debug_limb_gemm(rt, rf, engine=1, nlimbs=n)
            _same(gp, want, f"{tag} popcount N {cx.N} limbs {n} shape {nrt} x {nrf}")
            _same(gp, got, "popcount against the limb GEMM")
            gl = eng.debug_limb_gemm(rt, rf, engine=1, nlimbs=n, lower_only=True)
            kept = _kept_lower(nrt, nrf, 64, 64)
            assert kept[np.triu_indices(min(nrt, nrf))].all() and (nrt <= 64 or not kept.all())
            _same(gl, np.where(kept, want, FILL), f"{tag} popcount lower_only N {cx.N} shape {nrt} x {nrf}")
    return len(shapes)


def test_full_shape_sweep_at_three_chunks_five_limbs(engine):
    """N = 2200 (three chunks, the last partial), five limbs: every row-count pair, all limbs, the mixed path's high limbs (2, 3), what the gathered GEMM must
    equal (0, 2), and (1, 2); the popcount kernel on the same rows.  Controls: last partial chunk, top limb, carry of a -128 digit."""
    s0 = engine.gemm_stats()
    cx = _generic(engine, 2200, 5, seed=11)
    rng = np.random.default_rng(12)
    shapes = [(a, b) for a in NRT for b in NRF]
    n = _check_selection(cx, rng, shapes, 0, 5, popc=True, tag="generic")
    for limb0, k in ((2, 3), (0, 2), (1, 2)):
        n += _check_selection(cx, rng, shapes[5::3], limb0, k, tag="generic")
    # (2, 3) << 16 + (0, 2) is the whole sum: the identity the mixed path rests on
    assert np.array_equal(cx.gram(2, 3) * 65536 + cx.gram(0, 2), cx.gram(0, 5))

    rt, rf = cx.rows(rng, 300, 200)
    got = engine.debug_limb_gemm(rt, rf)
    _same(got, cx.gram()[np.ix_(rt, rf)], "all limbs")
    # control: the sequences of the last partial chunk dropped (positions >= 2048 of the GEMM's K loop, and of the popcount kernel's chunks of 1024 too)
    v = cx.vpart()
    v[_positions_of_last_partial_chunk(cx, 1024)] = 0
    assert not np.array_equal(got, _gram(cx.bits, v)[np.ix_(rt, rf)])
    # control: the top limb dropped
    assert not np.array_equal(got, cx.gram(0, 4)[np.ix_(rt, rf)])
    # control: the carry of a -128 digit dropped (the next limb one too low for those sequences)
    dw = cx.d.copy()
    for j in range(cx.J - 1):
        dw[j + 1] -= cx.d[j] == -128
    assert (cx.d[:-1] == -128).any()
    assert not np.array_equal(got, _gram(cx.bits, _vpart(dw, 0, 5))[np.ix_(rt, rf)])
    assert engine.gemm_stats() == s0
    print(f"N 2200, 5 limbs, F {cx.F}: {n} shape x selection cases equal the integer sums")


@pytest.mark.parametrize("N", sorted(SEQ_KW))
def test_every_sequence_count_every_limb_count(engine, N):
    """Unit weights (1 limb), five weight classes (5 limbs) and generic weights with planted extreme digits (2..6 limbs; six = the 3 + 3 launch), a reduced pair
    of shapes each; the selections (2, 3), (0, 2), (1, 2) at five limbs; the popcount kernel at 1, 5 and 6 limbs."""
    s0 = engine.gemm_stats()
    rng = np.random.default_rng(100 + N)
    ran = []
    cx = Ctx(engine, N, _unit(N), 1)
    assert cx.F == 0 and np.all(cx.V == 1)
    _check_selection(cx, rng, REDUCED, 0, 1, popc=True, tag="unit")
    ran.append("unit/1")
    w, sizes = _five_values(N)
    cx = Ctx(engine, N, w, 5)
    _check_five_values(cx, sizes)
    _check_selection(cx, rng, REDUCED, 0, 5, popc=True, tag="five values")
    ran.append("five/5")
    for J in (2, 3, 4, 5, 6):
        cx = _generic(engine, N, J, seed=1000 * J + N)
        if J == 6:
            assert cx.F == (8 * J - 2 if N < 1000 else (42 if N < 2048 else 41)), cx.F      # the sum bound 2^52 / sum(v) decides at six limbs
        else:
            assert cx.F == 8 * J - 2, cx.F
        _check_selection(cx, rng, REDUCED, 0, J, popc=J in (5, 6), tag="generic")
        if J == 5:
            for limb0, k in ((2, 3), (0, 2), (1, 2)):
                _check_selection(cx, rng, REDUCED[1:], limb0, k, tag="generic")
        if J >= 3:
            # control: the top limb dropped; at six limbs that is the accumulate of the second launch gone wrong
            rt, rf = cx.rows(rng, 129, 65)
            got = engine.debug_limb_gemm(rt, rf)
            assert not np.array_equal(got, cx.gram(0, J - 1)[np.ix_(rt, rf)])
            if N % 1024:
                v = cx.vpart()
                v[_positions_of_last_partial_chunk(cx, 1024)] = 0
                assert not np.array_equal(got, _gram(cx.bits, v)[np.ix_(rt, rf)])
        ran.append(f"generic/{J} F {cx.F}")
    assert engine.gemm_stats() == s0
    print(f"N {N} (KW {SEQ_KW[N]}): " + ", ".join(ran))


# ------------------------------------------------------------------------------------------------
# launch forms: lower_only, mask, list, strips
# ------------------------------------------------------------------------------------------------
def _tile_entries(mask, nrt, nrf):
    by, bx = _tile_of(nrt, nrf)
    return mask[by, bx].astype(bool)


@pytest.mark.parametrize("N,J", [(1100, 5), (2200, 6), (100, 3)])
def test_lower_only_mask_list_and_strips(engine, N, J):
    s0 = engine.gemm_stats()
    cx = _generic(engine, N, J, seed=77 + N)
    rng = np.random.default_rng(78 + N)
    eng = cx.eng
    done = 0
    for nrt, nrf in ((300, 200), (129, 65), (300, 40), (300, 320)):      # (320 columns: the third tile row keeps tiles too)
        rt, rf = cx.rows(rng, nrt, nrf)
        want = cx.gram()[np.ix_(rt, rf)]
        nby, nbx = -(-nrt // 128), 2 * -(-nrf // 128)
        full = eng.debug_limb_gemm(rt, rf)
        _same(full, want, "full launch")

        # lower_only: tiles with bx * 64 + 63 < by * 128 hold the fill in every entry, every other tile the sums; no entry on or above the diagonal is lost
        kept = _kept_lower(nrt, nrf)
        tt, ff = np.meshgrid(np.arange(nrt), np.arange(nrf), indexing="ij")
        assert kept[ff >= tt].all()
        if (nrt, nrf) == (300, 200):
            # (tile row 1 = to-rows 128..255 keeps the from-tiles that reach column 128; tile row 2 starts past the last of the 200 columns)
            assert kept[:128].all() and not kept[128:256, :128].any() and kept[128:256, 128:].all() and not kept[256:].any()
        lo = eng.debug_limb_gemm(rt, rf, lower_only=True)
        _same(lo, np.where(kept, want, FILL), f"lower_only {nrt} x {nrf}")
        if nrf >= 200:        # control: the rule one tile off, either way (with fewer columns no entry of the moved tiles is in the output)
            assert not np.array_equal(lo, np.where(_kept_lower(nrt, nrf, shift=1), want, FILL))
            assert not np.array_equal(lo, np.where(_kept_lower(nrt, nrf, shift=-1), want, FILL))

        # tile_mask alone: random masks, the empty one, with lower_only
        masks = [rng.integers(0, 2, (nby, nbx)).astype(np.uint8) for _ in range(3)]
        masks[1][0, 0], masks[1][-1, -1] = 1, 0
        masks[2] = masks[2] * 255                                       # any non-zero byte counts
        for m in masks + [np.zeros((nby, nbx), dtype=np.uint8), np.ones((nby, nbx), dtype=np.uint8)]:
            on = _tile_entries(m, nrt, nrf)
            gm = eng.debug_limb_gemm(rt, rf, tile_mask=m)
            _same(gm, np.where(on, want, FILL), f"mask {m.tolist()}")
            gml = eng.debug_limb_gemm(rt, rf, tile_mask=m, lower_only=True)
            _same(gml, np.where(on & kept, want, FILL), f"mask {m.tolist()} with lower_only")
            # the mask's tiles as a list (with the mask, as the engine passes them), in order and shuffled: the same buffer
            lst = np.array([(by << 16) | bx for by in range(nby) for bx in range(nbx) if m[by, bx]], dtype=np.uint32)
            for order in (lst, rng.permutation(lst)):
                _same(eng.debug_limb_gemm(rt, rf, tile_mask=m, tile_list=order), gm, f"list of mask {m.tolist()}")
            _same(eng.debug_limb_gemm(rt, rf, tile_list=lst), gm, "the list without the mask")
        # a list of one tile (the last one), and of none: LDW_OK, only fill
        one = np.array([((nby - 1) << 16) | (nbx - 1)], dtype=np.uint32)
        by, bx = _tile_of(nrt, nrf)
        _same(eng.debug_limb_gemm(rt, rf, tile_list=one), np.where((by == nby - 1) & (bx == nbx - 1), want, FILL), "list of one tile")
        none = eng.debug_limb_gemm(rt, rf, tile_list=np.zeros(0, dtype=np.uint32))
        assert np.all(none == FILL)
        # a list ignores lower_only (the host leaves those tiles out of the list): a tile above the rule is computed when listed
        _same(eng.debug_limb_gemm(rt, rf, tile_list=one, lower_only=True), np.where((by == nby - 1) & (bx == nbx - 1), want, FILL), "list of one tile, lower_only")

        # strips: every split of the tile rows into consecutive strips
        splits = {1: [[(0, 1)]], 2: [[(0, 2)], [(0, 1), (1, 2)]], 3: [[(0, 3)], [(0, 1), (1, 3)], [(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]]}[nby]
        for split in splits:
            comb = np.full_like(want, FILL)
            for b0, b1 in split:
                g = eng.debug_limb_gemm(rt, rf, by0=b0, by1=b1)
                inside = (by >= b0) & (by < b1)
                _same(g, np.where(inside, want, FILL), f"strip {b0}..{b1}")
                comb = np.where(inside, g, comb)
            _same(comb, full, f"the strips of {split}")
        _same(eng.debug_limb_gemm(rt, rf, by0=nby - 1, by1=-1, lower_only=True), np.where((by == nby - 1) & kept, want, FILL), "last strip, lower_only")
        done += 1
    assert engine.gemm_stats() == s0
    print(f"N {N}, {J} limbs: lower_only, 5 masks, their lists, strips on {done} shapes")


def test_refusals_launch_nothing(engine):
    cx = _generic(engine, 1000, 5, seed=5)
    rng = np.random.default_rng(6)
    rt, rf = cx.rows(rng, 300, 200)
    want = cx.gram()[np.ix_(rt, rf)]
    s0 = engine.gemm_stats()

    def refused(code, rows_t=rt, rows_f=rf, **kw):
        out = np.full((len(rows_t), len(rows_f)), 7, dtype=np.int64)
        with pytest.raises(L.LdwError) as err:
            engine.debug_limb_gemm(rows_t, rows_f, out=out, **kw)
        assert err.value.code == code, err.value
        assert np.all(out == 7)
        assert engine.gemm_stats() == s0

    refused(L.LDW_ERR_ARG, nlimbs=0)
    refused(L.LDW_ERR_ARG, nlimbs=7)
    refused(L.LDW_ERR_ARG, limb0=3, nlimbs=3)
    refused(L.LDW_ERR_ARG, limb0=-1, nlimbs=2)
    refused(L.LDW_ERR_ARG, nlimbs=5, by0=1, by1=1)
    refused(L.LDW_ERR_ARG, nlimbs=5, by0=2, by1=1)
    refused(L.LDW_ERR_ARG, nlimbs=5, by0=0, by1=4)
    refused(L.LDW_ERR_ARG, nlimbs=5, by0=1, by1=2, tile_list=np.array([1 << 16], dtype=np.uint32))
    refused(L.LDW_ERR_ARG, nlimbs=5, tile_list=np.array([3 << 16], dtype=np.uint32))          # a tile outside the grid is refused on the host
    refused(L.LDW_ERR_ARG, nlimbs=5, tile_list=np.array([4], dtype=np.uint32))
    refused(L.LDW_ERR_ARG, nlimbs=5, engine=2)
    refused(L.LDW_ERR_ARG, nlimbs=3, engine=1)                                                # the popcount engine takes all limbs
    refused(L.LDW_ERR_ARG, nlimbs=5, engine=1, by0=1, by1=2)
    for bad in (-1, cx.R + 1):
        r = rt.copy()
        r[5] = bad
        refused(L.LDW_ERR_ARG, rows_t=r, nlimbs=5)
        r = rf.copy()
        r[0] = bad
        refused(L.LDW_ERR_ARG, rows_f=r, nlimbs=5)
    with Engine(0) as fresh:                                                                   # no weights set
        fresh.set_alignment(_aln(1000)["states"])
        f0 = fresh.gemm_stats()
        out = np.full((len(rt), len(rf)), 7, dtype=np.int64)
        for e in (0, 1):
            with pytest.raises(L.LdwError) as err:
                fresh.debug_limb_gemm(rt, rf, engine=e, nlimbs=5, out=out)
            assert err.value.code == L.LDW_ERR_STATE, err.value
        with pytest.raises(L.LdwError) as err:
            fresh.debug_lo_units(np.zeros(64, dtype=np.int32), np.zeros(1, dtype=np.int32), [[[0], [], []]])
        assert err.value.code == L.LDW_ERR_STATE, err.value
        assert np.all(out == 7) and fresh.gemm_stats() == f0
    # the engine is as usable as before
    _same(engine.debug_limb_gemm(rt, rf), want, "after the refusals")
    assert engine.gemm_stats() == s0


# ------------------------------------------------------------------------------------------------
# the gathered low-limb GEMM
# ------------------------------------------------------------------------------------------------
def _lo_expected(cx, geo, from_snps, to_snps, lists, Glo, skip_chunk=None):
    """The whole raw buffer: fill; every chunk of 128 rows a list reaches written — the listed units' sums, 0 for absent rows, absent slots, padding lanes and
    the rows beyond the last unit.  skip_chunk = (tile, chunk of the tile counted through the classes): left unwritten (control)."""
    R = cx.R
    want = np.full(geo["glo_total"], FILL32, dtype=np.int32)
    ntiles = len(from_snps) // 64
    for t in range(ntiles):
        cm = int(geo["cmax"][t])
        ld = 64 * cm
        blk = want[int(geo["tile_base"][t]): int(geo["tile_base"][t]) + geo["RTlo"] * ld].reshape(geo["RTlo"], ld)
        cols = np.full(ld, R, dtype=np.int64)
        for ln in range(64):
            a = int(from_snps[64 * t + ln])
            if a >= 0:
                for i in range(min(cm, cx.nrows[a])):
                    cols[ln * cm + i] = cx.row0[a] + i
        seq = 0
        for lc in range(3):
            lst = np.asarray(lists[t][lc], dtype=np.int64)
            rows_n = len(lst) << lc
            nch = -(-rows_n // 128)
            trows = np.full(nch * 128, R, dtype=np.int64)
            for k, q in enumerate(lst):
                b = int(to_snps[q])
                for j in range(min(1 << lc, cx.nrows[b])):
                    trows[(k << lc) + j] = cx.row0[b] + j
            vals = Glo[np.ix_(trows, cols)].astype(np.int32)
            for ch in range(nch):
                if skip_chunk != (t, seq):
                    r0 = int(geo["rowbase"][lc]) + ch * 128
                    blk[r0: r0 + 128] = vals[ch * 128: ch * 128 + 128]
                seq += 1
    return want


def _lo_pools(cx):
    pool = {n: np.flatnonzero(cx.nrows == n) for n in (1, 2, 3, 4)}
    assert all(len(pool[n]) >= 5 for n in pool), {n: len(p) for n, p in pool.items()}      # 1, 2, 3 and 4 indicator rows occur
    assert set(PLANT_3ROWS) <= set(pool[3]) and set(PLANT_4ROWS) <= set(pool[4])
    return pool


def _explain_lo(got, want, geo):
    bad = np.flatnonzero(got != want)
    at = int(bad[0])
    t = int(np.searchsorted(geo["tile_base"], at, side="right")) - 1
    ld = 64 * int(geo["cmax"][t])
    row, col = divmod(at - int(geo["tile_base"][t]), ld)
    return f"{len(bad)} of {len(got)} int32 differ, first in tile {t} row {row} (chunk {row // 128}) int {col}: got {got[at]}, want {want[at]} (fill {FILL32})"


@pytest.mark.parametrize("N", sorted(SEQ_KW))
def test_gathered_low_limbs_equal_the_integer_sums(engine, N):
    """Five tiles — cmax 1, 2, 4, a tile nothing is listed for, a last tile with padding lanes — and per-class unit counts 0, 1, exactly one chunk of 128 rows
    (128, 64, 32 units) and the first count past it (129, 65, 33)."""
    cx = _generic(engine, N, 5, seed=300 + N)
    pool = _lo_pools(cx)
    rng = np.random.default_rng(301 + N)
    pick = lambda n, k: rng.choice(pool[n], k, replace=True)
    from_snps = np.concatenate([
        pick(1, 64),                                                                    # cmax 1
        rng.permutation(np.concatenate([pick(1, 40), pick(2, 24)])),                    # cmax 2
        rng.permutation(np.concatenate([pick(1, 30), pick(2, 20), pick(3, 8), pick(4, 6)])),   # cmax 4: three-row SNPs are slot-masked
        rng.permutation(np.concatenate([pick(1, 60), pick(2, 4)])),                     # nothing listed
        rng.permutation(np.concatenate([pick(1, 9), pick(2, 5), pick(3, 6), np.full(44, -1)])),   # padding lanes, three rows the widest: cmax 4
    ]).astype(np.int32)
    to_snps = rng.permutation(np.concatenate([pick(1, 140), pick(2, 70), pick(3, 25), pick(4, 15)])).astype(np.int32)
    cls = np.array([0 if cx.nrows[b] <= 1 else (1 if cx.nrows[b] == 2 else 2) for b in to_snps])
    slots = [np.flatnonzero(cls == lc) for lc in range(3)]
    listed = lambda counts: [rng.permutation(slots[lc])[:counts[lc]] for lc in range(3)]
    lists = [listed((128, 64, 32)), listed((129, 65, 33)), listed((1, 0, 1)), listed((0, 0, 0)), listed((0, 1, 0))]
    geo = engine.debug_lo_units(from_snps, to_snps, lists)
    assert list(geo["cmax"]) == [1, 2, 4, 2, 4]
    assert list(geo["rowbase"]) == [0, 256, 512] and geo["RTlo"] == 768 and list(geo["uoff"]) == [0, 140, 210] and geo["n_tf"] == 13
    Glo = cx.gram(0, 2)
    assert np.abs(Glo).max() < 2 ** 31
    want = _lo_expected(cx, geo, from_snps, to_snps, lists, Glo)
    got = geo["glo"]
    assert np.array_equal(got, want), _explain_lo(got, want, geo)
    # what the layout means: a whole tile of fill, chunks of fill behind one-chunk lists, zero rows behind the last unit of a two-chunk list
    t3 = want[int(geo["tile_base"][3]): int(geo["tile_base"][4])]
    assert np.all(t3 == FILL32)
    b1 = want[int(geo["tile_base"][1]): int(geo["tile_base"][2])].reshape(768, 128)
    assert np.all(b1[129:256] == 0) and np.all(b1[256 + 130: 512] == 0) and np.all(b1[512 + 132:] == 0) and (b1[:129] != 0).any()
    b0 = want[: int(geo["tile_base"][1])].reshape(768, 64)
    assert np.all(b0[128:256] == FILL32) and np.all(b0[384:512] == FILL32) and np.all(b0[640:] == FILL32)
    # the gathered sums are what the block-wide GEMM gives for limbs (0, 2) on the same rows
    rt = np.array([cx.row0[to_snps[q]] for q in lists[0][0][:100]], dtype=np.int32)
    rf = np.array([cx.row0[a] for a in from_snps[:64]], dtype=np.int32)
    _same(engine.debug_limb_gemm(rt, rf, limb0=0, nlimbs=2), Glo[np.ix_(rt, rf)], "limbs (0, 2) of the block-wide GEMM")
    assert np.array_equal(b0[:100], Glo[np.ix_(rt, rf)])
    # control: the top limb of the two dropped
    assert not np.array_equal(got, _lo_expected(cx, geo, from_snps, to_snps, lists, cx.gram(0, 1)))
    print(f"N {N}: {geo['glo_total']} int32 of 5 tiles equal the integer sums")


def test_gathered_low_limbs_more_chunks_than_workgroups(engine):
    """N = 100: 4 224 one-row units in one tile = 33 chunks for the 32 workgroups along x, beside a tile of a few chunks; the chunk index rotates by the
    workgroup's y, so no chunk may be lost or done twice.  Refusals of the hook."""
    cx = _generic(engine, 100, 5, seed=401)
    pool = _lo_pools(cx)
    rng = np.random.default_rng(402)
    pick = lambda n, k: rng.choice(pool[n], k, replace=True)
    from_snps = np.concatenate([rng.permutation(np.concatenate([pick(1, 50), pick(2, 14)])), rng.permutation(np.concatenate([pick(1, 20), pick(4, 3), np.full(41, -1)]))]).astype(np.int32)
    to_snps = np.concatenate([pick(1, 4224), pick(2, 70), pick(3, 3)]).astype(np.int32)
    lists = [[rng.permutation(4224), [], []], [rng.permutation(4224)[:200], 4224 + rng.permutation(70), [4224 + 70 + 1]]]
    geo = engine.debug_lo_units(from_snps, to_snps, lists)
    assert list(geo["cmax"]) == [2, 4] and list(geo["rowbase"]) == [0, 4224, 4224 + 256] and geo["RTlo"] == 4224 + 256 + 128 and geo["n_tf"] == 6
    assert 4224 == 33 * 128
    Glo = cx.gram(0, 2)
    want = _lo_expected(cx, geo, from_snps, to_snps, lists, Glo)
    got = geo["glo"]
    assert np.array_equal(got, want), _explain_lo(got, want, geo)
    # control: the 33rd chunk of the first tile dropped
    assert not np.array_equal(got, _lo_expected(cx, geo, from_snps, to_snps, lists, Glo, skip_chunk=(0, 32)))

    def refused(code, f=from_snps, t=to_snps, ls=lists):
        with pytest.raises(L.LdwError) as err:
            engine.debug_lo_units(f, t, ls)
        assert err.value.code == code, err.value

    f = from_snps.copy()
    f[3] = LS
    refused(L.LDW_ERR_ARG, f=f)
    f[3] = -2
    refused(L.LDW_ERR_ARG, f=f)
    t = to_snps.copy()
    t[0] = -1
    refused(L.LDW_ERR_ARG, t=t)
    refused(L.LDW_ERR_ARG, ls=[[[len(to_snps)], [], []], lists[1]])                  # a slot outside 0..nt-1
    refused(L.LDW_ERR_ARG, ls=[[[], [0], []], lists[1]])                             # a one-row SNP listed as a two-row unit
    refused(L.LDW_ERR_ARG, ls=[lists[0], [[], list(range(4224, 4294)) + [4224], []]])   # 71 units of a class the to side holds 70 of
    cx1 = Ctx(engine, 100, _unit(100), 1)                                            # one limb: the low-limb GEMM reads two
    with pytest.raises(L.LdwError) as err:
        cx1.eng.debug_lo_units(from_snps, to_snps, lists)
    assert err.value.code == L.LDW_ERR_STATE, err.value

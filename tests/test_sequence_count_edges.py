"""The MI engine at its sequence-count gates (pytest -m gpu): every kernel form the engine picks by the number of sequences N, run on
both sides of its switch, up to 70 000 sequences.

The forms and where they flip:
  - exact pair sums of the approximate path's listed pairs (launch_pairs_exact, ldw_pairs.hip): the bit walk against a per-position weight table
    in LDS (k_pair_sums_bits) within the default 64 KB up to Npad 8 192, with the 160-KB dynamic-LDS attribute up to Npad 20 480, beyond that
    the class-wise popcounts (k_pair_sums) with their segment tables in global memory; few weight classes take k_pair_sums with LDS tables;
  - the approximate path itself up to Npad 30 720 (prepare_apx_weights);
  - mixed precision up to N = 60 000 (the gathered low-limb sums are int32: |sum| <= N * 32 896);
  - the bit-row fill stages a state row in LDS up to Npad 61 440 (k_fill_rows_bits);
  - the popcount engine (LDW_ENGINE_HIST) up to N = 65 535 (its 16-bit limb sums are 32-bit);
  - Hamming weights at N = 70 000.
Each case proves through ldw_pair_form_report, ldw_path_report and the counters that it reached the form it targets, and checks against plain
references: joint sums bit-exact against numpy int64 sums of the engine's fixed-point weights, a dense block of fp64 MI against the C oracle
(both quirk modes), sampled link-table rows against the per-pair oracle, and whole passes of the default path (cold, warm, verify mode)
against the plain path bit for bit.  The weights are dyadic, w = k 2^-22 with N distinct integers k in [2^16, 2^22), so the fixed point holds
them exactly and the MI bar is MI_TIGHT.

Memory: the 70 000-sequence case computes Hamming weights four times; each call allocates about 39 GB of device memory for the int64 Rp x Rp
comparison matrix (Rp = 70 016), so it runs on a context of its own that is closed afterwards.  No case asks for the N x N shared counts
(20 GB as int32 at 70 000).
"""
import os
import time

import numpy as np
import pytest
import torch

import c_oracle
import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.dist import hamming_tile_strips
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu
MI_TIGHT = 1e-10       # what exactly held weights deliver
LS, BLK = 2_400, 1_200
LR_RETAIN = 4000.0     # 0.14 % of the 2.9e6 pairs: speculation is the automatic choice
PAIR_FORMS = ("bits_lds64", "bits_lds160", "classwise_lds", "classwise_global")
FI, TI = np.arange(0, 64), np.arange(BLK, BLK + 64)       # the dense sub-block: holds every planted SNP
EXTREMAL = [(0, 1), (1, 0), (0, 2), (3, 4), (0, BLK), (BLK, BLK + 1), (3, BLK + 1), (LS - 1, 0), (5, 5), (2, LS - 1)]

_ALIGNMENTS = {}


def _alignment(width, seed):
    """One (LS, width) synthetic alignment on the device, shared by the neighbouring N of a group (contiguous column slices)."""
    key = (width, seed)
    if key not in _ALIGNMENTS:
        _ALIGNMENTS.clear()
        syn = synth_alignment(LS, width, seed=seed, device="cuda", as_numpy=False)
        _ALIGNMENTS[key] = syn
    return _ALIGNMENTS[key]


def _states(syn, N):
    """Columns [0, N) of the group's alignment with extremal SNPs planted: rows 0, 1, BLK and LS - 1 carry minor state C in the same N / 2
    sequences (A elsewhere), row 2 is their complement, rows 3, 4 and BLK + 1 carry a single minor state (T in one sequence, G elsewhere)."""
    st = syn["states"][:, :N].contiguous()
    half = torch.zeros(N, dtype=torch.bool, device=st.device)
    half[torch.as_tensor(np.random.default_rng(N).permutation(N)[:N // 2], device=st.device)] = True
    a = torch.where(half, 1, 0).to(torch.uint8)
    for row in (0, 1, BLK, LS - 1):
        st[row] = a
    st[2] = torch.where(half, 0, 1).to(torch.uint8)
    one = torch.full((N,), 2, dtype=torch.uint8, device=st.device)
    one[N // 3] = 3
    for row in (3, 4, BLK + 1):
        st[row] = one
    return st


def _dyadic(N, seed):
    """N distinct dyadic weights k 2^-22, k in [2^16, 2^22): N weight classes over 1/64 .. 1, held exactly by the fixed point."""
    k = np.random.default_rng(seed).choice((1 << 22) - (1 << 16), size=N, replace=False) + (1 << 16)
    w = np.ldexp(k.astype(np.float64), -22)
    assert len(np.unique(w)) == N
    return w


def _planned_F(w, nlimbs=5):
    """The fixed-point exponent ldw_set_weights chooses (ldw_api.hip): V = round(v 2^F) fits nlimbs balanced base-256 digits, sum V < 2^52."""
    v = np.sqrt(w) ** 2
    lim_digits = 0.99 * np.ldexp(1.0, 8 * nlimbs - 1) / v.max()
    lim_sum = np.ldexp(1.0, 52) / float(np.sum(v, dtype=np.longdouble))
    return int(np.floor(np.log2(min(lim_digits, lim_sum))))


def _setup(eng, st, syn, hdw, nlimbs=0):
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(st)
    cnt = eng.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    if hdw is None:
        hdw = eng.hamming_weights(int(LS * 0.1))
    eng.set_weights(hdw, nlimbs)
    eng.set_snp_meta(r, uqe, syn["POS"], syn["paint"], float(syn["g"]))
    return hdw, r, uqe


def _check_joint_sums(eng, st, hdw):
    """Sampled pairs and the planted extremal ones: unweighted counts and fixed-point sums against numpy int64 sums of V (debug_apx_params)."""
    _, V, _ = eng.debug_apx_params()
    _, _, fb = eng.joint_tables([0], [1])
    assert np.array_equal(V, np.rint(np.ldexp(np.sqrt(hdw) ** 2, fb)).astype(np.int64))
    rng = np.random.default_rng(len(hdw))
    pa = np.concatenate([[p for p, _ in EXTREMAL], rng.integers(0, LS, 14)])
    pb = np.concatenate([[q for _, q in EXTREMAL], rng.integers(0, LS, 14)])
    cnt, fix, _ = eng.joint_tables(pa, pb)
    rows = st[torch.as_tensor(np.concatenate([pa, pb]), device=st.device)].cpu().numpy().astype(np.int64)
    for k in range(len(pa)):
        code = rows[k] * 5 + rows[len(pa) + k]
        want = np.zeros(25, dtype=np.int64)
        np.add.at(want, code, V)
        assert np.array_equal(cnt[k], np.bincount(code, minlength=25).reshape(5, 5)), (pa[k], pb[k])
        assert np.array_equal(fix[k].ravel(), want), (pa[k], pb[k])
    return int(np.abs(fix).max())


def _check_dense_mi(eng, st, hdw, r, uqe):
    """The 64 x 64 block (FI, TI) in both quirk modes: the reference mode against the C oracle, the intended mode against the per-pair oracle."""
    idx = np.concatenate([FI, TI])
    rows = st[torch.as_tensor(idx, device=st.device)].cpu().numpy()
    lf, lt = np.arange(len(FI)), np.arange(len(FI), len(idx))
    Mq = eng.mi_block(FI, TI, quirk=L.QUIRK_REFERENCE)
    Mi = eng.mi_block(FI, TI, quirk=L.QUIRK_INTENDED)
    ref = c_oracle.mi_block(rows, hdw, r[idx], uqe[idx], lf, lt)
    err = float(np.abs(Mq - ref).max())
    for a, b in ((0, 0), (0, 1), (1, 0), (2, 0), (3, 1), (4, 1), (63, 63), (17, 40)):
        err = max(err, abs(Mi[a, b] - orc.mi_pair_direct(rows, hdw, r[idx], uqe[idx], lf[a], lt[b])))
    assert err < MI_TIGHT, err
    assert Mq.max() > 0.5      # (the planted copies: not a block of near-zero values)
    return err, Mq


def _check_table_rows(eng, st, hdw, r, uqe):
    """Sampled rows of both link tables of the last pass against the per-pair oracle with the RXY the block read (quirk Q1)."""
    rng = np.random.default_rng(9)
    err = 0.0
    for ta, tb, tm in (eng.links(0), eng.links(1)):
        assert len(tm) > 0
        for k in rng.integers(0, len(tm), 8):
            a, b, mk = int(ta[k]), int(tb[k]), float(tm[k])
            rows = st[[a, b]].cpu().numpy()
            fa, tb0 = a // BLK * BLK, b // BLK * BLK
            nfb, ntb = min(BLK, LS - fa), min(BLK, LS - tb0)
            rxy = orc.q1_rxy(a - fa, b - tb0, nfb, ntb, r[fa:fa + nfb], r[tb0:tb0 + ntb])
            err = max(err, abs(mk - orc.mi_pair_direct(rows, hdw, r[[a, b]], uqe[[a, b]], 0, 1, rxy)))
    assert err < MI_TIGHT, err
    return err


def _passes(eng, syn, env=None):
    """Whole passes over LS SNPs in blocks of BLK: the plain path, then the default path cold and warm and verify mode.  No block is redone for
    an overflowing list; a speculation miss (a block whose guessed threshold was too high, run again without it) is allowed.  Returns per variant
    (sr table, lr table, block_stats, deltas of counters / path_report / overflow_report / span_report / ldw_pair_form_report)."""
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(LS, BLK)
    out = {}
    try:
        if env:
            os.environ[env] = "1"
        for key, (mixed, scr, path, cold) in dict(plain=(False, 0, 1, True), cold=(True, 1, 0, True), warm=(True, 1, 0, False),
                                                  verify=(True, 2, 0, False)).items():
            eng.set_mixed(mixed)
            eng.set_screen(scr)
            eng.set_path(path)
            if cold:
                eng.reset_speculation()
            before = (eng.counters(), eng.path_report(), eng.overflow_report(), eng.span_report(), eng.form_report())
            eng.mi_all_pairs(blocks, 20000.0, LR_RETAIN, approx)
            after = (eng.counters(), eng.path_report(), eng.overflow_report(), eng.span_report(), eng.form_report())
            d = {}
            for tag, b0, b1 in zip(("", "path_", "overflow_", "span_", ""), before, after):
                for k in b1:
                    if not isinstance(b1[k], str):
                        d[tag + k] = int(b1[k]) - int(b0[k])
            out[key] = (eng.links(0), eng.links(1), eng.block_stats(), d)
    finally:
        if env:
            os.environ.pop(env, None)
        eng.set_mixed(True)
        eng.set_screen(1)
        eng.set_path(0)
    for key in ("cold", "warm", "verify"):
        for which in (0, 1):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (key, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(out["plain"][2][k], out[key][2][k]), (key, k)
        d = out[key][3]
        assert d["screen_violations"] == 0, (key, d)
        assert d["overflow_pair_list"] == 0 and d["overflow_maybe_list"] == 0 and d["span_redone"] == 0, (key, d)
    assert out["plain"][3]["apx_blocks"] == 0 and out["plain"][3]["mixed_blocks"] == 0
    assert len(out["plain"][1][2]) > 1000 and len(out["plain"][0][2]) > 1000
    return out, len(blocks)


def _reached(out, nblocks, apx, mixed, form):
    """The default passes (cold, warm, verify) took the targeted path and pair-sum form; `form` None: no pair sums at all (no approximate path).
    (Verify mode evaluates every pair of its blocks in fp64 and lists none, so the pair sums run in the cold and warm passes only.)"""
    for key in ("cold", "warm", "verify"):
        d = out[key][3]
        listed = apx and key != "verify"
        if apx:
            assert d["apx_blocks"] > 0 and (d["apx_pairs_listed"] > 0) == listed, (key, d)
        else:
            assert d["apx_blocks"] == 0, (key, d)
        if mixed:
            assert d["mixed_blocks"] > 0, (key, d)
        else:
            assert d["mixed_blocks"] == 0, (key, d)
        if not apx and not mixed:     # the limb GEMM of all five limbs with the screen: blocks neither fast path took
            assert d["path_plain_blocks"] > 0, (key, d)
        for f in PAIR_FORMS:
            if f == form and listed:
                assert d[f] > 0, (key, f, d)
            else:
                assert d[f] == 0, (key, f, d)


def _misses(out):
    return "/".join(str(out[k][3]["spec_misses"]) for k in ("cold", "warm", "verify"))


def _report(tag, N, t0, **kw):
    print(f"[N = {N}] {tag}: " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()) +
          f", wall {time.time() - t0:.1f} s")


# ------------------------------------------------------------------------------------------------
# the pair-sum forms of the approximate path and its own gate
# ------------------------------------------------------------------------------------------------
# (width, seed of the group's alignment), N, form, extra environment
APX_CASES = {
    "bits_lds64_8192": ((8_193, 31), 8_192, "bits_lds64", None),
    "bits_lds160_8193": ((8_193, 31), 8_193, "bits_lds160", None),
    "bits_lds160_20480": ((30_720, 32), 20_480, "bits_lds160", None),
    "classwise_global_20481": ((30_720, 32), 20_481, "classwise_global", None),
    "classwise_global_4000_no_bits": ((30_720, 32), 4_000, "classwise_global", "LDW_NO_PAIR_BITS"),
    "apx_gate_30720": ((30_720, 32), 30_720, "classwise_global", None),
}


@pytest.mark.parametrize("case", list(APX_CASES))
def test_pair_sum_forms_on_both_sides_of_their_switches(engine, case):
    """N distinct dyadic weights (many weight classes): the exact pair sums take the bit walk within 64 KB of LDS up to Npad 8 192, with the
    160-KB attribute from Npad 8 320 up to 20 480, and the class-wise popcounts with global tables from Npad 20 608 (or at any N with
    LDW_NO_PAIR_BITS); the approximate path stays on up to its own gate Npad 30 720.  Tables of cold, warm and verify passes == plain path."""
    t0 = time.time()
    (width, seed), N, form, env = APX_CASES[case]
    syn = _alignment(width, seed)
    st = _states(syn, N)
    hdw, r, uqe = _setup(engine, st, syn, _dyadic(N, N))
    info, rep = engine.apx_info(), engine.path_report()
    assert info["usable"] and rep["apx_gate"].startswith("ok") and info["classes"] == N, (info, rep)
    big = _check_joint_sums(engine, st, hdw)
    err, _ = _check_dense_mi(engine, st, hdw, r, uqe)
    out, nb = _passes(engine, syn, env)
    _reached(out, nb, apx=True, mixed=False, form=form)
    err = max(err, _check_table_rows(engine, st, hdw, r, uqe))
    _report(case, N, t0, form=form, mi_err=err, largest_joint_sum=big, apx_blocks=out["warm"][3]["apx_blocks"], misses=_misses(out))


def test_few_weight_classes_take_the_lds_tables_above_the_bit_walk(engine):
    """Hamming weights at N = 24 000 (a few dozen weight classes): beyond the bit walk's 160 KB, but few segments per word, so the pair sums
    are class-wise with the segment tables in LDS."""
    t0 = time.time()
    syn = _alignment(30_720, 32)
    N = 24_000
    st = _states(syn, N)
    hdw, r, uqe = _setup(engine, st, syn, None)
    info = engine.apx_info()
    assert info["usable"] and info["classes"] < 200, info
    big = _check_joint_sums(engine, st, hdw)
    err, _ = _check_dense_mi(engine, st, hdw, r, uqe)
    out, nb = _passes(engine, syn)
    _reached(out, nb, apx=True, mixed=False, form="classwise_lds")
    err = max(err, _check_table_rows(engine, st, hdw, r, uqe))
    _report("classwise_lds_hamming", N, t0, classes=info["classes"], mi_err=err, largest_joint_sum=big)


# ------------------------------------------------------------------------------------------------
# mixed precision, the bit-row fill, the popcount engine
# ------------------------------------------------------------------------------------------------
LO_MIN = -32_896       # the most negative balanced two-digit value: -128 + 256 * -128


def _extremal_low_limb_weights(N, F=36):
    """Weights just below 1 whose fixed-point values all have the low limbs -128, -128: V = 2^36 - 32 896 - 2^16 j, j distinct in [0, 2^18)."""
    j = np.random.default_rng(N).choice(1 << 18, size=N, replace=False).astype(np.int64)
    V = (1 << F) + LO_MIN - (j << 16)
    return np.ldexp(V.astype(np.float64), -F), V


def test_mixed_precision_at_its_gate_with_extremal_low_limbs(engine):
    """N = 60 000, the largest N of mixed precision: every weight's two low limbs are -128, -128 (V = -32 896 mod 2^16), and SNPs sharing
    their minor state in N / 2 sequences (or their major state in N - 1) drive the int32 low-limb sums of gemm_lo_units_kernel to
    N / 2 * -32 896 and (N - 1) * -32 896 = -1.97e9, near -2^31.  The mixed blocks' tables == the plain path's."""
    t0 = time.time()
    N = 60_000
    syn = _alignment(70_000, 33)
    st = _states(syn, N)
    hdw, Vw = _extremal_low_limb_weights(N)
    assert _planned_F(hdw) == 36
    hdw, r, uqe = _setup(engine, st, syn, hdw)
    par, V, _ = engine.debug_apx_params()
    P = dict(zip(Engine.APX_PARAM_NAMES, par))
    assert int(P["F"]) == 36 and int(P["nlimbs"]) == 5
    assert np.array_equal(V, Vw)
    d0 = ((V + 128) & 255) - 128                  # the balanced digits ldw_set_weights takes: both low ones -128
    d1 = (((V - d0) // 256 + 128) & 255) - 128
    assert np.all(V % 65536 == LO_MIN % 65536) and np.all(d0 == -128) and np.all(d1 == -128)
    assert P["lo_abs_sum"] == pytest.approx(N * 32896 * 2.0 ** -36, rel=1e-12)
    big = _check_joint_sums(engine, st, hdw)
    err, _ = _check_dense_mi(engine, st, hdw, r, uqe)
    out, nb = _passes(engine, syn)
    assert not engine.apx_info()["usable"]
    _reached(out, nb, apx=False, mixed=True, form=None)
    err = max(err, _check_table_rows(engine, st, hdw, r, uqe))
    _report("mixed_gate_extremal_low_limbs", N, t0, mi_err=err, largest_joint_sum=big, mixed_blocks=out["warm"][3]["mixed_blocks"],
            lo_sum_bound=(N - 1) * 32896)


FILL_CASES = {"mixed_off_60001": (60_001, False), "fill_rows_lds_61440": (61_440, False), "fill_rows_global_61441": (61_441, True)}


@pytest.mark.parametrize("case", list(FILL_CASES))
def test_limb_paths_above_the_mixed_gate_and_the_bit_row_fill(engine, case):
    """N = 60 001: mixed precision off, the screen still on (5-limb GEMM, screened blocks; verify mode counts no loss).  Npad 61 440 / 61 568:
    the bit rows are filled with a state row staged in LDS / read from global memory (k_fill_rows_bits, ldw_pair_form_report)."""
    t0 = time.time()
    N, fill_global = FILL_CASES[case]
    syn = _alignment(70_000, 33)
    st = _states(syn, N)
    f0 = engine.form_report()["fill_rows_global"]
    hdw, r, uqe = _setup(engine, st, syn, _dyadic(N, N))
    big = _check_joint_sums(engine, st, hdw)
    err, _ = _check_dense_mi(engine, st, hdw, r, uqe)
    out, nb = _passes(engine, syn)
    _reached(out, nb, apx=False, mixed=False, form=None)
    fills = engine.form_report()["fill_rows_global"] - f0
    assert (fills > 0) == fill_global, fills
    err = max(err, _check_table_rows(engine, st, hdw, r, uqe))
    _report(case, N, t0, mi_err=err, largest_joint_sum=big, fill_rows_global=fills)


def test_popcount_engine_at_its_limit_equals_the_mfma_engine(engine):
    """N = 65 535, the popcount engine's limit (its 16-bit limb sums are 32-bit, exact up to N * 65 535 < 2^32): 6-limb weights whose two low
    16-bit limbs are 0xFFFF for every sequence (the third is below 2^14: V < 2^46 at F = 46), and SNPs that share their major state in N - 1
    sequences, so a limb sum reaches (N - 1) * 65 535.  Dense blocks equal the MFMA engine's bit for bit, and the C oracle."""
    t0 = time.time()
    N = 65_535
    syn = _alignment(70_000, 33)
    st = _states(syn, N)
    rng = np.random.default_rng(5)
    m = rng.integers(0, 24, N).astype(np.int64)
    m[rng.choice(N, 5, replace=False)] = rng.integers(8_000, 16_000, 5)
    Vw = (m << 32) + 0xFFFFFFFF
    hdw = np.ldexp(Vw.astype(np.float64), -46)
    assert _planned_F(hdw, 6) == 46
    hdw, r, uqe = _setup(engine, st, syn, hdw, nlimbs=6)
    par, V, _ = engine.debug_apx_params()
    P = dict(zip(Engine.APX_PARAM_NAMES, par))
    assert int(P["F"]) == 46 and int(P["nlimbs"]) == 6 and np.array_equal(V, Vw)
    assert np.all(V & 0xFFFF == 0xFFFF) and np.all((V >> 16) & 0xFFFF == 0xFFFF) and (V >> 32).max() < 1 << 14
    big = _check_joint_sums(engine, st, hdw)
    assert big >= (N - 1) * 0xFFFFFFFF       # (the major x major cell of the single-minor-state SNPs)
    blocks = ((FI, TI), (np.arange(0, 256), np.arange(0, 256)), (np.arange(BLK - 3, BLK + 300), np.arange(LS - 77, LS)))
    res = {}
    try:
        for kind in (L.ENGINE_MFMA, L.ENGINE_HIST):
            engine.set_engine(kind)
            res[kind] = [engine.mi_block(fi, ti, quirk=q) for fi, ti in blocks for q in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED)]
    finally:
        engine.set_engine(L.ENGINE_MFMA)
    for x, y in zip(res[L.ENGINE_MFMA], res[L.ENGINE_HIST]):
        assert np.array_equal(x, y)
    err, Mq = _check_dense_mi(engine, st, hdw, r, uqe)
    assert np.array_equal(Mq, res[L.ENGINE_HIST][0])
    _report("popcount_engine_limit", N, t0, mi_err=err, largest_joint_sum=big)


def test_popcount_engine_refuses_65536_sequences_and_the_context_goes_on(engine):
    """N = 65 536: LDW_ENGINE_HIST refuses with LDW_ERR_ARG (its 32-bit limb sums could wrap); the same context then gives the MFMA results
    it gave before the refusal."""
    t0 = time.time()
    N = 65_536
    syn = _alignment(70_000, 33)
    st = _states(syn, N)
    hdw, r, uqe = _setup(engine, st, syn, _dyadic(N, N))
    before = engine.mi_block(FI, TI)
    try:
        engine.set_engine(L.ENGINE_HIST)
        with pytest.raises(L.LdwError) as e:
            engine.mi_block(FI, TI)
        assert e.value.code == L.LDW_ERR_ARG and "65535" in str(e.value)
    finally:
        engine.set_engine(L.ENGINE_MFMA)
    assert np.array_equal(engine.mi_block(FI, TI), before)
    err, _ = _check_dense_mi(engine, st, hdw, r, uqe)
    _report("popcount_engine_refusal", N, t0, mi_err=err)


# ------------------------------------------------------------------------------------------------
# Hamming weights and a whole default pass at 70 000 sequences
# ------------------------------------------------------------------------------------------------
def test_hamming_weights_and_a_default_pass_at_70000_sequences():
    """N = 70 000 on a context of its own (each Hamming call allocates ~39 GB for the int64 comparison matrix): sampled Hamming weights
    against a direct count on the device, the neighbour counts of 3 strips of row tiles add up to the whole, and a full default pass with
    those weights (cold, warm, verify) equals the plain path."""
    t0 = time.time()
    N = 70_000
    syn = _alignment(70_000, 33)
    st = _states(syn, N)
    thresh = int(LS * 0.1)
    with Engine(0) as eng:
        hdw, r, uqe = _setup(eng, st, syn, None)
        assert 0 < hdw.min() and hdw.max() <= 1.0 and len(np.unique(hdw)) > 3
        for j in list(np.random.default_rng(3).integers(0, N, 6)) + [N // 3, N - 1]:
            diff = (st != st[:, int(j)][:, None]).sum(0)
            assert hdw[j] == 1.0 / (int((diff < thresh).sum()) + 1.0), j
        tot = np.zeros(N, dtype=np.int64)
        strips = hamming_tile_strips(N, 3)
        assert strips[0][0] == 0 and strips[-1][1] == (N + 127) // 128 and all(a[1] == b[0] for a, b in zip(strips[:-1], strips[1:]))
        for t0_, t1_ in strips:
            if t1_ > t0_:
                tot += eng.hamming_counts(thresh, t0_, t1_)
        assert np.array_equal(1.0 / (tot + 1.0), hdw)
        big = _check_joint_sums(eng, st, hdw)
        err, _ = _check_dense_mi(eng, st, hdw, r, uqe)
        out, nb = _passes(eng, syn)
        _reached(out, nb, apx=False, mixed=False, form=None)
        assert eng.form_report()["fill_rows_global"] > 0
        err = max(err, _check_table_rows(eng, st, hdw, r, uqe))
    _report("hamming_default_pass", N, t0, mi_err=err, largest_joint_sum=big, classes=len(np.unique(hdw)))

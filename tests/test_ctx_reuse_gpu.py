"""GPU: one context used for one problem after another (pytest -m gpu).  Every setter of the C ABI drops what its input made stale — the chain of
DESIGN.md 27 — and nothing else; these tests characterise that chain from outside: whatever a context has seen before, its link tables and block
statistics equal a fresh context's bit for bit, in the order the tables come in (as test_in_process_multi_context_equals_one_context compares them).

Problem A is the bundled snp_sample alignment (1268 SNPs x 400 sequences, blocks of 500); problem B its first 500 SNPs and every tenth sequence
(N = 40) with its own Hamming weights, blocks of 200: a smaller problem after a larger one, the shape class in which stale per-block flags once showed."""
import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine

pytestmark = pytest.mark.gpu

SR_DIST = 20000.0
NO_INPUT = "MI needs the alignment, the weights and the SNP meta data to be set first"


def load(eng, d, weights=True, meta=True):
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(d["states"])
    if weights:
        eng.set_weights(d["hdw"])
    if meta:
        eng.set_snp_meta(d["r"], d["uqe"], d["POS"], d["paint"], d["g"])


def run(eng, d, path=0, reset=False):
    eng.set_path(path)
    if reset:
        eng.reset_speculation()
    eng.mi_all_pairs(d["blocks"], SR_DIST, d["retain"], MIH.lr_links_approx(d["POS"], d["g"], SR_DIST))
    return eng.links(0), eng.links(1), eng.block_stats()


def same(x, y, what):
    for w in (0, 1):
        assert len(x[w][2]) == len(y[w][2]), (what, w, len(x[w][2]), len(y[w][2]))
        for u, v in zip(x[w], y[w]):
            assert np.array_equal(u, v), (what, w)
    for k in ("n_lr_total", "n_lr_kept", "n_sr"):
        assert np.array_equal(x[2][k], y[2][k]), (what, k)
    assert np.array_equal(x[2]["disc_thresh"], y[2]["disc_thresh"], equal_nan=True), what


def reports(eng):
    out = {}
    for name, rep in (("counters", eng.counters()), ("path", eng.path_report()), ("overflow", eng.overflow_report())):
        out.update({f"{name}.{k}": v for k, v in rep.items() if isinstance(v, int) and not isinstance(v, bool)})
    return out


@pytest.fixture(scope="module")
def problems(sample):
    A = {k: sample[k] for k in ("states", "hdw", "r", "uqe", "POS", "paint", "g")}
    A.update(blocks=MIH.make_blocks(1268, 500), retain=1e5)
    st = np.ascontiguousarray(sample["states"][:500, ::10])
    with Engine(0) as eng:
        eng.set_alignment(st)
        uqe = (eng.state_counts() > 0).T.astype(np.float64)
        hdw = eng.hamming_weights(50)
    B = dict(states=st, hdw=hdw, r=uqe.sum(axis=1), uqe=uqe, POS=sample["POS"][:500], paint=sample["paint"][:500], g=sample["g"],
             blocks=MIH.make_blocks(500, 200), retain=2e4)
    assert st.shape == (500, 40) and len(A["blocks"]) == 6 and len(B["blocks"]) == 6
    rng = np.random.default_rng(11)
    shift = 7 if int(A["POS"].max()) + 7 <= A["g"] else -1
    return dict(A=A, B=B, A_w2=dict(A, hdw=np.ascontiguousarray(A["hdw"][::-1])),            # other weights: the same ones, sequence by sequence reversed
                A_shift=dict(A, POS=(A["POS"] + shift).astype(np.int32)),                     # other positions, still ascending
                A_perm=dict(A, POS=np.ascontiguousarray(A["POS"][rng.permutation(1268)])))    # ... and in no order


@pytest.fixture(scope="module")
def fresh(problems):
    """(tables, apx_info, what the reports counted) of a fresh context's first pass on a problem, computed once per (problem, path)."""
    memo = {}

    def get(name, path=0):
        if (name, path) not in memo:
            with Engine(0) as eng:
                load(eng, problems[name])
                zero = reports(eng)
                assert not any(zero.values()), zero
                memo[name, path] = (run(eng, problems[name], path), eng.apx_info(), reports(eng))
        return memo[name, path]
    return get


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("reset", [True, False])
def test_a_then_b_then_a_on_one_context(problems, fresh, path, reset):
    with Engine(0) as eng:
        for step, name in enumerate("ABA"):
            load(eng, problems[name])
            got = run(eng, problems[name], path, reset)
            assert len(got[0][2]) > 0 and len(got[1][2]) > 0
            same(fresh(name, path)[0], got, (name, step, path, reset))


def test_new_weights_alone(problems, fresh):
    with Engine(0) as eng:
        load(eng, problems["A"])
        first = run(eng, problems["A"])
        eng.set_weights(problems["A_w2"]["hdw"])
        want = fresh("A_w2")
        assert eng.apx_info() == want[1]
        got = run(eng, problems["A_w2"])
        same(want[0], got, "weights alone")
        assert not np.array_equal(first[1][2], got[1][2])        # (they ARE other weights)


@pytest.mark.parametrize("other", ["A_shift", "A_perm"])
def test_new_snp_meta_alone(problems, fresh, other):
    with Engine(0) as eng:
        load(eng, problems["A"])
        run(eng, problems["A"])
        d = problems[other]
        eng.set_snp_meta(d["r"], d["uqe"], d["POS"], d["paint"], d["g"])
        same(fresh(other)[0], run(eng, d), other)


def test_new_alignment_alone_drops_weights_and_meta(problems, fresh):
    A = problems["A"]
    with Engine(0) as eng:
        load(eng, A)
        run(eng, A)
        eng.set_alignment(A["states"])
        with pytest.raises(L.LdwError) as e:
            run(eng, A)
        assert e.value.code == L.LDW_ERR_STATE and NO_INPUT in str(e.value)
        assert eng.path_report()["apx_gate"] == "weights not set"
        eng.set_weights(A["hdw"])
        eng.set_snp_meta(A["r"], A["uqe"], A["POS"], A["paint"], A["g"])
        same(fresh("A")[0], run(eng, A), "weights and meta again")


@pytest.mark.parametrize("path", [0, 1])
def test_reports_count_a_pass_after_reset_as_a_first_pass(problems, fresh, path):
    with Engine(0) as eng:
        load(eng, problems["A"])
        run(eng, problems["A"], path)
        before = reports(eng)
        run(eng, problems["A"], path, reset=True)
        after = reports(eng)
        assert {k: after[k] - before[k] for k in after} == fresh("A", path)[2]

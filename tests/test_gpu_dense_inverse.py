"""The dense inverse of the coarsest multigrid operator (csrc/amg_dense.hip) held to a long-double truth, shape by shape, through
femshell_amg_device_dense_inverse, and the product that applies it (k_dense_gemv_big) through femshell_amg_dense_apply.

The shapes (tests/helpers/dense_truth.py SHAPES) are the smallest at which each mechanism of the kernel family first exists; the
matrices, the truth and the plain-double restatement of the method are proven on the CPU in tests/test_dense_truth_cpu.py.
Bound of every accuracy check: err(device) <= 4 x max(err(restatement), n 2^-53) against the truth of the same matrix.  On the
graded family (b) the restatement is the method's own block structure in plain double, and cond(pivot block) 2^-53 stands beside
it (tests/helpers/dense_truth.py case): measured on an MI355X, the device is 509 x, 888 x, 62 x, 3560 x, 213 x,
7.7 x and 2.5 x above 4 x the SCALAR restatement at 1, 11, 21, 22, 32, 64 and 86 nodes (1.3e-7 against 9.3e-12 at 22 nodes) --
what explicitly formed pivot-block inverses cost, reproduced by the block restatement on the CPU -- and inside it at 128 and 171."""
import numpy as np
import pytest

from tests.helpers import dense_truth as dt
from tests.helpers import residual_truth
from tests.helpers.product import ensure_built, pkg

pytestmark = pytest.mark.gpu

KNOBS = ("FEMSHELL_AMG_DENSE_LOOKAHEAD", "FEMSHELL_AMG_DENSE_XCD_MAP", "FEMSHELL_AMG_DENSE_PANEL_SPLIT", "FEMSHELL_AMG_DENSE_TILE")
_device = {}  # the default build's FP64 inverse per case, computed once per module


@pytest.fixture(scope="module")
def fs():
    ensure_built()
    ctx = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _inverse(fs, c, **kw):
    return fs.amg_device_dense_inverse(*c["bcsr"], **kw)


def _default(fs, fam, which):
    key = (fam, which)
    if key not in _device:
        _device[key] = _inverse(fs, dt.case(fam, which))
    return _device[key]


def _host_dropped(c):
    import importlib

    H = importlib.import_module("fem-shell_amd.binding").amg_host_dense_inverse(*c["bcsr"])
    return int((np.diag(H) == 0.0).sum())


@pytest.mark.parametrize("fam,which", dt.ACCURACY_CASES, ids=["%s-%s" % k for k in dt.ACCURACY_CASES])
def test_inverse_against_the_long_double_truth(fs, fam, which):
    c = dt.case(fam, which)
    X, st = _default(fs, fam, which)
    e = dt.err(X, c["truth"])
    print("%s-%s n=%d n_pad=%d cond %.1e device %.2e restated %.2e block-restated %.2e lapack %.2e bound %.2e ratio %.2f"
          % (fam, which, c["n"], dt.n_pad(c["n"]), c["cond"], e, c["e_restated"], c["e_block"], c["e_lapack"], c["bound"], e / c["bound"]))
    assert st["n"] == c["n"] and st["dropped_directions"] == 0
    np.testing.assert_array_equal(X, X.T)
    assert e <= c["bound"], (e, c["bound"])


@pytest.mark.parametrize("nodes,dead", dt.PLANTED_CASES, ids=["%d-%s" % (n, "_".join(map(str, d))) for n, d in dt.PLANTED_CASES])
def test_planted_dead_directions(fs, nodes, dead):
    c = dt.case("d", (nodes, dead))
    X, st = _inverse(fs, c)
    e = dt.err(X, c["truth"])
    print("planted %d %s: device %.2e restated %.2e bound %.2e dropped %d" % (nodes, dead, e, c["e_restated"], c["bound"], st["dropped_directions"]))
    assert st["n"] == c["n"] and st["dropped_directions"] == len(dead) == _host_dropped(c)
    assert not X[list(dead), :].any() and not X[:, list(dead)].any()  # exactly zero
    np.testing.assert_array_equal(X, X.T)
    assert e <= c["bound"], (e, c["bound"])


@pytest.mark.parametrize("p", [70, 200])
@pytest.mark.parametrize("rel", [1e-9, 1e-13])
def test_verdict_either_side_of_the_drop_threshold(fs, p, rel):
    A = dt.near_threshold(43, p, rel)
    _, dropped, failed = dt.restated_inverse(A)
    assert failed is None and dropped == ([] if rel == 1e-9 else [p])
    X, st = fs.amg_device_dense_inverse(*dt.to_block_csr(A))
    assert st["dropped_directions"] == len(dropped)
    assert (X[p, p] == 0.0) == bool(dropped) and (not X[p, :].any()) == bool(dropped)


@pytest.mark.parametrize("lookahead", ["1", "0"])
@pytest.mark.parametrize("p", [70, 200])  # the failing pivot in sweep 0, and in a later sweep (its block comes from the look-ahead's stream)
def test_breakdown_is_an_error_return_and_the_context_goes_on(fs, monkeypatch, p, lookahead):
    import importlib

    binding = importlib.import_module("fem-shell_amd.binding")
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_LOOKAHEAD", lookahead)
    for A in (dt.clearly_negative(43, p), dt.zero_diagonal(43, p)):
        assert dt.restated_inverse(A)[2] == p
        bcsr = dt.to_block_csr(A)
        for call in (lambda: fs.amg_device_dense_inverse(*bcsr), lambda: binding.amg_host_dense_inverse(*bcsr)):
            with pytest.raises(pkg.FemShellError) as e:
                call()
            assert e.value.code == dt.BREAKDOWN, str(e.value)
        c = dt.case("a", 22)  # two sweeps: the look-ahead's counters and the second stream are in use again
        X, st = _inverse(fs, c)
        assert st["dropped_directions"] == 0 and dt.err(X, c["truth"]) <= c["bound"]


@pytest.mark.parametrize("fam,nodes", [("a", 22), ("b", 22), ("a", 86), ("b", 86), ("b", 171)])
def test_variants_that_only_redistribute_work_give_the_same_bits(fs, monkeypatch, fam, nodes):
    c = dt.case(fam, nodes)
    X0, _ = _default(fs, fam, nodes)
    for knob in KNOBS[:3]:
        monkeypatch.setenv(knob, "0")
        X, st = _inverse(fs, c)
        monkeypatch.delenv(knob)
        assert st["n"] == c["n"]
        np.testing.assert_array_equal(X, X0, err_msg=knob + "=0")
    # the trailing update on 128 x 128 tiles is another kernel (sixteen matrix-core tiles per wave): held to the truth (measured:
    # the default's bits at these shapes, which nothing promises)
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_TILE", "128")
    X, _ = _inverse(fs, c)
    monkeypatch.delenv("FEMSHELL_AMG_DENSE_TILE")
    e = dt.err(X, c["truth"])
    print("%s-%d tile 128: %.2e bound %.2e bits equal to the default: %s" % (fam, nodes, e, c["bound"], np.array_equal(X, X0)))
    np.testing.assert_array_equal(X, X.T)
    assert e <= c["bound"], (e, c["bound"])
    # stored in single precision: the FP64 result rounded once
    X32, _ = _inverse(fs, c, single_precision=True)
    np.testing.assert_array_equal(X32, X0.astype(np.float32).astype(np.float64))


def _n_pad6(nodes):
    return 6 * ((nodes + 31) // 32 * 32)  # a level's vectors are padded to whole slices of 32 nodes


# loop edges of k_dense_gemv_big (n / 2 pairs per row, 64 lanes, four pairs in flight per lane: the main loop needs lane + 192 < n / 2):
# 1, 21: tail only, lanes idle; 22: the tail's second round; 64: n / 2 = 192, the main loop never entered; 65: three lanes enter it;
# 86, 171: main loop and tail
@pytest.mark.parametrize("as_float", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("nodes", [1, 21, 22, 64, 65, 86, 171])
def test_dense_product_row_by_row(fs, nodes, as_float):
    n, n_pad6 = 6 * nodes, _n_pad6(nodes)
    rng = np.random.default_rng(77 + nodes)
    inv = rng.standard_normal((n, n)) * np.exp(rng.uniform(-3.0, 3.0, size=(n, n)))  # mixed signs, six decades
    b = rng.standard_normal(n)
    stored = inv.astype(np.float32).astype(np.float64) if as_float else inv
    prefill = np.full(n_pad6 + 8, np.nan)
    sentinels = rng.standard_normal(8)
    prefill[n_pad6:] = sentinels
    y = fs.amg_dense_apply(inv, b, n_pad6, as_float=as_float, y_prefill=prefill)
    LD = dt.LD
    truth = stored.astype(LD) @ b.astype(LD)
    budget = residual_truth.gamma(n + 2) * (np.abs(stored).astype(LD) @ np.abs(b).astype(LD))
    worst = float((np.abs(y[:n].astype(LD) - truth) / budget).max())
    print("gemv nodes %d %s: worst error / budget %.3f" % (nodes, "float" if as_float else "double", worst))
    assert worst <= 1.0
    assert np.array_equal(y[n:n_pad6], np.zeros(n_pad6 - n)), "rows [n, n_pad6) are zero"
    np.testing.assert_array_equal(y[n_pad6:], sentinels)

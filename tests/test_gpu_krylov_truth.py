"""The Krylov loops launch by launch: the two-stage reduction, the scalar phases, the vector kernels with their fused dot
products, and the loops themselves (cg_classic, cg_single_reduction, the flexible PCG of cg_amg) through the probes
femshell_cg_reduce and femshell_krylov_set / _launch / _get (csrc/api_krylov_probe.cpp), held to tests/helpers/krylov_truth.py.
Every tolerance is a derived bound (dot_bound, axpy_bound, the block-Jacobi readers' bound, the product's) or bitwise equality;
the truth, the restatement of the scalar phases and the planted defects these assertions catch are pinned on the CPU in
tests/test_krylov_truth_cpu.py.  The checks live in tests/helpers/krylov_cases.py, which tools/krylov_truth_report.py runs too
(profiles/krylov_steps_vs_exact.txt: how much of each bound the intact code uses).

What the chains prove: every probe-chained loop is, bit for bit, the x and the history of solve(rtol = 0, max_it = k) on the same
context -- the probes exercise the production sequence and not one beside it.

First run on an MI355X (profiles/krylov_steps_vs_exact.txt): no bug.  The reduction gives reduce_model's bits at every length
and uses at most 0.10 of its bound (n = 7); the updates use up to 0.995 of u (|result| + |alpha p|), which is as sharp as a
bound of two roundings gets, the block-Jacobi applications 0.25 of the readers' bound, the dots and the fused p.Kp at most 0.19
of theirs; all 80 chains are the solve bit for bit, with FEMSHELL_AMG_FUSE 0 and 3 alike; the crossings found lay between two
polls in eleven of fourteen solves (up to 63 iterations of no-ops behind the flag) and the iterate did not move."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import krylov_cases as kc
from tests.helpers import krylov_truth as kt
from tests.helpers.product import ROOT, ensure_built, pkg

pytestmark = pytest.mark.gpu

INVALID = -1  # include/femshell.h
CHILD_TIMEOUT = 600
P = kt.PHASES


@pytest.fixture(scope="module")
def bare():
    """a context without a mesh: all femshell_cg_reduce needs"""
    ensure_built()
    ctx = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    yield ctx
    ctx.close()


def storage(monkeypatch, symmetric, local="1"):
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", symmetric)
    monkeypatch.setenv("FEMSHELL_SPMV_LOCAL", local)
    return symmetric == "1"


# ------------------------------------------------------------------ (a) the reduction

@pytest.mark.parametrize("n", kt.REDUCE_LENGTHS)
def test_reduction_of_integers_one_hots_random_and_cancelling_words(bare, n):
    """Both group counts of k_cg_scalar (1 below 4096 partial sums, 64 from there on) at every length where the chunks change
    shape.  Integer words: red is the exact integer, and a lost or doubled word is named by the difference.  One word of 1.0 at
    both sides of every chunk boundary: 1.0.  Random and cancelling words: within gamma_len sum |.|, the bits of reduce_model,
    the same bits four times over, and the ticket back at zero behind every launch.  The probe's scalars are kept from call to
    call, so every launch starts from the ticket and the stage-1 sums the last one left, as the launches of a solve do."""
    rng = np.random.default_rng(n)
    for nsums in (1, 2, 3):
        for len3 in sorted({1, max(n // 2, 1), n}) if nsums == 3 else (0,):
            arrays = [kt.integer_partials(n), kt.integer_partials(n) + float(n), 3.0 * kt.integer_partials(len3)][:nsums]
            red, ticket = bare.cg_reduce(np.concatenate(arrays), n, nsums, len3)
            assert ticket == 0
            for a in range(3):
                if a < nsums:
                    kt.assert_reduction_exact(red[a], arrays[a], "n %d nsums %d len3 %d array %d" % (n, nsums, len3, a))
                else:
                    assert np.isnan(red[a])  # nobody wrote it
    for i in kt.chunk_edges(n):
        red, ticket = bare.cg_reduce(kt.one_hot(n, i), n)
        assert (red[0], ticket) == (1.0, 0), (n, i, red[0], ticket)
    worst = 0.0
    for name, p in (("random", kt.random_partials(rng, n)), ("cancelling", kt.cancelling(rng, n))):
        first = None
        for _ in range(4):
            red, ticket = bare.cg_reduce(p, n)
            assert ticket == 0
            first = red[0] if first is None else first
            assert kt.bits(red[0]) == kt.bits(first), "%s n %d: another launch, other bits" % (name, n)
        worst = max(worst, kt.assert_reduction_within(first, p, "%s n %d" % (name, n)))
        assert kt.bits(first) == kt.bits(kt.reduce_model(p)), "%s n %d: %r is not the model's %r" % (name, n, first, kt.reduce_model(p))
    print("reduction n %d (%d groups): largest share of the bound %.3f" % (n, kt.reduce_groups(n), worst))


def test_reduction_refuses_lengths_out_of_range(bare):
    for args in ((np.zeros(1), 0, 1, 0), (np.zeros(4), 2, 0, 0), (np.zeros(8), 2, 4, 0), (np.zeros(5), 2, 3, 0), (np.zeros(7), 2, 3, 3)):
        with pytest.raises(pkg.FemShellError) as e:
            pkg.binding._check(bare._L.femshell_cg_reduce(bare._h, args[1], args[2], args[3], pkg.binding._d(args[0]), pkg.binding._d(np.zeros(3)),
                                                          ctypes.byref(ctypes.c_uint32())))
        assert e.value.code == INVALID


# ------------------------------------------------------------------ (b) the scalar phases

NSUMS = {"none": 1, "init": 2, "alpha": 1, "beta": 2, "restart": 2, "fused_init": 3, "fused_step": 3, "flex_init": 1, "flex_rz0": 1,
         "flex_conv": 2, "flex_beta": 2, "flex_restart": 1, "flex_warm": 1}
BASE = dict(rz=3.7, alpha=0.61, beta=0.23, rr=1.9, bb=41.3, tol2=0.77, iters=2, done=0, red=[11.0, 12.0, 13.0],
            ring_rz=[3.7, 99.0], ring_alpha=[0.61, 98.0], pass_xx=0.0, pass_rhs_rr=0.0, pass_rtol=1e-8)
HIST_CAP, HIST_WORDS = 4, 8


@pytest.fixture(scope="module")
def small():
    ensure_built()
    fs = kc.context(pkg, "n33")
    yield fs
    fs.close()


def run_phase(fs, phase, scalars, red, rtol, gate=-1, cap=HIST_CAP):
    """one scalar_step launch of `phase` on the given scalars, red[] arriving through the partial sums (one word and zeros: the
    sum is that word); returns what the restatement says it must be"""
    G = fs.krylov_grid()
    nsums = NSUMS[phase]
    part = np.zeros(4 * G)
    for a in range(nsums):
        part[a * G] = red[a]
    s_in = kt.Scalars(**scalars)
    fs.krylov_set("partials", part)
    kc.set_scalars(fs, s_in)
    fs.krylov_set("history", np.full(HIST_WORDS, -7.0))
    fs.krylov_set("history_cap", cap)
    raw = kc.raw_scalars(fs)
    fs.krylov_launch("scalar_step", nsums, P[phase], 0, G if nsums == 3 else 0, gate, rtol=rtol)
    got, hist = kc.get_scalars(fs), fs.krylov_get("history", HIST_WORDS)
    label = "%s rtol %g gate %d red %r %r" % (phase, rtol, gate, list(red), {k: v for k, v in scalars.items() if BASE.get(k) != v})
    want, want_hist = s_in.copy(), np.full(HIST_WORDS, -7.0)
    if kt.gated(P[phase] if gate < 0 else gate, s_in.done):
        assert kc.raw_scalars(fs) == raw, label + ": a gated launch wrote the scalars"
    else:
        want.red[:nsums] = red[:nsums]
        kt.scalar_phase(P[phase], want, rtol, want_hist, cap)
        assert fs.krylov_get("scalars").ticket == 0
    kt.assert_scalars_equal(got, want, label)
    assert np.array_equal(kt.bits(hist), kt.bits(want_hist)), (label, hist, want_hist)


def test_every_scalar_phase_is_the_restatement_bit_for_bit(small):
    """Ordinary values; red zero, negative and NaN; r.r == tol2 exactly; the iteration count at the history cap, one below and one
    above; pass_xx / pass_rhs_rr zero and positive with a drop below, inside and above the clamps -- every variation through every
    phase, with rtol zero and positive: output scalars and history words equal scalar_phase bit for bit."""
    reds = [(2.3, 0.77000000000000013, 5.1), (2.3, 0.77, 5.1), (0.77, 2.3, 5.1), (0.0, 0.5, 5.1), (2.3, 0.0, 5.1), (2.3, 0.5, 0.0), (0.0, 0.0, 0.0),
            (-2.3, 0.5, 5.1), (2.3, -0.5, 5.1), (2.3, 0.5, -5.1), (np.nan, 0.5, 5.1), (2.3, np.nan, 5.1), (2.3, 0.5, np.nan),
            (2.3, 0.5, 1.3), (1e-300, 1e300, 1e-300), (np.inf, 0.5, 5.1)]
    variations = [{}] + [{"iters": HIST_CAP + d} for d in (-2, -1, 0, 1)] + [{"rz": 0.0}, {"alpha": 0.0}, {"bb": 0.0}, {"tol2": 0.0}]
    # a refinement pass: drop = 0.2 rtol sqrt(xx / ee) with ee = red[1]
    variations += [{"pass_xx": xx, "pass_rhs_rr": rhs, "pass_rtol": 1e-8} for xx, rhs in ((1.0, 0.0), (0.0, 3.3), (1.0, 3.3), (1e12, 3.3), (1e15, 3.3), (1e10, 3.3))]
    count = 0
    for phase in P:
        for var in variations:
            for red in reds:
                for rtol in (0.0, 1e-3):
                    run_phase(small, phase, dict(BASE, **var), red, rtol)
                    count += 1
    # the three clamp regimes were really there
    tol2 = set()
    for xx in (1.0, 1e12, 1e15, 1e10):
        s = kt.scalar_phase(kt.FLEX_CONV, kt.Scalars(**dict(BASE, pass_xx=xx, pass_rhs_rr=3.3, red=[2.3, 0.5, 0])), 0.0)
        tol2.add(float(s.tol2))
    assert {1e-6 * 1e-6 * 3.3, 1e-2 * 1e-2 * 3.3} < tol2 and len(tol2) == 4
    print("%d launches equal the restatement bit for bit" % count)


def test_the_gate_rule_launch_by_launch(small):
    """done in {0, 1, -1} crossed with every phase and every gate_phase: a gated launch leaves every word of the scalars and of
    the history untouched, any other is the restatement"""
    count = 0
    for phase in P:
        for done in (0, 1, -1):
            for gate in [-1] + sorted(P.values()):
                run_phase(small, phase, dict(BASE, done=done), (2.3, 0.5, 5.1), 1e-3, gate)
                count += 1
    print("%d launches" % count)


@pytest.mark.parametrize("symmetric", ["1", "0"])
def test_the_folded_step_is_fused_step_and_a_plain_update(monkeypatch, symmetric):
    """launch_cgcg_update(step = 0 / 1) against CG_PHASE_FUSED_STEP followed by launch_cgcg_update(step = -1) on the same inputs,
    both parities; ordinary sums, a converged and a broken step: the same alpha / beta / done / r.r / iterations / history, the
    ring's other half receives what the phase keeps in rz / alpha (and is left alone by a step that ends the solve), the half
    that was read stays, and the vectors and partial sums are those of the plain update with those scalars."""
    storage(monkeypatch, symmetric)
    fs = kc.context(pkg, "curved")
    G = fs.krylov_grid()
    rng = np.random.default_rng(5)
    b0 = fs.krylov_get("b")
    for par in (0, 1):
        for red in ((2.3, 0.9, 51.0), (2.3, 0.5, 51.0), (2.3, 0.9, 1.0), (2.3, 0.9, np.nan)):
            ring_rz, ring_alpha = [99.0, 99.0], [98.0, 98.0]
            ring_rz[par], ring_alpha[par] = 3.7, 0.61
            scal = dict(BASE, red=list(red), ring_rz=ring_rz, ring_alpha=ring_alpha)
            vec = kc.fill(fs, rng, **scal)
            fs.krylov_set("history", np.full(HIST_WORDS, -7.0))
            fs.krylov_set("history_cap", HIST_CAP)
            fs.krylov_launch("cgcg_update", par, 0)
            folded = kc.snapshot(fs)
            s_folded = kc.get_scalars(fs)
            # the restatement
            want = kt.Scalars(**scal)
            want_hist = np.full(HIST_WORDS, -7.0)
            kt.folded_step(want, par, want_hist, HIST_CAP)
            kt.assert_scalars_equal(s_folded, want, "folded step %d red %r" % (par, red))
            assert np.array_equal(kt.bits(fs.krylov_get("history", HIST_WORDS)), kt.bits(want_hist))
            # the phase and the plain update
            for k, a in vec.items():
                fs.krylov_set(k, a)
            part = np.full(4 * G, np.nan)
            part[:3 * G] = 0.0
            part[0], part[G], part[2 * G] = red
            fs.krylov_set("partials", part)
            kc.set_scalars(fs, kt.Scalars(**scal))
            fs.krylov_set("history", np.full(HIST_WORDS, -7.0))
            fs.krylov_set("history_cap", HIST_CAP)
            fs.krylov_launch("scalar_step", 3, P["fused_step"], G, G, -1)
            s_phase = kc.get_scalars(fs)
            fs.krylov_set("partials", np.full(4 * G, np.nan))
            fs.krylov_launch("cgcg_update", -1, 0)
            plain = kc.snapshot(fs)
            kt.assert_scalars_equal(s_folded, s_phase, "folded step %d against the phase, red %r" % (par, red), fields=kt.SCALAR_FIELDS + ("red",))
            kc.assert_untouched(plain, folded, "folded step %d red %r" % (par, red), but=("scalars",))
            if s_phase.done == 0:
                assert (s_folded.ring_rz[par ^ 1], s_folded.ring_alpha[par ^ 1]) == (s_phase.rz, s_phase.alpha)
                assert not np.array_equal(plain["x"], vec["x"])
            else:
                assert (s_folded.ring_rz[par ^ 1], s_folded.ring_alpha[par ^ 1]) == (99.0, 98.0)
                assert np.array_equal(plain["x"], vec["x"])  # the update behind a step that ended the solve is a no-op
            assert (s_folded.ring_rz[par], s_folded.ring_alpha[par]) == (3.7, 0.61)
    fs.krylov_set("b", b0)
    fs.close()


# ------------------------------------------------------------------ (c) the vector kernels, their partial sums, the fused product dot, the gates

SETTINGS = [("1", "1"), ("1", "0"), ("0", "1")]  # (FEMSHELL_SYMMETRIC, FEMSHELL_SPMV_LOCAL: the in-slice products on and off)


def report(out):
    used = {k: v for k, v in out.items() if v > 0.0}
    worst = max(used, key=used.get) if used else None
    print("%d checks, %d of them bitwise; largest share of a bound %.3f (%s)" % (len(out), len(out) - len(used), used.get(worst, 0.0), worst))
    assert all(v <= 1.0 for v in out.values())


@pytest.mark.parametrize("symmetric,local", SETTINGS)
@pytest.mark.parametrize("name", kc.MESHES)
def test_vector_steps_products_and_gates(monkeypatch, name, symmetric, local):
    """Every step of femshell_krylov_launch on one mesh under one storage.  Output vectors entry by entry against the long-double
    restatement (copies and zero fills bitwise) -- on symmetric storage also with the gather inside the update kernels, as
    production runs them; the fsum of each partial-sum array against exact_dot of the device's own output
    vectors (small integers: exactly, where no M^-1 is involved); the fused p.Kp against exact_dot(x, K x) of the exported matrix
    with the product's own bound on top, from p and from z, gather deferred or not, x on every dof or on the free ones; with done
    = 1 or -1 in the scalars every gated step leaves every word untouched."""
    sym = storage(monkeypatch, symmetric, local)
    fs = kc.context(pkg, name)
    out = {}
    out.update(kc.check_vector_steps(fs))
    if sym:
        out.update(kc.check_gathered_updates(fs))
    out.update(kc.check_product(fs, sym))
    out.update(kc.check_gating(fs, sym))
    fs.close()
    report(out)


def test_more_slices_than_workgroups(tmp_path):
    """FEMSHELL_SLICE_GRID=8 on the panel's 76 slices, both storages, in a child process (the cap is read once per process): a
    workgroup walks ten slices, and the classic chain is still the solve"""
    for symmetric in ("1", "0"):
        out = str(tmp_path / ("walk%s.npz" % symmetric))
        env = dict(os.environ, FEMSHELL_SLICE_GRID="8", FEMSHELL_SYMMETRIC=symmetric)
        r = subprocess.run([sys.executable, "-m", "tests.helpers.krylov_cases", out, "panel49"], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
        print(r.stdout[-2000:])
        assert r.returncode == 0, r.stdout[-3000:]
        got = {k: float(v) for k, v in np.load(out).items()}
        assert got.pop("panel49: grid") == 8.0
        report(got)


@pytest.mark.parametrize("symmetric", ["1", "0"])
@pytest.mark.parametrize("name", ["curved", "panel49", "strip", "mixed"])
def test_flexible_update_with_the_start_of_the_smoothing(monkeypatch, name, symmetric):
    """launch_pcg_update_start and the cycle as the recurrence issues it, on the meshes whose hierarchy has two levels or more
    (n33 is the exception: its 33 nodes are fewer than a coarsest level holds, its hierarchy has one level, cg_amg never takes the
    fused update there and the step refuses)."""
    sym = storage(monkeypatch, symmetric)
    fs = kc.context(pkg, name, pc="amg", refine_passes=0)
    assert len(fs.amg_levels()) >= 2
    out = kc.check_flexible_update_start(fs, sym)
    out.update(kc.check_pc_apply(fs))
    out.update(kc.check_gating(fs, sym, amg=True))
    fs.close()
    report(out)


# ------------------------------------------------------------------ (d) chained probes are the solve

@pytest.mark.parametrize("symmetric", ["1", "0"])
@pytest.mark.parametrize("name", ["curved", "panel49"])
def test_chained_probes_are_the_block_jacobi_solves(monkeypatch, name, symmetric):
    """k = 1, 2, 9, 17 iterations of the classic recurrence and of the single-reduction recurrence, folded and FEMSHELL_CG_FOLD=0"""
    sym = storage(monkeypatch, symmetric)
    fs = kc.context(pkg, name)
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "0")
    out = kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_classic(fs, k, sym), "classic")
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "1")
    for fold in ("1", "0"):
        monkeypatch.setenv("FEMSHELL_CG_FOLD", fold)
        out.update(kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_single_reduction(fs, k, sym, fold == "1"), "single reduction fold " + fold))
    fs.close()
    assert len(out) == 12


@pytest.mark.parametrize("fuse", ["0", "3"])
@pytest.mark.parametrize("symmetric", ["1", "0"])
@pytest.mark.parametrize("name", ["curved", "panel49"])
def test_chained_probes_are_the_multigrid_solve(monkeypatch, name, symmetric, fuse):
    """The flexible recurrence around pc_apply without refinement passes.  FEMSHELL_AMG_FUSE=0: pc_apply and the in-solve cycle are
    the same launches; 3 (the default): the update kernel takes the first step of the pre-smoothing, and the probes chain that too."""
    sym = storage(monkeypatch, symmetric)
    monkeypatch.setenv("FEMSHELL_AMG_FUSE", fuse)
    fs = kc.context(pkg, name, pc="amg", refine_passes=0)
    fused = fuse == "3" and len(fs.amg_levels()) > 1
    out = kc.assert_chain_is_the_solve(fs, lambda k: kc.chain_flexible(fs, k, sym, fused), "flexible fuse " + fuse)
    fs.close()
    assert len(out) == 4


# ------------------------------------------------------------------ (e) the flag is the stopping point

POLLS_CG = {8, 24, 56, 120, 184, 248, 312, 376, 440, 504, 568, 632, 696, 760, 824, 888, 952}  # DonePoll: 8, then steps of 16, 32, 64, 64 ...


def on_a_poll(method, k):
    return (k in POLLS_CG) if method != "amg" else (k in (1, 3) or (k >= 7 and (k - 7) % 4 == 0))  # AmgPoll: 1, 3, 7, 11, ...


@pytest.mark.parametrize("method", ["classic", "single", "amg"])
def test_the_converged_iterate_is_the_iterate_at_the_crossing(monkeypatch, method):
    """The host polls the done flag at a cadence of 8 rising to 64 iterations (multigrid: 1 rising to 4) and relies on every
    later kernel being a no-op.  Two meshes, rtol 1e-6 and 1e-10: len(history) == iterations; every entry but the last above
    rtol, the last at or below it (residual_history is sqrt(r.r / b.b)); history[-1] == rel_residual bitwise; and the returned x is bit for bit the x of
    solve(rtol = 0, max_it = iterations): nothing ran between the crossing and the poll that found it.  Where the four solves
    leave it open, a further tolerance is taken from the history so that one crossing falls on a poll and one between two."""
    storage(monkeypatch, "1")
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "1" if method == "single" else "0")
    seen = {}

    def crossing(fs, name, rtol):
        u, info = fs.solve(rtol=rtol, max_it=5000)
        h = fs.residual_history()
        k = info["iterations"]
        assert info["converged"] == 1 and len(h) == k > 0
        # (residual_history hands out sqrt(r.r / b.b) of the words in HBM.  The device compares r.r with fl(fl(rtol^2) b.b); the
        #  quotient, its root and that threshold carry four roundings between them, so an entry within 4 ulp of rtol could sit
        #  on either side: the comparison leaves that much)
        assert (h[:-1] > rtol * (1 - 2.0 ** -50)).all() and h[-1] <= rtol * (1 + 2.0 ** -50), (h[-3:], rtol)
        assert h[-1] == info["rel_residual"]
        u0, info0 = fs.solve(rtol=0.0, max_it=k)
        h0 = fs.residual_history()
        assert info0["iterations"] == k and info0["converged"] == 0
        assert np.array_equal(kt.bits(h), kt.bits(h0)), "the history of the converged solve is not that of the solve cut at its crossing"
        assert np.array_equal(kt.bits(u), kt.bits(u0)), "%s %s rtol %g: x moved between the crossing (iteration %d) and the poll" % (name, method, rtol, k)
        seen[(name, rtol)] = (k, on_a_poll(method, k))
        print("%s %s rtol %.3e: %d iterations, %s a poll" % (name, method, rtol, k, "on" if on_a_poll(method, k) else "between"))
        return h

    for name in ("curved", "strip"):
        fs = kc.context(pkg, name, pc="amg", refine_passes=0) if method == "amg" else kc.context(pkg, name)
        for rtol in (1e-6, 1e-10):
            h = crossing(fs, name, rtol)
        # a tolerance between two entries of the history puts the crossing at a chosen iteration: one on a poll, one off
        for want_on in (True, False):
            if not any(on == want_on for k, on in seen.values()):
                k = next(k for k in range(2, len(h)) if on_a_poll(method, k) == want_on and h[k - 1] < h[k - 2] and (h[:k - 1] > h[k - 1]).all())
                crossing(fs, name, float(np.sqrt(h[k - 1] * h[k - 2])))
        fs.close()
    assert any(on for k, on in seen.values()) and any(not on for k, on in seen.values()), seen


# ------------------------------------------------------------------ (f) two ranks on one GPU

FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
RANK_WORKER = os.path.join(ROOT, "tests", "helpers", "krylov_rank_worker.py")


def run_two_ranks(tmp_path, symmetric):
    """two processes on the one GPU behind the shared-memory stand-in for librccl, as tests/test_multirank_gpu.py runs its ranks"""
    subprocess.check_call(["make", "-C", FAKE_DIR, "-s"])
    env = dict(os.environ, FEMSHELL_RCCL_LIB=os.path.join(FAKE_DIR, "libfake_rccl.so"), FEMSHELL_HALO_OVERLAP="1", FEMSHELL_SYMMETRIC=symmetric)
    uid = str(tmp_path / ("uid%s.npy" % symmetric))
    outs = [str(tmp_path / ("rank%d_%s.npz" % (r, symmetric))) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, RANK_WORKER, str(r), "2", uid, outs[r]], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, "\n".join("--- rank %d\n%s" % (q, logs[q][-1500:]) for q in range(2)))
    return [dict(np.load(o)) for o in outs]


@pytest.mark.parametrize("symmetric", ["1", "0"])
def test_two_ranks_reduce_over_the_owned_rows_once(tmp_path, monkeypatch, symmetric):
    """The start and one probe-chained iteration of the single-reduction recurrence and the two dots of the flexible one on two
    ranks.  The all-reduced red[] is the same word on both ranks and equals the exact dot over the OWNED rows of the global vectors
    within dot_bound -- a ghost row counted by the rank that holds a copy of it would double its term; the fused z.Kz of the split
    product, interior slices beside the halo exchange and boundary slices behind it, against exact_dot(z, K z) of the whole
    matrix with the product's bound on top; and the product reports gi + gb partial sums, the grids of its two spans."""
    ensure_built()
    sym = storage(monkeypatch, symmetric)
    ranks = run_two_ranks(tmp_path, symmetric)
    xyz, tri, quad, dmask, loads, mat = kc.mesh("curved")
    n = len(xyz)
    own = [r["own"] for r in ranks]
    assert sorted(np.concatenate(own).tolist()) == list(range(n))
    whole = lambda key: sum(r[key] * np.isin(np.arange(n), o)[:, None] for r, o in zip(ranks, own))  # noqa: E731
    for r, o in zip(ranks, own):
        for key in ("init_r", "step_x", "step_q"):  # a rank hands out its owned rows and nothing else
            assert not r[key][np.setdiff1d(np.arange(n), o)].any()
    ref = kc.context(pkg, "curved")
    K = ref.export_bsr()[:3]
    ref.close()
    shares = {}
    for tag in ("init", "step"):
        assert np.array_equal(kt.bits(ranks[0][tag + "_red"]), kt.bits(ranks[1][tag + "_red"])) and int(ranks[0][tag + "_done"]) == 0
        red = ranks[0][tag + "_red"]
        r_, z_ = whole(tag + "_r"), whole(tag + "_z")
        shares[tag + " r.z"] = kt.assert_dot([red[0]], r_, z_, tag + " r.z")
        shares[tag + " r.r"] = kt.assert_dot([red[1]], r_, r_, tag + " r.r")
        truth, extra = kt.fused_dot_truth(K, z_)
        shares[tag + " z.Kz"] = kt.assert_dot([red[2]], z_, z_, tag + " z.Kz", truth=truth, bound=extra)
    # the whole w = K z of the iteration against the exact product, row by row, whoever owns the row
    z_ = whole("step_z")
    Kz = -kt.rt.exact(K, np.zeros(6 * n), z_.reshape(-1))
    bound = kt.rt.gamma(6.0 * kt.rt.blocks_per_row(K)) * kt.rt.scale(K, np.zeros(6 * n), z_.reshape(-1)) + kt.U * np.abs(Kz)
    shares["step K z"] = kt.within(whole("step_q").reshape(-1), Kz.astype(kt.LD), bound)
    for a, (name, vec) in enumerate((("x.x", whole("step_x")), ("r.r", whole("step_r")))):
        assert ranks[0]["two_dots"][a] == ranks[1]["two_dots"][a]
        shares["two_dots " + name] = kt.assert_dot([ranks[0]["two_dots"][a]], vec, vec, "two_dots " + name)
    # the lengths: the interior span's grid and the boundary span's
    for rank, r in enumerate(ranks):
        plan = pkg.build_plan(xyz, tri, quad, rank=rank, world_size=2)
        ni, nb = plan["n_interior_slices"], plan["n_slices"] - plan["n_interior_slices"]
        G = int(r["G"])
        want = sum(min(8 * ((c + 7) // 8), G) for c in (ni, nb) if c > 0)
        assert int(r["len3_init"]) == int(r["len3_step"]) == want and 0 < want <= 2 * G, (rank, ni, nb, G, int(r["len3_init"]), want)
    assert sym == (symmetric == "1")
    report(shares)


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_context_as_it_was():
    ensure_built()
    xyz, tri, quad, dmask, loads, mat = kc.mesh("n33")
    ctx = pkg.FemShell(*mat, device=0)
    x = np.zeros((len(xyz), 6))

    def refused(call):
        with pytest.raises(pkg.FemShellError) as e:
            call()
        assert e.value.code == INVALID, str(e.value)

    assert ctx.krylov_grid() == -1
    ctx.n_nodes = len(xyz)
    for call in (lambda: ctx.krylov_set("x", x), lambda: ctx.krylov_get("x"), lambda: ctx.krylov_launch("cg_init", 0)):
        refused(call)  # no mesh
    ctx.set_mesh(xyz, tri, quad)
    ctx.set_dirichlet(dmask)
    ctx.set_loads(loads)
    for call in (lambda: ctx.krylov_set("x", x), lambda: ctx.krylov_get("x"), lambda: ctx.krylov_launch("cg_init", 0)):
        refused(call)  # no assembled K
    ctx.assemble()
    refused(lambda: ctx.krylov_launch("cg_init", 0))  # K without its block-Jacobi inverse
    u0, info0 = ctx.solve(rtol=1e-10, max_it=2000)
    h0 = ctx.residual_history()
    G = ctx.krylov_grid()
    assert G == 8
    for call in (lambda: ctx.krylov_set("x", np.zeros(5)), lambda: ctx.krylov_set("partials", np.zeros(4 * G + 1)), lambda: ctx.krylov_get("partials", 4 * G + 1),
                 lambda: ctx.krylov_set("scalars", np.zeros(7)), lambda: ctx.krylov_set("history", np.zeros(4097)), lambda: ctx.krylov_get("history", 1),
                 lambda: ctx.krylov_set("history_cap", 1), lambda: ctx.krylov_launch("cg_init", 2), lambda: ctx.krylov_launch("cgcg_update", 2, 0),
                 lambda: ctx.krylov_launch("scalar_step", 4, 1, 0, 0, -1), lambda: ctx.krylov_launch("scalar_step", 1, 13, 0, 0, -1),
                 lambda: ctx.krylov_launch("scalar_step", 3, 6, 2 * G, 1, -1), lambda: ctx.krylov_launch("scalar_step", 1, 2, 2 * G + 1, 0, -1),
                 lambda: ctx.krylov_launch("scalar_step", 3, 6, 0, 0, -1), lambda: ctx.krylov_launch("scalar_step", 1, 2, 0, 0, 13),
                 lambda: ctx.krylov_launch("pcg_update_start", 0), lambda: ctx.krylov_launch("pc_apply", 0), lambda: ctx.krylov_launch("two_dots", 0, 7),
                 lambda: ctx.krylov_launch("cg_init", 0, rtol=-1.0), lambda: ctx.krylov_launch("cg_init", 0, rtol=np.nan),
                 lambda: pkg.binding._check(ctx._L.femshell_krylov_launch(ctx._h, 99, pkg.binding._i(np.zeros(5, np.int32)), 0.0, None, None))):
        refused(call)
    assert np.array_equal(ctx.get_solution(), u0)  # still the solution: nothing was written
    ctx.set_density(1.0)
    ctx.dynamics_begin(1e-3)
    refused(lambda: ctx.krylov_launch("cg_init", 0))  # dynamics is active
    ctx.dynamics_end()
    u1, info1 = ctx.solve(rtol=1e-10, max_it=2000)
    assert np.array_equal(u1, u0) and info1["iterations"] == info0["iterations"] and np.array_equal(ctx.residual_history(), h0)
    # a probe that wrote makes the solution stale (and a written b the right-hand side): the next solve is the first one again
    ctx.krylov_set("b", x)
    ctx.krylov_launch("cg_init", 0)
    with pytest.raises(pkg.FemShellError):
        ctx.get_solution()
    u2, info2 = ctx.solve(rtol=1e-10, max_it=2000)
    assert np.array_equal(u2, u0) and info2["iterations"] == info0["iterations"]
    ctx.close()

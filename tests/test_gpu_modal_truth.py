"""The block kernels of the eigen-solvers one launch at a time (femshell_modal_combine / _residual / _block_jacobi / _mask / _start,
csrc/api_modal_probe.cpp) held to tests/helpers/modal_truth.py: the truths and the derived bounds are described there and pinned,
with their planted defects, by tests/test_modal_truth_cpu.py.

Meshes: 33 nodes in two slices (384 rows: three tiles of the combine kernel; 64 padded nodes, fewer than the 128 residual
workgroups), the 475-node curved patch (480 padded nodes: four per residual workgroup, the last eight workgroups empty; 22.5
tiles; Dirichlet rows), the mixed patch, three strips with a density per section, a 128-node grid whose last residual workgroup
holds a node, and one flat 421 x 421 grid of 177 241 nodes, shared: more than 8192 tiles (the grid-stride trip of
k_block_combine) and 1385 nodes per residual workgroup (the thread-stride trip of k_block_residual).  Partial masks (0x07, 0x15)
and whole nodes (0x3F) are spread over every mesh.

Largest share of each bound used, as measured on an MI355X (printed by every test):
    combine, random coefficients     0.268 (33 nodes, all shapes), 0.347 (475 nodes, the thinner list)
    residual rows                    0.984 .. 0.999 on every mesh -- the bound is sharp: on a rotational dof theta m x is small
                                     beside kx, the error is the one rounding of the difference, and u |r| is reached where
                                     |r| lies just above a power of two
    residual partial sums            0.399 (33 nodes), 0.274 (475), 0.207 (three strips), 0.389 (128), < 0.001 (177 241)
    residual norms, end to end       0.031, 0.060, 0.037, 0.026, < 0.001 in the same order
    block-Jacobi                     0.5225 (475 nodes), 0.5226 (mixed patch; another entry, the same to three digits by
                                     chance), with symmetric and with full storage alike
Selection matrices, the sums in index order, the mask and the start vectors are bit for bit.

The restart path of LOBPCG (modal.cpp drops P and moves W, A W up through the W buffers) is not pinned here: no case restarts.
Counts read on an MI355X from the `restarts` that check_modes of tests/test_gpu_modal.py prints: 0 in every case of that module
(27, 176, 10, 26, 20, 27 iterations; free-free with shift 1e3: 6); 0 too for the free-free 12 x 10 patch with shift 1e3 at tol
1e-9 (8 iterations) and for the 12 x 10 patch with block-Jacobi at tol 1e-9 (227 iterations).  No knob forces it.
"""
import numpy as np
import pytest

from tests.helpers import meshes, sections
from tests.helpers import modal_truth as mt
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()

NU, E, T, RHO = 0.3, 2.1e5, 0.04, 7.8e-3
SECTION_RHO = np.array([7.8e-3, 2.7e-3, 4.4e-3])


def with_partial_masks(dmask):
    """whole nodes, partial patterns and free nodes whatever the mesh brought"""
    dmask = np.array(dmask, dtype=np.uint8)
    dmask[2::11] |= 0x07
    dmask[5::13] |= 0x15
    dmask[7::29] = 0x3F
    dmask[-1] = 0x15  # the last node keeps free dofs
    assert (dmask == 0).any() and (dmask == 0x3F).any()
    return dmask


class Ctx:
    def __init__(self, fs, dmask):
        self.fs, self.dmask, self.n = fs, dmask, fs.n_nodes
        self.n_pad = 32 * ((self.n + 31) // 32)
        self.free = mt.free_dofs(dmask, self.n)


def plain(m, density=True):
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    dmask = with_partial_masks(m.dirichlet_mask())
    fs.set_dirichlet(dmask)
    if density:
        fs.set_density(RHO)
    fs.set_preconditioner("jacobi")
    return Ctx(fs, dmask)


def sectioned(cs, section_rho=None):
    fs = pkg.FemShell(NU, E, T)
    dmask = with_partial_masks(cs.dmask)
    cs.apply(fs, bc=False, loads=False)
    fs.set_dirichlet(dmask)
    if section_rho is not None:
        fs.set_density(0.0, section_rho=section_rho)
    fs.set_preconditioner("jacobi")
    return Ctx(fs, dmask)


def build(name):
    if name == "two_slices":
        c = plain(meshes.structured(10, 2, 0, 0, 1, 1, "t"))
        assert c.n == 33 and c.n_pad == 64
    elif name == "patch":
        c = plain(sections.curved_patch(24, 18))
        assert c.n == 475 and c.n_pad == 480
    elif name == "full_grid":
        c = plain(meshes.structured(15, 7, 0, 0, 2, 1, "t"))
        assert c.n == 128 and c.n_pad == 128
    elif name == "mixed":
        c = sectioned(sections.mixed_patch())
    elif name == "strips":
        c = sectioned(sections.three_strips(), SECTION_RHO)
    else:
        assert name == "large"
        c = plain(meshes.structured(420, 420, 0, 0, 42, 42, "t"))
        assert c.n == 177241
        # what the mesh is there for: a second trip over the tiles of k_block_combine, several of k_block_residual's thread loop
        assert (6 * c.n_pad + 127) // 128 > 8192 and -(-c.n_pad // mt.GRID) > 256
    return c


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name not in made:
            made[name] = build(name)
        return made[name]

    yield get
    for c in made.values():
        c.fs.close()


def block(rng, cols, c):
    """random and non-zero on every row, the constrained dofs included"""
    X = rng.normal(size=(cols, 6 * c.n))
    assert (X != 0.0).all()
    return X


# ------------------------------------------------------------------ 1, 2. combine

def combine_sources(rng, q, c):
    return [block(rng, k, c) if k else None for k in q]


@pytest.mark.parametrize("name", ["two_slices", "patch"])
def test_combine_with_selection_matrices_is_exact(contexts, name):
    c = contexts(name)
    rng = np.random.default_rng(11)
    for q, n_out, extra in mt.COMBINE_SHAPES:
        sources = combine_sources(rng, q, c)
        Cm, pi, k = mt.selection(q, n_out, n_out + extra)
        Y, stray = c.fs.modal_combine(sources, Cm, n_out)
        mt.assert_selection(Y, sources, pi, k, "q %r, n_out %d, ldc %d" % (q, n_out, n_out + extra))
        assert stray == 0, (q, n_out, extra, stray)


def test_combine_takes_a_second_trip_over_the_tiles(contexts):
    c = contexts("large")
    rng = np.random.default_rng(12)
    sources = combine_sources(rng, (2,), c)
    Cm, pi, k = mt.selection((2,), 2, 2)
    Y, stray = c.fs.modal_combine(sources, Cm, 2)
    mt.assert_selection(Y, sources, pi, k, "large")  # (a tile never written reads as NaN)
    assert stray == 0


@pytest.mark.parametrize("name,shapes", [("two_slices", mt.COMBINE_SHAPES), ("patch", mt.COMBINE_SHAPES_THIN)])
def test_combine_with_random_coefficients_meets_the_bound(contexts, name, shapes):
    c = contexts(name)
    rng = np.random.default_rng(13)
    worst = 0.0
    for q, n_out, extra in shapes:
        sources = combine_sources(rng, q, c)
        Cm = rng.normal(size=(sum(q), n_out + extra))
        Y, stray = c.fs.modal_combine(sources, Cm, n_out)
        worst = max(worst, mt.assert_combine(Y, sources, Cm, n_out))
        assert stray == 0, (q, n_out, extra, stray)
        mt.assert_same_bits(c.fs.modal_combine(sources, Cm, n_out)[0], Y, "a second call")
    print("combine %s: largest share of the bound %.3f" % (name, worst))


def test_combine_refuses_what_the_contract_excludes(contexts):
    c = contexts("two_slices")
    S = np.ones((2, 6 * c.n))

    def refused(sources, Cm, n_out):
        with pytest.raises(pkg.FemShellError) as e:
            c.fs.modal_combine(sources, Cm, n_out)
        assert e.value.code == -1, e.value

    refused([None, None], np.zeros((0, 2)), 2)        # no source column
    refused([S], np.ones((2, 65)), 65)                # n_out > 64
    refused([S], np.ones((2, 1)), 0)                  # n_out < 1
    refused([S], np.ones((2, 1)), 2)                  # ldc < n_out
    refused([np.ones((97, 6 * c.n))], np.ones((97, 1)), 1)  # q > 96
    Y, stray = c.fs.modal_combine([S], np.ones((2, 1)), 1)  # ... and the context works on
    assert (Y == 2.0).all() and stray == 0


# ------------------------------------------------------------------ 3. residual

RESIDUAL_CASES = [("two_slices", mt.RESIDUAL_SHAPES), ("patch", mt.RESIDUAL_SHAPES), ("strips", mt.RESIDUAL_SHAPES[1:3]),
                  ("full_grid", mt.RESIDUAL_SHAPES[:2]), ("large", mt.RESIDUAL_SHAPES[:1])]


@pytest.mark.parametrize("name,shapes", RESIDUAL_CASES)
def test_residual_rows_sums_partials_and_norms(contexts, name, shapes):
    c = contexts(name)
    mass = c.fs.lumped_mass().reshape(-1)
    assert (mass > 0.0).all()  # (no free dof of zero mass on these meshes: the m > 0 guard stays untested)
    rng = np.random.default_rng(14)
    shares = np.zeros(3)
    for mb, cols in shapes:
        KX, X = block(rng, mb, c), block(rng, mb, c)
        theta = (1.0 + 0.37 * np.arange(mb)) / mass.mean()  # all distinct; theta m x of the size of kx
        R, norms, partials, stray = c.fs.modal_residual(KX, X, theta, cols)
        assert stray == 0 and R.shape == (len(cols), 6 * c.n)
        shares[0] = max(shares[0], mt.assert_residual_rows(R, KX, X, theta, cols, mass, c.free))
        mt.assert_residual_sums(norms, partials)
        shares[1] = max(shares[1], mt.assert_residual_partials(partials, R, mass, c.free, c.n_pad))
        shares[2] = max(shares[2], mt.assert_residual_norms(norms, KX, X, theta, cols, mass, c.free, c.n_pad))
        again = c.fs.modal_residual(KX, X, theta, cols)
        for a, b, what in zip(again[:3], (R, norms, partials), ("R", "norms", "partials")):
            mt.assert_same_bits(a, b, "a second call, " + what)
    print("residual %s: largest shares of the bounds: rows %.3f, partials %.3f, norms %.3f" % (name, *shares))


# ------------------------------------------------------------------ 4. block-Jacobi

@pytest.mark.parametrize("symmetric", ["default", "0"])
@pytest.mark.parametrize("name", ["patch", "mixed"])
def test_block_jacobi_on_a_block(monkeypatch, name, symmetric):
    if symmetric == "0":
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    c = build(name)
    Dinv = c.fs.block_jacobi_export(level=0)
    rng = np.random.default_rng(15)
    worst = 0.0
    for n in (1, 5, 32):
        R = block(rng, n, c)
        Z, stray = c.fs.modal_block_jacobi(R)
        assert stray == 0
        worst = max(worst, mt.assert_block_jacobi(Z, Dinv, R, c.free))
    print("block-Jacobi %s, FEMSHELL_SYMMETRIC %s: largest share of the bound %.3f" % (name, symmetric, worst))
    c.fs.close()


# ------------------------------------------------------------------ 5. mask

@pytest.mark.parametrize("n", [1, 32])
def test_mask_keeps_the_free_bits_and_zeroes_the_rest(contexts, n):
    c = contexts("two_slices")
    assert (c.dmask == 0).any()  # unconstrained nodes: the kernel's early return
    X = block(np.random.default_rng(16), n, c)
    Y, stray = c.fs.modal_mask(X)
    mt.assert_mask(Y, X, c.free)
    assert stray == 0


# ------------------------------------------------------------------ 6. start vectors

@pytest.mark.parametrize("n_cols", [1, 12, 32, 96])
def test_start_vectors_match_the_restatement_in_any_numbering(monkeypatch, contexts, n_cols):
    c = contexts("patch")
    X, stray = c.fs.modal_start(n_cols)
    mt.assert_start(X, c.free, n_cols)
    assert stray == 0 and (mt.bits(X[:, ~c.free]) == 0).all()
    m = sections.curved_patch(24, 18)
    perm = pkg.reorder_host("morton", m.xyz, m.tri)
    assert (perm != np.arange(c.n)).any()  # the renumbering moves nodes
    monkeypatch.setenv("FEMSHELL_REORDER", "morton")
    other = plain(m)
    Xm, stray = other.fs.modal_start(n_cols)
    other.fs.close()
    mt.assert_same_bits(Xm, X, "Morton order against the plain context")
    assert stray == 0


def test_start_vectors_of_the_large_mesh(contexts):
    c = contexts("large")
    X, stray = c.fs.modal_start(1)
    mt.assert_start(X, c.free, 1)
    assert stray == 0


# ------------------------------------------------------------------ refusals

def test_the_other_probes_refuse_and_leave_the_context_usable(contexts):
    c = contexts("two_slices")
    X = np.ones((2, 6 * c.n))

    def refused(call, *args):
        with pytest.raises(pkg.FemShellError) as e:
            call(*args)
        assert e.value.code == -1, e.value

    refused(c.fs.modal_residual, X, X, np.ones(2), [0, 2])    # a column index outside 0 .. mb - 1
    refused(c.fs.modal_residual, X, X, np.ones(2), [])        # no column
    refused(c.fs.modal_start, 0)
    refused(c.fs.modal_start, 97)
    refused(c.fs.modal_mask, np.ones((97, 6 * c.n)))
    refused(c.fs.modal_block_jacobi, np.ones((97, 6 * c.n)))
    bare = plain(meshes.structured(10, 2, 0, 0, 1, 1, "t"), density=False)
    refused(bare.fs.modal_residual, X, X, np.ones(2), [0])    # no density
    Y, stray = bare.fs.modal_mask(X)                          # ... and the context works on
    mt.assert_mask(Y, X, bare.free)
    bare.fs.close()
    empty = pkg.FemShell(NU, E, T)
    refused(empty.modal_start, 1)                             # no mesh
    empty.close()
    Y, stray = c.fs.modal_mask(X)
    mt.assert_mask(Y, X, c.free)
    assert stray == 0

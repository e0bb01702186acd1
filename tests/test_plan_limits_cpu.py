"""CPU tests of the symbolic plan at the limits of its encodings ("Limits of the plan's encodings"): the chunk
count of a block slot (8 bits: 765 contributions), an element's position in its slice (12 bits: 4095 elements), the LDS
position of a transposed product that stays in its slice (8 bits, 255 = through HBM), and the lines at which the kernels
change their path (the pipelined assembly kernel up to 128 contributions per slot).  Meshes: tests/helpers/meshes.py coil,
clique, many_hubs.  No GPU compute call is made."""
import numpy as np
import pytest

from tests.helpers import meshes
from tests.helpers.product import ensure_built
from tests.test_plan_cpu import _slot_lists_from_items

pkg = ensure_built()

UNSUPPORTED = -7


def most_chunks(plan):
    return int((plan["items"].reshape(-1, 4)[:, 0] >> 24).max())


@pytest.mark.parametrize("v,chunks", [(85, 29), (86, 29), (128, 43), (255, 85), (256, 86), (300, 100)])
def test_a_hub_of_v_triangles(monkeypatch, v, chunks):
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    xyz, tri = meshes.coil(v)
    assert len(xyz) == v + 2 and len(tri) == v
    p = pkg.build_plan(xyz, tri)
    assert p["symmetric"] == 1
    assert int(np.diff(p["pair_ptr"]).max()) == v          # the hub's diagonal slot
    assert most_chunks(p) == chunks == -(-v // 3)
    assert p["max_slice_elems"] == v and p["max_slice_width"] == 3
    assert int(p["in_width"].max()) == v + 1               # every ring node hands the hub a transposed product
    # the same hub numbered first: the same numbers
    q = pkg.build_plan(*meshes.coil(v, hub_last=False))
    assert int(np.diff(q["pair_ptr"]).max()) == v and most_chunks(q) == chunks and q["max_slice_elems"] == v


def test_the_pipelined_kernel_takes_slots_of_128_contributions_and_no_more(monkeypatch):
    monkeypatch.setenv("FEMSHELL_ASM_PIPE", "2")
    assert pkg.build_plan(*meshes.coil(128))["pipe"] == 1
    assert pkg.build_plan(*meshes.coil(129))["pipe"] == 0


def test_765_contributions_are_accepted_and_766_refused(monkeypatch):
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    p = pkg.build_plan(*meshes.coil(765))
    assert most_chunks(p) == 255 and int(np.diff(p["pair_ptr"]).max()) == 765
    assert p["n_multi_round_slices"] == 1
    with pytest.raises(pkg.FemShellError) as ei:
        pkg.build_plan(*meshes.coil(766))
    assert ei.value.code == UNSUPPORTED and "more than 765 contributions" in str(ei.value)
    # a refusal for a limit does not colour the report of an invalid mesh that follows it
    xyz, tri = meshes.coil(10)
    bad = tri.copy()
    bad[0, 0] = 99
    with pytest.raises(pkg.FemShellError) as ei:
        pkg.build_plan(xyz, bad)
    assert ei.value.code == -4


@pytest.mark.parametrize("v,width", [(40, 42), (41, 43), (62, 64), (63, 65)])
def test_full_storage_rows_of_the_hub(monkeypatch, v, width):
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    p = pkg.build_plan(*meshes.coil(v))
    assert p["symmetric"] == 0 and p["max_slice_width"] == width


@pytest.mark.parametrize("m,positions", [(18, 153), (19, 171), (22, 231), (23, 253), (24, 255), (32, 255)])
def test_in_slice_products_of_a_clique_up_to_the_cap_of_255(monkeypatch, m, positions):
    """Every pair of the m <= 32 nodes is a stored block inside the one slice: m (m - 1) / 2 transposed products, of which at
    most 255 get a position in LDS; the others keep 255 and go through HBM like a product that leaves the slice."""
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    xyz, tri = meshes.clique(m, offset_strips=False)
    assert len(xyz) == m
    p = pkg.build_plan(xyz, tri)
    assert p["n_slices"] == 1 and p["stored_blocks"] == m + m * (m - 1) // 2
    li, ll, gat, ins = p["loc_index"], p["loc_list"], p["gat_slots"], p["in_slots"]
    assert int(li[li != 255].max()) + 1 == positions == min(m * (m - 1) // 2, 255)
    listed = ins >= 0
    assert np.count_nonzero(listed) == m * (m - 1) // 2
    in_lds = listed & (ll != 255)
    assert sorted(ll[in_lds].tolist()) == list(range(positions))   # one position each, no gaps
    assert np.all(gat[in_lds] == -1)
    assert np.all(li[ins[in_lds]] == ll[in_lds])                     # the producer writes where the consumer reads
    spilled = listed & (ll == 255)
    assert np.count_nonzero(spilled) == m * (m - 1) // 2 - positions
    assert np.all(gat[spilled] == ins[spilled]) and np.all(gat[spilled] >= 0)
    assert np.all(li[ins[spilled]] == 255)                           # ... and nobody writes to LDS without a reader
    assert np.count_nonzero(li != 255) == positions
    if m in (24, 32):
        assert np.count_nonzero(spilled) > 0


def test_4160_elements_on_one_slice_are_refused():
    xyz, tri = meshes.many_hubs(32, 130)
    assert len(xyz) % 32 == 0 and len(tri) == 4160
    with pytest.raises(pkg.FemShellError) as ei:
        pkg.build_plan(xyz, tri)
    assert ei.value.code == UNSUPPORTED and "more than 4095 elements" in str(ei.value)


@pytest.mark.parametrize("mesh", ["coil300", "clique32", "clique32_strips"])
def test_work_items_of_deep_slots_carry_the_gather_lists(monkeypatch, mesh):
    """The check of test_work_items_of_both_assembly_kernels_carry_the_gather_lists on a slot of 100 chunks and on a slice of
    several rounds: every slot's chunks, in order, are its gather list, and all chunks of a slot sit in one round of 256 (they
    meet in LDS)."""
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    monkeypatch.setenv("FEMSHELL_ASM_PIPE", "0")
    xyz, tri = meshes.coil(300) if mesh == "coil300" else meshes.clique(32, offset_strips=(mesh == "clique32_strips"))
    plan = pkg.build_plan(xyz, tri)
    assert plan["pipe"] == 0
    per_slice = _slot_lists_from_items(plan)
    deepest = 0
    for s, slots in enumerate(per_slice):
        base, width = plan["slice_base"][s], plan["slice_width"][s]
        n_items = plan["item_ptr"][s + 1] - plan["item_ptr"][s]
        seen = 0
        for k in range(width):
            for n in range(32):
                idx = base + k * 32 + n
                want = list(plan["pairs16"][plan["pair_ptr"][idx]:plan["pair_ptr"][idx + 1]])
                if not want:
                    assert k * 32 + n not in slots
                    continue
                chunks = slots[k * 32 + n]
                nch = len(chunks)
                assert sorted(chunks) == list(range(nch)) and all(c[1] == nch for c in chunks.values())
                assert [p for c in range(nch) for p in chunks[c][2]] == [int(v) for v in want]
                assert all(len(chunks[c][2]) == 3 for c in range(nch - 1))  # only the last chunk may be short
                assert len({chunks[c][0] // 256 for c in range(nch)}) == 1    # one round of 256
                deepest = max(deepest, nch)
                seen += 1
                if mesh == "clique32" and k == 0:
                    assert nch == 6                                          # 16 or 17 triangles at every node
        assert seen == len(slots)
        if mesh == "clique32" or (mesh == "clique32_strips" and s == 1):
            assert n_items > 256                                             # several rounds
    assert deepest == {"coil300": 100, "clique32": 6, "clique32_strips": 7}[mesh]  # (strips: two more triangles at node 0)
    if mesh == "clique32":
        assert plan["n_multi_round_slices"] == plan["n_slices"] == 1


@pytest.mark.parametrize("mesh", ["coil300", "quad_petals258", "mixed_petals150", "clique32"])
def test_gather_lists_of_the_limit_meshes_reproduce_the_oracle_matrix(monkeypatch, mesh):
    """The numpy model of the assembly (tests/helpers/sell.py: every slot sums the element blocks of its gather list, a
    constrained diagonal entry is the length of the list) against the oracle, block by block: 1e-12 of the block's largest
    entry, the constrained diagonal -- 300 at the clamped hub -- exactly."""
    from tests.helpers import oracle, sell

    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    quad = np.zeros((0, 4), np.int32)
    tri = np.zeros((0, 3), np.int32)
    if mesh == "coil300":
        xyz, tri = meshes.coil(300)
    elif mesh == "quad_petals258":
        xyz, quad = meshes.quad_petals(258)
    elif mesh == "mixed_petals150":
        xyz, tri, quad = meshes.mixed_petals(150)
    else:
        xyz, tri = meshes.clique(32)
    n = len(xyz)
    dmask = np.zeros(n, np.uint8)
    dmask[::7] = np.random.default_rng(12).integers(1, 64, len(dmask[::7])).astype(np.uint8)
    dmask[n - 1] = 0x15
    mat = oracle.material(0.3, 2.1e5, 0.04)
    rowptr, colidx, vals, _ = oracle.assemble(xyz, tri, quad, mat, dmask, None)
    plan = pkg.build_plan(xyz, tri, quad)
    assert plan["n_own"] == n and plan["n_ghost"] == 0
    dm = np.zeros(plan["n_pad"], np.uint8)
    dm[:n] = dmask
    blocks = sell.assemble_from_plan(plan, mat, oracle, dm)
    assert len(blocks) == len(colidx)
    worst = 0.0
    for row, col, blk in blocks.values():
        q = rowptr[row] + np.searchsorted(colidx[rowptr[row]:rowptr[row + 1]], col)
        assert colidx[q] == col
        scale = np.abs(vals[q]).max()
        assert np.abs(blk - vals[q]).max() <= 1e-12 * scale
        worst = max(worst, np.abs(blk - vals[q]).max() / scale if scale > 0.0 else 0.0)
        if row == col:
            fixed = ((int(dmask[row]) >> np.arange(6)) & 1) == 1
            assert np.array_equal(np.diag(blk)[fixed], np.diag(vals[q])[fixed])
    print("%s: worst block %.2e" % (mesh, worst))
    if mesh == "coil300":
        hub = blocks[[k for k, b in blocks.items() if b[0] == n - 1 and b[1] == n - 1][0]][2]
        assert hub[0, 0] == hub[2, 2] == hub[4, 4] == 300.0

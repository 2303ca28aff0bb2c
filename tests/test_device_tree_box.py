"""The device tree's box (pipamd_device_tree_fits, interface version 500): host only, no GPU.  The shapes today's
device-tree tests run stay in it, in the flavour they run it; 65 ... 128 columns are in it; beyond, it is the host
schedulers'."""
import pytest

from piplib_amd import engine as eng, synth

# shapes (nvar, nparm, ni, nc) of tests/test_gpu_device_tree.py: random families, big parameter, deepest cut,
# unsimplified, tall, mixed; and of its 128-bit families
OLD64 = [(5, 2, 7, 2), (4, 3, 6, 3), (6, 1, 8, 1), (16, 3, 20, 3), (8, 2, 10, 2), (6, 0, 9, 0), (10, 4, 14, 1), (3, 5, 6, 4),
         (30, 2, 45, 2), (50, 3, 40, 2), (28, 1, 44, 1), (5, 3, 7, 2), (6, 1, 70, 1), (10, 2, 90, 2), (8, 0, 100, 0),
         (12, 3, 64, 2), (3, 1, 4, 1)]
OLD128 = [(16, 3, 20, 3), (10, 4, 14, 1), (4, 3, 6, 3), (30, 2, 45, 2), (28, 1, 44, 1)]
WIDE = {401: ((70, 1, 20, 2), 1, dict(cmax=2, nnz=2, pp=0.15)), 402: ((90, 2, 30, 4), 1, dict(cmax=1, nnz=2, pmax=1)),
        403: ((120, 2, 40, 4), 1, dict(cmax=1, nnz=2, pmax=1)), 404: ((100, 0, 50, 0), 1, dict(cmax=3, nnz=3)),
        405: ((80, 2, 24, 4), 0, dict(cmax=2, nnz=2, pmax=1)), 406: ((110, 1, 30, 2), 1, dict(cmax=2, nnz=2, pp=0.15)),
        407: ((75, 1, 80, 2), 1, dict(cmax=2, nnz=2, pp=0.15))}


def _one(nvar, nparm, ni, nc, nq=1):
    return synth.random_problems(1, 1, nvar, nparm, ni, nc, nq)[0]


def _family(seed):
    shape, nq, kw = WIDE[seed]
    return synth.sparse_parametric_problems(seed, 1, *shape, nq, **kw)[0]


def test_interface_version():
    assert eng.ABI_VERSION == 500
    assert eng.lib().pipamd_version() == 500


@pytest.mark.parametrize("shape", OLD64)
def test_todays_shapes_stay_in_the_box(shape):
    assert eng.device_tree_fits(_one(*shape)) == 1
    assert eng.device_tree_fits(_one(*shape, nq=0)) == 1


@pytest.mark.parametrize("shape", OLD128)
def test_todays_128bit_shapes_stay_in_the_box(shape):
    assert eng.device_tree_fits(_one(*shape), 128) == 1


@pytest.mark.parametrize("shape", [(64, 0, 20, 0), (64, 1, 20, 2), (90, 2, 30, 4), (117, 10, 20, 1), (120, 7, 40, 2),
                                   (127, 0, 104, 0), (126, 1, 30, 2)])
def test_65_to_128_columns_in_64_bits(shape):
    assert eng.device_tree_fits(_one(*shape)) == 1


@pytest.mark.parametrize("seed", sorted(WIDE))
def test_wide_families_in_64_bits(seed):
    assert eng.device_tree_fits(_family(seed)) == 1


def test_128_bits_follow_the_lds_rule():
    """a two-block image may take a workgroup's 160 KB: 406 (110 unknowns, 30 inequalities) fits, 407 (80 inequalities)
    does not"""
    for seed in (401, 402, 403, 404, 405, 406):
        assert eng.device_tree_fits(_family(seed), 128) == 1, seed
    assert eng.device_tree_fits(_family(407), 128) == 0


@pytest.mark.parametrize("shape", [(128, 0, 20, 0), (120, 8, 20, 1), (6, 1, 105, 1), (70, 1, 110, 2),
                                   (60, 55, 20, 1)])
def test_outside_the_box(shape):
    """129 columns, more than 104 inequalities, a context wider than one block with its spare columns"""
    assert eng.device_tree_fits(_one(*shape)) == 0
    assert eng.device_tree_fits(_one(*shape), 128) == 0


def test_bad_arguments():
    with pytest.raises(RuntimeError):
        eng.device_tree_fits(_one(5, 2, 7, 2), 32)


def test_edge_members_in_the_box():
    """the members of tests/device_tree_edges.py that sit on a limit of the box: 17 context rows with parameters (CR + 1 == SS
    == 64), 127 and 128 columns, 104 inequalities, 49 parameters, a context of 64 columns with its spare ones"""
    import device_tree_edges as dte
    taken = [dte.member("chain24_new10_nc17"), dte.member("cols127_new1"), dte.widen(dte.chain(0, nnew=1), 128),
             dte.member("cuts24_ni104"), dte.member("wide49_2_0")]
    assert eng.device_tree_fits(_one(11, 53, 20, 1)) == 1  # (nparm + newp + 1 == 64; in 128 bits the LDS rule decides)
    assert [(p.nc, p.nvar + p.nparm + 1, p.ni, p.nparm) for p in taken] == [
        (17, 46, 35, 34), (0, 127, 2, 1), (0, 128, 2, 1), (0, 49, 104, 0), (0, 51, 3, 49)]
    for p in taken:
        assert eng.device_tree_fits(p) == 1 and eng.device_tree_fits(p, 128) == 1
    for name in dte.MEMBERS:  # every member the GPU tests put at a reserve or one past it is given to the device tree
        assert eng.device_tree_fits(dte.member(name)) == 1 and eng.device_tree_fits(dte.member(name), 128) == 1, name


def test_edge_members_outside_the_box():
    """18 context rows with parameters (CR + 1 > SS), 105 inequalities, nparm + newp + 1 > 64 (65 columns, 54 parameters:
    two blocks leave 10 spare columns, the context would have 65)"""
    import device_tree_edges as dte
    out = [dte.chain(24, nnew=10, nc=18), dte.cuts(24, 81), dte.cuts(25, 80), _one(10, 54, 20, 1)]
    assert (out[0].nc, out[1].ni, out[2].ni) == (18, 105, 105)
    for p in out:
        assert eng.device_tree_fits(p) == 0 and eng.device_tree_fits(p, 128) == 0
    assert eng.device_tree_fits(dte.chain(0, nc=18, idle=20)) == 0  # (no fork or cut needed: the shape alone decides)
    assert eng.device_tree_fits(dte.chain(0, nc=17, idle=20)) == 1

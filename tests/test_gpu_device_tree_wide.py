"""-m gpu: the device-resident traiter() on problems of 65 ... 128 columns (two column blocks per wave,
pip_quast_kernel<QI, 2> of piplib_amd/csrc/pip_quast.hip).

The families are wide and sparse (synth.sparse_parametric_problems: many unknowns, few parameters, the shape of polyhedral
callers), screened with the CPU oracle.  Every problem's tape text and pivot count must be the oracle's, with the device
tree on and off; the share the device tree served is pinned per family (the measured share, rounded down to a tenth)."""
import os
import subprocess

import numpy as np
import pytest

import pipbatch as pb

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# seed: (shape (nvar, nparm, ni, nc), nq, generator arguments); 60 problems each
FAMILIES = {
    401: ((70, 1, 20, 2), 1, dict(cmax=2, nnz=2, pp=0.15)),
    402: ((90, 2, 30, 4), 1, dict(cmax=1, nnz=2, pmax=1)),
    403: ((120, 2, 40, 4), 1, dict(cmax=1, nnz=2, pmax=1)),
    404: ((100, 0, 50, 0), 1, dict(cmax=3, nnz=3)),
    405: ((80, 2, 24, 4), 0, dict(cmax=2, nnz=2, pmax=1)),
    406: ((110, 1, 30, 2), 1, dict(cmax=2, nnz=2, pp=0.15)),
    407: ((75, 1, 80, 2), 1, dict(cmax=2, nnz=2, pp=0.15)),
}
# share of the problems the oracle finishes that the device tree served, measured on an MI355X, rounded down to a tenth
# (404, no parameters, 50 inequalities: 8 of 60 need more than the 24 cut rows reserved and are handed back)
SHARE64 = {401: 1.0, 402: 1.0, 403: 1.0, 404: 0.8, 405: 1.0, 406: 1.0, 407: 1.0}
SHARE128 = {401: 1.0, 402: 1.0, 403: 1.0, 404: 0.8, 405: 1.0, 406: 1.0}


def _family(seed, count=60):
    from piplib_amd import synth
    shape, nq, kw = FAMILIES[seed]
    return synth.sparse_parametric_problems(seed, count, *shape, nq, **kw)


def _screen(probs, limit=3000, flags=0, exe=None):
    """(problem, oracle result) for the problems the CPU oracle (exe: the 64-bit one, or pb.ORACLEPIP128) finishes quickly"""
    keep = []
    for p in probs:
        try:
            r = pb.run_batch(exe or pb.ORACLEPIP, [p], flags, timeout=3).results[0]
        except subprocess.TimeoutExpired:
            continue
        if r.pivots <= limit:
            keep.append((p, r))
    return keep


def _same(keep, got):
    for (p, r), (text, rc, st, piv) in zip(keep, got):
        if r.status == pb.ST_ABORT:
            assert rc == -5, (rc, st)
            continue
        assert rc == 0, (rc, st)
        assert pb.squash(text) == pb.squash("void\n" if r.status == pb.ST_VOID else r.text)
        assert piv == r.pivots, (piv, r.pivots)


def _run(e, probs, bits, deepest=False):
    from piplib_amd import engine as eng
    if bits == 128:
        return eng.solve_tableaux_lockstep128(e, probs, deepest_cut=deepest)
    return eng.solve_tableaux(e, probs, lockstep=True, deepest_cut=deepest)


def _check(keep, share, bits=64, deepest=False):
    """keep against the oracle through the lock-step entry of `bits`, device tree on, then off; (served, handed back)"""
    from piplib_amd import engine as eng
    e = eng.Engine(0)
    probs = [p for p, _ in keep]
    got = _run(e, probs, bits, deepest)
    served, back = e.last_device_tree()
    assert served + back == sum(eng.device_tree_fits(p, bits) for p in probs), (served, back)
    _same(keep, got)
    done = sum(r.status != pb.ST_ABORT for _, r in keep)
    assert served >= share * done, (served, back, done)
    e.set_device_tree(False)  # the forest / tree alone: same answers, entry by entry
    assert _run(e, probs, bits, deepest) == got
    assert e.last_device_tree() == (0, 0)
    return served, back


@pytest.mark.parametrize("seed", sorted(FAMILIES))
def test_wide_families_vs_oracle(seed):
    """65 ... 121 columns, integer and rational, with and without parameters and context, 20 ... 80 inequalities"""
    from piplib_amd import engine as eng
    keep = _screen(_family(seed))
    assert len(keep) >= 16
    assert all(eng.device_tree_fits(p) == 1 for p, _ in keep)
    _check(keep, SHARE64[seed])


@pytest.mark.parametrize("seed", [401, 406])
def test_wide_deepest_cut_vs_oracle(seed):
    keep = _screen(_family(seed), flags=pb.F_DEEPEST)
    assert len(keep) >= 40
    _check(keep, 0.5, deepest=True)


@pytest.mark.parametrize("seed", [401, 402, 403, 404, 405, 406])
def test_wide_families_128bit_vs_oracle128(seed):
    """the overflow-safe flavour: its two-block instantiation against the 128-bit oracle"""
    from piplib_amd import engine as eng
    keep = _screen(_family(seed), exe=pb.ORACLEPIP128)
    assert len(keep) >= 16
    assert all(eng.device_tree_fits(p, 128) == 1 for p, _ in keep)
    _check(keep, SHARE128[seed], bits=128)


def test_wide_tall_128bit_family_is_not_taken():
    """407's image (80 inequalities, 128-bit entries) does not fit a workgroup's LDS: straight to the host schedulers"""
    from piplib_amd import engine as eng
    keep = _screen(_family(407, 20), exe=pb.ORACLEPIP128)
    assert len(keep) >= 10
    assert all(eng.device_tree_fits(p, 128) == 0 for p, _ in keep)
    served, back = _check(keep, 0.0, bits=128)
    assert (served, back) == (0, 0)


def test_wide_compute_dual_device_tree_vs_host_tree():
    """Compute_dual (TRAITER_DUAL, rational) on family 405 (80 unknowns, 2 parameters): same cells and pivot count as the
    host tree, served on the device"""
    from piplib_amd import engine as eng
    e_dev, e_host = eng.Engine(0), eng.Engine(0)
    e_host.set_device_tree(False)
    served = compared = 0
    for p in _family(405, 40):
        try:
            want = eng.traiter(e_host, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, eng.T_DUAL, p.ineq, p.ctx)
        except eng.SolverError:
            with pytest.raises(eng.SolverError):
                eng.traiter(e_dev, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, eng.T_DUAL, p.ineq, p.ctx)
            continue
        got = eng.traiter(e_dev, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, eng.T_DUAL, p.ineq, p.ctx)
        served += e_dev.last_device_tree()[0]
        assert got == want
        compared += 1
    assert compared >= 30 and served >= 0.9 * compared, (compared, served)


def _cols(seed, ncol, count=12, nparm=0, ni=24, nc=0, pp=0.15):
    from piplib_amd import synth
    return synth.sparse_parametric_problems(seed, count, ncol - 1 - nparm, nparm, ni, nc, 1, cmax=2, nnz=2, pp=pp)


@pytest.mark.parametrize("ncol", [64, 65, 118, 128])
def test_column_boundaries_served(ncol):
    """no new parameter needed (no parameters): 64 columns on one block, 65, 118 and 128 on two -- served"""
    from piplib_amd import engine as eng
    keep = _screen(_cols(420 + ncol, ncol))
    assert len(keep) >= 10
    assert all(eng.device_tree_fits(p) == 1 for p, _ in keep)
    served, back = _check(keep, 0.9)
    assert back == 0, (served, back)


def test_128_columns_with_a_parametric_cut_are_handed_back():
    """128 columns leave no spare column for a new parameter: a problem that needs one is handed back, answered right"""
    from piplib_amd import engine as eng
    keep = [(p, r) for p, r in _screen(_cols(431, 128, count=40, nparm=1, nc=2, pp=0.3)) if "newparm" in r.text]
    assert len(keep) >= 3
    e = eng.Engine(0)
    for p, r in keep:
        assert eng.device_tree_fits(p) == 1
        got = eng.solve_tableaux(e, [p], lockstep=True)
        assert e.last_device_tree() == (0, 1)
        _same([(p, r)], got)


def test_129_columns_are_not_tried():
    from piplib_amd import engine as eng
    keep = _screen(_cols(432, 129))
    assert len(keep) >= 10
    assert all(eng.device_tree_fits(p) == 0 for p, _ in keep)
    served, back = _check(keep, 0.0)
    assert (served, back) == (0, 0)


def test_narrow_and_wide_in_one_call():
    """narrow and wide problems in one call: answers in input order; the narrow ones served as in a call of their own"""
    from piplib_amd import engine as eng, synth
    narrow = _screen(synth.random_problems(141, 60, 5, 2, 7, 2, 1))
    wide = _screen(_family(401, 30))
    e = eng.Engine(0)
    _run(e, [p for p, _ in narrow], 64)
    alone_narrow = e.last_device_tree()
    _run(e, [p for p, _ in wide], 64)
    alone_wide = e.last_device_tree()
    both = narrow + wide
    order = np.random.default_rng(9).permutation(len(both))
    keep = [both[i] for i in order]
    got = _run(e, [p for p, _ in keep], 64)
    _same(keep, got)
    served, back = e.last_device_tree()
    assert (served, back) == (alone_narrow[0] + alone_wide[0], alone_narrow[1] + alone_wide[1])
    assert alone_narrow[0] >= 0.9 * len(narrow) and alone_wide[0] >= 0.5 * len(wide)


def test_one_problem_entries_on_a_wide_problem():
    """pipamd_traiter, pipamd_solve_tableau and their 128-bit counterparts serve a wide problem on the device"""
    from piplib_amd import engine as eng
    keep = [(p, r) for p, r in _screen(_family(401, 20)) if r.status == pb.ST_OK and "newparm" in r.text]
    p, r = keep[0]
    e = eng.Engine(0)
    for bits in (64, 128):
        text, piv = eng.solve_tableau(e, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, p.nq, p.ineq, p.ctx, bits=bits)
        assert e.last_device_tree()[0] == 1, bits
        assert pb.squash(text) == pb.squash(r.text) and piv == r.pivots
        eng.traiter(e, p.nvar, p.nparm, p.ni, p.nc, p.bigparm, eng.T_INT, p.ineq, p.ctx, bits=bits)
        assert e.last_device_tree()[0] == 1, bits


def _dat_text(probs):
    out = []
    for k, p in enumerate(probs):
        rows = lambda m: "".join("#[ " + " ".join(str(int(x)) for x in row) + " ]\n" for row in m)
        out.append(f"(\n( wide problem {k} )\n{p.nvar} {p.nparm} {p.ni} {p.nc} {p.bigparm} {p.nq}\n(\n{rows(p.ineq)})\n(\n{rows(p.ctx)})\n)\n")
    return "".join(out)


@pytest.mark.skipif(not pb.have_ref_gpu(), reason="oracle/_ref/refpip_gpu not built (no /root/reference)")
def test_wide_dat_through_the_reference_front_end(tmp_path):
    """the reference's own front end (tab_get, tape, sol_edit) with its traiter() on the GPU, on wide problems, against
    the reference's CPU build"""
    if not pb.have_ref():
        pytest.skip("oracle/_ref/refpip not built")
    keep = _screen(_family(401, 12)) + _screen(_family(406, 12))
    path = tmp_path / "wide.dat"
    path.write_text(_dat_text([p for p, r in keep if r.status != pb.ST_ABORT]))
    want = subprocess.run([pb.REFPIP, "dat", str(path)], capture_output=True, timeout=300)
    got = subprocess.run([pb.REFPIP_GPU, "dat", str(path)], capture_output=True, timeout=300)
    assert want.returncode == 0 and got.returncode == 0, got.stderr.decode()[-300:]
    assert "newparm" in want.stdout.decode("latin-1")
    assert pb.squash(got.stdout.decode("latin-1")) == pb.squash(want.stdout.decode("latin-1"))

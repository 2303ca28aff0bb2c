"""The wave-level steps of the device tree (piplib_amd/csrc/pip_quast.hip) -- classify_rows, sort_rows (and
sort_rows_tall), pivot_step, make_cut, deepen, find_quotient, build_sub, solve_plain -- each against Python ints
(tests/quast_step_model.py) on small tableaux aimed at their edges (tests/quast_step_cases.py).

pipamd_debug_quast_step (piplib_amd/csrc/pip_probe.hip) stages a case's image in LDS, calls the SHIPPED function of
QK<QI, NB> and writes back every word it can touch.  What a case owes follows its class at the instantiation's width:
`fits` -- every output word equals the model; `must` -- the return carries Q_WHY_OVERFLOW (the image may be half
rewritten); `may` -- either of the two.  One launch per function group and instantiation.  tests/test_quast_step_cases.py
(no GPU) checks the lists: classes per width, the cap on `may`, a fits and a must case per edge, the 64-bit list within the
128-bit one, the model against bigint_pip where they overlap.
"""
import ctypes as C
import time

import numpy as np
import pytest

import quast_step_cases as qc
import quast_step_model as qm

pytestmark = pytest.mark.gpu

INSTS = [(0, 64, 1), (1, 64, 2), (2, 128, 1), (3, 128, 2)]   # inst, entry bits, column blocks: QK<long long / __int128, NB>
E_INVALID = -1


class Probe:
    """the wrapper of pipamd_debug_quast_step: no public API, only what eng.lib() gives"""

    def __init__(self):
        import torch
        from piplib_amd import engine as eng
        self.torch = torch
        self.L = eng.lib()
        self.L.pipamd_debug_quast_step.restype = C.c_int
        self.L.pipamd_debug_quast_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int]
        self.e = eng.Engine(0)

    def launch(self, inst, blobs, nouts, fill=0, pad=2):
        """the cases' blobs in one call; returns (rc, out words, the cases' offsets into out)"""
        t = self.torch
        n = len(blobs)
        oin, oout, pos, opos = [], [], 2 + 2 * n, 0
        for b, no in zip(blobs, nouts):
            oin.append(pos)
            pos += len(b)
            oout.append(opos)
            opos += no
        total_out = opos + pad
        words = np.concatenate([np.array([pos, total_out] + oin + oout, dtype=np.uint64)] + list(blobs))
        din = t.from_numpy(words.view(np.int64)).cuda()
        dout = t.full((total_out,), fill, dtype=t.int64, device="cuda")
        assert din.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0
        rc = self.L.pipamd_debug_quast_step(self.e._h, inst, C.c_void_p(din.data_ptr()), pos, C.c_void_p(dout.data_ptr()), total_out, n)
        return rc, dout.cpu().numpy().view(np.uint64), oout

    def run(self, inst, Wb, nb, cases):
        """every case through instantiation `inst`; returns the list of what went wrong, and the classes met"""
        EW = Wb // 64
        outs = [qm.run(c, Wb, nb) for c in cases]
        wants = [qm.pack_out(o, EW) for o in outs]
        for c, w in zip(cases, wants):
            assert len(w) == qm.out_words(c, EW, nb), c.tag
        rc, got, oout = self.launch(inst, [qm.pack_in(c, EW) for c in cases], [len(w) for w in wants])
        assert rc == 0, rc
        wrong, met = [], {"fits": 0, "must": 0, "may": 0}
        for c, o, w, at in zip(cases, outs, wants, oout):
            gk = got[at:at + len(w)]
            ret, aux = int(gk[1].view(np.int64)), int(gk[2])
            flagged = qm.overflow_reported(c, ret, aux)
            met[o.cls] += 1
            if int(gk[0]) != 1:
                wrong.append("%s: status %d" % (c.tag, int(gk[0])))
            elif o.cls == "must":
                if not flagged:
                    wrong.append("%s: an intermediate leaves %d bits, returned %d aux %#x without Q_WHY_OVERFLOW" % (c.tag, Wb, ret, aux))
            elif not np.array_equal(gk, w) and not (o.cls == "may" and flagged):
                d = int(np.nonzero(gk != w)[0][0])
                wrong.append("%s (%s): output word %d is %#x, the model has %#x (returned %d aux %#x, model %d aux %#x)" % (
                    c.tag, o.cls, d, int(gk[d]), int(w[d]), ret, aux, o.ret, o.aux))
        return wrong, met


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.mark.parametrize("inst,Wb,nb", INSTS, ids=["w64-1", "w64-2", "w128-1", "w128-2"])
@pytest.mark.parametrize("name", list(qc.FUNCTIONS))
def test_step_against_python_ints(probe, name, inst, Wb, nb):
    """every case of the function group on QK<QI, NB>, word for word as its class says"""
    cases = qc.cases(name, Wb, nb)
    if nb == 2 and name in qc.ONE_BLOCK:
        assert cases == []   # as shipped: the context's functions and solve_plain run one column block
        return
    assert 10 <= len(cases) <= 400
    t0 = time.time()
    wrong, met = probe.run(inst, Wb, nb, cases)
    print("%s <%d, %d>: %d cases (%s), %.2f s" % (name, Wb, nb, len(cases), met, time.time() - t0))
    assert not wrong, "%d of %d cases:\n%s" % (len(wrong), len(cases), "\n".join(wrong[:20]))


def test_a_malformed_case_is_refused_and_nothing_runs(probe):
    """the host entry checks every index a step forms from the case; a call with one bad case is refused whole"""
    good = qc.cases("pivot_step", 64, 1)[0]
    base = qm.pack_in(good, 1)
    nout = qm.out_words(good, 1, 1)
    rc, got, _ = probe.launch(0, [base], [nout], fill=-7)
    assert rc == 0 and int(got[0]) == 1

    def broken(word, value):
        b = base.copy()
        b[word] = np.uint64(value & qm.M64)
        return b
    H, R = qm.QS_HDR, good.R
    bad = {
        "fn beyond the table": broken(0, 99), "W beyond the column blocks": broken(1, 65), "more slots than the image holds": broken(2, 4096),
        "nvar = ncol": broken(4, good.ncol), "ncol > W": broken(5, good.W + 1), "nligne > R": broken(6, R + 1),
        "bigparm beyond ncol": broken(8, good.ncol), "the pivot row beyond nligne": broken(9, good.nligne),
        "the pivot row a unit row": broken(9, next(k for k in range(R) if good.flag[k] & qm.UNIT)),
        "nparm >= CW": broken(13, good.CW), "nc > CR": broken(12, good.CR + 1), "ldet > MAXDET": broken(17, 5), "a reserved word set": broken(18, 1),
        "a slot beyond S": broken(H + R + good.pivi, good.S), "a unit column beyond nvar": broken(H + R + 2, good.nvar),
        "a flag beyond the six bits": broken(H, 64), "a denominator of 0": broken(H + 2 * R + qm.QS_POS + 4 + good.pivi, 0),
        "a negative denominator": broken(H + 2 * R + qm.QS_POS + 4, -3), "pos beyond a byte": broken(H + 2 * R, 256),
    }
    for why, blob in bad.items():
        rc, got, _ = probe.launch(0, [base, blob], [nout, nout], fill=-7)
        assert rc == E_INVALID, why
        assert (got.view(np.int64) == -7).all(), why   # not even the good case ran
    # an image beyond the dynamic LDS a kernel gets without opting in to more
    big = qc.tableau("too large", qm.QS_PIVOT, 2, 3, [[1, 1, -1]] * 100, None, 64)
    assert big.lds_bytes(128) > qm.LDS_MAX >= big.lds_bytes(64)
    rc, got, _ = probe.launch(2, [qm.pack_in(big, 2)], [qm.out_words(big, 2, 1)], fill=-7)
    assert rc == E_INVALID and (got.view(np.int64) == -7).all()
    # the one-block functions are refused on two blocks, and a truncated buffer anywhere
    fq = qc.cases("find_quotient", 64, 1)[0]
    rc, _, _ = probe.launch(1, [qm.pack_in(fq, 1)], [qm.out_words(fq, 1, 2)])
    assert rc == E_INVALID
    rc, _, _ = probe.launch(0, [base[:-1]], [nout])
    assert rc == E_INVALID
    rc, _, _ = probe.launch(0, [base], [nout], pad=0)
    assert rc == 0
    rc, _, _ = probe.launch(0, [base], [nout - 1], pad=0)
    assert rc == E_INVALID

"""-m gpu: the determinant replay on job headers and logs given here (pipamd_debug_det_replay, csrc/pip_probe.hip) against
tests/replay_model.py -- EVERY output word of every job: the limbs, ldet, the pivot count, the status, nlog.

The three bodies that walk a log -- pip_det_replay_kernel (a wave per job, 64 pairs pre-reduced per pass),
pip_det_replay_lanes_kernel (a lane per job, chunks of 8 or 4 pairs) and the lean kernel's spare blocks' instantiation of
the one-lane walk (chunks of PIP_LEAN_REPLAY_CH) -- at both entry widths, over the cases of tests/replay_cases.py (whose
classes tests/test_replay_cases.py checks on the CPU): log lengths around the chunk and pass sizes up to a full log, the
first overflow at every such place by both causes with pairs behind it that must not be walked, starting limbs at the
first-fit edges, every status (ST_NIL with and without the mark of a last pivot that is counted and not logged), jobs of
the other width and jobs off a list, and two replays in a row on one header."""
import ctypes as C

import numpy as np
import pytest

import replay_cases as rc
import replay_model as rm

pytestmark = pytest.mark.gpu

WHICH = {"wave-per-job": 0, "lane-per-job": 1, "spare-block-lane": 2}


class Probe:
    def __init__(self):
        import torch
        from piplib_amd import engine as eng
        self.torch = torch
        self.L = eng.lib()
        self.fn = self.L.pipamd_debug_det_replay  # exported by libpipamd.so, no part of include/piplib_amd.h
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self.e = eng.Engine(0)

    def run(self, which, bits, words, lst=None):
        """words: (njobs, HDR + LOGWORDS) uint64 -> (njobs, NOUT) uint64"""
        t = self.torch
        n = words.shape[0]
        din = t.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()
        dout = t.full((n, rc.NOUT), -1, dtype=t.int64, device="cuda")
        arr = (C.c_int * len(lst))(*lst) if lst is not None else None
        rc_ = self.fn(self.e._h, which, bits, C.c_void_p(din.data_ptr()), C.c_void_p(dout.data_ptr()), n, arr,
                      len(lst) if lst is not None else 0)
        assert rc_ == 0, rc_
        return dout.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def probe():
    return Probe()


def words_of(jobs):
    return np.array([rc.job_words(c) for c in jobs], dtype=np.uint64)


def differ(got, want, jobs):
    bad = [j for j in range(len(jobs)) if [int(x) for x in got[j]] != want[j]]
    if not bad:
        return None
    j = bad[0]
    c = jobs[j]
    return "%d of %d jobs differ, first: job %d (bits %d, ldet %d, npiv %d, status %d, nlog %d) got %s want %s" % (
        len(bad), len(jobs), j, c["bits"], c["ldet"], c["npiv"], c["status"], len(c["log"]),
        [hex(int(x)) for x in got[j]], [hex(x) for x in want[j]])


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("which", sorted(WHICH))
def test_replay_against_the_model(probe, which, W):
    for l in rc.launches(W):
        got = probe.run(WHICH[which], W, words_of(l["jobs"]), l["list"])
        msg = differ(got, rc.expected(l), l["jobs"])
        assert msg is None, "%s, %d bits, %d jobs, list %s: %s" % (which, W, len(l["jobs"]), l["list"] is not None, msg)


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("which", sorted(WHICH))
def test_two_replays_carry_the_limbs(probe, which, W):
    """log A, then log B on the header the first replay returned: as the model on A + B.  The limbs and ldet cross from
    one launch to the next in the header -- with 128-bit entries as two words a limb"""
    pairs = rc.carry_pairs(W)
    ew = W // 64
    first = probe.run(WHICH[which], W, words_of([a for a, _, _ in pairs]))
    second, want = [], []
    for (a, b, tail), o in zip(pairs, first):
        o = [int(x) for x in o]
        assert o == rc.expected(dict(bits=W, jobs=[a], list=None))[0]  # A alone
        limbs = [sum(o[ew * i + h] << (64 * h) for h in range(ew)) for i in range(4)]
        limbs = [x - (1 << W) if x >> (W - 1) else x for x in limbs]
        nxt = dict(bits=W, limbs=tuple(limbs), ldet=o[8], npiv=o[9] + len(b), status=o[10], aux=a["aux"], log=b, tail=tail)
        assert o[11] == 0
        second.append(nxt)
        whole = rm.replay(a["limbs"], a["ldet"], a["npiv"] + len(b), a["status"], a["log"] + b, W, a["aux"])
        want.append(rc.out_words(nxt, *whole))
    got = probe.run(WHICH[which], W, words_of(second))
    msg = differ(got, want, second)
    assert msg is None, msg


def test_probe_rejects_bad_arguments(probe):
    import torch
    w = torch.from_numpy(words_of(rc.pool(64)[:2]).view(np.int64)).cuda()
    out = torch.zeros((2, rc.NOUT), dtype=torch.int64, device="cuda")
    p, o = C.c_void_p(w.data_ptr()), C.c_void_p(out.data_ptr())
    two = (C.c_int * 2)(0, 2)
    assert probe.fn(None, 0, 64, p, o, 2, None, 0) != 0
    assert probe.fn(probe.e._h, 3, 64, p, o, 2, None, 0) != 0       # no such body
    assert probe.fn(probe.e._h, 0, 96, p, o, 2, None, 0) != 0       # no such width
    assert probe.fn(probe.e._h, 0, 64, None, o, 2, None, 0) != 0
    assert probe.fn(probe.e._h, 0, 64, p, o, 2, two, 2) != 0        # a list entry beyond the jobs
    assert probe.fn(probe.e._h, 0, 64, p, o, 2, two, 3) != 0        # a list longer than the jobs
    bad = words_of(rc.pool(64)[:2])
    bad[1, 11] = rm.DETLOG + 1                                      # more pairs than a log holds
    wb = torch.from_numpy(bad.view(np.int64)).cuda()
    assert probe.fn(probe.e._h, 0, 64, C.c_void_p(wb.data_ptr()), o, 2, None, 0) != 0
    assert probe.fn(probe.e._h, 0, 64, p, o, 0, None, 0) == 0

"""-m gpu: what pipamd_batch_load leaves in the workspace of a batch whose rows stay in the caller's array
(PIPAMD_T_ROWS_STAY, 64-bit entries): nothing of it depends on the rows.

The job headers and the row tables of every tableau are restated here in numpy (load_job_header, load_row_tables of
csrc/pip_kernels.hip over pip_block_layout of csrc/pip_job.h) and compared byte for byte, for the load in one piece and
in parts of 1, 64 and 7 tableaux (pipamd_batch_load_part with a non-zero `first`; the workspace is zeroed first, so that
the bytes no load writes compare too); solve() + fetch() must then give what the copying load gives.

Batches of 1, 63, 64, 65 and 130 tableaux; none of the shapes has pad columns (W == ncol).  (Round 6 tried a launch of
batch / 32 blocks, a wave per eight tableaux, for this load: the block-per-tableau launch takes 19 us for 10,000
tableaux on its own, the other 16 us, and the benchmark could not tell them apart -- DESIGN.md section 5.  This file
pins the bytes for whoever reshapes the load next.)"""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

JOB = np.dtype([("vals_off", "<i8"), ("rows_off", "<i8"), ("sol_off", "<i8"), ("state_off", "<i8"), ("log_off", "<i8"),
                ("nvar", "<i4"), ("nparm", "<i4"), ("ni", "<i4"), ("bigparm", "<i4"), ("tflags", "<i4"),
                ("L", "<i4"), ("S", "<i4"), ("W", "<i4"), ("status", "<i4"), ("aux", "<i4"), ("npiv", "<i4"), ("ncut", "<i4"),
                ("ldet", "<i4"), ("nupd", "<i4"), ("det", "<i8", (8,)), ("maxabs", "<u8"), ("nlog", "<i4"), ("pad_", "<i4"),
                ("state_nch", "<i4"), ("ebits", "<i4"), ("src_rows", "<i8"), ("home_sol_off", "<i8")])  # PipJob, pip_job.h
DETLOG, T_SORT, T_FRESHROWS, F_UNIT, F_UNKNOWN = 512, 256, 4096, 1, 32


def block_layout(nvar, S, W, sol_entries, nm):
    """pip_block_layout (pip_job.h) for 64-bit entries: int64 words from the block's first word"""
    L = (nvar + S + 1) & ~1
    vals = L + L
    sol = vals + S * W
    state = sol + ((sol_entries + 1) & ~1)
    log = state + ((S * nm + (3 * L + 7) // 8 + 1) & ~1)
    return L, vals, sol, state, log, log + 2 * DETLOG


def expected(desc, src_addr):
    """(headers as a JOB array, row tables as (den, flag, ref) per tableau, arena offset in bytes, block words)"""
    B, nvar, ni = desc.batch, desc.nvar, desc.ni
    assert JOB.itemsize == 200 and desc.nparm == 0
    S, W = ni + desc.cap_cuts, (nvar + 1 + 1) & ~1
    L, vals, sol, state, log, words = block_layout(nvar, S, W, nvar + nvar, 2)
    jobs = np.zeros(B, JOB)
    k = np.arange(B, dtype=np.int64)
    jobs["rows_off"] = k * words
    for name, off in (("vals_off", vals), ("sol_off", sol), ("state_off", state), ("log_off", log)):
        jobs[name] = k * words + off
    jobs["nvar"], jobs["ni"], jobs["bigparm"] = nvar, ni, -1
    jobs["tflags"] = (desc.tflags & ~(8192 | T_FRESHROWS)) | T_SORT | T_FRESHROWS
    jobs["L"], jobs["S"], jobs["W"] = L, S, W
    jobs["ldet"], jobs["ebits"] = 1, 64
    jobs["det"][:, 0] = 1
    jobs["src_rows"] = src_addr
    i = np.arange(L)
    den = (i < nvar + ni).astype(np.int64)
    flag = np.where(i < nvar, F_UNIT, np.where(i < nvar + ni, F_UNKNOWN, 0)).astype(np.int32)
    ref = np.where(i < nvar, i, np.where(i < nvar + ni, i - nvar, 0)).astype(np.int32)
    return jobs, (den, flag, ref), (B * 200 + 255) & ~255, words


def parts_of(rows):
    """the batch cut into parts of 1, 64, 7, 1, ... tableaux"""
    out, at, sizes = [], 0, [1, 64, 7]
    while at < rows.shape[0]:
        n = min(sizes[len(out) % 3], rows.shape[0] - at)
        out.append(rows[at:at + n].clone())  # (an array of its own: the headers must point into it)
        at += n
    return out


@pytest.mark.parametrize("cap_cuts", [0, None])
@pytest.mark.parametrize("nvar,ni", [(127, 64), (5, 3), (63, 32)])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 130])
def test_load_rows_stay(batch, nvar, ni, cap_cuts):
    import torch
    from piplib_amd import engine as eng, synth
    rows = torch.as_tensor(synth.lexmin_batch(8100 + batch, batch, nvar, ni)).to("cuda:0")
    ncol = nvar + 1

    def loaded(parts):
        e = eng.Engine(0)
        e.set_max_rows(ni + 1024)
        b = eng.Batch(e, rows, nvar, 0, tflags=eng.T_INT | eng.T_ROWS_STAY, cap_cuts=cap_cuts)
        b.ws.zero_()
        if parts is None:
            b.load()
        else:
            b.load_parts(parts)
        torch.cuda.synchronize()
        return e, b, b.ws.cpu().numpy().copy()

    e, b, ws = loaded(None)
    want_jobs, (den, flag, ref), arena, words = expected(b.desc, rows.data_ptr() + np.arange(batch, dtype=np.int64) * ni * ncol * 8)
    raw = ws.view(np.uint8)
    got_jobs = raw[:batch * 200].view(JOB)
    for name in JOB.names:
        assert (got_jobs[name] == want_jobs[name]).all(), name
    assert got_jobs.tobytes() == want_jobs.tobytes()
    L = int(want_jobs["L"][0])
    for k in range(batch):
        t = raw[arena + 8 * words * k:arena + 8 * words * k + 16 * L]
        assert t[:8 * L].view(np.int64).tobytes() == den.tobytes(), k
        assert t[8 * L:12 * L].view(np.int32).tobytes() == flag.tobytes(), k
        assert t[12 * L:].view(np.int32).tobytes() == ref.tobytes(), k
    # loads in parts: the same workspace but for the headers' pointers, which go into the parts' arrays
    parts = parts_of(rows)
    _, _, wp = loaded(parts)
    addr = np.concatenate([p.data_ptr() + np.arange(p.shape[0], dtype=np.int64) * ni * ncol * 8 for p in parts])
    want_parts = want_jobs.copy()
    want_parts["src_rows"] = addr
    assert wp.view(np.uint8)[:batch * 200].tobytes() == want_parts.tobytes()
    assert wp.view(np.uint8)[arena:].tobytes() == raw[arena:].tobytes()  # the same row tables, nothing else written
    # the solve from the rows that stayed against the solve from copied rows
    b.solve()
    b.fetch()
    e2 = eng.Engine(0)
    e2.set_max_rows(ni + 1024)
    c = eng.Batch(e2, rows, nvar, 0, tflags=eng.T_INT, cap_cuts=cap_cuts)
    c.load()
    c.solve()
    c.fetch()
    torch.cuda.synchronize()
    for x, y in ((b.status, c.status), (b.pivots, c.pivots), (b.cuts, c.cuts)):
        assert torch.equal(x, y)
    done = (c.status == eng.ST_SOLUTION).cpu().numpy()
    assert (b.sol_num.cpu().numpy()[done] == c.sol_num.cpu().numpy()[done]).all()
    assert (b.sol_den.cpu().numpy()[done] == c.sol_den.cpu().numpy()[done]).all()

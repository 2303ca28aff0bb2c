"""ctypes binding of the C ABI (include/piplib_amd.h) for tests and bench.py.

torch is used only for device memory and streams.  There is NO CPU fallback: if
libpipamd.so is missing or no GPU is visible, construction raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PIPAMD_LIB: tuning experiments with an alternative build of the same library (tools/ only)
LIB_PATH = os.environ.get("PIPAMD_LIB") or os.path.join(HERE, "libpipamd.so")

ST_RUN, ST_SOLUTION, ST_NIL, ST_NEED_COMPA, ST_NEED_PARMCUT, ST_OVERFLOW, ST_CAPACITY, ST_RANGE, ST_INTERNAL, ST_MAXCOL = range(10)
ST_BADINPUT = 10  # a system load_matrices(), load_sparse() or load_instances() could not take (PIPAMD_ST_BADINPUT)
T_INT, T_DUAL = 1, 2
T_NOSKIP = 2048
T_ROWS_STAY = 8192  # the rows of Batch.load stay valid until the next solve: no copy pass (include/piplib_amd.h)
SHIFT_MAX, SHIFT_URS = 1, -1  # Batch(shift=...): Maximize / Urs_unknowns (PIPAMD_SHIFT_MAX, PIPAMD_SHIFT_URS)


class BatchDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("batch", "nvar", "nparm", "ni", "bigparm", "tflags", "cap_cuts", "cap_newparm", "entier_bits")]


class System(C.Structure):
    """pipamd_system: the plain system of Batch(system=True) -- rows, equality rows (a host list), shift, simplify"""
    _fields_ = [("nrows", C.c_int32), ("neq", C.c_int32), ("eq_rows", C.POINTER(C.c_int32)), ("shift", C.c_int32),
                ("simplify", C.c_int32)]


class Matrices(C.Structure):
    """pipamd_matrices: the PolyLib matrices of Batch(matrices=True) -- room per system, shift, simplify, and the device
    array of the systems' row counts (NULL: max_rows each)"""
    _fields_ = [("max_rows", C.c_int32), ("shift", C.c_int32), ("simplify", C.c_int32), ("reserved", C.c_int32),
                ("d_nrows", C.c_void_p)]


class Sparse(C.Structure):
    """pipamd_sparse: the plain system of Batch(sparse=True) -- the System, then the entry count and the device arrays of
    row pointers (int64), columns (int32) and values (int64)"""
    _fields_ = [("sys", System), ("nnz", C.c_int64), ("d_row_ptr", C.c_void_p), ("d_cols", C.c_void_p), ("d_vals", C.c_void_p)]


class Instances(C.Structure):
    """pipamd_instances: the plain system of Batch(instances=True) -- the System, then the parameter count of the shared
    matrix and the device arrays of the matrix (nrows x (nvar + nparm + 1) int64) and the points (systems x nparm int64)"""
    _fields_ = [("sys", System), ("nparm", C.c_int32), ("reserved", C.c_int32), ("d_matrix", C.c_void_p), ("d_points", C.c_void_p)]


ABI_VERSION = 500  # include/piplib_amd.h PIPAMD_VERSION
_lib = None


def lib():
    """Load libpipamd.so (built by piplib_amd.build); raises if it is not there."""
    global _lib
    if _lib is None:
        # torch first: its wheel bundles the HIP runtime; loading ours before it would put a
        # second libamdhip64 in the process and torch would then see no GPU.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `python -m piplib_amd.build` (HIP extension is mandatory)")
        L = C.CDLL(LIB_PATH)
        if L.pipamd_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} is interface version {L.pipamd_version()}, this binding is written for "
                               f"{ABI_VERSION} (include/piplib_amd.h PIPAMD_VERSION): rebuild with `python -m piplib_amd.build`")
        L.pipamd_last_error.restype = C.c_char_p
        L.pipamd_batch_workspace_bytes.restype = C.c_size_t
        L.pipamd_batch_workspace_bytes.argtypes = [C.POINTER(BatchDesc)]
        L.pipamd_dense_pivot_bytes.restype = C.c_size_t
        L.pipamd_dense_pivot_bytes.argtypes = [C.POINTER(BatchDesc)]
        L.pipamd_engine_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.pipamd_engine_destroy.argtypes = [C.c_void_p]
        L.pipamd_engine_set_iter_limit.argtypes = [C.c_void_p, C.c_int]
        L.pipamd_engine_set_waves_per_job.argtypes = [C.c_void_p, C.c_int]
        L.pipamd_engine_set_round_pivots.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "pipamd_engine_set_round_rows"):
            L.pipamd_engine_set_round_rows.argtypes = [C.c_void_p, C.c_int]
        L.pipamd_last_solve_launches.argtypes = [C.c_void_p]
        L.pipamd_batch_load.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p, C.c_void_p]
        L.pipamd_batch_solve.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p]
        L.pipamd_batch_solve_async.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p]
        L.pipamd_batch_wait.argtypes = [C.c_void_p]
        L.pipamd_batch_poll.argtypes = [C.c_void_p]
        L.pipamd_batch_load_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p]
        if hasattr(L, "pipamd_batch_dual_part"):  # (Batch.dual_part says so where a PIPAMD_LIB build has none)
            L.pipamd_batch_dual_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.pipamd_batch_results.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc)] + [C.c_void_p] * 6
        L.pipamd_batch_load_shifted_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p, C.c_int,
                                                     C.c_int, C.c_int, C.c_void_p]
        L.pipamd_batch_results_shifted.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_int] + [C.c_void_p] * 6
        L.pipamd_engine_set_lean_big.argtypes = [C.c_void_p, C.c_int]
        L.pipamd_batch_load_system_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(System), C.c_void_p,
                                                    C.c_int, C.c_int, C.c_void_p]
        L.pipamd_batch_dual_system_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(System), C.c_void_p,
                                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pipamd_batch_load_matrices_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Matrices), C.c_void_p,
                                                      C.c_int, C.c_int, C.c_void_p]
        L.pipamd_batch_dual_matrices_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Matrices), C.c_void_p,
                                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "pipamd_batch_load_sparse_part"):  # (added since 500: a PIPAMD_LIB build may be older)
            L.pipamd_batch_load_sparse_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Sparse), C.c_int,
                                                        C.c_int, C.c_void_p]
            L.pipamd_batch_dual_sparse_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Sparse), C.c_int,
                                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "pipamd_batch_load_instances_part"):  # (added since 500: a PIPAMD_LIB build may be older)
            L.pipamd_batch_load_instances_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Instances),
                                                           C.c_int, C.c_int, C.c_void_p]
            L.pipamd_batch_dual_instances_part.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.POINTER(Instances),
                                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pipamd_batch_counters.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BatchDesc), C.c_void_p, C.c_void_p]
        L.pipamd_last_solve_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.pipamd_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"piplib_amd error {rc}: {lib().pipamd_last_error().decode()}")


class Engine:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().pipamd_engine_create(C.byref(self._h), int(device)))
        self.device = int(device)

    def close(self):
        if self._h:
            lib().pipamd_engine_destroy(self._h)
            self._h = C.c_void_p()

    def set_iter_limit(self, n):
        _check(lib().pipamd_engine_set_iter_limit(self._h, int(n)))

    def set_round_pivots(self, n):
        _check(lib().pipamd_engine_set_round_pivots(self._h, int(n)))

    def set_bulk_min(self, n):
        lib().pipamd_engine_set_bulk_min.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_bulk_min(self._h, int(n)))

    def set_device_tree(self, on):
        """pipamd_solve_tableaux_lockstep: try the device-resident traiter() first (default on)"""
        lib().pipamd_engine_set_device_tree.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_device_tree(self._h, int(bool(on))))

    def last_device_tree(self):
        """(problems the device tree finished, problems it handed back) in the last lock-step call"""
        a, b = C.c_int(0), C.c_int(0)
        lib().pipamd_last_device_tree.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _check(lib().pipamd_last_device_tree(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_device_tree_record(self, on):
        """testing aid: keep the device tree's result words of every problem of a call (default off)"""
        lib().pipamd_debug_device_tree_record.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_debug_device_tree_record(self._h, int(bool(on))))

    def debug_device_tree_records(self):
        """testing aid: (n, 6) int32 of the last call's problems, by input index -- result (Q_DONE 0, Q_VOID 1, Q_FALLBACK 2),
        cells, pivots, Q_WHY_* bits, ticks, tape cells written (csrc/pip_quast.h); -1 throughout where the device tree was not
        given the problem.  Recording must be on (debug_device_tree_record)."""
        import numpy as np
        L = lib()
        L.pipamd_debug_device_tree_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        n = L.pipamd_debug_device_tree_records(self._h, None, 0)
        _check(min(n, 0))
        out = np.full((n, 6), -1, np.int32)
        if n:
            _check(min(L.pipamd_debug_device_tree_records(self._h, out.ctypes.data_as(C.c_void_p), n), 0))
        return out

    def set_max_rows(self, rows):
        lib().pipamd_engine_set_max_rows.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_max_rows(self._h, int(rows)))

    def set_blocking_wait(self, on):
        lib().pipamd_engine_set_blocking_wait.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_blocking_wait(self._h, int(bool(on))))

    def set_lone_batches(self, on):
        """this engine's batches run one at a time (pipamd_engine_set_lone_batches)"""
        lib().pipamd_engine_set_lone_batches.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_lone_batches(self._h, int(bool(on))))

    def set_spare_replay(self, on):
        """the second lean launch's spare blocks replay the determinant logs of the finished tableaux (default on;
        pipamd_engine_set_spare_replay)"""
        lib().pipamd_engine_set_spare_replay.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_spare_replay(self._h, int(bool(on))))

    def set_lean2_waves(self, waves):
        """waves per tableau of the second lean launch: 4 (default, where its row capacity has that kernel) or 1
        (pipamd_engine_set_lean2_waves)"""
        lib().pipamd_engine_set_lean2_waves.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_lean2_waves(self._h, int(waves)))

    def set_lean64(self, on):
        """128-bit batches of 129 ... 256 columns start with pip_lean64_kernel (csrc/pip_lean.h; default off)"""
        lib().pipamd_engine_set_lean64.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_lean64(self._h, int(bool(on))))

    def set_lean_big(self, on):
        """bulk batches under a big parameter (Batch(shift=...), or nparm=1, bigparm=nvar + 1) start with the lean kernel's
        big-parameter flavour (csrc/pip_lean.h; default off: include/piplib_amd.h)"""
        _check(lib().pipamd_engine_set_lean_big(self._h, int(bool(on))))

    def set_tail_waves(self, n):
        lib().pipamd_engine_set_tail_waves.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_tail_waves(self._h, int(n)))

    def set_timing(self, on):
        lib().pipamd_engine_set_timing.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_engine_set_timing(self._h, int(bool(on))))

    def set_round_rows(self, n):
        _check(lib().pipamd_engine_set_round_rows(self._h, int(n)))

    def last_launch_ms(self, i):
        """duration of launch i of the last solve (HIP events on its stream; timing must be on)"""
        ms = C.c_float()
        lib().pipamd_last_launch_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        _check(lib().pipamd_last_launch_ms(self._h, int(i), C.byref(ms)))
        return float(ms.value)

    def debug_single_launch(self, on):
        """measurement aid: the next solves stop after their bulk launches (True / 1: the one-wave launches of a large
        batch; 2: after the lean launch alone, when the batch has one; 3: as 1, but without the determinant replay
        behind the launches, for tests that look at the logs) -- unfinished tableaux stay PIPAMD_ST_RUN"""
        lib().pipamd_debug_single_launch.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_debug_single_launch(self._h, int(on)))

    def debug_lean(self, on):
        """measurement / testing aid: bulk launches with (default) or without the lean kernel (csrc/pip_lean.h)"""
        lib().pipamd_debug_lean.argtypes = [C.c_void_p, C.c_int]
        _check(lib().pipamd_debug_lean(self._h, int(bool(on))))

    def last_solve_launches(self):
        return int(lib().pipamd_last_solve_launches(self._h))

    def set_waves_per_job(self, n):
        _check(lib().pipamd_engine_set_waves_per_job(self._h, int(n)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wide_to_int(a):
    """numpy (..., 2) int64 (low, high) pairs -> object array of Python ints (two's complement)."""
    import numpy as np
    lo = a[..., 0].astype(object) & ((1 << 64) - 1)
    hi = a[..., 1].astype(object)
    return hi * (1 << 64) + lo


class Batch:
    """A uniform batch of tableaux resident in HBM (layer 1 of the C ABI)."""

    def __init__(self, engine, rows, nvar, nparm, bigparm=-1, tflags=T_INT, cap_cuts=None, cap_newparm=0,
                 entier_bits=64, shape=None, shift=0, system=False, eq_rows=(), simplify=0, matrices=False, nrows=None, ni=None,
                 sparse=False, instances=False):
        """rows: (batch, ni, ncol) int64, host or device; or None with shape=(batch, ni, ncol) for a workspace whose
        tableaux come from load_parts().
        shift=SHIFT_MAX / SHIFT_URS: the lexicographic maximum / unknowns of either sign (pip_solve's Maximize,
        Urs_unknowns).  rows are then the PLAIN system, nvar + 1 columns (nparm=0): the batch is solved under a big
        parameter (nparm=1, bigparm=nvar + 1, set here), load() / load_part() go through pipamd_batch_load_shifted and
        fetch_shifted() decodes the answer into x_num, x_den.
        system=True: rows are the PLAIN system pip_solve takes, (batch, nrows, nvar + 1), of which the rows listed in
        eq_rows (strictly increasing, the same for every system) are equalities; shift may be 0 too; simplify=1 runs
        tab_simplify on the tableau (integer batches, as pip_solve does).  The tableau has nrows + len(eq_rows)
        inequalities; load() / load_part() go through pipamd_batch_load_system and dual_system() gives the dual as
        pip_solve lists it, one reduced pair per row of the system.
        matrices=True: rows are PolyLib matrices, (batch, max_rows, nvar + 2) with the marker first (0: an equality);
        nrows: an int32 tensor or array of the systems' row counts (None: max_rows each), kept on the device with the
        rows; ni: the room for the tallest tableau (rows + equalities; default 2 * max_rows).  shift and simplify as for
        system=True; load_matrices() / dual_matrices() go through pipamd_batch_load_matrices / pipamd_batch_dual_matrices,
        and a system the load cannot take ends ST_BADINPUT.
        sparse=True: the plain systems of system=True as sparse rows.  rows is (row_ptr, cols, vals) -- int64 offsets,
        batch * nrows + 1 of them, int32 columns (nvar: the constant) and int64 values, strictly increasing columns in a
        row --, or None for a workspace loaded with load_sparse_part(); shape=(batch, nrows, nvar + 1) is that of the dense
        expansion.  eq_rows, shift and simplify as for system=True; load_sparse() / dual_sparse() go through
        pipamd_batch_load_sparse / pipamd_batch_dual_sparse, and a system the load cannot take ends ST_BADINPUT.
        instances=True: the plain systems of system=True as ONE parametric system at many points.  rows is (matrix, points)
        -- matrix (nrows, nvar + nparm_of_the_matrix + 1) int64, unknowns | parameters | constant, and points (batch,
        nparm_of_the_matrix) int64 --; points may be an int, the batch size, for a workspace loaded with
        load_instances_part().  The nparm argument stays 0 (the tableaux have no parameters).  System b has the constants
        c_r + sum_k p_rk * points[b][k], computed exactly on the device; eq_rows, shift and simplify as for system=True;
        load_instances() / dual_instances() go through pipamd_batch_load_instances / pipamd_batch_dual_instances, and a
        system with a constant that does not fit the entry type ends ST_BADINPUT."""
        import torch
        self.torch = torch
        self.e = engine
        self.csr = None
        self.sparse = bool(sparse)
        if sparse:
            assert shape is not None and not matrices, "Batch(sparse=True) takes shape=(batch, nrows, nvar + 1)"
            dev = torch.device("cuda", engine.device)
            if rows is not None:
                self.csr = tuple((t if torch.is_tensor(t) else torch.as_tensor(t)).to(device=dev, dtype=dt).contiguous()
                                 for t, dt in zip(rows, (torch.int64, torch.int32, torch.int64)))
            rows, system = None, True
        self.inst = None
        self.instances = bool(instances)
        if instances:
            assert not sparse and not matrices and shape is None, "Batch(instances=True) takes rows=(matrix, points)"
            dev = torch.device("cuda", engine.device)
            matrix, points = rows
            matrix = (matrix if torch.is_tensor(matrix) else torch.as_tensor(matrix)).to(device=dev, dtype=torch.int64).contiguous()
            assert matrix.dim() == 2 and matrix.shape[1] >= nvar + 1, "matrix is (nrows, nvar + nparm + 1)"
            self.inst_nparm = matrix.shape[1] - nvar - 1
            if isinstance(points, int):
                shape, points = (points, matrix.shape[0], nvar + 1), None
            else:
                points = (points if torch.is_tensor(points) else torch.as_tensor(points)).to(device=dev, dtype=torch.int64).contiguous()
                points = points.reshape(points.shape[0], self.inst_nparm)
                shape = (points.shape[0], matrix.shape[0], nvar + 1)
            self.inst = (matrix, points)
            rows, system = None, True
        B, ni_in, ncol = rows.shape if rows is not None else shape
        self.shift = int(shift)
        self.system = None
        self.matrices = None
        if matrices:
            assert ncol == nvar + 2 and nparm == 0 and bigparm == -1 and not system and not eq_rows
            self.matrices = Matrices(ni_in, self.shift, int(simplify), 0, None)
            self.nrows = None
            if nrows is not None:
                dev = torch.device("cuda", engine.device)
                self.nrows = (nrows if torch.is_tensor(nrows) else torch.as_tensor(nrows)).to(device=dev, dtype=torch.int32).contiguous()
                assert self.nrows.shape == (B,)
                self.matrices.d_nrows = self.nrows.data_ptr()
            ni = int(ni) if ni is not None else 2 * ni_in
        else:
            assert ncol == nvar + nparm + 1 and nrows is None and ni is None
            ni = ni_in
        if system:
            assert nparm == 0 and bigparm == -1
            eq = [int(r) for r in eq_rows]
            self._eq = (C.c_int32 * max(1, len(eq)))(*eq)  # (kept alive with the batch: System points into it)
            self.system = System(ni, len(eq), C.cast(self._eq, C.POINTER(C.c_int32)) if eq else None, self.shift, int(simplify))
            ni += len(eq)
        elif not matrices:
            assert not eq_rows and not simplify
        # the form the batch's systems come in, decided here once: load() and load_part() route on it
        self.form = ("instances" if instances else "sparse" if sparse else "matrices" if matrices else "system" if system
                     else "shifted" if self.shift else "tableau")
        if self.shift:
            assert self.shift in (SHIFT_MAX, SHIFT_URS) and nparm == 0 and bigparm == -1
            nparm, bigparm = 1, nvar + 1
        if cap_cuts is None:
            cap_cuts = max(0, min(ni + 64, 2048 - ni)) if (tflags & T_INT) else 0
        self.desc = BatchDesc(B, nvar, nparm, ni, bigparm, tflags, cap_cuts, cap_newparm, entier_bits)
        self.entier_bits = entier_bits
        ew = 2 if entier_bits == 128 else 1
        self.dev = torch.device("cuda", engine.device)
        if rows is None:
            self.rows = None
        else:
            self.rows = rows if (torch.is_tensor(rows) and rows.is_cuda) else torch.as_tensor(rows, dtype=torch.int64).to(self.dev)
            self.rows = self.rows.contiguous()
        nbytes = lib().pipamd_batch_workspace_bytes(C.byref(self.desc))
        if nbytes == 0:
            raise RuntimeError(lib().pipamd_last_error().decode())
        self.ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=self.dev)
        self.status = torch.empty(B, dtype=torch.int32, device=self.dev)
        self.pivots = torch.empty(B, dtype=torch.int32, device=self.dev)
        self.cuts = torch.empty(B, dtype=torch.int32, device=self.dev)
        # 128-bit values come back as (low, high) int64 pairs: see wide_to_int()
        self.sol_num = torch.empty((B, nvar, nparm + 1) + ((2,) if ew == 2 else ()), dtype=torch.int64, device=self.dev)
        self.sol_den = torch.empty((B, nvar) + ((2,) if ew == 2 else ()), dtype=torch.int64, device=self.dev)
        if self.shift:  # fetch_shifted(): unknown i of tableau b is x_num / x_den, x_den == 0: unbounded
            self.x_num = torch.empty_like(self.sol_den)
            self.x_den = torch.empty_like(self.sol_den)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _source(self, form, *a):
        """The part `a` (its resident arrays, as the public method of `form` takes them) of a batch of that form: the C
        entry's arguments that describe it -- those between the descriptor and `first` --, its number of systems and
        the number of dual pairs per system."""
        t = self.torch
        if form in ("tableau", "shifted", "system"):
            rows, = a
            assert (form != "system" or self.system is not None) and rows.is_cuda and rows.is_contiguous()
            if form == "system":
                return [C.byref(self.system), C.c_void_p(rows.data_ptr())], int(rows.shape[0]), self.system.nrows
            shift = [self.shift] if form == "shifted" else []
            return [C.c_void_p(rows.data_ptr())] + shift, int(rows.shape[0]), self.desc.ni
        if form == "matrices":  # the batch's pipamd_matrices, with the part's own row counts
            rows, nrows = a
            assert self.matrices is not None and rows.is_cuda and rows.is_contiguous()
            assert tuple(rows.shape[1:]) == (self.matrices.max_rows, self.desc.nvar + 2)
            m = Matrices(self.matrices.max_rows, self.matrices.shift, self.matrices.simplify, 0, None)
            if nrows is not None:
                assert nrows.is_cuda and nrows.is_contiguous() and nrows.dtype == t.int32 and nrows.shape == (rows.shape[0],)
                m.d_nrows = nrows.data_ptr()
            return [C.byref(m), C.c_void_p(rows.data_ptr())], int(rows.shape[0]), self.matrices.max_rows
        if form == "sparse":  # the batch's system with the part's own arrays
            row_ptr, cols, vals = a
            assert self.sparse and all(x.is_cuda and x.is_contiguous() and x.dim() == 1 for x in (row_ptr, cols, vals))
            assert row_ptr.dtype == t.int64 and cols.dtype == t.int32 and vals.dtype == t.int64 and cols.numel() == vals.numel()
            count, rest = divmod(row_ptr.numel() - 1, max(1, self.system.nrows))
            assert rest == 0 and row_ptr.numel() >= 1, "row_ptr holds systems * nrows + 1 offsets"
            nnz = cols.numel()
            sp = Sparse(self.system, nnz, row_ptr.data_ptr(), cols.data_ptr() if nnz else None, vals.data_ptr() if nnz else None)
            return [C.byref(sp)], count, self.system.nrows
        points, matrix = a  # instances: the batch's system with the part's points and its matrix
        assert self.instances
        matrix = self.inst[0] if matrix is None else matrix
        assert matrix.is_cuda and matrix.is_contiguous() and matrix.dtype == t.int64 and matrix.shape == self.inst[0].shape
        assert points.is_cuda and points.is_contiguous() and points.dtype == t.int64
        assert points.dim() == 2 and points.shape[1] == self.inst_nparm
        ins = Instances(self.system, self.inst_nparm, 0, matrix.data_ptr(), points.data_ptr() if self.inst_nparm else None)
        return [C.byref(ins)], int(points.shape[0]), self.system.nrows

    def _entry(self, op, form):
        """pipamd_batch_<op>[_<form>]_part: the tableau entries carry no form in their name"""
        return getattr(lib(), "pipamd_batch_%s%s_part" % (op, "" if form == "tableau" else "_" + form))

    def _load(self, form, first, stream, *a):
        args, count, _ = self._source(form, *a)
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(self._entry("load", form)(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc), *args, int(first), count, st))

    def _dual(self, form, first, stream, out, *a):
        args, count, pairs = self._source(form, *a)
        num, den = out if out is not None else self._dual_out(pairs)
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(self._entry("dual", form)(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc), *args, int(first), count,
                                         C.c_void_p(num.data_ptr()), C.c_void_p(den.data_ptr()), st))
        return num, den

    def load(self):
        if self.form == "tableau":
            _check(lib().pipamd_batch_load(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc),
                                           C.c_void_p(self.rows.data_ptr()), self._stream()))
        elif self.form in ("shifted", "system"):
            self.load_part(self.rows, 0)
        else:
            getattr(self, "load_" + self.form)()

    def load_part(self, rows, first, stream=None):
        """tableaux first .. first + len(rows) - 1 of the batch from a resident row array (pipamd_batch_load_part)"""
        assert rows.is_cuda and rows.is_contiguous()
        assert self.matrices is None, "a Batch(matrices=True) is loaded with load_matrices_part(rows, nrows, first)"
        assert not self.sparse, "a Batch(sparse=True) is loaded with load_sparse_part(row_ptr, cols, vals, first)"
        assert not self.instances, "a Batch(instances=True) is loaded with load_instances_part(points, first)"
        self._load(self.form, first, stream, rows)

    def load_parts(self, parts, stream=None):
        """the whole batch from a list of resident row arrays (one pipamd_batch_load_part each)"""
        off = 0
        for part in parts:
            self.load_part(part, off, stream)
            off += part.shape[0]
        assert off == self.desc.batch

    def solve(self, stream=None):
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(lib().pipamd_batch_solve(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc), st))

    def solve_async(self, stream=None):
        """pipamd_batch_solve_async on `stream` (a raw hipStream_t handle; default: torch's current stream); one solve
        in flight per engine -- wait() before the next one, and before fetch()."""
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(lib().pipamd_batch_solve_async(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc), st))

    def wait(self):
        _check(lib().pipamd_batch_wait(self.e._h))

    def poll(self):
        """pipamd_batch_poll: 1 = the batch is done, 0 = still running (never blocks)"""
        rc = int(lib().pipamd_batch_poll(self.e._h))
        if rc < 0:
            _check(rc)
        return rc

    def fetch(self, stream=None):
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(lib().pipamd_batch_results(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc),
                                          C.c_void_p(self.status.data_ptr()), C.c_void_p(self.pivots.data_ptr()),
                                          C.c_void_p(self.cuts.data_ptr()), C.c_void_p(self.sol_num.data_ptr()),
                                          C.c_void_p(self.sol_den.data_ptr()), st))

    def fetch_shifted(self, stream=None):
        """pipamd_batch_results_shifted of a Batch(shift=...): status, pivots, cuts and the decoded answer x_num, x_den
        (sol_vector_edit: reduced, negated for SHIFT_MAX, x_den == 0 where the unknown is unbounded).  Does not synchronise."""
        assert self.shift
        st = C.c_void_p(stream) if stream is not None else self._stream()
        _check(lib().pipamd_batch_results_shifted(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc), self.shift,
                                              C.c_void_p(self.status.data_ptr()), C.c_void_p(self.pivots.data_ptr()),
                                              C.c_void_p(self.cuts.data_ptr()), C.c_void_p(self.x_num.data_ptr()),
                                              C.c_void_p(self.x_den.data_ptr()), st))

    def _dual_out(self, nrows):
        shape = (self.desc.batch, nrows) + ((2,) if self.entier_bits == 128 else ())
        return (self.torch.empty(shape, dtype=self.torch.int64, device=self.dev),
                self.torch.empty(shape, dtype=self.torch.int64, device=self.dev))

    def dual(self, stream=None):
        """pipamd_batch_dual after a solve with T_DUAL: device tensors (dual_num, dual_den) of shape (batch, ni) -- plus a
        trailing 2, (low, high), for 128-bit entries: see wide_to_int() --, the pairs solution_dual emits, not reduced;
        (0, 0) throughout for a tableau without a solution.  Does not synchronise."""
        if self.rows is None:
            raise RuntimeError("Batch.dual needs the rows the batch was loaded from: use dual_part() with load_parts()")
        return self.dual_part(self.rows, 0, stream)

    def dual_part(self, rows, first, stream=None, out=None):
        """pipamd_batch_dual_part for the tableaux first .. first + len(rows) - 1, loaded from the resident array `rows`
        (as load_part was given it); returns (dual_num, dual_den) of the whole batch's shape, only those tableaux written
        (pass the pair back as `out` to fill it part by part)."""
        assert rows.is_cuda and rows.is_contiguous()
        if not hasattr(lib(), "pipamd_batch_dual_part"):
            raise RuntimeError("libpipamd has no pipamd_batch_dual_part: rebuild the library")
        return self._dual("tableau", first, stream, out, rows)

    def load_system(self, stream=None):
        """pipamd_batch_load_system of a Batch(system=True): the whole batch from its resident plain rows"""
        return self.load_system_part(self.rows, 0, stream)

    def load_system_part(self, rows, first, stream=None):
        """pipamd_batch_load_system_part: tableaux first .. first + len(rows) - 1 from the resident plain systems `rows`"""
        self._load("system", first, stream, rows)

    def dual_system(self, stream=None):
        """pipamd_batch_dual_system after a solve with T_DUAL of a Batch(system=True): device tensors (dual_num, dual_den)
        of shape (batch, nrows) -- plus a trailing 2 for 128-bit entries --, one reduced pair per row of the system, an
        equality's two values merged; (0, 0) throughout for a tableau without a solution.  Does not synchronise."""
        if self.rows is None:
            raise RuntimeError("Batch.dual_system needs the rows the batch was loaded from: use dual_system_part()")
        return self.dual_system_part(self.rows, 0, stream)

    def dual_system_part(self, rows, first, stream=None, out=None):
        """pipamd_batch_dual_system_part for the tableaux first .. first + len(rows) - 1, loaded from the resident array
        `rows`; returns (dual_num, dual_den) of the whole batch's shape (pass the pair back as `out` to fill it part by part)."""
        return self._dual("system", first, stream, out, rows)

    def load_matrices(self, stream=None):
        """pipamd_batch_load_matrices of a Batch(matrices=True): the whole batch from its resident matrices and row counts"""
        return self.load_matrices_part(self.rows, self.nrows, 0, stream)

    def load_matrices_part(self, rows, nrows, first, stream=None):
        """pipamd_batch_load_matrices_part: tableaux first .. first + len(rows) - 1 from the resident matrices `rows` and
        their row counts `nrows` (a resident int32 tensor, or None: max_rows each)"""
        self._load("matrices", first, stream, rows, nrows)

    def dual_matrices(self, stream=None):
        """pipamd_batch_dual_matrices after a solve with T_DUAL of a Batch(matrices=True): device tensors (dual_num,
        dual_den) of shape (batch, max_rows) -- plus a trailing 2 for 128-bit entries --, one reduced pair per row of a
        system, (0, 0) beyond its rows and throughout for a tableau without a solution.  Does not synchronise."""
        if self.rows is None:
            raise RuntimeError("Batch.dual_matrices needs the matrices the batch was loaded from: use dual_matrices_part()")
        return self.dual_matrices_part(self.rows, self.nrows, 0, stream)

    def dual_matrices_part(self, rows, nrows, first, stream=None, out=None):
        """pipamd_batch_dual_matrices_part for the tableaux first .. first + len(rows) - 1, loaded from `rows` and `nrows`;
        returns (dual_num, dual_den) of the whole batch's shape (pass the pair back as `out` to fill it part by part)."""
        return self._dual("matrices", first, stream, out, rows, nrows)

    def load_sparse(self, stream=None):
        """pipamd_batch_load_sparse of a Batch(sparse=True): the whole batch from its resident CSR arrays"""
        return self.load_sparse_part(*self.csr, 0, stream)

    def load_sparse_part(self, row_ptr, cols, vals, first, stream=None):
        """pipamd_batch_load_sparse_part: tableaux first .. first + count - 1 from the resident CSR arrays of those systems
        (row_ptr: count * nrows + 1 offsets into cols / vals)"""
        self._load("sparse", first, stream, row_ptr, cols, vals)

    def dual_sparse(self, stream=None):
        """pipamd_batch_dual_sparse after a solve with T_DUAL of a Batch(sparse=True): device tensors (dual_num, dual_den)
        of shape (batch, nrows) -- plus a trailing 2 for 128-bit entries --, as dual_system() gives them; (0, 0)
        throughout for a tableau without a solution.  Does not synchronise."""
        if self.csr is None:
            raise RuntimeError("Batch.dual_sparse needs the arrays the batch was loaded from: use dual_sparse_part()")
        return self.dual_sparse_part(*self.csr, 0, stream)

    def dual_sparse_part(self, row_ptr, cols, vals, first, stream=None, out=None):
        """pipamd_batch_dual_sparse_part for the tableaux first .. first + count - 1, loaded from these CSR arrays; returns
        (dual_num, dual_den) of the whole batch's shape (pass the pair back as `out` to fill it part by part)."""
        return self._dual("sparse", first, stream, out, row_ptr, cols, vals)

    def load_instances(self, stream=None):
        """pipamd_batch_load_instances of a Batch(instances=True): the whole batch from its resident matrix and points"""
        return self.load_instances_part(self.inst[1], 0, stream)

    def load_instances_part(self, points, first, stream=None, matrix=None):
        """pipamd_batch_load_instances_part: tableaux first .. first + len(points) - 1, the systems of the resident `points`
        ((count, nparm) int64) under the batch's matrix, or under `matrix`, a resident one of the same shape"""
        self._load("instances", first, stream, points, matrix)

    def dual_instances(self, stream=None):
        """pipamd_batch_dual_instances after a solve with T_DUAL of a Batch(instances=True): device tensors (dual_num,
        dual_den) of shape (batch, nrows) -- plus a trailing 2 for 128-bit entries --, as dual_system() gives them; (0, 0)
        throughout for a tableau without a solution.  Does not synchronise."""
        if self.inst[1] is None:
            raise RuntimeError("Batch.dual_instances needs the points the batch was loaded from: use dual_instances_part()")
        return self.dual_instances_part(self.inst[1], 0, stream)

    def dual_instances_part(self, points, first, stream=None, out=None, matrix=None):
        """pipamd_batch_dual_instances_part for the tableaux first .. first + len(points) - 1, loaded from these points (and
        `matrix`, if not the batch's); returns (dual_num, dual_den) of the whole batch's shape (pass the pair back as `out`
        to fill it part by part)."""
        return self._dual("instances", first, stream, out, points, matrix)

    def counters(self):
        """dict of batch totals (pivots, cuts, rows_rewritten, finished) -- synchronises."""
        out = self.torch.zeros(4, dtype=self.torch.int64, device=self.dev)
        _check(lib().pipamd_batch_counters(self.e._h, C.c_void_p(self.ws.data_ptr()), C.byref(self.desc),
                                           C.c_void_p(out.data_ptr()), self._stream()))
        v = out.cpu().tolist()
        return {"pivots": v[0], "cuts": v[1], "rows_rewritten": v[2], "finished": v[3]}

    def last_solve_ms(self):
        ms = C.c_float()
        _check(lib().pipamd_last_solve_ms(self.e._h, C.byref(ms)))
        return float(ms.value)

    def pivot_bytes(self):
        return int(lib().pipamd_dense_pivot_bytes(C.byref(self.desc)))


def slow_converging(engine, rows, nvar, cut_rows=448, entier_bits=64):
    """Indices of the tableaux of an integer batch (nparm = 0) on which Gomory's cuts have not converged within
    `cut_rows` cut rows: the batch is solved once with that row budget (pipamd_engine_set_max_rows) and the tableaux left
    at PIPAMD_ST_CAPACITY are returned.  A property of the tableau and of the reference's algorithm (the number of
    cuts integrer() adds is the same on any correct implementation), not of this engine: on the synthetic families of
    piplib_amd/synth.py about 3 tableaux in 100,000 are of this kind, and on them the reference's own loop
    (traiter.c:665-789, unbounded expanser) does not end within minutes on a CPU either.  bench.py replaces them by
    their neighbours before it times anything (a benchmark workload must be one the reference finishes)."""
    import torch
    e2 = Engine(engine.device)
    ni = int(rows.shape[1])
    e2.set_max_rows(ni + cut_rows)
    b = Batch(e2, rows, nvar, 0, tflags=T_INT, entier_bits=entier_bits)
    b.load()
    b.solve()
    b.fetch()
    torch.cuda.synchronize(b.dev)
    idx = torch.nonzero(b.status == ST_CAPACITY).flatten().cpu().tolist()
    del b
    e2.close()
    return idx


class SolCell(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("param1", C.c_int64), ("param2", C.c_int64)]


SOL_NIL, SOL_IF, SOL_LIST, SOL_FORM, SOL_NEW, SOL_DIV, SOL_VAL = range(1, 8)


def _frac(n, d):
    import math
    g = math.gcd(n, d)
    return f" {n // g}" if g == abs(d) and d > 0 else (f" {n // g}/{d // g}" if g else f" {n}/{d}")


def tape_text(cells):
    """Test/bench harness only: the text the reference's sol_edit (sol.c:291-422) prints for a tape,
    cells = [(kind, param1, param2), ...].  An empty tape is the front ends' "void"."""
    if not cells:
        return "void\n"
    out = []

    def item(i):
        while cells[i][0] == SOL_NEW:
            out.append("(newparm %d " % cells[i][1])
            i = item(i + 1)
            out.append(")\n")
        k, a, b = cells[i]
        if k == SOL_NIL:
            out.append("()\n")
            return i + 1
        if k == SOL_IF:
            out.append("(if ")
            i = item(item(item(i + 1)))
            out.append(")\n")
            return i
        if k == SOL_LIST:
            out.append("(list ")
            i += 1
            for _ in range(a):
                i = item(i)
            out.append(")\n")
            return i
        if k == SOL_FORM:
            out.append("#[")
            for j in range(a):
                out.append(_frac(cells[i + 1 + j][1], cells[i + 1 + j][2]))
            out.append("]\n")
            return i + 1 + a
        if k == SOL_DIV:
            out.append("(div ")
            i = item(item(i + 1))
            out.append(")\n")
            return i
        if k == SOL_VAL:
            out.append(_frac(a, b))
            return i + 1
        raise ValueError(f"unknown tape cell kind {k}")

    i = 0
    while i < len(cells):
        i = item(i)
    return "".join(out)


def _take_cells(ptr, n):
    if not ptr or not n:
        return []
    arr = C.cast(ptr, C.POINTER(SolCell * n)).contents
    cells = [(c.kind, c.param1, c.param2) for c in arr]
    lib().pipamd_free(ptr)
    return cells


def _rows(ineq, ctx, ni, nc, nvar, nparm):
    import numpy as np
    a = np.ascontiguousarray(ineq, dtype=np.int64).reshape(ni, nvar + nparm + 1)
    c = np.ascontiguousarray(ctx, dtype=np.int64).reshape(nc, nparm + 1)
    return a, c


class SolCell128(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p1lo", C.c_int64), ("p1hi", C.c_int64),
                ("p2lo", C.c_int64), ("p2hi", C.c_int64)]


def _take_cells128(ptr, n):
    if not ptr or not n:
        return []
    arr = C.cast(ptr, C.POINTER(SolCell128 * n)).contents
    m = (1 << 64) - 1
    cells = [(c.kind, (c.p1hi << 64) | (c.p1lo & m), (c.p2hi << 64) | (c.p2lo & m)) for c in arr]
    lib().pipamd_free(ptr)
    return cells


def solve_tableau_cells(engine, nvar, nparm, ni, nc, bigparm, nq, ineq, ctx, simplify=True, deepest_cut=False, bits=64):
    """Layer 3: one problem in .dat form (host arrays) -> (tape cells, pivots); bits=128 runs the
    overflow-safe flavour (128-bit entries on the device and in the host tree).
    Raises SolverError(status) where the reference would have exit()ed."""
    a, c = _rows(ineq, ctx, ni, nc, nvar, nparm)
    L = lib()
    fn = L.pipamd_solve_tableau128 if bits == 128 else L.pipamd_solve_tableau
    fn.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    cells, n = C.c_void_p(), C.c_size_t(0)
    status, piv = C.c_int(0), C.c_int64(0)
    rc = fn(engine._h, nvar, nparm, ni, nc, bigparm, nq, C.c_void_p(a.ctypes.data),
            C.c_void_p(c.ctypes.data), int(bool(simplify)), int(bool(deepest_cut)),
            C.byref(cells), C.byref(n), C.byref(status), C.byref(piv))
    if rc == -5:
        raise SolverError(status.value, piv.value)
    _check(rc)
    return (_take_cells128 if bits == 128 else _take_cells)(cells, n.value), piv.value


def solve_tableau(engine, nvar, nparm, ni, nc, bigparm, nq, ineq, ctx, simplify=True, deepest_cut=False, bits=64):
    """solve_tableau_cells, with the tape printed as sol_edit would (tests compare texts)."""
    cells, piv = solve_tableau_cells(engine, nvar, nparm, ni, nc, bigparm, nq, ineq, ctx, simplify, deepest_cut, bits)
    return tape_text(cells), piv


def traiter(engine, nvar, nparm, ni, nc, bigparm, flags, tableau, context, deepest_cut=False, bits=64):
    """pipamd_traiter / pipamd_traiter128: one traiter() call -> (tape cells, pivots)."""
    a, c = _rows(tableau, context, ni, nc, nvar, nparm)
    L = lib()
    fn = L.pipamd_traiter128 if bits == 128 else L.pipamd_traiter
    fn.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    cells, n = C.c_void_p(), C.c_size_t(0)
    status, piv = C.c_int(0), C.c_int64(0)
    rc = fn(engine._h, nvar, nparm, ni, nc, bigparm, int(flags), int(bool(deepest_cut)),
            C.c_void_p(a.ctypes.data), C.c_void_p(c.ctypes.data), C.byref(cells), C.byref(n),
            C.byref(status), C.byref(piv))
    if rc == -5:
        raise SolverError(status.value, piv.value)
    _check(rc)
    return (_take_cells128 if bits == 128 else _take_cells)(cells, n.value), piv.value


def traiter_many(engine, problems, flags=None, deepest_cut=False, nthreads=8, bits=64):
    """pipamd_traiter_many / pipamd_traiter_many128: one traiter() call per problem (objects with nvar, nparm, ni, nc,
    bigparm, ineq, ctx; nq is ignored), flags[i] = 0, T_INT or T_DUAL (None: all 0).  Returns a list of
    (cells | None, rc, status, pivots), the cells as traiter() returns them, None where rc != 0."""
    L = lib()
    name = "pipamd_traiter_many128" if bits == 128 else "pipamd_traiter_many"
    if not hasattr(L, name):
        raise RuntimeError(f"libpipamd has no {name}: rebuild the library")
    fn = getattr(L, name)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    prep = PreparedProblems(problems)
    fl = None
    if flags is not None:
        if len(flags) != prep.n:
            raise ValueError("traiter_many: one flag per problem")
        fl = (C.c_int * max(1, prep.n))(*[int(f) for f in flags])
    _check(fn(engine._h, prep.n, prep.arr, fl, int(bool(deepest_cut)), int(nthreads),
              prep.cells, prep.ncell, prep.rcs, prep.sts, prep.piv))
    take = _take_cells128 if bits == 128 else _take_cells
    out = []
    for i in range(prep.n):
        cells = take(prep.cells[i], prep.ncell[i])
        out.append((cells if prep.rcs[i] == 0 else None, prep.rcs[i], prep.sts[i], prep.piv[i]))
    return out


class SolverError(RuntimeError):
    def __init__(self, status, pivots=0):
        super().__init__(f"solver stopped with PIPAMD_ST status {status}")
        self.status = status
        self.pivots = pivots


class PipProblem(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nvar", "nparm", "ni", "nc", "bigparm", "nq")] + \
               [("ineq", C.c_void_p), ("ctx", C.c_void_p)]


class PreparedProblems:
    """ctypes view of a list of problems (objects with nvar, nparm, ni, nc, bigparm, nq, ineq, ctx) and the
    result arrays of one pipamd_solve_tableaux* call"""

    def __init__(self, problems):
        import numpy as np
        self.n = n = len(problems)
        self.arr = (PipProblem * max(1, n))()
        self.keep = []
        for i, p in enumerate(problems):
            a = np.ascontiguousarray(p.ineq, dtype=np.int64).reshape(p.ni, p.nvar + p.nparm + 1)
            c = np.ascontiguousarray(p.ctx, dtype=np.int64).reshape(p.nc, p.nparm + 1)
            self.keep += [a, c]
            self.arr[i] = PipProblem(p.nvar, p.nparm, p.ni, p.nc, p.bigparm, p.nq, a.ctypes.data, c.ctypes.data)
        self.cells = (C.c_void_p * max(1, n))()
        self.ncell = (C.c_size_t * max(1, n))()
        self.rcs = (C.c_int * max(1, n))()
        self.sts = (C.c_int * max(1, n))()
        self.piv = (C.c_int64 * max(1, n))()

    def results(self, bits=64):
        """[(text | None, rc, status, pivots)]; frees the cells (bits=128: they are pipamd_sol_cell128)"""
        take = _take_cells128 if bits == 128 else _take_cells
        out = []
        for i in range(self.n):
            t = tape_text(take(self.cells[i], self.ncell[i])) if self.rcs[i] == 0 else None
            out.append((t, self.rcs[i], self.sts[i], self.piv[i]))
        return out


def device_tree_fits(problem, bits=64):
    """pipamd_device_tree_fits: 1 if the device-resident traiter() takes a problem of this shape in the `bits` (64 or 128)
    flavour (it may still hand it back at run time), 0 if the shape goes straight to the host schedulers.  No engine, no GPU."""
    prep = PreparedProblems([problem])
    L = lib()
    L.pipamd_device_tree_fits.argtypes = [C.c_void_p, C.c_int]
    rc = L.pipamd_device_tree_fits(prep.arr, int(bits))
    _check(min(rc, 0))
    return rc


def _many(fn_name, engine, prep, *ints):
    """one pipamd_solve_tableaux* call on prepared problems: (engine, n, problems, ints ..., the five result arrays)"""
    fn = getattr(lib(), fn_name)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * len(ints) + [C.c_void_p] * 5
    _check(fn(engine._h, prep.n, prep.arr, *[int(x) for x in ints], prep.cells, prep.ncell, prep.rcs, prep.sts, prep.piv))


def solve_tableaux128(engine, problems, simplify=True, deepest_cut=False, nthreads=8):
    """Many problems through pipamd_solve_tableaux128 (128-bit entries, a host thread and a TreeT<__int128> each).
    Returns a list of (text | None, rc, status, pivots)."""
    prep = PreparedProblems(problems)
    _many("pipamd_solve_tableaux128", engine, prep, bool(simplify), bool(deepest_cut), nthreads)
    return prep.results(bits=128)


def solve_tableaux_lockstep128(engine, problems, simplify=True, deepest_cut=False):
    """Many problems through pipamd_solve_tableaux_lockstep128 (128-bit entries, the lock-step scheduler).
    Returns a list of (text | None, rc, status, pivots)."""
    prep = PreparedProblems(problems)
    _many("pipamd_solve_tableaux_lockstep128", engine, prep, bool(simplify), bool(deepest_cut))
    return prep.results(bits=128)


def solve_prepared(engine, prep, simplify=True, deepest_cut=False, nthreads=8, lockstep=False):
    """the bare C call on prepared problems (what a C caller pays); prep.results() turns the cells into text"""
    if lockstep:
        _many("pipamd_solve_tableaux_lockstep", engine, prep, bool(simplify), bool(deepest_cut))
    else:
        _many("pipamd_solve_tableaux", engine, prep, bool(simplify), bool(deepest_cut), nthreads)


def solve_tableaux(engine, problems, simplify=True, deepest_cut=False, nthreads=8, lockstep=False):
    """Many problems (objects with nvar, nparm, ni, nc, bigparm, nq, ineq, ctx) through
    pipamd_solve_tableaux / pipamd_solve_tableaux_lockstep.  Returns a list of (text | None, rc, status, pivots)."""
    prep = PreparedProblems(problems)
    solve_prepared(engine, prep, simplify, deepest_cut, nthreads, lockstep)
    return prep.results()


# ---- pip_solve(inequnk, ineqpar, Bg, options) for many problems, from the PolyLib matrices (pipamd_pip_*)
PIP_NQ, PIP_MAXIMIZE, PIP_URS_PARMS, PIP_URS_UNKNOWNS, PIP_DUAL = 1, 2, 4, 8, 16


class PipSolveProblem(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nrows", "ncols", "ctx_rows", "ctx_cols", "bg", "options")] + \
               [("inequnk", C.c_void_p), ("ineqpar", C.c_void_p)]


class PipInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nvar", "nparm", "ni", "nc", "bigparm", "flags", "sol_bg", "urs_parms",
                                         "sol_flags", "is_void")] + [("row_off", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PipInput:
    """One pip_solve call: inequnk / ineqpar are 2-D int64 arrays in PolyLib form (marker column first) or None, bg the
    big parameter's tableau column or -1, options a sum of PIP_*.  shape = (nrows, ncols, ctx_rows, ctx_cols) overrides
    what the arrays say (tests of malformed problems)."""

    def __init__(self, inequnk, ineqpar=None, bg=-1, options=PIP_NQ, shape=None):
        self.inequnk, self.ineqpar, self.bg, self.options, self.shape = inequnk, ineqpar, bg, options, shape


class _PipPrepared:
    def __init__(self, problems):
        import numpy as np
        self.n = n = len(problems)
        self.arr = (PipSolveProblem * max(1, n))()
        self.info = (PipInfo * max(1, n))()
        self.keep = []
        for i, p in enumerate(problems):
            a = None if p.inequnk is None else np.ascontiguousarray(p.inequnk, dtype=np.int64)
            c = None if p.ineqpar is None else np.ascontiguousarray(p.ineqpar, dtype=np.int64)
            if (a is not None and a.ndim != 2) or (c is not None and c.ndim != 2):
                raise ValueError("pip problems take 2-D matrices")
            self.keep += [a, c]
            shape = p.shape or ((a.shape if a is not None else (0, 0)) + (c.shape if c is not None else (0, 0)))
            self.arr[i] = PipSolveProblem(*[int(x) for x in shape], int(p.bg), int(p.options),
                                          a.ctypes.data if a is not None else None,
                                          c.ctypes.data if c is not None and c.size else None)


def pip_tableaux(engine, problems):
    """pipamd_pip_tableaux: tab_Matrix2Tableau for many problems (PipInput-like objects), built on the device.
    Returns (infos, tableaux): infos[i] a dict of pipamd_pip_info, tableaux[i] = (domain rows, context rows) as int64
    arrays, or None for a void or malformed problem (infos[i]["nvar"] < 0: malformed)."""
    import numpy as np
    L = lib()
    if not hasattr(L, "pipamd_pip_tableaux"):
        raise RuntimeError("libpipamd has no pipamd_pip_tableaux: rebuild the library")
    prep = _PipPrepared(problems)
    fn = L.pipamd_pip_tableaux
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    rows, nw = C.c_void_p(), C.c_size_t(0)
    rc = fn(engine._h, prep.n, prep.arr, prep.info, C.byref(rows), C.byref(nw))
    if rc != -1:  # PIPAMD_E_INVALID with rows: some problem is malformed, the others are built
        _check(rc)
    flat = np.zeros(0, dtype=np.int64)
    if rows and nw.value:
        flat = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_int64)), shape=(nw.value,)).copy()
        L.pipamd_free(rows)
    infos, tabs = [], []
    for i in range(prep.n):
        f = prep.info[i].as_dict()
        infos.append(f)
        if f["nvar"] < 0 or f["is_void"]:
            tabs.append(None)
            continue
        w, cw = f["nvar"] + f["nparm"] + 1, f["nparm"] + 1
        o = f["row_off"]
        dom = flat[o:o + f["ni"] * w].reshape(f["ni"], w)
        o += f["ni"] * w
        tabs.append((dom, flat[o:o + f["nc"] * cw].reshape(f["nc"], cw)))
    return infos, tabs


def pip_solve_many(engine, problems, deepest_cut=False, nthreads=8, bits=64):
    """pipamd_pip_solve_many / pipamd_pip_solve_many128: pip_solve for many problems (PipInput-like objects) in one call.
    Returns a list of (cells | None, rc, status, pivots, info): the tape as pip_solve has it when traiter() returns (empty
    for a void answer, info["is_void"] = 1; None where rc != 0) and info, the dict of pipamd_pip_info."""
    L = lib()
    name = "pipamd_pip_solve_many128" if bits == 128 else "pipamd_pip_solve_many"
    if not hasattr(L, name):
        raise RuntimeError(f"libpipamd has no {name}: rebuild the library")
    prep = _PipPrepared(problems)
    n = prep.n
    cells, ncell = (C.c_void_p * max(1, n))(), (C.c_size_t * max(1, n))()
    rcs, sts, piv = (C.c_int * max(1, n))(), (C.c_int * max(1, n))(), (C.c_int64 * max(1, n))()
    fn = getattr(L, name)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    _check(fn(engine._h, n, prep.arr, int(bool(deepest_cut)), int(nthreads), prep.info, cells, ncell, rcs, sts, piv))
    take = _take_cells128 if bits == 128 else _take_cells
    out = []
    for i in range(n):
        got = take(cells[i], ncell[i])
        out.append((got if rcs[i] == 0 else None, rcs[i], sts[i], piv[i], prep.info[i].as_dict()))
    return out


# ---------------------------------------------------------------- a tape at many parameter points
class TapeShape(C.Structure):
    """pipamd_tape_shape"""
    _fields_ = [(n, C.c_int32) for n in ("nvar", "nparm", "ndual", "reserved")]


class TapeInfo(C.Structure):
    """pipamd_tape_info: what pipamd_tape_check counts"""
    _fields_ = [(n, C.c_int64) for n in ("leaves", "ifs", "news", "words")] + \
               [(n, C.c_int32) for n in ("slots", "depth", "staged", "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class TapeError(RuntimeError):
    """a tape pipamd_tape_check refuses: code is PIPAMD_E_INVALID (-1) or PIPAMD_E_TOOLARGE (-3)"""

    def __init__(self, code, why):
        super().__init__(f"piplib_amd error {code}: {why}")
        self.code = code


def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _cell_array(cells, bits):
    """(kind, param1, param2) tuples as an array of pipamd_sol_cell / pipamd_sol_cell128 (None for no cells)"""
    if bits not in (64, 128):
        raise ValueError("bits is 64 or 128")
    n = len(cells)
    if n == 0:
        return None
    if bits == 128:
        arr = (SolCell128 * n)()
        for c, (k, a, b) in zip(arr, cells):
            a, b = int(a), int(b)
            if not (-(1 << 127) <= a < (1 << 127) and -(1 << 127) <= b < (1 << 127)):
                raise OverflowError("a tape cell beyond 128 bits")
            c.kind, c.p1lo, c.p1hi, c.p2lo, c.p2hi = int(k), _s64(a), a >> 64, _s64(b), b >> 64
    else:
        arr = (SolCell * n)()
        for c, (k, a, b) in zip(arr, cells):
            c.kind, c.param1, c.param2 = int(k), int(a), int(b)
            if c.param1 != int(a) or c.param2 != int(b):
                raise OverflowError("a tape cell beyond int64")
    return arr


def _tape_fn(name, bits):
    L = lib()
    name += "128" if bits == 128 else ""
    if not hasattr(L, name):
        raise RuntimeError(f"libpipamd has no {name}: rebuild the library")
    return getattr(L, name)


SOL_SHIFT, SOL_NEGATE, SOL_REMOVE, SOL_DUAL = 1, 2, 4, 8


class TapeEdit(C.Structure):
    """pipamd_tape_edit: what pip_solve passes to sol_quast_edit"""
    _fields_ = [(n, C.c_int32) for n in ("sol_bg", "urs_parms", "sol_flags", "reserved")]


def _tape_edit(edit):
    """None, a dict with sol_bg / urs_parms / sol_flags (the dict of pipamd_pip_info will do; "reserved" is passed on if
    present) or a PipInfo -> TapeEdit or None"""
    if edit is None:
        return None
    get = edit.get if isinstance(edit, dict) else (lambda k, d=0: getattr(edit, k, d))
    return TapeEdit(int(get("sol_bg", 0)), int(get("urs_parms", 0)), int(get("sol_flags", 0)), int(get("reserved", 0)))


def tape_check(cells, nvar, nparm, ndual=0, bits=64, reserved=0, edit=None):
    """pipamd_tape_check / pipamd_tape_check128 on cells [(kind, param1, param2), ...]: the dict of pipamd_tape_info, or
    TapeError where the tape is refused.  With `edit` (see Tape): pipamd_tape_check_pip / _pip128.  Host only: needs
    neither an engine nor a GPU."""
    arr = _cell_array(cells, bits)
    info = TapeInfo()
    shape = TapeShape(int(nvar), int(nparm), int(ndual), int(reserved))
    if edit is not None:
        fn = _tape_fn("pipamd_tape_check_pip", bits)
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(TapeShape), C.POINTER(TapeEdit), C.POINTER(TapeInfo)]
        rc = fn(arr, len(cells), C.byref(shape), C.byref(_tape_edit(edit)), C.byref(info))
    else:
        fn = _tape_fn("pipamd_tape_check", bits)
        fn.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(TapeShape), C.POINTER(TapeInfo)]
        rc = fn(arr, len(cells), C.byref(shape), C.byref(info))
    if rc != 0:
        raise TapeError(rc, lib().pipamd_last_error().decode())
    return info.as_dict()


class Tape:
    """A solution tape compiled for one engine's device (pipamd_tape_compile), to be evaluated at parameter points
    (pipamd_tape_eval): solve a parametric problem once -- solve_tableau_cells, traiter, traiter_many -- and ask for the
    unknowns at as many points as needed.  eval() knows no context; sweep() tests the points of a box against one.  `edit` -- a dict or PipInfo with sol_bg,
    urs_parms and sol_flags, as pip_solve_many hands them out -- applies pip_solve's result edits
    (pipamd_tape_compile_pip, include/piplib_amd.h): a point then has `point_cols` values, the parameters as pip_solve's
    caller numbers them; nparm stays the parameter count of the tape as solved."""
    OUTPUTS = ("status", "leaf", "x_num", "x_den", "dual_num", "dual_den")

    def __init__(self, engine, cells, nvar, nparm, ndual=0, bits=64, edit=None):
        import torch
        self.torch = torch
        self.e = engine
        self.nvar, self.nparm, self.ndual, self.bits = int(nvar), int(nparm), int(ndual), int(bits)
        self.info = tape_check(cells, nvar, nparm, ndual, bits, edit=edit)
        self._h = C.c_void_p()
        arr = _cell_array(cells, bits)
        shape = TapeShape(self.nvar, self.nparm, self.ndual, 0)
        if edit is not None:
            fn = _tape_fn("pipamd_tape_compile_pip", bits)
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TapeShape), C.POINTER(TapeEdit), C.POINTER(C.c_void_p)]
            _check(fn(engine._h, arr, len(cells), C.byref(shape), C.byref(_tape_edit(edit)), C.byref(self._h)))
        else:
            fn = _tape_fn("pipamd_tape_compile", bits)
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TapeShape), C.POINTER(C.c_void_p)]
            _check(fn(engine._h, arr, len(cells), C.byref(shape), C.byref(self._h)))
        pc = lib().pipamd_tape_point_cols
        pc.argtypes = [C.c_void_p]
        self.point_cols = int(pc(self._h))
        self.dev = torch.device("cuda", engine.device)

    def close(self):
        if self._h:
            lib().pipamd_tape_free.argtypes = [C.c_void_p]
            lib().pipamd_tape_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _points(self, points):
        """-> (count, device tensor or None)"""
        t = self.torch
        if isinstance(points, int):
            assert self.point_cols == 0, "a count stands for points only when the tape has no parameters"
            return points, None
        points = (points if t.is_tensor(points) else t.as_tensor(points, dtype=t.int64)).to(device=self.dev, dtype=t.int64)
        points = points.reshape(points.shape[0], self.point_cols).contiguous()
        return int(points.shape[0]), (points if self.point_cols else None)

    def outputs(self, n, names=OUTPUTS):
        """fresh device tensors for `n` points: int32 status and leaf, int64 (n, nvar) / (n, ndual) values with a trailing
        2 -- (low, high) -- for 128-bit tapes"""
        t = self.torch
        ew = (2,) if self.bits == 128 else ()
        shapes = {"status": ((n,), t.int32), "leaf": ((n,), t.int32), "x_num": ((n, self.nvar) + ew, t.int64),
                  "x_den": ((n, self.nvar) + ew, t.int64), "dual_num": ((n, self.ndual) + ew, t.int64),
                  "dual_den": ((n, self.ndual) + ew, t.int64)}
        return {k: t.empty(shapes[k][0], dtype=shapes[k][1], device=self.dev) for k in names}

    def eval_into(self, points, out, stream=None):
        """pipamd_tape_eval into the tensors of `out`, a dict by the names of OUTPUTS; a name that is missing is passed
        as NULL.  One launch on `stream` (a raw hipStream_t handle; default: torch's current stream), no synchronisation."""
        n, pts = self._points(points)
        fn = lib().pipamd_tape_eval
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)
        ptrs = [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else None for k in self.OUTPUTS]
        _check(fn(self.e._h, self._h, n, C.c_void_p(pts.data_ptr()) if pts is not None else None, *ptrs, st))
        return out

    def eval(self, points, stream=None):
        """the tape at `points`, (n, point_cols) int64 on the host or the device (an int n when the tape has no parameters):
        device tensors (status, leaf, x_num, x_den) and, with ndual > 0, (dual_num, dual_den).  Does not synchronise."""
        n, pts = self._points(points)
        names = self.OUTPUTS if self.ndual else self.OUTPUTS[:4]
        out = self.eval_into(pts if pts is not None else n, self.outputs(n, names), stream)
        return tuple(out[k] for k in names)

    def _box(self, lo, hi):
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        assert len(lo) == len(hi) == self.point_cols, "a box has point_cols bounds on either side"
        n = max(1, self.point_cols)
        return (C.c_int64 * n)(*lo), (C.c_int64 * n)(*hi)

    def sweep_plan(self, lo, hi):
        """sweep_plan() for this tape: n_points, summary_words, binned"""
        return sweep_plan(self.info, self.bits, self.point_cols, lo, hi)

    def sweep_into(self, lo, hi, out, ctx=None, summary=None, stream=None):
        """pipamd_tape_sweep: the tape at every integer point of the box lo .. hi (inclusive; point k is the box in
        row-major order, the last column fastest, as numpy.indices has it) into the tensors of `out`, a dict by the names
        of OUTPUTS; a name that is missing is passed as NULL, and `out` may be empty.  ctx: None, or a host or device
        (n_ctx, point_cols + 2) int64 array of PolyLib rows (marker, coefficients, constant); a point that violates one
        ends ST_OUTSIDE.  summary: None, a device int64 tensor of sweep_plan()["summary_words"], or True to allocate one.
        Returns (summary or None, out).  A fill and one launch on `stream` (default: torch's current), no synchronisation."""
        t = self.torch
        fn = _tape_fn("pipamd_tape_sweep", 64)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9
        clo, chi = self._box(lo, hi)
        n_ctx, cptr = 0, None
        if ctx is not None:
            import numpy as np
            ctx = (ctx if t.is_tensor(ctx) else t.as_tensor(np.asarray(ctx, dtype=np.int64).reshape(-1, self.point_cols + 2))).to(device=self.dev, dtype=t.int64)
            ctx = ctx.reshape(-1, self.point_cols + 2).contiguous()
            n_ctx = int(ctx.shape[0])
            cptr = C.c_void_p(ctx.data_ptr()) if n_ctx else None
        if summary is True:
            summary = t.empty(8 + 2 * self.info["leaves"], dtype=t.int64, device=self.dev)
        if summary is not None:
            assert summary.dtype == t.int64 and summary.is_contiguous() and summary.numel() >= 8 + 2 * self.info["leaves"]
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        ptrs = [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else None for k in self.OUTPUTS]
        rc = fn(self.e._h, self._h, clo, chi, n_ctx, self.point_cols + 2, cptr,
                C.c_void_p(summary.data_ptr()) if summary is not None else None, *ptrs, st)
        if rc in (-1, -3):
            raise TapeError(rc, lib().pipamd_last_error().decode())
        _check(rc)
        self._ctx_alive = ctx  # (the rows stay allocated until the next sweep: the launch is asynchronous)
        return summary, out

    def sweep(self, lo, hi, ctx=None, outputs=OUTPUTS, stream=None):
        """the tape over the box lo .. hi with a summary: (summary tensor, dict of the per-point tensors named in
        `outputs`); outputs=() sweeps for the summary alone.  dual_num / dual_den are left out when the tape has no
        dual lists.  See sweep_into and sweep_summary."""
        names = tuple(k for k in outputs if self.ndual or not k.startswith("dual"))
        n = self.sweep_plan(lo, hi)["n_points"]
        return self.sweep_into(lo, hi, self.outputs(n, names), ctx, True, stream)

    # ---- a sweep's values reduced per unknown (pipamd_tape_sweep_values)
    def values_plan(self, lo, hi):
        """values_plan() for this tape: n_points, summary_words, work_bytes, staged"""
        return values_plan(self.info, self.bits, self.nvar, self.point_cols, lo, hi)

    def sweep_values_into(self, lo, hi, summary, work, ctx=None, stream=None):
        """pipamd_tape_sweep_values: over the box lo .. hi under the context `ctx` (box, order and rows as sweep_into has
        them), per unknown the counts, the minimum and the maximum with the smallest k that attains them, and the exact sum
        of the integer values handed out, into `summary`, a device int64 tensor of values_plan()["summary_words"]; `work`
        is a device tensor of at least values_plan()["work_bytes"] bytes.  Neither needs initialising.  Returns `summary`
        (see values_summary).  A fill and two launches on `stream` (default: torch's current), no synchronisation."""
        t = self.torch
        fn = _tape_fn("pipamd_tape_sweep_values", 64)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_size_t, C.c_void_p]
        clo, chi = self._box(lo, hi)
        n_ctx, cptr = 0, None
        if ctx is not None:
            import numpy as np
            ctx = (ctx if t.is_tensor(ctx) else t.as_tensor(np.asarray(ctx, dtype=np.int64).reshape(-1, self.point_cols + 2))).to(device=self.dev, dtype=t.int64)
            ctx = ctx.reshape(-1, self.point_cols + 2).contiguous()
            n_ctx = int(ctx.shape[0])
            cptr = C.c_void_p(ctx.data_ptr()) if n_ctx else None
        assert summary.dtype == t.int64 and summary.is_contiguous() and summary.numel() >= 8 + 16 * self.nvar
        assert work.is_contiguous()
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        rc = fn(self.e._h, self._h, clo, chi, n_ctx, self.point_cols + 2, cptr, C.c_void_p(summary.data_ptr()),
                C.c_void_p(work.data_ptr()), work.numel() * work.element_size(), st)
        if rc in (-1, -3):
            raise TapeError(rc, lib().pipamd_last_error().decode())
        _check(rc)
        self._ctx_alive = ctx  # (the rows stay allocated until the next sweep: the launch is asynchronous)
        return summary

    def sweep_values(self, lo, hi, ctx=None, stream=None):
        """sweep_values_into with a fresh summary and work tensor: the summary tensor (see values_summary)"""
        t = self.torch
        plan = self.values_plan(lo, hi)
        summary = t.empty(plan["summary_words"], dtype=t.int64, device=self.dev)
        work = t.empty(max(1, plan["work_bytes"] // 8), dtype=t.int64, device=self.dev)  # (never a null pointer)
        self._work_alive = work  # (until the next call: the launches are asynchronous)
        return self.sweep_values_into(lo, hi, summary, work, ctx, stream)

    # ---- two tapes compared by value at points (pipamd_tape_compare / pipamd_tape_compare_sweep)
    CMP_OUTPUTS = ("class", "where", "status_a", "status_b")

    def compare_plan(self, other, lo, hi):
        """compare_plan() for this tape against `other`: n_points, staged"""
        return compare_plan(self.info, self.bits, other.info, other.bits, self.point_cols, lo, hi)

    def compare_outputs(self, n, names=CMP_OUTPUTS):
        """fresh int32 device tensors for `n` points, by the names of CMP_OUTPUTS"""
        return {k: self.torch.empty((n,), dtype=self.torch.int32, device=self.dev) for k in names}

    def _compare_tail(self, out, summary, stream):
        t = self.torch
        if summary is True:
            summary = t.empty(CMP_WORDS, dtype=t.int64, device=self.dev)
        if summary is not None:
            assert summary.dtype == t.int64 and summary.is_contiguous() and summary.numel() >= CMP_WORDS
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        ptrs = [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else None for k in self.CMP_OUTPUTS]
        return summary, [C.c_void_p(summary.data_ptr()) if summary is not None else None] + ptrs + [st]

    @staticmethod
    def _compare_rc(rc):
        if rc in (-1, -3):
            raise TapeError(rc, lib().pipamd_last_error().decode())
        _check(rc)

    def compare_into(self, other, points, out, dual=False, summary=None, stream=None):
        """pipamd_tape_compare: this tape (a) against `other` (b), a Tape of the same engine, nvar and point_cols and of
        either cell width, at `points` as eval() takes them, into the int32 tensors of `out`, a dict by the names of
        CMP_OUTPUTS (a missing name is passed as NULL; `out` may be empty).  dual: compare the dual lists too
        (PIPAMD_CMP_DUAL).  summary: None, a device int64 tensor of CMP_WORDS, or True to allocate one.  Returns
        (summary or None, out).  A fill and one launch on `stream` (default: torch's current), no synchronisation."""
        n, pts = self._points(points)
        fn = _tape_fn("pipamd_tape_compare", 64)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64] + [C.c_void_p] * 7
        summary, tail = self._compare_tail(out, summary, stream)
        self._compare_rc(fn(self.e._h, self._h, other._h, CMP_DUAL if dual else 0, n,
                            C.c_void_p(pts.data_ptr()) if pts is not None else None, *tail))
        self._cmp_alive = pts  # (the points stay allocated until the next call: the launch is asynchronous)
        return summary, out

    def compare(self, other, points, dual=False, outputs=CMP_OUTPUTS, stream=None):
        """this tape against `other` at `points`, with a summary: (summary tensor, dict of the tensors named in
        `outputs`); outputs=() compares for the summary alone.  See compare_into and compare_summary."""
        n, pts = self._points(points)
        return self.compare_into(other, pts if pts is not None else n, self.compare_outputs(n, tuple(outputs)), dual, True, stream)

    def compare_sweep_into(self, other, lo, hi, out, ctx=None, dual=False, summary=None, stream=None):
        """pipamd_tape_compare_sweep: compare_into at every integer point of the box lo .. hi under the context `ctx`,
        box, order and rows as sweep_into has them; a point that violates a row is CMP_OUTSIDE."""
        t = self.torch
        fn = _tape_fn("pipamd_tape_compare_sweep", 64)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        clo, chi = self._box(lo, hi)
        n_ctx, cptr = 0, None
        if ctx is not None:
            import numpy as np
            ctx = (ctx if t.is_tensor(ctx) else t.as_tensor(np.asarray(ctx, dtype=np.int64).reshape(-1, self.point_cols + 2))).to(device=self.dev, dtype=t.int64)
            ctx = ctx.reshape(-1, self.point_cols + 2).contiguous()
            n_ctx = int(ctx.shape[0])
            cptr = C.c_void_p(ctx.data_ptr()) if n_ctx else None
        summary, tail = self._compare_tail(out, summary, stream)
        self._compare_rc(fn(self.e._h, self._h, other._h, CMP_DUAL if dual else 0, clo, chi, n_ctx, self.point_cols + 2, cptr, *tail))
        self._cmp_alive = ctx
        return summary, out

    def compare_sweep(self, other, lo, hi, ctx=None, dual=False, outputs=CMP_OUTPUTS, stream=None):
        """this tape against `other` over the box lo .. hi with a summary: (summary tensor, dict of the tensors named in
        `outputs`); outputs=() compares for the summary alone, whatever the size of the box."""
        n = self.compare_plan(other, lo, hi)["n_points"]
        return self.compare_sweep_into(other, lo, hi, self.compare_outputs(n, tuple(outputs)), ctx, dual, True, stream)


ST_OUTSIDE = 11  # pipamd_tape_sweep: the point violates a row of the context (PIPAMD_ST_OUTSIDE)
SWEEP_STATUS = (("solution", ST_SOLUTION), ("nil", ST_NIL), ("range", ST_RANGE), ("outside", ST_OUTSIDE))


class TapeSweepPlan(C.Structure):
    """struct pipamd_tape_sweep_plan"""
    _fields_ = [("n_points", C.c_int64), ("summary_words", C.c_int64), ("binned", C.c_int32), ("reserved", C.c_int32)]


def sweep_plan(info, bits, point_cols, lo, hi):
    """pipamd_tape_sweep_plan: {"n_points", "summary_words", "binned"} for a tape with `info` (the dict of tape_check, or a
    TapeInfo) swept over the box lo .. hi, or TapeError where the box is refused.  Host only."""
    fn = _tape_fn("pipamd_tape_sweep_plan", 64)
    fn.argtypes = [C.POINTER(TapeInfo), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TapeSweepPlan)]
    if isinstance(info, dict):
        info = TapeInfo(**{k: int(v) for k, v in info.items()})
    n = max(1, len(lo))
    clo, chi = (C.c_int64 * n)(*[int(v) for v in lo]), (C.c_int64 * n)(*[int(v) for v in hi])
    plan = TapeSweepPlan()
    rc = fn(C.byref(info), int(bits), int(point_cols), clo, chi, C.byref(plan))
    if rc != 0:
        raise TapeError(rc, lib().pipamd_last_error().decode())
    return {"n_points": int(plan.n_points), "summary_words": int(plan.summary_words), "binned": int(plan.binned)}


def sweep_summary(tensor, leaves):
    """a sweep's summary (device or host int64 tensor, or a sequence) as a dict: counts and first by status name
    ("solution", "nil", "range", "outside"; first: the smallest k, -1 if none), leaf_count and leaf_first by leaf ordinal"""
    w = [int(v) for v in (tensor.cpu().tolist() if hasattr(tensor, "cpu") else tensor)]
    L = int(leaves)
    assert len(w) >= 8 + 2 * L
    return {"counts": {n: w[i] for i, (n, _) in enumerate(SWEEP_STATUS)},
            "first": {n: w[4 + i] for i, (n, _) in enumerate(SWEEP_STATUS)},
            "leaf_count": w[8:8 + L], "leaf_first": w[8 + L:8 + 2 * L]}


VALUES_MAX_NVAR, VALUES_HEAD, VALUES_REC = 64, 8, 16


class TapeValuesPlan(C.Structure):
    """struct pipamd_tape_values_plan"""
    _fields_ = [("n_points", C.c_int64), ("summary_words", C.c_int64), ("work_bytes", C.c_int64), ("staged", C.c_int32),
                ("reserved", C.c_int32)]


def values_plan(info, bits, nvar, point_cols, lo, hi):
    """pipamd_tape_sweep_values_plan: {"n_points", "summary_words", "work_bytes", "staged"} for a tape with `info` (the
    dict of tape_check, or a TapeInfo) and `nvar` unknowns swept over the box lo .. hi, or TapeError where it is refused.
    Host only."""
    fn = _tape_fn("pipamd_tape_sweep_values_plan", 64)
    fn.argtypes = [C.POINTER(TapeInfo), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TapeValuesPlan)]
    if isinstance(info, dict):
        info = TapeInfo(**{k: int(v) for k, v in info.items()})
    n = max(1, len(lo))
    clo, chi = (C.c_int64 * n)(*[int(v) for v in lo]), (C.c_int64 * n)(*[int(v) for v in hi])
    plan = TapeValuesPlan()
    rc = fn(C.byref(info), int(bits), int(nvar), int(point_cols), clo, chi, C.byref(plan))
    if rc != 0:
        raise TapeError(rc, lib().pipamd_last_error().decode())
    return {"n_points": int(plan.n_points), "summary_words": int(plan.summary_words), "work_bytes": int(plan.work_bytes),
            "staged": int(plan.staged)}


def _signed(limbs):
    """little-endian int64 limbs of a two's complement number as a Python int"""
    v = sum((int(w) & ((1 << 64) - 1)) << (64 * i) for i, w in enumerate(limbs))
    return v - (1 << (64 * len(limbs))) if v >> (64 * len(limbs) - 1) else v


def values_summary(tensor, nvar):
    """the summary of sweep_values (device or host int64 tensor, or a sequence) in Python ints: counts and first by status
    name as sweep_summary has them, and "unknowns": per unknown a dict with n_int, n_frac, n_unbounded, min, k_min, max,
    k_max, sum"""
    w = [int(v) for v in (tensor.cpu().tolist() if hasattr(tensor, "cpu") else tensor)]
    assert len(w) >= VALUES_HEAD + VALUES_REC * int(nvar)
    out = {"counts": {n: w[i] for i, (n, _) in enumerate(SWEEP_STATUS)},
           "first": {n: w[4 + i] for i, (n, _) in enumerate(SWEEP_STATUS)}, "unknowns": []}
    for i in range(int(nvar)):
        r = w[VALUES_HEAD + VALUES_REC * i:VALUES_HEAD + VALUES_REC * (i + 1)]
        out["unknowns"].append({"n_int": r[0], "n_frac": r[1], "n_unbounded": r[2], "min": _signed(r[4:6]), "k_min": r[6],
                                "max": _signed(r[7:9]), "k_max": r[9], "sum": _signed(r[10:13])})
    return out


# pipamd_tape_compare: the class of a point (PIPAMD_CMP_*), the summary's words, the flag
CMP_SAME, CMP_STATUS, CMP_VALUE, CMP_RANGE, CMP_OUTSIDE = range(5)
CMP_CLASSES = ("same", "status", "value", "range", "outside")
CMP_WORDS = 10
CMP_DUAL = 1


class TapeComparePlan(C.Structure):
    """struct pipamd_tape_compare_plan"""
    _fields_ = [("n_points", C.c_int64), ("staged", C.c_int32), ("reserved", C.c_int32)]


def compare_plan(info_a, bits_a, info_b, bits_b, point_cols, lo, hi):
    """pipamd_tape_compare_plan: {"n_points", "staged"} for tapes with info_a / info_b (dicts of tape_check, or TapeInfo)
    of bits_a / bits_b compared over the box lo .. hi, or TapeError where the pair or the box is refused.  Host only."""
    fn = _tape_fn("pipamd_tape_compare_plan", 64)
    fn.argtypes = [C.POINTER(TapeInfo), C.c_int, C.POINTER(TapeInfo), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                   C.POINTER(TapeComparePlan)]
    infos = [TapeInfo(**{k: int(v) for k, v in i.items()}) if isinstance(i, dict) else i for i in (info_a, info_b)]
    n = max(1, len(lo))
    clo, chi = (C.c_int64 * n)(*[int(v) for v in lo]), (C.c_int64 * n)(*[int(v) for v in hi])
    plan = TapeComparePlan()
    rc = fn(C.byref(infos[0]), int(bits_a), C.byref(infos[1]), int(bits_b), int(point_cols), clo, chi, C.byref(plan))
    if rc != 0:
        raise TapeError(rc, lib().pipamd_last_error().decode())
    return {"n_points": int(plan.n_points), "staged": int(plan.staged)}


def compare_summary(tensor):
    """a comparison's summary (device or host int64 tensor, or a sequence) as {"counts": {...}, "first": {...}} by class
    name ("same", "status", "value", "range", "outside"; first: the smallest k, -1 if none)"""
    w = [int(v) for v in (tensor.cpu().tolist() if hasattr(tensor, "cpu") else tensor)]
    assert len(w) >= CMP_WORDS
    return {"counts": {n: w[i] for i, n in enumerate(CMP_CLASSES)}, "first": {n: w[5 + i] for i, n in enumerate(CMP_CLASSES)}}


class TapeSetInfo(C.Structure):
    """pipamd_tape_set_info"""
    _fields_ = [("words", C.c_int64)] + [(n, C.c_int32) for n in ("n", "bits", "point_cols", "nvar", "ndual", "slots")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TapeSet:
    """Compiled tapes (Tape objects of one engine and one width, edited or not) evaluated in ONE launch
    (pipamd_tape_set_create / pipamd_tape_set_eval): point k is of tape tape_index[k].  Points, unknowns and dual values
    are padded to the set's maxima (info["point_cols"], info["nvar"], info["ndual"]); a tape reads its first columns and
    values beyond its own counts are (0, 0).  The tapes may be closed once the set exists."""
    OUTPUTS = Tape.OUTPUTS

    def __init__(self, engine, tapes):
        import torch
        self.torch = torch
        self.e = engine
        L = lib()
        if not hasattr(L, "pipamd_tape_set_create"):
            raise RuntimeError("libpipamd has no pipamd_tape_set_create: rebuild the library")
        fn = L.pipamd_tape_set_create
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(TapeSetInfo)]
        n = len(tapes)
        arr = (C.c_void_p * max(1, n))(*[t._h.value if isinstance(t, Tape) else t for t in tapes])
        self._h = C.c_void_p()
        info = TapeSetInfo()
        rc = fn(engine._h, n, arr, C.byref(self._h), C.byref(info))
        if rc != 0:
            raise TapeError(rc, L.pipamd_last_error().decode())
        self.info = info.as_dict()
        self.n, self.bits = self.info["n"], self.info["bits"]
        self.point_cols, self.nvar, self.ndual = self.info["point_cols"], self.info["nvar"], self.info["ndual"]
        self.dev = torch.device("cuda", engine.device)

    def close(self):
        if self._h:
            lib().pipamd_tape_set_free.argtypes = [C.c_void_p]
            lib().pipamd_tape_set_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _args(self, tape_index, points):
        t = self.torch
        idx = (tape_index if t.is_tensor(tape_index) else t.as_tensor(tape_index, dtype=t.int32))
        idx = idx.to(device=self.dev, dtype=t.int32).reshape(-1).contiguous()
        n = int(idx.shape[0])
        if points is None:
            assert self.point_cols == 0, "points may be left out only when no tape of the set has parameters"
            return n, idx, None
        points = (points if t.is_tensor(points) else t.as_tensor(points, dtype=t.int64)).to(device=self.dev, dtype=t.int64)
        points = points.reshape(n, self.point_cols).contiguous()
        return n, idx, (points if self.point_cols else None)

    def outputs(self, n, names=OUTPUTS):
        """fresh device tensors for `n` points, shaped by the set's maxima (a trailing 2 for a 128-bit set)"""
        t = self.torch
        ew = (2,) if self.bits == 128 else ()
        shapes = {"status": ((n,), t.int32), "leaf": ((n,), t.int32), "x_num": ((n, self.nvar) + ew, t.int64),
                  "x_den": ((n, self.nvar) + ew, t.int64), "dual_num": ((n, self.ndual) + ew, t.int64),
                  "dual_den": ((n, self.ndual) + ew, t.int64)}
        return {k: t.empty(shapes[k][0], dtype=shapes[k][1], device=self.dev) for k in names}

    def eval_into(self, tape_index, points, out, stream=None):
        """pipamd_tape_set_eval into the tensors of `out`, a dict by the names of OUTPUTS; a name that is missing is
        passed as NULL.  One launch on `stream` (a raw hipStream_t handle; default: torch's current stream), no
        synchronisation."""
        n, idx, pts = self._args(tape_index, points)
        fn = lib().pipamd_tape_set_eval
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)
        ptrs = [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else None for k in self.OUTPUTS]
        _check(fn(self.e._h, self._h, n, C.c_void_p(idx.data_ptr()) if n else None,
                  C.c_void_p(pts.data_ptr()) if pts is not None and n else None, *ptrs, st))
        return out

    def eval(self, tape_index, points, stream=None):
        """the set at `points`, (n, point_cols) int64, point k of tape tape_index[k]: device tensors (status, leaf, x_num,
        x_den) and, where a tape of the set has dual lists, (dual_num, dual_den).  Does not synchronise."""
        n, idx, pts = self._args(tape_index, points)
        names = self.OUTPUTS if self.ndual else self.OUTPUTS[:4]
        out = self.eval_into(idx, pts, self.outputs(n, names), stream)
        return tuple(out[k] for k in names)

    def tape_info(self, i):
        """pipamd_tape_set_tape_info: what the set keeps of tape i -- the dict of its pipamd_tape_info with point_cols,
        nvar and ndual beside it -- or TapeError for an index outside the set"""
        fn = _tape_fn("pipamd_tape_set_tape_info", 64)
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(TapeInfo)] + [C.POINTER(C.c_int32)] * 3
        info, cols, nvar, ndual = TapeInfo(), C.c_int32(), C.c_int32(), C.c_int32()
        rc = fn(self._h, int(i), C.byref(info), C.byref(cols), C.byref(nvar), C.byref(ndual))
        if rc != 0:
            raise TapeError(rc, lib().pipamd_last_error().decode())
        return dict(info.as_dict(), point_cols=cols.value, nvar=nvar.value, ndual=ndual.value)

    def sweep_jobs(self, jobs):
        """pipamd_tape_set_sweep_create: jobs is a list of (tape, lo, hi, ctx or None) -- a tape index of the set, the
        inclusive bounds of a box of that tape's point_cols values, and None or (n_ctx, point_cols + 2) PolyLib rows on
        the host.  Returns a TapeSetSweep (which keeps this set alive), or TapeError where a job is refused."""
        return TapeSetSweep(self, jobs)


class TapeSweepJob(C.Structure):
    """pipamd_tape_sweep_job"""
    _fields_ = [("tape", C.c_int32), ("n_ctx", C.c_int32), ("lo", C.c_void_p), ("hi", C.c_void_p), ("ctx", C.c_void_p)]


def _sweep_jobs(jobs, point_cols):
    """[(tape, lo, hi, ctx or None)] -> (array of TapeSweepJob, the host arrays it points into).  point_cols(j): the
    columns of job j's tape, or None where it is not known (the rows are then taken as they are shaped)"""
    import numpy as np
    arr, keep = (TapeSweepJob * max(1, len(jobs)))(), []
    for j, (tape, lo, hi, ctx) in enumerate(jobs):
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
        assert len(lo) == len(hi), "a box has as many bounds on either side"
        cols = point_cols(j)
        n = max(1, len(lo))
        clo, chi = (C.c_int64 * n)(*lo), (C.c_int64 * n)(*hi)
        keep += [clo, chi]
        arr[j].tape, arr[j].n_ctx = int(tape), 0
        arr[j].lo, arr[j].hi = C.addressof(clo), C.addressof(chi)
        if ctx is not None and len(ctx):
            rows = np.ascontiguousarray(np.asarray(ctx, dtype=np.int64).reshape(-1, (len(lo) if cols is None else cols) + 2))
            keep.append(rows)
            arr[j].n_ctx, arr[j].ctx = int(rows.shape[0]), rows.ctypes.data
    return arr, keep


def set_sweep_plan(jobs, leaves, point_cols):
    """pipamd_tape_set_sweep_plan for jobs [(tape, lo, hi, ctx or None)] whose tapes have leaves[j] leaves and
    point_cols[j] point columns: {"points": [...], "summary_off": [...], "chunk_off": [...]}, or TapeError where a job is
    refused.  Host only."""
    fn = _tape_fn("pipamd_tape_set_sweep_plan", 64)
    fn.argtypes = [C.c_int] + [C.c_void_p] * 6
    n = len(jobs)
    arr, keep = _sweep_jobs(jobs, lambda j: int(point_cols[j]))
    cl, cc = (C.c_int64 * max(1, n))(*[int(v) for v in leaves]), (C.c_int32 * max(1, n))(*[int(v) for v in point_cols])
    pts, so, co = (C.c_int64 * max(1, n))(), (C.c_int64 * (n + 1))(), (C.c_int64 * (n + 1))()
    rc = fn(n, arr, cl, cc, pts, so, co)
    if rc != 0:
        raise TapeError(rc, lib().pipamd_last_error().decode())
    return {"points": list(pts)[:n], "summary_off": list(so), "chunk_off": list(co)}


class TapeSetSweep:
    """The jobs of a TapeSet -- a tape, a box, a context each -- swept in ONE launch with a summary per job
    (pipamd_tape_set_sweep_create / pipamd_tape_set_sweep_run).  summary_off[j] .. summary_off[j + 1] are job j's words of
    the summary tensor, laid out as Tape.sweep's; `leaves` has every job's leaf count."""

    def __init__(self, tset, jobs):
        self.torch = tset.torch
        self.set = tset  # (the set must outlive the sweep)
        self.e, self.dev = tset.e, tset.dev
        fn = _tape_fn("pipamd_tape_set_sweep_create", 64)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
        jobs = list(jobs)
        self.n = len(jobs)
        cols = {}

        def point_cols(j):
            t = int(jobs[j][0])
            if t not in cols:
                cols[t] = tset.tape_info(t)["point_cols"] if 0 <= t < tset.n else None
            assert cols[t] is None or len(jobs[j][1]) == cols[t], "a box has point_cols bounds on either side"
            return cols[t]

        arr, keep = _sweep_jobs(jobs, point_cols)
        so = (C.c_int64 * (self.n + 1))()
        self._h = C.c_void_p()
        rc = fn(self.e._h, tset._h, self.n, arr, C.byref(self._h), so)
        if rc in (-1, -3):
            raise TapeError(rc, lib().pipamd_last_error().decode())
        _check(rc)
        self.summary_off = list(so)
        self.words = self.summary_off[-1]
        self.leaves = [(b - a - 8) // 2 for a, b in zip(self.summary_off, self.summary_off[1:])]

    def close(self):
        if self._h:
            lib().pipamd_tape_set_sweep_free.argtypes = [C.c_void_p]
            lib().pipamd_tape_set_sweep_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_into(self, summary, stream=None):
        """pipamd_tape_set_sweep_run into `summary`, a contiguous device int64 tensor of at least summary_off[-1] words;
        it need not be initialised.  A fill and one launch on `stream` (default: torch's current), no synchronisation."""
        t = self.torch
        assert summary.dtype == t.int64 and summary.is_contiguous() and summary.numel() >= self.words
        fn = lib().pipamd_tape_set_sweep_run
        fn.argtypes = [C.c_void_p] * 4
        st = C.c_void_p(stream) if stream is not None else C.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        _check(fn(self.e._h, self._h, C.c_void_p(summary.data_ptr()) if self.words else None, st))
        return summary

    def run(self, stream=None):
        """run_into a fresh tensor of summary_off[-1] words"""
        return self.run_into(self.torch.empty(self.words, dtype=self.torch.int64, device=self.dev), stream)

    def summaries(self, tensor):
        """the summary tensor of a run as a list of what sweep_summary returns, per job (synchronises through the copy)"""
        w = tensor.cpu().tolist() if hasattr(tensor, "cpu") else list(tensor)
        return [sweep_summary(w[a:b], L) for a, b, L in zip(self.summary_off, self.summary_off[1:], self.leaves)]

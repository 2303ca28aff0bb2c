"""A solution tape evaluated at a parameter point, in Python ints: what pipamd_tape_check validates and counts, what
pipamd_tape_compile lays out and what pipamd_tape_eval computes per point, in both entry widths.  Cells are
(kind, param1, param2) as piplib_amd.engine hands them out.  The grammar (P = parameters in scope, nparm at the root):

    item := NEW(n) DIV FORM(P+1) VAL x (P+1) VAL(D)   item          n == P, every denominator 1, D > 0
          | IF FORM(P+1) VAL x (P+1)   item   item                  one positive denominator
          | LIST(nvar) { FORM(P+1) VAL x (P+1) } x nvar  [ LIST(ndual) { FORM(1) VAL } x ndual ]
          | NIL

A new parameter is floor((sum c_j theta_j + c) / D) (integrer.c:171-180) and is in scope for the one item behind it; a
condition takes its first item when sum n_j theta_j + n_c >= 0 (traiter.c:719-737); a leaf hands out every unknown
N / D in lowest terms, (0, 1) for N == 0 (traiter.c:262-268, 282-290).  Test helper only."""
from math import gcd

NIL, IF, LIST, FORM, NEW, DIV, VAL = range(1, 8)
ST_SOLUTION, ST_NIL, ST_RANGE = 1, 2, 7
E_INVALID, E_TOOLARGE = -1, -3

# the kernel's layout (include/piplib_amd.h, PIPAMD_TAPE_*)
MAX_SLOTS = 32       # largest P + 1 a tape may have
BLOCK = 128          # points per workgroup
LDS_BYTES = 65536    # parameters in scope + staged program


class TapeError(ValueError):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def _bad(why):
    raise TapeError(E_INVALID, why)


def parse(cells, nvar, nparm, ndual=0, bits=64, reserved=0):
    """(nodes, info).  nodes, in tape order: ("new", P, coefs, D) | ("if", P, nums, else_index) |
    ("leaf", P, ordinal, [(nums, den)] x nvar, [(num, den)] x ndual) | ("nil", P, ordinal); info: the counts of
    pipamd_tape_info.  Raises TapeError(E_INVALID) / TapeError(E_TOOLARGE) where pipamd_tape_check returns them."""
    assert bits in (64, 128)
    ew = bits // 64
    if nvar < 0 or nparm < 0 or ndual < 0:
        _bad("negative count")
    if reserved != 0:
        _bad("reserved")
    cells = [tuple(int(v) for v in c) for c in cells]
    n = len(cells)
    pos = 0

    def take(kind, what):
        nonlocal pos
        if pos >= n:
            _bad("truncated: " + what)
        c = cells[pos]
        if c[0] != kind:
            _bad(f"cell {pos}: kind {c[0]} where {what} belongs")
        pos += 1
        return c

    def form(length, what, one=False):
        f = take(FORM, what)
        if f[1] != length:
            _bad(f"{what}: form of {f[1]} values, not {length}")
        vals = [take(VAL, what) for _ in range(length)]
        den = vals[0][2] if vals else 1
        if den <= 0 or any(v[2] != den for v in vals) or (one and den != 1):
            _bad(f"{what}: denominators")
        return [v[1] for v in vals], den

    nodes = []
    info = {"leaves": 0, "ifs": 0, "news": 0, "words": 0, "slots": nparm + 1, "depth": 0}
    work = [(nparm, 1, None)] if n else []
    while work:
        P, depth, patch = work.pop()
        if patch is not None:
            nodes[patch][3] = len(nodes)
        info["slots"] = max(info["slots"], P + 1)
        info["depth"] = max(info["depth"], depth)
        if pos >= n:
            _bad("truncated: an item")
        kind, p1, _ = cells[pos]
        pos += 1
        if kind == NEW:
            if p1 != P:
                _bad(f"newparm {p1} with {P} parameters in scope")
            take(DIV, "div")
            coefs, _ = form(P + 1, "div", one=True)
            d = take(VAL, "divisor")
            if d[2] != 1 or d[1] <= 0:
                _bad("divisor")
            nodes.append(["new", P, coefs, d[1]])
            info["news"] += 1
            info["words"] += 1 + ew * (P + 2)
            work.append((P + 1, depth + 1, None))
        elif kind == IF:
            nums, _ = form(P + 1, "condition")
            nodes.append(["if", P, nums, None])
            info["ifs"] += 1
            info["words"] += 1 + ew * (P + 1)
            work.append((P, depth + 1, len(nodes) - 1))
            work.append((P, depth + 1, None))
        elif kind == LIST:
            if p1 != nvar:
                _bad(f"list of {p1} forms, not {nvar}")
            forms = [form(P + 1, "unknown") for _ in range(nvar)]
            duals = []
            if ndual:
                lst = take(LIST, "the dual list")
                if lst[1] != ndual:
                    _bad(f"dual list of {lst[1]} forms, not {ndual}")
                for _ in range(ndual):
                    v, den = form(1, "dual")
                    duals.append(reduce(v[0], den))
            nodes.append(["leaf", P, info["leaves"], forms, duals])
            info["leaves"] += 1
            info["words"] += 1 + ew * (nvar * (P + 2) + 2 * ndual)
        elif kind == NIL:
            nodes.append(["nil", P, info["leaves"]])
            info["leaves"] += 1
            info["words"] += 1
        else:
            _bad(f"cell {pos - 1}: kind {kind} where an item belongs")
    if pos != n:
        _bad("cells behind the end of the root item")
    if info["slots"] > MAX_SLOTS:
        raise TapeError(E_TOOLARGE, f"{info['slots']} slots")
    if info["words"] >= 1 << 31:
        raise TapeError(E_TOOLARGE, "program")
    info["staged"] = int(n > 0 and 8 * info["words"] + slot_bytes(info["slots"], bits) <= LDS_BYTES)
    return nodes, info


def slot_bytes(slots, bits):
    """LDS the parameters in scope take: one row of BLOCK values per parameter"""
    return (slots - 1) * BLOCK * (bits // 8)


def check(cells, nvar, nparm, ndual=0, bits=64, reserved=0):
    return parse(cells, nvar, nparm, ndual, bits, reserved)[1]


def reduce(n, d):
    """N / D, D > 0, as a leaf hands it out"""
    g = gcd(abs(n), d)
    return n // g, d // g


def _fits(v, bits):
    return -(1 << (bits - 1)) <= v < (1 << (bits - 1))


class _Range(Exception):
    pass


def _value(coefs, theta, bits):
    """sum c_j theta_j + c.  64: exact.  128: every product and every running sum, in cell order, must stay in 128 bits"""
    if bits == 64:
        return sum(c * t for c, t in zip(coefs, theta)) + coefs[-1]
    acc = 0
    for c, t in zip(coefs, theta):
        p = c * t
        if not _fits(p, 128):
            raise _Range()
        acc += p
        if not _fits(acc, 128):
            raise _Range()
    acc += coefs[-1]
    if not _fits(acc, 128):
        raise _Range()
    return acc


def evaluate(nodes, nvar, nparm, ndual, point, bits=64, trace=None):
    """(status, leaf, x, dual) at one point: x and dual are lists of reduced (numerator, denominator) pairs, (0, 0)
    throughout unless the status is ST_SOLUTION; leaf is -1 for an empty tape and a ST_RANGE point.  trace, a dict, gets
    the counts "news" (new parameters computed) and "zeros" (conditions that were exactly 0) added."""
    zeros = [(0, 0)] * nvar, [(0, 0)] * ndual
    theta = [int(t) for t in point]
    assert len(theta) == nparm
    if not nodes:
        return (ST_NIL, -1) + zeros
    pc = 0
    try:
        while True:
            nd = nodes[pc]
            P = nd[1]
            if nd[0] == "new":
                q = _value(nd[2], theta[:P], bits) // nd[3]
                if not _fits(q, bits):
                    raise _Range()
                theta[P:] = [q]
                pc += 1
                if trace is not None:
                    trace["news"] = trace.get("news", 0) + 1
            elif nd[0] == "if":
                v = _value(nd[2], theta[:P], bits)
                if trace is not None and v == 0:
                    trace["zeros"] = trace.get("zeros", 0) + 1
                assert nd[3] > pc
                pc = pc + 1 if v >= 0 else nd[3]
            elif nd[0] == "nil":
                return (ST_NIL, nd[2]) + zeros
            else:
                x = [reduce(_value(nums, theta[:P], bits), den) for nums, den in nd[3]]
                if not all(_fits(n, bits) for n, _ in x):
                    raise _Range()
                return ST_SOLUTION, nd[2], x, list(nd[4])
    except _Range:
        return (ST_RANGE, -1) + zeros


def evaluate_cells(cells, nvar, nparm, ndual, points, bits=64, trace=None):
    nodes, _ = parse(cells, nvar, nparm, ndual, bits)
    return [evaluate(nodes, nvar, nparm, ndual, p, bits, trace) for p in points]

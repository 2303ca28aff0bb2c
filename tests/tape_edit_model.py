"""pip_solve's result edits on a solution tape, in Python ints: sol_vector_edit (sol.c:435-512) and sol_quast_edit
(sol.c:664-734) applied to the nodes tape_model.parse gives, what pipamd_tape_check_pip counts, and the edited quast at
a point as pipamd_tape_eval hands it out for a tape of pipamd_tape_compile_pip, in both entry widths.

With P the raw parameters in scope, bg = sol_bg, U = urs_parms, first_urs = U + (bg >= 0): column j < nparm of a form is
dropped when j == bg under SOL_REMOVE or when first_urs <= j < first_urs + U; the kept columns are renumbered in order
and a point has nparm - (REMOVE ? 1 : 0) - U values.  Conditions and new-parameter forms are only thinned.  In a
solution list SOL_SHIFT turns the coefficient at bg into n_bg - D before any drop; where that is not 0 the unknown is
unbounded: denominator 0 in what is handed out, the numerator kept.  SOL_NEGATE negates the unknown's exact value at the
point, before the range check and the reduction.  Dual lists stay as they are.  Test helper only."""
from math import gcd

import tape_model as tm
from tape_model import E_INVALID, E_TOOLARGE, ST_NIL, ST_RANGE, ST_SOLUTION, TapeError

SOL_SHIFT, SOL_NEGATE, SOL_REMOVE, SOL_DUAL = 1, 2, 4, 8
NO_EDIT = dict(sol_bg=0, urs_parms=0, sol_flags=0)


def _fits(v, bits):
    return -(1 << (bits - 1)) <= v < (1 << (bits - 1))


class Edit:
    """the three fields of pipamd_pip_info against a tape of `nparm` parameters; TapeError(E_INVALID) where
    pipamd_tape_check_pip refuses them"""

    def __init__(self, tape_nparm, sol_bg=0, urs_parms=0, sol_flags=0, reserved=0, **_):
        nparm = tape_nparm  # (the dict of pipamd_pip_info may be passed whole: its other fields are not looked at)
        self.nparm, self.bg, self.urs, self.flags = nparm, sol_bg, urs_parms, sol_flags
        self.active = bool(sol_bg or urs_parms or sol_flags or reserved)
        self.first_urs = urs_parms + (1 if sol_bg >= 0 else 0)
        if self.active:
            rm = bool(sol_flags & SOL_REMOVE)
            if (reserved != 0 or sol_flags & ~15 or urs_parms < 0 or sol_bg >= nparm
                    or (sol_flags & (SOL_SHIFT | SOL_REMOVE) and sol_bg < 0) or self.first_urs + urs_parms > nparm
                    or (rm and urs_parms > 0 and self.first_urs <= sol_bg < self.first_urs + urs_parms)):
                raise TapeError(E_INVALID, "edit")
        else:
            self.bg, self.urs, self.flags, self.first_urs = -1, 0, 0, 0
        self.shift = bool(self.flags & SOL_SHIFT)
        self.negate = bool(self.flags & SOL_NEGATE)
        self.remove = bool(self.flags & SOL_REMOVE)
        self.ndrop = (1 if self.remove else 0) + self.urs

    def dropped(self, j):
        return j < self.nparm and ((self.remove and j == self.bg) or self.first_urs <= j < self.first_urs + self.urs)

    def keep(self, vals):
        return [v for j, v in enumerate(vals) if not self.dropped(j)]

    @property
    def point_cols(self):
        return self.nparm - self.ndrop


def edit_nodes(cells, nvar, nparm, ndual=0, edit=None, bits=64, reserved=0):
    """(nodes, info, stats).  nodes as tape_model.parse gives them, P counting kept columns, with
    ("leaf", P, ordinal, [(nums, den, unbounded)] x nvar, duals, negate) and ("if", P, nums, else_index, den); info: the dict of pipamd_tape_info as
    pipamd_tape_check_pip fills it; stats["dropped_nonzero"]: dropped coefficients of conditions and new-parameter forms
    that were not 0.  Raises TapeError where pipamd_tape_check_pip returns an error."""
    if nvar < 0 or nparm < 0 or ndual < 0 or reserved != 0:
        raise TapeError(E_INVALID, "shape")
    ed = Edit(nparm, **(edit or NO_EDIT))
    ew = bits // 64
    try:
        raw, rinfo = tm.parse(cells, nvar, nparm, ndual, bits, reserved)
    except TapeError as err:
        if err.code != E_TOOLARGE:
            raise
        # (slots are counted on kept columns: parse again without the limit)
        lim, tm.MAX_SLOTS = tm.MAX_SLOTS, 1 << 40
        try:
            raw, rinfo = tm.parse(cells, nvar, nparm, ndual, bits, reserved)
        finally:
            tm.MAX_SLOTS = lim
    # (tape_model keeps no condition's denominator; the conditions come in cell order: IF, FORM, the first VAL)
    if_dens = [cells[k + 2][2] for k, c in enumerate(cells) if c[0] == tm.IF]
    nodes, words, toolarge = [], 0, False
    stats = {"dropped_nonzero": 0}
    slots = nparm - ed.ndrop + 1
    for nd in raw:
        P = nd[1] - ed.ndrop
        slots = max(slots, P + 1)
        if nd[0] == "new":
            stats["dropped_nonzero"] += sum(1 for j, v in enumerate(nd[2]) if ed.dropped(j) and v != 0)
            nodes.append(["new", P, ed.keep(nd[2]), nd[3]])
            words += 1 + ew * (P + 2)
        elif nd[0] == "if":
            stats["dropped_nonzero"] += sum(1 for j, v in enumerate(nd[2]) if ed.dropped(j) and v != 0)
            nodes.append(["if", P, ed.keep(nd[2]), nd[3], int(if_dens.pop(0))])
            words += 1 + ew * (P + 1)
        elif nd[0] == "leaf":
            forms = []
            for nums, den in nd[3]:
                nums, unbounded = list(nums), False
                if ed.shift:
                    nums[ed.bg] -= den
                    unbounded = nums[ed.bg] != 0
                    toolarge = toolarge or not _fits(nums[ed.bg], bits)
                forms.append((ed.keep(nums), den, unbounded))
            nodes.append(["leaf", P, nd[2], forms, nd[4], ed.negate])
            words += 1 + ew * (nvar * (P + 2) + 2 * ndual)
        else:
            nodes.append(["nil", P, nd[2]])
            words += 1
    if slots > tm.MAX_SLOTS or words >= 1 << 31:
        raise TapeError(E_TOOLARGE, f"{slots} slots")
    if toolarge:
        raise TapeError(E_TOOLARGE, "shifted coefficient")
    info = dict(rinfo, words=words, slots=slots)
    info["staged"] = int(len(cells) > 0 and 8 * words + tm.slot_bytes(slots, bits) <= tm.LDS_BYTES)
    return nodes, info, stats


def check(cells, nvar, nparm, ndual=0, edit=None, bits=64, reserved=0):
    return edit_nodes(cells, nvar, nparm, ndual, edit, bits, reserved)[1]


def point_cols(nparm, edit=None):
    return Edit(nparm, **(edit or NO_EDIT)).point_cols


def evaluate(nodes, nvar, ndual, point, bits=64, trace=None):
    """(status, leaf, x, dual) of edited nodes at one point of point_cols values, as pipamd_tape_eval hands them out:
    x[i] = (+-N / g, D / g or 0).  trace gets "news", "zeros" and "unbounded" (unknowns handed out over 0) added."""
    zeros = [(0, 0)] * nvar, [(0, 0)] * ndual
    theta = [int(t) for t in point]
    if not nodes:
        return (ST_NIL, -1) + zeros
    pc = 0
    try:
        while True:
            nd = nodes[pc]
            P = nd[1]
            assert len(theta) >= P
            if nd[0] == "new":
                q = tm._value(nd[2], theta[:P], bits) // nd[3]
                if not _fits(q, bits):
                    raise tm._Range()
                theta[P:] = [q]
                pc += 1
                if trace is not None:
                    trace["news"] = trace.get("news", 0) + 1
            elif nd[0] == "if":
                v = tm._value(nd[2], theta[:P], bits)
                if trace is not None and v == 0:
                    trace["zeros"] = trace.get("zeros", 0) + 1
                pc = pc + 1 if v >= 0 else nd[3]
            elif nd[0] == "nil":
                return (ST_NIL, nd[2]) + zeros
            else:
                x = []
                for nums, den, unbounded in nd[3]:
                    N = tm._value(nums, theta[:P], bits)
                    if nd[5]:
                        N = -N
                        if bits == 128 and not _fits(N, 128):
                            raise tm._Range()
                    n, d = tm.reduce(N, den)
                    if not _fits(n, bits):
                        raise tm._Range()
                    x.append((n, 0 if unbounded else d))
                    if unbounded and trace is not None:
                        trace["unbounded"] = trace.get("unbounded", 0) + 1
                return ST_SOLUTION, nd[2], x, list(nd[4])
    except tm._Range:
        return (ST_RANGE, -1) + zeros


def evaluate_cells(cells, nvar, nparm, ndual, points, edit=None, bits=64, trace=None):
    nodes, _, _ = edit_nodes(cells, nvar, nparm, ndual, edit, bits)
    return [evaluate(nodes, nvar, ndual, p, bits, trace) for p in points]


# ---------------------------------------------------------------- the edited quast as pip_quast_print prints it
def _printed(nums, den, negate=False, unbounded=False):
    """a vector as sol_vector_edit stores it: every value reduced on its own, negated, over 0 throughout if unbounded"""
    out = []
    for n in nums:
        g = gcd(n, den)
        out.append((-(n // g) if negate else n // g, 0 if unbounded else den // g))
    return out


def quast(nodes):
    """the edited nodes as the tree sol_quast_edit builds, in the dict form pipsolve_model._print takes; the dual list
    behind a solution list becomes the `then` quast, as sol.c:706-708 has it"""
    def item(i):
        q = dict(newparm=[], list=None, cond=None, then=None, orelse=None)
        while nodes[i][0] == "new":
            nd = nodes[i]
            q["newparm"].append((nd[1], _printed(nd[2], 1), nd[3]))
            i += 1
        nd = nodes[i]
        if nd[0] == "if":
            q["cond"] = _printed(nd[2], _cond_den(nd))
            q["then"] = item(i + 1)
            q["orelse"] = item(nd[3])
        elif nd[0] == "leaf":
            q["list"] = [_printed(nums, den, nd[5], unb) for nums, den, unb in nd[3]]
            if nd[4]:
                q["then"] = dict(newparm=[], list=[[d] for d in nd[4]], cond=None, then=None, orelse=None)
        return q
    return item(0) if nodes else None


def _cond_den(nd):
    return nd[4] if len(nd) > 4 else 1


# ---------------------------------------------------------------- a printed (edited) quast -> nodes
def nodes_from_text(text, point_cols):
    """the nodes of the quast pip_quast_print printed (piplib.c:198-317; no dual lists), None for "void".  The edit is
    already in the text: nothing is dropped, shifted or negated here.  An unknown printed over 0 is unbounded; its
    printed numerators were reduced against a denominator the text no longer has, so its form is (numerators, 1) and only
    the mark can be held to it."""
    import tape_cases as tc
    toks = tc._TOKEN.findall(text)
    assert "".join(toks) == "".join(text.split()), "unknown text in a printed quast"
    if toks == ["void"]:
        return None
    nodes, pos, leaves = [], [0], [0]

    def tok():
        pos[0] += 1
        return toks[pos[0] - 1]

    def vector():
        assert tok() == "#["
        vals = []
        while toks[pos[0]] != "]":
            n, _, d = tok().partition("/")
            vals.append((int(n), int(d) if d else 1))
        tok()
        if any(d == 0 for _, d in vals):
            assert all(d == 0 for _, d in vals)
            return [n for n, _ in vals], 1, True
        den = 1
        for _, d in vals:
            assert d > 0
            den = den * d // gcd(den, d)
        return [n * (den // d) for n, d in vals], den, False

    def item(P):
        while toks[pos[0]] == "(newparm":
            tok()
            assert int(tok()) == P and tok() == "(div"
            nums, den, unb = vector()
            assert den == 1 and not unb and len(nums) == P + 1
            nodes.append(["new", P, nums, int(tok())])
            assert tok() == ")" and tok() == ")"
            P += 1
        t = tok()
        if t == "()":
            nodes.append(["nil", P, leaves[0]])
            leaves[0] += 1
        elif t == "(if":
            nums, den, unb = vector()
            assert not unb and len(nums) == P + 1
            at = len(nodes)
            nodes.append(["if", P, nums, None, den])
            item(P)
            nodes[at][3] = len(nodes)
            item(P)
            assert tok() == ")"
        else:
            assert t == "(list", t
            forms = []
            while toks[pos[0]] != ")":
                forms.append(vector())
                assert len(forms[-1][0]) == P + 1
            tok()
            nodes.append(["leaf", P, leaves[0], forms, [], False])
            leaves[0] += 1

    item(point_cols)
    assert pos[0] == len(toks)
    return nodes


def answer_of(result):
    """one evaluation as the fixtures record an answer: [[numerator, denominator], ...], None without a solution"""
    st, _, x, _ = result
    return [list(p) for p in x] if st == ST_SOLUTION else None


def same_answer(got, want):
    """a model or device answer against a recorded one: equal, except that of an unbounded unknown (denominator 0) only
    the mark is compared"""
    if got is None or want is None:
        return got is None and want is None
    return len(got) == len(want) and all((g[1] == 0 and w[1] == 0) or list(g) == list(w) for g, w in zip(got, want))

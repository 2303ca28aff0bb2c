"""Cases of the determinant-replay probe (pipamd_debug_det_replay, csrc/pip_probe.hip): job headers and logs, the
launches they go through, and what each launch must leave -- by tests/replay_model.py alone.

TEST INFRASTRUCTURE ONLY.  tests/test_replay_cases.py checks on the CPU that every class of the list below is met, by
what the MODEL says of a case, not by what its builder meant; tests/test_gpu_det_replay_probe.py runs them.

A case: dict(bits, limbs (4), ldet, npiv, status, aux, log [(pivot, dpiv)], tail [(pivot, dpiv)]) -- `tail` stands in the
log area behind the job's nlog pairs, where no replay may look; aux: the header's word of that name, which tells a job
that ended in a pivot without a column (counted, not logged).  A launch: dict(bits, jobs [case], list or None): the replay
of `bits`-bit entries over the jobs, all of them or the listed ones; a job of the other width, or off the list, comes
back as it went in.
"""
import functools
import math
import random

import replay_model as rm

LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512)
OVERFLOW_AT = (0, 3, 4, 7, 8, 63, 64, 65, 127, 128, "last")
JOBS = (1, 63, 64, 65, 130)
STATUSES = (rm.ST_RUN, rm.ST_SOLUTION, rm.ST_NIL, rm.ST_CAPACITY)
SMALL = (2, 3, 5, 7, 11, 13)
ALIEN = (1000003, 998244353)  # primes that no limb and no pivot of a case holds: a denominator with one overflows
HDR, LOGWORDS, NOUT = 16, 2 * rm.DETLOG * 2, 12  # words per job: header in, log area in, out (pip_probe.hip RP_*)
M64 = (1 << 64) - 1


def smooth(rng, bitlen):
    """a product of small primes of exactly `bitlen` bits (so that denominators find factors to take)"""
    x = 1
    while x.bit_length() < bitlen - 4:
        x *= rng.choice(SMALL)
    while x.bit_length() < bitlen:
        x *= 2
    assert x.bit_length() == bitlen
    return x


def held(limbs, ldet):
    """the small primes the limbs in use hold"""
    return [p for p in SMALL if any(x % p == 0 for x in limbs[:ldet])]


def candidate(rng, limbs, ldet, W):
    """a pair of one of the kinds the replay's pre-reduction tells apart"""
    kind = rng.randrange(8 if W == 128 else 6)
    a = rng.choice(held(limbs, ldet) or [1])           # a factor some limb can give
    b = rng.choice((1, 1, 2, 3, 5, 7, 11, 13, rng.getrandbits(rng.choice((2, 9, 20))) | 1))
    g = rng.choice((2, 3, 5, 7, 9, 35, 1 << 20))
    if kind == 0:
        return b, 1                                    # dp == 1: no gcd at all
    if kind == 1:
        while math.gcd(a, b) != 1:
            b += 1
        return b, a                                    # gcd 1, dp != 1
    if kind == 2:
        return g * b, g                                # gcd == dp
    if kind == 3:
        return g, g * a                                # gcd == pp
    if kind == 4:
        while math.gcd(a, b) != 1:
            b += 1
        return g * b, g * a                            # a gcd that is neither
    if kind == 5:
        return 1, 1
    if kind == 6:
        return b << 64, 1                              # 128 bits: zero low word
    return g << 64, (g << 64) * rng.choice((1, 2, 4))  # ... in both (the limbs must hold the powers of two that stay)


def walk(rng, limbs, ldet, W, n):
    """n pairs none of which overflows from the state (limbs, ldet); -> (log, limbs, ldet) behind them"""
    log = []
    limbs = tuple(limbs)
    while len(log) < n:
        for _ in range(40):
            pp, dp = candidate(rng, limbs, ldet, W)
            d = math.gcd(pp, dp)
            *nl, nd, ok = rm.det_model(limbs, ldet, pp // d, dp // d, W)
            if ok and pp.bit_length() < W and dp.bit_length() < W:
                break
        else:
            pp, dp, nl, nd = 1, 1, list(limbs), ldet
        log.append((pp, dp))
        limbs, ldet = tuple(nl), nd
    return log, limbs, ldet


def start_state(rng, W, ldet, edge):
    """ldet limbs in use, the last of them of `edge` bits (W - 2 and W - 1 are det_step's first-fit edges), the earlier
    ones full; junk behind them, which is no part of the number and must come back as it went"""
    limbs = [smooth(rng, W - 1) for _ in range(ldet - 1)] + [smooth(rng, edge)]
    junk = (rng.getrandbits(W - 3) | 1, -(rng.getrandbits(17) | 1), 12345, 7)
    return tuple(limbs + [junk[i] for i in range(ldet, 4)])


def overflow_pair(rng, cause, limbs, ldet, W):
    if cause == "factor":
        return rng.choice((1, 3, 10)), rng.choice(ALIEN)
    return (1 << (W - 1)) - 1, 1  # as wide as an entry gets: no limb has room for it


def overflowing_log(rng, limbs, ldet, W, n, at, cause):
    """n pairs from the state (limbs, ldet): `at` that do not overflow, one that does, then pairs that would change the
    limbs if they were walked and, two places on, one that would overflow again"""
    log, l2, d2 = walk(rng, limbs, ldet, W, at)
    log.append(overflow_pair(rng, cause, l2, d2, W))
    k = 0
    while len(log) < n:
        dp = rng.choice(held(l2, d2) or [1])
        log.append((1, rng.choice(ALIEN)) if k == 1 else (rng.choice([p for p in (2, 3, 5, 7) if p != dp]), dp))
        k += 1
    return log


def aux_of(i, status):
    """the header's aux of the i-th case of a loop: every other ST_NIL job ended in a pivot without a column (counted, not
    logged); under the other statuses the word means nothing, whatever it holds"""
    if status == rm.ST_NIL:
        return rm.AUX_NOCOLUMN if (i // 4) % 2 else 0
    return rm.AUX_NOCOLUMN if i % 5 == 0 else (0, 3, 70)[i % 3]


def make_case(rng, W, n, ldet=1, edge=None, status=rm.ST_RUN, extra=0, at=None, cause=None, aux=0):
    """a job with a log of n pairs; at: index of the first overflowing pair (None: none)"""
    limbs = start_state(rng, W, ldet, edge if edge else rng.choice((W - 2, W - 1, 5, W // 2)))
    if at is None:
        log, _, _ = walk(rng, limbs, ldet, W, n)
    else:
        log = overflowing_log(rng, limbs, ldet, W, n, at, cause)
    tail = [(11, 1), (1, ALIEN[0]), (5, 3)][:rm.DETLOG - n]
    unlogged = (status, aux) == (rm.ST_NIL, rm.AUX_NOCOLUMN)
    return dict(bits=W, limbs=limbs, ldet=ldet, npiv=n + extra + unlogged, status=status, aux=aux, log=log, tail=tail)


@functools.lru_cache(maxsize=None)
def pool(W):
    """every single-job case of width W (built once: the cases are shared and never changed)"""
    rng = random.Random(20260 + W)
    cs = []
    for i, n in enumerate(LENGTHS):  # lengths, without an overflow; the four statuses and three pivot counts in turn
        cs.append(make_case(rng, W, n, ldet=1 + i % 3, status=STATUSES[i % 4], extra=(0, 1, 700)[i % 3],
                            aux=aux_of(i, STATUSES[i % 4])))
    # the first-fit edges (log2 + log2 < B, and log2(1) is 1): a last limb of W - 2 bits takes a pivot of one bit and none
    # of two, one of W - 1 bits takes none at all -- with three limbs in use that is the fourth limb's overflow
    for ldet in (1, 2, 3):
        for edge in (W - 2, W - 1):
            c = make_case(rng, W, 9, ldet=ldet, edge=edge, status=STATUSES[(ldet + edge) % 4], extra=ldet)
            c["log"][:2] = [(1, 1), (2, 1)]
            cs.append(c)
    i = 0
    for at in OVERFLOW_AT:           # the first overflow at every place, by both causes, under every status
        for cause in ("factor", "limb"):
            for n in ((at + 1, at + 6) if at != "last" else (130, 512)):
                k = n - 1 if at == "last" else at
                if at != "last" and n == at + 1 and at not in (0, 64, 128):
                    continue  # (the overflow in the last place has its own rows)
                cs.append(make_case(rng, W, n, ldet=3 if cause == "limb" else 1 + i % 3, status=STATUSES[i % 4],
                                    extra=(0, 1, 700)[i % 3], at=k, cause=cause, aux=aux_of(i, STATUSES[i % 4])))
                i += 1
    return cs


def launches(W):
    """the launches of width W: every pool case in batches of JOBS jobs, among them jobs of the other width; then two
    batches under a list that names a subset in no order"""
    cs, other = pool(W), pool(192 - W)
    out, k = [], 0
    for nj in JOBS:
        jobs = []
        for j in range(nj):
            if j % 9 == 4 and nj > 1:
                jobs.append(other[(k + j) % len(other)])
            else:
                jobs.append(cs[k % len(cs)])
                k += 1
        out.append(dict(bits=W, jobs=jobs, list=None))
    assert k >= len(cs)
    rng = random.Random(77 + W)
    for nj in (65, 130):
        jobs = [other[j % len(other)] if j % 9 == 4 else cs[(3 * j + nj) % len(cs)] for j in range(nj)]
        lst = rng.sample(range(nj), nj // 2)
        assert lst != sorted(lst)
        out.append(dict(bits=W, jobs=jobs, list=lst))
    return out


def carry_pairs(W):
    """the same header under log A, which does not overflow, then under log B from where A left it; B overflows in every
    other one, by either cause.  -> list of (case with log A, log B, tail behind B)"""
    rng = random.Random(991 + W)
    out = []
    for i, (na, nb) in enumerate(((5, 9), (64, 64), (96, 160), (352, 160), (512, 512), (63, 1), (1, 65), (129, 8))):
        limb = i in (3, 7)
        a = make_case(rng, W, na, ldet=3 if limb else 1 + i % 3, status=STATUSES[i % 4], extra=i, aux=aux_of(i + 4, STATUSES[i % 4]))
        limbs, ldet, _, _, _ = rm.replay(a["limbs"], a["ldet"], a["npiv"], a["status"], a["log"], W)
        if i % 2:
            b = overflowing_log(rng, limbs, ldet, W, nb, nb // 2, "limb" if limb else "factor")
        else:
            b, _, _ = walk(rng, limbs, ldet, W, nb)
        out.append((a, b, [(13, 1), (1, ALIEN[1])][:rm.DETLOG - nb]))
    return out


# ------------------------------------------------------------------------------------------------ words
def _put(words, at, x, ew):
    for i in range(ew):
        words[at + i] = (x >> (64 * i)) & M64


def job_words(c):
    """the HDR + LOGWORDS words of a job, as unsigned 64-bit ints"""
    ew = c["bits"] // 64
    w = [0] * (HDR + LOGWORDS)
    for i, x in enumerate(c["limbs"]):
        _put(w, ew * i, x, ew)
    w[8], w[9], w[10], w[11], w[12], w[13] = c["ldet"], c["npiv"], c["status"], len(c["log"]), c["bits"], c["aux"] & M64
    for k, (pp, dp) in enumerate(list(c["log"]) + list(c["tail"])):
        _put(w, HDR + 2 * ew * k, pp, ew)
        _put(w, HDR + 2 * ew * k + ew, dp, ew)
    return w


def out_words(c, limbs, ldet, npiv, status, nlog):
    ew = c["bits"] // 64
    w = [0] * NOUT
    for i, x in enumerate(limbs):
        _put(w, ew * i, x, ew)
    w[8], w[9], w[10], w[11] = ldet, npiv & M64, status, nlog
    return w


def untouched(c):
    return out_words(c, c["limbs"], c["ldet"], c["npiv"], c["status"], len(c["log"]))


def expected(launch):
    """per job the NOUT words the launch must leave, by the model"""
    W, lst = launch["bits"], launch["list"]
    out = []
    for j, c in enumerate(launch["jobs"]):
        if c["bits"] != W or (lst is not None and j not in lst) or not c["log"]:
            out.append(untouched(c))
        else:
            out.append(out_words(c, *rm.replay(c["limbs"], c["ldet"], c["npiv"], c["status"], c["log"], W, c["aux"])))
    return out

"""The launch sequence of pipamd_batch_solve as piplib_amd/csrc/pip_plan.h decides it, on the CPU: tests/batch_plan_main.cpp
includes that header alone, is built with the host compiler under the address and undefined-behaviour sanitizers and run as
a child process.  The expected plans are literals, each worked out by hand from the launch calls BatchRun (pip_host.cpp)
made while it still decided the sequence itself, launch by launch (one call of its launch() per list below), not computed
by a second copy of the logic and not taken from the header's output.

A launch is [kernel, waves, budget, smax, whole_batch, replay_behind, spare_replay, full]; kernel 0 = the general kernel,
1 = lean, 2 = lean BIG, 3 = lean64; whole_batch 0 = the grid is the bound of the input list.  The last list is [logs
pending behind the bulk launches, spare_went, the one replay goes out a wave per job, tail_waves, stop (single_launch), the
replay goes out before the stop].  Unless the plan stops, the launch before the last list is the first tail launch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_INT, T_DUAL, T_DEEPEST, T_NOSKIP = 1, 2, 512, 2048    # include/piplib_amd.h PIPAMD_T_*
GEN, LEAN, BIG, LEAN64 = range(4)                       # pip_plan.h PipKernelFamily
FIELDS = ["batch", "nvar", "nparm", "bigparm", "ni", "S", "W", "ebits", "tflags",
          "round_pivots", "round_rows", "bulk_min", "iter_limit", "waves_per_job", "tail_waves", "lone_batches",
          "no_spare_replay", "lean2_one_wave", "no_lean", "no_lean2", "lean64", "lean_big", "single_launch", "lean64_fits"]
# the headline shape with a fresh engine's switches (iter_limit: PIPAMD_DETLOG, pipamd_engine_create)
HEAD = dict(batch=10000, nvar=127, nparm=0, bigparm=-1, ni=64, S=224, W=128, ebits=64, tflags=T_INT, iter_limit=512)
# 128-bit rows of 256 columns, the shape pip_lean64_kernel can take
WIDE = dict(HEAD, batch=1000, nvar=255, ni=128, S=300, W=256, ebits=128)
# one parameter, the big one, in rows of 128 columns
BIGP = dict(HEAD, nvar=125, nparm=1, bigparm=126)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "batch_plan_main.cpp"), "-o", exe], check=True, timeout=300)

    def run(cases):
        """cases: (PipPlanIn fields as a dict, expected plan) -> checks every plan"""
        lines = []
        for c, _ in cases:
            assert set(c) <= set(FIELDS), set(c) - set(FIELDS)
            lines.append(" ".join(str(int(c.get(f, 0))) for f in FIELDS))
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [[[int(x) for x in part.split()] for part in ln.split(";")] for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        for (c, want), got in zip(cases, out):
            assert got == want, ({k: v for k, v in c.items() if HEAD.get(k) != v}, got, want)
    return run


TAIL = [GEN, 4, 512, 224, 0, 0, 0, 1]        # the headline's tail launch: the catch-all replay follows it
LEAN1 = [LEAN, 1, 128, 112, 1, 0, 0, 1]      # ... its first lean launch: budget 128, 64 + 48 rows
LEAN2 = [LEAN, 4, 160, 160, 1, 0, 1, 1]      # ... its second: four waves, 64 + 96 rows, spare blocks replay
HEADLINE = [LEAN1, LEAN2, TAIL, [1, 1, 1, 4, 0, 0]]


def test_headline_and_switches(plans):
    plans([
        # both lean launches go out with PIPAMD_ROUND_PIVOTS; 128 + 160 <= 512: nobody replays behind itself
        (HEAD, HEADLINE),
        # round_pivots set: the k loop starts at K1, smax = ni + min(48, budget)
        (dict(HEAD, round_pivots=8), [[LEAN, 1, 8, 72, 1, 0, 0, 1], LEAN2, TAIL, [1, 1, 1, 4, 0, 0]]),
        (dict(HEAD, round_pivots=32), [[LEAN, 1, 32, 96, 1, 0, 0, 1], LEAN2, TAIL, [1, 1, 1, 4, 0, 0]]),
        # 400 + 160 > 512: defer is false, the first launch replays behind itself and no spare blocks replay; the second
        # lean launch still leaves its logs to the replay behind the tail, a lane per job
        (dict(HEAD, round_pivots=400), [[LEAN, 1, 400, 112, 1, 1, 0, 1], [LEAN, 4, 160, 160, 1, 0, 0, 1], TAIL, [1, 0, 0, 4, 0, 0]]),
        # round_rows: the first launch's image
        (dict(HEAD, round_rows=16), [[LEAN, 1, 128, 80, 1, 0, 0, 1], LEAN2, TAIL, [1, 1, 1, 4, 0, 0]]),
        # lone batches: no lean2, so the budget is 96; no second launch; the replay a wave per job
        (dict(HEAD, lone_batches=1), [[LEAN, 1, 96, 112, 1, 0, 0, 1], TAIL, [1, 0, 1, 4, 0, 0]]),
        # no_lean2: budget 96, the general kernel second with the same budget and image
        (dict(HEAD, no_lean2=1), [[LEAN, 1, 96, 112, 1, 0, 0, 1], [GEN, 1, 96, 112, 1, 0, 0, 1], TAIL, [1, 0, 0, 4, 0, 0]]),
        # no spare replay: the catch-all then goes out a lane per job
        (dict(HEAD, no_spare_replay=1), [LEAN1, [LEAN, 4, 160, 160, 1, 0, 0, 1], TAIL, [1, 0, 0, 4, 0, 0]]),
        (dict(HEAD, lean2_one_wave=1), [LEAN1, [LEAN, 1, 160, 160, 1, 0, 1, 1], TAIL, [1, 1, 1, 4, 0, 0]]),
        # no lean kernel: one general bulk launch (the `else` of lean2) with 96
        (dict(HEAD, no_lean=1), [[GEN, 1, 96, 112, 1, 0, 0, 1], TAIL, [1, 0, 0, 4, 0, 0]]),
        # iter_limit caps both budgets, the first image (64 + 40) and the tail
        (dict(HEAD, iter_limit=40), [[LEAN, 1, 40, 104, 1, 0, 0, 1], [LEAN, 4, 40, 160, 1, 0, 1, 1], [GEN, 4, 40, 224, 0, 0, 0, 1],
                                     [1, 1, 1, 4, 0, 0]]),
        # waves_per_job 4 / 8: no bulk launch; the tail replays behind itself
        (dict(HEAD, waves_per_job=4), [[GEN, 4, 512, 224, 0, 1, 0, 1], [0, 0, 0, 4, 0, 0]]),
        (dict(HEAD, waves_per_job=8), [[GEN, 8, 512, 224, 0, 1, 0, 1], [0, 0, 0, 8, 0, 0]]),
        (dict(HEAD, tail_waves=8), [LEAN1, LEAN2, [GEN, 8, 512, 224, 0, 0, 0, 1], [1, 1, 1, 8, 0, 0]]),
    ])


def test_class_table_edges(plans):
    def ni(n, *steps, last):
        return dict(HEAD, ni=n, S=n + 160), list(steps) + [[GEN, 4, 512, n + 160, 0, 0, 0, 1], last]
    both, one = [1, 1, 1, 4, 0, 0], [1, 0, 0, 4, 0, 0]
    plans([
        # ni + 48 = 64 | 65: lean class 64 | 96; the second launch (ni + 96 = 112 | 113) in class 112, one wave | 128, four
        ni(16, [LEAN, 1, 128, 64, 1, 0, 0, 1], [LEAN, 1, 160, 112, 1, 0, 1, 1], last=both),
        ni(17, [LEAN, 1, 128, 65, 1, 0, 0, 1], [LEAN, 4, 160, 113, 1, 0, 1, 1], last=both),
        # 96 | 97: class 96 | 112; second launch 144 | 145 in class 160
        ni(48, [LEAN, 1, 128, 96, 1, 0, 0, 1], [LEAN, 4, 160, 144, 1, 0, 1, 1], last=both),
        ni(49, [LEAN, 1, 128, 97, 1, 0, 0, 1], [LEAN, 4, 160, 145, 1, 0, 1, 1], last=both),
        # 112 | 113: the second launch at 160 has class 160, at 161 none: budget back to 96, the general kernel second
        ni(64, LEAN1, LEAN2, last=both),
        ni(65, [LEAN, 1, 96, 113, 1, 0, 0, 1], [GEN, 1, 96, 113, 1, 0, 0, 1], last=one),
        # 128 | 129: lean class 128 | 160, no second lean launch
        ni(80, [LEAN, 1, 96, 128, 1, 0, 0, 1], [GEN, 1, 96, 128, 1, 0, 0, 1], last=one),
        ni(81, [LEAN, 1, 96, 129, 1, 0, 0, 1], [GEN, 1, 96, 129, 1, 0, 0, 1], last=one),
        # 160 | 161: the last lean class | none: one general bulk launch
        ni(112, [LEAN, 1, 96, 160, 1, 0, 0, 1], [GEN, 1, 96, 160, 1, 0, 0, 1], last=one),
        ni(113, [GEN, 1, 96, 161, 1, 0, 0, 1], last=one),
        # S below ni + 96: the second launch's image is S (150: class 160, four waves)
        (dict(HEAD, S=150), [LEAN1, [LEAN, 4, 160, 150, 1, 0, 1, 1], [GEN, 4, 512, 150, 0, 0, 0, 1], both]),
        # ... and below ni + 48: both images are S (100: class 112, which has no four-wave kernel)
        (dict(HEAD, S=100), [[LEAN, 1, 128, 100, 1, 0, 0, 1], [LEAN, 1, 160, 100, 1, 0, 1, 1], [GEN, 4, 512, 100, 0, 0, 0, 1], both]),
        # W 126: lean, not FULL (nvar + 1 != 128)
        (dict(HEAD, nvar=125, W=126), [[LEAN, 1, 128, 112, 1, 0, 0, 0], [LEAN, 4, 160, 160, 1, 0, 1, 0], [GEN, 4, 512, 224, 0, 0, 0, 0], both]),
        # an odd W, and W 130: no lean launch
        (dict(HEAD, nvar=125, W=127), [[GEN, 1, 96, 112, 1, 0, 0, 0], [GEN, 4, 512, 224, 0, 0, 0, 0], one]),
        (dict(HEAD, W=130), [[GEN, 1, 96, 112, 1, 0, 0, 0], [GEN, 4, 512, 224, 0, 0, 0, 0], one]),
    ])


def test_bulk_min_edges(plans):
    lone_tail = [[GEN, 4, 512, 224, 0, 1, 0, 1], [0, 0, 0, 4, 0, 0]]   # no bulk launch: the tail replays behind itself
    plans([
        (dict(HEAD, batch=2047), lone_tail),                 # default bulk_min 2048
        (dict(HEAD, batch=2048), HEADLINE),
        (dict(HEAD, batch=2047, bulk_min=64), HEADLINE),
        (dict(HEAD, batch=63, bulk_min=64), lone_tail),
        (dict(HEAD, batch=64, bulk_min=64), HEADLINE),
    ])


def test_other_families(plans):
    gen_only = [[GEN, 1, 96, 112, 1, 0, 0, 1], TAIL, [1, 0, 0, 4, 0, 0]]
    wide_tail = [GEN, 4, 512, 300, 0, 1, 0, 0]
    plans([
        # one big parameter: without lean_big neither plain nor bigone; with it the BIG flavour twice, one wave each
        (BIGP, [[GEN, 1, 96, 112, 1, 0, 0, 0], [GEN, 4, 512, 224, 0, 0, 0, 0], [1, 0, 0, 4, 0, 0]]),
        (dict(BIGP, lean_big=1), [[BIG, 1, 128, 112, 1, 0, 0, 0], [BIG, 1, 160, 160, 1, 0, 1, 0], [GEN, 4, 512, 224, 0, 0, 0, 0],
                                  [1, 1, 1, 4, 0, 0]]),
        # ... a big parameter in column nvar + 1 of rows too wide for the lean kernel (nvar + 2 = 129 columns)
        (dict(HEAD, nparm=1, bigparm=128, W=130, lean_big=1), [[GEN, 1, 96, 112, 1, 0, 0, 0], [GEN, 4, 512, 224, 0, 0, 0, 0], [1, 0, 0, 4, 0, 0]]),
        # 128-bit, 256 columns, 1,000 tableaux: below bulk_min, the tail alone
        (WIDE, [wide_tail, [0, 0, 0, 4, 0, 0]]),
        # ... lean64 on and the image fits: pip_lean64_kernel over the batch with iter_limit, replaying behind itself
        (dict(WIDE, lean64=1, lean64_fits=1), [[LEAN64, 1, 512, 300, 1, 1, 0, 0], wide_tail, [0, 0, 0, 4, 0, 0]]),
        (dict(WIDE, lean64=1, lean64_fits=0), [wide_tail, [0, 0, 0, 4, 0, 0]]),
        (dict(WIDE, lean64=0, lean64_fits=1), [wide_tail, [0, 0, 0, 4, 0, 0]]),
        # ... its image holds at most 448 rows
        (dict(WIDE, S=500, lean64=1, lean64_fits=1), [[LEAN64, 1, 512, 448, 1, 1, 0, 0], [GEN, 4, 512, 500, 0, 1, 0, 0], [0, 0, 0, 4, 0, 0]]),
        # ... below its 128 tableaux: the tail alone, sixteen waves for a list of at most 256 tableaux
        (dict(WIDE, batch=127, lean64=1, lean64_fits=1), [[GEN, 16, 512, 300, 0, 1, 0, 0], [0, 0, 0, 4, 0, 0]]),
        # ... a 128-bit batch large enough for the bulk launch, lean64 refused or off: one general launch with 96
        (dict(WIDE, batch=4096, lean64=1, lean64_fits=0), [[GEN, 1, 96, 176, 1, 0, 0, 0], [GEN, 4, 512, 300, 0, 0, 0, 0], [1, 0, 0, 4, 0, 0]]),
        (dict(WIDE, batch=4096), [[GEN, 1, 96, 176, 1, 0, 0, 0], [GEN, 4, 512, 300, 0, 0, 0, 0], [1, 0, 0, 4, 0, 0]]),
        # T_DUAL, T_NOSKIP, T_DEEPEST: no lean launch
        (dict(HEAD, tflags=T_INT | T_DUAL), gen_only),
        (dict(HEAD, tflags=T_INT | T_NOSKIP), gen_only),
        (dict(HEAD, tflags=T_INT | T_DEEPEST), gen_only),
        (dict(WIDE, tflags=T_INT | T_DUAL, lean64=1, lean64_fits=1), [wide_tail, [0, 0, 0, 4, 0, 0]]),
        # rational: KA is 0, the first image has no spare row
        (dict(HEAD, tflags=0), [[LEAN, 1, 128, 64, 1, 0, 0, 1], LEAN2, TAIL, [1, 1, 1, 4, 0, 0]]),
    ])


def test_single_launch(plans):
    l64 = dict(WIDE, lean64=1, lean64_fits=1)
    plans([
        # 1: behind both bulk launches, the catch-all replay (a wave per job: spare blocks went) before the stop
        (dict(HEAD, single_launch=1), [LEAN1, LEAN2, [1, 1, 1, 4, 1, 1]]),
        # 2: behind the first lean launch, still shaped with the budget of the two; the replay a lane per job
        (dict(HEAD, single_launch=2), [LEAN1, [1, 0, 0, 4, 1, 1]]),
        # 3: as 1 without the replay
        (dict(HEAD, single_launch=3), [LEAN1, LEAN2, [1, 1, 1, 4, 1, 0]]),
        # 2 where the first launch replayed behind itself: nothing is pending at the stop
        (dict(HEAD, single_launch=2, round_pivots=400), [[LEAN, 1, 400, 112, 1, 1, 0, 1], [0, 0, 0, 4, 1, 0]]),
        # 2 without a lean launch acts as 1
        (dict(HEAD, single_launch=2, no_lean=1), [[GEN, 1, 96, 112, 1, 0, 0, 1], [1, 0, 0, 4, 1, 1]]),
        (dict(HEAD, single_launch=1, lone_batches=1), [[LEAN, 1, 96, 112, 1, 0, 0, 1], [1, 0, 1, 4, 1, 1]]),
        # no bulk launch: the first tail launch goes out (the solve stops behind it)
        (dict(HEAD, single_launch=1, waves_per_job=4), [[GEN, 4, 512, 224, 0, 1, 0, 1], [0, 0, 0, 4, 0, 0]]),
        # the lean64 launch replays behind itself: every level stops behind it without a replay
        (dict(l64, single_launch=1), [[LEAN64, 1, 512, 300, 1, 1, 0, 0], [0, 0, 0, 4, 1, 0]]),
        (dict(l64, single_launch=2), [[LEAN64, 1, 512, 300, 1, 1, 0, 0], [0, 0, 0, 4, 1, 0]]),
        (dict(l64, single_launch=3), [[LEAN64, 1, 512, 300, 1, 1, 0, 0], [0, 0, 0, 4, 1, 0]]),
    ])

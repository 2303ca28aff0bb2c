// tests/batch_plan_main.cpp -- drives piplib_amd/csrc/pip_plan.h alone, on the CPU (tests/test_batch_plan.py builds it
// with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child process).
// One case per line of stdin: the ints of PipPlanIn in the order of its members (lean64_fits last, 0 or 1).  One line of
// results each, lists separated by ";": a list of eight per launch -- the bulk steps, then the first tail launch unless
// the plan stops before it -- kernel, waves, budget, smax, whole_batch, replay_behind, spare_replay, full; the last
// list is pending, spare_went, catchall_waves, tail_waves, stop, stop_replay.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../piplib_amd/csrc/pip_plan.h"

static void put(const PipStep &s) {
  printf("%d %d %d %d %d %d %d %d ; ", s.kernel, s.waves, s.budget, s.smax, (int)s.whole_batch, (int)s.replay_behind,
         (int)s.spare_replay, (int)s.full);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    int v[24], n = 0;
    while (n < 24 && (is >> v[n])) n++;
    if (n != 24) {
      fprintf(stderr, "expected 24 integers, got %d: %s\n", n, line.c_str());
      return 2;
    }
    const PipPlanIn in{v[0],  v[1],  v[2],  v[3],  v[4],  v[5],  v[6],  v[7],  v[8],  v[9],  v[10], v[11],
                       v[12], v[13], v[14], v[15], v[16], v[17], v[18], v[19], v[20], v[21], v[22], v[23] != 0};
    const PipPlan p = pip_plan_batch(in);
    for (int i = 0; i < p.nsteps; i++) put(p.step[i]);
    if (!p.stop) put(pip_plan_tail(in, p.tail_waves, in.S, in.batch, p.pending));
    printf("%d %d %d %d %d %d\n", (int)p.pending, (int)p.spare_went, (int)p.catchall_waves, p.tail_waves, (int)p.stop,
           (int)p.stop_replay);
  }
  return 0;
}

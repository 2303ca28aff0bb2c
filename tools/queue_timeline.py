"""How the batches of a `bench.py` run share the hardware queues: a summary of a `rocprofv3 --kernel-trace` CSV.

    python tools/queue_timeline.py TRACE_kernel_trace.csv [--steps N]

Looks at kernel names, queue ids, stream ids (where the trace has them) and timestamps only.  --steps N: the region is
the last N batches of the trace (from the N-th last load kernel to the last results kernel: a plain bench.py run ends
with its timed region); without it, the whole trace.  Prints the distinct queue ids, the largest number of kernels
running at once, per queue the share of the region spent in each kernel name, and per batch the time from its load
kernel to its results kernel (a batch is the kernels of one stream between a load and the next results kernel; a trace
without stream ids pairs the k-th load of a queue with its k-th results kernel)."""
import argparse
import collections
import csv


def short(name):
    n = name[5:] if name.startswith("void ") else name
    for key in ("pip_lean_kernel<", "pip_advance_kernel<"):
        if n.startswith(key):  # keep the template arguments: they tell the launches apart
            return n[:n.index(">") + 1]
    n = n.split("(")[0].split("<")[0]
    return n if len(n) <= 48 else n[:45] + "..."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.csv)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r.get("Stream_Id"), short(r["Kernel_Name"])))
    rows.sort()
    loads = [r for r in rows if r[4].startswith("pip_batch_load")]
    results = [r for r in rows if r[4].startswith("pip_batch_results")]
    if not loads or not results:
        raise SystemExit("no pip_batch_load / pip_batch_results kernel in the trace")
    t0 = loads[-a.steps][0] if 0 < a.steps <= len(loads) else rows[0][0]
    t1 = max(r[1] for r in results)
    reg = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    span = t1 - t0
    print("region: %d kernels, %.3f ms, %d load kernels" % (len(reg), span / 1e6, sum(r[4].startswith("pip_batch_load") for r in reg)))
    queues = sorted({r[2] for r in reg}, key=lambda q: (len(q), q))
    print("queue ids: %d (%s)" % (len(queues), " ".join(queues)))
    ev = sorted([(r[0], 1) for r in reg] + [(r[1], -1) for r in reg])  # (an end sorts before a start at the same time)
    cur = peak = 0
    at = collections.Counter()  # ns spent with k kernels running
    last = t0
    for t, d in ev:
        at[cur] += t - last
        last = t
        cur += d
        peak = max(peak, cur)
    print("kernels running at once: at most %d; share of the region with k running: %s" %
          (peak, " ".join("%d:%.1f%%" % (k, 100.0 * at[k] / span) for k in sorted(at))))
    tot = collections.Counter()
    for q in queues:
        per = collections.Counter()
        for r in reg:
            if r[2] == q:
                per[r[4]] += r[1] - r[0]
                tot[r[4]] += r[1] - r[0]
        busy = sum(per.values())
        print("queue %s: busy %.1f%% of the region" % (q, 100.0 * busy / span))
        for k, v in per.most_common():
            if v * 1000 >= span:
                print("    %5.1f%%  %s" % (100.0 * v / span, k))
    nload = max(1, sum(r[4].startswith("pip_batch_load") for r in reg))
    print("kernel time per batch (sum over the region / load kernels):")
    for k, v in tot.most_common():
        if k.startswith("pip_"):
            print("    %7.3f ms  %s" % (v / 1e6 / nload, k))
    print("    %7.3f ms  all pip_ kernels: the queue time of a batch" % (sum(v for k, v in tot.items() if k.startswith("pip_")) / 1e6 / nload))
    # per batch: load -> results
    have_streams = all(r[3] not in (None, "") for r in reg)
    key = (lambda r: r[3]) if have_streams else (lambda r: r[2])
    lat = []
    open_loads = collections.defaultdict(collections.deque)
    for r in reg:
        if r[4].startswith("pip_batch_load"):
            open_loads[key(r)].append(r[0])
        elif r[4].startswith("pip_batch_results") and open_loads[key(r)]:
            # (a batch loaded in parts has several load kernels: its first one counts)
            first = open_loads[key(r)][0]
            open_loads[key(r)].clear()
            lat.append((r[1] - first) / 1e6)
    if not have_streams:  # FIFO pairing per queue: the k-th load with the k-th results kernel
        lat = []
        for q in queues:
            ls = [r[0] for r in reg if r[2] == q and r[4].startswith("pip_batch_load")]
            rs = [r[1] for r in reg if r[2] == q and r[4].startswith("pip_batch_results")]
            lat += [(e - s) / 1e6 for s, e in zip(ls, rs) if e > s]
    if lat:
        lat.sort()
        print("batches (%s): %d, load start -> results end: min %.2f ms, median %.2f ms, max %.2f ms, mean %.2f ms" %
              ("by stream id" if have_streams else "by queue, in order", len(lat), lat[0], lat[len(lat) // 2], lat[-1], sum(lat) / len(lat)))
        print("batches finished per ms of the region: %.3f (one per %.2f ms)" % (len(lat) / (span / 1e6), (span / 1e6) / len(lat)))


if __name__ == "__main__":
    main()

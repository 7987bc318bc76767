#!/usr/bin/env python3
"""What happens between two extension launches of the whole-read pass, from a rocprofv3 --kernel-trace run (CSV output).

usage: python3 scripts/pass_gap_timeline.py <..._kernel_trace.csv> [pass index, default: the last complete pass]

A pass's round loop runs on a host thread of its own (one per batch), so the dispatches of one Thread_Id between a k_long_init and
the k_long_finish behind it are one pass. For that pass the script lists, round by round, the intervals between

    k_long_extend end -> k_long_merge start / end -> k_long_select start -> k_long_order and publish end -> next k_long_extend start

with the hardware queue of every dispatch, and names the foreign kernels (other threads' dispatches) that occupied the same queue during
each interval, with the milliseconds of overlap. A summary over every complete pass of the trace follows."""
import csv
import sys
from collections import defaultdict


def short(name):
    n = name.replace("gcdev::", "").replace("void ", "")
    cut = n.find("(")
    return (n[:cut] if cut > 0 else n)[:44]


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"name": short(r["Kernel_Name"]), "queue": r.get("Queue_Id", "?"), "thread": r.get("Thread_Id", "?"), "stream": r.get("Stream_Id", "?"),
                         "start": int(r["Start_Timestamp"]), "end": int(r["End_Timestamp"]), "grid": r.get("Grid_Size_X", r.get("Grid_Size", "?"))})
    rows.sort(key=lambda r: r["start"])
    return rows


def passes_of(rows):
    by_thread = defaultdict(list)
    for r in rows:
        by_thread[r["thread"]].append(r)
    out = []
    for thread, rs in by_thread.items():
        cur = None
        for r in rs:
            if r["name"].startswith("k_long_init"):
                cur = [r]
            elif cur is not None:
                cur.append(r)
                if r["name"].startswith("k_long_finish"):
                    if sum(1 for x in cur if x["name"].startswith("k_long_extend<1")) > 0:
                        out.append((thread, cur))
                    cur = None
    out.sort(key=lambda p: p[1][0]["start"])
    return out


def foreign(rows, thread, queue, t0, t1):
    """foreign dispatches on `queue` that overlap [t0, t1): name -> ms of overlap"""
    got = defaultdict(float)
    if t1 <= t0:
        return got
    for r in rows:
        if r["start"] >= t1:
            break
        if r["thread"] == thread or r["queue"] != queue or r["end"] <= t0:
            continue
        got[r["name"]] += (min(r["end"], t1) - max(r["start"], t0)) / 1e6
    return got


def rounds_of(seq):
    """splits a pass into rounds: everything up to and including a k_long_merge"""
    rounds, cur = [], []
    for r in seq[1:]:
        cur.append(r)
        if r["name"].startswith("k_long_merge"):
            rounds.append(cur)
            cur = []
    return rounds, cur


def first(rs, prefix, last=False):
    hit = [r for r in rs if r["name"].startswith(prefix)]
    return (hit[-1] if last else hit[0]) if hit else None


def gaps_of(seq):
    """per round after the first: (extension end of the round before -> this round's first extension start, the small kernels' own time in between)"""
    rounds, tail = rounds_of(seq)
    out = []
    for k in range(1, len(rounds)):
        prev_ext = first(rounds[k - 1], "k_long_extend", last=True)
        ext = first(rounds[k], "k_long_extend<1")
        if not prev_ext or not ext:
            continue
        between = [r for r in rounds[k - 1] if r["start"] >= prev_ext["end"]] + [r for r in rounds[k] if r["start"] < ext["start"]]
        out.append(((ext["start"] - prev_ext["end"]) / 1e6, sum(r["end"] - r["start"] for r in between) / 1e6))
    return out


def main():
    rows = load(sys.argv[1])
    ps = passes_of(rows)
    if not ps:
        print("no complete whole-read pass in the trace")
        return
    which = int(sys.argv[2]) if len(sys.argv) > 2 else len(ps) - 1
    thread, seq = ps[which]
    t0 = seq[0]["start"]
    print(f"# {len(rows)} dispatches, {len(ps)} complete passes; pass {which} (host thread {thread}), times in ms from its k_long_init")
    queues = defaultdict(int)
    for _, s in ps:
        for r in s:
            if r["name"].startswith("k_long_extend<1"):
                queues[r["queue"]] += 1
    print(f"# k_long_extend<1> launches per hardware queue, all passes: {dict(sorted(queues.items()))}")
    pass_streams = set(r["stream"] for _, s in ps for r in s if r["name"].startswith("k_long_extend<1"))
    shared = defaultdict(int)
    for r in rows:
        if r["stream"] not in pass_streams and r["queue"] in queues:
            shared[r["queue"]] += 1
    print(f"# the round loop's stream id(s): {sorted(pass_streams)}; dispatches of OTHER streams on those queues, whole trace: {dict(sorted(shared.items())) or 'none'}")
    print("# dispatch                                     queue stream   start      end      dur | wait since the dispatch before it on this pass; foreign kernels on the same queue during that wait (ms of overlap)")
    rounds, tail = rounds_of(seq)
    last_end = seq[0]["end"]
    print(f"  {seq[0]['name']:44s} {seq[0]['queue']:>5s} {seq[0]['stream']:>6s} {0.0:8.3f} {(seq[0]['end'] - t0) / 1e6:8.3f} {(seq[0]['end'] - seq[0]['start']) / 1e6:8.3f} |")
    for k, rs in enumerate(rounds + ([tail] if tail else [])):
        print(f"## round {k + 1}" + ("" if k < len(rounds) else " (no work: the pass ends)"))
        for r in rs:
            wait = (r["start"] - last_end) / 1e6
            f = foreign(rows, thread, r["queue"], last_end, r["start"])
            note = ", ".join(f"{n} {ms:.2f}" for n, ms in sorted(f.items(), key=lambda x: -x[1])[:4] if ms >= 0.01)
            print(f"  {r['name']:44s} {r['queue']:>5s} {r['stream']:>6s} {(r['start'] - t0) / 1e6:8.3f} {(r['end'] - t0) / 1e6:8.3f} {(r['end'] - r['start']) / 1e6:8.3f} | {wait:7.3f}  {note}")
            last_end = max(last_end, r["end"])
    print("## per round of this pass: extension end -> next extension start, and the small kernels' own time inside it")
    for k, (gap, own) in enumerate(gaps_of(seq)):
        print(f"  round {k + 1} -> {k + 2}: gap {gap:7.3f} ms, own kernels {own:6.3f} ms, neither {gap - own:7.3f} ms")
    print("## every complete pass: rounds, sum of the gaps, of which own kernels; first extension start -> last merge end; sum of k_long_extend")
    tot_gap = tot_own = 0.0
    for i, (th, s) in enumerate(ps):
        g = gaps_of(s)
        ext = [r for r in s if r["name"].startswith("k_long_extend")]
        merges = [r for r in s if r["name"].startswith("k_long_merge")]
        span = (merges[-1]["end"] - ext[0]["start"]) / 1e6 if merges else 0.0
        print(f"  pass {i}: rounds {len(g) + 1}, gaps {sum(x[0] for x in g):7.3f} ms, own {sum(x[1] for x in g):6.3f} ms, span {span:8.3f} ms, extension kernels {sum(r['end'] - r['start'] for r in ext) / 1e6:8.3f} ms, queues {sorted(set(r['queue'] for r in ext))}")
        tot_gap += sum(x[0] for x in g)
        tot_own += sum(x[1] for x in g)
    print(f"# mean per pass: gaps {tot_gap / len(ps):.3f} ms, own kernels {tot_own / len(ps):.3f} ms, neither {(tot_gap - tot_own) / len(ps):.3f} ms")


if __name__ == "__main__":
    main()

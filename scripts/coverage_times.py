#!/usr/bin/env python3
"""Times of the coverage accumulators (gc_coverage_*; --coverage-out / --base-coverage-out) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp,
seed=7), 10 000 reads of 10 kb, seed 11). Not bench.py and gated by nothing: one JSON line. Reported: the device time of k_cov_add per batch by HIP events (the library's
GC_DEBUG_TIMES line; medians of --repeat batches after one warm-up) with and without the per-base depth and with the link table (--link-coverage-out /
--coverage-gfa-out / --supported-subgraph-out), beside the whole call's wall time with and without a handle; the finish step's wall time for each table and for the two
tagged graphs and the bytes that come down; and with --command the command's reads/s with -a x.gaf alone and with both tables beside it.
    python3 scripts/coverage_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K] [--command]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def note(text):
    print("[coverage_times] " + text, file=sys.stderr, flush=True)


def with_stderr_captured(fn):
    """fn() with file descriptor 2 in a temporary file: what the library printed while it ran."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            result = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return result, tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3, help="timed batches after one warm-up; the median is reported")
    ap.add_argument("--command", action="store_true", help="also python -m graphchainer_amd on the same files: -a alone, and with --coverage-out and --base-coverage-out")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    os.environ["GC_DEBUG_TIMES"] = "1"

    import numpy as np

    import graphchainer_amd as gca
    from graphchainer_amd.synth import SynthGraph

    gca.set_device(0)
    med = lambda v: round(float(np.median(v)), 3)   # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        gfa = os.path.join(tmp, "graph.gfa")
        sg = SynthGraph(args.backbone, seed=7)
        sg.write_gfa(gfa)
        reads = sg.sample_reads(args.reads, args.read_len, seed=11)
        ids = [b"read_%06d" % i for i in range(len(reads))]
        note("graph and reads written")
        out = {"graph_bp": int(args.backbone), "reads": len(reads), "read_len": args.read_len, "library": os.path.basename(gca.api.LIB_PATH)}
        graph = gca.AlignmentGraph(gfa)
        seeder = gca.MinimizerSeeder(graph)
        batch = gca.ReadBatch(reads)
        note("graph built")
        aligner = gca.Aligner(graph, seeder, long_pass=True, device_output=1)
        line = re.compile(r"coverage: k_cov_add over ([0-9]+) alignments in the cell pool and ([0-9]+) chained winners \(([0-9]+) cells up\), ([0-9.]+) ms on the device, ([0-9.]+) ms in all")
        out["device_ms"], out["align_batch_wall_ms_with_debug_times"], out["finish"] = {}, {}, {}
        for key, per_base, links in (("without_handle", None, False), ("bases_only", False, False), ("with_per_base_depth", True, False), ("bases_and_links", False, True), ("bases_only_again", False, False)):
            cov = gca.Coverage(graph, per_base=per_base, links=links) if per_base is not None else None
            aligner.set_coverage(cov)
            kernel, in_all, walls = [], [], []
            for i in range(args.repeat + 1):
                t0 = time.time()
                res, text = with_stderr_captured(lambda: aligner.align_batch(batch))
                wall = (time.time() - t0) * 1e3
                found = line.search(text)
                assert (found is not None) == (cov is not None), "GC_DEBUG_TIMES line of the coverage kernel:\n" + text[-2000:]
                if i:
                    walls.append(wall)
                    if found:
                        kernel.append(float(found.group(4)))
                        in_all.append(float(found.group(5)))
                if found and i == args.repeat:
                    out["alignments"], out["chained_winners"], out["winner_cells_uploaded"] = int(found.group(1)), int(found.group(2)), int(found.group(3))
                del res
            out["align_batch_wall_ms_with_debug_times"][key] = med(walls)
            if cov is not None:
                out["device_ms"][key] = {"k_cov_add": med(kernel), "counting_step_wall_with_upload_and_wait": med(in_all)}
                t0 = time.time()
                segments = cov.segment_table()
                seg_ms = (time.time() - t0) * 1e3
                finish = {"segment_table_ms": round(seg_ms, 3), "segment_table_bytes": len(segments), "segments": segments.count(b"\n") - 1}
                if per_base:
                    t0 = time.time()
                    runs = cov.base_table()
                    finish.update(base_table_ms=round((time.time() - t0) * 1e3, 3), base_table_bytes=len(runs), runs=runs.count(b"\n"),
                                  depth_bytes_on_the_device=4 * (int(graph.SizeInBP()) // 2))
                    del runs
                if links:
                    for name, spell in (("link_table", cov.link_table), ("coverage_gfa", lambda: b"".join(t for t, _ in cov.gfa_pieces())),
                                        ("supported_subgraph", lambda: b"".join(t for t, _ in cov.gfa_pieces(supported_only=True)))):
                        t0 = time.time()
                        text = spell()
                        finish.update({name + "_ms": round((time.time() - t0) * 1e3, 3), name + "_bytes": len(text), name + "_lines": text.count(b"\n")})
                        del text
                    finish["link_bytes_on_the_device"] = 16 * len(cov.link_counts()[0])
                out["finish"][key] = finish
                aligner.set_coverage(None)
                cov.close()
        note("batches timed")
        if args.command:
            os.environ.pop("GC_DEBUG_TIMES")
            fq = os.path.join(tmp, "reads.fq")
            with open(fq, "wb") as f:
                for i, r in zip(ids, reads):
                    f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
            code = ("import sys, json; from graphchainer_amd import cli; cfg = cli.resolve(sys.argv[1:]); c = cli.run(cfg); "
                    "print(json.dumps({'reads': c['reads'], 'seconds': c['seconds'], 'inflight': c['inflight'], 'batches': c['batches'], 'stage_seconds': c['stage_seconds']}))")
            both = ["--coverage-out", os.path.join(tmp, "c.tsv"), "--base-coverage-out", os.path.join(tmp, "b.bg.gz")]
            runs = {}
            for key, extra in (("warm_up", []), ("gaf", []), ("gaf_and_both_tables", both), ("gaf_again", []), ("gaf_and_both_tables_again", both)):
                run = subprocess.run([sys.executable, "-c", code, "-g", gfa, "-f", fq, "-a", os.path.join(tmp, "x.gaf")] + extra, capture_output=True, text=True, cwd=ROOT, timeout=1500)
                if run.returncode != 0:
                    raise RuntimeError(run.stderr[-2000:])
                c = json.loads(run.stdout.strip().splitlines()[-1])
                if key == "warm_up":        # the first run of the command on a box pays for cold files and libraries: not reported
                    continue
                runs[key] = {"reads_per_s": round(c["reads"] / c["seconds"], 1), "inflight": c["inflight"], "batches": c["batches"]}
            runs["table_bytes"] = {"c.tsv": os.path.getsize(both[1]), "b.bg.gz": os.path.getsize(both[3])}
            out["command"] = runs
        print(json.dumps(out))


if __name__ == "__main__":
    main()

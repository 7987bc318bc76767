#!/usr/bin/env python3
"""Times of the pileup (GC_COVERAGE_PILEUP; --pileup-out) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp, seed=7), 10 000 reads of 10 kb, seed 11).
Not bench.py and gated by nothing: one JSON line. Reported: the device time of k_cov_add per batch by HIP events (the library's GC_DEBUG_TIMES line; medians of --repeat
batches after one warm-up) with the per-base depth alone and with the pileup on the same batch, interleaved; the finish step's wall time (the table spelled on the
device, piece by piece, text down included) and its bytes; and with --command the command's reads/s with --base-coverage-out alone and with --pileup-out beside it,
interleaved, medians of --command-repeat runs each. --parent-library PATH: the same --base-coverage-out command also under that library (the parent commit's build of
libgraphchainer_amd.so), interleaved with the other two.
    python3 scripts/pileup_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K] [--command] [--command-repeat K] [--parent-library PATH]"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from coverage_times import with_stderr_captured   # noqa: E402


def note(text):
    print("[pileup_times] " + text, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3, help="timed batches per handle after one warm-up; the median is reported")
    ap.add_argument("--command", action="store_true", help="also python -m graphchainer_amd on the same files: --base-coverage-out alone, and with --pileup-out")
    ap.add_argument("--command-repeat", type=int, default=3)
    ap.add_argument("--parent-library", default="", help="the parent commit's libgraphchainer_amd.so: its --base-coverage-out run, interleaved")
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
        handles = {"per_base_depth": gca.Coverage(graph, per_base=True), "pileup": gca.Coverage(graph, pileup=True)}
        kernel, in_all, walls = {k: [] for k in handles}, {k: [] for k in handles}, {k: [] for k in handles}
        for i in range(args.repeat + 1):           # interleaved: depth, pileup, depth, pileup, ...
            for key, cov in handles.items():
                aligner.set_coverage(cov)
                t0 = time.time()
                res, text = with_stderr_captured(lambda: aligner.align_batch(batch))
                wall = (time.time() - t0) * 1e3
                found = line.search(text)
                assert found is not None, "GC_DEBUG_TIMES line of the coverage kernel:\n" + text[-2000:]
                if i:
                    walls[key].append(wall)
                    kernel[key].append(float(found.group(4)))
                    in_all[key].append(float(found.group(5)))
                out["alignments"], out["chained_winners"] = int(found.group(1)), int(found.group(2))
                del res
        aligner.set_coverage(None)
        out["k_cov_add_ms"] = {k: med(v) for k, v in kernel.items()}
        out["k_cov_add_ms_all"] = {k: [round(x, 3) for x in v] for k, v in kernel.items()}
        out["counting_step_wall_ms_with_upload_and_wait"] = {k: med(v) for k, v in in_all.items()}
        out["align_batch_wall_ms_with_debug_times"] = {k: med(v) for k, v in walls.items()}
        note("batches timed")
        cov = handles["pileup"]
        finish = {"bytes_on_the_device": 36 * (int(graph.SizeInBP()) // 2)}
        for key, (min_alt, fraction) in (("min_alt_1", (1, 0.0)), ("every_covered_base", (0, 0.0)), ("min_alt_2_fraction_0.2", (2, 0.2))):
            t0 = time.time()
            n_bytes = n_lines = 0
            for text, off in cov.pileup_pieces(min_alt, fraction):
                n_bytes += len(text)
                n_lines += len(off) - 1
            finish[key] = {"ms": round((time.time() - t0) * 1e3, 3), "bytes": n_bytes, "lines": n_lines}
        t0 = time.time()
        runs = handles["per_base_depth"].base_table()
        finish["base_table_for_scale"] = {"ms": round((time.time() - t0) * 1e3, 3), "bytes": len(runs)}
        del runs
        out["finish"] = finish
        for c in handles.values():
            c.close()
        aligner.close()
        note("tables spelled")
        if args.command:
            os.environ.pop("GC_DEBUG_TIMES")
            fq = os.path.join(tmp, "reads.fq")
            with open(fq, "wb") as f:
                for i, r in zip(ids, reads):
                    f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
            code = ("import sys, json; from graphchainer_amd import cli; cfg = cli.resolve(sys.argv[1:]); c = cli.run(cfg); "
                    "print(json.dumps({'reads': c['reads'], 'seconds': c['seconds'], 'inflight': c['inflight'], 'batches': c['batches']}))")
            depth = ["--base-coverage-out", os.path.join(tmp, "b.bg.gz")]
            kinds = [("base_coverage", depth, None), ("base_coverage_and_pileup", depth + ["--pileup-out", os.path.join(tmp, "p.tsv.gz")], None)]
            if args.parent_library:
                kinds.append(("parent_base_coverage", depth, os.path.abspath(args.parent_library)))
            rates = {k: [] for k, _, _ in kinds}
            for i in range(args.command_repeat + 1):          # the first round pays for cold files and libraries: not reported
                for key, extra, library in kinds:
                    env = dict(os.environ)
                    if library:
                        env["GC_LIBRARY"] = library
                    run = subprocess.run([sys.executable, "-c", code, "-g", gfa, "-f", fq, "-a", os.path.join(tmp, "x.gaf")] + extra, capture_output=True, text=True, cwd=ROOT, timeout=1500, env=env)
                    if run.returncode != 0:
                        raise RuntimeError(run.stderr[-2000:])
                    c = json.loads(run.stdout.strip().splitlines()[-1])
                    if i:
                        rates[key].append(round(c["reads"] / c["seconds"], 1))
                    note(f"command {key} round {i}")
            out["command_reads_per_s"] = {k: med(v) for k, v in rates.items()}
            out["command_reads_per_s_all"] = rates
            out["command_file_bytes"] = {"b.bg.gz": os.path.getsize(depth[1]), "p.tsv.gz": os.path.getsize(os.path.join(tmp, "p.tsv.gz"))}
        print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times of the corrected reads (gc_params::device_output & 8; --corrected-out) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp, seed=7), 10 000
reads of 10 kb, seed 11). Not bench.py and gated by nothing: one JSON line. Reported: the device time of the corrected reads' kernels by HIP events beside the output
encoder's from the same batches (the library's GC_DEBUG_TIMES line; medians of --repeat batches after one warm-up), the bytes that come down for them, the host's record
assembly and per-record gzip per batch, and with --command the command's reads/s for -a x.gaf alone, with --corrected-out c.fa and with c.fa.gz, each with its
stage_seconds and the stage that binds (the largest busy time per thread; the aligning workers that had a batch share theirs).
    python3 scripts/corrected_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K] [--command]"""
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
    print("[corrected_times] " + text, file=sys.stderr, flush=True)


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
    ap.add_argument("--command", action="store_true", help="also python -m graphchainer_amd on the same files: -a alone, + --corrected-out c.fa, + c.fa.gz")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    os.environ["GC_DEBUG_TIMES"] = "1"

    import numpy as np

    import graphchainer_amd as gca
    from graphchainer_amd import cli
    from graphchainer_amd.synth import SynthGraph

    gca.set_device(0)
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
        names = (gca.api.C.c_char_p * len(ids))(*ids)
        note("graph built")
        aligner = gca.Aligner(graph, seeder, long_pass=True, device_output=1 | 8)
        line = re.compile(r"k_out_encode \(both passes, k_out_place\) ([0-9.]+) ms; corrected reads \(k_corr_walk both passes, k_corr_place\) ([0-9.]+) ms, ([0-9.]+) MB")
        encode, corrected, walls, formats, gzips = [], [], [], [], []
        for i in range(args.repeat + 1):
            t0 = time.time()
            res, text = with_stderr_captured(lambda: aligner.align_batch(batch))
            wall = (time.time() - t0) * 1e3
            t0 = time.time()
            texts, _ = aligner.format_batch(res, batch, names, formats=("corrected",))
            fmt_ms = (time.time() - t0) * 1e3
            t0 = time.time()
            packed = cli.gzip_records(gca.api, texts["corrected"], texts["corrected_rec_off"])
            gz_ms = (time.time() - t0) * 1e3
            found = line.search(text)
            assert found, "no GC_DEBUG_TIMES line of the output kernels:\n" + text[-2000:]
            if i:
                encode.append(float(found.group(1)))
                corrected.append(float(found.group(2)))
                walls.append(wall)
                formats.append(fmt_ms)
                gzips.append(gz_ms)
            if i == args.repeat:
                n_out = int(res["read_out_off"][-1])
                out["alignments"] = n_out
                out["bytes_down"] = {"corrected_letters": int(res["out_corrected_off"][-1]), "corrected_offsets_and_counts": 12 * n_out + 8,
                                     "gaf_path_and_cigar_text": int(res["out_path_off"][-1]) + int(res["out_cigar_off"][-1])}
                out["records_bytes"], out["records_gz_bytes"] = len(texts["corrected"]), len(packed)
            del res, texts, packed
        med = lambda v: round(float(np.median(v)), 3)   # noqa: E731
        out["device_ms"] = {"k_out_encode": med(encode), "corrected_kernels": med(corrected)}
        out["host_ms_per_batch"] = {"align_batch_wall_with_debug_times": med(walls), "gc_format_corrected": med(formats), "gzip_per_record_on_device": med(gzips)}
        note("batches timed")
        if args.command:
            os.environ.pop("GC_DEBUG_TIMES")
            fq = os.path.join(tmp, "reads.fq")
            with open(fq, "wb") as f:
                for i, r in zip(ids, reads):
                    f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
            code = ("import sys, json; from graphchainer_amd import cli; cfg = cli.resolve(sys.argv[1:]); c = cli.run(cfg); "
                    "print(json.dumps({'reads': c['reads'], 'seconds': c['seconds'], 'inflight': c['inflight'], 'batches': c['batches'], 'stage_seconds': c['stage_seconds']}))")
            runs = {}
            for key, extra in (("warm_up", []), ("gaf", []), ("gaf_corrected_fa", ["--corrected-out", os.path.join(tmp, "c.fa")]), ("gaf_corrected_fa_gz", ["--corrected-out", os.path.join(tmp, "c.fa.gz")])):
                run = subprocess.run([sys.executable, "-c", code, "-g", gfa, "-f", fq, "-a", os.path.join(tmp, "x.gaf")] + extra, capture_output=True, text=True, cwd=ROOT, timeout=1500)
                if run.returncode != 0:
                    raise RuntimeError(run.stderr[-2000:])
                c = json.loads(run.stdout.strip().splitlines()[-1])
                stages = c["stage_seconds"]
                per_thread = {"read": stages["read"]["busy"], "parse": stages["parse"]["busy"], "align": stages["align"]["busy"] / max(1, min(c["inflight"], c["batches"])), "write": stages["write"]["busy"]}
                if key == "warm_up":        # the first run of the command on a box pays for cold files and libraries: not reported
                    continue
                runs[key] = {"reads_per_s": round(c["reads"] / c["seconds"], 1), "inflight": c["inflight"], "batches": c["batches"], "binding_stage": max(per_thread, key=per_thread.get), "stage_seconds": stages}
            out["command"] = runs
        print(json.dumps(out))


if __name__ == "__main__":
    main()

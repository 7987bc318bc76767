#!/usr/bin/env python3
"""Times of the device MUM / MEM seeder (MxmIndex, gc_seeds_mxm) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp, seed=7), 10 000 reads of 10 kb,
seed 11). Not bench.py and gated by nothing: one JSON line with the index build seconds and bytes, gc_seeds_mxm's wall and device milliseconds per batch for MEM and MUM at
min_len 20, count all, the hits per read, and beside them the minimizer path's seed-lookup kernel time for the same batch (kernel_us[0] of gc_align_batch) as the yardstick.
    python3 scripts/mxm_seeding_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per mode after one warm-up call; the median is reported")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

    import numpy as np

    import graphchainer_amd as gca
    from graphchainer_amd.synth import SynthGraph

    gca.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        gfa = os.path.join(tmp, "graph.gfa")
        sg = SynthGraph(args.backbone, seed=7)
        sg.write_gfa(gfa)
        reads = sg.sample_reads(args.reads, args.read_len, seed=11)
        graph = gca.AlignmentGraph(gfa)
        t0 = time.time()
        index = gca.MxmIndex(graph)
        create_s = time.time() - t0
        batch = gca.ReadBatch(reads)
        out = {"graph_bp": int(args.backbone), "reads": len(reads), "read_len": args.read_len, "min_len": args.min_len,
               "index_create_s": round(create_s, 3), "index_host_build_s": round(int(index.array("build_us")[0]) / 1e6, 3), "index_bytes": int(index.array("bytes")[0]),
               "text_letters": int(index.array("node_start")[-1])}
        for mode in ("mem", "mum"):
            walls, kernels, hits = [], [], 0
            for i in range(args.repeat + 1):
                t0 = time.time()
                seeds = index.seeds(batch, mode, count=None, min_len=args.min_len)
                wall = (time.time() - t0) * 1e3
                if i:
                    walls.append(wall)
                    kernels.append(seeds.kernel_ms)
                if i == args.repeat:
                    hits = sum(len(h) for h in seeds.hits())
                seeds.close()
            out[mode] = {"wall_ms": round(float(np.median(walls)), 3), "kernel_ms": round(float(np.median(kernels)), 3), "hits_per_read": round(hits / max(1, len(reads)), 2)}
        aligner = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=False)
        lookups = []
        for i in range(args.repeat + 1):
            res = aligner.align_batch(batch)
            if i:
                lookups.append(float(res["kernel_us"][0]))
        out["minimizer_seed_lookup_kernel_us"] = round(float(np.median(lookups)), 1)
        print(json.dumps(out))


if __name__ == "__main__":
    main()

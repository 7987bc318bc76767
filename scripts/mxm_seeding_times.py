#!/usr/bin/env python3
"""Times of the device MUM / MEM seeder (MxmIndex, gc_seeds_mxm) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp, seed=7), 10 000 reads of 10 kb,
seed 11). Not bench.py and gated by nothing: one JSON line with the index build seconds and bytes, gc_seeds_mxm's wall and device milliseconds per batch for MEM and MUM at
min_len 20, count all, the hits per read, and beside them the minimizer path's seed-lookup kernel time for the same batch (kernel_us[0] of gc_align_batch) as the yardstick.
"index_builds": the ways to the suffix array (gc_mxm_index_open), host and device builds interleaved, medians of --repeat after one warm-up round - host_build_s, device_build_s
(build_us: text and suffix array; *_sa_s: the suffix array alone), device_scratch_bytes and its bytes per text letter, rounds, cache_save_s (writing <prefix>.gcmxm after a build), cache_load_s (reading
and verifying it, build_us of an index opened on the existing file), the *_open_s wall times of the whole calls (upload and prefix table included) and cache_file_bytes.
    python3 scripts/mxm_seeding_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K] [--no-seeding]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def index_builds(gca, np, graph, tmp, repeat):
    """Host build, device build, cache save and cache load of the graph's index, interleaved, `repeat` rounds after one warm-up round."""
    def opened(**kw):
        t0 = time.time()
        index = gca.MxmIndex(graph, **kw)
        wall = time.time() - t0
        got = {k: int(index.array(k)[0]) for k in ("build_us", "sa_us", "build_mode", "build_rounds", "build_scratch_bytes", "cache_save_us")}
        got["open_s"], got["text_letters"] = wall, int(index.array("node_start")[-1])
        index.close()
        return got

    rows = {"host": [], "device": [], "save": [], "load": []}
    prefix = os.path.join(tmp, "index")
    for i in range(repeat + 1):
        host, device = opened(build="host"), opened(build="device")
        if os.path.exists(prefix + ".gcmxm"):
            os.remove(prefix + ".gcmxm")
        save, load = opened(build="device", cache_prefix=prefix), opened(build="device", cache_prefix=prefix)
        assert (host["build_mode"], device["build_mode"], save["build_mode"], load["build_mode"]) == (0, 1, 1, 2)
        if i:
            for key, row in (("host", host), ("device", device), ("save", save), ("load", load)):
                rows[key].append(row)

    def median(key, field, scale=1.0):
        return round(float(np.median([r[field] for r in rows[key]])) * scale, 4)

    letters = rows["device"][0]["text_letters"]
    scratch = rows["device"][0]["build_scratch_bytes"]
    return {"host_build_s": median("host", "build_us", 1e-6), "host_open_s": median("host", "open_s"), "host_rounds": rows["host"][0]["build_rounds"],
            "host_sa_s": median("host", "sa_us", 1e-6),
            "device_build_s": median("device", "build_us", 1e-6), "device_sa_s": median("device", "sa_us", 1e-6), "device_open_s": median("device", "open_s"), "rounds": rows["device"][0]["build_rounds"],
            "device_scratch_bytes": scratch, "device_scratch_bytes_per_letter": round(scratch / max(1, letters), 2),
            "cache_save_s": median("save", "cache_save_us", 1e-6), "cache_load_s": median("load", "build_us", 1e-6), "cache_load_open_s": median("load", "open_s"),
            "cache_file_bytes": os.path.getsize(prefix + ".gcmxm")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per mode after one warm-up call; the median is reported")
    ap.add_argument("--no-seeding", action="store_true", help="the index builds and the cache only")
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
        out["index_builds"] = index_builds(gca, np, graph, tmp, args.repeat)
        if args.no_seeding:
            print(json.dumps(out))
            return
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

#!/usr/bin/env python3
"""Times of the seeds-file path (SeedStore, gc_seed_store_open / gc_seeds_from_store) on bench.py's default graph and read set (config 2: SynthGraph(50.8 Mbp, seed=7),
10 000 reads of 10 kb, seed 11). Not bench.py and gated by nothing: one JSON line. The file is made from the batch's own minimizer hits (what keep_seeds returns, turned back
into node id, offset in the node and strand; one vg::Alignment per hit under the read's name, one group per read, one gzip member). Reported: the file's sizes, the store's
load split into inflate, framing, upload, decode and sort (medians of --repeat loads after one warm-up), the join per batch (wall and device milliseconds), beside them the same
hits through SeedBatch(...) from host arrays, and with --command the command's reads/s with -s beside its minimizer run on the same files. GC_LIBRARY selects a variant
build (make variant NAME=sfnolds FLAGS=-DGC_SEEDFILE_NO_LDS: the decode kernel without its LDS staging).
    python3 scripts/seedfile_times.py [--backbone BP] [--reads N] [--read-len L] [--repeat K] [--command]"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _varint(value):
    out = bytearray()
    while value >= 0x80:
        out.append((value & 0x7F) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def seeds_stream(ids, per_read):
    """One group per read: count, then size + message per hit. A message as vg writes it: path { mapping { position { node_id offset is_reverse } edit { from_length } } } name
    query_position, zero fields left out."""
    out = []
    for name, hits in zip(ids, per_read):
        name_field = b"\x1a" + _varint(len(name)) + name
        out.append(_varint(len(hits)))
        for node_id, offset, seq_pos, length, reverse in hits:
            position = (b"\x08" + _varint(node_id) if node_id else b"") + (b"\x10" + _varint(offset) if offset else b"") + (b"\x20\x01" if reverse else b"")
            edit = b"\x08" + _varint(length) if length else b""
            mapping = b"\x0a" + _varint(len(position)) + position + b"\x12" + _varint(len(edit)) + edit
            path = b"\x12" + _varint(len(mapping)) + mapping
            message = b"\x12" + _varint(len(path)) + path + name_field + (b"\x38" + _varint(seq_pos) if seq_pos else b"")
            out.append(_varint(len(message)))
            out.append(message)
    return b"".join(out)


def note(text):
    print("[seedfile_times] " + text, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3, help="timed loads and joins after one warm-up; the median is reported")
    ap.add_argument("--command", action="store_true", help="also python -m graphchainer_amd with -s and with the minimizer seeder on the same files")
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
        ids = [b"read_%06d" % i for i in range(len(reads))]
        note("graph and reads written")
        graph = gca.AlignmentGraph(gfa)
        batch = gca.ReadBatch(reads)
        note("graph built")
        res = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=False, keep_seeds=True).align_batch(batch)
        node_ids, node_offset = graph.array("nodeIDs"), graph.array("nodeOffset")
        node = np.asarray(res["seed_node"]).astype(np.int64)
        off = np.asarray(res["read_seed_off"]).astype(np.int64)
        flat = np.zeros(len(node), dtype=gca.api.SEED_HIT_DTYPE)
        flat["node_id"], flat["reverse"] = node_ids[node] // 2, node_ids[node] & 1
        flat["node_offset"] = node_offset[node] + np.asarray(res["seed_offset"])
        flat["seq_pos"], flat["match_len"], flat["raw_goodness"] = np.asarray(res["seed_seqpos"]), 15, 15
        del res
        per_read = [flat[off[r]:off[r + 1]] for r in range(len(reads))]
        raw = seeds_stream(ids, [list(zip(h["node_id"].tolist(), h["node_offset"].tolist(), h["seq_pos"].tolist(), h["match_len"].tolist(), h["reverse"].tolist())) for h in per_read])
        path = os.path.join(tmp, "seeds.gam")
        with open(path, "wb") as f:
            f.write(gzip.compress(raw, 6))
        out = {"graph_bp": int(args.backbone), "reads": len(reads), "read_len": args.read_len, "seeds": int(len(flat)), "seeds_per_read": round(len(flat) / max(1, len(reads)), 1),
               "inflated_bytes": len(raw), "file_bytes": os.path.getsize(path), "library": os.path.basename(gca.api.LIB_PATH)}
        del raw
        note("seeds file written: %d seeds" % len(flat))
        loads, joins = [], []
        store = None
        for i in range(args.repeat + 1):
            if store is not None:
                store.close()
            t0 = time.time()
            store = gca.SeedStore([path])
            info = store.info()
            info["wall_ms"] = (time.time() - t0) * 1e3
            if i:
                loads.append(info)
        assert loads[0]["seeds"] == len(flat)
        out["load"] = {k: round(float(np.median([l[k] for l in loads])), 3) for k in ("wall_ms", "inflate_ms", "frame_ms", "upload_ms", "decode_ms", "sort_ms", "host_ms", "device_ms")}
        out["load"].update(hbm_bytes=int(loads[0]["hbm_bytes"]), hbm_bytes_per_seed=round(loads[0]["hbm_bytes"] / max(1, len(flat)), 1), distinct_hashes=int(loads[0]["distinct_hashes"]))
        for i in range(args.repeat + 1):
            t0 = time.time()
            seeds = store.seeds(graph, batch, ids)
            wall = (time.time() - t0) * 1e3
            if i:
                joins.append((wall, seeds.kernel_ms))
            if i == args.repeat:
                got = seeds.hits()
                assert all(np.array_equal(g, w) for g, w in zip(got, per_read)), "the store's hits differ from the file's"
            seeds.close()
        out["join"] = {"wall_ms": round(float(np.median([j[0] for j in joins])), 3), "kernel_ms": round(float(np.median([j[1] for j in joins])), 3)}
        uploads = []
        for i in range(args.repeat + 1):
            t0 = time.time()
            seeds = gca.SeedBatch(graph, batch, per_read)
            if i:
                uploads.append((time.time() - t0) * 1e3)
            seeds.close()
        out["seed_batch_from_host_arrays_wall_ms"] = round(float(np.median(uploads)), 3)
        store.close()
        note("loads and joins timed")
        if args.command:
            fq = os.path.join(tmp, "reads.fq")
            with open(fq, "wb") as f:
                for i, r in zip(ids, reads):
                    f.write(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
            runs = {}
            for key, extra in (("seeds_file", ["-s", path, "--seeds-minimizer-density", "0"]), ("minimizer", [])):
                code = ("import sys, json; from graphchainer_amd import cli; cfg = cli.resolve(sys.argv[1:]); c = cli.run(cfg); print(json.dumps({'reads': c['reads'], 'seconds': c['seconds']}))")
                t0 = time.time()
                run = subprocess.run([sys.executable, "-c", code, "-g", gfa, "-f", fq, "-a", os.path.join(tmp, key + ".gaf")] + extra, capture_output=True, text=True, cwd=ROOT, timeout=1500)
                if run.returncode != 0:
                    raise RuntimeError(run.stderr[-2000:])
                counts = json.loads(run.stdout.strip().splitlines()[-1])
                runs[key] = {"reads_per_s": round(counts["reads"] / counts["seconds"], 1), "process_s": round(time.time() - t0, 2)}   # seconds: reading, aligning, writing; set-up (the store's load among it) left out
            out["command"] = runs
        print(json.dumps(out))


if __name__ == "__main__":
    main()

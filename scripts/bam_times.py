#!/usr/bin/env python3
"""Times of the device BAM loader (ReadBatch.from_bam_bgzf, gc_reads_parse_bam_bgzf) beside the FASTQ loader on the same reads as a BGZF .fq.gz. Not bench.py and gated by
nothing. One JSON line:

  "long"   bench.py's reads (10 000 x 10 kb): the BAM loader's walk, fields, names, unpack and total kernel_ms, the inflater's kernel_ms and the call's wall ms; the FASTQ
           loader's kernel_ms, inflater kernel_ms and wall ms for the same reads
  "short"  the same pair for 150 bp reads that fill 100 MB of BAM, where the serial walk is at its worst
  "command" with --command: python -m graphchainer_amd's end-to-end reads/s (reading, parsing, aligning, writing a GAF; setup left out) on the long reads as .bam and as
           BGZF .fq.gz, with the stage_seconds of the last round

Every figure comes from a child process of its own (the library is chosen when a process loads it), the legs alternating inside every round; the first call of a child is
a warm-up. With --parent-library PATH (a libgraphchainer_amd.so built from the parent commit) the .fq.gz legs run on that library too, "fastq_bgzf_parent": the spread of
its rounds is the margin for comparing the other figures.

    python3 scripts/bam_times.py [--reads N] [--read-len L] [--rounds K] [--short-bytes B] [--command] [--backbone BP] [--parent-library PATH]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bgzf_compress(data, level=1, block=65280):
    """data as bgzip frames it: gzip members of `block` bytes of text with their size in a BC subfield, and the empty block at the end."""
    out = []
    for k in list(range(0, len(data), block)) + [None]:
        piece = data[k:k + block] if k is not None else b""
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out)


def bam_stream(np, reads):
    """Unaligned BAM records (flag 4, quality 40, one RG tag) behind a header without references; the bases packed with numpy."""
    code = np.zeros(256, dtype=np.uint8)
    for k, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        code[c] = k
    out = [b"BAM\x01" + struct.pack("<I", 0) + struct.pack("<I", 0)]
    for i, r in enumerate(reads):
        name = b"read%d\x00" % i
        c = code[np.frombuffer(r, dtype=np.uint8)]
        if len(c) % 2:
            c = np.append(c, np.uint8(0))
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, 0, 4, len(r), -1, -1, 0) + name + ((c[0::2] << 4) | c[1::2]).tobytes() + b"\x28" * len(r) + b"RGZa\x00"
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


def write_inputs(np, reads, prefix):
    fastq = b"".join(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    bam = bam_stream(np, reads)
    with open(prefix + ".fq.gz", "wb") as f:
        f.write(bgzf_compress(fastq))
    with open(prefix + ".bam", "wb") as f:
        f.write(bgzf_compress(bam))
    return {"reads": len(reads), "fastq_text_bytes": len(fastq), "bam_text_bytes": len(bam)}


def child_loader(path, n_reads):
    """Two calls on the file, the second one timed."""
    import graphchainer_amd as gca
    gca.set_device(0)
    data = open(path, "rb").read()
    for _ in range(2):
        t0 = time.time()
        if path.endswith(".bam"):
            batch, ids, tail, consumed = gca.ReadBatch.from_bam_bgzf(b"", data, header=True)
        else:
            batch, ids, tail, consumed = gca.ReadBatch.from_bgzf(b"", data, "fastq")
        wall = (time.time() - t0) * 1e3
        row = {"wall_ms": wall, "kernel_ms": batch.kernel_ms, "inflate_kernel_ms": batch.bgzf["kernel_ms"], "upload_ms": batch.bgzf["upload_ms"]}
        if path.endswith(".bam"):
            row.update({k: batch.bam[k] for k in ("walk_ms", "fields_ms", "names_ms", "unpack_ms")})
        assert len(ids) == n_reads and tail == b"" and consumed == len(data)
        batch.close()
    print(json.dumps(row), flush=True)


def child_command(gfa, path, cache, out):
    from graphchainer_amd import cli
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    rows = []
    for _ in range(2):
        counts = cli.run(cli.resolve(["-g", gfa, "-f", path, "-a", out, "--index-cache", cache]))
        rows.append({"reads_per_s": counts["reads"] / counts["seconds"], "inflight": counts["inflight"], "batches": counts["batches"], "stage_seconds": counts["stage_seconds"]})
    print(json.dumps(rows[-1]), flush=True)


def child(argv, library, timeout):
    env = dict(os.environ)
    if library:
        env["GC_LIBRARY"] = library
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=timeout, env=env)
    lines = [line for line in out.stdout.splitlines() if line.startswith("{")]
    if out.returncode != 0 or not lines:
        sys.exit(f"a child failed (exit status {out.returncode}): {argv}\n" + out.stdout[-2000:] + out.stderr[-2000:])   # nothing more is started
    return json.loads(lines[-1])


def summarise(rows):
    keys = [k for k in rows[0] if isinstance(rows[0][k], (int, float))]
    out = {k: round(sorted(r[k] for r in rows)[len(rows) // 2], 2) for k in keys}
    out["rounds"] = {k: [round(r[k], 2) for r in rows] for k in keys if k in ("kernel_ms", "wall_ms", "walk_ms", "reads_per_s")}
    if "stage_seconds" in rows[-1]:
        out["stage_seconds"] = rows[-1]["stage_seconds"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--short-bytes", type=int, default=100_000_000, help="bytes of BAM text the 150 bp reads fill (0: leave the short reads out)")
    ap.add_argument("--command", action="store_true")
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--parent-library", default="")
    ap.add_argument("--timeout", type=int, default=600, help="seconds a child may take")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "loader":
            child_loader(args.child[1], int(args.child[2]))
        else:
            child_command(*args.child[1:5])
        return

    import numpy as np
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    result = {"rounds": args.rounds, "parent_library": bool(args.parent_library)}
    with tempfile.TemporaryDirectory() as tmp:
        sets = {"long": [bytes(letters[rng.integers(0, 4, args.read_len)]) for _ in range(args.reads)]}
        if args.short_bytes:
            per_record = 36 + 12 + 75 + 150 + 5
            sets["short"] = [bytes(letters[rng.integers(0, 4, 150)]) for _ in range(args.short_bytes // per_record)]
        if args.command:
            from graphchainer_amd.synth import SynthGraph
            sg = SynthGraph(args.backbone, seed=7)
            sg.write_gfa(os.path.join(tmp, "graph.gfa"))
            sets["long"] = [r if isinstance(r, bytes) else r.encode() for r in sg.sample_reads(args.reads, args.read_len, seed=11)]
        for name, reads in sets.items():
            prefix = os.path.join(tmp, name)
            result[name] = write_inputs(np, reads, prefix)
            legs = [("bam", prefix + ".bam", ""), ("fastq_bgzf", prefix + ".fq.gz", "")] + ([("fastq_bgzf_parent", prefix + ".fq.gz", args.parent_library)] if args.parent_library else [])
            rows = {leg: [] for leg, _, _ in legs}
            for _ in range(args.rounds):
                for leg, path, library in legs:
                    rows[leg].append(child(["--child", "loader", path, str(len(reads))], library, args.timeout))
            result[name].update({leg: summarise(v) for leg, v in rows.items()})
        if args.command:
            gfa, cache, out = os.path.join(tmp, "graph.gfa"), os.path.join(tmp, "index.gcidx"), os.path.join(tmp, "out.gaf")
            prefix = os.path.join(tmp, "long")
            legs = [("bam", prefix + ".bam", ""), ("fastq_bgzf", prefix + ".fq.gz", "")] + ([("fastq_bgzf_parent", prefix + ".fq.gz", args.parent_library)] if args.parent_library else [])
            rows = {leg: [] for leg, _, _ in legs}
            child(["--child", "command", gfa, prefix + ".fq.gz", cache, out], "", args.timeout)          # builds and saves the index cache
            for _ in range(args.rounds):
                for leg, path, library in legs:
                    rows[leg].append(child(["--child", "command", gfa, path, cache, out], library, args.timeout))
            result["command"] = {"graph_bp": args.backbone, "what": "reads/s of python -m graphchainer_amd -g graph.gfa -f reads -a out.gaf, the second of two runs of a process",
                                 **{leg: summarise(v) for leg, v in rows.items()}}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()

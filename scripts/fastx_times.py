#!/usr/bin/env python3
"""Times of the device FASTA / FASTQ loader (ReadBatch.from_text, gc_reads_parse) on about 100 MB of 10 kb reads, beside the host's way to the same batch. Not bench.py
and gated by nothing. Two JSON lines:

1. per input (FASTA of width 60, FASTQ, FASTQ.gz, and the FASTQ as BGZF - see below): the text's bytes; from_text's wall milliseconds and the loader's kernel_ms; the same reads cut from the text by the
   Python list comprehension the tests use and handed to ReadBatch(list) (cut_ms + upload_ms); for the .gz the host's zlib inflate on its own. Three rounds after one
   warm-up round, the two ways interleaved inside a round, medians. The BGZF file (blocks of 65 280 bytes of text at zlib level 1, as the .gz) has a row of its own,
   "fastq_bgzf": ReadBatch.from_bgzf's wall milliseconds with the inflater's scan, upload and kernel milliseconds and the loader's kernel_ms, beside the host's zlib over
   the same file followed by from_text.
2. with --command: the command line's end-to-end reads/s (reading, parsing, aligning, writing a GAF; graph and index setup left out) on bench.py's default graph and read
   set as a FASTQ file, as a one-member .fq.gz and as a BGZF .fq.gz, for every value of --inflight (0: not given, the command chooses) with the stage times of the last round, and
   bench.py --full's e2e.gaf reads/s of the same build on the same box when --bench is given too (that leg keeps five batches in flight and encodes on the device).

    python3 scripts/fastx_times.py [--reads N] [--read-len L] [--rounds K] [--command [--inflight K ...] [--batch-bytes B] [--backbone BP] [--bench]]"""
import argparse
import gzip
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


def inflate_members(data):
    """The host's zlib over a BGZF file, member by member, each cut out by its BSIZE (no copy of the rest of the file per member)."""
    out, view, at = [], memoryview(data), 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(zlib.decompressobj(47).decompress(view[at:at + size]))
        at += size
    return b"".join(out)


def bgzf_times(gca, np, fastq, n_reads, rounds):
    data = bgzf_compress(fastq)
    rows = {k: [] for k in ("device_wall_ms", "scan_ms", "upload_ms", "inflate_kernel_ms", "parse_kernel_ms", "host_inflate_ms", "host_from_text_ms")}
    for i in range(rounds + 1):
        t0 = time.time()
        batch, ids, tail, consumed = gca.ReadBatch.from_bgzf(b"", data, "fastq")
        t1 = time.time()
        stats, kernel_ms, blob = batch.bgzf, batch.kernel_ms, batch.blob
        batch.close()
        assert len(ids) == n_reads and consumed == len(data) and tail == b""
        t2 = time.time()
        text = inflate_members(data)
        t3 = time.time()
        host, host_ids, _ = gca.ReadBatch.from_text(text, "fastq")
        t4 = time.time()
        assert host_ids == ids and host.blob == blob
        host.close()
        if i:
            for k, v in (("device_wall_ms", (t1 - t0) * 1e3), ("scan_ms", stats["scan_ms"]), ("upload_ms", stats["upload_ms"]), ("inflate_kernel_ms", stats["kernel_ms"]),
                         ("parse_kernel_ms", kernel_ms), ("host_inflate_ms", (t3 - t2) * 1e3), ("host_from_text_ms", (t4 - t3) * 1e3)):
                rows[k].append(v)
    med = {k: round(float(np.median(v)), 2) for k, v in rows.items()}
    return {"file_bytes": len(data), "text_bytes": len(fastq), "blocks": stats["blocks"], "from_bgzf_wall_ms": med["device_wall_ms"], "scan_ms": med["scan_ms"], "upload_ms": med["upload_ms"],
            "inflate_kernel_ms": med["inflate_kernel_ms"], "inflate_kernel_GBps": round(len(fastq) / max(med["inflate_kernel_ms"], 1e-3) / 1e6, 2), "parse_kernel_ms": med["parse_kernel_ms"],
            "host_inflate_ms": med["host_inflate_ms"], "host_from_text_ms": med["host_from_text_ms"], "host_inflate_and_from_text_ms": round(med["host_inflate_ms"] + med["host_from_text_ms"], 2),
            "rounds": {k: [round(x, 2) for x in v] for k, v in rows.items()}}


def loader_times(gca, np, reads, rounds):
    fasta = b"".join(b">read%d\n" % i + b"".join(r[k:k + 60] + b"\n" for k in range(0, len(r), 60)) for i, r in enumerate(reads))
    fastq = b"".join(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    packed = gzip.compress(fastq, 1)

    def cut_fasta(text):         # the tests' way with a FASTA of one line per read does not fit width 60: join the lines of every record
        return [b"".join(rec.split(b"\n")[1:]) for rec in text.split(b">")[1:]]

    def cut_fastq(text):
        return text.split(b"\n")[1::4]

    inputs = {"fasta_width60": (fasta, "fasta", cut_fasta, None), "fastq": (fastq, "fastq", cut_fastq, None), "fastq_gz": (packed, "fastq", cut_fastq, zlib.decompressobj(47).decompress)}
    rows = {name: {"device_wall_ms": [], "kernel_ms": [], "cut_ms": [], "upload_ms": [], "inflate_ms": []} for name in inputs}
    for i in range(rounds + 1):
        for name, (data, fmt, cut, inflate) in inputs.items():
            t0 = time.time()
            text = zlib.decompressobj(47).decompress(data) if inflate else data
            t1 = time.time()
            batch, ids, _ = gca.ReadBatch.from_text(text, fmt)
            t2 = time.time()
            kernel_ms, n, blob = batch.kernel_ms, len(ids), batch.blob
            batch.close()
            t3 = time.time()
            cut_reads = cut(text)
            t4 = time.time()
            uploaded = gca.ReadBatch(cut_reads)
            t5 = time.time()
            assert n == len(reads) == len(cut_reads) and blob == uploaded.blob
            uploaded.close()
            if i:
                row = rows[name]
                row["inflate_ms"].append((t1 - t0) * 1e3)
                row["device_wall_ms"].append((t2 - t1) * 1e3)
                row["kernel_ms"].append(kernel_ms)
                row["cut_ms"].append((t4 - t3) * 1e3)
                row["upload_ms"].append((t5 - t4) * 1e3)
    out = {}
    for name, (data, _, _, inflate) in inputs.items():
        med = {k: round(float(np.median(v)), 2) for k, v in rows[name].items()}
        text_bytes = len(fastq) if inflate else len(data)
        out[name] = {"file_bytes": len(data), "text_bytes": text_bytes, "from_text_wall_ms": med["device_wall_ms"], "from_text_kernel_ms": med["kernel_ms"],
                     "from_text_GBps": round(text_bytes / med["device_wall_ms"] / 1e6, 2), "kernel_GBps": round(text_bytes / max(med["kernel_ms"], 1e-3) / 1e6, 2),
                     "host_cut_ms": med["cut_ms"], "host_upload_ms": med["upload_ms"], "host_cut_and_upload_ms": round(med["cut_ms"] + med["upload_ms"], 2)}
        if inflate:
            out[name]["host_inflate_ms"] = med["inflate_ms"]
    out["fastq_bgzf"] = bgzf_times(gca, np, fastq, len(reads), rounds)
    return out


def command_times(gca, args, tmp):
    from graphchainer_amd import cli
    from graphchainer_amd.synth import SynthGraph
    gfa, fq, cache = os.path.join(tmp, "graph.gfa"), os.path.join(tmp, "reads.fq"), os.path.join(tmp, "index.gcidx")
    sg = SynthGraph(args.backbone, seed=7)
    sg.write_gfa(gfa)
    reads = sg.sample_reads(args.reads, args.read_len, seed=11)
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            r = r if isinstance(r, bytes) else r.encode()
            f.write(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    with open(fq, "rb") as f, gzip.open(fq + ".gz", "wb", 1) as g:       # one member, as a compressor writes it
        while True:
            piece = f.read(1 << 24)
            if not piece:
                break
            g.write(piece)
    with open(fq, "rb") as f, open(os.path.join(tmp, "reads.bgzf.fq.gz"), "wb") as g:
        g.write(bgzf_compress(f.read()))
    legs = {"fastq": fq, "fastq_gz": fq + ".gz", "fastq_bgzf": os.path.join(tmp, "reads.bgzf.fq.gz")}
    rates = {leg: {k: [] for k in args.inflight} for leg in legs}
    last = {leg: {} for leg in legs}
    for i in range(args.rounds + 1):            # a warm-up round, then the runs alternating inside every round
        for leg, path in legs.items():
            for k in args.inflight:
                argv = ["-g", gfa, "-f", path, "-a", os.path.join(tmp, "out.gaf"), "--index-cache", cache] + (["--inflight", str(k)] if k else [])
                if args.batch_bytes:
                    argv += ["--batch-bytes", str(args.batch_bytes)]
                counts = cli.run(cli.resolve(argv))
                if i:
                    rates[leg][k].append(counts["reads"] / counts["seconds"])
                    last[leg][k] = counts
    name = lambda k: str(k) if k else "chosen"   # noqa: E731
    out = {"reads": len(reads), "read_len": args.read_len, "graph_bp": args.backbone, "rounds": args.rounds, "batch_bytes": args.batch_bytes or "default",
           "what": "python -m graphchainer_amd -g graph.gfa -f reads.fq[.gz] -a out.gaf [--inflight K]: reading, parsing on the device, aligning, formatting and writing; reads/s, "
                   "median and every round, per batches in flight (chosen: --inflight not given)"}
    for leg in legs:
        out[leg] = {name(k): {"reads_per_s": round(sorted(v)[len(v) // 2], 1), "rounds": [round(x, 1) for x in v], "inflight": last[leg][k]["inflight"], "batches": last[leg][k]["batches"],
                              "retired_workers": last[leg][k]["retired_workers"], "bgzf_blocks": last[leg][k]["bgzf_blocks"], "stage_seconds": last[leg][k]["stage_seconds"]} for k, v in rates[leg].items()}
    out["command_reads_per_s"] = out["fastq"][name(args.inflight[-1])]["reads_per_s"]
    if args.bench:
        bench = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--no-cpu-baseline", "--setup-dir", tmp], capture_output=True, text=True,
                               timeout=args.bench_timeout)
        lines = [line for line in bench.stdout.splitlines() if line.startswith("{") and '"e2e"' in line]
        if bench.returncode != 0 or not lines:
            sys.exit(f"bench.py --full failed (exit status {bench.returncode}):\n" + bench.stdout[-2000:] + bench.stderr[-2000:])
        out["bench_e2e_gaf_reads_per_s"] = json.loads(lines[-1])["e2e"]["gaf"]["reads_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--command", action="store_true")
    ap.add_argument("--backbone", type=int, default=50_800_000)
    ap.add_argument("--inflight", type=int, nargs="+", default=[0], help="with --command: the --inflight values to run, each in every round (0: not given, the command chooses)")
    ap.add_argument("--batch-bytes", type=int, default=0, help="with --command: the command's --batch-bytes (default: its own, 100 MB)")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-timeout", type=int, default=900, help="seconds the bench.py child may take")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

    import numpy as np

    import graphchainer_amd as gca

    gca.set_device(0)
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads = [bytes(letters[rng.integers(0, 4, args.read_len)]) for _ in range(args.reads)]
    print(json.dumps({"reads": args.reads, "read_len": args.read_len, "rounds": args.rounds, **loader_times(gca, np, reads, args.rounds)}), flush=True)
    if args.command:
        with tempfile.TemporaryDirectory() as tmp:
            print(json.dumps(command_times(gca, args, tmp)), flush=True)


if __name__ == "__main__":
    main()

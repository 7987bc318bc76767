"""The command line without a GPU: cli.resolve over a table of command lines (one row per rule taken from the reference's src/AlignerMain.cpp), the refused options,
and gc_reads_parse's host-side refusals."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graphchainer_amd import cli          # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa", "-a", "o.gaf"]
DEFAULTS = dict(bandwidth=10, ramp_bandwidth=0, max_cells_per_slice=-1, split_len=35, split_gap=35, colinear_gap=10000, seed_density=10.0, e_cutoff=-1.0, force_global=False,
                seed_extend_density=-1.0, extra_heuristic=False, colinear_chaining=True, selection_method=7, fast_mode=False, precise_clipping=0.0, x_drop=0)
MINIMIZER = {"kind": "minimizer", "length": 15, "window": 20, "keep_fraction": 1 - 0.001}

# (what the row is about, arguments after BASE, expected Aligner fields that differ from DEFAULTS, other expected Config attributes, a warning that must be printed)
ROWS = [
    ("the vg presets and the chaining defaults (:186-209)", [], {}, {"seeder": MINIMIZER, "min_cluster_size": 1, "threads": 1, "cigar_match_mismatch": False, "batch_bytes": 100 << 20, "device": 0}, None),
    ("long names, = and unambiguous prefixes", ["--bandwidth=12", "--colinear-ga", "500"], {"bandwidth": 12, "colinear_gap": 500}, {}, None),
    ("--sampling-step sets the gap (:236-243)", ["--sampling-step", "3", "--colinear-split-len", "20"], {"split_len": 20, "split_gap": 60}, {}, None),
    ("... and overrides --colinear-split-gap with a warning", ["--sampling-step", "2", "--colinear-split-gap", "9"], {"split_gap": 70}, {}, "WARNING: --sampling-step and --colinear-split-gap are both set!"),
    ("--sampling-step 1 leaves the gap alone", ["--sampling-step", "1", "--colinear-split-gap", "9"], {"split_gap": 9}, {}, None),
    ("--seeds-minimizer-ignore-frequent f is the seeder's 1 - f", ["--seeds-minimizer-ignore-frequent", "0.25", "--seeds-minimizer-length", "11", "--seeds-minimizer-windowsize", "7"], {},
     {"seeder": {"kind": "minimizer", "length": 11, "window": 7, "keep_fraction": 0.75}}, None),
    ("MUM seeds need the minimizer density at 0", ["--seeds-minimizer-density", "0", "--seeds-mum-count", "5", "--seeds-mxm-length", "12", "--seeds-mxm-cache-prefix", "/tmp/p"], {"seed_density": 0.0},
     {"seeder": {"kind": "mxm", "mode": "mum", "count": 5, "min_len": 12, "cache_prefix": "/tmp/p"}}, None),
    ("MEM seeds, -1 for all", ["--seeds-minimizer-density", "0", "--seeds-mem-count", "-1"], {"seed_density": 0.0}, {"seeder": {"kind": "mxm", "mode": "mem", "count": -1, "min_len": 20, "cache_prefix": ""}}, None),
    ("-B above -b", ["-b", "5", "-B", "6"], {"bandwidth": 5, "ramp_bandwidth": 6}, {}, None),
    ("-C", ["-C", "3000"], {"max_cells_per_slice": 3000}, {}, None),
    ("-C -1 is unlimited", ["-C", "-1"], {"max_cells_per_slice": -1}, {}, None),
    ("--precise-clipping", ["--precise-clipping", "0.75"], {"precise_clipping": 0.75}, {}, None),
    ("... below 0.501 warns", ["--precise-clipping", "0.4"], {"precise_clipping": 0.4}, {}, "Warning: precise clipping identity cutoff set below 0.501."),
    ("--X-drop with --precise-clipping", ["--X-drop", "30", "--precise-clipping", "0.9"], {"x_drop": 30, "precise_clipping": 0.9}, {}, None),
    ("--X-drop alone runs at 0.66 (:443-448)", ["--X-drop", "30"], {"x_drop": 30, "precise_clipping": 0.66}, {}, "--X-drop is set but --precise-clipping is not, using default value of --precise-clipping .66"),
    ("chaining sets try-all-seeds: the density is overridden (:449-453)", ["--seeds-extend-density", "0.002"], {"seed_extend_density": -1.0}, {},
     "WARNING: --try-all-seeds and --seeds-extend-density are both set! --seeds-extend-density will be ignored"),
    ("... -1 is no override", ["--seeds-extend-density", "-1"], {}, {}, None),
    ("without chaining the density stays", ["--no-colinear-chaining", "--seeds-extend-density", "0.002"], {"colinear_chaining": False, "selection_method": 0, "seed_extend_density": 0.002}, {}, None),
    ("--no-colinear-chaining selects greedily by length (:158)", ["--no-colinear-chaining"], {"colinear_chaining": False, "selection_method": 0}, {}, None),
    ("--schedule-inverse-E-sum", ["--no-colinear-chaining", "--schedule-inverse-E-sum"], {"colinear_chaining": False, "selection_method": 3}, {}, None),
    ("--schedule-inverse-E-product", ["--no-colinear-chaining", "--schedule-inverse-E-product"], {"colinear_chaining": False, "selection_method": 4}, {}, None),
    ("--schedule-score", ["--no-colinear-chaining", "--schedule-score"], {"colinear_chaining": False, "selection_method": 5}, {}, None),
    ("--schedule-length", ["--no-colinear-chaining", "--schedule-length"], {"colinear_chaining": False, "selection_method": 6}, {}, None),
    ("--greedy-length", ["--no-colinear-chaining", "--greedy-length"], {"colinear_chaining": False, "selection_method": 0}, {}, None),
    ("--greedy-E and --greedy-score are declared and never read", ["--no-colinear-chaining", "--greedy-E", "--greedy-score"], {"colinear_chaining": False, "selection_method": 0}, {}, None),
    ("--all-alignments", ["--all-alignments"], {"selection_method": 7}, {}, None),
    ("--all-alignments without chaining selects all (:260-265)", ["--no-colinear-chaining", "--all-alignments"], {"colinear_chaining": False, "selection_method": 7}, {}, None),
    ("... and sets try-all-seeds, which overrides the density (:263,449-453)", ["--no-colinear-chaining", "--all-alignments", "--seeds-extend-density", "0.002"],
     {"colinear_chaining": False, "selection_method": 7, "seed_extend_density": -1.0}, {}, "WARNING: --try-all-seeds and --seeds-extend-density are both set!"),
    ("--try-all-seeds without chaining: greedy by length, the density overridden", ["--no-colinear-chaining", "--try-all-seeds", "--seeds-extend-density", "0.5"],
     {"colinear_chaining": False, "selection_method": 0, "seed_extend_density": -1.0}, {}, "WARNING: --try-all-seeds and --seeds-extend-density are both set!"),
    ("--try-all-seeds without chaining and without a density changes nothing", ["--no-colinear-chaining", "--try-all-seeds"], {"colinear_chaining": False, "selection_method": 0}, {}, None),
    ("--greedy-length with chaining", ["--greedy-length"], {"selection_method": 0}, {}, None),
    ("--cigar-match-mismatch", ["--cigar-match-mismatch"], {}, {"cigar_match_mismatch": True}, None),
    ("--E-cutoff, --global-alignment, --extra-heuristic, --fast-mode", ["--E-cutoff", "1e-5", "--global-alignment", "--extra-heuristic", "--fast-mode"],
     {"e_cutoff": 1e-5, "force_global": True, "extra_heuristic": True, "fast_mode": True}, {}, None),
    ("--seeds-clustersize", ["--seeds-clustersize", "3"], {}, {"min_cluster_size": 3}, None),
    ("accepted and without effect", ["-t", "8", "--high-memory", "--verbose", "--short-verbose"], {}, {"threads": 8}, None),
    ("several -a, several files behind one -f", ["-a", "x.json", "-a", "y.gam", "-f", "a.fq", "b.fa.gz"], {}, {"outputs": {"gaf": "o.gaf", "json": "x.json", "gam": "y.gam"}, "reads": ["r.fa", "a.fq", "b.fa.gz"]}, None),
    ("own options", ["--batch-bytes", "3000", "--device", "2", "--index-cache", "i.gcidx"], {}, {"batch_bytes": 3000, "device": 2, "index_cache": "i.gcidx"}, None),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_resolve(row):
    _, args, fields, attributes, warning = row
    cfg = cli.resolve(BASE + args)
    assert cfg.aligner == {**DEFAULTS, **fields}
    assert cfg.graph == "g.gfa"
    for name, value in {"reads": ["r.fa"], "outputs": {"gaf": "o.gaf"}, **attributes}.items():
        got = getattr(cfg, name)
        assert got == (pytest.approx(value) if name == "seeder" and value["kind"] == "minimizer" else value), name
    if warning is None:
        assert cfg.warnings == []
    else:
        assert len(cfg.warnings) == 1 and cfg.warnings[0].startswith(warning)


# (what, whole command line, lines that stderr must hold)
ERRORS = [
    ("the three 'must be given'", [], ["graph file must be given", "read file must be given", "alignments-out must be given"]),
    ("--sampling-step is an integer", BASE + ["--sampling-step", "0.5"], ["the argument ('0.5') for option '--sampling-step' is invalid"]),
    ("--seeds-mum-count alone: the minimizer density is still 10", BASE + ["--seeds-mum-count", "5"], ["pick only one seeding method"]),
    ("no seeding method", BASE + ["--seeds-minimizer-density", "0"], ["pick a seeding method"]),
    ("-B must exceed -b", BASE + ["-B", "10"], ["ramp bandwidth must be higher than default bandwidth"]),
    ("-b 0", BASE + ["-b", "0"], ["default bandwidth must be >= 1"]),
    ("-t 0", BASE + ["-t", "0"], ["number of threads must be >= 1"]),
    ("precise clipping range", BASE + ["--precise-clipping", "1.0"], ["precise clipping identity cutoff must be between 0.001 and 0.999"]),
    ("X-drop floor", BASE + ["--X-drop", "0"], ["X-drop score cutoff must be > 1"]),
    ("two selection methods", BASE + ["--greedy-length", "--schedule-score"], ["pick only one method for selecting outputted alignments"]),
    ("unknown output suffix", ["-g", "g.gfa", "-f", "r.fa", "-a", "o.sam"], ["unknown output alignment format (o.sam), must be either .gaf, .gam or .json"]),
    ("every error is reported", BASE + ["-B", "3", "--X-drop", "0", "--seeds-mxm-length", "1"], ["X-drop score cutoff must be > 1", "ramp bandwidth must be higher than default bandwidth", "mum/mem minimum length must be >= 2"]),
    ("minimizer checks", BASE + ["--seeds-minimizer-length", "32", "--seeds-minimizer-ignore-frequent", "1", "--seeds-minimizer-density", "-2", "--seeds-extend-density", "0"],
     ["Maximum minimizer length is 31", "Minimizer discard fraction must be 0 <= x < 1", "Minimizer density can't be negative", "Seed extension density can't be negative"]),
    ("unknown option", BASE + ["--no-such-option"], ["unrecognised option '--no-such-option'"]),
    ("missing argument", ["-g"], ["the required argument for option '--graph' is missing"]),
    ("an option twice", BASE + ["-g", "h.gfa"], ["option '--graph' cannot be specified more than once"]),
]


@pytest.mark.parametrize("row", ERRORS, ids=[r[0] for r in ERRORS])
def test_errors_in_the_reference_s_words(row):
    _, argv, lines = row
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(argv)
    assert e.value.status == 1
    got = e.value.stderr.splitlines()
    assert got[-1] == "run with option -h for help"
    at = -1
    for line in lines:                       # all of them, in the reference's order
        assert line in got[at + 1:], (line, got)
        at = got.index(line, at + 1)


def test_warnings_and_errors_come_in_the_order_of_the_reference_s_checks():
    """The reference prints as it checks: the precise-clipping warning (:311) behind nothing, the output suffix error (:356) behind it, the X-drop note (:445) behind that."""
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(["-g", "g.gfa", "-f", "r.fa", "-a", "o.sam", "--precise-clipping", "0.4", "--sampling-step", "2", "--colinear-split-gap", "3", "-B", "4", "--seeds-extend-density", "0.1"])
    got = e.value.stderr.splitlines()
    assert [l.split(":")[0].split(" ")[0] for l in got] == ["WARNING", "Warning", "unknown", "ramp", "WARNING", "run"], got
    assert "--sampling-step" in got[0] and "--try-all-seeds" in got[4]


def test_a_truncated_or_damaged_gzip_file_is_an_error(tmp_path):
    """api._file_chunks (host only): members are inflated piece by piece and concatenated; a file that ends inside a member raises instead of ending the reads there, and
    bytes that are no gzip member raise zlib.error. cli.main turns both into one line and exit status 1."""
    import gzip
    import zlib
    from graphchainer_amd import api
    text = b"".join(b"@r%d\n" % i + b"ACGT" * 50 + b"\n+\n" + b"I" * 200 + b"\n" for i in range(200))
    whole = gzip.compress(text[:7000]) + gzip.compress(text[7000:])
    (tmp_path / "ok.fq.gz").write_bytes(whole)
    assert b"".join(api._file_chunks(str(tmp_path / "ok.fq.gz"), True, 1000)) == text
    assert max(len(c) for c in api._file_chunks(str(tmp_path / "ok.fq.gz"), True, 1000)) <= 1000
    (tmp_path / "cut.fq.gz").write_bytes(whole[:-20])
    with pytest.raises(EOFError):
        list(api._file_chunks(str(tmp_path / "cut.fq.gz"), True, 1000))
    (tmp_path / "junk.fq.gz").write_bytes(whole + b"not a gzip member at all")
    with pytest.raises(zlib.error):
        list(api._file_chunks(str(tmp_path / "junk.fq.gz"), True, 1000))
    assert list(api._file_chunks(str(tmp_path / "ok.fq.gz"), False, 1 << 20)) == [whole]


def test_output_files_leave_nothing_behind_when_one_cannot_be_opened(tmp_path):
    paths = {"gaf": str(tmp_path / "a.gaf"), "json": str(tmp_path / "no such directory" / "b.json")}
    with pytest.raises(OSError):
        with cli._Outputs(paths):
            pass
    assert list(tmp_path.iterdir()) == []
    with pytest.raises(RuntimeError):
        with cli._Outputs({"gaf": paths["gaf"]}) as out:
            out.write("gaf", b"x")
            raise RuntimeError("the run failed")
    assert list(tmp_path.iterdir()) == []
    with cli._Outputs({"gaf": paths["gaf"]}) as out:
        out.write("gaf", b"line\n")
    assert [p.name for p in tmp_path.iterdir()] == ["a.gaf"] and open(paths["gaf"], "rb").read() == b"line\n"


def test_help_and_version_exit_0():
    for flag in ("-h", "--help"):
        with pytest.raises(cli.CliExit) as e:
            cli.resolve([flag])
        assert e.value.status == 0 and "--alignments-out" in e.value.stderr
        for name in ("--threads", "--high-memory", "--verbose", "--short-verbose"):
            assert name in e.value.stderr.split("Accepted and without effect")[1]
        for name in cli.REFUSED:
            assert "--" + name in e.value.stderr.split("Not supported by this build")[1]
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(["--version"])
    assert e.value.status == 0 and e.value.stdout.startswith("Version ")


REFUSED = [[f"--{name}"] + (["5"] if cli.OPTIONS[name][1] else []) for name in cli.REFUSED]


@pytest.mark.parametrize("extra", REFUSED + [["vg"]], ids=[" ".join(r) for r in REFUSED] + ["a .vg graph"])
def test_refused_options_exit_1_before_the_library_is_loaded(extra):
    """One line that names the option and says "not supported by this build", exit status 1, and the process has not loaded the library."""
    argv = ["-g", "graph.vg", "-f", "r.fa", "-a", "o.gaf"] if extra == ["vg"] else BASE + extra
    program = ("import sys\nfrom graphchainer_amd import cli, api\nstatus = cli.main(sys.argv[1:])\n"
               "loaded = api._lib is not None or 'libgraphchainer_amd' in open('/proc/self/maps').read()\nprint('LOADED' if loaded else 'NOT LOADED')\nsys.exit(status)\n")
    out = subprocess.run([sys.executable, "-c", program] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 1 and out.stdout.strip() == "NOT LOADED", out.stdout + out.stderr
    lines = out.stderr.splitlines()
    named = ".vg" if extra == ["vg"] else extra[0]
    assert len(lines) == 2 and named in lines[0] and "not supported by this build" in lines[0] and lines[1] == "run with option -h for help"


def test_module_entry_point_reports_a_bad_command_line():
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd", "-a", "x.txt"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 1 and "graph file must be given" in out.stderr and "unknown output alignment format (x.txt)" in out.stderr and out.stdout == ""


def test_reads_parse_refuses_malformed_calls_before_a_device_is_needed():
    """gc_reads_parse checks its arguments on the host first: GC_ERR_INVALID (-1) with or without a GPU."""
    import graphchainer_amd as gca
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = gca.load_library()
    reads, table = C.c_void_p(), C.POINTER(gca.api.GcFastxTable)()
    lib.gc_reads_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(gca.api.GcFastxTable))]
    lib.gc_fastx_table_free.argtypes = [C.POINTER(gca.api.GcFastxTable)]
    text = b">a\nACGT\n"
    assert lib.gc_reads_parse(text, len(text), 1, 1, None, C.byref(table)) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_reads_parse(text, len(text), 1, 1, C.byref(reads), None) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_reads_parse(None, 5, 1, 1, C.byref(reads), C.byref(table)) == -1 and b"null" in lib.gc_last_error()
    for fmt in (0, 3, -1):
        assert lib.gc_reads_parse(text, len(text), fmt, 1, C.byref(reads), C.byref(table)) == -1 and b"format" in lib.gc_last_error()
    for flags in (2, 3, 1 << 31):
        assert lib.gc_reads_parse(text, len(text), 2, flags, C.byref(reads), C.byref(table)) == -1 and b"flag" in lib.gc_last_error()
    for length in ((1 << 32) - 16, 1 << 32, 1 << 40):
        assert lib.gc_reads_parse(text, length, 2, 0, C.byref(reads), C.byref(table)) == -1 and b"32-bit" in lib.gc_last_error()
    assert not reads.value and not table
    lib.gc_fastx_table_free(None)
    if gca.device_count() == 0:      # a well-formed call gets as far as the device: no CPU fallback
        assert lib.gc_reads_parse(text, len(text), 1, 1, C.byref(reads), C.byref(table)) == -3
    with pytest.raises(ValueError):
        gca.ReadBatch.from_text(text, "sam")
    assert {"gc_reads_parse", "gc_fastx_table_free"} <= set(gca.api.EXPORTED_SYMBOLS)

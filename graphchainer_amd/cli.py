"""The command line: `python -m graphchainer_amd -g graph.gfa -f reads.fq.gz -a out.gaf`, the reference's GraphChainer binary over this library. -f also takes unaligned
BAM (reads.bam), which the reference does not: its records are decoded on the device.

resolve(argv) -> Config turns a command line into what a run needs - the reference's option names, short forms, defaults, checks and messages
(src/AlignerMain.cpp:35-112,138-464) - and touches neither the library nor a device. main(argv) runs it (run, over pipeline.py): a reader thread, a parse thread (the reads are parsed on the device, about
--batch-bytes of file text per batch), up to --inflight workers per device of --devices, each with an Aligner of its own (the alignments are encoded on the device for the
writers chosen), and a writer thread: records written in input order, every output file through a temporary name and a rename.
--corrected-out / --corrected-clipped-out are GraphAligner's (the reference keeps their mechanism, src/Aligner.cpp:313-374, and dropped the two option lines): the
corrected reads, their pieces spelled on the device, beside -a or without it.
--coverage-out / --base-coverage-out are this build's own: how often every segment / every base of the graph lies under an alignment the run writes, counted on the
device while the traces are there (api.Coverage), one handle per device, merged and spelled at the end; beside -a or without it.
--link-coverage-out / --coverage-gfa-out / --supported-subgraph-out, this build's own too, come from the same handles: how often every link of the graph is walked, as a
table, as the graph itself with RC tags on segments and links, and as the part of the graph the alignments touch.
--pileup-out (with --pileup-min-alt / --pileup-min-alt-fraction), from the same handles as well: per base of the graph how the alignments written disagree with it -
mismatches by read letter, deletions, insertions before and after - written piece by piece.

Accepted and without effect: -t / --threads (checked >= 1), --high-memory, --verbose, --short-verbose (the progress text and the closing statistics are not
reproduced), and --greedy-E / --greedy-score, which the reference declares and never reads. --try-all-seeds (and --all-alignments, which sets it) does what it does
in the reference: it overrides --seeds-extend-density to -1 with a warning (src/AlignerMain.cpp:449-453); the whole-read call itself never tries all seeds
(src/Aligner.cpp:565, with and without chaining). Refused with one line and exit status 1, before anything is loaded: the options in REFUSED and a .vg graph.
"""
import math
import os
import re
import sys
import time
from dataclasses import dataclass, field

VERSION = "graphchainer_amd 1.0"
UNLIMITED = (1 << 64) - 1          # what the reference's size_t options hold after "-1"

# name -> (short form, value type or None for a switch, takes several values)
OPTIONS = {
    "graph": ("g", "string", False), "reads": ("f", "string", True), "alignments-out": ("a", "string", False),
    "sampling-step": (None, "long", False), "colinear-split-len": (None, "long", False), "colinear-split-gap": (None, "long", False), "colinear-gap": (None, "long", False),
    "fast-mode": (None, None, False),
    "help": ("h", None, False), "version": (None, None, False), "threads": ("t", "size", False), "verbose": (None, None, False), "short-verbose": (None, None, False),
    "E-cutoff": (None, "double", False), "all-alignments": (None, None, False), "extra-heuristic": (None, None, False), "try-all-seeds": (None, None, False),
    "global-alignment": (None, None, False), "optimal-alignment": (None, None, False), "X-drop": (None, "int", False), "precise-clipping": (None, "double", False),
    "cigar-match-mismatch": (None, None, False), "generate-path": (None, None, False), "generate-path-seed": (None, "long", False), "graph-statistics": (None, None, False),
    "seeds-clustersize": (None, "size", False), "seeds-extend-density": (None, "double", False), "seeds-minimizer-length": (None, "size", False),
    "seeds-minimizer-windowsize": (None, "size", False), "seeds-minimizer-density": (None, "double", False), "seeds-minimizer-ignore-frequent": (None, "double", False),
    "seeds-mum-count": (None, "size", False), "seeds-mem-count": (None, "size", False), "seeds-mxm-length": (None, "size", False), "seeds-mxm-cache-prefix": (None, "string", False),
    "seeds-file": ("s", "string", True), "seedless-DP": (None, None, False), "DP-restart-stride": (None, "size", False),
    "bandwidth": ("b", "size", False), "ramp-bandwidth": ("B", "size", False), "tangle-effort": ("C", "size", False), "high-memory": (None, None, False),
    "schedule-inverse-E-sum": (None, None, False), "schedule-inverse-E-product": (None, None, False), "schedule-score": (None, None, False), "schedule-length": (None, None, False),
    "greedy-length": (None, None, False), "greedy-E": (None, None, False), "greedy-score": (None, None, False), "no-colinear-chaining": (None, None, False),
    # this build's own
    "batch-bytes": (None, "size", False), "device": (None, "size", False), "index-cache": (None, "string", False),
    "inflight": (None, "size", False), "devices": (None, "string", False),
    "corrected-out": (None, "string", False), "corrected-clipped-out": (None, "string", False),   # GraphAligner's: the reference keeps their mechanism and dropped the two option lines
    "coverage-out": (None, "string", False), "base-coverage-out": (None, "string", False),
    "link-coverage-out": (None, "string", False), "coverage-gfa-out": (None, "string", False), "supported-subgraph-out": (None, "string", False),
    "pileup-out": (None, "string", False), "pileup-min-alt": (None, "size", False), "pileup-min-alt-fraction": (None, "double", False),
}
MAX_INFLIGHT = 5                   # the most the benchmark keeps in flight on a device (bench.py: BATCH_MS_BY_INFLIGHT ends there)
MAX_DEVICES = 16                   # the library's per-device slots
COVERAGE_GZ_PIECE = 1 << 20         # a .gz coverage table is written as gzip members of about this many bytes of whole lines
COVERAGE_OUTPUTS = (("coverage", "coverage-out"), ("base_coverage", "base-coverage-out"), ("link_coverage", "link-coverage-out"), ("coverage_gfa", "coverage-gfa-out"),
                    ("supported_subgraph", "supported-subgraph-out"), ("pileup", "pileup-out"))          # Config.coverage key, option
# spelled out in full: the abbreviations of --coverage-out that scripts use (--cov, --coverage) were there first and keep their meaning, and so do --p / --pr (--precise-clipping)
FULL_NAME_ONLY = ("coverage-gfa-out", "pileup-out", "pileup-min-alt", "pileup-min-alt-fraction")
LINK_OUTPUTS = ("link_coverage", "coverage_gfa", "supported_subgraph")     # these need the handles' link table
CORRECTED_SUFFIXES = (".fa", ".fasta", ".fa.gz", ".fasta.gz")   # src/AlignerMain.cpp:360,365 (a name shorter than a suffix does not end in it; the reference's substr would throw)
REFUSED = ("optimal-alignment", "seedless-DP", "DP-restart-stride", "generate-path", "generate-path-seed", "graph-statistics")
SELECT = {"greedy-length": 0, "schedule-inverse-E-sum": 3, "schedule-inverse-E-product": 4, "schedule-score": 5, "schedule-length": 6, "all-alignments": 7}   # GC_SELECT_*

HELP = """Mandatory parameters:
  -g [ --graph ] arg                    input graph (.gfa)
  -f [ --reads ] arg                    input reads (fasta, fastq or unaligned bam; fasta and fastq uncompressed or gzipped)
  -a [ --alignments-out ] arg           output alignment file (.gaf/.gam/.json), may be given several times

Colinear chaining parameters:
  --sampling-step arg                   Sampling step factor, an integer (default 1); sets --colinear-split-gap = ceil(arg * --colinear-split-len)
  --colinear-split-len arg              length of the fragments the read is split into [default 35]
  --colinear-split-gap arg              distance between consecutive fragments [default 35]
  --colinear-gap arg                    split the chain's path where consecutive anchors are further apart [default 10000]
  --fast-mode                           skip the edit distance computation after chaining (output the path instead of an alignment)
  --no-colinear-chaining                align as GraphAligner does, without chaining
  --greedy-length, --schedule-inverse-E-sum, --schedule-inverse-E-product, --schedule-score, --schedule-length
                                        how --no-colinear-chaining selects the alignments it writes (one at most)

General parameters:
  -h [ --help ]                         help message
  --version                             print version
  --E-cutoff arg                        discard alignments with E-value > arg
  --all-alignments                      return all alignments (the chaining default)
  --extra-heuristic                     use heuristics to discard more seed hits
  --try-all-seeds                       overrides --seeds-extend-density to -1 (the chaining default)
  --global-alignment                    force the read to be aligned end-to-end even if the alignment score is poor
  --X-drop arg                          X-drop heuristic to end alignment with score cutoff arg (int)
  --precise-clipping arg                clip the alignment ends with arg as the identity cutoff (float)
  --cigar-match-mismatch                M for matches and mismatches in the cigar string instead of = and X

Seeding parameters:
  --seeds-clustersize arg               discard seed clusters with fewer than arg seeds
  --seeds-extend-density arg            extend up to approximately the best (arg * sequence length) seeds (-1 for all)
  --seeds-minimizer-length arg          k-mer length for minimizer seeding [15]
  --seeds-minimizer-windowsize arg      window size for minimizer seeding [20]
  --seeds-minimizer-density arg         keep approximately (arg * sequence length) least common minimizers (-1 for all) [10]
  --seeds-minimizer-ignore-frequent arg ignore arg most frequent fraction of minimizers [0.001]
  --seeds-mum-count arg                 arg longest maximal unique matches fully contained in a node (-1 for all)
  --seeds-mem-count arg                 arg longest maximal exact matches fully contained in a node (-1 for all)
  --seeds-mxm-length arg                minimum length for maximal unique / exact matches [20]
  --seeds-mxm-cache-prefix arg          store the mum/mem seeding index on disk for reuse, or reuse it if it exists
  -s [ --seeds-file ] arg               external seeds (.gam)

Extension parameters:
  -b [ --bandwidth ] arg                alignment bandwidth [10]
  -B [ --ramp-bandwidth ] arg           ramp bandwidth
  -C [ --tangle-effort ] arg            tangle effort limit (-1 for unlimited)

This build's own:
  --batch-bytes arg                     bytes of read file text per batch [100 MB]
  --device arg                          GPU to run on [0]
  --devices arg                         GPUs to run on, comma-separated (0,1,2,3; at most 16): one copy of graph and index on each, the batches go to
                                        the one with the fewest outstanding. --device N means --devices N. (A device named twice gets two copies:
                                        that is for testing several copies on a one-GPU box.)
  --inflight arg                        batches in flight per GPU, >= 1 [chosen: at most 5, cut by the usable host CPUs and the device's free memory]
  --index-cache arg                     load the graph and minimizer index from this file if it exists, else build them and save them there.
                                        An existing file wins: it is checked for the minimizer length and window only, not against -g or
                                        --seeds-minimizer-ignore-frequent
  --corrected-out arg                   GraphAligner's: output corrected reads file (.fa/.fa.gz), every read with its aligned stretches
                                        replaced by the graph's letters along the alignment (upper case; the rest lower case)
  --corrected-clipped-out arg           GraphAligner's: output corrected clipped reads file (.fa/.fa.gz), one record per alignment
  --coverage-out arg                    table "#segment length bases" (tab-separated; gzipped for a .gz name): for every segment of the graph the
                                        number of its bases under the alignments written, each counted as often as it is covered
  --base-coverage-out arg               table "segment start end depth" (no header; 0-based, half-open, forward strand; gzipped for a .gz name): one
                                        line per stretch of equal non-zero depth. Holds 4 bytes per base of the graph on every device
  --link-coverage-out arg               table "#from from_orient to to_orient traversals" (tab-separated; gzipped for a .gz name): for every link of the
                                        graph how many of the alignments written walk it, on either strand. Holds 16 bytes per link on every device
  --coverage-gfa-out arg                the graph as GFA (gzipped for a .gz name) with coverage tags: RC:i on a segment is its "bases" count of
                                        --coverage-out (divide by LN:i for the mean depth), RC:i on a link its traversals. Letters in upper case.
                                        The option's name is not abbreviated (--cov stays --coverage-out)
  --supported-subgraph-out arg          the same GFA without the segments no alignment covers and the links no alignment walks
  --pileup-out arg                      table "#segment pos ref depth match mmA mmC mmG mmT mmN del ins_before ins_after" (tab-separated; gzipped for a
                                        .gz name): for every base where the alignments written disagree with the graph, how they do. Holds 36 bytes
                                        per base of the graph on every device. The three --pileup options are not abbreviated
  --pileup-min-alt arg (=1)             a base gets a line when its largest count other than match is at least this (0: every covered base)
  --pileup-min-alt-fraction arg (=0)    ... and at least this fraction of the base's depth (0 to 1)

Accepted and without effect: -t [ --threads ] arg (must be >= 1), --high-memory, --verbose, --short-verbose, --greedy-E, --greedy-score.
Not supported by this build: --optimal-alignment, --seedless-DP, --DP-restart-stride, --generate-path, --generate-path-seed,
--graph-statistics, a .vg graph.
"""


class CliExit(Exception):
    """The command line ends here: status and what goes to stderr (and to stdout for --version)."""

    def __init__(self, status, stderr="", stdout=""):
        super().__init__(stderr)
        self.status, self.stderr, self.stdout = status, stderr, stdout


@dataclass
class Config:
    graph: str = ""
    reads: list = field(default_factory=list)
    outputs: dict = field(default_factory=dict)          # "gaf" / "json" / "gam" -> path (the last one given of each kind, as the reference keeps it)
    corrected: dict = field(default_factory=dict)        # "corrected" / "corrected_clipped" -> path (--corrected-out / --corrected-clipped-out; a .gz name is compressed)
    coverage: dict = field(default_factory=dict)         # "coverage" / "base_coverage" / "link_coverage" / "coverage_gfa" / "supported_subgraph" / "pileup" -> path (COVERAGE_OUTPUTS; a .gz name is compressed)
    pileup_min_alt: int = 1                              # --pileup-min-alt / --pileup-min-alt-fraction: which bases of --pileup-out get a line
    pileup_min_fraction: float = 0.0
    aligner: dict = field(default_factory=dict)          # keyword arguments of api.Aligner
    min_cluster_size: int = 1                            # gc_params::min_cluster_size
    seeder: dict = field(default_factory=dict)           # {"kind": "minimizer", "length", "window", "keep_fraction"}, {"kind": "mxm", "mode", "count", "min_len", "cache_prefix"} or {"kind": "file", "paths"}
    cigar_match_mismatch: bool = False
    threads: int = 1
    batch_bytes: int = 100 << 20
    device: int = 0                                      # the first (or only) device
    devices: list = field(default_factory=lambda: [0])   # one replica of graph and index per entry
    inflight: int = 0                                    # batches in flight per replica; 0: chosen (choose_inflight)
    index_cache: str = ""
    warnings: list = field(default_factory=list)         # what the reference prints and goes on


def _convert(name, kind, text):
    bad = CliExit(1, f"the argument ('{text}') for option '--{name}' is invalid\nrun with option -h for help\n")
    if kind == "string":
        return text
    if kind in ("long", "int", "size"):
        if not re.fullmatch(r"[+-]?[0-9]+", text):
            raise bad
        value = int(text)
        if kind == "size":                     # the reference's size_t: a minus sign wraps, as its lexical_cast does
            if abs(value) > UNLIMITED:
                raise bad
            return value % (1 << 64)
        limit = 1 << (63 if kind == "long" else 31)
        if not -limit <= value < limit:
            raise bad
        return value
    if not re.fullmatch(r"[+-]?(([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?|inf(inity)?|nan)", text, flags=re.I):
        raise bad
    return float(text)


def parse(argv):
    """boost::program_options as the reference sets it up: --name arg, --name=arg, -n arg, -narg, unambiguous prefixes of long names; -f and -s take every token up to
    the next option. -> {name: [values]} (a switch: [])."""
    shorts = {short: name for name, (short, _, _) in OPTIONS.items() if short}

    def fail(text):
        raise CliExit(1, text + "\nrun with option -h for help\n")

    seen, i = {}, 0
    while i < len(argv):
        token = argv[i]
        i += 1
        attached = None
        if token.startswith("--") and len(token) > 2:
            key, eq, value = token[2:].partition("=")
            if key not in OPTIONS:
                guesses = [n for n in OPTIONS if n.startswith(key) and n not in FULL_NAME_ONLY]
                if len(guesses) > 1:
                    fail(f"option '--{key}' is ambiguous and matches " + ", ".join(f"'--{g}'" for g in sorted(guesses)))
                if not guesses:
                    fail(f"unrecognised option '--{key}'")
                key = guesses[0]
            name, shown = key, "--" + key
            if eq:
                attached = value
        elif token.startswith("-") and len(token) > 1 and token != "--":
            if token[1] not in shorts:
                fail(f"unrecognised option '{token}'")
            name, shown = shorts[token[1]], "--" + shorts[token[1]]
            if len(token) > 2:
                attached = token[2:]
        else:
            fail("too many positional options have been specified on the command line")
        _, kind, several = OPTIONS[name]
        if kind is None:
            if attached is not None:
                fail(f"option '{shown}' does not take any arguments")
            seen.setdefault(name, [])
            continue
        values = []
        if attached is not None:
            values.append(attached)
        elif i < len(argv):
            values.append(argv[i])
            i += 1
        else:
            fail(f"the required argument for option '{shown}' is missing")
        if several:
            while i < len(argv) and not (argv[i].startswith("-") and len(argv[i]) > 1):
                values.append(argv[i])
                i += 1
        if name in seen and not several and name != "alignments-out":
            fail(f"option '{shown}' cannot be specified more than once")
        seen.setdefault(name, []).extend(_convert(name, kind, v) for v in values)
    return seen


def resolve(argv):
    """Command line -> Config, or CliExit. Neither the library nor a device is touched."""
    vm = parse(list(argv))
    if "help" in vm:
        raise CliExit(0, HELP)
    if "version" in vm:
        raise CliExit(0, "", "Version " + VERSION + "\n")
    for name in REFUSED:
        if name in vm:
            raise CliExit(1, f"--{name} is not supported by this build\nrun with option -h for help\n")
    last = lambda name, default: vm[name][-1] if name in vm else default   # noqa: E731
    graph = last("graph", "")
    if len(graph) >= 3 and graph.endswith(".vg"):
        raise CliExit(1, f"a .vg graph ({graph}) is not supported by this build: give a .gfa\nrun with option -h for help\n")
    chaining = "no-colinear-chaining" not in vm

    cfg = Config()
    errors, messages = [], []          # messages: warnings and errors in the order of the reference's checks, as it prints them

    def warning(text):
        cfg.warnings.append(text)
        messages.append(text)

    def error(text):
        errors.append(text)
        messages.append(text)

    # GraphAligner's vg presets (:186-193), then the chaining defaults (:201-209)
    minimizer_density, minimizer_length, minimizer_window, extend_density, discard_fraction, bandwidth = 10.0, 15, 20, -1.0, 0.001, 10
    selection, try_all = (SELECT["all-alignments"], True) if chaining else (SELECT["greedy-length"], False)
    colinear_gap, split_len, split_gap, sampling_step = 10000, 35, 35, 1

    cfg.graph, cfg.reads = graph, list(vm.get("reads", []))
    outputs = list(vm.get("alignments-out", []))
    cfg.threads = last("threads", 1)
    bandwidth = last("bandwidth", bandwidth)
    extend_density = last("seeds-extend-density", extend_density)
    discard_fraction = last("seeds-minimizer-ignore-frequent", discard_fraction)
    cfg.min_cluster_size = last("seeds-clustersize", 1)
    minimizer_density = last("seeds-minimizer-density", minimizer_density)
    minimizer_length = last("seeds-minimizer-length", minimizer_length)
    minimizer_window = last("seeds-minimizer-windowsize", minimizer_window)
    mxm_length, mem_count, mum_count = last("seeds-mxm-length", 20), last("seeds-mem-count", 0), last("seeds-mum-count", 0)
    cache_prefix = last("seeds-mxm-cache-prefix", "")
    seed_files = list(vm.get("seeds-file", []))
    colinear_gap, split_len, split_gap = last("colinear-gap", colinear_gap), last("colinear-split-len", split_len), last("colinear-split-gap", split_gap)
    sampling_step = last("sampling-step", sampling_step)
    if sampling_step != 1:
        if "colinear-split-gap" in vm:
            warning("WARNING: --sampling-step and --colinear-split-gap are both set! --colinear-split-gap will be ignored, and set to (--sampling-step * --colinear-split-len)")
        split_gap = math.ceil(sampling_step * split_len)
    ramp, max_cells = last("ramp-bandwidth", 0), last("tangle-effort", UNLIMITED)
    if "try-all-seeds" in vm:
        try_all = True
    cfg.cigar_match_mismatch = "cigar-match-mismatch" in vm
    methods = 0
    for name in ("all-alignments", "greedy-length", "schedule-inverse-E-sum", "schedule-inverse-E-product", "schedule-score", "schedule-length"):
        if name in vm:
            selection = SELECT[name]
            methods += 1
            if name == "all-alignments":
                try_all = True
    e_cutoff = last("E-cutoff", -1.0)
    precise, cutoff = False, 0.5
    if "precise-clipping" in vm:
        precise, cutoff = True, vm["precise-clipping"][-1]
        if cutoff < 0.001 or cutoff > 0.999 or cutoff != cutoff:
            error("precise clipping identity cutoff must be between 0.001 and 0.999")
        if 0.001 <= cutoff < 0.501:
            warning("Warning: precise clipping identity cutoff set below 0.501. Output will almost certainly contain spurious alignments.")
    x_drop = 0
    if "X-drop" in vm:
        x_drop = vm["X-drop"][-1]
        if x_drop < 1:
            error("X-drop score cutoff must be > 1")
    if cfg.graph == "":
        error("graph file must be given")
    if not cfg.reads:
        error("read file must be given")
    corrected_out, clipped_out = last("corrected-out", ""), last("corrected-clipped-out", "")
    coverage_outs = [(fmt, last(option, "")) for fmt, option in COVERAGE_OUTPUTS]
    if not outputs and corrected_out == "" and clipped_out == "" and all(path == "" for _, path in coverage_outs):      # src/AlignerMain.cpp:335 (this build's own outputs count as the corrected reads do)
        error("alignments-out must be given")
    for path in outputs:
        if len(path) >= 4 and path.endswith(".gam"):
            cfg.outputs["gam"] = path
        elif len(path) >= 5 and path.endswith(".json"):
            cfg.outputs["json"] = path
        elif len(path) >= 4 and path.endswith(".gaf"):
            cfg.outputs["gaf"] = path
        else:
            error(f"unknown output alignment format ({path}), must be either .gaf, .gam or .json")
    for fmt, path in (("corrected", corrected_out), ("corrected_clipped", clipped_out)):          # src/AlignerMain.cpp:360-369
        if path != "":
            if not path.endswith(CORRECTED_SUFFIXES):
                error("unknown output corrected read format, must be .fa or .fa.gz")
            cfg.corrected[fmt] = path
    for fmt, path in coverage_outs:
        if path != "":
            cfg.coverage[fmt] = path
    cfg.pileup_min_alt, cfg.pileup_min_fraction = last("pileup-min-alt", 1), last("pileup-min-alt-fraction", 0.0)
    if not 0.0 <= cfg.pileup_min_fraction <= 1.0:          # (a NaN fails both comparisons)
        error("pileup minimum alternative fraction (--pileup-min-alt-fraction) must be between 0 and 1")
    if "pileup" not in cfg.coverage and ("pileup-min-alt" in vm or "pileup-min-alt-fraction" in vm):
        error("--pileup-min-alt and --pileup-min-alt-fraction need --pileup-out")
    if cfg.threads < 1:
        error("number of threads must be >= 1")
    if "inflight" in vm and vm["inflight"][-1] < 1:
        error("batches in flight (--inflight) must be >= 1")
    devices = None
    if "devices" in vm:
        text = vm["devices"][-1]
        if "device" in vm:
            error("--device and --devices are both set: give one of them")
        if not re.fullmatch(r"[0-9]+(,[0-9]+)*", text):
            error(f"--devices ({text}) must be a comma-separated list of device indices, as in 0,1,2,3")
        else:
            devices = [int(d) for d in text.split(",")]
            if len(devices) > MAX_DEVICES:
                error(f"--devices names {len(devices)} devices, this build runs on at most {MAX_DEVICES}")
    if bandwidth < 1:
        error("default bandwidth must be >= 1")
    if ramp != 0 and ramp <= bandwidth:
        error("ramp bandwidth must be higher than default bandwidth")
    if mxm_length < 2:
        error("mum/mem minimum length must be >= 2")
    if minimizer_length >= 32:
        error("Maximum minimizer length is 31")
    if discard_fraction < 0 or discard_fraction >= 1:
        error("Minimizer discard fraction must be 0 <= x < 1")
    if minimizer_density < 0 and minimizer_density != -1:
        error("Minimizer density can't be negative")
    if extend_density <= 0 and extend_density != -1:
        error("Seed extension density can't be negative")
    picked = (1 if mum_count != 0 else 0) + (1 if mem_count != 0 else 0) + (1 if minimizer_density != 0 else 0) + (1 if seed_files else 0)   # src/AlignerMain.cpp:407-410
    if picked == 0:
        error("pick a seeding method")
    if picked > 1:
        error("pick only one seeding method")
    if x_drop > 0 and not precise:
        warning("--X-drop is set but --precise-clipping is not, using default value of --precise-clipping .66")
        precise, cutoff = True, 0.66
    if try_all and "seeds-extend-density" in vm and vm["seeds-extend-density"][-1] != -1:
        warning("WARNING: --try-all-seeds and --seeds-extend-density are both set! --seeds-extend-density will be ignored")
        extend_density = -1.0
    if methods > 1:
        error("pick only one method for selecting outputted alignments")
    # what the library's fields can hold (the reference's are size_t and long long)
    for name, value, limit in (("bandwidth", bandwidth, 1 << 31), ("ramp-bandwidth", ramp, 1 << 31), ("colinear-split-len", split_len, 1 << 31), ("colinear-split-gap", split_gap, 1 << 31),
                               ("seeds-clustersize", cfg.min_cluster_size, 1 << 31), ("seeds-mxm-length", mxm_length, 1 << 32), ("seeds-minimizer-windowsize", minimizer_window, 1 << 31),
                               ("device", last("device", 0), 1 << 31), ("devices", max(devices or [0]), 1 << 31), ("inflight", last("inflight", 1), 1 << 31), ("tangle-effort", 0 if max_cells == UNLIMITED else max_cells, 1 << 63)):
        if not -limit <= value < limit:
            error(f"--{name} {value} is beyond what this build can hold")
    if errors:
        raise CliExit(1, "".join(line + "\n" for line in messages) + "run with option -h for help\n")

    if seed_files:
        cfg.seeder = {"kind": "file", "paths": seed_files}
    elif minimizer_density != 0:
        cfg.seeder = {"kind": "minimizer", "length": minimizer_length, "window": minimizer_window, "keep_fraction": 1 - discard_fraction}   # src/Aligner.cpp:1162
    else:
        count = mum_count if mum_count != 0 else mem_count
        cfg.seeder = {"kind": "mxm", "mode": "mum" if mum_count != 0 else "mem", "count": -1 if count == UNLIMITED else count, "min_len": mxm_length, "cache_prefix": cache_prefix}
    cfg.aligner = dict(
        bandwidth=bandwidth, ramp_bandwidth=ramp, max_cells_per_slice=-1 if max_cells == UNLIMITED else max_cells,
        split_len=split_len, split_gap=split_gap, colinear_gap=colinear_gap, seed_density=float(minimizer_density),
        e_cutoff=float(e_cutoff), force_global="global-alignment" in vm, seed_extend_density=float(extend_density), extra_heuristic="extra-heuristic" in vm,
        colinear_chaining=chaining, selection_method=selection, fast_mode="fast-mode" in vm,
        precise_clipping=float(cutoff) if precise else 0.0, x_drop=x_drop)
    cfg.batch_bytes = max(1, last("batch-bytes", 100 << 20))
    cfg.devices = devices if devices is not None else [last("device", 0)]
    cfg.device = cfg.devices[0]
    cfg.inflight = last("inflight", 0)
    cfg.index_cache = last("index-cache", "")
    return cfg


class _Outputs:
    """Every output file is written under a temporary name beside it and renamed when the run is complete; a run that fails leaves no file."""

    def __init__(self, paths):
        self.paths, self.files = dict(paths), {}

    def __enter__(self):
        try:
            for fmt, path in self.paths.items():
                self.files[fmt] = open(f"{path}.tmp{os.getpid()}", "wb")
        except BaseException as e:         # (a later file could not be opened: the earlier ones are closed and removed)
            self.__exit__(type(e), e, None)
            raise
        return self

    def write(self, fmt, data):
        self.files[fmt].write(data)

    def __exit__(self, kind, value, trace):
        for fmt, f in self.files.items():
            f.close()
            if kind is None:
                os.replace(f.name, self.paths[fmt])
            elif os.path.exists(f.name):
                os.unlink(f.name)
        return False


# Device memory a batch in flight is counted with ("Sizing"): the largest of its figures per read base - 190 bytes for 10 kb reads on graphs up to a
# few hundred Mbp, 280 for 50 kb reads, 420 at 960 Mbp - and the larger of its two whole-read scratch sizes per device (21 - 27 GB). Both err towards fewer batches
# in flight; what they still miss, the pipeline's out-of-memory retirement catches.
BATCH_BYTES_PER_READ_BASE = 420
LONG_SCRATCH_BYTES = 27 * 10 ** 9
# at least: a FASTQ record holds a quality letter per base, so a batch of B bytes of text holds at most B / 2 bases; a BAM record holds half a byte and a quality byte
# per base, so B inflated bytes hold at most B * 2 / 3
FILE_BYTES_PER_READ_BASE = {"fasta": 1, "fastq": 2, "bam": 1.5}


def usable_cpus():
    """CPUs this process can really use: the affinity mask, cut to the cgroup's CPU bandwidth quota when there is one (as bench.py reads it)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0 and period > 0:
                n = min(n, max(1, int(quota / period + 0.5)))
        except (OSError, ValueError):
            pass
    return max(1, n)


def choose_inflight(cpus, free_bytes, batch_bytes, fmt, replicas=1):
    """Batches in flight per replica when --inflight is not given; a pure function. At most MAX_INFLIGHT; one worker thread per usable CPU after one CPU for the reader
    and one for the writer are set aside, shared among the replicas; and as many batches as fit free_bytes - the device's free memory after set-up (a replica's share of
    it where several are on one device) - beside the whole-read scratch, a batch counted as batch_bytes of `fmt` text at BATCH_BYTES_PER_READ_BASE per base. Never below 1."""
    by_cpu = (int(cpus) - 2) // max(1, int(replicas))
    bases = max(1, int(batch_bytes) * 2 // 3 if fmt == "bam" else int(batch_bytes) // FILE_BYTES_PER_READ_BASE[fmt])
    by_memory = (int(free_bytes) - LONG_SCRATCH_BYTES) // (bases * BATCH_BYTES_PER_READ_BASE)
    return max(1, min(MAX_INFLIGHT, by_cpu, by_memory))


class _Replica:
    """One device's copy of what the workers read: graph, and minimizer index, MUM/MEM index or seed store."""

    def __init__(self, device):
        self.device, self.graph, self.seeder, self.index, self.store, self.coverage, self.setup_seconds = device, None, None, None, None, None, 0.0

    def close(self):
        for thing in (self.coverage, self.store, self.index, self.seeder, self.graph):
            if thing is not None:
                thing.close()
        self.coverage = self.store = self.index = self.seeder = self.graph = None


def _setup_replicas(cfg, api, replicas):
    """Graph and index of every replica, one after the other, as the single device has been set up. With several replicas and no --index-cache (no
    --seeds-mxm-cache-prefix) the first one's build is saved to a temporary file the others load, so the host build runs once."""
    import shutil
    import tempfile
    kind = cfg.seeder["kind"]
    minimizer = kind == "minimizer"
    tmp = tempfile.mkdtemp(prefix="graphchainer_amd.") if len(replicas) > 1 and (not cfg.index_cache or (kind == "mxm" and not cfg.seeder["cache_prefix"])) else None
    try:
        index_cache = cfg.index_cache or (os.path.join(tmp, "index.gcidx") if tmp else "")
        mxm_prefix = (cfg.seeder["cache_prefix"] or (os.path.join(tmp, "mxm") if tmp else None)) if kind == "mxm" else None
        for rep in replicas:
            started = time.time()
            api.set_device(rep.device)
            if index_cache and os.path.exists(index_cache):
                info = api.check_index_cache(index_cache)
                if minimizer and (not info["has_seeder"] or (info["k"], info["w"]) != (cfg.seeder["length"], cfg.seeder["window"])):
                    raise RuntimeError(f"{index_cache} holds no minimizer index of length {cfg.seeder['length']} and window {cfg.seeder['window']}")
                rep.graph, cached = api.load_index_cache(index_cache)
                if minimizer:
                    rep.seeder = cached
                elif cached is not None:
                    cached.close()
            else:
                rep.graph = api.AlignmentGraph(cfg.graph)
                if minimizer:
                    rep.seeder = api.MinimizerSeeder(rep.graph, cfg.seeder["length"], cfg.seeder["window"], cfg.seeder["keep_fraction"])
                if index_cache:
                    api.save_index_cache(rep.graph, rep.seeder, index_cache)
            if kind == "file":
                rep.store = api.SeedStore(cfg.seeder["paths"])             # every file, in command-line order, before any read is aligned (src/Aligner.cpp:1169-1190)
            elif not minimizer:
                rep.index = api.MxmIndex(rep.graph, cache_prefix=mxm_prefix)
            if cfg.coverage:               # the accumulators of this device, here so that choose_inflight measures the free memory with them in place
                rep.coverage = api.Coverage(rep.graph, per_base="base_coverage" in cfg.coverage, links=any(f in cfg.coverage for f in LINK_OUTPUTS), pileup="pileup" in cfg.coverage)
            rep.setup_seconds = time.time() - started
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


def device_output_for(cfg):
    """gc_params::device_output for the files cfg names: 1 / 2 the GAF pieces, 4 the vg::Path bytes, 8 the corrected reads' pieces. Coverage alone asks for the GAF pieces
    (the bit with the least to bring down) and leaves them unused: the output jobs the counting works from exist only with some bit set."""
    gaf = (2 if cfg.cigar_match_mismatch else 1) if "gaf" in cfg.outputs else 0
    bits = gaf | (4 if "json" in cfg.outputs or "gam" in cfg.outputs else 0) | (8 if cfg.corrected else 0)
    return bits or (1 if cfg.coverage else 0)


def gzip_lines(api, text, line_off, piece=COVERAGE_GZ_PIECE):
    """text as gzip members of whole lines, about `piece` bytes each, deflated on the device (gc_gzip_streams_lz); line_off: the byte offsets of the lines, the end included."""
    cuts, total = [0], len(text)
    for at in line_off[1:]:
        if int(at) - cuts[-1] >= piece:
            cuts.append(int(at))
    if cuts[-1] != total:
        cuts.append(total)
    return b"".join(api.gzip_streams([text[cuts[k]:cuts[k + 1]] for k in range(len(cuts) - 1)], lz=True))


def gzip_records(api, text, rec_off):
    """The records text[rec_off[k]:rec_off[k + 1]] as one gzip member each, deflated on the device (gc_gzip_streams_lz)."""
    return b"".join(api.gzip_streams([text[int(rec_off[k]):int(rec_off[k + 1])] for k in range(len(rec_off) - 1)], lz=True))


def run(cfg, stderr=sys.stderr):
    """Aligns cfg.reads to cfg.graph and writes cfg.outputs. Returns the counts it reports. Threads (pipeline.py): one reads the files and inflates a .gz, one cuts and
    parses (and chooses the replica of each batch before it parses it, so that the reads live on the device that aligns them), up to `inflight` workers per replica seed
    and align with an Aligner each, one writes the batches' bytes in input order."""
    import numpy as np

    from . import api, pipeline
    from_file = cfg.seeder["kind"] == "file"
    if from_file and not all(os.path.exists(p) for p in cfg.seeder["paths"]):
        raise CliExit(0, "No seeds file exists\n")            # src/Aligner.cpp:1185-1186: said, and the run ends with status 0 and no output
    devices = list(cfg.devices) if cfg.devices else [cfg.device]
    replicas = [_Replica(d) for d in devices]
    # what the chosen writers need: the whole-read pass and the two edit distances that pick the winner, and the final alignments encoded on the device, where their traces
    # are - the GAF pieces (= / X items, or M items with --cigar-match-mismatch) for a .gaf, the vg::Path bytes for a .json or .gam; no trace comes down (keep_traces=0)
    formats = tuple(f for f in ("gaf", "json", "gam") if f in cfg.outputs)
    corrected = tuple(f for f in ("corrected", "corrected_clipped") if f in cfg.corrected)       # the corrected reads' pieces are spelled on the device too (bit 8), also with no -a at all
    device_output = device_output_for(cfg)
    counts = {"reads": 0, "flagged": 0, "failed_assertion": 0, "capacity_exceeded": 0, "batches": 0, "seconds": 0.0, "bgzf_blocks": 0, "bam_skipped": 0}   # seconds: reading, aligning and writing, setup left out

    def make_aligner(r):
        rep = replicas[r]
        api.set_device(rep.device)         # the current device belongs to the thread: every call of this worker runs under it
        aligner = api.Aligner(rep.graph, rep.seeder, long_pass=True, edit_distances=True, keep_traces=0, device_output=device_output, **cfg.aligner)
        aligner.params.min_cluster_size = cfg.min_cluster_size
        if rep.coverage is not None:       # every worker of the replica counts into the replica's handle: a batch is counted by the worker that finishes it
            aligner.set_coverage(rep.coverage)
        return aligner

    def align(aligner, r, item):
        rep, (batch, ids) = replicas[r], item
        if rep.store is not None:
            seeds = rep.store.seeds(rep.graph, batch, ids)
        else:
            seeds = rep.index.seeds(batch, cfg.seeder["mode"], count=cfg.seeder["count"], min_len=cfg.seeder["min_len"]) if rep.index is not None else None
        try:
            if rep.coverage is None:
                out = aligner.align_batch(batch, seeds=seeds, gaf_names=ids, formats=formats + corrected, cigar_match_mismatch_merge=cfg.cigar_match_mismatch)
            else:
                # the batch is counted when align_batch returns. What follows must not send it to another worker (pipeline.py retires a worker whose error says
                # "out of memory" and hands its item on): it would be counted twice, so such an error ends the run instead
                out = aligner.align_batch(batch, seeds=seeds)
                try:
                    out.update(aligner.format_batch(out, batch, ids, formats + corrected, cfg.cigar_match_mismatch)[0])
                except RuntimeError as e:
                    raise RuntimeError("formatting a batch that was already counted into the coverage failed: " + str(e).replace(pipeline.OUT_OF_MEMORY, "out of device memory")) from e
        finally:
            if seeds is not None:
                seeds.close()
        failed, capacity = np.asarray(out["failed_assertion"]) != 0, np.asarray(out["capacity_exceeded"]) != 0
        texts = {f: out[f] for f in formats}
        for f in corrected:                # a .gz name: one gzip member per record, as zstr::ostream per call gives (src/Aligner.cpp:316-336), deflated on the device
            texts[f] = gzip_records(api, out[f], out[f + "_rec_off"]) if cfg.corrected[f].endswith(".gz") else out[f]
        return texts, len(ids), int(failed.sum()), int(capacity.sum()), int((failed | capacity).sum())

    try:
        _setup_replicas(cfg, api, replicas)
        inflight = cfg.inflight
        if not inflight:
            kinds = {api.fastx_file_format(p)[0] for p in cfg.reads} - {None}
            densest = min(kinds, key=FILE_BYTES_PER_READ_BASE.get) if kinds else "fastq"          # the format with the fewest bytes per base: the most bases in a batch
            chosen = []
            for rep in replicas:           # the same count for every replica: the smallest any of them can hold
                api.set_device(rep.device)
                free, _ = api.device_memory()
                chosen.append(choose_inflight(usable_cpus(), free // devices.count(rep.device), cfg.batch_bytes, densest, len(replicas)))
            inflight = min(chosen)
        reader_seconds = {}

        def source(choose):
            def place():
                api.set_device(replicas[choose()].device)
            with pipeline.Prefetch(api.file_pieces(cfg.reads, cfg.batch_bytes, bgzf="device"), name="pipeline-reader") as pieces:
                try:
                    yield from api.parse_pieces(pieces, before_parse=place, counts=counts)
                finally:
                    reader_seconds.update(busy=pieces.busy, waiting_in=0.0, waiting_out=pieces.waiting_out, parse_waiting_in=pieces.consumer_waiting)

        started = time.time()
        with _Outputs({**cfg.outputs, **cfg.corrected, **cfg.coverage}) as outputs:
            def write(result):
                texts, reads, failed, capacity, flagged = result
                for f in formats + corrected:
                    outputs.write(f, texts[f])
                counts["reads"] += reads
                counts["batches"] += 1
                counts["failed_assertion"] += failed
                counts["capacity_exceeded"] += capacity
                counts["flagged"] += flagged

            report = pipeline.run(source, make_aligner, align, write, replicas=len(replicas), inflight=inflight, release=lambda item: item[0].close())
            if cfg.coverage:               # every batch is in: the replicas' counts into the first one's, the tables spelled on its device
                total = replicas[0].coverage
                api.set_device(replicas[0].device)
                for rep in replicas[1:]:
                    total.merge(rep.coverage)
                for fmt, table in (("coverage", total.segment_table), ("base_coverage", total.base_table)):
                    if fmt in cfg.coverage:
                        text, line_off = table(line_offsets=True)
                        outputs.write(fmt, gzip_lines(api, text, line_off) if cfg.coverage[fmt].endswith(".gz") else text)
                for fmt, pieces in (("link_coverage", total.link_pieces), ("coverage_gfa", total.gfa_pieces), ("supported_subgraph", lambda: total.gfa_pieces(supported_only=True))):
                    if fmt in cfg.coverage:    # piece by piece: the text of a large graph is never whole on either side
                        for text, line_off in pieces():
                            outputs.write(fmt, gzip_lines(api, text, line_off) if cfg.coverage[fmt].endswith(".gz") else text)
                if "pileup" in cfg.coverage:
                    for text, line_off in total.pileup_pieces(cfg.pileup_min_alt, cfg.pileup_min_fraction):
                        if len(text):
                            outputs.write("pileup", gzip_lines(api, text, line_off) if cfg.coverage["pileup"].endswith(".gz") else text)
        counts["seconds"] = time.time() - started
    finally:
        for rep in replicas:
            rep.close()
    stages = report["stage_seconds"]
    waited = reader_seconds.pop("parse_waiting_in", 0.0)
    parse = stages["source"]
    counts.update(inflight=inflight, devices=devices, batches_per_replica=report["items_per_replica"], retired_workers=report["retired_workers"],
                  setup_seconds=[round(rep.setup_seconds, 3) for rep in replicas],
                  stage_seconds={"read": {k: round(v, 6) for k, v in reader_seconds.items()},
                                 "parse": {"busy": round(max(0.0, parse["busy"] - waited), 6), "waiting_in": round(waited, 6), "waiting_out": parse["waiting_out"]},
                                 "align": stages["work"], "write": stages["sink"]})
    if counts["bam_skipped"]:
        print(f"{counts['bam_skipped']} BAM records were left out (secondary or supplementary: flag 0x100 or 0x800)", file=stderr)
    if counts["flagged"]:
        print(f"{counts['flagged']} of {counts['reads']} reads were flagged and have no alignment written: {counts['failed_assertion']} failed an assertion "
              f"(a letter outside the nucleotide alphabet among them), {counts['capacity_exceeded']} exceeded a capacity", file=stderr)
    return counts


def main(argv=None):
    try:
        cfg = resolve(sys.argv[1:] if argv is None else argv)
    except CliExit as e:
        sys.stdout.write(e.stdout)
        sys.stderr.write(e.stderr)
        return e.status
    for line in cfg.warnings:
        print(line, file=sys.stderr)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # before the library is loaded: a batch in flight uses a dozen streams, and several share a device
    import zlib
    try:
        run(cfg)
    except CliExit as e:
        sys.stderr.write(e.stderr)
        return e.status
    except zlib.error as e:
        print(f"a gzipped read file could not be inflated: {e}", file=sys.stderr)
        return 1
    except (RuntimeError, OSError, EOFError) as e:
        print(f"{e}", file=sys.stderr)
        return 1
    return 0

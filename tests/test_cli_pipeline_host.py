"""--inflight and --devices without a GPU: what cli.resolve makes of them, their error lines, the help text, and the chooser of the batches in flight against
hand-computed cases."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graphchainer_amd import cli          # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa", "-a", "o.gaf"]


def test_resolve_takes_inflight_and_devices():
    cfg = cli.resolve(BASE + ["--inflight", "3", "--devices", "0,0,1"])
    assert cfg.inflight == 3 and cfg.devices == [0, 0, 1] and cfg.device == 0 and isinstance(cfg.device, int)
    cfg = cli.resolve(BASE)
    assert cfg.inflight == 0 and cfg.devices == [0] and cfg.device == 0
    cfg = cli.resolve(BASE + ["--device", "2"])
    assert cfg.device == 2 and isinstance(cfg.device, int) and cfg.devices == [2] and cfg.inflight == 0
    cfg = cli.resolve(BASE + ["--devices=3", "--inflight=1"])
    assert cfg.devices == [3] and cfg.device == 3 and cfg.inflight == 1
    cfg = cli.resolve(BASE + ["--devices", ",".join(str(d) for d in range(16))])
    assert cfg.devices == list(range(16))


ERRORS = [
    (["--inflight", "0"], "batches in flight (--inflight) must be >= 1"),
    (["--devices", "0,,1"], "--devices (0,,1) must be a comma-separated list of device indices, as in 0,1,2,3"),
    (["--devices", "0,a"], "--devices (0,a) must be a comma-separated list of device indices, as in 0,1,2,3"),
    (["--devices", "1,"], "--devices (1,) must be a comma-separated list of device indices, as in 0,1,2,3"),
    (["--devices", ",".join(["0"] * 17)], "--devices names 17 devices, this build runs on at most 16"),
    (["--device", "1", "--devices", "0,1"], "--device and --devices are both set: give one of them"),
]


@pytest.mark.parametrize("args, line", ERRORS, ids=[" ".join(e[0])[:40] for e in ERRORS])
def test_errors_in_resolves_usual_form(args, line):
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + args)
    assert e.value.status == 1
    assert e.value.stderr == line + "\nrun with option -h for help\n"
    assert cli.main(BASE + args) == 1


def test_help_lists_both_options_under_this_builds_own():
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(["-h"])
    text = e.value.stderr
    own, without_effect = text.index("This build's own:"), text.index("Accepted and without effect")
    for option in ("--inflight arg", "--devices arg", "--device arg"):
        assert own < text.index("  " + option) < without_effect
    assert "-t [ --threads ] arg (must be >= 1)" in text[without_effect:]


def test_the_prefixes_that_became_ambiguous():
    for prefix in ("--devi", "--in"):
        with pytest.raises(cli.CliExit) as e:
            cli.resolve(BASE + [prefix, "1"])
        assert e.value.status == 1 and "is ambiguous" in e.value.stderr
    assert cli.resolve(BASE + ["--inf", "2"]).inflight == 2 and cli.resolve(BASE + ["--ind", "x"]).index_cache == "x"


GB = 10 ** 9
# (cpus, free bytes, batch bytes, format, replicas) -> batches in flight. A batch of B bytes of text counts B bases as FASTA and B / 2 as FASTQ, 420 bytes of device
# memory each; the device's whole-read scratch counts 27 GB; one CPU each goes to the reader and the writer.
CHOICES = [
    ((16, 280 * GB, 100 << 20, "fastq", 1), 5),     # room for (280 - 27) / 22.0 = 11 and 14 CPUs: the cap of 5
    ((16, 280 * GB, 100 << 20, "fasta", 1), 5),     # 253 / 44.04 = 5.7
    ((16, 200 * GB, 100 << 20, "fasta", 1), 3),     # 173 / 44.04 = 3.9
    ((16, 72 * GB, 100 << 20, "fasta", 1), 1),      # 45 / 44.04 = 1.02: one fits
    ((16, 71 * GB, 100 << 20, "fasta", 1), 1),      # 44 / 44.04 < 1: still one, the least there is
    ((16, 20 * GB, 100 << 20, "fastq", 1), 1),      # less than the scratch alone
    ((4, 280 * GB, 100 << 20, "fastq", 1), 2),      # CPU-bound: 4 - reader - writer
    ((3, 280 * GB, 100 << 20, "fastq", 1), 1),
    ((1, 280 * GB, 100 << 20, "fastq", 1), 1),      # never below one
    ((16, 280 * GB, 3000, "fasta", 1), 5),          # tiny batches: the cap
    ((16, 280 * GB, 100 << 20, "fastq", 4), 3),     # 14 CPUs over four replicas
    ((8, 140 * GB, 100 << 20, "fastq", 2), 3),      # 6 CPUs over two replicas; memory: 113 / 22.0 = 5
    ((64, 115 * GB, 100 << 20, "fastq", 1), 3),     # 88 / 22.02 = 3.996
    ((64, 116 * GB, 100 << 20, "fastq", 1), 4),     # 89 / 22.02 = 4.04
]


@pytest.mark.parametrize("arguments, expected", CHOICES)
def test_choose_inflight_is_a_pure_function_of_its_arguments(arguments, expected):
    assert cli.choose_inflight(*arguments) == expected
    assert cli.choose_inflight(*arguments) == expected
    assert 1 <= expected <= cli.MAX_INFLIGHT == 5


def test_usable_cpus_is_cut_by_the_affinity_mask():
    n = cli.usable_cpus()
    assert 1 <= n <= (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count())

"""--corrected-out and --corrected-clipped-out on the command line (cli.resolve; no device): GraphAligner's two options, checked as the reference still checks their
file names (src/AlignerMain.cpp:335,360-369)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphchainer_amd import cli   # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa"]
BAD_FORMAT = "unknown output corrected read format, must be .fa or .fa.gz"


@pytest.mark.parametrize("suffix", [".fa", ".fasta", ".fa.gz", ".fasta.gz"])
def test_each_option_alone_together_and_without_alignments_out(suffix):
    cfg = cli.resolve(BASE + ["--corrected-out", "c" + suffix])
    assert cfg.corrected == {"corrected": "c" + suffix} and cfg.outputs == {}
    cfg = cli.resolve(BASE + ["--corrected-clipped-out", "cc" + suffix])
    assert cfg.corrected == {"corrected_clipped": "cc" + suffix} and cfg.outputs == {}
    cfg = cli.resolve(BASE + ["-a", "o.gaf", "--corrected-out", "c" + suffix, "--corrected-clipped-out", "cc" + suffix])
    assert cfg.corrected == {"corrected": "c" + suffix, "corrected_clipped": "cc" + suffix} and cfg.outputs == {"gaf": "o.gaf"}


@pytest.mark.parametrize("name", ["c.fq", "c.fa.bz2", "c.fasta.gzip", "c.gz", "fa", "c.FA", "c.fa.gz.tmp", "a"])
@pytest.mark.parametrize("option", ["--corrected-out", "--corrected-clipped-out"])
def test_each_bad_suffix_is_refused_with_the_reference_s_line(option, name):
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-a", "o.gaf", option, name])
    assert e.value.status == 1
    assert e.value.stderr.splitlines() == [BAD_FORMAT, "run with option -h for help"]


def test_both_bad_give_the_line_twice_in_the_reference_s_order_among_the_checks():
    """:340-359 the alignment files, :360-369 the two corrected files, :370 the thread count."""
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-a", "o.sam", "--corrected-out", "c.txt", "--corrected-clipped-out", "cc.txt", "-t", "0"])
    assert e.value.stderr.splitlines() == ["unknown output alignment format (o.sam), must be either .gaf, .gam or .json", BAD_FORMAT, BAD_FORMAT,
                                           "number of threads must be >= 1", "run with option -h for help"]


def test_alignments_out_must_be_given_only_when_no_output_at_all_is_named():
    with pytest.raises(cli.CliExit) as e:
        cli.resolve([])
    assert e.value.stderr.splitlines()[:3] == ["graph file must be given", "read file must be given", "alignments-out must be given"]
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE)
    assert e.value.stderr.splitlines() == ["alignments-out must be given", "run with option -h for help"]
    with pytest.raises(cli.CliExit) as e:                                   # a corrected file, even a badly named one, stands in for -a (:335 looks at the name only)
        cli.resolve(BASE + ["--corrected-out", "c.txt"])
    assert e.value.stderr.splitlines() == [BAD_FORMAT, "run with option -h for help"]


def test_help_lists_both_options_as_graphaligner_s():
    own = cli.HELP.split("This build's own:")[1].split("Accepted and without effect")[0]
    for name in ("--corrected-out arg", "--corrected-clipped-out arg"):
        line = [l for l in own.splitlines() if name in l]
        assert len(line) == 1 and "GraphAligner's" in line[0]
    assert "corrected-out" not in cli.REFUSED and "corrected-clipped-out" not in cli.REFUSED
    assert cli.OPTIONS["corrected-out"] == (None, "string", False) and cli.OPTIONS["corrected-clipped-out"] == (None, "string", False)


def test_bit_8_of_device_output_only_when_asked():
    f = cli.device_output_for
    assert f(cli.resolve(BASE + ["-a", "o.gaf"])) == 1
    assert f(cli.resolve(BASE + ["-a", "o.gaf", "--cigar-match-mismatch"])) == 2
    assert f(cli.resolve(BASE + ["-a", "o.gaf", "-a", "o.gam"])) == 1 | 4
    assert f(cli.resolve(BASE + ["-a", "o.gaf", "--corrected-out", "c.fa"])) == 1 | 8
    assert f(cli.resolve(BASE + ["-a", "o.json", "--corrected-clipped-out", "c.fa.gz"])) == 4 | 8
    assert f(cli.resolve(BASE + ["--corrected-out", "c.fa", "--corrected-clipped-out", "cc.fa"])) == 8
    with pytest.raises(cli.CliExit) as e:                                   # an option given twice is refused as for every single-valued option
        cli.resolve(BASE + ["--corrected-out", "a.fa", "--corrected-out", "b.fa"])
    assert "cannot be specified more than once" in e.value.stderr


def test_the_library_declares_and_exports_the_three_entry_points():
    from graphchainer_amd.api import EXPORTED_SYMBOLS, GcParams, GcResult
    import ctypes
    assert {"gc_format_corrected", "gc_format_corrected_trace", "gc_corrected_pieces"} <= set(EXPORTED_SYMBOLS)
    assert ctypes.sizeof(GcParams) == 216                                   # bit 8 lives in device_output: the struct did not grow
    names = [n for n, _ in GcResult._fields_]
    assert names[-3:] == ["device_output", "out_corrected_off", "out_corrected_text"]   # appended behind the last field of the layout before

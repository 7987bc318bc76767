"""--coverage-out and --base-coverage-out on the command line (cli.resolve, cli.device_output_for, cli.gzip_lines' cutting; no device): this build's own two options."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphchainer_amd import cli   # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa"]


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_each_option_alone_together_and_without_alignments_out(suffix):
    cfg = cli.resolve(BASE + ["--coverage-out", "c.tsv" + suffix])
    assert cfg.coverage == {"coverage": "c.tsv" + suffix} and cfg.outputs == {} and cfg.corrected == {}
    cfg = cli.resolve(BASE + ["--base-coverage-out", "b.bg" + suffix])
    assert cfg.coverage == {"base_coverage": "b.bg" + suffix} and cfg.outputs == {}
    cfg = cli.resolve(BASE + ["-a", "o.gaf", "--coverage-out=c.tsv" + suffix, "--base-coverage-out", "b.bg" + suffix])
    assert cfg.coverage == {"coverage": "c.tsv" + suffix, "base_coverage": "b.bg" + suffix} and cfg.outputs == {"gaf": "o.gaf"}
    assert cli.resolve(BASE + ["-a", "o.gaf"]).coverage == {}


def test_alignments_out_must_be_given_only_when_no_output_at_all_is_named():
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE)
    assert e.value.status == 1 and e.value.stderr.splitlines() == ["alignments-out must be given", "run with option -h for help"]
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(["--coverage-out", "c.tsv"])
    assert e.value.stderr.splitlines() == ["graph file must be given", "read file must be given", "run with option -h for help"]
    with pytest.raises(cli.CliExit) as e:                                   # an option given twice is refused as for every single-valued option
        cli.resolve(BASE + ["--coverage-out", "a.tsv", "--coverage-out", "b.tsv"])
    assert "cannot be specified more than once" in e.value.stderr
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--base-coverage-out"])
    assert "the required argument for option '--base-coverage-out' is missing" in e.value.stderr


def test_device_output_is_never_zero_when_coverage_is_asked_for():
    f = cli.device_output_for
    assert f(cli.resolve(BASE + ["--coverage-out", "c.tsv"])) == 1                      # the GAF pieces, unused: the output jobs exist only with some bit set
    assert f(cli.resolve(BASE + ["--base-coverage-out", "b.bg", "--cigar-match-mismatch"])) == 1
    assert f(cli.resolve(BASE + ["-a", "o.gaf", "--cigar-match-mismatch", "--coverage-out", "c.tsv"])) == 2
    assert f(cli.resolve(BASE + ["-a", "o.gam", "--coverage-out", "c.tsv"])) == 4
    assert f(cli.resolve(BASE + ["--corrected-out", "c.fa", "--base-coverage-out", "b.bg"])) == 8
    assert f(cli.resolve(BASE + ["-a", "o.gaf", "-a", "o.json", "--corrected-out", "c.fa", "--coverage-out", "c.tsv"])) == 1 | 4 | 8
    assert f(cli.resolve(BASE + ["-a", "o.gaf"])) == 1 and f(cli.resolve(BASE + ["--corrected-out", "c.fa"])) == 8      # as before


def test_help_options_and_what_stays_refused():
    own = cli.HELP.split("This build's own:")[1].split("Accepted and without effect")[0]
    for name in ("--coverage-out arg", "--base-coverage-out arg"):
        assert len([line for line in own.splitlines() if name in line]) == 1
    assert cli.OPTIONS["coverage-out"] == (None, "string", False) and cli.OPTIONS["base-coverage-out"] == (None, "string", False)
    assert cli.REFUSED == ("optimal-alignment", "seedless-DP", "DP-restart-stride", "generate-path", "generate-path-seed", "graph-statistics")
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--coverage-out", "c.tsv", "--graph-statistics"])
    assert e.value.stderr.splitlines()[0] == "--graph-statistics is not supported by this build"


def test_the_prefixes_in_use_still_name_one_option():
    cfg = cli.resolve(BASE + ["-a", "o.gaf", "--colinear-ga", "77", "--inf", "2"])
    assert cfg.aligner["colinear_gap"] == 77 and cfg.inflight == 2
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-a", "o.gaf", "--devi", "0"])
    assert e.value.stderr.splitlines()[0] == "option '--devi' is ambiguous and matches '--device', '--devices'"
    assert cli.resolve(BASE + ["--cov", "c.tsv", "--base", "b.bg"]).coverage == {"coverage": "c.tsv", "base_coverage": "b.bg"}
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-a", "o.gaf", "--in", "2"])
    assert "ambiguous" in e.value.stderr and "coverage" not in e.value.stderr
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--co", "c.tsv"])
    assert "ambiguous" in e.value.stderr and "'--coverage-out'" in e.value.stderr


class _Deflate:
    """Stands in for the api module: records the pieces handed to the device deflate."""

    def __init__(self):
        self.pieces = None

    def gzip_streams(self, streams, lz=False):
        assert lz
        self.pieces = list(streams)
        return [b"<" + s + b">" for s in streams]


def test_gz_pieces_are_whole_lines():
    lines = [b"seg%d\t%d\t%d\t%d\n" % (i, i, i + 7, 1 + i % 3) for i in range(200)]
    text = b"".join(lines)
    off = np.concatenate([[0], np.cumsum([len(line) for line in lines])]).astype(np.uint64)
    fake = _Deflate()
    out = cli.gzip_lines(fake, text, off, piece=100)
    assert b"".join(fake.pieces) == text and out == b"".join(b"<" + p + b">" for p in fake.pieces)
    assert len(fake.pieces) > 10 and all(p.endswith(b"\n") and 100 <= len(p) < 100 + max(map(len, lines)) for p in fake.pieces[:-1])
    assert cli.gzip_lines(fake, text, off) == b"<" + text + b">"                        # one piece below the piece size
    assert cli.gzip_lines(fake, b"", np.zeros(1, dtype=np.uint64)) == b"" and fake.pieces == []


def test_the_library_declares_the_entry_points_and_no_struct_grew():
    from graphchainer_amd.api import EXPORTED_SYMBOLS, Coverage, GcParams, GcParamsExt, GcResult
    assert {"gc_coverage_create", "gc_coverage_destroy", "gc_stream_set_coverage", "gc_coverage_add_traces", "gc_coverage_counts", "gc_coverage_merge",
            "gc_coverage_format_segments", "gc_coverage_format_bases"} <= set(EXPORTED_SYMBOLS)
    assert ctypes.sizeof(GcParams) == 216 and ctypes.sizeof(GcParamsExt) == 16
    assert [n for n, _ in GcResult._fields_][-3:] == ["device_output", "out_corrected_off", "out_corrected_text"]
    for method in ("add_traces", "counts", "merge", "segment_table", "base_table", "close"):
        assert callable(getattr(Coverage, method))

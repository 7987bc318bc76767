"""--link-coverage-out, --coverage-gfa-out and --supported-subgraph-out on the command line (cli.resolve, cli.device_output_for; no device), the library's new entry
points, and the link numbering of a handle against the model (that one needs a device for the graph and skips without)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import link_coverage_model as lm   # noqa: E402
from graphchainer_amd import cli   # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa"]
NEW = {"link-coverage-out": "link_coverage", "coverage-gfa-out": "coverage_gfa", "supported-subgraph-out": "supported_subgraph"}


@pytest.mark.parametrize("option", list(NEW))
@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_each_new_option_alone_stands_in_for_alignments_out(option, suffix):
    cfg = cli.resolve(BASE + ["--" + option, "x.out" + suffix])
    assert cfg.coverage == {NEW[option]: "x.out" + suffix} and cfg.outputs == {} and cfg.corrected == {}
    assert cli.device_output_for(cfg) == 1                                          # as for the two tables: the GAF pieces, unused
    cfg = cli.resolve(BASE + ["-a", "o.gaf", "--cigar-match-mismatch", f"--{option}=x.out" + suffix, "--coverage-out", "c.tsv"])
    assert cfg.coverage == {"coverage": "c.tsv", NEW[option]: "x.out" + suffix} and cfg.outputs == {"gaf": "o.gaf"} and cli.device_output_for(cfg) == 2
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--" + option])
    assert f"the required argument for option '--{option}' is missing" in e.value.stderr
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--" + option, "a", "--" + option, "b"])
    assert "cannot be specified more than once" in e.value.stderr


def test_all_five_together_and_the_help_lines():
    cfg = cli.resolve(BASE + ["--coverage-out", "c", "--base-coverage-out", "b", "--link-coverage-out", "l", "--coverage-gfa-out", "g", "--supported-subgraph-out", "s"])
    assert cfg.coverage == {"coverage": "c", "base_coverage": "b", "link_coverage": "l", "coverage_gfa": "g", "supported_subgraph": "s"}
    own = cli.HELP.split("This build's own:")[1].split("Accepted and without effect")[0]
    for option in NEW:
        assert len([line for line in own.splitlines() if f"--{option} arg" in line]) == 1 and cli.OPTIONS[option] == (None, "string", False)
    assert "mean depth" in own
    # the abbreviations in use before keep their meaning; the new names abbreviate where nothing was taken
    assert cli.resolve(BASE + ["--cov", "c.tsv"]).coverage == {"coverage": "c.tsv"} and cli.resolve(BASE + ["--coverage-", "c.tsv"]).coverage == {"coverage": "c.tsv"}
    assert cli.resolve(BASE + ["--link", "l", "--supp", "s"]).coverage == {"link_coverage": "l", "supported_subgraph": "s"}
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["--coverage-gfa", "g"])
    assert e.value.stderr.splitlines()[0] == "unrecognised option '--coverage-gfa'"


def test_the_library_exports_the_new_entry_points():
    import graphchainer_amd as gca
    from graphchainer_amd.api import EXPORTED_SYMBOLS, EXPORTED_SYMBOLS_NUMBERED, Coverage
    new = {"gc_coverage_create2", "gc_coverage_link_counts", "gc_coverage_format_links", "gc_coverage_format_gfa_segments", "gc_coverage_format_gfa_links"}
    assert new <= set(EXPORTED_SYMBOLS) | set(EXPORTED_SYMBOLS_NUMBERED)
    header = open(os.path.join(ROOT, "include", "graphchainer_amd.h")).read()
    declared = set(re.findall(r"\b(gc_[a-z0-9_]+)\s*\(", header))                 # (digits allowed: gc_coverage_create2)
    assert declared == set(EXPORTED_SYMBOLS) | set(EXPORTED_SYMBOLS_NUMBERED)
    assert re.search(r"#define GC_COVERAGE_PER_BASE 1u\n#define GC_COVERAGE_LINKS 2u\n", header) and (gca.api.GC_COVERAGE_PER_BASE, gca.api.GC_COVERAGE_LINKS) == (1, 2)
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = gca.load_library()
    for name in new:
        assert getattr(lib, name) is not None
    for method in ("link_counts", "link_table", "link_pieces", "gfa_pieces"):
        assert callable(getattr(Coverage, method))


def test_a_handles_links_are_numbered_as_the_model_numbers_them():
    import graphchainer_amd as gca
    if gca.device_count() < 1:
        pytest.skip("a handle's graph lives on a device")
    gfa = os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa")
    want = lm.links_of_gfa(gfa)
    assert len(want) > 0
    graph = gca.AlignmentGraph(gfa)
    for trimmed in (False, True):
        if trimmed:
            graph.trim_host()
        cov = gca.Coverage(graph, links=True)
        src, dst, counts = cov.link_counts()
        assert list(zip(src.tolist(), dst.tolist())) == want and not counts.any()
        cov.close()
    plain = gca.Coverage(graph)
    with pytest.raises(RuntimeError, match="without links"):
        plain.link_counts()
    plain.close()
    graph.close()

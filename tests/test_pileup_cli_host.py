"""--pileup-out, --pileup-min-alt and --pileup-min-alt-fraction on the command line (cli.resolve, cli.device_output_for; no device): this build's own three options."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphchainer_amd import cli   # noqa: E402

BASE = ["-g", "g.gfa", "-f", "r.fa"]


def _error_lines(argv):
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(argv)
    assert e.value.status == 1
    return e.value.stderr.splitlines()


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_the_three_options(suffix):
    cfg = cli.resolve(BASE + ["--pileup-out", "p.tsv" + suffix])
    assert cfg.coverage == {"pileup": "p.tsv" + suffix} and cfg.outputs == {} and (cfg.pileup_min_alt, cfg.pileup_min_fraction) == (1, 0.0)
    cfg = cli.resolve(BASE + ["-a", "o.gaf", "--pileup-out=p.tsv" + suffix, "--pileup-min-alt", "3", "--pileup-min-alt-fraction=0.25", "--base-coverage-out", "b.bg"])
    assert cfg.coverage == {"pileup": "p.tsv" + suffix, "base_coverage": "b.bg"} and cfg.outputs == {"gaf": "o.gaf"}
    assert (cfg.pileup_min_alt, cfg.pileup_min_fraction) == (3, 0.25)
    for fraction in ("0", "1", "1.0", "1e-3"):
        assert cli.resolve(BASE + ["--pileup-out", "p", "--pileup-min-alt-fraction", fraction]).pileup_min_fraction == float(fraction)
    assert cli.resolve(BASE + ["--pileup-out", "p", "--pileup-min-alt", "0"]).pileup_min_alt == 0
    plain = cli.resolve(BASE + ["-a", "o.gaf"])
    assert plain.coverage == {} and (plain.pileup_min_alt, plain.pileup_min_fraction) == (1, 0.0)


def test_pileup_out_alone_stands_in_for_alignments_out():
    assert _error_lines(BASE) == ["alignments-out must be given", "run with option -h for help"]
    cfg = cli.resolve(BASE + ["--pileup-out", "p.tsv"])
    assert cfg.outputs == {} and cli.device_output_for(cfg) == 1          # the GAF pieces, unused: the output jobs the counting works from exist only with some bit set
    assert cli.device_output_for(cli.resolve(BASE + ["--pileup-out", "p.tsv", "-a", "o.gam"])) == 4


@pytest.mark.parametrize("fraction", ["-0.1", "1.0000001", "2", "nan", "inf", "-inf"])
def test_a_fraction_outside_zero_to_one_is_an_error_line(fraction):
    assert _error_lines(BASE + ["--pileup-out", "p.tsv", "--pileup-min-alt-fraction=" + fraction]) == [
        "pileup minimum alternative fraction (--pileup-min-alt-fraction) must be between 0 and 1", "run with option -h for help"]


@pytest.mark.parametrize("extra", [["--pileup-min-alt", "2"], ["--pileup-min-alt-fraction", "0.5"], ["--pileup-min-alt", "2", "--pileup-min-alt-fraction", "0.5"]])
def test_a_threshold_without_pileup_out_is_an_error_line(extra):
    assert _error_lines(BASE + ["-a", "o.gaf"] + extra) == ["--pileup-min-alt and --pileup-min-alt-fraction need --pileup-out", "run with option -h for help"]
    assert _error_lines(BASE + ["-a", "o.gaf", "--base-coverage-out", "b.bg"] + extra)[0] == "--pileup-min-alt and --pileup-min-alt-fraction need --pileup-out"


def test_the_names_are_not_abbreviated_and_p_stays_precise_clipping():
    for name in ("pileup-out", "pileup-min-alt", "pileup-min-alt-fraction"):
        assert name in cli.FULL_NAME_ONLY
    for short in ("--p", "--pr", "--prec"):
        cfg = cli.resolve(BASE + ["-a", "o.gaf", short, "0.7"])
        assert cfg.coverage == {} and cli.resolve(BASE + ["-a", "o.gaf", "--precise-clipping", "0.7"]).aligner == cfg.aligner
    assert cli.parse(["--p", "0.7"]) == {"precise-clipping": [0.7]} and cli.parse(["--pr=0.7"]) == {"precise-clipping": [0.7]}
    for short in ("--pi", "--pileup", "--pileup-o", "--pileup-min", "--pileup-min-alt-f"):
        assert _error_lines(BASE + [short, "x"])[0] == f"unrecognised option '{short}'"
    assert "cannot be specified more than once" in _error_lines(BASE + ["--pileup-out", "a", "--pileup-out", "b"])[0]
    assert "the argument ('x') for option '--pileup-min-alt' is invalid" in _error_lines(BASE + ["--pileup-out", "a", "--pileup-min-alt", "x"])[0]


def test_help_has_the_three_lines_with_the_bytes_per_base():
    own = cli.HELP.split("This build's own:")[1].split("Accepted and without effect")[0]
    for name in ("--pileup-out arg", "--pileup-min-alt arg", "--pileup-min-alt-fraction arg"):
        assert len([line for line in own.splitlines() if name in line]) == 1, name
    assert "36 bytes" in own.split("--pileup-out arg")[1].split("--pileup-min-alt arg")[0]
    assert cli.OPTIONS["pileup-out"] == (None, "string", False) and cli.OPTIONS["pileup-min-alt"] == (None, "size", False) and cli.OPTIONS["pileup-min-alt-fraction"] == (None, "double", False)

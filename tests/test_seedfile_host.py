"""The seeds-file reader (-s / --seeds-file) without a GPU: the host framer (csrc/host/gc_seedfile_frame.hpp) and the per-message decoder every lane of k_sf_decode runs
(csrc/hip/gc_seedfile_core.hpp) built with g++ into an ordinary program (tests/seedfile_host/seedfile_host_test.cpp), once as it is and once more with
-fsanitize=address,undefined, and held to tests/seedfile_model.py - the reference's loop with Google's own parser - on hand-built messages and streams. Then the rows of
cli.resolve that -s adds."""
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seedfile_model as sm                        # noqa: E402
from graphchainer_amd import cli                   # noqa: E402


def vint(number, value):
    return sm.varint(number << 3) + sm.varint(value)


def blob(number, payload):
    return sm.varint(number << 3 | 2) + sm.varint(len(payload)) + payload


UNKNOWN = [vint(9, 300), sm.varint(10 << 3 | 1) + bytes(range(8)), blob(11, b"\xff\x00abc"), sm.varint(12 << 3 | 5) + b"\x01\x02\x03\x04"]   # wire types 0, 1, 2, 5


def position(node_id=None, offset=None, reverse=None, order=(0, 1, 2), extra=b""):
    parts = [b"" if node_id is None else vint(1, node_id), b"" if offset is None else vint(2, offset), b"" if reverse is None else vint(4, int(reverse))]
    return b"".join(parts[i] for i in order) + extra


def edit(from_length=None, extra=b""):
    return (b"" if from_length is None else vint(1, from_length)) + extra


def mapping(positions=(), edits=(), order="pe", extra=b""):
    p, e = b"".join(blob(1, x) for x in positions), b"".join(blob(2, x) for x in edits)
    return (p + e if order == "pe" else e + p) + extra


def path(mappings=(), extra=b""):
    return b"".join(blob(2, m) for m in mappings) + extra


def alignment(name=None, seq_pos=None, paths=(), order=(0, 1, 2), extra=b""):
    parts = [b"" if name is None else blob(3, name), b"" if seq_pos is None else vint(7, seq_pos), b"".join(blob(2, p) for p in paths)]
    return b"".join(parts[i] for i in order) + extra


PLAIN = alignment(b"read/1 extra words", 1234, [path([mapping([position(77, 31, True)], [edit(15)])])])
PATH_FIRST = alignment(b"read/2", 77, [path([mapping([position(78, 32, True)], [edit(16)])])], order=(2, 0, 1))


def good_messages():
    out = [PLAIN, sm.seed_message("r", 0, 0, 0, 0, False), sm.seed_message("read7", 12, 5, 900, 19, True)]
    m = mapping([position(5, 6, False)], [edit(21)])
    out += [alignment(b"o", 3, [path([m])], order=o) for o in itertools.permutations(range(3))]                       # fields in every order
    out += [alignment(b"p", 3, [path([mapping([position(5, 6, True, order=o)], [edit(21)], order=mo)])]) for o in itertools.permutations(range(3)) for mo in ("pe", "ep")]
    out += [alignment(b"z", None, [path([mapping([position()], [edit()])])]), alignment(None, None, [path([mapping([], [b""])])])]   # proto3 leaves zeros out
    for node_id, offset, seq_pos, length in ((-5, -1, -7, -3), (1 << 31, (1 << 32) - 1, (1 << 31) - 1, (1 << 31) - 1), ((1 << 32) + 5, (1 << 32) - 2, 0, -(1 << 31)), (-(1 << 63), 1 << 40, -1, 1 << 31)):
        out.append(alignment(b"n", seq_pos, [path([mapping([position(node_id, offset, True)], [edit(length)])])]))            # negative values: 10-byte varints
    for u in UNKNOWN:                                                                                                    # unknown fields at every level
        out.append(alignment(b"u", 8, [path([mapping([position(5, 6, True, extra=u)], [edit(21, extra=u)], extra=u)], extra=u)], extra=u))
        out.append(u + alignment(b"u", 8, [path([u + mapping([u + position(5, 6, True)], [u + edit(21)])])]))
    out.append(alignment(b"s", 4, [path([], extra=blob(1, b"pathname")), path([mapping([position(9, 1)], [edit(30)])]), path([mapping([position(8, 2)], [edit(31)])])]))   # path in several occurrences
    out.append(alignment(b"s2", 4, [path([mapping([position(9, 1)], [edit(2)])]), path([mapping([position(8, 2)], [edit(31)])])]))
    out.append(alignment(b"t", 4, [path([mapping([position(3, 9), position(None, 4, True)], [edit(7)])])]))              # two positions in one mapping are merged
    out.append(alignment(b"t", 4, [path([mapping([position(3, 9, True), position(None, None, False)], [edit(7), edit(99)]), mapping([position(1, 1)], [edit(1)])])]))   # later edits and mappings
    out.append(alignment(b"first", 4, [path([mapping([position(3, 9)], [edit(7)])])], extra=blob(3, b"last") + vint(7, 99)))   # a scalar given twice keeps the last
    out.append(vint(3, 5) + blob(7, b"xx") + alignment(b"w", 4, [path([mapping([position(3, 9)], [edit(7)])])]))           # known numbers with another wire type are unknown fields
    out.append(alignment(b"v", 4, [path([mapping([position(3, 9)], [edit(7)])])], extra=blob(1, b"ACGT") + vint(6, 5) + sm.varint(16 << 3 | 1) + bytes(8)))   # sequence, score, identity
    for n in (0, 1, 127, 128, 5000):                                                                                     # names across the size varint's widths
        out.append(alignment(bytes(65 + i % 26 for i in range(n)), 4, [path([mapping([position(3, 9)], [edit(7)])])]))
    return out


def refused_messages():
    m = mapping([position(5, 6, True)], [edit(21)])
    out = [alignment(b"a", 1, []), alignment(b"a", 1, [path([])]), alignment(b"a", 1, [path([mapping([position(1, 2)], [])])]),      # no mapping (no path; an empty path), no edit
           alignment(b"a", 1, [path([mapping([position(1, 2)], []), mapping([position(1, 2)], [edit(5)])])]),                       # the edit of a later mapping does not count
           alignment(b"a", 1, [path([m])], extra=sm.varint(7 << 3) + b"\x80" * 10 + b"\x00"),                                       # a varint of 11 bytes
           alignment(b"a", 1, [path([m])], extra=sm.varint(9 << 3 | 3) + sm.varint(9 << 3 | 4)),                                    # a group
           alignment(b"a", 1, [path([m + sm.varint(9 << 3 | 3) + sm.varint(9 << 3 | 4)])]),                                         # ... inside a mapping
           alignment(b"a", 1, [path([m])], extra=sm.varint(3 << 3 | 2) + sm.varint(5) + b"abcd"),                                   # a length past the message
           alignment(b"a", 1, [path([m])], extra=sm.varint(10 << 3 | 1) + bytes(7)), alignment(b"a", 1, [path([m])], extra=sm.varint(12 << 3 | 5) + bytes(3)),
           alignment(b"a", 1, [path([m]), path([mapping([position(1, 2)], [edit(5)]) + b"\x0a\x05"])])]                              # damage in a mapping that is not used
    out += [PLAIN[:k] for k in range(1, len(PLAIN))] + [PATH_FIRST[:k] for k in range(1, len(PATH_FIRST))]                         # a message cut at every byte
    return out


def streams():
    good = good_messages()
    out = [b"", sm.write_stream([good]), sm.write_stream([[m] for m in good]), sm.write_stream([good[:3], [], good[3:5], [], []]),
           sm.write_stream([[good[0], b"", good[1], b"", b""], [b""], good[2:4]]),                       # sizes of 0
           sm.write_stream([0, good[:2]]), sm.write_stream([[]]), sm.write_stream([good[:2], 0, 0, good[2:3], 0]),   # a first count of 0 ends the file; later ones do not
           sm.varint(2) + sm.varint((1 << 32) + len(good[0])) + good[0] + sm.varint(1 << 32) + sm.varint(len(good[1])) + good[1]]   # ReadVarint32 keeps the low 32 bits
    out += [sm.write_stream([[good[0], m, good[1]]]) for m in refused_messages()]
    whole = sm.write_stream([[good[0], PLAIN], [good[1]]])
    out += [whole[:k] for k in range(1, len(whole))]                                                     # the stream cut at every byte: counts, sizes and messages past its end
    out += [sm.write_stream([good[:1]]) + b"\x80" * 10 + b"\x01", sm.write_stream([good[:1]]) + sm.varint(1) + b"\xff" * 11, sm.write_stream([good[:1], 3])]
    return out


def _cases():
    all_streams = streams()
    cases = [(1 << 20, 0, s) for s in all_streams]
    cases += [(piece, feed, s) for s in all_streams[:9] for piece, feed in ((1, 1), (64, 7), (300, 0), (6000, 4096))]
    return cases


def _want(raw):
    try:
        return sm.read_stream(raw)
    except sm.SeedFileRefused as e:
        text = str(e)
        return "MAPPING" if "without a mapping" in text else "EDIT" if "without an edit" in text else "PARSE" if "does not parse" in text or "group" in text else "FRAME"


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def want(cases):
    memo = {}
    return [memo[s] if s in memo else memo.setdefault(s, _want(s)) for _, _, s in cases]


def _build(tmp, sanitize):
    out = str(tmp / ("seedfile_host_test_san" if sanitize else "seedfile_host_test"))
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(csrc, "hip"), "-I" + os.path.join(csrc, "host"),
                    os.path.join(ROOT, "tests", "seedfile_host", "seedfile_host_test.cpp"), "-o", out] + flags, check=True, timeout=600)
    return out


def _run(exe, tmp, cases):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for piece, feed, raw in cases:
            f.write(f"{piece} {feed} {raw.hex() or '-'}\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")
    got, at = [], 0
    for _ in cases:
        head = lines[at].split(" ")
        at += 1
        if head[0] == "ERR":
            got.append((head[1], None))
            continue
        n, pieces = int(head[1]), int(head[2])
        rows = []
        for row in lines[at:at + n]:
            name, *numbers = row.split(" ")
            rows.append((b"" if name == "-" else bytes.fromhex(name), tuple(int(x) for x in numbers[:6]), int(numbers[6])))
        at += n
        got.append((rows, pieces))
    return got


def _compare(got, want, cases):
    assert len(got) == len(want)
    hashes = {}
    for k, ((g, pieces), w, (piece, feed, raw)) in enumerate(zip(got, want, cases)):
        if isinstance(w, str):
            assert g == w, (k, piece, feed, raw[:200].hex())
            continue
        assert not isinstance(g, str), (k, g, raw[:200].hex())
        assert [(name, hit) for name, hit, _ in g] == w, (k, piece, feed, raw[:200].hex())
        if piece == 1 and g:
            assert pieces == len(g)                          # every message a piece of its own, the 5 000-byte one too
        for name, _, h in g:
            assert hashes.setdefault(name, h) == h           # one name, one hash
    assert len(set(hashes.values())) == len(hashes) > 10


def test_the_cases_cover_what_they_claim(cases, want):
    kinds = {w for w in want if isinstance(w, str)}
    assert kinds == {"MAPPING", "EDIT", "PARSE", "FRAME"}
    parsed = [w for w in want if not isinstance(w, str)]
    assert any(len(w) > 40 for w in parsed) and [] in parsed
    hits = {hit for w in parsed for _, hit in w}
    assert {h[1] for h in hits} >= {0xFFFFFFFF, 0xFFFFFFFE, 0} and {h[2] for h in hits} >= {0xFFFFFFFF, (1 << 31) - 1}
    assert {h[0] for h in hits} >= {-5, -(1 << 31), 5, 0} and {h[3] for h in hits} >= {(1 << 32) - 3, 1 << 31, (1 << 31) - 1}
    assert {len(name) for w in parsed for name, _ in w} >= {0, 1, 127, 128, 5000}
    cut = [sm.write_stream([[m[:k]]]) for m in (PLAIN, PATH_FIRST) for k in range(1, len(m))]
    assert {_want(s) if isinstance(_want(s), str) else "OK" for s in cut} == {"PARSE", "MAPPING", "OK"}   # a message cut behind its path still parses: then it is a seed


def test_framer_and_decoder_on_the_host_equal_the_model(tmp_path, cases, want):
    _compare(_run(_build(tmp_path, False), tmp_path, cases), want, cases)


def test_framer_and_decoder_under_the_address_and_undefined_sanitizers(tmp_path, cases, want):
    """The same inputs through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded): every stream and every message lies in
    an allocation of exactly its length, so a read past the end of either stops the program."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _compare(_run(_build(tmp_path, True), tmp_path, cases), want, cases)


BASE = ["-g", "graph.gfa", "-f", "r.fa", "-a", "o.gaf"]


def test_seeds_file_is_a_seeding_method_of_the_command_line():
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-s", "a.gam"])                                   # beside the default minimizer density of 10
    assert e.value.status == 1 and "pick only one seeding method" in e.value.stderr
    cfg = cli.resolve(BASE + ["-s", "a.gam", "b.gam", "--seeds-minimizer-density", "0"])
    assert cfg.seeder == {"kind": "file", "paths": ["a.gam", "b.gam"]} and cfg.aligner["seed_density"] == 0.0
    with pytest.raises(cli.CliExit) as e:
        cli.resolve(BASE + ["-s", "a.gam", "--seeds-minimizer-density", "0", "--seeds-mum-count", "5"])
    assert e.value.status == 1 and "pick only one seeding method" in e.value.stderr
    assert cli.resolve(BASE + ["-sa.gam", "--seeds-minimizer-density", "0"]).seeder == {"kind": "file", "paths": ["a.gam"]}
    assert cli.resolve(BASE + ["--seeds-file", "a.gam", "--seeds-file=b.gam", "--seeds-minimizer-density", "0"]).seeder["paths"] == ["a.gam", "b.gam"]
    assert "seeds-file" not in cli.REFUSED and "--seeds-file" in cli.HELP.split("Seeding parameters")[1].split("Extension parameters")[0]
    assert "seeds-file" not in cli.HELP.split("Not supported by this build")[1]


def test_a_missing_seeds_file_ends_the_run_with_status_0_before_anything_is_loaded(tmp_path, capsys):
    out = tmp_path / "o.gaf"
    status = cli.main(["-g", str(tmp_path / "none.gfa"), "-f", str(tmp_path / "none.fa"), "-a", str(out), "-s", str(tmp_path / "none.gam"), "--seeds-minimizer-density", "0"])
    assert status == 0 and capsys.readouterr().err == "No seeds file exists\n" and not out.exists()

"""The MUM / MEM index built on the device and kept on disk (gc_mxm_index_open; MxmIndex(graph, build=..., cache_prefix=...)). All suffixes of the text are distinct, so the
suffix array has one right value and the device build is held to the host build element for element:
  1. array("sa") of a device-built index equals a host-built one's: a variant graph, homopolymers / STRs / a tandem array, the IUPAC graph (separators inside segments), two
     identical segments plus a prefix of them, and hand-made texts shorter than the first key and at and around a wave and a block;
  2. the doubling loop was exercised where the input holds a repeat longer than the first key (a condition on the inputs, computed here from the host's array);
  3. the seeds from a device-built index are those from a host-built one, as ordered lists;
  4. the cache: built and written, then loaded, byte-identical after a host and a device build; a foreign, damaged or truncated file is refused by name and left alone;
The device build's refusal of a text of 2^31 - 1 letters or more cannot be provoked with a real graph and the library has no switch that moves the limit: the predicate is
held at its boundary on the CPU (tests/mxm_cache_host), the call site is left to code reading.
Graphs and their two indexes are made once and shared (as test_mxm_seeds_gpu.py's Case)."""
import ctypes as C
import os
import random
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lowcomplexity as lc                                  # noqa: E402
import mxm_model as mm                                      # noqa: E402
from graphchainer_amd.synth import SynthGraph              # noqa: E402  (test inputs)
from test_gpu_parity import gca                             # noqa: E402,F401  (the fixture)

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_SHARED = {}
TINY = (1, 20, 63, 64, 65, 256, 257)   # text letters, separators included (1: one letter and its separator, the shortest text a segment makes)
FIRST_KEY = 21                          # letters of the builders' first sort key


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("mxm_build")


class Pair:
    """A graph with a host-built and a device-built index, and the model's text."""

    def __init__(self, gca, gfa, reads=None):   # noqa: F811
        self.gfa, self.reads = gfa, reads
        self.text = mm.Text(mm.gfa_segments(gfa))
        self.graph = gca.AlignmentGraph(gfa)
        self.host = gca.MxmIndex(self.graph, build="host")
        self.device = gca.MxmIndex(self.graph, build="device")
        self.batch = gca.ReadBatch(reads) if reads else None


def _write_segments(path, segments):
    with open(path, "w") as f:
        for i, s in enumerate(segments, 1):
            f.write(f"S\t{i}\t{s}\n")


def _tiny_segments(n):
    """Segments whose text has n letters, separators included: a period-3 sequence and a prefix of it, so that ties run across the separator and past the text's end."""
    if n == 1:
        return ["A"]           # (text: the letter and its separator)
    a = 2 * n // 3 - 1
    b = n - 2 - a
    unit = ("ACG" * (n // 3 + 1))
    return [unit[:a], unit[:b]]


def pair(gca, workdir, name):   # noqa: F811
    if name in _SHARED:
        return _SHARED[name]
    gfa = str(workdir / f"{name}.gfa")
    reads = None
    if name == "variant":
        sg = SynthGraph(40_000, seed=37)
        sg.write_gfa(gfa)
        reads = sg.sample_reads(3, 1200, seed=6, p_del=0.01, p_sub=0.01, p_ins=0.01)
        reads.append(reads[0].translate(_COMP)[::-1])
    elif name == "tier_a":
        lc.tier("a")[0].write_gfa(gfa)
    elif name == "iupac":
        from letters_inputs import rewrite_gfa
        sg = SynthGraph(40_000, seed=23, repeats=3)
        plain = str(workdir / "iupac_plain.gfa")
        sg.write_gfa(plain)
        assert len(rewrite_gfa(sg, plain, gfa)) > 100   # IUPAC codes written into segments: separators inside them
    elif name == "twins":
        rng = random.Random(99)
        s = "".join(rng.choice("ACGT") for _ in range(3000))
        _write_segments(gfa, [s, s, s[:1000]])
    else:
        _write_segments(gfa, _tiny_segments(int(name.split("_")[1])))
    _SHARED[name] = Pair(gca, gfa, reads)
    return _SHARED[name]


def _one(index, name):
    return int(index.array(name)[0])


@pytest.mark.parametrize("name", ["variant", "tier_a", "iupac", "twins"] + [f"tiny_{n}" for n in TINY])
def test_device_built_suffix_array_is_the_host_built_one(gca, workdir, name):   # noqa: F811
    p = pair(gca, workdir, name)
    n = len(p.text.T)
    if name.startswith("tiny_"):
        assert n == max(2, int(name.split("_")[1]))
    if name == "iupac":
        assert p.text.T.count(b"$") - len(p.text.ids) > 100   # separators inside segments
    host, device = p.host.array("sa"), p.device.array("sa")
    assert len(host) == n and np.array_equal(np.sort(host), np.arange(n))
    assert np.array_equal(device, host)
    for key in ("node_start", "node_id"):
        assert np.array_equal(p.device.array(key), p.host.array(key))
    assert p.device.array("node_start").tolist() == p.text.starts and p.device.array("node_id").tolist() == p.text.ids
    assert (_one(p.host, "build_mode"), _one(p.device, "build_mode")) == (0, 1)
    assert _one(p.host, "build_scratch_bytes") == 0 and _one(p.device, "build_scratch_bytes") >= 29 * n
    assert _one(p.device, "build_rounds") == _one(p.host, "build_rounds")   # the same groups refined with the same h: the two builders take the same number of rounds
    assert _one(p.device, "bytes") == _one(p.host, "bytes") and _one(p.device, "build_us") > 0


def _longest_common_prefix_of_neighbours(T, sa):
    """The longest common prefix of two suffixes that are neighbours in sa (separators compare equal, as in the builders' order)."""
    best = 0
    n = len(T)
    for a, b in zip(sa[:-1], sa[1:]):
        room = n - max(a, b)
        if room <= best or T[a:a + best + 1] != T[b:b + best + 1]:
            continue
        lo, hi = best + 1, room   # T[a:a+lo] == T[b:b+lo] holds; the longest such length by bisection
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if T[a:a + mid] == T[b:b + mid]:
                lo = mid
            else:
                hi = mid - 1
        best = lo
    return best


@pytest.mark.parametrize("name,repeat", [("twins", 500), ("tier_a", 250)])
def test_doubling_rounds_were_run(gca, workdir, name, repeat):   # noqa: F811
    """A repeat longer than the first key leaves tied groups after the first sort. The condition on the input - the longest common prefix of SA neighbours - is computed from
    the host's array: at least 500 letters on the identical segments (3 000 in fact). On the tier-a graph it is 250, not 500: the variant sites cut that graph's homopolymers
    and arrays into segments of at most 285 letters and every segment ends in a separator, so no repeat of the text is longer - still twelve times the first key. Two such
    suffixes stay tied until the known prefix, 21 x 2^rounds, exceeds their common prefix, which is asserted from the rounds the builders report."""
    p = pair(gca, workdir, name)
    lcp = _longest_common_prefix_of_neighbours(p.text.T, p.host.array("sa").tolist())
    assert lcp >= repeat > FIRST_KEY
    rounds = _one(p.device, "build_rounds")
    assert rounds >= 1
    assert FIRST_KEY * 2 ** rounds > lcp and _one(p.host, "build_rounds") == rounds
    assert _one(p.device, "build_mode") == 1 and _one(p.device, "build_scratch_bytes") >= 29 * len(p.text.T) and _one(p.host, "build_scratch_bytes") == 0
    assert p.device.array("node_start").tolist() == p.text.starts


def _seeds(index, batch, mode, min_len):
    return [[tuple(h) for h in per_read.tolist()] for per_read in index.seeds(batch, mode, count=None, min_len=min_len).hits()]


def test_seeds_from_a_device_built_index(gca, workdir):   # noqa: F811
    p = pair(gca, workdir, "variant")
    for mode in ("mem", "mum"):
        for min_len in (20, 5):
            want = _seeds(p.host, p.batch, mode, min_len)
            assert sum(len(w) for w in want) > 60
            assert _seeds(p.device, p.batch, mode, min_len) == want, (mode, min_len)


def _stat(path):
    return os.stat(path).st_mtime_ns, open(path, "rb").read()


def test_cache_round_trip(gca, workdir):   # noqa: F811
    p = pair(gca, workdir, "variant")
    cache = workdir / "cache"
    cache.mkdir()
    prefix_d, prefix_h = str(cache / "device"), str(cache / "host")
    built = gca.MxmIndex(p.graph, build="device", cache_prefix=prefix_d)
    assert _one(built, "build_mode") == 1 and os.path.exists(prefix_d + ".gcmxm") and _one(built, "cache_save_us") > 0
    before = _stat(prefix_d + ".gcmxm")
    loaded = gca.MxmIndex(p.graph, build="device", cache_prefix=prefix_d)
    assert _one(loaded, "build_mode") == 2 and _one(loaded, "build_rounds") == 0 and _one(loaded, "build_scratch_bytes") == 0 and _one(loaded, "cache_save_us") == 0
    assert _stat(prefix_d + ".gcmxm") == before
    for key in ("sa", "node_start", "node_id"):
        assert np.array_equal(loaded.array(key), p.host.array(key)) and np.array_equal(built.array(key), p.host.array(key)), key
    for mode, min_len in (("mem", 20), ("mum", 20), ("mem", 5)):
        assert _seeds(loaded, p.batch, mode, min_len) == _seeds(p.host, p.batch, mode, min_len), (mode, min_len)
    by_host = gca.MxmIndex(p.graph, build="host", cache_prefix=prefix_h)
    assert _one(by_host, "build_mode") == 0
    assert open(prefix_h + ".gcmxm", "rb").read() == before[1]   # byte-identical after a host build and after a device build
    assert sorted(os.listdir(cache)) == ["device.gcmxm", "host.gcmxm"]   # no temporary file remains
    info = gca.api.mxm_cache_check(prefix_d)
    assert (info["version"], info["text_letters"], info["segments"], info["file_bytes"]) == (1, len(p.text.T), len(p.text.ids), len(before[1]))


def _open(gca, graph, build, prefix):   # noqa: F811
    lib = gca.load_library()
    options = gca.api.GcMxmOptions()
    lib.gc_mxm_options_default(C.byref(options))
    options.build = build
    options.cache_prefix = prefix.encode() if prefix else None
    handle = C.c_void_p()
    rc = lib.gc_mxm_index_open(graph.handle, C.byref(options), C.byref(handle))
    return rc, handle.value, lib.gc_last_error().decode()


def test_cache_refusals(gca, workdir):   # noqa: F811
    """GC_ERR_GRAPH (-2), the file named in gc_last_error, the file as it was, no index returned: another graph's cache, a flipped byte in the suffix array, a truncated file."""
    p, other = pair(gca, workdir, "variant"), pair(gca, workdir, "iupac")
    refusals = workdir / "refusals"
    refusals.mkdir()
    good_prefix = str(refusals / "good")
    gca.MxmIndex(p.graph, build="device", cache_prefix=good_prefix).close()
    good = open(good_prefix + ".gcmxm", "rb").read()
    n = len(p.text.T)

    def refused(graph, data, needle, build=1):
        prefix = str(refusals / "victim")
        with open(prefix + ".gcmxm", "wb") as f:
            f.write(data)
        before = _stat(prefix + ".gcmxm")
        rc, handle, message = _open(gca, graph, build, prefix)
        assert rc == -2 and not handle, (rc, message)
        assert prefix + ".gcmxm" in message and needle in message, message
        assert _stat(prefix + ".gcmxm") == before

    refused(other.graph, good, "another graph")
    refused(other.graph, good, "another graph", build=0)
    flipped = bytearray(good)
    flipped[len(good) - 8 - 2 * n] ^= 0x04   # the middle of the suffix array (4 n bytes before the checksum)
    refused(p.graph, bytes(flipped), "checksum")
    refused(p.graph, good[:len(good) // 2], "truncated")
    refused(p.graph, good[:-1], "truncated")
    shutil.copyfile(good_prefix + ".gcmxm", str(refusals / "victim.gcmxm"))
    rc, handle, message = _open(gca, p.graph, 1, str(refusals / "victim"))   # and the undamaged bytes under the same name load
    assert rc == 0 and handle, message
    gca.load_library().gc_mxm_index_destroy(handle)
    assert sorted(os.listdir(refusals)) == ["good.gcmxm", "victim.gcmxm"]

"""CPU-side check of csrc/host/gc_switches.hpp, the one place the library reads its GC_* variables: tests/switches_host/switches_test.cpp sets the environment case by
case and prints gc::Switches::fromEnvironment(). The expected values below restate the expressions the reading sites had before the header existed (atoi / atol /
atoll / atof, then the site's own comparison or clamp), not the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every field with nothing set: INTEGRATION.md §7's defaults
DEFAULTS = {
    "hostThreads": "unset", "batchThreads": "unset", "buildThreads": "unset", "resultCacheMin": str(32 << 20),
    "spinSync": "2", "syncPollUs": "40", "longToken": "1", "shareLongScratch": "1", "onePassAtATime": "1", "longTokens": "unset", "debugTimes": "0", "debugEd": "0",
    "hostAnchors": "0", "extLazy": "1", "extendSlab": "0", "hostStitch": "0", "stitchClass": "unset", "chainPlainScan": "0",
    "edFirstK": "unset", "seederBuildOnHost": "0", "buildReferenceContainers": "0",
    "testExtMaxItems": "unset", "testExtMaxPending": "unset", "testExtMaxTrace": "unset", "testExtRetryMaxItems": "unset", "testLongMaxItems": "unset",
    "testLongMaxCols": "unset", "testLongCellsPerBase": "unset", "testLongMaxAlignments": "unset", "testLongScratchGb": "unset", "testStitchSetMax": "unset",
    "testStitchBfsCap": "unset", "testSeedFilterBits": "unset", "testFailLong": "unset", "testLongForceFallback": "0", "testLongRegCap": "unset",
    "testLongMaxBlocks": "unset", "testLongTeam": "unset", "testLongOrder": "1", "testLongSpeculate": "unset", "testChainForceScratch": "0",
    "testPoolFirstGuess": "unset", "testPoolShrinkFloor": str(64 << 20), "testResultCachePoison": "0", "testUploadSlice": str(64 << 20),
}


def _cases():
    """(environment, the fields that differ from DEFAULTS)."""
    cases = [("-", {})]

    def one(name, field, pairs):
        for value, want in pairs:
            cases.append((f"{name}={value}", {} if want is None else {field: str(want)}))

    # ---- host set-up. max(1, atoi): one below, at and above the bound
    one("GC_HOST_THREADS", "hostThreads", [(0, 1), (1, 1), (2, 2), (12, 12)])
    one("GC_BATCH_THREADS", "batchThreads", [(0, 1), (1, 1), (2, 2), (6, 6)])
    one("GC_BUILD_THREADS", "buildThreads", [(-3, None), (0, None), (1, 1), (2, 2), (24, 24)])                  # atol, values below 1 are ignored
    one("GC_RESULT_CACHE_MIN", "resultCacheMin", [(0, 1), (1, 1), (2, 2), (4096, 4096), (1 << 33, 1 << 33)])    # max(1, atoll)
    # ---- run time
    one("GC_SPIN_SYNC", "spinSync", [(0, 0), (1, 1), (2, 2)])                                                  # atoi, as it is
    one("GC_SYNC_POLL_US", "syncPollUs", [(0, 1), (1, 1), (2, 2), (100, 100)])
    for value, share, one_at_a_time in ((-1, 0, 1), (0, 0, 0), (1, 1, 1), (2, 1, 1)):                           # shared scratch: >= 1; one pass at a time: not "set and 0"
        cases.append((f"GC_LONG_TOKEN={value}", {"longToken": str(value), "shareLongScratch": str(share), "onePassAtATime": str(one_at_a_time)}))
    one("GC_LONG_TOKENS", "longTokens", [(0, 1), (1, 1), (2, 2), (3, 2)])                                       # 1..LONG_TOKENS_MAX (2)
    one("GC_DEBUG_TIMES", "debugTimes", [(1, 1), (0, 1), ("", 1)])                                              # set at all
    one("GC_DEBUG_ED", "debugEd", [(1, 1), (0, 1), ("", 1)])
    # ---- fall-back paths. "exactly 0 turns the default off" (the empty string is atoi's 0), "exactly 1", "any non-zero value"
    one("GC_EXT_LAZY", "extLazy", [(0, 0), (1, 1), (2, 1), ("", 0)])
    for name, field in (("GC_HOST_ANCHORS", "hostAnchors"), ("GC_EXTEND_SLAB", "extendSlab"), ("GC_CHAIN_PLAIN_SCAN", "chainPlainScan"),
                        ("GC_BUILD_REFERENCE_CONTAINERS", "buildReferenceContainers")):
        one(name, field, [(0, 0), (1, 1), (2, 0), ("", 0)])
    one("GC_HOST_STITCH", "hostStitch", [(0, 0), (1, 1), (2, 1), ("", 0)])
    one("GC_STITCH_CLASS", "stitchClass", [(3, 3), (0, 0), (2, 0), (4, 0)])                                     # 3 if the value is 3, else 0
    one("GC_ED_FIRST_K", "edFirstK", [(0, 1), (1, 1), (2, 2), (72, 72)])
    one("GC_SEEDER_BUILD", "seederBuildOnHost", [("host", 1), ("device", 0)])
    # ---- test hooks. The capacities are atoll as it is: 0 and negative values are values (GC_TEST_LONG_MAX_COLS=0: no column store)
    for name, field in (("GC_TEST_EXT_MAX_ITEMS", "testExtMaxItems"), ("GC_TEST_EXT_MAX_PENDING", "testExtMaxPending"), ("GC_TEST_EXT_MAX_TRACE", "testExtMaxTrace"),
                        ("GC_TEST_LONG_MAX_ITEMS", "testLongMaxItems"), ("GC_TEST_LONG_MAX_COLS", "testLongMaxCols"), ("GC_TEST_LONG_CELLS_PER_BASE", "testLongCellsPerBase"),
                        ("GC_TEST_STITCH_SET_MAX", "testStitchSetMax"), ("GC_TEST_STITCH_BFS_CAP", "testStitchBfsCap")):
        one(name, field, [(123, 123), (0, 0), (-1, -1), (1 << 35, 1 << 35)])
    one("GC_TEST_EXT_RETRY_MAX_ITEMS", "testExtRetryMaxItems", [(7, 8), (8, 8), (9, 9), (100, 100)])            # >= 8
    one("GC_TEST_LONG_MAX_ALIGNMENTS", "testLongMaxAlignments", [(0, 1), (1, 1), (2, 2), (40, 40), (65535, 65535), (65536, 65536), (65537, 65536)])
    one("GC_TEST_LONG_SCRATCH_GB", "testLongScratchGb", [(0, 1), (1, 1), (2, 2), (48, 48)])
    one("GC_TEST_SEED_FILTER_BITS", "testSeedFilterBits", [(9, 10), (10, 10), (11, 11), (20, 20), (29, 29), (30, 30), (31, 30)])
    one("GC_TEST_FAIL_LONG", "testFailLong", [(5, 5), (0, 0), (-1, -1)])                                        # atol; the site checks the range against the batch
    one("GC_TEST_LONG_FORCE_FALLBACK", "testLongForceFallback", [(1, 1), (0, 1), ("", 1)])
    one("GC_TEST_LONG_REG_CAP", "testLongRegCap", [(0, 1), (1, 1), (2, 2), (8, 8), (63, 63), (64, 64), (65, 64)])
    one("GC_TEST_LONG_MAX_BLOCKS", "testLongMaxBlocks", [(0, 1), (1, 1), (2, 2), (64, 64)])
    one("GC_TEST_LONG_TEAM", "testLongTeam", [(3, None), (128, None), (0, None), (16, 16), (1, 1), (64, 64)])    # only 1, 2, 4, ..., 64 count
    one("GC_TEST_LONG_ORDER", "testLongOrder", [(0, 0), (1, 1), (2, 2)])
    one("GC_TEST_LONG_SPECULATE", "testLongSpeculate", [(0, 1), (1, 1), (2, 2), (3, 2)])
    one("GC_TEST_CHAIN_FORCE_SCRATCH", "testChainForceScratch", [(1, 1), (0, 1), ("", 1)])
    one("GC_TEST_POOL_FIRST_GUESS", "testPoolFirstGuess", [(-1, 0), (0, 0), (0.5, 0.5), (2, 2)])                # max(0.0, atof)
    one("GC_TEST_POOL_SHRINK_FLOOR", "testPoolShrinkFloor", [(-1, 0), (0, 0), (1, 1), (4096, 4096)])            # max(0, atoll)
    one("GC_TEST_RESULT_CACHE_POISON", "testResultCachePoison", [(1, 1), (0, 1), ("", 1)])
    one("GC_TEST_UPLOAD_SLICE", "testUploadSlice", [(0, 1), (1, 1), (2, 2), (1000, 1000)])
    # several at once, as the GPU tests set them
    cases.append(("GC_LONG_TOKEN=0 GC_LONG_TOKENS=2 GC_TEST_LONG_TEAM=2 GC_DEBUG_TIMES=1",
                  {"longToken": "0", "shareLongScratch": "0", "onePassAtATime": "0", "longTokens": "2", "testLongTeam": "2", "debugTimes": "1"}))
    return cases


def _build(tmp_path, flags=()):
    exe = str(tmp_path / "switches_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "switches_host", "switches_test.cpp"), "-o", exe], check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_switches_are_parsed_as_their_sites_parsed_them(tmp_path, sanitize):
    """Defaults with a clean environment; for every variable an ordinary value; one value below, at and above every bound; 0 / 1 / 2 / empty for the exact-value switches;
    both flags derived from GC_LONG_TOKEN. The second case is the same stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if sanitize else ())
    cases = _cases()
    env = {k: v for k, v in os.environ.items() if not k.startswith("GC_")}
    env["GC_EXT_LAZY"] = "0"   # (what the program inherits must not leak into a case)
    run = subprocess.run([exe], input="".join(c[0] + "\n" for c in cases), capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for (setting, differs), line in zip(cases, got):
        fields = dict(item.split("=", 1) for item in line.split())
        assert fields.keys() == DEFAULTS.keys(), setting
        want = {**DEFAULTS, **differs}
        wrong = {k: (fields[k], want[k]) for k in want if fields[k] != want[k]}
        assert not wrong, (setting, wrong)


def test_every_variable_of_the_header_has_a_case():
    import re
    header = open(os.path.join(ROOT, "graphchainer_amd", "csrc", "host", "gc_switches.hpp")).read()
    names = set(re.findall(r'getenv\("(GC_[A-Z0-9_]+)"\)', header))
    tried = {item.split("=")[0] for setting, _ in _cases() for item in setting.split() if item != "-"}
    assert names == tried, (sorted(names - tried), sorted(tried - names))

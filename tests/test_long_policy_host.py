"""CPU-side check of csrc/host/gc_long_policy.hpp, the whole-read pass's sizing and growth rules: tests/long_policy_host/long_policy_test.cpp reads a rule and its arguments
per line and prints the rule's value. The expected values below restate the expressions the pass held inline before the header existed (quoted above each group, C++
integer division and the casts to uint32_t spelled out), not the header; the literals among them were worked out by hand from the same expressions."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 0xffffffff
GB = 1 << 30


def u32(x):
    return x & U32


def _cases():
    """(input line, expected output line)."""
    cases = []

    def case(rule, args, want):
        cases.append((" ".join([rule] + [str(a) for a in args]), " ".join(str(w) for w in want) if isinstance(want, (list, tuple)) else str(want)))

    # ---- firstAlnCap = (uint32_t)std::max<uint64_t>(32, maxReadLen / 512): below, at and above the bound
    for length, literal in ((1, 32), (511 * 32, 32), (512 * 32, 32), (512 * 33 - 1, 32), (512 * 33, 33), (50000, 97)):
        assert u32(max(32, length // 512)) == literal
        case("firstcap", [length], literal)

    # ---- cellBudgetFor: b += perBase * (offsets[r + 1] - offsets[r]) + 1024 over the reads
    for per_base, lens, literal in ((4, [1, 10000, 50000], 243076), (2, [], 0), (256, [50000], 12801024), (8, [512 * 32] * 3, 396288)):
        assert sum(per_base * n + 1024 for n in lens) == literal
        case("cellbudget", [per_base] + lens, literal)

    # ---- the pass rerun is refused when next > 256 || cellBudgetFor(next) * sizeof(LongCell) > (64ull << 30)
    for per_base, cells, cell_bytes, literal in ((255, 1, 8, 0), (256, 1, 8, 0), (257, 1, 8, 1), (8, 64 * GB // 8 - 1, 8, 0), (8, 64 * GB // 8, 8, 0), (8, 64 * GB // 8 + 1, 8, 1),
                                                 (256, 64 * GB // 16, 16, 0), (256, 64 * GB // 16 + 1, 16, 1)):
        assert int(per_base > 256 or cells * cell_bytes > 64 * GB) == literal
        case("refused", [per_base, cells, cell_bytes], literal)

    # ---- next = std::max<uint64_t>(cur + 2, (asked + asked / 2 + bases - 1) / bases); asked = 170667 on 1000 bases lands exactly on 256 per base
    for cur, asked, bases, literal in ((4, 0, 1000, 6), (4, 3999, 1000, 6), (4, 4000, 1000, 6), (4, 4001, 1000, 7), (4, 10000, 1000, 15), (4, 170000, 1000, 255), (4, 170667, 1000, 256),
                                       (4, 170668, 1000, 257), (254, 170667, 1000, 256), (255, 170667, 1000, 257), (9, 7, 1, 11), (2, 1 << 40, 1 << 20, 1572864)):
        assert max(cur + 2, (asked + asked // 2 + bases - 1) // bases) == literal
        case("rerun", [cur, asked, bases], literal)

    # ---- the fallback's doubling: std::min<uint64_t>(256, cur * 2)
    for cur, literal in ((4, 8), (127, 254), (128, 256), (129, 256), (256, 256)):
        assert min(256, cur * 2) == literal
        case("doubled", [cur], literal)

    # ---- maxSlices = (uint32_t)(L / 64 + 3); maxItems = (uint32_t)std::max<uint64_t>(8192, (L / 64 + 3) * 24); maxPending = 96;
    #      maxTrace = globalOrClip ? (uint32_t)(2 * L + 2 + 512) : (uint32_t)(L + L / 2 + 512); the default column store (int64_t)(3 * L + 4096)
    #      (8192 / 24 is no integer: 341 slices stay at the bound, 342 - L = 21696 - pass it)
    for length in (1, 511 * 32, 512 * 32, 21695, 21696, 50000):
        for g in (0, 1):
            case("sizes", [length, g], [u32(length // 64 + 3), u32(max(8192, (length // 64 + 3) * 24)), 96, u32(2 * length + 2 + 512) if g else u32(length + length // 2 + 512), 3 * length + 4096])
    assert cases[-1][1] == "784 18816 96 100514 154096" and cases[-2][1] == "784 18816 96 75512 154096"     # 50 000 bases
    assert cases[-12][1] == "3 8192 96 513 4099" and cases[-11][1] == "3 8192 96 516 4099"                  # one base
    assert cases[-6][1].split()[1] == "8192" and cases[-4][1].split()[1] == "8208"                           # 21 695 and 21 696 bases

    # ---- roundTraceBudget += 4 * ((globalOrClip ? 2 * len + 2 : len + len / 2) + 1024) over the reads
    for g, lens, literal in ((0, [1, 10001], 68200), (1, [1, 10001], 88224), (0, [], 0), (1, [50000], 404104)):
        assert sum(4 * ((2 * n + 2 if g else n + n // 2) + 1024) for n in lens) == literal
        case("roundtrace", [g] + lens, literal)

    # ---- workCapacity = 8 * n + 64
    for n, literal in ((0, 64), (1, 72), (10000, 80064)):
        case("workcap", [n], literal)

    # ---- scratchLanes = min(min(workCapacity + 64, 2 * n + 128), max(2048, min(65536 + 64, scratchBudget / (waveWords * 8)))): each bound from both sides
    def lanes(work_capacity, n, budget, wave_words):
        return min(min(work_capacity + 64, 2 * n + 128), max(2048, min(65536 + 64, budget // (wave_words * 8))))
    big = 1000000   # reads enough that the first min does not bind
    for args, literal in (((80064, 10000, 48 * GB, 100000), 20128), ((8 * big + 64, big, 48 * GB, 1000), 65600), ((8 * big + 64, big, 65599 * 8000, 1000), 65599),
                          ((8 * big + 64, big, 65600 * 8000, 1000), 65600), ((8 * big + 64, big, 65601 * 8000, 1000), 65600), ((8 * big + 64, big, 2047 * 8000, 1000), 2048),
                          ((8 * big + 64, big, 2048 * 8000, 1000), 2048), ((8 * big + 64, big, 2049 * 8000, 1000), 2049), ((72, 1, 48 * GB, 1000), 130), ((64, 0, 48 * GB, 1000), 128),
                          ((10, 1000, 48 * GB, 1000), 74), ((8 * 960 + 64, 960, 48 * GB, 100000), 2048), ((8 * 959 + 64, 959, 48 * GB, 100000), 2046), ((8 * 961 + 64, 961, 1, 100000), 2048)):
        assert lanes(*args) == literal
        case("lanes", args, literal)

    # ---- candidates per read and round:
    #      maxCand = 1;
    #      if (round > 0 && lastWork > 0) maxCand = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, (2 * n) / lastWork));
    #      if (round > 0 && lastWork < 8192) maxCand = 8;
    #      if (round > 0 && lastWork > 0) maxCand = (uint32_t)std::min<uint64_t>(maxCand, std::max<uint64_t>(1, (8 * n) / lastWork));
    def cand(rnd, last_work, n):
        c = 1
        if rnd > 0 and last_work > 0:
            c = min(8, max(1, (2 * n) // last_work))
        if rnd > 0 and last_work < 8192:
            c = 8
        if rnd > 0 and last_work > 0:
            c = min(c, max(1, (8 * n) // last_work))
        return c
    n = 10000
    for rnd, last_work, reads, literal in ((0, U32, n, 1), (0, 0, n, 1), (0, 100, n, 1), (1, 0, n, 8), (1, 1, n, 8), (1, 8191, n, 8), (1, 8192, n, 2), (1, 10000, n, 2), (1, 10001, n, 1),
                                           (1, 2 * n, n, 1), (1, 8 * n, n, 1), (7, 2500, n, 8), (4095, 2 * n, n, 1),
                                           (1, 0, 100, 8), (1, 1, 100, 8), (1, 100, 100, 8), (1, 101, 100, 7), (1, 2 * 100, 100, 4), (1, 8 * 100, 100, 1), (1, 8 * 100 + 1, 100, 1),
                                           (1, 8191, 4096, 4), (1, 8192, 4096, 1), (1, 8192, 4 * 8192, 8), (1, 8192, 4 * 8192 - 1, 7), (1, 8192, 8192, 2)):
        assert cand(rnd, last_work, reads) == literal
        case("cand", [rnd, last_work, reads], literal)

    # ---- blocks = std::min<uint32_t>((nWorkItems + team - 1) / team, (uint32_t)std::max<uint64_t>(1, (scratchLanes - 64) / team))
    for work, team, lanes_, literal in ((20000, 1, 20128, 20000), (20063, 1, 20128, 20063), (20064, 1, 20128, 20064), (20065, 1, 20128, 20064), (100, 8, 20128, 13), (1, 64, 130, 1),
                                        (1000, 64, 100, 1), (1000, 64, 64, 1), (1000, 2, 130, 33), (65, 2, 130, 33), (67, 2, 130, 33), (64, 2, 130, 32)):
        assert min((work + team - 1) // team, max(1, (lanes_ - 64) // team)) == literal
        case("blocks", [work, team, lanes_], literal)
    # ---- retryBlocks = std::min<uint32_t>(128, (uint32_t)std::max<uint64_t>(1, (scratchLanes - 64) / 2))
    for lanes_, literal in ((64, 1), (66, 1), (68, 2), (130, 33), (318, 127), (320, 128), (322, 128), (20128, 128)):
        assert min(128, max(1, (lanes_ - 64) // 2)) == literal
        case("retryblocks", [lanes_], literal)

    # ---- a read's alignment slots: limit = std::min<uint32_t>(1 << 16, std::max<uint32_t>(1, seeds)); if (cap >= limit) skip;
    #      next = (uint32_t)std::min<uint64_t>(limit, 4ull * cap); if (total + next >= 0xffffffffull) skip
    def grow(cap, seeds, total):
        limit = min(1 << 16, max(1, seeds))
        if cap >= limit:
            return "skip"
        nxt = min(limit, 4 * cap)
        return "skip" if total + nxt >= U32 else nxt
    for cap, seeds, total, literal in ((32, 1000, 320000, 128), (32, 100, 320000, 100), (32, 128, 0, 128), (32, 129, 0, 128), (32, 127, 0, 127), (31, 32, 0, 32), (32, 32, 0, "skip"),
                                       (33, 32, 0, "skip"), (32, 0, 0, "skip"), (1, 0, 0, "skip"), (1, 1, 0, "skip"), (1, 2, 0, 2), (16384, 100000, 0, 65536), (16383, 100000, 0, 65532),
                                       (65535, 100000, 0, 65536), (65535, 65536, 0, 65536), (65535, 65535, 0, "skip"), (65536, 100000, 0, "skip"), (65536, U32, 0, "skip"),
                                       (32, 1000, U32 - 129, 128), (32, 1000, U32 - 128, "skip"), (32, 1000, U32 - 127, "skip"), (32, 1000, U32, "skip")):
        assert grow(cap, seeds, total) == literal
        case("alngrow", [cap, seeds, total], literal)

    # ---- longTokenCount: the override, or streamBatchesDone > 0 && 2 * nReads + 128 <= LONG_WAVE_SLOTS (5120) && extensionsPerBase < 0.2 ? 2 : 1
    for forced, reads, done, share, literal in (("-", 2495, 1, "0.1", 2), ("-", 2496, 1, "0.1", 2), ("-", 2497, 1, "0.1", 1), ("-", 100, 0, "0.1", 1), ("-", 100, 7, "0.19", 2),
                                                ("-", 100, 1, "0.2", 1), ("-", 100, 1, "0.42", 1), (1, 100, 1, "0.1", 1), (2, 10000, 0, "0.42", 2), ("-", 0, 1, "0", 2)):
        assert (forced if forced != "-" else (2 if done > 0 and 2 * reads + 128 <= 5120 and float(share) < 0.2 else 1)) == literal
        case("tokens", [forced, reads, done, share], literal)
    return cases


def _build(tmp_path, flags=()):
    exe = str(tmp_path / "long_policy_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "long_policy_host", "long_policy_test.cpp"), "-o", exe], check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_sizing_and_growth_rules_are_the_expressions_the_pass_held(tmp_path, sanitize):
    """Per rule one value below, at and above every min / max bound: read lengths 1, 511 x 32, 512 x 32 and 50 000; lastWork 0, 1, 8191, 8192, 2 n and 8 n; a slot capacity at
    and just under its limit; slot totals around 0xffffffff - next; a request count that lands exactly on 256 cells per base. The second case is the same stand-alone program
    under the address and undefined-behaviour sanitizers."""
    exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if sanitize else ())
    cases = _cases()
    run = subprocess.run([exe], input="".join(c[0] + "\n" for c in cases), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    wrong = [(line, have, want) for (line, want), have in zip(cases, got) if have != want]
    assert not wrong, wrong


def test_every_rule_of_the_header_has_a_case():
    import re
    header = open(os.path.join(ROOT, "graphchainer_amd", "csrc", "host", "gc_long_policy.hpp")).read()
    program = open(os.path.join(ROOT, "tests", "long_policy_host", "long_policy_test.cpp")).read()
    functions = set(re.findall(r"^inline [\w:<>]+ (long\w+)\(", header, re.M))
    assert len(functions) == 14 and all("gc::" + f + "(" in program for f in functions), sorted(functions)
    rules = set(re.findall(r'rule == "(\w+)"', program))
    tried = {line.split()[0] for line, _ in _cases()}
    assert rules == tried and len(rules) == len(functions), (sorted(rules - tried), sorted(tried - rules))

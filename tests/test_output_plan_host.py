"""CPU-side check of csrc/host/gc_output_plan.hpp, the device output encoder's host rules: tests/output_plan_host/output_plan_test.cpp reads a rule and its arguments per
line and prints the rule's result. The expected values below restate the expressions batch/gc_batch_output.inc held inline before the header existed (quoted above each
group), not the header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = "-"   # ~0ull: an entry without an encoder job (a chained winner)


def _cases():
    """(input line, expected output line)."""
    cases = []

    def case(rule, args, want):
        cases.append((" ".join([rule] + [str(a) for a in args]), " ".join(str(w) for w in want)))

    # ---- the job order of one read:
    #      for (uint32_t k : gl.longSelected) items.push_back(Item { gl.longAlns[k].start, k });
    #      auto byStart = [](const Item& l, const Item& rr) { return l.start < rr.start; };
    #      std::sort(items.begin(), items.end(), byStart);   // src/Aligner.cpp:1003
    #      std::sort(items.begin(), items.end(), byStart);   // :1023 (an unstable sort may move ties even in a sorted list)
    #      for (const Item& it : items) jobAln.push_back(it.aln);
    #      Up to 16 items libstdc++'s std::sort is an insertion sort, so ties keep their order (Python's sorted is stable too); beyond 16 only distinct starts are tried here.
    def order(starts):
        items = list(range(len(starts)))
        for _ in range(2):
            items = sorted(items, key=lambda i: starts[i])
        return items
    seventeen = [(7 * i + 3) % 17 * 100 + 5 for i in range(17)]   # 17 distinct starts, neither sorted nor reversed: past the insertion-sort threshold
    assert len(set(seventeen)) == 17 and seventeen != sorted(seventeen) and seventeen != sorted(seventeen, reverse=True)
    for starts, literal in (([], []), ([40], [0]), ([500, 10, 300], [1, 2, 0]), ([10, 300, 500], [0, 1, 2]), ([500, 300, 10], [2, 1, 0]),
                            ([30, 10, 30, 20], [1, 3, 0, 2]),                                           # two equal starts
                            ([50, 20, 50, 10, 50], [3, 1, 0, 2, 4]),                                    # three equal starts
                            ([9, 4, 9, 4, 9, 1, 0, 7, 7, 3, 2, 8, 6, 5, 4, 9], [6, 5, 10, 9, 1, 3, 14, 13, 12, 7, 8, 11, 0, 2, 4, 15]),   # 16 alignments, ties of two, three and four
                            (seventeen, None), (sorted(seventeen), list(range(17))), (sorted(seventeen, reverse=True), list(range(16, -1, -1)))):
        assert len(starts) <= 16 or len(set(starts)) == len(starts)
        assert literal is None or order(starts) == literal, order(starts)
        case("order", starts, order(starts))

    # ---- the entries after the decision (n reads; glue[r].longFailed, glue[r].chainWins):
    #      readOutOff.assign(n + 1, 0); outEntries.clear(); outJobOfEntry.clear();
    #      for (uint64_t r = 0; r < n; r++) {
    #          readOutOff[r] = outEntries.size();
    #          if (gl.longFailed) continue;
    #          if (gl.chainWins) { outEntries.push_back(OutEntry { (uint32_t)r, 0, 1 }); outJobOfEntry.push_back(~0ull); continue; }
    #          for (uint64_t k = readJobBegin[r]; k < readJobBegin[r + 1]; k++) { outEntries.push_back(OutEntry { (uint32_t)r, jobAln[k], 0 }); outJobOfEntry.push_back(k); }
    #      }
    #      readOutOff[n] = outEntries.size();
    def entries(reads):
        """reads: (failed, wins, [alignment of every job]) per read."""
        read_out_off, out, job_of_entry, k = [], [], [], 0
        for r, (failed, wins, alns) in enumerate(reads):
            read_out_off.append(len(out))
            if not failed and wins:
                out.append((r, 0, 1))
                job_of_entry.append(NONE)
            elif not failed:
                for i, a in enumerate(alns):
                    out.append((r, a, 0))
                    job_of_entry.append(k + i)
            k += len(alns)
        read_out_off.append(len(out))
        return read_out_off, out, job_of_entry
    keep2, keep1, keep3 = (0, 0, [4, 1]), (0, 0, [2]), (0, 0, [5, 0, 3])
    for reads, literal in (
            ([], "0 | |"),                                                                        # an empty batch
            ([(1, 0, []), (1, 0, [3]), (1, 1, [2, 0])], "0 0 0 0 | |"),                           # every read failed (with and without jobs, one of them a winner besides)
            ([keep2, keep1, keep3], "0 2 3 6 | 0:4:0 0:1:0 1:2:0 2:5:0 2:0:0 2:3:0 | 0 1 2 3 4 5"),   # no winner: the identity
            ([(0, 1, [4, 1]), keep1, keep3], "0 1 2 5 | 0:0:1 1:2:0 2:5:0 2:0:0 2:3:0 | - 2 3 4 5"),   # the winner first
            ([keep2, keep1, (0, 1, [5, 0, 3])], "0 2 3 4 | 0:4:0 0:1:0 1:2:0 2:0:1 | 0 1 2 -"),         # last (three jobs dropped)
            ([keep2, (0, 1, [2]), keep3], "0 2 3 6 | 0:4:0 0:1:0 1:0:1 2:5:0 2:0:0 2:3:0 | 0 1 - 3 4 5"),   # in the middle: equal counts, no identity
            ([keep1, (0, 1, []), keep1], "0 1 2 3 | 0:2:0 1:0:1 2:2:0 | 0 - 1"),                      # a winner with no job of its own
            ([keep2, (1, 0, [7, 7]), keep1, (1, 0, []), keep1], "0 2 2 3 3 4 | 0:4:0 0:1:0 2:2:0 4:2:0 | 0 1 4 5"),   # failed reads between kept ones: their jobs are skipped
            ([(0, 0, []), keep1], "0 0 1 | 1:2:0 | 0"),                                             # a read without a selected alignment
            ([(0, 1, [9]), keep1], "0 1 2 | 0:0:1 1:2:0 | - 1")):                                   # the case allkept must refuse (below)
        read_out_off, out, job_of_entry = entries(reads)
        want = read_out_off + ["|"] + ["%d:%d:%d" % e for e in out] + ["|"] + job_of_entry
        assert " ".join(str(w) for w in want) == literal, " ".join(str(w) for w in want)
        case("entries", ["%d:%d:%s" % (f, w, ",".join(str(a) for a in alns) or "-") for f, w, alns in reads], want)

    # ---- compaction of one piece stream (nOut entries; the stream's job offsets jobOff[nJobs + 1]):
    #      for (uint64_t e = 0; e < nOut; e++) {
    #          res->out_corrected_off[e] = corrBytes;
    #          const uint64_t k = outJobOfEntry[e];
    #          if (k != ~0ull) corrBytes += hCorrOffsets[k + 1] - hCorrOffsets[k];
    #      }
    #      res->out_corrected_off[nOut] = corrBytes;
    #      (and the same for path, CIGAR and vg bytes with hOutOffsets[which * stride + k])
    def offsets(job_of_entry, job_off):
        at, off = 0, []
        for k in job_of_entry:
            off.append(at)
            if k != NONE:
                at += job_off[k + 1] - job_off[k]
        return off + [at, at]   # the last offset and the returned total
    job_off = [0, 5, 5, 12, 12, 12, 20]   # six jobs: 5, 0, 7, 0, 0 and 8 bytes
    for job_of_entry, offs, literal in (
            ([], [0], [0, 0]),                                                   # no entry
            ([0, 1, 2, 3, 4, 5], job_off, job_off + [20]),                       # the identity reproduces the job offsets (zero-length pieces among them)
            ([NONE, 1, 2, 3, 4, 5], job_off, [0, 0, 0, 7, 7, 7, 15, 15]),        # a winner's entry: begin = end; the total is the sum of the kept lengths
            ([0, 1, NONE, 5], job_off, [0, 5, 5, 5, 13, 13]),                    # jobs 2-4 dropped for one winner in the middle
            ([0, 1, 2, NONE], job_off, [0, 5, 5, 12, 12, 12]),                   # the winner last
            ([NONE, NONE], [0], [0, 0, 0, 0]),                                   # winners only, a batch without jobs
            ([2, 5], job_off, [0, 7, 15, 15]),
            ([1, 3, 4], job_off, [0, 0, 0, 0, 0])):                              # zero-length pieces only
        assert offsets(job_of_entry, offs) == literal, offsets(job_of_entry, offs)
        assert literal[-1] == sum(offs[k + 1] - offs[k] for k in job_of_entry if k != NONE)
        case("offsets", job_of_entry + ["/"] + offs, literal)

    # ---- the whole-blob copy is taken when
    #      bool allKept = nOut == nOutJobs;   // no chained winner: the device's blobs are the result's, job k is entry k
    #      for (uint64_t e = 0; e < nOut && allKept; e++) allKept = outJobOfEntry[e] == e;   // (a winner's one entry can stand where a read's one dropped job was: the counts alone do not tell)
    def all_kept(n_jobs, job_of_entry):
        return int(len(job_of_entry) == n_jobs and all(k == e for e, k in enumerate(job_of_entry)))
    for n_jobs, job_of_entry, literal in ((0, [], 1), (1, [0], 1), (6, [0, 1, 2, 3, 4, 5], 1),        # the identity
                                          (2, [NONE, 1], 0),     # read 0's one job dropped for its chained winner, read 1's kept: nOut == nOutJobs == 2
                                          (2, [0, NONE], 0),     # equal counts again, the winner last
                                          (6, [NONE, 2, 3, 4, 5], 0), (6, [0, 1, NONE], 0), (3, [0, 1, NONE, 2], 0), (0, [NONE], 0), (1, [NONE], 0),   # any winner
                                          (6, [0, 1, 2, 5], 0), (3, [0, 1], 0)):    # a failed read's jobs skipped: fewer entries than jobs
        assert all_kept(n_jobs, job_of_entry) == literal
        case("allkept", [n_jobs] + job_of_entry, [literal])
    return cases


def _build(tmp_path, flags=()):
    exe = str(tmp_path / "output_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "output_plan_host", "output_plan_test.cpp"), "-o", exe], check=True, timeout=600)
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_job_order_entries_and_compaction_are_the_expressions_the_batch_held(tmp_path, sanitize):
    """Job order: zero, one and three alignments, sorted and reversed starts, ties of two to four among at most 16 (insertion sort: the stable order), 17 distinct starts.
    Entries: empty, all failed, no winner, a winner first / last / in the middle, with no job and with three, failed reads between kept ones. Compaction: zero-length pieces,
    winners, identity. allKept: equal counts with a winner first and last. The second case is the same stand-alone program under the address and undefined-behaviour
    sanitizers."""
    exe = _build(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if sanitize else ())
    cases = _cases()
    run = subprocess.run([exe], input="".join(c[0] + "\n" for c in cases), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [line.strip() for line in run.stdout.split("\n")[:-1]]
    assert len(got) == len(cases)
    wrong = [(line, have, want) for (line, want), have in zip(cases, got) if have != want]
    assert not wrong, wrong


def test_every_rule_of_the_header_has_a_case():
    header = open(os.path.join(ROOT, "graphchainer_amd", "csrc", "host", "gc_output_plan.hpp")).read()
    program = open(os.path.join(ROOT, "tests", "output_plan_host", "output_plan_test.cpp")).read()
    functions = set(re.findall(r"^inline [\w:<>]+ (output\w+)\(", header, re.M))
    assert len(functions) == 4 and all("gc::" + f + "(" in program for f in functions), sorted(functions)
    rules = set(re.findall(r'rule == "(\w+)"', program))
    tried = {line.split()[0] for line, _ in _cases()}
    assert rules == tried and len(rules) == len(functions), (sorted(rules - tried), sorted(tried - rules))

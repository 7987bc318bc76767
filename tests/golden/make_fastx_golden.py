"""Pins the read loader to the REFERENCE'S OWN reader (run in the build container only; the outputs are committed).

What of the reference runs here: `FastQ::streamFastqFromFile` of its `src/fastqloader.h`, as the reader thread calls it
(`src/Aligner.cpp:167-187`, includeQuality == false). This script writes a small driver of our own (a `main` that calls it)
and a stub `zstr.hpp` of our own into a temporary directory, compiles the driver against the reference tree there, runs it
on the fixtures below and records what it yields. Only the inputs (tests/golden/fastx/*.{fa,fq}) and the recorded results
(tests/golden/fastx.expected.json) are committed; neither the reference's text nor the binary is.

The fixtures hold no empty FASTQ sequence or quality line and no FASTQ cut off inside a record: there the reference calls
line.back() on an empty string, which is undefined behaviour (DESIGN.md §9 defines it for this project).

    python tests/golden/make_fastx_golden.py [REFERENCE_TREE]
"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include "fastqloader.h"
static void hex(const std::string& s) { if (s.empty()) printf("-"); for (unsigned char c : s) printf("%02x", c); }
int main(int argc, char** argv)
{
	FastQ::streamFastqFromFile(argv[1], false, [](FastQ& read) { hex(read.seq_id); printf(" "); hex(read.sequence); printf("\n"); });
	return 0;
}
"""

ZSTR_STUB = r"""
#pragma once
#include <fstream>
namespace zstr { class ifstream : public std::ifstream { public: using std::ifstream::ifstream; }; }
"""


def fixtures():
    rng = random.Random(20260)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))   # noqa: E731
    wrap = lambda s, w: "".join(s[i:i + w] + "\n" for i in range(0, len(s), w))   # noqa: E731
    f = {
        # the eight cases of the loader's specification
        "case1.fa": ">a x y\nACGT\nAC\n\n>b\nGG",
        "case2_crlf.fa": ">a\r\nAC\r\nGT\r\n>b\r\n>c\r\nT\r\n",
        "case3_junk.fa": "junk\n>a\nAC\n",
        "case4.fq": "@a d\nACGT\n+\n@III\n@b\nGG\n+\nII",
        "case5.fq": "\nxx\n@a\r\nAC\r\n+\r\nII\r\n@b\nGG\n+\nII\n@c",
        "case6_empty.fa": "",
        "case6_empty.fq": "",
        "case7_header_only.fa": ">a",
        "case8_header_line.fa": ">a\n",
        # and more
        "width1.fa": ">one\n" + wrap(seq(97), 1) + ">two words\n" + wrap(seq(3), 1) + ">none\n>last\n" + wrap(seq(40), 1),
        "width60.fa": ">r0 first\n" + wrap(seq(1000), 60) + "\n>r1\n" + wrap(seq(60), 60) + ">r2\n" + wrap(seq(121), 60) + ">r3\n" + seq(59) + "\n",
        "lost_tail.fa": ">a\nACGT\nGGCC",
        "lost_header.fa": ">a\nACGT\n>b",
        "junk_then_header.fa": "junk\n>b",
        "cr_only_lines.fa": ">a\r\n\r\nAC\r\r\n\r\n>\r\nG\n",
        "quality_marks.fq": "@q0\n" + seq(50) + "\n+\n@" + "I" * 49 + "\n@q1 x\n" + seq(7) + "\n+q1 x\n>" + "I" * 6 + "\n@q2\n" + seq(130) + "\n+\n" + "@" * 130 + "\n",
        "crlf.fq": "@c0 one\r\n" + seq(33) + "\r\n+\r\n" + "I" * 33 + "\r\n@c1\r\n" + seq(64) + "\r\n+\r\n" + "#" * 64 + "\r\n",
        "ids.fa": ">id with blanks  and\ttabs\t\n" + seq(20) + "\n> leading blank\n" + seq(5) + "\n>\n" + seq(4) + "\n>>double\n" + seq(3) + "\n",
        "ids.fq": "@id with blanks  and\ttabs\t\n" + seq(20) + "\n+\n" + "I" * 20 + "\n@ leading blank\n" + seq(5) + "\n+\nIIIII\nskipped\n\n@@double\n" + seq(3) + "\n+\nIII\n",
        "not_a_header_first.fq": "ACGT\n+\n@a\nAC\n+\nII\n",
        "other_name.txt": ">a\nACGT\n",
    }
    return {k: v.encode("latin-1") for k, v in f.items()}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GC_REFERENCE_TREE", "")
    if not os.path.exists(os.path.join(ref, "src", "fastqloader.h")):
        sys.exit("give the reference tree (the directory that holds src/fastqloader.h)")
    out_dir = os.path.join(HERE, "fastx")
    os.makedirs(out_dir, exist_ok=True)
    expected = {}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
        open(os.path.join(tmp, "zstr.hpp"), "w").write(ZSTR_STUB)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + tmp, "-I" + os.path.join(ref, "src"), os.path.join(tmp, "driver.cpp"), "-o", exe])
        for name, data in sorted(fixtures().items()):
            path = os.path.join(out_dir, name)
            with open(path, "wb") as f:
                f.write(data)
            got = subprocess.run([exe, path], capture_output=True, text=True, check=True, timeout=60).stdout
            unhex = lambda h: "" if h == "-" else bytes.fromhex(h).decode("latin-1")   # noqa: E731
            records = [line.split(" ") for line in got.splitlines()]
            expected[name] = {"ids": [unhex(r[0]) for r in records], "sequences": [unhex(r[1]) for r in records]}
    with open(os.path.join(HERE, "fastx.expected.json"), "w") as f:
        json.dump(expected, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(expected)} fixtures, {sum(len(v['ids']) for v in expected.values())} records")


if __name__ == "__main__":
    main()

// Drives csrc/host/gc_output_plan.hpp (the device output encoder's host rules) on the CPU. Every input line is a case, a rule's name and its arguments ("-": no job, ~0):
//   order start...                        the starts of one read's selected alignments, alignment i at position i    -> the alignments in job order
//   entries failed:wins:aln,aln,...  ...  per read its two flags and the alignments of its jobs ("-": no job)       -> readOutOff... | read:aln:source ... | job ...
//   offsets job... / jobOff...            the entries' jobs, then the stream's job offsets (jobs + 1 of them)        -> the entries' offsets and, last, the total
//   allkept nJobs job...                  the number of jobs, then the entries' jobs                                 -> 0 or 1
// and one line of output per case. tests/test_output_plan_host.py holds the expected values; built with -fsanitize=address,undefined the same run has to stay clean.
#include "gc_output_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static uint64_t number(const std::string& t) { return t == "-" ? gc::OUTPUT_NO_JOB : strtoull(t.c_str(), nullptr, 10); }
static void print(uint64_t v, const char* after) { if (v == gc::OUTPUT_NO_JOB) printf("-%s", after); else printf("%llu%s", (unsigned long long)v, after); }
static std::vector<std::string> split(const std::string& s, char by)
{
	std::vector<std::string> parts;
	std::istringstream in(s);
	for (std::string item; std::getline(in, item, by);) parts.push_back(item);
	return parts;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty()) continue;
		std::istringstream in(line);
		std::string rule;
		in >> rule;
		std::vector<std::string> text;
		for (std::string item; in >> item;) text.push_back(item);
		if (rule == "order") {
			std::vector<gc::OutputJobItem> items;
			for (size_t i = 0; i < text.size(); i++) items.push_back(gc::OutputJobItem { (uint32_t)number(text[i]), (uint32_t)i });
			gc::outputJobOrder(items);
			for (size_t i = 0; i < items.size(); i++) printf("%s%u", i ? " " : "", items[i].aln);
			printf("\n");
		}
		else if (rule == "entries") {
			const uint64_t n = text.size();
			std::vector<uint8_t> failed, wins;
			std::vector<uint64_t> readJobBegin;
			std::vector<uint32_t> jobAln;
			for (const std::string& t : text) {
				const std::vector<std::string> f = split(t, ':');
				if (f.size() != 3) { fprintf(stderr, "a read is failed:wins:alignments: %s\n", line.c_str()); return 2; }
				failed.push_back(f[0] == "1"); wins.push_back(f[1] == "1");
				readJobBegin.push_back(jobAln.size());
				if (f[2] != "-") for (const std::string& a : split(f[2], ',')) jobAln.push_back((uint32_t)number(a));
			}
			readJobBegin.push_back(jobAln.size());
			std::vector<uint64_t> readOutOff { 77 }, jobOfEntry { 77 };   // (what an earlier batch left is replaced)
			std::vector<gc::OutputEntry> entries { gc::OutputEntry { 7, 7, 7 } };
			gc::outputEntries(n, [&](uint64_t r) { return failed[r] != 0; }, [&](uint64_t r) { return wins[r] != 0; }, readJobBegin.data(), jobAln.data(), readOutOff, entries, jobOfEntry);
			for (size_t i = 0; i < readOutOff.size(); i++) printf("%s%llu", i ? " " : "", (unsigned long long)readOutOff[i]);
			printf(" |");
			for (const gc::OutputEntry& e : entries) printf(" %u:%u:%u", e.read, e.aln, (unsigned)e.source);
			printf(" |");
			for (uint64_t k : jobOfEntry) { printf(" "); print(k, ""); }
			printf("\n");
		}
		else if (rule == "offsets") {
			std::vector<uint64_t> jobOfEntry, jobOff;
			bool second = false;
			for (const std::string& t : text) { if (t == "/") second = true; else (second ? jobOff : jobOfEntry).push_back(number(t)); }
			for (uint64_t k : jobOfEntry) if (k != gc::OUTPUT_NO_JOB && k + 1 >= jobOff.size()) { fprintf(stderr, "a job beyond the offsets: %s\n", line.c_str()); return 2; }
			std::vector<uint64_t> entryOff(jobOfEntry.size() + 1, 77);
			const uint64_t total = gc::outputPieceOffsets(jobOfEntry.data(), jobOfEntry.size(), jobOff.data(), entryOff.data());
			for (uint64_t o : entryOff) print(o, " ");
			print(total, "\n");
		}
		else if (rule == "allkept") {
			if (text.empty()) { fprintf(stderr, "too few arguments: %s\n", line.c_str()); return 2; }
			std::vector<uint64_t> jobOfEntry;
			for (size_t i = 1; i < text.size(); i++) jobOfEntry.push_back(number(text[i]));
			printf("%d\n", (int)gc::outputAllKept(jobOfEntry.data(), jobOfEntry.size(), number(text[0])));
		}
		else { fprintf(stderr, "unknown rule: %s\n", line.c_str()); return 2; }
	}
	return 0;
}

// Drives csrc/host/gc_selection.hpp (SelectAlignments: the E cut-off, the three greedy comparators, the four schedule scorers, All) on the CPU. Every input line is
//   method graphSize readSize eCutoff n  start end score  (n triples)
// and gives one output line: the indices of the alignments kept, in the order they are returned. tests/test_graphaligner_model.py compares them with the selection of
// tests/graphaligner_model.py; built with -fsanitize=address,undefined the same run has to stay clean.
#include "gc_evalue.hpp"
#include "gc_selection.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
	const gc::EValueModel model(0.7);
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty()) continue;
		std::istringstream in(line);
		int method = 0;
		size_t graphSize = 0, readSize = 0, n = 0;
		double eCutoff = -1;
		if (!(in >> method >> graphSize >> readSize >> eCutoff >> n)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
		std::vector<gc::SelectItem> alignments(n);
		for (size_t i = 0; i < n; i++) if (!(in >> alignments[i].start >> alignments[i].end >> alignments[i].score)) { fprintf(stderr, "short line: %s\n", line.c_str()); return 2; }
		const std::vector<uint32_t> kept = gc::selectAlignments(alignments, method, graphSize, readSize, eCutoff, model);
		for (size_t i = 0; i < kept.size(); i++) printf(i ? " %u" : "%u", kept[i]);
		printf("\n");
	}
	return 0;
}

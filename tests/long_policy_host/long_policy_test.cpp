// Drives csrc/host/gc_long_policy.hpp (the whole-read pass's sizing and growth rules) on the CPU. Every input line is a case, a rule's name and its arguments in decimal:
//   firstcap L | cellbudget perBase len... | refused perBase cells cellBytes | rerun cur asked bases | doubled cur | sizes L globalOrClip | roundtrace globalOrClip len...
//   workcap n | lanes workCapacity n budget waveWords | cand round lastWork n | blocks nWork team lanes | retryblocks lanes | alngrow cap seeds total
//   tokens override|- n batchesDone extensionsPerBase
// and one line of output per case: the rule's value(s), "skip" for a read that gets no more slots. tests/test_long_policy_host.py holds the expected values; built with
// -fsanitize=address,undefined the same run has to stay clean.
#include "gc_long_policy.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

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
		std::vector<uint64_t> a;
		for (const std::string& t : text) a.push_back(t == "-" ? 0 : strtoull(t.c_str(), nullptr, 10));
		auto need = [&](size_t k) { if (a.size() < k) { fprintf(stderr, "too few arguments: %s\n", line.c_str()); exit(2); } };
		// (read lengths -> the offsets array the rules take)
		auto offsetsFrom = [&](size_t first) { std::vector<uint64_t> off(1, 0); for (size_t i = first; i < a.size(); i++) off.push_back(off.back() + a[i]); return off; };
		if (rule == "firstcap") { need(1); printf("%u\n", gc::longFirstAlnCap(a[0])); }
		else if (rule == "cellbudget") { need(1); const auto off = offsetsFrom(1); printf("%llu\n", (unsigned long long)gc::longCellBudget(off.data(), off.size() - 1, a[0])); }
		else if (rule == "refused") { need(3); printf("%d\n", (int)gc::longCellPoolRefused(a[0], a[1], a[2])); }
		else if (rule == "rerun") { need(3); printf("%llu\n", (unsigned long long)gc::longCellsPerBaseForRerun(a[0], a[1], a[2])); }
		else if (rule == "doubled") { need(1); printf("%llu\n", (unsigned long long)gc::longCellsPerBaseDoubled(a[0])); }
		else if (rule == "sizes") { need(2); const gc::LongExtendSizes s = gc::longExtendSizes(a[0], a[1] != 0); printf("%u %u %u %u %lld\n", s.maxSlices, s.maxItems, s.maxPending, s.maxTrace, (long long)s.defaultCols); }
		else if (rule == "roundtrace") { need(1); const auto off = offsetsFrom(1); printf("%llu\n", (unsigned long long)gc::longRoundTraceBudget(off.data(), off.size() - 1, a[0] != 0)); }
		else if (rule == "workcap") { need(1); printf("%llu\n", (unsigned long long)gc::longWorkCapacity(a[0])); }
		else if (rule == "lanes") { need(4); printf("%llu\n", (unsigned long long)gc::longScratchLanes(a[0], a[1], a[2], a[3])); }
		else if (rule == "cand") { need(3); printf("%u\n", gc::longCandidatesPerRead((int)a[0], (uint32_t)a[1], a[2])); }
		else if (rule == "blocks") { need(3); printf("%u\n", gc::longRoundBlocks((uint32_t)a[0], (uint32_t)a[1], a[2])); }
		else if (rule == "retryblocks") { need(1); printf("%u\n", gc::longRetryBlocks(a[0])); }
		else if (rule == "alngrow") { need(3); const std::optional<uint32_t> next = gc::longAlnSlotGrowth((uint32_t)a[0], (uint32_t)a[1], a[2]); if (next) printf("%u\n", *next); else printf("skip\n"); }
		else if (rule == "tokens") {
			need(4);
			const std::optional<int> forced = text[0] == "-" ? std::nullopt : std::optional<int>((int)a[0]);
			printf("%d\n", gc::longTokenCount(forced, a[1], a[2], strtod(text[3].c_str(), nullptr)));
		}
		else { fprintf(stderr, "unknown rule: %s\n", line.c_str()); return 2; }
	}
	return 0;
}

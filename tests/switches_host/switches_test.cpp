// Drives csrc/host/gc_switches.hpp (gc::Switches::fromEnvironment: every GC_* variable's parsing rule) on the CPU. Every input line is a case:
//   NAME=VALUE NAME=VALUE ...     (a lone "-": nothing set; "NAME=" sets the empty string)
// Every GC_* variable is removed from the environment, the line's are set, and the snapshot is printed as one line of field=value ("unset" for an
// empty optional). tests/test_switches_host.py holds the expected values; built with -fsanitize=address,undefined the same run has to stay clean.
#include "gc_switches.hpp"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

extern char** environ;

template <typename T> static std::string text(const std::optional<T>& v) { return v ? std::to_string(*v) : "unset"; }
static std::string text(const std::optional<double>& v) { char b[64] = "unset"; if (v) snprintf(b, sizeof b, "%g", *v); return b; }

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		if (line.empty()) continue;
		std::vector<std::string> stale;
		for (char** e = environ; *e; e++) if (!strncmp(*e, "GC_", 3)) stale.push_back(std::string(*e).substr(0, std::string(*e).find('=')));
		for (const std::string& name : stale) unsetenv(name.c_str());
		std::istringstream in(line);
		for (std::string item; in >> item;) {
			if (item == "-") continue;
			const size_t eq = item.find('=');
			if (eq == std::string::npos) { fprintf(stderr, "bad item: %s\n", item.c_str()); return 2; }
			setenv(item.substr(0, eq).c_str(), item.substr(eq + 1).c_str(), 1);
		}
		const gc::Switches s = gc::Switches::fromEnvironment();
		std::ostringstream out;
		out << "hostThreads=" << text(s.hostThreads) << " batchThreads=" << text(s.batchThreads) << " buildThreads=" << text(s.buildThreads) << " resultCacheMin=" << s.resultCacheMin
			<< " spinSync=" << s.spinSync << " syncPollUs=" << s.syncPollUs << " longToken=" << s.longToken << " shareLongScratch=" << s.shareLongScratch() << " onePassAtATime=" << s.onePassAtATime()
			<< " longTokens=" << text(s.longTokens) << " debugTimes=" << s.debugTimes << " debugEd=" << s.debugEd
			<< " hostAnchors=" << s.hostAnchors << " extLazy=" << s.extLazy << " extendSlab=" << s.extendSlab
			<< " hostStitch=" << s.hostStitch << " stitchClass=" << text(s.stitchClass) << " chainPlainScan=" << s.chainPlainScan << " edFirstK=" << text(s.edFirstK)
			<< " seederBuildOnHost=" << s.seederBuildOnHost << " buildReferenceContainers=" << s.buildReferenceContainers
			<< " testExtMaxItems=" << text(s.testExtMaxItems) << " testExtMaxPending=" << text(s.testExtMaxPending) << " testExtMaxTrace=" << text(s.testExtMaxTrace)
			<< " testExtRetryMaxItems=" << text(s.testExtRetryMaxItems) << " testLongMaxItems=" << text(s.testLongMaxItems) << " testLongMaxCols=" << text(s.testLongMaxCols)
			<< " testLongCellsPerBase=" << text(s.testLongCellsPerBase) << " testLongMaxAlignments=" << text(s.testLongMaxAlignments) << " testLongScratchGb=" << text(s.testLongScratchGb)
			<< " testStitchSetMax=" << text(s.testStitchSetMax) << " testStitchBfsCap=" << text(s.testStitchBfsCap) << " testSeedFilterBits=" << text(s.testSeedFilterBits)
			<< " testFailLong=" << text(s.testFailLong) << " testLongForceFallback=" << s.testLongForceFallback << " testLongRegCap=" << text(s.testLongRegCap)
			<< " testLongMaxBlocks=" << text(s.testLongMaxBlocks) << " testLongTeam=" << text(s.testLongTeam) << " testLongOrder=" << s.testLongOrder
			<< " testLongSpeculate=" << text(s.testLongSpeculate) << " testChainForceScratch=" << s.testChainForceScratch << " testPoolFirstGuess=" << text(s.testPoolFirstGuess)
			<< " testPoolShrinkFloor=" << s.testPoolShrinkFloor << " testResultCachePoison=" << s.testResultCachePoison << " testUploadSlice=" << s.testUploadSlice;
		printf("%s\n", out.str().c_str());
	}
	return 0;
}

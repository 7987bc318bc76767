// The seed store's two test switches as csrc/host/gc_switches.hpp reads them: per input line "-" or "NAME=value ..." the environment is set, Switches::fromEnvironment()
// is taken and the two fields are printed; then the variables are removed again.
#include "gc_switches.hpp"
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::vector<std::string> names;
		std::istringstream items(line);
		std::string item;
		while (items >> item) {
			if (item == "-") continue;
			const size_t eq = item.find('=');
			names.push_back(item.substr(0, eq));
			setenv(names.back().c_str(), item.substr(eq + 1).c_str(), 1);
		}
		const gc::Switches s = gc::Switches::fromEnvironment();
		std::cout << "testSeedfilePiece=" << s.testSeedfilePiece << " testSeedfileHashBits=" << s.testSeedfileHashBits << "\n";
		for (const std::string& n : names) unsetenv(n.c_str());
	}
	return 0;
}

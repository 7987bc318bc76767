// SelectAlignments (src/AlignmentSelection.{h,cpp}) over (alignmentStart, alignmentEnd, alignmentScore) triples: host code with no HIP dependency, so a CPU
// program can call it (tests/selection_host/selection_test.cpp). Doubles in the reference's operation order; alignmentIncompatible's cut-off is a float as there.
// The sorts run libstdc++'s std::sort over an index vector with the reference's comparators, so the unstable tie order is the reference's by construction.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace gc {

struct SelectItem { size_t start, end, score; };   // AlignmentItem::alignmentStart / alignmentEnd / alignmentScore

// SelectionMethod, src/AlignmentSelection.h:14-24 (the public header's GC_SELECT_* carry the same numbers)
enum SelectionMethod { SelectGreedyLength, SelectGreedyScore, SelectGreedyE, SelectScheduleInverseESum, SelectScheduleInverseEProduct, SelectScheduleScore, SelectScheduleLength, SelectAll };

// an overlap larger than 5 % of the shorter alignment (src/AlignmentSelection.cpp:9-31)
inline bool alignmentIncompatible(const SelectItem& left, const SelectItem& right)
{
	const float overlapIncompatibleFractionCutoff = 0.05;
	auto minOverlapLen = std::min((left.end - left.start), (right.end - right.start)) * overlapIncompatibleFractionCutoff;
	size_t leftStart = left.start, leftEnd = left.end, rightStart = right.start, rightEnd = right.end;
	if (leftStart > rightStart) { std::swap(leftStart, rightStart); std::swap(leftEnd, rightEnd); }
	int overlap = 0;
	if (leftEnd > rightStart) overlap = leftEnd - rightStart;
	return overlap > minOverlapLen;
}

// GreedySelectAlignments, src/AlignmentSelection.h:36-54: indices into `alignments`, in the order they are taken
template <typename Compare>
std::vector<uint32_t> greedySelect(const std::vector<SelectItem>& alignments, Compare better)
{
	std::vector<size_t> items;
	for (size_t i = 0; i < alignments.size(); i++) items.push_back(i);
	std::sort(items.begin(), items.end(), [&alignments, better](size_t left, size_t right) { return better(alignments[left], alignments[right]); });
	std::vector<uint32_t> result;
	for (auto i : items) {
		if (!std::any_of(result.begin(), result.end(), [&alignments, i](uint32_t existing) { return alignmentIncompatible(alignments[existing], alignments[i]); })) result.push_back((uint32_t)i);
	}
	return result;
}

// ScheduleSelectAlignments, src/AlignmentSelection.h:56-96: the best-scoring compatible set, from its last alignment backwards. (The reference reads items[0] of an
// empty list, which --E-cutoff can leave it with; an empty list gives an empty selection here.)
template <typename Scorer>
std::vector<uint32_t> scheduleSelect(const std::vector<SelectItem>& alignments, Scorer scorer)
{
	std::vector<uint32_t> result;
	if (alignments.empty()) return result;
	std::vector<size_t> items;
	for (size_t i = 0; i < alignments.size(); i++) items.push_back(i);
	std::sort(items.begin(), items.end(), [&alignments](size_t left, size_t right) { return alignments[left].end < alignments[right].end; });
	const size_t none = std::numeric_limits<size_t>::max();
	std::vector<size_t> backtrace(items.size(), none);
	std::vector<double> score(items.size(), 0);
	for (size_t i = 0; i < items.size(); i++) {
		double rawScore = scorer(alignments[items[i]]);
		score[i] = rawScore;
		for (size_t j = 0; j < i; j++) {
			if (alignmentIncompatible(alignments[items[i]], alignments[items[j]])) continue;
			if (score[j] + rawScore > score[i]) { backtrace[i] = j; score[i] = score[j] + rawScore; }
		}
	}
	size_t maxPos = 0;
	for (size_t i = 0; i < items.size(); i++) if (score[i] > score[maxPos]) maxPos = i;
	while (maxPos != none) { result.push_back((uint32_t)items[maxPos]); maxPos = backtrace[maxPos]; }
	return result;
}

// SelectAlignments, src/AlignmentSelection.cpp:53-99. EModel: gc::EValueModel (alignmentScore / evalue / keeps). Returns indices into `all`, in the order the
// reference returns the alignments: --E-cutoff first (list order kept), then the method over what is left.
template <typename EModel>
std::vector<uint32_t> selectAlignments(const std::vector<SelectItem>& all, int method, size_t graphSize, size_t readSize, double eCutoff, const EModel& model)
{
	std::vector<SelectItem> alignments;
	std::vector<uint32_t> origin;
	for (size_t i = 0; i < all.size(); i++) {
		if (!model.keeps(eCutoff, graphSize, readSize, all[i].end - all[i].start, all[i].score)) continue;
		alignments.push_back(all[i]);
		origin.push_back((uint32_t)i);
	}
	auto length = [](const SelectItem& a) { return a.end - a.start; };
	auto evalue = [&](const SelectItem& a) { return model.evalue(graphSize, readSize, length(a), a.score); };
	auto alnScore = [&](const SelectItem& a) { return model.alignmentScore(length(a), a.score); };
	std::vector<uint32_t> picked;
	switch (method) {
		case SelectGreedyLength:   // longer is better, after that lower score is better
			picked = greedySelect(alignments, [](const SelectItem& left, const SelectItem& right) {
				if ((left.end - left.start) > (right.end - right.start)) return true;
				if ((right.end - right.start) > (left.end - left.start)) return false;
				if (left.score < right.score) return true;
				return false;
			});
			break;
		case SelectGreedyScore: picked = greedySelect(alignments, [&](const SelectItem& left, const SelectItem& right) { return alnScore(left) > alnScore(right); }); break;
		case SelectGreedyE: picked = greedySelect(alignments, [&](const SelectItem& left, const SelectItem& right) { return evalue(left) < evalue(right); }); break;   // lower E-value is better
		case SelectScheduleInverseESum: picked = scheduleSelect(alignments, [&](const SelectItem& a) { return 1.0 / evalue(a); }); break;
		case SelectScheduleInverseEProduct: picked = scheduleSelect(alignments, [&](const SelectItem& a) { return -log(evalue(a)); }); break;
		case SelectScheduleScore: picked = scheduleSelect(alignments, [&](const SelectItem& a) { return alnScore(a); }); break;
		case SelectScheduleLength: picked = scheduleSelect(alignments, [](const SelectItem& a) { return (a.end - a.start) + 0.5 - 0.5 / (a.score); }); break;
		default:
		case SelectAll:
			for (size_t i = 0; i < alignments.size(); i++) picked.push_back((uint32_t)i);
			break;
	}
	for (uint32_t& i : picked) i = origin[i];
	return picked;
}

} // namespace gc

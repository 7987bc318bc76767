// The MUM / MEM index's suffix array built on the device (gc_mxm_index_open with GC_MXM_BUILD_DEVICE): what host/gc_mxm_build.hpp's mxmSuffixArray does, restated for the GPU.
// The order is the host builder's - separator < a < c < g < t, a suffix that is a prefix of another first, every position of the text - and all suffixes are distinct, so the
// result equals the host's element for element.
//   first key    k_sa_first_key: 21 letters at 3 bits from the codes in HBM (0 beyond the text, separator 1, letters 2..5: the host's key), one radix sort of (key, position)
//   groups       k_sa_place puts the sorted positions into their slots of the SA and marks the head of every run of equal keys with its slot; an inclusive max-scan turns
//                that into "slot of my group's first member", k_sa_rank writes it as rank[position] and flags the members of groups with more than one member; a
//                DeviceSelect keeps their slots: the active set
//   doubling     per round, over the active set only: k_sa_compose makes (group start << 32) | (i + h < n ? rank[i + h] + 1 : 0) for every active position, one radix sort
//                of the active (key, position) pairs; groups are contiguous slot ranges and the key's high half is the group start, so the sorted list maps onto the
//                ascending slot list in order (k_sa_place again). The new ranks are written (k_sa_rank) only after every key of the round has been composed - compose is a
//                launch of its own, the host builder stages them in `fresh` for the same reason. Then select, h doubles, and ONE host read per round: the active count.
// Every round is a global radix sort; the late rounds' tied groups are not sorted inside a wave (gc_stdsort_wave.hpp could) - on the texts measured the first sort is the
// cost and the rounds are few and small.
// Scratch, allocated here and freed before the call returns (only the SA stays): the codes (1 byte per letter), two key and two position buffers for the sorts' double
// buffers (16 + 8), the ranks (4) = 29 bytes per text letter, plus 8 bytes per letter still tied after the first sort (two slot lists) and hipCUB's temporary storage.
// The sorted-out halves of the double buffers hold the round's head slots, group slots and flags, so a round allocates nothing.
#include "gc_kernels.hpp"
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <vector>

namespace gcdev {

namespace {

constexpr uint32_t SA_KEY_LETTERS = 21;

__global__ void __launch_bounds__(256) k_sa_first_key(const uint8_t* __restrict__ codes, uint32_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ pos)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	uint64_t k = 0;
	for (uint32_t j = 0; j < SA_KEY_LETTERS && (uint64_t)i + j < n; j++) k |= (uint64_t)(codes[i + j] + 1u) << (60 - 3 * j);
	key[i] = k;
	pos[i] = i;
}

__global__ void __launch_bounds__(256) k_sa_compose(const uint32_t* __restrict__ slot, uint32_t m, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ rank, uint32_t n, uint64_t h,
	uint64_t* __restrict__ key, uint32_t* __restrict__ pos)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint32_t i = sa[slot[j]];
	const uint64_t second = (uint64_t)i + h < n ? (uint64_t)rank[i + h] + 1 : 0;
	key[j] = ((uint64_t)rank[i] << 32) | second;
	pos[j] = i;
}

// slot == nullptr: the first sort, item j belongs into slot j
__global__ void __launch_bounds__(256) k_sa_place(const uint32_t* __restrict__ slot, uint32_t m, const uint64_t* __restrict__ key, const uint32_t* __restrict__ pos, uint32_t* __restrict__ sa,
	uint32_t* __restrict__ headSlot)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	const uint32_t s = slot ? slot[j] : j;
	sa[s] = pos[j];
	headSlot[j] = (j == 0 || key[j] != key[j - 1]) ? s : 0u;   // (slots ascend, so the running maximum is the last head's)
}

__global__ void __launch_bounds__(256) k_sa_rank(uint32_t m, const uint64_t* __restrict__ key, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ groupSlot, uint32_t* __restrict__ rank,
	uint8_t* __restrict__ keep)
{
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= m) return;
	rank[pos[j]] = groupSlot[j];
	const uint64_t k = key[j];
	const bool head = j == 0 || key[j - 1] != k, last = j + 1 == m || key[j + 1] != k;
	keep[j] = (head && last) ? 0 : 1;
}

#define SA_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

struct Scratch {   // the build's allocations: freed when it goes, their peak counted
	std::vector<void*> live;
	uint64_t bytes = 0;
	hipError_t get(void** p, size_t n)
	{
		const size_t want = n ? n : 1;
		const hipError_t e = hipMalloc(p, want);
		if (e == hipSuccess) { live.push_back(*p); bytes += want; }
		return e;
	}
	~Scratch() { for (void* p : live) (void)hipFree(p); }
};

inline uint32_t blocksOf(uint32_t m) { return (m + 255u) / 256u; }

} // namespace

hipError_t launchMxmSuffixArray(hipStream_t q, const uint8_t* hostCodes, uint32_t n, uint32_t* sa, MxmSaBuild& info)
{
	info = MxmSaBuild {};
	if (!n) return hipSuccess;
	if (n >= 0x7fffffffu) return hipErrorInvalidValue;   // (MXM_DEVICE_BUILD_MAX: the caller refuses such a text by name before it comes here: hipCUB counts in int)
	Scratch scratch;
	StreamDrain drain { q };   // (declared after `scratch`: nothing is freed while a kernel of this build may still run)
	uint8_t* codes = nullptr;
	uint64_t *keyA = nullptr, *keyB = nullptr;
	uint32_t *posA = nullptr, *posB = nullptr, *rank = nullptr, *count = nullptr;
	SA_TRY(scratch.get((void**)&codes, n));
	SA_TRY(scratch.get((void**)&keyA, (size_t)n * 8));
	SA_TRY(scratch.get((void**)&keyB, (size_t)n * 8));
	SA_TRY(scratch.get((void**)&posA, (size_t)n * 4));
	SA_TRY(scratch.get((void**)&posB, (size_t)n * 4));
	SA_TRY(scratch.get((void**)&rank, (size_t)n * 4));
	SA_TRY(scratch.get((void**)&count, 256));
	int slotBits = 1;
	while (slotBits < 32 && (1ull << slotBits) < n) slotBits++;
	// hipCUB's temporary storage: every primitive is asked what it needs for this call's size before it runs, and the buffer grows when that is more than it has
	void* temp = nullptr;
	size_t tempBytes = 0;
	auto withTemp = [&](auto&& primitive) -> hipError_t {
		size_t need = 0;
		SA_TRY(primitive((void*)nullptr, need));
		if (need > tempBytes) {
			SA_TRY(hipStreamSynchronize(q));
			SA_TRY(scratch.get(&temp, need + 256));   // (the smaller one stays until the end: it is a few kilobytes)
			tempBytes = need;
		}
		need = tempBytes;
		return primitive(temp, need);
	};

	SA_TRY(hipMemcpyAsync(codes, hostCodes, n, hipMemcpyHostToDevice, q));
	hipLaunchKernelGGL(k_sa_first_key, dim3(blocksOf(n)), dim3(256), 0, q, (const uint8_t*)codes, n, keyA, posA);
	SA_TRY(hipGetLastError());

	// one refinement: the m (key, position) pairs in keyA / posA are sorted, placed into `slot` (nullptr: slots 0 .. m - 1), ranked, and the slots still tied come out in
	// nextSlot (nullptr: in the sorted-out key buffer, whose address is returned through tiedIn) with their number in mNext
	auto refine = [&](const uint32_t* slot, uint32_t m, int endBit, uint32_t* nextSlot, uint32_t** tiedIn, uint32_t& mNext) -> hipError_t {
		hipcub::DoubleBuffer<uint64_t> k(keyA, keyB);
		hipcub::DoubleBuffer<uint32_t> p(posA, posB);
		SA_TRY(withTemp([&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k, p, (int)m, 0, endBit, q); }));
		const uint64_t* key = k.Current();
		const uint32_t* pos = p.Current();
		uint32_t *headSlot = (uint32_t*)k.Alternate(), *groupSlot = headSlot + m;   // (8 m bytes: two arrays of m words)
		uint8_t* keep = (uint8_t*)p.Alternate();
		hipLaunchKernelGGL(k_sa_place, dim3(blocksOf(m)), dim3(256), 0, q, slot, m, key, pos, sa, headSlot);
		SA_TRY(hipGetLastError());
		SA_TRY(withTemp([&](void* t, size_t& b) { return hipcub::DeviceScan::InclusiveScan(t, b, (const uint32_t*)headSlot, groupSlot, hipcub::Max(), (int)m, q); }));
		hipLaunchKernelGGL(k_sa_rank, dim3(blocksOf(m)), dim3(256), 0, q, m, key, pos, (const uint32_t*)groupSlot, rank, keep);
		SA_TRY(hipGetLastError());
		if (slot) { SA_TRY(withTemp([&](void* t, size_t& b) { return hipcub::DeviceSelect::Flagged(t, b, slot, (const uint8_t*)keep, nextSlot, count, (int)m, q); })); }
		else {
			// (headSlot is read by nothing any more: the first sort's tied slots go there until their number is known)
			SA_TRY(withTemp([&](void* t, size_t& b) { return hipcub::DeviceSelect::Flagged(t, b, hipcub::CountingInputIterator<uint32_t>(0), (const uint8_t*)keep, headSlot, count, (int)m, q); }));
			*tiedIn = headSlot;
		}
		SA_TRY(hipMemcpyAsync(&mNext, count, 4, hipMemcpyDeviceToHost, q));
		return hipStreamSynchronize(q);
	};

	uint32_t m = 0, *tied = nullptr;
	SA_TRY(refine(nullptr, n, 63, nullptr, &tied, m));
	uint32_t *slotA = nullptr, *slotB = nullptr;
	if (m) {
		SA_TRY(scratch.get((void**)&slotA, (size_t)m * 4));
		SA_TRY(scratch.get((void**)&slotB, (size_t)m * 4));
		SA_TRY(hipMemcpyAsync(slotA, tied, (size_t)m * 4, hipMemcpyDeviceToDevice, q));
	}
	for (uint64_t h = SA_KEY_LETTERS; m; h *= 2) {
		if (h > 2ull * n) return hipErrorUnknown;   // (cannot happen: all suffixes differ within n letters)
		info.rounds++;
		hipLaunchKernelGGL(k_sa_compose, dim3(blocksOf(m)), dim3(256), 0, q, (const uint32_t*)slotA, m, (const uint32_t*)sa, (const uint32_t*)rank, n, h, keyA, posA);
		SA_TRY(hipGetLastError());
		uint32_t mNext = 0;
		SA_TRY(refine(slotA, m, 32 + slotBits, slotB, nullptr, mNext));
		if (mNext > m) return hipErrorUnknown;
		m = mNext;
		uint32_t* t = slotA; slotA = slotB; slotB = t;
	}
	info.scratchBytes = scratch.bytes;
	return hipSuccess;
}

} // namespace gcdev

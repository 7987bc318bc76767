// Seeds from GAM files (gc_seed_store_open; the reference's -s / --seeds-file: stream::for_each, src/stream.hpp:81-123, and the lambda at src/Aligner.cpp:1177-1180), the parts
// that compile for the host as well as for the device (tests/seedfile_host):
//   sfVarint        one base-128 varint with bounds: at most 10 bytes, bits beyond the 64th are dropped (protobuf's ReadVarint64)
//   sfDecode        one serialized vg::Alignment -> the SeedHit the reference's lambda builds from it, the span of its name and a status. Protobuf's rules: unknown fields are
//                   skipped by wire type, a scalar given twice keeps the last value, a singular sub-message given twice is merged, a repeated one is appended. So mapping(0) is
//                   the first `mapping` over all occurrences of `path`, its position the field-wise merge of every `position` inside that element, edit(0) that element's first
//                   `edit`. Every sub-message of the schema is walked, used or not: a damaged second mapping fails the message as it fails protobuf's parser.
//   sfNameHash      the 64-bit key a seed is stored under and a read is looked up with (FNV-1a and a finishing mix); the join compares the name bytes as well
// Field numbers: src/vg.proto (tests/vg_descriptor.py: FIELDS). Strings are bytes here: a name is not checked for UTF-8.
// A value gc_seed_hit cannot hold becomes one that k_seed_resolve or the join's checks refuse; nothing is clamped into range.
#pragma once
#include <cstdint>
#include "gc_seedhits_core.hpp"

#if defined(__HIPCC__)
#define GC_SF_HD __host__ __device__ __forceinline__
#else
#define GC_SF_HD inline
#endif

namespace gcdev {

enum SfStatus : uint32_t { SF_OK = 0, SF_NO_MAPPING = 1, SF_NO_EDIT = 2, SF_PARSE = 3 };

constexpr uint32_t SF_BLOCK = 256;                     // threads per block of every kernel
constexpr uint32_t SF_WAVE_TILE = 8192;                // decode: LDS bytes a wave stages its 64 messages in
constexpr uint32_t SF_WAVES = SF_BLOCK / 64;

struct SfSeed {
	SeedHit hit;
	uint32_t nameStart, nameLen;   // the name's bytes inside the message (the last `name` field; 0, 0 when there is none)
	uint32_t status;
};

// false: the bytes end inside the varint, or it has more than 10 bytes
GC_SF_HD bool sfVarint(const uint8_t* p, uint32_t& at, uint32_t end, uint64_t& value)
{
	uint64_t v = 0;
	for (uint32_t i = 0; i < 10; i++) {
		if (at >= end) return false;
		const uint8_t b = p[at++];
		if (i < 9) v |= (uint64_t)(b & 0x7f) << (7 * i); else v |= (uint64_t)(b & 1) << 63;
		if (!(b & 0x80)) { value = v; return true; }
	}
	return false;
}

// One field's tag, and for wire type 2 the payload [at, at + len) checked against `end`. false: the message does not parse
struct SfField { uint32_t number, wire; uint64_t value; uint32_t len; };
GC_SF_HD bool sfField(const uint8_t* p, uint32_t& at, uint32_t end, SfField& f)
{
	uint64_t tag = 0;
	if (!sfVarint(p, at, end, tag)) return false;
	f.number = (uint32_t)(tag >> 3);
	f.wire = (uint32_t)(tag & 7);
	f.value = 0; f.len = 0;
	if (f.number == 0) return false;
	if (f.wire == 0) return sfVarint(p, at, end, f.value);
	if (f.wire == 1) { if (end - at < 8) return false; at += 8; return true; }
	if (f.wire == 5) { if (end - at < 4) return false; at += 4; return true; }
	if (f.wire != 2) return false;                     // groups (3, 4) and the two unassigned types
	uint64_t len = 0;
	if (!sfVarint(p, at, end, len)) return false;
	if (len > (uint64_t)(end - at)) return false;
	f.len = (uint32_t)len;
	return true;                                        // (the caller walks or skips the payload: at += len)
}

struct SfState {
	int64_t nodeId = 0, offset = 0;
	int32_t fromLength = 0, queryPosition = 0;
	bool reverse = false, haveMapping = false, haveEdit = false;
	uint32_t nameStart = 0, nameLen = 0;
};

// a message that is only checked: every field skipped by wire type (Edit and Position of a later mapping have no sub-messages)
GC_SF_HD bool sfSkipAll(const uint8_t* p, uint32_t at, uint32_t end)
{
	SfField f;
	while (at < end) { if (!sfField(p, at, end, f)) return false; at += f.len; }
	return true;
}

GC_SF_HD bool sfPosition(const uint8_t* p, uint32_t at, uint32_t end, SfState* s)
{
	SfField f;
	while (at < end) {
		if (!sfField(p, at, end, f)) return false;
		at += f.len;
		if (!s || f.wire != 0) continue;
		if (f.number == 1) s->nodeId = (int64_t)f.value;
		else if (f.number == 2) s->offset = (int64_t)f.value;
		else if (f.number == 4) s->reverse = f.value != 0;
	}
	return true;
}

GC_SF_HD bool sfEdit(const uint8_t* p, uint32_t at, uint32_t end, SfState* s)
{
	SfField f;
	while (at < end) {
		if (!sfField(p, at, end, f)) return false;
		at += f.len;
		if (s && f.wire == 0 && f.number == 1) s->fromLength = (int32_t)(uint32_t)f.value;
	}
	return true;
}

// s: null for a mapping behind the first one
GC_SF_HD bool sfMapping(const uint8_t* p, uint32_t at, uint32_t end, SfState* s)
{
	SfField f;
	while (at < end) {
		if (!sfField(p, at, end, f)) return false;
		if (f.wire == 2 && f.number == 1) { if (!sfPosition(p, at, at + f.len, s)) return false; }
		else if (f.wire == 2 && f.number == 2) {
			const bool first = s && !s->haveEdit;
			if (!sfEdit(p, at, at + f.len, first ? s : nullptr)) return false;
			if (first) s->haveEdit = true;
		}
		at += f.len;
	}
	return true;
}

GC_SF_HD bool sfPath(const uint8_t* p, uint32_t at, uint32_t end, SfState& s)
{
	SfField f;
	while (at < end) {
		if (!sfField(p, at, end, f)) return false;
		if (f.wire == 2 && f.number == 2) {
			const bool first = !s.haveMapping;
			s.haveMapping = true;
			if (!sfMapping(p, at, at + f.len, first ? &s : nullptr)) return false;
		}
		at += f.len;
	}
	return true;
}

// the message is p[0, len); p may point into LDS or into global memory
GC_SF_HD SfSeed sfDecode(const uint8_t* p, uint32_t len)
{
	SfState s;
	SfSeed out {};
	out.status = SF_PARSE;
	uint32_t at = 0;
	SfField f;
	while (at < len) {
		if (!sfField(p, at, len, f)) return out;
		if (f.wire == 2 && f.number == 2) { if (!sfPath(p, at, at + f.len, s)) return out; }
		else if (f.wire == 2 && f.number == 3) { s.nameStart = at; s.nameLen = f.len; }
		else if (f.wire == 0 && f.number == 7) s.queryPosition = (int32_t)(uint32_t)f.value;
		at += f.len;
	}
	out.nameStart = s.nameStart; out.nameLen = s.nameLen;
	if (!s.haveMapping) { out.status = SF_NO_MAPPING; return out; }
	if (!s.haveEdit) { out.status = SF_NO_EDIT; return out; }
	out.status = SF_OK;
	// the reference's conversions to SeedHit's int and size_t fields, then to gc_seed_hit's 32 bits: what does not fit becomes 2^32 - 1, which no node and no read holds
	out.hit.nodeId = (int32_t)s.nodeId;
	out.hit.nodeOffset = s.offset < 0 || s.offset > 0xfffffffell ? 0xffffffffu : (uint32_t)s.offset;
	out.hit.seqPos = s.queryPosition < 0 ? 0xffffffffu : (uint32_t)s.queryPosition;
	out.hit.matchLen = (uint32_t)s.fromLength;
	out.hit.rawGoodness = (uint32_t)s.fromLength;
	out.hit.reverse = s.reverse ? 1u : 0u;
	return out;
}

// keepBits: GC_TEST_SEEDFILE_HASH_BITS (64: all)
GC_SF_HD uint64_t sfNameHash(const uint8_t* name, uint32_t len, uint32_t keepBits)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (uint32_t i = 0; i < len; i++) { h ^= name[i]; h *= 0x100000001b3ull; }
	h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
	return keepBits >= 64 ? h : h & ((1ull << keepBits) - 1);
}

GC_SF_HD bool sfSameName(const uint8_t* a, const uint8_t* b, uint32_t len)
{
	for (uint32_t i = 0; i < len; i++) if (a[i] != b[i]) return false;
	return true;
}

#if defined(__HIPCC__)
// ---- the device side (gc_seedfile.hip). What a store keeps in HBM per seed: the 24-byte record, 8 bytes of sorted hash, 4 of the sorted order, 12 of name reference
// (offset and length) and the name's bytes: 48 bytes and the name. The inflated text of a piece is freed once it is decoded.
struct SfStoreView {
	const SeedHit* hits;          // [n] in file order, files in command-line order
	const uint64_t* sortedHash;   // [n] ascending
	const uint32_t* order;        // [n] message of every sorted position: equal hashes in file order (a stable sort)
	const uint64_t* nameOff;      // [n] where the message's name lies in namePool
	const uint32_t* nameLen;      // [n]
	const uint8_t* namePool;
	uint32_t n;
	uint32_t hashBits;
};
size_t sfTempBytes(uint32_t nMessages, uint32_t nReads);
hipError_t sfDecodePiece(hipStream_t q, const uint8_t* piece, const uint32_t* msgOff, uint32_t nMessages, uint64_t firstMessage, uint32_t hashBits, SeedHit* hits, uint64_t* hash,
	uint32_t* nameStart, uint32_t* nameLen, unsigned long long* firstBad);
hipError_t sfScanNameLengths(hipStream_t q, void* temp, size_t tempBytes, const uint32_t* nameLen, uint32_t nMessages, uint32_t* nameOffLocal);
hipError_t sfCopyNames(hipStream_t q, const uint8_t* piece, const uint32_t* msgOff, const uint32_t* nameStart, const uint32_t* nameLen, const uint32_t* nameOffLocal, uint32_t nMessages,
	uint64_t poolAt, uint8_t* pool, uint64_t* nameOff);
hipError_t sfSortStore(hipStream_t q, void* temp, size_t tempBytes, const uint64_t* hash, uint32_t n, uint64_t* sortedHash, uint32_t* order, uint32_t* iota, uint32_t* distinct);
hipError_t sfJoinCount(hipStream_t q, const SfStoreView& s, const uint8_t* names, const uint64_t* nameOff, uint32_t nReads, uint32_t* first, uint64_t* count);
hipError_t sfJoinScan(hipStream_t q, void* temp, size_t tempBytes, const uint64_t* count, uint32_t nReads, uint64_t* off64);
hipError_t sfJoinGather(hipStream_t q, const SfStoreView& s, const uint8_t* names, const uint64_t* nameOff, uint32_t nReads, const uint32_t* first, const uint64_t* off64, const uint64_t* readOff,
	SeedHit* hits, uint32_t* readHitOff, unsigned long long* badLen, unsigned long long* badGoodness);
#endif

} // namespace gcdev

// The framing of a seeds file (the loop of stream::for_each, src/stream.hpp:93-116) over inflated bytes that arrive in any pieces: groups of `varint64 count` and count x
// (`varint32 size`, size bytes). A first count of 0 ends the file at once (:97), a later one is an empty group (:116), a size of 0 gives no message (:109), and reading ends
// where no further count begins. Defined here: a count or size cut by the end of the stream, a varint of more than 10 bytes and a message cut by the end are errors.
// The messages' bytes are gathered back to back into a piece with their offsets; a piece is handed on once it holds pieceBytes or more and ends with a message, so a
// message longer than a piece makes the piece grow and nobody ever holds a whole file. Standard library only: tests/seedfile_host builds it without HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

namespace gc {

struct SeedFileError : std::runtime_error { using std::runtime_error::runtime_error; };

class SeedFileFramer {
public:
	// sink(bytes, byte count, msgOff [n + 1] into bytes, n, index of the piece's first message among the file's non-empty ones)
	using Sink = std::function<void(const uint8_t*, size_t, const uint32_t*, uint32_t, uint64_t)>;
	static constexpr size_t PIECE_MOST = 0xfffffff0u;   // offsets inside a piece are 32 bits

	SeedFileFramer(size_t pieceBytes, Sink sink) : pieceBytes_(pieceBytes ? pieceBytes : 1), sink_(std::move(sink)) { off_.push_back(0); }

	uint64_t messages() const { return messages_; }        // size-prefixed messages seen, the empty ones among them
	uint64_t seeds() const { return seeds_; }              // ... that were not empty

	void push(const uint8_t* data, size_t n)
	{
		size_t at = 0;
		while (at < n && !done_) {
			if (state_ == BODY) {
				const size_t take = std::min<size_t>(n - at, left_);
				if (piece_.size() + take > PIECE_MOST) throw SeedFileError("a message of 2^32 - 16 bytes or more at byte " + std::to_string(pos_ + at));
				piece_.insert(piece_.end(), data + at, data + at + take);
				at += take; left_ -= take;
				if (!left_) endMessage();
				continue;
			}
			const uint8_t b = data[at++];
			if (varBytes_ == 10) throw SeedFileError(std::string("a ") + (state_ == COUNT ? "count" : "size") + " of more than 10 bytes at byte " + std::to_string(pos_ + at - 1 - varBytes_));
			if (varBytes_ < 9) var_ |= (uint64_t)(b & 0x7f) << (7 * varBytes_); else var_ |= (uint64_t)(b & 1) << 63;
			varBytes_++;
			if (b & 0x80) continue;
			const uint64_t v = var_;
			var_ = 0; varBytes_ = 0;
			if (state_ == COUNT) {
				if (!v && firstCount_) { done_ = true; break; }
				firstCount_ = false;
				remaining_ = v;
				if (remaining_) state_ = SIZE;
			} else {
				messages_++;
				left_ = (uint32_t)v;                         // ReadVarint32 keeps the low 32 bits
				if (left_) { state_ = BODY; } else { remaining_--; if (!remaining_) state_ = COUNT; }
			}
		}
		pos_ += n;
	}

	// the stream has ended
	void finish()
	{
		if (!done_) {
			if (state_ == BODY) throw SeedFileError("message " + std::to_string(seeds_) + " runs past the end of the stream (" + std::to_string(left_) + " bytes missing)");
			if (varBytes_) throw SeedFileError(std::string("a ") + (state_ == COUNT ? "count" : "size") + " is cut by the end of the stream at byte " + std::to_string(pos_ - varBytes_));
			if (state_ == SIZE) throw SeedFileError("a group's count runs past the end of the stream (" + std::to_string(remaining_) + " messages missing at byte " + std::to_string(pos_) + ")");
		}
		flush();
	}

private:
	enum State { COUNT, SIZE, BODY };

	void endMessage()
	{
		off_.push_back((uint32_t)piece_.size());
		seeds_++;
		remaining_--;
		state_ = remaining_ ? SIZE : COUNT;
		if (piece_.size() >= pieceBytes_) flush();
	}

	void flush()
	{
		if (off_.size() > 1) sink_(piece_.data(), piece_.size(), off_.data(), (uint32_t)(off_.size() - 1), firstOfPiece_);
		firstOfPiece_ = seeds_;
		piece_.clear();
		off_.assign(1, 0);
	}

	size_t pieceBytes_;
	Sink sink_;
	State state_ = COUNT;
	bool firstCount_ = true, done_ = false;
	uint64_t var_ = 0, remaining_ = 0, pos_ = 0, messages_ = 0, seeds_ = 0, firstOfPiece_ = 0;
	uint32_t varBytes_ = 0, left_ = 0;
	std::vector<uint8_t> piece_;
	std::vector<uint32_t> off_;
};

} // namespace gc

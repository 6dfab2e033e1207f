// The field slots of a streaming pipeline and the tickets that name their queries (pp_pipeline.hpp).  Plain C++17, no HIP: tests/cpp/test_ticket_table.cpp
// drives it alone.  A slot is free, in flight (submitted, its completion record not yet polled) or held (polled with release = 0: its plan stays readable
// by ticket until the ticket is released).  Every by-ticket entry of the pipeline asks resolve() / slot_of(), and a held slot becomes free in release() only.
#pragma once

#include <stdint.h>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace pph {

constexpr int kSlotBits = 20;                 // pipeline list / ring entries: field slot in the low bits, the slot's generation above
constexpr uint32_t kSlotMask = (1u << kSlotBits) - 1u;
constexpr uint32_t kGenMask = (1u << (31 - kSlotBits)) - 1u; // (entries are non-negative int32)

class TicketTable {
public:
	enum class State : uint8_t { Free, InFlight, Held };
	struct Taken {
		int32_t slot = -1;  // -1: no room
		int32_t entry = 0;  // slot | generation << kSlotBits: what the slot lists, the rings and the claim words carry
		uint64_t ticket = 0;
	};
	struct Resolved {
		std::vector<int32_t> slots; // of the tickets, in their order
		std::string error;          // not empty: names the first offending ticket (and slots is empty)
	};

	/// every slot free, slot 0 handed out first, tickets counted from 0
	void reset(int capacity)
	{
		free_.resize((size_t)capacity);
		for (int i = 0; i < capacity; i++)
			free_[(size_t)i] = capacity - 1 - i;
		ticketOfSlot_.assign((size_t)capacity, 0);
		state_.assign((size_t)capacity, State::Free);
		gen_.assign((size_t)capacity, 0u);
		slotOfTicket_.clear();
		nTickets_ = 0;
	}
	int free_slots() const { return (int)free_.size(); }
	uint64_t ticket_of(int32_t slot) const { return ticketOfSlot_[(size_t)slot]; }

	/// a free slot goes in flight under a new ticket; its generation (times the slot has been filled) runs 1 ... kGenMask, then 1 again, never 0
	Taken take()
	{
		Taken t;
		if (free_.empty())
			return t;
		t.slot = free_.back();
		free_.pop_back();
		uint32_t& gen = gen_[(size_t)t.slot];
		gen = gen >= kGenMask ? 1u : gen + 1u;
		t.entry = (int32_t)((uint32_t)t.slot | (gen << kSlotBits));
		t.ticket = nTickets_++;
		state_[(size_t)t.slot] = State::InFlight;
		ticketOfSlot_[(size_t)t.slot] = t.ticket;
		slotOfTicket_[t.ticket] = t.slot;
		return t;
	}
	/// the query in `slot` has ended: held for the caller, or (hold = false) released at once.  false: no such slot, or it is not in flight
	bool complete(int32_t slot, bool hold)
	{
		if (slot < 0 || (size_t)slot >= state_.size() || state_[(size_t)slot] != State::InFlight)
			return false;
		state_[(size_t)slot] = State::Held;
		return hold || release(ticketOfSlot_[(size_t)slot]);
	}
	/// the one place a held slot becomes free.  false: the ticket is not held
	bool release(uint64_t ticket)
	{
		const auto it = slotOfTicket_.find(ticket);
		if (it == slotOfTicket_.end() || state_[(size_t)it->second] != State::Held)
			return false;
		state_[(size_t)it->second] = State::Free;
		free_.push_back(it->second);
		slotOfTicket_.erase(it);
		return true;
	}
	/// slot of a held ticket, -1 otherwise
	int32_t slot_of(uint64_t ticket) const
	{
		const auto it = slotOfTicket_.find(ticket);
		return it == slotOfTicket_.end() || state_[(size_t)it->second] != State::Held ? -1 : it->second;
	}
	/// the slots of n tickets that must all be held (and, with rejectDuplicates, distinct); `verb` says what the caller does with held queries
	/// ("post-processed", "re-validated", ...).  Changes nothing.
	Resolved resolve(int n, const uint64_t* tickets, const char* verb, bool rejectDuplicates) const
	{
		Resolved r;
		std::unordered_set<uint64_t> seen;
		r.slots.reserve((size_t)n);
		for (int i = 0; i < n && r.error.empty(); i++) {
			const auto refuse = [&](const std::string& why) { r.error = "ticket " + std::to_string(tickets[i]) + why; };
			const auto it = slotOfTicket_.find(tickets[i]);
			if (it == slotOfTicket_.end())
				refuse(" is unknown or already released");
			else if (state_[(size_t)it->second] != State::Held)
				refuse(std::string(" is still in flight (or was not polled with release = 0): only completed, held queries are ") + verb);
			else if (rejectDuplicates && !seen.insert(tickets[i]).second)
				refuse(" is given twice");
			else
				r.slots.push_back(it->second);
		}
		if (!r.error.empty())
			r.slots.clear();
		return r;
	}

private:
	std::vector<int32_t> free_;
	std::vector<uint64_t> ticketOfSlot_;
	std::vector<State> state_;
	std::vector<uint32_t> gen_; // times the slot has been filled: tags its list / ring entries and its claim word
	std::unordered_map<uint64_t, int32_t> slotOfTicket_;
	uint64_t nTickets_ = 0;
};

} // namespace pph

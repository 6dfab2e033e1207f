// The streaming pipeline's slots and tickets (pathplanning_amd/csrc/pp_ticket_table.hpp) alone: no GPU, no library.  Built with the address and
// undefined-behaviour sanitizers by pathplanning_amd/build.py (build_ticket_table_test) and run by tests/test_ticket_table_host.py; exit status 0 = every case held.
#include "pp_ticket_table.hpp"

#include <cstdio>
#include <cstdlib>

using pph::TicketTable;

#define CHECK(cond)                                                              \
	do {                                                                         \
		if (!(cond)) {                                                           \
			fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
			exit(1);                                                             \
		}                                                                        \
	} while (0)

static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

/// what a refusal must not change: the free count and every ticket's slot_of
struct Snapshot {
	int free;
	std::vector<int32_t> slotOf;
	Snapshot(const TicketTable& t, uint64_t tickets) : free(t.free_slots())
	{
		for (uint64_t k = 0; k < tickets; k++)
			slotOf.push_back(t.slot_of(k));
	}
	bool operator==(const Snapshot& o) const { return free == o.free && slotOf == o.slotOf; }
};

int main()
{
	TicketTable t;
	t.reset(4);
	CHECK(t.free_slots() == 4);

	// slots come out 0, 1, 2, 3 with tickets 0 ... 3 and generation 1; a fifth take finds no room and changes nothing
	for (int i = 0; i < 4; i++) {
		const TicketTable::Taken k = t.take();
		CHECK(k.slot == i && k.ticket == (uint64_t)i);
		CHECK(k.entry == (int32_t)((uint32_t)i | (1u << pph::kSlotBits)));
		CHECK(t.ticket_of(i) == (uint64_t)i);
		CHECK(t.slot_of(k.ticket) == -1); // in flight, not held
	}
	CHECK(t.free_slots() == 0);
	CHECK(t.take().slot == -1);
	CHECK(t.free_slots() == 0 && t.slot_of(4) == -1);

	// complete: only a slot in flight; held slots answer slot_of
	CHECK(!t.complete(-1, true) && !t.complete(4, true));
	CHECK(t.complete(1, true));
	CHECK(t.slot_of(1) == 1);
	CHECK(!t.complete(1, true)); // held
	CHECK(t.slot_of(1) == 1 && t.free_slots() == 0);
	CHECK(!t.release(0));        // in flight: not released
	CHECK(!t.release(77));       // unknown
	CHECK(t.free_slots() == 0);

	// complete(hold) then release gives the slot back; the next take reuses it with the generation advanced and a new ticket
	CHECK(t.release(1));
	CHECK(t.free_slots() == 1 && t.slot_of(1) == -1);
	CHECK(!t.release(1));        // released already
	CHECK(!t.complete(1, true)); // free
	CHECK(t.free_slots() == 1);
	{
		const TicketTable::Taken k = t.take();
		CHECK(k.slot == 1 && k.ticket == 4);
		CHECK(k.entry == (int32_t)(1u | (2u << pph::kSlotBits)));
		CHECK(t.slot_of(4) == -1 && t.slot_of(1) == -1);
	}
	// complete without hold frees at once
	CHECK(t.complete(3, false));
	CHECK(t.free_slots() == 1 && t.slot_of(3) == -1 && !t.release(3));

	// now: ticket 0 in flight (slot 0), 1 released, 2 in flight (slot 2), 3 released, 4 in flight (slot 1).  Hold 0 and 2.
	CHECK(t.complete(0, true) && t.complete(2, true));
	{
		const uint64_t good[2] = { 2, 0 };
		const TicketTable::Resolved r = t.resolve(2, good, "post-processed", true);
		CHECK(r.error.empty() && r.slots == (std::vector<int32_t> { 2, 0 }));
		CHECK(t.resolve(0, nullptr, "post-processed", true).error.empty());
	}
	struct Refusal {
		uint64_t tickets[3];
		bool distinct;
		const char* what;
	};
	const Refusal refusals[] = {
		{ { 0, 99, 4 }, true, "ticket 99 is unknown or already released" },  // unknown (in front of one in flight: the FIRST offender is named)
		{ { 0, 4, 99 }, true, "ticket 4 is still in flight (or was not polled with release = 0): only completed, held queries are re-validated" },
		{ { 2, 1, 4 }, false, "ticket 1 is unknown or already released" },   // released
		{ { 2, 0, 2 }, true, "ticket 2 is given twice" },
	};
	for (const Refusal& f : refusals) {
		const Snapshot before(t, 6);
		const TicketTable::Resolved r = t.resolve(3, f.tickets, "re-validated", f.distinct);
		CHECK(r.error == f.what);
		CHECK(r.slots.empty());
		CHECK(Snapshot(t, 6) == before);
	}
	{
		// without duplicate rejection a repeated ticket is served twice
		const uint64_t twice[3] = { 2, 0, 2 };
		const TicketTable::Resolved r = t.resolve(3, twice, "read", false);
		CHECK(r.error.empty() && r.slots == (std::vector<int32_t> { 2, 0, 2 }));
		// the verb is the caller's
		const uint64_t flying[1] = { 4 };
		CHECK(contains(t.resolve(1, flying, "read", false).error, "held queries are read"));
	}

	// one slot through kGenMask + 2 fills: the generation runs 1 ... kGenMask, then 1 again, never 0, and the entry stays a non-negative int32
	TicketTable g;
	g.reset(4);
	for (uint32_t fill = 1; fill <= pph::kGenMask + 2u; fill++) {
		const TicketTable::Taken k = g.take();
		CHECK(k.slot == 0 && k.ticket == (uint64_t)(fill - 1));
		CHECK(k.entry >= 0);
		const uint32_t gen = (uint32_t)k.entry >> pph::kSlotBits;
		CHECK(((uint32_t)k.entry & pph::kSlotMask) == 0u);
		CHECK(gen == (fill <= pph::kGenMask ? fill : fill - pph::kGenMask));
		CHECK(gen != 0u && gen <= pph::kGenMask);
		CHECK(g.complete(0, true));
		CHECK(g.slot_of(k.ticket) == 0);
		CHECK(g.release(k.ticket));
		CHECK(g.slot_of(k.ticket) == -1 && g.free_slots() == 4);
	}
	printf("ticket table ok\n");
	return 0;
}

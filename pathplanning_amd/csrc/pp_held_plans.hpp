// pp_held_plans -- who holds finished plans, and the one host route by which a service reaches them.  Included by pp_planner.hip behind the kernels (it
// names their argument types) and in front of pp_planner and pp_pipeline, which both keep one buffer group per service.
//
// Finished plans (path records, Reeds-Shepp log, result record) are held by a batch planner, as queries 0 .. n-1 of its last batch, or by a pipeline, as
// the slots of held tickets.  A service over them -- post-processing, re-validation, the stamp, the locate call, the speed profile, the conflict call, the delay call without and with tracked movers, the broad phase, the timetable look-ups, the waits at stops, the retime call -- has one core (post_process_plans,
// revalidate_plans, stamp_plans, locate_plans, speed_profile_plans, conflict_plans, deconflict_plans, deconflict_tracks_plans, candidate_pairs_plans, timetable_plans, deconflict_waits_plans, retime_plans in pp_planner.hip) that takes a HeldPlans and goes through held_grow and held_run; its two extern "C"
// entries check what is the holder's own and describe the holder (batch_plans, pipe_plans).
#pragma once

#include <initializer_list>
#include <type_traits>
#include <unordered_map>

struct pp_planner;

namespace {

struct HeldPlans {
	pp_planner* pl = nullptr;              // the buffer set: paths, rsLogs, results, args
	hipStream_t stream = nullptr;          // the stream the call runs on and alone synchronises: the context's (batch planner), the control stream (pipeline)
	const pp_footprint* footprint = nullptr; // the holder's footprint, or none
	ppd::MapView ownView {};               // the view of the holder's own map its plans travel with when the service has no target map
	int n = 0;                             // plans of this call
	bool byTicket = false;                 // false: the identity over n queries (no slot list is copied, the kernel gets nullptr)
	const uint64_t* tickets = nullptr;     // by ticket: the call's tickets ...
	std::vector<int32_t> slots;            // ... and their resolved slots, in call order
	size_t rows = 0;                       // plans a buffer group is made to hold: the call's n, or a batch planner's maxBatch
	std::vector<pph::DeviceMem>* parked = nullptr; // null: outgrown buffers are freed at once; else the place they are parked while mayFree is false
	bool mayFree = true;                   // a pipeline frees nothing with queries in flight: hipFree waits for every stream of the device, i.e. for the grid

	Footprint foot() const { return footprint ? footprint->fp : Footprint {}; } // (n = 0: the point validator)
	std::string name(int i) const { return byTicket ? "ticket " + std::to_string(tickets[i]) : "query " + std::to_string(i); } // plan i in a refusal
};

/// a service without per-plan arguments
struct NoPlanArg {};

/// The buffers of one service: the slot list (by ticket only), the per-plan arguments, the result records, by the index of a plan in the call
template <typename Arg, typename Rec>
struct HeldBuffers {
	pph::Dev<int32_t> slots;
	pph::Dev<Arg> args;
	pph::Dev<Rec> out;
	size_t rows = 0; // plans they hold; 0 until every one of them exists
};

/// Post-processing's buffers and what it keeps of its last call.  A batch planner indexes them by query with a stride of `points`, a pipeline by the
/// compact index of a ticket in the last call's list.
struct PostGroup {
	pph::Dev<double> ratios, resampled, smoothed, edgeEnd;
	pph::Dev<uint8_t> cusp, optimise;
	HeldBuffers<NoPlanArg, pp_post_result> rec; // the slot list and the result records
	size_t samples = 0;  // samples the five sample buffers hold (58 bytes each); 0 until every one of them exists
	size_t edgeRows = 0; // plans edgeEnd holds
	int points = 0;     // the last call's max_points: its sample limit and the buffers' per-plan stride
	std::vector<pp_post_result> host;                  // the last call's results
	std::unordered_map<uint64_t, int32_t> indexOfTicket; // by ticket: tickets of the last call that are still held -> compact index

	PostBuffers buffers() const { return PostBuffers { ratios, resampled, smoothed, cusp, optimise, edgeEnd, rec.out }; }
	/// `count` samples from sample index `from` of the buffers to sample index `to` of the caller's arrays (those it wants), on stream s
	hipError_t copy_out(size_t from, size_t count, size_t to, double* sampledHost, uint8_t* cuspHost, double* smoothedHost, hipStream_t s) const
	{
		hipError_t e = hipSuccess;
		if (sampledHost && count)
			e = hipMemcpyAsync(sampledHost + to * 3, resampled + from * 3, count * 24, hipMemcpyDeviceToHost, s);
		if (cuspHost && count && e == hipSuccess)
			e = hipMemcpyAsync(cuspHost + to, cusp + from, count, hipMemcpyDeviceToHost, s);
		if (smoothedHost && count && e == hipSuccess)
			e = hipMemcpyAsync(smoothedHost + to * 3, smoothed + from * 3, count * 24, hipMemcpyDeviceToHost, s);
		return e;
	}
};

/// The speed profile's buffers: the records, and one row of max_samples (s, v, t) triples per plan, which the kernel also works in
struct SpeedGroup {
	HeldBuffers<SpeedArg, pp_speed_profile_result> rec;
	pph::Dev<double> rows;
	size_t samples = 0; // samples `rows` holds (24 bytes each)
	/// What the holder remembers of its most recent speed-profile call that returned PP_OK, for the services that read `rows` where the kernel left
	/// them (the conflict call): per plan its row and what the record said, once the call's stride and acceleration limits.  A batch planner keys the
	/// plans by query index, a pipeline by ticket, as PostGroup::indexOfTicket does; a later call replaces all of it, a released ticket loses its entry.
	struct Profile {
		int32_t row, status, nSamples;
	};
	std::unordered_map<uint64_t, Profile> profileOf;
	int maxSamples = 0;
	double aAcc = 0.0, aDec = 0.0;
};

/// The conflict call's buffers: per plan the slot list, the start time and profile row, and the trajectory record; the trajectory itself, one array per
/// component and plan-major (pp_conflicts.hpp); the pair list (absent when the call pairs every i < j) and the pair records
struct ConflictGroup {
	HeldBuffers<ConflictArg, pp_trajectory_result> rec;
	pph::Dev<double> traj;
	size_t doubles = 0; // doubles `traj` holds
	pph::Dev<int32_t> pairs;
	size_t listed = 0; // pairs `pairs` holds (8 bytes each)
	pph::Dev<pp_conflict_result> out;
	size_t pairRows = 0; // pair records `out` holds
};

/// What the delay call adds to the conflict call's buffers (it forms its extended trajectory in ConflictGroup's `rec` and `traj`, grown for n x (T + D)
/// columns): per plan its place in the level order, the start of its partner list and its decided delay; the lists of lower-index partners; the records
struct DelayGroup {
	pph::Dev<int32_t> members, offsets, delays;
	size_t vehicles = 0; // plans they hold (`offsets` one more)
	pph::Dev<int32_t> partners;
	size_t listed = 0; // partners `partners` holds (4 bytes each)
	pph::Dev<pp_delay_result> out;
	size_t rows = 0; // records `out` holds
};

/// What the delay call with tracked movers adds to the delay call's buffers: the track set as uploaded (offsets, radii, waypoint rows), the tracks' positions on
/// the lattice, one array per component and track-major (pp_tracks.hpp), and the (vehicle, track) records
struct TrackGroup {
	pph::Dev<int32_t> offsets;
	pph::Dev<double> radii;
	size_t tracks = 0; // tracks they hold (`offsets` one more)
	pph::Dev<double> waypoints;
	size_t rows = 0; // waypoint rows `waypoints` holds (24 bytes each)
	pph::Dev<double> samples;
	size_t doubles = 0; // doubles `samples` holds (16 bytes per track and lattice time)
	pph::Dev<pp_track_result> out;
	size_t records = 0; // records `out` holds
};

/// The broad phase's buffers (it forms its extended trajectory in ConflictGroup's `rec` and `traj`, as the delay call does): the boxes, one array per
/// component and box-major, then plan (pp_pairs.hpp); per plan the count of its row, the row's offset in the list (two more: the total and the plans
/// with a box) and whether it has a box; the pair list and the first box of every pair
struct PairGroup {
	pph::Dev<double> boxes;
	size_t doubles = 0; // doubles `boxes` holds (32 bytes per plan and box)
	pph::Dev<long long> counts, offsets;
	pph::Dev<int32_t> boxed;
	size_t plans = 0; // plans they hold (`offsets` two more)
	pph::Dev<int32_t> pairs, firstBox;
	size_t listed = 0; // pairs they hold (8 + 4 bytes each)
};

/// The timetable call's buffers: per plan the slot list, the profile row (a ConflictArg whose start time is not read) and the plan record; the values
/// looked up and their records; the stop lists, max_stops rows per plan
struct TimetableGroup {
	HeldBuffers<ConflictArg, pp_timetable_plan> rec;
	pph::Dev<double> values;
	pph::Dev<pp_timetable_result> results;
	size_t lookups = 0; // look-ups they hold (8 + 128 bytes each)
	pph::Dev<pp_timetable_stop> stops;
	size_t listed = 0; // stops `stops` holds (32 bytes each)
};

/// What the call with waits at stops adds to the delay call's buffers (it forms its extended trajectory in ConflictGroup's `rec` and `traj` and keeps its level
/// order and partner lists in DelayGroup's, as the delay call does): per plan the committed wait, the start-wait flag, the count of its places and the wait it
/// was given (what the vehicles below read); the places, max(max_places, 1) rows per plan; the records
struct WaitGroup {
	pph::Dev<pp_wait_fixed> fixed;
	pph::Dev<uint8_t> noStart;
	pph::Dev<int32_t> counts;
	pph::Dev<WaitState> states;
	pph::Dev<pp_wait_result> out;
	size_t vehicles = 0; // plans they hold
	pph::Dev<pp_wait_place> places;
	size_t listed = 0; // places `places` holds (64 bytes each)
};

/// The retime call's buffers: per plan the slot list (uploaded by held_run, not read by the kernel), the profile row (a ConflictArg whose start time is
/// not read) and the record; the start of each plan's holds in the call's list; the holds
struct RetimeGroup {
	HeldBuffers<ConflictArg, pp_retime_result> rec;
	pph::Dev<int32_t> offsets;
	size_t plans = 0; // plans `offsets` holds (one entry more)
	pph::Dev<pp_hold> holds;
	size_t listed = 0; // holds `holds` holds (16 bytes each)
};

/// Buffers that hold `capacity` units are made to hold `wanted` ({buffer, bytes}; 0 bytes: the holder does not use it).  A holder that may not free now
/// parks a buffer that has to grow, and the parked ones go when a call finds that it may.  The capacity is 0 until every buffer exists again: a failed
/// allocation must not leave a stale capacity behind.
inline hipError_t held_grow(const HeldPlans& h, size_t& capacity, size_t wanted, std::initializer_list<std::pair<pph::DeviceMem*, size_t>> buffers)
{
	if (h.mayFree && h.parked)
		h.parked->clear();
	if (capacity >= wanted)
		return hipSuccess;
	capacity = 0;
	for (const auto& [buffer, bytes] : buffers) {
		if (bytes == 0)
			continue;
		if (!h.mayFree && buffer->get())
			h.parked->emplace_back(std::move(*buffer));
		if (const hipError_t e = buffer->alloc(bytes))
			return e;
	}
	capacity = wanted;
	return hipSuccess;
}

template <typename Arg, typename Rec>
hipError_t held_grow(const HeldPlans& h, HeldBuffers<Arg, Rec>& b)
{
	return held_grow(h, b.rows, h.rows,
		{ { &b.slots, h.byTicket ? h.rows * 4 : 0 }, { &b.args, std::is_empty<Arg>::value ? 0 : h.rows * sizeof(Arg) }, { &b.out, h.rows * sizeof(Rec) } });
}

/// ... post-processing's sample and edge buffers, for max_points samples per plan; the last call's results go with buffers that are given up
inline hipError_t held_grow(const HeldPlans& h, PostGroup& g, int maxPoints, int maxPath)
{
	const size_t samples = h.rows * (size_t)maxPoints;
	if (g.samples < samples) {
		g.host.clear();
		g.indexOfTicket.clear();
	}
	if (const hipError_t e = held_grow(h, g.samples, samples,
			{ { &g.ratios, samples * 8 }, { &g.resampled, samples * 24 }, { &g.smoothed, samples * 24 }, { &g.cusp, samples }, { &g.optimise, samples } }))
		return e;
	return held_grow(h, g.edgeRows, h.rows, { { &g.edgeEnd, h.rows * (size_t)(maxPath + 1) * 8 } });
}

/// One kernel over the plans of `h`, and its h.n result records back: the service's buffers made large enough, the slot list up (by ticket), the per-plan
/// arguments up (`plans`, if the service has any), launch(slotsDev) -> hipError_t, the records down, and the holder's stream -- no other -- synchronised; then the
/// records to the caller (and into *keep, for a service that keeps them).  Legal on a pipeline with queries in flight: the row that finished a slot wrote its path
/// records, Reeds-Shepp log and result record BEFORE its completion record (finish() in pp_planner_rows.hpp), the host saw that record with an acquire load in
/// pp_pipeline_poll, and nothing writes the slot again until it is released and refilled.
template <typename Arg, typename Rec, typename Launch>
int held_run(const HeldPlans& h, HeldBuffers<Arg, Rec>& b, const std::vector<Arg>& plans, Rec* resultsHost, Launch launch, std::vector<Rec>* keep = nullptr)
{
	const size_t n = (size_t)h.n;
	hipStream_t s = h.stream;
	PP_HIP_TRY(held_grow(h, b));
	// (pageable sources: staged before the calls return)
	if (h.byTicket)
		PP_HIP_TRY(hipMemcpyAsync(b.slots, h.slots.data(), n * 4, hipMemcpyHostToDevice, s));
	if (!plans.empty())
		PP_HIP_TRY(hipMemcpyAsync(b.args, plans.data(), n * sizeof(Arg), hipMemcpyHostToDevice, s));
	PP_HIP_TRY(launch(h.byTicket ? (const int32_t*)b.slots : nullptr));
	std::vector<Rec> host(n);
	PP_HIP_TRY(hipMemcpyAsync(host.data(), b.out, n * sizeof(Rec), hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	if (resultsHost) // (a caller may not want them)
		std::copy(host.begin(), host.end(), resultsHost);
	if (keep)
		keep->swap(host);
	return PP_OK;
}

} // namespace

// Where can a lower-priority vehicle wait -- at its start, or at a stop its timetable already has -- so that it stays clear of those above it
// (include/pp_hip.h, "waits at stops that clear conflicts")?  Included by pp_planner.hip behind pp_timetable.hpp: k_wait_places reads the planner's
// PathRec / RsLogEntry / DevResult records through PostEdge / load_edge of pp_postprocess.hpp and the (s, v, t) rows where k_speed_profile_tickets
// left them; k_wait_level reads the EXTENDED trajectory k_trajectory_tickets writes (pp_conflicts.hpp, pp_deconflict.hpp) and the places, and nothing
// else of a plan.  Both read no map and write nothing but their own buffers.  The arrive column, the position under a wait, the place filter and the
// candidate order are pp_wait_rule.hpp's; stops are the timetable call's (ppm::is_stop, ppm::arrive_time); key, discs and separation are the delay
// call's.
//   k_wait_places  workgroup i (64 lanes) lists the places of plan i: slot slots[i] of a buffer set (slots == nullptr: slot i) with the start time and
//                  the profile rows of args[i].  Dynamic LDS as k_timetable_tickets: edgeS[maxPath] doubles, then edgeL[maxPath] doubles.
//                  1. lengths and S_e, k_timetable_tickets' step 1;  2. the wave walks the rows 64 at a time; a lane whose row stands forms the arrive
//                  column by binary search; a ballot of the qualifying lanes gives a place its ordinal (the count of the blocks before plus the
//                  qualifying lanes below), and the first maxPlaces write their record: no atomic, the same bytes on every run.  A fixed vehicle
//                  lists its one row (lane 0), or nothing: count -1 says that the row does not qualify.
//   k_wait_level   workgroup v (64 lanes) decides vehicle i = members[v] of one level: every partner j < i of its list was decided by an earlier
//                  launch on the same stream, and that order is the only synchronisation there is.  k_delay_level's scan, restated: candidates are
//                  wave-uniform, lanes take m = lane, lane + 64, ..., the vehicle's own position and each partner's go through ppw::source -- a column
//                  of the trajectory or the standing pose of a place record, which every lane loads from the same address -- a lane stops at its
//                  first time in conflict, one 64-bit min-reduction per candidate by xor-shuffles, lane 0 writes the record and the vehicle's state.
#pragma once

static_assert(sizeof(pp_wait_params) == 56, "pp_wait_params layout");
static_assert(sizeof(pp_wait_fixed) == 8, "pp_wait_fixed layout");
static_assert(sizeof(pp_wait_result) == 80, "pp_wait_result layout");
static_assert(sizeof(pp_wait_place) == 64, "pp_wait_place layout");

struct WaitCall { // what both kernels know of a call beside the lattice
	int D;          // the largest wait, in lattice steps
	int maxPlaces;  // places listed per free vehicle
	int stride;     // rows of the place array per vehicle: max(maxPlaces, 1)
	int reserved;
};

struct WaitState { // what a decided vehicle leaves for the vehicles below it
	int32_t kind;   // kWaitUnscheduled; ppw::kNoWait; ppw::kStart; else the slot of its place
	int32_t column; // the arrive column of that place
	int32_t steps;  // d
	int32_t reserved;
};
static_assert(sizeof(WaitState) == 16, "WaitState layout");

constexpr int kWaitLanes = 64;
constexpr int kWaitUnscheduled = -3;
constexpr int kWaitNoPlace = -1; // counts[i]: a fixed row that does not qualify

/// kFixed: the call has committed waits (`fixed` is an array); without them every vehicle is free and `fixed` is not read
template <bool kFixed>
__global__ void __launch_bounds__(kWaitLanes) k_wait_places(SearchArgs A, ConflictLattice L, WaitCall C, int nPlans, const int32_t* __restrict__ slots,
	const ConflictArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results,
	const double* __restrict__ rows, const pp_wait_fixed* __restrict__ fixed, pp_wait_place* __restrict__ places, int32_t* __restrict__ counts)
{
	extern __shared__ double waitLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = waitLds;             // [maxPath]: S_e at e - 1
	double* const edgeL = waitLds + A.maxPath; // [maxPath]: the length of edge e at e - 1
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const ConflictArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const double* const row = rows + (size_t)arg.row * (size_t)L.maxSamples * 3;
	pp_wait_place* const place = places + (size_t)q * (size_t)C.stride;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	const int fixedRow = kFixed ? fixed[q].row : ppw::kFree;
	if (arg.nSamples < 1 || arg.nSamples > L.maxSamples || res.r.status != 0 || nPath < 1 || nPath > A.maxPath) { // (k_trajectory_tickets' status -1)
		if (lane == 0)
			counts[q] = 0;
		return;
	}
	const int nEdges = nPath - 1, N = arg.nSamples;
	const long long kE = L.k0 - C.D, columns = (long long)L.T + C.D;
	// ---------------- 1: lengths, S_e
	for (int e = lane + 1; e <= nEdges; e += kWaitLanes)
		edgeL[e - 1] = load_edge(A, recs, nPath, e, rslog, nRsLog).length();
	__syncthreads();
	if (lane == 0) {
		double length = 0.0;
		for (int e = 1; e <= nEdges; e++) { // PushBack, path_composite.h:33-39
			edgeS[e - 1] = length;
			length += edgeL[e - 1];
		}
	}
	__syncthreads();
	// ---------------- 2: the places
	const unsigned long long lanesBelow = (1ull << lane) - 1;
	const bool isFixed = fixedRow != ppw::kFree;
	// (a fixed vehicle walks one block of one row, in lane 0; a start wait none)
	const int first = isFixed ? fixedRow : 0, end = isFixed ? (fixedRow >= 0 && fixedRow < N ? fixedRow + 1 : first) : N;
	int nPlaces = 0;
	for (int base = first; base < end; base += kWaitLanes) {
		const int j = base + lane;
		const bool stands = j < end && ppm::is_stop(row[3 * (size_t)j + 1]);
		double tArrive = 0.0;
		long long a = columns;
		if (stands) {
			tArrive = ppm::arrive_time(row, j, L.aAcc, L.aDec);
			a = ppw::arrive_column(kE, columns, L.dt, arg.tStart, tArrive);
		}
		const bool listed = stands && (isFixed ? ppw::fixed_qualifies(j, N, true, a, columns) : ppw::is_place(j, N, a, C.D, columns));
		const unsigned long long listing = __ballot(listed);
		const int ordinal = nPlaces + __popcll(listing & lanesBelow);
		if (listed && ordinal < C.stride && (isFixed || ordinal < C.maxPlaces)) {
			pp_wait_place pl {};
			pl.row = j;
			pl.column = (int32_t)a;
			pl.s = row[3 * (size_t)j];
			pl.t_arrive = tArrive;
			Pose p;
			if (nEdges == 0) {
				const PathRec only = recs[0];
				p = Pose { only.x, only.y, only.t };
			} else {
				const int e = ppl::edge_of(edgeS, nEdges, pl.s);
				p = load_edge(A, recs, nPath, e, rslog, nRsLog).interpolate(ppl::ratio_of(pl.s, edgeS[e - 1], edgeL[e - 1]));
			}
			pl.pose[0] = p.x;
			pl.pose[1] = p.y;
			pl.pose[2] = p.t;
			sincos(p.t, &pl.sin_theta, &pl.cos_theta);
			place[ordinal] = pl;
		}
		nPlaces += __popcll(listing);
	}
	if (lane == 0) {
		if (isFixed)
			counts[q] = fixedRow >= 0 && nPlaces == 0 ? kWaitNoPlace : nPlaces;
		else
			counts[q] = nPlaces < C.maxPlaces ? nPlaces : C.maxPlaces;
	}
}

/// Where the vehicle whose trajectory is x (component c at + c * component) is at column c under the wait (kind, a, d) whose place record is `place`:
/// false where it is absent
__device__ __forceinline__ bool wait_position(const double* x, size_t component, bool heading, int kind, int a, int d, const pp_wait_place* place, int c, double& px,
	double& py, double& sn, double& cs)
{
	const long long at = kind >= 0 ? ppw::source(c, a, d) : (kind == ppw::kStart ? ppw::source_start(c, d) : (long long)c);
	sn = 0.0;
	cs = 1.0;
	if (at == ppw::kStanding) {
		px = place->pose[0];
		py = place->pose[1];
		if (heading) {
			sn = place->sin_theta;
			cs = place->cos_theta;
		}
		return true;
	}
	px = x[(size_t)at];
	if (px != px) // (absent)
		return false;
	py = x[component + (size_t)at];
	if (heading) {
		sn = x[4 * component + (size_t)at];
		cs = x[5 * component + (size_t)at];
	}
	return true;
}

/// ... and its arc length there (lane 0, for the blocker's record)
__device__ __forceinline__ double wait_length(const double* x, size_t component, int kind, int a, int d, const pp_wait_place* place, int c)
{
	const long long at = kind >= 0 ? ppw::source(c, a, d) : (kind == ppw::kStart ? ppw::source_start(c, d) : (long long)c);
	return at == ppw::kStanding ? place->s : x[3 * component + (size_t)at];
}

/// kHeading: a disc of the footprint sits off the reference point, so the trajectory has its sin / cos components and a place's are read
template <bool kHeading>
__global__ void __launch_bounds__(kWaitLanes) k_wait_level(Footprint F, ConflictLattice L, WaitCall C, int nPlans, int nMembers, const int32_t* __restrict__ members,
	const int32_t* __restrict__ offsets, const int32_t* __restrict__ partners, const ConflictArg* __restrict__ args, const double* __restrict__ traj,
	const pp_trajectory_result* __restrict__ plans, const pp_wait_fixed* __restrict__ fixed, const uint8_t* __restrict__ noStart, const pp_wait_place* __restrict__ places,
	const int32_t* __restrict__ counts, WaitState* states, pp_wait_result* __restrict__ out)
{
	const int v = blockIdx.x, lane = threadIdx.x;
	if (v >= nMembers)
		return;
	const int i = members[v], D = C.D;
	pp_wait_result rec {}; // (every field zero)
	rec.place = ppw::kNoWait;
	rec.row = rec.wait_steps = rec.blocker = -1;
	const pp_wait_fixed fx = fixed ? fixed[i] : pp_wait_fixed { ppw::kFree, 0 };
	const bool isFixed = fx.row != ppw::kFree;
	const int count = counts[i];
	if (plans[i].status < 0 || count == kWaitNoPlace) {
		rec.status = plans[i].status < 0 ? -1 : -2;
		if (lane == 0) {
			states[i] = WaitState { kWaitUnscheduled, 0, 0, 0 };
			out[i] = rec;
		}
		return;
	}
	const size_t columns = (size_t)L.T + (size_t)D, component = (size_t)nPlans * columns;
	const double* const xi = traj + (size_t)i * columns; // component c at + c * component
	const pp_wait_place* const mine = places + (size_t)i * (size_t)C.stride;
	constexpr bool heading = kHeading;
	const int pFirst = offsets[i], pEnd = offsets[i + 1];
	// the candidates: a free vehicle's d = 0, then for d = 1 .. D the start (if it may) and its places; a fixed vehicle's one
	const int S = isFixed ? 0 : ((noStart && noStart[i]) ? 0 : 1), P = isFixed ? 0 : count, per = S + P;
	const long long nCandidates = isFixed ? 1 : ppw::candidates(D, S, P);
	uint64_t blocker = ppy::kNoKey, atZero = ppy::kNoKey;
	int blockedKind = ppw::kNoWait, blockedA = 0, blockedD = 0, blockedSlot = 0;
	int chosenKind = kWaitUnscheduled, chosenA = 0, chosenD = 0, chosenSlot = 0;
	long long nTried = 0;
	int d = isFixed ? fx.steps : 0, r = 0;
	for (long long o = 0; o < nCandidates; o++) { // (wave-uniform)
		int kind = ppw::kNoWait, a = 0, slotOf = 0;
		if (d > 0) {
			if (isFixed)
				kind = fx.row == ppw::kStart ? ppw::kStart : 0;
			else
				kind = S && r == 0 ? ppw::kStart : r - S;
			if (kind >= 0) {
				slotOf = kind;
				a = mine[slotOf].column;
			}
		}
		uint64_t best = ppy::kNoKey;
		if (o > 0 && kind >= 0 && atZero != ppy::kNoKey && ppw::rejected_with_the_first(a, ppy::time_of(atZero, nPlans), D))
			best = atZero; // (the shortcut: where it was at every time up to the first conflict of d = 0)
		else {
			for (int m = lane; m < L.T && best == ppy::kNoKey; m += kWaitLanes) {
				double ax, ay, asn, acs;
				if (!wait_position(xi, component, heading, kind, a, d, mine + slotOf, m + D, ax, ay, asn, acs))
					continue;
				for (int k = pFirst; k < pEnd; k++) {
					const int j = partners[k];
					const WaitState sj = states[j];
					if (sj.kind == kWaitUnscheduled) // (as if absent)
						continue;
					double bx, by, bsn, bcs;
					if (!wait_position(traj + (size_t)j * columns, component, heading, sj.kind, sj.column, sj.steps,
							places + (size_t)j * (size_t)C.stride + (sj.kind > 0 ? sj.kind : 0), m + D, bx, by, bsn, bcs))
						continue;
					double sep = __builtin_huge_val();
					for (int da = 0; da < F.n; da++) { // (wave-uniform trip counts)
						double cax, cay;
						disc_centre(F, da, ax, ay, asn, acs, cax, cay);
						for (int db = 0; db < F.n; db++) {
							double cbx, cby;
							disc_centre(F, db, bx, by, bsn, bcs, cbx, cby);
							sep = ppv::min_of(sep, ppc::separation(cax - cbx, cay - cby, (double)F.r[da], (double)F.r[db]));
						}
					}
					if (ppc::in_conflict(sep, L.margin)) {
						const uint64_t key = ppy::key(m, nPlans, j);
						if (ppy::before(key, best))
							best = key;
					}
				}
			}
			for (int off = 32; off > 0; off >>= 1) {
				const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)best, off, 64);
				if (ppy::before(other, best))
					best = other;
			}
		}
		if (o == 0)
			atZero = best;
		nTried++;
		if (best == ppy::kNoKey || isFixed) { // (a fixed vehicle is scheduled whatever its one candidate meets)
			chosenKind = kind;
			chosenA = a;
			chosenD = d;
			chosenSlot = slotOf;
		}
		if (best != ppy::kNoKey) {
			blocker = best;
			blockedKind = kind;
			blockedA = a;
			blockedD = d;
			blockedSlot = slotOf;
		} else
			break;
		if (o == 0) {
			d = 1;
			r = 0;
		} else if (++r == per) {
			r = 0;
			d++;
		}
	}
	if (lane != 0)
		return;
	const bool scheduled = chosenKind != kWaitUnscheduled;
	const bool rejected = blocker != ppy::kNoKey; // (some candidate was: the last one of them is described)
	rec.status = isFixed ? (rejected ? 2 : 0) : (scheduled ? 0 : 1);
	rec.n_tried = (int32_t)nTried;
	rec.t_start = args[i].tStart;
	if (scheduled) {
		rec.wait_steps = chosenD;
		if (chosenKind < 0) { // (no wait, or the start: the delay call's expression, also for d = 0)
			rec.place = chosenKind;
			rec.t_start = args[i].tStart + (double)chosenD * L.dt;
		} else {
			const pp_wait_place pl = mine[chosenSlot];
			rec.place = chosenSlot;
			rec.row = pl.row;
			rec.t_hold = ppc::lattice_time(L.k0 - D, chosenA, L.dt);
			rec.t_resume = ppc::lattice_time(L.k0 - D, (long long)chosenA + chosenD, L.dt);
			rec.s_wait = pl.s;
		}
	}
	if (rejected) {
		const int m = ppy::time_of(blocker, nPlans), j = ppy::partner_of(blocker, nPlans);
		const WaitState sj = states[j];
		rec.blocker = j;
		rec.t_block = ppc::lattice_time(L.k0, m, L.dt);
		rec.s_block[0] = wait_length(xi, component, blockedKind, blockedA, blockedD, mine + blockedSlot, m + D);
		rec.s_block[1] = wait_length(traj + (size_t)j * columns, component, sj.kind, sj.column, sj.steps, places + (size_t)j * (size_t)C.stride + (sj.kind > 0 ? sj.kind : 0), m + D);
	}
	states[i] = scheduled ? WaitState { chosenKind, chosenA, chosenD, 0 } : WaitState { kWaitUnscheduled, 0, 0, 0 };
	out[i] = rec;
}

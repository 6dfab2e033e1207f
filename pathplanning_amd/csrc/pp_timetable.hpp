// Questions to the timetable a speed-profile call left on the device: where is the vehicle, how fast, on which pose and how far from its next stop at
// a time since its start or at an arc length, and where does the plan stand and for how long (include/pp_hip.h, "timetable look-ups and stops")?
// Included by pp_planner.hip behind pp_pairs.hpp: it reads the planner's PathRec / RsLogEntry / DevResult records where the search left them, through
// PostEdge / load_edge of pp_postprocess.hpp, and the (s, v, t) rows where k_speed_profile_tickets left them.  It reads no map and writes nothing but
// its own buffers.  The arithmetic is pp_timetable_rule.hpp's (and pp_conflict_rule.hpp's, and, for arc length -> (edge, ratio), pp_locate_rule.hpp's),
// which host programs run too.
//   k_timetable_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) with the profile
//                        rows of args[i] (a ConflictArg whose start time is not read), and writes out[i], the plan's stops[i][0 .. n_listed) and
//                        lookups[i][0 .. P).
// Dynamic LDS, as k_trajectory_tickets (trajectory_lds_bytes): edgeS[maxPath] doubles, then edgeL[maxPath] doubles.
//  1. every lane forms the lengths of edges lane + 1, lane + 65, ...; lane 0 turns them into S_e, the sequential root-first sum -- k_trajectory_tickets'
//     step 1;
//  2. the stops: the wave walks the rows 64 at a time, in order; a ballot of v == 0 gives a stop its ordinal, the count of the blocks before plus the
//     stops below its lane, and the first max_stops are written.  No atomic: the list is in row order and has the same bytes on every run;
//  3. behind a fence and a barrier (the lanes read stops other lanes wrote) the lanes take look-ups lane, lane + 64, ...: the row search and the step
//     forward (by time) or inverted (by arc length), the edge and the ratio, the pose, direction and curvature of the path object, and the binary search
//     of the listed stops for the next one; one 128-byte record each.
#pragma once

static_assert(sizeof(pp_timetable_params) == 16, "pp_timetable_params layout");
static_assert(sizeof(pp_timetable_plan) == 40, "pp_timetable_plan layout");
static_assert(sizeof(pp_timetable_stop) == 32, "pp_timetable_stop layout");
static_assert(sizeof(pp_timetable_result) == 128, "pp_timetable_result layout");

struct TimetableCall { // what the kernel knows of a call
	int by;         // 0: by arc length; 1: by time
	int maxStops;   // rows of the stop list per plan
	int nPoints;    // P look-ups per plan
	int maxSamples; // the stride of the profile rows, in samples
	double aAcc, aDec; // of the speed-profile call whose rows these are
};

constexpr int kTimetableLanes = 64;

__global__ void __launch_bounds__(kTimetableLanes) k_timetable_tickets(SearchArgs A, TimetableCall C, int nPlans, const int32_t* __restrict__ slots,
	const ConflictArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results,
	const double* __restrict__ rows, const double* __restrict__ values, pp_timetable_stop* stops, pp_timetable_result* __restrict__ lookups,
	pp_timetable_plan* __restrict__ out)
{
	extern __shared__ double timetableLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = timetableLds;             // [maxPath]: S_e at e - 1
	double* const edgeL = timetableLds + A.maxPath; // [maxPath]: the length of edge e at e - 1
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const ConflictArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const double* const row = rows + (size_t)arg.row * (size_t)C.maxSamples * 3;
	const double* const value = values + (size_t)q * (size_t)C.nPoints;
	pp_timetable_result* const lookup = lookups + (size_t)q * (size_t)C.nPoints;
	pp_timetable_stop* const stop = stops + (size_t)q * (size_t)C.maxStops;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	pp_timetable_plan rec {}; // (every field zero)
	if (arg.nSamples < 1 || arg.nSamples > C.maxSamples || res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		pp_timetable_result none {};
		none.status = -1;
		for (int p = lane; p < C.nPoints; p += kTimetableLanes)
			lookup[p] = none;
		rec.status = -1;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	const int nEdges = nPath - 1, N = arg.nSamples;
	// ---------------- 1: lengths, S_e
	for (int e = lane + 1; e <= nEdges; e += kTimetableLanes)
		edgeL[e - 1] = load_edge(A, recs, nPath, e, rslog, nRsLog).length();
	__syncthreads();
	if (lane == 0) {
		double length = 0.0;
		for (int e = 1; e <= nEdges; e++) { // PushBack, path_composite.h:33-39
			edgeS[e - 1] = length;
			length += edgeL[e - 1];
		}
	}
	// ---------------- 2: the stops
	const unsigned long long lanesBelow = (1ull << lane) - 1;
	int nStops = 0;
	for (int base = 0; base < N; base += kTimetableLanes) {
		const int j = base + lane;
		const bool stands = j < N && ppm::is_stop(row[3 * (size_t)j + 1]);
		const unsigned long long standing = __ballot(stands);
		const int ordinal = nStops + __popcll(standing & lanesBelow);
		if (stands && ordinal < C.maxStops) {
			pp_timetable_stop st {};
			st.row = j;
			st.s = row[3 * (size_t)j];
			st.t_arrive = ppm::arrive_time(row, j, C.aAcc, C.aDec);
			st.t_depart = row[3 * (size_t)j + 2];
			stop[ordinal] = st;
		}
		nStops += __popcll(standing);
	}
	const int nListed = nStops < C.maxStops ? nStops : C.maxStops;
	const double end = row[3 * (size_t)(N - 1) + 2];
	if (lane == 0) {
		rec.n_samples = N;
		rec.n_stops = nStops;
		rec.n_listed = nListed;
		rec.s_first = row[0];
		rec.s_last = row[3 * (size_t)(N - 1)];
		rec.duration = end;
		out[q] = rec;
	}
	__threadfence_block(); // the stops, and lane 0's S_e, to the lanes that read them below
	__syncthreads();
	// ---------------- 3: the look-ups
	for (int p = lane; p < C.nPoints; p += kTimetableLanes) {
		const ppm::Sample at = C.by ? ppm::at_time(row, N, value[p], C.aAcc, C.aDec) : ppm::at_length(row, N, value[p], C.aAcc, C.aDec);
		pp_timetable_result r {}; // (every field zero)
		r.status = at.status;
		r.row = at.row;
		r.s = at.s;
		r.t = at.t;
		r.v = at.v;
		r.a = at.a;
		if (nEdges == 0) {
			const PathRec only = recs[0];
			r.pose[0] = only.x;
			r.pose[1] = only.y;
			r.pose[2] = only.t;
		} else {
			const int e = ppl::edge_of(edgeS, nEdges, at.s);
			const double ratio = ppl::ratio_of(at.s, edgeS[e - 1], edgeL[e - 1]);
			const PostEdge E = load_edge(A, recs, nPath, e, rslog, nRsLog);
			const Pose pose = E.interpolate(ratio);
			const int d = E.direction(ratio);
			r.edge = e;
			r.direction = d == rs::kFwd ? ppv::kForward : (d == rs::kBwd ? ppv::kReverse : ppv::kNoDirection);
			r.ratio = ratio;
			r.kappa = E.curvature(ratio);
			r.pose[0] = pose.x;
			r.pose[1] = pose.y;
			r.pose[2] = pose.t;
		}
		r.next_stop = ppm::next_stop(&stop->row, (int)(sizeof(pp_timetable_stop) / 4), nListed, at.row);
		if (r.next_stop >= 0) {
			const pp_timetable_stop st = stop[r.next_stop];
			r.s_to_stop = st.s - at.s;
			r.t_to_stop = st.t_arrive - at.t;
		}
		r.t_remaining = end - at.t;
		lookup[p] = r;
	}
}

// How fast may the vehicle drive along the plan held for it, and when does it arrive where?  Per sample of the stamp's schedule inside a window of
// arc length: the speed and the time (include/pp_hip.h, "speed profiles along held plans").  One wave per plan; included by pp_planner.hip behind
// pp_locate.hpp (it reads the planner's PathRec / RsLogEntry / DevResult records where the search left them, through PostEdge / load_edge of
// pp_postprocess.hpp).  It reads the target map's distance grid when the call has a clearance term and no map otherwise, and writes nothing but
// its own sample rows and records.  The arithmetic is pp_speed_rule.hpp's (and, for the sample schedule, pp_stamp_rule.hpp's), which host
// programs run too.
//   k_speed_profile_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) with the
//                            window and the end speeds of args[i], and writes rows[i][0 .. n_samples) = (s, v, t) and out[i].
// Dynamic LDS: edgeS[maxPath] doubles, edgeL[maxPath] doubles, then edgeFirst[maxPath + 1] ints.
//  1. every lane forms the lengths of edges lane + 1, lane + 65, ...; lane 0 turns them into S_e, the sequential root-first sum
//     (pp_revalidate_result::length bit for bit), and the sample counts into each edge's first sample index -- k_stamp_tickets' prologue, except that
//     the lengths stay in LDS: a sample's arc length then needs no path object;
//  2. the count: the wave walks the schedule 64 samples at a time and finds the first sample inside the window and N (arc lengths only).  The window
//     is one run of the schedule, so sample i of the SEQUENCE is sample first + i of the schedule.  N == 0 and N > maxSamples end here;
//  3. forward over the sequence in blocks of 64, lane l on sample base + l: pose, direction, curvature and, if asked, the disc look-ups; the carried
//     direction and the cusp flag from two ballots; w; A and its inclusive min-scan (six wave shifts, the carry of earlier blocks in a register);
//     the row gets (s, w, fwd), fwd replaced by -1 at a cusp stop (where it is 0: F <= A = -(2 a s), and fwd >= 0 everywhere);
//  4. backward over the blocks: B and its min-scan from the back, e, v, the peak; the step to the next sample (lane + 1, or the first sample of the
//     block behind) gives dt and the dwell; the row gets (s, v, dt);
//  5. forward again: t is the sum of the steps before a sample, formed in sample order -- 64 dependent additions per block, every lane keeping the sum
//     that stands before its own step.  A tree-shaped scan was tried first: its partial sums round differently from lane to lane, so that t went DOWN
//     by an ulp across a step of zero (a junction); the sequential sum cannot, costs a few microseconds per plan, and has the definition's bits.
//     The row gets (s, v, t).
// A lane reads back only what it wrote itself (sample i is lane i % 64's in every pass), so the passes need no fence between them.
#pragma once

struct SpeedArg { // per plan of a call
	double from, to;     // the window in arc length (-inf / +inf: open)
	double vStart, vEnd; // speeds at the first and the last sample of the sequence
};
static_assert(sizeof(SpeedArg) == 32, "SpeedArg layout");
static_assert(sizeof(pp_speed_profile_result) == 72, "pp_speed_profile_result layout");

constexpr int kSpeedLanes = 64;
/// dynamic LDS of a launch for a buffer set of path capacity maxPath
inline size_t speed_lds_bytes(int maxPath) { return (size_t)maxPath * 16 + ((size_t)maxPath + 2) / 2 * 8; }

/// sample j of the schedule: its edge (0: a one-pose plan), its ratio on it and, returned, its arc length -- k_stamp_tickets' expressions on the same values
__device__ __forceinline__ double speed_sample(const double* edgeS, const double* edgeL, const int* edgeFirst, int nEdges, double spacing, int j, int& edge, double& ratio)
{
	edge = 0;
	ratio = 0.0;
	if (nEdges == 0)
		return 0.0;
	int lo = 1, hi = nEdges; // the last edge whose first sample is <= j
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (edgeFirst[mid - 1] <= j)
			lo = mid;
		else
			hi = mid - 1;
	}
	edge = lo;
	const double l = edgeL[lo - 1];
	ratio = pps::sample_ratio(j - edgeFirst[lo - 1], pps::edge_steps(l, spacing));
	return pps::sample_arc_length(edgeS[lo - 1], ratio, l);
}

/// the direction (ppv::kForward / kReverse) of the highest lane of `moving`, whose forward lanes are `forward`
__device__ __forceinline__ int speed_direction_of_last(unsigned long long moving, unsigned long long forward)
{
	return (forward >> (63 - __clzll((long long)moving))) & 1 ? ppv::kForward : ppv::kReverse;
}

__global__ void __launch_bounds__(kSpeedLanes) k_speed_profile_tickets(SearchArgs A, Footprint F, ppv::Limits L, double spacing, int maxSamples, int nPlans,
	const int32_t* __restrict__ slots, const SpeedArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase,
	const DevResult* __restrict__ results, double* __restrict__ rows, pp_speed_profile_result* __restrict__ out)
{
	extern __shared__ double speedLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = speedLds;                             // [maxPath]: S_e at e - 1 (the plan's length behind the last)
	double* const edgeL = speedLds + A.maxPath;                 // [maxPath]: the length of edge e at e - 1
	int* const edgeFirst = (int*)(speedLds + 2 * (size_t)A.maxPath); // [maxPath + 1]: samples of edge e, then the index of its first one
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const SpeedArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	double* const row = rows + (size_t)q * (size_t)maxSamples * 3;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	pp_speed_profile_result rec {}; // (every field zero)
	if (res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		rec.status = res.r.status != 0 || nPath < 1 ? -1 : -4;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	const int nEdges = nPath - 1;
	// ---------------- 1: lengths, S_e, first sample indices
	for (int e = lane + 1; e <= nEdges; e += kSpeedLanes) {
		const double l = load_edge(A, recs, nPath, e, rslog, nRsLog).length();
		edgeL[e - 1] = l;
		edgeFirst[e - 1] = pps::edge_steps(l, spacing) + 1;
	}
	__syncthreads();
	if (lane == 0) {
		double length = 0.0;
		int first = 0;
		for (int e = 1; e <= nEdges; e++) { // PushBack, path_composite.h:33-39
			const int count = edgeFirst[e - 1];
			edgeS[e - 1] = length;
			edgeFirst[e - 1] = first;
			length += edgeL[e - 1];
			first += count;
		}
		edgeFirst[nEdges] = nEdges > 0 ? first : 1; // (a one-pose plan has one sample: its pose, at s = 0)
		edgeS[nEdges > 0 ? nEdges : 0] = length;   // (maxPath >= nPath = nEdges + 1 entries)
	}
	__syncthreads();
	const int total = edgeFirst[nEdges];
	rec.length = edgeS[nEdges > 0 ? nEdges : 0]; // (from here on the three arrays are only read)
	// ---------------- 2: the first sample inside the window and N
	int first = 0, N = 0;
	for (int base = 0; base < total; base += kSpeedLanes) {
		const int j = base + lane;
		bool inside = false;
		if (j < total) {
			int edge;
			double ratio;
			inside = pps::in_window(speed_sample(edgeS, edgeL, edgeFirst, nEdges, spacing, j, edge, ratio), arg.from, arg.to);
		}
		const unsigned long long in = __ballot(inside);
		if (in != 0 && N == 0)
			first = base + __ffsll((long long)in) - 1;
		N += __popcll(in);
	}
	rec.n_samples = N;
	if (N == 0 || N > maxSamples) { // (wave-uniform)
		rec.status = N == 0 ? 1 : -5;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	// ---------------- 3: forward: s, the cusp flag, w, the forward limit
	constexpr double kInf = __builtin_huge_val();
	const unsigned long long lanesBelow = (1ull << lane) - 1, lanesUpTo = lanesBelow | (1ull << lane);
	int carriedDir = ppv::kNoDirection, nCusps = 0;
	double carry = kInf; // F of the blocks before this one
	double clBest = kInf, clBestS = 0.0, sFirst = 0.0;
	for (int base = 0; base < N; base += kSpeedLanes) {
		const int i = base + lane;
		const bool active = i < N;
		double s = 0.0, kappa = 0.0;
		float cl = 0.0f;
		int own = ppv::kNoDirection;
		if (active) {
			int edge;
			double ratio;
			s = speed_sample(edgeS, edgeL, edgeFirst, nEdges, spacing, first + i, edge, ratio);
			Pose p;
			if (nEdges == 0) {
				const PathRec only = recs[0];
				p = Pose { only.x, only.y, only.t };
			} else {
				const PostEdge E = load_edge(A, recs, nPath, edge, rslog, nRsLog);
				p = E.interpolate(ratio);
				const int d = E.direction(ratio);
				own = d == rs::kFwd ? ppv::kForward : (d == rs::kBwd ? ppv::kReverse : ppv::kNoDirection);
				kappa = E.curvature(ratio);
			}
			if (L.clearanceGain > 0.0) { // (wave-uniform: without the term no map is read)
				float clearance, border;
				if (fp_state_valid(A.m, F, p.x, p.y, p.t, clearance, border))
					cl = clearance;
				if (ppv::lower_clearance((double)cl, s, clBest, clBestS)) {
					clBest = (double)cl;
					clBestS = s;
				}
			}
		}
		// the direction a sample counts with is the one of the last sample at or before it that moves (ppv::carried_direction down the chain)
		const unsigned long long moving = __ballot(own != ppv::kNoDirection), forward = __ballot(own == ppv::kForward);
		const unsigned long long upTo = moving & lanesUpTo, below = moving & lanesBelow;
		const int dir = upTo ? speed_direction_of_last(upTo, forward) : carriedDir;
		const int previous = below ? speed_direction_of_last(below, forward) : carriedDir;
		const bool cusp = active && i > 0 && ppv::is_cusp(dir, previous);
		if (moving)
			carriedDir = speed_direction_of_last(moving, forward);
		nCusps += __popcll(__ballot(cusp));
		const double w = ppv::cap_squared(ppv::cap(L, dir, kappa, cl), cusp, i == 0, i == N - 1, arg.vStart, arg.vEnd);
		double f = active ? ppv::forward_key(w, s, L.aAcc) : kInf;
		for (int off = 1; off < kSpeedLanes; off <<= 1) {
			const double o = __shfl_up(f, off, 64);
			if (lane >= off)
				f = ppv::min_of(f, o);
		}
		f = ppv::min_of(f, carry);
		carry = __shfl(f, kSpeedLanes - 1, 64);
		if (active) {
			row[3 * (size_t)i] = s;
			row[3 * (size_t)i + 1] = w;
			row[3 * (size_t)i + 2] = cusp ? -1.0 : ppv::forward_limit(f, s, L.aAcc);
		}
		if (base == 0)
			sFirst = __shfl(s, 0, 64);
	}
	// ---------------- 4: backward: the backward limit, e, v, the step times
	carry = kInf; // G of the blocks behind this one
	double vPeak = 0.0, sLast = 0.0;
	double nextS = 0.0, nextV = 0.0; // the first sample of the block behind
	int nextCusp = 0;
	for (int base = (N - 1) / kSpeedLanes * kSpeedLanes; base >= 0; base -= kSpeedLanes) {
		const int i = base + lane;
		const bool active = i < N;
		double s = 0.0, w = 0.0, fwd = 0.0;
		int cusp = 0;
		if (active) {
			s = row[3 * (size_t)i];
			w = row[3 * (size_t)i + 1];
			fwd = row[3 * (size_t)i + 2];
			cusp = fwd < 0.0;
			if (cusp)
				fwd = 0.0;
		}
		double g = active ? ppv::backward_key(w, s, L.aDec) : kInf;
		for (int off = 1; off < kSpeedLanes; off <<= 1) {
			const double o = __shfl_down(g, off, 64);
			if (lane + off < kSpeedLanes)
				g = ppv::min_of(g, o);
		}
		g = ppv::min_of(g, carry);
		carry = __shfl(g, 0, 64);
		const double v = active ? ppv::speed(ppv::envelope(w, fwd, ppv::backward_limit(g, s, L.aDec))) : 0.0;
		vPeak = v > vPeak ? v : vPeak;
		double s1 = __shfl_down(s, 1, 64), v1 = __shfl_down(v, 1, 64);
		int cusp1 = __shfl_down(cusp, 1, 64);
		if (lane == kSpeedLanes - 1) {
			s1 = nextS;
			v1 = nextV;
			cusp1 = nextCusp;
		}
		if (base + kSpeedLanes >= N) // the last block: sample N - 1 is lane (N - 1) % 64's
			sLast = __shfl(s, (N - 1) & (kSpeedLanes - 1), 64);
		nextS = __shfl(s, 0, 64);
		nextV = __shfl(v, 0, 64);
		nextCusp = __shfl(cusp, 0, 64);
		if (active) {
			double dt = 0.0;
			if (i + 1 < N)
				dt = ppv::step_time(s1 - s, v, v1, L.aAcc, L.aDec) + (cusp1 ? L.dwell : 0.0);
			row[3 * (size_t)i + 1] = v;
			row[3 * (size_t)i + 2] = dt;
		}
	}
	// ---------------- 5: forward: the times
	double clock = 0.0, duration = 0.0; // t of the block's first sample
	for (int base = 0; base < N; base += kSpeedLanes) {
		const int i = base + lane;
		const bool active = i < N;
		const double dt = active ? row[3 * (size_t)i + 2] : 0.0;
		double t = 0.0;
#pragma unroll 8
		for (int l = 0; l < kSpeedLanes; l++) { // (wave-uniform: every lane adds the same 64 steps in the same order, and keeps the sum before its own)
			if (l == lane)
				t = clock;
			clock = clock + __shfl(dt, l, 64);
		}
		if (active)
			row[3 * (size_t)i + 2] = t;
		if (base + kSpeedLanes >= N)
			duration = __shfl(t, (N - 1) & (kSpeedLanes - 1), 64);
	}
	// ---------------- the record
	for (int off = 32; off > 0; off >>= 1) {
		const double ov = __shfl_xor(vPeak, off, 64), oc = __shfl_xor(clBest, off, 64), os = __shfl_xor(clBestS, off, 64);
		vPeak = ov > vPeak ? ov : vPeak;
		if (ppv::lower_clearance(oc, os, clBest, clBestS)) {
			clBest = oc;
			clBestS = os;
		}
	}
	if (lane == 0) {
		rec.status = 0;
		rec.n_cusps = nCusps;
		rec.s_first = sFirst;
		rec.s_last = sLast;
		rec.duration = duration;
		rec.v_peak = vPeak;
		rec.min_clearance = clBest; // (+inf without the clearance term)
		rec.s_min_clearance = clBestS;
		out[q] = rec;
	}
}

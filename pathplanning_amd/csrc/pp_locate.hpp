// Where is a vehicle on the plan held for it?  The point of a held plan closest to a vehicle pose, with the arc length, edge, ratio, path pose,
// errors and travel direction there (include/pp_hip.h, "locating vehicles on held plans").  One wave per plan; included by pp_planner.hip
// behind pp_stamp.hpp (it reads the planner's PathRec / RsLogEntry / DevResult records where the search left them, through PostEdge / load_edge
// of pp_postprocess.hpp).  It reads no map and writes nothing but its own records.  The arithmetic is pp_locate_rule.hpp's (and, for the sample
// schedule, pp_stamp_rule.hpp's), which host programs run too.
//   k_locate_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) with the
//                     vehicle pose and the window of args[i], and writes out[i].
// Dynamic LDS: edgeS[maxPath] doubles, then edgeFirst[maxPath + 1] ints, as in k_stamp_tickets.
//  1. every lane forms the lengths of edges lane + 1, lane + 65, ...;
//  2. lane 0 turns them into S_e, the sequential root-first sum (pp_revalidate_result::length bit for bit: the order is part of the result),
//     and the sample counts into each edge's first sample index;
//  3. stage 1: the lanes take 64 consecutive samples of the stamp's schedule per pass: edge by binary search, pose by PostEdge::interpolate,
//     the window test, the cost; a lane keeps its best under the (c, s) order, the wave reduces with __shfl_xor;
//  4. stage 2: the 66 points of the global lattice i * spacing / 32 around the winner's arc length, in two passes of the SAME loop body
//     (one copy of load_edge and interpolate in the kernel's text), the same reduction;
//  5. lane 0 writes the record.
// A junction pose is sampled twice with one arc length, as the end of edge e and as the start of edge e + 1: the second names the point (as
// "the largest e with S_e <= u" does for a lattice point), the first is counted in n_samples and is no candidate -- otherwise rounding noise
// in two equal poses would choose the edge.  A candidate that ties with the best so far in cost AND arc length does not replace it; across
// lanes the earlier candidate of the schedule wins such a tie, and the stage-1 winner comes before every lattice point.
#pragma once

struct LocateArg { // per plan of a call
	double pose[3];  // the vehicle
	double from, to; // the window in arc length (-inf / +inf: open)
};
static_assert(sizeof(LocateArg) == 40, "LocateArg layout");
static_assert(sizeof(pp_locate_result) == 96, "pp_locate_result layout");

constexpr int kLocateLanes = 64;
/// dynamic LDS of a launch for a buffer set of path capacity maxPath
inline size_t locate_lds_bytes(int maxPath) { return (size_t)maxPath * 8 + ((size_t)maxPath + 2) / 2 * 8; }

__global__ void __launch_bounds__(kLocateLanes) k_locate_tickets(SearchArgs A, double spacing, double headingWeight, int nPlans, const int32_t* __restrict__ slots,
	const LocateArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results,
	pp_locate_result* __restrict__ out)
{
	extern __shared__ double locateLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = locateLds;                      // [maxPath]: edge e at e - 1: its length, then S_e
	int* const edgeFirst = (int*)(locateLds + A.maxPath); // [maxPath + 1]: samples of edge e, then the index of its first one
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const LocateArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	pp_locate_result rec {}; // (every field zero)
	if (res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		rec.status = res.r.status != 0 || nPath < 1 ? -1 : -4;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	const int nEdges = nPath - 1;
	// ---------------- 1, 2: lengths, S_e, first sample indices
	for (int e = lane + 1; e <= nEdges; e += kLocateLanes) {
		const double l = load_edge(A, recs, nPath, e, rslog, nRsLog).length();
		edgeS[e - 1] = l;
		edgeFirst[e - 1] = pps::edge_steps(l, spacing) + 1;
	}
	__syncthreads();
	if (lane == 0) {
		double length = 0.0;
		int first = 0;
		for (int e = 1; e <= nEdges; e++) { // PushBack, path_composite.h:33-39
			const double l = edgeS[e - 1];
			const int count = edgeFirst[e - 1];
			edgeS[e - 1] = length;
			edgeFirst[e - 1] = first;
			length += l;
			first += count;
		}
		edgeFirst[nEdges] = nEdges > 0 ? first : 1; // (a one-pose plan has one sample: its pose, at s = 0)
		edgeS[nEdges > 0 ? nEdges : 0] = length;   // (maxPath >= nPath = nEdges + 1 entries)
	}
	__syncthreads();
	const int total = edgeFirst[nEdges];
	const double length = edgeS[nEdges > 0 ? nEdges : 0]; // (from here on both arrays are only read)
	rec.length = length;
	// ---------------- 3, 4: the two stages, one loop body
	const double delta = ppl::lattice_step(spacing);
	constexpr double kNone = __builtin_huge_val();
	constexpr int kLatticeOrder = 0x40000000; // lattice points come behind every sample (a plan has at most 2^30 + 2^11 samples: order stays below 2^31)
	// the best candidate so far: after a reduction every lane holds the wave's
	double bestC = kNone, bestS = kNone, bestRatio = 0.0, bestX = 0.0, bestY = 0.0, bestT = 0.0;
	int bestEdge = 0, bestDir = 1, bestOrder = 0x7FFFFFFF;
	int nSamples = 0;
	int64_t latticeFirst = 0;
	for (int stage = 0; stage < 2; stage++) {
		const int count = stage == 0 ? total : (nEdges > 0 ? ppl::kLatticePoints : 0);
		for (int base = 0; base < count; base += kLocateLanes) {
			const int j = base + lane;
			bool inside = false, candidate = true;
			if (j < count) {
				Pose p { 0.0, 0.0, 0.0 };
				double s = 0.0, ratio = 0.0;
				int edge = 0, dir = 1;
				if (nEdges == 0) {
					const PathRec only = recs[0];
					p = Pose { only.x, only.y, only.t };
					inside = pps::in_window(s, arg.from, arg.to);
				} else {
					if (stage == 0) {
						int lo = 1, hi = nEdges; // the last edge whose first sample is <= j
						while (lo < hi) {
							const int mid = (lo + hi + 1) >> 1;
							if (edgeFirst[mid - 1] <= j)
								lo = mid;
							else
								hi = mid - 1;
						}
						edge = lo;
						inside = true;
					} else {
						inside = ppl::lattice_point(latticeFirst + j, delta, length, arg.from, arg.to, s);
						if (inside)
							edge = ppl::edge_of(edgeS, nEdges, s);
					}
					if (inside) { // (a lattice point outside the plan or the window has no edge)
						const PostEdge E = load_edge(A, recs, nPath, edge, rslog, nRsLog);
						const double l = E.length();
						if (stage == 0) {
							const int k = j - edgeFirst[edge - 1], n = pps::edge_steps(l, spacing);
							ratio = pps::sample_ratio(k, n);
							s = pps::sample_arc_length(edgeS[edge - 1], ratio, l);
							inside = pps::in_window(s, arg.from, arg.to);
							candidate = !ppl::names_next_edge(k, n, edge, nEdges); // (counted, but the next edge's first sample stands for the junction)
						} else
							ratio = ppl::ratio_of(s, edgeS[edge - 1], l);
						p = E.interpolate(ratio);
						dir = E.direction(ratio) == rs::kBwd ? -1 : 1;
					}
				}
				if (inside && candidate) {
					const double c = ppl::cost(ppl::error_of(arg.pose[0], arg.pose[1], arg.pose[2], p.x, p.y, p.t), headingWeight);
					if (ppl::better(c, s, bestC, bestS)) {
						bestC = c;
						bestS = s;
						bestRatio = ratio;
						bestX = p.x;
						bestY = p.y;
						bestT = p.t;
						bestEdge = edge;
						bestDir = dir;
						bestOrder = stage == 0 ? j : kLatticeOrder + j;
					}
				}
			}
			if (stage == 0)
				nSamples += __popcll(__ballot(inside));
		}
		// the wave's best under (c, s), then the order of the schedule; its lane hands the candidate to every lane
		double c = bestC, s = bestS;
		int order = bestOrder, winner = lane;
		for (int off = 32; off > 0; off >>= 1) {
			const double oc = __shfl_xor(c, off, 64), os = __shfl_xor(s, off, 64);
			const int oo = __shfl_xor(order, off, 64), ow = __shfl_xor(winner, off, 64);
			if (ppl::better(oc, os, c, s) || (oc == c && os == s && oo < order)) {
				c = oc;
				s = os;
				order = oo;
				winner = ow;
			}
		}
		bestC = c;
		bestS = s;
		bestOrder = order;
		bestRatio = __shfl(bestRatio, winner, 64);
		bestX = __shfl(bestX, winner, 64);
		bestY = __shfl(bestY, winner, 64);
		bestT = __shfl(bestT, winner, 64);
		bestEdge = __shfl(bestEdge, winner, 64);
		bestDir = __shfl(bestDir, winner, 64);
		if (stage == 0) {
			rec.n_samples = nSamples;
			if (nSamples == 0) { // (wave-uniform)
				rec.status = 1;
				if (lane == 0)
					out[q] = rec;
				return;
			}
			latticeFirst = ppl::lattice_first(bestS, delta);
		}
	}
	// ---------------- 5: the record
	if (lane == 0) {
		const ppl::Error err = ppl::error_of(arg.pose[0], arg.pose[1], arg.pose[2], bestX, bestY, bestT);
		double sn, cs;
		sincos(bestT, &sn, &cs);
		rec.status = 0;
		rec.edge = bestEdge;
		rec.direction = bestDir;
		rec.s = bestS;
		rec.ratio = bestRatio;
		rec.distance = sqrt(err.ex * err.ex + err.ey * err.ey);
		rec.along = cs * err.ex + sn * err.ey;
		rec.lateral = cs * err.ey - sn * err.ex;
		rec.heading_error = err.dtheta;
		rec.pose[0] = bestX;
		rec.pose[1] = bestY;
		rec.pose[2] = bestT;
		out[q] = rec;
	}
}

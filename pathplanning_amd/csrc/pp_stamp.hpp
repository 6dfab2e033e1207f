// Held plans stamped into a map's occupancy grid: the cells the vehicle's discs cover at sample poses along a plan (include/pp_hip.h,
// "stamping held plans into a map").  One wave per plan; included by pp_planner.hip behind pp_revalidate.hpp (it reads the planner's
// PathRec / RsLogEntry / DevResult records where the search left them, through PostEdge / load_edge of pp_postprocess.hpp).  The sample
// schedule and the cell rule are pp_stamp_rule.hpp's, which a host program runs too.
//   k_stamp_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) with the
//                    value and the window of args[i], and writes out[i].
// Dynamic LDS: edgeS[maxPath] doubles, then edgeFirst[maxPath + 1] ints, then the disc centres of 64 samples.
//  1. every lane forms the lengths of edges lane + 1, lane + 65, ... (load_edge is the expensive part of the prologue);
//  2. lane 0 turns them into S_e, the sequential root-first sum (pp_revalidate_result::length bit for bit: the order is part of the result),
//     and the sample counts into each edge's first sample index;
//  3. the lanes take 64 consecutive samples of the plan: edge by binary search, pose by PostEdge::interpolate, the window test, the K disc
//     centres into LDS;
//  4. the wave rasterises the bounding box of every (sample in the window, disc) with its lanes across the cells, consecutive lanes on
//     consecutive columns of a row (= consecutive addresses): the centre test, an agent-scope load that skips cells already >= value (most of
//     them: consecutive samples overlap), a vector atomic max for the rest.
// The grid after the call does not depend on the order of plans, samples or lanes: max is commutative, and a stale load can only
// read a SMALLER value than the cell holds (values never decrease during the call), which costs an atomic, never a cell.
#pragma once

struct StampArg { // per plan of a call
	double from, to; // the window in arc length (-inf / +inf: open)
	int32_t value;
	int32_t pad;
};
static_assert(sizeof(StampArg) == 24, "StampArg layout");

constexpr int kStampLanes = 64;
#ifndef PP_STAMP_SKIP_LOAD
#define PP_STAMP_SKIP_LOAD 1 // 0: every covered cell gets the atomic (a build for measuring what the load saves: DESIGN.md 4.10)
#endif
/// dynamic LDS of a launch for a buffer set of path capacity maxPath
inline size_t stamp_lds_bytes(int maxPath) { return (size_t)maxPath * 8 + ((size_t)maxPath + 2) / 2 * 8 + (size_t)kStampLanes * kFootprintMaxDiscs * 16; }

__global__ void __launch_bounds__(kStampLanes) k_stamp_tickets(SearchArgs A, Footprint F, double spacing, float margin, int nPlans, const int32_t* __restrict__ slots,
	const StampArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results, int32_t* occ,
	pp_stamp_result* __restrict__ out)
{
	extern __shared__ double stampLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = stampLds;                                // [maxPath]: edge e at e - 1: its length, then S_e
	int* const edgeFirst = (int*)(stampLds + A.maxPath);           // [maxPath + 1]: samples of edge e, then the index of its first one
	double* const centres = stampLds + A.maxPath + (A.maxPath + 2) / 2; // [64][kFootprintMaxDiscs][2]
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const StampArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	if (res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		if (lane == 0)
			out[q] = pp_stamp_result { res.r.status != 0 || nPath < 1 ? -1 : -4, 0, { 0, -1, 0, -1 }, 0.0 };
		return;
	}
	const int nEdges = nPath - 1;
	const pps::Grid g { A.m.rows, A.m.cols, (double)A.m.res, A.m.gx, A.m.gy };
	// ---------------- 1, 2: lengths, S_e, first sample indices
	for (int e = lane + 1; e <= nEdges; e += kStampLanes) {
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
	// ---------------- 3, 4
	int nSamples = 0;
	int rowMin = 0x7FFFFFFF, rowMax = -1, colMin = 0x7FFFFFFF, colMax = -1;
	for (int base = 0; base < total; base += kStampLanes) {
		const int j = base + lane;
		bool inside = false;
		if (j < total) {
			Pose p;
			double s = 0.0;
			if (nEdges == 0) {
				const PathRec only = recs[0];
				p = Pose { only.x, only.y, only.t };
			} else {
				int lo = 1, hi = nEdges; // the last edge whose first sample is <= j
				while (lo < hi) {
					const int mid = (lo + hi + 1) >> 1;
					if (edgeFirst[mid - 1] <= j)
						lo = mid;
					else
						hi = mid - 1;
				}
				const PostEdge E = load_edge(A, recs, nPath, lo, rslog, nRsLog);
				const double l = E.length();
				const double ratio = pps::sample_ratio(j - edgeFirst[lo - 1], pps::edge_steps(l, spacing));
				s = pps::sample_arc_length(edgeS[lo - 1], ratio, l);
				p = E.interpolate(ratio);
			}
			inside = pps::in_window(s, arg.from, arg.to);
			if (inside) {
				double sn = 0.0, cs = 1.0;
				if (F.anyOffset)
					sincos(p.t, &sn, &cs);
				for (int i = 0; i < F.n; i++) {
					double cx, cy;
					disc_centre(F, i, p.x, p.y, sn, cs, cx, cy);
					centres[(lane * kFootprintMaxDiscs + i) * 2] = cx;
					centres[(lane * kFootprintMaxDiscs + i) * 2 + 1] = cy;
				}
			}
		}
		__syncthreads();
		unsigned long long todo = __ballot(inside);
		nSamples += __popcll(todo);
		while (todo) {
			const int k = __ffsll((long long)todo) - 1; // wave-uniform
			todo &= todo - 1;
			for (int i = 0; i < F.n; i++) {
				const double cx = centres[(k * kFootprintMaxDiscs + i) * 2], cy = centres[(k * kFootprintMaxDiscs + i) * 2 + 1];
				const double R = pps::effective_radius(F.r[i], margin);
				int r0, r1, c0, c1;
				pps::axis_range(cx, R, g.gx, g.res, g.rows, r0, r1);
				pps::axis_range(cy, R, g.gy, g.res, g.cols, c0, c1);
				if (r0 > r1 || c0 > c1)
					continue;
				// lanes across the box: `across` consecutive columns of `down` rows at a time
				const int width = c1 - c0 + 1;
				const int across = width < kStampLanes ? width : kStampLanes, down = kStampLanes / across;
				const int lr = lane / across, lc = lane - lr * across;
				for (int rb = r0; rb <= r1; rb += down)
					for (int cb = c0; cb <= c1; cb += across) {
						const int row = rb + lr, col = cb + lc;
						if (lr < down && row <= r1 && col <= c1 && pps::covers(g, row, col, cx, cy, R)) {
							rowMin = row < rowMin ? row : rowMin;
							rowMax = row > rowMax ? row : rowMax;
							colMin = col < colMin ? col : colMin;
							colMax = col > colMax ? col : colMax;
							int32_t* const cell = occ + ((size_t)row * g.cols + col);
#if PP_STAMP_SKIP_LOAD
							// (an agent-scope load is served by L2, where the atomics of this wave's earlier samples are visible; a load through
							// the CU's L1 may keep reading the line as it was before them, and then nothing is skipped)
							if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < arg.value)
#endif
								atomicMax(cell, arg.value);
						}
					}
			}
		}
		__syncthreads(); // the centres are rewritten by the next 64 samples
	}
	// ---------------- the record
	for (int off = 32; off > 0; off >>= 1) {
		const int a = __shfl_xor(rowMin, off, 64), b = __shfl_xor(rowMax, off, 64), c = __shfl_xor(colMin, off, 64), d = __shfl_xor(colMax, off, 64);
		rowMin = a < rowMin ? a : rowMin;
		rowMax = b > rowMax ? b : rowMax;
		colMin = c < colMin ? c : colMin;
		colMax = d > colMax ? d : colMax;
	}
	if (lane == 0) {
		const bool none = rowMax < 0;
		out[q] = pp_stamp_result { 0, nSamples, { none ? 0 : rowMin, rowMax, none ? 0 : colMin, none ? -1 : colMax }, length };
	}
}

// Is a plan handed out earlier still collision-free on a map that has changed since?  One wave per plan; included by pp_planner.hip
// behind pp_postprocess.hpp (it reads the planner's PathRec / RsLogEntry / DevResult records where the search left them, through that
// file's PostEdge / load_edge).
//   k_revalidate_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) and
//                         writes out[i].
// The plan's edges are the search's own path objects -- a constant-steer arc per node, the Reeds-Shepp path of the analytic expansion
// at the end -- and every edge is marched by the predicate the search used on it (is_path_valid, or is_path_valid_fp with the gain
// pp_check_arcs_footprint / pp_check_rs_paths_footprint define), but against A.m, the TARGET map's view at the time of the call: the grid
// pointer, the bounds and the validator's tunables all come from there.  Of a footprint only the discs are used (fp_state_valid reads the
// view's float distance grid, never the footprint's bitmaps, which belong to the footprint's own map).
// Lane l marches edges l + 1, l + 65, ... until one of them is blocked; the wave reduces to the lowest blocked edge.  IsPathValid never
// samples ratio 1 of a path, so the last pose of the plan gets the state check on top (status 2 when only that fails).  Lengths are the
// sequential root-first sum of the post-processing prologue (pp_post_result::length bit for bit), by lane 0.
#pragma once

__global__ void __launch_bounds__(64) k_revalidate_tickets(SearchArgs A, Footprint F, int nPlans, const int32_t* __restrict__ slots, const PathRec* __restrict__ pathBase,
	const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results, pp_revalidate_result* __restrict__ out)
{
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const MapView& m = A.m;
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	if (res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		if (lane == 0)
			out[q] = pp_revalidate_result { res.r.status != 0 || nPath < 1 ? -1 : -4, nPath > 0 ? nPath - 1 : 0, 0, 1.0f, 0.0, 0.0 };
		return;
	}
	const int nEdges = nPath - 1;
	// ---------------- the marches: this lane's lowest blocked edge and IsPathValid's `last` of it
	int blocked = 0x7FFFFFFF;
	float ratio = 1.0f;
	for (int e = lane + 1; e <= nEdges; e += 64) {
		const PostEdge E = load_edge(A, recs, nPath, e, rslog, nRsLog);
		float last = 1.0f;
		int checks = 0;
		bool ok;
		if (E.kind == 1)
			ok = F.n > 0 ? is_path_valid_fp(m, F, fp_gain(F, fabs(E.arc.kappa)), E.arc, E.arc.init, last, checks) : is_path_valid(m, E.arc, E.arc.init, last, checks);
		else
			ok = F.n > 0 ? is_path_valid_fp(m, F, fp_gain(F, 1.0 / A.rmin), E.rsp, E.rsp.init, last, checks) : is_path_valid(m, E.rsp, E.rsp.init, last, checks);
		if (!ok) {
			blocked = e;
			ratio = last;
			break; // (this lane's later edges lie further along the plan)
		}
	}
	int first = blocked;
	for (int off = 32; off > 0; off >>= 1) {
		const int o = __shfl_xor(first, off, 64);
		first = o < first ? o : first;
	}
	const bool anyBlocked = first != 0x7FFFFFFF;
	const float firstRatio = __shfl(ratio, anyBlocked ? (first - 1) & 63 : 0, 64); // edge e is lane (e - 1) % 64's, and that lane stopped at it
	if (lane != 0)
		return;
	// ---------------- lane 0: the state check of the last pose, the lengths, the record
	const PathRec goal = recs[0]; // (records are stored goal first)
	bool goalValid;
	if (F.n > 0) {
		float clearance, border;
		goalValid = fp_state_valid(m, F, goal.x, goal.y, goal.t, clearance, border);
	} else {
		float d;
		goalValid = is_state_valid(m, goal.x, goal.y, goal.t, d);
	}
	double length = 0.0, validLength = 0.0;
	for (int e = 1; e <= nEdges; e++) { // PushBack, path_composite.h:33-39: the order is part of the result
		const double l = load_edge(A, recs, nPath, e, rslog, nRsLog).length();
		if (anyBlocked && e == first)
			validLength = length + (double)firstRatio * l;
		length += l;
	}
	if (!anyBlocked)
		validLength = length;
	out[q] = pp_revalidate_result { anyBlocked ? 1 : (goalValid ? 0 : 2), nEdges, anyBlocked ? first : 0, anyBlocked ? firstRatio : 1.0f, validLength, length };
}

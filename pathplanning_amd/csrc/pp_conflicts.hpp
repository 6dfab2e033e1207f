// Do two vehicles, each driving the plan held for it on the timetable of its speed profile, ever come too close at the same time, and where and
// when first (include/pp_hip.h, "space-time conflicts between held plans")?  Included by pp_planner.hip behind pp_speed_profile.hpp: it reads the
// planner's PathRec / RsLogEntry / DevResult records where the search left them, through PostEdge / load_edge of pp_postprocess.hpp, and the (s, v, t)
// rows where k_speed_profile_tickets left them.  It reads no map and writes nothing but its own buffers.  The arithmetic is pp_conflict_rule.hpp's
// (and, for arc length -> (edge, ratio), pp_locate_rule.hpp's), which host programs run too.  Two kernels, so that poses cost O(n T) and not O(n^2 T):
//   k_trajectory_tickets  workgroup i (64 lanes) works on field slot slots[i] of a buffer set (slots == nullptr: slot i, the batch form) with the
//                         start time and the profile rows of args[i], and writes the plan's pose at every lattice time and out[i].
//   k_conflict_pairs      workgroup p (64 lanes) works on pair p: pairs[p] = (a, b), or -- pairs == nullptr -- the p-th pair i < j in row-major order.
// The trajectory is one array per component (x, y, theta, s, sin theta, cos theta), plan-major: component c of plan i at time m is
// traj[(c * nPlans + i) * T + m], so consecutive lanes (consecutive m) store and later load consecutive addresses.  A time at which the vehicle is
// absent has a NaN in every component; the pair kernel asks x.  The last two components exist only when a disc of the footprint sits off the reference
// point: the pair kernel then needs no trigonometry of its own.
// k_trajectory_tickets, dynamic LDS: edgeS[maxPath] doubles, then edgeL[maxPath] doubles.
//  1. every lane forms the lengths of edges lane + 1, lane + 65, ...; lane 0 turns them into S_e, the sequential root-first sum
//     (pp_revalidate_result::length bit for bit) -- k_speed_profile_tickets' step 1 without the sample counts;
//  2. the lanes take lattice times m = lane, lane + 64, ...: the row of the profile by binary search, the position within its step, the edge and the
//     ratio, the pose by PostEdge::interpolate;
//  3. the record: counts add, the first and the last time present are a min and a max, each with its arc length.
// k_conflict_pairs: the lanes take m = lane, lane + 64, ...; where both are present, the minimum over disc pairs of the separation; per lane the count
// of such times, the count in conflict, the (separation, tau) minimum and the first time in conflict; then the same four across the wave.  Only min and
// integer sums are formed across lanes, so no result depends on the order of evaluation.
#pragma once

struct ConflictArg { // per plan of a call
	double tStart;
	int32_t row;      // the plan's row of the holder's speed-profile rows
	int32_t nSamples; // N of its profile; 0: the profile's status is not 0
};
static_assert(sizeof(ConflictArg) == 16, "ConflictArg layout");
static_assert(sizeof(pp_conflict_params) == 40, "pp_conflict_params layout");
static_assert(sizeof(pp_trajectory_result) == 32, "pp_trajectory_result layout");
static_assert(sizeof(pp_conflict_result) == 80, "pp_conflict_result layout");

struct ConflictLattice { // what both kernels know of a call
	long long k0;    // tau_m = (double)(k0 + m) * dt
	int T;           // 1 .. 2^20 lattice times
	int holdBefore, holdAfter;
	int maxSamples;  // the stride of the profile rows, in samples
	double dt, margin;
	double aAcc, aDec; // of the speed-profile call whose rows these are
};

constexpr int kConflictLanes = 64;
constexpr int kTrajectoryComponents = 6; // x, y, theta, s, sin theta, cos theta
/// dynamic LDS of a k_trajectory_tickets launch for a buffer set of path capacity maxPath
inline size_t trajectory_lds_bytes(int maxPath) { return (size_t)maxPath * 16; }

__global__ void __launch_bounds__(kConflictLanes) k_trajectory_tickets(SearchArgs A, ConflictLattice L, int withHeading, int nPlans, const int32_t* __restrict__ slots,
	const ConflictArg* __restrict__ args, const PathRec* __restrict__ pathBase, const RsLogEntry* __restrict__ rsLogBase, const DevResult* __restrict__ results,
	const double* __restrict__ rows, double* __restrict__ traj, pp_trajectory_result* __restrict__ out)
{
	extern __shared__ double conflictLds[];
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	double* const edgeS = conflictLds;             // [maxPath]: S_e at e - 1 (the plan's length behind the last)
	double* const edgeL = conflictLds + A.maxPath; // [maxPath]: the length of edge e at e - 1
	const int slot = slots ? slots[q] : q;
	const DevResult res = results[slot];
	const ConflictArg arg = args[q];
	const PathRec* const recs = pathBase + (size_t)slot * A.maxPath;
	const RsLogEntry* const rslog = rsLogBase + (size_t)slot * kRsLogCap;
	const double* const row = rows + (size_t)arg.row * (size_t)L.maxSamples * 3;
	const size_t T = (size_t)L.T, component = (size_t)nPlans * T;
	double* const tx = traj + (size_t)q * T; // component c at tx + c * component
	const int nPath = res.r.n_path;
	const int nRsLog = res.nRsLog < 0 ? 0 : (res.nRsLog > kRsLogCap ? kRsLogCap : res.nRsLog);
	const int nComponents = withHeading ? kTrajectoryComponents : 4;
	constexpr double kAbsent = __builtin_nan("");
	pp_trajectory_result rec {}; // (every field zero)
	rec.first = rec.last = -1;
	if (arg.nSamples < 1 || arg.nSamples > L.maxSamples || res.r.status != 0 || nPath < 1 || nPath > A.maxPath) {
		for (int m = lane; m < L.T; m += kConflictLanes)
			for (int c = 0; c < nComponents; c++)
				tx[c * component + m] = kAbsent;
		rec.status = -1;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	const int nEdges = nPath - 1, N = arg.nSamples;
	// ---------------- 1: lengths, S_e
	for (int e = lane + 1; e <= nEdges; e += kConflictLanes)
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
	// ---------------- 2: the pose at every lattice time
	int nPresent = 0, first = 0x7FFFFFFF, last = -1;
	double sEnter = 0.0, sLeave = 0.0;
	for (int m = lane; m < L.T; m += kConflictLanes) {
		const double tau = ppc::lattice_time(L.k0, m, L.dt);
		double s;
		if (!ppc::position(row, N, tau - arg.tStart, L.aAcc, L.aDec, L.holdBefore, L.holdAfter, s)) {
			for (int c = 0; c < nComponents; c++)
				tx[c * component + m] = kAbsent;
			continue;
		}
		Pose p;
		if (nEdges == 0) {
			const PathRec only = recs[0];
			p = Pose { only.x, only.y, only.t };
		} else {
			const int e = ppl::edge_of(edgeS, nEdges, s);
			p = load_edge(A, recs, nPath, e, rslog, nRsLog).interpolate(ppl::ratio_of(s, edgeS[e - 1], edgeL[e - 1]));
		}
		tx[m] = p.x;
		tx[component + m] = p.y;
		tx[2 * component + m] = p.t;
		tx[3 * component + m] = s;
		if (withHeading) { // (wave-uniform)
			double sn, cs;
			sincos(p.t, &sn, &cs);
			tx[4 * component + m] = sn;
			tx[5 * component + m] = cs;
		}
		if (nPresent == 0) { // (a lane's times ascend)
			first = m;
			sEnter = s;
		}
		last = m;
		sLeave = s;
		nPresent++;
	}
	// ---------------- 3: the record
	for (int off = 32; off > 0; off >>= 1) {
		const int oFirst = __shfl_xor(first, off, 64), oLast = __shfl_xor(last, off, 64);
		const double oEnter = __shfl_xor(sEnter, off, 64), oLeave = __shfl_xor(sLeave, off, 64);
		nPresent += __shfl_xor(nPresent, off, 64);
		if (oFirst < first) {
			first = oFirst;
			sEnter = oEnter;
		}
		if (oLast > last) {
			last = oLast;
			sLeave = oLeave;
		}
	}
	if (lane == 0) {
		rec.status = nPresent > 0 ? 0 : 1;
		rec.n_present = nPresent;
		if (nPresent > 0) {
			rec.first = first;
			rec.last = last;
			rec.s_enter = sEnter;
			rec.s_leave = sLeave;
		}
		out[q] = rec;
	}
}

__global__ void __launch_bounds__(kConflictLanes) k_conflict_pairs(Footprint F, ConflictLattice L, int nPlans, long long nPairs, const int32_t* __restrict__ pairs,
	const double* __restrict__ traj, const pp_trajectory_result* __restrict__ plans, pp_conflict_result* __restrict__ out)
{
	const long long p = blockIdx.x;
	const int lane = threadIdx.x;
	if (p >= nPairs)
		return;
	int a, b;
	if (pairs) {
		a = pairs[2 * p];
		b = pairs[2 * p + 1];
	} else
		ppc::pair_of(nPlans, p, a, b);
	constexpr double kInf = __builtin_huge_val();
	pp_conflict_result rec {}; // (every field zero)
	if (plans[a].status < 0 || plans[b].status < 0) {
		rec.status = -1;
		if (lane == 0)
			out[p] = rec;
		return;
	}
	const size_t T = (size_t)L.T, component = (size_t)nPlans * T;
	const double *const xa = traj + (size_t)a * T, *const xb = traj + (size_t)b * T; // component c at + c * component
	int nTimes = 0, nConflict = 0, mFirst = -1, mMin = -1;
	double tauFirst = kInf, sepMin = kInf, tauMin = kInf;
	for (int m = lane; m < L.T; m += kConflictLanes) {
		const double ax = xa[m], bx = xb[m];
		if (ax != ax || bx != bx) // (absent)
			continue;
		const double ay = xa[component + m], by = xb[component + m];
		double asn = 0.0, acs = 1.0, bsn = 0.0, bcs = 1.0;
		if (F.anyOffset) { // (wave-uniform)
			asn = xa[4 * component + m];
			acs = xa[5 * component + m];
			bsn = xb[4 * component + m];
			bcs = xb[5 * component + m];
		}
		double sep = kInf;
		for (int i = 0; i < F.n; i++) { // (wave-uniform trip counts)
			double cax, cay;
			disc_centre(F, i, ax, ay, asn, acs, cax, cay);
			for (int j = 0; j < F.n; j++) {
				double cbx, cby;
				disc_centre(F, j, bx, by, bsn, bcs, cbx, cby);
				sep = ppv::min_of(sep, ppc::separation(cax - cbx, cay - cby, (double)F.r[i], (double)F.r[j]));
			}
		}
		const double tau = ppc::lattice_time(L.k0, m, L.dt);
		nTimes++;
		if (ppc::in_conflict(sep, L.margin)) {
			nConflict++;
			if (ppc::earlier(tau, tauFirst)) {
				tauFirst = tau;
				mFirst = m;
			}
		}
		if (mMin < 0 || ppc::closer(sep, tau, sepMin, tauMin)) {
			sepMin = sep;
			tauMin = tau;
			mMin = m;
		}
	}
	for (int off = 32; off > 0; off >>= 1) {
		const double oTauFirst = __shfl_xor(tauFirst, off, 64), oSep = __shfl_xor(sepMin, off, 64), oTauMin = __shfl_xor(tauMin, off, 64);
		const int oFirst = __shfl_xor(mFirst, off, 64), oMin = __shfl_xor(mMin, off, 64);
		nTimes += __shfl_xor(nTimes, off, 64);
		nConflict += __shfl_xor(nConflict, off, 64);
		if (oFirst >= 0 && (mFirst < 0 || ppc::earlier(oTauFirst, tauFirst))) {
			tauFirst = oTauFirst;
			mFirst = oFirst;
		}
		if (oMin >= 0 && (mMin < 0 || ppc::closer(oSep, oTauMin, sepMin, tauMin))) {
			sepMin = oSep;
			tauMin = oTauMin;
			mMin = oMin;
		}
	}
	if (lane == 0) {
		rec.min_separation = kInf;
		if (nTimes == 0)
			rec.status = 2;
		else {
			rec.status = nConflict > 0 ? 1 : 0;
			rec.n_times = nTimes;
			rec.n_conflict = nConflict;
			if (nConflict > 0) {
				rec.t_first = tauFirst;
				rec.s_first[0] = xa[3 * component + mFirst];
				rec.s_first[1] = xb[3 * component + mFirst];
			}
			rec.min_separation = sepMin;
			rec.t_min = tauMin;
			rec.s_min[0] = xa[3 * component + mMin];
			rec.s_min[1] = xb[3 * component + mMin];
		}
		out[p] = rec;
	}
}

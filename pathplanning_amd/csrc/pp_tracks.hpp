// Start delays that also clear tracked movers -- discs that move along timed waypoints and belong to nobody's plans (include/pp_hip.h, "start delays
// that clear conflicts and tracked movers").  Included by pp_planner.hip behind pp_deconflict.hpp: it reads the extended trajectory k_trajectory_tickets
// writes (pp_conflicts.hpp) as k_delay_level does, the uploaded track set, and nothing else.  It reads no map and writes nothing but its own buffers.
// The waypoint search, the track's position and the partner index of a track are pp_track_rule.hpp's; column, key and levels are pp_delay_rule.hpp's;
// discs and separation are the conflict call's (disc_centre, ppc::separation, ppc::in_conflict).
//   k_track_samples       workgroup k (64 lanes) samples track k on the T lattice times of k0 .. k1 (tracks are never delayed): lanes take m = lane,
//                         lane + 64, ... and write x and y, one array per component, track-major: samples[(c * M + k) * T + m], a NaN in both where the
//                         track is absent.  Consecutive lanes store, and later load, consecutive addresses: the trajectory's layout.
//   k_delay_level_tracks  workgroup v (64 lanes) decides vehicle i = members[v] of one level.  It restates k_delay_level's scan of the lower-index
//                         partners and, at a lattice time without a vehicle conflict (a track's key is above every vehicle's there), scans the M
//                         tracks in ascending order up to the first one in conflict.  One min-reduction of the key m * (n + M) + partner by shuffles;
//                         no key: the candidate is clear.  Lane 0 writes delays[i] and the pp_delay_result.
//   k_track_pairs         workgroup i * M + k (64 lanes): k_conflict_pairs with vehicle i at column m + D - c_i, c_i its reported candidate (its delay, or
//                         D for status 1), and the samples of track k as the other party.  Launched once behind the last level: every delay record is
//                         there.  Only min and integer sums are formed across lanes.
// Every loop is bounded by D, T, M and the partner count.  No LDS.
#pragma once

static_assert(sizeof(pp_track_set) == 32, "pp_track_set layout");
static_assert(sizeof(pp_track_result) == 64, "pp_track_result layout");

constexpr int kTrackLanes = 64;

struct TrackView { // the uploaded track set and its samples, as the kernels see them
	int M;
	const int32_t* offsets;  // [M + 1]
	const double* waypoints; // [offsets[M]][3]
	const double* radii;     // [M]
	double* samples;         // [2][M][T]
};

__global__ void __launch_bounds__(kTrackLanes) k_track_samples(ConflictLattice L, TrackView K)
{
	const int k = blockIdx.x, lane = threadIdx.x;
	if (k >= K.M)
		return;
	const int first = K.offsets[k], W = K.offsets[k + 1] - first;
	const double* const waypoints = K.waypoints + 3 * (size_t)first;
	const size_t T = (size_t)L.T, component = (size_t)K.M * T;
	double* const sx = K.samples + (size_t)k * T;
	constexpr double kAbsent = __builtin_nan("");
	for (int m = lane; m < L.T; m += kTrackLanes) {
		double x = kAbsent, y = kAbsent;
		if (!ppk::position(waypoints, W, ppc::lattice_time(L.k0, m, L.dt), x, y))
			x = y = kAbsent;
		sx[m] = x;
		sx[component + m] = y;
	}
}

__global__ void __launch_bounds__(kDelayLanes) k_delay_level_tracks(Footprint F, ConflictLattice L, int D, int nPlans, int nMembers, const int32_t* __restrict__ members,
	const int32_t* __restrict__ offsets, const int32_t* __restrict__ partners, const ConflictArg* __restrict__ args, const double* __restrict__ traj,
	const pp_trajectory_result* __restrict__ plans, int nTracks, const double* __restrict__ samples, const double* __restrict__ radii, int32_t* delays,
	pp_delay_result* __restrict__ out)
{
	const int v = blockIdx.x, lane = threadIdx.x;
	if (v >= nMembers)
		return;
	const int i = members[v];
	pp_delay_result rec {}; // (every field zero)
	rec.delay_steps = rec.blocker = -1;
	if (plans[i].status < 0) {
		rec.status = -1;
		if (lane == 0) {
			delays[i] = -1;
			out[i] = rec;
		}
		return;
	}
	const size_t columns = (size_t)L.T + (size_t)D, component = (size_t)nPlans * columns;
	const size_t T = (size_t)L.T, trackComponent = (size_t)nTracks * T;
	const double* const xi = traj + (size_t)i * columns; // component c at + c * component
	const int pFirst = offsets[i], pEnd = offsets[i + 1];
	uint64_t blocker = ppy::kNoKey;
	int dBlocked = 0, chosen = -1, nTried = 0;
	for (int d = 0; d <= D; d++) { // (wave-uniform)
		uint64_t best = ppy::kNoKey;
		for (int m = lane; m < L.T && best == ppy::kNoKey; m += kDelayLanes) {
			const size_t ci = (size_t)ppy::column(m, D, d);
			const double ax = xi[ci];
			if (ax != ax) // (absent)
				continue;
			const double ay = xi[component + ci];
			double asn = 0.0, acs = 1.0;
			if (F.anyOffset) { // (wave-uniform)
				asn = xi[4 * component + ci];
				acs = xi[5 * component + ci];
			}
			for (int k = pFirst; k < pEnd; k++) {
				const int j = partners[k];
				const int dj = delays[j];
				if (dj < 0) // (not scheduled: as if absent)
					continue;
				const double* const xj = traj + (size_t)j * columns;
				const size_t cj = (size_t)ppy::column(m, D, dj);
				const double bx = xj[cj];
				if (bx != bx)
					continue;
				const double by = xj[component + cj];
				double bsn = 0.0, bcs = 1.0;
				if (F.anyOffset) {
					bsn = xj[4 * component + cj];
					bcs = xj[5 * component + cj];
				}
				double sep = __builtin_huge_val();
				for (int a = 0; a < F.n; a++) { // (wave-uniform trip counts)
					double cax, cay;
					disc_centre(F, a, ax, ay, asn, acs, cax, cay);
					for (int b = 0; b < F.n; b++) {
						double cbx, cby;
						disc_centre(F, b, bx, by, bsn, bcs, cbx, cby);
						sep = ppv::min_of(sep, ppc::separation(cax - cbx, cay - cby, (double)F.r[a], (double)F.r[b]));
					}
				}
				if (ppc::in_conflict(sep, L.margin)) {
					const uint64_t key = ppk::key(m, nPlans, nTracks, j);
					if (ppy::before(key, best))
						best = key;
				}
			}
			// the tracks, partners n .. n + M - 1: above every vehicle at this time, ascending among themselves
			for (int k = 0; k < nTracks && best == ppy::kNoKey; k++) {
				const double tx = samples[(size_t)k * T + m];
				if (tx != tx)
					continue;
				const double ty = samples[trackComponent + (size_t)k * T + m], R = radii[k];
				double sep = __builtin_huge_val();
				for (int a = 0; a < F.n; a++) {
					double cax, cay;
					disc_centre(F, a, ax, ay, asn, acs, cax, cay);
					sep = ppv::min_of(sep, ppc::separation(cax - tx, cay - ty, (double)F.r[a], R));
				}
				if (ppc::in_conflict(sep, L.margin))
					best = ppk::key(m, nPlans, nTracks, ppk::partner_of_track(nPlans, k));
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)best, off, 64);
			if (ppy::before(other, best))
				best = other;
		}
		nTried++;
		if (best == ppy::kNoKey) {
			chosen = d;
			break;
		}
		blocker = best;
		dBlocked = d;
	}
	if (lane != 0)
		return;
	rec.status = chosen >= 0 ? 0 : 1;
	rec.delay_steps = chosen;
	rec.n_tried = nTried;
	rec.t_start = chosen >= 0 ? args[i].tStart + (double)chosen * L.dt : args[i].tStart;
	if (blocker != ppy::kNoKey) {
		const int m = ppk::time_of(blocker, nPlans, nTracks), j = ppk::partner_of(blocker, nPlans, nTracks);
		rec.blocker = j;
		rec.t_block = ppc::lattice_time(L.k0, m, L.dt);
		rec.s_block[0] = xi[3 * component + (size_t)ppy::column(m, D, dBlocked)];
		if (!ppk::is_track(nPlans, j)) // (a track has no arc length: zero)
			rec.s_block[1] = traj[(size_t)j * columns + 3 * component + (size_t)ppy::column(m, D, delays[j])];
	}
	delays[i] = chosen;
	out[i] = rec;
}

__global__ void __launch_bounds__(kTrackLanes) k_track_pairs(Footprint F, ConflictLattice L, int D, int nPlans, int nTracks, const double* __restrict__ traj,
	const pp_delay_result* __restrict__ decided, const double* __restrict__ samples, const double* __restrict__ radii, pp_track_result* __restrict__ out)
{
	const long long p = blockIdx.x;
	const int lane = threadIdx.x;
	if (p >= (long long)nPlans * nTracks)
		return;
	const int i = (int)(p / nTracks), k = (int)(p % nTracks);
	constexpr double kInf = __builtin_huge_val();
	pp_track_result rec {}; // (every field zero)
	const int status = decided[i].status;
	if (status < 0) {
		rec.status = -1;
		if (lane == 0)
			out[p] = rec;
		return;
	}
	const int candidate = status == 0 ? decided[i].delay_steps : D; // the reported candidate
	const size_t columns = (size_t)L.T + (size_t)D, component = (size_t)nPlans * columns;
	const size_t T = (size_t)L.T, trackComponent = (size_t)nTracks * T;
	const double* const xa = traj + (size_t)i * columns + (size_t)ppy::column(0, D, candidate); // time m, component c at xa[c * component + m]
	const double* const xb = samples + (size_t)k * T;
	const double R = radii[k];
	int nTimes = 0, nConflict = 0, mFirst = -1, mMin = -1;
	double tauFirst = kInf, sepMin = kInf, tauMin = kInf;
	for (int m = lane; m < L.T; m += kTrackLanes) {
		const double ax = xa[m], bx = xb[m];
		if (ax != ax || bx != bx) // (absent)
			continue;
		const double ay = xa[component + m], by = xb[trackComponent + m];
		double asn = 0.0, acs = 1.0;
		if (F.anyOffset) { // (wave-uniform)
			asn = xa[4 * component + m];
			acs = xa[5 * component + m];
		}
		double sep = kInf;
		for (int a = 0; a < F.n; a++) { // (wave-uniform trip count)
			double cax, cay;
			disc_centre(F, a, ax, ay, asn, acs, cax, cay);
			sep = ppv::min_of(sep, ppc::separation(cax - bx, cay - by, (double)F.r[a], R));
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
				rec.s_first = xa[3 * component + mFirst];
			}
			rec.min_separation = sepMin;
			rec.t_min = tauMin;
			rec.s_min = xa[3 * component + mMin];
		}
		out[p] = rec;
	}
}

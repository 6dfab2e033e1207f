// How long must a lower-priority vehicle wait at its start so that it stays clear of those above it (include/pp_hip.h, "start delays that clear
// conflicts")?  Included by pp_planner.hip behind pp_conflicts.hpp: it reads the trajectory layout k_trajectory_tickets writes -- here the EXTENDED
// trajectory of T + D columns per plan, an unchanged launch of that kernel over the lattice indices k0 - D .. k1 -- and nothing else of a plan.  It
// reads no map and writes nothing but its own buffers.  The column of a delayed vehicle, the key of a conflict and the levels are
// pp_delay_rule.hpp's; discs and separation are the conflict call's (disc_centre, ppc::separation, ppc::in_conflict).
//   k_delay_level  workgroup v (64 lanes) decides vehicle i = members[v] of one level: every partner j < i of its list was decided by an earlier
//                  launch on the same stream, and that order is the only synchronisation there is.
// Candidates d = 0, 1, .. D ascend, the same for the whole wave.  Per candidate the lanes take m = lane, lane + 64, ...: the vehicle's own column
// m + D - d once, then its partners -- the partner's delay from `delays` (negative: not scheduled, ignored), its column m + D - d_j, the separation
// through the stored sin / cos as k_conflict_pairs forms it.  A lane stops at its first time in conflict (its later times have larger keys) after
// it has seen every partner there; the wave's smallest key (m, j) is one min-reduction by shuffles; no key: the candidate is clear, the wave
// leaves the loop, lane 0 writes the record and the vehicle's delay.  Every loop is bounded by D, T and the partner count.
#pragma once

static_assert(sizeof(pp_delay_params) == 48, "pp_delay_params layout");
static_assert(sizeof(pp_delay_result) == 48, "pp_delay_result layout");

constexpr int kDelayLanes = 64;

__global__ void __launch_bounds__(kDelayLanes) k_delay_level(Footprint F, ConflictLattice L, int D, int nPlans, int nMembers, const int32_t* __restrict__ members,
	const int32_t* __restrict__ offsets, const int32_t* __restrict__ partners, const ConflictArg* __restrict__ args, const double* __restrict__ traj,
	const pp_trajectory_result* __restrict__ plans, int32_t* delays, pp_delay_result* __restrict__ out)
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
		const int m = ppy::time_of(blocker, nPlans), j = ppy::partner_of(blocker, nPlans);
		rec.blocker = j;
		rec.t_block = ppc::lattice_time(L.k0, m, L.dt);
		rec.s_block[0] = xi[3 * component + (size_t)ppy::column(m, D, dBlocked)];
		rec.s_block[1] = traj[(size_t)j * columns + 3 * component + (size_t)ppy::column(m, D, delays[j])];
	}
	delays[i] = chosen;
	out[i] = rec;
}

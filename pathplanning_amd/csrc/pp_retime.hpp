// Decided waits written into the timetable a speed-profile call left on the device: a hold of w seconds at a stop of row r is t_k += w for every
// k >= r (include/pp_hip.h, "decided waits written into the timetables").  Included by pp_planner.hip behind pp_timetable.hpp.  It reads no plan
// record and no map: only the (s, v, t) rows where k_speed_profile_tickets left them, whose t column it rewrites in place, and its own buffers.  The
// arithmetic is pp_retime_rule.hpp's, which host programs run too.
//   k_retime_tickets  workgroup i (64 lanes) works on the profile rows of args[i] (a ConflictArg whose start time is not read) with the holds
//                     holds[offsets[i] .. offsets[i + 1]) of the call's list, ascending by row, and writes out[i].
// Dynamic LDS: the prefix sums P_h of the plan's holds, 8 bytes each (the launch gives 8 * the most holds of one plan: at most 8 KiB).
//  1. the lanes take holds lane, lane + 64, ...: v_r, t_r and row r - 1 of the ORIGINAL rows give the two predicates; a ballot per block of 64 and
//     a running minimum give the first offending hold in list order.  No atomic.  A plan with an offender is left as it is;
//  2. lane 0 forms P_h sequentially into LDS;
//  3. behind a barrier the wave walks the rows from the first hold's row to N - 1, 64 at a time: each lane finds h(k) by binary search in the
//     plan's hold rows and stores t_k + P_h(k) -- 16 of every 24 row bytes move, and that is what bounds the kernel;
//  4. lane 0 writes the record.
#pragma once

static_assert(sizeof(pp_hold) == 16, "pp_hold layout");
static_assert(sizeof(pp_retime_result) == 40, "pp_retime_result layout");
static_assert(sizeof(pp_hold) == ppr::kHoldInts * 4 && sizeof(pp_hold) == ppr::kHoldDoubles * 8 && offsetof(pp_hold, row) == 4 && offsetof(pp_hold, seconds) == 8,
	"pp_hold as pp_retime_rule.hpp sees it");

struct RetimeCall { // what the kernel knows of a call
	int maxSamples;    // the stride of the profile rows, in samples
	int reserved;
	double aAcc, aDec; // of the speed-profile call whose rows these are
};

constexpr int kRetimeLanes = 64;
/// dynamic LDS of a k_retime_tickets launch whose longest per-plan hold list has `most` entries
inline size_t retime_lds_bytes(int most) { return (size_t)most * 8; }

__global__ void __launch_bounds__(kRetimeLanes) k_retime_tickets(RetimeCall C, int nPlans, const ConflictArg* __restrict__ args, const int32_t* __restrict__ offsets,
	const pp_hold* __restrict__ holds, double* rows, pp_retime_result* __restrict__ out)
{
	extern __shared__ double retimeLds[]; // P_h
	const int q = blockIdx.x, lane = threadIdx.x;
	if (q >= nPlans)
		return;
	const ConflictArg arg = args[q];
	pp_retime_result rec {}; // (every field zero)
	rec.bad_hold = -1;
	if (arg.nSamples < 1 || arg.nSamples > C.maxSamples) {
		rec.status = ppr::kNoProfile;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	const int N = arg.nSamples, first = offsets[q];
	int count = offsets[q + 1] - first;
	count = count < 0 ? 0 : (count > ppr::kMaxHolds ? ppr::kMaxHolds : count); // (the host refuses more)
	double* const row = rows + (size_t)arg.row * (size_t)C.maxSamples * 3;
	const pp_hold* const hold = holds + first;
	const double before = row[3 * (size_t)(N - 1) + 2];
	rec.n_holds = count;
	rec.first_row = -1;
	rec.duration_before = before;
	rec.duration = before;
	// ---------------- 1: the first offending hold, on the rows as they are
	int bad = -1;
	for (int base = 0; base < count && bad < 0; base += kRetimeLanes) {
		const int h = base + lane;
		const bool offends = h < count && ppr::hold_status(row, N, hold[h].row, hold[h].seconds, C.aAcc, C.aDec) != ppr::kApplied;
		const unsigned long long offending = __ballot(offends);
		if (offending)
			bad = base + __ffsll((long long)offending) - 1;
	}
	if (bad >= 0) { // (the same in every lane)
		rec.status = ppr::hold_status(row, N, hold[bad].row, hold[bad].seconds, C.aAcc, C.aDec);
		rec.bad_hold = first + bad;
		if (lane == 0)
			out[q] = rec;
		return;
	}
	if (count == 0) {
		if (lane == 0)
			out[q] = rec;
		return;
	}
	// ---------------- 2: P_h
	if (lane == 0)
		ppr::prefix(&hold->seconds, ppr::kHoldDoubles, count, retimeLds);
	__syncthreads(); // P_h to every lane; and every read of step 1 lies before the first store of step 3
	// ---------------- 3: t'_k = t_k + P_h(k)
	const int from = hold[0].row;
	for (int base = from; base < N; base += kRetimeLanes) {
		const int k = base + lane;
		if (k < N) {
			const int h = ppr::hold_of(&hold->row, ppr::kHoldInts, count, k); // (>= 0: k >= the first hold's row)
			row[3 * (size_t)k + 2] = ppr::retimed(row[3 * (size_t)k + 2], retimeLds[h]);
		}
	}
	// ---------------- 4: the record
	if (lane == 0) {
		rec.first_row = from;
		rec.held = retimeLds[count - 1];
		rec.duration = ppr::retimed(before, retimeLds[count - 1]); // (row N - 1 belongs to the last hold; the bits lane (N - 1 - from) % 64 stored)
		out[q] = rec;
	}
}

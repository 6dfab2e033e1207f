// Which pairs of held plans can meet at all (include/pp_hip.h, "the pairs that can meet")?  A space-time broad phase for the conflict call and the
// delay calls, which all take a pair list.  Included by pp_planner.hip behind pp_deconflict.hpp: it reads the x and y components of the EXTENDED
// trajectory k_trajectory_tickets writes over k0 - D .. k1 (T + D columns per plan, plan-major) and nothing else of a plan; it reads no map and
// writes nothing but its own buffers.  The boxes, the reach and the test are pp_pair_rule.hpp's.  Three kernels, every workgroup one wave of 64 lanes:
//   k_plan_boxes       workgroup i: per block b of B lattice times the bounding box of plan i's reference point over the columns a time of the block
//                      can read under any delay 0 .. D.  The lanes stride over the columns, the lanes' boxes are merged by xor-shuffles (min and max
//                      only: no result depends on the order), lane 0 writes.  One array per component and box-major, then plan:
//                      box[(c * NB + b) * n + i], so consecutive lanes of k_box_pairs (consecutive partners j) load consecutive addresses.
//   k_box_pairs<Fill>  workgroup i: row i of the pair matrix.  The lanes take the partners j = i + 1 + lane, + 64, ...; the blocks b ascend up to the
//                      lane's first hit, row i's own box of block b being the same for the whole wave.  Count pass (Fill = false): a ballot and a
//                      popcount per 64 partners, lane 0 writes the row's count.  Fill pass: the same code finds the same hits; a pair's place in the
//                      list is the row's offset, plus the hits of earlier chunks, plus the lane's rank inside the ballot -- ascending (i, j) without
//                      an atomic, so the list is the same bytes on every run.  Only places below maxPairs are written.
//   k_pair_offsets     one workgroup: the exclusive scan of the n row counts (int64), behind it the total and the number of plans with a box.
// The three run one behind the other on the holder's stream; that order is the only synchronisation there is.
#pragma once

static_assert(sizeof(pp_pair_params) == 56, "pp_pair_params layout");
static_assert(sizeof(pp_pair_summary) == 32, "pp_pair_summary layout");

constexpr int kPairLanes = 64;
constexpr int kBoxComponents = 4; // xmin, ymin, xmax, ymax

struct BoxView { // the boxes of a call: component c of box b of plan i at box[(c * NB + b) * n + i]
	int n, NB;
	double* box;
	__device__ __forceinline__ ppb::Box load(int b, int i) const
	{
		const size_t stride = (size_t)NB * (size_t)n, at = (size_t)b * (size_t)n + (size_t)i;
		return ppb::Box { box[at], box[stride + at], box[2 * stride + at], box[3 * stride + at] };
	}
	__device__ __forceinline__ void store(int b, int i, const ppb::Box& v) const
	{
		const size_t stride = (size_t)NB * (size_t)n, at = (size_t)b * (size_t)n + (size_t)i;
		box[at] = v.xmin;
		box[stride + at] = v.ymin;
		box[2 * stride + at] = v.xmax;
		box[3 * stride + at] = v.ymax;
	}
};

__global__ void __launch_bounds__(kPairLanes) k_plan_boxes(int T, int D, int B, BoxView V, const double* __restrict__ traj, int32_t* __restrict__ boxed)
{
	const int i = blockIdx.x, lane = threadIdx.x;
	if (i >= V.n)
		return;
	const size_t columns = (size_t)T + (size_t)D, component = (size_t)V.n * columns;
	const double* const x = traj + (size_t)i * columns; // y at + component
	int any = 0;
	for (int b = 0; b < V.NB; b++) { // (wave-uniform)
		const int64_t from = ppb::first_column(b, B), to = ppb::last_column(b, B, T, D);
		ppb::Box mine = ppb::no_box();
		for (int64_t c = from + lane; c <= to; c += kPairLanes)
			ppb::accumulate(mine, x[c], x[component + c]);
		for (int off = 32; off > 0; off >>= 1) {
			const ppb::Box other { __shfl_xor(mine.xmin, off, 64), __shfl_xor(mine.ymin, off, 64), __shfl_xor(mine.xmax, off, 64), __shfl_xor(mine.ymax, off, 64) };
			ppb::merge(mine, other);
		}
		if (lane == 0)
			V.store(b, i, mine);
		any |= ppb::exists(mine) ? 1 : 0;
	}
	if (lane == 0)
		boxed[i] = any;
}

template <bool Fill>
__global__ void __launch_bounds__(kPairLanes) k_box_pairs(BoxView V, double reach, long long maxPairs, const long long* __restrict__ offsets, long long* __restrict__ counts,
	int32_t* __restrict__ pairs, int32_t* __restrict__ firstBox)
{
	const int i = blockIdx.x, lane = threadIdx.x;
	if (i >= V.n)
		return;
	const long long base = Fill ? offsets[i] : 0;
	if (Fill && base >= maxPairs) // (the row's places, and those of every row behind it, lie behind the caller's rows)
		return;
	long long found = 0;
	for (int first = i + 1; first < V.n; first += kPairLanes) { // (wave-uniform)
		const int j = first + lane;
		bool live = j < V.n;
		int hit = -1;
		for (int b = 0; b < V.NB && __any(live); b++) {
			const ppb::Box mine = V.load(b, i); // (the same for every lane)
			if (live && ppb::can_meet(mine, V.load(b, j), reach)) {
				hit = b;
				live = false;
			}
		}
		const unsigned long long hits = __ballot(hit >= 0);
		if (Fill && hit >= 0) {
			const long long at = base + found + (long long)__popcll(hits & ((1ull << lane) - 1ull));
			if (at < maxPairs) {
				pairs[2 * at] = i;
				pairs[2 * at + 1] = j;
				firstBox[at] = hit;
			}
		}
		found += (long long)__popcll(hits);
	}
	if (!Fill && lane == 0)
		counts[i] = found;
}

/// offsets[0 .. n - 1]: the exclusive scan of counts; offsets[n]: the total; offsets[n + 1]: how many plans have a box.  One wave: 64 counts per step, an
/// inclusive scan by shuffles, the running total carried along (integers: exact in any order)
__global__ void __launch_bounds__(kPairLanes) k_pair_offsets(int n, const long long* __restrict__ counts, const int32_t* __restrict__ boxed, long long* __restrict__ offsets)
{
	const int lane = threadIdx.x;
	long long carry = 0, nBoxed = 0;
	for (int first = 0; first < n; first += kPairLanes) { // (wave-uniform)
		const int i = first + lane;
		const long long mine = i < n ? counts[i] : 0;
		long long upTo = mine;
		for (int off = 1; off < kPairLanes; off <<= 1) {
			const long long below = __shfl_up(upTo, off, 64);
			if (lane >= off)
				upTo += below;
		}
		if (i < n) {
			offsets[i] = carry + (upTo - mine);
			nBoxed += boxed[i] != 0 ? 1 : 0;
		}
		carry += __shfl(upTo, kPairLanes - 1, 64);
	}
	for (int off = 32; off > 0; off >>= 1)
		nBoxed += __shfl_xor(nBoxed, off, 64);
	if (lane == 0) {
		offsets[n] = carry;
		offsets[n + 1] = nBoxed;
	}
}

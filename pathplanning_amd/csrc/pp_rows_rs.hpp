// Out-of-line pieces of the rows kernels (pp_planner_rows.hpp): code a row enters rarely, kept out of the expansion loop's text.
//
// Included ONCE by pp_planner.hip (inside its anonymous namespace, after Node / SearchArgs / wave_lds_sync, before the two includes
// of pp_planner_rows.hpp).
//
// Why functions and not blocks of the kernel: the expansion loop is what eight search waves per pair of compute units run through, each
// at a point of its own, out of one instruction cache; the Reeds-Shepp attempt (0.9 % of the expansions) was more than half of the
// kernel's text and its register peak decided what the allocator spilled INSIDE the loop.  Called, its text lies outside the
// loop and its peak is its own ("code size and layout").
//
// Rules these functions keep:
//   * everything comes in BY VALUE and goes back by value: a row variable whose address escapes lives in scratch for the whole loop;
//   * what they need of the kernel's by-value arguments (SearchArgs, the footprint) is read from the kernel-argument segment itself
//     (rows_kernargs(): its address is taken in the kernel and passed as a number): scalar loads of memory that exists anyway -- handing
//     `A` over by reference makes a private copy of it per lane;
//   * a row enters whole (control flow diverges between rows, never inside one), so the row primitives work as in the kernel;
//   * no recursion, no indirect call: the private segment stays a static size (kMaxPrivateBytes, tests/test_kernel_resources.py);
//   * the arithmetic is the kernel's, expression by expression: results are compared byte for byte.
#pragma once

/// per-wave staging of the rows kernels in LDS: the children of the node being expanded (per row; kept until the next expansion so that a
/// child popped right away is read back from LDS instead of HBM), the spill buffer and the f-band counters of the open list
struct RowsWaveLds {
	static constexpr int kS = kRowsPerWave * kRowSlots;
	double c_x[kS], c_y[kS], c_t[kS], c_cost[kS], c_total[kS], c_len[kS], c_h[kS], c_sin[kS], c_cos[kS];
	double f_x[kS], f_y[kS], f_t[kS], f_tot[kS]; // open-list node already in the child's cell (shortcut test)
	HeapEntry spill[kRowsPerWave][kRowLanes];
	// f-bands of the open list (pp_search_device.hpp): entries per ring slot, four u8 counters per word
	uint32_t bandCnt[kRowsPerWave][kBands / 4];
	uint32_t c_key[kS], c_state[kS], f_for[kS];
	float c_d0[kS]; // obstacle distance at the child's pose (< 0: invalid state), see Node::dist0
	int rsChecks[kRowsPerWave];
	double rsPre[kRowsPerWave][24]; // rs::Path::make_prefix of the row's Reeds-Shepp attempt (23 doubles)
	int16_t c_action[kS];
	uint8_t c_flags[kS], c_valid[kS]; // flags: 1 = valid child, 2 = an earlier child of the batch shares its cell
};
static_assert(offsetof(RowsWaveLds, bandCnt) % 16 == 0 && sizeof(RowsWaveLds) % 16 == 0, "band counters are copied as uint4");

/// The head of the kernel-argument segment of every rows kernel: `SearchArgs A` is their first argument, and the footprint form's
/// `Footprint foot` their second (arguments lie in the segment at their natural alignment, as members do in a struct).
struct RowsKernargHead {
	SearchArgs A;
	Footprint foot; // k_hybrid_search_rows_footprint only
};
/// the segment's address, taken IN THE KERNEL (the builtin yields null in a called function) and handed on as a plain number
__device__ __forceinline__ uint64_t rows_kernarg_segment()
{
	return (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
}
/// ... and the called function's view of it: the number is wave-uniform (read from the first lane, so the compiler knows) and names constant
/// memory, so members are fetched with scalar loads
__device__ __forceinline__ const RowsKernargHead& rows_kernargs(const uint64_t segment)
{
	typedef const __attribute__((address_space(4))) RowsKernargHead* SegPtr;
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)segment), hi = __builtin_amdgcn_readfirstlane((uint32_t)(segment >> 32));
	return *(const RowsKernargHead*)(SegPtr)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

/// The KERNEL's view of its own by-value arguments inside the expansion loop.  Read as `A.member`, every member is a loop invariant: the compiler
/// loads them all in front of the loop, finds far more than a wave's ~100 SGPRs and parks the rest in lanes of a spill VGPR -- one v_readlane (a VALU
/// issue slot, a double two) per use inside the loop.  Here the segment's address passes through an empty asm, so the loads stay behind it: wide
/// scalar loads (one instruction on the scalar-memory port for up to sixteen dwords) of constant memory at the head of the phase that uses them, and
/// the values are dead at the phase's end.  Same memory, same values; DESIGN.md section 4.4, "scalar spills".
__device__ __forceinline__ const RowsKernargHead& rows_kernargs_here()
{
	typedef const __attribute__((address_space(4))) RowsKernargHead* SegPtr;
	uint64_t segment = rows_kernarg_segment();
	asm volatile("" : "+s"(segment));
	return *(const RowsKernargHead*)(SegPtr)(uintptr_t)segment;
}

/// The one copy of the f64 sincos that the constant-steer arcs of an expansion share (end point, Voronoi sample, march samples, truncation,
/// Voronoi term of a truncated arc): inlined, each use carries ocml's argument reduction and polynomials -- about 200 instructions and nine
/// hoisted coefficient pairs a site.  Values come and go in registers.
struct SinCosPair {
	double s, c;
};
__device__ __attribute__((noinline)) SinCosPair rows_arc_sincos(const double t)
{
	SinCosPair r;
	sincos(t, &r.s, &r.c);
	return r;
}
struct SinCosShared {
	PPD_INLINE static void eval(double t, double& s, double& c)
	{
		const SinCosPair r = rows_arc_sincos(t);
		s = r.s;
		c = r.c;
	}
};
using RowsArc = ArcSCT<SinCosShared>;

/// The libm calls of the Reeds-Shepp formulas (pp_rs_device.hpp: rs::MathInline), one out-of-line copy each: the twelve formula bodies, the
/// prefix and the march's samples hold some forty uses, and a row enters them on 0.9 % of its expansions -- inlined they were 96 KB of text
/// that a wave streamed through the instruction cache its neighbours run their loop from.
#define PP_ROWS_MATH1(name) \
	__device__ __attribute__((noinline)) double rows_##name(const double x) { return ::name(x); }
PP_ROWS_MATH1(sin)
PP_ROWS_MATH1(cos)
PP_ROWS_MATH1(acos)
PP_ROWS_MATH1(asin)
#undef PP_ROWS_MATH1
__device__ __attribute__((noinline)) double rows_atan2(const double y, const double x) { return ::atan2(y, x); }
__device__ __attribute__((noinline)) double rows_fmod(const double x, const double y) { return ::fmod(x, y); }
struct RowsMath {
	PPD_INLINE static double sin(double x) { return rows_sin(x); }
	PPD_INLINE static double cos(double x) { return rows_cos(x); }
	PPD_INLINE static double atan2(double y, double x) { return rows_atan2(y, x); }
	PPD_INLINE static double acos(double x) { return rows_acos(x); }
	PPD_INLINE static double asin(double x) { return rows_asin(x); }
	PPD_INLINE static double fmod(double x, double y) { return rows_fmod(x, y); }
};

/// The Reeds-Shepp path of an attempt as the march, the end pose and the Voronoi term see it (cf. rs::PrefixedPath): ONE copy of
/// interpolate_prefix -- five motions, straight or turn -- instead of one per use.  The path lies in the attempt's own frame.
__device__ __attribute__((noinline)) Pose rows_rs_interpolate(const rs::PathT<RowsMath>* const path, const double* const pre, const double ratio)
{
	return path->interpolate_prefix(pre, ratio);
}
struct RowsRsPath {
	const rs::PathT<RowsMath>* path;
	const double* pre;
	double length;
	PPD_INLINE Pose interpolate(double ratio) const { return rows_rs_interpolate(path, pre, ratio); }
};

/// what a Reeds-Shepp attempt hands back to its row (the candidate child itself is staged in slot kRowRs of the row's staging)
struct RowsRsResult {
	int word;     // the optimal word, -1: none (then nothing else is meaningful and nothing was marched)
	int checks;   // state checks of the march
	int valid;    // the march succeeded and the child is staged
	int boundary; // (lane 0 of the row) the child's DiscretizePose quotient lay on a lattice line: the guard-band count
	double t, u, v;
};

/// The Reeds-Shepp analytic expansion of one popped node (hybrid_a_star.cpp:81-88 after the gate; GetOptimalPath, reeds_shepp.cpp:654-683):
/// lane l of the row evaluates words l, l + 16, l + 32; the winner's path is marched by one lane; a valid one is staged as child kRowRs
/// with its cost, heuristic and key-map state.  The caller keeps the counters and pushes the staged child.
template <bool kFoot>
__device__ __attribute__((noinline)) RowsRsResult rows_rs_attempt(const double px, const double py, const double pt, const double pSin, const double pCos, const double gx_,
	const double gy_, const double gt_, const double pPathCost, const float* const field, const uint32_t* const keymap, RowsWaveLds* const Wp, const uint64_t kernargs)
{
	const RowsKernargHead& K = rows_kernargs(kernargs);
	const SearchArgs& A = K.A;
	const MapView& m = A.m;
	RowsWaveLds& W = *Wp;
	const int lane = threadIdx.x & 63;
	const int rl = lane & (kRowLanes - 1);
	const int row = lane >> 4;
	const int sb = row * kRowSlots;
	const Pose ppose = { px, py, pt };
	const Pose goal = { gx_, gy_, gt_ };
	RowsRsResult R;
	R.word = -1;
	R.checks = 0;
	R.valid = 0;
	R.boundary = 0;
	R.t = R.u = R.v = 0.0;
	Pose rel;
	{
		// goal - start (geometry/2dplane.h:65-79) with the stored sin/cos of the node's heading
		const double dx = goal.x - ppose.x, dy = goal.y - ppose.y;
		const double s = -pSin, c = pCos;
		rel.x = c * dx + (-s) * dy;
		rel.y = s * dx + c * dy;
		rel.t = wrap_theta(wrap_theta(goal.t - ppose.t));
	}
	rel.x = rel.x / A.rmin;
	rel.y = rel.y / A.rmin;
	float wcost = __builtin_huge_valf();
	int wword = 0x7FFFFFFF;
	double wt = 0, wu = 0, wv = 0;
#pragma unroll 1
	for (int k = 0; k < rs::kNumWords / kRowLanes; k++) {
		const int w = rl + kRowLanes * k;
		double gx, gy, gt, t_, u_, v_;
		rs::goal_variant(rel, w % 4, gx, gy, gt);
		const double length = rs::base_lengths<RowsMath>(w / 4, gx, gy, gt, t_, u_, v_);
		if (!(length == rs::inf())) {
			rs::Segment sg;
			rs::word_segment(w, t_, u_, v_, sg);
			const float cst = rs::compute_cost(sg, A.rmin, A.rsRev, A.rsFwd, A.rsSw);
			// NaN and +inf never win a `cost < optimalCost` test; words ascend, so the first strict minimum is kept
			if (cst < __builtin_huge_valf() && cst < wcost) {
				wcost = cst;
				wword = w;
				wt = t_;
				wu = u_;
				wv = v_;
			}
		}
	}
	// first strictly-lowest float cost in word order (costs are >= 0: their bit patterns order like the values)
	const uint32_t bestBits = row_min_u32(__float_as_uint(wcost));
	const bool mine = wword != 0x7FFFFFFF && __float_as_uint(wcost) == bestBits;
	const uint32_t wsel = row_min_u32(mine ? (uint32_t)wword : 0xFFFFFFFFu);
	const int word = wsel == 0xFFFFFFFFu ? -1 : (int)wsel;
	if (word < 0)
		return R;
	const int owner = word & (kRowLanes - 1);
	const double bt = row_read_f64(wt, lane, owner), bu = row_read_f64(wu, lane, owner), bv = row_read_f64(wv, lane, owner);
	// the winner's path is validated by one lane (the adaptive march is sequential)
	if (rl == 0) {
		rs::PathT<RowsMath> path;
		path.init = ppose;
		rs::word_segment(word, bt, bu, bv, path.seg);
		path.rmin = A.rmin;
		path.length = path.seg.length * A.rmin; // PathSegment::GetLength
		float lastRatio;
		int checks = 0;
		// every sample of the march continues from the stored start of its motion instead of walking the word from its
		// beginning (same operations on the same values: rs::Path::make_prefix)
		double* const pre = W.rsPre[row];
		path.make_prefix(pre);
		const RowsRsPath ppath = { &path, pre, path.length };
		bool valid;
		if constexpr (kFoot)
			valid = is_path_valid_fp(m, K.foot, fp_gain(K.foot, 1.0 / A.rmin), ppath, path.init, lastRatio, checks);
		else
			valid = is_path_valid(m, ppath, path.init, lastRatio, checks);
		W.c_valid[sb + kRowRs] = 0;
		W.rsChecks[row] = checks;
		if (valid) {
			const double pathAndSwitchingCosts = (double)rs::compute_cost(path.seg, A.rmin, A.rsRev, A.rsFwd, A.rsSw); // PathReedsShepp::ComputeCost
			const Pose child = ppath.interpolate(1.0);
			int ix, iy, it;
			R.boundary = discretize_pose(child, A.rp.lat, A.rp.headingAlias, ix, iy, it) ? 1 : 0;
			const double voro = voronoi_cost(m, ppath, A.rp.voroDiagRes, A.rp.voronoiMult);
			const double cost = pathAndSwitchingCosts + voro;
			uint32_t key;
			if (A.ks.pack(ix, iy, it, key)) {
				double s_, c_;
				SinCosShared::eval(child.t, s_, c_);
				const double hh = combined_heuristic_sc(A.heur, m, field, goal, child, s_, c_);
				W.c_valid[sb + kRowRs] = 1;
				W.c_key[sb + kRowRs] = key;
				W.c_x[sb + kRowRs] = child.x;
				W.c_y[sb + kRowRs] = child.y;
				W.c_t[sb + kRowRs] = child.t;
				W.c_cost[sb + kRowRs] = pPathCost + cost;
				W.c_total[sb + kRowRs] = (pPathCost + cost) + hh;
				W.c_len[sb + kRowRs] = path.length;
				W.c_h[sb + kRowRs] = hh;
				W.c_sin[sb + kRowRs] = s_;
				W.c_cos[sb + kRowRs] = c_;
				if constexpr (kFoot) {
					float rd0, rb;
					W.c_d0[sb + kRowRs] = fp_state_valid_sc(m, K.foot, child.x, child.y, child.t, s_, c_, rd0, rb) ? rd0 : -1.0f;
				} else {
					float rd0;
					W.c_d0[sb + kRowRs] = is_state_valid(m, child.x, child.y, child.t, rd0) ? rd0 : -1.0f;
				}
				W.c_state[sb + kRowRs] = keymap[key];
				W.c_action[sb + kRowRs] = (int16_t)(1000 + word);
			}
		}
	}
	wave_lds_sync();
	R.word = word;
	R.checks = W.rsChecks[row];
	R.valid = W.c_valid[sb + kRowRs];
	R.t = bt;
	R.u = bu;
	R.v = bv;
	return R;
}

/// what a row keeps of a query it has just claimed
struct RowsClaim {
	double gx, gy, gt; // the goal, theta wrapped
	int boundary;      // the start's DiscretizePose quotient lay on a lattice line (guard band)
};

/// A row that has claimed query q prepares its buffers (InitializeSearch, a_star.h:350-364): clears the slot's key map (it still holds the row's
/// previous query) and the f-band counters, seeds the engine, writes the root node and marks its cell explored.  The row's registers (open
/// list, counters) are reset by the caller, which also puts the root into the front buffer.
template <bool kFoot>
__device__ __attribute__((noinline)) RowsClaim rows_claim_init(const int q, const float* const field, Node* const nodes, uint32_t* const keymap, unsigned long long* const mt,
	uint32_t* const bandCnt, const double* const starts, const double* const goals, const uint64_t* const seeds, const uint64_t kernargs)
{
	const RowsKernargHead& K = rows_kernargs(kernargs);
	const SearchArgs& A = K.A;
	const MapView& m = A.m;
	const int rl = threadIdx.x & (kRowLanes - 1);
	{
		const size_t n = A.ks.size(), n4 = n / 4;
		const uint4 z = { 0, 0, 0, 0 };
		if ((((uintptr_t)keymap) & 15) == 0) {
			for (size_t i = rl; i < n4; i += kRowLanes)
				reinterpret_cast<uint4*>(keymap)[i] = z;
			for (size_t i = n4 * 4 + rl; i < n; i += kRowLanes)
				keymap[i] = 0;
		} else {
			for (size_t i = rl; i < n; i += kRowLanes)
				keymap[i] = 0;
		}
		wave_vmem_sync();
	}
	// goal / start poses go through the Pose2d constructor on the caller's side (theta wrapped)
	const Pose start = { starts[3 * q], starts[3 * q + 1], wrap_theta(starts[3 * q + 2]) };
	const Pose goal = { goals[3 * q], goals[3 * q + 1], wrap_theta(goals[3 * q + 2]) };
	wave_lds_sync();
	for (int i = rl; i < kBands / 4; i += kRowLanes)
		bandCnt[i] = 0u;
	wave_lds_sync();
	if (rl == 0)
		Mt64::seed(mt, seeds[q]);
	double rs_, rc_;
	sincos(start.t, &rs_, &rc_);
	int ix, iy, it;
	const bool startOnBoundary = discretize_pose(start, A.rp.lat, A.rp.headingAlias, ix, iy, it);
	uint32_t key = kNoKey;
	const bool ok = A.ks.pack(ix, iy, it, key);
	if (rl == 0) {
		Node root;
		root.x = start.x;
		root.y = start.y;
		root.t = start.t;
		root.pathCost = 0.0;
		root.totalCost = 0.0;
		root.length = 0.0;
		root.h = combined_heuristic_sc(A.heur, m, field, goal, start, rs_, rc_);
		root.sinT = rs_;
		root.cosT = rc_;
		root.parent = -1;
		root.key = ok ? key : kNoKey;
		root.action = -1;
		root.dead = 0;
		if constexpr (kFoot) {
			float cl, bd;
			root.dist0 = fp_state_valid_sc(m, K.foot, start.x, start.y, start.t, rs_, rc_, cl, bd) ? cl : -1.0f;
		} else {
			float d0;
			root.dist0 = is_state_valid(m, start.x, start.y, start.t, d0) ? d0 : -1.0f;
		}
		nodes[0] = root;
		if (ok)
			keymap[key] = kExplored; // the root is inserted in the explored set at init (a_star.h:361)
	}
	RowsClaim C;
	C.gx = goal.x;
	C.gy = goal.y;
	C.gt = goal.t;
	C.boundary = startOnBoundary ? 1 : 0;
	return C;
}

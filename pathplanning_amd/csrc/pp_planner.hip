// hybrid_astar_batch -- HybridAStar::SearchPath graph search (algo/hybrid_a_star.cpp:237-257,
// 59-173; algo/a_star.h:326-427; utils/frontier.h) for a batch of independent queries.
//
// Two kernels share the search state layout below:
//   k_hybrid_search       one wave per query (latency: the plugin's single-query path, profiling, and the
//                         continuation of queries the rows kernel hands over);
//   k_hybrid_search_rows  four queries per wave on a persistent grid (throughput; pp_planner_rows.hpp).
// k_hybrid_search -- one wave (64 lanes) per query, all per-query state in HBM:
//   lanes      = motion primitives of the node being expanded (rollout + IsPathValid +
//                Voronoi cost + heuristic per child), then the 48 Reeds-Shepp words of the
//                analytic expansion;
//   open list  = 64-ary heap, pop is one coalesced 1 KiB load + wave arg-min per level;
//   membership = dense key map over (x cell, y cell, heading bin): unseen / in the open list
//                (node index) / explored -- replaces Frontier::Find + the explored hash set;
//   RNG        = the query's own mt19937_64 (utils/random.h), twist done by the wave.
// Results are bit-identical to the sequential reference as long as libm and OCML agree on
// the discrete outcomes (cells, validity); continuous poses agree to ~1e-15.
#include "pp_search_device.hpp"
#include "pp_row_primitives.hpp"
#include "pp_stamp_rule.hpp"
#include "pp_locate_rule.hpp"
#include "pp_speed_rule.hpp"
#include "pp_conflict_rule.hpp"
#include "pp_delay_rule.hpp"
#include "pp_wait_rule.hpp"
#include "pp_track_rule.hpp"
#include "pp_pair_rule.hpp"
#include "pp_timetable_rule.hpp"
#include "pp_retime_rule.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

using namespace ppd;

namespace {

struct Node { // 96 bytes
	double x, y, t;
	double pathCost, totalCost;
	double length;     // arc length after truncation / RS path length
	double h;          // combined heuristic of this pose (reused as the RS gate input when it is expanded)
	double sinT, cosT; // sin / cos of t (reused as the initial-heading terms of the children's arcs)
	int32_t parent;
	uint32_t key;      // packed discrete pose
	int16_t action;    // -1 root, 0..P-1 constant-steer primitive, 1000 + word for Reeds-Shepp
	uint8_t dead;      // removed from the open list by ProcessPossibleShortcut
	uint8_t pad0;
	float dist0;       // obstacle distance at this pose, < 0 when the pose is not a valid state: the first sample of every
	                   // child arc's validity march (IsPathValid samples the start pose first) without a dependent load
	uint8_t pad[8];
};
static_assert(sizeof(Node) == 96, "Node layout");

/// One node of a solution path, written by the search kernel when the query ends (goal first, root last): the node
/// records themselves live in per-slot buffers that the next query of the slot overwrites.
struct PathRec {
	double x, y, t, length;
	int32_t action; // Node::action
	int32_t node;   // node index (matches RsLogEntry::node)
};
static_assert(sizeof(PathRec) == 40, "PathRec layout");

/// A query handed from the four-queries-per-wave kernel to the one-query-per-wave kernel after its first
/// `suspendAfter` expansions: everything that is not already in the slot's node / heap / key-map / engine buffers.
struct SuspendRec {
	int32_t q, slot;
	int32_t heapSize, nNodes, nExpanded, nRngDraws, nRsAttempts, nRsLog, mtIdx;
	uint32_t seq;
	long long stateChecks, pathChecks; // totals so far (arcs + Reeds-Shepp)
	long long bandLo;                  // bottom of the f-band window (slot counts are saved next to the bands)
	int32_t nOutside, pad;             // open-list entries in bands + heap
};

struct RsLogEntry {
	int32_t node, word;
	double t, u, v;
};
constexpr int kRsLogCap = 64;

struct KeySpace {
	int x0, y0, t0; // smallest representable discrete coordinate
	int nx, ny, nt;
	PPD_INLINE bool pack(int ix, int iy, int it, uint32_t& key) const
	{
		const int kx = ix - x0, ky = iy - y0, kt = it - t0;
		if (kx < 0 || kx >= nx || ky < 0 || ky >= ny || kt < 0 || kt >= nt)
			return false;
		key = (uint32_t)((kx * ny + ky) * nt + kt);
		return true;
	}
	__host__ __device__ void unpack(uint32_t key, int& ix, int& iy, int& it) const
	{
		it = (int)(key % (uint32_t)nt) + t0;
		const uint32_t r = key / (uint32_t)nt;
		iy = (int)(r % (uint32_t)ny) + y0;
		ix = (int)(r / (uint32_t)ny) + x0;
	}
	__host__ __device__ size_t size() const { return (size_t)nx * ny * nt; }
};

/// A child whose DiscretizePose quotient lay within 1e-9 cells of a lattice line (pp_device.hpp: near_integer), logged by the
/// one-query-per-wave kernel for pp_planner_certify_lattice: the node it was generated from, the primitive, the (possibly truncated)
/// arc length and the cell the DEVICE put it in.  kind 1: constant-steer child; 2: Reeds-Shepp child (not recomputable on the host)
struct GuardRec {
	int32_t parent;
	int16_t prim, kind;
	double length;
	int32_t ix, iy, it, pad;
};
static_assert(sizeof(GuardRec) == 32, "GuardRec layout");
constexpr int kGuardLogCap = 64; // records kept per query (the count goes on)

struct SearchArgs {
	MapView m;
	pph::RolloutParams rp;
	pph::PrimTable prims;
	HeurView heur;
	KeySpace ks;
	double rmin;
	float rsRev, rsFwd, rsSw; // Reeds-Shepp cost weights as floats (reeds_shepp.cpp:654)
	int maxNodes;
	int maxPath; // PathRec entries per query
	int suspendAfter;  // rows kernel: expansions after which a query is set aside for the one-query kernel (0 = never)
	int extraSlots;    // buffer slots beyond the rows' own, taken by rows whose query was set aside
	int searchRows;    // rows the planner's buffers were sized for (spare slots start here)
	int listCap;       // capacity of each SuspendRec list: one record per spare slot + one per row
	int rowsWaves;     // rows kernel: waves of this launch (the grid is rounded up to whole workgroups)
	size_t cells;
	int64_t fieldElems; // floats per query in costFields (8 x 8-tiled obstacle-heuristic field)
	GuardRec* guardLog; // [queries][kGuardLogCap], nullptr: no log (throughput planners)
	int* guardCount;    // [queries]
};

struct DevResult {
	pp_query_result r;
	int32_t solutionNode;
	int32_t nRsLog;
};

constexpr uint32_t kExplored = 0xFFFFFFFFu;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;


// kProfile: diagnostic build only -- accumulates shader-clock cycles per phase into `prof`
// (8 words per query); the product path launches kProfile = false, where no stamp executes.
// One wave per block: LDS operations of a wave complete in program order, so lanes only need the
// compiler not to reorder around the hand-off.  __syncthreads() would also drain every outstanding
// HBM store (s_waitcnt vmcnt(0)), ~1-2k cycles each time.
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}
/// waits until this wave's global stores are visible to its other lanes' loads
__device__ __forceinline__ void wave_vmem_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_wave_barrier();
}

/// GetPath (a_star.h:254-288): walks the parent chain from the solution node; records are written goal first.
/// Returns the number of nodes on the path (it may exceed `cap`: only the first `cap` records are stored).
/// hostPoses (pipeline: pp_pipeline_get_paths): the first hostCap poses also go, as (x, y, theta) triples in the same order, to the query's
/// slot of a ring in pinned host memory -- the plan leaves the GPU with its completion record, no copy and no kernel at fetch time.
__device__ inline int write_path(const Node* nodes, int solutionNode, PathRec* out, int cap, double* hostPoses = nullptr, int hostCap = 0)
{
	int depth = 0;
	for (int k = solutionNode; k >= 0;) {
		const Node nd = nodes[k];
		if (depth < hostCap) {
			hostPoses[3 * depth] = nd.x;
			hostPoses[3 * depth + 1] = nd.y;
			hostPoses[3 * depth + 2] = nd.t;
		}
		if (depth < cap) {
			PathRec pr;
			pr.x = nd.x;
			pr.y = nd.y;
			pr.t = nd.t;
			pr.length = nd.length;
			pr.action = nd.action;
			pr.node = k;
			out[depth] = pr;
		}
		depth++;
		k = nd.parent;
	}
	return depth;
}

__device__ __forceinline__ void guard_log(const SearchArgs& A, int q, int parent, int prim, int kind, double length, int ix, int iy, int it)
{
	if (!A.guardLog)
		return;
	const int pos = atomicAdd(A.guardCount + q, 1);
	if (pos < kGuardLogCap) {
		GuardRec r;
		r.parent = parent;
		r.prim = (int16_t)prim;
		r.kind = (int16_t)kind;
		r.length = length;
		r.ix = ix;
		r.iy = iy;
		r.it = it;
		r.pad = 0;
		A.guardLog[(size_t)q * kGuardLogCap + pos] = r;
	}
}

enum { PH_POP = 0, PH_LOAD, PH_HEUR, PH_CHILD, PH_DUP, PH_INSERT, PH_WRITE, PH_RS, PH_COUNT };
constexpr int kSlots = 65; // staging: one slot per lane + one for the Reeds-Shepp child
constexpr int kRsSlot = 64;

#ifndef PP_SEARCH_WAVES_PER_SIMD
#define PP_SEARCH_WAVES_PER_SIMD 2 // 256 VGPRs: no spills on the per-expansion critical path (128 + 4 batches in flight measured ~10 % faster but needs ~240 GB)
#endif
// The body of the one-wave-per-query search lives in pp_search_body.hpp and is compiled into two kernels: k_hybrid_search (kFootprint = false:
// the reference's point validator, `foot` unused) and k_hybrid_search_footprint (kFootprint = true: every "is this pose / arc / Reeds-Shepp
// path valid" goes through the footprint `foot`, pp_footprint_device.hpp, and Node::dist0 holds the footprint's clearance instead of the
// obstacle distance).  A textual include, not a shared device function: handing the kernel's arguments to a function changed the registers
// and scratch of k_hybrid_search, which tests/test_kernel_resources.py pins.
template <bool kProfile>
__global__ void __launch_bounds__(64, PP_SEARCH_WAVES_PER_SIMD) k_hybrid_search(SearchArgs A, int nQueries, const double* __restrict__ starts, const double* __restrict__ goals,
	const uint64_t* __restrict__ seeds, const float* __restrict__ costFields, Node* __restrict__ nodesBase, HeapEntry* __restrict__ heapBase,
	uint32_t* __restrict__ keymapBase, uint32_t* __restrict__ expandedBase, RsLogEntry* __restrict__ rsLogBase, PathRec* __restrict__ pathBase,
	DevResult* __restrict__ results, unsigned long long* __restrict__ prof, const SuspendRec* __restrict__ resume, const int* __restrict__ nResume,
	const unsigned long long* __restrict__ mtBase, HeapEntry* __restrict__ bandBase, double bandInvW, uint8_t* __restrict__ bandMetaBase)
{
	constexpr bool kFootprint = false;
	const Footprint foot {}; // placeholder: never read where !kFootprint
#define PP_SEARCH_BODY_INCLUDER 1
#include "pp_search_body.hpp"
#undef PP_SEARCH_BODY_INCLUDER
}

/// One wave per query with a vehicle footprint (pp_planner_set_footprint): batches only, no phase profile and no continuation of
/// set-aside queries (planners of the rows kernel take no footprint).
__global__ void __launch_bounds__(64, PP_SEARCH_WAVES_PER_SIMD) k_hybrid_search_footprint(SearchArgs A, Footprint foot, int nQueries, const double* __restrict__ starts,
	const double* __restrict__ goals, const uint64_t* __restrict__ seeds, const float* __restrict__ costFields, Node* __restrict__ nodesBase, HeapEntry* __restrict__ heapBase,
	uint32_t* __restrict__ keymapBase, uint32_t* __restrict__ expandedBase, RsLogEntry* __restrict__ rsLogBase, PathRec* __restrict__ pathBase,
	DevResult* __restrict__ results, HeapEntry* __restrict__ bandBase, double bandInvW, uint8_t* __restrict__ bandMetaBase)
{
	// placeholders for the arguments this kernel does not have: constants, so the body's profiling and continuation branches (`if (kProfile)`,
	// `resume ? ... : ...`) fold away at compile time
	constexpr bool kFootprint = true, kProfile = false;
	unsigned long long* const prof = nullptr;         // phase profile: not collected
	const SuspendRec* const resume = nullptr;         // no continuation of set-aside queries ...
	const int* const nResume = nullptr;               // ... so no count of them
	const unsigned long long* const mtBase = nullptr; // ... and no saved engine states
#define PP_SEARCH_BODY_INCLUDER 1
#include "pp_search_body.hpp"
#undef PP_SEARCH_BODY_INCLUDER
}

// ---- streaming pipeline (pp_pipeline.hpp): what the persistent search grid shares with the wavefront kernel and the host ----
/// device memory, zeroed at creation
struct PipeCtl {
	unsigned long long readyTail;  // field slots appended to the ready ring by the wavefront kernel (absolute count)
	unsigned long long readyHead;  // entries claimed by search rows
	unsigned long long doneTail;   // completion records reserved
	unsigned long long nSubmitted; // queries handed to the wavefront kernel so far (written by the host, in stream order before a top-up launch)
	int stop;                      // host: leave as soon as the rows are idle
	int pad;
	unsigned long long quiesce;    // host: every result of the first `quiesce` submitted queries has been polled -- idle waves need not wait for more
	unsigned long long urgentTail; // urgent ring (WavefrontPublish::urgent): entries appended by k_pipe_scatter
	unsigned long long urgentHead; // entries claimed by wavefront workgroups
};
/// completion record in PINNED HOST memory: the row writes the result, then the stamp ((position + 1) << 32 | slot); the host consumes
/// records in position order as their stamps appear
struct PipeDone {
	unsigned long long stamp;
	DevResult r;
	unsigned long long readyTail, readyHead; // the queue counters as the announcing row saw them (pp_pipeline_backlog)
};
struct PipeView {
	PipeCtl* ctl = nullptr; // nullptr: the kernel works on a batch (no pipeline)
	unsigned long long* ready = nullptr;
	unsigned long long readyMask = 0;
	PipeDone* done = nullptr;
	unsigned long long doneMask = 0;
	int* waveAlive = nullptr;         // [waves] 1 while a wave of some launch owns that wave index (and with it the rows' buffers)
	unsigned long long lingerTicks = 0; // loop passes an idle wave stays although every submitted query has been claimed: the next submission is usually on its way
	double* pathHost = nullptr;       // pinned host memory, [capacity][pathHostCap][3]: the solution path's poses, goal first (write_path)
	int pathHostCap = 0;
	unsigned long long idleTicks = 0; // loop passes (~4 us each: a sleep and three polls) a wave waits without work before it leaves on its own
};

// The rows kernel's text is compiled twice (see the head of pp_planner_rows.hpp): k_hybrid_search_rows<kPiped>, then
// k_hybrid_search_rows_footprint<kPiped>, of which only the pipeline form is instantiated (pp_pipeline_set_footprint).
#include "pp_rows_rs.hpp" // their out-of-line pieces: the Reeds-Shepp attempt, a claimed query's initialisation
#define PP_ROWS_FOOTPRINT 0
#include "pp_planner_rows.hpp"
#undef PP_ROWS_FOOTPRINT
#define PP_ROWS_FOOTPRINT 1
#include "pp_planner_rows.hpp"
#undef PP_ROWS_FOOTPRINT
// ... and so is the post-processing kernel's (see the head of pp_postprocess.hpp): k_postprocess, then k_postprocess_tickets
#define PP_POST_TICKETS 0
#include "pp_postprocess.hpp"
#undef PP_POST_TICKETS
#define PP_POST_TICKETS 1
#include "pp_postprocess.hpp"
#undef PP_POST_TICKETS
// re-validation of plans against a changed map (one wave per plan; PostEdge / load_edge of the file above)
#include "pp_revalidate.hpp"
// held plans stamped into a map's occupancy grid (one wave per plan; the same PostEdge / load_edge)
#include "pp_stamp.hpp"
// vehicles located on their held plans (one wave per plan; the same PostEdge / load_edge and the stamp's sample schedule)
#include "pp_locate.hpp"
// speed profiles and arrival times along held plans (one wave per plan; the same PostEdge / load_edge and the stamp's sample schedule)
#include "pp_speed_profile.hpp"
// space-time conflicts between held plans on the timetables of their speed profiles (one wave per plan, then one per pair; the same PostEdge / load_edge)
#include "pp_conflicts.hpp"
// start delays that clear those conflicts, by priority (one wave per vehicle of a level, one launch per level; reads the trajectory layout of the file above)
#include "pp_deconflict.hpp"
// ... and tracked movers beside them (one wave per track, per vehicle of a level, per (vehicle, track); the same trajectory layout)
#include "pp_tracks.hpp"
// the pairs that can meet at all: boxes per plan and block of lattice times, then the all-pairs box test (one wave per plan, per row; the same trajectory layout)
#include "pp_pairs.hpp"
// questions to a plan's timetable: look-ups by arc length or by time and the list of its stops (one wave per plan)
#include "pp_timetable.hpp"
// waits at the start or at a timetable's stops that clear conflicts, by priority (one wave per plan lists the places, then one wave per vehicle of a level)
#include "pp_waits.hpp"
// decided waits written into a plan's timetable: t_k += the holds at or before row k, in place (one wave per plan)
#include "pp_retime.hpp"

} // namespace

// who holds finished plans, and the buffer groups and the one launch route of the services that work on them
#include "pp_held_plans.hpp"

// ---------------------------------------------------------------------------
struct pp_planner {
	pp_map* map = nullptr;
	pp_hybrid_params params {};
	int maxBatch = 0, maxNodes = 0;
	SearchArgs args {};
	pph::NonHoloDesc nh {};
	std::vector<double> deltas;
	// device
	// (pph::Dev / pph::Event own what they hold and release it with the planner; the kernels get raw pointers)
	pph::Dev<double> table;
	bool tableReady = false;
	pph::Dev<float> costFields;
	pph::DeviceMem wfWorkspace;
	int64_t wfBytesPerSlot = 0;
	int wfSlots = 0;
	pph::Dev<int32_t> wfError;
	pph::Dev<int> tilesCtl;               // control words of the tile form of the wavefront (pp_wavefront_tiles.hip; zero at allocation, set back by its kernels)
	pph::Dev<int32_t> tilesFallback;      // [maxBatch] goals it hands to the ordered kernel
	pph::Dev<Node> nodes;
	pph::Dev<HeapEntry> heaps;
	pph::Dev<uint32_t> keymaps;
	pph::Dev<uint32_t> expanded;
	pph::Dev<RsLogEntry> rsLogs;
	pph::Dev<DevResult> results;
	pph::Dev<unsigned long long> prof;    // diagnostic phase cycles, [maxBatch][PH_COUNT]
	bool profile = false;
	pph::Dev<unsigned long long> mtStates; // [searchRows][312] mt19937_64 engine state per row (rows kernel)
	int* nextQuery = nullptr;               // not owned: wfError + 2, {query counter of the persistent rows kernel, set-aside count}
	pph::Dev<SuspendRec> suspended;         // [listCap] queries set aside by the rows kernel
	pph::Dev<int32_t> order;                // [maxBatch] query indices, probable longest first (rows kernel)
	pph::Dev<float> orderKeys;              // [maxBatch] field value at each query's start pose (the sort key)
	pph::Dev<HeapEntry> bands;              // [slots][kBands * kBandCap] f-bands of the open list
	pph::Dev<uint8_t> bandMeta;             // [slots][kBands] slot fill counts of set-aside queries
	double bandInvW = 64.0;                 // bands are 1 / bandInvW wide in total cost
	int searchWaves = 0;                    // resident waves of k_hybrid_search_rows on this device
	int searchRows = 0;                     // rows (= search buffer slots) this planner runs with
	bool rowsKernel = false;                // four-queries-per-wave kernel (throughput) vs one query per wave (latency)
	pph::Dev<GuardRec> guardLog;            // [maxBatch][kGuardLogCap] lattice-line children (one-query-per-wave planners only)
	pph::Dev<int> guardCount;               // [maxBatch]
	pph::Dev<PathRec> paths;                // [maxBatch][maxPath] solution paths, goal first
	int maxPath = 0;
	pph::Dev<double> dStarts, dGoals;
	pph::Dev<uint64_t> dSeeds;
	pph::Event e0, e1, e2;
	hipEvent_t startAfter = nullptr; // not owned: another planner's e1; one-shot, the next batch waits for it (pp_planner_start_after_fields_of)
	float wavefrontMs = 0, searchMs = 0;
	int lastBatch = 0;
	pp_pipeline* owner = nullptr; // not owned: the pipeline this planner is the buffer set of (set with pipelineOwned)
	pp_footprint* footprint = nullptr; // pp_planner_set_footprint (a reference is held): the search asks the footprint, not the point validator
	pph::ClearanceViews clearance; // pp_planner_set_heuristic_clearance / pp_pipeline_set_heuristic_clearance: the occupancy the field launches read (radius 0: the map's own)
	bool pipelineOwned = false; // the buffer set of a pp_pipeline (pp_pipeline_planner()): its rows and field slots belong to the pipeline's kernels
	std::vector<DevResult> hostResults;
	// the services over the plans of the last batch (pp_held_plans.hpp): buffers for maxBatch plans, allocated at a service's first call and indexed by query
	PostGroup post;
	HeldBuffers<NoPlanArg, pp_revalidate_result> reval;
	HeldBuffers<StampArg, pp_stamp_result> stamp;
	HeldBuffers<LocateArg, pp_locate_result> locate;
	SpeedGroup speed;
	ConflictGroup conflict;
	DelayGroup delay;
	TrackGroup track;
	PairGroup pair;
	TimetableGroup timetable;
	RetimeGroup retime;
	WaitGroup wait;
};

namespace {

using pph::set_error;

// Scratch the planner's kernels need per lane (largest private segment among them; tests/test_kernel_resources.py keeps
// the figure honest against the built code object) and the number of hardware queues whose first dispatch may still have to
// allocate it after this planner took its memory (GPU_MAX_HW_QUEUES; reserved for a process that gives the runtime up to 16).
constexpr size_t kMaxPrivateBytes = 1024;
constexpr size_t kReserveQueues = 16;

// One launch function per search kernel: every launch site -- batch, continuation, pipeline, warm-up -- goes through these, so a
// kernel argument is added in one place.  A warm-up is nQueries = 0 on a grid of one: the kernels leave before they dereference
// anything, which is what lets warm_up_kernels run them while the planner's buffers are still null.
struct Queries { // device arrays
	int n;
	const double *starts, *goals;
	const uint64_t* seeds;
};

/// k_hybrid_search<kProfile> on `grid` waves; resume: the continuation of the queries the rows kernel set aside (their records, the
/// count behind the rows' query counter, the rows' engine states) instead of a batch of its own
template <bool kProfile>
hipError_t launch_search(pp_planner* p, hipStream_t s, int grid, const Queries& q, bool resume = false)
{
	hipLaunchKernelGGL(k_hybrid_search<kProfile>, dim3(grid), dim3(64), 0, s, p->args, q.n, q.starts, q.goals, q.seeds, p->costFields.get(), p->nodes.get(), p->heaps.get(),
		p->keymaps.get(), p->expanded.get(), p->rsLogs.get(), p->paths.get(), p->results.get(), p->prof.get(), resume ? p->suspended.get() : nullptr,
		resume ? p->nextQuery + 1 : nullptr, resume ? p->mtStates.get() : nullptr, p->bands.get(), p->bandInvW, p->bandMeta.get());
	return hipGetLastError();
}

hipError_t launch_search_footprint(pp_planner* p, hipStream_t s, int grid, const Footprint& foot, const Queries& q)
{
	hipLaunchKernelGGL(k_hybrid_search_footprint, dim3(grid), dim3(64), 0, s, p->args, foot, q.n, q.starts, q.goals, q.seeds, p->costFields.get(), p->nodes.get(), p->heaps.get(),
		p->keymaps.get(), p->expanded.get(), p->rsLogs.get(), p->paths.get(), p->results.get(), p->bands.get(), p->bandInvW, p->bandMeta.get());
	return hipGetLastError();
}

/// k_hybrid_search_rows<kPiped> on args.rowsWaves waves (at least one workgroup).  Batch form: q.n queries handed out through the planner's
/// counters, in `order` if given, set aside after args.suspendAfter expansions; pipeline form: the rows take field slots through `pipe`.
template <bool kPiped>
hipError_t launch_search_rows(pp_planner* p, hipStream_t s, const SearchArgs& args, const Queries& q, const int32_t* order, const PipeView& pipe)
{
	constexpr int kWg = kPiped ? 1 : PP_ROWS_WAVES_PER_WG; // waves per workgroup (see k_hybrid_search_rows)
	const int waves = args.rowsWaves > 0 ? args.rowsWaves : 1;
	int* const ctl = kPiped ? nullptr : p->nextQuery; // {query counter, set-aside count}, spare slots handed out at wfError + 7; null in a warm-up
	hipLaunchKernelGGL(k_hybrid_search_rows<kPiped>, dim3((waves + kWg - 1) / kWg), dim3(64 * kWg), 0, s, args, q.n, q.starts, q.goals, q.seeds, p->costFields.get(), p->nodes.get(),
		p->heaps.get(), p->keymaps.get(), p->expanded.get(), p->rsLogs.get(), p->paths.get(), p->mtStates.get(), p->results.get(), ctl, kPiped ? nullptr : p->suspended.get(), order,
		args.suspendAfter, ctl ? ctl + 1 : nullptr, ctl ? ctl + 5 : nullptr, p->bands.get(), p->bandInvW, p->bandMeta.get(), pipe);
	return hipGetLastError();
}

/// k_hybrid_search_rows_footprint<true>: the pipeline form of the rows kernel with a vehicle footprint (pp_pipeline_set_footprint).  The same
/// grid and arguments as launch_search_rows<true>, plus the footprint by value.
hipError_t launch_search_rows_footprint(pp_planner* p, hipStream_t s, const SearchArgs& args, const Footprint& foot, const Queries& q, const PipeView& pipe)
{
	const int waves = args.rowsWaves > 0 ? args.rowsWaves : 1;
	hipLaunchKernelGGL(k_hybrid_search_rows_footprint<true>, dim3(waves), dim3(64), 0, s, args, foot, q.n, q.starts, q.goals, q.seeds, p->costFields.get(), p->nodes.get(),
		p->heaps.get(), p->keymaps.get(), p->expanded.get(), p->rsLogs.get(), p->paths.get(), p->mtStates.get(), p->results.get(), (int*)nullptr, (SuspendRec*)nullptr,
		(const int32_t*)nullptr, args.suspendAfter, (int*)nullptr, (int*)nullptr, p->bands.get(), p->bandInvW, p->bandMeta.get(), pipe);
	return hipGetLastError();
}

/// k_stamp_tickets over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_stamp(hipStream_t s, const SearchArgs& args, const Footprint& foot, const pp_stamp_params* params, int count, const int32_t* slotsDev, const StampArg* argsDev,
	pp_planner* p, int32_t* occ, pp_stamp_result* outDev)
{
	hipLaunchKernelGGL(k_stamp_tickets, dim3(count > 0 ? count : 1), dim3(kStampLanes), stamp_lds_bytes(args.maxPath), s, args, foot, params ? params->spacing : 1.0,
		params ? params->margin : 0.0f, count, slotsDev, argsDev, p->paths.get(), p->rsLogs.get(), p->results.get(), occ, outDev);
	return hipGetLastError();
}

/// k_locate_tickets over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_locate(hipStream_t s, const SearchArgs& args, const pp_locate_params* params, int count, const int32_t* slotsDev, const LocateArg* argsDev, pp_planner* p,
	pp_locate_result* outDev)
{
	hipLaunchKernelGGL(k_locate_tickets, dim3(count > 0 ? count : 1), dim3(kLocateLanes), locate_lds_bytes(args.maxPath), s, args, params ? params->spacing : 1.0,
		params ? params->heading_weight : 0.0, count, slotsDev, argsDev, p->paths.get(), p->rsLogs.get(), p->results.get(), outDev);
	return hipGetLastError();
}

/// k_speed_profile_tickets over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_speed_profile(hipStream_t s, const SearchArgs& args, const Footprint& foot, const pp_speed_profile_params* params, int maxSamples, int count,
	const int32_t* slotsDev, const SpeedArg* argsDev, pp_planner* p, double* rowsDev, pp_speed_profile_result* outDev)
{
	ppv::Limits limits {};
	if (params)
		limits = ppv::Limits { params->v_max_forward, params->v_max_reverse, params->a_acc, params->a_dec, params->a_lat, params->dwell, params->clearance_gain, params->v_floor };
	hipLaunchKernelGGL(k_speed_profile_tickets, dim3(count > 0 ? count : 1), dim3(kSpeedLanes), speed_lds_bytes(args.maxPath), s, args, foot, limits, params ? params->spacing : 1.0,
		maxSamples, count, slotsDev, argsDev, p->paths.get(), p->rsLogs.get(), p->results.get(), rowsDev, outDev);
	return hipGetLastError();
}

/// k_trajectory_tickets over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_trajectory(hipStream_t s, const SearchArgs& args, const ConflictLattice& lattice, bool withHeading, int count, const int32_t* slotsDev,
	const ConflictArg* argsDev, pp_planner* p, const double* rowsDev, double* trajDev, pp_trajectory_result* outDev)
{
	hipLaunchKernelGGL(k_trajectory_tickets, dim3(count > 0 ? count : 1), dim3(kConflictLanes), trajectory_lds_bytes(args.maxPath), s, args, lattice, withHeading ? 1 : 0, count,
		slotsDev, argsDev, p->paths.get(), p->rsLogs.get(), p->results.get(), rowsDev, trajDev, outDev);
	return hipGetLastError();
}

/// k_conflict_pairs over `count` pairs of `plans` trajectories (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_conflict_pairs(hipStream_t s, const Footprint& discs, const ConflictLattice& lattice, int plans, long long count, const int32_t* pairsDev,
	const double* trajDev, const pp_trajectory_result* plansDev, pp_conflict_result* outDev)
{
	hipLaunchKernelGGL(k_conflict_pairs, dim3((unsigned)(count > 0 ? count : 1)), dim3(kConflictLanes), 0, s, discs, lattice, plans, count, pairsDev, trajDev, plansDev, outDev);
	return hipGetLastError();
}

/// k_delay_level over the `count` vehicles `membersDev` of one level (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_delay_level(hipStream_t s, const Footprint& discs, const ConflictLattice& lattice, int maxDelay, int plans, int count, const int32_t* membersDev,
	const int32_t* offsetsDev, const int32_t* partnersDev, const ConflictArg* argsDev, const double* trajDev, const pp_trajectory_result* plansDev, int32_t* delaysDev,
	pp_delay_result* outDev)
{
	hipLaunchKernelGGL(k_delay_level, dim3((unsigned)(count > 0 ? count : 1)), dim3(kDelayLanes), 0, s, discs, lattice, maxDelay, plans, count, membersDev, offsetsDev, partnersDev,
		argsDev, trajDev, plansDev, delaysDev, outDev);
	return hipGetLastError();
}

/// k_track_samples over the tracks of `view`
hipError_t launch_track_samples(hipStream_t s, const ConflictLattice& lattice, const TrackView& view)
{
	hipLaunchKernelGGL(k_track_samples, dim3((unsigned)(view.M > 0 ? view.M : 1)), dim3(kTrackLanes), 0, s, lattice, view);
	return hipGetLastError();
}

/// k_delay_level_tracks over the `count` vehicles `membersDev` of one level: launch_delay_level's arguments, and the tracks' samples and radii
hipError_t launch_delay_level_tracks(hipStream_t s, const Footprint& discs, const ConflictLattice& lattice, int maxDelay, int plans, int count, const int32_t* membersDev,
	const int32_t* offsetsDev, const int32_t* partnersDev, const ConflictArg* argsDev, const double* trajDev, const pp_trajectory_result* plansDev, const TrackView& view,
	int32_t* delaysDev, pp_delay_result* outDev)
{
	hipLaunchKernelGGL(k_delay_level_tracks, dim3((unsigned)(count > 0 ? count : 1)), dim3(kDelayLanes), 0, s, discs, lattice, maxDelay, plans, count, membersDev, offsetsDev,
		partnersDev, argsDev, trajDev, plansDev, view.M, (const double*)view.samples, view.radii, delaysDev, outDev);
	return hipGetLastError();
}

/// k_track_pairs over every (vehicle, track) of `plans` vehicles and the tracks of `view`, behind the last level
hipError_t launch_track_pairs(hipStream_t s, const Footprint& discs, const ConflictLattice& lattice, int maxDelay, int plans, const double* trajDev,
	const pp_delay_result* decidedDev, const TrackView& view, pp_track_result* outDev)
{
	hipLaunchKernelGGL(k_track_pairs, dim3((unsigned)((size_t)plans * (size_t)view.M)), dim3(kTrackLanes), 0, s, discs, lattice, maxDelay, plans, view.M, trajDev, decidedDev,
		(const double*)view.samples, view.radii, outDev);
	return hipGetLastError();
}

/// k_plan_boxes over the plans of `view`: the extended trajectory trajDev of T + D columns per plan, B lattice times per box
hipError_t launch_plan_boxes(hipStream_t s, int T, int maxDelay, int timesPerBox, const BoxView& view, const double* trajDev, int32_t* boxedDev)
{
	hipLaunchKernelGGL(k_plan_boxes, dim3((unsigned)view.n), dim3(kPairLanes), 0, s, T, maxDelay, timesPerBox, view, trajDev, boxedDev);
	return hipGetLastError();
}

/// k_box_pairs over the rows of `view`: the count pass (fill == false: countsDev) or the fill pass (offsetsDev from k_pair_offsets; at most maxPairs pairs written)
hipError_t launch_box_pairs(hipStream_t s, bool fill, const BoxView& view, double reach, long long maxPairs, const long long* offsetsDev, long long* countsDev, int32_t* pairsDev,
	int32_t* firstBoxDev)
{
	if (fill)
		hipLaunchKernelGGL(k_box_pairs<true>, dim3((unsigned)view.n), dim3(kPairLanes), 0, s, view, reach, maxPairs, offsetsDev, countsDev, pairsDev, firstBoxDev);
	else
		hipLaunchKernelGGL(k_box_pairs<false>, dim3((unsigned)view.n), dim3(kPairLanes), 0, s, view, reach, maxPairs, offsetsDev, countsDev, pairsDev, firstBoxDev);
	return hipGetLastError();
}

/// k_pair_offsets between the two: one workgroup
hipError_t launch_pair_offsets(hipStream_t s, int plans, const long long* countsDev, const int32_t* boxedDev, long long* offsetsDev)
{
	hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(kPairLanes), 0, s, plans, countsDev, boxedDev, offsetsDev);
	return hipGetLastError();
}

/// k_timetable_tickets over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_timetable(hipStream_t s, const SearchArgs& args, const TimetableCall& call, int count, const int32_t* slotsDev, const ConflictArg* argsDev, pp_planner* p,
	const double* rowsDev, const double* valuesDev, pp_timetable_stop* stopsDev, pp_timetable_result* lookupsDev, pp_timetable_plan* outDev)
{
	hipLaunchKernelGGL(k_timetable_tickets, dim3(count > 0 ? count : 1), dim3(kTimetableLanes), trajectory_lds_bytes(args.maxPath), s, args, call, count, slotsDev, argsDev,
		p->paths.get(), p->rsLogs.get(), p->results.get(), rowsDev, valuesDev, stopsDev, lookupsDev, outDev);
	return hipGetLastError();
}

/// k_retime_tickets over `count` >= 1 plans whose longest hold list has `most` entries (the kernel has no private segment: no warm-up dispatch)
hipError_t launch_retime(hipStream_t s, const RetimeCall& call, int count, int most, const ConflictArg* argsDev, const int32_t* offsetsDev, const pp_hold* holdsDev,
	double* rowsDev, pp_retime_result* outDev)
{
	hipLaunchKernelGGL(k_retime_tickets, dim3(count), dim3(kRetimeLanes), retime_lds_bytes(most), s, call, count, argsDev, offsetsDev, holdsDev, rowsDev, outDev);
	return hipGetLastError();
}

/// k_wait_places over `count` plans of buffer set p (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_wait_places(hipStream_t s, const SearchArgs& args, const ConflictLattice& lattice, const WaitCall& call, int count, const int32_t* slotsDev,
	const ConflictArg* argsDev, pp_planner* p, const double* rowsDev, const pp_wait_fixed* fixedDev, pp_wait_place* placesDev, int32_t* countsDev)
{
	if (fixedDev)
		hipLaunchKernelGGL(k_wait_places<true>, dim3(count > 0 ? count : 1), dim3(kWaitLanes), trajectory_lds_bytes(args.maxPath), s, args, lattice, call, count, slotsDev, argsDev,
			p->paths.get(), p->rsLogs.get(), p->results.get(), rowsDev, fixedDev, placesDev, countsDev);
	else
		hipLaunchKernelGGL(k_wait_places<false>, dim3(count > 0 ? count : 1), dim3(kWaitLanes), trajectory_lds_bytes(args.maxPath), s, args, lattice, call, count, slotsDev, argsDev,
			p->paths.get(), p->rsLogs.get(), p->results.get(), rowsDev, fixedDev, placesDev, countsDev);
	return hipGetLastError();
}

/// k_wait_level over the `count` vehicles `membersDev` of one level (count = 0 on a grid of one: the warm-up, which dereferences nothing)
hipError_t launch_wait_level(hipStream_t s, const Footprint& discs, const ConflictLattice& lattice, const WaitCall& call, int plans, int count, const int32_t* membersDev,
	const int32_t* offsetsDev, const int32_t* partnersDev, const ConflictArg* argsDev, const double* trajDev, const pp_trajectory_result* plansDev, const pp_wait_fixed* fixedDev,
	const uint8_t* noStartDev, const pp_wait_place* placesDev, const int32_t* countsDev, WaitState* statesDev, pp_wait_result* outDev)
{
	if (discs.anyOffset)
		hipLaunchKernelGGL(k_wait_level<true>, dim3((unsigned)(count > 0 ? count : 1)), dim3(kWaitLanes), 0, s, discs, lattice, call, plans, count, membersDev, offsetsDev, partnersDev,
			argsDev, trajDev, plansDev, fixedDev, noStartDev, placesDev, countsDev, statesDev, outDev);
	else
		hipLaunchKernelGGL(k_wait_level<false>, dim3((unsigned)(count > 0 ? count : 1)), dim3(kWaitLanes), 0, s, discs, lattice, call, plans, count, membersDev, offsetsDev, partnersDev,
			argsDev, trajDev, plansDev, fixedDev, noStartDev, placesDev, countsDev, statesDev, outDev);
	return hipGetLastError();
}

/// An empty dispatch of each kernel that works on held plans (post-processing in the holder's form), on stream s, which is drained behind each: the queue
/// allocates their scratch here, where a failure is an error code (see warm_up_kernels).  *service names the service whose kernel failed.
hipError_t warm_up_held_kernels(pp_planner* p, hipStream_t s, bool byTicket, const char** service)
{
	hipError_t e = hipSuccess;
	auto ok = [&](const char* name, hipError_t launched) {
		*service = name;
		e = launched != hipSuccess ? launched : hipStreamSynchronize(s);
		return e == hipSuccess;
	};
	if (byTicket)
		hipLaunchKernelGGL(k_postprocess_tickets, dim3(1), dim3(kPostThreads), 64, s, p->args, PostParams {}, Footprint {}, 0, (const int32_t*)nullptr, (const PathRec*)nullptr,
			(const RsLogEntry*)nullptr, (const DevResult*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, PostBuffers {});
	else
		hipLaunchKernelGGL(k_postprocess, dim3(1), dim3(kPostThreads), 64, s, p->args, PostParams {}, 0, (const PathRec*)nullptr, (const RsLogEntry*)nullptr, (const DevResult*)nullptr,
			(const uint32_t*)nullptr, (const uint32_t*)nullptr, PostBuffers {});
	if (!ok("post-processing", hipGetLastError()))
		return e;
	hipLaunchKernelGGL(k_revalidate_tickets, dim3(1), dim3(64), 0, s, p->args, Footprint {}, 0, (const int32_t*)nullptr, (const PathRec*)nullptr, (const RsLogEntry*)nullptr,
		(const DevResult*)nullptr, (pp_revalidate_result*)nullptr);
	if (ok("re-validation", hipGetLastError()) && ok("stamp", launch_stamp(s, p->args, Footprint {}, nullptr, 0, nullptr, nullptr, p, nullptr, nullptr)))
		if (ok("locate", launch_locate(s, p->args, nullptr, 0, nullptr, nullptr, p, nullptr)))
			if (ok("speed profile", launch_speed_profile(s, p->args, Footprint {}, nullptr, 1, 0, nullptr, nullptr, p, nullptr, nullptr)))
				if (ok("conflict trajectories", launch_trajectory(s, p->args, ConflictLattice {}, false, 0, nullptr, nullptr, p, nullptr, nullptr, nullptr)))
					(void)ok("conflict pairs", launch_conflict_pairs(s, Footprint {}, ConflictLattice {}, 0, 0, nullptr, nullptr, nullptr, nullptr));
	if (e == hipSuccess)
		(void)ok("delay levels", launch_delay_level(s, Footprint {}, ConflictLattice {}, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
	if (e == hipSuccess)
		(void)ok("timetable", launch_timetable(s, p->args, TimetableCall {}, 0, nullptr, nullptr, p, nullptr, nullptr, nullptr, nullptr, nullptr));
	// (both forms of k_wait_places have a private segment; the second one's `fixed` is any address that is not null: an empty dispatch dereferences nothing)
	if (e == hipSuccess && ok("wait places", launch_wait_places(s, p->args, ConflictLattice {}, WaitCall {}, 0, nullptr, nullptr, p, nullptr, nullptr, nullptr, nullptr)) &&
		ok("wait places", launch_wait_places(s, p->args, ConflictLattice {}, WaitCall {}, 0, nullptr, nullptr, p, nullptr, (const pp_wait_fixed*)p->results.get(), nullptr, nullptr)))
		(void)ok("wait levels", launch_wait_level(s, Footprint {}, ConflictLattice {}, WaitCall {}, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
			nullptr, nullptr, nullptr, nullptr));
	return e;
}

/// Empty dispatches of the kernels a batch launches, on the planner's stream, then a synchronisation: the queue
/// allocates their scratch here, where a failure is an error code, not at the first batch, where it is an abort.
int warm_up_kernels(pp_planner* p, pp_map* map)
{
	hipStream_t s = map->ctx->stream;
	pph::Dev<int32_t> ctl;
	PP_HIP_TRY(ctl.alloc(64));
	hipError_t e = hipMemsetAsync(ctl, 0, 64, s);
	if (e == hipSuccess)
		e = pph::warm_up_wavefront(s, map->view(), ctl);
	if (e == hipSuccess && map->occBits && pph::wavefront_tiles_supported(map->desc.rows, map->desc.cols))
		e = pph::warm_up_wavefront_tiles(s, map->view(), (int*)ctl.get() + 8);
	const Queries noQueries {};
	if (e == hipSuccess) {
		SearchArgs none = p->args;
		none.rowsWaves = 0; // every wave of the rows kernel leaves at once
		none.listCap = 0;
		e = launch_search_rows<false>(p, s, none, noQueries, nullptr, PipeView {});
	}
	if (e == hipSuccess)
		e = launch_search<false>(p, s, 1, noQueries);
	const char* service = nullptr;
	if (e == hipSuccess)
		e = warm_up_held_kernels(p, s, false, &service);
	if (e == hipSuccess)
		e = hipStreamSynchronize(s);
	if (e != hipSuccess)
		return pph::hip_fail(e, "planner kernel warm-up (scratch allocation)");
	return PP_OK;
}

/// The primitive table of the search kernels from the steering-angle list (StatePropagator::m_deltas): children in list order,
/// forward then backward each (hybrid_a_star.cpp:65-77); curvature per primitive with the host's libm
int primitives_from_deltas(pp_planner* p)
{
	const int P = 2 * (int)p->deltas.size();
	if (P < 2 || P > pph::kMaxPrimitives) {
		set_error("between 1 and " + std::to_string(pph::kMaxPrimitives / 2) + " steering angles (two motion primitives each)");
		return PP_ERR_INVALID;
	}
	const double wheelbase = p->params.wheelbase, rearToCenter = 0.0;
	pph::PrimTable& T = p->args.prims;
	T.n = P;
	for (size_t d = 0; d < p->deltas.size(); d++) {
		// ConstantSteer, kinematic_bicycle_model.cpp:13-17 with rearToCenter = 0
		const double tanSteering = std::tan(p->deltas[d]);
		const double beta = std::atan(rearToCenter * tanSteering / wheelbase);
		const double cosBeta = std::cos(beta);
		const double DthetaDdist = cosBeta * tanSteering / wheelbase;
		T.kappa[2 * d] = DthetaDdist;
		T.invKappa[2 * d] = T.invKappa[2 * d + 1] = DthetaDdist != 0.0 ? 1 / DthetaDdist : 0.0;
		T.backward[2 * d] = 0;
		T.kappa[2 * d + 1] = DthetaDdist;
		T.backward[2 * d + 1] = 1;
	}
	return PP_OK;
}

/// the map a plan is re-validated against (pp_planner_revalidate, pp_pipeline_revalidate): of the owner's context, with a distance grid
int revalidate_check_target(const pp_map* own, const pp_map* target)
{
	if (target->ctx != own->ctx) {
		set_error("the target map belongs to another context than the planner's map");
		return PP_ERR_INVALID;
	}
	if (!target->dist) {
		set_error("the target map has no distance grid: pp_map_upload_dist2, pp_map_upload_distance or pp_map_update_gvd first");
		return PP_ERR_INVALID;
	}
	return PP_OK;
}

/// The arguments of a stamp that do not depend on who holds the plans (pp_planner_stamp, pp_pipeline_stamp): the target's context, the
/// parameters, and the per-plan values and windows, which go into `plans` (h.name(i) names plan i in a refusal)
int stamp_check(const HeldPlans& h, const pp_map* target, const int32_t* values, const double* from_length, const double* to_length, const pp_stamp_params* params,
	std::vector<StampArg>& plans)
{
	const pp_map* const own = h.pl->map;
	const int n = h.n;
	if (target->ctx != own->ctx) {
		set_error("the target map belongs to another context than the planner's map");
		return PP_ERR_INVALID;
	}
	if (!params) {
		set_error("invalid arguments (null params: a pp_stamp_params with spacing > 0 is needed)");
		return PP_ERR_INVALID;
	}
	if (!std::isfinite(params->spacing) || !(params->spacing > 0.0)) {
		set_error("invalid arguments (the stamp's spacing is finite and > 0 metres)");
		return PP_ERR_INVALID;
	}
	if (!std::isfinite(params->margin) || params->margin < 0.0f) {
		set_error("invalid arguments (the stamp's margin is finite and >= 0 metres)");
		return PP_ERR_INVALID;
	}
	plans.resize((size_t)n);
	for (int i = 0; i < n; i++) {
		StampArg& a = plans[(size_t)i];
		a.from = from_length ? from_length[i] : -HUGE_VAL;
		a.to = to_length ? to_length[i] : HUGE_VAL;
		a.value = values ? values[i] : 0;
		a.pad = 0;
		if (a.value < 0) {
			set_error(h.name(i) + " has the negative value " + std::to_string(a.value) + ": a stamp writes occupancy ids >= 0 (-1 is a free cell)");
			return PP_ERR_INVALID;
		}
		if (a.from != a.from || a.to != a.to) {
			set_error(h.name(i) + " has a NaN in its window");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// the discs a stamp uses: the holder's footprint, or the point validator seen as one -- the disc (0, 0, minSafeRadius) of the holder's OWN map
Footprint stamp_discs(const pp_footprint* fp, const pp_map* own)
{
	if (fp)
		return fp->fp;
	Footprint f {};
	f.n = 1;
	f.r[0] = own->minSafeRadius;
	return f;
}

/// a target without an int32 occupancy grid gets one, all -1 (as pp_map_set_cells does), complete before the call's stream goes on
int stamp_prepare_target(pp_map* map)
{
	if (map->occ32)
		return PP_OK;
	const size_t n = map->cells();
	PP_HIP_TRY(map->occ32.ensure(n * 4));
	PP_HIP_TRY(hipMemsetAsync(map->occ32, 0xFF, n * 4, map->ctx->stream));
	PP_HIP_TRY(hipStreamSynchronize(map->ctx->stream));
	return PP_OK;
}

/// What every occupancy writer does afterwards, behind a stamp that is complete: the views (occVersion goes up; clearance views and bit rows follow as
/// they do today), and the edit journal, which does not know the cells written -- the next reference-order update re-seeds from the device grid
int stamp_finish_target(pp_map* map)
{
	map->journal.clear();
	map->journal.shrink_to_fit();
	map->journalLost = true;
	if (int rc = pph::refresh_occupancy_views(map, map->ctx->stream))
		return rc;
	PP_HIP_TRY(hipStreamSynchronize(map->ctx->stream));
	return PP_OK;
}

/// The arguments of a locate call that do not depend on who holds the plans (pp_planner_locate, pp_pipeline_locate): the parameters, the
/// vehicle poses and the windows, which go into `plans` (h.name(i) names plan i in a refusal)
int locate_check(const HeldPlans& h, const double* poses, const double* from_length, const double* to_length, const pp_locate_params* params, std::vector<LocateArg>& plans)
{
	const int n = h.n;
	if (n > 0 && !params) {
		set_error("invalid arguments (null params: a pp_locate_params with spacing > 0 is needed)");
		return PP_ERR_INVALID;
	}
	if (params && (!std::isfinite(params->spacing) || !(params->spacing > 0.0))) {
		set_error("invalid arguments (the locate call's spacing is finite and > 0 metres)");
		return PP_ERR_INVALID;
	}
	if (params && (!std::isfinite(params->heading_weight) || !(params->heading_weight >= 0.0))) {
		set_error("invalid arguments (the locate call's heading_weight is finite and >= 0 metres per radian)");
		return PP_ERR_INVALID;
	}
	if (n > 0 && !poses) {
		set_error("invalid arguments (null poses_host: one vehicle pose (x, y, theta) per plan is needed)");
		return PP_ERR_INVALID;
	}
	plans.resize((size_t)n);
	for (int i = 0; i < n; i++) {
		LocateArg& a = plans[(size_t)i];
		for (int k = 0; k < 3; k++)
			a.pose[k] = poses[(size_t)i * 3 + k];
		a.from = from_length ? from_length[i] : -HUGE_VAL;
		a.to = to_length ? to_length[i] : HUGE_VAL;
		if (!std::isfinite(a.pose[0]) || !std::isfinite(a.pose[1]) || !std::isfinite(a.pose[2])) {
			set_error(h.name(i) + " has a vehicle pose that is not finite");
			return PP_ERR_INVALID;
		}
		if (a.from != a.from || a.to != a.to) {
			set_error(h.name(i) + " has a NaN in its window");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// The arguments of a speed-profile call that do not depend on who holds the plans (pp_planner_speed_profile, pp_pipeline_speed_profile): the target's
/// context and -- with a clearance term -- its distance grid, the parameters, the sample limit, and the per-plan windows and end speeds, which go into
/// `plans` (h.name(i) names plan i in a refusal)
int speed_check(const HeldPlans& h, const pp_map* target, const double* from_length, const double* to_length, const double* v_start, const double* v_end,
	const pp_speed_profile_params* params, int max_samples, std::vector<SpeedArg>& plans)
{
	const int n = h.n;
	if (target->ctx != h.pl->map->ctx) {
		set_error("the target map belongs to another context than the planner's map");
		return PP_ERR_INVALID;
	}
	if (n > 0 && !params) {
		set_error("invalid arguments (null params: a pp_speed_profile_params is needed)");
		return PP_ERR_INVALID;
	}
	if (params) {
		const std::pair<const char*, double> positive[] = { { "spacing", params->spacing }, { "v_max_forward", params->v_max_forward }, { "v_max_reverse", params->v_max_reverse },
			{ "a_acc", params->a_acc }, { "a_dec", params->a_dec }, { "a_lat", params->a_lat } };
		for (const auto& [name, value] : positive)
			if (!std::isfinite(value) || !(value > 0.0)) {
				set_error(std::string("invalid arguments (the speed profile's ") + name + " is finite and > 0)");
				return PP_ERR_INVALID;
			}
		const std::pair<const char*, double> nonNegative[] = { { "dwell", params->dwell }, { "clearance_gain", params->clearance_gain }, { "v_floor", params->v_floor } };
		for (const auto& [name, value] : nonNegative)
			if (!std::isfinite(value) || !(value >= 0.0)) {
				set_error(std::string("invalid arguments (the speed profile's ") + name + " is finite and >= 0)");
				return PP_ERR_INVALID;
			}
		if (params->clearance_gain > 0.0 && !target->dist) {
			set_error("the target map has no distance grid, which a clearance_gain > 0 reads: pp_map_upload_dist2, pp_map_upload_distance or pp_map_update_gvd first");
			return PP_ERR_INVALID;
		}
	}
	if (max_samples < 1) {
		set_error("invalid arguments (max_samples >= 1, got " + std::to_string(max_samples) + ")");
		return PP_ERR_INVALID;
	}
	plans.resize((size_t)n);
	for (int i = 0; i < n; i++) {
		SpeedArg& a = plans[(size_t)i];
		a.from = from_length ? from_length[i] : -HUGE_VAL;
		a.to = to_length ? to_length[i] : HUGE_VAL;
		a.vStart = v_start ? v_start[i] : 0.0;
		a.vEnd = v_end ? v_end[i] : 0.0;
		if (a.from != a.from || a.to != a.to) {
			set_error(h.name(i) + " has a NaN in its window");
			return PP_ERR_INVALID;
		}
		if (!std::isfinite(a.vStart) || !(a.vStart >= 0.0) || !std::isfinite(a.vEnd) || !(a.vEnd >= 0.0)) {
			set_error(h.name(i) + " has a v_start or v_end that is not finite and >= 0");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// The arguments of a conflict call that do not depend on who holds the plans (pp_planner_conflicts, pp_pipeline_conflicts): the parameters and the
/// lattice they span, the start times and the pair list (h.name(i) names plan i in a refusal)
int conflict_check(const HeldPlans& h, const double* t_start, int n_pairs, const int32_t* pairs, const pp_conflict_params* params, ConflictLattice& lattice)
{
	const int n = h.n;
	if (n > 0 && !t_start) {
		set_error("invalid arguments (null t_start: one start time per plan is needed)");
		return PP_ERR_INVALID;
	}
	if (n > 0 && !params) {
		set_error("invalid arguments (null params: a pp_conflict_params is needed)");
		return PP_ERR_INVALID;
	}
	lattice = ConflictLattice {};
	if (params) {
		if (!std::isfinite(params->t_from) || !std::isfinite(params->t_to) || !(params->t_from <= params->t_to)) {
			set_error("invalid arguments (the conflict call's t_from and t_to are finite and t_from <= t_to)");
			return PP_ERR_INVALID;
		}
		if (!std::isfinite(params->dt) || !(params->dt > 0.0)) {
			set_error("invalid arguments (the conflict call's dt is finite and > 0 seconds)");
			return PP_ERR_INVALID;
		}
		if (!std::isfinite(params->margin) || !(params->margin >= 0.0)) {
			set_error("invalid arguments (the conflict call's margin is finite and >= 0 metres)");
			return PP_ERR_INVALID;
		}
		const int64_t k0 = ppc::lattice_begin(params->t_from, params->dt), T = ppc::lattice_count(k0, ppc::lattice_end(params->t_to, params->dt));
		if (T < 1 || T > ppc::kMaxTimes) {
			set_error("invalid arguments (the horizon holds " + (T < 1 ? std::string("no") : "more than " + std::to_string(ppc::kMaxTimes)) +
				" lattice times k * dt: 1 <= T <= " + std::to_string(ppc::kMaxTimes) + ")");
			return PP_ERR_INVALID;
		}
		if ((params->hold_before != 0 && params->hold_before != 1) || (params->hold_after != 0 && params->hold_after != 1)) {
			set_error("invalid arguments (the conflict call's hold_before and hold_after are 0 or 1)");
			return PP_ERR_INVALID;
		}
		lattice.k0 = k0;
		lattice.T = (int)T;
		lattice.holdBefore = params->hold_before;
		lattice.holdAfter = params->hold_after;
		lattice.dt = params->dt;
		lattice.margin = params->margin;
	}
	for (int i = 0; i < n; i++)
		if (!std::isfinite(t_start[i])) {
			set_error(h.name(i) + " has a t_start that is not finite");
			return PP_ERR_INVALID;
		}
	if (n_pairs < 0) {
		set_error("invalid arguments (n_pairs >= 0, got " + std::to_string(n_pairs) + ")");
		return PP_ERR_INVALID;
	}
	if (!pairs) {
		const int64_t all = (int64_t)n * (n - 1) / 2;
		if (n_pairs != all) {
			set_error("invalid arguments (null pairs means every pair i < j: n_pairs == n (n - 1) / 2 = " + std::to_string(all) + ", got " + std::to_string(n_pairs) + ")");
			return PP_ERR_INVALID;
		}
		return PP_OK;
	}
	for (int p = 0; p < n_pairs; p++) {
		const int32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
		if (a < 0 || a >= n || b < 0 || b >= n) {
			set_error("pair " + std::to_string(p) + " = (" + std::to_string(a) + ", " + std::to_string(b) + ") has an index outside 0 .. n - 1 = " + std::to_string(n - 1));
			return PP_ERR_INVALID;
		}
		if (a == b) {
			set_error("pair " + std::to_string(p) + " = (" + std::to_string(a) + ", " + std::to_string(b) + ") pairs a plan with itself");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// The arguments of a delay call (pp_planner_deconflict, pp_pipeline_deconflict): the conflict call's, and the largest delay.  `lattice` is the conflict call's,
/// of T columns from k0 on; the extended one is formed where the trajectory is launched.
int delay_check(const HeldPlans& h, const double* t_start, int n_pairs, const int32_t* pairs, const pp_delay_params* params, ConflictLattice& lattice)
{
	if (int rc = conflict_check(h, t_start, n_pairs, pairs, params ? &params->lattice : nullptr, lattice))
		return rc;
	if (!params)
		return PP_OK; // (n == 0)
	if (params->max_delay_steps < 0) {
		set_error("invalid arguments (max_delay_steps >= 0, got " + std::to_string(params->max_delay_steps) + ")");
		return PP_ERR_INVALID;
	}
	if ((int64_t)lattice.T + params->max_delay_steps > ppc::kMaxTimes) {
		set_error("invalid arguments (the extended trajectory holds T + max_delay_steps = " + std::to_string((int64_t)lattice.T + params->max_delay_steps) +
			" lattice times: at most " + std::to_string(ppc::kMaxTimes) + ")");
		return PP_ERR_INVALID;
	}
	if (params->reserved != 0) {
		set_error("invalid arguments (the delay call's reserved field is zero)");
		return PP_ERR_INVALID;
	}
	return PP_OK;
}

/// The arguments of a call with waits at stops (pp_planner_deconflict_waits, pp_pipeline_deconflict_waits): the delay call's, the number of places, and per plan the
/// start-wait flag and the committed wait (either may be NULL)
int wait_check(const HeldPlans& h, const double* t_start, const uint8_t* no_start_wait, const pp_wait_fixed* fixed, int n_pairs, const int32_t* pairs,
	const pp_wait_params* params, ConflictLattice& lattice)
{
	if (int rc = delay_check(h, t_start, n_pairs, pairs, params ? &params->delay : nullptr, lattice))
		return rc;
	if (!params)
		return PP_OK; // (n == 0)
	if (params->max_places < 0 || params->max_places > ppw::kMaxPlaces) {
		set_error("invalid arguments (max_places in 0 .. " + std::to_string(ppw::kMaxPlaces) + ", got " + std::to_string(params->max_places) + ")");
		return PP_ERR_INVALID;
	}
	if (params->reserved != 0) {
		set_error("invalid arguments (the wait call's reserved field is zero)");
		return PP_ERR_INVALID;
	}
	for (int i = 0; i < h.n; i++) {
		if (no_start_wait && no_start_wait[i] > 1) {
			set_error(h.name(i) + " has a no_start_wait flag that is neither 0 nor 1 (" + std::to_string(no_start_wait[i]) + ")");
			return PP_ERR_INVALID;
		}
		if (fixed && fixed[i].row < ppw::kFree) {
			set_error(h.name(i) + " has a fixed row below -2 (" + std::to_string(fixed[i].row) + ")");
			return PP_ERR_INVALID;
		}
		if (fixed && (fixed[i].steps < 0 || fixed[i].steps > params->delay.max_delay_steps)) {
			set_error(h.name(i) + " has fixed steps outside 0 .. max_delay_steps = " + std::to_string(params->delay.max_delay_steps) + " (" + std::to_string(fixed[i].steps) + ")");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// The track set of a delay call over T lattice times (pp_planner_deconflict_tracks, pp_pipeline_deconflict_tracks): ppk::validate's verdict as a refusal
/// that names the first offender.  NULL is no track.
int tracks_check(const pp_track_set* tracks, int64_t T)
{
	if (!tracks)
		return PP_OK;
	const ppk::Verdict v = ppk::validate(tracks->n_tracks, tracks->reserved, tracks->offsets, tracks->waypoints, tracks->radii, T);
	if (v.fault == ppk::kValid)
		return PP_OK;
	const std::string M = std::to_string(tracks->n_tracks), at = std::to_string(v.index), of = " of track " + std::to_string(v.track);
	switch (v.fault) {
	case ppk::kReserved: set_error("invalid arguments (the track set's reserved field is zero)"); break;
	case ppk::kCount: set_error("invalid arguments (0 <= n_tracks <= " + std::to_string(ppk::kMaxTracks) + ", got " + M + ")"); break;
	case ppk::kNullOffsets: set_error("invalid arguments (null offsets with n_tracks = " + M + ")"); break;
	case ppk::kNullWaypoints: set_error("invalid arguments (null waypoints with n_tracks = " + M + ")"); break;
	case ppk::kNullRadii: set_error("invalid arguments (null radii with n_tracks = " + M + ")"); break;
	case ppk::kFirstOffset: set_error("invalid arguments (the track set's offsets[0] is 0, got " + std::to_string(tracks->offsets[0]) + ")"); break;
	case ppk::kOffsetOrder: set_error("track " + at + " owns no waypoint: offsets are strictly increasing, got offsets[" + at + "] = " + std::to_string(tracks->offsets[v.index]) +
			" and offsets[" + std::to_string(v.index + 1) + "] = " + std::to_string(tracks->offsets[v.index + 1])); break;
	case ppk::kWaypointCount: set_error("invalid arguments (the track set holds offsets[n_tracks] = " + std::to_string(tracks->offsets[tracks->n_tracks]) +
			" waypoints: at most " + std::to_string(ppk::kMaxWaypoints) + ")"); break;
	case ppk::kSampleCount: set_error("invalid arguments (n_tracks * T = " + std::to_string((int64_t)tracks->n_tracks * T) + " track samples: at most " +
			std::to_string(ppk::kMaxSamples) + ")"); break;
	case ppk::kWaypointValue: set_error("waypoint " + at + of + " holds a value that is not finite"); break;
	case ppk::kWaypointOrder: set_error("waypoint " + at + of + " has a time that is not above the one before it: times are strictly increasing within a track"); break;
	default: set_error("track " + at + " has a radius that is not finite and >= 0"); break;
	}
	return PP_ERR_INVALID;
}

/// The arguments of a broad-phase call (pp_planner_candidate_pairs, pp_pipeline_candidate_pairs): the delay call's without a pair list, the block length and
/// the caller's rows.  NULL params pass only with n == 0, as in the delay call.
int pair_check(const HeldPlans& h, const double* t_start, const pp_pair_params* params, const int32_t* pairs_host, ConflictLattice& lattice)
{
	const int32_t none[2] = { 0, 0 }; // (an empty list that exists: the call has no pair list of its own to check)
	if (int rc = delay_check(h, t_start, 0, none, params ? &params->delay : nullptr, lattice))
		return rc;
	if (!params)
		return PP_OK; // (n == 0)
	if (params->times_per_box < 1 || params->times_per_box > ppb::kMaxTimesPerBox) {
		set_error("invalid arguments (1 <= times_per_box <= " + std::to_string(ppb::kMaxTimesPerBox) + ", got " + std::to_string(params->times_per_box) + ")");
		return PP_ERR_INVALID;
	}
	if (params->max_pairs < 0) {
		set_error("invalid arguments (max_pairs >= 0, got " + std::to_string(params->max_pairs) + ")");
		return PP_ERR_INVALID;
	}
	if (!pairs_host && params->max_pairs > 0) {
		set_error("invalid arguments (null pairs_host with max_pairs = " + std::to_string(params->max_pairs) + ")");
		return PP_ERR_INVALID;
	}
	const int64_t boxes = (int64_t)h.n * ppb::box_count(lattice.T, params->times_per_box);
	if (boxes > ppb::kMaxBoxes) {
		set_error("invalid arguments (n * NB = " + std::to_string(boxes) + " boxes: at most " + std::to_string(ppb::kMaxBoxes) + ")");
		return PP_ERR_INVALID;
	}
	return PP_OK;
}

/// The arguments of a timetable call (pp_planner_timetable, pp_pipeline_timetable) that do not depend on who holds the plans: the parameters, the count of
/// look-ups and the values (h.name(i) names plan i in a refusal)
int timetable_check(const HeldPlans& h, int n_points, const double* values_host, const pp_timetable_params* params)
{
	if (h.n == 0)
		return PP_OK;
	if (!params) {
		set_error("invalid arguments (null params: a pp_timetable_params is needed)");
		return PP_ERR_INVALID;
	}
	if (params->by != 0 && params->by != 1) {
		set_error("invalid arguments (the timetable call's by is 0, arc lengths, or 1, times: got " + std::to_string(params->by) + ")");
		return PP_ERR_INVALID;
	}
	if (params->max_stops < 0 || params->max_stops > ppm::kMaxStops) {
		set_error("invalid arguments (0 <= max_stops <= " + std::to_string(ppm::kMaxStops) + ", got " + std::to_string(params->max_stops) + ")");
		return PP_ERR_INVALID;
	}
	if (params->reserved[0] != 0 || params->reserved[1] != 0) {
		set_error("invalid arguments (the reserved fields of pp_timetable_params are zero)");
		return PP_ERR_INVALID;
	}
	if (n_points < 0 || (int64_t)h.n * n_points > ppm::kMaxLookups) {
		set_error("invalid arguments (n_points >= 0 and n * n_points <= " + std::to_string(ppm::kMaxLookups) + ", got n_points = " + std::to_string(n_points) + " for " +
			std::to_string(h.n) + " plans)");
		return PP_ERR_INVALID;
	}
	if (n_points > 0 && !values_host) {
		set_error("invalid arguments (null values_host with n * n_points = " + std::to_string((int64_t)h.n * n_points) + " look-ups)");
		return PP_ERR_INVALID;
	}
	for (int i = 0; i < h.n; i++)
		for (int p = 0; p < n_points; p++)
			if (!std::isfinite(values_host[(size_t)i * (size_t)n_points + (size_t)p])) {
				set_error(h.name(i) + " has a value that is not finite (look-up " + std::to_string(p) + ")");
				return PP_ERR_INVALID;
			}
	return PP_OK;
}

/// ... and what the holder remembers of its last speed-profile call for the plans of h: their rows, into `plans`, and the call's stride and limits, into `lattice`
int conflict_profiles(const HeldPlans& h, const SpeedGroup& g, const double* t_start, ConflictLattice& lattice, std::vector<ConflictArg>& plans)
{
	plans.resize((size_t)h.n);
	for (int i = 0; i < h.n; i++) {
		const auto it = g.profileOf.find(h.byTicket ? h.tickets[i] : (uint64_t)i);
		if (it == g.profileOf.end()) {
			set_error(h.name(i) + " has no speed profile: run speed_profile first (it was not in the holder's last speed-profile call, or has been released since)");
			return PP_ERR_INVALID;
		}
		const SpeedGroup::Profile& f = it->second;
		const bool profiled = f.status == 0 && f.nSamples >= 1;
		plans[(size_t)i] = ConflictArg { t_start[i], profiled ? f.row : 0, profiled ? f.nSamples : 0 };
	}
	lattice.maxSamples = g.maxSamples;
	lattice.aAcc = g.aAcc;
	lattice.aDec = g.aDec;
	return PP_OK;
}

/// ... the same for a timetable call, which has no start times: the rows into `plans`, the call into `call`
int timetable_profiles(const HeldPlans& h, const SpeedGroup& g, int n_points, const pp_timetable_params* params, std::vector<ConflictArg>& plans, TimetableCall& call)
{
	call = TimetableCall {};
	if (h.n == 0)
		return PP_OK;
	const std::vector<double> noStart((size_t)h.n, 0.0);
	ConflictLattice lattice {};
	if (int rc = conflict_profiles(h, g, noStart.data(), lattice, plans))
		return rc;
	call = TimetableCall { params->by, params->max_stops, n_points, lattice.maxSamples, lattice.aAcc, lattice.aDec };
	return PP_OK;
}

/// The hold list of a retime call (pp_planner_retime, pp_pipeline_retime) as far as it does not depend on the profiles: the count, the pointer, every
/// plan index, seconds and row >= 1, the order and the holds per plan (h.name(i) names plan i in a refusal)
int retime_check(const HeldPlans& h, int n_holds, const pp_hold* holds)
{
	if (h.n == 0)
		return PP_OK;
	if (n_holds < 0) {
		set_error("invalid arguments (n_holds >= 0, got " + std::to_string(n_holds) + ")");
		return PP_ERR_INVALID;
	}
	if (n_holds > 0 && !holds) {
		set_error("invalid arguments (null holds with n_holds = " + std::to_string(n_holds) + ")");
		return PP_ERR_INVALID;
	}
	int run = 0; // holds of the current plan so far
	for (int k = 0; k < n_holds; k++) {
		const pp_hold& x = holds[k];
		const std::string which = "hold " + std::to_string(k);
		if (x.plan < 0 || x.plan >= h.n) {
			set_error("invalid arguments (" + which + " names plan " + std::to_string(x.plan) + " of " + std::to_string(h.n) + ")");
			return PP_ERR_INVALID;
		}
		if (x.row == 0) {
			set_error(h.name(x.plan) + ": " + which + " is at row 0, which cannot be held (t_0 = 0): shift the plan's t_start instead");
			return PP_ERR_INVALID;
		}
		if (x.row < 1) {
			set_error(h.name(x.plan) + ": " + which + " is at row " + std::to_string(x.row) + " (a hold's row is 1 .. N - 1)");
			return PP_ERR_INVALID;
		}
		if (!std::isfinite(x.seconds)) {
			set_error(h.name(x.plan) + ": " + which + " has seconds that are not finite");
			return PP_ERR_INVALID;
		}
		if (k > 0 && (x.plan < holds[k - 1].plan || (x.plan == holds[k - 1].plan && x.row <= holds[k - 1].row))) {
			set_error("invalid arguments (the holds are strictly ascending in (plan, row): " + which + " is not behind the one before it)");
			return PP_ERR_INVALID;
		}
		run = k > 0 && x.plan == holds[k - 1].plan ? run + 1 : 1;
		if (run > ppr::kMaxHolds) {
			set_error(h.name(x.plan) + " has more than " + std::to_string(ppr::kMaxHolds) + " holds");
			return PP_ERR_INVALID;
		}
	}
	return PP_OK;
}

/// ... and against what the holder remembers of its last speed-profile call: the rows into `plans`, the call into `call`, a hold's row against the N of
/// its plan's profile (a plan without one gets status -1 and its holds are skipped), the start of every plan's holds into `offsets` (n + 1) and the most
/// holds of one plan into `most`
int retime_profiles(const HeldPlans& h, const SpeedGroup& g, int n_holds, const pp_hold* holds, std::vector<ConflictArg>& plans, RetimeCall& call, std::vector<int32_t>& offsets,
	int& most)
{
	call = RetimeCall {};
	most = 0;
	if (h.n == 0)
		return PP_OK;
	const std::vector<double> noStart((size_t)h.n, 0.0);
	ConflictLattice lattice {};
	if (int rc = conflict_profiles(h, g, noStart.data(), lattice, plans))
		return rc;
	call = RetimeCall { lattice.maxSamples, 0, lattice.aAcc, lattice.aDec };
	offsets.assign((size_t)h.n + 1, 0);
	for (int k = 0; k < n_holds; k++) {
		const pp_hold& x = holds[k];
		const int N = plans[(size_t)x.plan].nSamples;
		if (N > 0 && x.row > N - 1) {
			set_error(h.name(x.plan) + ": hold " + std::to_string(k) + " is at row " + std::to_string(x.row) + " of a profile of " + std::to_string(N) +
				" rows (a hold's row is 1 .. N - 1)");
			return PP_ERR_INVALID;
		}
		offsets[(size_t)x.plan + 1]++;
	}
	for (int i = 0; i < h.n; i++) {
		most = std::max(most, (int)offsets[(size_t)i + 1]);
		offsets[(size_t)i + 1] += offsets[(size_t)i];
	}
	return PP_OK;
}

// ---- the services over held plans, one core each (pp_held_plans.hpp); both holders' extern "C" entries end here

/// the plans of a batch planner's last batch: queries 0 .. n-1
HeldPlans batch_plans(pp_planner* p, int n)
{
	HeldPlans h;
	h.pl = p;
	h.stream = p->map->ctx->stream;
	h.footprint = p->footprint;
	h.ownView = p->args.m;
	h.n = n;
	h.rows = (size_t)p->maxBatch;
	return h;
}

/// what the batch entries refuse first: a null planner, a count outside the last batch, a pipeline's buffer set (`byTicket`: the pipeline's entry for it)
int batch_check(const pp_planner* p, int n, const char* byTicket)
{
	if (!p || n < 0 || n > p->lastBatch) {
		set_error("invalid arguments (0 <= n_queries <= last batch)");
		return PP_ERR_INVALID;
	}
	if (p->pipelineOwned) {
		set_error(std::string("this planner is a pipeline's buffer set: ") + byTicket);
		return PP_ERR_INVALID;
	}
	return PP_OK;
}

/// a copy of the buffer set's search arguments under `view`: the set's own `args`, which a pipeline's top-up launches read, are not written
SearchArgs held_args(const HeldPlans& h, const ppd::MapView& view)
{
	SearchArgs args = h.pl->args;
	args.m = view;
	return args;
}

/// HybridAStar::SearchPath's post-processing of the plans of h under h.ownView: k_postprocess over a batch planner's queries, k_postprocess_tickets (which
/// also checks the smoothed path against the holder's footprint) over held slots.  The results stay in `g` for the getters.
int post_process_plans(const HeldPlans& h, PostGroup& g, float path_interpolation, const pp_smoother_params* smoother, int max_points, pp_post_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	pp_map* const map = pl->map;
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	PP_HIP_TRY(held_grow(h, g, max_points, pl->maxPath));
	const PostParams pp = post_params(path_interpolation, smoother, pl->params.min_turning_radius, max_points);
	const SearchArgs args = held_args(h, h.ownView);
	const uint32_t *obst = map->obstLabel[map->obstResult].get(), *voro = map->voroLabel[map->voroResult].get();
	if (int rc = held_run(h, g.rec, {}, results_host, [&](const int32_t* slotsDev) {
			const size_t lds = (size_t)max_points * 16;
			if (slotsDev)
				hipLaunchKernelGGL(k_postprocess_tickets, dim3(h.n), dim3(kPostThreads), lds, h.stream, args, pp, h.foot(), h.n, slotsDev, pl->paths.get(), pl->rsLogs.get(),
					pl->results.get(), obst, voro, g.buffers());
			else
				hipLaunchKernelGGL(k_postprocess, dim3(h.n), dim3(kPostThreads), lds, h.stream, args, pp, h.n, pl->paths.get(), pl->rsLogs.get(), pl->results.get(), obst, voro,
					g.buffers()); // (g.rec has been sized by now)
			return hipGetLastError();
		}, &g.host))
		return rc;
	g.points = max_points;
	return PP_OK;
}

/// Are the plans of h still collision-free on `target` under its view of this moment (every writer of a map's grids has drained the map's stream before it returned)?
int revalidate_plans(const HeldPlans& h, HeldBuffers<NoPlanArg, pp_revalidate_result>& b, pp_map* target, pp_revalidate_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const SearchArgs args = held_args(h, target->view());
	return held_run(h, b, {}, results_host, [&](const int32_t* slotsDev) {
		hipLaunchKernelGGL(k_revalidate_tickets, dim3(h.n), dim3(64), 0, h.stream, args, h.foot(), h.n, slotsDev, pl->paths.get(), pl->rsLogs.get(), pl->results.get(), b.out.get());
		return hipGetLastError();
	});
}

/// The plans of h stamped into `target`'s occupancy grid (`plans`: stamp_check's) under the target's view of this moment, with the holder's footprint or its
/// own map's point-validator disc.  The target's views are refreshed on the target's own stream once the holder's stream has been drained, i.e. behind the stamp.
int stamp_plans(const HeldPlans& h, HeldBuffers<StampArg, pp_stamp_result>& b, pp_map* target, const std::vector<StampArg>& plans, const pp_stamp_params* params,
	pp_stamp_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	if (int rc = stamp_prepare_target(target))
		return rc;
	const SearchArgs args = held_args(h, target->view());
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	if (int rc = held_run(h, b, plans, results_host,
			[&](const int32_t* slotsDev) { return launch_stamp(h.stream, args, discs, params, h.n, slotsDev, b.args.get(), pl, target->occ32.get(), b.out.get()); }))
		return rc;
	return stamp_finish_target(target);
}

/// The vehicles of `plans` (locate_check's) located on the plans of h.  The kernel reads and writes no map: the launch travels with the holder's own view.
int locate_plans(const HeldPlans& h, HeldBuffers<LocateArg, pp_locate_result>& b, const std::vector<LocateArg>& plans, const pp_locate_params* params,
	pp_locate_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const SearchArgs args = held_args(h, h.ownView);
	return held_run(h, b, plans, results_host,
		[&](const int32_t* slotsDev) { return launch_locate(h.stream, args, params, h.n, slotsDev, b.args.get(), pl, b.out.get()); });
}

/// Speeds and arrival times along the plans of h (`plans`: speed_check's).  With a clearance term the launch travels with the target's view of this moment and
/// the holder's footprint, or the point validator of the TARGET seen as one disc; without one it reads no map and travels with the holder's own view.  The
/// sample rows come back behind the kernel on the holder's stream, in the synchronisation held_run makes for the records, and the first n_samples rows of
/// every profiled plan go on to the caller's array.
int speed_profile_plans(const HeldPlans& h, SpeedGroup& g, pp_map* target, const std::vector<SpeedArg>& plans, const pp_speed_profile_params* params, int max_samples,
	double* samples_host, pp_speed_profile_result* results_host)
{
	g.profileOf.clear(); // (what the holder remembers of its last call ends here, whatever happens below: the rows are about to be rewritten)
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	PP_HIP_TRY(held_grow(h, g.samples, h.rows * (size_t)max_samples, { { &g.rows, h.rows * (size_t)max_samples * 24 } }));
	const bool clearance = params->clearance_gain > 0.0;
	const SearchArgs args = held_args(h, clearance ? target->view() : h.ownView);
	Footprint discs {};
	if (clearance) {
		discs = h.foot();
		if (!h.footprint) {
			discs.n = 1;
			discs.r[0] = target->minSafeRadius;
		}
	}
	const size_t stride = (size_t)max_samples * 3;
	std::vector<double> staged(samples_host ? (size_t)h.n * stride : 0);
	std::vector<pp_speed_profile_result> recs;
	if (int rc = held_run(h, g.rec, plans, results_host, [&](const int32_t* slotsDev) {
			if (const hipError_t e = launch_speed_profile(h.stream, args, discs, params, max_samples, h.n, slotsDev, g.rec.args.get(), pl, g.rows.get(), g.rec.out.get()))
				return e;
			return samples_host ? hipMemcpyAsync(staged.data(), g.rows.get(), staged.size() * 8, hipMemcpyDeviceToHost, h.stream) : hipSuccess;
		}, &recs))
		return rc;
	if (samples_host)
		for (size_t i = 0; i < (size_t)h.n; i++)
			if (recs[i].status == 0)
				std::copy(staged.begin() + i * stride, staged.begin() + i * stride + (size_t)recs[i].n_samples * 3, samples_host + i * stride);
	for (int i = 0; i < h.n; i++)
		g.profileOf[h.byTicket ? h.tickets[i] : (uint64_t)i] = SpeedGroup::Profile { i, recs[(size_t)i].status, recs[(size_t)i].n_samples };
	g.maxSamples = max_samples;
	g.aAcc = params->a_acc;
	g.aDec = params->a_dec;
	return PP_OK;
}

/// Trajectories of the plans of h on the lattice and the separation of `n_pairs` pairs of them (`plans`, `lattice`: conflict_check's and conflict_profiles').  Both
/// kernels, the pair list before them and every copy behind them run on the holder's stream, which held_run synchronises once.  The trajectory comes down only for a
/// caller that wants poses, and is interleaved here.
int conflict_plans(const HeldPlans& h, ConflictGroup& g, const SpeedGroup& speed, const std::vector<ConflictArg>& plans, const ConflictLattice& lattice, int n_pairs,
	const int32_t* pairs, double* poses_host, pp_trajectory_result* plans_host, pp_conflict_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const size_t n = (size_t)h.n, T = (size_t)lattice.T, nPairs = (size_t)n_pairs, component = n * T;
	PP_HIP_TRY(held_grow(h, g.doubles, component * kTrajectoryComponents, { { &g.traj, component * kTrajectoryComponents * 8 } }));
	if (pairs)
		PP_HIP_TRY(held_grow(h, g.listed, nPairs, { { &g.pairs, nPairs * 8 } }));
	PP_HIP_TRY(held_grow(h, g.pairRows, nPairs, { { &g.out, nPairs * sizeof(pp_conflict_result) } }));
	const SearchArgs args = held_args(h, h.ownView);
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	std::vector<double> staged(poses_host ? component * 3 : 0);
	std::vector<pp_conflict_result> recs(results_host ? nPairs : 0);
	if (int rc = held_run(h, g.rec, plans, plans_host, [&](const int32_t* slotsDev) {
			hipError_t e = hipSuccess;
			if (pairs && nPairs)
				e = hipMemcpyAsync(g.pairs, pairs, nPairs * 8, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = launch_trajectory(h.stream, args, lattice, discs.anyOffset != 0, h.n, slotsDev, g.rec.args.get(), pl, speed.rows.get(), g.traj.get(), g.rec.out.get());
			if (e == hipSuccess && nPairs)
				e = launch_conflict_pairs(h.stream, discs, lattice, h.n, (long long)nPairs, pairs ? g.pairs.get() : nullptr, g.traj.get(), g.rec.out.get(), g.out.get());
			if (e == hipSuccess && !recs.empty())
				e = hipMemcpyAsync(recs.data(), g.out, nPairs * sizeof(pp_conflict_result), hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && !staged.empty())
				e = hipMemcpyAsync(staged.data(), g.traj, staged.size() * 8, hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	std::copy(recs.begin(), recs.end(), results_host);
	if (poses_host)
		for (size_t i = 0; i < component; i++) // (plan-major in both: plan i, time m is i * T + m)
			for (size_t c = 0; c < 3; c++)
				poses_host[i * 3 + c] = staged[c * component + i];
	return PP_OK;
}

/// Start delays of the plans of h (`plans`, `lattice`: delay_check's and conflict_profiles'; D: the largest delay in lattice steps).  The host orders the vehicles
/// by level and lists each one's lower-index partners (pp_delay_rule.hpp); the extended trajectory is k_trajectory_tickets on the lattice k0 - D .. k1, in the
/// conflict call's buffers; then one k_delay_level per level.  Uploads, launches and the copy of the records run on the holder's stream, which held_run
/// synchronises once.
int deconflict_plans(const HeldPlans& h, ConflictGroup& c, DelayGroup& g, const SpeedGroup& speed, const std::vector<ConflictArg>& plans, const ConflictLattice& lattice, int D,
	int n_pairs, const int32_t* pairs, pp_delay_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const size_t n = (size_t)h.n, columns = (size_t)lattice.T + (size_t)D, nListed = (size_t)n_pairs, component = n * columns;
	std::vector<int32_t> offsets(n + 1), cursor(n), list(nListed), level(n), members(n);
	ppy::partner_offsets(h.n, n_pairs, pairs, offsets.data());
	ppy::partner_list(h.n, n_pairs, pairs, offsets.data(), cursor.data(), list.data());
	const int nLevels = ppy::levels(h.n, offsets.data(), list.data(), level.data());
	std::vector<int32_t> first((size_t)nLevels + 1);
	ppy::members_by_level(h.n, nLevels, level.data(), first.data(), members.data());
	PP_HIP_TRY(held_grow(h, c.doubles, component * kTrajectoryComponents, { { &c.traj, component * kTrajectoryComponents * 8 } }));
	PP_HIP_TRY(held_grow(h, g.vehicles, n, { { &g.members, n * 4 }, { &g.offsets, (n + 1) * 4 }, { &g.delays, n * 4 } }));
	if (nListed)
		PP_HIP_TRY(held_grow(h, g.listed, nListed, { { &g.partners, nListed * 4 } }));
	PP_HIP_TRY(held_grow(h, g.rows, n, { { &g.out, n * sizeof(pp_delay_result) } }));
	const SearchArgs args = held_args(h, h.ownView);
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	ConflictLattice extended = lattice;
	extended.k0 = lattice.k0 - D;
	extended.T = lattice.T + D;
	std::vector<pp_delay_result> recs(results_host ? n : 0);
	if (int rc = held_run(h, c.rec, plans, (pp_trajectory_result*)nullptr, [&](const int32_t* slotsDev) {
			hipError_t e = hipMemcpyAsync(g.members, members.data(), n * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(g.offsets, offsets.data(), (n + 1) * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && nListed)
				e = hipMemcpyAsync(g.partners, list.data(), nListed * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = launch_trajectory(h.stream, args, extended, discs.anyOffset != 0, h.n, slotsDev, c.rec.args.get(), pl, speed.rows.get(), c.traj.get(), c.rec.out.get());
			for (int l = 0; l < nLevels && e == hipSuccess; l++)
				e = launch_delay_level(h.stream, discs, lattice, D, h.n, first[(size_t)l + 1] - first[(size_t)l], g.members.get() + first[(size_t)l], g.offsets.get(),
					g.partners.get(), c.rec.args.get(), c.traj.get(), c.rec.out.get(), g.delays.get(), g.out.get());
			if (e == hipSuccess && !recs.empty())
				e = hipMemcpyAsync(recs.data(), g.out, n * sizeof(pp_delay_result), hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	std::copy(recs.begin(), recs.end(), results_host);
	return PP_OK;
}

/// Waits at the start or at stops of the plans of h (`plans`, `lattice`: wait_check's and conflict_profiles').  deconflict_plans with three additions on the holder's
/// stream: the flags and the committed waits go up; k_wait_places lists every plan's places behind the extended trajectory; and every level is k_wait_level.  The
/// places and their counts come down only for a caller that wants them.  held_run synchronises the stream once.
int deconflict_waits_plans(const HeldPlans& h, ConflictGroup& c, DelayGroup& g, WaitGroup& w, const SpeedGroup& speed, const std::vector<ConflictArg>& plans,
	const ConflictLattice& lattice, const pp_wait_params* params, const uint8_t* no_start_wait, const pp_wait_fixed* fixed, int n_pairs, const int32_t* pairs,
	int32_t* n_places_host, pp_wait_place* places_host, pp_wait_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const int D = params->delay.max_delay_steps;
	const WaitCall call { D, params->max_places, params->max_places > 0 ? params->max_places : 1, 0 };
	const size_t n = (size_t)h.n, columns = (size_t)lattice.T + (size_t)D, nListed = (size_t)n_pairs, component = n * columns, stride = (size_t)call.stride;
	std::vector<int32_t> offsets(n + 1), cursor(n), list(nListed), level(n), members(n);
	ppy::partner_offsets(h.n, n_pairs, pairs, offsets.data());
	ppy::partner_list(h.n, n_pairs, pairs, offsets.data(), cursor.data(), list.data());
	const int nLevels = ppy::levels(h.n, offsets.data(), list.data(), level.data());
	std::vector<int32_t> first((size_t)nLevels + 1);
	ppy::members_by_level(h.n, nLevels, level.data(), first.data(), members.data());
	PP_HIP_TRY(held_grow(h, c.doubles, component * kTrajectoryComponents, { { &c.traj, component * kTrajectoryComponents * 8 } }));
	PP_HIP_TRY(held_grow(h, g.vehicles, n, { { &g.members, n * 4 }, { &g.offsets, (n + 1) * 4 }, { &g.delays, n * 4 } }));
	if (nListed)
		PP_HIP_TRY(held_grow(h, g.listed, nListed, { { &g.partners, nListed * 4 } }));
	PP_HIP_TRY(held_grow(h, w.vehicles, n,
		{ { &w.fixed, n * sizeof(pp_wait_fixed) }, { &w.noStart, n }, { &w.counts, n * 4 }, { &w.states, n * sizeof(WaitState) }, { &w.out, n * sizeof(pp_wait_result) } }));
	PP_HIP_TRY(held_grow(h, w.listed, n * stride, { { &w.places, n * stride * sizeof(pp_wait_place) } }));
	const SearchArgs args = held_args(h, h.ownView);
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	ConflictLattice extended = lattice;
	extended.k0 = lattice.k0 - D;
	extended.T = lattice.T + D;
	const pp_wait_fixed* const fixedDev = fixed ? w.fixed.get() : nullptr;
	const uint8_t* const noStartDev = no_start_wait ? w.noStart.get() : nullptr;
	std::vector<pp_wait_result> recs(results_host ? n : 0);
	std::vector<int32_t> counts(n_places_host || places_host ? n : 0);
	std::vector<pp_wait_place> listedPlaces(places_host ? n * stride : 0);
	if (int rc = held_run(h, c.rec, plans, (pp_trajectory_result*)nullptr, [&](const int32_t* slotsDev) {
			hipError_t e = hipMemcpyAsync(g.members, members.data(), n * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(g.offsets, offsets.data(), (n + 1) * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && nListed)
				e = hipMemcpyAsync(g.partners, list.data(), nListed * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && fixed)
				e = hipMemcpyAsync(w.fixed, fixed, n * sizeof(pp_wait_fixed), hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && no_start_wait)
				e = hipMemcpyAsync(w.noStart, no_start_wait, n, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = launch_trajectory(h.stream, args, extended, discs.anyOffset != 0, h.n, slotsDev, c.rec.args.get(), pl, speed.rows.get(), c.traj.get(), c.rec.out.get());
			if (e == hipSuccess)
				e = launch_wait_places(h.stream, args, lattice, call, h.n, slotsDev, c.rec.args.get(), pl, speed.rows.get(), fixedDev, w.places.get(), w.counts.get());
			for (int l = 0; l < nLevels && e == hipSuccess; l++)
				e = launch_wait_level(h.stream, discs, lattice, call, h.n, first[(size_t)l + 1] - first[(size_t)l], g.members.get() + first[(size_t)l], g.offsets.get(),
					g.partners.get(), c.rec.args.get(), c.traj.get(), c.rec.out.get(), fixedDev, noStartDev, w.places.get(), w.counts.get(), w.states.get(), w.out.get());
			if (e == hipSuccess && !recs.empty())
				e = hipMemcpyAsync(recs.data(), w.out, n * sizeof(pp_wait_result), hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && !counts.empty())
				e = hipMemcpyAsync(counts.data(), w.counts, n * 4, hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && !listedPlaces.empty())
				e = hipMemcpyAsync(listedPlaces.data(), w.places, listedPlaces.size() * sizeof(pp_wait_place), hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	std::copy(recs.begin(), recs.end(), results_host);
	for (size_t i = 0; i < counts.size(); i++) {
		const size_t listedHere = counts[i] > 0 ? (size_t)counts[i] : 0; // (kWaitNoPlace: a fixed row that does not qualify lists nothing)
		if (n_places_host)
			n_places_host[i] = (int32_t)listedHere;
		if (places_host)
			std::copy(listedPlaces.begin() + i * stride, listedPlaces.begin() + i * stride + listedHere, places_host + i * stride);
	}
	return PP_OK;
}

/// Start delays of the plans of h that also clear the movers of `tracks` (tracks_check's; NULL or n_tracks == 0: none).  deconflict_plans with three additions on the
/// holder's stream: the track set goes up and k_track_samples samples it on the lattice's T times in front of the levels; every level is k_delay_level_tracks; and
/// for a caller that wants the (vehicle, track) records k_track_pairs runs once behind the last level.  held_run synchronises the stream once.
int deconflict_tracks_plans(const HeldPlans& h, ConflictGroup& c, DelayGroup& g, TrackGroup& t, const SpeedGroup& speed, const std::vector<ConflictArg>& plans,
	const ConflictLattice& lattice, int D, int n_pairs, const int32_t* pairs, const pp_track_set* tracks, pp_delay_result* results_host, pp_track_result* track_results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const size_t n = (size_t)h.n, columns = (size_t)lattice.T + (size_t)D, nListed = (size_t)n_pairs, component = n * columns;
	const size_t M = tracks ? (size_t)tracks->n_tracks : 0, nRows = M ? (size_t)tracks->offsets[M] : 0, nSamples = M * (size_t)lattice.T;
	const size_t nRecords = track_results_host ? n * M : 0;
	if (nRecords > 0x7FFFFFFFull) {
		set_error("invalid arguments (n * n_tracks = " + std::to_string(nRecords) + " track records: at most 2^31 - 1)");
		return PP_ERR_INVALID;
	}
	std::vector<int32_t> offsets(n + 1), cursor(n), list(nListed), level(n), members(n);
	ppy::partner_offsets(h.n, n_pairs, pairs, offsets.data());
	ppy::partner_list(h.n, n_pairs, pairs, offsets.data(), cursor.data(), list.data());
	const int nLevels = ppy::levels(h.n, offsets.data(), list.data(), level.data());
	std::vector<int32_t> first((size_t)nLevels + 1);
	ppy::members_by_level(h.n, nLevels, level.data(), first.data(), members.data());
	PP_HIP_TRY(held_grow(h, c.doubles, component * kTrajectoryComponents, { { &c.traj, component * kTrajectoryComponents * 8 } }));
	PP_HIP_TRY(held_grow(h, g.vehicles, n, { { &g.members, n * 4 }, { &g.offsets, (n + 1) * 4 }, { &g.delays, n * 4 } }));
	if (nListed)
		PP_HIP_TRY(held_grow(h, g.listed, nListed, { { &g.partners, nListed * 4 } }));
	PP_HIP_TRY(held_grow(h, g.rows, n, { { &g.out, n * sizeof(pp_delay_result) } }));
	PP_HIP_TRY(held_grow(h, t.tracks, M, { { &t.offsets, (M + 1) * 4 }, { &t.radii, M * 8 } }));
	PP_HIP_TRY(held_grow(h, t.rows, nRows, { { &t.waypoints, nRows * 24 } }));
	PP_HIP_TRY(held_grow(h, t.doubles, nSamples * 2, { { &t.samples, nSamples * 16 } }));
	PP_HIP_TRY(held_grow(h, t.records, nRecords, { { &t.out, nRecords * sizeof(pp_track_result) } }));
	const SearchArgs args = held_args(h, h.ownView);
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	ConflictLattice extended = lattice;
	extended.k0 = lattice.k0 - D;
	extended.T = lattice.T + D;
	const TrackView view { (int)M, t.offsets.get(), t.waypoints.get(), t.radii.get(), t.samples.get() };
	std::vector<pp_delay_result> recs(results_host ? n : 0);
	std::vector<pp_track_result> trackRecs(nRecords);
	if (int rc = held_run(h, c.rec, plans, (pp_trajectory_result*)nullptr, [&](const int32_t* slotsDev) {
			hipError_t e = hipMemcpyAsync(g.members, members.data(), n * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(g.offsets, offsets.data(), (n + 1) * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && nListed)
				e = hipMemcpyAsync(g.partners, list.data(), nListed * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && M)
				e = hipMemcpyAsync(t.offsets, tracks->offsets, (M + 1) * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && M)
				e = hipMemcpyAsync(t.radii, tracks->radii, M * 8, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && M)
				e = hipMemcpyAsync(t.waypoints, tracks->waypoints, nRows * 24, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && M)
				e = launch_track_samples(h.stream, lattice, view);
			if (e == hipSuccess)
				e = launch_trajectory(h.stream, args, extended, discs.anyOffset != 0, h.n, slotsDev, c.rec.args.get(), pl, speed.rows.get(), c.traj.get(), c.rec.out.get());
			for (int l = 0; l < nLevels && e == hipSuccess; l++)
				e = launch_delay_level_tracks(h.stream, discs, lattice, D, h.n, first[(size_t)l + 1] - first[(size_t)l], g.members.get() + first[(size_t)l], g.offsets.get(),
					g.partners.get(), c.rec.args.get(), c.traj.get(), c.rec.out.get(), view, g.delays.get(), g.out.get());
			if (e == hipSuccess && nRecords)
				e = launch_track_pairs(h.stream, discs, lattice, D, h.n, c.traj.get(), g.out.get(), view, t.out.get());
			if (e == hipSuccess && !recs.empty())
				e = hipMemcpyAsync(recs.data(), g.out, n * sizeof(pp_delay_result), hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && nRecords)
				e = hipMemcpyAsync(trackRecs.data(), t.out, nRecords * sizeof(pp_track_result), hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	std::copy(recs.begin(), recs.end(), results_host);
	std::copy(trackRecs.begin(), trackRecs.end(), track_results_host);
	return PP_OK;
}

/// The pairs of the plans of h that can meet (`plans`, `lattice`: pair_check's and conflict_profiles').  The extended trajectory is formed as deconflict_plans
/// forms it, in the conflict call's buffers; then k_plan_boxes, k_box_pairs to count, k_pair_offsets, k_box_pairs to fill, all on the holder's stream.  The stream
/// is synchronised once inside to learn n_found, which sizes the copy of the list, and once by held_run behind the copies.
int candidate_pairs_plans(const HeldPlans& h, ConflictGroup& c, PairGroup& g, const SpeedGroup& speed, const std::vector<ConflictArg>& plans, const ConflictLattice& lattice,
	const pp_pair_params* params, int32_t* pairs_host, int32_t* first_box_host, double* boxes_host, pp_pair_summary* summary)
{
	if (summary)
		*summary = pp_pair_summary {};
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const int D = params->delay.max_delay_steps, B = params->times_per_box;
	const size_t n = (size_t)h.n, columns = (size_t)lattice.T + (size_t)D, component = n * columns;
	const size_t NB = (size_t)ppb::box_count(lattice.T, B), nBoxes = n * NB;
	const long long all = (long long)n * (long long)(n - 1) / 2, room = params->max_pairs < all ? params->max_pairs : all; // (no more pairs than there are)
	PP_HIP_TRY(held_grow(h, c.doubles, component * kTrajectoryComponents, { { &c.traj, component * kTrajectoryComponents * 8 } }));
	PP_HIP_TRY(held_grow(h, g.doubles, nBoxes * kBoxComponents, { { &g.boxes, nBoxes * kBoxComponents * 8 } }));
	PP_HIP_TRY(held_grow(h, g.plans, n, { { &g.counts, n * 8 }, { &g.offsets, (n + 2) * 8 }, { &g.boxed, n * 4 } }));
	if (room)
		PP_HIP_TRY(held_grow(h, g.listed, (size_t)room, { { &g.pairs, (size_t)room * 8 }, { &g.firstBox, (size_t)room * 4 } }));
	const SearchArgs args = held_args(h, h.ownView);
	const Footprint discs = stamp_discs(h.footprint, pl->map);
	double R = 0.0;
	for (int a = 0; a < discs.n; a++) {
		const double r = ppb::disc_reach(discs.ox[a], discs.oy[a], (double)discs.r[a]);
		if (r > R)
			R = r;
	}
	const double reach = ppb::reach(lattice.margin, R);
	ConflictLattice extended = lattice;
	extended.k0 = lattice.k0 - D;
	extended.T = lattice.T + D;
	const BoxView view { h.n, (int)NB, g.boxes.get() };
	long long tail[2] = { 0, 0 }; // n_found, n_boxed
	size_t written = 0;
	std::vector<int32_t> list, first;
	std::vector<double> staged(boxes_host ? nBoxes * kBoxComponents : 0);
	if (int rc = held_run(h, c.rec, plans, (pp_trajectory_result*)nullptr, [&](const int32_t* slotsDev) {
			hipError_t e = launch_trajectory(h.stream, args, extended, discs.anyOffset != 0, h.n, slotsDev, c.rec.args.get(), pl, speed.rows.get(), c.traj.get(), c.rec.out.get());
			if (e == hipSuccess)
				e = launch_plan_boxes(h.stream, lattice.T, D, B, view, c.traj.get(), g.boxed.get());
			if (e == hipSuccess)
				e = launch_box_pairs(h.stream, false, view, reach, room, nullptr, g.counts.get(), nullptr, nullptr);
			if (e == hipSuccess)
				e = launch_pair_offsets(h.stream, h.n, g.counts.get(), g.boxed.get(), g.offsets.get());
			if (e == hipSuccess && room)
				e = launch_box_pairs(h.stream, true, view, reach, room, g.offsets.get(), nullptr, g.pairs.get(), g.firstBox.get());
			if (e == hipSuccess)
				e = hipMemcpyAsync(tail, g.offsets.get() + n, sizeof tail, hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess)
				e = hipStreamSynchronize(h.stream); // (n_found sizes the copy)
			if (e != hipSuccess)
				return e;
			written = (size_t)(tail[0] < room ? tail[0] : room);
			list.resize(written * 2);
			first.resize(first_box_host ? written : 0);
			if (written)
				e = hipMemcpyAsync(list.data(), g.pairs, written * 8, hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && !first.empty())
				e = hipMemcpyAsync(first.data(), g.firstBox, written * 4, hipMemcpyDeviceToHost, h.stream);
			if (e == hipSuccess && !staged.empty())
				e = hipMemcpyAsync(staged.data(), g.boxes, staged.size() * 8, hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	std::copy(list.begin(), list.end(), pairs_host);
	std::copy(first.begin(), first.end(), first_box_host);
	if (boxes_host)
		for (size_t i = 0; i < n; i++)
			for (size_t b = 0; b < NB; b++)
				for (size_t k = 0; k < (size_t)kBoxComponents; k++)
					boxes_host[(i * NB + b) * kBoxComponents + k] = staged[(k * NB + b) * n + i];
	if (summary) {
		summary->n_found = tail[0];
		summary->n_written = (int32_t)written;
		summary->n_boxes = (int32_t)NB;
		summary->reach = reach;
		summary->n_boxed = (int32_t)tail[1];
	}
	return PP_OK;
}

/// Look-ups into the timetables of the plans of h and their stop lists (`plans`, `call`: timetable_check's and timetable_profiles').  The values go up, the kernel
/// and every copy behind it run on the holder's stream, which held_run synchronises once.  The stop lists come down whole and only the listed rows of each plan
/// reach the caller's array.
int timetable_plans(const HeldPlans& h, TimetableGroup& g, const SpeedGroup& speed, const std::vector<ConflictArg>& plans, const TimetableCall& call, const double* values_host,
	pp_timetable_plan* plans_host, pp_timetable_stop* stops_host, pp_timetable_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	const size_t n = (size_t)h.n, lookups = n * (size_t)call.nPoints, listed = n * (size_t)call.maxStops;
	if (lookups)
		PP_HIP_TRY(held_grow(h, g.lookups, lookups, { { &g.values, lookups * 8 }, { &g.results, lookups * sizeof(pp_timetable_result) } }));
	if (listed)
		PP_HIP_TRY(held_grow(h, g.listed, listed, { { &g.stops, listed * sizeof(pp_timetable_stop) } }));
	const SearchArgs args = held_args(h, h.ownView);
	std::vector<pp_timetable_stop> staged(stops_host ? listed : 0);
	std::vector<pp_timetable_result> recs(results_host ? lookups : 0);
	std::vector<pp_timetable_plan> kept;
	if (int rc = held_run(
			h, g.rec, plans, plans_host,
			[&](const int32_t* slotsDev) {
				hipError_t e = hipSuccess;
				if (lookups)
					e = hipMemcpyAsync(g.values, values_host, lookups * 8, hipMemcpyHostToDevice, h.stream);
				if (e == hipSuccess)
					e = launch_timetable(h.stream, args, call, h.n, slotsDev, g.rec.args.get(), pl, speed.rows.get(), lookups ? g.values.get() : nullptr,
						listed ? g.stops.get() : nullptr, lookups ? g.results.get() : nullptr, g.rec.out.get());
				if (e == hipSuccess && !recs.empty())
					e = hipMemcpyAsync(recs.data(), g.results, lookups * sizeof(pp_timetable_result), hipMemcpyDeviceToHost, h.stream);
				if (e == hipSuccess && !staged.empty())
					e = hipMemcpyAsync(staged.data(), g.stops, listed * sizeof(pp_timetable_stop), hipMemcpyDeviceToHost, h.stream);
				return e;
			},
			&kept))
		return rc;
	std::copy(recs.begin(), recs.end(), results_host);
	if (!staged.empty())
		for (size_t i = 0; i < n; i++) // (rows behind n_listed stay as the caller left them)
			std::copy(staged.begin() + i * (size_t)call.maxStops, staged.begin() + i * (size_t)call.maxStops + (size_t)kept[i].n_listed, stops_host + i * (size_t)call.maxStops);
	return PP_OK;
}

/// The holds of a call written into the timetables of the plans of h (`plans`, `call`, `offsets`, `most`: retime_check's and retime_profiles').  Offsets and
/// holds go up, the kernel rewrites the t column of the speed-profile group's rows in place, and every copy runs behind it on the holder's stream, which
/// held_run synchronises once.  When the rows are wanted, the span of the rows buffer the call's plans lie in comes down in one copy, and the first N rows of
/// every plan with a profile go on to the caller's array.
int retime_plans(const HeldPlans& h, RetimeGroup& g, SpeedGroup& speed, const std::vector<ConflictArg>& plans, const RetimeCall& call, const std::vector<int32_t>& offsets,
	int most, int n_holds, const pp_hold* holds, double* rows_host, pp_retime_result* results_host)
{
	if (h.n == 0)
		return PP_OK;
	pp_planner* const pl = h.pl;
	PP_HIP_TRY(hipSetDevice(pl->map->ctx->device));
	PP_HIP_TRY(held_grow(h, g.plans, h.rows, { { &g.offsets, (h.rows + 1) * 4 } }));
	if (n_holds)
		PP_HIP_TRY(held_grow(h, g.listed, (size_t)n_holds, { { &g.holds, (size_t)n_holds * sizeof(pp_hold) } }));
	const size_t stride = (size_t)call.maxSamples * 3;
	size_t lo = SIZE_MAX, hi = 0; // the rows of the speed-profile group that plans of this call with a profile use
	if (rows_host)
		for (const ConflictArg& a : plans)
			if (a.nSamples > 0) {
				lo = std::min(lo, (size_t)a.row);
				hi = std::max(hi, (size_t)a.row + 1);
			}
	std::vector<double> staged(lo < hi ? (hi - lo) * stride : 0);
	if (int rc = held_run(h, g.rec, plans, results_host, [&](const int32_t*) {
			hipError_t e = hipMemcpyAsync(g.offsets, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess && n_holds)
				e = hipMemcpyAsync(g.holds, holds, (size_t)n_holds * sizeof(pp_hold), hipMemcpyHostToDevice, h.stream);
			if (e == hipSuccess)
				e = launch_retime(h.stream, call, h.n, most, g.rec.args.get(), g.offsets.get(), n_holds ? g.holds.get() : nullptr, speed.rows.get(), g.rec.out.get());
			if (e == hipSuccess && !staged.empty())
				e = hipMemcpyAsync(staged.data(), speed.rows.get() + lo * stride, staged.size() * 8, hipMemcpyDeviceToHost, h.stream);
			return e;
		}))
		return rc;
	if (!staged.empty())
		for (size_t i = 0; i < (size_t)h.n; i++)
			if (plans[i].nSamples > 0) {
				const double* const from = staged.data() + ((size_t)plans[i].row - lo) * stride;
				std::copy(from, from + (size_t)plans[i].nSamples * 3, rows_host + i * stride);
			}
	return PP_OK;
}

void free_planner(pp_planner* p)
{
	if (!p)
		return;
#if PP_ROWS_STATS
	{
		unsigned long long h[24] = {};
		if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_rowsStats), sizeof h) == hipSuccess) {
			fprintf(stderr, "[rows stats] wave iterations with 1/2/3/4 busy rows: %llu %llu %llu %llu\n", h[1], h[2], h[3], h[4]);
			static const char* const names[14] = { "take", "set-aside", "pop+refill", "node", "child validity", "march", "truncate+cost", "cell-node+staging", "insert", "write", "rs", "endpoint", "keymap+heuristics", "voronoi" };
			unsigned long long tot = 0, it = h[1] + h[2] + h[3] + h[4];
			for (int i = 0; i < 14; i++)
				tot += h[8 + i];
			for (int i = 0; i < 14; i++)
				fprintf(stderr, "[rows stats]   %-18s %5.1f %%  %8.0f clk / wave iteration\n", names[i], 100.0 * (double)h[8 + i] / (double)(tot ? tot : 1), (double)h[8 + i] / (double)(it ? it : 1));
		}
	}
#endif
	pp_map* map = p->map;
	pph::footprint_release(p->footprint);
	delete p;
	pph::map_release(map); // the planner kept its map (and through it the context) alive
}

} // namespace

enum class PlannerUse { Batches, Pipeline, PipelineLogged };
static int create_planner(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, int32_t search_rows, PlannerUse use, pp_planner** out);

extern "C" {

int pp_planner_create(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, pp_planner** out)
{
	return pp_planner_create_ex(map, params, max_batch, max_nodes_per_query, 0, out);
}

int pp_planner_create_ex(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, int32_t search_rows, pp_planner** out)
{
	return create_planner(map, params, max_batch, max_nodes_per_query, search_rows, PlannerUse::Batches, out);
}

/// use: Batches = pp_planner_create_ex's planner; Pipeline / PipelineLogged = the buffer set of a streaming pipeline (pp_pipeline.hpp):
/// max_batch field slots, always the rows kernel, no hand-over lists, the expansion log only when asked for (4 B x max_nodes per slot)
static int create_planner(pp_map* map, const pp_hybrid_params* params, int32_t max_batch, int32_t max_nodes_per_query, int32_t search_rows, PlannerUse use, pp_planner** out)
{
	const bool forPipeline = use != PlannerUse::Batches;
	if (!map || !params || !out || max_batch < 1 || max_nodes_per_query < 16 || search_rows < 0) {
		set_error("invalid arguments");
		return PP_ERR_INVALID;
	}
	if (!map->dist || !map->occ8 || !map->pathcost) {
		set_error("map set incomplete: upload dist2, occupancy and path cost first");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(map->ctx->device));
	auto* p = new pp_planner();
	p->map = map;
	__atomic_add_fetch(&map->refs, 1, __ATOMIC_RELAXED);
	p->params = *params;
	p->maxBatch = max_batch;
	p->maxNodes = max_nodes_per_query;

	// StatePropagator constructor, hybrid_a_star.cpp:13-29: deltas {0, +d1, -d1, +d2, -d2, ...}
	const double wheelbase = params->wheelbase, rearToCenter = 0.0;
	// GetSteeringAngleFromTurningRadius, kinematic_bicycle_model.cpp:34-41
	const double deltaMax = std::atan(wheelbase / std::sqrt(std::pow(params->min_turning_radius, 2) - std::pow(rearToCenter, 2)));
	p->deltas.push_back(0.0);
	for (unsigned int i = 0; i < params->num_generated_motion / 2; i++) {
		double delta = (i + 1) / 2.0 * deltaMax;
		p->deltas.push_back(delta);
		p->deltas.push_back(-delta);
	}
	SearchArgs& A = p->args;
	A.m = map->view();
	if (int rc = primitives_from_deltas(p)) {
		free_planner(p);
		return rc;
	}
	A.rp.arcLength = params->spatial_resolution * 1.5;
	A.rp.spatialRes = params->spatial_resolution;
	A.rp.angularRes = params->angular_resolution;
	A.rp.lat.set(params->spatial_resolution, params->angular_resolution);
	A.rp.forwardMult = params->forward_cost_multiplier;
	A.rp.reverseMult = params->reverse_cost_multiplier;
	A.rp.voronoiMult = params->voronoi_cost_multiplier;
	A.rp.voroDiagRes = (float)(map->desc.resolution * std::sqrt(2.0));
	A.rp.headingAlias = params->heading_alias;
	int32_t dims[3];
	double offs[2];
	if (int rc = pp_nonholo_dims(map->desc.lower, map->desc.upper, params, dims, offs)) {
		free_planner(p);
		return rc;
	}
	A.heur.nx = dims[0];
	A.heur.ny = dims[1];
	A.heur.na = dims[2];
	A.heur.spatialRes = params->spatial_resolution;
	A.heur.angularRes = params->angular_resolution;
	A.heur.lat.set(params->spatial_resolution, params->angular_resolution);
	A.heur.offX = offs[0];
	A.heur.offY = offs[1];
	A.heur.minMult = std::min(params->reverse_cost_multiplier, params->forward_cost_multiplier);
	A.heur.negativeKRead = params->negative_k_read;
	// ObstaclesHeuristic constructor, heuristics.cpp:97-104
	A.heur.obstDiagRes = (float)(std::sqrt(2) * map->desc.resolution);
	A.heur.obstCostMult = (float)(std::min(params->reverse_cost_multiplier, params->forward_cost_multiplier) * map->desc.resolution);
	A.rmin = params->min_turning_radius;
	A.rsRev = (float)params->reverse_cost_multiplier;
	A.rsFwd = (float)params->forward_cost_multiplier;
	A.rsSw = (float)params->direction_switching_cost;
	A.maxNodes = max_nodes_per_query;
	A.maxPath = max_nodes_per_query < 2048 ? max_nodes_per_query : 2048;
	p->maxPath = A.maxPath;
	A.cells = map->cells();
	A.fieldElems = (int64_t)field_tiled_elems(map->desc.rows, map->desc.cols);
	// key space: every discrete pose a state inside the bounds (plus one arc of slack) can take
	{
		const double sres = params->spatial_resolution, ares = params->angular_resolution;
		const double slack = A.rp.arcLength + 1.0;
		KeySpace& ks = A.ks;
		ks.x0 = (int)std::floor((map->desc.lower[0] - slack) / sres) - 1;
		ks.y0 = (int)std::floor((map->desc.lower[1] - slack) / sres) - 1;
		ks.nx = (int)std::ceil((map->desc.upper[0] + slack) / sres) + 1 - ks.x0 + 1;
		ks.ny = (int)std::ceil((map->desc.upper[1] + slack) / sres) + 1 - ks.y0 + 1;
		// heading bins: (int)(wrap(theta) / ares) in [-tmax, tmax]; with the reference's Release-build aliasing
		// (Appendix A Q6) every bin is folded into [-3, 3] by Pose2<int>::WrapTheta
		int tmax = (int)(M_PI / ares) + 1;
		if (params->heading_alias && tmax > 3)
			tmax = 3;
		ks.t0 = -tmax;
		ks.nt = 2 * tmax + 1;
		ks.nt = (ks.nt + 3) / 4 * 4; // keeps every query's key map 16-byte aligned
	}

	const size_t B = (size_t)max_batch, N = (size_t)max_nodes_per_query;
	const size_t tableBytes = (size_t)dims[0] * dims[1] * dims[2] * sizeof(double);
	p->wfBytesPerSlot = pph::wavefront_workspace_bytes(map->desc.rows, map->desc.cols);
	{
		const int resident = pph::wavefront_resident_blocks();
		p->wfSlots = max_batch < resident ? max_batch : resident;
	}
	{
		int perCu = 0, dev = 0;
		hipDeviceProp_t prop;
		p->searchWaves = 2048;
		if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
			hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_hybrid_search_rows<false>, 64 * PP_ROWS_WAVES_PER_WG, 0) == hipSuccess && perCu >= 1)
			p->searchWaves = perCu * PP_ROWS_WAVES_PER_WG * prop.multiProcessorCount;
		// Which search kernel?  The four-queries-per-wave kernel (pp_planner_rows.hpp) issues ~4x fewer instructions per
		// expansion and needs node/heap/key-map buffers only for its resident rows, so many batches fit in HBM at once;
		// the one-query-per-wave kernel advances a single query ~1.4x faster.  Throughput-sized planners take the
		// former, small ones (the plugin's single-query path) the latter.  PP_SEARCH_ROWS=0/1 forces either.
		const char* env = getenv("PP_SEARCH_ROWS");
		p->rowsKernel = forPipeline || (env && (env[0] == '0' || env[0] == '1') ? env[0] == '1' : max_batch > 64);
		// rows (= buffer slots) of the persistent grid: as many as can be resident, unless the caller shares the GPU
		// between several planners (bench.py: resident rows / batches in flight)
		int rows = p->searchWaves * kRowsPerWave;
		if (search_rows > 0 && search_rows < rows)
			rows = search_rows;
		const int wanted = (max_batch + kRowsPerWave - 1) / kRowsPerWave * kRowsPerWave;
		if (wanted < rows)
			rows = wanted;
		p->searchRows = (rows + kRowsPerWave - 1) / kRowsPerWave * kRowsPerWave;
		// A batch ends with its longest query (65 k expansions when a goal is unreachable for the car).  Queries that reach
		// `suspendAfter` expansions are set aside by the rows kernel (open list flushed into the heap, scalars in a
		// SuspendRec, the row goes on in a spare slot) and finished one query per wave, 14 instead of ~25 us per expansion.
		// Only the extreme tail moves: per expansion the rows kernel is the cheaper one and the GPU is capacity-bound with
		// eight batches in flight (measured: 32768 -> 10.2 k plans/s, 8192 -> 8.0 k, never -> 9.8 k).  PP_SEARCH_SUSPEND_AFTER=0:
		// no hand-over.
		// tuning knobs from the environment are clamped to their meaningful ranges: none of them may change results or
		// make an allocation size negative
		auto env_int = [](const char* name, int dflt, int lo, int hi) {
			const char* v = getenv(name);
			if (!v || !*v)
				return dflt;
			const long x = strtol(v, nullptr, 10);
			return (int)(x < lo ? lo : (x > hi ? hi : x));
		};
		A.suspendAfter = p->rowsKernel && !forPipeline ? env_int("PP_SEARCH_SUSPEND_AFTER", 32768, 0, 1 << 30) : 0; // (a pipeline's rows keep their queries)
		A.extraSlots = A.suspendAfter > 0 ? env_int("PP_SEARCH_EXTRA_SLOTS", (max_batch + 15) / 16, 0, max_batch) : 0; // queries that may be set aside (the rest stays)
		A.searchRows = p->searchRows;
		A.listCap = A.extraSlots + p->searchRows;
	}
	hipError_t e = hipSuccess;
	// Headroom.  The kernels this planner launches need scratch (private segment: k_hybrid_search_rows 408 B, k_wavefront
	// 132 B, k_hybrid_search 112 B per lane, tools/kernel_resources.py), which the runtime allocates per hardware queue at a
	// kernel's FIRST dispatch: private bytes x 64 lanes x every wave slot of the device.  A planner that takes the last byte
	// of HBM makes that allocation fail and the runtime aborts the process (round 1: HSA_STATUS_ERROR_OUT_OF_RESOURCES in
	// k_wavefront after a 2048-row planner).  So: (i) the kernels are dispatched once with empty grids BEFORE the large
	// allocations, which makes this stream's queue allocate its scratch now, and (ii) the planner refuses to take memory
	// beyond free - reserve, where the reserve covers the same scratch for the other hardware queues a process may use.
	size_t planned = 0;
	std::vector<std::pair<pph::DeviceMem*, size_t>> wanted; // taken below, after the warm-up and the headroom check
	auto alloc = [&](pph::DeviceMem& mem, size_t bytes) {
		bytes = bytes ? bytes : 1;
		wanted.push_back({ &mem, bytes });
		planned += (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1); // the allocator works in 2 MiB granules
	};
	alloc(p->table, tableBytes);
	alloc(p->costFields, B * (size_t)A.fieldElems * sizeof(float));
	alloc(p->wfWorkspace, (size_t)p->wfBytesPerSlot * p->wfSlots);
	alloc(p->tilesCtl, 64);
	alloc(p->tilesFallback, B * 4);
	alloc(p->wfError, 32); // control block: {wavefront error flag, wavefront goal counter, rows query counter, set-aside count, (unused),
	                                // (unused), wavefront done counter, spare slots handed out}
	// search buffers: one set per resident row (rows kernel) or per query (one-query-per-wave kernel)
	const size_t S = p->rowsKernel ? (size_t)p->searchRows + (size_t)A.extraSlots : B;
	alloc(p->suspended, (size_t)(A.listCap > 0 ? A.listCap : 1) * sizeof(SuspendRec));
	alloc(p->mtStates, (p->rowsKernel ? S : 1) * Mt64::N * sizeof(unsigned long long));
	alloc(p->nodes, S * N * sizeof(Node));
	alloc(p->bands, S * (size_t)(kBands * kBandCap) * sizeof(HeapEntry));
	alloc(p->bandMeta, S * (size_t)kBands);
	alloc(p->heaps, S * N * sizeof(HeapEntry));
	alloc(p->keymaps, S * A.ks.size() * 4);
	if (use != PlannerUse::Pipeline) // (a pipeline keeps the expansion log only for parity tests: 4 B x max_nodes per field slot)
		alloc(p->expanded, B * N * 4);
	alloc(p->order, B * 4);
	alloc(p->orderKeys, B * 4);
	alloc(p->paths, B * (size_t)A.maxPath * sizeof(PathRec));
	alloc(p->rsLogs, B * kRsLogCap * sizeof(RsLogEntry));
	alloc(p->results, B * sizeof(DevResult));
	if (!p->rowsKernel) { // the lattice-line log of pp_planner_certify_lattice: planners that keep the tree per query
		alloc(p->guardLog, B * (size_t)kGuardLogCap * sizeof(GuardRec));
		alloc(p->guardCount, B * 4);
	}
	alloc(p->prof, (forPipeline ? 1 : B) * PH_COUNT * sizeof(unsigned long long));
	alloc(p->dStarts, B * 24);
	alloc(p->dGoals, B * 24);
	alloc(p->dSeeds, B * 8);
	{
		if (int rc = warm_up_kernels(p, map)) {
			free_planner(p);
			return rc;
		}
		size_t freeB = 0, totalB = 0;
		e = hipMemGetInfo(&freeB, &totalB);
		int dev = 0;
		hipDeviceProp_t prop;
		size_t reserve = (size_t)1 << 30;
		if (e == hipSuccess && hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
			const size_t waveSlots = (size_t)prop.multiProcessorCount * 32; // 8 waves on each of a CU's 4 SIMDs
			reserve += (size_t)kMaxPrivateBytes * 64 * waveSlots * kReserveQueues;
		}
		if (e == hipSuccess && planned + reserve > freeB) {
			free_planner(p);
			set_error("planner needs " + std::to_string(planned >> 20) + " MiB, the device has " + std::to_string(freeB >> 20) + " MiB free and " +
				std::to_string(reserve >> 20) + " MiB stay reserved for kernel scratch");
			return PP_ERR_CAPACITY;
		}
		for (auto& w : wanted)
			if (e == hipSuccess)
				e = w.first->alloc(w.second);
	}
	if (e == hipSuccess)
		e = hipMemset(p->tilesCtl, 0, 64);
	if (e == hipSuccess)
		e = p->e0.create();
	if (e == hipSuccess)
		e = p->e1.create();
	if (e == hipSuccess)
		e = p->e2.create();
	if (e != hipSuccess) {
		free_planner(p);
		return pph::hip_fail(e, "planner allocation");
	}
	A.heur.table = p->table;
	A.guardLog = p->guardLog;
	A.guardCount = p->guardCount;
	p->nextQuery = p->wfError + 2;
	p->nh.nx = dims[0];
	*out = p;
	return PP_OK;
}

int pp_planner_destroy(pp_planner* planner)
{
	if (!planner)
		return PP_OK;
	(void)hipSetDevice(planner->map->ctx->device);
	(void)hipStreamSynchronize(planner->map->ctx->stream);
	free_planner(planner);
	return PP_OK;
}

int pp_planner_num_primitives(pp_planner* planner) { return planner ? planner->args.prims.n : 0; }

int pp_planner_set_footprint(pp_planner* planner, pp_footprint* fp)
{
	if (!planner) {
		set_error("null planner");
		return PP_ERR_INVALID;
	}
	if (fp) {
		if (planner->pipelineOwned) {
			set_error("this planner is a pipeline's buffer set: the pipeline's search grid gets its footprint from pp_pipeline_set_footprint, not from its planner");
			return PP_ERR_INVALID;
		}
		if (planner->rowsKernel) {
			set_error("this planner runs the four-queries-per-wave rows kernel, which takes no footprint: create the planner with max_batch <= 64, or with PP_SEARCH_ROWS=0 "
					  "in the environment");
			return PP_ERR_INVALID;
		}
		if (fp->map != planner->map) {
			set_error("the footprint belongs to another map than the planner's: create one for the planner's map with pp_footprint_create");
			return PP_ERR_INVALID;
		}
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	hipStream_t s = planner->map->ctx->stream;
	PP_HIP_TRY(hipStreamSynchronize(s)); // a batch in flight keeps the footprint it was launched with
	if (fp) {
		// an empty dispatch: the queue allocates the kernel's scratch here, where a failure is an error code (see warm_up_kernels)
		PP_HIP_TRY(launch_search_footprint(planner, s, 1, fp->fp, Queries {}));
		PP_HIP_TRY(hipStreamSynchronize(s));
		__atomic_add_fetch(&fp->refs, 1, __ATOMIC_RELAXED);
	}
	pp_footprint* old = planner->footprint;
	planner->footprint = fp;
	pph::footprint_release(old);
	return PP_OK;
}

int pp_planner_set_heuristic_clearance(pp_planner* planner, float radius)
{
	if (!planner) {
		set_error("null planner");
		return PP_ERR_INVALID;
	}
	if (int rc = pph::clearance_check_radius(radius))
		return rc;
	if (planner->pipelineOwned) {
		set_error("this planner is a pipeline's buffer set: the pipeline's field launches get their clearance from pp_pipeline_set_heuristic_clearance, not from its planner");
		return PP_ERR_INVALID;
	}
	if (radius == planner->clearance.radius)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	PP_HIP_TRY(hipStreamSynchronize(planner->map->ctx->stream)); // a batch in flight keeps the views it was launched with
	planner->clearance.radius = radius; // (the views are built by the next batch, on the map's stream in front of its field launch)
	return PP_OK;
}

int pp_planner_heuristic_clearance(pp_planner* planner, float* radius)
{
	if (!planner || !radius) {
		set_error("null argument");
		return PP_ERR_INVALID;
	}
	*radius = planner->clearance.radius;
	return PP_OK;
}

int pp_planner_set_primitives(pp_planner* planner, int32_t n_steering_angles, const double* steering_angles)
{
	if (!planner || !steering_angles || n_steering_angles < 1) {
		set_error("invalid arguments");
		return PP_ERR_INVALID;
	}
	if (planner->owner && pp_pipeline_in_flight(planner->owner) > 0) {
		// the persistent search grid received its primitive table when its waves were launched: waves of later launches would get the new
		// one, and a query's result would depend on which wave claims it
		set_error("the pipeline has queries in flight: poll them all before changing the primitives");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	PP_HIP_TRY(hipStreamSynchronize(planner->map->ctx->stream)); // a batch in flight keeps the table it was launched with
	const std::vector<double> before = planner->deltas;
	planner->deltas.assign(steering_angles, steering_angles + n_steering_angles);
	if (int rc = primitives_from_deltas(planner)) {
		planner->deltas = before;
		(void)primitives_from_deltas(planner);
		return rc;
	}
	return PP_OK;
}

int pp_planner_set_nonholo_table(pp_planner* planner, const double* table_host)
{
	if (!planner) {
		set_error("null planner");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	hipStream_t s = planner->map->ctx->stream;
	const HeurView& h = planner->args.heur;
	const size_t bytes = (size_t)h.nx * h.ny * h.na * sizeof(double);
	if (table_host) {
		PP_HIP_TRY(hipMemcpyAsync(planner->table, table_host, bytes, hipMemcpyHostToDevice, s));
	} else {
		if (int rc = pp_nonholo_build_dev(planner->map->ctx, planner->map->desc.lower, planner->map->desc.upper, &planner->params, planner->table))
			return rc;
	}
	PP_HIP_TRY(hipStreamSynchronize(s));
	planner->tableReady = true;
	return PP_OK;
}

int pp_planner_start_after_fields_of(pp_planner* planner, pp_planner* predecessor)
{
	if (!planner || !predecessor || planner == predecessor || planner->map->ctx->device != predecessor->map->ctx->device) {
		set_error("two different planners on the same device");
		return PP_ERR_INVALID;
	}
	planner->startAfter = predecessor->e1; // recorded behind the predecessor's wavefront launch; never recorded = no wait
	return PP_OK;
}

int pp_planner_get_nonholo_table(pp_planner* planner, double* table_host)
{
	if (!planner || !table_host || !planner->tableReady) {
		set_error("table not available");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	const HeurView& h = planner->args.heur;
	PP_HIP_TRY(hipMemcpy(table_host, planner->table, (size_t)h.nx * h.ny * h.na * sizeof(double), hipMemcpyDeviceToHost));
	return PP_OK;
}

int pp_planner_search_batch_dev(pp_planner* planner, int32_t n_queries, const double* starts_dev, const double* goals_dev, const uint64_t* seeds_dev)
{
	if (!planner || n_queries < 0 || n_queries > planner->maxBatch || (n_queries > 0 && (!starts_dev || !goals_dev || !seeds_dev))) {
		set_error("invalid arguments (n_queries must be <= max_batch)");
		return PP_ERR_INVALID;
	}
	if (planner->pipelineOwned) {
		set_error("this planner is a pipeline's buffer set (pp_pipeline_planner): queries go through pp_pipeline_submit");
		return PP_ERR_INVALID;
	}
	if (planner->footprint && planner->profile) {
		set_error("phase profiling (pp_planner_set_profiling) is not available with a footprint: clear one of the two");
		return PP_ERR_INVALID;
	}
	if (n_queries == 0)
		return PP_OK;
	planner->speed.profileOf.clear(); // the speed profiles the planner remembers are the last batch's plans'
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	if (!planner->tableReady)
		if (int rc = pp_planner_set_nonholo_table(planner, nullptr))
			return rc;
	hipStream_t s = planner->map->ctx->stream;
	planner->args.m = planner->map->view(); // validator tunables may have changed
	const MapView& m = planner->args.m;
	if (planner->startAfter) { // phase this batch behind another planner's (throughput use, several batches in flight)
		PP_HIP_TRY(hipStreamWaitEvent(s, planner->startAfter, 0));
		planner->startAfter = nullptr;
	}
	PP_HIP_TRY(hipMemsetAsync(planner->wfError, 0, 32, s)); // the step's only fill: every counter of every kernel
	if (planner->guardCount)
		PP_HIP_TRY(hipMemsetAsync(planner->guardCount, 0, (size_t)n_queries * 4, s));
	PP_HIP_TRY(hipEventRecord(planner->e0, s));
	// the rows kernel hands the queries out longest-first (order written by the wavefront kernel's last workgroup)
	static const bool lpt = !(getenv("PP_SEARCH_ORDER") && getenv("PP_SEARCH_ORDER")[0] == '0');
	const bool ordered = planner->rowsKernel && lpt && n_queries <= 4096 && n_queries > planner->searchRows;
	// ObstaclesHeuristic::Update for every query's goal (hybrid_a_star.cpp:249)
#ifdef PP_ENABLE_DEBUG_SKIP // diagnostic builds only (tools/build_variant.py skip -DPP_ENABLE_DEBUG_SKIP=1; bench.py --debug-skip): the shipped
	// library always runs both kernels.  1 = no wavefront launch, 2 = no search launch, 3 = set-aside queries are dropped
	const char* const dbgEnv = getenv("PP_DEBUG_SKIP");
	const int dbgSkip = dbgEnv ? atoi(dbgEnv) : 0;
#else
	constexpr int dbgSkip = 0;
#endif
	if (dbgSkip != 1) {
		// a heuristic clearance: the field kernels read the planner's views of the occupancy (brought up to date here, on this stream) instead of the map's
		const bool inflated = planner->clearance.radius != 0.0f;
		if (inflated)
			if (int rc = pph::clearance_prepare(planner->map, planner->clearance, nullptr))
				return rc;
		MapView wm = m;
		if (inflated)
			wm.occ8 = planner->clearance.blocked8; // (what the ordered kernel reads; the search kernels never read occupancy)
		pph::WavefrontLaunch L;
		L.nGoals = n_queries;
		L.goalPoses = goals_dev;
		L.cost = planner->costFields;
		L.tiledOut = true;
		L.workspace = planner->wfWorkspace.get();
		L.workspaceBytesPerSlot = planner->wfBytesPerSlot;
		L.nSlots = planner->wfSlots;
		L.errorFlag = planner->wfError;
		L.countersZeroed = true;
		if (ordered) {
			L.orderStarts = starts_dev;
			L.orderOut = planner->order;
		}
		L.doneCounter = planner->wfError + 6;
		L.orderKeys = planner->orderKeys;
		L.pub.tilesCtl = planner->tilesCtl;
		L.pub.tilesFallback = planner->tilesFallback;
		L.pub.occBits = inflated ? planner->clearance.bits.get() : planner->map->occBits.get();
		PP_HIP_TRY(pph::launch_wavefront(s, wm, L));
	}
	PP_HIP_TRY(hipEventRecord(planner->e1, s));
	const Queries batch { n_queries, starts_dev, goals_dev, seeds_dev };
	if (dbgSkip == 2) {
	} else if (planner->rowsKernel) {
		// four queries per wave, taken from a counter by a persistent grid (pp_planner_rows.hpp)
		const int wavesWanted = (n_queries + kRowsPerWave - 1) / kRowsPerWave;
		const int wavesMax = planner->searchRows / kRowsPerWave;
		const int grid = wavesWanted < wavesMax ? wavesWanted : wavesMax;
		planner->args.rowsWaves = grid;
		PP_HIP_TRY(launch_search_rows<false>(planner, s, planner->args, batch, ordered ? planner->order.get() : nullptr, PipeView {}));
		if (planner->args.suspendAfter > 0 && dbgSkip != 3) // whatever was set aside: one wave per query (the block count is read on the device)
			PP_HIP_TRY(launch_search<false>(planner, s, planner->args.listCap, batch, /*resume=*/true));
	} else if (planner->footprint)
		PP_HIP_TRY(launch_search_footprint(planner, s, n_queries, planner->footprint->fp, batch));
	else if (planner->profile)
		PP_HIP_TRY(launch_search<true>(planner, s, n_queries, batch));
	else
		PP_HIP_TRY(launch_search<false>(planner, s, n_queries, batch));
	PP_HIP_TRY(hipEventRecord(planner->e2, s));
	planner->lastBatch = n_queries;
	return PP_OK;
}

int pp_planner_fetch_results(pp_planner* planner, int32_t n_queries, pp_query_result* results_host)
{
	if (!planner || n_queries < 0 || n_queries > planner->lastBatch || (n_queries > 0 && !results_host)) {
		set_error("invalid arguments");
		return PP_ERR_INVALID;
	}
	if (planner->pipelineOwned) {
		set_error("this planner is a pipeline's buffer set: its results arrive through pp_pipeline_poll");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	hipStream_t s = planner->map->ctx->stream;
	planner->hostResults.resize(planner->lastBatch);
	int32_t err = 0;
	PP_HIP_TRY(hipMemcpyAsync(planner->hostResults.data(), planner->results, (size_t)planner->lastBatch * sizeof(DevResult), hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipMemcpyAsync(&err, planner->wfError, 4, hipMemcpyDeviceToHost, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	(void)hipEventElapsedTime(&planner->wavefrontMs, planner->e0, planner->e1);
	(void)hipEventElapsedTime(&planner->searchMs, planner->e1, planner->e2);
	if (err) {
		set_error("obstacle-heuristic open list exceeded its workspace");
		return PP_ERR_CAPACITY;
	}
	for (int i = 0; i < n_queries; i++)
		results_host[i] = planner->hostResults[i].r;
	return PP_OK;
}

int pp_planner_search_batch(pp_planner* planner, int32_t n_queries, const double* starts_host, const double* goals_host, const uint64_t* seeds_host,
	pp_query_result* results_host)
{
	if (!planner || n_queries < 0 || n_queries > planner->maxBatch || (n_queries > 0 && (!starts_host || !goals_host || !seeds_host || !results_host))) {
		set_error("invalid arguments (n_queries must be <= max_batch)");
		return PP_ERR_INVALID;
	}
	if (planner->pipelineOwned) {
		set_error("this planner is a pipeline's buffer set (pp_pipeline_planner): queries go through pp_pipeline_submit");
		return PP_ERR_INVALID;
	}
	if (n_queries == 0)
		return PP_OK;
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	hipStream_t s = planner->map->ctx->stream;
	PP_HIP_TRY(hipMemcpyAsync(planner->dStarts, starts_host, (size_t)n_queries * 24, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(planner->dGoals, goals_host, (size_t)n_queries * 24, hipMemcpyHostToDevice, s));
	PP_HIP_TRY(hipMemcpyAsync(planner->dSeeds, seeds_host, (size_t)n_queries * 8, hipMemcpyHostToDevice, s));
	if (int rc = pp_planner_search_batch_dev(planner, n_queries, planner->dStarts, planner->dGoals, planner->dSeeds))
		return rc;
	return pp_planner_fetch_results(planner, n_queries, results_host);
}

int pp_planner_debug_nodes(pp_planner* planner, int32_t q, int32_t max_nodes, int32_t* parents_host, double* poses_host, double* costs_host, int32_t* dead_host)
{
	if (!planner || q < 0 || q >= planner->lastBatch || (int)planner->hostResults.size() <= q || max_nodes < 0) {
		set_error("no fetched result for this query (call pp_planner_fetch_results first)");
		return PP_ERR_INVALID;
	}
	if (planner->rowsKernel) {
		set_error("node records are kept per query by the one-query-per-wave kernel only (PP_SEARCH_ROWS=0 or max_batch <= 64)");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	int n = planner->hostResults[q].r.n_nodes;
	if (n > max_nodes)
		n = max_nodes;
	std::vector<Node> nodes(n);
	if (n)
		PP_HIP_TRY(hipMemcpy(nodes.data(), planner->nodes + (size_t)q * planner->maxNodes, (size_t)n * sizeof(Node), hipMemcpyDeviceToHost));
	for (int i = 0; i < n; i++) {
		if (parents_host)
			parents_host[i] = nodes[i].parent;
		if (poses_host) {
			poses_host[3 * i] = nodes[i].x;
			poses_host[3 * i + 1] = nodes[i].y;
			poses_host[3 * i + 2] = nodes[i].t;
		}
		if (costs_host) {
			costs_host[2 * i] = nodes[i].pathCost;
			costs_host[2 * i + 1] = nodes[i].totalCost;
		}
		if (dead_host)
			dead_host[i] = nodes[i].dead;
	}
	return PP_OK;
}

int pp_planner_debug_node_actions(pp_planner* planner, int32_t q, int32_t max_nodes, int32_t* action_host, double* length_host)
{
	if (!planner || q < 0 || q >= planner->lastBatch || (int)planner->hostResults.size() <= q || max_nodes < 0) {
		set_error("no fetched result for this query (call pp_planner_fetch_results first)");
		return PP_ERR_INVALID;
	}
	if (planner->rowsKernel) {
		set_error("node records are kept per query by the one-query-per-wave kernel only (PP_SEARCH_ROWS=0 or max_batch <= 64)");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	int n = planner->hostResults[q].r.n_nodes;
	if (n > max_nodes)
		n = max_nodes;
	std::vector<Node> nodes(n);
	if (n)
		PP_HIP_TRY(hipMemcpy(nodes.data(), planner->nodes + (size_t)q * planner->maxNodes, (size_t)n * sizeof(Node), hipMemcpyDeviceToHost));
	for (int i = 0; i < n; i++) {
		if (action_host)
			action_host[i] = nodes[i].action;
		if (length_host)
			length_host[i] = nodes[i].length;
	}
	return PP_OK;
}

/// SURVEY 7.3 H2 as a contract.  The search kernel flags every child whose DiscretizePose quotient lies within 1e-9 cells of a lattice
/// line (n_lattice_boundary_hits) -- the only poses a last-bit difference between this libm and glibc could put into another cell
/// (pose differences are ~1e-15) -- and, on planners that keep the tree, logs them: parent node, primitive, arc length, the cell the
/// device chose.  Here the host recomputes (i) every CREATED constant-steer node and (ii) every LOGGED constant-steer child with the
/// C library the reference links (glibc sin / cos), each along its own chain of ancestors from the start pose -- the arithmetic the
/// reference performs (KinematicBicycleModel::ConstantSteer, models/kinematic_bicycle_model.cpp:5-32, through
/// PathConstantSteer::Interpolate with the stored, possibly truncated, length) -- and discretises it (HybridAStar::DiscretizePose,
/// algo/hybrid_a_star.h:104-111).  n_cell_mismatches: recomputed cells that differ from the device's.  n_unverified: flagged events
/// that cannot be recomputed here (a Reeds-Shepp child on a lattice line; log entries beyond the 64 kept per query).
/// Both 0 certifies the query's discrete outputs against the reference's arithmetic; else: hand the query to the CPU reference.
/// Needs the tree, i.e. a planner of the one-query-per-wave kind (max_batch <= 64 or PP_SEARCH_ROWS=0); queries of a throughput planner
/// or pipeline that report n_lattice_boundary_hits > 0 are re-planned on such a planner (same device code, same results) first.
int pp_planner_certify_lattice(pp_planner* planner, int32_t q, int32_t* n_checked, int32_t* n_cell_mismatches, int32_t* n_unverified, double* max_pose_difference)
{
	if (!planner || q < 0 || q >= planner->lastBatch || (int)planner->hostResults.size() <= q) {
		set_error("no fetched result for this query (call pp_planner_fetch_results first)");
		return PP_ERR_INVALID;
	}
	if (planner->rowsKernel || !planner->guardLog) {
		set_error("the search tree and the lattice-line log are kept per query by the one-query-per-wave kernel only (PP_SEARCH_ROWS=0 or max_batch <= 64)");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	const int n = planner->hostResults[q].r.n_nodes;
	std::vector<Node> nodes((size_t)(n > 0 ? n : 0));
	if (n > 0)
		PP_HIP_TRY(hipMemcpy(nodes.data(), planner->nodes + (size_t)q * planner->maxNodes, (size_t)n * sizeof(Node), hipMemcpyDeviceToHost));
	int nLog = 0;
	PP_HIP_TRY(hipMemcpy(&nLog, planner->guardCount + q, 4, hipMemcpyDeviceToHost));
	const int kept = nLog < kGuardLogCap ? nLog : kGuardLogCap;
	std::vector<GuardRec> log((size_t)kept);
	if (kept > 0)
		PP_HIP_TRY(hipMemcpy(log.data(), planner->guardLog + (size_t)q * kGuardLogCap, (size_t)kept * sizeof(GuardRec), hipMemcpyDeviceToHost));
	const SearchArgs& A = planner->args;
	auto wrap = [](double t) { // geometry/2dplane.h:36-45
		while (t > M_PI)
			t -= 2 * M_PI;
		while (t < -M_PI)
			t += 2 * M_PI;
		return t;
	};
	auto cell = [&](double x, double y, double t, int c[3]) { // hybrid_a_star.h:104-111 (x86 conversions), Pose2<int>::WrapTheta's aliasing (Appendix A Q6) when the planner models it
		c[0] = (int)(x / A.rp.spatialRes);
		c[1] = (int)(y / A.rp.spatialRes);
		int it = (int)(wrap(t) / A.rp.angularRes);
		if (A.rp.headingAlias) {
			while ((double)it > M_PI)
				it = (int)((double)it - 2 * M_PI);
			while ((double)it < -M_PI)
				it = (int)((double)it + 2 * M_PI);
		}
		c[2] = it;
	};
	auto steer = [&](double& x, double& y, double& t, int prim, double length) { // kinematic_bicycle_model.cpp:5-32 with beta = 0
		const double kappa = A.prims.kappa[prim];
		const double dist = A.prims.backward[prim] ? -length : length;
		if (std::fabs(kappa) > 1e-9) {
			const double t0 = t;
			t += dist * kappa;
			x += 1 / kappa * (std::sin(t) - std::sin(t0));
			y += 1 / kappa * (-std::cos(t) + std::cos(t0));
		} else {
			x += dist * std::cos(t);
			y += dist * std::sin(t);
		}
	};
	std::vector<double> hx((size_t)n), hy((size_t)n), ht((size_t)n);
	int checked = 0, bad = 0, unverified = nLog - kept;
	double worst = 0.0;
	for (int i = 0; i < n; i++) {
		const Node& nd = nodes[(size_t)i];
		const int a = nd.action;
		if (nd.parent < 0 || nd.parent >= i || a < 0 || a >= A.prims.n) { // root; Reeds-Shepp child (its pose is the path's end, not an arc's)
			hx[(size_t)i] = nd.x;
			hy[(size_t)i] = nd.y;
			ht[(size_t)i] = nd.t;
			continue;
		}
		double x = hx[(size_t)nd.parent], y = hy[(size_t)nd.parent], t = ht[(size_t)nd.parent];
		steer(x, y, t, a, nd.length);
		hx[(size_t)i] = x;
		hy[(size_t)i] = y;
		ht[(size_t)i] = t;
		int ch[3], cd[3];
		cell(x, y, t, ch);
		cell(nd.x, nd.y, nd.t, cd);
		checked++;
		if (ch[0] != cd[0] || ch[1] != cd[1] || ch[2] != cd[2])
			bad++;
		const double d = std::fmax(std::fmax(std::fabs(x - nd.x), std::fabs(y - nd.y)), std::fabs(t - nd.t));
		worst = d > worst ? d : worst;
	}
	for (const GuardRec& g : log) { // children on a lattice line, created or not
		if (g.kind != 1 || g.parent < 0 || g.parent >= n || g.prim < 0 || g.prim >= A.prims.n) {
			unverified++;
			continue;
		}
		double x = hx[(size_t)g.parent], y = hy[(size_t)g.parent], t = ht[(size_t)g.parent];
		steer(x, y, t, g.prim, g.length);
		int ch[3];
		cell(x, y, t, ch);
		checked++;
		if (ch[0] != g.ix || ch[1] != g.iy || ch[2] != g.it)
			bad++;
	}
	if (n_checked)
		*n_checked = checked;
	if (n_cell_mismatches)
		*n_cell_mismatches = bad;
	if (n_unverified)
		*n_unverified = unverified;
	if (max_pose_difference)
		*max_pose_difference = worst;
	return PP_OK;
}

int pp_planner_search_rows(pp_planner* planner) { return planner && planner->rowsKernel ? planner->searchRows : 0; }

int pp_planner_set_profiling(pp_planner* planner, int32_t enable)
{
	if (!planner) {
		set_error("null planner");
		return PP_ERR_INVALID;
	}
	if (enable && planner->rowsKernel) {
		set_error("phase profiling exists for the one-query-per-wave kernel only: create the planner with PP_SEARCH_ROWS=0");
		return PP_ERR_INVALID;
	}
	planner->profile = enable != 0;
	return PP_OK;
}

int pp_planner_phase_cycles(pp_planner* planner, int32_t n_queries, uint64_t* cycles_host)
{
	if (!planner || n_queries < 0 || n_queries > planner->lastBatch || !cycles_host) {
		set_error("invalid arguments");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	PP_HIP_TRY(hipMemcpy(cycles_host, planner->prof, (size_t)n_queries * PH_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return PP_OK;
}

int pp_planner_postprocess(pp_planner* planner, int32_t n_queries, float path_interpolation, const pp_smoother_params* smoother, int32_t max_points, pp_post_result* results_host)
{
	if (!planner || n_queries < 0 || n_queries > planner->lastBatch || max_points < 8 || max_points > 8 * kPostThreads || !(path_interpolation > 0.0f)) {
		set_error("invalid arguments (n_queries <= last batch, 8 <= max_points <= 2048, path_interpolation > 0)");
		return PP_ERR_INVALID;
	}
	if (int rc = post_check_grids(planner->map))
		return rc;
	if (n_queries == 0)
		return PP_OK;
	planner->args.m = planner->map->view(); // the planner's own map as it is now
	return post_process_plans(batch_plans(planner, n_queries), planner->post, path_interpolation, smoother, max_points, results_host);
}

int pp_planner_get_processed_path(pp_planner* planner, int32_t q, double* sampled_host, uint8_t* cusp_host, double* smoothed_host)
{
	if (!planner || q < 0 || q >= (int)planner->post.host.size()) {
		set_error("no post-processed result for this query (pp_planner_postprocess first)");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	const PostGroup& g = planner->post;
	hipStream_t s = planner->map->ctx->stream;
	PP_HIP_TRY(g.copy_out((size_t)q * (size_t)g.points, (size_t)g.host[q].n_points, 0, sampled_host, cusp_host, smoothed_host, s));
	PP_HIP_TRY(hipStreamSynchronize(s));
	return PP_OK;
}

int pp_planner_revalidate(pp_planner* planner, pp_map* target, int32_t n_queries, pp_revalidate_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_revalidate re-validates its held tickets"))
		return rc;
	pp_map* const map = target ? target : planner->map;
	if (int rc = revalidate_check_target(planner->map, map))
		return rc;
	return revalidate_plans(batch_plans(planner, n_queries), planner->reval, map, results_host);
}

int pp_planner_stamp(pp_planner* planner, pp_map* target, int32_t n_queries, const int32_t* values, const double* from_length, const double* to_length,
	const pp_stamp_params* params, pp_stamp_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_stamp stamps its held tickets"))
		return rc;
	pp_map* const map = target ? target : planner->map;
	const HeldPlans h = batch_plans(planner, n_queries);
	std::vector<StampArg> plans;
	if (int rc = stamp_check(h, map, values, from_length, to_length, params, plans))
		return rc;
	return stamp_plans(h, planner->stamp, map, plans, params, results_host);
}

int pp_planner_speed_profile(pp_planner* planner, pp_map* target, int32_t n_queries, const double* from_length, const double* to_length, const double* v_start,
	const double* v_end, const pp_speed_profile_params* params, int32_t max_samples, double* samples_host, pp_speed_profile_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_speed_profile profiles its held tickets"))
		return rc;
	pp_map* const map = target ? target : planner->map;
	const HeldPlans h = batch_plans(planner, n_queries);
	std::vector<SpeedArg> plans;
	if (int rc = speed_check(h, map, from_length, to_length, v_start, v_end, params, max_samples, plans))
		return rc;
	return speed_profile_plans(h, planner->speed, map, plans, params, max_samples, samples_host, results_host);
}

int pp_planner_conflicts(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs, const pp_conflict_params* params,
	double* poses_host, pp_trajectory_result* plans_host, pp_conflict_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_conflicts looks at its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	ConflictLattice lattice;
	if (int rc = conflict_check(h, t_start, n_pairs, pairs, params, lattice))
		return rc;
	std::vector<ConflictArg> plans;
	if (int rc = conflict_profiles(h, planner->speed, t_start, lattice, plans))
		return rc;
	return conflict_plans(h, planner->conflict, planner->speed, plans, lattice, n_pairs, pairs, poses_host, plans_host, results_host);
}

int pp_planner_deconflict(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs, const pp_delay_params* params,
	pp_delay_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_deconflict schedules its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	ConflictLattice lattice;
	if (int rc = delay_check(h, t_start, n_pairs, pairs, params, lattice))
		return rc;
	std::vector<ConflictArg> plans;
	if (int rc = conflict_profiles(h, planner->speed, t_start, lattice, plans))
		return rc;
	return deconflict_plans(h, planner->conflict, planner->delay, planner->speed, plans, lattice, params ? params->max_delay_steps : 0, n_pairs, pairs, results_host);
}

int pp_planner_deconflict_tracks(pp_planner* planner, int32_t n_queries, const double* t_start, int32_t n_pairs, const int32_t* pairs, const pp_delay_params* params,
	const pp_track_set* tracks, pp_delay_result* results_host, pp_track_result* track_results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_deconflict_tracks schedules its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	ConflictLattice lattice;
	if (int rc = delay_check(h, t_start, n_pairs, pairs, params, lattice))
		return rc;
	if (h.n == 0)
		return PP_OK; // (whatever the tracks)
	if (int rc = tracks_check(tracks, lattice.T))
		return rc;
	std::vector<ConflictArg> plans;
	if (int rc = conflict_profiles(h, planner->speed, t_start, lattice, plans))
		return rc;
	return deconflict_tracks_plans(h, planner->conflict, planner->delay, planner->track, planner->speed, plans, lattice, params->max_delay_steps, n_pairs, pairs, tracks,
		results_host, track_results_host);
}

int pp_planner_deconflict_waits(pp_planner* planner, int32_t n_queries, const double* t_start, const uint8_t* no_start_wait, const pp_wait_fixed* fixed, int32_t n_pairs,
	const int32_t* pairs, const pp_wait_params* params, int32_t* n_places_host, pp_wait_place* places_host, pp_wait_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_deconflict_waits schedules its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	ConflictLattice lattice;
	if (int rc = wait_check(h, t_start, no_start_wait, fixed, n_pairs, pairs, params, lattice))
		return rc;
	std::vector<ConflictArg> plans;
	if (int rc = conflict_profiles(h, planner->speed, t_start, lattice, plans))
		return rc;
	return deconflict_waits_plans(h, planner->conflict, planner->delay, planner->wait, planner->speed, plans, lattice, params, no_start_wait, fixed, n_pairs, pairs,
		n_places_host, places_host, results_host);
}

int pp_planner_candidate_pairs(pp_planner* planner, int32_t n_queries, const double* t_start, const pp_pair_params* params, int32_t* pairs_host, int32_t* first_box_host,
	double* boxes_host, pp_pair_summary* summary)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_candidate_pairs lists the pairs of its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	ConflictLattice lattice;
	if (int rc = pair_check(h, t_start, params, pairs_host, lattice))
		return rc;
	std::vector<ConflictArg> plans;
	if (int rc = conflict_profiles(h, planner->speed, t_start, lattice, plans))
		return rc;
	return candidate_pairs_plans(h, planner->conflict, planner->pair, planner->speed, plans, lattice, params, pairs_host, first_box_host, boxes_host, summary);
}

int pp_planner_timetable(pp_planner* planner, int32_t n_queries, int32_t n_points, const double* values_host, const pp_timetable_params* params, pp_timetable_plan* plans_host,
	pp_timetable_stop* stops_host, pp_timetable_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_timetable looks its held tickets' timetables up"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	if (int rc = timetable_check(h, n_points, values_host, params))
		return rc;
	std::vector<ConflictArg> plans;
	TimetableCall call;
	if (int rc = timetable_profiles(h, planner->speed, n_points, params, plans, call))
		return rc;
	return timetable_plans(h, planner->timetable, planner->speed, plans, call, values_host, plans_host, stops_host, results_host);
}

int pp_planner_retime(pp_planner* planner, int32_t n_queries, int32_t n_holds, const pp_hold* holds, double* rows_host, pp_retime_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_retime writes holds into its held tickets' timetables"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	if (int rc = retime_check(h, n_holds, holds))
		return rc;
	std::vector<ConflictArg> plans;
	std::vector<int32_t> offsets;
	RetimeCall call;
	int most = 0;
	if (int rc = retime_profiles(h, planner->speed, n_holds, holds, plans, call, offsets, most))
		return rc;
	return retime_plans(h, planner->retime, planner->speed, plans, call, offsets, most, n_holds, holds, rows_host, results_host);
}

int pp_planner_locate(pp_planner* planner, int32_t n_queries, const double* poses_host, const double* from_length, const double* to_length, const pp_locate_params* params,
	pp_locate_result* results_host)
{
	if (int rc = batch_check(planner, n_queries, "pp_pipeline_locate locates vehicles on its held tickets"))
		return rc;
	const HeldPlans h = batch_plans(planner, n_queries);
	std::vector<LocateArg> plans;
	if (int rc = locate_check(h, poses_host, from_length, to_length, params, plans))
		return rc;
	return locate_plans(h, planner->locate, plans, params, results_host);
}

int pp_planner_last_timings(pp_planner* planner, float* wavefront_ms, float* search_ms)
{
	if (!planner) {
		set_error("null planner");
		return PP_ERR_INVALID;
	}
	if (wavefront_ms)
		*wavefront_ms = planner->wavefrontMs;
	if (search_ms)
		*search_ms = planner->searchMs;
	return PP_OK;
}

int pp_planner_get_path(pp_planner* planner, int32_t q, double* poses_host, int32_t* kind_host, int32_t* prim_host, double* length_host, double* tuv_host)
{
	if (!planner || q < 0 || q >= planner->lastBatch || (int)planner->hostResults.size() <= q) {
		set_error("no fetched result for this query (call pp_planner_fetch_results first)");
		return PP_ERR_INVALID;
	}
	const DevResult& r = planner->hostResults[q];
	if (r.r.status != 0 || r.solutionNode < 0)
		return PP_OK; // empty path
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	const int n = r.r.n_path;
	if (n > planner->maxPath) {
		set_error("solution path longer than the planner's path buffer");
		return PP_ERR_CAPACITY;
	}
	std::vector<PathRec> recs(n); // goal first (write_path)
	if (n)
		PP_HIP_TRY(hipMemcpy(recs.data(), planner->paths + (size_t)q * planner->maxPath, (size_t)n * sizeof(PathRec), hipMemcpyDeviceToHost));
	std::vector<RsLogEntry> rslog(r.nRsLog);
	if (r.nRsLog)
		PP_HIP_TRY(hipMemcpy(rslog.data(), planner->rsLogs + (size_t)q * kRsLogCap, (size_t)r.nRsLog * sizeof(RsLogEntry), hipMemcpyDeviceToHost));
	for (int i = 0; i < n; i++) {
		const PathRec& nd = recs[n - 1 - i];
		if (poses_host) {
			poses_host[3 * i] = nd.x;
			poses_host[3 * i + 1] = nd.y;
			poses_host[3 * i + 2] = nd.t;
		}
		const int kind = nd.action < 0 ? 0 : (nd.action >= 1000 ? 2 : 1);
		if (kind_host)
			kind_host[i] = kind;
		if (prim_host)
			prim_host[i] = kind == 2 ? nd.action - 1000 : nd.action;
		if (length_host)
			length_host[i] = nd.length;
		if (tuv_host) {
			tuv_host[3 * i] = tuv_host[3 * i + 1] = tuv_host[3 * i + 2] = 0.0;
			if (kind == 2)
				for (const auto& le : rslog)
					if (le.node == nd.node) {
						tuv_host[3 * i] = le.t;
						tuv_host[3 * i + 1] = le.u;
						tuv_host[3 * i + 2] = le.v;
					}
		}
	}
	return PP_OK;
}

int pp_planner_get_expanded(pp_planner* planner, int32_t q, int32_t* cells_host)
{
	if (!planner || q < 0 || q >= planner->lastBatch || (int)planner->hostResults.size() <= q || !cells_host) {
		set_error("no fetched result for this query (call pp_planner_fetch_results first)");
		return PP_ERR_INVALID;
	}
	if (!planner->expanded) {
		set_error("this planner keeps no expansion log (a pipeline created with log_expansions = 0)");
		return PP_ERR_INVALID;
	}
	const DevResult& r = planner->hostResults[q];
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	const int ne = r.r.n_expanded;
	if (ne == 0)
		return PP_OK;
	std::vector<uint32_t> keys(ne); // packed discrete pose of every expanded node, in expansion order
	PP_HIP_TRY(hipMemcpy(keys.data(), planner->expanded + (size_t)q * planner->maxNodes, (size_t)ne * 4, hipMemcpyDeviceToHost));
	const KeySpace& ks = planner->args.ks;
	for (int i = 0; i < ne; i++) {
		int ix = 0, iy = 0, it = 0;
		if (keys[i] != kNoKey)
			ks.unpack(keys[i], ix, iy, it);
		cells_host[3 * i] = ix;
		cells_host[3 * i + 1] = iy;
		cells_host[3 * i + 2] = it;
	}
	return PP_OK;
}

int pp_planner_get_obstacle_field(pp_planner* planner, int32_t q, float* cost_host)
{
	if (!planner || q < 0 || q >= planner->maxBatch || !cost_host) {
		set_error("invalid arguments (q is a query of the last batch, or a field slot of a pipeline)");
		return PP_ERR_INVALID;
	}
	PP_HIP_TRY(hipSetDevice(planner->map->ctx->device));
	if (!planner->pipelineOwned)
		PP_HIP_TRY(hipStreamSynchronize(planner->map->ctx->stream));
	const int rows = planner->map->desc.rows, cols = planner->map->desc.cols;
	std::vector<float> tiled((size_t)planner->args.fieldElems);
	PP_HIP_TRY(hipMemcpy(tiled.data(), planner->costFields + (size_t)q * (size_t)planner->args.fieldElems, tiled.size() * sizeof(float), hipMemcpyDeviceToHost));
	for (int r = 0; r < rows; r++)
		for (int c = 0; c < cols; c++)
			cost_host[(size_t)r * cols + c] = tiled[field_tiled_index(cols, r, c)];
	return PP_OK;
}

} // extern "C"

#include "pp_pipeline.hpp"

// Internal host-side declarations shared by the .hip translation units of libpphip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/pp_hip.h"
#include "pp_device.hpp"
#include "pp_footprint_device.hpp"
#include "pp_ticket_table.hpp"

namespace pph {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define PP_HIP_TRY(expr)                       \
	do {                                       \
		hipError_t _e = (expr);                \
		if (_e != hipSuccess)                  \
			return pph::hip_fail(_e, #expr);   \
	} while (0)

// ---- owners of GPU resources -----------------------------------------------
// Move-only; the destructor releases.  Everything on the host side of libpphip.so that allocates device or pinned memory, or creates
// an event or a stream, holds it in one of these: no function frees by hand, and an early return cannot leak.
template <typename H, hipError_t (*Release)(H)>
class Owner {
protected:
	H h_ = nullptr;

public:
	Owner() = default;
	Owner(Owner&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
	~Owner() { reset(); }
	void reset()
	{
		if (h_)
			(void)Release(h_);
		h_ = nullptr;
	}
	H get() const { return h_; }
};
struct DeviceMem : Owner<void*, hipFree> {
	/// a zero-byte request still yields a valid pointer
	hipError_t alloc(size_t bytes)
	{
		reset();
		return hipMalloc(&h_, bytes ? bytes : 1);
	}
	/// allocates only if empty
	hipError_t ensure(size_t bytes) { return h_ ? hipSuccess : alloc(bytes); }
	template <typename T>
	T* as() const { return (T*)h_; }
};
/// a DeviceMem that reads as a T* (the members of the long-lived handles)
template <typename T>
struct Dev : DeviceMem {
	T* get() const { return (T*)h_; }
	operator T*() const { return (T*)h_; }
	T* operator->() const { return (T*)h_; }
};
/// pinned host memory, read as a T*
template <typename T>
struct Pinned : Owner<void*, hipHostFree> {
	hipError_t alloc(size_t bytes)
	{
		reset();
		return hipHostMalloc(&h_, bytes ? bytes : 1, hipHostMallocDefault);
	}
	T* get() const { return (T*)h_; }
	operator T*() const { return (T*)h_; }
};
struct Event : Owner<hipEvent_t, hipEventDestroy> {
	hipError_t create(unsigned flags = hipEventDefault) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
	operator hipEvent_t() const { return h_; }
};
/// non-blocking streams (all of this library's are)
struct Stream : Owner<hipStream_t, hipStreamDestroy> {
	hipError_t create() { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
	hipError_t create(int priority) { return h_ ? hipSuccess : hipStreamCreateWithPriority(&h_, hipStreamNonBlocking, priority); }
	operator hipStream_t() const { return h_; }
};

constexpr int kMaxPrimitives = 128;
struct PrimTable {
	int n;
	double kappa[kMaxPrimitives];
	double invKappa[kMaxPrimitives]; // 1 / kappa as the host divides it (= the device's own `1 / kappa`, both correctly rounded); unused when |kappa| <= 1e-9
	int8_t backward[kMaxPrimitives];
};

struct RolloutParams {
	double arcLength;        // 1.5 * spatialResolution (hybrid_a_star.cpp:115)
	double spatialRes, angularRes;
	ppd::Resolutions lat;    // the same two with their reciprocals (discretize_pose)
	double forwardMult, reverseMult, voronoiMult;
	float voroDiagRes;       // (float)(resolution * sqrt(2.0)), hybrid_a_star.cpp:38
	int headingAlias;
};

struct NonHoloDesc {
	int nx, ny, na;
	double spatialRes, angularRes, offX, offY;
	double rmin;
	float reverseCost, forwardCost, switchCost;
	double minMult; // min(reverse, forward) as doubles (heuristics.cpp:90)
	int negativeKRead;
};

// ---- launchers (pp_kernels_basic.hip) ------------------------------------
hipError_t launch_d2_to_distance(hipStream_t s, const int32_t* d2, float* dist, int64_t n, float res);
hipError_t launch_occ_to_u8(hipStream_t s, const int32_t* occ, uint8_t* occ8, int64_t n);
hipError_t launch_check_states(hipStream_t s, const ppd::MapView& m, int64_t n, const double* poses, uint8_t* valid);
hipError_t launch_check_states_fused(hipStream_t s, const ppd::MapView& m, int64_t n, uint64_t seed, uint64_t* count);
hipError_t launch_check_arcs(hipStream_t s, const ppd::MapView& m, int64_t n, const double* from, const double* kappa, const double* length, const int32_t* dir,
	uint8_t* valid, float* last);
hipError_t launch_check_segments(hipStream_t s, const ppd::MapView& m, int64_t n, const double* from, const double* to, uint8_t* valid);
hipError_t launch_rollout(hipStream_t s, const ppd::MapView& m, const RolloutParams& rp, const PrimTable& prims, int64_t nParents, const double* parents,
	uint8_t* valid, double* pose, int32_t* key, double* cost, double* length);
hipError_t launch_rs_solve(hipStream_t s, int64_t n, const double* from, const double* to, double rmin, float rev, float fwd, float sw, int32_t* word,
	double* tuv, float* cost, double* segLength);
/// bits[cell / 32] bit (cell % 32) = dist[cell] >= minSafeRadius
hipError_t launch_valid_bits(hipStream_t s, const float* dist, int64_t cells, float minSafeRadius, uint32_t* bits);
hipError_t launch_nonholo_build(hipStream_t s, const NonHoloDesc& d, double* table);
hipError_t launch_knn(hipStream_t s, int64_t nPoints, const double* pts, int64_t nQueries, const double* q, int k, int32_t* idx, double* d2);

// ---- wavefront (pp_wavefront.hip) -----------------------------------------
struct WavefrontWorkspace;
int64_t wavefront_workspace_bytes(int rows, int cols);
/// workgroups of the wavefront kernel that are resident at once on the current device (occupancy API x CUs)
int wavefront_resident_blocks();
/// one empty dispatch of the wavefront kernel (no goal to take): makes the stream's queue allocate the kernel's scratch now;
/// ctlDev: >= 8 zeroed bytes of device memory (error flag, goal counter)
hipError_t warm_up_wavefront(hipStream_t s, const ppd::MapView& m, int32_t* ctlDev);
/// Pipeline use of the wavefront kernel (pp_pipeline.hpp): entry i of a launch works on field slot slotList[i] (goal pose and output
/// field are indexed by the slot), and every finished slot is appended to the ready ring the search grid consumes.
/// (list and ring entries are slot | generation << kSlotBits: pp_ticket_table.hpp)
struct WavefrontPublish {
	const int32_t* slotList = nullptr;
	unsigned long long* readyTail = nullptr; // entries appended so far (absolute)
	unsigned long long* ready = nullptr;     // ring of (position + 1) << 32 | slot
	unsigned long long readyMask = 0;        // ring size - 1 (a power of two)
	int* goalCounter = nullptr;              // the launch's goal counter when it is not the word behind the error flag (the pipeline keeps
	                                         // the error flag in pinned host memory, where no device atomic should go)
	int* exitCounter = nullptr;              // != nullptr: the last workgroup to leave sets goalCounter (and this word) back to 0 for the stream's next
	                                         // launch -- a 4-byte memset in front of every launch is a kernel that waits tens of ms for a free
	                                         // slot on a GPU filled with long-running workgroups
	// Goals that should not wait for their launch's turn (pp_pipeline.hpp, "urgent"): a ring of stamped slot numbers shared by ALL launches of a
	// pipeline -- a workgroup of any launch in flight serves it before it takes the next goal of its own list -- and one claim word per slot
	// (generation << 1 -> generation << 1 | 1 by whoever builds the slot's field: a slot sits in its launch's list AND, if urgent, in the ring;
	// list and ring entries are slot | generation << kSlotBits, see k_wavefront's hand-out).
	unsigned long long* urgent = nullptr;
	unsigned long long* urgentHead = nullptr; // entries claimed so far (absolute)
	unsigned long long urgentMask = 0;
	int* claimed = nullptr;
	// The tile form of the wavefront (pp_wavefront_tiles.hip) builds the fields when the caller provides its control words; the goals it cannot
	// certify (a tie of its fixed-point equation, a run that does not settle) are rebuilt by the ordered kernel, launched behind it on the same stream.
	const uint64_t* occBits = nullptr; // pp_map::occBits: the occupancy as padded bit rows (word (row + 1) * wpr + col / 64 + 1, bit col % 64; one word of padding on
	                                   // every side, everything outside the map occupied; occ_bits_dims), rebuilt with occ8
	uint32_t* tilesQueue = nullptr;   // optional: tilesQueueWaves regions of wavefront_tiles_queue_words() words, one per wave of a launch (the tile queue in global memory)
	int tilesQueueWaves = 0;
	int* tilesCtl = nullptr;          // >= 8 ints, zero at allocation (the kernels set them back): tile goal counter, exit counter, handed-over count, ordered goal counter, exit counter
	int32_t* tilesFallback = nullptr; // [>= number of goals a launch may take] the handed-over goals
	unsigned long long* tilesStats = nullptr; // optional, 16 words: goals, tile visits, rounds, candidate passes, cells, handed over, wave cycles, ...
	// optional: the ordered kernel's launch over the handed-over goals goes to this stream, behind `fallbackEvent` recorded on the launching
	// stream -- so that the launching stream's NEXT tile launch does not wait for it (a dozen goals of 4096 take the ordered kernel 70-110 ms on
	// a busy chip: a third of a wavefront stream's time when it ran in line).  The caller keeps tilesCtl / tilesFallback / the workspace
	// untouched until that launch has finished.
	hipStream_t fallbackStream = nullptr;
	hipEvent_t fallbackEvent = nullptr;
	// (set by launch_wavefront for the ordered kernel's launch over the handed-over goals)
	const int* nGoalsDev = nullptr;   // the launch's number of goals lives on the device
	int* resetOnExit = nullptr;       // one more word the last workgroup sets back to 0
	bool agentPoseLoads = false;      // read goal poses with agent-scope loads although no claim words are in use
};
/// occupancy bits of the tile form (WavefrontPublish::occBits): words per row and rows of the padded word grid
void occ_bits_dims(int rows, int cols, int& wpr, int& nWordRows);
hipError_t launch_occ_bits(hipStream_t s, const uint8_t* occ8, int rows, int cols, uint64_t* bits);
/// Both occupancy views of a heuristic clearance (include/pp_hip.h, "heuristic clearance") in one pass over dist + occ8: blocked8[cell] =
/// occ8[cell] != 0 || !(dist[cell] >= radius), and the same as padded bit rows in the layout of launch_occ_bits
hipError_t launch_clearance_views(hipStream_t s, const float* dist, const uint8_t* occ8, int rows, int cols, float radius, uint8_t* blocked8, uint64_t* bits);
bool wavefront_tiles_supported(int rows, int cols);
int wavefront_tiles_resident_blocks(int rows, int cols);
/// words of global memory per wave of a launch for the tile queue (0: the map is small enough for the queue to stay in LDS)
size_t wavefront_tiles_queue_words(int rows, int cols);
hipError_t warm_up_wavefront_tiles(hipStream_t s, const ppd::MapView& m, int* ctlDev);
/// What launch_wavefront runs: nGoals wavefronts.  Every pointer is device memory unless it says otherwise; a caller names the fields it sets.
struct WavefrontLaunch {
	int nGoals = 0;
	const int32_t* goalCells = nullptr; // [nGoals] row * cols + col, or -1 (goal outside the map -> field stays +inf)
	const double* goalPoses = nullptr;  // instead: (x, y, theta) triples from which the kernel derives the goal cells itself (goalCells unused)
	float* cost = nullptr;              // [nGoals][rows * cols] row-major (the public a8 entry points), or ...
	bool tiledOut = false;              // ... [nGoals][field_tiled_elems] in the 8 x 8-tiled layout of pp_device.hpp (what the search kernel reads)
	void* workspace = nullptr;          // nSlots x workspaceBytesPerSlot (wavefront_workspace_bytes)
	int64_t workspaceBytesPerSlot = 0;
	int nSlots = 0;
	int32_t* errorFlag = nullptr;       // {overflow flag, next-goal counter (unless pub.goalCounter)}
	bool countersZeroed = false;        // the caller has already cleared errorFlag[0..1] on the stream
	unsigned long long* prof = nullptr; // optional: 20 counters per goal (the profiling build of the ordered kernel, no tile form)
	// optional (nGoals <= 4096): the last workgroup writes the goal indices ordered by decreasing field value at the start pose (x, y, theta
	// triples) to orderOut -- the planner's hand-out order; orderKeys[nGoals] is its scratch, *doneCounter must be 0
	const double* orderStarts = nullptr;
	int32_t* orderOut = nullptr;
	int* doneCounter = nullptr;
	float* orderKeys = nullptr;
	WavefrontPublish pub;
};
hipError_t launch_wavefront_tiles(hipStream_t s, const ppd::MapView& m, const WavefrontLaunch& L);
hipError_t launch_order_by_key(hipStream_t s, int n, const float* keysDev, int32_t* orderOutDev);
/// is the tile form in use (PP_WF_TILES=0 switches it off: every goal through the ordered kernel)
bool wavefront_tiles_enabled();
hipError_t launch_wavefront(hipStream_t s, const ppd::MapView& m, const WavefrontLaunch& L);

} // namespace pph

struct pp_ctx;
struct pp_map;
namespace pph {
struct GvdReference;
void gvd_reference_free(pp_map* map); // pp_gvd.hip
/// occ8 and occBits from occ32 (every writer of the occupancy grid ends here)
int refresh_occupancy_views(pp_map* map, hipStream_t s);
void ctx_release(pp_ctx* ctx); // drops one reference, frees at zero
void map_release(pp_map* map);
/// every writer of pp_map::dist ends here (after the write is enqueued on the map's stream)
void dist_changed(pp_map* map);
} // namespace pph

// Lifetimes: a map keeps its context alive and a planner its map (reference counts), so the handles may be destroyed
// in any order -- e.g. by a garbage collector that finalises a reference cycle in arbitrary order.  pp_*_destroy drops
// the caller's reference; the object goes when the last dependent has gone.  Device memory, events and streams are held by the
// owners above and go with their handle: the *_release functions only count references and wait for the stream.
struct pp_ctx {
	int refs = 1;
	int device = 0;
	hipStream_t stream = nullptr; // not owned: the caller's stream, or `ownStream` below
	pph::Stream ownStream;        // empty when the caller brought a stream
	pph::Event ev0, ev1;
};

struct pp_map {
	int refs = 1;
	pp_ctx* ctx = nullptr;
	pp_map_desc desc {};
	float minSafeRadius = 1.0f, minInterp = 0.1f;
	pph::Dev<int32_t> d2;
	pph::Dev<float> dist;
	pph::Dev<float> pathcost;
	pph::Dev<uint8_t> occ8;
	pph::Dev<uint32_t> validBits; // one bit per cell: dist >= minSafeRadius
	uint64_t distVersion = 0;      // counts the writes of `dist` (pph::dist_changed): a footprint rebuilds its bitmaps when it lags behind
	uint64_t occVersion = 0;       // counts the writes of occ8 / occBits (pph::refresh_occupancy_views): with distVersion the stamp of a ClearanceViews
	pph::Dev<uint64_t> occBits;    // occupancy as padded bit rows (WavefrontPublish::occBits), rebuilt whenever occ8 is
	// map authoring / field construction on the device (pp_gvd.hip)
	pph::Dev<int32_t> occ32;       // occupancy ids as the reference holds them (-1 free)
	pph::Dev<uint32_t> obstLabel[2]; // nearest obstacle cell (row << 16 | col), ping-pong
	pph::Dev<uint32_t> voroLabel[2]; // nearest Voronoi-edge cell
	int obstResult = 0, voroResult = 0;            // which of the two holds the fixed point
	pph::Dev<int32_t> voroD2;
	pph::Dev<uint8_t> voroEdge;
	pph::Dev<int32_t> gvdFlag;
	// reference-order field construction (pp_brushfire_host.hpp): the host brushfire's persistent state and the ordered cell
	// edits (cell, value pairs) made since it last ran.  journalReset: the grid was replaced as a whole before the recorded
	// edits (pp_map_upload_occupancy); journalLost: edits were dropped, the next run re-seeds from the device grid.
	pph::GvdReference* gvdRef = nullptr;
	std::vector<int32_t> journal;
	bool journalReset = false, journalLost = false;
	ppd::MapView view() const;
	size_t cells() const { return (size_t)desc.rows * desc.cols; }
};

/// A vehicle footprint bound to one map (include/pp_hip.h).  It keeps its map alive; its validity bitmaps (one per distinct
/// radius, the map's own layout: pp_map::validBits) follow the map's distance grid through pp_map::distVersion.
struct pp_footprint {
	int refs = 1;
	pp_map* map = nullptr;
	ppd::Footprint fp {};
	int nRadii = 0;
	float radii[ppd::kFootprintMaxDiscs] = {};
	pph::Dev<uint32_t> bits;   // nRadii bitmaps, wordsPer 32-bit words apart
	uint32_t wordsPer = 0;
	uint64_t bitsVersion = 0;  // the map's distVersion the bitmaps were built from
	bool bitsBuilt = false;
};
namespace pph {
/// The occupancy views of a heuristic clearance (include/pp_hip.h, "heuristic clearance"): what the wavefront kernels read in place of
/// pp_map::occ8 / pp_map::occBits when the radius is > 0.  Owned by whoever launches the fields with it (a planner, a pipeline's planner, one
/// call of pp_obstacle_heuristic_clearance), so two owners with different radii on one map never share a buffer.  Built lazily on the map's
/// stream and stamped with the map's distVersion and occVersion: a writer of either grid makes them stale (the model: footprint_prepare).
struct ClearanceViews {
	float radius = 0.0f; // 0: off, the launch takes the map's own views
	Dev<uint8_t> blocked8;
	Dev<uint64_t> bits;
	float builtRadius = 0.0f;
	uint64_t distVersion = 0, occVersion = 0;
	bool built = false;
	bool stale(const pp_map* map) const { return !built || builtRadius != radius || distVersion != map->distVersion || occVersion != map->occVersion; }
};
/// PP_ERR_INVALID with a message unless radius is finite and >= 0
int clearance_check_radius(float radius);
/// radius 0: nothing.  Otherwise checks that the map has a distance and an occupancy grid (PP_ERR_INVALID with a message) and brings the views up
/// to date on the map's stream; *rebuilt (optional) tells whether a kernel was enqueued.
int clearance_prepare(pp_map* map, ClearanceViews& cv, bool* rebuilt);
/// Checks that `fp` belongs to `map` and that the map has a distance grid (PP_ERR_INVALID with a message otherwise);
/// needBits: also brings the footprint's bitmaps up to date with the map's distance grid, on the map's stream.
int footprint_prepare(pp_map* map, pp_footprint* fp, bool needBits);
void footprint_release(pp_footprint* fp); // drops one reference, frees at zero
hipError_t launch_check_states_footprint(hipStream_t s, const ppd::MapView& m, const pp_footprint* fp, int64_t n, const double* poses, uint8_t* valid, float* clearance);
} // namespace pph

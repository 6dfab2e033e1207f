// HybridAStarPipeline::Stamp (pp_pipeline_stamp) through the C++ mirror: plans held by ticket are stamped on the device into the occupancy grid
// of a SECOND map, and the grid is compared with the one-query mirror's path objects of the same plans (HybridAStar::GetGraphSearchPath:
// PathConstantSteer arcs and the PathReedsShepp connection) sampled every `spacing` and rasterised here, disc by disc, by the rule of
// include/pp_hip.h.  A cell whose centre lies within 1e-7 m of a disc's rim for some sample is left out (host and device poses differ around
// 1e-12 m); every other cell must match, value included.  Then the fields of the stamped map are rebuilt and a pose on a stamped cell is
// invalid; a windowed stamp into the pipeline's own map; a ticket that is not held throws.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <map>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

using Stamped = HybridAStarPipeline::Stamped;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

struct Plan {
	Status status = Status::Failure;
	std::vector<Pose2d> nodes;
	std::vector<Ref<PathNonHolonomicSE2Base>> edges;
};

constexpr double kBand = 1e-7;

/// what the rule says about every cell of `map` for the plans' samples inside [from, to]: in[cell] = the largest value of a plan that decidedly covers
/// it (-1: none), band[cell] = some sample's rim passes within kBand of its centre
struct Expected {
	std::vector<int> in;
	std::vector<char> band;
	int samples = 0;
};
void rasterise(Expected& x, OccupancyMap& map, const Pose2d& pose, double R, int value)
{
	const int rows = map.Rows(), cols = map.Columns();
	const Point2d origin = map.GridCellToWorldPosition({ 0, 0 });
	const double res = (double)map.resolution;
	const int r0 = (int)std::floor((pose.x() - R - origin.x()) / res) - 1, r1 = (int)std::floor((pose.x() + R - origin.x()) / res) + 1;
	const int c0 = (int)std::floor((pose.y() - R - origin.y()) / res) - 1, c1 = (int)std::floor((pose.y() + R - origin.y()) / res) + 1;
	for (int r = std::max(r0, 0); r <= std::min(r1, rows - 1); r++)
		for (int c = std::max(c0, 0); c <= std::min(c1, cols - 1); c++) {
			const double dx = origin.x() + (r + 0.5) * res - pose.x(), dy = origin.y() + (c + 0.5) * res - pose.y();
			const double d = std::sqrt(dx * dx + dy * dy);
			const size_t i = (size_t)r * cols + c;
			if (d <= R - kBand)
				x.in[i] = std::max(x.in[i], value);
			else if (d <= R + kBand)
				x.band[i] = 1;
		}
}
int expect(Expected& x, OccupancyMap& map, const Plan& p, double R, double spacing, double from, double to, int value)
{
	int samples = 0;
	if (p.status != Status::Success || p.nodes.empty())
		return 0;
	if (p.edges.empty()) {
		if (0.0 >= from && 0.0 <= to) {
			rasterise(x, map, p.nodes[0], R, value);
			samples++;
		}
		return samples;
	}
	double before = 0.0;
	for (const auto& e : p.edges) {
		const double L = e->GetLength();
		const int n = L > 0 ? (int)std::ceil(L / spacing) : 0;
		for (int k = 0; k <= n; k++) {
			const double ratio = n ? (double)k / (double)n : 0.0, s = before + ratio * L;
			if (s >= from && s <= to) {
				rasterise(x, map, e->Interpolate(ratio), R, value);
				samples++;
			}
		}
		before += L;
	}
	return samples;
}

} // namespace

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f), reserve = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map), reserveValidator = makeRef<StateValidatorOccupancyMap>(space, reserve);
	for (const auto& wl : walls) {
		assert(map->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
		assert(reserve->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
	}
	GVD(map).Update();
	GVD(reserve).Update();

	const int n = 12, maxNodes = 32768;
	HybridAStar::SearchParameters params;
	HybridAStar one(params, 1, maxNodes);
	HybridAStarPipeline pipe(params, 16, maxNodes, 16);
	uint64_t lcg = 4242;
	auto uniform = [&](double lo, double hi) {
		lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
		return lo + (hi - lo) * (double)(lcg >> 11) / 9007199254740992.0;
	};
	auto validPose = [&]() {
		for (int tries = 0; tries < 100000; tries++) {
			const Pose2d p(uniform(-9.0, 9.0), uniform(-9.0, 9.0), uniform(-M_PI, M_PI));
			if (validator->IsStateValid(p))
				return p;
		}
		assert(!"no valid pose in 100000 draws");
		return Pose2d();
	};
	std::vector<Pose2d> starts, goals;
	std::vector<uint64_t> seeds;
	for (int i = 0; i < n; i++) {
		starts.push_back(validPose());
		goals.push_back(validPose());
		seeds.push_back(9100 + (uint64_t)i);
	}
	assert(one.Initialize(validator));
	std::vector<Plan> plans((size_t)n);
	for (int i = 0; i < n; i++) {
		one.SetInitState(starts[(size_t)i]);
		one.SetGoalState(goals[(size_t)i]);
		one.SetSeed(seeds[(size_t)i]);
		Plan& p = plans[(size_t)i];
		p.status = one.SearchPath();
		if (p.status == Status::Success) {
			p.nodes = one.GetGraphSearchNodes();
			p.edges = one.GetGraphSearchPath();
			assert(p.edges.size() + 1 == p.nodes.size());
		}
	}
	assert(pipe.Initialize(validator));
	std::vector<uint64_t> tickets;
	assert(pipe.Submit(starts, goals, seeds, &tickets) == n);
	std::map<uint64_t, int> indexOf;
	for (int i = 0; i < n; i++)
		indexOf[tickets[(size_t)i]] = i;
	std::vector<uint64_t> held;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<HybridAStarPipeline::Result> out;
	while ((int)held.size() < n) {
		pipe.Poll(out, 4096, true);
		for (const auto& r : out) {
			assert(r.status == plans[(size_t)indexOf.at(r.ticket)].status);
			held.push_back(r.ticket);
		}
		if (out.empty())
			std::this_thread::sleep_for(std::chrono::microseconds(200));
		assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
	}
	// ---- whole plans into the second map, values 10 + query index, over the walls' own ids
	const int rows = reserve->Rows(), cols = reserve->Columns();
	const size_t cells = (size_t)rows * cols;
	std::vector<int> before(cells);
	for (size_t i = 0; i < cells; i++)
		before[i] = reserve->GetOccupancyValue((int)(i / cols), (int)(i % cols));
	const double spacing = 0.13, R = (double)validator->minSafeRadius + (double)0.05f;
	std::vector<int32_t> values;
	for (uint64_t t : held)
		values.push_back(10 + indexOf.at(t));
	const std::vector<Stamped> got = pipe.Stamp(held, reserveValidator, spacing, 0.05f, values);
	assert(got.size() == held.size());
	Expected x;
	x.in.assign(cells, -1);
	x.band.assign(cells, 0);
	int solved = 0;
	for (size_t k = 0; k < held.size(); k++) {
		const Plan& p = plans[(size_t)indexOf.at(held[k])];
		const int samples = expect(x, *reserve, p, R, spacing, -HUGE_VAL, HUGE_VAL, values[k]);
		double length = 0.0;
		for (const auto& e : p.edges)
			length += e->GetLength();
		if (p.status != Status::Success) {
			assert(got[k].status == Stamped::Status::NoPlan && got[k].numSamples == 0 && got[k].Empty());
			continue;
		}
		solved++;
		assert(got[k].status == Stamped::Status::Stamped && got[k].numSamples == samples && !got[k].Empty());
		assert(std::fabs(got[k].length - length) <= 1e-9);
	}
	size_t stamped = 0, undecided = 0;
	int sampleRow = -1, sampleCol = -1;
	for (size_t i = 0; i < cells; i++) {
		const int now = reserve->GetOccupancyValue((int)(i / cols), (int)(i % cols));
		if (x.in[i] >= 0)
			stamped++;
		if (x.band[i]) {
			undecided++;
			continue;
		}
		const int want = std::max(before[i], x.in[i]);
		if (now != want) {
			std::printf("cell (%d, %d): the grid holds %d, the path objects say %d (before: %d)\n", (int)(i / cols), (int)(i % cols), now, want, before[i]);
			assert(false);
		}
		if (x.in[i] >= 0 && sampleRow < 0) {
			sampleRow = (int)(i / cols);
			sampleCol = (int)(i % cols);
		}
	}
	std::printf("%d plans of %d queries stamped: %zu cells, %zu left out in the 1e-7 m band\n", solved, n, stamped, undecided);
	assert(solved >= 8 && stamped > 1000 && undecided * 1000 <= stamped);
	// ---- the fields follow when they are rebuilt: a pose on a stamped cell's centre is invalid then
	GVD(reserve).Update();
	const Point2d corner = reserve->GridCellToWorldPosition({ sampleRow, sampleCol });
	assert(!reserveValidator->IsStateValid(Pose2d(corner.x() + 0.05, corner.y() + 0.05, 0.0)));
	// ---- a window of the first 2 m into the pipeline's own map (nothing is in flight)
	std::vector<double> from(held.size(), 0.0), to(held.size(), 2.0);
	const std::vector<Stamped> own = pipe.Stamp(held, nullptr, spacing, 0.0f, {}, from, to);
	Expected y;
	y.in.assign(cells, -1);
	y.band.assign(cells, 0);
	for (size_t k = 0; k < held.size(); k++) {
		const Plan& p = plans[(size_t)indexOf.at(held[k])];
		assert(own[k].numSamples == expect(y, *map, p, (double)validator->minSafeRadius, spacing, 0.0, 2.0, 0));
		assert(own[k].length == got[k].length);
	}
	for (size_t i = 0; i < cells; i++)
		if (!y.band[i] && y.in[i] >= 0)
			assert(map->GetOccupancyValue((int)(i / cols), (int)(i % cols)) >= 0);
	// ---- a ticket that is not held throws, and the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Stamp({ held[0] }, reserveValidator, spacing);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	assert(pipe.Stamp({ held[1] }, reserveValidator, spacing).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline stamp: Stamp(tickets) == the path objects sampled and rasterised one by one, on a second map and windowed on the own map\n");
	return 0;
}

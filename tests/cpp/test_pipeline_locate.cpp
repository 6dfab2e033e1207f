// HybridAStarPipeline::Locate (pp_pipeline_locate) through the C++ mirror: vehicles are placed beside plans held by ticket and located on the device,
// and every answer is compared with the one-query mirror's path objects of the same plan (HybridAStar::GetGraphSearchPath: PathConstantSteer arcs and
// the PathReedsShepp connection) searched here, candidate by candidate, by the two stages of include/pp_hip.h.  Host and device poses differ around
// 1e-12 m, so the comparison is on the cost: the cost of the device's (edge, ratio), evaluated with the path objects, is within 1e-9 m^2 of the least
// cost over all candidates, and the record's pose and errors are those of that point.  Then a window, a one-pose plan, a failed query and a ticket that
// is not held.  Needs a GPU.
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

using Located = HybridAStarPipeline::Located;

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

constexpr double kTwoPi = 6.283185307179586, kEps = 1e-9;

double cost(const Pose2d& v, const Pose2d& p, double w)
{
	const double ex = v.x() - p.x(), ey = v.y() - p.y(), a = v.theta - p.theta, d = a - kTwoPi * std::rint(a / kTwoPi);
	return (ex * ex + ey * ey) + (w * d) * (w * d);
}

/// the least cost over the candidates of both stages, by the path objects (the plan has edges); `samples`: stage-1 samples inside the window
double least_cost(const Plan& p, const Pose2d& v, double spacing, double w, double from, double to, int& samples)
{
	std::vector<double> S;
	double before = 0.0, best = HUGE_VAL, s1 = 0.0;
	samples = 0;
	for (const auto& e : p.edges) {
		const double L = e->GetLength();
		const int n = L > 0 ? (int)std::ceil(L / spacing) : 0;
		S.push_back(before);
		for (int k = 0; k <= n; k++) {
			const double ratio = n ? (double)k / (double)n : 0.0, s = before + ratio * L;
			if (s >= from && s <= to) {
				samples++;
				const double c = cost(v, e->Interpolate(ratio), w);
				if (c < best) {
					best = c;
					s1 = s;
				}
			}
		}
		before += L;
	}
	if (samples == 0)
		return best;
	const double delta = spacing / 32, length = before;
	const long long i0 = (long long)std::floor(s1 / delta);
	for (long long i = i0 - 32; i <= i0 + 33; i++) {
		const double u = (double)i * delta;
		if (!(u >= 0.0 && u <= length && u >= from && u <= to))
			continue;
		size_t e = 0;
		while (e + 1 < S.size() && S[e + 1] <= u)
			e++;
		const double L = p.edges[e]->GetLength();
		best = std::min(best, cost(v, p.edges[e]->Interpolate(L > 0 ? std::min((u - S[e]) / L, 1.0) : 0.0), w));
	}
	return best;
}

void check(const Plan& p, const Pose2d& v, const Located& got, double spacing, double w, double from = -HUGE_VAL, double to = HUGE_VAL)
{
	int samples = 0;
	const double best = least_cost(p, v, spacing, w, from, to, samples);
	double length = 0.0;
	for (const auto& e : p.edges)
		length += e->GetLength();
	assert(got.numSamples == samples && std::fabs(got.length - length) <= 1e-9);
	if (samples == 0) {
		assert(got.status == Located::Status::NoSampleInWindow && got.edge == 0 && got.s == 0.0);
		return;
	}
	assert(got.status == Located::Status::Located && got.edge >= 1 && got.edge <= (int)p.edges.size() && got.ratio >= 0.0 && got.ratio <= 1.0);
	assert(got.s >= from && got.s <= to && got.s >= 0.0 && got.s <= length);
	const auto& e = p.edges[(size_t)got.edge - 1];
	const Pose2d at = e->Interpolate(got.ratio);
	const double c = cost(v, at, w);
	if (!(std::fabs(c - best) <= kEps)) {
		std::printf("edge %d ratio %.17g: cost %.17g by the path object, the least over the candidates is %.17g\n", got.edge, got.ratio, c, best);
		assert(false);
	}
	assert(std::fabs(got.pose.x() - at.x()) <= 1e-9 && std::fabs(got.pose.y() - at.y()) <= 1e-9 && std::fabs(std::remainder(got.pose.theta - at.theta, kTwoPi)) <= 1e-9);
	const double ex = v.x() - at.x(), ey = v.y() - at.y();
	assert(std::fabs(got.distance - std::sqrt(ex * ex + ey * ey)) <= 1e-9);
	assert(std::fabs(got.along - (std::cos(at.theta) * ex + std::sin(at.theta) * ey)) <= 1e-9);
	assert(std::fabs(got.lateral - (std::cos(at.theta) * ey - std::sin(at.theta) * ex)) <= 1e-9);
	assert(std::fabs(std::remainder(got.headingError - (v.theta - at.theta), kTwoPi)) <= 1e-9 && std::fabs(got.headingError) <= M_PI + 1e-12);
	assert(got.direction == (e->GetDirection(got.ratio) == Direction::Backward ? -1 : 1));
}

} // namespace

int main()
{
	std::array<Pose2d, 2> bounds = { Pose2d(-10, -10, -M_PI), Pose2d(10, 10, M_PI) };
	Ref<StateSpaceSE2> space = makeRef<StateSpaceSE2>(bounds);
	const double walls[2][5] = { { 8.0, 0.6, -5.0, 1.0, 0.0 }, { 8.0, 0.6, 5.5, -2.0, 0.3 } };
	Ref<ObstacleListOccupancyMap> map = makeRef<ObstacleListOccupancyMap>(0.1f);
	Ref<StateValidatorOccupancyMap> validator = makeRef<StateValidatorOccupancyMap>(space, map);
	for (const auto& wl : walls)
		assert(map->AddObstacle(wall(wl[0], wl[1], wl[2], wl[3], wl[4])));
	GVD(map).Update();

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
		goals.push_back(i == n - 1 ? starts.back() : validPose()); // the last query: start == goal, a one-pose plan
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
	assert(plans[(size_t)n - 1].status == Status::Success && plans[(size_t)n - 1].edges.empty());
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
	// ---- three rounds of vehicles beside their plans: a point of the plan, pushed up to 0.4 m sideways and turned by up to 0.3 rad
	const double spacing = 0.13;
	int located = 0;
	for (int round = 0; round < 3; round++) {
		const double w = round == 1 ? 1.5 : 0.0;
		std::vector<Pose2d> vehicles;
		for (uint64_t t : held) {
			const Plan& p = plans[(size_t)indexOf.at(t)];
			if (p.edges.empty()) {
				vehicles.push_back(p.status == Status::Success ? Pose2d(p.nodes[0].x() + 0.2, p.nodes[0].y() - 0.1, p.nodes[0].theta) : Pose2d(1.0, 2.0, 0.5));
				continue;
			}
			const auto& e = p.edges[(size_t)(uniform(0.0, 1.0) * (double)p.edges.size()) % p.edges.size()];
			const Pose2d at = e->Interpolate(uniform(0.0, 1.0));
			const double side = uniform(-0.4, 0.4);
			vehicles.push_back(Pose2d(at.x() - side * std::sin(at.theta), at.y() + side * std::cos(at.theta), at.theta + uniform(-0.3, 0.3)));
		}
		const std::vector<Located> got = pipe.Locate(held, vehicles, spacing, w);
		assert(got.size() == held.size());
		for (size_t k = 0; k < held.size(); k++) {
			const Plan& p = plans[(size_t)indexOf.at(held[k])];
			if (p.status != Status::Success) {
				assert(got[k].status == Located::Status::NoPlan && got[k].numSamples == 0 && got[k].length == 0.0 && got[k].s == 0.0);
				continue;
			}
			if (p.edges.empty()) {
				assert(got[k].status == Located::Status::Located && got[k].edge == 0 && got[k].numSamples == 1 && got[k].s == 0.0 && got[k].length == 0.0);
				assert(std::fabs(got[k].distance - std::sqrt(0.05)) <= 1e-12 && got[k].pose.x() == p.nodes[0].x() && got[k].pose.y() == p.nodes[0].y());
				continue;
			}
			check(p, vehicles[k], got[k], spacing, w);
			assert(got[k].distance <= 0.65); // (cost <= 0.4^2 + (1.5 * 0.3)^2 at the point the vehicle was pushed from, and a lattice point lies within 2.1 mm of it)
			located++;
		}
		// ---- the same vehicles, the plan's second half only, then a window behind the plan
		if (round == 2) {
			std::vector<double> from, to, beyond;
			for (size_t k = 0; k < held.size(); k++) {
				from.push_back(0.5 * got[k].length);
				to.push_back(got[k].length);
				beyond.push_back(got[k].length + 1.0);
			}
			const std::vector<Located> half = pipe.Locate(held, vehicles, spacing, w, from, to), none = pipe.Locate(held, vehicles, spacing, w, beyond);
			for (size_t k = 0; k < held.size(); k++) {
				const Plan& p = plans[(size_t)indexOf.at(held[k])];
				if (p.status != Status::Success || p.edges.empty())
					continue;
				check(p, vehicles[k], half[k], spacing, w, from[k], to[k]);
				check(p, vehicles[k], none[k], spacing, w, beyond[k], HUGE_VAL);
				assert(none[k].status == Located::Status::NoSampleInWindow);
			}
		}
	}
	std::printf("%d vehicles located on the plans of %d queries\n", located, n);
	assert(located >= 24);
	// ---- a ticket that is not held throws, and the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Locate({ held[0] }, { Pose2d(0, 0, 0) }, spacing);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	assert(pipe.Locate({ held[1] }, { Pose2d(0, 0, 0) }, spacing).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline locate: Locate(tickets, poses) == the least cost over the path objects' candidates, whole plans and windowed\n");
	return 0;
}

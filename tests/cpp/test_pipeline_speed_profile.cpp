// HybridAStarPipeline::SpeedProfile (pp_pipeline_speed_profile) through the C++ mirror: plans are held by ticket and profiled on the device, and every
// answer is compared with a plain sequential sweep made here over the one-query mirror's path objects of the same plan (HybridAStar::GetGraphSearchPath:
// PathConstantSteer arcs and the PathReedsShepp connection): the samples of include/pp_hip.h's schedule, a cap per sample from the object's direction
// and curvature, a forward pass limited by a_acc, a backward pass limited by a_dec, the times summed in order.  The sweep and the device's closed form
// round differently (the closed form's keys at the magnitude of 2 a s), so speeds are compared within 1e-9 m/s and times within 1e-9 relative.  Then a
// window with end speeds, the sample limit, a one-pose plan, a failed query and a ticket that is not held.  Needs a GPU.
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

using Profiled = HybridAStarPipeline::SpeedProfiled;
using Limits = HybridAStarPipeline::SpeedLimits;

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

/// |curvature| of a path object at `ratio`: the arc's, or that of the Reeds-Shepp motion GetDirection reads
double curvature(const Ref<PathNonHolonomicSE2Base>& e, double ratio)
{
	if (const auto* arc = dynamic_cast<const PathConstantSteer*>(e.get()))
		return std::fabs(arc->GetModel()->Curvature(arc->GetSteeringAngle()));
	const auto* rsp = dynamic_cast<const PathReedsShepp*>(e.get());
	assert(rsp);
	const pp_rs_path& r = rsp->Record();
	double len = 0.0;
	for (int i = 0; i < 5; i++) {
		if (!std::isfinite(r.motion_length[i]) || r.direction[i] == 2)
			break;
		len += r.motion_length[i] * r.min_turning_radius;
		if (ratio * r.length <= len)
			return r.steer[i] == 1 ? 0.0 : 1.0 / r.min_turning_radius;
	}
	return 0.0;
}

struct Sweep {
	std::vector<double> s, v, t;
	int cusps = 0;
};

Sweep sweep(const Plan& p, double spacing, const Limits& L, double from, double to, double vStart, double vEnd)
{
	Sweep out;
	std::vector<double> w;
	std::vector<int> cusp;
	int previous = 0;
	double before = 0.0;
	auto sample = [&](double s, int own, double kappa) {
		if (!(s >= from && s <= to))
			return;
		const int dir = own == 0 ? previous : own;
		const bool stop = !out.s.empty() && dir != 0 && previous != 0 && dir != previous;
		double c = dir == 1 ? L.vMaxForward : L.vMaxReverse;
		if (kappa > 0.0)
			c = std::min(c, std::sqrt(L.aLat / kappa));
		out.s.push_back(s);
		w.push_back(stop ? 0.0 : c * c);
		cusp.push_back(stop);
		out.cusps += stop;
		previous = dir;
	};
	if (p.edges.empty())
		sample(0.0, 0, 0.0);
	for (const auto& e : p.edges) {
		const double len = e->GetLength();
		const int n = len > 0 ? (int)std::ceil(len / spacing) : 0;
		for (int k = 0; k <= n; k++) {
			const double ratio = n ? (double)k / (double)n : 0.0;
			const Direction d = e->GetDirection(ratio);
			sample(before + ratio * len, d == Direction::Forward ? 1 : (d == Direction::Backward ? -1 : 0), curvature(e, ratio));
		}
		before += len;
	}
	const size_t n = out.s.size();
	if (n == 0)
		return out;
	w[0] = std::min(w[0], vStart * vStart);
	w[n - 1] = std::min(w[n - 1], vEnd * vEnd);
	for (size_t j = 1; j < n; j++)
		w[j] = std::min(w[j], w[j - 1] + 2.0 * L.aAcc * (out.s[j] - out.s[j - 1]));
	for (size_t j = n - 1; j-- > 0;)
		w[j] = std::min(w[j], w[j + 1] + 2.0 * L.aDec * (out.s[j + 1] - out.s[j]));
	out.t.assign(n, 0.0);
	for (size_t j = 0; j < n; j++)
		out.v.push_back(std::sqrt(w[j]));
	for (size_t j = 0; j + 1 < n; j++) {
		const double ds = out.s[j + 1] - out.s[j], both = out.v[j] + out.v[j + 1];
		double dt = 0.0;
		if (ds != 0.0 && both > 0.0)
			dt = 2.0 * ds / both;
		else if (ds != 0.0) {
			const double x = ds * L.aDec / (L.aAcc + L.aDec);
			dt = std::sqrt(2.0 * x / L.aAcc) + std::sqrt(2.0 * (ds - x) / L.aDec);
		}
		out.t[j + 1] = out.t[j] + dt + (cusp[j + 1] ? L.dwell : 0.0);
	}
	return out;
}

void check(const Plan& p, const Profiled& got, double spacing, const Limits& L, double from = -HUGE_VAL, double to = HUGE_VAL, double vStart = 0.0, double vEnd = 0.0)
{
	const Sweep want = sweep(p, spacing, L, from, to, vStart, vEnd);
	double length = 0.0;
	for (const auto& e : p.edges)
		length += e->GetLength();
	assert(got.numSamples == (int)want.s.size() && std::fabs(got.length - length) <= 1e-9);
	if (want.s.empty()) {
		assert(got.status == Profiled::Status::NoSampleInWindow && got.s.empty() && got.duration == 0.0);
		return;
	}
	assert(got.status == Profiled::Status::Profiled && got.numCusps == want.cusps && got.s.size() == want.s.size() && got.v.size() == want.s.size() && got.t.size() == want.s.size());
	double peak = 0.0;
	for (size_t j = 0; j < want.s.size(); j++) {
		if (!(std::fabs(got.s[j] - want.s[j]) <= 1e-9 && std::fabs(got.v[j] - want.v[j]) <= 1e-9 && std::fabs(got.t[j] - want.t[j]) <= 1e-9 * std::max(want.t[j], 1e-3))) {
			std::printf("sample %zu: s %.17g v %.17g t %.17g on the device, %.17g %.17g %.17g by the sweep\n", j, got.s[j], got.v[j], got.t[j], want.s[j], want.v[j], want.t[j]);
			assert(false);
		}
		peak = std::max(peak, got.v[j]);
	}
	assert(got.sFirst == got.s.front() && got.sLast == got.s.back() && got.duration == got.t.back() && got.vPeak == peak && got.t.front() == 0.0);
	assert(got.v.front() <= vStart && got.v.back() <= vEnd);
	assert(std::isinf(got.minClearance) && got.sMinClearance == 0.0); // (no clearance term)
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
	// ---- whole plans from rest to rest, under two sets of limits
	Limits slow;
	slow.vMaxForward = 3.0;
	slow.vMaxReverse = 1.0;
	slow.aAcc = 0.7;
	slow.aDec = 1.9;
	slow.aLat = 0.8;
	slow.dwell = 2.0;
	int profiled = 0, cusps = 0;
	for (const auto& [spacing, L] : { std::pair<double, Limits>(0.13, Limits()), std::pair<double, Limits>(0.31, slow) }) {
		const std::vector<Profiled> got = pipe.SpeedProfile(held, spacing, L);
		assert(got.size() == held.size());
		for (size_t k = 0; k < held.size(); k++) {
			const Plan& p = plans[(size_t)indexOf.at(held[k])];
			if (p.status != Status::Success) {
				assert(got[k].status == Profiled::Status::NoPlan && got[k].numSamples == 0 && got[k].length == 0.0 && got[k].s.empty());
				continue;
			}
			check(p, got[k], spacing, L);
			if (p.edges.empty()) {
				assert(got[k].numSamples == 1 && got[k].s[0] == 0.0 && got[k].v[0] == 0.0 && got[k].duration == 0.0);
				continue;
			}
			assert(got[k].v.front() == 0.0 && got[k].v.back() == 0.0 && got[k].duration > 0.0);
			profiled++;
			cusps += got[k].numCusps;
		}
	}
	// ---- the second half of every plan with end speeds, a window behind the plan, and one sample too few
	{
		const double spacing = 0.13;
		const Limits L;
		const std::vector<Profiled> whole = pipe.SpeedProfile(held, spacing, L);
		std::vector<double> from, to, beyond, vs, ve;
		for (size_t k = 0; k < held.size(); k++) {
			from.push_back(0.5 * whole[k].length);
			to.push_back(whole[k].length);
			beyond.push_back(whole[k].length + 1.0);
			vs.push_back(2.5);
			ve.push_back(1.0);
		}
		const std::vector<Profiled> half = pipe.SpeedProfile(held, spacing, L, 2048, from, to, vs, ve), none = pipe.SpeedProfile(held, spacing, L, 2048, beyond);
		for (size_t k = 0; k < held.size(); k++) {
			const Plan& p = plans[(size_t)indexOf.at(held[k])];
			if (p.status != Status::Success || p.edges.empty())
				continue;
			check(p, half[k], spacing, L, from[k], to[k], vs[k], ve[k]);
			check(p, none[k], spacing, L, beyond[k], HUGE_VAL);
			assert(none[k].status == Profiled::Status::NoSampleInWindow);
			const std::vector<Profiled> few = pipe.SpeedProfile({ held[k] }, spacing, L, whole[k].numSamples - 1);
			assert(few[0].status == Profiled::Status::TooManySamples && few[0].numSamples == whole[k].numSamples && few[0].s.empty() && few[0].duration == 0.0);
		}
	}
	std::printf("%d profiles of the plans of %d queries, %d cusp stops\n", profiled, n, cusps);
	assert(profiled >= 16);
	// ---- a ticket that is not held throws, and the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.SpeedProfile({ held[0] }, 0.1);
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	assert(pipe.SpeedProfile({ held[1] }, 0.1).size() == 1);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline speed profile: SpeedProfile(tickets) == the sweep over the plan's samples, whole plans and windowed\n");
	return 0;
}

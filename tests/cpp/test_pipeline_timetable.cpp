// HybridAStarPipeline::Timetable (pp_pipeline_timetable) through the C++ mirror: plans are held by ticket and profiled on the device (SpeedProfile,
// which also downloads the rows), and the look-ups and the stop lists are compared with a plain sequential loop made here over those rows -- linear
// searches and the definition of include/pp_hip.h written out in its order, without the rule header the kernel compiles.  Everything taken from the
// rows (status, row, s, t, v, a, the stops, the distances to the next stop) is compared EXACTLY (the program is built without contraction); the pose is
// compared with the pose Conflicts returns for the same time since the start (the same path readers on the same arc length: exactly).  Then: max_stops
// of 0 and 1, no values, a ticket that is not held, a held one without a profile.  Needs a GPU.
#undef NDEBUG
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../../pathplanning_amd/host/map_authoring.hpp"

using namespace Planner;

namespace {

using Limits = HybridAStarPipeline::SpeedLimits;
using Horizon = HybridAStarPipeline::ConflictHorizon;
using Profiled = HybridAStarPipeline::SpeedProfiled;
using Timetabled = HybridAStarPipeline::Timetabled;

Ref<Obstacle> wall(double dx, double dy, double x, double y, double theta)
{
	Ref<Obstacle> o = makeRef<Obstacle>();
	o->SetShape(makeRef<RectangleShape>(dx, dy));
	o->SetPose(Pose2d(x, y, theta));
	return o;
}

bool sameBits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

double stepTime(double ds, double v0, double v1, double aAcc, double aDec)
{
	if (ds == 0.0)
		return 0.0;
	if (v0 + v1 > 0.0)
		return (2.0 * ds) / (v0 + v1);
	const double x = ds * aDec / (aAcc + aDec);
	return std::sqrt(2.0 * x / aAcc) + std::sqrt(2.0 * (ds - x) / aDec);
}

/// the stops of a profile, by the definition
std::vector<Timetabled::Stop> stopsOf(const Profiled& p, const Limits& L)
{
	std::vector<Timetabled::Stop> out;
	for (int j = 0; j < p.numSamples; j++)
		if (p.v[j] == 0.0) {
			Timetabled::Stop st;
			st.row = j;
			st.s = p.s[j];
			st.tDepart = p.t[j];
			st.tArrive = j == 0 ? 0.0 : p.t[j - 1] + stepTime(p.s[j] - p.s[j - 1], p.v[j - 1], p.v[j], L.aAcc, L.aDec);
			out.push_back(st);
		}
	return out;
}

/// one look-up, by the definition (pose, edge, ratio, direction and kappa are not formed here)
Timetabled::LookUp lookUp(const Profiled& p, const Limits& L, bool byTime, double value, const std::vector<Timetabled::Stop>& listed)
{
	using Status = Timetabled::LookUp::Status;
	const int N = p.numSamples;
	const double aAcc = L.aAcc, aDec = L.aDec;
	Timetabled::LookUp u;
	u.status = Status::Inside;
	int j = 0;
	if (byTime) {
		if (value < 0.0) {
			u.status = Status::Before;
			value = 0.0;
		}
		if (value > p.t[N - 1]) {
			u.status = Status::Behind;
			value = p.t[N - 1];
		}
		for (int k = 0; k < N; k++)
			if (p.t[k] <= value)
				j = k;
		u.t = value;
		if (j == N - 1 || p.s[j + 1] - p.s[j] == 0.0) {
			u.s = p.s[j];
			u.v = p.v[j];
		} else {
			const double s0 = p.s[j], s1 = p.s[j + 1], v0 = p.v[j], v1 = p.v[j + 1], ds = s1 - s0, delta = value - p.t[j], m = stepTime(ds, v0, v1, aAcc, aDec);
			if (delta >= m) {
				u.s = s1;
				u.v = v1;
			} else {
				double s;
				if (v0 + v1 > 0.0) {
					u.a = (v1 - v0) / m;
					u.v = v0 + u.a * delta;
					s = s0 + (v0 + (0.5 * u.a) * delta) * delta;
				} else {
					const double x = ds * aDec / (aAcc + aDec), ta = std::sqrt(2.0 * x / aAcc);
					if (delta <= ta) {
						u.v = aAcc * delta;
						u.a = aAcc;
						s = s0 + (0.5 * aAcc) * delta * delta;
					} else {
						const double r = m - delta;
						u.v = aDec * r;
						u.a = -aDec;
						s = s1 - (0.5 * aDec) * r * r;
					}
				}
				u.s = s < s0 ? s0 : (s > s1 ? s1 : s);
			}
		}
	} else {
		if (value < p.s[0]) {
			u.status = Status::Before;
			value = p.s[0];
		}
		if (value > p.s[N - 1]) {
			u.status = Status::Behind;
			value = p.s[N - 1];
		}
		for (int k = 0; k < N; k++)
			if (p.s[k] <= value)
				j = k;
		u.s = value;
		if (j == N - 1) {
			u.t = p.t[j];
			u.v = p.v[j];
		} else {
			const double s0 = p.s[j], s1 = p.s[j + 1], v0 = p.v[j], v1 = p.v[j + 1], ds = s1 - s0, sigma = value - s0, m = stepTime(ds, v0, v1, aAcc, aDec);
			double delta;
			if (v0 + v1 > 0.0) {
				u.a = (v1 - v0) / m;
				if (sigma == 0.0) {
					delta = 0.0;
					u.v = v0;
				} else {
					double w = v0 * v0 + (2.0 * u.a) * sigma;
					if (!(w > 0.0))
						w = 0.0;
					u.v = std::sqrt(w);
					delta = (2.0 * sigma) / (v0 + u.v);
				}
			} else {
				const double x = ds * aDec / (aAcc + aDec);
				if (sigma == 0.0) {
					delta = 0.0;
					u.v = v0;
					u.a = aAcc;
				} else if (sigma <= x) {
					delta = std::sqrt(2.0 * sigma / aAcc);
					u.v = aAcc * delta;
					u.a = aAcc;
				} else {
					const double r = std::sqrt(2.0 * (ds - sigma) / aDec);
					delta = m - r;
					u.v = aDec * r;
					u.a = -aDec;
				}
			}
			if (!(delta >= 0.0))
				delta = 0.0;
			if (delta > m)
				delta = m;
			u.t = p.t[j] + delta;
		}
	}
	u.row = j;
	u.nextStop = -1;
	for (size_t k = 0; k < listed.size() && u.nextStop < 0; k++)
		if (listed[k].row > j)
			u.nextStop = (int)k;
	if (u.nextStop >= 0) {
		u.sToStop = listed[(size_t)u.nextStop].s - u.s;
		u.tToStop = listed[(size_t)u.nextStop].tArrive - u.t;
	}
	u.tRemaining = p.t[N - 1] - u.t;
	return u;
}

long long compare(const std::vector<Timetabled>& got, const std::vector<Profiled>& profiles, const Limits& L, const std::vector<std::vector<double>>& values, bool byTime, int maxStops)
{
	long long compared = 0;
	assert(got.size() == profiles.size());
	for (size_t i = 0; i < got.size(); i++) {
		const Profiled& p = profiles[i];
		const Timetabled& g = got[i];
		if (p.status != Profiled::Status::Profiled) {
			assert(g.status == Timetabled::Status::NoProfile && g.numSamples == 0 && g.numStops == 0 && g.stops.empty());
			for (const auto& u : g.lookUps)
				assert(u.status == Timetabled::LookUp::Status::NoProfile && u.s == 0.0 && u.t == 0.0 && u.row == 0 && u.nextStop == 0);
			continue;
		}
		std::vector<Timetabled::Stop> stops = stopsOf(p, L);
		assert(g.status == Timetabled::Status::Profiled && g.numSamples == p.numSamples && g.numStops == (int)stops.size());
		assert(sameBits(g.sFirst, p.s.front()) && sameBits(g.sLast, p.s.back()) && sameBits(g.duration, p.t.back()));
		if ((int)stops.size() > maxStops)
			stops.resize((size_t)(maxStops > 0 ? maxStops : 0));
		assert(g.stops.size() == stops.size());
		for (size_t k = 0; k < stops.size(); k++) {
			assert(g.stops[k].row == stops[k].row && sameBits(g.stops[k].s, stops[k].s) && sameBits(g.stops[k].tArrive, stops[k].tArrive) && sameBits(g.stops[k].tDepart, stops[k].tDepart));
			assert(stops[k].tArrive <= stops[k].tDepart);
		}
		assert(g.lookUps.size() == (values.empty() ? 0 : values[i].size()));
		for (size_t k = 0; k < g.lookUps.size(); k++) {
			const Timetabled::LookUp want = lookUp(p, L, byTime, values[i][k], stops);
			const Timetabled::LookUp& u = g.lookUps[k];
			if (!(u.status == want.status && u.row == want.row && sameBits(u.s, want.s) && sameBits(u.t, want.t) && sameBits(u.v, want.v) && sameBits(u.a, want.a) &&
					u.nextStop == want.nextStop && sameBits(u.sToStop, want.sToStop) && sameBits(u.tToStop, want.tToStop) && sameBits(u.tRemaining, want.tRemaining))) {
				std::printf("plan %zu, value %.17g by %s: row %d s %.17g t %.17g v %.17g a %.17g next %d on the device, row %d s %.17g t %.17g v %.17g a %.17g next %d by the loop\n", i,
					values[i][k], byTime ? "time" : "length", u.row, u.s, u.t, u.v, u.a, u.nextStop, want.row, want.s, want.t, want.v, want.a, want.nextStop);
				assert(false);
			}
			assert(u.ratio >= 0.0 && u.ratio <= 1.0 && u.kappa >= 0.0 && u.direction >= -1 && u.direction <= 1);
			compared++;
		}
	}
	return compared;
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
	assert(pipe.Initialize(validator));
	std::vector<uint64_t> tickets;
	assert(pipe.Submit(starts, goals, seeds, &tickets) == n);
	std::vector<uint64_t> held;
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<HybridAStarPipeline::Result> out;
	while ((int)held.size() < n) {
		pipe.Poll(out, 4096, true);
		for (const auto& r : out)
			held.push_back(r.ticket);
		if (out.empty())
			std::this_thread::sleep_for(std::chrono::microseconds(200));
		assert(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60));
	}
	const double spacing = 0.2;
	Limits L;
	L.dwell = 0.75;
	const std::vector<Profiled> profiles = pipe.SpeedProfile(held, spacing, L);
	int profiled = 0;
	for (const Profiled& p : profiles)
		profiled += p.status == Profiled::Status::Profiled;
	assert(profiled >= n / 2);
	// ---- 70 values per plan (two passes of the kernel's lane loop and a remainder): before, behind, on rows, inside dwells, anywhere
	const size_t P = 70;
	long long compared = 0;
	for (const bool byTime : { false, true }) {
		std::vector<std::vector<double>> values(held.size());
		for (size_t i = 0; i < held.size(); i++) {
			const Profiled& p = profiles[i];
			const bool ok = p.status == Profiled::Status::Profiled;
			const std::vector<double>& col = byTime ? p.t : p.s;
			const double lo = ok ? col.front() : 0.0, hi = ok ? col.back() : 1.0;
			values[i] = { lo - 0.5, hi + 0.5, lo, hi };
			for (int k = 0; ok && k < 16; k++)
				values[i].push_back(col[(size_t)(uniform(0.0, 1.0) * (double)(col.size() - 1))]);
			if (ok && byTime)
				for (const auto& st : stopsOf(p, L))
					if (st.tArrive < st.tDepart && values[i].size() < 40)
						values[i].push_back(st.tArrive + 0.4 * (st.tDepart - st.tArrive));
			while (values[i].size() < P)
				values[i].push_back(uniform(lo, hi));
		}
		for (const int maxStops : { 16, 1, 0 })
			compared += compare(pipe.Timetable(held, values, byTime, maxStops), profiles, L, values, byTime, maxStops);
		if (byTime) { // the pose at a time since the start is the pose Conflicts gives at tau = t_start + u: the same readers on the same arc length
			Horizon h;
			h.tFrom = 0.0;
			h.tTo = 6.0;
			h.dt = 0.25;
			const std::vector<double> zero(held.size(), 0.0);
			const HybridAStarPipeline::Conflicted traj = pipe.Conflicts(held, zero, h, true); // (every pair: the pair records are not looked at)
			std::vector<std::vector<double>> lattice(held.size());
			for (auto& v : lattice)
				for (int m = 0; m <= 24; m++)
					v.push_back((double)m * h.dt);
			const std::vector<Timetabled> at = pipe.Timetable(held, lattice, true);
			for (size_t i = 0; i < held.size(); i++)
				for (size_t m = 0; m < lattice[i].size() && profiles[i].status == Profiled::Status::Profiled; m++) {
					const Pose2d& pose = traj.plans[i].poses[m];
					const Timetabled::LookUp& u = at[i].lookUps[m];
					assert((u.status == Timetabled::LookUp::Status::Inside) == !std::isnan(pose.x()));
					if (!std::isnan(pose.x()))
						assert(std::fabs(u.pose.x() - pose.x()) <= 1e-9 && std::fabs(u.pose.y() - pose.y()) <= 1e-9 && std::fabs(std::remainder(u.pose.theta - pose.theta, 2.0 * M_PI)) <= 1e-9);
				}
		}
	}
	std::printf("%lld look-ups compared\n", compared);
	assert(compared >= (long long)(6 * P) * (n / 2));
	// ---- no values: plans and stops only
	const std::vector<Timetabled> bare = pipe.Timetable(held, {});
	for (size_t i = 0; i < held.size(); i++)
		// (v_start = v_end = 0: both ends stand; the one-pose plan has one sample, which is both)
		assert(bare[i].lookUps.empty() && (profiles[i].status != Profiled::Status::Profiled ||
											  (bare[i].numStops >= (profiles[i].numSamples > 1 ? 2 : 1) && bare[i].stops.front().row == 0 && bare[i].stops.front().tArrive == 0.0)));
	// ---- a ticket that is not held throws; a held one without a profile is refused by the library; the pipeline goes on
	pipe.Release({ held[0] });
	bool threw = false;
	try {
		pipe.Timetable({ held[0], held[1] }, {});
	} catch (const std::invalid_argument&) {
		threw = true;
	}
	assert(threw);
	pipe.SpeedProfile({ held[1] }, spacing, L);
	threw = false;
	try {
		pipe.Timetable({ held[1], held[2] }, {});
	} catch (const std::exception& e) {
		threw = std::string(e.what()).find("speed_profile first") != std::string::npos;
	}
	assert(threw);
	const std::vector<Timetabled> one = pipe.Timetable({ held[1] }, { { 0.0 } }, true);
	assert(one.size() == 1 && one[0].lookUps.size() == 1 && one[0].lookUps[0].t == 0.0);
	held.erase(held.begin());
	pipe.Release(held);
	assert(pipe.FreeSlots() == 16);
	std::printf("pipeline timetable: Timetable(tickets, values) == the sequential loop over the downloaded rows\n");
	return 0;
}

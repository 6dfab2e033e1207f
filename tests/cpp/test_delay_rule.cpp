// The rule of a delay call (pathplanning_amd/csrc/pp_delay_rule.hpp) run on the host: the same text k_delay_level compiles for the device and the
// host side of the call runs.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_delay_rule_host.py.  It checks itself
// (exit status 1 and a line on stderr at the first failure) and prints every value, which the Python test compares with tests/delay_restatement.py.
//   C <T> <D> <d> <m> <column()>                 the column mapping
//   K <m> <n> <j> <key()> <time_of()> <partner_of()>
//   B <key> <best> <before()>                    the order of keys, ties among them
//   G <name> <n> <nPairs> <listed: 0 / 1>        a pair list follows (listed 0: pairs == nullptr, every pair)
//   P <a> <b>                                    one line per pair (also for listed 0: pair_at())
//   O <offsets[0 .. n]>
//   N <list>
//   V <level[0 .. n - 1]>
//   F <first[0 .. levels]>
//   M <members>
// Checked here: every column lies inside 0 .. T + D - 1 (d = 0, d = D; D = 0; T = 1); a key gives its (m, j) back and orders as (m, j) does; every
// partner is below its vehicle and above its level; a level's members ascend; the arrays are written exactly to their ends (the sanitizer sees a
// write past them: every vector is sized to the element).
#include "pp_delay_rule.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace {

[[noreturn]] void fail(const char* what, long long a, long long b)
{
	std::fprintf(stderr, "FAILED %s: %lld against %lld\n", what, a, b);
	std::exit(1);
}

void columns(int T, int D)
{
	const int ds[] = { 0, 1, D / 2, D - 1, D };
	const int ms[] = { 0, 1, T / 2, T - 2, T - 1 };
	for (int d : ds)
		for (int m : ms) {
			if (d < 0 || d > D || m < 0 || m >= T)
				continue;
			const int64_t c = ppy::column(m, D, d);
			if (c < 0 || c >= (int64_t)T + D)
				fail("column outside the extended trajectory", c, (int64_t)T + D);
			std::printf("C %d %d %d %d %lld\n", T, D, d, m, (long long)c);
		}
	if (ppy::column(0, D, D) != 0 || ppy::column(T - 1, D, 0) != (int64_t)T + D - 1)
		fail("the ends of the extended trajectory", ppy::column(0, D, D), ppy::column(T - 1, D, 0));
}

void keys()
{
	const int64_t ns[] = { 1, 2, 48, 4096, 1 << 20 };
	const int64_t ms[] = { 0, 1, 63, 64, (1 << 20) - 1 };
	for (int64_t n : ns)
		for (int64_t m : ms)
			for (int64_t j : { (int64_t)0, n / 2, n - 1 }) {
				const uint64_t k = ppy::key(m, n, j);
				if (ppy::time_of(k, n) != m || ppy::partner_of(k, n) != j || k == ppy::kNoKey)
					fail("a key gives its time and partner back", ppy::time_of(k, n), m);
				std::printf("K %lld %lld %lld %llu %d %d\n", (long long)m, (long long)n, (long long)j, (unsigned long long)k, ppy::time_of(k, n), ppy::partner_of(k, n));
			}
	// the order is (m, j)'s, and equal keys are not before each other
	const int64_t n = 48;
	const std::pair<int64_t, int64_t> mj[] = { { 3, 5 }, { 3, 5 }, { 3, 6 }, { 4, 0 }, { 2, 47 }, { 0, 0 } };
	for (const auto& a : mj)
		for (const auto& b : mj) {
			const uint64_t ka = ppy::key(a.first, n, a.second), kb = ppy::key(b.first, n, b.second);
			const bool want = a.first < b.first || (a.first == b.first && a.second < b.second);
			if (ppy::before(ka, kb) != want)
				fail("the order of keys", (long long)ka, (long long)kb);
			std::printf("B %llu %llu %d\n", (unsigned long long)ka, (unsigned long long)kb, ppy::before(ka, kb) ? 1 : 0);
		}
	for (const auto& a : mj)
		if (!ppy::before(ppy::key(a.first, n, a.second), ppy::kNoKey) || ppy::before(ppy::kNoKey, ppy::key(a.first, n, a.second)))
			fail("every key is before no key", a.first, a.second);
	std::printf("B %llu %llu %d\n", (unsigned long long)ppy::kNoKey, (unsigned long long)ppy::kNoKey, ppy::before(ppy::kNoKey, ppy::kNoKey) ? 1 : 0);
}

void graph(const char* name, int n, const std::vector<std::pair<int, int>>* listed)
{
	std::vector<int32_t> flat;
	if (listed)
		for (const auto& p : *listed) {
			flat.push_back(p.first);
			flat.push_back(p.second);
		}
	const int32_t* const pairs = listed ? flat.data() : nullptr;
	const int64_t nPairs = listed ? (int64_t)listed->size() : (int64_t)n * (n - 1) / 2;
	std::printf("G %s %d %lld %d\n", name, n, (long long)nPairs, listed ? 1 : 0);
	for (int64_t p = 0; p < nPairs; p++) {
		int a, b;
		ppy::pair_at(n, pairs, p, a, b);
		std::printf("P %d %d\n", a, b);
	}
	std::vector<int32_t> offsets((size_t)n + 1), cursor((size_t)n), list((size_t)nPairs), level((size_t)n), members((size_t)n);
	ppy::partner_offsets(n, nPairs, pairs, offsets.data());
	if (offsets[0] != 0 || offsets[(size_t)n] != nPairs)
		fail("the offsets end at the number of pairs", offsets[(size_t)n], nPairs);
	ppy::partner_list(n, nPairs, pairs, offsets.data(), cursor.data(), list.data());
	const int nLevels = ppy::levels(n, offsets.data(), list.data(), level.data());
	std::vector<int32_t> first((size_t)nLevels + 1);
	ppy::members_by_level(n, nLevels, level.data(), first.data(), members.data());
	for (int i = 0; i < n; i++)
		for (int32_t k = offsets[(size_t)i]; k < offsets[(size_t)i + 1]; k++)
			if (list[(size_t)k] < 0 || list[(size_t)k] >= i || level[(size_t)list[(size_t)k]] >= level[(size_t)i])
				fail("a partner is below its vehicle and on a lower level", list[(size_t)k], i);
	if (first[0] != 0 || first[(size_t)nLevels] != n || (n == 0) != (nLevels == 0))
		fail("the levels hold every vehicle", first[(size_t)nLevels], n);
	for (int l = 0; l < nLevels; l++) {
		if (first[(size_t)l + 1] <= first[(size_t)l])
			fail("no level is empty", l, nLevels);
		for (int32_t k = first[(size_t)l]; k < first[(size_t)l + 1]; k++)
			if (level[(size_t)members[(size_t)k]] != l || (k > first[(size_t)l] && members[(size_t)k - 1] >= members[(size_t)k]))
				fail("a level's members are its own and ascend", members[(size_t)k], l);
	}
	auto print = [](const char* tag, const std::vector<int32_t>& v) {
		std::printf("%s", tag);
		for (int32_t x : v)
			std::printf(" %d", x);
		std::printf("\n");
	};
	print("O", offsets);
	print("N", list);
	print("V", level);
	print("F", first);
	print("M", members);
}

} // namespace

int main()
{
	for (int T : { 1, 2, 63, 64, 65, 130, 601 })
		for (int D : { 0, 1, 63, 64, 65, 300 })
			columns(T, D);
	columns(1, (1 << 20) - 1);
	columns((1 << 20), 0);
	keys();
	const std::vector<std::pair<int, int>> none, chain = { { 0, 1 }, { 1, 2 }, { 2, 3 }, { 3, 4 }, { 4, 5 }, { 5, 6 } },
											   star = { { 0, 1 }, { 2, 0 }, { 0, 3 }, { 4, 0 }, { 0, 5 } },
											   twice = { { 0, 1 }, { 1, 0 }, { 2, 1 }, { 0, 1 }, { 3, 1 }, { 2, 1 }, { 2, 3 } },
											   mixed = { { 7, 2 }, { 2, 0 }, { 5, 7 }, { 1, 6 }, { 6, 7 }, { 3, 4 }, { 8, 4 }, { 0, 8 } };
	graph("empty-0", 0, &none);
	graph("empty-5", 5, &none);
	graph("one", 1, nullptr);
	graph("chain", 7, &chain);
	graph("star", 6, &star);
	graph("twice", 4, &twice);
	graph("mixed", 9, &mixed);
	graph("all-2", 2, nullptr);
	graph("all-12", 12, nullptr);
	std::vector<std::pair<int, int>> explicit12;
	for (int i = 0; i < 12; i++)
		for (int j = i + 1; j < 12; j++)
			explicit12.push_back({ i, j });
	graph("explicit-12", 12, &explicit12);
	std::printf("delay rule ok\n");
	return 0;
}

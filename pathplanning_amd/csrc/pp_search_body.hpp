// Body of the one-wave-per-query Hybrid-A* search kernels: included inside k_hybrid_search<kProfile> and k_hybrid_search_footprint
// (pp_planner.hip), NOT a header of its own.  The including kernel provides the arguments (A, nQueries, starts, goals, seeds, costFields,
// nodesBase, heapBase, keymapBase, expandedBase, rsLogBase, pathBase, results, prof, resume, nResume, mtBase, bandBase, bandInvW,
// bandMetaBase), the constants kProfile and kFootprint, and the footprint `foot` (read only where kFootprint).
#ifndef PP_SEARCH_BODY_INCLUDER
#error "pp_search_body.hpp is the body of the search kernels of pp_planner.hip; it is not a header to include elsewhere"
#endif
	// Two uses: (a) one block per query of the batch, buffers indexed by the query (resume == nullptr);
	// (b) continuation of the queries the rows kernel suspended: one block per SuspendRec, buffers indexed by its slot.
	if (resume ? ((int)blockIdx.x >= *nResume || (int)blockIdx.x >= A.listCap) : (int)blockIdx.x >= nQueries)
		return;
	const SuspendRec rec = resume ? resume[blockIdx.x] : SuspendRec {};
	const int q = resume ? rec.q : (int)blockIdx.x;
	const size_t slot = resume ? (size_t)rec.slot : (size_t)q;
	const int lane = threadIdx.x;
#if PP_SEARCH_SETPRIO
	__builtin_amdgcn_s_setprio(3); // see k_hybrid_search_rows
#endif
	unsigned long long phase[PH_COUNT] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	unsigned long long tlast = 0;
	if (kProfile)
		tlast = clock64();
#define PP_STAMP(i)                                \
	if (kProfile) {                                \
		const unsigned long long now_ = clock64(); \
		phase[i] += now_ - tlast;                  \
		tlast = now_;                              \
	}

	__shared__ unsigned long long mt[Mt64::N];
	// staging of the children of the node being expanded; kept until the next expansion so that a
	// child popped right away is read back from LDS instead of HBM
	__shared__ double c_x[kSlots], c_y[kSlots], c_t[kSlots], c_cost[kSlots], c_total[kSlots], c_len[kSlots], c_h[kSlots], c_sin[kSlots], c_cos[kSlots];
	__shared__ uint32_t c_key[kSlots], c_state[kSlots];
	__shared__ float c_d0[kSlots];
	__shared__ uint8_t c_valid[kSlots];
	__shared__ int16_t c_action[kSlots];
	__shared__ int s_rsChecks;
	__shared__ double s_rsPre[24]; // rs::Path::make_prefix of the Reeds-Shepp attempt (23 doubles)
	__shared__ HeapEntry s_spill[16]; // entries that left the front buffer during this expansion
	__shared__ uint8_t s_bandCnt[kBands]; // f-bands of the open list (pp_search_device.hpp): entries per ring slot

	const MapView& m = A.m;
	const int P = A.prims.n;
	const int maxNodes = A.maxNodes;
	Node* nodes = nodesBase + slot * maxNodes;
	HeapEntry* heap = heapBase + slot * maxNodes;
	HeapEntry* bands = bandBase + slot * (size_t)(kBands * kBandCap);
	uint32_t* keymap = keymapBase + slot * A.ks.size();
	uint32_t* expanded = expandedBase + (size_t)q * maxNodes;
	RsLogEntry* rsLog = rsLogBase + (size_t)q * kRsLogCap;
	const float* field = costFields + (size_t)q * A.fieldElems;

	// goal / start poses go through the Pose2d constructor on the caller's side (theta wrapped)
	const Pose start = { starts[3 * q], starts[3 * q + 1], wrap_theta(starts[3 * q + 2]) };
	const Pose goal = { goals[3 * q], goals[3 * q + 1], wrap_theta(goals[3 * q + 2]) };

	// ---- InitializeSearch, a_star.h:350-364 (a resumed query finds its key map, nodes and heap in the slot)
	if (!resume) {
		const size_t n = A.ks.size();
		const size_t n4 = n / 4;
		if ((((uintptr_t)keymap) & 15) == 0) {
			uint4 z = { 0, 0, 0, 0 };
			for (size_t i = lane; i < n4; i += 64)
				reinterpret_cast<uint4*>(keymap)[i] = z;
			for (size_t i = n4 * 4 + lane; i < n; i += 64)
				keymap[i] = 0;
		} else {
			for (size_t i = lane; i < n; i += 64)
				keymap[i] = 0;
		}
	}
	int myNode = -1; // node index of the child staged in this lane's slot (-1: none / not pushed)
	int rsNode = -1; // same for the Reeds-Shepp slot (wave-uniform)
	// Prefetch of the probable NEXT pop: while a node is expanded, lane k < 24 loads 32-bit word k of the record at the
	// head of the open list.  If that node is popped next (and is not a staged child) its fields come out of these
	// registers with v_readlane instead of a dependent HBM round trip.
	int pfNode = -1;
	uint32_t pfWord = 0u;
	bool pfDead = false; // the prefetched node was replaced (ProcessPossibleShortcut) after it was fetched
	if (!resume) {
		if (lane == 0)
			Mt64::seed(mt, seeds[q]);
	} else {
		for (int i = lane; i < Mt64::N; i += 64)
			mt[i] = mtBase[slot * Mt64::N + i]; // the engine state the rows kernel left in the slot
	}
	FrontLane front;
	front_clear(front);
	int frontCount = 0;
	int heapSize = resume ? rec.heapSize : 0;
	HeapEntry heapTop;
	heapTop.ckey = ~0ull;
	heapTop.nseq = ~0u;
	heapTop.node = 0;
	if (resume && heapSize > 0)
		heapTop = heap[0]; // the whole open list was flushed into the heap when the query was suspended
	// band window: fresh queries start it a little below the root's band; a resumed query brings its window and the
	// slot counts (saved next to the bands when it was set aside)
	uint8_t* const bandMeta = reinterpret_cast<uint8_t*>(bandMetaBase) + slot * (size_t)kBands;
	for (int i = lane; i < kBands; i += 64)
		s_bandCnt[i] = resume ? bandMeta[i] : (uint8_t)0;
	long long bandLo = resume ? rec.bandLo : 0;
	bool bandLoSet = resume != nullptr;
	int nOutside = resume ? rec.nOutside : 0; // open-list entries outside the front buffer (bands + heap + spill buffer)
	// lower bound of everything outside (a resumed query starts with the lowest possible bound: nothing enters the empty
	// front buffer before the first refill)
	unsigned long long lowK = resume ? 0ull : ~0ull;
	unsigned int lowS = resume ? 0u : ~0u;
	int nNodes = resume ? rec.nNodes : 1;
	unsigned int seq = resume ? rec.seq : 1;
	bool startOnBoundary = false;
	if (!resume) {
		double rs_, rc_;
		sincos(start.t, &rs_, &rc_);
		int ix, iy, it;
		startOnBoundary = discretize_pose(start, A.rp.lat, A.rp.headingAlias, ix, iy, it);
		uint32_t key = kNoKey;
		const bool ok = A.ks.pack(ix, iy, it, key);
		if (lane == 0) {
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
			if constexpr (kFootprint) {
				float cl, bd;
				root.dist0 = fp_state_valid_sc(m, foot, start.x, start.y, start.t, rs_, rc_, cl, bd) ? cl : -1.0f;
			} else {
				float d0;
				root.dist0 = is_state_valid(m, start.x, start.y, start.t, d0) ? d0 : -1.0f;
			}
			nodes[0] = root;
			if (ok)
				keymap[key] = kExplored; // the root is inserted in the explored set at init (a_star.h:361)
		}
		HeapEntry e;
		e.ckey = cost_key(0.0);
		e.nseq = 0xFFFFFFFFu;
		e.node = 0;
		HeapEntry sp;
		front_insert(front, frontCount, e, lane, sp);
	}
	int mtIdx = resume ? rec.mtIdx : Mt64::N; // engine freshly seeded: first draw twists
	__syncthreads();

	int nExpanded = resume ? rec.nExpanded : 0, nRngDraws = resume ? rec.nRngDraws : 0, nRsAttempts = resume ? rec.nRsAttempts : 0,
		nRsLog = resume ? rec.nRsLog : 0;
	// this lane's arcs; the totals of the suspended part ride in lane 0
	long long laneStateChecks = resume && lane == 0 ? rec.stateChecks : 0, lanePathChecks = resume && lane == 0 ? rec.pathChecks : 0;
	long long rsStateChecks = 0, rsPathChecks = 0;     // wave-uniform (Reeds-Shepp children)
	if (lane == 0)
		lanePathChecks += (long long)startOnBoundary << kGuardShift; // (guard band, pp_device.hpp: the count shares this counter's upper bits)
	int status = -1, solutionNode = -1;
	double solutionCost = __builtin_huge_val();

	// Entries that leave the front buffer are staged in LDS and flushed to the HBM heap in one go:
	// the flush loads all their heap parents in parallel (one memory round trip); only when some
	// entry really has to move up does lane 0 fall back to one-by-one sift-ups.
	int nSpill = 0;
	auto flush_spills = [&]() {
		if (nSpill == 0)
			return;
		__syncthreads();
		// every entry goes to the ring slot of its f-band when that slot is free or already serves the band and has
		// room; else to the heap.  One lane routes them: band counters live in LDS, so nothing here waits for HBM
		// except the occasional heap sift.
		if (lane == 0) {
			int hs = heapSize;
			for (int i = 0; i < nSpill; i++) {
				const HeapEntry e = s_spill[i];
				const long long B = band_of_key(e.ckey, bandInvW);
				const int sl = (int)(B & (kBands - 1));
				const int cnt = s_bandCnt[sl];
				if (B >= bandLo && B < bandLo + kBands && cnt < kBandCap) {
					bands[sl * kBandCap + cnt] = e;
					s_bandCnt[sl] = (uint8_t)(cnt + 1);
					s_spill[i].node = 0xFFFFFFFFu; // marks "not in the heap" for the loop below
				} else {
					heap_push(heap, hs, e);
				}
			}
		}
		__syncthreads();
		for (int i = 0; i < nSpill; i++) {
			const HeapEntry e = s_spill[i];
			if (e.node == 0xFFFFFFFFu)
				continue;
			if (heapSize == 0 || heap_before(e, heapTop))
				heapTop = e;
			heapSize++;
		}
		nSpill = 0;
		__syncthreads();
	};
	auto spill = [&](const HeapEntry& e) {
		if (!bandLoSet) { // the window starts one cost unit below the first entry that leaves the front buffer
			bandLo = (band_of_key(e.ckey, bandInvW) - 64) & ~3ll;
			bandLoSet = true;
		}
		if (lane == 0)
			s_spill[nSpill] = e;
		nSpill++;
		nOutside++;
		if (key_before(e.ckey, e.nseq, lowK, lowS)) {
			lowK = e.ckey;
			lowS = e.nseq;
		}
		if (nSpill == 16)
			flush_spills();
	};
	// An entry joins the front buffer exactly when "front <= everything outside" demands or allows it: it beats the
	// buffer's last entry (then it must; if the buffer is full that last entry leaves), or the buffer has room and the
	// entry beats the lower bound of the outside part.  (Checked against oracle traces by a CPU model of this policy.)
	auto push_open = [&](const HeapEntry& e) {
		bool toFront = true;
		if (frontCount < PP_FRONT_CAP)
			toFront = nOutside == 0 || key_before(e.ckey, e.nseq, lowK, lowS) ||
				(frontCount > 0 && key_before(e.ckey, e.nseq, lane_read64(front.ckey, frontCount - 1), lane_read(front.nseq, frontCount - 1)));
		if (toFront) {
			HeapEntry sp;
			if (front_insert(front, frontCount, e, lane, sp))
				spill(sp);
		} else {
			spill(e);
		}
	};
	// The front buffer ran empty: load the lowest band (all of it: one coalesced load), sort it in the wave, then pull in
	// whatever the heap holds below the buffer's last entry.
	auto refill = [&]() {
		flush_spills();
		// lowest non-empty band: the slots are scanned in ring order from the window's bottom, 64 per step (entries
		// cluster right above the current cost, so the first step nearly always hits)
		long long bAbs = 0x7FFFFFFFFFFFFFFFll;
		for (int step = 0; step < kBands / 64; step++) {
			const long long b = bandLo + step * 64 + lane;
			const unsigned long long hitm = __ballot(s_bandCnt[(int)(b & (kBands - 1))] > 0);
			if (hitm) {
				bAbs = bandLo + step * 64 + (__ffsll((long long)hitm) - 1);
				break;
			}
		}
		long long loadedTop = bandLo - 1; // highest band that has certainly been emptied
		if (bAbs != 0x7FFFFFFFFFFFFFFFll) {
			// the 64 lanes take the aligned group of four consecutive bands that contains the lowest one (4 x 16 entries,
			// contiguous in memory): lane l -> band (group << 2 | l >> 4), entry l & 15
			const long long bn = ((bAbs >> 2) << 2) | (long long)(lane >> 4);
			const int sl = (int)(bn & (kBands - 1));
			const int cntSl = s_bandCnt[sl];
			const bool mineBand = cntSl > 0 && bn >= bandLo && bn < bandLo + kBands;
			const bool have = mineBand && (lane & 15) < cntSl;
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
			__builtin_amdgcn_s_waitcnt(0); // lane 0's band stores
			HeapEntry e;
			e.ckey = ~0ull;
			e.nseq = ~0u;
			e.node = 0;
			if (have)
				e = bands[sl * kBandCap + (lane & 15)];
			const int n = __popcll(__ballot(have));
			wave_sort_entries(e.ckey, e.nseq, e.node, lane);
			front.ckey = e.ckey;
			front.nseq = e.nseq;
			front.node = e.node;
			frontCount = n;
			nOutside -= n;
			__syncthreads();
			if (mineBand && (lane & 15) == 0)
				s_bandCnt[sl] = 0;
			__syncthreads();
			bandLo = bAbs & ~3ll;           // every band below the lowest one was empty: the window moves up (multiple of 4)
			loadedTop = ((bAbs >> 2) << 2) | 3; // the group's bands inside the window are empty now
		}
		// (the bound of the outside part is rebuilt from here: spill() lowers it for every entry the loop below pushes out of a full buffer
		// -- those go back into bands at or below `loadedTop` when the spill buffer fills up, where the band-boundary term further down does
		// not see them.  Without this a later, worse entry could enter the buffer ahead of them: found on a 44 597-expansion query of the
		// full-size batch, whose expansion order left the oracle's at expansion 41 196; tests/test_gpu_fullsize.py)
		lowK = ~0ull;
		lowS = ~0u;
		// heap entries that come before the buffer's last entry (or, with an empty buffer, the heap's best) move in
		while (heapSize > 0 && (frontCount == 0 || key_before(heapTop.ckey, heapTop.nseq, lane_read64(front.ckey, frontCount - 1), lane_read(front.nseq, frontCount - 1)))) {
			__syncthreads();
			const HeapEntry he = heap_pop_wave(heap, heapSize, lane, heapTop);
			__syncthreads();
			nOutside--;
			HeapEntry sp;
			if (front_insert(front, frontCount, he, lane, sp))
				spill(sp);
		}
		// lower bound of what is outside now: the heap's best, the start of the first band that was not loaded, the spill
		// buffer
		if (heapSize > 0 && key_before(heapTop.ckey, heapTop.nseq, lowK, lowS)) {
			lowK = heapTop.ckey;
			lowS = heapTop.nseq;
		}
		{
			const unsigned long long bk = cost_key((double)(loadedTop + 1) / bandInvW);
			if (bk < lowK || (bk == lowK && 0u < lowS)) {
				lowK = bk;
				lowS = 0u; // below every entry of that band
			}
		}
		for (int i = 0; i < nSpill; i++) {
			const HeapEntry e = s_spill[i];
			if (key_before(e.ckey, e.nseq, lowK, lowS)) {
				lowK = e.ckey;
				lowS = e.nseq;
			}
		}
	};

	// ---- SearchPath main loop, a_star.h:337-345
	while (frontCount > 0 || nOutside > 0) {
		if (frontCount == 0)
			refill();
		const HeapEntry top = front_pop(front, frontCount, lane); // the front holds the global best entries
		PP_STAMP(PH_POP);
		const int ni = (int)top.node;
		// ---- the popped node: from the staging of the previous expansion when it is one of its children
		double px, py, pt, pPathCost, pH, pSin, pCos;
		uint32_t pKey;
		float pDist0;
		bool pDead = false;
		{
			const unsigned long long hit = __ballot(myNode == ni);
			int slot = hit ? (__ffsll((long long)hit) - 1) : (rsNode == ni ? kRsSlot : -1);
			if (slot >= 0) {
				px = c_x[slot];
				py = c_y[slot];
				pt = c_t[slot];
				pPathCost = c_cost[slot];
				pH = c_h[slot];
				pSin = c_sin[slot];
				pCos = c_cos[slot];
				pKey = c_key[slot];
				pDist0 = c_d0[slot];
			} else if (ni == pfNode) {
				auto dbl = [&](int wi) { return __hiloint2double((int)lane_read(pfWord, wi + 1), (int)lane_read(pfWord, wi)); };
				px = dbl(0);
				py = dbl(2);
				pt = dbl(4);
				pPathCost = dbl(6);
				pH = dbl(12);
				pSin = dbl(14);
				pCos = dbl(16);
				pKey = lane_read(pfWord, 19);
				pDead = pfDead || ((lane_read(pfWord, 20) >> 16) & 0xFFu) != 0u;
				pDist0 = __uint_as_float(lane_read(pfWord, 21));
			} else {
				const Node nd = nodes[ni];
				px = nd.x;
				py = nd.y;
				pt = nd.t;
				pPathCost = nd.pathCost;
				pH = nd.h;
				pSin = nd.sinT;
				pCos = nd.cosT;
				pKey = nd.key;
				pDead = nd.dead != 0;
				pDist0 = nd.dist0;
			}
		}
		wave_lds_sync(); // staging is about to be overwritten
		if (pDead)
			continue; // entry of a node replaced by ProcessPossibleShortcut
		const Pose ppose = { px, py, pt };
		if (identical_poses(ppose, goal)) { // IsSolution, hybrid_a_star.h:193-196
			status = 0;
			solutionNode = ni;
			solutionCost = pPathCost;
			break;
		}
		// ---- Expand, a_star.h:377-409
		if (lane == 0) {
			if (pKey != kNoKey)
				keymap[pKey] = kExplored; // children in the parent's own cell are caught by a key compare below
			expanded[nExpanded] = pKey; // the expansion log holds the packed discrete pose of each expanded node
		}
		rsNode = -1;
		nExpanded++;
		int pix, piy, pit;
		discretize_pose(ppose, A.rp.lat, A.rp.headingAlias, pix, piy, pit);
		PP_STAMP(PH_LOAD);
		// RS gate input (hybrid_a_star.cpp:81): the heuristic of this pose was computed when the node was created
		const double hCost = pH;
		PP_STAMP(PH_HEUR);

		bool capacity = false;
		// ---- constant-steer children, reference order p = 2*deltaIndex + direction (hybrid_a_star.cpp:65-77)
		for (int base = 0; base < P; base += 64) {
			const int p = base + lane;
			bool ok = false;
			uint32_t key = kNoKey, st = 0u;
			Pose child = ppose;
			double cs = pSin, cc = pCos;
			double gcost = 0.0, total = 0.0, len = 0.0, hh = 0.0;
			float d0 = -1.0f;
			if (p < P) {
				ArcSC a;
				a.init = ppose;
				a.sinF = pSin;
				a.cosF = pCos;
				a.kappa = A.prims.kappa[p];
				a.invKappa = A.prims.invKappa[p];
				a.length = A.rp.arcLength;
				a.backward = A.prims.backward[p];
				child = a.interpolate_sc(1.0, cs, cc);
				int ix, iy, it;
				const bool onLine = discretize_pose(child, A.rp.lat, A.rp.headingAlias, ix, iy, it);
				lanePathChecks += (long long)onLine << kGuardShift;
				if (onLine) // logged at once (nothing kept live across the march): if the arc gets truncated this entry is moot, and a
					guard_log(A, q, ni, p, 1, a.length, ix, iy, it); // mismatch on it only sends the query to the CPU reference needlessly
				PP_STAMP(PH_HEUR); // [diagnostic: endpoint]
				// look-ups of the full-length child are issued before the validity march so that their
				// latency overlaps it (they are redone only when the arc gets truncated)
				bool packed = A.ks.pack(ix, iy, it, key);
				if (packed)
					st = keymap[key];
				HeurLoads hl;
				combined_heuristic_issue(A.heur, m, field, goal, child, cs, cc, hl);
				// Voronoi term of the full-length arc: its only map read (the last sample, Q8) is issued with the look-ups
				float voroRaw;
				voronoi_cost_issue(m, a, A.rp.voroDiagRes, voroRaw);
				float lastValidRatio;
				int checks = 0;
				ok = true;
				lanePathChecks++;
				// validity / distance of the child's own pose: the first march sample of ITS children (not a counted check)
				float cd0;
				bool cIn, pathValid;
				if constexpr (kFootprint) {
					cIn = false;
					pathValid = is_arc_valid_fp_from(m, foot, fp_gain(foot, fabs(a.kappa)), a, pDist0, lastValidRatio, checks);
				} else {
					cIn = is_state_valid_issue(m, child.x, child.y, child.t, cd0);
					pathValid = is_path_valid_from(m, a, a.init, pDist0, lastValidRatio, checks);
				}
				PP_STAMP(PH_DUP); // [diagnostic: look-up issue + validity march]
				// the values the look-ups above fetched (loaded under the march)
				hh = combined_heuristic_finish(A.heur, hl);
				const double voroFull = voronoi_cost_finish(voroRaw, A.rp.voroDiagRes, A.rp.voronoiMult);
				if constexpr (kFootprint) {
					float cb;
					d0 = pathValid && fp_state_valid_sc(m, foot, child.x, child.y, child.t, cs, cc, cd0, cb) ? cd0 : -1.0f; // (a truncated arc's child is checked below)
				} else
					d0 = is_state_valid_finish(m, cIn, cd0) ? cd0 : -1.0f;
				if (!pathValid) {
					// PathConstantSteer::Truncate, paths/path_constant_steer.cpp:16-20
					child = a.interpolate_sc((double)lastValidRatio, cs, cc);
					a.length *= (double)lastValidRatio;
					const bool onLineT = discretize_pose(child, A.rp.lat, A.rp.headingAlias, ix, iy, it);
					lanePathChecks += (long long)onLineT << kGuardShift;
					if (onLineT)
						guard_log(A, q, ni, p, 1, a.length, ix, iy, it); // the truncated child is the one that counts
					if (ix == pix && iy == piy && it == pit)
						ok = false;
					else {
						packed = A.ks.pack(ix, iy, it, key);
						if (packed)
							st = keymap[key];
						hh = combined_heuristic_sc(A.heur, m, field, goal, child, cs, cc);
						if constexpr (kFootprint) {
							float cb;
							d0 = fp_state_valid_sc(m, foot, child.x, child.y, child.t, cs, cc, cd0, cb) ? cd0 : -1.0f;
						} else
							d0 = is_state_valid(m, child.x, child.y, child.t, cd0) ? cd0 : -1.0f;
					}
				}
				laneStateChecks += checks;
				if (ok) {
					const double pathCost = (a.backward ? A.rp.reverseMult : A.rp.forwardMult) * a.length;
					const double voro = pathValid ? voroFull : voronoi_cost(m, a, A.rp.voroDiagRes, A.rp.voronoiMult);
					const double cost = pathCost + 0.0 + voro; // switching cost is always 0 (hybrid_a_star.cpp:142)
					len = a.length;
					gcost = pPathCost + cost;
					total = gcost + hh; // a_star.h:387-388
					if (!packed)
						ok = false; // outside the key map (cannot happen for poses inside the bounds)
				}
			}
			if (ok && key == pKey)
				st = kExplored; // the parent's cell was marked explored just above (a_star.h:381)
			// open-list node already in this child's cell: its pose / cost (needed by ProcessPossibleShortcut) is fetched
			// by the child's own lane now, all lanes at once, instead of one dependent load per child in the loop below
			double fpx = 0.0, fpy = 0.0, fpt = 0.0, fptot = 0.0;
			uint32_t fpFor = 0u;
			wave_vmem_sync(); // node records written by earlier expansions
			if (ok && st != 0u && st != kExplored) {
				const Node* fn = nodes + (st - 1u);
				fpx = fn->x;
				fpy = fn->y;
				fpt = fn->t;
				fptot = fn->totalCost;
				fpFor = st;
			}
			if (base == 0) {
				// probable next pop (head of the front buffer or of the heap) -> pfWord
				const int cand = frontCount > 0 ? (int)lane_read(front.node, 0) : -1; // the front holds the global best
				pfNode = cand;
				pfDead = false;
				if (cand >= 0 && lane < 24)
					pfWord = reinterpret_cast<const uint32_t*>(nodes + cand)[lane];
			}
			// does an EARLIER valid child of this batch share my cell?  (then my prefetched state may be stale)
			bool dup = false;
			const int cnt = min(64, P - base);
			for (int e = 0; e < cnt; e++) {
				const uint32_t ke = lane_read(key, e);
				const int ve = (int)lane_read(ok ? 1u : 0u, e);
				if (e < lane && ve && ke == key)
					dup = true;
			}
			// staging for the pop that follows (read back from LDS when one of these children is expanded next)
			c_key[lane] = key;
			c_x[lane] = child.x;
			c_y[lane] = child.y;
			c_t[lane] = child.t;
			c_cost[lane] = gcost;
			c_total[lane] = total;
			c_len[lane] = len;
			c_h[lane] = hh;
			c_sin[lane] = cs;
			c_cos[lane] = cc;
			c_d0[lane] = d0;
			myNode = -1;
			wave_lds_sync();
			PP_STAMP(PH_CHILD);
			// ---- insertion in child order, wave-uniform (a_star.h:391-402 + hybrid_a_star.h:199-205);
			// every per-child value is read from its lane's registers (v_readlane), not from memory
			const unsigned long long totalBits = (unsigned long long)__double_as_longlong(total);
			// Most children change nothing (their cell is explored, or holds an open-list node they do not beat): every
			// lane settles that for its own child, and only the children that push, replace, share a cell with an
			// earlier child of the batch or lack the prefetched record walk the serial path below, in child order.
			bool need = false;
			if (lane < cnt && ok) {
				if (dup || st == 0u)
					need = true;
				else if (st != kExplored) {
					if (fpFor == st) {
						const Pose fpp = { fpx, fpy, fpt };
						need = identical_poses(fpp, child) && fptot > total; // ProcessPossibleShortcut would replace it
					} else {
						need = true;
					}
				}
			}
			for (unsigned long long todo = __ballot(need); todo; todo &= todo - 1ull) {
				const int c = __ffsll((long long)todo) - 1;
				const uint32_t ckey = lane_read(key, c);
				uint32_t cst = lane_read(st, c);
				if (lane_read(dup ? 1u : 0u, c)) {
					wave_vmem_sync(); // lane 0's key-map writes of this batch
					cst = keymap[ckey];
				}
				const double ctotal = __longlong_as_double((long long)lane_read64(totalBits, c));
				bool push = false;
				if (cst == 0u) {
					push = true; // !inFrontier && !inExplored
				} else if (cst != kExplored) {
					// in the open list: replace only if the poses are identical and the new path is strictly cheaper
					const int fi = (int)cst - 1;
					const unsigned long long hitf = __ballot(myNode == fi);
					Pose fp;
					double ftotal;
					if (hitf) {
						const int fs = __ffsll((long long)hitf) - 1;
						fp = { c_x[fs], c_y[fs], c_t[fs] };
						ftotal = c_total[fs];
					} else if (lane_read(fpFor, c) == cst) {
						fp.x = __longlong_as_double((long long)lane_read64((unsigned long long)__double_as_longlong(fpx), c));
						fp.y = __longlong_as_double((long long)lane_read64((unsigned long long)__double_as_longlong(fpy), c));
						fp.t = __longlong_as_double((long long)lane_read64((unsigned long long)__double_as_longlong(fpt), c));
						ftotal = __longlong_as_double((long long)lane_read64((unsigned long long)__double_as_longlong(fptot), c));
					} else {
						wave_vmem_sync();
						const Node fn = nodes[fi];
						fp = { fn.x, fn.y, fn.t };
						ftotal = fn.totalCost;
					}
					const Pose cp = { c_x[c], c_y[c], c_t[c] };
					if (identical_poses(fp, cp) && ftotal > ctotal) {
						if (fi == pfNode)
							pfDead = true;
						if (lane == 0)
							nodes[fi].dead = 1;
						if (myNode == fi)
							myNode = -1; // its staged copy must not be used any more
						push = true;
					}
				}
				if (push) {
					if (nNodes >= maxNodes) {
						capacity = true;
						break;
					}
					const int idx = nNodes++;
					if (lane == c)
						myNode = idx;
					if (lane == 0)
						keymap[ckey] = (uint32_t)idx + 1u;
					HeapEntry e;
					e.ckey = cost_key(ctotal);
					e.nseq = 0xFFFFFFFFu - seq;
					seq++;
					e.node = (uint32_t)idx;
					push_open(e);
				}
			}
			PP_STAMP(PH_INSERT);
			// ---- every lane writes the node record of its own child
			if (myNode >= 0) {
				Node nd;
				nd.x = child.x;
				nd.y = child.y;
				nd.t = child.t;
				nd.pathCost = gcost;
				nd.totalCost = total;
				nd.length = len;
				nd.h = hh;
				nd.sinT = cs;
				nd.cosT = cc;
				nd.parent = ni;
				nd.key = key;
				nd.action = (int16_t)p;
				nd.dead = 0;
				nd.dist0 = d0;
				nodes[myNode] = nd;
			}
			PP_STAMP(PH_WRITE);
			if (capacity)
				break;
		}
		if (capacity) {
			status = -4;
			break;
		}

		// ---- Reeds-Shepp analytic expansion, gated (hybrid_a_star.cpp:81-88): the RNG is drawn
		// only when hCost >= 10 (short-circuit ||)
		bool tryRs = hCost < 10.0;
		if (!tryRs) {
			if (mtIdx >= Mt64::N) {
				Mt64::twist_wave(mt, lane);
				mtIdx = 0;
			}
			const double u = Mt64::uniform01(Mt64::temper(mt[mtIdx]));
			mtIdx++;
			nRngDraws++;
			tryRs = u < 10.0 / (hCost * hCost);
		}
		if (tryRs) {
			nRsAttempts++;
			// GetOptimalPath (reeds_shepp.cpp:654-683): lane w evaluates word w
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
			double wt = 0, wu = 0, wv = 0;
			bool wvalid = false;
			if (lane < rs::kNumWords) {
				double gx, gy, gt;
				rs::goal_variant(rel, lane % 4, gx, gy, gt);
				const double length = rs::base_lengths(lane / 4, gx, gy, gt, wt, wu, wv);
				if (!(length == rs::inf())) {
					rs::Segment sg;
					rs::word_segment(lane, wt, wu, wv, sg);
					wcost = rs::compute_cost(sg, A.rmin, A.rsRev, A.rsFwd, A.rsSw);
					wvalid = wcost < __builtin_huge_valf(); // NaN and +inf never win a `cost < optimalCost` test
				}
			}
			// first strictly-lowest float cost in word order
			float best = wvalid ? wcost : __builtin_huge_valf();
#pragma unroll
			for (int off = 32; off > 0; off >>= 1)
				best = fminf(best, __shfl_xor(best, off, 64));
			const unsigned long long match = __ballot(wvalid && wcost == best);
			const int word = match ? (__ffsll((long long)match) - 1) : -1;
			if (word >= 0) {
				const double bt = __shfl(wt, word, 64), bu = __shfl(wu, word, 64), bv = __shfl(wv, word, 64);
				// the winner's path is validated by one lane (the adaptive march is sequential)
				if (lane == 0) {
					rs::Path path;
					path.init = ppose;
					rs::word_segment(word, bt, bu, bv, path.seg);
					path.rmin = A.rmin;
					path.length = path.seg.length * A.rmin; // PathSegment::GetLength
					float lastRatio;
					int checks = 0;
					path.make_prefix(s_rsPre); // (see k_hybrid_search_rows)
					const rs::PrefixedPath ppath = { path, s_rsPre, path.length };
					bool valid;
					if constexpr (kFootprint)
						valid = is_path_valid_fp(m, foot, fp_gain(foot, 1.0 / A.rmin), ppath, path.init, lastRatio, checks);
					else
						valid = is_path_valid(m, ppath, path.init, lastRatio, checks);
					c_valid[kRsSlot] = 0;
					s_rsChecks = checks;
					if (valid) {
						const double pathAndSwitchingCosts = (double)rs::compute_cost(path.seg, A.rmin, A.rsRev, A.rsFwd, A.rsSw); // PathReedsShepp::ComputeCost
						const Pose child = ppath.interpolate(1.0);
						int ix, iy, it;
						const bool onLineR = discretize_pose(child, A.rp.lat, A.rp.headingAlias, ix, iy, it);
						lanePathChecks += (long long)onLineR << kGuardShift;
						if (onLineR)
							guard_log(A, q, ni, word, 2, path.length, ix, iy, it);
						const double voro = voronoi_cost(m, ppath, A.rp.voroDiagRes, A.rp.voronoiMult);
						const double cost = pathAndSwitchingCosts + voro;
						uint32_t key;
						if (A.ks.pack(ix, iy, it, key)) {
							double s_, c_;
							sincos(child.t, &s_, &c_);
							const double hh = combined_heuristic_sc(A.heur, m, field, goal, child, s_, c_);
							c_valid[kRsSlot] = 1;
							c_key[kRsSlot] = key;
							c_x[kRsSlot] = child.x;
							c_y[kRsSlot] = child.y;
							c_t[kRsSlot] = child.t;
							c_cost[kRsSlot] = pPathCost + cost;
							c_total[kRsSlot] = (pPathCost + cost) + hh;
							c_len[kRsSlot] = path.length;
							c_h[kRsSlot] = hh;
							c_sin[kRsSlot] = s_;
							c_cos[kRsSlot] = c_;
							if constexpr (kFootprint) {
								float rd0, rb;
								c_d0[kRsSlot] = fp_state_valid_sc(m, foot, child.x, child.y, child.t, s_, c_, rd0, rb) ? rd0 : -1.0f;
							} else {
								float rd0;
								c_d0[kRsSlot] = is_state_valid(m, child.x, child.y, child.t, rd0) ? rd0 : -1.0f;
							}
							c_state[kRsSlot] = keymap[key];
							c_action[kRsSlot] = (int16_t)(1000 + word);
						}
					}
				}
				wave_lds_sync();
				rsPathChecks++;
				rsStateChecks += (long long)s_rsChecks;
				if (c_valid[kRsSlot]) {
					const uint32_t ckey = c_key[kRsSlot];
					const uint32_t cst = c_state[kRsSlot];
					bool push = false;
					if (cst == 0u)
						push = true;
					else if (cst != kExplored) {
						const int fi = (int)cst - 1;
						const unsigned long long hitf = __ballot(myNode == fi);
						Pose fp;
						double ftotal;
						if (hitf) {
							const int fs = __ffsll((long long)hitf) - 1;
							fp = { c_x[fs], c_y[fs], c_t[fs] };
							ftotal = c_total[fs];
						} else {
							wave_vmem_sync();
							const Node fn = nodes[fi];
							fp = { fn.x, fn.y, fn.t };
							ftotal = fn.totalCost;
						}
						const Pose cp = { c_x[kRsSlot], c_y[kRsSlot], c_t[kRsSlot] };
						if (identical_poses(fp, cp) && ftotal > c_total[kRsSlot]) {
							if (fi == pfNode)
								pfDead = true;
							if (lane == 0)
								nodes[fi].dead = 1;
							if (myNode == fi)
								myNode = -1;
							push = true;
						}
					}
					if (push) {
						if (nNodes >= maxNodes) {
							status = -4;
							break;
						}
						const int idx = nNodes++;
						if (lane == 0) {
							Node nd;
							nd.x = c_x[kRsSlot];
							nd.y = c_y[kRsSlot];
							nd.t = c_t[kRsSlot];
							nd.pathCost = c_cost[kRsSlot];
							nd.totalCost = c_total[kRsSlot];
							nd.length = c_len[kRsSlot];
							nd.h = c_h[kRsSlot];
							nd.sinT = c_sin[kRsSlot];
							nd.cosT = c_cos[kRsSlot];
							nd.parent = ni;
							nd.key = ckey;
							nd.action = c_action[kRsSlot];
							nd.dead = 0;
							nd.dist0 = c_d0[kRsSlot];
							nodes[idx] = nd;
							keymap[ckey] = (uint32_t)idx + 1u;
							if (nRsLog < kRsLogCap) {
								RsLogEntry le;
								le.node = idx;
								le.word = word;
								le.t = bt;
								le.u = bu;
								le.v = bv;
								rsLog[nRsLog] = le;
							}
						}
						rsNode = idx;
						nRsLog++;
						HeapEntry e;
						e.ckey = cost_key(c_total[kRsSlot]);
						e.nseq = 0xFFFFFFFFu - seq;
						seq++;
						e.node = (uint32_t)idx;
						push_open(e);
					}
				}
				wave_lds_sync();
			}
		}
		PP_STAMP(PH_RS);
	}
	if (kProfile && lane == 0)
		for (int i = 0; i < PH_COUNT; i++)
			prof[(size_t)q * PH_COUNT + i] = phase[i];
#undef PP_STAMP

	// lane-local counters -> totals
	for (int off = 32; off > 0; off >>= 1) {
		laneStateChecks += __shfl_xor(laneStateChecks, off, 64);
		lanePathChecks += __shfl_xor(lanePathChecks, off, 64);
	}
	const long long nStateChecks = laneStateChecks + rsStateChecks;
	const long long pathChecksPacked = lanePathChecks + rsPathChecks;
	const long long pathChecks = pathChecksPacked & kGuardMask;
	__syncthreads();
	if (lane == 0) {
		DevResult r;
		r.r.n_lattice_boundary_hits = (int32_t)(pathChecksPacked >> kGuardShift);
		r.r.reserved = 0;
		r.r.status = status;
		r.r.n_expanded = nExpanded;
		r.r.n_nodes = nNodes;
		r.r.n_path = 0;
		if (status == 0)
			r.r.n_path = write_path(nodes, solutionNode, pathBase + (size_t)q * A.maxPath, A.maxPath);
		r.r.cost = solutionCost;
		r.r.n_rng_draws = nRngDraws;
		r.r.n_rs_attempts = nRsAttempts;
		r.r.n_state_checks = nStateChecks;
		r.r.n_path_checks = pathChecks;
		r.solutionNode = solutionNode;
		r.nRsLog = nRsLog < kRsLogCap ? nRsLog : kRsLogCap;
		results[q] = r;
	}

// orlg_group_body.h -- the TEXT of orlg_rmsa_group_kernel's body (orlg_group_kernels.hip), from the first statement to the last.
// Not a header to include at file scope: it is included INSIDE a function that has the kernel's template arguments (W, STATS,
// HBMQ, DEFER, TRAFFIC, TRACE), the constants `LEAN`, `CAUSE`, `ASSIGN`, `CUT` and `USAGE` and the parameters `p` in scope -- once in the kernel itself and once in
// orlg_rmsa_group_body, which gives the DEFER instantiations their second, lean body.  Why the text and not only the function:
// a kernel whose body arrives through an inlined function compiles to slightly different code than one that holds the text
// (other spill placement, a few dozen instructions either way), and the instantiations without a lean body are to stay,
// byte for byte, the code objects they were.
//
// LEAN compiles out what a first-fit launch without per-step outputs and with discrete bit rates never runs: the external,
// path-only, DeepRMSA and load-balancing policies, the validation of an external action, the per-step outputs (`done`
// included) and the continuous bit-rate refill.  Everything else is the same operations on the same values -- the graph statistics
// of an accepted provision too, but later: LEAN logs what _update_network_stats consumes and works the log off in batches
// (orlg_graph_log.h, group_graph_replay).
    static_assert(!DEFER || (STATS >= 2 && !HBMQ), "the deferred link statistics belong to long launches with full statistics");
    static_assert(!(TRACE && TRAFFIC), "a trace handle has no arrival rates");
    static_assert(!LEAN || DEFER, "the lean body belongs to the long launches");
    static_assert(!CAUSE || (!HBMQ && !DEFER), "the blocking cause belongs to the plain kind");
    static_assert(!ASSIGN || (!HBMQ && !DEFER), "the assignment rules belong to the plain kind");
    static_assert(!CUT || ASSIGN, "the fewest-cuts window is an assignment rule");
    static_assert(!USAGE || (ASSIGN && !CUT), "most-used windows and the best-window route are assignment rules of their own");
    // LEAN keeps two of the step's books on the lanes, because nothing in a lean launch reads them before a ticket ends (DESIGN 2.5,
    // round 20; orlg_group_plan.h gives the lean body to handles of at most 2 * ORLG_GL bit rates only):
    // LANE_HIST: lane gl of a row counts the arrivals (h_req) and the accepted provisions (h_acc) with the bit-rate indices gl (low
    // 16 bits) and gl + 16 (high 16 bits) since the last flush; the four histograms and the eight counters follow from them in
    // books_flush -- at an episode's end, when the ticket's state leaves, and every ORLG_LEAN_FLUSH_STEPS steps of a ticket, so that no
    // field overflows.  Between flushes the counters rest in the scalars record, as the graph log's three doubles do
    // LANE_SUMS: sum_span and sum_gaps are lane partials (group_link_stats, PART): lane 0 of the row starts with the state's
    // value, every lane adds its own links' differences, and the row sum is formed where orlg_glog_pack and the state store read it
    constexpr bool LANE_HIST = LEAN, LANE_SUMS = LEAN;
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int g = lane >> 4, gl = lane & 15;
    const Tab tb = make_tab(smem, p);
    // one MT19937 staging buffer per workgroup (a refill happens every ~15 steps per wave and takes a fraction of a step),
    // handed from wave to wave with a lock word behind it: LDS per wave decides how many environments a CU keeps resident
    uint32_t *mt_lds = reinterpret_cast<uint32_t *>(smem + p.l_shared_bytes);
    int *mt_lock = reinterpret_cast<int *>(smem + p.l_shared_bytes + p.g_mt);
    if (threadIdx.x == 0) *mt_lock = 0;
    __syncthreads();
    unsigned char *wbase = smem + p.l_shared_bytes + p.g_mt + 16 + (size_t)wib * p.g_wave_bytes;
    // this row's environment: slice g of every array of the wave's region (array-major: OrlgParams::g_occ ...)
    u64 *occ = reinterpret_cast<u64 *>(wbase + p.g_occ) + g * p.NW;
    double *qtime = nullptr;
    uint32_t *qdesc = nullptr;
    if constexpr (!HBMQ) {
        qtime = reinterpret_cast<double *>(wbase + p.g_qtime) + g * p.Q;
        qdesc = reinterpret_cast<uint32_t *>(wbase + p.g_qdesc) + g * p.Q;
    }
    // (DEFER: the link statistics are touched by group_link_replay only, a few times per launch: they stay in HBM, and the 704
    // bytes per environment they took of the LDS buy a twelfth wave per CU)
    double *lst = DEFER ? nullptr : reinterpret_cast<double *>(wbase + p.g_lstat) + g * 4 * p.E;
    int32_t *lint = reinterpret_cast<int32_t *>(wbase + p.g_lint) + g * p.lint_stride;
    // DEFER: the links' summaries (lsum_pack) take the place of the statistics' slices; built whenever a quad's state is loaded,
    // kept by every provision and release -- LDS only, the state in HBM does not hold them
    u64 *lsum = DEFER ? reinterpret_cast<u64 *>(wbase + p.g_lstat) + g * p.E : nullptr;

    const int E = p.E, S = p.S, K = p.K, N = p.N, NBR = p.NBR, Q = p.Q, NW = p.NW;
    constexpr bool NET = STATS >= 1;
    constexpr bool FULL = STATS >= 2;
    const double INF = __longlong_as_double((long long)ORLG_INF_BITS);
    // the network compactness after a step's releases is read by two per-step outputs only (a provision's statistics pass
    // computes its own, and the state that leaves does not hold it): a launch that asks for neither leaves the two float64
    // divisions out.  Wave-uniform: a scalar branch
    const bool out_comp = !LEAN && (p.out_mask & ((1 << ORLG_OUT_COMPACT) | (1 << ORLG_OUT_COMPACT_DIFF))) != 0;
    SEC_DECL_G

    // ------------------------------------------------------------------ work queue over quads of environments
    // quad q = environments 4q .. 4q+3; the first quad of a wave is its own index, the rest come from the ticket counter
    // (long launches) or by striding (short ones), as in the wave-per-environment kernel
    // A long launch hands its quads out in CHUNKS of steps (OrlgParams::n_chunks): with whole launches as tickets the last round
    // of a batch that is not a multiple of the resident waves runs at a fraction of the occupancy for a whole launch's time
    // (B = 65 536: 5.33 rounds); a chunk of a quad goes to whichever wave draws it, after the wave that ran the chunk before
    // has published the quad's state (progress[quad]; release / acquire at agent scope: another CU, maybe another XCD).
    const int n_quads = (p.B + ORLG_GE - 1) / ORLG_GE;
    const int n_chunks = p.n_chunks > 1 ? p.n_chunks : 1;
    const int n_tix = n_quads * n_chunks;
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    // (with chunks EVERY ticket is drawn, a wave's first one too: a ticket that waits for its predecessor must be able to count on
    // a RUNNING wave holding it -- a statically assigned ticket of a workgroup that is not resident yet, because another kernel
    // shares the device, would be waited for by the very waves that keep that workgroup out)
    const int n_static = n_chunks > 1 ? 0 : (n_waves < n_tix ? n_waves : n_tix);
    int tix = (int)(blockIdx.x * (blockDim.x >> 6)) + wib;
    if (n_chunks == 1 && tix >= n_tix) return;
    uint32_t nxt_tk = 0;
    if (n_chunks > 1 && lane == 0) nxt_tk = atomicAdd(p.ticket, 1u);
    for (bool first = n_chunks == 1;; first = false) {
    if (!first) {
        if (p.ticket_stride) {
            tix += n_waves;
            if (tix >= n_tix) break;
        } else {
            const uint32_t tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt_tk) - p.ticket_base;
            if (tk >= (uint32_t)(n_tix - n_static)) break;
            tix = n_static + (int)tk;
        }
    }
    int chunk = 0, quad = tix;
    if (n_chunks > 1) { chunk = tix / n_quads; quad = tix - chunk * n_quads; }
    const int t0 = n_chunks > 1 ? chunk * p.chunk_steps : 0;   // first step of this ticket within the launch
    SEC(1);  // state load
    if (!p.ticket_stride && lane == 0) nxt_tk = atomicAdd(p.ticket, 1u);
    if (chunk > 0) {
        // the quad's state as the previous chunk left it: one relaxed poll, one acquire, the wait for its invalidate -- then
        // plain loads (MI355X_MICROARCH.md, inter-workgroup visibility)
        if (lane == 0)
            while (__hip_atomic_load(p.progress + quad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)chunk) __builtin_amdgcn_s_sleep(16);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const int env_raw = quad * ORLG_GE + g;
    const bool act = env_raw < p.B;          // rows past the batch's end idle (they load the last environment and store nothing)
    const int env = act ? env_raw : p.B - 1;

    // ------------------------------------------------------------------ HBM -> LDS
    // occupancy, link statistics, span caches of the quad's environments: linear copies (rows past the batch's end take a
    // copy of the last environment's slices afterwards)
    const int env0 = quad * ORLG_GE;
    const int nact = p.B - env0 < ORLG_GE ? p.B - env0 : ORLG_GE;
    quad_copy(wbase + p.g_occ, p.occ + (size_t)env0 * NW, nact * NW * 8, lane);
    if (FULL && !DEFER) quad_copy(wbase + p.g_lstat, p.lstat + (size_t)env0 * 4 * E, nact * 4 * E * 8, lane);
    // the bit-rate histograms are only ever incremented (and zeroed at an episode's end): they stay in HBM and take L2 atomics
    // without return -- 336 bytes of LDS per environment decide how many waves a CU keeps resident.  Every access
    // is an atomic, so that the updates of one address arrive at L2 in program order.
    int32_t *ghist = p.hist + (size_t)env * 4 * NBR;
    // DEFER: the same addresses formed where they are used, from a wave-uniform base (the quad's first environment: scalar
    // registers) and the row's 32-bit byte offset -- as per-lane 64-bit pointers they are loop invariants the step loop has no
    // registers for, and a reload from scratch is a load: the wave waits for everything it has in flight
    [[maybe_unused]] char *hist_q = reinterpret_cast<char *>(p.hist + (size_t)env0 * 4 * NBR);
    [[maybe_unused]] const uint32_t hist_row = (uint32_t)((env - env0) * 4 * NBR) * 4u;
    // (histogram `which`, entry i; the other instantiations keep the statements they had, so that they stay the code they were)
    [[maybe_unused]] auto hist_at = [&](int which, int i) -> int32_t * {
        return reinterpret_cast<int32_t *>(hist_q + (hist_row + (uint32_t)(which * NBR + i) * 4u));
    };
    if (NET) quad_copy(wbase + p.g_lint, p.lint + (size_t)env0 * p.lint_stride, nact * p.lint_stride * 4, lane);
    if (nact < ORLG_GE) {   // the batch's last quad only
        wave_sync();
        if (!act) {
            const int gs_ = nact - 1;
            for (int i = gl; i < NW; i += ORLG_GL) occ[i] = (reinterpret_cast<u64 *>(wbase + p.g_occ) + gs_ * NW)[i];
            if (FULL && !DEFER) for (int i = gl; i < 4 * E; i += ORLG_GL) lst[i] = (reinterpret_cast<double *>(wbase + p.g_lstat) + gs_ * 4 * E)[i];
            if (NET) for (int i = gl; i < p.lint_stride; i += ORLG_GL) lint[i] = (reinterpret_cast<int32_t *>(wbase + p.g_lint) + gs_ * p.lint_stride)[i];
        }
    }
    // the link-update log of this row's environment (DEFER), and its link statistics where they live: HBM
    uint4 *llog = DEFER ? p.llog + (size_t)env * E * ORLG_LLOG_CAP : nullptr;
    if (DEFER) lst = p.lstat + (size_t)env * 4 * E;
    bool need_replay = false;
    const OrlgEnvScalars *gs = p.scal + env;
    double current_time = gs->current_time, req_arrival = gs->req_arrival, req_holding = gs->req_holding;
    double g_thr = gs->g_throughput, g_comp = gs->g_compactness, g_lu = gs->g_last_update;
    [[maybe_unused]] long long cnt = gs->c[gl & 7];  // counter gl & 7 (lanes 8..15 mirror lanes 0..7); LANE_HIST: not read, the counters stay in the record
    long long sum_bitrate_running = gs->sum_bitrate_running, episodes_done = gs->episodes_done;
    int sum_sh = gs->sum_slots_hops, n_running = gs->n_running;
    int req_src = gs->req_src, req_dst = gs->req_dst, req_br = gs->req_br, req_sid = gs->req_sid;
    int mt_idx = gs->mt_idx, new_service = gs->new_service, q_overflow = gs->q_overflow;
    int ring_pos = gs->ring_pos, ring_cnt = gs->ring_cnt;
    int sum_span = gs->sum_span, sum_gaps = gs->sum_gaps;
    if (LANE_SUMS && gl != 0) { sum_span = 0; sum_gaps = 0; }   // (lane partials: the state's sums on the row's first lane)
    int eproc = (int)gs->c[2];
    wave_sync();
    // LANE_HIST: the accumulators, and the flush of the rows `rows` -- the histograms take atomics without return, as everywhere (the
    // updates of one address stay in program order); the counters are row sums of the accumulators (services) and of accumulator x
    // bit rate, added to the record by the row's first eight lanes.  `episode`: the flush of an episode's end, which leaves the
    // episode counters as reset(only_episode_counters=True) with a pending service does (below).  Cold: a few times per environment
    // and launch.  Its addresses are formed where they are used, from the quad's wave-uniform bases and the row's place in the quad
    // (cold_row): every one of them is a loop invariant, and the compiler keeps a hoisted invariant in a register or in scratch
    // across the whole step loop -- the empty asm makes the row's place a value it cannot hoist, and hist_q, hist_row and hist_at
    // have no use in this body
    // (lane_one: what the lane adds for a request of bit-rate index br -- 1 in the field of br on the lane of br, 0 elsewhere; br_one:
    // that of the pending request, which counts at its arrival and, a step later, where it is accepted)
    [[maybe_unused]] uint32_t h_req = 0u, h_acc = 0u;
    [[maybe_unused]] auto lane_one = [&](int br) -> uint32_t { return (br & (ORLG_GL - 1)) == gl ? 1u << (br & ORLG_GL) : 0u; };
    [[maybe_unused]] uint32_t br_one = lane_one(req_br);
    [[maybe_unused]] auto cold_row = [&]() -> uint32_t {
        uint32_t r = (uint32_t)(env - env0);
        asm volatile("" : "+v"(r));
        return r;
    };
    [[maybe_unused]] auto hist_lean = [&](uint32_t row, int which, int i) -> int32_t * {
        return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(p.hist + (size_t)env0 * 4 * NBR) + ((row * 4u + (uint32_t)which) * (uint32_t)NBR + (uint32_t)i) * 4u);
    };
    [[maybe_unused]] auto books_flush = [&](const bool rows, const bool episode) {
        const int gh = gl + ORLG_GL;
        const int rate_lo = gl < NBR ? tb.bit_rates[gl] : 0, rate_hi = gh < NBR ? tb.bit_rates[gh] : 0;
        const int req_lo = (int)(h_req & 0xffffu), req_hi = (int)(h_req >> 16), acc_lo = (int)(h_acc & 0xffffu), acc_hi = (int)(h_acc >> 16);
        const long long n_req = row_add_i32(req_lo + req_hi), n_acc = row_add_i32(acc_lo + acc_hi);
        const long long b_req = row_add_i64((long long)req_lo * rate_lo + (long long)req_hi * rate_hi);
        const long long b_acc = row_add_i64((long long)acc_lo * rate_lo + (long long)acc_hi * rate_hi);
        if (rows) {
            const uint32_t row = cold_row();
            if (gl < NBR && req_lo) { atomicAdd(hist_lean(row, 0, gl), req_lo); atomicAdd(hist_lean(row, 2, gl), req_lo); }
            if (gh < NBR && req_hi) { atomicAdd(hist_lean(row, 0, gh), req_hi); atomicAdd(hist_lean(row, 2, gh), req_hi); }
            if (gl < NBR && acc_lo) { atomicAdd(hist_lean(row, 1, gl), acc_lo); atomicAdd(hist_lean(row, 3, gl), acc_lo); }
            if (gh < NBR && acc_hi) { atomicAdd(hist_lean(row, 1, gh), acc_hi); atomicAdd(hist_lean(row, 3, gh), acc_hi); }
            if (gl < 8) {
                int64_t *c = reinterpret_cast<OrlgEnvScalars *>(reinterpret_cast<char *>(p.scal + env0) + row * (uint32_t)sizeof(OrlgEnvScalars))->c + gl;
                long long v = *c + ((gl & 4) ? ((gl & 1) ? b_acc : b_req) : ((gl & 1) ? n_acc : n_req));
                if (episode) v = gl == 2 ? 1 : (gl == 6 ? tb.bit_rates[req_br] : ((gl == 3 || gl == 7) ? 0 : v));
                *c = v;
            }
            h_req = 0u; h_acc = 0u;
        }
    };
    // LEAN: the graph statistics are logged per accepted provision and worked off in batches (orlg_graph_log.h, group_graph_replay):
    // entry k of the row's environment on lane k of the row, lg_cnt of them.  g_thr, g_comp, g_lu and comp_cur are then names
    // nothing reads: between two replays the three doubles rest in the scalars record, and the body has no use for the compactness
    [[maybe_unused]] OrlgGraphEntry lg = {0.0, 0u, 0u, 0u};
    [[maybe_unused]] int lg_cnt = 0;
    double comp_cur = 1.0;
    if (NET && !LEAN) comp_cur = network_compactness(sum_span, sum_sh, sum_gaps, E);
    if (DEFER)   // the summaries of all E links, from the occupancy just loaded
        group_link_stats<W, true, false, true, 2>(lane, occ, nullptr, lint, tb, S, E, nullptr, E, 0.0, sum_span, sum_gaps, comp_cur,
                                                  0, 0.0, g_thr, g_comp, g_lu, nullptr, nullptr, lsum);
    // release queue: a time-sorted ring in LDS (OrlgParams::qtime) -- q_n entries from slot q_head on; the row keeps the time of
    // its head in a register, so that a step without a due release touches no queue memory.  q_head is the head's slot in LDS: it
    // starts a ticket where the state has it and falls behind by one slot per insert from the head's side (queue insert)
    int q_head = gs->q_head, q_n = n_running < Q ? n_running : Q;   // (n_running also counts services an overflow lost)
    // only the live part of the ring moves between HBM and LDS (a launch of one step would otherwise spend most of its
    // traffic on empty slots); LDS slots outside it are never read
    const int q_head0 = q_head;
    int q_pops = 0;   // releases of this launch: the head may lap the ring (a 1000-step launch pops ~8 x Q entries)
    if constexpr (HBMQ) {
        qtime = p.qtime + (size_t)env * Q;
        qdesc = p.qdesc + (size_t)env * Q;
    } else {
        const double *gqt = p.qtime + (size_t)env * Q;
        const uint32_t *gqd = p.qdesc + (size_t)env * Q;
        for (int j = gl; j < q_n; j += 2 * ORLG_GL) {   // two slots per lane and pass: four requests in flight, then four writes
            int pos = q_head + j;
            pos -= pos >= Q ? Q : 0;
            int pos2 = pos + ORLG_GL;
            pos2 -= pos2 >= Q ? Q : 0;
            const bool two = j + ORLG_GL < q_n;
            const double t0 = gqt[pos];
            const uint32_t d0 = gqd[pos];
            double t1 = 0.0;
            uint32_t d1 = 0u;
            if (two) { t1 = gqt[pos2]; d1 = gqd[pos2]; }
            qtime[pos] = t0; qdesc[pos] = d0;
            if (two) { qtime[pos2] = t1; qdesc[pos2] = d1; }
        }
    }
    wave_sync();
    double next_rel = q_n > 0 ? qtime[q_head] : INF;
    // ... and the head's descriptor with it: a release starts from a register, the path record one round trip earlier
    uint32_t next_desc = q_n > 0 ? qdesc[q_head] : 0u;
    const int cidx = gl & 7;
    [[maybe_unused]] int cause_cnt = 0;   // CAUSE: lane c of the row counts this ticket's steps with cause c
    int req_base = tb.pair_base[req_src * N + req_dst];  // first path record of the pending request's node pair

    const int n_iter = n_chunks > 1 ? (p.n_steps - t0 < p.chunk_steps ? p.n_steps - t0 : p.chunk_steps) : p.n_steps;
    const int policy = p.policy;
    for (int t = 0; t < n_iter; ++t) {
        SEC(2);  // policy
        // the arrival this step ends with is requested now (the ring entry is known unless a refill comes first)
        double pf_iat = 0.0, pf_ht = 0.0;
        uint32_t pf_rq = 0;
        const bool pf_ok = ring_cnt > 0;
        if (pf_ok) {
            const size_t ro = (size_t)env * ORLG_RING + ring_pos;
            pf_iat = p.ring_iat[ro]; pf_ht = p.ring_ht[ro]; pf_rq = p.ring_req[ro];
        }
        // ========================================================== policy: pick (path, slot)
        const int base = req_base;
        int a_path = K, a_slot = S;  // rejection (rmsa_env.py:871,913)
        int ff_n = 1, ff_hops = 0;
        if constexpr (ASSIGN) {
            // An assignment rule other than the reference's first fit (include/orlg.h ORLG_ASSIGN_*, orlg_assign.h): the policy is
            // the route -- the first path (sp), the first path that has a window (sap), of the paths that have one the path
            // with the most free slots, ties to the first (llp; rmsa_env.py:854-937), or the agent's path (rmsa_env.py:982-1005) --
            // and the rule's key decides the slot on it: one maximum over the path's W lanes, one minimum over the row
            constexpr int PP = ORLG_GL / W;  // candidate paths per pass
            const int rule = p.assign;
            const bool given = policy == ORLG_POLICY_PATH_EXT;
            int path0 = 0;
            bool a_ok = true;
            if (given) {
                const int a = p.actions[env];
                a_ok = a >= 0 && a < K;
                path0 = a_ok ? a : 0;
            }
            const bool llp = policy == ORLG_POLICY_LLP;
            const int kmax = (given || policy == ORLG_POLICY_SP) ? 1 : K;
            const int ps = gl / W, w = gl - ps * W;
            int found = 0x7fffffff, found_key = 0x7fffffff;
            // CUT: the fewest-cuts window (OrlgParams::assign == ORLG_ASSIGN_MIN_CUT, orlg_step_min_cut; orlg_cut.h) has a hop loop of
            // its own, which counts per window start the links it would cut; the rules' loop below is compiled out, as this one is
            // without CUT.  Its route "fewest cuts" (ORLG_POLICY_MIN_CUT) ranks the paths by their window's cuts as llp ranks them
            // by free slots: row minima of (rank, path), the earlier pass wins a tie
            [[maybe_unused]] const bool ranked = llp || policy == ORLG_POLICY_MIN_CUT;
            for (int p0 = 0; CUT && p0 < kmax; p0 += PP) {
                if (!ranked && ballot(act && a_ok && found == 0x7fffffff) == 0ull) break;
                const int pp = p0 + ps;
                const bool on = ps < PP && pp < kmax && a_ok;
                int hops_pp, n;
                u64 x;
                const uint32_t sk = seg_max<W>(cut_word_key<W>(occ, tb.recs, base + path0 + pp, w, on, tb.nslots + req_br * ORLG_NSLOT_STRIDE, S,
                                                               hops_pp, n, x));   // the path's key, on its first lane
                const bool head = on && w == 0 && sk != 0u;
                const int payload = head ? (((((path0 + pp) << 10) | cut_key_slot(sk)) << 14) | (n << 4) | hops_pp) : 0x7fffffff;
                if (ranked) {
                    const uint32_t fs = seg_add<W>((uint32_t)popc64(x));
                    const uint32_t rank = llp ? 1023u - fs : (uint32_t)cut_key_cuts(sk);
                    const int key = head ? (int)((rank << 6) | (uint32_t)pp) : 0x7fffffff;
                    const int bk = row_min_i32(key);
                    const int bp = row_min_i32(key == bk ? payload : 0x7fffffff);
                    if (bk < found_key) { found_key = bk; found = bp; }
                    continue;
                }
                const int best = row_min_i32(payload);
                if (found == 0x7fffffff) found = best;
            }
            // USAGE: orlg_step_window under the rule MOST_USED or the route BEST_WINDOW (orlg_usage.h) -- the rules' loop below with
            // the rule MOST_USED beside the four (its key reads the prefix sums of the slot usage, which the row computes from the
            // occupancy this step meets) and with a ranked route that compares the paths' keys themselves: a key is 27 bits, so the
            // row takes the minimum of the inverted rank first and then, among the paths that hold it, the lowest payload (the path
            // is its top field).  The other two loops are compiled out, as this one is without USAGE
            if constexpr (USAGE) {
                int32_t *uincl = reinterpret_cast<int32_t *>(smem + p.l_shared_bytes + p.g_mt + 16 + (size_t)(blockDim.x >> 6) * p.g_wave_bytes) +
                                 (wib * ORLG_GE + g) * (ORLG_USAGE_BYTES(W) / 4);
                if (rule == ORLG_ASSIGN_MOST_USED) {
                    usage_prefix<W, 1>(occ, uincl, E, S, lane);
                    wave_sync();
                }
                const bool ranked_w = llp || policy == ORLG_POLICY_BEST_WINDOW;
                for (int p0 = 0; p0 < kmax; p0 += PP) {
                    if (!ranked_w && ballot(act && a_ok && found == 0x7fffffff) == 0ull) break;
                    const int pp = p0 + ps;
                    const bool on = ps < PP && pp < kmax && a_ok;
                    int se_pp, hops_pp;
                    const u64 x = group_path_word_rec<W>(occ, tb.recs, base + path0 + pp, w, on, se_pp, hops_pp) & valid_mask(S, w);
                    int n = 1;
                    if (on) n = tb.nslots[req_br * ORLG_NSLOT_STRIDE + se_pp];
                    const uint32_t sk = seg_max<W>(window_word_key<W>(uincl, x, n, w, rule));   // the path's key, on its first lane
                    const bool head = on && w == 0 && sk != 0u;
                    const int payload = head ? (((((path0 + pp) << 10) | window_key_slot(sk, rule)) << 14) | (n << 4) | hops_pp) : 0x7fffffff;
                    if (ranked_w) {
                        const uint32_t fs = seg_add<W>((uint32_t)popc64(x));
                        const int inv = head ? (int)(llp ? 1023u - fs : 0x7ffffffeu - sk) : 0x7fffffff;
                        const int bk = row_min_i32(inv);
                        const int bp = row_min_i32(inv == bk ? payload : 0x7fffffff);
                        if (bk < found_key) { found_key = bk; found = bp; }
                        continue;
                    }
                    const int best = row_min_i32(payload);
                    if (found == 0x7fffffff) found = best;
                }
            }
            for (int p0 = 0; !CUT && !USAGE && p0 < kmax; p0 += PP) {
                if (!llp && ballot(act && a_ok && found == 0x7fffffff) == 0ull) break;
                const int pp = p0 + ps;
                const bool on = ps < PP && pp < kmax && a_ok;
                int se_pp, hops_pp;
                const u64 x = group_path_word_rec<W>(occ, tb.recs, base + path0 + pp, w, on, se_pp, hops_pp) & valid_mask(S, w);
                int n = 1;
                if (on) n = tb.nslots[req_br * ORLG_NSLOT_STRIDE + se_pp];
                const uint32_t sk = seg_max<W>(assign_word_key<W>(x, n, w, rule));   // the path's key, on its first lane
                const bool head = on && w == 0 && sk != 0u;
                const int payload = head ? (((((path0 + pp) << 10) | assign_key_slot(sk, rule)) << 14) | (n << 4) | hops_pp) : 0x7fffffff;
                if (llp) {
                    // most free slots, then lowest path (as the first-fit form below)
                    const uint32_t fs = seg_add<W>((uint32_t)popc64(x));
                    const int key = head ? (int)(((1023u - fs) << 6) | (uint32_t)pp) : 0x7fffffff;
                    const int bk = row_min_i32(key);
                    const int bp = row_min_i32(key == bk ? payload : 0x7fffffff);
                    if (bk < found_key) { found_key = bk; found = bp; }
                    continue;
                }
                const int best = row_min_i32(payload);
                if (found == 0x7fffffff) found = best;
            }
            if (found != 0x7fffffff) { a_path = found >> 24; a_slot = (found >> 14) & 1023; ff_n = (found >> 4) & 1023; ff_hops = found & 15; }
        } else if (!LEAN && policy == ORLG_POLICY_EXT) {
            a_path = p.actions[2 * env];
            a_slot = p.actions[2 * env + 1];
        } else {
            constexpr int PP = ORLG_GL / W;  // candidate paths per pass
            // The first-fit family: the lowest start of a free window of n slots below S - n on the first path that has one
            // (rmsa_env.py:854-913), over one given path for PathOnlyFirstFitAction (rmsa_env.py:982-1005).  The DeepRMSA family
            // (deeprmsa_env.py:48-58, rmsa_env.py:774-804): the start of the b-th free BLOCK (maximal free run) of >= n slots --
            // block 0 of the first path that has one for the heuristics, block a % j of path a / j for an agent action.
            // (LEAN: first fit over the first path or over all K, nothing else)
            const bool deep = !LEAN && (policy == ORLG_POLICY_DEEP_SP || policy == ORLG_POLICY_DEEP_SAP || policy == ORLG_POLICY_DEEP_EXT);
            const bool given = !LEAN && (policy == ORLG_POLICY_PATH_EXT || policy == ORLG_POLICY_DEEP_EXT);  // the agent names the path
            int path0 = 0, blk = 0;
            bool a_ok = true;
            if (given) {
                const int a = p.actions[env];
                if (policy == ORLG_POLICY_DEEP_EXT) {
                    a_ok = a >= 0 && a < K * p.j;
                    path0 = a_ok ? a / p.j : 0;
                    blk = a_ok ? a - path0 * p.j : 0;
                } else {
                    a_ok = a >= 0 && a < K;
                    path0 = a_ok ? a : 0;
                }
            }
            // Load balancing (least_loaded_path_first_fit, rmsa_env.py:893-937): of the paths that have a window, the one with the
            // most free slots on it (ties: the first), its first fit.
            const bool llp = !LEAN && policy == ORLG_POLICY_LLP;
            const int kmax = (given || policy == ORLG_POLICY_SP || (!LEAN && policy == ORLG_POLICY_DEEP_SP)) ? 1 : K;
            const int ps = gl / W, w = gl - ps * W;
            int found = 0x7fffffff, found_key = 0x7fffffff;
            // First fit starts below S - n (exclusive: rmsa_env.py:860-871).  Slots at and beyond S are stored as not free, so a free
            // window of n slots lies inside [0, S) and starts below S - n exactly when it does not hold slot S - 1: the first-fit
            // family looks for its windows with that one slot cleared, and no start needs masking afterwards.  (Slot S - 1 is in
            // word (S - 1) >> 6, not always the last of the W words.)  The DeepRMSA family has no such limit: nothing cleared.
            const u64 lastbit = (!deep && w == ((S - 1) >> 6)) ? 1ull << ((S - 1) & 63) : 0ull;
            for (int p0 = 0; p0 < kmax; p0 += PP) {
                if (!llp && ballot(act && a_ok && found == 0x7fffffff) == 0ull) break;
                const int pp = p0 + ps;
                bool on = ps < PP && pp < kmax && a_ok;
                int se_pp, hops_pp;
                int n = 1;
                // the pass's path record (an inactive lane keeps a zero record, group_path_word_rec's): the pass below is written ONCE,
                // from the record -- with the pass in both arms of the branch the lean body carried three scratch reloads into
                // the step loop
                uint4 rq = make_uint4(0u, 0u, 0u, 0u);
                if (LEAN && p0 > 0) {
                    // A first-fit pass after the first (LEAN: first fit, and the links' summaries exist): only the rows that have no
                    // window yet look on, and only at the paths whose links all have a free run of n (group_path_candidate, which
                    // also loads the record and the slot count); a pass that no row of the batch has such a path for would find
                    // nothing and is left out.  Left out, not the last: with three passes the last one may hold the window the
                    // middle one cannot.  Rows past the batch's end do not vote.  (The full body of the DEFER instantiations could
                    // run the same test -- lsum is there -- but it costs that body spilled registers, and no long launch runs it)
                    SEC(16);  // longest-run test
                    on = group_path_candidate<W>(lane, lsum, tb, base + path0 + pp, base, w, on && found == 0x7fffffff, req_br, rq, n);
                    SEC(2);
                    if (ballot(act && on) == 0ull) continue;
                } else if (on) {
                    rq = *reinterpret_cast<const uint4 *>(tb.recs + (base + path0 + pp));
                }
                const u64 x = group_path_word_of<W>(occ, rq, w, on, se_pp, hops_pp);
                if (!(LEAN && p0 > 0) && on) n = tb.nslots[req_br * ORLG_NSLOT_STRIDE + se_pp];
                u64 r = run_starts<W>(x & ~lastbit, n, w);
                const u64 xprev = lane_prev_u64(x);
                if (deep) {
                    // block starts: free slots whose predecessor is not free
                    r &= x & ~((x << 1) | (w > 0 ? xprev >> 63 : 0ull));
                    if (!LEAN && policy == ORLG_POLICY_DEEP_EXT) {
                        // the blk-th block of the path (its words are the row's first W lanes): blocks in the words before this one
                        const int cntw = popc64(r);
                        int incl = cntw, o;
                        o = lane_back_i32<1>(incl); incl += o;
                        o = lane_back_i32<2>(incl); incl += o;
                        o = lane_back_i32<4>(incl); incl += o;
                        const int kth = blk - (incl - cntw);  // which block of this word
                        for (int q = 0; q < p.j; ++q)
                            if (q < kth) r &= r - 1;
                        if (kth < 0 || kth >= cntw) r = 0ull;
                    }
                }
                // key: (path, start slot) decide; the path's slot count and hops ride along in the low bits
                if (llp) {
                    // per path, on its first lane: free slots of the path-wide mask and its first fit (none: 0)
                    const uint32_t fs = seg_add<W>((uint32_t)popc64(x));
                    const uint32_t fit = seg_max<W>(r ? (uint32_t)(0x7fff - (64 * w + ctz64(r))) : 0u);
                    const bool head = on && w == 0 && fit != 0u;
                    // most free slots, then lowest path: six bits of path (k W <= 64 allows k = 64; four bits let a path 16 and
                    // above spill into the free-slot count)
                    const int key = head ? (int)(((1023u - fs) << 6) | (uint32_t)pp) : 0x7fffffff;
                    const int bk = row_min_i32(key);
                    const int payload = (head && key == bk) ? ((((pp << 10) | (0x7fff - (int)fit)) << 14) | (n << 4) | hops_pp) : 0x7fffffff;
                    const int bp = row_min_i32(payload);
                    if (bk < found_key) { found_key = bk; found = bp; }
                    continue;
                }
                const int cand = r ? (((((path0 + pp) << 10) | (64 * w + ctz64(r))) << 14) | (n << 4) | hops_pp) : 0x7fffffff;
                const int best = row_min_i32(cand);
                if (found == 0x7fffffff) found = best;
            }
            if (found != 0x7fffffff) { a_path = found >> 24; a_slot = (found >> 14) & 1023; ff_n = (found >> 4) & 1023; ff_hops = found & 15; }
        }

        // ========================================================== RMSAEnv.step (rmsa_env.py:222-341)
        SEC(3);  // validate + provision
        const double prev_compact = comp_cur;
        bool accepted = false;
        const bool in_range = act && a_path >= 0 && a_path < K && a_slot >= 0 && a_slot < S;
        const int gid = base + (in_range ? a_path : 0);
        const OrlgPathRec *rec = tb.recs + gid;
        int hops = ff_hops, n = ff_n;
        if (LEAN || policy != ORLG_POLICY_EXT) {
            accepted = in_range;  // a first-fit result is a free window by construction
        } else {
            hops = rec->hops;
            n = tb.nslots[req_br * ORLG_NSLOT_STRIDE + rec->se];
            // is_path_free on the chosen window: word gl of the path on lane gl
            const bool on = in_range && gl < W;
            const u64 x = path_word<W>(occ, tb.recs, gid, gl < W ? gl : 0, on);
            const u64 m = on ? window_mask(a_slot, n, gl) : 0ull;
            const uint32_t bad = row_ballot((x & m) != m, lane);
            accepted = in_range && a_slot + n <= S && bad == 0u;
        }
        const int br_val = tb.bit_rates[req_br];
        // CAUSE: the blocking cause of the rows that are not accepted, on the occupancy the step met (include/orlg.h ORLG_CAUSE_*)
        [[maybe_unused]] int cause = 0;
        if constexpr (CAUSE) {
            const bool refused = act && !accepted;
            if (ballot(refused) != 0ull) {
                const int level = group_fit_level<W>(lane, occ, tb, base, K, S, req_br, refused);
                cause = refused ? ORLG_CAUSE_CAPACITY + level : ORLG_CAUSE_ACCEPTED;
            }
            if (act) cause_cnt += gl == cause ? 1 : 0;
        }
        // ---- _provision_path (rmsa_env.py:462-513)
        // (with network statistics the statistics pass below clears the window as it reads the links' words)
        if (!NET) group_apply_window<W>(lane, occ, rec->link, accepted ? hops : 0, a_slot, n, false);
        // DEFER: the step's one wait for vector memory, where it is free -- the ring prefetch and the previous step's last log stores
        // and histogram atomics were issued at least a policy pass ago, and from here on the step issues stores and atomics
        // without return only, which nothing in it waits for
        if constexpr (DEFER) vm_drain();
        if (accepted) {
            sum_sh += n * hops;
            n_running += 1;
            sum_bitrate_running += br_val;
            if constexpr (LANE_HIST) {
                h_acc += br_one;
            } else {
                cnt += (cidx == 1 || cidx == 3) ? 1 : ((cidx == 5 || cidx == 7) ? br_val : 0);
                if constexpr (DEFER) {
                    if (gl == 0) { atomicAdd(hist_at(1, req_br), 1); atomicAdd(hist_at(3, req_br), 1); }
                } else {
                    if (gl == 0) { atomicAdd(ghist + NBR + req_br, 1); atomicAdd(ghist + 3 * NBR + req_br, 1); }
                }
            }
        }
        SEC(4);  // statistics at provision
        if (NET)
            group_link_stats<W, FULL, !LEAN, DEFER, DEFER ? 1 : 0, true, LANE_SUMS, LEAN>(lane, occ, lst, lint, tb, S, E, rec->link, accepted ? hops : 0,
                                                                           current_time, sum_span, sum_gaps, comp_cur, sum_sh,
                                                                           (double)sum_bitrate_running, g_thr, g_comp, g_lu, llog,
                                                                           &need_replay, lsum, a_slot, n);
        if constexpr (LEAN) {
            // _update_network_stats (rmsa_env.py:537-560) of an accepted row, logged: what it consumes, as the pass above left it
            const bool logs = accepted && hops > 0;
            OrlgGraphEntry ne;
            // (LANE_SUMS: the step's one join of the two partial sums over the row)
            orlg_glog_pack(ne, current_time, sum_bitrate_running, LANE_SUMS ? row_add_i32(sum_span) : sum_span, sum_sh,
                           LANE_SUMS ? row_add_i32(sum_gaps) : sum_gaps);
            if (logs && gl == lg_cnt) lg = ne;
            lg_cnt += logs ? 1 : 0;
            if (ballot(lg_cnt >= ORLG_GLOG_CAP) != 0ull) {   // a row's log is full: every row works its log off
                SEC(15);  // graph replay
                group_graph_replay(lane, lg, lg_cnt, p.scal + env, E);
                vm_drain();   // a cold block ends drained: the hot path it rejoins then needs no wait for this block's loads
            }
        }
        SEC(5);  // queue insert
        {
            // ---- _add_release (optical_network_env.py:178-189): the new entry goes behind every entry that is not later, and the
            // ring makes room from the nearer end -- each row its own.  A row whose entry is not earlier than its middle one scans
            // from the top: chunks of 16 entries anchored at the last one (entries q_n - 16 .. q_n - 1, then sixteen lower each
            // time; the partial chunk is the one at the head), the later entries move up one slot.  A row whose entry is earlier
            // scans from the head upward: the entries that are not later move DOWN one slot, and so does the head (q_head is the
            // head in LDS; the state that leaves has the conventional one, see the state store).  Either scan runs until it has
            // found the place: the side is a guess at the shorter way, nothing depends on it.  A chunk's reads precede its
            // writes.  The ring in HBM (one-step launches) keeps its head where the other kernel and the oracle have it: from
            // the top only
            const double rel = req_arrival + req_holding;
            bool ins = accepted && (act || !HBMQ);   // (a row past the batch's end must not touch the last environment's ring in HBM)
            if (ins && q_n >= Q) { q_overflow = 1; ins = false; }
            bool down = false;
            if constexpr (!HBMQ) {
                if (ins && q_n > 0) {
                    int pm = q_head + (q_n >> 1);
                    pm -= pm >= Q ? Q : 0;
                    down = rel < qtime[pm];
                }
            }
            // The lanes count from the near end: lane gl of a chunk looks at the gl-th entry of those not looked at yet, from the
            // top downward or from the head upward.  Sorted: the entries of a chunk that move are its near end
            bool found = !ins || q_n == 0;
            int m = q_n;       // how many entries move: all of them, unless the scan finds one that stays
            int left = q_n;    // entries not looked at yet
            int j = down ? gl : q_n - 1 - gl;
            int hd = down ? q_head - 1 : q_head + 1;   // where the head's entry goes if it moves: down, the new head
            hd = hd < 0 ? Q - 1 : (hd == Q ? 0 : hd);
            while (ballot(!found) != 0ull) {
                const bool scan = !found;
                const bool valid = scan && gl < left;
                int pos = q_head + j;
                pos -= pos >= Q ? Q : 0;
                double tq = 0.0;
                uint32_t dq = 0u;
                if (valid) { tq = qtime[pos]; dq = qdesc[pos]; }
                const bool moves = valid && (tq > rel) != down;   // up: the later ones; down: the ones that are not later
                int pos1 = hd + j;
                pos1 -= pos1 >= Q ? Q : 0;
                if (moves) { qtime[pos1] = tq; qdesc[pos1] = dq; }
                const uint32_t stay = row_ballot(valid && !moves, lane);
                if (scan) {
                    if (stay) { m = q_n - left + __builtin_ctz(stay); found = true; }
                    else if (left <= ORLG_GL) found = true;
                    else { left -= ORLG_GL; j += down ? ORLG_GL : -ORLG_GL; }
                }
            }
            if (ins) {
                const int r = down ? m : q_n - m;   // how many entries stay below the new one
                if (down) q_head = hd;
                int pr = q_head + r;
                pr -= pr >= Q ? Q : 0;
                const uint32_t desc = (uint32_t)gid | ((uint32_t)a_slot << 14) | ((uint32_t)req_br << 24);
                if (gl == 0) {
                    qtime[pr] = rel;
                    qdesc[pr] = desc;
                }
                q_n += 1;
                // the new head only if strictly earlier (then r = 0): an entry with the head's time goes behind it
                if (rel < next_rel) { next_rel = rel; next_desc = desc; }
            }
            wave_sync();
        }

        SEC(6);  // outputs
        // per-step outputs (first lane of the row)
        if (!LEAN && p.out_mask && act && gl == 0) {
            const size_t o = (size_t)(t0 + t) * p.B + env;
            const int om = p.out_mask;
            if (om & (1 << ORLG_OUT_PATH)) ORLG_GPTR(int32_t, tb.outs[ORLG_OUT_PATH])[o] = a_path;
            if (om & (1 << ORLG_OUT_SLOT)) ORLG_GPTR(int32_t, tb.outs[ORLG_OUT_SLOT])[o] = a_slot;
            if (om & (1 << ORLG_OUT_ACCEPTED)) ORLG_GPTR(uint8_t, tb.outs[ORLG_OUT_ACCEPTED])[o] = accepted ? 1 : 0;
            if (om & (1 << ORLG_OUT_REWARD))
                ORLG_GPTR(double, tb.outs[ORLG_OUT_REWARD])[o] =
                    p.reward_mode == 1 ? (accepted ? 1.0 : -1.0) : (accepted ? 1.0 : 0.0);
            if (om & (1 << ORLG_OUT_REQUEST))
                ORLG_GPTR(orlg_v4i, tb.outs[ORLG_OUT_REQUEST])[o] = orlg_v4i{req_sid, req_src, req_dst, br_val};
            if (om & (1 << ORLG_OUT_ARRIVAL)) ORLG_GPTR(double, tb.outs[ORLG_OUT_ARRIVAL])[o] = req_arrival;
            if (om & (1 << ORLG_OUT_HOLDING)) ORLG_GPTR(double, tb.outs[ORLG_OUT_HOLDING])[o] = req_holding;
            if (om & (1 << ORLG_OUT_COMPACT)) ORLG_GPTR(double, tb.outs[ORLG_OUT_COMPACT])[o] = comp_cur;
            if (om & (1 << ORLG_OUT_COMPACT_DIFF))
                ORLG_GPTR(double, tb.outs[ORLG_OUT_COMPACT_DIFF])[o] = prev_compact - comp_cur;
            if (FULL && (om & (1 << ORLG_OUT_AVG_LINK_COMPACT)))
                ORLG_GPTR(double, tb.outs[ORLG_OUT_AVG_LINK_COMPACT])[o] = np_mean(lst + 2 * E, E);
            if (FULL && (om & (1 << ORLG_OUT_AVG_LINK_UTIL)))
                ORLG_GPTR(double, tb.outs[ORLG_OUT_AVG_LINK_UTIL])[o] = np_mean(lst, E);
            if constexpr (CAUSE) {
                if (p.o_cause) ORLG_GPTR(uint8_t, p.o_cause)[o] = (uint8_t)cause;
            }
        }
        new_service = 0;

        // ============================================================== _next_service (rmsa_env.py:643-695)
        SEC(7);  // next arrival
        {
            // a row whose ring ran dry: the whole wave generates the next ORLG_RING arrivals of that environment
            bool dry = act && ring_cnt == 0;
            for (u64 m = ballot(dry); m; m = ballot(dry)) {
                SEC(8);  // refill
                const int src_lane = ctz64(m) & 48;
                const int env_s = __builtin_amdgcn_readlane(env, src_lane);
                int idx_s = __builtin_amdgcn_readlane(mt_idx, src_lane);
                if constexpr (TRACE) {
                    // (idx_s: the environment's cursor into its trace)
                    const int got = refill_requests_trace<false>(p.tr_arrival, p.tr_holding, p.tr_req, p.ring_iat + (size_t)env_s * ORLG_RING,
                                                                 p.ring_ht + (size_t)env_s * ORLG_RING, p.ring_req + (size_t)env_s * ORLG_RING,
                                                                 &idx_s, p.tr_len, env_s);
                    ring_visible();
                    if constexpr (DEFER) vm_drain();   // (a cold block ends drained)
                    if ((lane & 48) == src_lane) { ring_cnt = got; ring_pos = 0; mt_idx = idx_s; dry = false; }
                    continue;
                }
                // the MT19937 state travels HBM -> registers -> (lock) LDS -> registers (unlock) -> HBM: the workgroup's staging
                // buffer is held for the regeneration and the draws only, not for the HBM round trips
                // (the sequence is written out here and in orlg_phy_kernels.hip: as one shared function it changed 99 kernels' registers, orlg_requests.h)
                static_assert(ORLG_MT_N * 4 == 156 * 16, "MT19937 state = 156 rows of 16 bytes");
                const uint4 *g_mt = reinterpret_cast<const uint4 *>(p.mt + (size_t)env_s * ORLG_MT_N);
                uint4 *l_mt = reinterpret_cast<uint4 *>(mt_lds);
                uint4 m0 = g_mt[lane], m1 = g_mt[lane + 64], m2 = make_uint4(0u, 0u, 0u, 0u);
                if (lane < 156 - 128) m2 = g_mt[lane + 128];
                if (lane == 0) {
                    while (atomicCAS(mt_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(4);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                l_mt[lane] = m0; l_mt[lane + 64] = m1;
                if (lane < 156 - 128) l_mt[lane + 128] = m2;
                wave_sync();
                double arrival_lambda = p.arrival_lambda, holding_lambda = p.holding_lambda;
                if constexpr (TRAFFIC) orlg_env_rates(kernarg_params()->rates, env_s, arrival_lambda, holding_lambda);   // (the rates of env_s)
                const int got = (!LEAN && p.br_width > 0)   // bit_rate_selection="continuous"
                    ? refill_requests_cont<false>(mt_lds, p.ring_iat + (size_t)env_s * ORLG_RING, p.ring_ht + (size_t)env_s * ORLG_RING,
                                                  p.ring_req + (size_t)env_s * ORLG_RING, tb.src_cum, tb.dst_cum, &idx_s, N, p.br_width,
                                                  arrival_lambda, holding_lambda)
                    : refill_requests<false>(mt_lds, p.ring_iat + (size_t)env_s * ORLG_RING, p.ring_ht + (size_t)env_s * ORLG_RING,
                                             p.ring_req + (size_t)env_s * ORLG_RING, tb.src_cum, tb.dst_cum, tb.br_cum, &idx_s, N,
                                             NBR, arrival_lambda, holding_lambda, env_s);
                m0 = l_mt[lane]; m1 = l_mt[lane + 64];
                if (lane < 156 - 128) m2 = l_mt[lane + 128];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // this wave's reads of the buffer are done
                if (lane == 0) atomicExch(mt_lock, 0);
                uint4 *o_mt = reinterpret_cast<uint4 *>(p.mt + (size_t)env_s * ORLG_MT_N);
                o_mt[lane] = m0; o_mt[lane + 64] = m1;
                if (lane < 156 - 128) o_mt[lane + 128] = m2;
                ring_visible();
                if constexpr (DEFER) vm_drain();   // (a cold block ends drained)
                if ((lane & 48) == src_lane) { ring_cnt = got; ring_pos = 0; mt_idx = idx_s; dry = false; }
            }
            SEC(7);
            double r_iat = pf_iat, r_ht = pf_ht;
            uint32_t rq = pf_rq;
            if (!pf_ok) {
                const size_t ro = (size_t)env * ORLG_RING + ring_pos;
                r_iat = p.ring_iat[ro]; r_ht = p.ring_ht[ro]; rq = p.ring_req[ro];
                if constexpr (DEFER) vm_drain();   // (a cold block ends drained; these three are read at once anyway)
            }
            if (act) {
                const double at = TRACE ? r_iat : current_time + r_iat;   // (a trace's ring holds the arrival time itself)
                ring_pos += 1; ring_cnt -= 1;
                current_time = at;
                req_src = (int)(rq & 0xffu); req_dst = (int)((rq >> 8) & 0xffu); req_br = (int)(rq >> 16);
                req_base = tb.pair_base[req_src * N + req_dst];
                req_sid = eproc;
                new_service = 1;
                eproc += 1;
                req_arrival = at; req_holding = r_ht;
                if constexpr (LANE_HIST) {
                    br_one = lane_one(req_br);
                    h_req += br_one;
                } else {
                    const int bv = tb.bit_rates[req_br];
                    cnt += (cidx == 0 || cidx == 2) ? 1 : ((cidx == 4 || cidx == 6) ? bv : 0);
                    if constexpr (DEFER) {
                        if (gl == 0) { atomicAdd(hist_at(0, req_br), 1); atomicAdd(hist_at(2, req_br), 1); }
                    } else {
                        if (gl == 0) { atomicAdd(ghist + req_br, 1); atomicAdd(ghist + 2 * NBR + req_br, 1); }
                    }
                }
            }

            // ---- release every service with release time <= now, in time order (rmsa_env.py:689-695): the ring's head
            bool released = false;
            for (;;) {
                SEC(9);  // release scan
                const bool rel_now = act && next_rel <= current_time;
                if (ballot(rel_now) == 0ull) break;
                SEC(10);  // release apply
                if constexpr (DEFER) {
                    // ---- _release_path (rmsa_env.py:515-535), for the head A and -- in the same pass -- for the entry B behind it
                    // where B is due as well, both paths have at most 8 hops and they share no link: the two releases then touch
                    // disjoint occupancy words, summaries, span-cache entries and link logs at one `current_time`, and what joins
                    // them are integer sums, so the order between them leaves no trace.  Lanes 0..7 of the row take A's hops, lanes
                    // 8..15 B's.  Anything else -- a shared link, a longer path, a third due service -- waits for the next pass.
                    //
                    // Four passes of ten have no due B in any row, so the wave votes once and such a pass
                    // takes the PLAIN prelude: every lane of a row serves A, its place in the row is its hop, one entry leaves the
                    // ring -- no link masks, no trade between the halves.  A's descriptor is in a register when the pass begins,
                    // so A's 16-byte record is asked for first, next to B's ring entry, and waits for no compare; the plain
                    // prelude takes hops, se and the lane's link from that register copy.  The preludes hand ONE
                    // group_release_links its arguments, the lane's link among them.
                    // (slots outside the ring's live part were never written: B is read only where it exists)
                    const uint32_t d_a = rel_now ? next_desc : 0u;   // (the head's descriptor came with its time)
                    const uint4 rec_a = *reinterpret_cast<const uint4 *>(tb.recs + (int)(d_a & 0x3fff));
                    double b_rel = INF;
                    uint32_t b_desc = 0u;
                    if (rel_now && q_n >= 2) {
                        const int qb = q_head + 1 == Q ? 0 : q_head + 1;
                        b_rel = qtime[qb]; b_desc = qdesc[qb];
                    }
                    const bool b_due = b_rel <= current_time;   // (false in a row that releases nothing: idle rows do not vote)
                    const int bri_a = (int)(d_a >> 24);
                    // what the pass does, per lane: hop `r_hop` of `r_hops` over `r_link`, window [r_s, r_s + r_n); per row: the
                    // entries that leave the ring and what leaves the running sums with them
                    int r_link, r_hop, r_hops, r_s, r_n, pops, br_out, sh_out;
                    if (ballot(b_due) == 0ull) {
                        // ---- no row has a due B: A alone on the whole row (lanes 8..15 matter to a path of more than 8 hops only)
                        r_hops = rel_now ? (int)(rec_a.x & 0xffu) : 0;
                        r_n = tb.nslots[bri_a * ORLG_NSLOT_STRIDE + (int)((rec_a.x >> 8) & 0xffu)];
                        br_out = tb.bit_rates[bri_a];
                        r_link = group_rec_byte(rec_a, (gl + 2) & 15);   // (lanes 14, 15: no hop of any path, never used)
                        r_hop = gl;
                        r_s = (int)((d_a >> 14) & 0x3ff);
                        pops = 1;
                        sh_out = r_n * r_hops;
                    } else {
                        // ---- some row may release two: lanes 0..7 of a row take A's hops, lanes 8..15 B's
                        const bool up = gl >= 8;
                        // the lane's service: its descriptor, path record, window and hop count (the record byte by byte: both
                        // records in registers and a select between them measured slower)
                        const bool mine = up ? b_due : rel_now;
                        const uint32_t d = up ? b_desc : d_a;   // (a B that is not due is a real entry: `mine` keeps its lanes off)
                        const int s0 = (int)((d >> 14) & 0x3ff), bri2 = (int)(d >> 24);
                        const int hop = gl & 7;
                        const OrlgPathRec *rec2 = tb.recs + (int)(d & 0x3fff);
                        const int hops2 = mine ? (int)rec2->hops : 0;
                        const int n2 = tb.nslots[bri2 * ORLG_NSLOT_STRIDE + rec2->se];
                        const int br2 = mine ? tb.bit_rates[bri2] : 0;
                        const int link2 = (int)rec2->link[hop];
                        // the links of each half as bits (link mod 64): exact up to 64 links, beyond them a false conflict costs
                        // one pass and nothing else
                        const u64 lbits = half_row_or_u64(hop < hops2 ? 1ull << (link2 & 63) : 0ull);
                        const u64 obits = ((u64)(uint32_t)row_swap8_i32((int)(uint32_t)(lbits >> 32)) << 32) | (uint32_t)row_swap8_i32((int)(uint32_t)lbits);
                        const int hops_o = row_swap8_i32(hops2), n_o = row_swap8_i32(n2), br_o = row_swap8_i32(br2);   // the other half's
                        const bool pair = b_due && hops2 <= 8 && hops_o <= 8 && (lbits & obits) == 0ull;
                        // A alone: the whole row is A's, its upper lanes take A's link from the register copy
                        const bool a_up = up && !pair;
                        const int hops_a = up ? hops_o : hops2, n_a = up ? n_o : n2, br_a = up ? br_o : br2;
                        const int hops_b = up ? hops2 : hops_o, n_b = up ? n2 : n_o, br_b = up ? br2 : br_o;
                        r_link = a_up ? group_rec_byte(rec_a, (gl + 2) & 15) : link2;
                        r_hop = pair ? hop : gl;
                        r_hops = a_up ? hops_a : hops2;
                        r_s = a_up ? (int)((d_a >> 14) & 0x3ff) : s0;
                        r_n = a_up ? n_a : n2;
                        pops = pair ? 2 : 1;
                        br_out = br_a + (pair ? br_b : 0);
                        sh_out = n_a * hops_a + (pair ? n_b * hops_b : 0);
                    }
                    if (rel_now) {
                        // (the ring in LDS leaves a popped slot as it is: the state store writes the (+inf, 0) of the slots that left)
                        q_head += pops;
                        q_head -= q_head >= Q ? Q : 0;
                        q_pops += pops;
                        q_n -= pops;
                        n_running -= pops;
                        sum_bitrate_running -= br_out;
                        sum_sh -= sh_out;
                        released = true;
                        next_rel = q_n > 0 ? qtime[q_head] : INF;   // the next entry
                        next_desc = q_n > 0 ? qdesc[q_head] : 0u;
                    }
                    // the window and its links' statistics in one pass, lane = hop (group_release_links; ends with a wave_sync)
                    group_release_links<W, LANE_SUMS>(lane, occ, lsum, lint, S, r_link, r_hop, r_hops, r_s, r_n, current_time, sum_span, sum_gaps,
                                           llog, need_replay);
                    SEC(11);  // statistics at release: the log replays only
                } else {
                    // ---- _release_path (rmsa_env.py:515-535)
                    const uint32_t d = rel_now ? next_desc : 0u;   // (the head's descriptor came with its time)
                    const int gid2 = (int)(d & 0x3fff), s0 = (int)((d >> 14) & 0x3ff), bri2 = (int)(d >> 24);
                    const OrlgPathRec *rec2 = tb.recs + gid2;
                    const int hops2 = rec2->hops;
                    const int n2 = tb.nslots[bri2 * ORLG_NSLOT_STRIDE + rec2->se];
                    if (rel_now) {
                        // (the ring in LDS leaves a popped slot as it is: the state store writes the (+inf, 0) of the slots that left)
                        if (HBMQ && gl == 0) { qtime[q_head] = INF; qdesc[q_head] = 0u; }
                        q_head = q_head + 1 == Q ? 0 : q_head + 1;
                        q_pops += 1;
                        q_n -= 1;
                        n_running -= 1;
                        sum_bitrate_running -= tb.bit_rates[bri2];
                        sum_sh -= n2 * hops2;
                        released = true;
                    }
                    group_apply_window<W>(lane, occ, rec2->link, rel_now ? hops2 : 0, s0, n2, true);   // (ends with a wave_sync)
                    if (rel_now) {   // the next entry
                        next_rel = q_n > 0 ? qtime[q_head] : INF;
                        next_desc = q_n > 0 ? qdesc[q_head] : 0u;
                    }
                    SEC(11);  // statistics at release
                    if (NET)
                        group_link_stats<W, FULL, false, DEFER>(lane, occ, lst, lint, tb, S, E, rec2->link, rel_now ? hops2 : 0,
                                                                current_time, sum_span, sum_gaps, comp_cur, sum_sh, 0.0, g_thr, g_comp,
                                                                g_lu, llog, &need_replay);
                }
                if (DEFER && ballot(need_replay) != 0ull) {   // (a link's log never grows past ORLG_LLOG_FLUSH + 1 entries)
                    SEC(14);  // link replay
                    group_link_replay(lane, lst, lint, tb, S, E, llog);
                    vm_drain();   // (a cold block ends drained: without it the release loop's head waits on every pass)
                    need_replay = false;
                    SEC(11);
                }
            }
            if (NET && out_comp && released) comp_cur = network_compactness(sum_span, sum_sh, sum_gaps, E);
        }

        if (DEFER && ballot(need_replay) != 0ull) {   // a link's log is filling up: every row works its logs off
            SEC(14);  // link replay
            group_link_replay(lane, lst, lint, tb, S, E, llog);
            vm_drain();   // (a cold block ends drained)
            need_replay = false;
        }
        // ============================================================== done / episode reset
        SEC(12);
        {
            const bool done = act && eproc == p.episode_length;
            if (!LEAN && act && gl == 0 && (p.out_mask & (1 << ORLG_OUT_DONE)))
                ORLG_GPTR(uint8_t, tb.outs[ORLG_OUT_DONE])[(size_t)(t0 + t) * p.B + env] = done ? 1 : 0;
            if (ballot(done && p.auto_reset)) {
                // reset(only_episode_counters=True) with a pending service (rmsa_env.py:343-389)
                // (LANE_HIST: what the lanes hold of the episode that ends goes to the histograms before they are zeroed, and the
                // flush leaves the episode counters as the statements below leave `cnt`)
                if constexpr (LANE_HIST) books_flush(done && p.auto_reset, true);
                if (done && p.auto_reset) {
                    if constexpr (LANE_HIST) {
                        const uint32_t row = cold_row();
                        for (int i = gl; i < NBR; i += ORLG_GL) { atomicExch(hist_lean(row, 2, i), 0); atomicExch(hist_lean(row, 3, i), 0); }
                    } else if constexpr (DEFER) {
                        for (int i = gl; i < NBR; i += ORLG_GL) { atomicExch(hist_at(2, i), 0); atomicExch(hist_at(3, i), 0); }
                    } else {
                        for (int i = gl; i < NBR; i += ORLG_GL) { atomicExch(ghist + 2 * NBR + i, 0); atomicExch(ghist + 3 * NBR + i, 0); }
                    }
                    eproc = 1;
                    episodes_done += 1;
                    if constexpr (!LANE_HIST) {
                        const int bv = tb.bit_rates[req_br];
                        if (cidx == 2) cnt = 1;
                        if (cidx == 3 || cidx == 7) cnt = 0;
                        if (cidx == 6) cnt = bv;
                    }
                }
                wave_sync();
                if constexpr (LANE_HIST) {
                    if (done && p.auto_reset && gl == 0) atomicExch(hist_lean(cold_row(), 2, req_br), 1);
                } else if constexpr (DEFER) {
                    if (done && p.auto_reset && gl == 0) atomicExch(hist_at(2, req_br), 1);
                } else {
                    if (done && p.auto_reset && gl == 0) atomicExch(ghist + 2 * NBR + req_br, 1);
                }
                wave_sync();
                if constexpr (LANE_HIST) vm_drain();   // (a cold block ends drained: the flush loaded the counters)
            }
        }
        if constexpr (LANE_HIST) {
            // a field of the accumulators grows by at most one a step: a ticket of very many steps flushes in time (wave-uniform)
            static_assert(ORLG_LEAN_FLUSH_STEPS < 0x10000 && (ORLG_LEAN_FLUSH_STEPS & (ORLG_LEAN_FLUSH_STEPS - 1)) == 0, "16-bit fields");
            if ((t & (ORLG_LEAN_FLUSH_STEPS - 1)) == ORLG_LEAN_FLUSH_STEPS - 1) {
                books_flush(act, false);
                vm_drain();
            }
        }
    }

    SEC(14);  // link replay
    if (DEFER) group_link_replay(lane, lst, lint, tb, S, E, llog);   // (the state that leaves carries no pending updates)
    if constexpr (LEAN) {
        // ... and no pending graph statistics: the next chunk of the quad may go to another wave
        SEC(15);  // graph replay
        if (ballot(lg_cnt > 0) != 0ull) group_graph_replay(lane, lg, lg_cnt, p.scal + env, E);
    }
    // ... and nothing on the lanes: the histograms and the counters complete, the two sums joined (the atomics and the stores are
    // covered by the wait and the release below, as the state's are)
    if constexpr (LANE_HIST) books_flush(act, false);
    [[maybe_unused]] const int span_row = LANE_SUMS ? row_add_i32(sum_span) : sum_span, gaps_row = LANE_SUMS ? row_add_i32(sum_gaps) : sum_gaps;
    // ------------------------------------------------------------------ LDS -> HBM
    SEC(13);  // state store
    wave_sync();
    {
        const int env0 = quad * ORLG_GE;
        const int nact = p.B - env0 < ORLG_GE ? p.B - env0 : ORLG_GE;
        quad_copy(p.occ + (size_t)env0 * NW, wbase + p.g_occ, nact * NW * 8, lane);
        if (FULL && !DEFER) quad_copy(p.lstat + (size_t)env0 * 4 * E, wbase + p.g_lstat, nact * 4 * E * 8, lane);
        if (NET) quad_copy(p.lint + (size_t)env0 * p.lint_stride, wbase + p.g_lint, nact * p.lint_stride * 4, lane);
    }
    if constexpr (CAUSE) {
        // (the chunks of a quad's launch may run on different waves: every ticket adds its counts, atomics without return)
        if (act && gl < ORLG_NUM_CAUSES && cause_cnt && p.o_cause_counts) atomicAdd(p.o_cause_counts + (size_t)env * ORLG_NUM_CAUSES + gl, cause_cnt);
    }
    if (act) {
        int q_headc = q_head;   // the head the state has
        if constexpr (!HBMQ) {
            // the ring from where its head was at the start to its last entry: (+inf, 0) in the slots popped since then, the live
            // entries behind them; the number of pops, not the head's distance modulo Q, says how far that is: a head that went
            // round the ring has emptied slots beyond (q_head - q_head0) % Q + q_n whose old entries HBM would otherwise keep.
            // HBM has the CONVENTIONAL ring, whose head moves by pops only (q_head0 + q_pops): the ring in LDS is the same
            // sorted sequence, rotated down by the ticket's downward inserts -- entry i of it goes from q_head + i to
            // q_headc + i, and a slot of the span that holds no entry is one that was popped
            double *gqt = p.qtime + (size_t)env * Q;
            uint32_t *gqd = p.qdesc + (size_t)env * Q;
            q_headc = q_head0 + (int)((uint32_t)q_pops % (uint32_t)Q);
            q_headc -= q_headc >= Q ? Q : 0;
            int span = q_pops + q_n;
            span = span > Q ? Q : span;
            for (int j = gl; j < span; j += ORLG_GL) {
                int pos = q_head0 + j;
                pos -= pos >= Q ? Q : 0;
                int i = pos - q_headc;
                i += i < 0 ? Q : 0;
                int src = q_head + i;
                src -= src >= Q ? Q : 0;
                double tq = INF;
                uint32_t dq = 0u;
                if (i < q_n) { tq = qtime[src]; dq = qdesc[src]; }
                gqt[pos] = tq; gqd[pos] = dq;
            }
        }
        OrlgEnvScalars *go = p.scal + env;
        if constexpr (!LANE_HIST) {   // (LANE_HIST: the record has them, books_flush)
            if (gl < 8) go->c[gl] = cnt;
        }
        if (gl == 8) {
            go->current_time = current_time;
            go->req_arrival = req_arrival; go->req_holding = req_holding;
            if (!LEAN) { go->g_throughput = g_thr; go->g_compactness = g_comp; go->g_last_update = g_lu; }   // (LEAN: group_graph_replay's)
            go->sum_bitrate_running = sum_bitrate_running;
            go->episodes_done = episodes_done;
            go->sum_slots_hops = sum_sh; go->n_running = n_running;
            go->req_src = req_src; go->req_dst = req_dst; go->req_br = req_br; go->req_sid = req_sid;
            go->mt_idx = mt_idx; go->new_service = new_service; go->q_overflow = q_overflow;
            go->ring_pos = ring_pos; go->ring_cnt = ring_cnt;
            go->sum_span = span_row; go->sum_gaps = gaps_row; go->q_head = q_headc;
            if (q_overflow) *p.err_flag = 1;   // reported by the next entry point that waits for the stream
        }
    }
    wave_sync();
    if (n_chunks > 1) {
        // publish: this wave's stores complete, the XCD's L2 written back, then the flag (the explicit waits: the compiler may
        // drop the one behind the release)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(p.progress + quad, (uint32_t)(chunk + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    SEC(0);
    }  // work queue
    SEC_FLUSH;

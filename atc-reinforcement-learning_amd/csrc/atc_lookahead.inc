// atc_lookahead.inc — k_lookahead: the what-if query of include/atc_step.h (atc_lookahead).  Included by atc_step.hip behind the step
// kernels: it is k_skip's loop (step_part_a / step_part_b<SKIP>, the same four accumulators) run for M candidate action blocks from
// the SAME state, with every store to atc_state_t compiled out (the RO flag of the two step halves) and one small set of verdicts
// stored per (candidate, env).
//   Mapping: one lane per aircraft slot, W lanes per env, 256 slots per workgroup, like k_skip.  A workgroup serves ONE tile of 256
//   slots and `cpg` consecutive candidates of it (candidates per group, a launch argument: 1 = one workgroup per (tile, candidate),
//   M = one workgroup per tile that loops over all candidates); for each candidate it loads the tile's state again — 10 KB that the
//   first candidate brought into the L2 of this workgroup's XCD and that nothing writes — decodes that candidate's actions and runs
//   the step loop.  The workgroups of a tile are numbered so that they land on ONE XCD, next to each other in dispatch order
//   (look_tile): a tile's state lines come from HBM once, whatever cpg is.  Which cpg ships, and what the other costs: DESIGN.md §3c.
//   WIDE headings (include/atc_step.h, ABI 19) are handed from step to step through the side record in memory, which this kernel
//   may not write: an env-candidate in which a heading or an accepted heading target is saturated — at load, or after the first half
//   of any step — is marked "not evaluated" (`nev`), takes its last step there and stores zeros.  Its lanes compute on whatever the
//   unwritten side record holds until then; nothing of that is stored.
//   FULL: flags, ac_reward, min_sep or obs is requested (each a run-time null test); the fast form compiles all four out, and with
//   them the group minimum and the observation's normalisation (dead once nothing reads StepVals::o).
//   ARGUMENTS: `out` carries obs, reward, ac_reward, done, flags, min_sep of atc_lookahead_out_t, the other fields null.  The step halves
//   re-read st, out and q from the kernarg segment by StepArgs offsets: the static_assert behind the kernel holds its own parameter list
//   (KernArgs, atc_kernarg.h) to them.

// Workgroup id -> (tile, candidate group).  Workgroups are dealt round-robin to the 8 XCDs, so ids are laid out in chunks of
// 8 tiles x `groups`: id = (chunk * groups + g) * 8 + j serves tile 8 chunk + j — every group of a tile has the same id mod 8 (one
// XCD, one L2) and the groups of a tile are `8` ids apart (dispatched together).  Ids past the last tile (the last chunk's padding)
// leave at once.
__device__ __forceinline__ bool look_tile(int groups, int tiles, uint32_t* tile, int* g) {
    const uint32_t id = blockIdx.x, j = id & 7u, cg = id >> 3;
    const uint32_t chunk = cg / (uint32_t)groups;
    *g = (int)(cg - chunk * (uint32_t)groups);
    *tile = chunk * 8u + j;
    return *tile < (uint32_t)tiles;
}

template <int W, bool FULL>
__global__ void __launch_bounds__(kBlock, ATC_SKIP_WAVES)
k_lookahead(const float* __restrict__ blob, int off_grid, int B, int N, int K_steps, int M, atc_state_t st,
            const float* __restrict__ actions, atc_out_t out, atc_params_t p, StepDerived q, uint8_t* n_steps, int cpg, int groups, int tiles) {
    constexpr bool ONE = false, LAT = false;   // (QGET: the multi-step form — kernarg re-reads inside the step)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* pos = reinterpret_cast<float4*>(smem);                    // [2 kBlock] pair-scan staging (W >= 32)
    float* obs_stage = smem + (W >= 32 ? 2 * kBlock * 4 : 0);  // [4 waves][64 x 10] obs transpose
    const float* __restrict__ K = blob;
    const float* __restrict__ grid = off_grid ? blob + off_grid : nullptr;
    uint32_t tile;
    int grp;
    if (!look_tile(groups, tiles, &tile, &grp)) return;
    const LaneIds d = make_ids<W, false>(tile * kBlock, B, N);
    const size_t BN = (size_t)(uint32_t)B * (uint32_t)N;
    const int m_end = min(M, (grp + 1) * cpg);
    for (int m = grp * cpg; m < m_end; ++m) {
        // ---- the env's state, read only: the same loads as k_skip's (a later candidate finds the lines in L2) ----------------
        const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
        const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
        EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
        const int4 ps = *at<int4>(st.ac, d.i * 16u);
        const double h0 = *at<double>(st.alt, d.i * 8u);
        const Float3 act = *at<Float3>(actions + (size_t)m * BN * 3u, times12(d.i));   // candidate m's block
        const int4 la0 = *at<int4>(st.last_act, d.i * 16u);
        LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};

        Targets tg = {0u, 0.0f, 0};
        uint64_t refused_blk = 0ull;
        bool refused_known = false;
        bool all_active = false, mask_dirty = true;
        QRates qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
        settle_state(ls, es);
        float sum_r = 0.0f, sum_env = 0.0f, min_d2 = 1e30f;
        uint32_t or_fl = 0u;
        uint64_t live = __builtin_amdgcn_ballot_w64(d.env_valid);   // lanes of envs that have not taken their last step (uniform per env)
        // lanes of envs that are not evaluated (uniform per env): a WIDE heading or heading target, here at load
        uint64_t nev = 0ull;
        {
            const bool wide = d.lane_valid && (is_wide(ls.a.phi) || is_wide(ls.la_p));
            if (ATC_RARE(__builtin_amdgcn_ballot_w64(wide) != 0ull)) nev = __builtin_amdgcn_ballot_w64(group_ballot<W>(wide, d.lane) != 0ull);
        }
        for (int step = 0; live != 0ull; ++step) {
            LaneIds dl = d;
            const bool lane_live = ((live >> d.lane) & 1ull) != 0ull;
            dl.env_valid = lane_live;
            dl.lane_valid = d.lane_valid && lane_live;
            atc_params_t pl = p;
            const int zk = opaque_zero();   // this step's opaque zero (see k_step)
            pl.mode += (uint32_t)zk;
            const StepOut so = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // (nothing is stored per step)
            const QRates qr = qr_next;
            const QScan qs = QGET(s);
            if (ATC_RARE(step == 0)) tg = decode_targets(qr, act);
            const bool repeated = step != 0;
            if (ATC_RARE(mask_dirty)) {
                all_active = (__builtin_amdgcn_ballot_w64(!(dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u))) |
                              __builtin_amdgcn_ballot_w64(max(ls.a.phi, ls.la_p) == INT32_MAX) | __builtin_amdgcn_ballot_w64(min(ls.a.phi, ls.la_p) == INT32_MIN)) == 0ull;
                mask_dirty = false;
            }
            const Mid mid = step_part_a<false, false, false, true>(grid, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es, repeated,
                                                                   all_active, st.phi_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(nullptr));
            refused_known = true;
            // a heading or an accepted heading target that this step saturated: the step would have written the side record
            {
                const bool wide = dl.lane_valid && (max(ls.a.phi, ls.la_p) == INT32_MAX || min(ls.a.phi, ls.la_p) == INT32_MIN);
                if (ATC_RARE(__builtin_amdgcn_ballot_w64(wide) != 0ull)) nev |= __builtin_amdgcn_ballot_w64(group_ballot<W>(wide, d.lane) != 0ull);
            }
            StepVals sv;
            Float3 nxt = act;
            int scan_skip = 0;
            uint32_t scan_mask = 0u;
            const bool quiet = step_part_b<W, FULL, false, false, false, true, true>(K, grid, pl, q, qs, zk, N, dl, mid, ls, es, so, st.stats, st.phi_wide, pos, obs_stage,
                                                                                      nullptr, nxt, qr_next, scan_skip, scan_mask, nullptr, nullptr, &sv);
            if (ATC_RARE(!quiet)) mask_dirty = true;
            // acc = r1; acc = acc + r2; ...  (the first step assigns: 0 + r would turn a -0 into +0)
            sum_r = repeated ? sum_r + sv.r : sv.r;
            sum_env = repeated ? sum_env + sv.env_r : sv.env_r;
            or_fl |= sv.fl;
            if (FULL) min_d2 = fminf(min_d2, sv.min_d2);
            // envs that have just taken their last step: done, the block's K-th, or not evaluated
            const uint64_t fin = (step + 1 >= K_steps) ? live : (live & (__builtin_amdgcn_ballot_w64(sv.done) | nev));
            if (fin != 0ull) {
                LaneIds df = d;
                const bool mine = ((fin >> d.lane) & 1ull) != 0ull;
                df.env_valid = mine;
                df.lane_valid = d.lane_valid && mine;
                df.wave_full = d.wave_full && fin == ~0ull;
                bool done = sv.done;
                int n = step + 1;
                float ms = (min_d2 >= 1e30f) ? 1e30f : sqrtf(min_d2);
                if (ATC_RARE((fin & nev) != 0ull)) {   // not evaluated: every word of this (candidate, env) is zero
                    const bool zero = ((nev >> d.lane) & 1ull) != 0ull;
#pragma unroll
                    for (int c = 0; c < ATC_OBS_DIM; ++c) sv.o[c] = zero ? 0.0f : sv.o[c];
                    sum_r = zero ? 0.0f : sum_r;
                    sum_env = zero ? 0.0f : sum_env;
                    or_fl = zero ? 0u : or_fl;
                    ms = zero ? 0.0f : ms;
                    done = done && !zero;
                    n = zero ? 0 : n;
                }
                const atc_out_t o_end = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), opaque_zero());
                const size_t mB = (size_t)m * (uint32_t)B, mBN = (size_t)m * BN;   // candidate m's rows of the [M][...] outputs
                if (FULL && o_end.obs) store_obs_rows(o_end.obs + mBN * ATC_OBS_DIM, df, sv.o, obs_stage);
                if (FULL && df.lane_valid) {
                    if (o_end.flags) stream_store(at<uint16_t>(o_end.flags + mBN, d.i * 2u), (uint16_t)or_fl);
                    if (o_end.ac_reward) *at<float>(o_end.ac_reward + mBN, d.i * 4u) = sum_r;
                }
                if (mine && d.k == 0) {
                    *at<float>(o_end.reward + mB, (uint32_t)d.e * 4u) = sum_env;
                    *at<uint8_t>(o_end.done + mB, (uint32_t)d.e) = done ? 1 : 0;
                    if (FULL && o_end.min_sep) *at<float>(o_end.min_sep + mB, (uint32_t)d.e * 4u) = ms;
                    if (n_steps) *at<uint8_t>(n_steps + mB, (uint32_t)d.e) = (uint8_t)n;
                }
                live &= ~fin;
            }
        }
    }
}
static_assert(kernargs_like_step<decltype(k_lookahead<1, false>)>(), ATC_KERNARGS_REFUSAL);

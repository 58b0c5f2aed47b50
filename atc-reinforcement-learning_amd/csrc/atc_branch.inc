// atc_branch.inc — k_branch (atc_branch) and k_select (atc_state_select) of include/atc_step.h.  Included by atc_step.hip behind the
// look-ahead kernels.
//   k_branch is k_lookahead with the states KEPT: the same tile / candidate-group mapping (look_tile, cpg), the same read-only loads of
//   the source env, k_skip's step loop — and every (candidate m, env e) stores its state into child env m B + e of a second batch at its
//   last executed step, where k_skip stores its own.  The step halves run WITHOUT the read-only flag: the per-episode record update of an
//   auto-reset and the side-record stores of WIDE headings go to the CHILD's rows.  Both are addressed by the source env id (the reset
//   draws are keyed by it, include/atc_step.h), so the halves are handed the child batch's stats / phi_wide bases advanced by m B envs
//   (NB, "named bases": a kernarg re-read cannot carry a per-candidate base).  The child's per-episode record must hold the source's
//   before the first step that can reset: it is copied at load.
//   WIDE headings follow the look-ahead's rule: an env-candidate with a saturated heading or heading target — at load, or after the
//   first half of any step — is "not evaluated" (`nev`).  Its lanes run the rest of that step as lanes without an env (no reset, no
//   record update), its outputs are zeros, and its child rows are the SOURCE's, loaded again on that rare path (src is never written)
//   together with the side records of the source's saturated aircraft.
//   FULL is k_skip's: ac_reward or min_sep is requested (the per-aircraft reward sums, the value scan and the group minimum are compiled
//   out of the other form).  obs and flags are what a child env's bound outputs always hold, as atc_step_skip's required outputs: both
//   forms store them behind a run-time null test, like k_skip's fast form does — k_lookahead's FULL (any of the four) would send every
//   AtcVecEnv.branch through the heavy form (measured at 65 536 x 16, K = 4, M = 4: 420 us against 183 us without the two outputs).
//   ARGUMENTS: k_lookahead's, then `dst`, the CHILD batch of M B envs; `st` is the SOURCE batch, read only.  The step halves re-read st, out
//   and q from the kernarg segment by StepArgs offsets, and the kernel re-reads dst, its LAST parameter, at the offset its own parameter
//   list gives (KernArgs, atc_kernarg.h); the static_assert behind the kernel holds that list to StepArgs.

// candidate m's rows of a batch of M B envs: every array advanced by m B envs, so that the source's env and aircraft ids index them
__device__ __forceinline__ atc_state_t child_rows(const atc_state_t& dst, size_t mB, size_t mBN) {
    atc_state_t c;
    c.ac = dst.ac + mBN * 4u;
    c.alt = dst.alt + mBN;
    c.last_act = dst.last_act + mBN * 4u;
    c.env = dst.env + mB * ATC_ENV_WORDS;
    c.stats = dst.stats + mB * ATC_STAT_WORDS;
    c.phi_wide = dst.phi_wide + mBN * 4u;
    return c;
}

template <int W, bool FULL>
__global__ void __launch_bounds__(kBlock, ATC_SKIP_WAVES)
k_branch(const float* __restrict__ blob, int off_grid, int B, int N, int K_steps, int M, atc_state_t st,
         const float* __restrict__ actions, atc_out_t out, atc_params_t p, StepDerived q, uint8_t* n_steps, int cpg, int groups, int tiles,
         atc_state_t dst) {
    constexpr bool ONE = false, LAT = false;   // (QGET: the multi-step form — kernarg re-reads inside the step)
    constexpr size_t dst_off = KernArgs<decltype(k_branch<W, FULL>)>::last();   // where `dst` lies: re-read at an env's last step
    static_assert(ATC_STAT_WORDS == 8, "the per-episode record is copied as two 16-byte pieces");
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
        const size_t mB = (size_t)m * (uint32_t)B, mBN = (size_t)m * BN;   // candidate m's rows of the child batch and of the outputs
        // ---- the env's state, read only: k_lookahead's loads -----------------------------------------------------------------
        const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
        const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
        EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
        const int4 ps = *at<int4>(st.ac, d.i * 16u);
        const double h0 = *at<double>(st.alt, d.i * 8u);
        const Float3 act = *at<Float3>(actions + mBN * 3u, times12(d.i));   // candidate m's block
        const int4 la0 = *at<int4>(st.last_act, d.i * 16u);
        LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};
        // the child's bases as the step halves address them (by the source's ids), and its per-episode record = the source's
        int32_t* const ch_stats = dst.stats + mB * ATC_STAT_WORDS;
        double* const ch_wide = dst.phi_wide + mBN * 4u;
        if (d.env_valid && d.k == 0) {
            const int4* sr = at<int4>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u));
            const int4 s0 = sr[0], s1 = sr[1];
            int4* cr = at<int4>(ch_stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u));
            cr[0] = s0;
            cr[1] = s1;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (read again by every lane of the env on the auto-reset path: see step_part_b)

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
            // (an env that is not evaluated runs as lanes without an env: nothing of it reaches the child's records)
            const bool lane_live = (((live & ~nev) >> d.lane) & 1ull) != 0ull;
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
            const Mid mid = step_part_a<false, false, false, false, true>(grid, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es,
                                                                          repeated, all_active, ch_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(nullptr));
            refused_known = true;
            // a heading or an accepted heading target that this step saturated: from here the env is not evaluated
            {
                const bool wide = dl.lane_valid && (max(ls.a.phi, ls.la_p) == INT32_MAX || min(ls.a.phi, ls.la_p) == INT32_MIN);
                if (ATC_RARE(__builtin_amdgcn_ballot_w64(wide) != 0ull)) {
                    nev |= __builtin_amdgcn_ballot_w64(group_ballot<W>(wide, d.lane) != 0ull);
                    const bool ok = (((live & ~nev) >> d.lane) & 1ull) != 0ull;
                    dl.env_valid = ok;
                    dl.lane_valid = d.lane_valid && ok;
                }
            }
            StepVals sv;
            Float3 nxt = act;
            int scan_skip = 0;
            uint32_t scan_mask = 0u;
            const bool quiet = step_part_b<W, FULL, false, false, false, true, false, true>(K, grid, pl, q, qs, zk, N, dl, mid, ls, es, so, ch_stats, ch_wide, pos,
                                                                                             obs_stage, nullptr, nxt, qr_next, scan_skip, scan_mask, nullptr, nullptr, &sv);
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
                const int zs = opaque_zero();
                const atc_state_t ch = child_rows(kernarg_reread<atc_state_t>(dst_off, zs), mB, mBN);
                if (ATC_RARE((fin & nev) != 0ull)) {   // not evaluated: every output word of this (candidate, env) is zero ...
                    const bool zero = ((nev >> d.lane) & 1ull) != 0ull;
#pragma unroll
                    for (int c = 0; c < ATC_OBS_DIM; ++c) sv.o[c] = zero ? 0.0f : sv.o[c];
                    sum_r = zero ? 0.0f : sum_r;
                    sum_env = zero ? 0.0f : sum_env;
                    or_fl = zero ? 0u : or_fl;
                    ms = zero ? 0.0f : ms;
                    done = done && !zero;
                    n = zero ? 0 : n;
                    // ... and its child rows are the source's (the per-episode record already is: copied at load, never written since)
                    if (zero) {
                        const atc_state_t src = kernarg_reread<atc_state_t>(offsetof(StepArgs, st), zs);
                        const int4 re = *at<int4>(src.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
                        const int4 rp = *at<int4>(src.ac, d.i * 16u);
                        const double rh = *at<double>(src.alt, d.i * 8u);
                        const int4 rl = *at<int4>(src.last_act, d.i * 16u);
                        es = EnvState{re.x, re.y, __int_as_float(re.z), (uint64_t)(uint32_t)re.w | ((uint64_t)hi0 << 32)};
                        ls = LaneState{{rp.x, rp.y, rh, rp.z, (uint32_t)rp.w}, (uint32_t)rl.x, __hiloint2double(rl.w, rl.z), rl.y, false};
                        if (df.lane_valid && (is_wide(rp.z) || is_wide(rl.y))) {   // the side record of a saturated aircraft, whole
                            const int4* ws = at<int4>(src.phi_wide, d.i * 32u);
                            const int4 w0 = ws[0], w1 = ws[1];
                            int4* wd = at<int4>(ch.phi_wide, d.i * 32u);
                            wd[0] = w0;
                            wd[1] = w1;
                        }
                    }
                }
                const atc_out_t o_end = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), zs);
                if (o_end.obs) store_obs_rows(o_end.obs + mBN * ATC_OBS_DIM, df, sv.o, obs_stage);
                if (df.lane_valid) {
                    if (o_end.flags) stream_store(at<uint16_t>(o_end.flags + mBN, d.i * 2u), (uint16_t)or_fl);
                    if (FULL && o_end.ac_reward) *at<float>(o_end.ac_reward + mBN, d.i * 4u) = sum_r;
                }
                if (mine && d.k == 0) {
                    *at<float>(o_end.reward + mB, (uint32_t)d.e * 4u) = sum_env;
                    *at<uint8_t>(o_end.done + mB, (uint32_t)d.e) = done ? 1 : 0;
                    if (FULL && o_end.min_sep) *at<float>(o_end.min_sep + mB, (uint32_t)d.e * 4u) = ms;
                    if (n_steps) *at<uint8_t>(n_steps + mB, (uint32_t)d.e) = (uint8_t)n;
                }
                // the child's state: k_skip's stores, into candidate m's rows (the child starts from unwritten memory: the last-action
                // record is stored whether it changed or not)
                ls.la_changed = true;
                store_lane_state(ch, df, ls, true);
                store_env_state<W>(ch, df, es, hi0);
                live &= ~fin;
            }
        }
    }
}

static_assert(kernargs_like_step<decltype(k_branch<1, false>)>(), ATC_KERNARGS_REFUSAL);

// ---------------------------------------------------------------------------------------------------------------
// k_select (atc_state_select): dst env e takes src env index[e]'s rows — a gather of whole records, no arithmetic.  Flat mapping: one
// lane per aircraft slot of dst (e = slot / N, k = slot % N); the 16-byte aircraft and last-action records and the side record of a
// saturated aircraft move as 16-byte pieces, the altitude as its 8 bytes, and lane k == 0 moves the env's two records.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_select(int N, int B_dst, atc_state_t dst, int B_src, atc_state_t src, const int32_t* __restrict__ index, const uint8_t* __restrict__ mask) {
    const uint32_t slot = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (slot >= (uint32_t)B_dst * (uint32_t)N) return;
    const uint32_t e = slot / (uint32_t)N, k = slot - e * (uint32_t)N;
    if (mask && mask[e] == 0) return;
    const int32_t j = index[e];
    if (j < 0 || j >= B_src) return;
    const uint32_t is = (uint32_t)j * (uint32_t)N + k;   // (B N 40 < 4 GiB for both batches: 32-bit byte offsets)
    const int4 a = *at<int4>(src.ac, is * 16u);
    const double h = *at<double>(src.alt, is * 8u);
    const int4 la = *at<int4>(src.last_act, is * 16u);
    *at<int4>(dst.ac, slot * 16u) = a;
    *at<double>(dst.alt, slot * 8u) = h;
    *at<int4>(dst.last_act, slot * 16u) = la;
    if (is_wide(a.z) || is_wide(la.y)) {
        const int4* ws = at<int4>(src.phi_wide, is * 32u);
        const int4 w0 = ws[0], w1 = ws[1];
        int4* wd = at<int4>(dst.phi_wide, slot * 32u);
        wd[0] = w0;
        wd[1] = w1;
    }
    if (k == 0) {
        *at<int4>(dst.env, e * (ATC_ENV_WORDS * 4u)) = *at<int4>(src.env, (uint32_t)j * (ATC_ENV_WORDS * 4u));
        const int4* sr = at<int4>(src.stats, (uint32_t)j * (ATC_STAT_WORDS * 4u));
        const int4 s0 = sr[0], s1 = sr[1];
        int4* dr = at<int4>(dst.stats, e * (ATC_STAT_WORDS * 4u));
        dr[0] = s0;
        dr[1] = s1;
    }
}

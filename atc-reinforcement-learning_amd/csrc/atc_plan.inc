// atc_plan.inc — k_plan: the plan query of include/atc_step.h (atc_lookahead_plan).  Included by atc_step.hip behind atc_lookahead.inc:
// it is k_lookahead (same look_tile / cpg mapping, same read-only loads, same live / fin / nev masks, step_part_a / step_part_b with
// the RO flag) whose candidate is a SEQUENCE of H action blocks, each held for K steps — state, last-action record and counters stay
// in registers across the H segments, where a host chain of atc_step_skip calls stores and reloads them H times.
//   Segments.  Live envs advance in lockstep, so "this step is the last of its segment" is wave-uniform (`left`, counted down like
//   k_step's held blocks).  At a segment's end the kernel folds the segment's reward sums into the candidate's totals (two-level
//   sums, both sequential: what a host loop over atc_step_skip outputs computes), stores the segment's reward, takes the next block's
//   decoded targets and clears `repeated` / `refused_known`: the next step carries a fresh decision and does the action bookkeeping
//   against the record the previous segment left in registers.  `mask_dirty` is set too — a fresh atc_step_skip launch establishes
//   all_active at its first step.  flags, min_sep and the step count run on across segments.
//   The next block's 12 bytes per lane are requested inside the segment's last step (step_part_b's act_next, k_step's `nxt`), behind
//   the MVA gather and ahead of the scan: the boundary does not wait for memory.
//   An env that reports done (auto-reset or not), or that is not evaluated (WIDE, see k_lookahead), takes its last step there: a plan
//   never spans two episodes.  It stores its verdicts then, and zeros into the seg_reward words of the segments it did not run — for
//   a not-evaluated env also over those it did run (same lane, same address, later store).
//   FULL: as in k_lookahead.  seg_reward is a run-time null test in both forms.
//   ARGUMENTS: `out` carries obs, reward, ac_reward, done, flags, min_sep of atc_plan_out_t, the other fields null.  The step halves re-read
//   st, out and q from the kernarg segment by StepArgs offsets: the static_assert behind the kernel holds its own parameter list
//   (KernArgs, atc_kernarg.h) to them.

template <int W, bool FULL>
__global__ void __launch_bounds__(kBlock, ATC_SKIP_WAVES)
k_plan(const float* __restrict__ blob, int off_grid, int B, int N, int K_steps, int H, int M, atc_state_t st,
       const float* __restrict__ actions, atc_out_t out, atc_params_t p, StepDerived q, uint16_t* n_steps, float* seg_reward, int cpg,
       int groups, int tiles) {
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
        // ---- the env's state, read only: k_lookahead's loads (a later candidate finds the lines in L2) --------------------------
        const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
        const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
        EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
        const int4 ps = *at<int4>(st.ac, d.i * 16u);
        const double h0 = *at<double>(st.alt, d.i * 8u);
        const size_t mH = (size_t)m * (uint32_t)H;                                   // candidate m's first block / seg_reward row
        Float3 act = *at<Float3>(actions + mH * BN * 3u, times12(d.i));   // block 0 of candidate m
        const int4 la0 = *at<int4>(st.last_act, d.i * 16u);
        LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};

        Targets tg = {0u, 0.0f, 0};
        uint64_t refused_blk = 0ull;
        bool refused_known = false;
        bool all_active = false, mask_dirty = true;
        QRates qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
        settle_state(ls, es);
        float seg_r = 0.0f, seg_env = 0.0f;   // the running segment's sums (atc_step_skip's accumulators)
        float tot_r = 0.0f, tot_env = 0.0f;   // the sums of the finished segments' sums
        float min_d2 = 1e30f;
        uint32_t or_fl = 0u;
        int h = 0, left = K_steps;            // the running segment, and the steps it still has
        bool seg_start = true;                // this step is the first of its segment: a fresh decision
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
            if (ATC_RARE(step == 0)) tg = decode_targets(qr, act);   // (later blocks: decoded at the segment end below)
            const bool repeated = !seg_start;
            if (ATC_RARE(mask_dirty)) {
                all_active = (__builtin_amdgcn_ballot_w64(!(dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u))) |
                              __builtin_amdgcn_ballot_w64(max(ls.a.phi, ls.la_p) == INT32_MAX) | __builtin_amdgcn_ballot_w64(min(ls.a.phi, ls.la_p) == INT32_MIN)) == 0ull;
                mask_dirty = false;
            }
            const Mid mid = step_part_a<false, false, false, true>(grid, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es, repeated,
                                                                   all_active, st.phi_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(nullptr));
            refused_known = true;
            seg_start = false;
            // a heading or an accepted heading target that this step saturated: the step would have written the side record
            {
                const bool wide = dl.lane_valid && (max(ls.a.phi, ls.la_p) == INT32_MAX || min(ls.a.phi, ls.la_p) == INT32_MIN);
                if (ATC_RARE(__builtin_amdgcn_ballot_w64(wide) != 0ull)) nev |= __builtin_amdgcn_ballot_w64(group_ballot<W>(wide, d.lane) != 0ull);
            }
            // the segment's last step requests the next block (none behind the plan's last segment)
            const bool seg_end = --left == 0;
            const bool plan_end = seg_end && h + 1 >= H;
            const float* act_next = nullptr;
            if (ATC_RARE(seg_end && !plan_end)) act_next = actions + (mH + (uint32_t)(h + 1)) * BN * 3u;
            StepVals sv;
            Float3 nxt = act;
            int scan_skip = 0;
            uint32_t scan_mask = 0u;
            const bool quiet = step_part_b<W, FULL, false, false, false, true, true>(K, grid, pl, q, qs, zk, N, dl, mid, ls, es, so, st.stats, st.phi_wide, pos, obs_stage,
                                                                                      act_next, nxt, qr_next, scan_skip, scan_mask, nullptr, nullptr, &sv);
            if (ATC_RARE(!quiet)) mask_dirty = true;
            // acc = r1; acc = acc + r2; ...  (a segment's first step assigns: 0 + r would turn a -0 into +0)
            seg_r = repeated ? seg_r + sv.r : sv.r;
            seg_env = repeated ? seg_env + sv.env_r : sv.env_r;
            or_fl |= sv.fl;
            if (FULL) min_d2 = fminf(min_d2, sv.min_d2);
            // envs that have just taken their last step: done, the plan's last, or not evaluated
            const uint64_t fin = plan_end ? live : (live & (__builtin_amdgcn_ballot_w64(sv.done) | nev));
            if (ATC_RARE(seg_end || fin != 0ull)) {
                // the candidate's totals with this segment in: acc = r_0; acc = acc + r_1; ...
                const float te = h ? tot_env + seg_env : seg_env;
                const float tr = h ? tot_r + seg_r : seg_r;
                const bool zero = ((nev >> d.lane) & 1ull) != 0ull;   // (only read for lanes of `fin`: a live env is not in nev)
                const size_t hB = (mH + (uint32_t)h) * (uint32_t)B;    // row [m][h] of seg_reward
                // this segment's reward: at a segment's end for every live env, otherwise for the envs that stop inside it
                const uint64_t seg_mask = seg_end ? live : fin;
                if (seg_reward && ((seg_mask >> d.lane) & 1ull) != 0ull && d.k == 0)
                    *at<float>(seg_reward + hB, (uint32_t)d.e * 4u) = zero ? 0.0f : seg_env;
                if (fin != 0ull) {
                    LaneIds df = d;
                    const bool mine = ((fin >> d.lane) & 1ull) != 0ull;
                    df.env_valid = mine;
                    df.lane_valid = d.lane_valid && mine;
                    df.wave_full = d.wave_full && fin == ~0ull;
                    bool done = sv.done;
                    int n = step + 1;
                    float ms = (min_d2 >= 1e30f) ? 1e30f : sqrtf(min_d2);
                    float sum_env = te, sum_r = tr;
                    uint32_t fl_end = or_fl;
                    if (ATC_RARE((fin & nev) != 0ull)) {   // not evaluated: every word of this (candidate, env) is zero
#pragma unroll
                        for (int c = 0; c < ATC_OBS_DIM; ++c) sv.o[c] = zero ? 0.0f : sv.o[c];
                        sum_r = zero ? 0.0f : sum_r;
                        sum_env = zero ? 0.0f : sum_env;
                        fl_end = zero ? 0u : fl_end;
                        ms = zero ? 0.0f : ms;
                        done = done && !zero;
                        n = zero ? 0 : n;
                    }
                    const atc_out_t o_end = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), opaque_zero());
                    const size_t mB = (size_t)m * (uint32_t)B, mBN = (size_t)m * BN;   // candidate m's rows of the [M][...] outputs
                    if (FULL && o_end.obs) store_obs_rows(o_end.obs + mBN * ATC_OBS_DIM, df, sv.o, obs_stage);
                    if (FULL && df.lane_valid) {
                        if (o_end.flags) stream_store(at<uint16_t>(o_end.flags + mBN, d.i * 2u), (uint16_t)fl_end);
                        if (o_end.ac_reward) *at<float>(o_end.ac_reward + mBN, d.i * 4u) = sum_r;
                    }
                    if (mine && d.k == 0) {
                        *at<float>(o_end.reward + mB, (uint32_t)d.e * 4u) = sum_env;
                        *at<uint8_t>(o_end.done + mB, (uint32_t)d.e) = done ? 1 : 0;
                        if (FULL && o_end.min_sep) *at<float>(o_end.min_sep + mB, (uint32_t)d.e * 4u) = ms;
                        if (n_steps) *at<uint16_t>(n_steps + mB, (uint32_t)d.e * 2u) = (uint16_t)n;
                        if (seg_reward) {
                            // the segments this env did not run; a not-evaluated env also zeroes the ones it did
                            float* row0 = seg_reward + mH * (uint32_t)B;
                            for (int hh = 0; hh < H; ++hh)
                                if (hh > h || (zero && hh < h)) *at<float>(row0 + (size_t)hh * (uint32_t)B, (uint32_t)d.e * 4u) = 0.0f;
                        }
                    }
                    live &= ~fin;
                }
                if (seg_end) {   // the next step opens segment h + 1 with block h + 1 (requested above, waited for in step_part_b)
                    tot_env = te;
                    tot_r = tr;
                    ++h;
                    left = K_steps;
                    seg_start = true;
                    refused_known = false;
                    mask_dirty = true;
                    if (act_next) {
                        tg = decode_targets(QGET(r), nxt);
                        act = nxt;
                    }
                }
            }
        }
    }
}
static_assert(kernargs_like_step<decltype(k_plan<1, false>)>(), ATC_KERNARGS_REFUSAL);

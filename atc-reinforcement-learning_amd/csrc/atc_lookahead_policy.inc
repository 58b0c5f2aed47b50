// atc_lookahead_policy.inc — k_lookahead_policy: the closed-loop plan query of include/atc_step.h (atc_lookahead_policy).  Included by
// atc_step.hip behind atc_policy.inc, whose policy_decide it calls (and, through it, plan_draw_clamp of atc_plan_sampled.inc).
//   k_lookahead_policy is k_plan_sampled (csrc/atc_plan_sampled.inc) line for line — the tile / candidates-per-group mapping, the
//   read-only loads, the live / fin / nev masks, the two-level reward sums, the RO form of the two step halves — with the action block
//   DECIDED where k_plan_sampled draws it: a copy of the text, not a flag on k_plan_sampled or on rollout_policy_body (the precedent of
//   both: every other kernel keeps its machine code).  What differs:
//   - the decision of segment h is policy_decide<ATC_POLICY_IN> on the observation the segment's predecessor ended with.  As in the
//     rollout the ten words are carried over the loop's back edge and the decision stands at the TOP of a segment's first step, so that
//     segment 0 (which reads the lane's row of obs0) and every later one share ONE evaluation site: one copy of the MLP's code.  The
//     site is wave-uniform (a segment boundary is the same step for every env of a candidate) and rare (once per K steps).
//   - a lane whose env has taken its last step feeds zeros to the decision: its stale observation — the raw reset observation behind a
//     look-ahead reset — would otherwise switch the whole wavefront to the float64 form of layer 1.
//   - `first` (nullable) stands where k_plan_sampled has the mean rows: candidate m's block of segment 0, loaded where k_lookahead loads
//     its block; the policy then decides segments 1 .. H-1 with decision numbers decision0, decision0 + 1, ...
//   - the policy's terms ride in ONE struct behind the shared list and are re-read from the kernarg segment at the decision (the rollout's
//     PolicyTrafficTail pattern): nothing of them is carried across the step loop.
//   THE KEY: aircraft index (m B + e) N + k and decision number decision0 + (h - h0) — what atc_rollout_policy uses on the child batch
//   atc_branch / atc_state_select would make of the candidates (candidate m of env e = child env m B + e).  The host refuses M B N >= 2^32.
//   Every store is a plain vector store; there is no workgroup barrier beyond those of the step halves.

// The policy's terms: the last parameter of k_lookahead_policy, read by kernarg re-read where they are used
struct LookPolicyTail {
    const float* obs0;     // [B N 10]: what segment 0's decision sees (not read where `first` is given)
    const float* pw;       // atc_policy_t.w
    uint64_t seed;
    uint32_t decision0;
    uint32_t pflags;       // atc_policy_t.flags
    float* flown;          // [M][H][B N 3], nullable
    float* logp;           // [M][H][B N], nullable
};

// wavefronts per SIMD the kernel is register-budgeted for (<= 168 VGPRs): the rollout's three — the 64 hidden activations are live next
// to what the plan loop carries.  -DATC_LOOK_POLICY_WAVES=n: A/B builds.
#ifndef ATC_LOOK_POLICY_WAVES
#define ATC_LOOK_POLICY_WAVES 3
#endif

template <int W, bool FULL>
__global__ void __launch_bounds__(kBlock, ATC_LOOK_POLICY_WAVES)
k_lookahead_policy(const float* __restrict__ blob, int off_grid, int B, int N, int K_steps, int H, int M, atc_state_t st,
                   const float* __restrict__ first, atc_out_t out, atc_params_t p, StepDerived q, uint16_t* n_steps, float* seg_reward, int cpg,
                   int groups, int tiles, LookPolicyTail pt_arg) {
    constexpr bool ONE = false, LAT = false;   // (QGET: the multi-step form — kernarg re-reads inside the step)
    constexpr size_t PT_OFF = KernArgs<decltype(k_lookahead_policy<W, FULL>)>::last();   // (pt_arg: a kernarg re-read at the decision)
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
    const int h0 = first ? 1 : 0;              // the first segment the policy decides
    const int m_end = min(M, (grp + 1) * cpg);
    for (int m = grp * cpg; m < m_end; ++m) {
        // ---- the env's state, read only: k_lookahead's loads (a later candidate finds the lines in L2) --------------------------
        const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
        const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
        EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
        const int4 ps = *at<int4>(st.ac, d.i * 16u);
        const double alt0 = *at<double>(st.alt, d.i * 8u);
        const size_t mH = (size_t)m * (uint32_t)H;                                   // candidate m's seg_reward row
        // segment 0: candidate m's block of `first`, or — decided at the top of step 0 — the policy on the lane's row of obs0 (an idle
        // lane reads the last aircraft's row: in bounds, its decision is never stored)
        Float3 act = {0.0f, 0.0f, 0.0f};
        float x[ATC_OBS_DIM];
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) x[c] = 0.0f;
        if (first) {
            act = *at<Float3>(first + (size_t)m * BN * 3u, times12(d.i));
        } else {
            const float* obs0 = kernarg_reread<const float*>(PT_OFF + offsetof(LookPolicyTail, obs0), opaque_zero());
            const float2* r0 = at<float2>(obs0, times40(d.i));
#pragma unroll
            for (int c = 0; c < ATC_OBS_DIM / 2; ++c) {
                const float2 v = r0[c];
                x[2 * c] = v.x;
                x[2 * c + 1] = v.y;
            }
        }
        const int4 la0 = *at<int4>(st.last_act, d.i * 16u);
        LaneState ls = {{ps.x, ps.y, alt0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};

        Targets tg = {0u, 0.0f, 0};
        uint64_t refused_blk = 0ull;
        bool refused_known = false;
        bool all_active = false, mask_dirty = true;
        QRates qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
        settle_state(ls, es);
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) asm volatile("" : "+v"(x[c]));   // (waited for here, like the state: see settle_state)
        asm volatile("" : "+v"(act.a), "+v"(act.b), "+v"(act.c));
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
            const bool repeated = !seg_start;
            if (ATC_RARE(seg_start)) {   // the segment's block: decided here from what the step before stored (obs0 at step 0), or `first`
                const LookPolicyTail pt = kernarg_reread<LookPolicyTail>(PT_OFF, zk);
                const size_t row = (mH + (uint32_t)h) * BN;   // row [m][h] of flown and logp, in aircraft
                if (h >= h0) {
                    float xin[ATC_OBS_DIM];
#pragma unroll
                    for (int c = 0; c < ATC_OBS_DIM; ++c) xin[c] = dl.lane_valid ? x[c] : 0.0f;
                    const PolicyDecision dec = policy_decide<ATC_POLICY_IN>(pt.pw, zk, xin, pt.seed, pt.decision0 + (uint32_t)(h - h0), (uint32_t)((size_t)m * BN) + d.i,
                                                                            (pt.pflags & ATC_POLICY_DETERMINISTIC) != 0u);
                    act = dec.a;
                    if (pt.logp && dl.lane_valid) *at<float>(pt.logp + row, d.i * 4u) = dec.logp;
                }
                if (pt.flown && dl.lane_valid) *at<Float3>(pt.flown + row * 3u, times12(d.i)) = act;
                tg = decode_targets(qr, act);
            }
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
            const bool seg_end = --left == 0;
            const bool plan_end = seg_end && h + 1 >= H;
            StepVals sv;
            Float3 nxt = act;
            int scan_skip = 0;
            uint32_t scan_mask = 0u;
            const bool quiet = step_part_b<W, FULL, false, false, false, true, true>(K, grid, pl, q, qs, zk, N, dl, mid, ls, es, so, st.stats, st.phi_wide, pos, obs_stage,
                                                                                      nullptr, nxt, qr_next, scan_skip, scan_mask, nullptr, nullptr, &sv);
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
                    float o_fin[ATC_OBS_DIM];   // (a copy: sv.o itself goes on to the next decision)
#pragma unroll
                    for (int c = 0; c < ATC_OBS_DIM; ++c) o_fin[c] = sv.o[c];
                    if (ATC_RARE((fin & nev) != 0ull)) {   // not evaluated: every word of this (candidate, env) is zero
#pragma unroll
                        for (int c = 0; c < ATC_OBS_DIM; ++c) o_fin[c] = zero ? 0.0f : o_fin[c];
                        sum_r = zero ? 0.0f : sum_r;
                        sum_env = zero ? 0.0f : sum_env;
                        fl_end = zero ? 0u : fl_end;
                        ms = zero ? 0.0f : ms;
                        done = done && !zero;
                        n = zero ? 0 : n;
                    }
                    const atc_out_t o_end = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), opaque_zero());
                    const size_t mB = (size_t)m * (uint32_t)B, mBN = (size_t)m * BN;   // candidate m's rows of the [M][...] outputs
                    if (FULL && o_end.obs) store_obs_rows(o_end.obs + mBN * ATC_OBS_DIM, df, o_fin, obs_stage);
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
                if (seg_end) {   // the next step opens segment h + 1 with a fresh decision (at its top, from sv.o below)
                    tot_env = te;
                    tot_r = tr;
                    ++h;
                    left = K_steps;
                    seg_start = true;
                    refused_known = false;
                    mask_dirty = true;
                }
            }
            // what the next decision sees, if the next step opens a segment: the observation as stored
#pragma unroll
            for (int c = 0; c < ATC_OBS_DIM; ++c) x[c] = sv.o[c];
        }
    }
}
static_assert(kernargs_like_step<decltype(k_lookahead_policy<1, false>)>() && KernArgs<decltype(k_lookahead_policy<1, false>)>::last() != 0, ATC_KERNARGS_REFUSAL);

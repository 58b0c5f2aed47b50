// atc_policy.inc — atc_rollout_policy (include/atc_step.h): T steps with the decisions of a 10 -> 64 -> 64 -> 3 tanh MLP and a diagonal
// Gaussian taken INSIDE the launch.  Included by atc_step.hip behind atc_branch.inc.
//   k_rollout_policy is the multi-step k_step's loop — state loaded once, step_part_a / step_part_b per step, state written once — as
//   a copy of the text, not a flag on k_step (the precedent of k_plan_sampled: k_step's instances keep their machine code).  The step
//   runs in its SKIP form, which hands the step's values back in registers (StepVals), and this kernel stores them per step the way
//   the tail of step_part_b does: observation rows through store_obs_rows, then the flag word, reward and done.  The observation
//   registers of a step are carried over the loop's back edge (nothing else of the step is live there) and the first step of the
//   next block evaluates the policy on them; decision 0 reads obs0.  One evaluation site, so one copy of the MLP's code.
//   THE MLP.  One lane per aircraft slot evaluates its own row: layer 1 unrolled (640 fmaf — in float64 where a wavefront holds an input
//   above 4 in magnitude, see there —, 64 activations kept in vector registers),
//   layer 2 as a loop over the 64 output neurons with the 64 inputs unrolled — four partial sums, so that no fmaf waits for the one
//   before it — and layer 3 folded into that loop (each tanh(h2_j) goes straight into the three output sums; h2 is never stored).
//   WEIGHTS are read through the constant address space at wave-uniform indices: scalar loads (s_load_dwordx8 / x16 into scalar
//   registers, which the fmaf takes as an operand), 20 KB per decision and wavefront out of the scalar cache / L2.  Why not LDS
//   broadcasts: a wave-uniform ds_read_b128 costs 4 LDS cycles for 4 weights = 16 VALU cycles of fmaf per SIMD, and the four SIMDs of a
//   CU share one LDS — the pipe would be exactly saturated before the step's own LDS stages (pair scan, observation transpose) ask
//   for anything; the scalar path leaves LDS and the vector registers alone.  Why not v_mfma_f32_32x32x2f32: its rate is the packed
//   fp32 VALU's (twice the plain fmaf's), but its A / B operands want activation k of aircraft l in lane l + 32 (k & 1): the
//   activations of a lane-per-aircraft layout would have to cross lane halves before and after each layer (DESIGN.md section 3k).
//   The base pointer goes through the block's opaque zero, or the (invariant) weight loads are hoisted out of the step loop and the
//   scalar registers holding them spilled to vector-register lanes.
//   THE DRAW: integers, key, u1, u2 exact; logf / cosf / sqrtf / expf / tanhf are the device library's (the file is built without
//   fast-math and with -ffp-contract=off).  tests/policy_ref.py restates everything in numpy.
//   TRAFFIC (atc_rollout_policy_traffic, k_rollout_policy_traffic<W, KT>): the same loop with one more stage at the decision site — the
//   query of atc_observe_traffic(KT) on the state in registers, through the device functions k_traffic itself calls (atc_traffic.inc),
//   stored and fed to a first layer of 10 + 7 KT inputs.  See rollout_policy_body.
// the seven parts of the packed array for an input row of IN words (10: atc_policy_t.w; 10 + 7 K: atc_policy_traffic_t.w)
template <int IN>
struct PolOff {
    enum { W1 = 0, B1 = ATC_POLICY_HIDDEN * IN, W2 = B1 + ATC_POLICY_HIDDEN, B2 = W2 + ATC_POLICY_HIDDEN * ATC_POLICY_HIDDEN, W3 = B2 + ATC_POLICY_HIDDEN,
           B3 = W3 + 3 * ATC_POLICY_HIDDEN, LOGSTD = B3 + 3, WORDS = LOGSTD + 3 };
};
static_assert(PolOff<ATC_POLICY_IN>::WORDS == ATC_POLICY_WORDS && ATC_POLICY_IN == ATC_OBS_DIM && ATC_POLICY_HIDDEN == 64, "atc_policy_t.w layout");
static_assert(PolOff<ATC_POLICY_TRAFFIC_IN(1)>::WORDS == ATC_POLICY_TRAFFIC_WORDS(1) && PolOff<ATC_POLICY_TRAFFIC_IN(4)>::WORDS == ATC_POLICY_TRAFFIC_WORDS(4) &&
              ATC_POLICY_TRAFFIC_WORDS(1) == 5510 && ATC_POLICY_TRAFFIC_WORDS(2) == 5958 && ATC_POLICY_TRAFFIC_WORDS(4) == 6854, "atc_policy_traffic_t.w layout");
#define ATC_POL_TWO_PI 6.2831853071795864769f
#define ATC_POL_LOGP_C 2.7568155996140185f   // 1.5 log(2 pi)

typedef __attribute__((address_space(4))) const float* pol_wptr;   // constant address space: uniform indices become scalar loads

struct PolicyDecision {
    Float3 u;      // the unclamped sample (atc_policy_out_t.action)
    Float3 a;      // what is flown: plan_draw_clamp(u)
    float logp;
};

// one standard normal by Box-Muller from 64 mixed bits: u1 in (0, 1] from the top 24 bits, u2 in [0, 1) from bits 16..39
__device__ __forceinline__ float policy_z(uint64_t key, uint32_t c) {
    const uint64_t w = mix64(key ^ (uint64_t)(c + 1u));
    const float u1 = (float)((uint32_t)(w >> 40) + 1u) * 0x1p-24f;
    const float u2 = (float)((uint32_t)(w >> 16) & 0xffffffu) * 0x1p-24f;
    return sqrtf(-2.0f * logf(u1)) * cosf(ATC_POL_TWO_PI * u2);
}

template <int IN>
__device__ __forceinline__ PolicyDecision policy_decide(const float* w_arg, int zk, const float* x, uint64_t seed, uint32_t decision, uint32_t i,
                                                        bool deterministic) {
    typedef PolOff<IN> O;
    pol_wptr w = (pol_wptr)(uintptr_t)w_arg;
    asm volatile("" : "+s"(w) : "s"(zk));
    // Layer 1.  Normalised observations lie in [-1, 1] and the fp32 sum is good to 1e-7.  Unnormalised ones reach 1.5e4 (the altitude
    // words, and the raw reset observation behind an auto-reset): the fp32 partial sums then round by up to 1e-3, and a neuron whose
    // sum happens to land near 0 — one in 10^4 — hands an error of that size through tanh's slope to the outputs.  A wavefront that
    // holds such an input sums this layer in float64 (the products are exact there); the choice is wave-uniform.
    float h1[ATC_POLICY_HIDDEN];
    float xmax = 0.0f;
#pragma unroll
    for (int c = 0; c < IN; ++c) xmax = fmaxf(xmax, fabsf(x[c]));
    if (ATC_RARE(__builtin_amdgcn_ballot_w64(!(xmax <= 4.0f)) != 0ull)) {
        double xd[IN];
#pragma unroll
        for (int c = 0; c < IN; ++c) xd[c] = (double)x[c];
#pragma unroll
        for (int j = 0; j < ATC_POLICY_HIDDEN; ++j) {
            double s = (double)w[O::B1 + j];
#pragma unroll
            for (int c = 0; c < IN; ++c) s = __builtin_fma((double)w[O::W1 + j * IN + c], xd[c], s);
            h1[j] = (float)s;
        }
    } else {
#pragma unroll
        for (int j = 0; j < ATC_POLICY_HIDDEN; ++j) {
            float s = w[O::B1 + j];
#pragma unroll
            for (int c = 0; c < IN; ++c) s = fmaf(w[O::W1 + j * IN + c], x[c], s);
            h1[j] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < ATC_POLICY_HIDDEN; ++j) h1[j] = tanhf(h1[j]);
    float mu[3] = {w[O::B3 + 0], w[O::B3 + 1], w[O::B3 + 2]};
#pragma unroll 1
    for (int j = 0; j < ATC_POLICY_HIDDEN; ++j) {
        pol_wptr row = w + O::W2 + j * ATC_POLICY_HIDDEN;
        float s0 = w[O::B2 + j], s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int c = 0; c < ATC_POLICY_HIDDEN; c += 4) {
            s0 = fmaf(row[c + 0], h1[c + 0], s0);
            s1 = fmaf(row[c + 1], h1[c + 1], s1);
            s2 = fmaf(row[c + 2], h1[c + 2], s2);
            s3 = fmaf(row[c + 3], h1[c + 3], s3);
        }
        const float h2 = tanhf((s0 + s1) + (s2 + s3));
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = fmaf(w[O::W3 + c * ATC_POLICY_HIDDEN + j], h2, mu[c]);
    }
    PolicyDecision dec;
    dec.logp = 0.0f;
    if (deterministic) {
        dec.u = Float3{mu[0], mu[1], mu[2]};
    } else {
        const uint64_t key = mix64(mix64(seed ^ (uint64_t)decision) ^ (uint64_t)i);
        float u[3], lp = 0.0f;
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const float ls = w[O::LOGSTD + c];
            const float z = policy_z(key, c);
            u[c] = mu[c] + expf(ls) * z;
            lp += -0.5f * (z * z) - ls;
        }
        dec.u = Float3{u[0], u[1], u[2]};
        dec.logp = lp - ATC_POL_LOGP_C;
    }
    dec.a = Float3{plan_draw_clamp(dec.u.a), plan_draw_clamp(dec.u.b), plan_draw_clamp(dec.u.c)};   // (a NaN gives -1)
    return dec;
}

// ARGUMENTS of both kernels: k_step's up to `q` (obs0 where it has the actions; `out` carries obs, reward, done, flags of atc_policy_out_t,
// the other fields null), then the policy's.  The loop re-reads hold, st, out and q from the kernarg segment by StepArgs offsets: the
// static_assert behind each kernel holds its own parameter list (KernArgs, atc_kernarg.h) to them.
// k_rollout_policy_traffic's list is k_rollout_policy's, then what the traffic stage reads — by kernarg re-read at the decision, at the offset
// that list gives its last parameter, so that nothing of it is carried across the step loop.  (The kernarg segment packs the parameters flat:
// a struct that nested the first list would be padded to its own alignment of 64 and name a later offset.)
struct PolicyTrafficTail {
    TrafficArgs tq;     // the host's traffic_common: the uniform terms of atc_observe_traffic
    float* traffic;     // atc_policy_traffic_out_t.traffic, nullable
};

// ENDS (atc_rollout_policy_ends, k_rollout_policy_ends<W, KT>): the three nullable per-decision outputs, read by kernarg re-read where
// they are stored — control at the decision, term_obs and term_flags at the step that ends an episode, term_flags' zero at a block's
// last step.  What the loop carries for them is one predicate per env: the block has ended an episode already.
struct PolicyEnds {
    float* term_obs;        // atc_policy_ends_out_t.term_obs
    uint16_t* term_flags;   // .term_flags
    uint8_t* control;       // .control
};

// TERM (atc_rollout_policy_term, k_rollout_policy_term<W, KT>, KT = 1, 2, 4): ENDS plus one more nullable per-decision output, the traffic
// records of the state term_obs describes — the query of the decision site (traffic_self / traffic_select / traffic_record: the same bits)
// run once more at the step that ends an episode, on the wave-uniform ballot(ends_now) path.
//   THE TERMINAL STATE is a snapshot, not a new form of the step: every change a step makes to an aircraft (speed, altitude, heading,
//   position) is made in step_part_a; step_part_b changes it only by the spawn of its auto-reset path.  So ls.a between the two halves IS the
//   state the episode ends in, with or without ATC_M_AUTO_RESET, and a copy taken there (x, y, the float64 altitude, heading counts, speed:
//   six registers) survives the spawn.  The active mask at the end is the mask before the second half less the aircraft this step hands
//   over: the ballot of ATC_F_WON over the env's lanes that step_part_b itself takes (not under ATC_M_KEEP_ACTIVE), recomputed here from
//   the flag word it returns; the copy of the mask is two more registers.  step_part_a and step_part_b are untouched, and every addition to
//   rollout_policy_body stands behind `if constexpr (TERMQ)`: the other kernels' device code is what it was (tools/isa_compare.py).
//   WIDE headings: the exact counts of a WIDE terminal heading are in the aircraft's row of st.phi_wide, written by step_part_a of this
//   step or an earlier one.  The spawn writes no side record (a spawned heading is plain), and no later step has run yet: the row is read
//   here, behind step_part_b, by the lane that wrote it, and holds the terminal heading.
//   LDS (W >= 32): the selection stages (x, y, tag) in the wavefront's own quarter of the pair-scan staging area, which this step's pair
//   scan has finished reading (a wavefront's LDS operations are issued and executed in order); the same wave-level fences as at the
//   decision site order the stage against its readers and against the next stage or pair scan.  No workgroup barrier: the path is taken
//   by whole wavefronts that hold an ending env, not by the workgroup.
//   The decision site's text is not factored out into a function shared with this one: that site's machine code is pinned.
struct PolicyTerm {
    float* term_traffic;    // atc_policy_term_out_t.term_traffic
};

// EVAL (atc_policy_eval, k_policy_eval<W, KT>): the loop with every per-step and per-decision store compiled out.  What leaves the launch is
// the env's record of ATC_EVAL_WORDS words — read at the start (or cleared), held in registers uniformly over the env's lanes like the env
// state, updated on the rare path where a step ends an episode, written once by lane k == 0 — and the last step's observation.
struct PolicyEval {
    int32_t* record;     // atc_policy_eval_out_t.record
    float* obs_last;     // .obs_last, nullable
    uint32_t flags;      // .flags
};

// wavefronts per SIMD k_rollout_policy is register-budgeted for (<= 168 VGPRs): the 64 hidden activations are live next to what the
// step carries across its loop, which the step's own 5 - 6 do not hold.  -DATC_POLICY_WAVES=n: A/B builds.
#ifndef ATC_POLICY_WAVES
#define ATC_POLICY_WAVES 3
#endif
// The loop of both kernels.  KT = 0: k_rollout_policy, the policy sees the ten own words.  KT = 1, 2, 4: k_rollout_policy_traffic — at a
// block's first step the traffic query of atc_observe_traffic(KT) is evaluated on the state in registers (traffic_self / traffic_select /
// traffic_record of atc_traffic.inc: k_traffic's arithmetic, so the same bits), stored, and its words 0..6 per record widen the input row.
// An env never leaves its wavefront: W = 32 / 64 stage (x, y, tag) in the wavefront's own quarter of the pair-scan staging area (idle
// between steps), ordered by wave-level waits — no workgroup barrier anywhere in the decision.
// TT_OFF: where the kernel's PolicyTrafficTail lies in ITS kernarg segment (the body serves three parameter lists); ET_OFF: where its
// PolicyEnds lies, 0 for the kernels that have none (ENDS below); EV_OFF: where its PolicyEval lies, 0 for all but k_policy_eval (EVAL);
// TQ_OFF: where its PolicyTerm lies, 0 for all but k_rollout_policy_term (TERM above).
template <int W, int KT, size_t TT_OFF = 0, size_t ET_OFF = 0, size_t EV_OFF = 0, size_t TQ_OFF = 0>
__device__ __forceinline__ void rollout_policy_body(const float* __restrict__ blob, int off_grid, int B, int N, int T, atc_state_t st, const float* __restrict__ obs0,
                                                    atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
                                                    float* __restrict__ action, float* __restrict__ logp) {
    constexpr bool ONE = false, LAT = false, FULL = false;   // (QGET: the multi-step form — kernarg re-reads inside the step)
    constexpr bool ENDS = ET_OFF != 0;
    constexpr bool EVAL = EV_OFF != 0;
    constexpr bool TERMQ = TQ_OFF != 0;
    static_assert(!(ENDS && EVAL), "k_policy_eval stores none of the per-decision outputs");
    static_assert(!TERMQ || (ENDS && KT > 0), "the terminal traffic records belong to the ends of a policy that sees traffic");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* pos = reinterpret_cast<float4*>(smem);                    // [2 kBlock] pair-scan staging (W >= 32)
    float* obs_stage = smem + (W >= 32 ? 2 * kBlock * 4 : 0);  // [4 waves][64 x 10] obs transpose
    const float* __restrict__ K = blob;
    const float* __restrict__ grid = off_grid ? blob + off_grid : nullptr;
    const uint32_t BN = (uint32_t)B * (uint32_t)N;
    const LaneIds d = make_ids<W, false>(blockIdx.x * kBlock, B, N);

    const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
    const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
    EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
    const int4 ps = *at<int4>(st.ac, d.i * 16u);
    const double h0 = *at<double>(st.alt, d.i * 8u);
    const int4 la0 = *at<int4>(st.last_act, d.i * 16u);
    LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};
    // what decision 0 sees: the lane's row of obs0 (an idle lane reads the last aircraft's row: in bounds, its decision is never stored)
    float x[ATC_OBS_DIM];
    {
        const float2* r0 = at<float2>(obs0, times40(d.i));
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM / 2; ++c) {
            const float2 v = r0[c];
            x[2 * c] = v.x;
            x[2 * c + 1] = v.y;
        }
    }

    Float3 act = {0.0f, 0.0f, 0.0f};   // the clamped action of the current block
    Targets tg = {0u, 0.0f, 0};
    uint64_t refused_blk = 0ull;
    bool refused_known = false;
    bool all_active = false, mask_dirty = true;
    int left = 0;                 // steps the current block is still flown for
    uint32_t blk = 0u;            // the number of the coming decision
    bool ended = false;           // ENDS: an earlier step of the current block ended an episode of this lane's env
    // EVAL: words 0 .. 11 of the env's record (the initial values under ATC_EVAL_CLEAR), and this lane's OR of its flag words
    int4 ev_n = make_int4(0, 0, 0, 0);                              // episodes, wins, below-MVA ends, outside ends
    int ev_conflict = 0, ev_timeout = 0, ev_steps = 0;
    float ev_sum = 0.0f, ev_sq = 0.0f, ev_min = __builtin_inff(), ev_max = -__builtin_inff();
    uint32_t ev_or = 0u, ev_or0 = 0u;
    if constexpr (EVAL) {
        const PolicyEval ev = kernarg_reread<PolicyEval>(EV_OFF, opaque_zero());
        if (!(ev.flags & ATC_EVAL_CLEAR)) {   // (d.e is clamped for lanes without an env: in bounds, never stored)
            const int4* rec = at<int4>(ev.record, (uint32_t)d.e * (ATC_EVAL_WORDS * 4u));
            const int4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
            ev_n = r0;
            ev_conflict = r1.x; ev_timeout = r1.y; ev_steps = r1.z; ev_sum = __int_as_float(r1.w);
            ev_sq = __int_as_float(r2.x); ev_min = __int_as_float(r2.y); ev_max = __int_as_float(r2.z); ev_or0 = (uint32_t)r2.w;
            asm volatile("" : "+v"(ev_n.x), "+v"(ev_n.y), "+v"(ev_n.z), "+v"(ev_n.w), "+v"(ev_conflict), "+v"(ev_timeout), "+v"(ev_steps));   // (waited for here: see settle_state)
            asm volatile("" : "+v"(ev_sum), "+v"(ev_sq), "+v"(ev_min), "+v"(ev_max), "+v"(ev_or0));
        }
    }
    QRates qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
    settle_state(ls, es);
#pragma unroll
    for (int c = 0; c < ATC_OBS_DIM; ++c) asm volatile("" : "+v"(x[c]));   // (waited for here, like the state: see settle_state)
    for (int step = 0; step < T; ++step) {
        const size_t sBN = (size_t)step * BN, sB = (size_t)step * (uint32_t)B;
        LaneIds dl = d;
        atc_params_t pl = p;
        const int zk = opaque_zero();   // this step's opaque zero (see k_step)
        pl.mode += (uint32_t)zk;
        const StepOut so = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // (the step stores nothing itself)
        const QRates qr = qr_next;
        const QScan qs = QGET(s);
        const bool first = left == 0;   // this step opens a block: a fresh decision, from the observation the step before it stored
        if (ATC_RARE(first)) {
            left = kernarg_reread<int>(offsetof(StepArgs, hold), zk);
            PolicyDecision dec;
            if constexpr (KT == 0) {
                dec = policy_decide<ATC_POLICY_IN>(pw, zk, x, seed, decision0 + blk, dl.i, (pflags & ATC_POLICY_DETERMINISTIC) != 0u);
            } else {
                // ---- the traffic query on the state the env is in now: what step b hold - 1 left, or the fresh spawn after an auto-reset ----
                const PolicyTrafficTail tt = kernarg_reread<PolicyTrafficTail>(TT_OFF, zk);
                int phi = ls.a.phi;
                if (ATC_RARE(is_wide(phi))) phi = phi_wrap(*at<double>(wide_base<false>(st.phi_wide, zk), dl.i * 32u));   // the exact counts, as the step reads them
                const TrafficSelf me = traffic_self(ls.a.x, ls.a.y, ls.a.h, phi, ls.a.v, tt.tq);
                const bool under = dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u);
                const int tag = under ? dl.k : -1;
                uint64_t best[KT];
                if constexpr (W >= 32) {
                    float* sl = reinterpret_cast<float*>(pos) + 8 * (dl.tid & ~63);   // this wavefront's quarter: [64] x | [64] y | [64] tag
                    sl[dl.lane] = me.x;
                    sl[64 + dl.lane] = me.y;
                    reinterpret_cast<int*>(sl)[128 + dl.lane] = tag;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const int gb = dl.lane & ~(W - 1);
                    traffic_select<W, KT>(best, me.x, me.y, tag, dl.k, N, sl + gb, sl + 64 + gb, reinterpret_cast<const int*>(sl) + 128 + gb);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the reads above, before the next step's pair scan stages over them)
                    __builtin_amdgcn_wave_barrier();
                } else {
                    traffic_select<W, KT>(best, me.x, me.y, tag, dl.k, N, nullptr, nullptr, nullptr);
                }
                constexpr int IN = ATC_POLICY_TRAFFIC_IN(KT);
                float xin[IN];
#pragma unroll
                for (int c = 0; c < ATC_OBS_DIM; ++c) xin[c] = x[c];
                float4* dst = reinterpret_cast<float4*>(tt.traffic + ((size_t)blk * BN + dl.i) * (size_t)(KT * ATC_TRAFFIC_DIM));   // (64-bit: 32 K bytes per aircraft)
#pragma unroll
                for (int r = 0; r < KT; ++r) {
                    float4 ra, rb;
                    traffic_record<W>(best[r], under, dl.lane, me, tt.tq, ra, rb);
                    if constexpr (!EVAL) {
                        if (tt.traffic && dl.lane_valid) {
                            dst[2 * r] = ra;
                            dst[2 * r + 1] = rb;
                        }
                    }
                    float* xr = xin + ATC_OBS_DIM + 7 * r;   // words 0..6: word 7 (the slot) is stored, not an input
                    xr[0] = ra.x; xr[1] = ra.y; xr[2] = ra.z; xr[3] = ra.w;
                    xr[4] = rb.x; xr[5] = rb.y; xr[6] = rb.z;
                }
                dec = policy_decide<IN>(pw, zk, xin, seed, decision0 + blk, dl.i, (pflags & ATC_POLICY_DETERMINISTIC) != 0u);
            }
            if constexpr (!EVAL) {
                if (dl.lane_valid) {
                    *at<Float3>(action + (size_t)blk * BN * 3u, times12(dl.i)) = dec.u;
                    if (logp) *at<float>(logp + (size_t)blk * BN, dl.i * 4u) = dec.logp;
                }
            }
            if constexpr (ENDS) {   // which aircraft this decision controls: the active mask of the state it is taken in
                uint8_t* const control = kernarg_reread<uint8_t*>(ET_OFF + offsetof(PolicyEnds, control), zk);
                const bool under = ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u) != 0u;
                if (control && dl.lane_valid) *at<uint8_t>(control + (size_t)blk * BN, dl.i) = under ? 1 : 0;
                ended = false;
            }
            act = dec.a;
            tg = decode_targets(qr, act);
            refused_known = false;
            ++blk;
        }
        --left;
        const bool repeated = !first && __builtin_amdgcn_ballot_w64(es.t == 0) == 0ull;
        if (ATC_RARE(mask_dirty)) {
            all_active = (__builtin_amdgcn_ballot_w64(!(dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u))) |
                          __builtin_amdgcn_ballot_w64(max(ls.a.phi, ls.la_p) == INT32_MAX) | __builtin_amdgcn_ballot_w64(min(ls.a.phi, ls.la_p) == INT32_MIN)) == 0ull;
            mask_dirty = false;
        }
        const Mid m = step_part_a<false, false>(grid, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es, repeated, all_active,
                                                st.phi_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(nullptr));
        refused_known = true;
        StepVals sv;
        Float3 nxt = act;
        int scan_skip = 0;
        uint32_t scan_mask = 0u;
        // (ENDS: the step that ends an episode stores the terminal observation itself, ahead of the spawn that overwrites it)
        constexpr size_t TERM_OFF = ENDS ? ET_OFF + offsetof(PolicyEnds, term_obs) : 0;
        const size_t ends_row = (size_t)(blk - 1u) * BN;   // the current block's row of the [D] outputs, in aircraft
        // (TERMQ: the state this step ends in, should it end an episode — the second half changes an aircraft by its spawn only — and the mask before its hand-overs)
        [[maybe_unused]] const Aircraft term_a = ls.a;
        [[maybe_unused]] const uint64_t term_mask = es.amask;
        const bool quiet = step_part_b<W, FULL, false, false, false, true, false, false, TERM_OFF>(K, grid, pl, q, qs, zk, N, dl, m, ls, es, so, st.stats, st.phi_wide,
                                                                                                   pos, obs_stage, nullptr, nxt, qr_next, scan_skip, scan_mask, nullptr,
                                                                                                   nullptr, &sv, ends_row * ATC_OBS_DIM, !ended);
        if (ATC_RARE(!quiet)) mask_dirty = true;
        if constexpr (ENDS) {
            const bool ends_now = sv.done && !ended;   // the block's ending step for this env (uniform over the env's lanes)
            if (ATC_RARE(__builtin_amdgcn_ballot_w64(ends_now) != 0ull)) {
                const PolicyEnds en = kernarg_reread<PolicyEnds>(ET_OFF, zk);
                const int seen = group_or_i<W>(dl.lane_valid ? (int)(sv.fl & 0xffffu) : 0);   // the env's flag words as flags[t] stores them
                if (ends_now) {
                    if (en.term_flags && dl.k == 0) *at<uint16_t>(en.term_flags + (size_t)(blk - 1u) * (uint32_t)B, (uint32_t)dl.e * 2u) = (uint16_t)(ATC_TERM_ENDED | (uint32_t)seen);
                    // without an auto-reset the stored observation is the terminal one
                    if (!(pl.mode & ATC_M_AUTO_RESET) && en.term_obs && dl.lane_valid) store_obs(at<float>(en.term_obs + ends_row * ATC_OBS_DIM, times40(dl.i)), sv.o);
                    ended = true;
                }
                if constexpr (TERMQ) {
                    // ---- the traffic query on the state term_obs describes: the decision site's, on the snapshot (wave-uniform: every lane runs it, the ending envs' store) ----
                    float* const term_traffic = kernarg_reread<float*>(TQ_OFF, zk);
                    if (term_traffic) {
                        const PolicyTrafficTail tt = kernarg_reread<PolicyTrafficTail>(TT_OFF, zk);
                        uint64_t mask = term_mask;   // less this step's hand-overs, as step_part_b takes them
                        if (!(pl.mode & ATC_M_KEEP_ACTIVE)) mask &= ~group_ballot<W>((sv.fl & ATC_F_WON) != 0, dl.lane);
                        int phi = term_a.phi;
                        if (ATC_RARE(is_wide(phi))) phi = phi_wrap(*at<double>(wide_base<false>(st.phi_wide, zk), dl.i * 32u));   // the exact counts: the spawn wrote no side record
                        const TrafficSelf me = traffic_self(term_a.x, term_a.y, term_a.h, phi, term_a.v, tt.tq);
                        const bool under = dl.lane_valid && ((dl.k < 32 ? ((uint32_t)mask >> dl.k) : ((uint32_t)(mask >> 32) >> (dl.k - 32))) & 1u);
                        const int tag = under ? dl.k : -1;
                        uint64_t best[KT > 0 ? KT : 1];
                        if constexpr (W >= 32) {
                            float* sl = reinterpret_cast<float*>(pos) + 8 * (dl.tid & ~63);   // this wavefront's quarter, behind this step's pair scan: [64] x | [64] y | [64] tag
                            sl[dl.lane] = me.x;
                            sl[64 + dl.lane] = me.y;
                            reinterpret_cast<int*>(sl)[128 + dl.lane] = tag;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            const int gb = dl.lane & ~(W - 1);
                            traffic_select<W, (KT > 0 ? KT : 1)>(best, me.x, me.y, tag, dl.k, N, sl + gb, sl + 64 + gb, reinterpret_cast<const int*>(sl) + 128 + gb);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the reads above, before the next decision or pair scan stages over them)
                            __builtin_amdgcn_wave_barrier();
                        } else {
                            traffic_select<W, (KT > 0 ? KT : 1)>(best, me.x, me.y, tag, dl.k, N, nullptr, nullptr, nullptr);
                        }
                        float4* dst = reinterpret_cast<float4*>(term_traffic + (ends_row + dl.i) * (size_t)(KT * ATC_TRAFFIC_DIM));   // (64-bit: 32 K bytes per aircraft)
#pragma unroll
                        for (int r = 0; r < KT; ++r) {
                            float4 ra, rb;
                            traffic_record<W>(best[r], under, dl.lane, me, tt.tq, ra, rb);
                            if (ends_now && dl.lane_valid) {   // (rows of an env whose block did not end here are left alone: term_obs's rule)
                                dst[2 * r] = ra;
                                dst[2 * r + 1] = rb;
                            }
                        }
                    }
                }
            }
            if (left == 0) {   // the block's last step: no ending step in it stores the zero
                uint16_t* const term_flags = kernarg_reread<uint16_t*>(ET_OFF + offsetof(PolicyEnds, term_flags), zk);
                if (term_flags && !ended && dl.env_valid && dl.k == 0) *at<uint16_t>(term_flags + (size_t)(blk - 1u) * (uint32_t)B, (uint32_t)dl.e * 2u) = 0;
            }
        }
        if constexpr (EVAL) {
            ev_or |= dl.lane_valid ? (sv.fl & 0xffffu) : 0u;
            if (ATC_RARE(__builtin_amdgcn_ballot_w64(sv.done) != 0ull)) {
                const int seen = group_or_i<W>(dl.lane_valid ? (int)(sv.fl & 0xffffu) : 0);   // the env's flag words as flags[t] would store them
                // The ended episode's length, return and win bit are the words the step has just written to the per-episode record
                // (done && ATC_M_AUTO_RESET, which the host requires: lane k == 0 wrote them, every lane of the env reads them back —
                // one wavefront, whose memory operations are issued in order; the fences are the ones step_part_b pairs with).
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int32_t* stats = kernarg_reread<int32_t*>(offsetof(StepArgs, st) + offsetof(atc_state_t, stats), zk);
                const int4 s1 = *at<int4>(stats, (uint32_t)dl.e * (ATC_STAT_WORDS * 4u));   // episodes, ep_length, ep_return, win_bits
                if (sv.done) {
                    const float r = __int_as_float(s1.z);
                    ev_n.x += 1;
                    ev_n.y += s1.w & 1;
                    ev_n.z += (seen & ATC_F_BELOW_MVA) ? 1 : 0;
                    ev_n.w += (seen & ATC_F_OUTSIDE) ? 1 : 0;
                    ev_conflict += (seen & ATC_F_CONFLICT) ? 1 : 0;
                    ev_timeout += (seen & ATC_F_TIMEOUT) ? 1 : 0;
                    ev_steps += s1.y;
                    ev_sum = ev_sum + r;
                    ev_sq = ev_sq + (r * r);   // (the file is built with -ffp-contract=off: a product, then an add)
                    ev_min = fminf(ev_min, r);
                    ev_max = fmaxf(ev_max, r);
                }
            }
        } else {
            // ---- this step's row of the [T][...] outputs: the tail of step_part_b (observation first, the three small stores last) ----
            const atc_out_t o_t = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), zk);
            store_obs_rows(o_t.obs + sBN * ATC_OBS_DIM, dl, sv.o, obs_stage);
            if (dl.lane_valid) stream_store(at<uint16_t>(o_t.flags + sBN, dl.i * 2u), (uint16_t)sv.fl);
            if (dl.env_valid && dl.k == 0) {
                *at<float>(o_t.reward + sB, (uint32_t)dl.e * 4u) = sv.env_r;
                *at<uint8_t>(o_t.done + sB, (uint32_t)dl.e) = sv.done ? 1 : 0;
            }
        }
        // what the next decision sees, if the next step opens a block: the observation as stored
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) x[c] = sv.o[c];
    }
    const atc_state_t st_end = kernarg_reread<atc_state_t>(offsetof(StepArgs, st), opaque_zero());
    store_lane_state(st_end, d, ls, true);
    store_env_state<W>(st_end, d, es, hi0);
    if constexpr (EVAL) {
        const PolicyEval ev = kernarg_reread<PolicyEval>(EV_OFF, opaque_zero());
        const uint32_t seen_all = ev_or0 | (uint32_t)group_or_i<W>((int)ev_or);
        if (ev.obs_last) store_obs_rows(ev.obs_last, d, x, obs_stage);   // (T >= 1: x holds the last step's observation as stored)
        if (d.env_valid && d.k == 0) {
            int4* rec = at<int4>(ev.record, (uint32_t)d.e * (ATC_EVAL_WORDS * 4u));
            int4 r3 = make_int4(0, 0, 0, 0);   // launch steps and the three reserved words: read here, nothing of them is carried
            if (!(ev.flags & ATC_EVAL_CLEAR)) r3 = rec[3];
            r3.x += T;
            rec[0] = ev_n;
            rec[1] = make_int4(ev_conflict, ev_timeout, ev_steps, __float_as_int(ev_sum));
            rec[2] = make_int4(__float_as_int(ev_sq), __float_as_int(ev_min), __float_as_int(ev_max), (int)seen_all);
            rec[3] = r3;
        }
    }
}

template <int W>
__global__ void __launch_bounds__(kBlock, ATC_POLICY_WAVES)
k_rollout_policy(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st, const float* __restrict__ obs0,
                 atc_out_t out, atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
                 float* __restrict__ action, float* __restrict__ logp) {
    rollout_policy_body<W, 0>(blob, off_grid, B, N, T, st, obs0, p, q, pw, seed, decision0, pflags, action, logp);   // (hold, out: kernarg re-reads)
}
static_assert(kernargs_hold_like_step<decltype(k_rollout_policy<1>)>(), ATC_KERNARGS_REFUSAL);

// KT: the compiled list length = atc_policy_traffic_t.traffic_k (1, 2, 4)
template <int W, int KT>
__global__ void __launch_bounds__(kBlock, ATC_POLICY_WAVES)
k_rollout_policy_traffic(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st, const float* __restrict__ obs0,
                         atc_out_t out, atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
                         float* __restrict__ action, float* __restrict__ logp, PolicyTrafficTail tt) {
    // (tt: a kernarg re-read at the decision, at the offset this list gives its last parameter)
    rollout_policy_body<W, KT, KernArgs<decltype(k_rollout_policy_traffic<W, KT>)>::last()>(blob, off_grid, B, N, T, st, obs0, p, q, pw, seed, decision0, pflags,
                                                                                          action, logp);
}
static_assert(kernargs_hold_like_step<decltype(k_rollout_policy_traffic<1, 1>)>(), ATC_KERNARGS_REFUSAL);

// KT = 0, 1, 2, 4: atc_policy_traffic_t.traffic_k as atc_rollout_policy_ends takes it.  One parameter list for all four (tt is not read
// where KT = 0): k_rollout_policy_traffic's, then the three pointers.
template <int W, int KT>
__global__ void __launch_bounds__(kBlock, ATC_POLICY_WAVES)
k_rollout_policy_ends(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st, const float* __restrict__ obs0,
                      atc_out_t out, atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
                      float* __restrict__ action, float* __restrict__ logp, PolicyTrafficTail tt, PolicyEnds en) {
    // (tt, en: kernarg re-reads where they are used, at the offsets this list gives them)
    typedef KernArgs<decltype(k_rollout_policy_ends<W, KT>)> A;
    rollout_policy_body<W, KT, A::template of<PolicyTrafficTail>(), A::last()>(blob, off_grid, B, N, T, st, obs0, p, q, pw, seed, decision0, pflags, action, logp);
}
static_assert(kernargs_hold_like_step<decltype(k_rollout_policy_ends<1, 0>)>() && KernArgs<decltype(k_rollout_policy_ends<1, 0>)>::last() != 0, ATC_KERNARGS_REFUSAL);
// KT = 1, 2, 4.  The parameter list is k_rollout_policy_ends', then the one pointer.
template <int W, int KT>
__global__ void __launch_bounds__(kBlock, ATC_POLICY_WAVES)
k_rollout_policy_term(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st, const float* __restrict__ obs0,
                      atc_out_t out, atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
                      float* __restrict__ action, float* __restrict__ logp, PolicyTrafficTail tt, PolicyEnds en, PolicyTerm tr) {
    // (tt, en, tr: kernarg re-reads where they are used, at the offsets this list gives them)
    typedef KernArgs<decltype(k_rollout_policy_term<W, KT>)> A;
    rollout_policy_body<W, KT, A::template of<PolicyTrafficTail>(), A::template of<PolicyEnds>(), 0, A::last()>(blob, off_grid, B, N, T, st, obs0, p, q, pw, seed, decision0,
                                                                                                                pflags, action, logp);
}
static_assert(kernargs_hold_like_step<decltype(k_rollout_policy_term<1, 1>)>() && KernArgs<decltype(k_rollout_policy_term<1, 1>)>::last() != 0, ATC_KERNARGS_REFUSAL);
static_assert(KernArgs<decltype(k_rollout_policy_term<1, 1>)>::of<PolicyEnds>() == KernArgs<decltype(k_rollout_policy_ends<1, 1>)>::last(),
              "k_rollout_policy_term's list is k_rollout_policy_ends', then the pointer");
static_assert(ATC_POLICY_TRAFFIC_WORDS(0) == ATC_POLICY_WORDS && ATC_POLICY_TRAFFIC_IN(0) == ATC_POLICY_IN, "traffic_k == 0 is the ten-word policy");

// KT = 0, 1, 2, 4 as k_rollout_policy_ends takes it.  The parameter list is k_rollout_policy_traffic's — out, action and logp are passed
// as zeros and never read — then the record's three fields.
// REQUIRES ATC_M_AUTO_RESET in p.mode (the host refuses the call without it, check_policy_eval_call): the ended episode's length, return and
// win bit are re-loaded from the per-episode record, which step_part_b writes on its auto-reset path only.  Without the reset a done step
// would count the words of an EARLIER episode, silently; a host that relaxes the refusal has to hand the pair back through StepVals instead.
template <int W, int KT>
__global__ void __launch_bounds__(kBlock, ATC_POLICY_WAVES)
k_policy_eval(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st, const float* __restrict__ obs0,
              atc_out_t out, atc_params_t p, StepDerived q, const float* __restrict__ pw, uint64_t seed, uint32_t decision0, uint32_t pflags,
              float* __restrict__ action, float* __restrict__ logp, PolicyTrafficTail tt, PolicyEval ev) {
    // (tt, ev: kernarg re-reads where they are used, at the offsets this list gives them)
    typedef KernArgs<decltype(k_policy_eval<W, KT>)> A;
    rollout_policy_body<W, KT, A::template of<PolicyTrafficTail>(), 0, A::last()>(blob, off_grid, B, N, T, st, obs0, p, q, pw, seed, decision0, pflags, action, logp);
}
static_assert(kernargs_hold_like_step<decltype(k_policy_eval<1, 0>)>() && KernArgs<decltype(k_policy_eval<1, 0>)>::last() != 0, ATC_KERNARGS_REFUSAL);

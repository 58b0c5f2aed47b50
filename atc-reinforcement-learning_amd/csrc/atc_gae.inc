// atc_gae.inc — k_gae (atc_gae, include/atc_step.h) and k_gae_boot (atc_gae_boot): the per-step rewards and dones of a rollout and the values of one batched forward
// turned into advantages and returns, one transition per decision, in one launch.  Included by atc_step.hip behind atc_policy.inc.
//   Mapping: ONE LANE PER COLUMN i = e * NV + k, workgroups of one wavefront (kGaeBlock = 64).  [D][C] has C contiguous, so row d of
//   values, adv and ret is a coalesced access across the wavefront; the NV lanes of an env read the same reward and done words (one
//   address, served once); the [D][B] block outputs are stored by the env's lane k == 0.  A lane only ever touches its own column and
//   its env's words: no LDS, nothing is synchronised, and an idle lane of the last workgroup returns before its first load.
//   Operation by operation (-ffp-contract=off: every product and sum is rounded once, nothing is fused).  The launch walks the steps in
//   the order the recurrence consumes them — d descending from D - 1, j = 0 .. hold - 1 ascending inside a block — as ONE flat sequence
//   of T = D * hold steps, kGaeDepth steps a chunk.  (d, j) is the same in every lane, so the cursor and its branches are scalar.
//     block:   j == 0: g = 1, R = r, n = 1, term = done != 0;  j > 0 and !term: g = g * gamma, R = R + (r * g), n = n + 1, term = done != 0
//              (ATC_GAE_PER_DECISION runs the same two operations with the factor 1.0f in gamma's place: g stays 1.0f and r * 1.0f is r,
//              bit for bit, so R = R + r).  A word behind the block's first done is loaded but only ever reaches the dead arm of a select.
//     G = g_{hold-1} * gamma: `hold` products from 1.0f, evaluated by the launch itself in the arithmetic that evaluates g (under
//              ATC_GAE_PER_DECISION G = gamma); c = G * lam.
//     j == hold - 1: term: delta = R - V[d], A = delta;  else: delta = (R + (G * V[d+1])) - V[d], A = delta + (c * A_next)
//              adv[d] = A, ret[d] = A + V[d], A_next = A; V[d+1] of the next block is this block's V[d]: one values word per block.
//   PIPELINE.  The recurrence is serial in d, but no address depends on it: the loads of chunk q + 1 (its rewards and dones, and V[d] at
//   each step that ends a block) are issued into a second register set before the arithmetic of chunk q starts, so up to 2 * kGaeDepth
//   steps of a lane are in flight and the dependent chain only ever waits for the older set.
//   Every [D] and [T] offset is a size_t.
constexpr int kGaeBlock = 64;
constexpr int kGaeDepth = 8;

struct GaeCursor {      // the (d, j) of the next step of the flat sequence; d < 0: past the end.  Wave-uniform.
    int d, j;
    __device__ __forceinline__ bool live() const { return d >= 0; }
    __device__ __forceinline__ void advance(int hold) {
        if (++j == hold) {
            j = 0;
            --d;
        }
    }
};

__device__ __forceinline__ float gae_word(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }   // one NaN (atc_plan_score's rule)

// BOOT (k_gae_boot, atc_gae_boot): a block whose episode ended at a step the caller marks as truncated (trunc[d][e] != 0) bootstraps from
// boot[d][i], the value of the state it ended in, discounted by Gn = g * gamma with g the running product at the block's last counted
// step: delta = (R + (Gn * boot)) - V[d], A = delta.  The two words are loaded with V[d], into the prefetched register set; a boot word that
// is not selected only reaches the dead arm of a select.
template <bool BOOT>
__device__ __forceinline__ void gae_body(int B, int NV, int D, int hold, const float* __restrict__ reward, const uint8_t* __restrict__ done,
                                         const float* __restrict__ values, const float* __restrict__ adv_next, const float* __restrict__ boot,
                                         const uint8_t* __restrict__ trunc, const atc_gae_t& gp, const atc_gae_out_t& out) {
    const size_t Bs = (size_t)(uint32_t)B, C = Bs * (uint32_t)NV;
    const size_t i0 = (size_t)blockIdx.x * (uint32_t)kGaeBlock, i = i0 + threadIdx.x;
    if (i >= C) return;                                                // idle lanes neither load nor store (nothing below synchronises)
    // every address below is a wave-uniform pointer (the row, and the workgroup's first column or env: scalar arithmetic) plus one of
    // three small per-lane byte offsets, so a load or store keeps no 64-bit address in vector registers
    const size_t e0 = i0 / (uint32_t)NV, e = i / (uint32_t)NV;
    const bool first_of_env = i == e * (uint32_t)NV;                   // the lane that stores the env's [D][B] words
    const bool per_column = (gp.flags & ATC_GAE_REWARD_PER_COLUMN) != 0u;
    const uint32_t col_off = threadIdx.x * 4u, env_lane = (uint32_t)(e - e0), env_off = env_lane * 4u;
    const size_t r_row = per_column ? C : Bs, r_first = per_column ? i0 : e0;
    const uint32_t r_off = per_column ? col_off : env_off;
    const float step_gamma = (gp.flags & ATC_GAE_PER_DECISION) ? 1.0f : gp.gamma;
    float G = gp.gamma;
    if (!(gp.flags & ATC_GAE_PER_DECISION)) {
        G = 1.0f;
        for (int j = 0; j < hold; ++j) G = G * gp.gamma;               // g_{hold-1} * gamma; 1.0f * gamma is gamma
    }
    const float c = G * gp.lam;
    float* const __restrict__ adv = out.adv;
    float* const __restrict__ ret = out.ret;
    float* const __restrict__ block_reward = out.block_reward;
    uint8_t* const __restrict__ block_done = out.block_done;
    uint8_t* const __restrict__ block_steps = out.block_steps;
    const bool store_reward = block_reward != nullptr && (per_column || first_of_env);
    auto word = [](const float* row, uint32_t off) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + off); };
    auto word_at = [](float* row, uint32_t off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(row) + off); };

    float a_next = adv_next ? word(adv_next + i0, col_off) : 0.0f;
    float v_next = word(values + ((size_t)(uint32_t)D * C + i0), col_off);

    // one chunk of the flat sequence into a register set: no address depends on the recurrence
    GaeCursor ld{D - 1, 0};
    auto load = [&](float (&r)[kGaeDepth], uint32_t (&dn)[kGaeDepth], float (&v)[kGaeDepth], float (&bt)[kGaeDepth], uint32_t (&tr)[kGaeDepth]) {
#pragma unroll
        for (int u = 0; u < kGaeDepth; ++u) {
            r[u] = 0.0f;
            dn[u] = 0u;
            v[u] = 0.0f;
            bt[u] = 0.0f;
            tr[u] = 0u;
            if (ld.live()) {
                const size_t t = (size_t)(uint32_t)ld.d * (uint32_t)hold + (uint32_t)ld.j;
                r[u] = word(reward + (t * r_row + r_first), r_off);
                dn[u] = (done + (t * Bs + e0))[env_lane];
                if (ld.j == hold - 1) {
                    v[u] = word(values + ((size_t)(uint32_t)ld.d * C + i0), col_off);
                    if (BOOT) {
                        bt[u] = word(boot + ((size_t)(uint32_t)ld.d * C + i0), col_off);
                        tr[u] = (trunc + ((size_t)(uint32_t)ld.d * Bs + e0))[env_lane];
                    }
                }
                ld.advance(hold);
            }
        }
    };
    // ... and its arithmetic: the block's fold, and at the block's last step the recurrence and the stores
    GaeCursor at{D - 1, 0};
    float g = 1.0f, R = 0.0f;
    uint32_t n = 0u;
    bool term = false;
    auto compute = [&](const float (&r)[kGaeDepth], const uint32_t (&dn)[kGaeDepth], const float (&v)[kGaeDepth], const float (&bt)[kGaeDepth],
                       const uint32_t (&tr)[kGaeDepth]) {
#pragma unroll
        for (int u = 0; u < kGaeDepth; ++u) {
            if (!at.live()) break;
            if (at.j == 0) {
                g = 1.0f;
                R = r[u];
                n = 1u;
                term = dn[u] != 0u;
            } else {
                const float g1 = g * step_gamma;
                const float R1 = R + (r[u] * g1);
                const bool open = !term;                               // (a word behind the first done only reaches the dead arm)
                g = open ? g1 : g;
                R = open ? R1 : R;
                n = open ? n + 1u : n;
                term = open ? dn[u] != 0u : true;
            }
            if (at.j == hold - 1) {
                const float vd = v[u];
                float A;
                if (term) {
                    A = R - vd;
                    if (BOOT) {
                        const float Gn = g * gp.gamma;
                        const float delta = (R + (Gn * bt[u])) - vd;
                        A = tr[u] != 0u ? delta : A;
                    }
                } else {
                    const float delta = (R + (G * v_next)) - vd;
                    A = delta + (c * a_next);
                }
                const size_t row = (size_t)(uint32_t)at.d;
                *word_at(adv + (row * C + i0), col_off) = gae_word(A);
                *word_at(ret + (row * C + i0), col_off) = gae_word(A + vd);
                if (store_reward) *word_at(block_reward + (row * r_row + r_first), r_off) = gae_word(R);
                if (first_of_env) {
                    if (block_done) (block_done + (row * Bs + e0))[env_lane] = term ? 1 : 0;
                    if (block_steps) (block_steps + (row * Bs + e0))[env_lane] = (uint8_t)n;
                }
                a_next = A;
                v_next = vd;
            }
            at.advance(hold);
        }
    };

    float r0[kGaeDepth], v0[kGaeDepth], b0[kGaeDepth], r1[kGaeDepth], v1[kGaeDepth], b1[kGaeDepth];
    uint32_t d0[kGaeDepth], t0[kGaeDepth], d1[kGaeDepth], t1[kGaeDepth];
    load(r0, d0, v0, b0, t0);
    while (at.live()) {
        load(r1, d1, v1, b1, t1);
        compute(r0, d0, v0, b0, t0);
        load(r0, d0, v0, b0, t0);
        compute(r1, d1, v1, b1, t1);
    }
}

__global__ void __launch_bounds__(kGaeBlock)
k_gae(int B, int NV, int D, int hold, const float* __restrict__ reward, const uint8_t* __restrict__ done, const float* __restrict__ values,
      const float* __restrict__ adv_next, atc_gae_t gp, atc_gae_out_t out) {
    gae_body<false>(B, NV, D, hold, reward, done, values, adv_next, nullptr, nullptr, gp, out);
}

__global__ void __launch_bounds__(kGaeBlock)
k_gae_boot(int B, int NV, int D, int hold, const float* __restrict__ reward, const uint8_t* __restrict__ done, const float* __restrict__ values,
           const float* __restrict__ adv_next, const float* __restrict__ boot, const uint8_t* __restrict__ trunc, atc_gae_t gp, atc_gae_out_t out) {
    gae_body<true>(B, NV, D, hold, reward, done, values, adv_next, boot, trunc, gp, out);
}

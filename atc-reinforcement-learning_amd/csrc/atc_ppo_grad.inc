// atc_ppo_grad.inc — k_ppo_grad<KT> and k_ppo_grad_reduce (atc_ppo_policy_grad, include/atc_step.h): the clipped PPO surrogate loss of the
// policy of atc_policy.inc on stored decisions and its gradient with respect to the packed weights.  Included by atc_step.hip behind
// atc_gae.inc.
//   MAPPING.  G workgroups of ONE wavefront; workgroup g takes the tiles of 64 rows g, g + G, ...; in the forward and in the data
//   gradients LANE = ROW, in the weight gradients LANE = OUTPUT NEURON j: lane j owns row j of dW1 (IN accumulators) and of dW2 (64),
//   db1[j], db2[j] and column j of dW3 (3) — 5 k to 6.9 k accumulators per workgroup, in registers over the workgroup's whole tile loop,
//   written once, with plain vector stores, to the workgroup's row of `scratch`.  db3 and dlog_std are per-lane sums, folded over the
//   lanes at the end.
//   FORWARD: policy_decide's arithmetic in its operation order (the wave-uniform float64 first layer included), weights through the
//   constant address space at wave-uniform indices (scalar loads).  What differs: x, h1 and h2 are staged in LDS as [word][lane] with a
//   row stride of 65 words, so that lane l reading [c][l] (a row's own word) and lane j reading [j][r] (neuron j of row r) are both
//   conflict-free, and a wave-uniform [c][r] is a broadcast.
//   BACKWARD.  dmu, dlog_std per lane.  dW3 += dmu^T h2 (lane j reads h2[j][r], dmu[k][r] broadcast).  Then one loop over j, like the
//   forward's: dh2_j from three scalar weights, dz2_j = dh2_j (1 - h2_j^2) written over h2_j in place, dh1 += W2[j][:] dz2_j with the
//   row W2[j][:] in scalar registers.  dW2 += dz2^T h1: per row r of the tile lane j reads dz2[j][r] once and 64 broadcast words
//   h1[c][r] — VALU fmaf, one per accumulator (DESIGN.md section 3o: why not the matrix unit).  dz1 = dh1 (1 - h1^2) over h1 in place,
//   dW1 += dz1^T x likewise.  A stage is overwritten only behind its last reader: the workgroup is one wavefront, whose LDS operations
//   complete in program order; the fences keep the compiler from moving them.
//   A ROW THAT DOES NOT PARTICIPATE (beyond R, index out of range, mask == 0) loads nothing but its index and mask byte: its x is 0 by a
//   select and its dmu, dlog_std and statistics are 0 by selects, so its dz2 and dz1 are exactly 0.  A tile without a participating row
//   is skipped.
//   DETERMINISM: no atomics.  An accumulator adds its tile's rows in the order r = 0 .. 63 and the tiles in the order the workgroup
//   takes them; k_ppo_grad_reduce adds the G partial rows in the order of g in float64, rounds once and divides by n last.
constexpr int kPpoBlock = 64;
constexpr int kPpoStride = 65;      // words between two rows of an LDS stage
constexpr int kPpoReduceBlock = 256;

__device__ __forceinline__ void ppo_lds_order() {   // LDS accesses before and after keep their order (one wavefront: the hardware's order is the program's)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int KT>
__global__ void __launch_bounds__(kPpoBlock)
k_ppo_grad(int R_src, int R, const float* __restrict__ w_arg, const float* __restrict__ obs_rows, const float* __restrict__ traffic,
           const float* __restrict__ action, const float* __restrict__ logp_old, const float* __restrict__ adv, const uint8_t* __restrict__ mask,
           const int32_t* __restrict__ index, atc_ppo_grad_t gp, float* __restrict__ logp_new, float* __restrict__ scratch) {
    constexpr int IN = ATC_POLICY_TRAFFIC_IN(KT), H = ATC_POLICY_HIDDEN, S = kPpoStride;
    typedef PolOff<IN> O;
    __shared__ float xs[IN * S], h1s[H * S], h2s[H * S], dms[6 * S];
    const int lane = threadIdx.x;
    float aW1[IN], aW2[H], aW3[3] = {0.0f, 0.0f, 0.0f}, ab1 = 0.0f, ab2 = 0.0f, ab3[3] = {0.0f, 0.0f, 0.0f}, als[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < IN; ++c) aW1[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < H; ++c) aW2[c] = 0.0f;
    uint32_t n_part = 0u, n_cut = 0u;
    float sum_l = 0.0f, sum_kl = 0.0f, sum_ratio = 0.0f, max_dlogp = 0.0f;
    const float lo = 1.0f - gp.clip, hi = 1.0f + gp.clip;
    const int tiles = (int)(((long long)R + (kPpoBlock - 1)) / kPpoBlock);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int zk = opaque_zero();       // this tile's opaque zero: the weight loads stay inside the loop (policy_decide)
        pol_wptr w = (pol_wptr)(uintptr_t)w_arg;
        asm volatile("" : "+s"(w) : "s"(zk));
        const long long i = (long long)tile * kPpoBlock + lane;
        bool part = i < (long long)R;
        size_t src = (size_t)i;
        if (index) {
            const int32_t v = part ? index[i] : -1;
            part = part && v >= 0 && v < R_src;
            src = (size_t)(uint32_t)v;
        }
        if (part && mask) part = mask[src] != 0;
        if (__builtin_amdgcn_ballot_w64(part) == 0ull) continue;

        float x[IN], u[3] = {0.0f, 0.0f, 0.0f}, lp_old = 0.0f, a_raw = 0.0f;
#pragma unroll
        for (int c = 0; c < IN; ++c) x[c] = 0.0f;
        if (part) {
            const float* o = obs_rows + src * ATC_OBS_DIM;
#pragma unroll
            for (int c = 0; c < ATC_OBS_DIM; ++c) x[c] = o[c];
            if constexpr (KT > 0) {
                const float* t = traffic + src * (size_t)(KT * ATC_TRAFFIC_DIM);
#pragma unroll
                for (int r = 0; r < KT; ++r)
#pragma unroll
                    for (int c = 0; c < 7; ++c) x[ATC_OBS_DIM + 7 * r + c] = t[r * ATC_TRAFFIC_DIM + c];
            }
            const float* a = action + src * 3u;
            u[0] = a[0];
            u[1] = a[1];
            u[2] = a[2];
            lp_old = logp_old[src];
            a_raw = adv[src];
        }
        ppo_lds_order();                    // (the tile before this one has read its stages)
#pragma unroll
        for (int c = 0; c < IN; ++c) xs[c * S + lane] = x[c];

        // ---- forward: policy_decide, with h1 and h2 kept ----
        float h1[H];
        float xmax = 0.0f;
#pragma unroll
        for (int c = 0; c < IN; ++c) xmax = fmaxf(xmax, fabsf(x[c]));
        if (ATC_RARE(__builtin_amdgcn_ballot_w64(!(xmax <= 4.0f)) != 0ull)) {
            double xd[IN];
#pragma unroll
            for (int c = 0; c < IN; ++c) xd[c] = (double)x[c];
#pragma unroll
            for (int j = 0; j < H; ++j) {
                double s = (double)w[O::B1 + j];
#pragma unroll
                for (int c = 0; c < IN; ++c) s = __builtin_fma((double)w[O::W1 + j * IN + c], xd[c], s);
                h1[j] = (float)s;
            }
        } else {
#pragma unroll
            for (int j = 0; j < H; ++j) {
                float s = w[O::B1 + j];
#pragma unroll
                for (int c = 0; c < IN; ++c) s = fmaf(w[O::W1 + j * IN + c], x[c], s);
                h1[j] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < H; ++j) {
            h1[j] = tanhf(h1[j]);
            h1s[j * S + lane] = h1[j];
        }
        float mu[3] = {w[O::B3 + 0], w[O::B3 + 1], w[O::B3 + 2]};
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
            pol_wptr row = w + O::W2 + j * H;
            float s0 = w[O::B2 + j], s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
            for (int c = 0; c < H; c += 4) {
                s0 = fmaf(row[c + 0], h1[c + 0], s0);
                s1 = fmaf(row[c + 1], h1[c + 1], s1);
                s2 = fmaf(row[c + 2], h1[c + 2], s2);
                s3 = fmaf(row[c + 3], h1[c + 3], s3);
            }
            const float h2 = tanhf((s0 + s1) + (s2 + s3));
            h2s[j * S + lane] = h2;
#pragma unroll
            for (int c = 0; c < 3; ++c) mu[c] = fmaf(w[O::W3 + c * H + j], h2, mu[c]);
        }

        // ---- the loss of the row and its gradient with respect to mu and log_std ----
        float d[3], sigma[3], lp = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ls = w[O::LOGSTD + c];
            sigma[c] = expf(ls);
            d[c] = (u[c] - mu[c]) / sigma[c];
            lp += -0.5f * (d[c] * d[c]) - ls;
        }
        const float logp = lp - ATC_POL_LOGP_C;
        const float dlogp = logp - lp_old;
        const float ratio = expf(dlogp);
        const float A = (a_raw - gp.adv_shift) * gp.adv_scale;
        const float clamped = ratio < lo ? lo : (ratio > hi ? hi : ratio);     // (a NaN stays a NaN, as in torch.clamp)
        const float t1 = ratio * A, t2 = clamped * A;
        const float loss = -(t1 < t2 ? t1 : t2);
        const bool flows = A >= 0.0f ? !(ratio > hi) : !(ratio < lo);
        const float gl = flows ? -(A * ratio) : 0.0f;                          // dL/dlogp
        float dmu[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dmu[c] = part ? gl * (d[c] / sigma[c]) : 0.0f;
            const float dl = part ? gl * (d[c] * d[c] - 1.0f) : 0.0f;
            ab3[c] += dmu[c];
            als[c] += dl;
            dms[c * S + lane] = dmu[c];
        }
        n_part += part ? 1u : 0u;
        n_cut += part && !flows ? 1u : 0u;
        sum_l = part ? sum_l + loss : sum_l;
        sum_kl = part ? sum_kl - dlogp : sum_kl;
        sum_ratio = part ? sum_ratio + ratio : sum_ratio;
        max_dlogp = part ? fmaxf(max_dlogp, fabsf(dlogp)) : max_dlogp;
        if (logp_new && part) logp_new[i] = logp;
        ppo_lds_order();

        // ---- dW3 += dmu^T h2 (lane j: column j) ----
#pragma unroll 4
        for (int r = 0; r < kPpoBlock; ++r) {
            const float t = h2s[lane * S + r];
#pragma unroll
            for (int k = 0; k < 3; ++k) aW3[k] = fmaf(dms[k * S + r], t, aW3[k]);
        }
        ppo_lds_order();

        // ---- lane = row: dz2 over h2 in place, dh1 = W2^T dz2 ----
        float dh1[H];
#pragma unroll
        for (int c = 0; c < H; ++c) dh1[c] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
            pol_wptr row = w + O::W2 + j * H;
            float dh2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) dh2 = fmaf(w[O::W3 + k * H + j], dmu[k], dh2);
            const float h2 = h2s[j * S + lane];
            const float dz2 = dh2 * (1.0f - h2 * h2);
            h2s[j * S + lane] = dz2;
#pragma unroll
            for (int c = 0; c < H; ++c) dh1[c] = fmaf(row[c], dz2, dh1[c]);
        }
        ppo_lds_order();

        // ---- dW2 += dz2^T h1, db2 += dz2 (lane j: row j) ----
#pragma unroll 2
        for (int r = 0; r < kPpoBlock; ++r) {
            const float a2 = h2s[lane * S + r];
            ab2 += a2;
#pragma unroll
            for (int c = 0; c < H; ++c) aW2[c] = fmaf(a2, h1s[c * S + r], aW2[c]);
        }
        ppo_lds_order();

        // ---- lane = row: dz1 over h1 in place ----
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const float h = h1s[c * S + lane];
            h1s[c * S + lane] = dh1[c] * (1.0f - h * h);
        }
        ppo_lds_order();

        // ---- dW1 += dz1^T x, db1 += dz1 (lane j: row j) ----
#pragma unroll 2
        for (int r = 0; r < kPpoBlock; ++r) {
            const float a1 = h1s[lane * S + r];
            ab1 += a1;
#pragma unroll
            for (int c = 0; c < IN; ++c) aW1[c] = fmaf(a1, xs[c * S + r], aW1[c]);
        }
    }

    // ---- the workgroup's partial row: [WORDS] gradient sums, then n, sum L, sum (logp_old - logp), cut, sum ratio, max |dlogp|, 0, 0 ----
    float* const P = scratch + (size_t)blockIdx.x * (size_t)(O::WORDS + ATC_PPO_GRAD_STATS);
#pragma unroll
    for (int c = 0; c < IN; ++c) P[O::W1 + lane * IN + c] = aW1[c];
    P[O::B1 + lane] = ab1;
#pragma unroll
    for (int c = 0; c < H; ++c) P[O::W2 + lane * H + c] = aW2[c];
    P[O::B2 + lane] = ab2;
#pragma unroll
    for (int k = 0; k < 3; ++k) P[O::W3 + k * H + lane] = aW3[k];
    // the per-lane sums, folded over the 64 lanes in lane order in float64 by lanes 0 .. 5, one word each
    ppo_lds_order();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dms[k * S + lane] = ab3[k];
        dms[(3 + k) * S + lane] = als[k];
    }
    ppo_lds_order();
    if (lane < 6) {
        double s = 0.0;
        for (int l = 0; l < kPpoBlock; ++l) s += (double)dms[lane * S + l];
        P[O::B3 + lane] = (float)s;         // (b3[3] and log_std[3] are adjacent)
    }
    static_assert(O::LOGSTD == O::B3 + 3, "b3 and log_std are adjacent");
    ppo_lds_order();
    dms[0 * S + lane] = __uint_as_float(n_part);
    dms[1 * S + lane] = sum_l;
    dms[2 * S + lane] = sum_kl;
    dms[3 * S + lane] = __uint_as_float(n_cut);
    dms[4 * S + lane] = sum_ratio;
    dms[5 * S + lane] = max_dlogp;
    ppo_lds_order();
    if (lane < 6) {
        float word;
        if (lane == ATC_PPO_STAT_N || lane == ATC_PPO_STAT_CUT) {          // counts: exact, kept as integer bit patterns
            uint32_t n = 0u;
            for (int l = 0; l < kPpoBlock; ++l) n += __float_as_uint(dms[lane * S + l]);
            word = __uint_as_float(n);
        } else if (lane == ATC_PPO_STAT_DLOGP_MAX) {
            float m = 0.0f;
            for (int l = 0; l < kPpoBlock; ++l) m = fmaxf(m, dms[lane * S + l]);
            word = m;
        } else {
            double s = 0.0;
            for (int l = 0; l < kPpoBlock; ++l) s += (double)dms[lane * S + l];
            word = (float)s;
        }
        P[O::WORDS + lane] = word;
    } else if (lane < ATC_PPO_GRAD_STATS) {
        P[O::WORDS + lane] = 0.0f;
    }
}

// one lane per word of grad and of stats: the G partial rows in the order of g, in float64, rounded once; the division by n last
__global__ void __launch_bounds__(kPpoReduceBlock)
k_ppo_grad_reduce(int words, int G, const float* __restrict__ scratch, float* __restrict__ grad, float* __restrict__ stats) {
    const int wd = (int)(blockIdx.x * kPpoReduceBlock + threadIdx.x);
    if (wd >= words + ATC_PPO_GRAD_STATS) return;
    const size_t stride = (size_t)(words + ATC_PPO_GRAD_STATS);
    uint64_t n = 0ull;
    for (int g = 0; g < G; ++g) n += (uint64_t)__float_as_uint(scratch[(size_t)g * stride + (size_t)(words + ATC_PPO_STAT_N)]);
    const float nf = (float)n;
    if (wd < words) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)scratch[(size_t)g * stride + (size_t)wd];
        const float v = (float)s;
        grad[wd] = n ? v / nf : 0.0f;
        return;
    }
    const int q = wd - words;
    float out = 0.0f;
    if (q == ATC_PPO_STAT_N) {
        out = nf;
    } else if (q == ATC_PPO_STAT_CUT) {
        uint64_t c = 0ull;
        for (int g = 0; g < G; ++g) c += (uint64_t)__float_as_uint(scratch[(size_t)g * stride + (size_t)wd]);
        out = n ? (float)c / nf : 0.0f;
    } else if (q == ATC_PPO_STAT_DLOGP_MAX) {
        float m = 0.0f;
        for (int g = 0; g < G; ++g) m = fmaxf(m, scratch[(size_t)g * stride + (size_t)wd]);
        out = n ? m : 0.0f;
    } else if (q == ATC_PPO_STAT_LOSS || q == ATC_PPO_STAT_KL || q == ATC_PPO_STAT_RATIO) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)scratch[(size_t)g * stride + (size_t)wd];
        const float v = (float)s;
        out = n ? v / nf : 0.0f;
    }
    stats[q] = out;
}
